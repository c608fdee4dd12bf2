// project_clear_device.h -- one round of the projection onto TSRs and out of contact (project_clear_kernels.hip), as
// project_clear.cpp launches it after penetration_kernel has evaluated the rounds' iterates.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_types.h"
#include "project_device.h"      // ORC_PROJECT_LANES, ORC_PROJECT_MAX_STEPS, ORC_PROJECT_MAX_Q, ORC_PROJECT_LDS_BYTES, orc_project_stride, the statuses

enum : int { ORC_CLEAR_ON_AND_CLEAR = 0, ORC_CLEAR_ON = 1, ORC_CLEAR_OFF = 2 };      // the classes of an iterate's key

// Query q is the row cur[q] with the constraint tsrs[tsr_of_q[q]] (tsr_of_q NULL: tsrs[0]); the model is the batch's.  The
// rule is or_cdchomp_amd/project_clear.py; a launch is its round `it` for every row whose `done` is 0.
// What lives between the launches is in global memory: cur [n_q][n] (the iterate, which penetration_kernel reads as its
// configs and this kernel replaces with the next), done, best_cls, best_val and the outputs.  Within a launch a lane's state is
// `stride` reals -- h [KMAX], J [KMAX][n], the iterate [n], the gradient and then the push [n] -- at ws + q stride, or in LDS at
// lane x stride when ws is NULL (project_device.h: the same rule, the same stride).  aws [nj][6][n_q] is tsr_eval_point's.
//   cost [n_q][2], grad [n_q][n], clear [n_q][2]: what penetration_kernel wrote for cur at the margins + slack
//   start [n_q][n]: the input in `real`; given [n_q][n]: the caller's doubles.  rows_out is filled with `given` by the caller;
//     an entry of a better iterate that equals start's is written as given's (what never moved comes back bit for bit)
//   resid_out, steps_out, status_out [n_q], clear_out [n_q][2]: of the best iterate (round 0 writes them all); a row with a
//     non-finite entry: NaN, NaN, 0, ORC_PROJECT_NOT_FINITE
//   count [max_steps + 1], zeroed by the caller: count[it] takes the rows that go on to round it + 1
template <typename real>
struct DevProjectClear
{
   const DevModel<real> * model;
   const DevTsr<real> * tsrs;
   const int * tsr_of_q;
   real * cur;
   const real * start;
   const double * given;
   const real * lower, * upper;  // [n] (-inf / +inf without a box)
   const double * cost, * grad, * clear;
   int n_q, n, it, max_steps, stride;
   real tol, mu, step_cap, push_cap;
   double margin_field, margin_self;      // the margins proper: what `clear` is held to
   real * ws;
   real * aws;
   int * done;                   // [n_q] zeroed by the caller; nonzero: the row is frozen
   int * best_cls;               // [n_q]
   real * best_val;              // [n_q]
   int * count;
   double * rows_out, * resid_out, * clear_out;
   int * steps_out, * status_out;
};

// kmax: 3 when no constraint of the call enforces more rows, else 6
hipError_t orc_launch_project_clear_step(const DevProjectClear<double> & v, int kmax, hipStream_t stream);
hipError_t orc_launch_project_clear_step(const DevProjectClear<float> & v, int kmax, hipStream_t stream);
