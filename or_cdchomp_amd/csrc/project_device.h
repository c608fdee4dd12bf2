// project_device.h -- the value and Jacobian of TSRs at given configurations, and the projection of configurations onto
// TSRs (project_kernels.hip), as project.cpp launches them.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_types.h"

#define ORC_PROJECT_LANES      64             // queries of a workgroup: one wavefront, one lane per query
#define ORC_PROJECT_MAX_STEPS  256            // the cap of max_steps: it bounds every lane's loop
#define ORC_PROJECT_MAX_Q      (1 << 22)
// a workgroup's per-lane state lives in LDS up to this many bytes (four workgroups on a CU, one per SIMD); beyond, in `ws`
#define ORC_PROJECT_LDS_BYTES  (40 * 1024)

enum : int { ORC_PROJECT_DONE = 0, ORC_PROJECT_STALLED = 1, ORC_PROJECT_OUT_OF_STEPS = 2, ORC_PROJECT_NOT_FINITE = 3 };

// Query q is the row configs[q] with the constraint tsrs[tsr_of_q[q]] (tsr_of_q NULL: tsrs[0]); the model is the batch's.
// A lane's state is `stride` reals -- h [KMAX], J [KMAX][n], the current row [n], the best row [n] -- at ws + q stride, or in LDS
// at lane x stride when ws is NULL (orc_project_stride: odd, so that the lanes' entries fall into different banks).
// aws [nj][6][n_q] is tsr_eval_point's workspace in global memory, column q.
//   max_steps < 0: the evaluation alone.  h_out [n_q][6] and jac_out [n_q][6][n] take the k enforced rows (the caller zeroes
//     both: rows from k on stay zero); a row with a non-finite entry has NaN there.
//   max_steps >= 0: the projection (or_cdchomp_amd/project.py is the rule).  An entry of rows_out [n_q][n] is written where the
//     answer differs from the input's entry (the caller fills rows_out with the input: what never moved comes back bit for bit,
//     in a precision-32 batch too), resid_out, steps_out, status_out [n_q] always; a row with a non-finite entry: NaN, NaN, 0, ORC_PROJECT_NOT_FINITE.
template <typename real>
struct DevProject
{
   const DevModel<real> * model;
   const DevTsr<real> * tsrs;
   const int * tsr_of_q;
   const real * configs;         // [n_q][n]
   const real * lower, * upper;  // [n] (the projection: -inf / +inf without a box)
   int n_q, n, max_steps, stride;
   real tol, mu, step_cap;
   real * ws;
   real * aws;
   double * h_out, * jac_out;
   double * rows_out, * resid_out;
   int * steps_out, * status_out;
};

// reals of a lane's state for `kmax` rows (3 or 6) of a Jacobian with n columns
inline int orc_project_stride(int n, int kmax) { return (kmax + kmax*n + 2*n) | 1; }
// kmax: 3 when no constraint of the call enforces more rows, else 6 (the kernel's instantiations, as tsr_eval_point's)
hipError_t orc_launch_project(const DevProject<double> & v, int kmax, hipStream_t stream);
hipError_t orc_launch_project(const DevProject<float> & v, int kmax, hipStream_t stream);
