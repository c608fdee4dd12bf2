// verdict_device.h -- the collision verdict that plans its own samples (verdict_kernels.hip), as batch.cpp launches it.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_types.h"

// Collision verdict of the trajectories of a batch with the retiming and the sample planning on the device: what
// DevVerdict (dev_types.h) takes as offs / seg / u, the kernel derives from the trajectory and vmax.
template <typename real>
struct DevVerdictPlan
{
   const DevModel<real> * model;
   const DevSdf<real> * sdfs;  // [n_scenes][n_sdfs]
   int n_sdfs;                 // fields of the largest scene
   const int * scene_of_run;   // [n_runs] (DevBatch::scene_of_run)
   const int * scene_nsdf;     // [n_scenes]
   int n_runs, n_points, n;
   int col0;                   // first column the retiming reads (7 with a floating base)
   int chunk;                  // samples walked at a time (<= 64, a multiple of 4)
   const real * traj;          // [n_runs][n_points][n]
   const double * vmax;        // [n - col0] velocity limits of the retimed columns
   const int * slot_xml;       // [Sa lanes] XML index of the sphere in a slot, -1: empty
   // the self-collision leg, as in DevVerdict
   int n_pairs;
   const int * pairs;          // [n_pairs][4]
   const real * pair_rsum;     // [n_pairs]
   const real * inact_pos;     // [inactive spheres][3]
   unsigned long long * key_out;   // [n_runs] as DevVerdict::key_out
   double * depth_out;         // [n_runs] penetration depth of the first contact (the caller zeroes it)
   double * time_out;          // [n_runs] its time on the retimed trajectory, -1 without a contact
   int * n_samples_out;        // [n_runs] samples the run's trajectory has (all of them, also when the walk stops at a contact)
   int * too_long;             // [1] set when a run has 2^30 samples or more: nothing of that run is walked (the caller zeroes it)
};

hipError_t orc_launch_verdict_planned(const DevVerdictPlan<double> & v, size_t lds, hipStream_t stream, int tree);
hipError_t orc_launch_verdict_planned(const DevVerdictPlan<float> & v, size_t lds, hipStream_t stream, int tree);
// dynamic LDS of collision_verdict_planned_kernel
size_t orc_verdict_planned_lds_bytes(int n_points, int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk);
