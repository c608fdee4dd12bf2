// launch.h -- the launch wrappers of chomp_kernel.hip, hmc_kernels.hip, multistart_kernels.hip and sdf_kernels.hip, as the host layer calls them: the
// iterate and seed wrappers are overloaded by precision, the others take `int precision` (64 or 32) and a `void *` array.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_types.h"

// the row of kernel_table.h that (variant, block, precision) names; hipErrorInvalidValue when the library holds no such kernel
hipError_t orc_launch_iterate(const DevBatch<double> & b, size_t lds, hipStream_t stream, int variant, int block);
hipError_t orc_launch_iterate(const DevBatch<float> & b, size_t lds, hipStream_t stream, int variant, int block);
// straight-line seed trajectories (instantiated for double and float)
template <typename real>
hipError_t orc_launch_seed(real * traj, const double * starts, const double * goals, int n_runs, int n_points, int n, int floating, hipStream_t stream);

// hmc_kernels.hip: the generators' state [625][n_runs] and every run's next resample iteration; the plan of a call's iterations
hipError_t orc_launch_hmc_seed(uint32_t * state, int * next, const unsigned int * seeds, int n_runs, hipStream_t stream);
hipError_t orc_launch_hmc_plan(uint32_t * state, int * next, int n_runs, int iter_begin, int iter_end, int cap, size_t mn, double lambda,
   int precision, void * noise, int * iters, int * overflow, hipStream_t stream);
// multistart_kernels.hip
size_t orc_perturb_lds_bytes(int m, int n);
hipError_t orc_launch_perturb(void * traj, int precision, int n_runs, int n_points, int n, int m, const unsigned int * seeds, int D,
   const double * genU, const double * genV, double scale, const double * lim_lo, const double * lim_hi, size_t lds,
   const int * source_of_run, hipStream_t stream);
hipError_t orc_launch_respawn_rank(const double * costs, const int * status, const unsigned long long * verdict_key, int mode, int column, int keep,
   int n_groups, const int * group_offs, const int * members, int max_group, int * source_of_run, int * n_survivors, hipStream_t stream);
hipError_t orc_launch_respawn_copy(void * traj, void * AG, int precision, int * leapfrog_first, const int * source_of_run,
   int n_runs, int n_points, int n, int m, hipStream_t stream);
// The rule of a selection, in the kernarg block of its kernels: which runs are eligible and what is minimised among them.
struct SelectRule
{
   const double * costs; const int * status;   // [n_runs][3], [n_runs]: what the last iterate call left (a candidate: run_candidate.h)
   const unsigned long long * verdict_key;     // [n_runs] keys of the collision verdict: a run with a contact is not eligible; NULL: not asked for
   const double * clear; const int * n_samples;   // [n_runs][2], [n_runs] of the last clearance: a run that was not walked or whose
   double margin;                              // fmin of the two is under `margin` is not eligible; both NULL: no margin
   int column;                                 // the key: costs[run][column] for 0..2; 3 (with clear): minus the clearance, the largest first
};
// the best run per group: the lowest key, the eligible runs, the lowest run that has the key, (a rule with clear) its clearance
hipError_t orc_launch_select(const SelectRule & rule, const int * group, int n_runs, int n_groups, unsigned long long * key, int * count, int * best,
   double * best_clear, hipStream_t stream);
hipError_t orc_launch_gather_rows(const void * traj, int precision, const int * rows, int n_sel, size_t row_len, double * out, hipStream_t stream);
// sdf_kernels.hip: occupancy -> signed distance field; the whole field of a body from the world's boxes and triangles (host arrays in, host array out)
hipError_t orc_sdf_from_occupancy_device(const double * occ, double * sdf_out, const int sizes[3], const double lengths[3],
   hipStream_t st);
hipError_t orc_sdf_build_device(const int sizes[3], const double lengths[3], const double grid_xform[12], const double grid_pose[7],
   double cube_extent, int n_boxes, const double * boxes, int n_tris, const double * tris, double * sdf_out, hipStream_t st);
