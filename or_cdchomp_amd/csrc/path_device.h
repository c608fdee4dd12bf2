// path_device.h -- the clearance of given paths and of segments between waypoints (path_kernels.hip), as path_clearance.cpp
// launches it.
#pragma once
#include <hip/hip_runtime.h>
#include "verdict_device.h"

// The walk of clearance_kernel (clearance_kernels.hip) over paths that are no run's trajectory: query q is n_rows rows of n
// columns, retimed and sampled as a run is (verdict_plan.h) and tested against the scene of the run it names, with the batch's
// model.  The rows come from `paths`, or, with paths NULL (n_rows 2), from the waypoints traj[run][from] and traj[run][to] of
// the walk's trajectories.  Four kernels, on one stream in this order:
//   count    a lane per query: the too-long rule and the exact number of samples            -> count
//   fill     a lane per query: (query, seg, u, time) of each of its samples, from offs[q] on  -> e_*
//   walk     a workgroup per `chunk` consecutive ENTRIES of that list, whichever queries they belong to: rows, FK, the tests;
//            per entry and leg the smallest gap and the lowest key at it                      -> e_gap, e_key
//   reduce   a wavefront per query: the minimum over its entries in sample order             -> the outputs
// The host cuts a call into rounds of consecutive queries whose entries fit the workspace; `count` runs once over the call,
// the other three once per round, on the round's slice of the per-query arrays (offs: relative to the round's first entry).
// Of the walk's fields key_out and depth_out are not used.
template <typename real>
struct DevPathClearance : DevVerdictWalk<real>
{
   int col0;                   // first column the retiming reads (7 with a floating base)
   const double * vmax;        // [n - col0] velocity limits of the retimed columns
   int max_samples;            // a query with C-space length / 0.04 >= max_samples is too long: nothing of it is walked
   int n_q, n_rows;
   const int * run_of_q;       // [n_q] the run (of this shard) whose scene query q is tested against; NULL: run 0
   const int * from_of_q;      // [n_q] with paths NULL: the query's two rows are traj[run][from] and traj[run][to]
   const int * to_of_q;
   const real * paths;         // [n_q][n_rows][n], or NULL: waypoints
   int * count;                // [n_q] samples of the query, ORC_VERDICT_TOO_LONG for one that is too long
   const int * offs;           // [n_q] the query's first entry in the workspace
   int n_entries;              // entries of the round
   int * e_query;              // [n_entries] the query (of the round) an entry belongs to
   int * e_seg;                // [n_entries] the segment of the query's rows the sample lies on
   double * e_u;               // [n_entries] its position on the segment, 0..1
   double * e_time;            // [n_entries] its time on the retimed path
   double * e_gap;             // [n_entries][2] the entry's smallest gap, [0] over the fields and [1] over the pairs (+inf: none)
   unsigned int * e_key;       // [n_entries][2] XML sphere << 16 | field, or the other sphere of a pair; ORC_PATH_NONE without one
   // per query what DevClearance reports per run (clearance_device.h), with the same keys: NaN, ORC_VERDICT_NONE and time -1
   // for a query that is too long
   double * clear_out;              // [n_q][2]
   unsigned long long * ckey_out;   // [n_q][2]
   double * ctime_out;              // [n_q][2]
   int * n_samples_out;             // [n_q]
};

#define ORC_PATH_NONE       0xffffffffu
#define ORC_PATH_MAX_Q      (1 << 22)
#define ORC_PATH_MAX_ROWS   4096
// entries of the workspace (48 bytes each): one query of the largest max_samples has 2^20 + 2 at most
#define ORC_PATH_WORKSPACE  (1 << 21)

hipError_t orc_launch_path_count(const DevPathClearance<double> & v, hipStream_t stream);
hipError_t orc_launch_path_count(const DevPathClearance<float> & v, hipStream_t stream);
// fill, walk and reduce of one round
hipError_t orc_launch_path_round(const DevPathClearance<double> & v, size_t lds, hipStream_t stream, int tree);
hipError_t orc_launch_path_round(const DevPathClearance<float> & v, size_t lds, hipStream_t stream, int tree);
// dynamic LDS of path_walk_kernel
size_t orc_path_walk_lds_bytes(int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk);
