// config_device.h -- the clearance of given configurations and of waypoints (config_kernels.hip), as config_clearance.cpp
// launches it.
#pragma once
#include <hip/hip_runtime.h>
#include "verdict_device.h"

// The per-sample body of the walk (verdict_walk.h) without a trajectory around it: a query is one row of n columns, tested
// against the scene of the run it names.  The rows come from `configs`, or, with configs NULL, from the waypoints
// traj[run][point] of the walk's trajectories.  Of the walk's fields key_out and depth_out are not used, and chunk is the number of
// consecutive queries a workgroup takes.
template <typename real>
struct DevConfigClearance : DevVerdictWalk<real>
{
   int n_q;
   const int * run_of_q;       // [n_q] the run (of this shard) whose scene query q is tested against; NULL: run 0
   const int * point_of_q;     // [n_q] with configs NULL: query q is traj[run_of_q[q]][point_of_q[q]]
   const real * configs;       // [n_q][n], or NULL: waypoints.  configs, run_of_q and point_of_q all NULL: every waypoint in
                               // storage order, query q is traj[q / n_points][q % n_points] against run q / n_points
   // per query two minima, [0] over the fields and [1] over the pairs, widened to double (+inf: nothing to take a minimum of;
   // NaN: the row has a non-finite entry and was not evaluated), and the key of the item of lowest key among those that attain it:
   //   key [0]: XML sphere << 16 | field      key [1]: XML sphere a << 16 | XML sphere b      ORC_CONFIG_NONE without one
   double * clear_out;         // [n_q][2]
   unsigned int * ckey_out;    // [n_q][2]
};

#define ORC_CONFIG_NONE   0xffffffffu
#define ORC_CONFIG_MAX_Q  (1 << 22)

hipError_t orc_launch_config_clearance(const DevConfigClearance<double> & v, size_t lds, hipStream_t stream, int tree);
hipError_t orc_launch_config_clearance(const DevConfigClearance<float> & v, size_t lds, hipStream_t stream, int tree);
size_t orc_config_clearance_lds_bytes(int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk);
