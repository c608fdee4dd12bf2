// penetration_device.h -- the penetration cost of given configurations and of waypoints and its gradient
// (penetration_kernels.hip), as penetration.cpp launches it.
#pragma once
#include <hip/hip_runtime.h>
#include "config_device.h"

// A query of config_clearance_kernel (config_device.h: the row, the run whose scene it is tested against, the two minima and
// their keys) with two margins.  Beside the minima, per query:
//   cost [0] = 1/2 sum max(0, margin_field - (val - r))^2 over the live active spheres x the fields that contain them
//   cost [1] = 1/2 sum max(0, margin_self - (dist - rsum))^2 over the pairs
//   grad [c] = d(cost[0] + cost[1]) / d row[c], the derivative with respect to the caller's row (a floating base: through the
//              renormalisation of its quaternion)
// all NaN for a row with a non-finite entry.
template <typename real>
struct DevPenetration : DevConfigClearance<real>
{
   real margin_field, margin_self;
   // the pairs by sphere: slot s of the position row has the entries sph_pair_list[sph_pair_offs[s] .. sph_pair_offs[s+1]),
   // ascending by pair.  An entry is pair << 3 | owner << 2 | role: role 0 the slot is end a of the pair, 1 end b, 2 neither
   // (a pair of two inactive spheres, listed once with the first live slot); owner: this entry adds the pair's cost (end a, or
   // end b when a is inactive)
   const int * sph_pair_offs;  // [Sa + 1]
   const int * sph_pair_list;
   double * cost_out;          // [n_q][2]
   double * grad_out;          // [n_q][n] (the caller zeroes it: a column no joint owns stays zero)
};

hipError_t orc_launch_penetration(const DevPenetration<double> & v, size_t lds, hipStream_t stream, int tree);
hipError_t orc_launch_penetration(const DevPenetration<float> & v, size_t lds, hipStream_t stream, int tree);
size_t orc_penetration_lds_bytes(int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk);
