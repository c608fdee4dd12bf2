// config_kernels.hip -- the clearance of given configurations and of waypoints (orc_batch_config_clearance,
// orc_batch_waypoint_clearance): the per-sample body of the verdict's walk (verdict_walk.h) without a trajectory and a sample
// clock around it.  A query is one row; it is tested against the scene of the run it names, with the batch's model.
//
// A workgroup takes `chunk` consecutive queries: the model is staged as the walk stages it, the rows are COPIED into the walk's
// rows_s (from the uploaded configurations or from traj[run][point]; no a0 + (a1 - a0) u), then verdict_renormalise and
// verdict_fk, whose text is the walk's.  The wavefront that ran FK for a query (20 per wavefront, fk.h's triads) also tests it:
// its 64 lanes stride over the live spheres x the fields of the query's scene, then over the pairs, each lane keeping (gap, key)
// under the strict `<` of clearance_offer (clearance_kernels.hip) with the lowest key among equals; the lanes reduce by
// shuffles.  So a query's answer is its wavefront's alone: no LDS atomic, no workgroup barrier behind FK, no floating-point
// atomic, and nothing of it depends on the query's place in the list or on what shares its chunk.
#include <hip/hip_runtime.h>
#include <math.h>
#include <atomic>
#include "dev_types.h"
#include "config_device.h"

#pragma clang fp contract(fast)
namespace {

#include "sdf_lookup.h"
#include "fk.h"
#include "verdict_walk.h"
#include "wave.h"           // config_query.h's wave_min
#include "config_query.h"

template <typename real, bool TREE>
__global__ __launch_bounds__(ORC_BLOCK)
void config_clearance_kernel(DevConfigClearance<real> v)
{
   extern __shared__ __align__(16) unsigned char smem_raw[];
   const int lane = threadIdx.x & 63;
   const ConfigQuery<real> Q = config_query_prologue<real, TREE>(v, smem_raw, 0, [](int, const real *, const ModelView<real> &) {});
   const VerdictLds<real> & L = Q.L;
   const ModelView<real> & mod = Q.mod;
   for (int s=Q.s_begin; s<Q.s_end; s++)
   {
      const size_t q = (size_t)(Q.q0 + s);
      if (Q.bad_s[s])      // (wave-uniform)
      {
         if (lane < 2)
         {
            v.clear_out[q*2 + lane] = __longlong_as_double(0x7ff8000000000000LL);
            v.ckey_out[q*2 + lane] = ORC_CONFIG_NONE;
         }
         continue;
      }
      const DevSdf<real> * sdfs; int n_fields;
      verdict_scene<real>(v, __builtin_amdgcn_readfirstlane(Q.run_s[s]), sdfs, n_fields);
      ConfigMin<real> best[2];      // [0] fields, [1] pairs
      for (int leg=0; leg<2; leg++) { best[leg].val = M<real>::inf(); best[leg].key = ORC_CONFIG_NONE; }
      config_tests<real>(v, mod, sdfs, n_fields, s, lane, L, best[0], best[1]);
      for (int leg=0; leg<2; leg++) config_report<real>(best[leg], lane, v.clear_out + q*2 + leg, v.ckey_out + q*2 + leg);
   }
}

} // namespace

hipError_t orc_launch_config_clearance(const DevConfigClearance<double> & v, size_t lds, hipStream_t stream, int tree)
{
   return launch_config_query<DevConfigClearance<double>, config_clearance_kernel<double, true>, config_clearance_kernel<double, false>>(v, lds, stream, tree);
}
hipError_t orc_launch_config_clearance(const DevConfigClearance<float> & v, size_t lds, hipStream_t stream, int tree)
{
   return launch_config_query<DevConfigClearance<float>, config_clearance_kernel<float, true>, config_clearance_kernel<float, false>>(v, lds, stream, tree);
}

// dynamic LDS of config_clearance_kernel: the queries' header, then what the walk holds
size_t orc_config_clearance_lds_bytes(int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk) { return config_query_lds_bytes(n, Sa, Sa_real, nj, real_size, chunk, 0); }
