// clearance_kernels.hip -- the clearance of a batch's runs (orc_batch_clearance, orc_batch_select_clear): how far every run
// stays from the fields of its scene and from itself, at exactly the samples the collision verdict looks at.
//
// clearance_kernel is, like collision_verdict_planned_kernel (verdict_kernels.hip), a shell around the planned walk of
// verdict_planned.h: one workgroup per run, a fifth wavefront that retimes the run and steps the sample times a chunk ahead
// (verdict_plan.h: the host's arithmetic, rounding for rounding), four wavefronts that interpolate the rows, run FK and
// look the spheres up (verdict_walk.h) -- one text for both kernels, so both look at the same samples.  Where the verdict's
// policy stops at the first contact, this one never stops and every thread keeps a running minimum of the gap of its
// items: `value - radius` over the live spheres in every field that contains them, `distance - radius sum` over the pairs of
// the self-collision leg -- the subtractions the verdict compares to zero.  A walk without a stop needs a bound of its own:
// the caller's max_samples stands where the verdict has 2^30, decided by the planner's first lane before anything is walked.
//
// The workgroup's minimum is taken once, after the walk, and does not depend on a schedule: the values by shuffles within
// a wavefront, the four wavefronts' minima through LDS, and among the threads that hold the minimum a 64-bit atomicMin of
// the item's key -- an integer minimum, the same in any order.  No floating-point atomic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <atomic>
#include "dev_types.h"
#include "clearance_device.h"
#include "run_candidate.h"

#define ORC_CL_HEADER  64                   // bytes of the kernel's LDS header: the two keys, the plan's flags (verdict_planned.h), four wave minima

#pragma clang fp contract(off)
namespace {

#include "verdict_plan.h"

} // namespace

#pragma clang fp contract(fast)
namespace {

#include "sdf_lookup.h"
#include "fk.h"
#include "verdict_walk.h"
#include "verdict_planned.h"
#include "wave.h"           // wave_min

// a thread's running minimum of one leg: the items reach a thread in ascending key order, so `<` keeps the lowest key
template <typename real>
struct ClearMin
{
   real val;
   unsigned long long key;
   double time;
};

template <typename real>
__device__ __forceinline__ void clearance_offer(ClearMin<real> & m, real gap, int sample, int a, int b, const double * times, int s)
{
   if (gap < m.val)      // (a NaN is ignored; +inf -- a poisoned cell, a merged field's "no field here" -- is never below)
   {
      m.val = gap;
      m.key = ((unsigned long long) sample << 32) | ((unsigned long long) a << 16) | (unsigned long long) b;
      m.time = times[s];
   }
}

// verdict_tests (verdict_walk.h) with a minimum in place of the contact: the chunk's `count` samples, the run's samples
// sbase .., their times in `times`
template <typename real>
__device__ __forceinline__ void clearance_tests(const DevVerdictWalk<real> & v, const ModelView<real> & mod, const DevSdf<real> * sdfs, int n_fields,
   int sbase, int count, int tid, const VerdictLds<real> & L, const double * times, ClearMin<real> & fld, ClearMin<real> & slf)
{
   const int Sa = mod.Sa;
   for (int item=tid; item<count*Sa; item+=ORC_BLOCK)
   {
      const int s = item / Sa, slot = item - s*Sa;
      if (!((mod.live_mask >> slot) & 1ull)) continue;
      const real * p = L.pos_s + s*L.pstr + slot*3;
      const real radius = L.srad_s[slot];
      for (int i=0; i<n_fields; i++)
      {
         const DevSdf<real> & F = sdfs[i];
         real gp[3], gg[3], val;
#pragma unroll
         for (int k=0; k<3; k++)
            gp[k] = F.Rgw[k*3+0]*p[0] + F.Rgw[k*3+1]*p[1] + F.Rgw[k*3+2]*p[2] + F.tgw[k];
         if (sdf_lookup(F, gp, val, gg)) continue;                 // outside this field
         clearance_offer<real>(fld, val - radius, sbase + s, L.xml_s[slot], i, times, s);
      }
   }
   for (int item=tid; item<count*v.n_pairs; item+=ORC_BLOCK)
   {
      const int s = item / v.n_pairs, pi = item - s*v.n_pairs;
      const int ea = v.pairs[pi*4+0], eb = v.pairs[pi*4+1];
      const real * pa = (ea >= 0) ? L.pos_s + s*L.pstr + ea*3 : v.inact_pos + (-1 - ea)*3;
      const real * pb = (eb >= 0) ? L.pos_s + s*L.pstr + eb*3 : v.inact_pos + (-1 - eb)*3;
      const real dx = pa[0]-pb[0], dy = pa[1]-pb[1], dz = pa[2]-pb[2];
      const real dist = M<real>::sqrt_(dx*dx + dy*dy + dz*dz);
      const real rs = v.pair_rsum[pi];
      clearance_offer<real>(slf, dist - rs, sbase + s, v.pairs[pi*4+2], v.pairs[pi*4+3], times, s);
   }
}

// what a run that was not walked reports (tid 0)
template <typename real>
__device__ __forceinline__ void clearance_not_walked(const DevClearance<real> & v, int run, int mark)
{
   for (int leg=0; leg<2; leg++)
   {
      v.clear_out[(size_t) run*2 + leg] = __longlong_as_double(0x7ff8000000000000LL);
      v.ckey_out[(size_t) run*2 + leg] = ORC_VERDICT_NONE;
      v.ctime_out[(size_t) run*2 + leg] = -1.0;
   }
   v.n_samples_out[run] = mark;
}

template <typename real, bool TREE>
__global__ __launch_bounds__(ORC_VP_BLOCK)
void clearance_kernel(DevClearance<real> v)
{
   extern __shared__ __align__(16) unsigned char smem_raw[];
   const DevModel<real> & gmod = *v.model;
   const int run = blockIdx.x, tid = threadIdx.x;
   const bool planner = tid >= ORC_VP_WORKERS;
   if (!planned_examined<real>(v, run))
   {
      if (tid == 0) clearance_not_walked(v, run, ORC_VERDICT_SKIPPED);
      return;
   }
   const int n = v.n, np = v.n_points, chunk = v.chunk;
   const DevSdf<real> * sdfs; int n_fields;
   verdict_scene<real>(v, run, sdfs, n_fields);
   unsigned long long * key_s = (unsigned long long *) smem_raw;     // [2]: the lowest key at the minimum, fields and pairs
   double * wmin_s = (double *)(smem_raw + 32);                      // [4]: the wavefronts' minima of the leg being reduced
   const PlannedLds<real> P = planned_lds(smem_raw, ORC_CL_HEADER, gmod, np, n, chunk);
   verdict_stage<real, ORC_VP_BLOCK>(gmod, v.slot_xml, P.walk, tid);
   if (tid == 0) { key_s[0] = ORC_VERDICT_NONE; key_s[1] = ORC_VERDICT_NONE; }
   const ModelView<real> mod = verdict_model_view(gmod, n, P.walk);

   const real * traj = v.traj + (size_t) run * np * n;
   PlannedClock c;
   // (the verdict's rule with the caller's cap: a run it passes has at most max_samples + 2 samples, so a walk without a stop ends)
   if (planned_prologue<real>(v, traj, v.max_samples, tid, P, c))
   {
      if (tid == 0) clearance_not_walked(v, run, ORC_VERDICT_TOO_LONG);
      return;
   }
   // the walk's policy: the minima of a chunk, and no stop
   ClearMin<real> best[2];      // [0] fields, [1] pairs
   for (int leg=0; leg<2; leg++) { best[leg].val = M<real>::inf(); best[leg].key = ORC_VERDICT_NONE; best[leg].time = -1.0; }
   planned_walk<real, TREE, false>(v, mod, traj, tid, P, c, nullptr, [&](int sbase, int count, const double * times) {
      clearance_tests<real>(v, mod, sdfs, n_fields, sbase, count, tid, P.walk, times, best[0], best[1]); });

   // ---- the workgroup's two minima, and at each the lowest key
   for (int leg=0; leg<2; leg++)
   {
      if (!planner)
      {
         const real w = wave_min<real>(best[leg].val);
         if ((tid & 63) == 0) wmin_s[tid >> 6] = (double) w;
      }
      __syncthreads();
      const double lowest = ::fmin(::fmin(wmin_s[0], wmin_s[1]), ::fmin(wmin_s[2], wmin_s[3]));
      const bool mine = !planner && best[leg].key != ORC_VERDICT_NONE && (double) best[leg].val == lowest;
      if (mine) atomicMin(&key_s[leg], best[leg].key);
      __syncthreads();
      const unsigned long long first = key_s[leg];
      if (first == ORC_VERDICT_NONE)
      {
         if (tid == 0)
         {
            v.clear_out[(size_t) run*2 + leg] = (double) M<real>::inf();
            v.ckey_out[(size_t) run*2 + leg] = ORC_VERDICT_NONE;
            v.ctime_out[(size_t) run*2 + leg] = -1.0;
         }
      }
      else if (mine && best[leg].key == first)      // (one thread: an item belongs to one thread)
      {
         v.clear_out[(size_t) run*2 + leg] = (double) best[leg].val;
         v.ckey_out[(size_t) run*2 + leg] = first;
         v.ctime_out[(size_t) run*2 + leg] = best[leg].time;
      }
   }
   if (tid == ORC_VP_WORKERS) v.n_samples_out[run] = c.planned;
}

} // namespace

template <typename real>
static hipError_t launch_clearance_t(const DevClearance<real> & v, size_t lds, hipStream_t stream, int tree)
{
   if (!planned_args_ok<real>(v)) return hipErrorInvalidValue;
   if (v.max_samples < 1 || v.max_samples > ORC_CLEARANCE_MAX_SAMPLES) return hipErrorInvalidValue;
   return launch_verdict_kernels<DevClearance<real>, clearance_kernel<real, true>, clearance_kernel<real, false>>(v, ORC_VP_BLOCK, lds, stream, tree);
}
hipError_t orc_launch_clearance(const DevClearance<double> & v, size_t lds, hipStream_t stream, int tree) { return launch_clearance_t<double>(v, lds, stream, tree); }
hipError_t orc_launch_clearance(const DevClearance<float> & v, size_t lds, hipStream_t stream, int tree) { return launch_clearance_t<float>(v, lds, stream, tree); }

// dynamic LDS of clearance_kernel (the carve-up at its top): the header, the plan's arrays, then what the walk holds
size_t orc_clearance_lds_bytes(int n_points, int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk)
{
   return planned_lds_bytes(ORC_CL_HEADER, n_points, n, Sa, Sa_real, nj, real_size, chunk);
}
