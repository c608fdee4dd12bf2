// clearance_kernels.hip -- the clearance of a batch's runs (orc_batch_clearance, orc_batch_select_clear): how far every run
// stays from the fields of its scene and from itself, at exactly the samples the collision verdict looks at.
//
// clearance_kernel has the shape of collision_verdict_planned_kernel (verdict_kernels.hip): one workgroup per run, a fifth
// wavefront that retimes the run and steps the sample times a chunk ahead (verdict_plan.h: the host's arithmetic, rounding
// for rounding), four wavefronts that interpolate the rows, run FK and look the spheres up (verdict_walk.h).  Where the
// verdict stops at the first contact, this walk goes to the end and every thread keeps a running minimum of the gap of its
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

#define ORC_CL_WORKERS ORC_BLOCK            // threads that walk the samples (verdict_walk.h)
#define ORC_CL_BLOCK   (ORC_BLOCK + 64)     // ... and the planner's wavefront
#define ORC_CL_HEADER  64                   // bytes: the two keys, the sample counts of the two chunk buffers, the too-long flag, four wave minima

#pragma clang fp contract(off)
namespace {

#include "verdict_plan.h"

} // namespace

#pragma clang fp contract(fast)
namespace {

#include "sdf_lookup.h"
#include "fk.h"
#include "verdict_walk.h"

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

template <typename real>
__device__ __forceinline__ real wave_min(real x)
{
   for (int d=32; d>=1; d>>=1) x = M<real>::min_(x, __shfl_xor(x, d));
   return x;
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
__global__ __launch_bounds__(ORC_CL_BLOCK)
void clearance_kernel(DevClearance<real> v)
{
   extern __shared__ __align__(16) unsigned char smem_raw[];
   const DevModel<real> & gmod = *v.model;
   const int run = blockIdx.x, tid = threadIdx.x;
   const bool planner = tid >= ORC_CL_WORKERS;
   // ---- is the run examined at all?  One answer for the workgroup, before anything is staged and before the first barrier
   if (v.examine || v.cand_status)
   {
      const int walk = v.examine ? (v.examine[run] != 0) : (orc_run_candidate(v.cand_status[run], v.cand_costs[(size_t) run*3]) ? 1 : 0);
      if (!__builtin_amdgcn_readfirstlane(walk))
      {
         if (tid == 0) clearance_not_walked(v, run, ORC_VERDICT_SKIPPED);
         return;
      }
   }
   const int n = v.n, np = v.n_points, chunk = v.chunk;
   const DevSdf<real> * sdfs; int n_fields;
   verdict_scene<real>(v, run, sdfs, n_fields);
   unsigned long long * key_s = (unsigned long long *) smem_raw;     // [2]: the lowest key at the minimum, fields and pairs
   int * cnt_s = (int *)(smem_raw + 16);                             // [2]: samples in either chunk buffer
   int * long_s = (int *)(smem_raw + 24);                            // [1]: the run has too many samples
   double * wmin_s = (double *)(smem_raw + 32);                      // [4]: the wavefronts' minima of the leg being reduced
   double * times_s = (double *)(smem_raw + ORC_CL_HEADER);          // [2][chunk]
   double * u_s = times_s + 2*chunk;                                 // [2][chunk]
   double * dtm_s = u_s + 2*chunk;                                   // [np]
   double * tstart_s = dtm_s + np;                                   // [np]
   int * seg_s = (int *)(tstart_s + np);                             // [2][chunk]
   const VerdictLds<real> L = verdict_lds((unsigned char *)(seg_s + 2*chunk), gmod, n, chunk);
   verdict_stage<real, ORC_CL_BLOCK>(gmod, v.slot_xml, L, tid);
   if (tid == 0) { key_s[0] = ORC_VERDICT_NONE; key_s[1] = ORC_VERDICT_NONE; dtm_s[0] = 0.0; }
   const ModelView<real> mod = verdict_model_view(gmod, n, L);

   const real * traj = v.traj + (size_t) run * np * n;
   // ---- the plan's prologue: a lane per segment, then one lane for the sums that have an order
   for (int i=1+tid; i<np; i+=ORC_CL_BLOCK) plan_segment(traj, i, n, v.col0, v.vmax, dtm_s[i], tstart_s[i]);
   __syncthreads();
   double time = 0.0, step_time = 0.0, duration = 0.0;      // the planner's first lane keeps the clock
   int planned = 0;
   if (tid == ORC_CL_WORKERS)
   {
      double total_dist;
      plan_totals(np, dtm_s, tstart_s, total_dist, duration);
      step_time = plan_step_time(total_dist, duration);
      // the verdict's rule with the caller's cap: decided before anything is walked.  A run it passes has at most
      // max_samples + 2 samples, and its step advances the clock, so the loop below ends
      const bool too_long = duration > 0.0 && (total_dist / 0.04 >= (double) v.max_samples || step_time <= 0.0);
      long_s[0] = too_long ? 1 : 0;
      planned = too_long ? 0 : plan_times(time, step_time, duration, times_s, chunk);
      cnt_s[0] = planned;
   }
   __syncthreads();
   if (long_s[0])      // (workgroup-uniform)
   {
      if (tid == 0) clearance_not_walked(v, run, ORC_VERDICT_TOO_LONG);
      return;
   }
   if (planner && tid - ORC_CL_WORKERS < cnt_s[0])
   {
      const int k = tid - ORC_CL_WORKERS;
      seg_s[k] = plan_locate(times_s[k], np, dtm_s, tstart_s, u_s[k]);
   }
   __syncthreads();

   ClearMin<real> best[2];      // [0] fields, [1] pairs
   for (int leg=0; leg<2; leg++) { best[leg].val = M<real>::inf(); best[leg].key = ORC_VERDICT_NONE; best[leg].time = -1.0; }
   for (int ci=0; ; ci++)
   {
      const int buf = (ci & 1) * chunk, nbuf = chunk - buf;
      const int count = cnt_s[ci & 1];
      if (count == 0) break;
      if (tid == ORC_CL_WORKERS)
      {
         const int more = plan_times(time, step_time, duration, times_s + nbuf, chunk);
         cnt_s[(ci + 1) & 1] = more;
         planned += more;
      }
      if (!planner) verdict_rows(traj, seg_s, u_s, buf, count, n, tid, L);
      __syncthreads();
      if (planner && tid - ORC_CL_WORKERS < cnt_s[(ci + 1) & 1])
      {
         const int k = nbuf + tid - ORC_CL_WORKERS;
         seg_s[k] = plan_locate(times_s[k], np, dtm_s, tstart_s, u_s[k]);
      }
      verdict_renormalise(mod, count, tid, L);      // (tid < count: workers)
      __syncthreads();
      if (!planner) verdict_fk<real, TREE>(mod, count, tid, L);
      __syncthreads();
      if (!planner) clearance_tests<real>(v, mod, sdfs, n_fields, ci * chunk, count, tid, L, times_s + buf, best[0], best[1]);
      __syncthreads();      // (the next pass writes the rows, and the pass after it this chunk's times)
      if (count < chunk) break;
   }

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
   if (tid == ORC_CL_WORKERS) v.n_samples_out[run] = planned;
}

} // namespace

template <typename real>
static hipError_t launch_clearance_t(const DevClearance<real> & v, size_t lds, hipStream_t stream, int tree)
{
   static std::atomic<unsigned long long> attr_set{0ull};      // (the dynamic-LDS attribute is per device and per kernel)
   if (v.n_points < 2 || v.chunk < 4 || v.chunk > 64 || (v.chunk & 3)) return hipErrorInvalidValue;
   if (v.max_samples < 1 || v.max_samples > ORC_CLEARANCE_MAX_SAMPLES) return hipErrorInvalidValue;
   int dev = 0;
   if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
   if (!((attr_set.load() >> dev) & 1ull))
   {
      hipError_t e = hipFuncSetAttribute((const void *) clearance_kernel<real, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160*1024 - 256);
      if (e == hipSuccess) e = hipFuncSetAttribute((const void *) clearance_kernel<real, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160*1024 - 256);
      if (e != hipSuccess) return e;
      attr_set.fetch_or(1ull << dev);
   }
   if (lds > 160*1024 - 256) return hipErrorInvalidValue;
   if (tree) hipLaunchKernelGGL((clearance_kernel<real, true>), dim3(v.n_runs), dim3(ORC_CL_BLOCK), lds, stream, v);
   else hipLaunchKernelGGL((clearance_kernel<real, false>), dim3(v.n_runs), dim3(ORC_CL_BLOCK), lds, stream, v);
   return hipGetLastError();
}
hipError_t orc_launch_clearance(const DevClearance<double> & v, size_t lds, hipStream_t stream, int tree) { return launch_clearance_t<double>(v, lds, stream, tree); }
hipError_t orc_launch_clearance(const DevClearance<float> & v, size_t lds, hipStream_t stream, int tree) { return launch_clearance_t<float>(v, lds, stream, tree); }

// dynamic LDS of clearance_kernel (the carve-up at its top): the header, the plan's arrays, then what the walk holds
size_t orc_clearance_lds_bytes(int n_points, int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk)
{
   const size_t plan = (size_t) ORC_CL_HEADER + ((size_t) 4*chunk + (size_t) 2*n_points) * sizeof(double) + (size_t) 2*chunk * sizeof(int);
   return plan + verdict_walk_lds_bytes(n, Sa, Sa_real, nj, real_size, chunk);
}
