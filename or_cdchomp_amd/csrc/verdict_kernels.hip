// verdict_kernels.hip -- the collision verdict of a batch: the first contact of every run's trajectory with a field of its
// scene or of the robot with itself, on a sample every 0.04 rad of C-space distance along the retimed trajectory, as the
// reference's re-check in gettraj (src/orcdchomp_mod.cpp:2958-3006).  One workgroup per run walks the run's samples up to
// 64 at a time (DevVerdictWalk::chunk); the walk is verdict_walk.h, and both kernels here are made of it.
//
// collision_verdict_kernel (orc_batch_collision_verdict, gettraj's own re-check) walks samples the host planned:
// Module::batch_collision_verdict reads every trajectory back, retimes it (retime_linear), lays the samples
// (plan_collision_samples) and uploads the list.  In collision_verdict_planned_kernel (orc_batch_collision_verdict_device,
// orc_batch_select_best with require_collision_free, orc_batch_respawn) the run's workgroup does that itself: a fifth
// wavefront, the planner, retimes the run and steps the sample times a chunk ahead of the four wavefronts that walk them,
// so no trajectory leaves the device and no sample list exists.  It can be asked about a subset of the runs
// (orc_batch_collision_verdict_subset, orc_batch_set_verdict_scope): a caller's byte per run, or the candidates of
// run_candidate.h; the workgroup of any other run returns before it stages anything.
//
// The planning arithmetic is the host's, rounding for rounding (module.py verdict_samples is its specification): doubles
// for either precision, no fused multiply-add, the sums in index order, time advanced by repeated addition.  What is
// parallel is only what has no order: a segment's dtm and length (one lane per segment) and a sample's segment, which
// is a search -- the host's running `tseg0 + dtm[seg+1]` is the addition that forms tstart[seg+1], so the segment of a
// sample is the number of s in 1 .. n_points-2 with tstart[s] < time.
#include <hip/hip_runtime.h>
#include <math.h>
#include <atomic>
#include "dev_types.h"
#include "verdict_device.h"
#include "run_candidate.h"

#define ORC_VD_WORKERS ORC_BLOCK            // threads that walk the samples (verdict_walk.h)
#define ORC_VD_BLOCK   (ORC_BLOCK + 64)     // ... and the planner's wavefront
#define ORC_VD_HEADER  32                   // bytes: the first contact's key, the sample counts of the two chunk buffers, the too-long flag

// ---- the plan: the host's arithmetic (module.cpp retime_linear, plan_collision_samples) ----------------------------------
#pragma clang fp contract(off)
namespace {

#include "verdict_plan.h"

} // namespace

// ---- the walk (verdict_walk.h) and the two kernels around it ----------------------------------------------------------------
#pragma clang fp contract(fast)
namespace {

#include "sdf_lookup.h"
#include "fk.h"
#include "verdict_walk.h"

template <typename real, bool TREE>
__global__ __launch_bounds__(ORC_BLOCK)
void collision_verdict_kernel(DevVerdict<real> v)
{
   extern __shared__ __align__(16) unsigned char smem_raw[];
   const DevModel<real> & gmod = *v.model;
   const int run = blockIdx.x, tid = threadIdx.x;
   const int n = v.n, np = v.n_points, chunk = v.chunk;
   const DevSdf<real> * sdfs; int n_fields;
   verdict_scene<real>(v, run, sdfs, n_fields);
   unsigned long long * key_s = (unsigned long long *) smem_raw;     // [2]: the first contact's key (DevVerdictWalk::key_out)
   const VerdictLds<real> L = verdict_lds(smem_raw + 16, gmod, n, chunk);
   verdict_stage<real, ORC_BLOCK>(gmod, v.slot_xml, L, tid);
   if (tid == 0) key_s[0] = ORC_VERDICT_NONE;
   const ModelView<real> mod = verdict_model_view(gmod, n, L);
   __syncthreads();

   const real * traj = v.traj + (size_t) run * np * n;
   const int s0 = v.offs[run], s1 = v.offs[run+1];
   double my_depth = 0.0; unsigned long long my_key = ORC_VERDICT_NONE;
   for (int base=s0; base<s1; base+=chunk)
   {
      const int count = (s1 - base < chunk) ? s1 - base : chunk;
      verdict_rows(traj, v.seg, v.u, base, count, n, tid, L);
      __syncthreads();
      verdict_renormalise(mod, count, tid, L);
      __syncthreads();
      verdict_fk<real, TREE>(mod, count, tid, L);
      __syncthreads();
      verdict_tests<real>(v, mod, sdfs, n_fields, base - s0, count, tid, L, my_key, my_depth, key_s);
      __syncthreads();
      if (key_s[0] != ORC_VERDICT_NONE) break;          // a contact in this chunk: later samples cannot come first
      __syncthreads();
   }
   __syncthreads();
   const unsigned long long first = key_s[0];
   if (tid == 0) v.key_out[run] = first;
   if (first != ORC_VERDICT_NONE && my_key == first) v.depth_out[run] = my_depth;
}

template <typename real, bool TREE>
__global__ __launch_bounds__(ORC_VD_BLOCK)
void collision_verdict_planned_kernel(DevVerdictPlan<real> v)
{
   extern __shared__ __align__(16) unsigned char smem_raw[];
   const DevModel<real> & gmod = *v.model;
   const int run = blockIdx.x, tid = threadIdx.x;
   const bool planner = tid >= ORC_VD_WORKERS;
   // ---- is the run examined at all?  One answer for the workgroup (the run is the block's index and the tables are read at
   // that index, a uniform address; readfirstlane makes the branch a scalar one whatever loads the compiler picks), taken
   // before anything is staged and before the first barrier
   if (v.examine || v.cand_status)
   {
      const int walk = v.examine ? (v.examine[run] != 0) : (orc_run_candidate(v.cand_status[run], v.cand_costs[(size_t) run*3]) ? 1 : 0);
      if (!__builtin_amdgcn_readfirstlane(walk))
      {
         if (tid == 0) { v.key_out[run] = ORC_VERDICT_NONE; v.time_out[run] = -1.0; v.n_samples_out[run] = ORC_VERDICT_SKIPPED; }
         return;
      }
   }
   const int n = v.n, np = v.n_points, chunk = v.chunk;
   const DevSdf<real> * sdfs; int n_fields;
   verdict_scene<real>(v, run, sdfs, n_fields);
   unsigned long long * key_s = (unsigned long long *) smem_raw;     // [1]: the first contact's key (DevVerdictWalk::key_out)
   int * cnt_s = (int *)(smem_raw + 8);                              // [2]: samples in either chunk buffer
   int * long_s = (int *)(smem_raw + 16);                            // [1]: the run has too many samples
   double * times_s = (double *)(smem_raw + ORC_VD_HEADER);          // [2][chunk]
   double * u_s = times_s + 2*chunk;                                 // [2][chunk]
   double * dtm_s = u_s + 2*chunk;                                   // [np]
   double * tstart_s = dtm_s + np;                                   // [np]
   int * seg_s = (int *)(tstart_s + np);                             // [2][chunk]
   const VerdictLds<real> L = verdict_lds((unsigned char *)(seg_s + 2*chunk), gmod, n, chunk);
   verdict_stage<real, ORC_VD_BLOCK>(gmod, v.slot_xml, L, tid);
   if (tid == 0) { key_s[0] = ORC_VERDICT_NONE; dtm_s[0] = 0.0; }
   const ModelView<real> mod = verdict_model_view(gmod, n, L);

   const real * traj = v.traj + (size_t) run * np * n;
   // ---- the plan's prologue: a lane per segment, then one lane for the sums that have an order
   for (int i=1+tid; i<np; i+=ORC_VD_BLOCK) plan_segment(traj, i, n, v.col0, v.vmax, dtm_s[i], tstart_s[i]);
   __syncthreads();
   double time = 0.0, step_time = 0.0, duration = 0.0;      // the planner's first lane keeps the clock
   int planned = 0;
   if (tid == ORC_VD_WORKERS)
   {
      double total_dist;
      plan_totals(np, dtm_s, tstart_s, total_dist, duration);
      step_time = plan_step_time(total_dist, duration);
      // decided before anything is walked; a step that does not advance the clock (an underflow) would never end
      const bool too_long = duration > 0.0 && (total_dist / 0.04 >= (double) ORC_VD_MAX_SAMPLES || step_time <= 0.0);
      long_s[0] = too_long ? 1 : 0;
      planned = too_long ? 0 : plan_times(time, step_time, duration, times_s, chunk);
      cnt_s[0] = planned;
   }
   __syncthreads();
   if (long_s[0])      // (workgroup-uniform)
   {
      if (tid == 0)
      {
         v.key_out[run] = ORC_VERDICT_NONE; v.time_out[run] = -1.0;
         if (v.long_marks_run) v.n_samples_out[run] = ORC_VERDICT_TOO_LONG;
         else { v.n_samples_out[run] = 0; *v.too_long = 1; }
      }
      return;
   }
   if (planner && tid - ORC_VD_WORKERS < cnt_s[0])
   {
      const int k = tid - ORC_VD_WORKERS;
      seg_s[k] = plan_locate(times_s[k], np, dtm_s, tstart_s, u_s[k]);
   }
   __syncthreads();

   double my_depth = 0.0; unsigned long long my_key = ORC_VERDICT_NONE;
   int ci = 0;                                               // the chunk the workers walk; the planner fills the other buffer with the next
   for (;; ci++)
   {
      const int buf = (ci & 1) * chunk, nbuf = chunk - buf;
      const int count = cnt_s[ci & 1];
      if (count == 0) break;
      const int sbase = ci * chunk;                          // (samples before this chunk)
      if (tid == ORC_VD_WORKERS)
      {
         const int more = plan_times(time, step_time, duration, times_s + nbuf, chunk);
         cnt_s[(ci + 1) & 1] = more;
         planned += more;
      }
      if (!planner) verdict_rows(traj, seg_s, u_s, buf, count, n, tid, L);
      __syncthreads();
      if (planner && tid - ORC_VD_WORKERS < cnt_s[(ci + 1) & 1])
      {
         const int k = nbuf + tid - ORC_VD_WORKERS;
         seg_s[k] = plan_locate(times_s[k], np, dtm_s, tstart_s, u_s[k]);
      }
      verdict_renormalise(mod, count, tid, L);      // (tid < count: workers)
      __syncthreads();
      if (!planner) verdict_fk<real, TREE>(mod, count, tid, L);
      __syncthreads();
      if (!planner) verdict_tests<real>(v, mod, sdfs, n_fields, sbase, count, tid, L, my_key, my_depth, key_s);
      __syncthreads();
      const bool done = key_s[0] != ORC_VERDICT_NONE || count < chunk;      // a contact in this chunk: later samples cannot come first
      __syncthreads();
      if (done) break;
   }
   // the samples behind a contact are counted all the same, when the caller wants their number; a run that is too long only
   // by that count and must not fail the call reports nothing of its walk (kernel arguments: the same for every workgroup)
   if (v.count_rest && v.long_marks_run)
   {
      if (tid == ORC_VD_WORKERS)
      {
         planned = plan_count_rest(time, step_time, duration, planned);
         long_s[0] = planned >= ORC_VD_MAX_SAMPLES ? 1 : 0;
      }
      __syncthreads();
      if (long_s[0])
      {
         if (tid == 0) { v.key_out[run] = ORC_VERDICT_NONE; v.time_out[run] = -1.0; v.n_samples_out[run] = ORC_VERDICT_TOO_LONG; }
         return;
      }
   }
   const unsigned long long first = key_s[0];
   if (tid == 0)
   {
      v.key_out[run] = first;
      // (the chunk of the first contact is the last one walked: its times are still in its buffer)
      v.time_out[run] = (first != ORC_VERDICT_NONE) ? times_s[(ci & 1) * chunk + ((int)(first >> 32) - ci * chunk)] : -1.0;
   }
   if (first != ORC_VERDICT_NONE && my_key == first) v.depth_out[run] = my_depth;
   if (tid == ORC_VD_WORKERS)
   {
      if (v.count_rest && !v.long_marks_run)
      {
         planned = plan_count_rest(time, step_time, duration, planned);
         if (planned >= ORC_VD_MAX_SAMPLES) *v.too_long = 1;
      }
      v.n_samples_out[run] = planned;
   }
}

} // namespace

// One launcher for either kernel's two instantiations of a precision; the dynamic-LDS attribute is per device and per
// kernel, and set for both on a device's first launch.
template <typename Args, void (*KTREE)(Args), void (*KCHAIN)(Args)>
static hipError_t launch_verdict_kernels(const Args & v, int block, size_t lds, hipStream_t stream, int tree)
{
   static std::atomic<unsigned long long> attr_set{0ull};
   int dev = 0;
   if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
   if (!((attr_set.load() >> dev) & 1ull))
   {
      hipError_t e = hipFuncSetAttribute((const void *) KTREE, hipFuncAttributeMaxDynamicSharedMemorySize, 160*1024 - 256);
      if (e == hipSuccess) e = hipFuncSetAttribute((const void *) KCHAIN, hipFuncAttributeMaxDynamicSharedMemorySize, 160*1024 - 256);
      if (e != hipSuccess) return e;
      attr_set.fetch_or(1ull << dev);
   }
   if (lds > 160*1024 - 256) return hipErrorInvalidValue;
   if (tree) hipLaunchKernelGGL(KTREE, dim3(v.n_runs), dim3(block), lds, stream, v);
   else hipLaunchKernelGGL(KCHAIN, dim3(v.n_runs), dim3(block), lds, stream, v);
   return hipGetLastError();
}

template <typename real>
static hipError_t launch_verdict_t(const DevVerdict<real> & v, size_t lds, hipStream_t stream, int tree)
{
   return launch_verdict_kernels<DevVerdict<real>, collision_verdict_kernel<real, true>, collision_verdict_kernel<real, false>>(v, ORC_BLOCK, lds, stream, tree);
}
hipError_t orc_launch_verdict(const DevVerdict<double> & v, size_t lds, hipStream_t stream, int tree) { return launch_verdict_t<double>(v, lds, stream, tree); }
hipError_t orc_launch_verdict(const DevVerdict<float> & v, size_t lds, hipStream_t stream, int tree) { return launch_verdict_t<float>(v, lds, stream, tree); }

template <typename real>
static hipError_t launch_verdict_planned_t(const DevVerdictPlan<real> & v, size_t lds, hipStream_t stream, int tree)
{
   if (v.n_points < 2 || v.chunk < 4 || v.chunk > 64 || (v.chunk & 3)) return hipErrorInvalidValue;
   return launch_verdict_kernels<DevVerdictPlan<real>, collision_verdict_planned_kernel<real, true>, collision_verdict_planned_kernel<real, false>>(v, ORC_VD_BLOCK, lds, stream, tree);
}
hipError_t orc_launch_verdict_planned(const DevVerdictPlan<double> & v, size_t lds, hipStream_t stream, int tree) { return launch_verdict_planned_t<double>(v, lds, stream, tree); }
hipError_t orc_launch_verdict_planned(const DevVerdictPlan<float> & v, size_t lds, hipStream_t stream, int tree) { return launch_verdict_planned_t<float>(v, lds, stream, tree); }

// dynamic LDS of the kernels (the carve-ups at their tops): the kernel's header, in the planned kernel the plan's arrays, then
// what the walk holds
size_t orc_verdict_lds_bytes(int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk)
{
   return 16 + verdict_walk_lds_bytes(n, Sa, Sa_real, nj, real_size, chunk);
}
size_t orc_verdict_planned_lds_bytes(int n_points, int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk)
{
   const size_t plan = (size_t) ORC_VD_HEADER + ((size_t) 4*chunk + (size_t) 2*n_points) * sizeof(double) + (size_t) 2*chunk * sizeof(int);
   return plan + verdict_walk_lds_bytes(n, Sa, Sa_real, nj, real_size, chunk);
}
