// verdict_kernels.hip -- the collision verdict of a batch: the first contact of every run's trajectory with a field of its
// scene or of the robot with itself, on a sample every 0.04 rad of C-space distance along the retimed trajectory, as the
// reference's re-check in gettraj (src/orcdchomp_mod.cpp:2958-3006).  One workgroup per run walks the run's samples up to
// 64 at a time (DevVerdictWalk::chunk); the walk is verdict_walk.h, and both kernels here are made of it.
//
// collision_verdict_kernel (orc_batch_collision_verdict, gettraj's own re-check) walks samples the host planned:
// Module::batch_collision_verdict reads every trajectory back, retimes it (retime_linear), lays the samples
// (plan_collision_samples) and uploads the list.  In collision_verdict_planned_kernel (orc_batch_collision_verdict_device,
// orc_batch_select_best with require_collision_free, orc_batch_respawn) the run's workgroup does that itself, so no
// trajectory leaves the device and no sample list exists: the kernel is a shell around the planned walk of
// verdict_planned.h (the examined-run decision, the plan's LDS, the prologue, the chunk loop with the planner wavefront),
// which clearance_kernels.hip shares.  What is the verdict's own stays here: the policy that runs verdict_tests and stops
// behind the chunk of the first contact, the count of the samples behind a contact, and what is written back.
//
// The planning arithmetic is the host's, rounding for rounding (verdict_plan.h; module.py verdict_samples is its
// specification): doubles for either precision, no fused multiply-add, the sums in index order, time advanced by repeated
// addition.
#include <hip/hip_runtime.h>
#include <math.h>
#include <atomic>
#include "dev_types.h"
#include "verdict_device.h"
#include "run_candidate.h"

#define ORC_VD_HEADER  32                   // bytes of the planned kernel's LDS header: the first contact's key, 8 unused, the plan's flags (verdict_planned.h)

// ---- the plan: the host's arithmetic (module.cpp retime_linear, plan_collision_samples) ----------------------------------
#pragma clang fp contract(off)
namespace {

#include "verdict_plan.h"

} // namespace

// ---- the walk (verdict_walk.h), the planned walk (verdict_planned.h) and the two kernels around them ----------------------------------------------------------------
#pragma clang fp contract(fast)
namespace {

#include "sdf_lookup.h"
#include "fk.h"
#include "verdict_walk.h"
#include "verdict_planned.h"

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

// what a run that was not walked reports (tid 0)
template <typename real>
__device__ __forceinline__ void verdict_not_walked(const DevVerdictPlan<real> & v, int run, int mark)
{
   v.key_out[run] = ORC_VERDICT_NONE; v.time_out[run] = -1.0; v.n_samples_out[run] = mark;
}

template <typename real, bool TREE>
__global__ __launch_bounds__(ORC_VP_BLOCK)
void collision_verdict_planned_kernel(DevVerdictPlan<real> v)
{
   extern __shared__ __align__(16) unsigned char smem_raw[];
   const DevModel<real> & gmod = *v.model;
   const int run = blockIdx.x, tid = threadIdx.x;
   if (!planned_examined<real>(v, run))
   {
      if (tid == 0) verdict_not_walked(v, run, ORC_VERDICT_SKIPPED);
      return;
   }
   const int n = v.n, np = v.n_points, chunk = v.chunk;
   const DevSdf<real> * sdfs; int n_fields;
   verdict_scene<real>(v, run, sdfs, n_fields);
   unsigned long long * key_s = (unsigned long long *) smem_raw;     // [1]: the first contact's key (DevVerdictWalk::key_out)
   const PlannedLds<real> P = planned_lds(smem_raw, ORC_VD_HEADER, gmod, np, n, chunk);
   verdict_stage<real, ORC_VP_BLOCK>(gmod, v.slot_xml, P.walk, tid);
   if (tid == 0) key_s[0] = ORC_VERDICT_NONE;
   const ModelView<real> mod = verdict_model_view(gmod, n, P.walk);

   const real * traj = v.traj + (size_t) run * np * n;
   PlannedClock c;
   if (planned_prologue<real>(v, traj, ORC_VD_MAX_SAMPLES, tid, P, c))
   {
      if (tid == 0)
      {
         verdict_not_walked(v, run, v.long_marks_run ? ORC_VERDICT_TOO_LONG : 0);
         if (!v.long_marks_run) *v.too_long = 1;
      }
      return;
   }
   // the walk's policy: the verdict's tests, and a stop behind the chunk of the first contact
   double my_depth = 0.0; unsigned long long my_key = ORC_VERDICT_NONE;
   const int ci = planned_walk<real, TREE, true>(v, mod, traj, tid, P, c, key_s, [&](int sbase, int count, const double *) {
      verdict_tests<real>(v, mod, sdfs, n_fields, sbase, count, tid, P.walk, my_key, my_depth, key_s); });
   // the samples behind a contact are counted all the same, when the caller wants their number; a run that is too long only
   // by that count and must not fail the call reports nothing of its walk (kernel arguments: the same for every workgroup)
   if (v.count_rest && v.long_marks_run)
   {
      if (tid == ORC_VP_WORKERS)
      {
         c.planned = plan_count_rest(c.time, c.step_time, c.duration, c.planned);
         P.long_s[0] = c.planned >= ORC_VD_MAX_SAMPLES ? 1 : 0;
      }
      __syncthreads();
      if (P.long_s[0])
      {
         if (tid == 0) verdict_not_walked(v, run, ORC_VERDICT_TOO_LONG);
         return;
      }
   }
   const unsigned long long first = key_s[0];
   if (tid == 0)
   {
      v.key_out[run] = first;
      // (the chunk of the first contact is the last one walked: its times are still in its buffer)
      v.time_out[run] = (first != ORC_VERDICT_NONE) ? P.times_s[(ci & 1) * chunk + ((int)(first >> 32) - ci * chunk)] : -1.0;
   }
   if (first != ORC_VERDICT_NONE && my_key == first) v.depth_out[run] = my_depth;
   if (tid == ORC_VP_WORKERS)
   {
      if (v.count_rest && !v.long_marks_run)
      {
         c.planned = plan_count_rest(c.time, c.step_time, c.duration, c.planned);
         if (c.planned >= ORC_VD_MAX_SAMPLES) *v.too_long = 1;
      }
      v.n_samples_out[run] = c.planned;
   }
}

} // namespace

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
   if (!planned_args_ok<real>(v)) return hipErrorInvalidValue;
   return launch_verdict_kernels<DevVerdictPlan<real>, collision_verdict_planned_kernel<real, true>, collision_verdict_planned_kernel<real, false>>(v, ORC_VP_BLOCK, lds, stream, tree);
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
   return planned_lds_bytes(ORC_VD_HEADER, n_points, n, Sa, Sa_real, nj, real_size, chunk);
}
