// verdict_planned.h -- the device-planned walk over a run's samples, once, for the two kernels made of it:
// collision_verdict_planned_kernel (verdict_kernels.hip), which stops at the first contact, and clearance_kernel
// (clearance_kernels.hip), which goes to the end.  One workgroup per run, ORC_VP_BLOCK threads: a fifth wavefront, the
// planner, retimes the run and steps the sample times a chunk ahead (verdict_plan.h: the host's arithmetic) of the four
// wavefronts that walk them (verdict_walk.h).  The two kernels look at exactly the same samples because this text is
// compiled into both.
//
// Included inside the including file's namespace after <atomic>, verdict_plan.h, run_candidate.h and verdict_walk.h, with the
// contraction of the walk in force.  Nothing here is floating-point arithmetic: the plan's is verdict_plan.h's, under
// contract(off), and the walk's is verdict_walk.h's.  A kernel calls, in this order and with nothing that returns early
// in between: planned_examined, planned_lds, its own verdict_stage and the first values of its header, planned_prologue,
// planned_walk.
#pragma once

#define ORC_VP_WORKERS ORC_BLOCK            // threads that walk the samples (verdict_walk.h)
#define ORC_VP_BLOCK   (ORC_BLOCK + 64)     // ... and the planner's wavefront
#define ORC_VP_FLAGS   16                   // byte of a kernel's LDS header at which the plan's three ints sit (the 16 before: the kernel's keys)

// Is the run examined at all?  One answer for the workgroup (the run is the block's index and the tables are read at that
// index, a uniform address; readfirstlane makes the branch a scalar one whatever loads the compiler picks).  Taken before
// anything is staged and before the first barrier: the workgroup of a run that is not examined writes its report and returns.
template <typename real>
__device__ __forceinline__ bool planned_examined(const DevVerdictPlanned<real> & v, int run)
{
   if (!v.examine && !v.cand_status) return true;
   const int walk = v.examine ? (v.examine[run] != 0) : (orc_run_candidate(v.cand_status[run], v.cand_costs[(size_t) run*3]) ? 1 : 0);
   return __builtin_amdgcn_readfirstlane(walk) != 0;
}

// the plan's part of a workgroup's dynamic LDS: three ints in the kernel's header, its arrays behind the header, then the walk's
template <typename real>
struct PlannedLds
{
   int * cnt_s;          // [2] samples in either chunk buffer
   int * long_s;         // [1] the run has too many samples
   double * times_s;     // [2][chunk]
   double * u_s;         // [2][chunk]
   double * dtm_s;       // [n_points]
   double * tstart_s;    // [n_points]
   int * seg_s;          // [2][chunk]
   VerdictLds<real> walk;
};

template <typename real>
__device__ __forceinline__ PlannedLds<real> planned_lds(unsigned char * smem, int header, const DevModel<real> & gmod, int np, int n, int chunk)
{
   PlannedLds<real> P;
   P.cnt_s = (int *)(smem + ORC_VP_FLAGS);
   P.long_s = P.cnt_s + 2;
   P.times_s = (double *)(smem + header);
   P.u_s = P.times_s + 2*chunk;
   P.dtm_s = P.u_s + 2*chunk;
   P.tstart_s = P.dtm_s + np;
   P.seg_s = (int *)(P.tstart_s + np);
   P.walk = verdict_lds((unsigned char *)(P.seg_s + 2*chunk), gmod, n, chunk);
   return P;
}

// bytes of that carve-up behind a header of `header` bytes (32 at least, a multiple of 8)
inline size_t planned_lds_bytes(size_t header, int n_points, int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk)
{
   const size_t plan = header + ((size_t) 4*chunk + (size_t) 2*n_points) * sizeof(double) + (size_t) 2*chunk * sizeof(int);
   return plan + verdict_walk_lds_bytes(n, Sa, Sa_real, nj, real_size, chunk);
}

// what either launcher refuses of the shared arguments
template <typename real>
inline bool planned_args_ok(const DevVerdictPlanned<real> & v) { return v.n_points >= 2 && v.chunk >= 4 && v.chunk <= 64 && !(v.chunk & 3); }

// the clock: the planner's first lane keeps it, in the other threads it stays as it starts
struct PlannedClock
{
   double time, step_time, duration;
   int planned;          // samples laid so far
};

// segment and position of the sample in place k of the chunk buffers (a lane of the planner each)
template <typename real>
__device__ __forceinline__ void planned_locate(int k, int np, const PlannedLds<real> & P)
{
   P.seg_s[k] = plan_locate(P.times_s[k], np, P.dtm_s, P.tstart_s, P.u_s[k]);
}

// The prologue: a lane per segment, then one lane for the sums that have an order, the too-long rule against `cap`, the
// times of the first chunk and their segments.  Returns whether the run is too long, one answer for the workgroup: then
// nothing is walked, and the kernel writes its report and returns.  Holds the workgroup's first three barriers; what the
// kernel staged before the call is visible after it.
template <typename real>
__device__ __forceinline__ bool planned_prologue(const DevVerdictPlanned<real> & v, const real * traj, int cap, int tid, const PlannedLds<real> & P, PlannedClock & c)
{
   const int n = v.n, np = v.n_points, chunk = v.chunk;
   if (tid == 0) P.dtm_s[0] = 0.0;
   for (int i=1+tid; i<np; i+=ORC_VP_BLOCK) plan_segment(traj, i, n, v.col0, v.vmax, P.dtm_s[i], P.tstart_s[i]);
   __syncthreads();
   c.time = 0.0; c.step_time = 0.0; c.duration = 0.0; c.planned = 0;
   if (tid == ORC_VP_WORKERS)
   {
      double total_dist;
      plan_totals(np, P.dtm_s, P.tstart_s, total_dist, c.duration);
      c.step_time = plan_step_time(total_dist, c.duration);
      const bool too_long = plan_too_long(total_dist, c.step_time, c.duration, cap);
      P.long_s[0] = too_long ? 1 : 0;
      c.planned = too_long ? 0 : plan_times(c.time, c.step_time, c.duration, P.times_s, chunk);
      P.cnt_s[0] = c.planned;
   }
   __syncthreads();
   if (P.long_s[0]) return true;      // (workgroup-uniform)
   if (tid >= ORC_VP_WORKERS && tid - ORC_VP_WORKERS < P.cnt_s[0]) planned_locate(tid - ORC_VP_WORKERS, np, P);
   __syncthreads();
   return false;
}

// The chunk loop: the workers walk chunk ci while the planner fills the other buffer with the next.  What is done with a
// chunk's items and whether the walk may end before the samples do is the kernel's, its policy:
//    tests(sbase, count, times)   the workers' call on the chunk's `count` samples: the run's samples sbase .., their times
//    STOPS, stop_word             a compile-time property: the walk ends behind the chunk in which tests set the shared word
//                                 *stop_word (LDS) to anything but ORC_VERDICT_NONE -- a contact: later samples cannot come first
// A policy that does not stop pays neither the second barrier of a chunk's end nor the look at the shared word.  Returns the
// chunk the walk ended in: the last one walked when it stopped or ran out in a partial chunk, whose times are still in
// buffer `ci & 1`.
template <typename real, bool TREE, bool STOPS, typename Tests>
__device__ __forceinline__ int planned_walk(const DevVerdictPlanned<real> & v, const ModelView<real> & mod, const real * traj, int tid,
   const PlannedLds<real> & P, PlannedClock & c, const unsigned long long * stop_word, Tests && tests)
{
   const int n = v.n, np = v.n_points, chunk = v.chunk;
   const bool planner = tid >= ORC_VP_WORKERS;
   const VerdictLds<real> & L = P.walk;
   int ci = 0;
   for (;; ci++)
   {
      const int buf = (ci & 1) * chunk, nbuf = chunk - buf;
      const int count = P.cnt_s[ci & 1];
      if (count == 0) break;
      if (tid == ORC_VP_WORKERS)
      {
         const int more = plan_times(c.time, c.step_time, c.duration, P.times_s + nbuf, chunk);
         P.cnt_s[(ci + 1) & 1] = more;
         c.planned += more;
      }
      if (!planner) verdict_rows(traj, P.seg_s, P.u_s, buf, count, n, tid, L);
      __syncthreads();
      if (planner && tid - ORC_VP_WORKERS < P.cnt_s[(ci + 1) & 1]) planned_locate(nbuf + tid - ORC_VP_WORKERS, np, P);
      verdict_renormalise(mod, count, tid, L);      // (tid < count: workers)
      __syncthreads();
      if (!planner) verdict_fk<real, TREE>(mod, count, tid, L);
      __syncthreads();
      if (!planner) tests(ci * chunk, count, P.times_s + buf);
      __syncthreads();      // (the next pass writes the rows, and the pass after it this chunk's times)
      if constexpr (STOPS)
      {
         const bool done = *stop_word != ORC_VERDICT_NONE || count < chunk;
         __syncthreads();
         if (done) break;
      }
      else if (count < chunk) break;
   }
   return ci;
}

// One launcher for a kernel's two instantiations of a precision (host code: the including file has <atomic>); the dynamic-LDS
// attribute is per device and per kernel, and set for both on a device's first launch.
template <typename Args, void (*KTREE)(Args), void (*KCHAIN)(Args)>
static hipError_t launch_verdict_kernels(const Args & v, int block, size_t lds, hipStream_t stream, int tree)
{
   static std::atomic<unsigned long long> attr_set{0ull};
   int dev = 0;
   if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
   if (!((attr_set.load() >> dev) & 1ull))
   {
      hipError_t e = hipFuncSetAttribute((const void *) KTREE, hipFuncAttributeMaxDynamicSharedMemorySize, ORC_VERDICT_LDS_LIMIT);
      if (e == hipSuccess) e = hipFuncSetAttribute((const void *) KCHAIN, hipFuncAttributeMaxDynamicSharedMemorySize, ORC_VERDICT_LDS_LIMIT);
      if (e != hipSuccess) return e;
      attr_set.fetch_or(1ull << dev);
   }
   if (lds > ORC_VERDICT_LDS_LIMIT) return hipErrorInvalidValue;
   if (tree) hipLaunchKernelGGL(KTREE, dim3(v.n_runs), dim3(block), lds, stream, v);
   else hipLaunchKernelGGL(KCHAIN, dim3(v.n_runs), dim3(block), lds, stream, v);
   return hipGetLastError();
}
