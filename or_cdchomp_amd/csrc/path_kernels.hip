// path_kernels.hip -- the clearance of given paths and of segments between waypoints (orc_batch_path_clearance,
// orc_batch_waypoint_segment_clearance): what clearance_kernel (clearance_kernels.hip) reports for a run that holds the path as
// its trajectory, for paths that are no run's.  Where that kernel gives every run a workgroup of its own, whose chunks a short
// path leaves mostly empty, the samples of all queries are laid into one list here and a workgroup walks `chunk` consecutive
// entries of it, whichever queries they belong to (path_device.h has the four kernels and their order).
//
// The plan is verdict_plan.h's arithmetic under contract(off), in doubles for either precision: plan_step_time, plan_too_long
// and the clock's repeated addition are its functions; the segment's time and length are plan_segment's statements on two row
// pointers (the rows of a waypoint segment are not adjacent in memory); and a lane that walks its own clock forwards finds
// the sample's segment by moving on while `tstart[seg + 1] < time`, the loop of module.py verdict_samples, which gives what
// plan_locate's bisection gives because tstart does not decrease.  So no table of a query's segments is kept anywhere, and
// the rows of a query may be many.
//
// The walk is verdict_walk.h's text: verdict_stage, the rows by verdict_rows' expression on the query's own rows,
// verdict_renormalise, verdict_fk; then, as in config_clearance_kernel (config_kernels.hip), the wavefront that ran FK for an
// entry tests it with its 64 lanes and reduces by shuffles.  An entry's answer is its wavefront's alone, and a query's the
// minimum over its entries in sample order, taken by one wavefront: nothing depends on what shares a chunk, on a query's place
// in the list or on the round it fell into.  No floating-point atomic, no atomic at all.
#include <hip/hip_runtime.h>
#include <math.h>
#include <atomic>
#include "dev_types.h"
#include "config_device.h"   // config_query.h is written against it
#include "path_device.h"

#define ORC_PATH_LANES 256                  // queries per workgroup of the count and fill kernels

#pragma clang fp contract(off)
namespace {

#include "verdict_plan.h"

// the run a query names
template <typename real>
__device__ __forceinline__ int path_run(const DevPathClearance<real> & v, int q) { return v.run_of_q ? v.run_of_q[q] : 0; }

// row i of query q: of the uploaded rows, or the waypoint `from` (i 0) or `to` (i 1) of the query's run
template <typename real>
__device__ __forceinline__ const real * path_row(const DevPathClearance<real> & v, int q, int i)
{
   if (v.paths) return v.paths + ((size_t) q * v.n_rows + i) * v.n;
   const int point = i ? v.to_of_q[q] : v.from_of_q[q];
   return v.traj + ((size_t) path_run(v, q) * v.n_points + point) * v.n;
}

// plan_segment (verdict_plan.h) on two row pointers: the same statements in the same order
template <typename real>
__device__ __forceinline__ void path_segment(const real * lo_row, const real * hi_row, int n, int col0, const double * vmax, double & dtm, double & len)
{
   double dt = 0.0, d2 = 0.0;
   for (int j=col0; j<n; j++)
   {
      const double lo = (double) lo_row[j], hi = (double) hi_row[j];
      const double v = vmax[j-col0] > 0.0 ? vmax[j-col0] : 1.0;
      const double c = ::fabs(hi - lo) / v;
      dt = dt < c ? c : dt;                  // std::max(dt, c): a NaN candidate is ignored
      const double d = lo - hi;
      d2 += d*d;
   }
   dtm = dt; len = ::sqrt(d2);
}

struct PathPlan
{
   double duration, step_time;
   bool too_long;
};

// plan_totals' two sums in index order, the step and the too-long rule
template <typename real>
__device__ __forceinline__ PathPlan path_plan(const DevPathClearance<real> & v, int q)
{
   double td = 0.0, du = 0.0;
   for (int i=1; i<v.n_rows; i++)
   {
      double dtm, len;
      path_segment<real>(path_row(v, q, i-1), path_row(v, q, i), v.n, v.col0, v.vmax, dtm, len);
      td += len;
      du += dtm;
   }
   PathPlan p;
   p.duration = du;
   p.step_time = plan_step_time(td, du);
   p.too_long = plan_too_long(td, p.step_time, du, v.max_samples);
   return p;
}

// a lane per query: is it too long, and how many samples has it (a query the rule passes has max_samples + 2 at most; the
// bound is held here too, so that what the fill kernel writes stays inside the workspace whatever the rows hold)
template <typename real>
__global__ __launch_bounds__(ORC_PATH_LANES)
void path_count_kernel(DevPathClearance<real> v)
{
   const int q = blockIdx.x * ORC_PATH_LANES + threadIdx.x;
   if (q >= v.n_q) return;
   const PathPlan p = path_plan<real>(v, q);
   int k = ORC_VERDICT_TOO_LONG;
   if (!p.too_long)
   {
      double time = 0.0;
      k = 0;
      while (k < v.max_samples + 2 && time < p.duration) { time += p.step_time; k++; }
   }
   v.count[q] = k;
}

// a lane per query: its samples into the list, count[q] entries from offs[q] on
template <typename real>
__global__ __launch_bounds__(ORC_PATH_LANES)
void path_fill_kernel(DevPathClearance<real> v)
{
   const int q = blockIdx.x * ORC_PATH_LANES + threadIdx.x;
   if (q >= v.n_q) return;
   const int cnt = v.count[q];
   if (cnt <= 0) return;
   const PathPlan p = path_plan<real>(v, q);
   const size_t e0 = (size_t) v.offs[q];
   // the segment the clock is on: tstart[seg], dtm[seg + 1] and their sum tstart[seg + 1], as plan_totals adds them
   int seg = 0;
   double tseg0 = 0.0, dnext, len;
   path_segment<real>(path_row(v, q, 0), path_row(v, q, 1), v.n, v.col0, v.vmax, dnext, len);
   double time = 0.0;
   for (int k=0; k<cnt; k++)
   {
      while (seg < v.n_rows - 2 && tseg0 + dnext < time)
      {
         tseg0 += dnext;
         seg++;
         path_segment<real>(path_row(v, q, seg), path_row(v, q, seg+1), v.n, v.col0, v.vmax, dnext, len);
      }
      v.e_query[e0 + k] = q;
      v.e_seg[e0 + k] = seg;
      v.e_u[e0 + k] = dnext > 0.0 ? (time - tseg0) / dnext : 0.0;
      v.e_time[e0 + k] = time;
      time += p.step_time;
   }
}

} // namespace

#pragma clang fp contract(fast)
namespace {

#include "sdf_lookup.h"
#include "fk.h"
#include "verdict_walk.h"
#include "wave.h"           // config_query.h's wave_min
#include "config_query.h"   // ConfigMin, config_offer, config_tests: the per-sample tests of config_clearance_kernel

// The spheres of sample s whose centres are finite, as a mask over the slots (a slot per lane; Sa <= 64 as live_mask has it).
// A row with a NaN entry went through FK: the spheres it moves have NaN centres, whose gaps would be NaN or +inf, which no
// minimum takes -- and the cell such a centre would be looked up in is anybody's guess.  They are taken out of the live mask of
// this sample instead, so that nothing is indexed by them.
template <typename real>
__device__ __forceinline__ unsigned long long path_finite_slots(int Sa, int s, int lane, const VerdictLds<real> & L)
{
   const real inf = M<real>::inf();
   bool ok = false;
   if (lane < Sa)
   {
      const real * p = L.pos_s + s*L.pstr + lane*3;
      ok = M<real>::fabs_(p[0]) < inf && M<real>::fabs_(p[1]) < inf && M<real>::fabs_(p[2]) < inf;
   }
   return __ballot(ok);
}

// the wavefront's minimum of a leg of an entry and the lowest key at it, written by the lane that holds that item
template <typename real>
__device__ __forceinline__ void path_report(const ConfigMin<real> & m, int lane, double * gap_out, unsigned int * key_out)
{
   const real lowest = wave_min<real>(m.val);
   const bool mine = m.key != ORC_PATH_NONE && m.val == lowest;
   unsigned int key = mine ? m.key : ORC_PATH_NONE;
   for (int d=32; d>=1; d>>=1) { const unsigned int o = __shfl_xor(key, d); key = o < key ? o : key; }
   if (key == ORC_PATH_NONE)
   {
      if (lane == 0) { *gap_out = (double) M<real>::inf(); *key_out = ORC_PATH_NONE; }
   }
   else if (mine && m.key == key) { *gap_out = (double) m.val; *key_out = key; }      // (one lane: an item belongs to one lane)
}

// bytes of the kernel's LDS header before the walk's part: per entry its query and its run
__host__ __device__ inline size_t path_walk_header_bytes(int chunk) { return (size_t) chunk * 8; }

template <typename real, bool TREE>
__global__ __launch_bounds__(ORC_BLOCK)
void path_walk_kernel(DevPathClearance<real> v)
{
   extern __shared__ __align__(16) unsigned char smem_raw[];
   const DevModel<real> & gmod = *v.model;
   const int tid = threadIdx.x, lane = tid & 63;
   const int n = v.n, chunk = v.chunk;
   const int e0 = blockIdx.x * chunk;
   const int count = (v.n_entries - e0 < chunk) ? v.n_entries - e0 : chunk;      // (the launcher's grid: count >= 1)
   int * run_s = (int *) smem_raw;                  // [chunk] the run of the entry's query
   const VerdictLds<real> L = verdict_lds(smem_raw + path_walk_header_bytes(chunk), gmod, n, chunk);
   verdict_stage<real, ORC_BLOCK>(gmod, v.slot_xml, L, tid);
   const ModelView<real> mod = verdict_model_view(gmod, n, L);
   if (tid < count) run_s[tid] = v.run_of_q ? v.run_of_q[v.e_query[e0 + tid]] : 0;
   // the rows: verdict_rows' expression, every entry on the rows of its own query
   for (int e=tid; e<count*n; e+=ORC_BLOCK)
   {
      const int s = e / n, c = e - s*n;
      const int q = v.e_query[e0 + s], sg = v.e_seg[e0 + s];
      const real uu = (real) v.e_u[e0 + s];
      real a0, a1;
      if (v.paths)
      {
         const real * row = v.paths + ((size_t) q * v.n_rows + sg) * n;
         a0 = row[c]; a1 = row[n + c];
      }
      else
      {
         const real * run_rows = v.traj + (size_t)(v.run_of_q ? v.run_of_q[q] : 0) * v.n_points * n;
         a0 = run_rows[(size_t) v.from_of_q[q]*n + c]; a1 = run_rows[(size_t) v.to_of_q[q]*n + c];
      }
      L.rows_s[s*n + c] = a0 + (a1 - a0) * uu;
   }
   __syncthreads();
   verdict_renormalise(mod, count, tid, L);      // (tid < count)
   __syncthreads();
   verdict_fk<real, TREE>(mod, count, tid, L);
   // what the wavefront's lanes stored for its 20 entries is read by its other lanes: a wavefront's LDS operations execute in
   // program order, and the compiler keeps them on their side of this point
   __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
   __builtin_amdgcn_wave_barrier();
   __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
   const int s_begin = (tid >> 6) * 20;
   const int s_end = (s_begin + 20 < count) ? s_begin + 20 : count;
   for (int s=s_begin; s<s_end; s++)
   {
      const size_t e = (size_t)(e0 + s);
      const DevSdf<real> * sdfs; int n_fields;
      verdict_scene<real>(v, __builtin_amdgcn_readfirstlane(run_s[s]), sdfs, n_fields);
      ConfigMin<real> best[2];      // [0] fields, [1] pairs
      for (int leg=0; leg<2; leg++) { best[leg].val = M<real>::inf(); best[leg].key = ORC_PATH_NONE; }
      ModelView<real> seen = mod;      // (config_tests reads Sa and live_mask of it)
      seen.live_mask &= path_finite_slots<real>(mod.Sa, s, lane, L);
      config_tests<real>(v, seen, sdfs, n_fields, s, lane, L, best[0], best[1]);
      for (int leg=0; leg<2; leg++) path_report<real>(best[leg], lane, v.e_gap + e*2 + leg, v.e_key + e*2 + leg);
   }
}

// a wavefront per query: the minimum over its entries, which reach a lane in ascending sample order (`<` keeps the lowest
// sample), then over the lanes with the lowest key among equals -- clearance_kernel's rule
template <typename real>
__global__ __launch_bounds__(ORC_BLOCK)
void path_reduce_kernel(DevPathClearance<real> v)
{
   const int lane = threadIdx.x & 63;
   const int q = blockIdx.x * (ORC_BLOCK / 64) + (threadIdx.x >> 6);
   if (q >= v.n_q) return;      // (wave-uniform)
   const int cnt = v.count[q];
   if (cnt < 0)
   {
      if (lane < 2)
      {
         v.clear_out[(size_t) q*2 + lane] = __longlong_as_double(0x7ff8000000000000LL);
         v.ckey_out[(size_t) q*2 + lane] = ORC_VERDICT_NONE;
         v.ctime_out[(size_t) q*2 + lane] = -1.0;
      }
      if (lane == 0) v.n_samples_out[q] = cnt;
      return;
   }
   const size_t e0 = cnt ? (size_t) v.offs[q] : 0;
   for (int leg=0; leg<2; leg++)
   {
      double val = M<double>::inf(), time = -1.0;
      unsigned long long key = ORC_VERDICT_NONE;
      for (int i=lane; i<cnt; i+=64)
      {
         const double gap = v.e_gap[(e0 + i)*2 + leg];
         const unsigned int k = v.e_key[(e0 + i)*2 + leg];
         if (k != ORC_PATH_NONE && gap < val)
         {
            val = gap;
            key = ((unsigned long long) i << 32) | (unsigned long long) k;
            time = v.e_time[e0 + i];
         }
      }
      const double lowest = wave_min<double>(val);
      const bool mine = key != ORC_VERDICT_NONE && val == lowest;
      unsigned long long first = mine ? key : ORC_VERDICT_NONE;
      for (int d=32; d>=1; d>>=1) { const unsigned long long o = __shfl_xor(first, d); first = o < first ? o : first; }
      if (first == ORC_VERDICT_NONE)
      {
         if (lane == 0)
         {
            v.clear_out[(size_t) q*2 + leg] = M<double>::inf();
            v.ckey_out[(size_t) q*2 + leg] = ORC_VERDICT_NONE;
            v.ctime_out[(size_t) q*2 + leg] = -1.0;
         }
      }
      else if (mine && key == first)      // (one lane: an entry belongs to one lane)
      {
         v.clear_out[(size_t) q*2 + leg] = val;
         v.ckey_out[(size_t) q*2 + leg] = first;
         v.ctime_out[(size_t) q*2 + leg] = time;
      }
   }
   if (lane == 0) v.n_samples_out[q] = cnt;
}

} // namespace

template <typename real>
static bool path_args_ok(const DevPathClearance<real> & v)
{
   if (v.n_q < 1 || v.n_q > ORC_PATH_MAX_Q || v.n_rows < 2 || v.n_rows > ORC_PATH_MAX_ROWS) return false;
   if (v.max_samples < 1 || v.max_samples > (1 << 20)) return false;
   if (!v.paths && (v.n_rows != 2 || !v.from_of_q || !v.to_of_q)) return false;
   return v.n >= 1 && v.col0 >= 0 && v.col0 < v.n && v.vmax && v.count;
}

template <typename real>
static hipError_t launch_path_count_t(const DevPathClearance<real> & v, hipStream_t stream)
{
   if (!path_args_ok(v)) return hipErrorInvalidValue;
   const int blocks = (v.n_q + ORC_PATH_LANES - 1) / ORC_PATH_LANES;
   hipLaunchKernelGGL(path_count_kernel<real>, dim3(blocks), dim3(ORC_PATH_LANES), 0, stream, v);
   return hipGetLastError();
}
hipError_t orc_launch_path_count(const DevPathClearance<double> & v, hipStream_t stream) { return launch_path_count_t<double>(v, stream); }
hipError_t orc_launch_path_count(const DevPathClearance<float> & v, hipStream_t stream) { return launch_path_count_t<float>(v, stream); }

template <typename real>
static hipError_t launch_path_round_t(const DevPathClearance<real> & v, size_t lds, hipStream_t stream, int tree)
{
   static std::atomic<unsigned long long> attr_set{0ull};
   if (!path_args_ok(v) || !v.offs || v.n_entries < 0 || v.n_entries > ORC_PATH_WORKSPACE) return hipErrorInvalidValue;
   if (v.chunk < 4 || v.chunk > 64 || (v.chunk & 3) || lds > ORC_VERDICT_LDS_LIMIT) return hipErrorInvalidValue;
   int dev = 0;
   if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
   if (!((attr_set.load() >> dev) & 1ull))
   {
      hipError_t e = hipFuncSetAttribute((const void *) path_walk_kernel<real, true>, hipFuncAttributeMaxDynamicSharedMemorySize, ORC_VERDICT_LDS_LIMIT);
      if (e == hipSuccess) e = hipFuncSetAttribute((const void *) path_walk_kernel<real, false>, hipFuncAttributeMaxDynamicSharedMemorySize, ORC_VERDICT_LDS_LIMIT);
      if (e != hipSuccess) return e;
      attr_set.fetch_or(1ull << dev);
   }
   if (v.n_entries > 0)
   {
      hipLaunchKernelGGL(path_fill_kernel<real>, dim3((v.n_q + ORC_PATH_LANES - 1) / ORC_PATH_LANES), dim3(ORC_PATH_LANES), 0, stream, v);
      const int blocks = (v.n_entries + v.chunk - 1) / v.chunk;
      if (tree) hipLaunchKernelGGL((path_walk_kernel<real, true>), dim3(blocks), dim3(ORC_BLOCK), lds, stream, v);
      else hipLaunchKernelGGL((path_walk_kernel<real, false>), dim3(blocks), dim3(ORC_BLOCK), lds, stream, v);
   }
   const int per_block = ORC_BLOCK / 64;
   hipLaunchKernelGGL(path_reduce_kernel<real>, dim3((v.n_q + per_block - 1) / per_block), dim3(ORC_BLOCK), 0, stream, v);
   return hipGetLastError();
}
hipError_t orc_launch_path_round(const DevPathClearance<double> & v, size_t lds, hipStream_t stream, int tree) { return launch_path_round_t<double>(v, lds, stream, tree); }
hipError_t orc_launch_path_round(const DevPathClearance<float> & v, size_t lds, hipStream_t stream, int tree) { return launch_path_round_t<float>(v, lds, stream, tree); }

// dynamic LDS of path_walk_kernel: the entries' header, then what the walk holds
size_t orc_path_walk_lds_bytes(int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk)
{
   return path_walk_header_bytes(chunk) + verdict_walk_lds_bytes(n, Sa, Sa_real, nj, real_size, chunk);
}
