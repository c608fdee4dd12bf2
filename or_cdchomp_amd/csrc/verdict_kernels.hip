// verdict_kernels.hip -- the collision verdict of a batch with the samples planned on the device
// (orc_batch_collision_verdict_device, orc_batch_select_best with require_collision_free).
//
// collision_verdict_kernel (chomp_kernel.hip) walks samples the host planned: Module::batch_collision_verdict reads every
// trajectory back, retimes it (retime_linear), lays a sample every 0.04 rad of C-space distance (plan_collision_samples)
// and uploads the list.  Here the run's workgroup does that itself: a fifth wavefront, the planner, retimes the run and
// steps the sample times a chunk ahead of the four wavefronts that walk them, so no trajectory leaves the device and no
// sample list exists.  The walk -- rows, FK (fk.h), field tests, pair tests, the key of the first contact -- is that
// kernel's, statement for statement: the two verdicts agree bit for bit.
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

#define ORC_VD_WORKERS ORC_BLOCK            // threads that walk the samples, as in collision_verdict_kernel
#define ORC_VD_BLOCK   (ORC_BLOCK + 64)     // ... and the planner's wavefront
#define ORC_VD_HEADER  32                   // bytes: the first contact's key, the sample counts of the two chunk buffers, the too-long flag
#define ORC_VD_MAX_SAMPLES (1 << 30)        // the sample index sits above bit 32 of the key, under ORC_VERDICT_NONE

// ---- the plan: the host's arithmetic (module.cpp retime_linear, plan_collision_samples) ----------------------------------
#pragma clang fp contract(off)
namespace {

// segment i (rows i-1 and i): its time at the largest velocity the limits allow, and its length
template <typename real>
__device__ __forceinline__ void plan_segment(const real * traj, int i, int n, int col0, const double * vmax, double & dtm, double & len)
{
   double dt = 0.0, d2 = 0.0;
   for (int j=col0; j<n; j++)
   {
      const double lo = (double) traj[(size_t)(i-1)*n + j], hi = (double) traj[(size_t) i*n + j];
      const double v = vmax[j-col0] > 0.0 ? vmax[j-col0] : 1.0;
      const double c = ::fabs(hi - lo) / v;
      dt = dt < c ? c : dt;                  // std::max(dt, c): a NaN candidate is ignored
      const double d = lo - hi;
      d2 += d*d;
   }
   dtm = dt; len = ::sqrt(d2);
}

// in: tstart[i] = length of segment i; out: tstart[i] = time at which segment i ends (tstart[0] = 0, tstart[np-1] = duration)
__device__ __forceinline__ void plan_totals(int np, const double * dtm, double * tstart, double & total_dist, double & duration)
{
   double td = 0.0, du = 0.0;
   tstart[0] = 0.0;
   for (int i=1; i<np; i++)
   {
      td += tstart[i];
      du += dtm[i];
      tstart[i] = du;
   }
   total_dist = td; duration = du;
}

__device__ __forceinline__ double plan_step_time(double total_dist, double duration)
{
   return total_dist > 0.0 ? duration * 0.04 / total_dist : duration + 1.0;
}

// the next samples' times, `cap` at most; returns their number
__device__ __forceinline__ int plan_times(double & time, double step_time, double duration, double * out, int cap)
{
   int k = 0;
   while (k < cap && time < duration) { out[k++] = time; time += step_time; }
   return k;
}

// the samples nobody walks
__device__ __forceinline__ int plan_count_rest(double time, double step_time, double duration, int have)
{
   while (have < ORC_VD_MAX_SAMPLES && time < duration) { time += step_time; have++; }
   return have;
}

// segment of a sample and its position on it
__device__ __forceinline__ int plan_locate(double time, int np, const double * dtm, const double * tstart, double & u)
{
   int lo = 0, hi = np - 2;                  // the largest s in 1 .. np-2 with tstart[s] < time (tstart does not decrease), or 0
   while (lo < hi)
   {
      const int mid = (lo + hi + 1) >> 1;
      if (tstart[mid] < time) lo = mid; else hi = mid - 1;
   }
   const double d = dtm[lo+1];
   u = d > 0.0 ? (time - tstart[lo]) / d : 0.0;
   return lo;
}

} // namespace

// ---- the walk: the arithmetic of collision_verdict_kernel ------------------------------------------------------------------
#pragma clang fp contract(fast)
namespace {

#include "sdf_lookup.h"
#include "fk.h"

template <typename real, bool TREE>
__global__ __launch_bounds__(ORC_VD_BLOCK)
void collision_verdict_planned_kernel(DevVerdictPlan<real> v)
{
   extern __shared__ __align__(16) unsigned char smem_raw[];
   const DevModel<real> & gmod = *v.model;
   const int run = blockIdx.x, tid = threadIdx.x;
   const bool planner = tid >= ORC_VD_WORKERS;
   const int n = v.n, np = v.n_points, nj = gmod.nj, Sa = gmod.Sa;
   const int pstr = (Sa*3) | 1, astr = (nj*6) | 1, chunk = v.chunk;
   // the run's scene: its slice of the descriptors and its field count
   const int scene = v.scene_of_run ? v.scene_of_run[run] : 0;
   const int n_fields = v.scene_nsdf ? v.scene_nsdf[scene] : v.n_sdfs;
   const DevSdf<real> * sdfs = v.sdfs + (size_t) scene * v.n_sdfs;
   unsigned long long * key_s = (unsigned long long *) smem_raw;     // [1]: the first contact's key (sample << 32 | pair bit << 31 | sphere << 16 | field or partner)
   int * cnt_s = (int *)(smem_raw + 8);                              // [2]: samples in either chunk buffer
   int * long_s = (int *)(smem_raw + 16);                            // [1]: the run has too many samples
   double * times_s = (double *)(smem_raw + ORC_VD_HEADER);          // [2][chunk]
   double * u_s = times_s + 2*chunk;                                 // [2][chunk]
   double * dtm_s = u_s + 2*chunk;                                   // [np]
   double * tstart_s = dtm_s + np;                                   // [np]
   int * seg_s = (int *)(tstart_s + np);                             // [2][chunk]
   real * lds = (real *)(seg_s + 2*chunk);
   real * rows_s = lds;                                              // [chunk][n]
   real * pos_s = rows_s + ((chunk*n + 3) & ~3);                     // [chunk][pstr]
   real * ax_s = pos_s + ((chunk*pstr + 3) & ~3);                    // [chunk][astr]
   real * base_s = ax_s + ((chunk*astr + 3) & ~3);                   // [12]
   real * srad_s = base_s + 12;                                      // [Sa]
   int * slot_s = (int *)(srad_s + ((Sa + 3) & ~3));                 // [Sa_real]
   int * xml_s = slot_s + ((gmod.Sa_real + 3) & ~3);                 // [Sa]
   int * jctl_s = xml_s + ((Sa + 3) & ~3);                           // [nj][2]
   for (int e=tid; e<12; e+=ORC_VD_BLOCK) base_s[e] = (e < 9) ? gmod.base_R[e] : gmod.base_t[e-9];
   for (int e=tid; e<Sa; e+=ORC_VD_BLOCK) { srad_s[e] = gmod.sph_radius[e]; xml_s[e] = v.slot_xml[e]; }
   for (int e=tid; e<gmod.Sa_real; e+=ORC_VD_BLOCK) slot_s[e] = gmod.slot_of[e];
   for (int e=tid; e<nj; e+=ORC_VD_BLOCK) { jctl_s[2*e] = gmod.joints[e].packed; jctl_s[2*e+1] = 0; }
   if (tid == 0) { key_s[0] = ORC_VERDICT_NONE; dtm_s[0] = 0.0; }
   ModelView<real> mod;
   mod.nj = nj; mod.n = n; mod.floating = gmod.floating; mod.tree = gmod.tree; mod.Sa = Sa; mod.S = gmod.S; mod.GS = gmod.GS;
   mod.base_sph_begin = gmod.base_sph_begin; mod.base_sph_end = gmod.base_sph_end; mod.jt_scan = 0;
   mod.Sa_real = gmod.Sa_real; mod.placed = gmod.placed; mod.live_mask = gmod.live_mask; mod.slot_of = slot_s;
   mod.base_R = base_s; mod.base_t = base_s + 9;
   mod.jctl = jctl_s; mod.sph_affects = nullptr; mod.n_static = 0; mod.empty_mask = 0u;
   mod.jpk = (const __attribute__((address_space(4))) int *) gmod.jpacked;
   mod.jpk2 = (const __attribute__((address_space(4))) int *) gmod.jpacked2;
   mod.sph_pos_c = (const __attribute__((address_space(4))) real (*)[3]) gmod.sph_pos;
   mod.joints_c = (const __attribute__((address_space(4))) DevJoint<real> *) gmod.joints;
   mod.slot_c = (const __attribute__((address_space(4))) int *) gmod.slot_of;
   mod.fkj = (const __attribute__((address_space(4))) DevFkJoint<real> *) gmod.fkj;

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
      if (tid == 0) { v.key_out[run] = ORC_VERDICT_NONE; v.time_out[run] = -1.0; v.n_samples_out[run] = 0; *v.too_long = 1; }
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
      // rows of the samples: a0 + (a1 - a0) u on their segments
      if (!planner)
         for (int e=tid; e<count*n; e+=ORC_VD_WORKERS)
         {
            const int s = e / n, c = e - s*n;
            const int sg = seg_s[buf + s];
            const real uu = (real) u_s[buf + s];
            const real a0 = traj[sg*n + c], a1 = traj[(sg+1)*n + c];
            rows_s[s*n + c] = a0 + (a1 - a0) * uu;
         }
      __syncthreads();
      if (planner && tid - ORC_VD_WORKERS < cnt_s[(ci + 1) & 1])
      {
         const int k = nbuf + tid - ORC_VD_WORKERS;
         seg_s[k] = plan_locate(times_s[k], np, dtm_s, tstart_s, u_s[k]);
      }
      if (mod.floating && tid < count)
      {
         real * row = rows_s + tid*n;
         const real len = M<real>::sqrt_(row[3]*row[3] + row[4]*row[4] + row[5]*row[5] + row[6]*row[6]);
         const real inv = (real)1 / len;
         row[3] *= inv; row[4] *= inv; row[5] *= inv; row[6] *= inv;
      }
      __syncthreads();
      if (!planner)
      {
         // 20 samples per wavefront (fk.h: triads of lanes)
         const int lane16 = tid & 15, triad = (lane16 * 11) >> 5;
         const int s = (tid >> 6) * 20 + ((tid >> 4) & 3) * 5 + triad;
         const bool valid = (lane16 < 15) && (s < count);
         const int sr = valid ? s : 0;
         fk_waypoint_triad<real, TREE>(mod, rows_s + sr*n, 0, 0, nj, true, (lane16 < 15) ? lane16 - 3*triad : 0, valid, pos_s + sr*pstr, ax_s + sr*astr);
      }
      __syncthreads();
      if (!planner)
      {
         for (int item=tid; item<count*Sa; item+=ORC_VD_WORKERS)
         {
            const int s = item / Sa, slot = item - s*Sa;
            if (!((mod.live_mask >> slot) & 1ull)) continue;
            const real * p = pos_s + s*pstr + slot*3;
            const real radius = srad_s[slot];
            for (int i=0; i<n_fields; i++)
            {
               const DevSdf<real> & F = sdfs[i];
               real gp[3], gg[3], val;
#pragma unroll
               for (int k=0; k<3; k++)
                  gp[k] = F.Rgw[k*3+0]*p[0] + F.Rgw[k*3+1]*p[1] + F.Rgw[k*3+2]*p[2] + F.tgw[k];
               if (sdf_lookup(F, gp, val, gg)) continue;                 // outside this field
               if (val - radius < (real)0)
               {
                  const unsigned long long key = ((unsigned long long)(sbase + s) << 32) | ((unsigned long long) xml_s[slot] << 16) | (unsigned long long) i;
                  if (key < my_key) { my_key = key; my_depth = (double)(radius - val); }
                  atomicMin(&key_s[0], key);
               }
            }
         }
         // self collision: a pair of spheres on links that may collide overlaps
         for (int item=tid; item<count*v.n_pairs; item+=ORC_VD_WORKERS)
         {
            const int s = item / v.n_pairs, pi = item - s*v.n_pairs;
            const int ea = v.pairs[pi*4+0], eb = v.pairs[pi*4+1];
            const real * pa = (ea >= 0) ? pos_s + s*pstr + ea*3 : v.inact_pos + (-1 - ea)*3;
            const real * pb = (eb >= 0) ? pos_s + s*pstr + eb*3 : v.inact_pos + (-1 - eb)*3;
            const real dx = pa[0]-pb[0], dy = pa[1]-pb[1], dz = pa[2]-pb[2];
            const real dist = M<real>::sqrt_(dx*dx + dy*dy + dz*dz);
            const real rs = v.pair_rsum[pi];
            if (dist - rs < (real)0)
            {
               const unsigned long long key = ((unsigned long long)(sbase + s) << 32) | (1ull << 31) | ((unsigned long long) v.pairs[pi*4+2] << 16) | (unsigned long long) v.pairs[pi*4+3];
               if (key < my_key) { my_key = key; my_depth = (double)(rs - dist); }
               atomicMin(&key_s[0], key);
            }
         }
      }
      __syncthreads();
      const bool done = key_s[0] != ORC_VERDICT_NONE || count < chunk;      // a contact in this chunk: later samples cannot come first
      __syncthreads();
      if (done) break;
   }
   const unsigned long long first = key_s[0];
   if (tid == 0)
   {
      v.key_out[run] = first;
      // (the chunk of the first contact is the last one walked: its times are still in its buffer)
      v.time_out[run] = (first != ORC_VERDICT_NONE) ? times_s[(ci & 1) * chunk + ((int)(first >> 32) - ci * chunk)] : -1.0;
   }
   if (first != ORC_VERDICT_NONE && my_key == first) v.depth_out[run] = my_depth;
   // the samples behind a contact are counted all the same
   if (tid == ORC_VD_WORKERS)
   {
      planned = plan_count_rest(time, step_time, duration, planned);
      v.n_samples_out[run] = planned;
      if (planned >= ORC_VD_MAX_SAMPLES) *v.too_long = 1;
   }
}

} // namespace

template <typename real>
static hipError_t launch_verdict_planned_t(const DevVerdictPlan<real> & v, size_t lds, hipStream_t stream, int tree)
{
   static std::atomic<unsigned long long> attr_set{0ull};
   int dev = 0;
   if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
   if (!((attr_set.load() >> dev) & 1ull))
   {
      hipError_t e = hipFuncSetAttribute((const void *) collision_verdict_planned_kernel<real, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160*1024 - 256);
      if (e == hipSuccess) e = hipFuncSetAttribute((const void *) collision_verdict_planned_kernel<real, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160*1024 - 256);
      if (e != hipSuccess) return e;
      attr_set.fetch_or(1ull << dev);
   }
   if (lds > 160*1024 - 256 || v.n_points < 2 || v.chunk < 4 || v.chunk > 64 || (v.chunk & 3)) return hipErrorInvalidValue;
   if (tree) hipLaunchKernelGGL((collision_verdict_planned_kernel<real, true>), dim3(v.n_runs), dim3(ORC_VD_BLOCK), lds, stream, v);
   else hipLaunchKernelGGL((collision_verdict_planned_kernel<real, false>), dim3(v.n_runs), dim3(ORC_VD_BLOCK), lds, stream, v);
   return hipGetLastError();
}
hipError_t orc_launch_verdict_planned(const DevVerdictPlan<double> & v, size_t lds, hipStream_t stream, int tree) { return launch_verdict_planned_t<double>(v, lds, stream, tree); }
hipError_t orc_launch_verdict_planned(const DevVerdictPlan<float> & v, size_t lds, hipStream_t stream, int tree) { return launch_verdict_planned_t<float>(v, lds, stream, tree); }

// dynamic LDS of collision_verdict_planned_kernel (the carve-up at its top): the plan's arrays in front of what
// collision_verdict_kernel holds (orc_verdict_lds_bytes)
size_t orc_verdict_planned_lds_bytes(int n_points, int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk)
{
   const int pstr = (Sa*3) | 1, astr = (nj*6) | 1;
   auto r4 = [](int x) { return (x + 3) & ~3; };
   const size_t plan = (size_t) ORC_VD_HEADER + ((size_t) 4*chunk + (size_t) 2*n_points) * sizeof(double) + (size_t) 2*chunk * sizeof(int);
   const size_t reals = (size_t) r4(chunk*n) + r4(chunk*pstr) + r4(chunk*astr) + 12 + r4(Sa);
   const size_t ints = (size_t) r4(Sa_real) + r4(Sa);
   return plan + reals * real_size + ints * 4 + (size_t) nj * 8 + 64;
}
