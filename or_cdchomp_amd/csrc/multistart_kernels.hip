// multistart_kernels.hip -- multi-start batches: perturbed seed trajectories, the best run per problem, the rows of the
// winners, all on the device (orc_batch_perturb, orc_batch_select_best, orc_batch_gettraj_runs).
//
// The reference has no multi-start; K runs of one planning problem start from one straight line (seed_traj_kernel) and are
// K identical runs unless something diversifies them.  perturb_kernel adds to the moving waypoints of every run a smooth
// random displacement  delta = scale * A^-1 xi,  xi unit Gaussians of a GSL stream of the call's own (mt_wave.h) and A the
// batch's smoothness metric: the covariance CHOMP's own prior gives a trajectory, zero at the fixed ends.  A^-1 is applied
// through the generators of its semiseparable form (host_math.h: Ainv[i][j] = sum_k U[k][i] V[k][j] for i <= j, rank D; for
// derivative 1 the generators are the closed form (i+1), (m-j) / ((m+1) a) of a tridiag(-1, 2, -1)):
//    x_i = sum_k U[k][i] S_k(i) + V[k][i] P_k(i),   S_k(i) = sum_{j >= i} V[k][j] g_j,   P_k(i) = sum_{j < i} U[k][j] g_j.
// Everything in double, for fp32 batches too: the call runs once per batch, not once per iteration.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "dev_types.h"
#include "mt_wave.h"

namespace {

__device__ __forceinline__ double wave_prefix_excl(double v)      // sum over the lanes below
{
   const int lane = threadIdx.x & 63;
   for (int d=1; d<64; d<<=1) { const double t = __shfl_up(v, d); if (lane >= d) v += t; }
   const double e = __shfl_up(v, 1);
   return lane ? e : 0.0;
}
__device__ __forceinline__ double wave_suffix_excl(double v)      // sum over the lanes above
{
   const int lane = threadIdx.x & 63;
   for (int d=1; d<64; d<<=1) { const double t = __shfl_down(v, d); if (lane + d < 64) v += t; }
   const double e = __shfl_down(v, 1);
   return lane < 63 ? e : 0.0;
}

// One wavefront (= one workgroup) per run.  xi is staged in LDS ([m][n] doubles in front of the generator's state);
// lane l owns the rows [l R, (l+1) R), R = ceil(m / 64), of every column: its partial sums go through one prefix and one suffix wave scan per generator, then it walks its rows.
// A run's result depends on its seed, the scale and the batch's parameters only: nothing here reads the run's index
// but the addresses.
template <typename real>
__global__ __launch_bounds__(64)
void perturb_kernel(real * traj, int n_points, int n, int m, const unsigned int * seeds, int D,
   const double * genU, const double * genV, double scale, const double * lim_lo, const double * lim_hi)
{
   extern __shared__ double smem[];
   const int run = blockIdx.x, lane = threadIdx.x & 63;
   const size_t mn = (size_t) m * n;
   double * x = smem;
   MtWave g; g.mt = (uint32_t *)(smem + mn);
   g.seed(seeds[run]);
   g.gaussians(x, mn, 1.0);
   __syncthreads();
   const int R = (m + 63) / 64;
   const int i0 = (lane * R < m) ? lane * R : m, i1 = (i0 + R < m) ? i0 + R : m;
   for (int c=0; c<n; c++)
   {
      double p[ORC_SS_MAX_RANK], s[ORC_SS_MAX_RANK];
      for (int k=0; k<ORC_SS_MAX_RANK; k++)
      {
         double lp = 0.0, ls = 0.0;
         if (k < D)
            for (int i=i1-1; i>=i0; i--)
            {
               const double gi = x[(size_t) i*n + c];
               lp += genU[(size_t) k*m + i] * gi;
               ls += genV[(size_t) k*m + i] * gi;
            }
         p[k] = wave_prefix_excl(lp);
         s[k] = wave_suffix_excl(ls) + ls;      // S_k at this lane's first row
      }
      for (int i=i0; i<i1; i++)
      {
         const double gi = x[(size_t) i*n + c];
         double v = 0.0;
         for (int k=0; k<ORC_SS_MAX_RANK; k++)
            if (k < D)
            {
               const double u = genU[(size_t) k*m + i], w = genV[(size_t) k*m + i];
               v += u * s[k] + w * p[k];
               p[k] += u * gi;
               s[k] -= w * gi;
            }
         x[(size_t) i*n + c] = v;
      }
   }
   __syncthreads();
   real * T = traj + ((size_t) run * n_points + 1) * n;      // (the moving rows: both ends are fixed)
   for (size_t e=lane; e<mn; e+=64)
   {
      const int c = (int)(e % n);
      double v = (double) T[e] + scale * x[e];
      v = fmin(fmax(v, lim_lo[c]), lim_hi[c]);
      T[e] = (real) v;
   }
}

// ---- the best run per group -------------------------------------------------------------------------------------
// doubles as unsigned keys of the same order (-0 made +0 first: equal costs must tie)
__device__ __forceinline__ unsigned long long cost_key(double c)
{
   const unsigned long long b = (unsigned long long) __double_as_longlong(c + 0.0);
   return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// verdict_key: the runs' keys of the collision verdict (verdict_kernels.hip), or NULL when the verdict is not asked for
__device__ __forceinline__ bool run_eligible(const double * costs, const int * status, const unsigned long long * verdict_key, int r)
{
   const int st = status[r];
   const double c = costs[(size_t) r*3];
   return (st == 0 || st == 1) && isfinite(c) && !(verdict_key && verdict_key[r] != ORC_VERDICT_NONE);
}

// column: which of a run's costs (0 total, 1 obs, 2 smooth) is the key that is minimised; eligibility does not depend on it
// pass 1: the lowest cost key of every group's eligible runs and their number
__global__ void select_cost_kernel(const double * costs, const int * status, const unsigned long long * verdict_key, const int * group, int n_runs, int column,
   unsigned long long * key, int * count)
{
   const int r = blockIdx.x * blockDim.x + threadIdx.x;
   if (r >= n_runs || !run_eligible(costs, status, verdict_key, r)) return;
   atomicMin(&key[group[r]], cost_key(costs[(size_t) r*3 + column]));
   atomicAdd(&count[group[r]], 1);
}
// pass 2: the lowest index among the runs that have it
__global__ void select_run_kernel(const double * costs, const int * status, const unsigned long long * verdict_key, const int * group, int n_runs, int column,
   const unsigned long long * key, int * best)
{
   const int r = blockIdx.x * blockDim.x + threadIdx.x;
   if (r >= n_runs || !run_eligible(costs, status, verdict_key, r)) return;
   if (cost_key(costs[(size_t) r*3 + column]) == key[group[r]]) atomicMin(&best[group[r]], r);
}

// ---- rows of the trajectory array, as doubles -----------------------------------------------------------------------
template <typename real>
__global__ void gather_rows_kernel(const real * traj, const int * rows, int n_sel, size_t row_len, double * out)
{
   const size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
   if (e >= row_len) return;
   for (int q=blockIdx.y; q<n_sel; q+=gridDim.y) out[(size_t) q * row_len + e] = (double) traj[(size_t) rows[q] * row_len + e];
}

template <typename real>
hipError_t launch_perturb(real * traj, int n_runs, int n_points, int n, int m, const unsigned int * seeds, int D,
   const double * genU, const double * genV, double scale, const double * lim_lo, const double * lim_hi, size_t lds,
   hipStream_t stream)
{
   if (lds > 64 * 1024)
   {
      const hipError_t e = hipFuncSetAttribute((const void *) perturb_kernel<real>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
      if (e != hipSuccess) return e;
   }
   hipLaunchKernelGGL(perturb_kernel<real>, dim3(n_runs), dim3(64), lds, stream, traj, n_points, n, m, seeds, D, genU, genV, scale,
      lim_lo, lim_hi);
   return hipGetLastError();
}

} // namespace

// LDS of one run's workgroup: xi, then the generator's state (the caller refuses m n > BatchShard::ORC_PERTURB_MAX_MN, module.h)
size_t orc_perturb_lds_bytes(int m, int n)
{
   return (size_t) m * n * sizeof(double) + 624 * sizeof(uint32_t);
}
hipError_t orc_launch_perturb_f64(double * traj, int n_runs, int n_points, int n, int m, const unsigned int * seeds, int D,
   const double * genU, const double * genV, double scale, const double * lim_lo, const double * lim_hi, size_t lds, hipStream_t stream)
{
   return launch_perturb<double>(traj, n_runs, n_points, n, m, seeds, D, genU, genV, scale, lim_lo, lim_hi, lds, stream);
}
hipError_t orc_launch_perturb_f32(float * traj, int n_runs, int n_points, int n, int m, const unsigned int * seeds, int D,
   const double * genU, const double * genV, double scale, const double * lim_lo, const double * lim_hi, size_t lds, hipStream_t stream)
{
   return launch_perturb<float>(traj, n_runs, n_points, n, m, seeds, D, genU, genV, scale, lim_lo, lim_hi, lds, stream);
}
// key [n_groups] (all bits set), count [n_groups] (0) and best [n_groups] (INT_MAX) are the caller's to initialise
hipError_t orc_launch_select_best(const double * costs, const int * status, const unsigned long long * verdict_key, const int * group, int n_runs, int column,
   unsigned long long * key, int * count, int * best, hipStream_t stream)
{
   const dim3 grid((n_runs + 255) / 256), block(256);
   hipLaunchKernelGGL(select_cost_kernel, grid, block, 0, stream, costs, status, verdict_key, group, n_runs, column, key, count);
   hipLaunchKernelGGL(select_run_kernel, grid, block, 0, stream, costs, status, verdict_key, group, n_runs, column, key, best);
   return hipGetLastError();
}
hipError_t orc_launch_gather_rows(const void * traj, int precision, const int * rows, int n_sel, size_t row_len, double * out, hipStream_t stream)
{
   const dim3 grid((unsigned)((row_len + 255) / 256), n_sel < 65535 ? n_sel : 65535), block(256);
   if (precision == 64) hipLaunchKernelGGL(gather_rows_kernel<double>, grid, block, 0, stream, (const double *) traj, rows, n_sel, row_len, out);
   else hipLaunchKernelGGL(gather_rows_kernel<float>, grid, block, 0, stream, (const float *) traj, rows, n_sel, row_len, out);
   return hipGetLastError();
}
