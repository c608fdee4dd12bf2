// multistart_kernels.hip -- multi-start batches: perturbed seed trajectories, the best run per problem, the rows of the
// winners, the losing runs respawned from the winners, all on the device (orc_batch_perturb, orc_batch_select_best,
// orc_batch_gettraj_runs, orc_batch_respawn), and the best run per problem among those that clear a margin
// (orc_batch_select_clear).
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
#include "launch.h"
#include "mt_wave.h"
#include "run_candidate.h"
#include "cost_key.h"

namespace {

#include "wave.h"           // wave_prefix_excl, wave_suffix_excl

// One wavefront (= one workgroup) per run.  xi is staged in LDS ([m][n] doubles in front of the generator's state);
// lane l owns the rows [l R, (l+1) R), R = ceil(m / 64), of every column: its partial sums go through one prefix and one suffix wave scan per generator, then it walks its rows.
// A run's result depends on its seed, the scale and the batch's parameters only: nothing here reads the run's index
// but the addresses.
// source_of_run: NULL (orc_batch_perturb: every run), or the plan of a respawn: a run that is its own source is a survivor
// and its workgroup leaves it alone.
template <typename real>
__global__ __launch_bounds__(64)
void perturb_kernel(real * traj, int n_points, int n, int m, const unsigned int * seeds, int D,
   const double * genU, const double * genV, double scale, const double * lim_lo, const double * lim_hi, const int * source_of_run)
{
   extern __shared__ double smem[];
   const int run = blockIdx.x, lane = threadIdx.x & 63;
   if (source_of_run && source_of_run[run] == run) return;      // (the whole workgroup: nobody waits at a barrier)
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

// ---- the best run per group (orc_batch_select_best[_by], orc_batch_select_clear) ----------------------------------------
// Is run r eligible under the rule (launch.h: SelectRule), and with what key?  A candidate (run_candidate.h); with verdict_key
// (verdict_kernels.hip) one without a contact; with clear (what clearance_kernel left of the candidates) one that was walked
// (not too long) and whose smaller minimum is at least `margin`.  The key is that of the column's cost (0 total, 1 obs,
// 2 smooth) or, column 3, of minus the clearance: the largest first.  Eligibility does not depend on the column.
__device__ __forceinline__ bool select_key(const SelectRule & s, int r, unsigned long long & key)
{
   if (!orc_run_candidate(s.status[r], s.costs[(size_t) r*3]) || (s.verdict_key && s.verdict_key[r] != ORC_VERDICT_NONE)) return false;
   double c = 0.0;
   if (s.clear)
   {
      c = fmin(s.clear[(size_t) r*2], s.clear[(size_t) r*2 + 1]);
      if (!(s.n_samples[r] >= 0 && c >= s.margin)) return false;
   }
   key = cost_key(s.column < 3 ? s.costs[(size_t) r*3 + s.column] : -c);
   return true;
}
// pass 1: the lowest key of every group's eligible runs and their number
__global__ void select_cost_kernel(SelectRule rule, const int * group, int n_runs, unsigned long long * key, int * count)
{
   const int r = blockIdx.x * blockDim.x + threadIdx.x;
   unsigned long long k;
   if (r >= n_runs || !select_key(rule, r, k)) return;
   atomicMin(&key[group[r]], k);
   atomicAdd(&count[group[r]], 1);
}
// pass 2: the lowest index among the runs that have it
__global__ void select_run_kernel(SelectRule rule, const int * group, int n_runs, const unsigned long long * key, int * best)
{
   const int r = blockIdx.x * blockDim.x + threadIdx.x;
   unsigned long long k;
   if (r >= n_runs || !select_key(rule, r, k)) return;
   if (k == key[group[r]]) atomicMin(&best[group[r]], r);
}
// pass 3 (a rule with clear): the winners' clearance
__global__ void select_clear_margin_kernel(const double * clear, const int * count, const int * best, int n_groups, double * best_clear)
{
   const int g = blockIdx.x * blockDim.x + threadIdx.x;
   if (g >= n_groups) return;
   const int r = best[g];
   best_clear[g] = count[g] > 0 ? fmin(clear[(size_t) r*2], clear[(size_t) r*2 + 1]) : __longlong_as_double(0x7ff8000000000000LL);
}

// ---- rows of the trajectory array, as doubles -----------------------------------------------------------------------
template <typename real>
__global__ void gather_rows_kernel(const real * traj, const int * rows, int n_sel, size_t row_len, double * out)
{
   const size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
   if (e >= row_len) return;
   for (int q=blockIdx.y; q<n_sel; q+=gridDim.y) out[(size_t) q * row_len + e] = (double) traj[(size_t) rows[q] * row_len + e];
}

// ---- respawn: every group's survivors, and the losing runs made copies of them (orc_batch_respawn) -------------------
// One workgroup of four wavefronts per group; the group's runs are members[group_offs[g] .. group_offs[g+1]), ascending.
// A member's order key is (class, cost_key of its cost column, its position in the list): class 0 a candidate, 1 a candidate
// that collides (mode 2: behind every free one), 2 not a candidate (behind everything; never ranked).  The keys are staged
// in LDS; a wavefront takes one member at a time and its lanes 64 others, and the member's rank is the number of set bits
// of the ballots "this one comes before it": a count, no atomics, the same whatever the schedule.  Then the first
// wavefront walks the list once, 64 positions a step, numbers the runs that do not survive by a prefix count of the
// survivors' ballot and deals them the survivors in rank order, round and round.
// LDS per member: the key (8 bytes), the survivor of its rank (4), its class (1), whether it survives (1).
__global__ __launch_bounds__(256)
void respawn_rank_kernel(const double * costs, const int * status, const unsigned long long * verdict_key, int mode, int column, int keep,
   const int * group_offs, const int * members, int * source_of_run, int * n_survivors)
{
   extern __shared__ double smem[];
   const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int G = group_offs[g+1] - group_offs[g];
   const int * mem = members + group_offs[g];
   if (G <= 0) { if (tid == 0) n_survivors[g] = 0; return; }
   unsigned long long * key = (unsigned long long *) smem;
   int * surv = (int *)(key + G);
   unsigned char * cls = (unsigned char *)(surv + G);
   unsigned char * stays = cls + G;
   for (int i=tid; i<G; i+=256)
   {
      const int r = mem[i];
      const bool hit = mode != 0 && verdict_key[r] != ORC_VERDICT_NONE;
      const bool cand = orc_run_candidate(status[r], costs[(size_t) r*3]) && !(mode == 1 && hit);
      cls[i] = cand ? ((mode == 2 && hit) ? 1 : 0) : 2;
      key[i] = cost_key(costs[(size_t) r*3 + column]);
   }
   __syncthreads();
   int n_cand = 0;      // (every wavefront counts for itself)
   for (int j0=0; j0<G; j0+=64)
   {
      const int j = j0 + lane;
      n_cand += __popcll(__builtin_amdgcn_ballot_w64(j < G && cls[j] < 2));
   }
   const int n_surv = keep < n_cand ? keep : n_cand;
   for (int i=wave; i<G; i+=4)
   {
      const int ci = cls[i];
      const unsigned long long ki = key[i];
      if (ci == 2) { if (lane == 0) stays[i] = 0; continue; }      // (the same for the whole wavefront)
      int rank = 0;
      for (int j0=0; j0<G; j0+=64)
      {
         const int j = j0 + lane;
         bool before = false;
         if (j < G)
         {
            const int cj = cls[j];
            const unsigned long long kj = key[j];
            before = cj < ci || (cj == ci && (kj < ki || (kj == ki && j < i)));
         }
         rank += __popcll(__builtin_amdgcn_ballot_w64(before));
      }
      if (lane == 0)
      {
         stays[i] = rank < n_surv;
         if (rank < n_surv) surv[rank] = mem[i];
      }
   }
   __syncthreads();
   if (wave != 0) return;
   int below = 0;      // survivors in front of this step's positions
   for (int j0=0; j0<G; j0+=64)
   {
      const int j = j0 + lane;
      const bool s = j < G && stays[j];
      const unsigned long long mask = __builtin_amdgcn_ballot_w64(s);
      if (j < G)
      {
         const int loser = j - (below + __popcll(mask & ((1ull << lane) - 1ull)));      // its number among the group's other runs
         const int r = mem[j];
         source_of_run[r] = s ? r : (n_surv ? surv[loser % n_surv] : -1);
      }
      below += __popcll(mask);
   }
   if (lane == 0) n_survivors[g] = n_surv;
}

// One workgroup per run; a survivor (its own source) is not touched, so a source is never written: safe in place.  The
// line is seed_traj_kernel's statement on the run's own stored ends.
template <typename real>
__global__ __launch_bounds__(256)
void respawn_copy_kernel(real * traj, real * AG, int * leapfrog_first, const int * source_of_run, int n_points, int n, int m)
{
   const int r = blockIdx.x, s = source_of_run[r];
   if (s == r) return;
   const size_t mn = (size_t) m * n;
   real * T = traj + ((size_t) r * n_points + 1) * n;      // (the moving rows: both ends are fixed)
   real * A = AG + (size_t) r * mn;
   if (s >= 0)
   {
      const real * Ts = traj + ((size_t) s * n_points + 1) * n;
      const real * As = AG + (size_t) s * mn;
      for (size_t e=threadIdx.x; e<mn; e+=blockDim.x) { T[e] = Ts[e]; A[e] = As[e]; }
      if (threadIdx.x == 0) leapfrog_first[r] = leapfrog_first[s];
      return;
   }
   const real * first = traj + (size_t) r * n_points * n, * last = first + (size_t)(n_points - 1) * n;
   for (size_t e=threadIdx.x; e<mn; e+=blockDim.x)
   {
      const int i = (int)(e / n) + 1, c = (int)(e % n);
      const double sv = (double) first[c], gv = (double) last[c];
      T[e] = (real)(sv + (gv - sv) * i / (n_points - 1));
      A[e] = (real) 0;
   }
   if (threadIdx.x == 0) leapfrog_first[r] = 1;
}

template <typename real>
hipError_t launch_perturb(real * traj, int n_runs, int n_points, int n, int m, const unsigned int * seeds, int D,
   const double * genU, const double * genV, double scale, const double * lim_lo, const double * lim_hi, size_t lds,
   const int * source_of_run, hipStream_t stream)
{
   if (lds > 64 * 1024)
   {
      const hipError_t e = hipFuncSetAttribute((const void *) perturb_kernel<real>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
      if (e != hipSuccess) return e;
   }
   hipLaunchKernelGGL(perturb_kernel<real>, dim3(n_runs), dim3(64), lds, stream, traj, n_points, n, m, seeds, D, genU, genV, scale,
      lim_lo, lim_hi, source_of_run);
   return hipGetLastError();
}

} // namespace

// LDS of one run's workgroup: xi, then the generator's state (the caller refuses m n > ORC_PERTURB_MAX_MN, multistart.h)
size_t orc_perturb_lds_bytes(int m, int n)
{
   return (size_t) m * n * sizeof(double) + 624 * sizeof(uint32_t);
}
// source_of_run: NULL, or the plan of a respawn (its survivors are skipped)
hipError_t orc_launch_perturb(void * traj, int precision, int n_runs, int n_points, int n, int m, const unsigned int * seeds, int D,
   const double * genU, const double * genV, double scale, const double * lim_lo, const double * lim_hi, size_t lds,
   const int * source_of_run, hipStream_t stream)
{
   if (precision == 64) return launch_perturb<double>((double *) traj, n_runs, n_points, n, m, seeds, D, genU, genV, scale, lim_lo, lim_hi, lds, source_of_run, stream);
   return launch_perturb<float>((float *) traj, n_runs, n_points, n, m, seeds, D, genU, genV, scale, lim_lo, lim_hi, lds, source_of_run, stream);
}
// LDS of a group's workgroup: 14 bytes per member of the largest group (the caller refuses groups over
// ORC_RESPAWN_MAX_GROUP, multistart.h: 56 KB, inside what a kernel has without asking)
size_t orc_respawn_rank_lds_bytes(int max_group)
{
   return ((size_t) max_group * 14 + 15) & ~(size_t) 15;
}
// verdict_key may be NULL with mode 0; source_of_run [n_runs of the shard] and n_survivors [n_groups] are written in full
// when every run is a member of one group
hipError_t orc_launch_respawn_rank(const double * costs, const int * status, const unsigned long long * verdict_key, int mode, int column, int keep,
   int n_groups, const int * group_offs, const int * members, int max_group, int * source_of_run, int * n_survivors, hipStream_t stream)
{
   if (n_groups < 1) return hipSuccess;
   hipLaunchKernelGGL(respawn_rank_kernel, dim3(n_groups), dim3(256), orc_respawn_rank_lds_bytes(max_group), stream, costs, status, verdict_key,
      mode, column, keep, group_offs, members, source_of_run, n_survivors);
   return hipGetLastError();
}
hipError_t orc_launch_respawn_copy(void * traj, void * AG, int precision, int * leapfrog_first, const int * source_of_run,
   int n_runs, int n_points, int n, int m, hipStream_t stream)
{
   if (precision == 64) hipLaunchKernelGGL(respawn_copy_kernel<double>, dim3(n_runs), dim3(256), 0, stream, (double *) traj, (double *) AG, leapfrog_first, source_of_run, n_points, n, m);
   else hipLaunchKernelGGL(respawn_copy_kernel<float>, dim3(n_runs), dim3(256), 0, stream, (float *) traj, (float *) AG, leapfrog_first, source_of_run, n_points, n, m);
   return hipGetLastError();
}
// key [n_groups] (all bits set), count [n_groups] (0) and best [n_groups] (above every run index) are the caller's to initialise;
// best_clear [n_groups] is written in full when the rule has clear (the winner's fmin, NaN without a winner), else not at all
hipError_t orc_launch_select(const SelectRule & rule, const int * group, int n_runs, int n_groups, unsigned long long * key, int * count, int * best,
   double * best_clear, hipStream_t stream)
{
   const dim3 grid((n_runs + 255) / 256), block(256);
   hipLaunchKernelGGL(select_cost_kernel, grid, block, 0, stream, rule, group, n_runs, key, count);
   hipLaunchKernelGGL(select_run_kernel, grid, block, 0, stream, rule, group, n_runs, key, best);
   if (rule.clear) hipLaunchKernelGGL(select_clear_margin_kernel, dim3((n_groups + 255) / 256), block, 0, stream, rule.clear, count, best, n_groups, best_clear);
   return hipGetLastError();
}
hipError_t orc_launch_gather_rows(const void * traj, int precision, const int * rows, int n_sel, size_t row_len, double * out, hipStream_t stream)
{
   const dim3 grid((unsigned)((row_len + 255) / 256), n_sel < 65535 ? n_sel : 65535), block(256);
   if (precision == 64) hipLaunchKernelGGL(gather_rows_kernel<double>, grid, block, 0, stream, (const double *) traj, rows, n_sel, row_len, out);
   else hipLaunchKernelGGL(gather_rows_kernel<float>, grid, block, 0, stream, (const float *) traj, rows, n_sel, row_len, out);
   return hipGetLastError();
}
