// hmc_kernels.hip -- the momentum resampling plan of HMC runs, drawn on the device.
//
// The reference resamples a run's momentum at iterations spaced by exponential waiting times and
// fills it with Gaussian noise from the run's own GSL stream (gsl_rng_default = mt19937,
// gsl_ran_gaussian = polar Box-Muller, gsl_rng_uniform; src/orcdchomp_mod.cpp:2303-2304,
// 2755-2768).  The runs are independent; one wavefront per run produces its stream (published MT19937
// recurrence and tempering; GSL seeds 0 as 4357) and writes the noise blocks and their iterations for
// the iterate kernel.  State layout [625][n_runs] (word i of
// all runs contiguous; row 624 is the stream position), so that lockstep runs read coalesced.
// A batch's stream lives either here or in the host's GslRng objects (hmc.cpp: HmcPlanner picks at create).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "launch.h"
#include "mt_wave.h"

namespace {

__global__ void hmc_seed_kernel(uint32_t * state, int * next, const unsigned int * seeds, int n_runs)
{
   const int k = blockIdx.x * blockDim.x + threadIdx.x;
   if (k >= n_runs) return;
   uint32_t * st = state + k;
   unsigned long seed = seeds ? seeds[k] : 0;
   if (seed == 0) seed = 4357;
   uint32_t prev = (uint32_t)(seed & 0xffffffffUL);
   st[0] = prev;
   for (int i=1; i<624; i++)
   {
      prev = (uint32_t)(1812433253UL * (prev ^ (prev >> 30)) + (uint32_t) i);
      st[(size_t) i * n_runs] = prev;
   }
   st[(size_t) 624 * n_runs] = 624;
   next[k] = 0;
}

// the plan of the iterations [iter_begin, iter_end) of one iterate call: which of them resample run
// k's momentum (written relative to iter_begin; the comparison of the reference is `iter ==
// hmc_resample_iter` with iter restarting at 0 in every call), and the noise.
//
// One WAVEFRONT per run draws its stream (struct MtWave, mt_wave.h: the twist of the state 64 words at a time, 64 pairs of
// polar Box-Muller tried at once and the accepted ones compacted with a ballot).
// (One thread per run, the first version, took 48-115 ms per call for config 4's 4096 runs, as long as
// the 100 iterations it planned: profiles/r02_config4_kernel_stats.csv.)
#define ORC_HMC_WAVES 4

template <typename real>
__global__ __launch_bounds__(64 * ORC_HMC_WAVES)
void hmc_plan_kernel(uint32_t * state, int * next, int n_runs, int iter_begin, int iter_end, int cap, size_t mn,
   double lambda, real * noise, int * iters, int * overflow)
{
   __shared__ uint32_t lst[624 * ORC_HMC_WAVES];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   const int k = blockIdx.x * ORC_HMC_WAVES + wave;
   if (k >= n_runs) return;                       // wave-uniform
   MtWave g; g.mt = lst + 624 * wave; g.has_carry = 0; g.carry = 0;
   for (int i=lane; i<624; i+=64) g.mt[i] = state[(size_t) i * n_runs + k];
   g.mti = (int) state[(size_t) 624 * n_runs + k];
   __builtin_amdgcn_wave_barrier();
   int nx = next[k], r = 0;
   for (int q=lane; q<cap; q+=64) iters[(size_t) k * cap + q] = -1;
   while (nx >= iter_begin && nx < iter_end)
   {
      if (r >= cap) { if (lane == 0) atomicOr(overflow, 1); break; }
      const double alpha = 100.0 * exp(0.02 * nx);                 // src/orcdchomp_mod.cpp:2759-2762
      const double sigma = 1.0 / sqrt(alpha);
      real * out = noise + ((size_t) k * cap + r) * mn;
      g.gaussians(out, mn, sigma);
      if (lane == 0) iters[(size_t) k * cap + r] = nx - iter_begin;
      r++;
      nx += 1 + (int)(-log(g.uniform()) / lambda);
   }
   __builtin_amdgcn_wave_barrier();
   // (a pending carry cannot survive to here: a twist is only made to take words, which takes the carry first)
   for (int i=lane; i<624; i+=64) state[(size_t) i * n_runs + k] = g.mt[i];
   if (lane == 0) { state[(size_t) 624 * n_runs + k] = (uint32_t) g.mti; next[k] = nx; }
}

} // namespace

hipError_t orc_launch_hmc_seed(uint32_t * state, int * next, const unsigned int * seeds, int n_runs, hipStream_t stream)
{
   hipLaunchKernelGGL(hmc_seed_kernel, dim3((n_runs + 63) / 64), dim3(64), 0, stream, state, next, seeds, n_runs);
   return hipGetLastError();
}
hipError_t orc_launch_hmc_plan(uint32_t * state, int * next, int n_runs, int iter_begin, int iter_end, int cap, size_t mn, double lambda,
   int precision, void * noise, int * iters, int * overflow, hipStream_t stream)
{
   const dim3 grid((n_runs + ORC_HMC_WAVES - 1) / ORC_HMC_WAVES), block(64 * ORC_HMC_WAVES);
   if (precision == 64) hipLaunchKernelGGL(hmc_plan_kernel<double>, grid, block, 0, stream, state, next, n_runs, iter_begin, iter_end, cap, mn, lambda, (double *) noise, iters, overflow);
   else hipLaunchKernelGGL(hmc_plan_kernel<float>, grid, block, 0, stream, state, next, n_runs, iter_begin, iter_end, cap, mn, lambda, (float *) noise, iters, overflow);
   return hipGetLastError();
}
