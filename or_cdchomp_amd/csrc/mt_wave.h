// mt_wave.h -- GSL's default generator (mt19937, polar Box-Muller) drawn by ONE WAVEFRONT per stream.
//
// Shared by the kernels that draw on the device what the reference draws from a run's own GSL stream
// (gsl_rng_default = mt19937, gsl_ran_gaussian, gsl_rng_uniform; src/orcdchomp_mod.cpp:2303-2304, 2755-2768):
// the momentum resampling plan of HMC runs (hmc_kernels.hip) and the seed perturbation of multi-start batches
// (multistart_kernels.hip).  A stream is sequential in the reference, but every step of it is either a whole-state
// operation or independent per pair of outputs:
//   * the MT19937 twist of the 624-word state: lane i of a 64-lane step reads mt[i], mt[i+1],
//     mt[i+397] and writes mt[i]; the steps run in order, which is exactly the recurrence's order of
//     dependence (a step only reads words of later steps before they change, and new words of
//     earlier steps);
//   * polar Box-Muller (gsl_ran_gaussian): an attempt takes two outputs and is accepted or not on
//     their own merit, so the k-th Gaussian is the k-th accepted PAIR of the stream: 64 pairs are
//     tried at once, the accepted ones are compacted with a ballot, and the stream position moves
//     to the end of the last pair used;
//   * gsl_rng_uniform_pos skips an output word that is 0 (probability 2^-32 per word, i.e. about
//     once per 50 launches of 4096 runs): a chunk that contains one is redone by a one-at-a-time walk
//     (seeds 7603642 and 7627928 have one among their first 535 words: tests/hmc_stream.py, NOTES/hmc-stream.md).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

struct MtWave
{
   uint32_t * mt;          // [624] in LDS, this run's state
   int mti;                // next unread word of the state (624: none left)
   int has_carry;          // the last word of the previous state is still unread ...
   uint32_t carry;         // ... and this is its tempered value
   static __device__ __forceinline__ uint32_t temper(uint32_t k)
   {
      k ^= (k >> 11);
      k ^= (k << 7) & 0x9d2c5680U;
      k ^= (k << 15) & 0xefc60000U;
      k ^= (k >> 18);
      return k;
   }
   // gsl_rng_set: the state of a fresh stream (seed 0 is GSL's 4357); every lane walks the same recurrence and
   // writes the words of its own column, so the state is complete after a wave barrier
   __device__ __forceinline__ void seed(unsigned long s)
   {
      const int lane = threadIdx.x & 63;
      if (s == 0) s = 4357;
      uint32_t prev = (uint32_t)(s & 0xffffffffUL);
      if (lane == 0) mt[0] = prev;
      for (int i=1; i<624; i++)
      {
         prev = (uint32_t)(1812433253UL * (prev ^ (prev >> 30)) + (uint32_t) i);
         if ((i & 63) == lane) mt[i] = prev;
      }
      mti = 624; has_carry = 0; carry = 0;
      __builtin_amdgcn_wave_barrier();
   }
   __device__ __forceinline__ int avail() const { return has_carry + (624 - mti); }
   // word j of the unread stream (j < avail()), tempered
   __device__ __forceinline__ uint32_t peek(int j) const
   {
      if (j < has_carry) return carry;
      return temper(mt[mti + j - has_carry]);
   }
   __device__ __forceinline__ void consume(int words)
   {
      mti += words - has_carry;      // (words >= 1 whenever a carry is pending)
      has_carry = 0;
   }
   // the next 624 words; a single unread word of the old state is kept as the carry
   __device__ __forceinline__ void twist()
   {
      const int lane = threadIdx.x & 63;
      if (mti == 623) { carry = temper(mt[623]); has_carry = 1; }
      for (int base=0; base<624; base+=64)
      {
         const int i = base + lane;
         if (i < 624)
         {
            const uint32_t a = mt[i], b = mt[(i + 1 == 624) ? 0 : i + 1], c = mt[(i + 397 >= 624) ? i + 397 - 624 : i + 397];
            const uint32_t y = (a & 0x80000000U) | (b & 0x7fffffffU);
            mt[i] = c ^ (y >> 1) ^ ((y & 1U) ? 0x9908b0dfU : 0U);
         }
         __builtin_amdgcn_wave_barrier();
      }
      mti = 0;
   }
   // one word, one at a time (every lane computes the same): gsl_rng_get
   __device__ __forceinline__ uint32_t get()
   {
      if (avail() == 0) twist();
      const uint32_t k = peek(0);
      consume(1);
      return k;
   }
   __device__ __forceinline__ double uniform() { return get() / 4294967296.0; }
   __device__ __forceinline__ double uniform_pos() { double x; do { x = uniform(); } while (x == 0); return x; }
   __device__ double gaussian_one(double sigma)
   {
      double x, y, r2;
      do
      {
         x = -1 + 2 * uniform_pos();
         y = -1 + 2 * uniform_pos();
         r2 = x*x + y*y;
      }
      while (r2 > 1.0 || r2 == 0);
      return sigma * y * sqrt(-2.0 * log(r2) / r2);
   }
   // the next `count` values of gsl_ran_gaussian(sigma), written to out[0 .. count) by the lanes that drew them
   template <typename real>
   __device__ __forceinline__ void gaussians(real * out, size_t count, double sigma)
   {
      const int lane = threadIdx.x & 63;
      size_t done = 0;
      while (done < count)
      {
         if (avail() < 2) { twist(); }
         const int pairs = (avail() / 2 < 64) ? avail() / 2 : 64;
         const bool mine = (lane < pairs);
         const uint32_t w1 = mine ? peek(2*lane) : 1u, w2 = mine ? peek(2*lane + 1) : 1u;
         if (__builtin_amdgcn_ballot_w64(w1 == 0u || w2 == 0u) != 0ull)
         {
            // an output word that uniform_pos skips: this Gaussian by the one-at-a-time walk
            const double v = gaussian_one(sigma);
            if (lane == 0) out[done] = (real) v;
            done++;
            continue;
         }
         const double x = -1 + 2 * (w1 / 4294967296.0), y = -1 + 2 * (w2 / 4294967296.0);
         const double r2 = x*x + y*y;
         const bool acc = mine && !(r2 > 1.0 || r2 == 0);
         const unsigned long long accm = __builtin_amdgcn_ballot_w64(acc);
         const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(accm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) accm, 0u));
         const size_t need = count - done;
         const int cnt = __popcll(accm);
         if (acc && (size_t) rank < need) out[done + rank] = (real)(sigma * y * sqrt(-2.0 * log(r2) / r2));
         if ((size_t) cnt >= need)
         {
            // the stream stops behind the pair of the last Gaussian wanted
            const unsigned long long lastm = __builtin_amdgcn_ballot_w64(acc && (size_t) rank == need - 1);
            consume(2 * (__builtin_ctzll(lastm) + 1));
            done = count;
         }
         else { consume(2 * pairs); done += cnt; }
      }
   }
};
