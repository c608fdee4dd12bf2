// fast_math.h -- the iterate kernel's reciprocal, square root and small integer division: the hardware seeds plus
// Newton/Goldschmidt steps, ~1 ulp, a third of the instructions of the IEEE division / sqrt expansions.
//
// Included by chomp_kernel.hip inside its namespace, after sdf_lookup.h (M<real>).
#pragma once

// 1/x
__device__ __forceinline__ double rcp_fast(double x)
{
   double r = __builtin_amdgcn_rcp(x);
   r = fma(fma(-x, r, 1.0), r, r);
   r = fma(fma(-x, r, 1.0), r, r);
   return r;
}
__device__ __forceinline__ float rcp_fast(float x) { return 1.0f / x; }

// returns sqrt(x); *inv = 1/sqrt(x), for x > 0 known (pair distances: the caller substitutes 1 where there is no pair): the
// Goldschmidt core, without the guards for x == 0.  (One Goldschmidt step would do for the square root -- 1.1e-16 over 2^20 values,
// scripts/ubench/rsq_prec.hip -- but leaves its reciprocal at 4e-15, and the three instructions saved per
// pair evaluation do not show in the throughput: kept at two.)
__device__ __forceinline__ double sqrt_rsq_pos(double x, double * inv)
{
   double r = __builtin_amdgcn_rsq(x);
   double g = x * r, h = 0.5 * r;
#pragma unroll
   for (int k=0; k<2; k++)
   {
      const double e = fma(-h, g, 0.5);
      g = fma(g, e, g);
      h = fma(h, e, h);
   }
   const double d = fma(-g, g, x);
   g = fma(d, h, g);
   *inv = 2.0 * h;
   return g;
}
// the same for any x >= 0: the core plus its guard.  x == 0 gives 0 and inf.
__device__ __forceinline__ double sqrt_rsq(double x, double * inv)
{
   double i;
   const double g = sqrt_rsq_pos(x, &i);
   const bool zero = !(x > 0.0);
   *inv = zero ? M<double>::inf() : i;
   return zero ? 0.0 : g;
}
__device__ __forceinline__ float sqrt_rsq(float x, float * inv)
{
   const float g = ::sqrtf(x);
   *inv = 1.0f / g;
   return g;
}
__device__ __forceinline__ float sqrt_rsq_pos(float x, float * inv) { return sqrt_rsq(x, inv); }

// e / n for 0 <= e < 2^20 without the ~35-instruction integer division: (e + 0.5)/n is at least
// 0.5/n away from an integer, far more than the rounding of the float product.  rn = 1.0f / n.
__device__ __forceinline__ int div_n(int e, float rn) { return (int)(((float) e + 0.5f) * rn); }
