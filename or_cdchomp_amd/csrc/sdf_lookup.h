// sdf_lookup.h -- the field lookup of the kernels (cost phases of chomp_kernel.hip, the collision verdicts) and the
// precision's math functions it is written in.  Included inside the including file's own namespace, after dev_types.h.
#pragma once

// NS1 ceiling experiment (scripts/ns1_ceiling.sh): with ORC_ABLATE_SDFLDS the four cell reads of a
// lookup go to LDS (the tile's position buffer stands in for a staged field: wrong values, the same
// instruction stream), which bounds from above what ANY LDS staging of the field could gain
#ifdef ORC_ABLATE_SDFLDS
#define ORC_SDF_IDX(i) ((i) & 1023)
#else
#define ORC_SDF_IDX(i) (i)
#endif

template <typename real> struct M;
template <> struct M<double>
{
   static __device__ __forceinline__ double sqrt_(double x) { return ::sqrt(x); }
   static __device__ __forceinline__ double floor_(double x) { return ::floor(x); }
   static __device__ __forceinline__ double fabs_(double x) { return ::fabs(x); }
   static __device__ __forceinline__ double max_(double a, double b) { return ::fmax(a, b); }
   static __device__ __forceinline__ double min_(double a, double b) { return ::fmin(a, b); }
   static __device__ __forceinline__ void sincos_(double x, double * s, double * c) { ::sincos(x, s, c); }
   static __device__ __forceinline__ double inf() { return __longlong_as_double(0x7ff0000000000000LL); }
};
template <> struct M<float>
{
   static __device__ __forceinline__ float sqrt_(float x) { return ::sqrtf(x); }
   static __device__ __forceinline__ float floor_(float x) { return ::floorf(x); }
   static __device__ __forceinline__ float fabs_(float x) { return ::fabsf(x); }
   static __device__ __forceinline__ float max_(float a, float b) { return ::fmaxf(a, b); }
   static __device__ __forceinline__ float min_(float a, float b) { return ::fminf(a, b); }
   static __device__ __forceinline__ void sincos_(float x, float * s, float * c) { ::sincosf(x, s, c); }
   static __device__ __forceinline__ float inf() { return __int_as_float(0x7f800000); }
};

// ---------------------------------------------------------------------------
// SDF lookup: cd_grid_lookup_index + cd_grid_double_interp + cd_grid_double_grad
// fused (they read the same four cells).  src/libcd/grid.c:191-209, 331-454.
// returns 0 and value/grad, or 1 when p is outside the field.
template <typename real>
__device__ __forceinline__ int sdf_lookup(const DevSdf<real> & f, const real p[3], real & value, real grad[3])
{
   // the reference divides (x = p/len, centre = (0.5+sub)/size*len, slope = diff*size/len);
   // here the three quotients per axis are host-precomputed reciprocals (<= 1 ulp apart)
   int sub[3];
#pragma unroll
   for (int d=0; d<3; d++)
   {
      const real x = p[d] * f.inv_length[d];
      if (x < (real)0) return 1;
      if (x > (real)1) return 1;
      int sb = (int) M<real>::floor_(x * (real) f.size[d]);
      if (sb == f.size[d]) sb--;
      sub[d] = sb;
   }
   const int stride[3] = { f.size[1] * f.size[2], f.size[2], 1 };
   const int index = sub[0]*stride[0] + sub[1]*stride[1] + sub[2];
   const real v0 = f.data[ORC_SDF_IDX(index)];
   real va[3], vb[3], center[3];
#pragma unroll
   for (int d=0; d<3; d++)
   {
      center[d] = ((real)0.5 + (real) sub[d]) * f.cell[d];
      bool prev;
      if (sub[d] == 0) prev = false;
      else if (sub[d] == f.size[d]-1) prev = true;
      else prev = (p[d] < center[d]);
      const real vn = f.data[ORC_SDF_IDX(prev ? index - stride[d] : index + stride[d])];
      va[d] = prev ? v0 : vn;      // "after"
      vb[d] = prev ? vn : v0;      // "before"
   }
   const real inf = M<real>::inf();
   real v = v0;
   bool poisoned = (v0 == inf);
   // the reference walks the axes last to first (z, y, x)
#pragma unroll
   for (int d=2; d>=0; d--)
   {
      if (va[d] == inf || vb[d] == inf) poisoned = true;
      real diff = va[d];
      diff -= vb[d];
      const real slope = diff * f.size_over_len[d];
      grad[d] = slope;
      v += slope * (p[d] - center[d]);
   }
   value = poisoned ? inf : v;
   return 0;
}
