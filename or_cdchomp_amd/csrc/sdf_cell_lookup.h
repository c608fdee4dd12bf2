// sdf_cell_lookup.h -- the field lookup in cell units (DevSdfCell) of the cost passes with one lookup per lane, cost_gs16.h
// and cost_pairs.h (the many-sphere pass splits its lookup in two: sdf_issue / sdf_finish of cost_generic.h).  Included by
// chomp_kernel.hip inside its namespace, in front of the cost headers.  Reference: src/libcd/grid.c:191-209, 331-454.
#pragma once

// The lookup for ONE field whose axes are the world's, in cell units (DevSdfCell), the descriptor in scalar registers:
// g = sol p + t per axis, value = v0 + sum (after - before) (g - (sub + 0.5)), world gradient = sol (after - before).
// Returns whether p is inside the field (value / gradient are only meaningful then).
template <typename real, typename CD>
__device__ __forceinline__ bool sdf_lookup_cell_aligned(const CD & F, const real p[3], real & value, real gw[3])
{
   real fr[3]; bool prev[3];
   bool inb = true;
   int off = 0;
#pragma unroll
   for (int k=0; k<3; k++)
   {
      const real gx = F.M[4*k] * p[k] + F.t[k];
      inb = inb && !(gx < (real)0) && !(gx > F.fsize[k]);
      real fl = M<real>::floor_(gx);
      fl = M<real>::max_(M<real>::min_(fl, F.fsize_m1[k]), (real)0);      // g == size: the last cell (grid.c:203); outside: clamped, masked by inb
      fr[k] = (gx - fl) - (real)0.5;
      prev[k] = (fl == (real)0) ? false : ((fl == F.fsize_m1[k]) ? true : (fr[k] < (real)0));
      off += (int) fl * ((k == 2) ? (int) sizeof(real) : F.stride_b[k]);
   }
   const char * base = (const char *) F.data;
   const real v0 = *(const real *)(base + off);
   real vn[3];
#pragma unroll
   for (int k=0; k<3; k++)
   {
      const int sb = (k == 2) ? (int) sizeof(real) : F.stride_b[k];
      vn[k] = *(const real *)(base + (off + (prev[k] ? -sb : sb)));
   }
   const real inf = M<real>::inf();
   bool poisoned = (v0 == inf);
   real v = v0;
#pragma unroll
   for (int k=2; k>=0; k--)                     // the reference walks the axes z, y, x
   {
      poisoned = poisoned || (vn[k] == inf);
      const real dd = vn[k] - v0;
      const real df = prev[k] ? -dd : dd;       // after - before
      gw[k] = F.W[4*k] * df;
      v += df * fr[k];
   }
   value = poisoned ? inf : v;
   return inb;
}

// The same lookup in fp64 with fewer issue slots: which side the one-sided difference looks at is a SIGN (+-1.0: one
// select of a high word) instead of a flag, so the neighbour's offset is one fused multiply-add, `after - before` one product
// (exact: the factor is +-1), and the cell offset is formed in fp64 (exact below 2^53) and converted once: no quarter-rate
// integer multiply, no 64-bit address arithmetic (unsigned 32-bit offsets against the field's base in scalar registers).
// Bit-identical to sdf_lookup_cell_aligned.
template <typename CD>
__device__ __forceinline__ bool sdf_lookup_cell_aligned_lean(const CD & F, const double p[3], double & value, double gw[3])
{
   double fr[3], sgn[3], fl[3];
   bool inb = true;
   // the descriptor's scalars in one burst in front of the tests (a chain of `&&` makes a ladder of branches with a scalar load and a wait on
   // every rung, as in cost_generic.h)
   double Md[3], td[3], fsd[3], fmd[3];
#pragma unroll
   for (int k=0; k<3; k++) { Md[k] = F.M[4*k]; td[k] = F.t[k]; fsd[k] = F.fsize[k]; fmd[k] = F.fsize_m1[k]; }
#pragma unroll
   for (int k=0; k<3; k++) { __asm__ volatile("" : "+s"(Md[k])); __asm__ volatile("" : "+s"(td[k])); __asm__ volatile("" : "+s"(fsd[k])); __asm__ volatile("" : "+s"(fmd[k])); }
#pragma unroll
   for (int k=0; k<3; k++)
   {
      const double gx = Md[k] * p[k] + td[k];
      inb = inb & !(gx < 0.0) & !(gx > fsd[k]);
      double f0 = M<double>::floor_(gx);
      f0 = M<double>::max_(M<double>::min_(f0, fmd[k]), 0.0);
      fl[k] = f0;
      fr[k] = (gx - f0) - 0.5;
      // -1: the cell before (previous) is the other end of the difference; +1: the cell after
      const int hi_mid = (fr[k] < 0.0) ? (int) 0xBFF00000 : 0x3FF00000;
      const int hi_end = (f0 == fmd[k]) ? (int) 0xBFF00000 : hi_mid;
      sgn[k] = __hiloint2double((f0 == 0.0) ? 0x3FF00000 : hi_end, 0);
   }
   const double offr = fma(fl[0], F.stride_r[0], fma(fl[1], F.stride_r[1], fl[2] * F.stride_r[2]));
   const char * base = (const char *) F.data;
   const double v0 = *(const double *)(base + (unsigned int) (int) offr);
   double vn[3];
#pragma unroll
   for (int k=0; k<3; k++)
      vn[k] = *(const double *)(base + (unsigned int) (int) fma(sgn[k], F.stride_r[k], offr));
   const double inf = M<double>::inf();
   bool poisoned = (v0 == inf);
   double v = v0;
#pragma unroll
   for (int k=2; k>=0; k--)                     // the reference walks the axes z, y, x
   {
      poisoned = poisoned || (vn[k] == inf);
      const double df = sgn[k] * (vn[k] - v0);  // after - before
      gw[k] = F.W[4*k] * df;
      v += df * fr[k];
   }
   value = poisoned ? inf : v;
   return inb;
}

// ... and for a field in general position (rotated against the world): g = M p + t, world gradient W (after - before)
template <typename real, typename CD>
__device__ __forceinline__ bool sdf_lookup_cell(const CD & F, const real p[3], real & value, real gw[3])
{
   real fr[3]; bool prev[3];
   bool inb = true;
   int off = 0;
#pragma unroll
   for (int k=0; k<3; k++)
   {
      const real gx = F.M[k*3+0]*p[0] + F.M[k*3+1]*p[1] + F.M[k*3+2]*p[2] + F.t[k];
      inb = inb && !(gx < (real)0) && !(gx > F.fsize[k]);
      real fl = M<real>::floor_(gx);
      fl = M<real>::max_(M<real>::min_(fl, F.fsize_m1[k]), (real)0);
      fr[k] = (gx - fl) - (real)0.5;
      prev[k] = (fl == (real)0) ? false : ((fl == F.fsize_m1[k]) ? true : (fr[k] < (real)0));
      off += (int) fl * ((k == 2) ? (int) sizeof(real) : F.stride_b[k]);
   }
   const char * base = (const char *) F.data;
   const real v0 = *(const real *)(base + off);
   real vn[3];
#pragma unroll
   for (int k=0; k<3; k++)
   {
      const int sb = (k == 2) ? (int) sizeof(real) : F.stride_b[k];
      vn[k] = *(const real *)(base + (off + (prev[k] ? -sb : sb)));
   }
   const real inf = M<real>::inf();
   bool poisoned = (v0 == inf);
   real v = v0, df[3];
#pragma unroll
   for (int k=2; k>=0; k--)                     // the reference walks the axes z, y, x
   {
      poisoned = poisoned || (vn[k] == inf);
      const real dd = vn[k] - v0;
      df[k] = prev[k] ? -dd : dd;               // after - before
      v += df[k] * fr[k];
   }
#pragma unroll
   for (int k=0; k<3; k++) gw[k] = F.W[k*3+0]*df[0] + F.W[k*3+1]*df[1] + F.W[k*3+2]*df[2];
   value = poisoned ? inf : v;
   return inb;
}
