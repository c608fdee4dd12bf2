// band.h -- A T + B of the smoothness metric, row by row: the tridiagonal Toeplitz row of derivative 1 (smooth_grad), the band
// row of any other metric (band_row), and the two passes over the trajectory that need the latter as functions of their own
// (band_gradient_pass for the update phase, band_cost_pass for the cost sums).
//
// Included by chomp_kernel.hip inside its namespace, after wave.h and fast_math.h.
#pragma once

// Row i, column c of A T + B for a higher derivative (|D| >= 2, or derivative 1 without a start boundary), in the
// accumulation type `acc` (double for fp32 runs: the band's entries are ~1/dt^4, 1e7 for 200 waypoints, and the row's sum is of
// order one to a hundred -- summed in fp32 the rounding alone is of that order; `tab` is then the band in double).
// bt_out: the row's term of B alone (beta_s[i] q_start + beta_g[i] q_goal).
// Away from the D rows at either end the band is Toeplitz and B is zero (DevBatch::band_toeplitz, checked on the host): the
// 2D+1 coefficients are scalars of the kernarg block.  The end rows read their coefficients from the table -- all loads issued
// before the first use (a loop over a run-time D made one L2 round trip per coefficient: 4 k cycles per entry, a third of the
// update phase of a `derivative 2` run).
template <typename real, typename acc, typename BT>
__device__ __forceinline__ acc band_row(const BT & b, const real * tab, const real * T_s, int i, int c, acc & bt_out)
{
   constexpr int R = ORC_SS_MAX_RANK;
   const int m = b.m, n = b.n;
   const int D = (b.D < 0) ? -b.D : b.D;      // (-1: tridiagonal without a start boundary, DevBatch::D)
   const bool dbl = (sizeof(acc) == 8 && sizeof(real) == 4);
   // (the Toeplitz row's coefficients first, all of them and before any branch: scalar loads of the kernarg block that are then
   // certain to execute, so the compiler can move them out of the callers' loops)
   acc cf[R+1];
#pragma unroll
   for (int k=0; k<=R; k++) cf[k] = dbl ? (acc) b.band_c64[k] : (acc) b.band_c[k];
   const int toep = b.band_toeplitz;      // (set only with solve_mode 3: the end rows are in the metric's table)
   if (D >= 2 && D <= R && toep && sizeof(acc) == 8)
   {
      // Every lane evaluates the Toeplitz row (at a clamped row index, so that all reads are unconditional); the wavefronts that
      // hold one of the D rows at either end then evaluate that row from the metric's table as well -- 2D+1 coefficients and the two
      // couplings, contiguous, read unconditionally (a lane that has no end row reads row 0; coefficients of columns outside the
      // matrix are stored as zeros and meet a clamped trajectory row) -- and the lanes pick.  As predicated reads the end rows
      // cost ~300 vector instructions of address arithmetic and branches for the two wavefronts that hold them: 4 k cycles per pass.
      const bool is_end = !(i >= D && i < m - D);
      const int ic = (i < D) ? D : ((i >= m - D) ? m - D - 1 : i);
      const real * rowT = T_s + (ic+1)*n + c;
      acc sum = (acc)0;
      switch (D)      // (wave-uniform; the sums run from k = -D upwards, the order of the reference's dense row)
      {
      case 2:
#pragma unroll
         for (int k=-2; k<=2; k++) sum += cf[k < 0 ? -k : k] * (acc) rowT[k*n];
         break;
      case 3:
#pragma unroll
         for (int k=-3; k<=3; k++) sum += cf[k < 0 ? -k : k] * (acc) rowT[k*n];
         break;
      default:
#pragma unroll
         for (int k=-4; k<=4; k++) sum += cf[k < 0 ? -k : k] * (acc) rowT[k*n];
         break;
      }
      acc bt = (acc)0;
#if defined(ORC_ABLATE_BANDEND)      // (timing experiments: the end rows take the Toeplitz row -- wrong results)
      if (false)
#else
      if (__builtin_amdgcn_ballot_w64(is_end) != 0ull)
#endif
      {
         const int er = is_end ? ((i < D) ? i : i - (m - 2*D)) : 0;
         const double * row = (const double *) tab + 2*D*m + er * (2*D + 3);
         const acc bte = (acc) row[2*D+1] * (acc) T_s[c] + (acc) row[2*D+2] * (acc) T_s[(b.n_points-1)*n + c];
         acc se = bte;
         auto end_row = [&](auto dd) {
            constexpr int DD = decltype(dd)::value;
#pragma unroll
            for (int k=-DD; k<=DD; k++)
            {
               const int r = i + k, rc = (r < 0) ? 0 : ((r >= m) ? m - 1 : r);
               se += (acc) row[k+DD] * (acc) T_s[(rc+1)*n + c];
            }
         };
         switch (D)
         {
         case 2: end_row(std::integral_constant<int, 2>{}); break;
         case 3: end_row(std::integral_constant<int, 3>{}); break;
         default: end_row(std::integral_constant<int, 4>{}); break;
         }
         sum = is_end ? se : sum;
         bt = is_end ? bte : bt;
      }
      bt_out = bt;
      return sum;
   }
   const acc * tabA = dbl ? (const acc *) b.metric64 : (const acc *) b.Aband;
   const acc * tbs = dbl ? tabA + (size_t)(2*D + 1) * m : (const acc *) b.beta_s;
   const acc * tbg = dbl ? tbs + m : (const acc *) b.beta_g;
   const acc bt = tbs[i] * (acc) T_s[c] + tbg[i] * (acc) T_s[(b.n_points-1)*n + c];
   bt_out = bt;
   acc sum = bt;
   if (D <= R)
   {
      acc a[2*R+1], t[2*R+1];
#pragma unroll
      for (int q=0; q<2*R+1; q++)
      {
         const int k = q - R, r = i + k;
         const bool ok = (k >= -D) && (k <= D) && (r >= 0) && (r < m);
         a[q] = ok ? tabA[(size_t)(k+D) * m + i] : (acc)0;
         t[q] = ok ? (acc) T_s[(r+1)*n + c] : (acc)0;
      }
#pragma unroll
      for (int q=0; q<2*R+1; q++)
      {
         const int k = q - R, r = i + k;
         if ((k >= -D) && (k <= D) && (r >= 0) && (r < m)) sum += a[q] * t[q];
      }
      return sum;
   }
   for (int k=-D; k<=D; k++)
   {
      const int r = i + k;
      if (r < 0 || r >= m) continue;
      sum += tabA[(size_t)(k+D) * m + i] * (acc) T_s[(r+1)*n + c];
   }
   return sum;
}

// (A T + B)[i][c] of the tridiagonal Toeplitz metric of derivative 1: the end rows couple to the fixed endpoints with a_off.
// T_s holds all n_points rows (row 0 = start, row n_points-1 = goal).
template <typename real, typename BT>
__device__ __forceinline__ real smooth_grad(const BT & b, const real * T_s, int i, int c)
{
   const int n = b.n;
   // In double whatever `real` is (the same bits in fp64; a product of two floats is exact in double), and rounded once: the row is a
   // second difference, its terms of size a |T|, its value a |T''| dt^2, and float rounds it at a |T| 2^-24.  Of the gradient that is as
   // much as the waypoints' own float rounding moves it; but A^-1 takes A dT back to dT, while it passes this error on at its full
   // size: A^-1 G of a 34-waypoint fp32 run was off by 4e-5 of its largest row, 56 x what the float rounding of the waypoints moves it
   // (NOTES/first-iteration.md).  phase_costs_body forms the row the same way.
   if (sizeof(real) == 4)
      return (real)((double) b.a_diag * (double) T_s[(i+1)*n + c] + (double) b.a_off * ((double) T_s[i*n + c] + (double) T_s[(i+2)*n + c]));
   return b.a_diag * T_s[(i+1)*n + c] + b.a_off * (T_s[i*n + c] + T_s[(i+2)*n + c]);
}
// The two passes over the trajectory that need A T + B, for a metric that is not that one (a higher derivative; derivative 1
// without a start boundary): G = G/m + A T + B of the update phase and 0.5 tr(T^T A T) + tr(B^T T) of the cost pass, as FUNCTIONS of
// their own -- inlined, band_row tripled the lean update phase of every `derivative 1` kernel (2.1 k -> 5.4 k instructions) and cost
// BASELINE configs[1] 1 % through the instruction cache alone (profiles/r06_ab_experiments.txt).
template <typename real, int BLOCK>
__device__ __attribute__((noinline)) void band_gradient_pass(const void * kp, const real * tab_in, const real * T_in, const real * Gc_in, real * G_in, int tid)
{
   // (the kernarg block's address, wave-uniform again: an address in the constant address space, so through uni64 as it stands)
   const __attribute__((address_space(4))) DevBatch<real> & b = *(const __attribute__((address_space(4))) DevBatch<real> *) uni64((unsigned long long) kp);
   const real * tab = uniform_ptr(tab_in), * T_s = uniform_ptr(T_in);
   const real * Gc = uniform_ptr(Gc_in);
   real * G_s = uniform_ptr(G_in);
   const int n = b.n, mn = b.m*n;
   const float rn_f = 1.0f / (float) n;
   for (int e=tid; e<mn; e+=BLOCK)
   {
      const int i = div_n(e, rn_f), c = e - i*n;
      real g = Gc[e];
      g *= b.inv_m;
      if (sizeof(real) == 4 && b.metric64) { double bt; g += (real) band_row<real, double>(b, tab, T_s, i, c, bt); }
      else { real bt; g += band_row<real, real>(b, tab, T_s, i, c, bt); }
      G_s[e] = g;
   }
}
template <typename real, int BLOCK>
__device__ __attribute__((noinline)) double band_cost_pass(const void * kp, const real * tab_in, const real * T_in, int tid)
{
   const __attribute__((address_space(4))) DevBatch<real> & b = *(const __attribute__((address_space(4))) DevBatch<real> *) uni64((unsigned long long) kp);
   const real * tab = uniform_ptr(tab_in), * T_s = uniform_ptr(T_in);
   const int n = b.n, mn = b.m*n;
   const float rn_f = 1.0f / (float) n;
   double acc = 0.0;
   for (int e=tid; e<mn; e+=BLOCK)
   {
      const int i = div_n(e, rn_f), c = e - i*n;
      if (sizeof(real) == 4 && b.metric64)
      {
         // fp32 and a higher derivative: the band's entries are ~1/dt^4 and the sum is of order one, so this one sum is
         // taken in double from the band in double (the trajectory is what it is: its rounding costs ~1e-5 of the sum)
         double bt;
         const double sd = band_row<real, double>(b, tab, T_s, i, c, bt);
         acc += (double) T_s[n + e] * (0.5 * (sd + bt));
      }
      else
      {
         real bt;
         const real sg = band_row<real, real>(b, tab, T_s, i, c, bt);
         acc += (double) T_s[n + e] * (0.5 * ((double) sg + (double) bt));
      }
   }
   return acc;
}
