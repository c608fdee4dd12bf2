// metric_solve.h -- x = A^-1 g for the smoothness metric of the CHOMP iteration, in its four forms: parallel cyclic reduction,
// the dense inverse, the closed-form scans of the tridiagonal Toeplitz metric (derivative 1) and the scans over the generators
// of a band metric's semiseparable inverse (a higher derivative); metric_solve picks by DevBatch::solve_mode.  The column
// forms (toeplitz_scan_column_any, semisep_scan_column_any) serve the joint-limit rounds of limit_rounds.h as well.
//
// Included by chomp_kernel.hip inside its namespace, after wave.h and fast_math.h.
#pragma once

// ---------------------------------------------------------------------------
// parallel cyclic reduction with precomputed multipliers: x = A^-1 d for all n
// columns at once.  src holds d [m][n]; the result ends up in the returned
// buffer (src or tmp).  Coefficients: pcr[l][0][i] (towards i-s), pcr[l][1][i]
// (towards i+s), then the inverse of the reduced diagonal.
template <typename real, int BLOCK, typename BT>
__device__ __forceinline__ real * pcr_solve(const BT & b, const real * tab, real * src, real * tmp, int tid)
{
   const int m = b.m, n = b.n, mn = m*n;
   const float rn = 1.0f / (float) n;
   real * cur = src;
   real * nxt = tmp;
   int stride = 1;
   for (int l=0; l<b.pcr_levels; l++)
   {
      const real * ka = tab + (size_t)(b.pcr_sym ? l : 2*l) * m;
      const real * kc = ka + m;
      for (int e=tid; e<mn; e+=BLOCK)
      {
         const int i = div_n(e, rn);
         real d = cur[e];
         if (i - stride >= 0) d += ka[i] * cur[e - stride*n];
         if (i + stride < m)  d += (b.pcr_sym ? ka[m-1-i] : kc[i]) * cur[e + stride*n];
         nxt[e] = d;
      }
      __syncthreads();
      real * t = cur; cur = nxt; nxt = t;
      stride <<= 1;
   }
   const real * invb = tab + (size_t)(b.pcr_rows - 1) * m;
   for (int e=tid; e<mn; e+=BLOCK)
      cur[e] *= invb[div_n(e, rn)];
   __syncthreads();
   return cur;
}

// dense fallback (derivative D >= 2): x = Ainv d
template <typename real, int BLOCK, typename BT>
__device__ __forceinline__ real * dense_solve(const BT & b, real * src, real * tmp, int tid)
{
   const int m = b.m, n = b.n, mn = m*n;
   for (int e=tid; e<mn; e+=BLOCK)
   {
      const int i = e / n, c = e - i*n;
      real s = (real)0;
      for (int k=0; k<m; k++) s += b.Ainv[(size_t) i*m + k] * src[k*n + c];
      tmp[e] = s;
   }
   __syncthreads();
   return tmp;
}

// The closed-form scan solve below for trajectories of more than 64 ORC_SCAN_RPL moving waypoints (round 6): the lane's rows read
// twice instead of held in registers -- a pass for the lane's two partial sums, the wave scans, a pass that forms x row by row
// (the rows-after sum by taking the lane's own rows off the suffix scan's inclusive value) -- still ONE barrier per solve, where
// cyclic reduction pays one per level: 300 waypoints ran at 0.6 of the waypoint-iterations/s of 258 (profiles/r06_long_trajectories.txt).
template <typename real, typename PT>
__device__ __forceinline__ void toeplitz_scan_column_long(PT buf, int m, int n, int c, int rpl, real kinv)
{
   const int lane = threadIdx.x & 63;
   const int row0 = lane*rpl;
   real sp = 0, sq = 0;
   for (int r=0; r<rpl; r++)
   {
      const int row = row0 + r;
      if (row >= m) break;
      const real g = buf[row*n + c];
      sp += g * (real)(row + 1); sq += g * (real)(m - row);
   }
   const real ip = wave_prefix_incl(sp);
   real run_p = __shfl_up(ip, 1, 64); if (lane == 0) run_p = 0;      // rows before this lane's
   real run_q = wave_suffix_incl(sq);                                // rows from this lane's first on
   for (int r=0; r<rpl; r++)
   {
      const int row = row0 + r;
      if (row >= m) break;
      const real g = buf[row*n + c];
      const real wp = (real)(row + 1), wq = (real)(m - row);
      run_p += g * wp;                                               // rows up to row r
      run_q -= g * wq;                                               // rows after row r
      buf[row*n + c] = kinv * (wq * run_p + wp * run_q);
   }
}

// one column of toeplitz_scan_solve, by the calling wavefront: buf[:, c] <- A^-1 buf[:, c]
template <typename real, typename PT>
__device__ __forceinline__ void toeplitz_scan_column(PT buf, int m, int n, int c, int rpl, real kinv)
{
   const int lane = threadIdx.x & 63;
   real g[ORC_SCAN_RPL], wp[ORC_SCAN_RPL], wq[ORC_SCAN_RPL];
   real sp = 0, sq = 0;
#pragma unroll
   for (int r=0; r<ORC_SCAN_RPL; r++)
   {
      const int row = lane*rpl + r;
      const bool valid = (r < rpl) && (row < m);
      g[r] = valid ? buf[row*n + c] : (real)0;
      wp[r] = (real)(row + 1); wq[r] = (real)(m - row);
      sp += g[r] * wp[r];
      sq += g[r] * wq[r];
   }
   // sums over the lanes before / after this one
   const real ip = wave_prefix_incl(sp), is = wave_suffix_incl(sq);
   real run_p = __shfl_up(ip, 1, 64);   if (lane == 0) run_p = 0;
   real run_q = __shfl_down(is, 1, 64); if (lane == 63) run_q = 0;
   real q[ORC_SCAN_RPL];
#pragma unroll
   for (int r=ORC_SCAN_RPL-1; r>=0; r--) { q[r] = run_q; run_q += g[r] * wq[r]; }      // rows after row r
#pragma unroll
   for (int r=0; r<ORC_SCAN_RPL; r++)
   {
      const int row = lane*rpl + r;
      run_p += g[r] * wp[r];                                                             // rows up to row r
      const real x = kinv * (wq[r] * run_p + wp[r] * q[r]);
      if ((r < rpl) && (row < m)) buf[row*n + c] = x;
   }
}
template <typename real, typename PT>
__device__ __forceinline__ void toeplitz_scan_column_any(PT buf, int m, int n, int c, real kinv)
{
   const int rpl = (m + 63) >> 6;
   if (rpl <= ORC_SCAN_RPL) toeplitz_scan_column<real>(buf, m, n, c, rpl, kinv);
   else toeplitz_scan_column_long<real>(buf, m, n, c, rpl, kinv);
}

// x = A^-1 g in place for the tridiagonal Toeplitz metric A = ca tridiag(-1, 2, -1) (derivative 1),
// all n columns of buf [m][n].  The inverse is known in closed form,
//    Ainv[i][v] = (min(i,v)+1) (m - max(i,v)) / ((m+1) ca),
// so x_i = kinv ( (m-i) sum_{v<=i} (v+1) g_v  +  (i+1) sum_{v>i} (m-v) g_v ): one prefix and one
// suffix sum per column.  A wavefront owns a column at a time, a lane `rpl` consecutive rows
// (m <= 64 ORC_SCAN_RPL); the sums across lanes are wave scans, so the whole solve costs one barrier
// where cyclic reduction costs one per level.  (The reference multiplies by the dense inverse,
// src/libcd/chomp.c:525-548: the same products, summed in another order.)
template <typename real, int BLOCK, typename BT>
__device__ __forceinline__ real * toeplitz_scan_solve(const BT & b, real * buf, int tid)
{
   const int m = b.m, n = b.n;
   const int lane = tid & 63, wave = tid >> 6;
   const int rpl = (m + 63) >> 6;
   const real kinv = (real)(-1) / ((real)(m + 1) * b.a_off);      // 1/((m+1) ca), ca = -a_off
   if (rpl > ORC_SCAN_RPL)      // (more than 256 moving waypoints: the rows are read twice instead of held in registers, above)
   {
      for (int c=wave; c<n; c+=BLOCK/64) toeplitz_scan_column_long<real>(buf, m, n, c, rpl, kinv);
      __syncthreads();
      return buf;
   }
   for (int c=wave; c<n; c+=BLOCK/64)      // (toeplitz_scan_column's body, spelled out: as a call of it the update phases compile to other code)
   {
      real g[ORC_SCAN_RPL], wp[ORC_SCAN_RPL], wq[ORC_SCAN_RPL];
      real sp = 0, sq = 0;
#pragma unroll
      for (int r=0; r<ORC_SCAN_RPL; r++)
      {
         const int row = lane*rpl + r;
         const bool valid = (r < rpl) && (row < m);
         g[r] = valid ? buf[row*n + c] : (real)0;
         wp[r] = (real)(row + 1); wq[r] = (real)(m - row);
         sp += g[r] * wp[r];
         sq += g[r] * wq[r];
      }
      // sums over the lanes before / after this one
      const real ip = wave_prefix_incl(sp), is = wave_suffix_incl(sq);
      real run_p = __shfl_up(ip, 1, 64);   if (lane == 0) run_p = 0;
      real run_q = __shfl_down(is, 1, 64); if (lane == 63) run_q = 0;
      real q[ORC_SCAN_RPL];
#pragma unroll
      for (int r=ORC_SCAN_RPL-1; r>=0; r--) { q[r] = run_q; run_q += g[r] * wq[r]; }      // rows after row r
#pragma unroll
      for (int r=0; r<ORC_SCAN_RPL; r++)
      {
         const int row = lane*rpl + r;
         run_p += g[r] * wp[r];                                                             // rows up to row r
         const real x = kinv * (wq[r] * run_p + wp[r] * q[r]);
         if ((r < rpl) && (row < m)) buf[row*n + c] = x;
      }
   }
   __syncthreads();
   return buf;
}

// x = A^-1 g for the band metric of a higher derivative (A = K_D^T K_D / N_D, half-bandwidth D = RANK: penta-diagonal for
// `derivative 2`, hepta-diagonal for 3; src/libcd/chomp.c:239-340), one column of buf [m][n] in place, by the calling wavefront.
// The inverse of a band matrix is semiseparable: Ainv[i][j] = sum_k U[k][i] V[k][j] for i <= j (generators from the host,
// host_math.cpp build_semisep; the mirror image below the diagonal), so
//    x_i = sum_k U[k][i] S_k(i) + V[k][i] P_k(i),   S_k(i) = sum_{j >= i} V[k][j] g_j,   P_k(i) = sum_{j < i} U[k][j] g_j:
// RANK prefix and RANK suffix sums per column where the Toeplitz metric of derivative 1 has one of each
// (toeplitz_scan_column).  A lane owns `rpl` consecutive rows; the sums across lanes are wave scans, in double for either
// precision of the run.  REGS: the lane's rows and table entries stay in registers (rpl <= 4); else they are read again in the
// second pass (any rpl).  The reference multiplies by the dense inverse (chomp.c:525-548, dgetrf + dgetri at 393-403).
template <typename real, int RANK, bool REGS, typename PT>
__device__ __forceinline__ void semisep_scan_column(PT buf, int m, int n, int c, int rpl, const double * U, const double * V)
{
   const int lane = threadIdx.x & 63;
   const int row0 = lane*rpl;
   double su[RANK], sv[RANK];
#pragma unroll
   for (int k=0; k<RANK; k++) { su[k] = 0.0; sv[k] = 0.0; }
   if (REGS)
   {
      // (reads are unconditional, from a clamped row: a predicated read is a branch around it plus its 64-bit address arithmetic,
      // and a lone wavefront issues a vector instruction every ~9 cycles; rows past the end take part with g = 0)
      double g[4], u[RANK][4], v[RANK][4];
#pragma unroll
      for (int r=0; r<4; r++)
      {
         if (r >= rpl) { g[r] = 0.0; for (int k=0; k<RANK; k++) { u[k][r] = 0.0; v[k][r] = 0.0; } continue; }      // (wave-uniform)
         const int row = row0 + r, rc = (row < m) ? row : m - 1;
         const double gv = (double) buf[rc*n + c];
         g[r] = (row < m) ? gv : 0.0;
#pragma unroll
         for (int k=0; k<RANK; k++)
         {
            u[k][r] = U[k*m + rc]; v[k][r] = V[k*m + rc];
            su[k] += u[k][r] * g[r]; sv[k] += v[k][r] * g[r];
         }
      }
      double P[RANK], S[RANK];
#pragma unroll
      for (int k=0; k<RANK; k++)
      {
         const double ip = wave_prefix_incl(su[k]);
         P[k] = __shfl_up(ip, 1, 64); if (lane == 0) P[k] = 0.0;      // rows before this lane's
         S[k] = wave_suffix_incl(sv[k]);                              // rows from this lane's first on
      }
#pragma unroll
      for (int r=0; r<4; r++)
      {
         if (r >= rpl) continue;
         const int row = row0 + r;
         double x = 0.0;
#pragma unroll
         for (int k=0; k<RANK; k++) x += u[k][r] * S[k] + v[k][r] * P[k];
         if (row < m) buf[row*n + c] = (real) x;
#pragma unroll
         for (int k=0; k<RANK; k++) { P[k] += u[k][r] * g[r]; S[k] -= v[k][r] * g[r]; }
      }
      return;
   }
   for (int r=0; r<rpl; r++)
   {
      const int row = row0 + r;
      if (row >= m) break;
      const double g = (double) buf[row*n + c];
#pragma unroll
      for (int k=0; k<RANK; k++) { su[k] += U[k*m + row] * g; sv[k] += V[k*m + row] * g; }
   }
   double P[RANK], S[RANK];
#pragma unroll
   for (int k=0; k<RANK; k++)
   {
      const double ip = wave_prefix_incl(su[k]);
      P[k] = __shfl_up(ip, 1, 64); if (lane == 0) P[k] = 0.0;
      S[k] = wave_suffix_incl(sv[k]);
   }
   for (int r=0; r<rpl; r++)
   {
      const int row = row0 + r;
      if (row >= m) break;
      const double g = (double) buf[row*n + c];
      double x = 0.0;
#pragma unroll
      for (int k=0; k<RANK; k++)
      {
         const double uk = U[k*m + row], vk = V[k*m + row];
         x += uk * S[k] + vk * P[k];
         P[k] += uk * g; S[k] -= vk * g;
      }
      buf[row*n + c] = (real) x;
   }
}
template <typename real, typename PT>
__device__ __forceinline__ void semisep_scan_column_any(PT buf, int m, int n, int c, int rank, const double * U, const double * V)
{
   const int rpl = (m + 63) >> 6;
   if (rpl <= 4)
      switch (rank)
      {
      case 2: semisep_scan_column<real, 2, true>(buf, m, n, c, rpl, U, V); break;
      case 3: semisep_scan_column<real, 3, true>(buf, m, n, c, rpl, U, V); break;
      default: semisep_scan_column<real, 4, true>(buf, m, n, c, rpl, U, V); break;
      }
   else
      switch (rank)
      {
      case 2: semisep_scan_column<real, 2, false>(buf, m, n, c, rpl, U, V); break;
      case 3: semisep_scan_column<real, 3, false>(buf, m, n, c, rpl, U, V); break;
      default: semisep_scan_column<real, 4, false>(buf, m, n, c, rpl, U, V); break;
      }
}
// all n columns of buf [m][n] in place, a wavefront per column at a time: ONE barrier, like the scan solve of derivative 1.
// A column that is zero throughout (the joint-limit rounds solve for a Gjlimit with a few non-zero columns) is left alone.
template <typename real, int BLOCK>
__device__ __attribute__((noinline)) real * semisep_solve_call(real * buf_in, const real * tab_in, int m_in, int n_in, int rank_in, int tid)
{
   // (a function of its own: six instantiations of the column solve, of no interest to a `derivative 1` run's instruction cache)
   const int m = __builtin_amdgcn_readfirstlane(m_in), n = __builtin_amdgcn_readfirstlane(n_in), rank = __builtin_amdgcn_readfirstlane(rank_in);
   real * buf = uniform_ptr(buf_in);
   const real * tab = uniform_ptr(tab_in);
   const int lane = tid & 63, wave = tid >> 6;
   const int rpl = (m + 63) >> 6;
   const double * U = (const double *) tab, * V = U + rank*m;      // (the metric's tables: DevBatch::ss_rank)
   for (int c=wave; c<n; c+=BLOCK/64)
   {
      bool any = false;
      for (int r=0; r<rpl; r++) { const int row = lane*rpl + r; any = any || ((row < m) && buf[row*n + c] != (real)0); }
      if (__ballot(any) == 0ull) continue;
      semisep_scan_column_any<real>(buf, m, n, c, rank, U, V);
   }
   __syncthreads();
   return buf;
}

template <typename real, int BLOCK, typename BT>
__device__ __forceinline__ real * metric_solve(const BT & b, const real * tab, real * src, real * tmp, int tid)
{
   if (b.solve_mode == 2) return toeplitz_scan_solve<real, BLOCK>(b, src, tid);
   if (b.solve_mode == 3) return semisep_solve_call<real, BLOCK>(src, tab, b.m, b.n, b.ss_rank, tid);
   return b.solve_mode == 0 ? pcr_solve<real, BLOCK>(b, tab, src, tmp, tid) : dense_solve<real, BLOCK>(b, src, tmp, tid);
}
