// limit_rounds.h -- the joint-limit projection rounds of the CHOMP iteration (src/libcd/chomp.c:608-655), by ONE wavefront: the
// rounds through G in LDS (limit_rounds_wave_with, for either metric's column solve), the register forms of limit_regs.h behind
// their dispatch by columns and rows per lane, and the four functions the update phase calls (limit_rounds_call*).
//
// Included by chomp_kernel.hip inside its namespace, after metric_solve.h (the column solves).
#pragma once

// Joint-limit projection rounds (src/libcd/chomp.c:608-655) for the tridiagonal Toeplitz metric,
// executed by ONE wavefront (the caller's; the others wait at the barrier that follows): a round has
// no barrier in it.  Lane = `rpl` consecutive waypoints, loop over the columns.  A round is:
// violations of every entry -> Gjlimit in G (dense) and the largest violation (wave arg-max, ties
// to the first row-major index) -> GA = A^-1 Gjlimit by the scan solve, only for the columns that
// have a violation -> T += 1.01 Gjlimit[l]/GA[l] * GA on those columns.
// Returns the number of rounds made (1000: the caller sets the status).
// SOLVE: solve_col(c) replaces column c of G_s by A^-1 of it (the calling wavefront's work)
template <typename real, typename PT, typename PG, typename PJ, typename SOLVE>
__device__ __forceinline__ int limit_rounds_wave_with(PT T_s, PG G_s, PJ jl_s, int m, int n, SOLVE solve_col, long long * dbg_total)
{
   const int lane = threadIdx.x & 63;
   const int rpl = (m + 63) >> 6;
   const float rn = 1.0f / (float) n;
   const int mn = m*n;
   int rounds;
   for (rounds=0; rounds<1000; rounds++)
   {
      // violations of all entries, in row-major order (lane + 64 k): Gjlimit, the largest one
      // (first index on ties) and the set of columns that have one
      real best = 0; int best_e = 0x7fffffff;
      unsigned long long mycols = 0ull;
      // four entries of the lane per trip: their reads and short dependent chains overlap (one entry
      // per trip pays the full latency of each)
#pragma unroll 1
      for (int e0=lane; e0<mn; e0+=4*64)
      {
         real gk[4]; int ck[4];
#pragma unroll
         for (int k=0; k<4; k++)
         {
            const int e = e0 + 64*k;
            const bool ok = (e < mn);
            const int i = div_n(ok ? e : 0, rn), c = (ok ? e : 0) - i*n;
            const real t = ok ? T_s[n + e] : (real)0;
            const real lo = jl_s[c], hi = jl_s[n+c];
            // lo - t when below, hi - t when above, else 0 (at most one of the two terms is non-zero)
            real g = M<real>::max_(lo - t, (real)0) + M<real>::min_(hi - t, (real)0);
            g = ok ? g : (real)0;
            if (ok) G_s[e] = g;
            gk[k] = g; ck[k] = c;
         }
         // arg-max of the four, then against the running one: a later entry wins only when strictly larger
         const real a0 = M<real>::fabs_(gk[0]), a1 = M<real>::fabs_(gk[1]), a2 = M<real>::fabs_(gk[2]), a3 = M<real>::fabs_(gk[3]);
         const bool l01 = (a1 > a0), l23 = (a3 > a2);
         const real a01 = l01 ? a1 : a0, a23 = l23 ? a3 : a2;
         const int e01 = l01 ? e0 + 64 : e0, e23 = l23 ? e0 + 192 : e0 + 128;
         const bool l2 = (a23 > a01);
         const real a4 = l2 ? a23 : a01; const int e4 = l2 ? e23 : e01;
         const bool better = (a4 > best);
         best = better ? a4 : best;
         best_e = better ? e4 : best_e;
#pragma unroll
         for (int k=0; k<4; k++) mycols |= (gk[k] != (real)0) ? (1ull << ck[k]) : 0ull;
      }
      wave_argmax(best, best_e);
      if (!(best > (real)0)) break;                   // nothing violated
      // columns with a violated entry: OR of the lanes' masks (DPP inside the rows, then the four rows)
      unsigned int clo = (unsigned int) mycols, chi = (unsigned int)(mycols >> 32);
      clo |= (unsigned int) dpp_move<0xB1>((int) clo); chi |= (unsigned int) dpp_move<0xB1>((int) chi);     // quad_perm [1,0,3,2]
      clo |= (unsigned int) dpp_move<0x4E>((int) clo); chi |= (unsigned int) dpp_move<0x4E>((int) chi);     // quad_perm [2,3,0,1]
      clo |= (unsigned int) dpp_move<0x141>((int) clo); chi |= (unsigned int) dpp_move<0x141>((int) chi);   // row_half_mirror
      clo |= (unsigned int) dpp_move<0x140>((int) clo); chi |= (unsigned int) dpp_move<0x140>((int) chi);   // row_mirror
      const unsigned int lo32 = __builtin_amdgcn_readlane((int) clo, 0) | __builtin_amdgcn_readlane((int) clo, 16)
                              | __builtin_amdgcn_readlane((int) clo, 32) | __builtin_amdgcn_readlane((int) clo, 48);
      const unsigned int hi32 = __builtin_amdgcn_readlane((int) chi, 0) | __builtin_amdgcn_readlane((int) chi, 16)
                              | __builtin_amdgcn_readlane((int) chi, 32) | __builtin_amdgcn_readlane((int) chi, 48);
      const unsigned long long cols = ((unsigned long long) hi32 << 32) | lo32;      // wave-uniform
      const int ge = best_e;
      const int gi = div_n(ge, rn), gc = ge - gi*n;
      const real gl = G_s[ge];                        // Gjlimit[largest]
      if (dbg_total) *dbg_total += __popcll(cols);
      for (int c=0; c<n; c++)
         if ((cols >> c) & 1ull) solve_col(c);
      const real sc = ((real)1.01 * gl) * rcp_fast(G_s[gi*n + gc]);
      for (int c=0; c<n; c++)
         if ((cols >> c) & 1ull)
         {
            for (int r=0; r<rpl; r++)      // (any number of rows per lane: trajectories of more than 256 moving waypoints come here)
            {
               const int row = lane*rpl + r;
               if (row < m) T_s[n + row*n + c] += sc * G_s[row*n + c];
            }
         }
   }
   return rounds;
}
template <typename real, typename PT, typename PG, typename PJ>
__device__ __forceinline__ int limit_rounds_wave(PT T_s, PG G_s, PJ jl_s, int m, int n, real kinv, long long * dbg_total)
{
   const int rpl = (m + 63) >> 6;
   (void) rpl;
   return limit_rounds_wave_with<real>(T_s, G_s, jl_s, m, n, [&](int c) { toeplitz_scan_column_any<real>(G_s, m, n, c, kinv); }, dbg_total);
}
// ... and for the band metric of a higher derivative (solve_mode 3): the same rounds with the band inverse applied through its
// generators, one wavefront, no barrier inside (m <= 64 ORC_SCAN_RPL: the lane's rows in registers).  A function of its own,
// like limit_rounds_call: rare, branchy code that should not take part in the update phase's register allocation.
template <typename real, int SHAPE>
__device__ __attribute__((noinline)) int limit_rounds_semisep_call(real * T_gen, real * G_gen, const real * jl_gen, int m_in, int n_in, int rank_in,
   const double * U_in, const double * V_in)
{
   const int m = __builtin_amdgcn_readfirstlane(m_in), n = __builtin_amdgcn_readfirstlane(n_in), rank = __builtin_amdgcn_readfirstlane(rank_in);
   const double * U = uniform_ptr(U_in), * V = uniform_ptr(V_in);
   return limit_rounds_wave_with<real>(T_gen, G_gen, jl_gen, m, n, [&](int c) { semisep_scan_column_any<real>(G_gen, m, n, c, rank, U, V); }, nullptr);
}


#include "limit_regs.h"
// (A forwarding level of its own, on purpose: with the two folded into one function the rounds inline one level less deep, and the
// compiled limit_rounds_call* functions come out different -- other registers, another schedule.  To be folded by a change that is
// timed on the card anyway.)
template <typename real, int NC, int RPL, typename PT, typename PJ>
__device__ __forceinline__ int limit_rounds_regs(PT T_s, PJ jl_s, int m, int n, real kinv, unsigned long long cols, long long * dbg)
{
   return limit_rounds_regs_masks<real, NC, RPL>(T_s, jl_s, m, n, kinv, cols, dbg);
}
template <typename real, int NC, typename PT, typename PJ>
__device__ __forceinline__ int limit_rounds_regs_rpl(PT T_s, PJ jl_s, int m, int n, real kinv, unsigned long long cols, long long * dbg)
{
   const int rpl = (m + 63) >> 6;
   switch (rpl)
   {
   case 1: return limit_rounds_regs<real, NC, 1>(T_s, jl_s, m, n, kinv, cols, dbg);
   case 2: return limit_rounds_regs<real, NC, 2>(T_s, jl_s, m, n, kinv, cols, dbg);
   case 3: return limit_rounds_regs<real, NC, 3>(T_s, jl_s, m, n, kinv, cols, dbg);
   default: return limit_rounds_regs<real, NC, 4>(T_s, jl_s, m, n, kinv, cols, dbg);
   }
}

// The joint-limit rounds of one iteration as a FUNCTION CALL of the wavefront that makes them: the
// rounds are long, rare, branchy code with a register appetite of their own; inlined into the
// iterate kernel they take part in its register allocation and cost the cost phase its registers
// (measured: +6 % kernel time when the variants for 4..8 columns were added inline).  One copy per
// precision serves every kernel variant.  T_s / G_s / jl_s are LDS addresses.
struct LimResult { int rounds; long long kinds; };      // kinds: closed-form | register scans << 20 | general loop << 40

// PART: 1 one or two columns only; 2 three columns and more.  The rounds of one or two columns are a function of their own: its
// register appetite, and with it the callee-saved registers a call saves and restores, is a third of the large cases'
template <typename real, int PART, typename PT>
__device__ __forceinline__ LimResult limit_rounds_body(PT T_s, real * G_gen, const real * jl_gen, int m_in, int n_in, real kinv_in,
   unsigned long long viol_cols_in)
{
   // arguments arrive in vector registers: tell the compiler they are wave-uniform
   const int m = __builtin_amdgcn_readfirstlane(m_in), n = __builtin_amdgcn_readfirstlane(n_in);
   const real kinv = unir(kinv_in);
   const unsigned long long viol_cols = uni64(viol_cols_in);
   typedef __attribute__((address_space(3))) real * lds_ptr;
   typedef const __attribute__((address_space(3))) real * lds_cptr;
   lds_ptr G_s = (lds_ptr) G_gen; lds_cptr jl_s = (lds_cptr) jl_gen;
   LimResult res; res.rounds = 0; res.kinds = 0;
   long long * dg = &res.kinds;
   const int nc = __popcll(viol_cols);
   if (m > 64*ORC_SCAN_RPL)
   {
      // more than 256 moving waypoints: the register forms hold at most four rows per lane; the rounds through G in LDS (still one
      // wavefront, no barrier inside a round; until round 6 such runs took the workgroup loop with a cyclic-reduction solve per round)
      res.rounds = limit_rounds_wave<real>(T_s, G_s, jl_s, m, n, kinv, nullptr);
      res.kinds += (long long) res.rounds << 40;
      return res;
   }
   if (PART == 1)
   {
      if (nc == 1) res.rounds = limit_rounds_regs_rpl<real, 1>(T_s, jl_s, m, n, kinv, viol_cols, dg);
      else res.rounds = limit_rounds_regs_rpl<real, 2>(T_s, jl_s, m, n, kinv, viol_cols, dg);
      return res;
   }
   switch (nc)
   {
   case 1: case 2: break;      // (PART 2 is never called with one or two)
   case 3: res.rounds = limit_rounds_regs_rpl<real, 3>(T_s, jl_s, m, n, kinv, viol_cols, dg); break;
   default:
      // four to eight columns (a trajectory that is leaving its limits for good, the 1000-round
      // aborts among them): still register-resident when a lane holds at most two waypoints
      if (m <= 128 && nc <= 8)
      {
         switch (nc)
         {
         case 4: res.rounds = limit_rounds_regs<real, 4, 2>(T_s, jl_s, m, n, kinv, viol_cols, dg); break;
         case 5: res.rounds = limit_rounds_regs<real, 5, 2>(T_s, jl_s, m, n, kinv, viol_cols, dg); break;
         case 6: res.rounds = limit_rounds_regs<real, 6, 2>(T_s, jl_s, m, n, kinv, viol_cols, dg); break;
         case 7: res.rounds = limit_rounds_regs<real, 7, 2>(T_s, jl_s, m, n, kinv, viol_cols, dg); break;
         default: res.rounds = limit_rounds_regs<real, 8, 2>(T_s, jl_s, m, n, kinv, viol_cols, dg); break;
         }
         break;
      }
      if (m <= 256 && nc <= 7)      // 200-waypoint runs (BASELINE configs[3]: seven arm columns can leave their limits)
      {
         switch (nc)
         {
         case 4: res.rounds = limit_rounds_regs<real, 4, 4>(T_s, jl_s, m, n, kinv, viol_cols, dg); break;
         case 5: res.rounds = limit_rounds_regs<real, 5, 4>(T_s, jl_s, m, n, kinv, viol_cols, dg); break;
         case 6: res.rounds = limit_rounds_regs<real, 6, 4>(T_s, jl_s, m, n, kinv, viol_cols, dg); break;
         default: res.rounds = limit_rounds_regs<real, 7, 4>(T_s, jl_s, m, n, kinv, viol_cols, dg); break;
         }
         break;
      }
      res.rounds = limit_rounds_wave<real>(T_s, G_s, jl_s, m, n, kinv, nullptr);
      res.kinds += (long long) res.rounds << 40;
      break;
   }
   return res;
}
// the trajectory in LDS (every kernel but the large-robot plans that leave it in global memory)
template <typename real, int SHAPE>      // SHAPE: a copy per register budget of the calling kernels (the budget follows the callers')
__device__ __attribute__((noinline)) LimResult limit_rounds_call(real * T_gen, real * G_gen, const real * jl_gen, int m, int n, real kinv,
   unsigned long long viol_cols)
{
   typedef __attribute__((address_space(3))) real * lds_ptr;
   return limit_rounds_body<real, 2>((lds_ptr) T_gen, G_gen, jl_gen, m, n, kinv, viol_cols);
}
template <typename real, int SHAPE>
__device__ __attribute__((noinline)) LimResult limit_rounds_call_global(real * T_gen, real * G_gen, const real * jl_gen, int m, int n, real kinv,
   unsigned long long viol_cols)
{
   return limit_rounds_body<real, 2>(T_gen, G_gen, jl_gen, m, n, kinv, viol_cols);
}
// ... and the same for one or two columns (nearly every call of a 7-dof arm)
template <typename real, int SHAPE>
__device__ __attribute__((noinline)) LimResult limit_rounds_call_small(real * T_gen, real * G_gen, const real * jl_gen, int m, int n, real kinv,
   unsigned long long viol_cols)
{
   typedef __attribute__((address_space(3))) real * lds_ptr;
   return limit_rounds_body<real, 1>((lds_ptr) T_gen, G_gen, jl_gen, m, n, kinv, viol_cols);
}
template <typename real, int SHAPE>
__device__ __attribute__((noinline)) LimResult limit_rounds_call_global_small(real * T_gen, real * G_gen, const real * jl_gen, int m, int n, real kinv,
   unsigned long long viol_cols)
{
   return limit_rounds_body<real, 1>(T_gen, G_gen, jl_gen, m, n, kinv, viol_cols);
}
