// wave.h -- lane and wavefront primitives of the gfx950 kernels (64 lanes), one definition each: DPP moves, sums, minima,
// arg-max and scans over the lanes, reads of another lane, and the way back into scalar registers for a wave-uniform value.
//
// Included inside the including file's anonymous namespace (like sdf_lookup.h, and after it where it is there), by every kernel
// file that uses one of them: chomp_kernel.hip and its headers, clearance_kernels.hip, config_kernels.hip and
// penetration_kernels.hip (config_query.h's minima), multistart_kernels.hip.  The contraction pragma in force is the
// including file's.  Nothing here touches memory: LDS scratch, where a function needs it, is the caller's.
#pragma once

// v of the lane that the DPP control CTRL names, 0 where it names none (inside a row of 16 lanes: no LDS pipe)
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v)
{
   int lo = __double2loint(v), hi = __double2hiint(v);
   lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
   hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
   return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ float dpp_move(float v)
{
   return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_move(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }

// sum over aligned groups of GS lanes (GS a power of two <= 64); every lane of the group
// receives the total.  Up to 16 lanes stay inside a DPP row (no LDS pipe).
template <typename real>
__device__ __forceinline__ real group_sum(real v, int GS)
{
   if (GS >= 2)  v += dpp_move<0xB1>(v);      // quad_perm [1,0,3,2]
   if (GS >= 4)  v += dpp_move<0x4E>(v);      // quad_perm [2,3,0,1]
   if (GS >= 8)  v += dpp_move<0x141>(v);     // row_half_mirror
   if (GS >= 16) v += dpp_move<0x140>(v);     // row_mirror
   if (GS >= 32) v += __shfl_xor(v, 16, 64);
   if (GS >= 64) v += __shfl_xor(v, 32, 64);
   return v;
}

template <typename real>
__device__ __forceinline__ real dpp_row_max(real v)
{
   real o;
   o = dpp_move<0xB1>(v);  v = o > v ? o : v;
   o = dpp_move<0x4E>(v);  v = o > v ? o : v;
   o = dpp_move<0x141>(v); v = o > v ? o : v;
   o = dpp_move<0x140>(v); v = o > v ? o : v;
   return v;
}
// lane ln's v in every lane, ln being wave-uniform: a read through the scalar unit, no LDS round trip as a shuffle makes
__device__ __forceinline__ double read_lane(double v, int ln)
{
   const int lo = __builtin_amdgcn_readlane(__double2loint(v), ln), hi = __builtin_amdgcn_readlane(__double2hiint(v), ln);
   return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float read_lane(float v, int ln) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), ln)); }
// value of `v` in the lane whose byte address (lane * 4) is `addr4`, a lane of each lane's own choice: ds_bpermute, no memory behind it
__device__ __forceinline__ double lane_fetch(double v, int addr4)
{
   const int lo = __builtin_amdgcn_ds_bpermute(addr4, __double2loint(v)), hi = __builtin_amdgcn_ds_bpermute(addr4, __double2hiint(v));
   return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float lane_fetch(float v, int addr4) { return __int_as_float(__builtin_amdgcn_ds_bpermute(addr4, __float_as_int(v))); }

// wavefront arg-max of (value >= 0, index), ties to the smallest index; every lane gets the result.
// Row maxima by DPP, rows combined through readlane; the owner is found with a ballot.
template <typename real>
__device__ __forceinline__ void wave_argmax(real & best, int & best_e)
{
   real m = dpp_row_max(best);
   // the four row maxima (lanes 0, 16, 32, 48 hold them after the row reduction)
   const real m0 = read_lane(m, 0), m1 = read_lane(m, 16), m2 = read_lane(m, 32), m3 = read_lane(m, 48);
   const real ma = m0 > m1 ? m0 : m1, mb = m2 > m3 ? m2 : m3;
   const real mm = ma > mb ? ma : mb;
   if (!(mm > (real)0)) { best = 0; best_e = 0x7fffffff; return; }      // nothing to find (wave-uniform)
   unsigned long long cand = __ballot(best == mm);
   int win = 0x7fffffff;
   while (cand)                       // one iteration unless two lanes tie exactly
   {
      const int ln = __builtin_ctzll(cand);
      cand &= cand - 1;
      const int e = __builtin_amdgcn_readlane(best_e, ln);
      win = e < win ? e : win;
   }
   best = mm; best_e = win;
}

// the wavefront's sum / minimum in the butterfly's order (lane distance 32, 16, .. 1): every lane ends with the same bits
template <typename real>
__device__ __forceinline__ real wave_sum(real v)
{
#pragma unroll
   for (int o=32; o>0; o>>=1) v += __shfl_xor(v, o, 64);
   return v;
}
template <typename real> struct M;      // (sdf_lookup.h: the precision's math functions; a file that takes minima includes it)
template <typename real>
__device__ __forceinline__ real wave_min(real x)
{
   for (int d=32; d>=1; d>>=1) x = M<real>::min_(x, __shfl_xor(x, d));
   return x;
}

// the partial sums of a workgroup's wavefronts, added in a fixed pairwise order
template <int BLOCK>
__device__ __forceinline__ double sum_partials(const double * r)
{
   if (BLOCK == 128) return r[0] + r[1];
   if (BLOCK == 192) return (r[0] + r[1]) + r[2];
   if (BLOCK == 256) return (r[0] + r[1]) + (r[2] + r[3]);
   return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));      // 512 threads
}
// sum over the whole workgroup; every thread receives the result.
template <int BLOCK>
__device__ __forceinline__ double block_sum(double v, double * red, int tid)
{
   v = wave_sum(v);
   __syncthreads();
   if ((tid & 63) == 0) red[tid >> 6] = v;
   __syncthreads();
   return sum_partials<BLOCK>(red);
}

// Two pairs of scans over the 64 lanes of a wavefront.  They add the same terms in DIFFERENT ORDERS, so their results differ
// in the last bits and the two are not interchangeable bit for bit: a caller's results are held to the pair it has.
//
// inclusive prefix / suffix sums: Kogge-Stone inside the 16-lane DPP rows (lane distance 1, 2, 4, 8), then the row totals
// through v_readlane, the totals of the rows before (after) this one added among themselves first and to the lane's value last
// (no LDS, no barrier)
template <typename real>
__device__ __forceinline__ real wave_prefix_incl(real v)
{
   v += dpp_move<0x111>(v);      // row_shr:1 (lane i takes lane i-1, 0 before the row)
   v += dpp_move<0x112>(v);
   v += dpp_move<0x114>(v);
   v += dpp_move<0x118>(v);
   const real t0 = read_lane(v, 15), t1 = read_lane(v, 31), t2 = read_lane(v, 47);
   const int row = (threadIdx.x & 63) >> 4;
   real add = (row >= 1) ? t0 : (real)0;
   add += (row >= 2) ? t1 : (real)0;
   add += (row >= 3) ? t2 : (real)0;
   return v + add;
}
// (the suffix sums inside the 16-lane rows alone: lane i ends with the sum over the lanes i .. 15 of its row)
template <typename real>
__device__ __forceinline__ real row_suffix_incl(real v)
{
   v += dpp_move<0x101>(v);      // row_shl:1 (lane i takes lane i+1, 0 past the row)
   v += dpp_move<0x102>(v);      // row_shl:2
   v += dpp_move<0x104>(v);      // row_shl:4
   v += dpp_move<0x108>(v);      // row_shl:8
   return v;
}
template <typename real>
__device__ __forceinline__ real wave_suffix_incl(real v)
{
   v = row_suffix_incl(v);
   const real t1 = read_lane(v, 16), t2 = read_lane(v, 32), t3 = read_lane(v, 48);
   const int row = (threadIdx.x & 63) >> 4;
   real add = (row <= 2) ? t3 : (real)0;
   add += (row <= 1) ? t2 : (real)0;
   add += (row <= 0) ? t1 : (real)0;
   return v + add;
}
// exclusive prefix / suffix sums (the lanes below / above, without the lane's own): Kogge-Stone over all 64 lanes by shuffles
// (lane distance 1, 2, 4, .. 32), then the neighbour's inclusive value
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

// A function that is called (not inlined) receives its arguments in vector registers: loop bounds, base addresses and the
// kernarg block then count as "divergent", loops over them are run by lane masks and their address arithmetic by the vector
// pipe.  These put a wave-uniform value back into scalar registers.  (A 64-bit value through uni64, never by OR-ing
// readfirstlane's low half in as the int it returns: that sign-extends, and an address with bit 31 set turns wild.)
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned long long uni64(unsigned long long v)
{
   const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned) v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
   return ((unsigned long long) hi << 32) | lo;
}
__device__ __forceinline__ double unir(double v) { return __longlong_as_double((long long) uni64((unsigned long long) __double_as_longlong(v))); }
__device__ __forceinline__ float unir(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
template <typename T>
__device__ __forceinline__ T * uniform_ptr(T * p) { return (T *) uni64((unsigned long long) p); }
