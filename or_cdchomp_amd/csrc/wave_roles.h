// wave_roles.h -- which wavefront of a workgroup does what in the iterate kernel.  No HIP in here: the host tests include it.
//
// The phases of chomp_iterate_kernel hand out their work by a LOGICAL thread index: the hardware index rotated by whole
// wavefronts, (threadIdx.x + 64 rot) mod BLOCK.  The lane within the wavefront is the hardware's (DPP, ds_bpermute, __shfl and
// v_readlane code never sees the rotation); `rot` is wave-uniform.  Everything a run computes is a function of the logical index
// alone -- the partial sums of the wavefronts are added in logical order (sum_partials) -- so every rotation gives the same bits.
//
// The work that does not fill a workgroup is dealt from both ends: the partial cost rounds, the joint-limit rounds and the
// single-thread bookkeeping go to the FIRST logical wavefronts (they always did), the FK groups to the LAST ones.  For the
// headline plan (256 threads, tiles of 50 + 48: FK of 52 and 50 rows = three groups of 20, cost rounds 16 16 16 2 | 16 16 16)
// wavefront 0 makes 7 cost passes and the limit rounds, wavefronts 1..3 make 2 FK walks and 6 cost passes each; with the FK
// groups on the first wavefronts, wavefront 0 carried 1.2 times the mean of the vector instructions and wavefront 3 0.8 times.
#pragma once

#if defined(__HIPCC__)
#define ORC_WR_FN __host__ __device__ inline
#else
#define ORC_WR_FN inline
#endif

// the iteration's low three bits travel to the phase functions in bits 24..26 of an integer argument (chomp_kernel.hip pack_it):
// the arguments that carry them (a tile's end <= m, the resample slot < max_resamples, a flag) must stay below 2^24
#define ORC_IT_SHIFT 24

namespace orc {

// ORC_WAVE_ROTATE (Switches::wave_rotate, DevBatch::wave_rotate): where `rot` comes from
//   0 none; 1 the workgroup index (bits 8..: workgroups 256 apart share a CU when the grid's first wave of workgroups is placed);
//   2 the workgroup index plus the iteration number
constexpr int WAVE_ROTATE_MAX = 2;

// the rotation of a workgroup in an iteration (`it_bits`: the low three bits of the iteration number), in wavefronts
ORC_WR_FN int wave_rot(int mode, int block_idx, int it_bits, int block)
{
   if (mode <= 0) return 0;
   const int waves = block >> 6;
   const int v = ((block_idx >> 8) & 7) + ((mode >= 2) ? (it_bits & 7) : 0);      // 0 .. 14
   return (waves & (waves - 1)) ? v % waves : (v & (waves - 1));
}

// the logical index of hardware thread `hw` (0 <= hw < block, 0 <= rot < block/64; block a multiple of 64)
ORC_WR_FN int logical_tid(int hw, int rot, int block)
{
   const int t = hw + (rot << 6);
   if ((block & (block - 1)) == 0) return t & (block - 1);
   return (t >= block) ? t - block : t;
}

// FK: a group of 20 waypoints is walked by one wavefront (nseg == 1) or by a pair of neighbouring wavefronts (nseg == 2, a chain
// that then branches: DevModel::fk_split); `waves / nseg` groups are walked per round.  Group g of a round goes to the last
// wavefronts: logical wavefront (or pair) waves/nseg - 1 - g.
ORC_WR_FN int fk_groups(int block, int nseg) { return (block >> 6) / nseg; }
ORC_WR_FN int fk_group_of_wave(int lwave, int block, int nseg) { return fk_groups(block, nseg) - 1 - lwave / nseg; }
ORC_WR_FN int fk_seg_of_wave(int lwave, int nseg) { return (nseg == 2) ? (lwave & 1) : 0; }
// a wavefront that has no waypoint among the `nfk` of a tile in any round (it only meets the phase's barrier)
ORC_WR_FN bool fk_wave_idle(int lwave, int block, int nseg, int nfk) { return fk_group_of_wave(lwave, block, nseg) * 20 >= nfk; }

} // namespace orc
