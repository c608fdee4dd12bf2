// wave_roles_driver.cpp -- csrc/wave_roles.h on the host (tests/test_wave_roles_host.py): the logical thread index is a permutation
// that moves whole wavefronts and keeps the lane, the rotation stays inside the workgroup, and the FK phase's hand-out of waypoint
// groups to the LAST wavefronts walks every waypoint of a tile exactly once per segment.
#include <cstdio>
#include <vector>
#include "wave_roles.h"

using namespace orc;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } failures++; } } while (0)

int main()
{
   const int blocks[4] = { 128, 192, 256, 512 };
   long mappings = 0, walks = 0;
   for (int block : blocks)
   {
      const int waves = block / 64;
      // the index mapping, every rotation
      for (int rot=0; rot<waves; rot++)
      {
         std::vector<int> seen(block, 0), wave_of(waves, -1);
         for (int hw=0; hw<block; hw++)
         {
            const int t = logical_tid(hw, rot, block);
            CHECK(t >= 0 && t < block, "block %d rot %d hw %d -> %d", block, rot, hw, t);
            if (t < 0 || t >= block) continue;
            seen[t]++;
            CHECK((t & 63) == (hw & 63), "block %d rot %d hw %d -> %d: the lane moved", block, rot, hw, t);
            if (wave_of[hw >> 6] < 0) wave_of[hw >> 6] = t >> 6;
            CHECK(wave_of[hw >> 6] == (t >> 6), "block %d rot %d hw %d -> %d: a wavefront was split", block, rot, hw, t);
            CHECK((t >> 6) == ((hw >> 6) + rot) % waves, "block %d rot %d hw %d -> %d: not the rotation", block, rot, hw, t);
            mappings++;
         }
         for (int t=0; t<block; t++) CHECK(seen[t] == 1, "block %d rot %d: logical index %d taken %d times", block, rot, t, seen[t]);
      }
      CHECK(logical_tid(block - 1, 0, block) == block - 1 && logical_tid(0, 0, block) == 0, "block %d: rot 0 is not the identity", block);
      // the rotation of a workgroup in an iteration
      for (int mode=0; mode<=WAVE_ROTATE_MAX; mode++)
         for (int wg=0; wg<8192; wg++)
            for (int it=0; it<8; it++)
            {
               const int rot = wave_rot(mode, wg, it, block);
               CHECK(rot >= 0 && rot < waves, "block %d mode %d workgroup %d iteration %d: rot %d", block, mode, wg, it, rot);
               if (mode == 0) CHECK(rot == 0, "mode 0 rotates");
               if (mode == 1) CHECK(rot == wave_rot(1, wg, 0, block), "mode 1 reads the iteration");
            }
      // workgroups 256 apart (the ones that share a CU in the grid's first wave) get distinct rotations, as many as there are
      for (int wg=0; wg<256; wg++)
         for (int k=1; k<waves && k<8; k++)
            CHECK(wave_rot(1, wg, 0, block) != wave_rot(1, wg + 256*k, 0, block), "block %d: workgroups %d and %d rotate alike", block, wg, wg + 256*k);
      // ... and a workgroup walks through all of them with the iterations
      for (int it=0; it+1<8; it++)
         CHECK(wave_rot(2, 0, it + 1, block) == (wave_rot(2, 0, it, block) + 1) % waves, "block %d: mode 2 does not step with the iteration", block);

      // the FK hand-out (phase_fk_body's loop, restated): nfk waypoints, `groups` groups of 20 per round
      for (int nseg=1; nseg<=2; nseg++)
      {
         if (nseg == 2 && waves % 2) continue;
         const int groups = fk_groups(block, nseg);
         CHECK(groups * nseg == waves, "block %d nseg %d: %d groups", block, nseg, groups);
         CHECK(fk_group_of_wave(waves - 1, block, nseg) == 0, "block %d nseg %d: group 0 is not on the last wavefront", block, nseg);
         for (int nfk=1; nfk<=4*20*waves; nfk++)
         {
            std::vector<int> walked(2 * nfk, 0);
            for (int lw=0; lw<waves; lw++)
            {
               const int group = fk_group_of_wave(lw, block, nseg), seg = fk_seg_of_wave(lw, nseg);
               CHECK(group >= 0 && group < groups && seg >= 0 && seg < nseg, "block %d nseg %d wave %d: group %d seg %d", block, nseg, lw, group, seg);
               int mine = 0;
               for (int w0=0; w0<nfk; w0+=groups*20)
               {
                  if (w0 + group * 20 >= nfk) continue;
                  for (int k=0; k<20; k++)
                  {
                     const int w = w0 + group * 20 + k;
                     if (w < nfk) { walked[2*w + seg]++; mine++; }
                  }
               }
               CHECK(fk_wave_idle(lw, block, nseg, nfk) == (mine == 0), "block %d nseg %d nfk %d wave %d: idle %d, walked %d", block, nseg, nfk, lw,
                     (int) fk_wave_idle(lw, block, nseg, nfk), mine);
               // the wavefronts with work are the last ones: no idle wavefront after a busy one
               if (lw + nseg < waves && mine > 0)
                  CHECK(!fk_wave_idle(lw + nseg, block, nseg, nfk), "block %d nseg %d nfk %d: wave %d walks, wave %d idles", block, nseg, nfk, lw, lw + nseg);
            }
            for (int w=0; w<nfk; w++)
               for (int seg=0; seg<nseg; seg++)
                  CHECK(walked[2*w + seg] == 1, "block %d nseg %d nfk %d: waypoint %d segment %d walked %d times", block, nseg, nfk, w, seg, walked[2*w + seg]);
            walks++;
         }
      }
   }
   // the headline: 256 threads, FK of 52 and 50 rows -- wavefront 0 idles in both, 1..3 walk 12 / 20 / 20 and 10 / 20 / 20
   CHECK(fk_wave_idle(0, 256, 1, 52) && fk_wave_idle(0, 256, 1, 50) && !fk_wave_idle(1, 256, 1, 50), "the headline's FK roles");
   std::printf("mappings %ld walks %ld failures %d\n", mappings, walks, failures);
   return failures ? 1 : 0;
}
