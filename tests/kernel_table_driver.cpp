// kernel_table_driver.cpp -- every plan of plan_iterate names a kernel the library holds, at an occupancy the kernel's registers allow.
// Built and run by tests/test_kernel_table.py with a host compiler (csrc/plan.cpp + this file; no GPU, no HIP).
//
// The grid: every variant mask the fold can emit (robot_variant over the robot's facts, scene_variant over the scenes' two) in both
// precisions x threads asked for {0, 128, 192, 256, 512} x workgroups per CU asked for {0, 3, 4} x overlapping launches x TSR
// constraints x a free start x trajectory lengths x the planner's switches.  What the fold rules out is left out the same way
// (choose_lanes, fold.cpp: no pair list with a free start, under ORC_BLOCK_THREADS, or for 128 / 192 threads asked for).
// An input refused with "does not fit the LDS" is passed over; so that this hides nothing, every cell (variant, precision, threads
// asked for, per CU asked for, constrained) has to hold at least one input that plans.
#include "stages.h"
#include "kernel_table.h"
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <stdexcept>
#include <tuple>

using namespace orc;

namespace {

struct Facts { bool tree; int GS; bool floating; int nj; bool pairs; int variant; };

// the robots: one set of facts per distinct variant mask of robot_variant
std::vector<Facts> robots()
{
   std::vector<Facts> out;
   std::set<int> seen;
   for (int tree=0; tree<2; tree++) for (int GS : { 8, 16, 32, 64 }) for (int floating=0; floating<2; floating++)
   for (int jt_scan=0; jt_scan<3; jt_scan++) for (int placed=0; placed<2; placed++) for (int nj : { 7, 20 }) for (int no_kind=0; no_kind<2; no_kind++)
   for (int pairs=0; pairs<2; pairs++)
   {
      if (placed && GS != 16) continue;                                             // (choose_lanes places spheres on a 16-lane row only)
      if (pairs && !(GS == 32 && jt_scan == (tree ? 2 : 1) && !no_kind)) continue;   // (choose_lanes: who takes the pair list)
      const int variant = robot_variant(tree, GS, floating, jt_scan, placed, nj, pairs, no_kind);
      if (seen.insert(variant).second) out.push_back({ tree != 0, GS, floating != 0, nj, pairs != 0, variant });
   }
   return out;
}

struct Setting { const char * name; int value; };      // one planner switch set (value < 0: none)

Switches switches_of(const Setting & s)
{
   Switches sw;
   Switches::Int * which = !strcmp(s.name, "ORC_WGS") ? &sw.wgs : !strcmp(s.name, "ORC_BLOCK_THREADS") ? &sw.block_threads : !strcmp(s.name, "ORC_TILE_M") ? &sw.tile_m : nullptr;
   if (which) { which->set = true; which->value = s.value; }
   if (!strcmp(s.name, "ORC_WGS128")) sw.wgs128 = s.value;
   return sw;
}

} // namespace

int main()
{
   // ORC_WGS and ORC_WGS128 within the kernels' register budgets (3 x 256 threads, 8 x 128): an experiment that asks for more
   // residents than the registers allow is what the switch is for, not a planner fault
   const Setting settings[] = { { "", -1 }, { "ORC_WGS", 1 }, { "ORC_WGS", 2 }, { "ORC_WGS", 3 }, { "ORC_BLOCK_THREADS", 128 }, { "ORC_BLOCK_THREADS", 192 },
      { "ORC_BLOCK_THREADS", 256 }, { "ORC_BLOCK_THREADS", 512 }, { "ORC_WGS128", 4 }, { "ORC_WGS128", 6 }, { "ORC_TILE_M", 8 }, { "ORC_TILE_M", 33 } };
   // 1 .. 98: the bench's lengths and the short-trajectory shapes; 400: several tiles; 1500, 4000: G and the trajectory leave the LDS
   const int lengths[] = { 1, 8, 32, 50, 98, 400, 1500, 4000 };
   long plans = 0, refused = 0, failures = 0, lds_above_registers = 0;
   std::set<int> reached;
   std::map<std::tuple<int, int, int, int, int>, long> cells;

   for (const Facts & r : robots())
   for (int scene=0; scene<3; scene++)                // several fields | one aligned field, inactive spheres left | ... none left
   for (int bytes : { 8, 4 })
   for (int asked : { 0, 128, 192, 256, 512 })
   for (int per_cu : { 0, 3, 4 })
   for (int overlapping=0; overlapping<2; overlapping++)
   for (int tsrs=0; tsrs<2; tsrs++)
   for (int free_start=0; free_start<2; free_start++)
   {
      if (r.pairs && (free_start || asked == 128 || asked == 192)) continue;
      PlanInput in;
      in.variant = scene_variant(r.variant, scene >= 1, scene == 2);
      if (scene >= 1 && in.variant == r.variant) continue;      // (the scenes' bits do not reach this family: one pass over it)
      in.GS = r.GS; in.nj = r.nj; in.n = r.nj + (r.floating ? 7 : 0);
      in.Sa = (r.GS == 16) ? ((in.variant & ORC_VAR_KIND) ? 16 : 12) : (r.GS * 3) / 4;
      in.S = in.Sa + (scene == 2 ? 0 : 4);
      in.n_sdfs = (scene >= 1) ? 1 : 2;
      in.pair_entries = r.pairs ? 8 * r.GS : 0;
      in.real_bytes = (size_t) bytes; in.sdf_bytes = (bytes == 8) ? sizeof(DevSdf<double>) : sizeof(DevSdf<float>);
      in.n_tsrs = tsrs; in.tsr_kmax = tsrs ? 6 : 0; in.free_start = free_start; in.derivative = 1;
      in.overlapping = overlapping != 0; in.module_threads = asked; in.module_per_cu = per_cu;
      const auto cell = std::make_tuple(in.variant, bytes, asked, per_cu, tsrs | free_start);
      cells[cell] += 0;
      for (int m : lengths)
      for (const Setting & s : settings)
      {
         if (r.pairs && !strcmp(s.name, "ORC_BLOCK_THREADS")) continue;
         in.m = m;
         // a free start has no Toeplitz metric: cyclic reduction with its compact table (pack_metric); else the closed-form scan solve
         in.solve_mode = free_start ? 0 : 2;
         in.pcr_rows = 0;
         if (free_start) { int levels = 0; while ((1 << levels) < m) levels++; in.pcr_rows = levels + 1; }
         IteratePlan P;
         try { P = plan_iterate(in, switches_of(s)); }
         catch (const std::runtime_error & e)
         {
            if (!strstr(e.what(), "does not fit the LDS")) { printf("FAIL unexpected error: %s\n", e.what()); failures++; }
            refused++;
            continue;
         }
         plans++; cells[cell]++;
         const KernelKey k = kernel_of(P.variant, P.block, bytes);
         bool bad = !kernel_exists(k);
         for (int i=0; i<N_ITERATE_KERNELS && !bad; i++) if (ITERATE_KERNELS[i] == k) reached.insert(i);
         // the plan sized its share of the LDS for P.per_cu resident workgroups: the row's registers must hold as many
         if (!bad && workgroups_per_cu(k) < P.per_cu) bad = true;
         if (!bad && workgroups_per_cu(k) < P.workgroups_per_cu()) lds_above_registers++;
         if (bad && failures++ < 40)
            printf("FAIL variant %d fp%d asked %d per_cu %d overlapping %d tsrs %d free_start %d m %d %s=%d: plan variant %d block %d sized for %d per CU -> <%d,%d,%d,%d,%d,%d> %s\n",
               in.variant, bytes * 8, asked, per_cu, overlapping, tsrs, free_start, m, s.name, s.value, P.variant, P.block, P.per_cu,
               k.real_bytes, k.tree, k.gs16, k.block, k.kind, k.wgs, kernel_exists(k) ? "allows fewer" : "is no kernel");
      }
   }
   long empty = 0;
   for (const auto & c : cells)
      if (c.second == 0 && empty++ < 40)
         printf("FAIL empty cell: variant %d fp%d asked %d per_cu %d constrained %d\n", std::get<0>(c.first), std::get<1>(c.first) * 8, std::get<2>(c.first), std::get<3>(c.first), std::get<4>(c.first));
   for (int i=0; i<N_ITERATE_KERNELS; i++)
      if (!reached.count(i))
      {
         const KernelKey & k = ITERATE_KERNELS[i];
         printf("unreached <%s, %d, %d, %d, %d, %d>\n", k.real_bytes == 8 ? "double" : "float", k.tree, k.gs16, k.block, k.kind, k.wgs);
      }
   printf("plans %ld refused %ld cells %zu empty %ld rows %d reached %zu failures %ld lds_above_registers %ld\n",
      plans, refused, cells.size(), empty, N_ITERATE_KERNELS, reached.size(), failures, lds_above_registers);
   return (failures || empty) ? 1 : 0;
}
