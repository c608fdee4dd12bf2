// plan.cpp -- the launch plan of the iterate kernel (stages.h: plan_iterate): workgroup shape, tile size, what lives in LDS.
//
// The kernel is latency bound: resident workgroups per CU (up to the register budget, ORC_WGS_PER_CU) multiply throughput
// almost linearly, every tile costs an FK pass per 64 waypoints and the cost phase rounds of four wavefronts.  Every option
// (workgroups per CU, cyclic-reduction tables in LDS or read through L2, momentum AG in LDS or in global memory, ...) gets
// its largest tile; the one with the best estimated throughput wins.
// The plan is a function of the robot, the run parameters and the module's settings only, never of the batch (a run's bits
// must not depend on what shares its batch): PlanInput has nothing else in it.
#include "stages.h"
#include "kernel_table.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>

namespace orc {

namespace {

const size_t LDS_PER_CU = 160*1024;
// LDS is handed out in 1280-byte granules (measured: three 53512-byte workgroups share a CU, three 54184-byte ones do not)
const size_t LDS_GRANULE = 1280;
// The cycle model (figures measured on the WAM workload and the 30-dof tree, scripts/phase_profile*.py):
const double FK_WAYPOINTS_PER_WAVE = 20.0;     // an FK pass of the workgroup covers 20 waypoints per wavefront (fk.h: triads of lanes)
const double FK_PASS_PER_JOINT = 1.7e3;        // an FK pass costs ~1.7k cycles per joint
const double ROUND_GS16 = 11e3;                // a round of the 16-lane cost phase ~11k
const double ROUND_PAIRS = 9e3;                // ... of the pair-list family
const double ROUND_PER_SPHERE = 350.0;         // ... of the generic one ~350 per active sphere
const double FIXED_PER_ITERATION = 30e3;       // the phases that do not scale with the tiles, at 256 threads
const double PCR_THROUGH_L2 = 1e3, AG_GLOBAL = 2e3, G_GLOBAL = 2e3, T_GLOBAL_STAGED = 4e3, T_GLOBAL_IN_PLACE = 12e3;
const double PER_EXTRA_WAVE = 0.05;            // throughput lost per wavefront per SIMD beyond the first
const double SHAPE_192 = 0.90;                 // four workgroups of three wavefronts measured 7-10 % below three of four at equal wavefronts per SIMD

// workgroup shapes: 256 threads (four wavefronts) at up to three workgroups per CU, or 192 threads
// (three wavefronts) at four per CU: the same twelve wavefronts and register budget, a quarter
// less LDS per run, and the 1024 runs of BASELINE configs[1] resident at once on 256 CUs
struct Shape { int block, wgs; };

// what the switches and the caller force in one pass over the shapes (0 / -1: nothing)
struct Forced { int tile = 0, pcr = -1, ag = -1, g = -1, tl = -1, block = 0; };

// one choice of what lives where
struct Option { int with_pcr, ag_lds, g_lds, t_lds; };

std::vector<Shape> shapes_of(const PlanInput & in, const Switches & sw, int max_wgs, bool budget4, int force_block, bool can128)
{
   auto has = [&in](int block) { return kernel_exists(kernel_of(in.variant, block, (int) in.real_bytes)); };
   std::vector<Shape> shapes;
   for (int wgs=max_wgs; wgs>=(budget4 ? 4 : 1); wgs--) shapes.push_back({ 256, wgs });
   if (max_wgs >= 3 && has(192)) shapes.push_back({ 192, 4 });      // (the pair-list family is built for 256-thread workgroups)
   // a caller that asked for the 192-thread shape gets it for runs that do not fit four to a CU as well
   if (force_block == 192) for (int wgs=3; wgs>=1; wgs--) shapes.push_back({ 192, wgs });
   // the latency shape: eight wavefronts on one run, one run per CU (a lone wavefront issues a vector
   // instruction every ~9 cycles: two per SIMD halve the time of an iteration; for batches smaller than the chip)
   if (force_block == 512 && has(512)) shapes.push_back({ 512, 1 });
   // two wavefronts on a run, up to eight runs per CU (the kernels exist for the fp64 16-lane family of a fixed-base chain at
   // 128 registers): runs with TSR constraints, whose elimination is the work of two wavefronts (csrc/tsr.h), keep all
   // sixteen wavefronts of a CU at it instead of eight
   if (force_block == 128 && can128) for (int wgs=sw.wgs128; wgs>=4; wgs--) shapes.push_back({ 128, wgs });
   return shapes;
}

// does the option apply to this run, under what is forced?
bool option_allowed(const PlanInput & in, const Forced & force, const Option & o)
{
   if (force.g >= 0 && o.g_lds != force.g) return false;
   if (!o.t_lds && o.g_lds) return false;                      // the trajectory in global memory: after G went there
   if (!o.t_lds && in.free_start) return false;                // start_tsr: the workgroup's copy has a row the global rows do not
   if (force.tl >= 0 && o.t_lds != force.tl && !o.g_lds) return false;
   if (!o.t_lds && in.GS == 16 && in.n_tsrs > 0) return false; // (the constraint phase of the 16-lane kernels reads the LDS copy)
   if (o.with_pcr && !in.pcr_rows) return false;
   if (force.pcr >= 0 && o.with_pcr != force.pcr && in.pcr_rows) return false;
   if (!o.ag_lds && !in.use_momentum) return false;
   if (force.ag >= 0 && o.ag_lds != force.ag && in.use_momentum) return false;
   return true;
}

// estimated throughput of a shape with tiles of t moving waypoints
double score_of(const PlanInput & in, const Shape & sh, const Option & o, int t, int flags)
{
   const int lanes_per_wp = (in.GS == 16) ? 16 : in.GS;
   const int tiles = (in.m + t - 1) / t;
   const double fk_passes = tiles * std::ceil((t + 2) / (sh.block / 64 * FK_WAYPOINTS_PER_WAVE));
   const double rounds = tiles * std::ceil(t * (double) lanes_per_wp / sh.block);
   const double fk_pass = FK_PASS_PER_JOINT * in.nj;
   const double round_cycles = (in.GS == 16) ? ROUND_GS16 : ((in.variant & ORC_VAR_PAIRS) ? ROUND_PAIRS : ROUND_PER_SPHERE * in.Sa);
   const double cycles = fk_pass * fk_passes + round_cycles * rounds + FIXED_PER_ITERATION * (256.0 / sh.block) + (o.with_pcr ? 0.0 : PCR_THROUGH_L2) + (o.ag_lds ? 0.0 : AG_GLOBAL)
                       + (o.g_lds ? 0.0 : G_GLOBAL) + (o.t_lds ? 0.0 : ((flags & ORC_LDS_T_STAGED) ? T_GLOBAL_STAGED : T_GLOBAL_IN_PLACE));
   const double waves_per_simd = sh.wgs * sh.block / 256.0;
   return sh.wgs * (1.0 - PER_EXTRA_WAVE * (waves_per_simd - 1.0)) * (sh.block == 192 ? SHAPE_192 : 1.0) / cycles;
}

// the largest tile of the option that fits the shape's share of the LDS; `best` takes it when its score is the best so far
void try_option(const PlanInput & in, const Switches & sw, const Forced & force, const Shape & sh, const Option & o, IteratePlan & best, double & best_score)
{
   const size_t budget = (LDS_PER_CU / sh.wgs / LDS_GRANULE) * LDS_GRANULE - (sh.wgs == 1 ? 1024 : 0);
   // T in global memory: the update phase and the cost sums work on a copy staged in the dead tile buffers (round 4)
   // unless the run has constraints (their phase reads the trajectory where FK does) or ORC_T_STAGED=0
   const bool want_staged = !o.t_lds && in.n_tsrs == 0 && !sw.t_staged_off;
   int flags = ((in.solve_mode == 2 || in.solve_mode == 3) ? ORC_LDS_SMALL_WORK : 0) | (o.g_lds ? 0 : ORC_LDS_G_GLOBAL) | (o.t_lds ? 0 : ORC_LDS_T_GLOBAL)
             | (want_staged ? ORC_LDS_T_STAGED : 0);
   auto lds_bytes = [&](int t, int fl) {
      return (size_t) lds_layout(in.m + 2, in.n, in.Sa, in.S, in.nj, t, o.with_pcr ? in.pcr_rows : 0, (int) in.real_bytes,
                                 in.use_momentum && o.ag_lds, in.n_sdfs, (int) in.sdf_bytes, fl, in.pair_entries).total_bytes;
   };
   for (int t=(in.m < 254 ? in.m : 254); t>=1; t--)
   {
      if (force.tile > 0 && t != (force.tile < in.m ? force.tile : in.m)) continue;
      size_t need = lds_bytes(t, flags);
      if (need > budget && (flags & ORC_LDS_T_STAGED))
      {
         // (tiles too small to hold the copy: the trajectory is iterated in place through L2)
         const size_t plain = lds_bytes(t, flags & ~ORC_LDS_T_STAGED);
         if (plain <= budget) { need = plain; flags &= ~ORC_LDS_T_STAGED; }
      }
      if (need > budget) continue;
      const double score = score_of(in, sh, o, t, flags);
      if (score > best_score)
      {
         best_score = score; best.tile_m = t; best.pcr_in_lds = o.with_pcr; best.ag_in_lds = o.ag_lds; best.lds_bytes = need; best.block = sh.block; best.per_cu = sh.wgs;
         best.g_in_lds = o.g_lds; best.lds_flags = flags; best.t_in_lds = o.t_lds;
      }
      break;                                   // largest tile of this plan
   }
}

// Tile boundaries.  A tile of s moving waypoints costs ceil(s * lanes per waypoint / threads) rounds of
// the workgroup in the cost phase; equal tiles of the largest size are not always the cheapest cut
// (98 waypoints in tiles of at most 34 at 16 per round: 33 + 33 + 32 is 3 + 3 + 2 rounds, 34 + 32 + 32
// is 3 + 2 + 2): whole rounds in all tiles but one, when that one still fits.
void cut_tiles(IteratePlan & P, int m, int lanes_per_wp)
{
   P.n_tiles = (m + P.tile_m - 1) / P.tile_m;
   P.tile_first = P.tile_rest = P.tile_m;
   const int unit = std::max(1, P.block / lanes_per_wp);      // waypoints of one round
   const int full = (P.tile_m / unit) * unit;
   if (full > 0 && P.n_tiles > 1)
   {
      const int first = m - full * (P.n_tiles - 1);
      auto rounds = [&](int a, int rest) {
         int r = (a + unit - 1) / unit, left = m - a;
         for (int k=1; k<P.n_tiles; k++) { const int v = std::min(rest, left); r += (v + unit - 1) / unit; left -= v; }
         return r;
      };
      if (first > 0 && first <= P.tile_m && rounds(first, full) < rounds(P.tile_m, P.tile_m)) { P.tile_first = first; P.tile_rest = full; }
   }
}

// the structured solve of the constraint step keeps its augmented block in the axis tile buffer (dead during the update phase)
void size_tsr_solve(IteratePlan & P, const PlanInput & in, const Switches & sw)
{
   if (in.n_tsrs == 0 || in.derivative != 1 || sw.tsr_dense) return;
   const int N = in.n + in.tsr_kmax, Wd = N + in.n + 1;
   const size_t need = (size_t) N * Wd + (size_t) in.n * (in.n + 1) + in.n + (size_t)(in.tsr_kmax + 2) * sizeof(int) / in.real_bytes + 2;
   const size_t have = (size_t)(P.tile_m + 2) * P.lay.astr;
   if (Wd <= 64 && need <= have) { P.tsr_structured = 1; P.tsr_wcap = N * Wd; P.tsr_nmax = N; }
}

} // namespace

IteratePlan plan_iterate(const PlanInput & in, const Switches & sw)
{
   const int variant = in.variant;
   auto has = [&](int var, int block) { return kernel_exists(kernel_of(var, block, (int) in.real_bytes)); };
   const int max_wgs_budget = waves_per_simd((int) in.real_bytes, in.GS == 16, 256);      // (the family's register budget)
   const int max_wgs_default = sw.wgs.set ? sw.wgs.value : max_wgs_budget;
   // A caller that knows its batches fit the chip in one wave of four workgroups per CU but not of three (769..1024 runs: the
   // 1024 of BASELINE configs[1]) can ask for the 192-thread shape for the whole module: orc_set_workgroup_threads (measured, one
   // launch of 1024 WAM runs: 9.3 M it/s against 8.4 M; from 4096 runs on the order is reversed).
   int force_block_asked = in.module_threads ? in.module_threads : in.params_threads;
   if (force_block_asked == 512 && !has(variant, 512)) force_block_asked = 0;      // (the pair list of a tree or an fp32 run has no latency shape)
   // orc_set_workgroups_per_cu(4): the fp64 16-lane kernels of a fixed-base chain also exist at 128 VGPRs, four 256-thread
   // workgroups per CU (three tiles instead of two for the WAM): +3 % when launches overlap, -3 % one launch at a time
   int want_wgs = in.module_per_cu ? in.module_per_cu : in.params_per_cu;
   // What the caller did not say, the planner chooses -- from the robot, the run parameters and the MODULE's settings.
   // Runs with TSR constraints and the pair-list family are faster at four workgroups per CU whatever the launch pattern (the
   // constraint step +50 %, held4 +20 %); a module whose launches overlap (orc_set_num_streams >= 2) also takes the four-per-CU
   // kernels of a fixed-base chain (+3-5 %) and, for constrained runs, the 128-thread shape (eight runs per CU: +18 %).  One
   // launch of <= 1024 unconstrained runs at a time is 3 % faster with the kernels' own budget, which is the default there.
   // 3 = "the kernels' own budget", said explicitly.
   const bool can128 = has(variant, 128);
   if (want_wgs == 0 && ((in.n_tsrs > 0 && !(variant & ORC_VAR_FLOATING)) || (variant & ORC_VAR_PAIRS) || (in.overlapping && !(variant & ORC_VAR_FLOATING)))) want_wgs = 4;
   if (want_wgs == 3) want_wgs = 0;
   // (the planner's own 128 is a preference, tried in a pass of its own: a long constrained trajectory that has no 128-thread plan --
   // 40 KB of LDS at four per CU -- is planned like any other run afterwards; a caller's orc_set_workgroup_threads stays binding)
   // ... and so is the 128-thread shape for SHORT trajectories (round 6): a run of at most 32 moving waypoints has two rounds of work for
   // two wavefronts where four wavefronts idle through most of its phases (8 waypoints 52.8 -> 77 M it/s, 16: +8 %, 34: +11 %; from 50
   // on the 256-thread shapes are ahead again: scripts/diag/short_traj_shapes.py, profiles/r06_regime_sweep.txt)
   const bool short128 = in.m <= 32 && !sw.no_short128;
   const bool planner128 = force_block_asked == 0 && ((in.overlapping && in.n_tsrs > 0) || short128) && can128 && !in.free_start && !sw.block_threads.set;
   const bool kernels_at_4 = has(variant | ORC_VAR_WGS4, 256);

   IteratePlan P;
   bool budget4 = false;
   // Pass -1: the planner's own 128-thread shape.  Pass 0: the four-per-CU budget where it is wanted.  Pass 1: the default budget (a run
   // the four-per-CU budget has no room for -- a long trajectory).  Pass 2: without the experiments' switches (a run that has no plan
   // under them -- a forced tile of 33 waypoints at four workgroups per CU, the gradient rows forced out of LDS for a trajectory of
   // three points: the switches are preferences)
   for (int pass=(planner128 ? -1 : 0); pass<3 && !P.tile_m; pass++)
   {
      const bool relax = (pass == 2);
      int max_wgs = relax ? max_wgs_budget : max_wgs_default;
      Forced force;
      force.block = (pass == -1) ? 128 : force_block_asked;
      if (!relax) { force.tile = sw.tile_m.set ? sw.tile_m.value : 0; force.pcr = sw.pcr_lds.set ? sw.pcr_lds.value : -1; force.ag = sw.ag_lds.set ? sw.ag_lds.value : -1; }
      budget4 = (pass == 0) && (want_wgs == 4) && kernels_at_4 && (force.block == 0 || force.block == 256)
                && !sw.block_threads.set && !sw.wgs.set && !sw.tile_m.set;      // (the experiments' switches come first)
      if (budget4) { max_wgs = 4; force.block = 256; }
      if (sw.block_threads.set && !relax) force.block = sw.block_threads.value;
      if (sw.g_lds.set && !relax) force.g = sw.g_lds.value;
      if (sw.t_lds.set && !relax) force.tl = sw.t_lds.value;
      P = IteratePlan();
      double best_score = -1.0;
      const std::vector<Shape> shapes = shapes_of(in, sw, max_wgs, budget4, force.block, can128);
      if (force.block == 128 && !can128) force.block = 0;      // (a robot the shape is not built for keeps its default)
      for (const Shape & sh : shapes)
      {
         if (force.block && sh.block != force.block) continue;
         for (int with_pcr=1; with_pcr>=0; with_pcr--)
            for (int ag_lds=1; ag_lds>=0; ag_lds--)
               for (int g_lds=1; g_lds>=0; g_lds--)
                  for (int t_lds=1; t_lds>=0; t_lds--)
                  {
                     const Option o = { with_pcr, ag_lds, g_lds, t_lds };
                     if (option_allowed(in, force, o)) try_option(in, sw, force, sh, o, P, best_score);
                  }
      }
   }
   if (!P.tile_m) throw std::runtime_error("run does not fit the LDS of one CU!");
   P.variant = variant | (budget4 ? ORC_VAR_WGS4 : 0);
   cut_tiles(P, in.m, (in.GS == 16) ? 16 : in.GS);
   P.lay = lds_layout(in.m + 2, in.n, in.Sa, in.S, in.nj, P.tile_m, P.pcr_in_lds ? in.pcr_rows : 0, (int) in.real_bytes,
                      in.use_momentum && P.ag_in_lds, in.n_sdfs, (int) in.sdf_bytes, P.lds_flags, in.pair_entries);
   size_tsr_solve(P, in, sw);
   if (sw.debug_plan)
      fprintf(stderr, "orc plan: %d threads per workgroup, tile_m %d (%d tiles, first of %d) lds %zu bytes (%d workgroups per CU) pcr_in_lds %d ag_in_lds %d g_in_lds %d t_in_lds %d solve_mode %d\n", P.block, P.tile_m,
              P.n_tiles, P.tile_first, P.lds_bytes, P.workgroups_per_cu(), P.pcr_in_lds, P.ag_in_lds, P.g_in_lds, P.t_in_lds, in.solve_mode);
   return P;
}

} // namespace orc
