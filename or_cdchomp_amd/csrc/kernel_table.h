// kernel_table.h -- which instantiations of chomp_iterate_kernel<real, TREE, GS16, BLOCK, KIND, WGS> the library holds.
//
// The one list that the launcher (chomp_kernel.hip launch_iterate_t expands it), the planner (plan.cpp) and the fold
// (fold.cpp) share; no HIP in here.  A plan names a kernel by its variant mask (the ORC_VAR_ bits of dev_types.h), its block
// size and its precision: kernel_of maps the three to a row key, kernel_exists looks the key up -- exactly: a key without a
// row is refused by the launcher (hipErrorInvalidValue), never served by a neighbour.
#pragma once
#include "dev_types.h"

// One line per instantiation: X(sizeof(real), TREE, GS16, BLOCK, KIND, WGS).  KIND: 0 nothing about the cost phase is known at
// compile time; with GS16 1 | one aligned field 2 | floating base 4 | no inactive sphere left 8; without GS16 1: the J^T form
// is known; the dense pair list 16, 26 its lean form.  WGS: wavefronts per SIMD the registers are budgeted for, 0: the
// family's own (waves_per_simd below).  The order is the order of the functions in the code object: new rows go last.
#define ORC_ITERATE_KERNELS(X) \
   /* fp64 fixed-base 16-lane chain at 128 VGPRs, 128 threads: eight workgroups per CU (orc_set_workgroup_threads(128)) */ \
   X(8, 0, 1, 128, 1, 4) X(8, 0, 1, 128, 3, 4) X(8, 0, 1, 128, 11, 4) \
   /* 17 .. 32 active spheres, fp64: the dense pair list (cost_pairs.h), lean = one aligned field, no inactive sphere left, fixed */ \
   /* base.  A tree (the WAM with its finger dofs active that holds something) at four per CU and at its own budget ... */ \
   X(8, 1, 0, 256, 26, 4) X(8, 1, 0, 256, 16, 4) X(8, 1, 0, 256, 26, 0) X(8, 1, 0, 256, 16, 0) \
   /* ... a chain: the latency shape, four per CU, its own budget.  No 16-lane form, no 192-thread shape */ \
   X(8, 0, 0, 512, 26, 0) X(8, 0, 0, 512, 16, 0) X(8, 0, 0, 256, 26, 4) X(8, 0, 0, 256, 16, 4) X(8, 0, 0, 256, 26, 0) X(8, 0, 0, 256, 16, 0) \
   /* the many-sphere path with its J^T form known (fixed base), trees and chains */ \
   X(8, 1, 0, 512, 1, 0) X(8, 1, 0, 192, 1, 0) X(8, 1, 0, 256, 1, 0) X(8, 0, 0, 512, 1, 0) X(8, 0, 0, 192, 1, 0) X(8, 0, 0, 256, 1, 0) \
   /* fp64 fixed-base 16-lane chains at 128 VGPRs, four 256-thread workgroups per CU (orc_set_workgroups_per_cu(4)); 15: the */ \
   /* floating base with one aligned field of BASELINE configs[3] */ \
   X(8, 0, 1, 256, 1, 4) X(8, 0, 1, 256, 3, 4) X(8, 0, 1, 256, 11, 4) X(8, 0, 1, 256, 15, 4) \
   /* a 16-lane chain with its spheres placed on the row, every kind at the three shapes of the default budget */ \
   X(8, 0, 1, 512, 1, 0) X(8, 0, 1, 192, 1, 0) X(8, 0, 1, 256, 1, 0) X(8, 0, 1, 512, 3, 0) X(8, 0, 1, 192, 3, 0) X(8, 0, 1, 256, 3, 0) \
   X(8, 0, 1, 512, 5, 0) X(8, 0, 1, 192, 5, 0) X(8, 0, 1, 256, 5, 0) X(8, 0, 1, 512, 7, 0) X(8, 0, 1, 192, 7, 0) X(8, 0, 1, 256, 7, 0) \
   X(8, 0, 1, 512, 11, 0) X(8, 0, 1, 192, 11, 0) X(8, 0, 1, 256, 11, 0) X(8, 0, 1, 512, 15, 0) X(8, 0, 1, 192, 15, 0) X(8, 0, 1, 256, 15, 0) \
   /* any robot: nothing known at compile time */ \
   X(8, 0, 0, 512, 0, 0) X(8, 1, 0, 512, 0, 0) X(8, 0, 1, 512, 0, 0) X(8, 1, 1, 512, 0, 0) \
   X(8, 0, 0, 256, 0, 0) X(8, 1, 0, 256, 0, 0) X(8, 0, 1, 256, 0, 0) X(8, 1, 1, 256, 0, 0) \
   X(8, 0, 0, 192, 0, 0) X(8, 1, 0, 192, 0, 0) X(8, 0, 1, 192, 0, 0) X(8, 1, 1, 192, 0, 0) \
   /* fp32.  The pair list: 256 threads at the fp32 many-sphere budget (four per CU), trees and chains; no latency shape */ \
   X(4, 1, 0, 256, 26, 0) X(4, 1, 0, 256, 16, 0) X(4, 0, 0, 256, 26, 0) X(4, 0, 0, 256, 16, 0) \
   /* the many-sphere path with its J^T form known (BASELINE configs[4] is the 256-thread tree) */ \
   X(4, 1, 0, 512, 1, 0) X(4, 1, 0, 192, 1, 0) X(4, 1, 0, 256, 1, 0) X(4, 0, 0, 512, 1, 0) X(4, 0, 0, 192, 1, 0) X(4, 0, 0, 256, 1, 0) \
   /* a 16-lane chain with its spheres placed on the row (no 128-VGPR copies in fp32) */ \
   X(4, 0, 1, 512, 1, 0) X(4, 0, 1, 192, 1, 0) X(4, 0, 1, 256, 1, 0) X(4, 0, 1, 512, 3, 0) X(4, 0, 1, 192, 3, 0) X(4, 0, 1, 256, 3, 0) \
   X(4, 0, 1, 512, 5, 0) X(4, 0, 1, 192, 5, 0) X(4, 0, 1, 256, 5, 0) X(4, 0, 1, 512, 7, 0) X(4, 0, 1, 192, 7, 0) X(4, 0, 1, 256, 7, 0) \
   X(4, 0, 1, 512, 11, 0) X(4, 0, 1, 192, 11, 0) X(4, 0, 1, 256, 11, 0) X(4, 0, 1, 512, 15, 0) X(4, 0, 1, 192, 15, 0) X(4, 0, 1, 256, 15, 0) \
   /* any robot */ \
   X(4, 0, 0, 512, 0, 0) X(4, 1, 0, 512, 0, 0) X(4, 0, 1, 512, 0, 0) X(4, 1, 1, 512, 0, 0) \
   X(4, 0, 0, 256, 0, 0) X(4, 1, 0, 256, 0, 0) X(4, 0, 1, 256, 0, 0) X(4, 1, 1, 256, 0, 0) \
   X(4, 0, 0, 192, 0, 0) X(4, 1, 0, 192, 0, 0) X(4, 0, 1, 192, 0, 0) X(4, 1, 1, 192, 0, 0)

namespace orc {

struct KernelKey { int real_bytes, tree, gs16, block, kind, wgs; };
constexpr bool operator==(const KernelKey & a, const KernelKey & b)
{ return a.real_bytes == b.real_bytes && a.tree == b.tree && a.gs16 == b.gs16 && a.block == b.block && a.kind == b.kind && a.wgs == b.wgs; }

#define ORC_KERNEL_ROW(BYTES, TREE, GS16, BLOCK, KIND, WGS) { BYTES, TREE, GS16, BLOCK, KIND, WGS },
constexpr KernelKey ITERATE_KERNELS[] = { ORC_ITERATE_KERNELS(ORC_KERNEL_ROW) };
#undef ORC_KERNEL_ROW
constexpr int N_ITERATE_KERNELS = (int)(sizeof(ITERATE_KERNELS) / sizeof(ITERATE_KERNELS[0]));

constexpr bool kernel_exists(const KernelKey & k)
{
   for (int i=0; i<N_ITERATE_KERNELS; i++) if (ITERATE_KERNELS[i] == k) return true;
   return false;
}

// The kernel a plan names: its variant mask, block size and precision.  (The 128-thread kernels are built for four wavefronts
// per SIMD only, so the shape implies that budget.)
constexpr KernelKey kernel_of(int variant, int block, int real_bytes)
{
   const bool one_field = (variant & ORC_VAR_ONE_FIELD) != 0, floating = (variant & ORC_VAR_FLOATING) != 0;
   const bool no_inact = one_field && (variant & ORC_VAR_NO_INACT);
   int kind = 0;
   if (variant & ORC_VAR_PAIRS) kind = (no_inact && !floating) ? 26 : 16;
   else if ((variant & ORC_VAR_KIND) && !(variant & ORC_VAR_GS16)) kind = 1;
   else if (variant & ORC_VAR_KIND) kind = 1 | (one_field ? 2 : 0) | (floating ? 4 : 0) | (no_inact ? 8 : 0);
   return { real_bytes, (variant & ORC_VAR_TREE) ? 1 : 0, (variant & ORC_VAR_GS16) ? 1 : 0, block, kind, ((variant & ORC_VAR_WGS4) || block == 128) ? 4 : 0 };
}

// The register budget of a family in wavefronts per SIMD, the second argument of the kernels' launch bounds (3: 168 VGPRs, 12
// wavefronts per CU as 3 x 256 or 4 x 192 threads; 2 for the one-run-per-CU shape of 512).  The fp32 many-sphere kernels are
// built for FOUR (128 VGPRs, four 256-thread workgroups per CU, smaller tiles): measured on BASELINE configs[4] 1.61 -> 1.74
// M it/s; the fp64 16-lane kernels at four gain 3 % with overlapping launches and lose 3 % one launch at a time (config 2),
// lose 5 % on config 4: left at three, with copies at four (WGS 4) where a plan asks for them.
constexpr int waves_per_simd(int real_bytes, bool gs16, int block)
{ return (block == 512) ? 2 : ((real_bytes == 4 && !gs16) ? ORC_WGS_PER_CU_FP32_MANY : ORC_WGS_PER_CU); }
// ... and the workgroups of a row's block size that its registers let a CU hold
constexpr int workgroups_per_cu(const KernelKey & k)
{ return (k.wgs ? k.wgs : waves_per_simd(k.real_bytes, k.gs16 != 0, k.block)) * 256 / k.block; }

// The robot's part of the variant mask (fold.cpp fold_robot; `pairs`: choose_lanes gave it the dense pair list) ...
constexpr int robot_variant(bool tree, int GS, bool floating, int jt_scan, bool placed, int nj, bool pairs, bool no_kind)
{
   int variant = (tree ? ORC_VAR_TREE : 0) | ((GS == 16) ? ORC_VAR_GS16 : 0);
   if (GS == 16 && !tree && jt_scan == 1 && placed && nj <= 16 && !no_kind)
      variant |= ORC_VAR_KIND | (floating ? ORC_VAR_FLOATING : 0);      // the variants that know all this at compile time (phase_cost KIND)
   if (GS != 16 && !floating && jt_scan == (tree ? 2 : 1) && !no_kind && !pairs)
      variant |= ORC_VAR_KIND;                    // many-sphere path: the J^T form is known
   if (pairs) variant |= ORC_VAR_PAIRS | (floating ? ORC_VAR_FLOATING : 0);      // the 32-lane family with the dense pair list
   return variant;
}
// ... and the scenes' (BatchShard::build_device, batch.cpp): one field with the world's axes in every scene, no inactive sphere left
constexpr int scene_variant(int variant, bool one_aligned, bool no_inactive)
{ return ((variant & (ORC_VAR_KIND | ORC_VAR_PAIRS)) && one_aligned) ? (variant | ORC_VAR_ONE_FIELD | (no_inactive ? ORC_VAR_NO_INACT : 0)) : variant; }

#ifdef ORC_FAST_BUILD
// Experiment builds of the kernel file (make var DEFS=-DORC_FAST_BUILD=2): only the kernels of one bench leg are compiled, half a
// minute instead of three; the launcher refuses every other row.
//   4: BASELINE configs[3] (floating base, KIND 15) at the default shape and at four workgroups per CU
//   5: BASELINE configs[4] (fp32, the many-sphere pass of a tree with its J^T form known)
//   6: the WAM that holds a box (a chain's lean pair list) at both budgets
//   7: the TSR-constrained WAM: the kernels of 2 and KIND 11 at eight 128-thread workgroups per CU
//   any other value (2): config 2, the fp64 fixed-base chain with placed spheres, one aligned field, no inactive sphere left
//      (KIND 11), at 256 threads of both budgets and at 192
constexpr bool kernel_compiled(const KernelKey & k)
{
   const bool chain16 = k.real_bytes == 8 && k.gs16 && !k.tree;
   switch (ORC_FAST_BUILD)
   {
   case 4: return chain16 && k.kind == 15 && k.block == 256;
   case 5: return k.real_bytes == 4 && k.tree && !k.gs16 && k.kind == 1 && k.block == 256;
   case 6: return k.real_bytes == 8 && !k.tree && !k.gs16 && k.kind == 26 && k.block == 256;
   case 7: return chain16 && k.kind == 11 && k.block != 512;
   default: return chain16 && k.kind == 11 && (k.block == 256 || k.block == 192);
   }
}
#else
constexpr bool kernel_compiled(const KernelKey &) { return true; }
#endif

} // namespace orc
