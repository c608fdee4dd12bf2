// chomp_kernel.hip -- the CHOMP iteration as one fused gfx950 kernel.
//
// One workgroup (256 threads = 4 wavefronts; 192 or 512 on request) owns one run for all n_iter
// iterations of a launch.  The trajectory, gradient and momentum of the run stay in LDS for the
// whole launch; HBM is touched for the trajectory/momentum at launch start and end, for the SDF
// gathers, and for three cost doubles.  The kernel itself is a thin loop around PHASE FUNCTIONS
// (real calls: a register allocation per phase, see the comment at struct Env).
//
// Per iteration (reference call stack: SURVEY.md 3.3):
//   tiles of waypoints {
//     phase_fk    lane = (waypoint, world axis)  sphere_cost_pre  src/orcdchomp_mod.cpp:988-1093  (fk.h)
//     phase_cost  lane = (waypoint, sphere)      sphere_cost      src/orcdchomp_mod.cpp:1134-1327 (cost_gs16.h, cost_generic.h)
//                 J^T by a wrench suffix scan over the spheres of a waypoint -> G row
//   }
//   phase_update  lane = (waypoint, dof)         cd_chomp_iterate src/libcd/chomp.c:490-655
//                 G/m + A T + B; A^-1 G (closed-form Toeplitz scans, cyclic reduction or dense);
//                 [phase_tsr: the hard constraints, src/libcd/chomp.c:550-600, tsr.h]; T -= AG/lambda;
//                 limit_rounds_call: the joint-limit projection rounds by one wavefront
//   phase_costs   obstacle and smoothness cost (chomp.c:484-491, 660-677), quaternion renormalisation
//
// Differences from the reference that are deliberate (all inside the stated tolerance):
// the dense m x m products are replaced by the band of A and a structured solve; the per-sphere
// 3 x n Jacobians are never formed (J^T x is evaluated as axis . ((p - anchor) x force)); a
// self-collision pair is evaluated once for both of its spheres.
//
// The layers, in inclusion order (each a header included inside this file's namespace; this file keeps the kernarg helpers,
// Env, the convergence state, the phases, the kernel, seed_traj_kernel and the launchers):
//   sdf_lookup.h     M<real>, the precision's math functions, and the field lookup
//   fast_math.h      rcp_fast, sqrt_rsq, sqrt_rsq_pos, div_n
//   wave.h           lane and wavefront primitives: DPP moves, sums, arg-max, scans, lane reads, uni / uni64 / unir / uniform_ptr
//   metric_solve.h   A^-1 g: cyclic reduction, dense, Toeplitz scans, semiseparable scans; metric_solve
//   limit_rounds.h   the joint-limit rounds by one wavefront (over limit_regs.h: the register forms); limit_rounds_call*
//   band.h           A T + B: band_row, smooth_grad, band_gradient_pass, band_cost_pass
//   sdf_cell_lookup.h   the field lookup in cell units of the two cost passes with one lookup per lane
//   cost_gs16.h, cost_pairs.h, self_mfma.h, cost_generic.h      the cost phase by the robot's number of active spheres
//   fk.h             forward kinematics of a tile's waypoints
//   tsr.h            the hard constraints (over tsr_point.h, tsr_form.h), behind Env and the convergence state
// Three minutes of compile time hang on these.  With the host files this one shares dev_types.h, kernel_table.h, launch.h and
// wave_roles.h and nothing else: a change to a header of the host layer (batch.h, module.h, ...) does not cost the kernel build.
#include <hip/hip_runtime.h>
#include <math.h>
#include <atomic>
#include <type_traits>
#include <utility>
#include "dev_types.h"
#include "kernel_table.h"
#include "launch.h"
#include "wave_roles.h"

// the device arithmetic may fuse a*b+c (the host files are built with -ffp-contract=off so that
// the SDF build stays bit-identical to the reference; the kernels are held to a tolerance)
#pragma clang fp contract(fast)


namespace {

#include "sdf_lookup.h"
#include "fast_math.h"
#include "wave.h"
#include "metric_solve.h"
#include "limit_rounds.h"
#include "band.h"

// entries of a thread whose gradient / momentum rows the update phase reads ahead where they live in global memory and a thread has more than four
constexpr int UPDATE_BATCH = 4;
// waypoints per lane in the 16-sphere cost phase (1: registers go to a third workgroup per CU instead)
constexpr int GS16_U = 1;
// wave priorities of the phases (s_setprio): the latency-bound ones go first when they have something to issue
constexpr int PRIO_FK = 3, PRIO_COST = 0, PRIO_UPDATE = 3;
constexpr int PRIO_COST_LAST = 2;      // the last round of a tile: it is what the tile's barrier waits for

#include "sdf_cell_lookup.h"
#include "cost_gs16.h"
#include "cost_pairs.h"
#include "self_mfma.h"
#include "cost_generic.h"
#include "fk.h"

// ---------------------------------------------------------------------------
// The iterate kernel is a thin loop around PHASE FUNCTIONS (real calls, not inlined): every phase
// gets a register allocation of its own, as if it were a kernel, while the run's state stays in LDS
// across them.  Inlined into one function the phases took part in each other's allocation: values
// of the update phase lived across the cost phase, the SGPR tuples of the kernarg block were spilled
// and reloaded in its inner loops, and any change to a rare path moved the spills of the hot one.
// A phase function receives the address of the kernarg block (DevBatch, read with scalar loads where
// it is used) and a few wave-uniform scalars, and derives the LDS carve-up again (scalar arithmetic).
// This file is compiled with -mllvm -enable-ipra=0 (the Makefile's KFLAGS).  With the compiler's inter-procedural register
// allocation a caller takes every callee-saved SCALAR register its callee touches for lost, although the callee saves and restores
// it (in VGPR lanes: the target has no scalar spill to memory), and saves its own copy around the call as well: the save is paid
// twice.  Without it the callers rely on the calling convention (NOTES/call-overhead.md).
template <typename real> using KArg = const __attribute__((address_space(4))) DevBatch<real>;
template <typename real> using KModel = const __attribute__((address_space(4))) DevModel<real>;

template <typename real>
__device__ __forceinline__ KArg<real> * uniform_kernarg(const void * p) { return (KArg<real> *) uni64((unsigned long long) p); }
// the kernarg block again, as an address the compiler knows nothing about: what is read through it is read where it is used, by a
// scalar load, and is not kept in a register from an earlier read (the kernel's loop, between its phase calls)
template <typename real>
__device__ __forceinline__ KArg<real> * fresh_kernarg(const void * p)
{
   unsigned long long v = (unsigned long long) p;
   __asm__ volatile("" : "+s"(v));
   return (KArg<real> *) v;
}
// the scene of this workgroup's run (wave-uniform; DevBatch::scene_of_run)
template <typename BT>
__device__ __forceinline__ int run_scene(const BT & b)
{
   return (b.n_scenes > 1) ? uni(((const __attribute__((address_space(4))) int *) b.scene_of_run)[blockIdx.x]) : 0;
}

// the record of this workgroup's run's four parameters (wave-uniform; DevBatch::run_params): row blockIdx.x of the table when
// the batch has one, the batch's own record in the kernarg block otherwise.  This select is the only place where the two differ
template <typename real, typename BT>
__device__ __forceinline__ const __attribute__((address_space(4))) RunParams<real> * run_params_of(const BT & b)
{
   typedef const __attribute__((address_space(4))) RunParams<real> * P;
   return (P) uni64(b.run_params ? (unsigned long long)(b.run_params + blockIdx.x) : (unsigned long long) &b.shared);
}

// The LOGICAL thread index every phase hands its work out by (wave_roles.h): the hardware index rotated by `rot` whole
// wavefronts, the lane unchanged.  `rot` is wave-uniform -- the switch from the kernarg block, the workgroup index, and the low bits
// of the iteration number, which the kernel's loop packs into an argument the phase takes anyway (pack_it: the loop carries no
// scalar more across the calls) -- so it costs a phase call a handful of scalar instructions and two vector ones.
// The compiler is told the range: the cost passes address with 24-bit multiplies that depend on it.
template <int BLOCK, typename BT>
__device__ __forceinline__ int orc_tid(const BT & b, int it_bits)
{
   const int rot = orc::wave_rot(b.wave_rotate, (int) blockIdx.x, it_bits, BLOCK);
   const int t = orc::logical_tid((int) threadIdx.x, rot, BLOCK);
   __builtin_assume(t >= 0 && t < BLOCK);
   return t;
}
constexpr int IT_SHIFT = ORC_IT_SHIFT;      // (the payloads stay below 2^24: checked where a launch is prepared, batch.cpp)
__device__ __forceinline__ int pack_it(int v, int it) { return v | ((it & 7) << IT_SHIFT); }
__device__ __forceinline__ int packed_it(int v) { return (v >> IT_SHIFT) & 7; }
__device__ __forceinline__ int packed_arg(int v) { return v & ((1 << IT_SHIFT) - 1); }
// the thread that keeps the phase timers: the first of the last logical wavefront, which takes part in every phase (the first
// wavefronts only meet the barrier of an FK phase that has fewer groups than the workgroup has wavefronts)
template <int BLOCK> __device__ __forceinline__ bool marks(int tid) { return tid == BLOCK - 64; }

// the LDS carve-up and the views derived from it (everything here is wave-uniform)
template <typename real>
struct Env
{
   double * red; int * redi; unsigned int * colmask_s;
   long long * phc_s;                      // [8] per-phase cycle counters (diagnostics), thread 0
   real * T_s, * G_s, * Gc, * W_s, * pos_s, * ax_s, * srad_s, * sinact_s, * jl_s, * r2_s, * pcr_s, * base_s;
   real * T_u;                             // the trajectory as the update phase and the cost sums see it: T_s, or its staged copy (DevBatch::t_staged)
   int * slink_s, * jtype_s, * jcol_s, * slot_s;
   int * jctl_s; DevSdf<real> * sdfs_s; unsigned long long * saff_s, * sallow_s;
   real * pent_s; int * pgat_s;            // the staged self-collision pair list (cost_pairs.h): entries { rsum, first | second << 8 } [pr_rounds][32][2 reals], gather words [pr_rounds][32][2]
   real * traj_g, * AG_g, * AG_s;
   const real * pcr_tab;
   int pstr, astr;
   ModelView<real> mod;
};

template <typename real, bool GS16, typename BT>
__device__ __forceinline__ Env<real> make_env(const BT & b, unsigned char * smem_raw)
{
   Env<real> E;
   const int run = blockIdx.x;
   const int n = b.n, m = b.m, mn = m*n;
   const int nj = b.ms.nj, Sa = b.ms.Sa, S = b.ms.S;
   const auto & L = b.lay;          // computed on the host (lds_layout, dev_types.h)
   E.red = (double *) smem_raw;                            // [8] reduction scratch
   E.redi = (int *)(E.red + 16);                           // [8] (red: [16] doubles, one or two per wavefront)
   E.colmask_s = (unsigned int *)(E.redi + 8);             // [2] columns with an entry outside its joint limits after the step
   E.phc_s = (long long *)(smem_raw + ORC_LDS_HEADER - 64);
   real * lds = (real *)(smem_raw + ORC_LDS_HEADER);
   E.traj_g = b.traj + (size_t) run * b.np_global * n;      // (np_global == n_points unless the start point is a variable)
   // [np][n]; the kernels of the generic cost path may leave it in global memory (large robots: the
   // LDS then holds tiles only and a third workgroup fits the CU); __syncthreads orders the accesses
   // of a workgroup's wavefronts to it
   E.T_s  = !b.t_in_lds ? E.traj_g : lds + L.T;      // (the 16-lane kernels too, since round 4: long runs trade the LDS copy for larger tiles)
   E.T_u  = (!b.t_in_lds && b.t_staged) ? lds + L.Tu : E.T_s;
   E.G_s  = lds + L.G;                                     // [m][n] (inside the tile buffers when !g_in_lds: update phase only)
   E.Gc = b.g_in_lds ? E.G_s : b.Gcost + (size_t) run * mn;   // where the cost phase puts its gradient rows
   E.W_s  = lds + L.W;                                     // [m][n] work
   E.pos_s = lds + L.pos;                                  // [tile_m+2][Sa][3]
   E.ax_s = lds + L.ax;                                    // [tile_m+2][nj][6]
   E.pstr = L.pstr; E.astr = L.astr;                       // padded waypoint strides of pos_s / ax_s
   E.srad_s = lds + L.srad;                                // [S] sphere radii
   E.sinact_s = lds + L.sinact;                            // [S-Sa][3] inactive sphere centres
   E.jl_s = lds + L.jl;                                    // [2][n] joint limits
   E.r2_s = lds + L.r2;                                    // [8][16] squared ranges of the self-collision row rotations
   E.pcr_s = lds + L.pcr;                                  // cyclic-reduction tables (when staged)
   E.slink_s = (int *)(smem_raw + L.ints_bytes);           // [S] link of each sphere
   E.jtype_s = E.slink_s + S;                              // [nj]
   E.jcol_s = E.jtype_s + nj;                              // [nj]
   E.slot_s = E.jcol_s + nj;                               // [Sa_real] slot of the k-th active sphere (sorted order)
   E.base_s = E.pcr_s + (((b.pcr_in_lds ? b.pcr_rows : 0)*m + 3) & ~3);     // base frame [12]
   E.jctl_s = (int *)(smem_raw + L.joints_bytes);
   E.sdfs_s = (DevSdf<real> *)(smem_raw + L.sdfs_bytes);
   E.saff_s = (unsigned long long *)(smem_raw + L.saff_bytes);
   E.sallow_s = (unsigned long long *)(smem_raw + L.sallow_bytes);
   E.pent_s = (real *)(smem_raw + L.ptab_bytes);
   E.pgat_s = (int *)(E.pent_s + b.ms.pr_rounds * b.ms.GS * 2);      // (GS = 16 or 32 lanes per round and waypoint)
   ModelView<real> & mod = E.mod;
   mod.nj = nj; mod.n = n; mod.floating = b.ms.floating; mod.tree = b.ms.tree; mod.Sa = Sa; mod.S = S; mod.GS = b.ms.GS; mod.jt_scan = b.ms.jt_scan;
   mod.Sa_real = b.ms.Sa_real; mod.placed = b.ms.placed; mod.live_mask = b.ms.live_mask; mod.slot_of = E.slot_s;
   mod.base_sph_begin = b.ms.base_sph_begin; mod.base_sph_end = b.ms.base_sph_end;
   mod.base_R = E.base_s; mod.base_t = E.base_s + 9;
   mod.jctl = E.jctl_s; mod.sph_affects = E.saff_s; mod.sph_allowed = E.sallow_s;
   mod.jpk = (const __attribute__((address_space(4))) int *) b.model->jpacked;
   mod.jpk2 = (const __attribute__((address_space(4))) int *) b.model->jpacked2;
   mod.sph_pos_c = (const __attribute__((address_space(4))) real (*)[3]) b.model->sph_pos;
   mod.joints_c = (const __attribute__((address_space(4))) DevJoint<real> *) b.model->joints;
   mod.slot_c = (const __attribute__((address_space(4))) int *) b.model->slot_of;
   mod.fkj = (const __attribute__((address_space(4))) DevFkJoint<real> *) b.model->fkj;
   mod.n_static = b.ms.n_static;
   mod.empty_mask = b.ms.placed ? (unsigned int)(~(b.ms.live_mask | b.ms.static_mask) & 0xFFFFull) : 0u;
   mod.static_slot_c = (const __attribute__((address_space(4))) int *) b.model->static_slot;
   mod.static_pos_c = (const __attribute__((address_space(4))) real (*)[3]) b.model->static_pos;
   mod.rp = run_params_of<real>(b);
   {
      // the run's scene: its index and field count by scalar loads (one scene: scene 0 with all the batch's fields)
      const int scene = run_scene(b);
      mod.n_sdfs = (b.n_scenes > 1) ? uni(((const __attribute__((address_space(4))) int *) b.scene_nsdf)[scene]) : b.n_sdfs;
      mod.sdfc = (const __attribute__((address_space(4))) DevSdfCell<real> *) b.sdfc + (size_t) scene * b.sdfc_stride;
   }
   E.AG_g = b.AG + (size_t) run * mn;
   // momentum: in LDS for the launch, or in place in global memory (every entry is read and written
   // by the same thread, e = tid + k BLOCK, in all loops that touch it)
   E.AG_s = b.ag_in_lds ? lds + L.AG : E.AG_g;             // [m][n]
   E.pcr_tab = b.pcr_in_lds ? E.pcr_s : b.pcr;
   return E;
}

extern __shared__ __align__(16) unsigned char orc_smem[];

// ---- convergence stop (orc_batch_set_convergence) ----
// Its state lives in free bytes of the LDS header, and the phase functions keep it (not the kernel's loop: the loop's
// scalars are held across the phase calls, and one more of them spills on the headline kernel): the previous iteration's
// total cost in this call (NaN: none yet, so that the call's first iteration is never settled), the settled iterations in
// a row, and the stop flag the loop reads.  A launch that continues a call (carry_status) picks up where the last one left
// it (DevBatch::conv_prev / conv_streak, written back by phase_finish).
#define ORC_LDS_CONV 176      // bytes [176, 192) of the header: after the timer mark, before the phase counters
struct ConvState { double prev; int streak, stop; };
static_assert(ORC_LDS_CONV + sizeof(ConvState) <= ORC_LDS_HEADER - 64, "the convergence state overlaps the phase counters");
__device__ __forceinline__ ConvState * conv_state() { return (ConvState *)(orc_smem + ORC_LDS_CONV); }

// phase_setup, thread 0 (a barrier follows): the stop flag is clear in every launch
template <typename real>
__device__ __forceinline__ void conv_begin(KArg<real> & b, int run)
{
   ConvState * cs = conv_state();
   cs->stop = 0;
   if (b.conv_patience)
   {
      cs->prev = b.carry_status ? b.conv_prev[run] : __longlong_as_double(0x7ff8000000000000LL);
      cs->streak = b.carry_status ? b.conv_streak[run] : 0;
   }
}

// phase_costs, after a complete iteration with costs (obs, smooth) (workgroup-uniform): the rule of convergence_stop
// (or_cdchomp_amd/module.py); raises the stop flag when the streak reaches the patience
template <typename real>
__device__ __forceinline__ void conv_step(KArg<real> & b, double obs_in, double smooth_in, int tid)
{
   ConvState * cs = conv_state();
   const double obs = unir(obs_in), smooth = unir(smooth_in);
   const double tot = obs + smooth;                  // (the trace's column 0)
   const double prev = unir(cs->prev);
   const bool settled = ::fabs(prev - tot) <= b.conv_rtol * ::fabs(prev) && obs <= b.conv_obs_max;
   const int streak = settled ? uni(cs->streak) + 1 : 0;
   __syncthreads();                                  // (every wavefront has read the state)
   if (tid == 0) { cs->prev = tot; cs->streak = streak; cs->stop = (streak >= b.conv_patience) ? 1 : 0; }
   __syncthreads();
}

#include "tsr.h"

// per-phase cycle counters (diagnostics: b.phase_cycles == null in production), kept in the LDS header
template <typename real, typename BT>
__device__ __forceinline__ void phase_mark(const BT & b, const Env<real> & E, int slot, bool marker)
{
   if (b.phase_cycles && marker)
   {
      long long * tm = (long long *)((unsigned char *) E.red + 168);
      const long long now = clock64();
      if (slot >= 0) E.phc_s[slot] += now - *tm;
      *tm = now;
   }
}

// ---- staging: the run's trajectory and everything read-only the iteration touches, into LDS ----
template <typename real, bool TREE, bool GS16, int BLOCK, int WGS = 0>      // (WGS: a copy per register budget of the calling kernels, see WavesPerSimd)
__device__ __attribute__((noinline)) void phase_setup(const void * kp)
{
   KArg<real> & b = *uniform_kernarg<real>(kp);
   const Env<real> E = make_env<real, GS16>(b, orc_smem);
   const DevModel<real> & gmod = *b.model;      // global copy: read once
   const int tid = orc_tid<BLOCK>(b, 0);
   const int n = b.n, m = b.m, np = b.n_points, mn = m*n;
   const int nj = E.mod.nj, Sa = E.mod.Sa, S = E.mod.S;
   // where this wavefront sits (diagnostics: b.wave_hwid == null in production): its hardware-ID register, read once per launch
   // (scripts/wave_placement.py; one record per hardware wavefront of the run's workgroup) and, in bits 8.. of the second word, the
   // logical wavefront it is in the launch's last iteration (what ORC_WAVE_ROTATE made of it)
   if (b.wave_hwid && (threadIdx.x & 63) == 0)
   {
      unsigned int * rec = b.wave_hwid + ((size_t) blockIdx.x * 8 + (threadIdx.x >> 6)) * 2;
      rec[0] = __builtin_amdgcn_s_getreg(ORC_GETREG_HW_ID);
      rec[1] = __builtin_amdgcn_s_getreg(ORC_GETREG_XCC_ID) | ((unsigned int)(orc_tid<BLOCK>(b, (b.n_iter - 1) & 7) >> 6) << 8);
   }
   if (b.t_in_lds)
   {
      // start_tsr: the start point is the first moving row.  The row in front of it is not a trajectory
      // point (no start boundary in the metric); it holds a copy of the point AFTER the start point, so that
      // the regular cost pass sees the start point at rest (cost_gs16.h START)
      const int skip = b.free_start ? n : 0;
      for (int e=tid; e<np*n; e+=BLOCK) E.T_s[e] = E.traj_g[(e < skip) ? e + skip : e - skip];
   }
   for (int e=tid; e<S; e+=BLOCK) { E.srad_s[e] = gmod.sph_radius[e]; E.slink_s[e] = gmod.sph_link[e]; }
   for (int e=tid; e<(S-Sa)*3; e+=BLOCK) E.sinact_s[e] = gmod.sph_inactive_pos[e/3][e%3];
   for (int e=tid; e<nj; e+=BLOCK)
   {
      // (the joints' fixed transforms and axes are read by scalar loads from the model: fk.h)
      const DevJoint<real> & J = gmod.joints[e];
      E.jtype_s[e] = J.type; E.jcol_s[e] = J.col;
      E.jctl_s[2*e] = J.packed;
      E.jctl_s[2*e+1] = (J.aff_begin & 255) | ((J.aff_end & 255) << 8) | ((J.type & 255) << 16) | ((J.col & 255) << 24);
   }
   for (int e=tid; e<(E.mod.placed ? E.mod.Sa : E.mod.Sa_real); e+=BLOCK) E.slot_s[e] = gmod.slot_of[e];      // (placed: all 16 entries, see DevModel::slot_of)
   for (int e=tid; e<Sa; e+=BLOCK) E.saff_s[e] = gmod.sph_affects[e];
   for (int e=tid; e<12; e+=BLOCK) E.base_s[e] = (e < 9) ? gmod.base_R[e] : gmod.base_t[e-9];
   {
      // word-wise copy of the run's scene's field descriptors
      const int * src2 = (const int *)(b.sdfs + (size_t) run_scene(b) * b.n_sdfs); int * dst2 = (int *) E.sdfs_s;
      for (int e=tid; e<E.mod.n_sdfs*(int)(sizeof(DevSdf<real>)/4); e+=BLOCK) dst2[e] = src2[e];
   }
#ifdef ORC_ABLATE_SDFLDS
   __syncthreads();
   if (tid < E.mod.n_sdfs) E.sdfs_s[tid].data = E.pos_s;
#endif
   for (int e=tid; e<n; e+=BLOCK) { E.jl_s[e] = b.jl_lo[e]; E.jl_s[n+e] = b.jl_hi[e]; }
   if (!GS16)
      for (int e=tid; e<b.ms.pr_rounds*b.ms.GS; e+=BLOCK)
      {
         const int src = (e / b.ms.GS) * 32 + (e % b.ms.GS);      // (the model's tables have 32 entries per round)
         E.pent_s[2*e] = gmod.pr_rsum[src]; *(int *)(E.pent_s + 2*e + 1) = gmod.pr_ab[src];
         E.pgat_s[2*e] = gmod.pr_gat[2*src]; E.pgat_s[2*e+1] = gmod.pr_gat[2*src+1];
      }
   if (b.pcr_in_lds)
      for (int e=tid; e<b.pcr_rows*m; e+=BLOCK) E.pcr_s[e] = b.pcr[e];
   if (b.use_momentum && b.ag_in_lds) for (int e=tid; e<mn; e+=BLOCK) E.AG_s[e] = E.AG_g[e];
   if (tid < 2) E.colmask_s[tid] = 0u;
   if (tid < 8) E.phc_s[tid] = 0;
   if (tid == 0) conv_begin<real>(b, blockIdx.x);
   __syncthreads();

   if (!GS16 && b.ms.pr_rounds == 0 && tid < 64)
   {
      // the spheres a sphere can collide with: active, on another link (src/orcdchomp_mod.cpp:1255-1256)
      unsigned long long allow = 0ull;
      if (tid < Sa)
         for (int o=0; o<Sa; o++)
            if (E.slink_s[o] != E.slink_s[tid]) allow |= 1ull << o;
      E.sallow_s[tid] = allow;
   }
   if (GS16 && tid < 64)
   {
      // squared range of the pair (lane, lane rotated by K) for the row rotations of the
      // self-collision term; -1: the pair never counts (same link, or a lane without a sphere).
      // The partner's identity comes through the same DPP rotation the cost phase uses.
      const int srow = tid & 15;
      const unsigned long long live_mask = E.mod.live_mask | b.ms.static_mask;      // lanes that hold a sphere, static ones included
      const bool has = ((live_mask >> srow) & 1ull) != 0;
      const real rad = has ? E.srad_s[srow] : (real)0;
      const int link = has ? E.slink_s[srow] : -1 - srow;
      const real eps_self = b.epsilon_self;
#define ORC_R2(K) do { \
         const int sp_ = dpp_move<0x120 + K>(srow); \
         const real ro_ = dpp_move<0x120 + K>(rad); \
         const int lo_ = dpp_move<0x120 + K>(link); \
         const real R_ = rad + ro_ + eps_self; \
         if (tid < 16) E.r2_s[(K-1)*16 + srow] = (has && ((live_mask >> sp_) & 1ull) && lo_ != link) ? R_ * R_ : (real)(-1); \
      } while (0)
      ORC_R2(1); ORC_R2(2); ORC_R2(3); ORC_R2(4); ORC_R2(5); ORC_R2(6); ORC_R2(7); ORC_R2(8);
#undef ORC_R2
   }
   __syncthreads();
   phase_mark<real>(b, E, -1, marks<BLOCK>(tid));
}

// ---- hmc momentum resample (src/orcdchomp_mod.cpp:2755-2768): AG <- the call's noise slot ----
template <typename real, bool GS16, int BLOCK, int WGS = 0>
__device__ __attribute__((noinline)) void phase_hmc(const void * kp, int slot_in)
{
   KArg<real> & b = *uniform_kernarg<real>(kp);
   const int slot = packed_arg(uni(slot_in)), tid = orc_tid<BLOCK>(b, packed_it(uni(slot_in)));
   const Env<real> E = make_env<real, GS16>(b, orc_smem);
   const int mn = b.m * b.n;
   const real * nz = b.noise + ((size_t) blockIdx.x * b.max_resamples + slot) * mn;
   for (int e=tid; e<mn; e+=BLOCK) E.AG_s[e] = nz[e];
   __syncthreads();
}

// copy `count` reals between global memory and LDS with eight loads in flight per thread (a plain loop waits for every
// load before it issues the next: a round trip through L2 or the Infinity Cache per 2 KB)
template <typename real, int BLOCK>
__device__ __forceinline__ void copy_batched(real * dst, const real * src, int count, int tid)
{
   int e = tid;
   for (; e + 7*BLOCK < count; e += 8*BLOCK)
   {
      real v[8];
#pragma unroll
      for (int q=0; q<8; q++) v[q] = src[e + q*BLOCK];
#pragma unroll
      for (int q=0; q<8; q++) dst[e + q*BLOCK] = v[q];
   }
   for (; e < count; e += BLOCK) dst[e] = src[e];
}

// ---- FK phase of one tile: lane = (waypoint, world axis) (sphere_cost_pre, src/orcdchomp_mod.cpp:988-1093) ----
template <typename real, bool TREE, bool GS16, int BLOCK, int WGS = 0>
__device__ __forceinline__ void phase_fk_body(const void * kp, int ts_in, int te_in)
{
   KArg<real> & b = *uniform_kernarg<real>(kp);
   const int ts = uni(ts_in), te = packed_arg(uni(te_in));
   const Env<real> E = make_env<real, GS16>(b, orc_smem);
   const int tid = orc_tid<BLOCK>(b, packed_it(uni(te_in))), n = b.n;
   const int nfk = te - ts + 2;          // waypoints ts .. te+1 (global index)
   __builtin_amdgcn_s_setprio(PRIO_FK);          // latency-bound phases go first when they have something to issue
   // a wavefront walks 20 waypoints: five triads of lanes (x, y, z rows) in each of its four rows of 16.  A robot whose
   // joint tree is a chain that then branches (DevModel::fk_split) is walked by PAIRS of wavefronts: one takes the
   // joints up to fk_b_begin, the other the chain (without storing) and the joints from fk_b_begin on
   const int lane16 = tid & 15, triad = (lane16 * 11) >> 5, wave = uni(tid >> 6);      // (the compiler must know the walk's joint indices as uniform: scalar loads)
   const int nseg = (b.ms.fk_split && (BLOCK/64) % 2 == 0) ? 2 : 1;
   // (the groups go to the LAST wavefronts: the first ones have the partial cost rounds and the joint-limit rounds, wave_roles.h)
   const int seg = orc::fk_seg_of_wave(wave, nseg), group = orc::fk_group_of_wave(wave, BLOCK, nseg), groups = orc::fk_groups(BLOCK, nseg);
   const int nj = E.mod.nj;
   const int n_anc = seg ? b.ms.fk_nanc : 0, j_begin = seg ? b.ms.fk_b_begin : 0, j_end = (nseg == 2 && !seg) ? b.ms.fk_b_begin : nj;
   const int wv = group * 20 + ((tid >> 4) & 3) * 5 + triad;
   for (int w0=0; w0<nfk; w0+=groups*20)
   {
      if (w0 + group * 20 >= nfk) continue;             // a wavefront without a waypoint in this round (wave-uniform)
      const int w = w0 + wv;
      const bool valid = (lane16 < 15) && (w < nfk);
      const int wr = valid ? w : 0;
      fk_waypoint_triad<real, TREE>(E.mod, E.T_s + (ts + wr)*n, n_anc, j_begin, j_end, seg == 0, (lane16 < 15) ? lane16 - 3*triad : 0, valid,
                                    E.pos_s + wr*E.pstr, E.ax_s + wr*E.astr, !b.t_in_lds);
   }
   __syncthreads();
   phase_mark<real>(b, E, 0, marks<BLOCK>(tid));
}
template <typename real, bool TREE, bool GS16, int BLOCK, int WGS = 0>
__device__ __attribute__((noinline)) void phase_fk(const void * kp, int ts_in, int te_in)
{
   phase_fk_body<real, TREE, GS16, BLOCK, WGS>(kp, ts_in, te_in);
}

// ---- start_tsr: the cost pass of the start point alone (one-sided velocity; cost_gs16.h START), after the
// regular pass of its tile.  A function of its own: inside phase_cost its registers and code were in the way
// of the regular pass (1 % of config 2's throughput without ever running) ----
template <typename real, bool TREE, bool GS16, int BLOCK, int WGS = 0>
__device__ __attribute__((noinline)) double phase_cost_start(const void * kp, int do_iteration_in, double cost_lane)
{
   KArg<real> & b = *uniform_kernarg<real>(kp);
   const bool do_iteration = packed_arg(uni(do_iteration_in)) != 0;
   const int tid = orc_tid<BLOCK>(b, packed_it(uni(do_iteration_in)));
   Env<real> E = make_env<real, GS16>(b, orc_smem);
   E.mod.live_mask |= b.ms.static_mask;
   const real inv_eps = E.mod.rp->inv_epsilon, inv_eps_self = b.inv_epsilon_self;
   if constexpr (GS16)
      cost_tile_gs16<real, GS16_U, BLOCK, KArg<real>, true>(b, E.mod, 0, 1, do_iteration, E.T_s, E.Gc, E.pos_s, E.ax_s, E.srad_s, E.sinact_s, E.r2_s,
                                                          E.slink_s, E.jtype_s, E.jcol_s, inv_eps, inv_eps_self, cost_lane, tid);
   else
      cost_tile_generic<real, BLOCK, KArg<real>, true>(b, E.mod, E.sdfs_s, 0, 1, do_iteration, E.T_s, E.Gc, E.pos_s, E.ax_s, E.srad_s, E.sinact_s,
                                                      E.slink_s, E.jtype_s, E.jcol_s, E.pstr, E.astr, inv_eps, inv_eps_self, cost_lane, nullptr, tid);
   __syncthreads();
   return cost_lane;
}

// ---- cost phase of one tile: lane = (waypoint, sphere) (sphere_cost, src/orcdchomp_mod.cpp:1134-1327) ----
// KIND: what the kernel variant knows about the workload at compile time (bits; 0 = nothing).
//   1  a chain of at most 16 joints whose spheres are placed on the row (DevModel::jt_scan == 1, placed == 1:
//      the WAM of the BASELINE configurations), with a fixed base unless bit 4 says it floats: the J^T code
//      has one form instead of a branch over five, and one lane group finishes all joints
//   2  one signed distance field whose axes are the world's (a kinbody that is only translated): no loop
//      over fields, no best-of-N bookkeeping across it, no rotation of point and gradient
//   8  (with 1 and 2) no inactive sphere is left for the loop over them
// The pass has no register to spare, so what it need not keep alive is time: 122.4 -> 117.3 ms for 16 384
// WAM runs with bit 1, -> 112.2 ms with both (instantiated: 0, 1, 3, 11, and 5, 7, 15 for the floating base).
// ITER: the pass belongs to an iteration (forces and gradient rows), or is the cost-only pass that ends a call.
template <typename real, bool TREE, bool GS16, int BLOCK, int KIND = 0, bool ITER = true>
__device__ __forceinline__ double phase_cost_body(const void * kp, int ts_in, int te_in, double cost_lane)
{
   KArg<real> & b = *uniform_kernarg<real>(kp);
   const int ts = uni(ts_in), te = packed_arg(uni(te_in));
   const int tid = orc_tid<BLOCK>(b, packed_it(uni(te_in)));
   const bool do_iteration = ITER;
   Env<real> E = make_env<real, GS16>(b, orc_smem);
   if constexpr (GS16 && (KIND & 1) != 0) { E.mod.floating = (KIND & 4) ? 1 : 0; E.mod.jt_scan = 1; E.mod.placed = 1; }
   // the many-sphere path: bit 1 = a fixed base and the J^T ranges of a chain (1) or of a tree in depth-first order (2)
   if constexpr (!GS16 && (KIND & 1) != 0) { E.mod.floating = 0; E.mod.jt_scan = TREE ? 2 : 1; }
   E.mod.live_mask |= b.ms.static_mask;      // the static spheres' lanes take part in the row's pairs
   const real inv_eps = E.mod.rp->inv_epsilon, inv_eps_self = b.inv_epsilon_self;      // (formed once, on the host: RunParams)
   __builtin_amdgcn_s_setprio(PRIO_COST);
   if constexpr (GS16)
      cost_tile_gs16<real, GS16_U, BLOCK, KArg<real>, false, (KIND & 2) != 0, (KIND & 1) != 0, (KIND & 8) != 0>(b, E.mod, ts, te, do_iteration, E.T_s, E.Gc, E.pos_s, E.ax_s, E.srad_s, E.sinact_s, E.r2_s,
                                         E.slink_s, E.jtype_s, E.jcol_s, inv_eps, inv_eps_self, cost_lane, tid);
   else if constexpr ((KIND & 16) != 0)
   {
      // 17 .. 32 active spheres on a chain: the dense pair list (KIND 16; 16 | 2 | 8: one field with the world's axes, a fixed
      // base, no inactive sphere left for the loop over them)
      if constexpr ((KIND & 2) != 0) E.mod.floating = 0;
      cost_tile_pairs<real, BLOCK, KArg<real>, (KIND & 2) != 0, (KIND & 8) != 0>(b, E.mod, ts, te, do_iteration, E.T_s, E.Gc, E.pos_s, E.ax_s, E.srad_s, E.sinact_s,
                                         E.slink_s, E.pent_s, E.pgat_s, inv_eps, inv_eps_self, cost_lane, tid);
   }
   else
   {
#ifdef ORC_COST_TIMERS
      long long * gdbg = (blockIdx.x == 0 && threadIdx.x == 0) ? orc_cost_dbg : nullptr;
#else
      long long * gdbg = nullptr;
#endif
      cost_tile_generic<real, BLOCK>(b, E.mod, E.sdfs_s, ts, te, do_iteration, E.T_s, E.Gc, E.pos_s, E.ax_s, E.srad_s, E.sinact_s,
                                     E.slink_s, E.jtype_s, E.jcol_s, E.pstr, E.astr, inv_eps, inv_eps_self, cost_lane, gdbg, tid);
   }
   __syncthreads();
#ifdef ORC_COST_TIMERS
   if constexpr (!GS16 && (KIND & 16) == 0) if (threadIdx.x == 0 && blockIdx.x == 0 && ts > 0 && !do_iteration && te == b.m)
      printf("generic cost sections (cycles of wavefront 0 of run 0, whole launch): obstacle %lld inactive+pass1 %lld pass2 %lld jt %lld | pass-2 trips %lld fields used %lld wave passes %lld\n",
             orc_cost_dbg[0], orc_cost_dbg[1], orc_cost_dbg[2], orc_cost_dbg[3], orc_cost_dbg[4], orc_cost_dbg[5], orc_cost_dbg[6]);
   if constexpr (!GS16 && (KIND & 16) != 0) if (threadIdx.x == 0 && blockIdx.x == 0 && ts > 0 && !do_iteration && te == b.m)
      printf("pair-list cost sections (cycles of wavefront 0 of run 0, whole launch): setup %lld obstacle %lld self %lld jt %lld between %lld\n",
             orc_cost_dbg[0], orc_cost_dbg[1], orc_cost_dbg[2], orc_cost_dbg[3], orc_cost_dbg[4]);
   if constexpr (GS16) if (threadIdx.x == 0 && blockIdx.x == 0 && ts > 0 && !do_iteration)
      printf("cost sections (cycles of wavefront 0, whole launch): setup %lld obstacle %lld self %lld jt %lld between %lld\n",
             orc_cost_dbg[0], orc_cost_dbg[1], orc_cost_dbg[2], orc_cost_dbg[3], orc_cost_dbg[4]);
#endif
   phase_mark<real>(b, E, 1, marks<BLOCK>(tid));
   return cost_lane;
}
template <typename real, bool TREE, bool GS16, int BLOCK, int KIND = 0, bool ITER = true, int WGS = 0>
__device__ __attribute__((noinline)) double phase_cost(const void * kp, int ts_in, int te_in, double cost_lane)
{
   return phase_cost_body<real, TREE, GS16, BLOCK, KIND, ITER>(kp, ts_in, te_in, cost_lane);
}

// ---- update phase (cd_chomp_iterate, src/libcd/chomp.c:490-655): G/m + A T + B, A^-1 G, the step,
// the joint-limit rounds.  Returns the number of limit rounds made (1000: "ran too many joint limit fixes").
// Runs of the common kind (tridiagonal Toeplitz metric by the scan solve, at most 64 dofs, no debug read-back) take a copy of the update
// phase compiled without the other paths: fewer live scalars, fewer registers saved and restored per call.
// LEAN 1 / 2: the caller has checked solve_mode == 2, n <= 64, no lim_generic, no Gdbg, and no TSR constraint (1) or some (2) (the kernel's loop)
// The body is shared by phase_update and phase_update_costs (below): they form the kernarg reference, the LDS views and the
// logical thread index once and hand them in.
template <typename real, bool TREE, bool GS16, int BLOCK, int WGS = 0, int LEAN = 0>
__device__ __forceinline__ int phase_update_body(const void * kp, KArg<real> & b, const Env<real> & E, int tid, int it, int leapfrog_first)
{
   const int run = blockIdx.x;
   const int n = b.n, m = b.m, mn = m*n;
   const float rn_f = 1.0f / (float) n;        // for div_n
   double * red = E.red; int * redi = E.redi; unsigned int * colmask_s = E.colmask_s;
   real * T_s = E.T_u, * G_s = E.G_s, * Gc = E.Gc, * W_s = E.W_s, * jl_s = E.jl_s, * AG_g = E.AG_g, * AG_s = E.AG_s;
   const real * pcr_tab = E.pcr_tab;
   const bool staged = !b.t_in_lds && b.t_staged;
   if (staged)
   {
      // the trajectory lives in global memory (FK reads it there, larger tiles in exchange); this phase works on a copy in the
      // tile buffers, which are dead by now: one coalesced read here and one write at the end instead of stencils and
      // column scans through L2 (the preceding cost pass ended with a barrier)
      copy_batched<real, BLOCK>(T_s, E.traj_g, b.n_points*n, tid);
      __syncthreads();
   }

   __builtin_amdgcn_s_setprio(PRIO_UPDATE);
   if (tid < 2) colmask_s[tid] = 0u;       // read last after the previous step's barrier, set again after the next one
   // G = G/m + A T + B   (chomp.c:492, 515-522)
   const bool band = !LEAN && b.D != 1;      // (a metric that is not the tridiagonal Toeplitz one: its pass is a function of its own)
   if (band) band_gradient_pass<real, BLOCK>(kp, pcr_tab, T_s, Gc, G_s, tid);
   // (four entries of a thread per trip, their gradient rows read first: where the plan keeps the rows in global memory a plain
   // loop made one round trip through L2 per entry, eleven in a row for a 200-waypoint run of 14 dofs: BASELINE configs[3] +2 %;
   // for the three entries per thread of a 7 x 100 run it costs 0.7 %: those take the plain loop)
   const bool batched = mn > 4*BLOCK;      // (workgroup-uniform)
   if (band) {}
   else if (batched && !b.g_in_lds)
   for (int e0=tid; e0<mn; e0+=UPDATE_BATCH*BLOCK)
   {
      real gq[UPDATE_BATCH];
#pragma unroll
      for (int q=0; q<UPDATE_BATCH; q++) { const int e = e0 + q*BLOCK; gq[q] = (e < mn) ? Gc[e] : (real)0; }
#pragma unroll
      for (int q=0; q<UPDATE_BATCH; q++)
      {
         int e = e0 + q*BLOCK;
         if (e >= mn) break;
         // (the entry's index is opaque to the compiler from here on: it had split `q*BLOCK` off the index arithmetic into the
         // instructions' immediate offsets, T_s[c] = *(T_s + (e0 - i n) + q*BLOCK) -- a base BELOW the trajectory for the first
         // rows; these are FLAT accesses, whose aperture the hardware takes from the base alone: with the trajectory at the
         // start of LDS the base lay outside the LDS aperture and the access faulted (a 12-dof tree with derivative 2))
         __asm__ volatile("" : "+v"(e));
         const int i = div_n(e, rn_f), c = e - i*n;
         real g = gq[q];
         g *= b.inv_m;
         g += smooth_grad<real>(b, T_s, i, c);
         G_s[e] = g;
      }
   }
   else
   for (int e=tid; e<mn; e+=BLOCK)
   {
      const int i = div_n(e, rn_f), c = e - i*n;
      real g = Gc[e];
      g *= b.inv_m;
      g += smooth_grad<real>(b, T_s, i, c);
      G_s[e] = g;
   }
   __syncthreads();
   if (!LEAN && b.Gdbg)
      for (int e=tid; e<mn; e+=BLOCK) b.Gdbg[(size_t) run*mn + e] = G_s[e];
   // X = A^-1 G   (chomp.c:525-548)
   real * X = LEAN ? toeplitz_scan_solve<real, BLOCK>(b, G_s, tid) : metric_solve<real, BLOCK>(b, pcr_tab, G_s, W_s, tid);
   // T -= AG/lambda   (chomp.c:604-605)
   const real step = (real)(-1) / E.mod.rp->lambda;
   // the step also notes which columns left their limits (what the first scan of the
   // joint-limit loop would find, chomp.c:615-639): bit c of colmask_s
   unsigned long long viol = 0ull;
   if (LEAN == 2 || (LEAN == 0 && b.n_tsrs > 0))
   {
      // hard constraints (chomp.c:550-600): the unconstrained update AG is completed first, the
      // constraint step moves the trajectory itself, then T -= AG/lambda as always
      if (!b.use_momentum)
         for (int e=tid; e<mn; e+=BLOCK) AG_g[e] = X[e];
      else
      {
         const real sc = (leapfrog_first ? (real)0.5 : (real)1) / E.mod.rp->lambda;
         for (int e=tid; e<mn; e+=BLOCK) AG_s[e] = AG_s[e] + sc * X[e];
      }
      __threadfence_block();
      __syncthreads();
      phase_mark<real>(b, E, 3, marks<BLOCK>(tid));
      phase_tsr<real, GS16, BLOCK, WGS>(kp, tid);
      phase_mark<real>(b, E, 2, marks<BLOCK>(tid));      // (slot 2: the constraint step)
      const real * AGc = b.use_momentum ? AG_s : AG_g;
      for (int e=tid; e<mn; e+=BLOCK)
      {
         const real t = T_s[n + e] + step * AGc[e];
         T_s[n + e] = t;
         const int c = e - div_n(e, rn_f)*n;
         viol |= (t < jl_s[c] || t > jl_s[n+c]) ? (1ull << c) : 0ull;
      }
   }
   else if (!b.use_momentum)
   {
      // AG = X is not carried between iterations: keep only the last one (read-back state)
      // (with the convergence stop on, every iteration may be the run's last: AG is kept every time)
      const bool keep = (it == b.n_iter - 1) || (!LEAN && b.Gdbg != nullptr) || b.conv_patience != 0;
      for (int e=tid; e<mn; e+=BLOCK)
      {
         const real x = X[e];
         if (keep) AG_g[e] = x;
         const real t = T_s[n + e] + step * x;
         T_s[n + e] = t;
         const int c = e - div_n(e, rn_f)*n;
         viol |= (t < jl_s[c] || t > jl_s[n+c]) ? (1ull << c) : 0ull;
      }
   }
   else
   {
      const real sc = (leapfrog_first ? (real)0.5 : (real)1) / E.mod.rp->lambda;
      // (the momentum rows likewise: read four entries ahead where they live in global memory)
      if (batched && !b.ag_in_lds)
      for (int e0=tid; e0<mn; e0+=UPDATE_BATCH*BLOCK)
      {
         real aq[UPDATE_BATCH];
#pragma unroll
         for (int q=0; q<UPDATE_BATCH; q++) { const int e = e0 + q*BLOCK; aq[q] = (e < mn) ? AG_s[e] : (real)0; }
#pragma unroll
         for (int q=0; q<UPDATE_BATCH; q++)
         {
            int e = e0 + q*BLOCK;
            if (e >= mn) break;
            __asm__ volatile("" : "+v"(e));      // (as above: no q*BLOCK in the immediate offset of a FLAT access)
            const real ag = aq[q] + sc * X[e];
            AG_s[e] = ag;
            const real t = T_s[n + e] + step * ag;
            T_s[n + e] = t;
            const int c = e - div_n(e, rn_f)*n;
            viol |= (t < jl_s[c] || t > jl_s[n+c]) ? (1ull << c) : 0ull;
         }
      }
      else
      for (int e=tid; e<mn; e+=BLOCK)
      {
         const real ag = AG_s[e] + sc * X[e];
         AG_s[e] = ag;
         const real t = T_s[n + e] + step * ag;
         T_s[n + e] = t;
         const int c = e - div_n(e, rn_f)*n;
         viol |= (t < jl_s[c] || t > jl_s[n+c]) ? (1ull << c) : 0ull;
      }
   }
   if (viol)
   {
      if ((unsigned int) viol) atomicOr(&colmask_s[0], (unsigned int) viol);
      if ((unsigned int)(viol >> 32)) atomicOr(&colmask_s[1], (unsigned int)(viol >> 32));
   }
   __syncthreads();
   phase_mark<real>(b, E, 3, marks<BLOCK>(tid));

   // joint-limit projection (chomp.c:608-655)
   int num_limadjs = 0;
   bool lim_done = false;
#ifdef ORC_ABLATE_LIM
   const unsigned long long viol_cols = 0ull;      // timing experiments: no joint-limit rounds
#else
   const unsigned long long viol_cols = ((unsigned long long) colmask_s[1] << 32) | colmask_s[0];      // workgroup-uniform
#endif
   if (LEAN || (b.solve_mode == 2 && n <= 64 && !b.lim_generic))
   {
      lim_done = true;
      if (viol_cols != 0ull)
      {
         // one wavefront makes all rounds (no barrier inside them), the others wait here
         if (tid < 64)
         {
            const real kinv = (real)(-1) / ((real)(m + 1) * b.a_off);      // 1/((m+1) ca), ca = -a_off
            constexpr int SH = (BLOCK == 512) ? 1 : (WGS ? 2 : 0);
            const bool few = __popcll(viol_cols) <= 2;      // (workgroup-uniform)
            const LimResult lr = (b.t_in_lds || staged)
               ? (few ? limit_rounds_call_small<real, SH>(T_s, G_s, jl_s, m, n, kinv, viol_cols) : limit_rounds_call<real, SH>(T_s, G_s, jl_s, m, n, kinv, viol_cols))
               : (few ? limit_rounds_call_global_small<real, SH>(T_s, G_s, jl_s, m, n, kinv, viol_cols) : limit_rounds_call_global<real, SH>(T_s, G_s, jl_s, m, n, kinv, viol_cols));
            if (b.phase_cycles && tid == 0) E.phc_s[7] += lr.kinds;
            if (tid == 0) redi[0] = lr.rounds;
         }
         __syncthreads();
         num_limadjs = redi[0];
         __syncthreads();             // redi is reused by the reductions below
      }
   }
   if (!LEAN && !lim_done && b.solve_mode == 3 && n <= 64 && !b.lim_generic)
   {
      // a higher derivative: the rounds by one wavefront, the band inverse through its generators (no barrier inside a round)
      lim_done = true;
      if (viol_cols != 0ull)
      {
         if (tid < 64)
         {
            constexpr int SH = (BLOCK == 512) ? 1 : (WGS ? 2 : 0);
            const double * U = (const double *) pcr_tab;
            const int r = limit_rounds_semisep_call<real, SH>(T_s, G_s, jl_s, m, n, b.ss_rank, U, U + b.ss_rank*m);
            if (tid == 0) redi[0] = r;
         }
         __syncthreads();
         num_limadjs = redi[0];
         __syncthreads();
      }
   }
   // (no column left its limits in the step: the first scan of the loop would find nothing)
   if (!LEAN && !lim_done && (viol_cols != 0ull || b.lim_generic))
   for (; num_limadjs<1000; num_limadjs++)
   {
      real best = 0; int best_e = 0x7fffffff;
      for (int e=tid; e<mn; e+=BLOCK)
      {
         const int i = div_n(e, rn_f), c = e - i*n;
         const real t = T_s[n + e];
         real gj = 0;
         if (t < jl_s[c]) gj = jl_s[c] - t;
         if (t > jl_s[n+c]) gj = jl_s[n+c] - t;
         G_s[e] = gj;
         const real a = M<real>::fabs_(gj);
         if (a > best) { best = a; best_e = e; }
      }
      // workgroup arg-max, ties to the smallest index (first in row-major scan)
      wave_argmax(best, best_e);
      __syncthreads();
      if ((tid & 63) == 0) { red[tid >> 6] = (double) best; redi[tid >> 6] = best_e; }
      __syncthreads();
      double gb = red[0]; int ge = redi[0];
#pragma unroll
      for (int w=1; w<BLOCK/64; w++)
         if (red[w] > gb || (red[w] == gb && redi[w] < ge)) { gb = red[w]; ge = redi[w]; }
      if (gb == 0.0) break;                  // nothing violated anywhere in the workgroup
      const int gi = div_n(ge, rn_f), gc = ge - gi*n;
      const real gl = G_s[ge];               // Gjlimit[largest]

      // GA = A^-1 Gjlimit.  Gjlimit is sparse (a few violated entries): for the tridiagonal
      // Toeplitz metric (D == 1) the columns of A^-1 are known in closed form,
      //    Ainv[i][k] = (min(i,k)+1) (m - max(i,k)) / ((m+1) ca),   A = ca tridiag(-1,2,-1),
      // so GA is a short sum per element instead of a full solve.
      bool sparse_done = false;
      if (b.D == 1 && b.solve_mode != 1)
      {
         const int K = (mn + BLOCK - 1) / BLOCK;       // elements per thread
         int * cnt = (int *) W_s;                               // [K][waves] counts per (slice, wave)
         int * lst = cnt + 64;                                  // [64][2]  (row, column) of a violated entry
         real * lval = (real *)(lst + 128);                     // [64] its Gjlimit value
         const int lane = tid & 63, wave = tid >> 6;
         if (K * (BLOCK/64) <= 64)
         {
            for (int k=0; k<K; k++)
            {
               const int e = tid + k*BLOCK;
               const bool v = (e < mn) && (G_s[e] != (real)0);
               const unsigned long long mask = __ballot(v);
               if (lane == 0) cnt[k*(BLOCK/64) + wave] = __popcll(mask);
            }
            __syncthreads();
            int total = 0;
            for (int q=0; q<K*(BLOCK/64); q++) total += cnt[q];
            if (total <= 64)
            {
               for (int k=0; k<K; k++)
               {
                  const int e = tid + k*BLOCK;
                  const bool v = (e < mn) && (G_s[e] != (real)0);
                  const unsigned long long mask = __ballot(v);
                  if (v)
                  {
                     int off = 0;
                     for (int q=0; q<k*(BLOCK/64) + wave; q++) off += cnt[q];
                     off += __popcll(mask & ((1ull << lane) - 1ull));
                     const int i = div_n(e, rn_f);
                     lst[2*off] = i; lst[2*off+1] = e - i*n;
                     lval[off] = G_s[e];
                  }
               }
               __syncthreads();
               const real kinv = (real)(-1) / ((real)(m + 1) * b.a_off);     // 1/((m+1) ca), ca = -a_off
               // the entry the scale is taken from
               real ga_l = 0;
               for (int v=0; v<total; v++)
               {
                  const int iv = lst[2*v], cv = lst[2*v+1];
                  if (cv == gc)
                  {
                     const int lo = iv < gi ? iv : gi, hi = iv < gi ? gi : iv;
                     ga_l += lval[v] * (real)((lo + 1) * (m - hi));
                  }
               }
               const real sc = (real)1.01 * gl / (ga_l * kinv);
               for (int e=tid; e<mn; e+=BLOCK)
               {
                  const int i = div_n(e, rn_f), c = e - i*n;
                  real ga = 0;
                  for (int v=0; v<total; v++)
                  {
                     const int iv = lst[2*v], cv = lst[2*v+1];
                     if (cv == c)
                     {
                        const int lo = iv < i ? iv : i, hi = iv < i ? i : iv;
                        ga += lval[v] * (real)((lo + 1) * (m - hi));
                     }
                  }
                  T_s[n + e] += sc * (ga * kinv);
               }
               __syncthreads();
               sparse_done = true;
            }
         }
      }
      if (!sparse_done)
      {
         __syncthreads();
         real * GA = metric_solve<real, BLOCK>(b, pcr_tab, G_s, W_s, tid);
         const real sc = (real)1.01 * gl / GA[ge];
         __syncthreads();
         for (int e=tid; e<mn; e+=BLOCK) T_s[n + e] += sc * GA[e];
         __syncthreads();
      }
   }
   if (staged)
   {
      // the moving rows back to global memory (the end points do not move); every path above ended with a barrier
      copy_batched<real, BLOCK>(E.traj_g + n, T_s + n, mn, tid);
      __syncthreads();
   }
   phase_mark<real>(b, E, 4, marks<BLOCK>(tid));
   if (b.phase_cycles && tid == 0) E.phc_s[6] += num_limadjs;   // rounds (phc[7]: kinds of rounds, see LimResult)
   return num_limadjs;
}
template <typename real, bool TREE, bool GS16, int BLOCK, int WGS = 0, int LEAN = 0>
__device__ __attribute__((noinline)) int phase_update(const void * kp, int it_in, int leapfrog_first_in)
{
   KArg<real> & b = *uniform_kernarg<real>(kp);
   const int it = uni(it_in), leapfrog_first = uni(leapfrog_first_in);
   const Env<real> E = make_env<real, GS16>(b, orc_smem);
   const int tid = orc_tid<BLOCK>(b, it & 7);
   return phase_update_body<real, TREE, GS16, BLOCK, WGS, LEAN>(kp, b, E, tid, it, leapfrog_first);
}

// ---- the two costs of a pass: obstacle cost of the trajectory the gradient was taken at
// (chomp.c:484-491: the sum the cost phase left in the lanes, over m) and smoothness cost of the
// (updated) trajectory (chomp.c:660-677): 0.5 tr(T^T A T) + tr(B^T T) + trC, evaluated before the
// quaternion renormalisation of the same iteration, as in the reference (cd_chomp_iterate returns
// before mod.cpp:2806-2808 runs); then that renormalisation.
struct PassCosts { double obs, smooth; };
template <typename real, bool GS16, int BLOCK>
__device__ __forceinline__ PassCosts phase_costs_body(const void * kp, KArg<real> & b, const Env<real> & E, int tid, bool do_iteration, double cost_lane)
{
   const int n = b.n, m = b.m, np = b.n_points, mn = m*n;
   const float rn_f = 1.0f / (float) n;
   const real * T_s = E.T_u;
   const bool staged = !b.t_in_lds && b.t_staged;
   if (staged && !do_iteration)
   {
      // the cost-only pass that ends a call: no update phase has staged the trajectory
      copy_batched<real, BLOCK>(E.T_u, E.traj_g, np*n, tid);
      __syncthreads();
   }
   PassCosts pc;
   __builtin_amdgcn_s_setprio(PRIO_UPDATE);
   {
      double acc = 0.0;
      if (b.D != 1) acc = band_cost_pass<real, BLOCK>(kp, E.pcr_tab, T_s, tid);
      else
      for (int e=tid; e<mn; e+=BLOCK)
      {
         const int i = div_n(e, rn_f), c = e - i*n;
         // (A T + B) as smooth_grad forms it, but in double whatever `real` is (the same bits in fp64): this sum weighs the row's rounding
         // by T itself, not by a change of T, and in float the second difference is rounded at a |T| 2^-24 -- 3e-6 of the smoothness cost
         // of a 34-waypoint fp32 run, 20-40 x what the float rounding of its waypoints moves it (NOTES/first-iteration.md); a product of two
         // floats is exact in double.  A higher derivative's band_cost_pass does the same.
         const double sg = (double) b.a_diag * (double) T_s[(i+1)*n + c] + (double) b.a_off * ((double) T_s[i*n + c] + (double) T_s[(i+2)*n + c]);
         const double bt = (double) b.a_off * ((i == 0 ? (double) T_s[c] : 0.0) + (i == m-1 ? (double) T_s[(np-1)*n + c] : 0.0));
         acc += (double) T_s[n + e] * (0.5 * (sg + bt));
      }
      double ss = 0.0, sg2 = 0.0, gg = 0.0;
      if (tid < n)
      {
         const double s0 = (double) T_s[tid], g0 = (double) T_s[(np-1)*n + tid];
         ss = s0*s0; sg2 = s0*g0; gg = g0*g0;
      }
      acc += 0.5 * (b.kss*ss + 2.0*b.ksg*sg2 + b.kgg*gg);
      // both sums through one pair of barriers
      const double a = wave_sum(cost_lane), c2 = wave_sum(acc);
      __syncthreads();
      if ((tid & 63) == 0) { E.red[tid >> 6] = a; E.red[8 + (tid >> 6)] = c2; }
      __syncthreads();
      pc.obs = sum_partials<BLOCK>(E.red);
      pc.smooth = sum_partials<BLOCK>(E.red + 8);
      pc.obs /= (double) m;
   }
   phase_mark<real>(b, E, 5, marks<BLOCK>(tid));

   // start_tsr: the row in front of the start point follows the point after it (see phase_setup)
   if (do_iteration && b.free_start)
   {
      real * Tw = E.T_s;
      if (tid < n) Tw[tid] = Tw[2*n + tid];
      __syncthreads();
   }
   // floating base: renormalise the quaternion of every row (mod.cpp:2806-2808)
   if (do_iteration && E.mod.floating)
   {
      real * Tw = E.T_u;
      for (int w=tid; w<np; w+=BLOCK)
      {
         real * row = Tw + w*n;
         const real len = M<real>::sqrt_(row[3]*row[3] + row[4]*row[4] + row[5]*row[5] + row[6]*row[6]);
         const real inv = (real)1 / len;
         row[3] *= inv; row[4] *= inv; row[5] *= inv; row[6] *= inv;
         if (staged) { real * g = E.traj_g + w*n; g[3] = row[3]; g[4] = row[4]; g[5] = row[5]; g[6] = row[6]; }      // (the copy's rows go back where FK reads them)
      }
      __syncthreads();
   }
   if (b.conv_patience && do_iteration) conv_step<real>(b, pc.obs, pc.smooth, tid);
   return pc;
}
// the cost-only pass that ends a call (do_iteration == false: no update in front of it, it stages the trajectory itself), and the
// second of the two calls of the general update mode, which is not fused
template <typename real, bool GS16, int BLOCK, int WGS = 0>
__device__ __attribute__((noinline)) PassCosts phase_costs(const void * kp, int do_iteration_in, double cost_lane)
{
   KArg<real> & b = *uniform_kernarg<real>(kp);
   const bool do_iteration = packed_arg(uni(do_iteration_in)) != 0;
   const Env<real> E = make_env<real, GS16>(b, orc_smem);
   const int tid = orc_tid<BLOCK>(b, packed_it(uni(do_iteration_in)));
   return phase_costs_body<real, GS16, BLOCK>(kp, b, E, tid, do_iteration, cost_lane);
}

// ---- update and costs of an iteration in one call: both run on every wavefront, one straight after the other, on the same (staged)
// trajectory, so the second call's register saves, kernarg reference, LDS views and thread index are saved.  The costs part is
// not made when the limit rounds gave up (chomp.c:651-655: the caller sets status -1 and leaves the loop) ----
struct UpdateCosts { double obs, smooth; int num_limadjs; };
template <typename real, bool TREE, bool GS16, int BLOCK, int WGS = 0, int LEAN = 0>
__device__ __attribute__((noinline)) UpdateCosts phase_update_costs(const void * kp, int it_in, int leapfrog_first_in, double cost_lane)
{
   KArg<real> & b = *uniform_kernarg<real>(kp);
   const int it = uni(it_in), leapfrog_first = uni(leapfrog_first_in);
   const Env<real> E = make_env<real, GS16>(b, orc_smem);
   const int tid = orc_tid<BLOCK>(b, it & 7);
   UpdateCosts uc;
   uc.obs = 0.0; uc.smooth = 0.0;
   uc.num_limadjs = uni(phase_update_body<real, TREE, GS16, BLOCK, WGS, LEAN>(kp, b, E, tid, it, leapfrog_first));
   if (uc.num_limadjs < 1000)
   {
      const PassCosts pc = phase_costs_body<real, GS16, BLOCK>(kp, b, E, tid, true, cost_lane);
      uc.obs = pc.obs; uc.smooth = pc.smooth;
   }
   return uc;
}

// ---- write back: trajectory, momentum, costs, status ----
template <typename real, bool GS16, int BLOCK, int WGS = 0>
__device__ __attribute__((noinline)) void phase_finish(const void * kp, int status_in, int iters_done_in, int leapfrog_first_in, int have_costs_in,
   double done_obs, double done_smooth)
{
   KArg<real> & b = *uniform_kernarg<real>(kp);
   int status = uni(status_in);
   const int iters_done = uni(iters_done_in), leapfrog_first = uni(leapfrog_first_in), have_costs = uni(have_costs_in);
   const Env<real> E = make_env<real, GS16>(b, orc_smem);
   const int run = blockIdx.x, tid = orc_tid<BLOCK>(b, 0);      // (after the last iteration's barrier: any rotation serves)
   const int n = b.n, m = b.m, np = b.n_points, mn = m*n;
   __syncthreads();
   // a run the convergence stop ended (in this launch, or in an earlier one of the call) reports status 1
   if (b.conv_patience)
   {
      const ConvState * cs = conv_state();
      if (status == 0 && uni(cs->streak) >= b.conv_patience) status = 1;
      if (tid == 0) { b.conv_prev[run] = cs->prev; b.conv_streak[run] = cs->streak; }
   }
   if (b.t_in_lds)
   {
      const int skip = b.free_start ? n : 0;
      for (int e=skip+tid; e<np*n; e+=BLOCK) E.traj_g[e - skip] = E.T_s[e];
   }
   if (b.use_momentum && b.ag_in_lds) for (int e=tid; e<mn; e+=BLOCK) E.AG_g[e] = E.AG_s[e];
   if (tid == 0)
   {
      if (b.phase_cycles) for (int k=0; k<8; k++) b.phase_cycles[(size_t) run*8 + k] = E.phc_s[k];
      // an aborted run reports the costs of its last complete pass (none in this launch: what it had)
      if (have_costs)
      {
         b.costs[(size_t) run*3 + 0] = done_obs + done_smooth;
         b.costs[(size_t) run*3 + 1] = done_obs;
         b.costs[(size_t) run*3 + 2] = done_smooth;
      }
      b.status[run] = status;
      b.iters_done[run] = (b.carry_status ? b.iters_done[run] : 0) + iters_done;
      b.leapfrog_first[run] = leapfrog_first;
   }
   // the iterations an aborted run did not make have no log line in the reference: NaN rows
   if (b.trace && status != 0)
      for (int e=iters_done*3 + tid; e<b.n_iter*3; e+=BLOCK)
         b.trace[(size_t) run * b.n_iter * 3 + e] = __longlong_as_double(0x7ff8000000000000LL);
}

// ---------------------------------------------------------------------------
// The kernel: one workgroup = one run for all iterations of the launch; the loop below only
// sequences the phase functions and carries the few scalars that cross iterations.
// second argument of the launch bounds: wavefronts per SIMD = the register budget of the family (kernel_table.h waves_per_simd)
template <typename real, bool TREE, bool GS16, int BLOCK, int KIND = 0, int WGS = 0>      // WGS: 0 the family's own budget, 4: four workgroups of 256 per CU (128 VGPRs)
__global__ __launch_bounds__(BLOCK, (WGS ? WGS : orc::waves_per_simd(sizeof(real), GS16, BLOCK)))
void chomp_iterate_kernel(const DevBatch<real> b)
{
   const void * kp = (const void *) __builtin_amdgcn_kernarg_segment_ptr();      // DevBatch b is the kernel's only argument
   const int run = blockIdx.x;

   // a launch that continues an iterate call: the run left its joint limits in an earlier launch of the call, the
   // reference has thrown out of the call by now (workgroup-uniform).  A run that converged in an earlier launch of the
   // call (status 1) makes no more iterations, but takes the call's final cost-only pass (n_iter == 0)
   if (b.carry_status && b.status[run] != 0 && (b.status[run] != 1 || b.n_iter != 0)) return;

   phase_setup<real, TREE, GS16, BLOCK, WGS>(kp);

   int leapfrog_first = uni(b.leapfrog_first[run]);      // (the loop's state is wave-uniform: said so, it lives in scalar registers across the phase calls instead of being spilled around them)
   // every iterate call starts afresh: the reference throws out of the call in which a run leaves
   // its joint limits, the run itself stays usable (src/orcdchomp_mod.cpp:2799-2803)
   int status = 0;
   int next_resample = 0;      // index into this call's resample list

   // co-resident workgroups that start in lockstep stay in lockstep (all in the one-wave FK phase
   // together, then all in the cost phase): delaying every other one interleaves their phases
   if (b.stagger_mode && b.stagger_mode != 9)
   {
      const bool late = (b.stagger_mode == 1) ? (blockIdx.x & 1) : ((blockIdx.x >> 8) & 1);
      if (late) for (int k=0; k<b.stagger_sleeps; k++) __builtin_amdgcn_s_sleep(127);
   }

   // costs of the last pass that ran to its end, and the iterations completed by this launch
   double done_obs = 0.0, done_smooth = 0.0;
   int have_costs = 0;
   int iters_done = 0;

   // The loop carries across the phase calls only what crosses iterations (kp, it, tk, status, leapfrog_first, next_resample,
   // iters_done, have_costs, done_obs, done_smooth, cost_lane).  Every field of the kernarg block it tests is read where it is
   // tested, through a reference formed anew after each call (fresh_kernarg: the compiler cannot tell it from a new address, so it
   // keeps no field alive across a call -- a scalar load from the scalar cache instead of a register carried through VGPR lanes
   // around every call; this target has no scalar spill to memory)
   KArg<real> * bp = fresh_kernarg<real>(kp);
   for (int it=0; it<bp->n_iter + (bp->final_eval ? 1 : 0); it++)
   {
      bp = fresh_kernarg<real>(kp);
      const bool do_iteration = (it < bp->n_iter);
      // the convergence stop (orc_batch_set_convergence): phase_costs raised the flag after the run's last complete
      // iteration; its remaining iterations are passed over, on to the final cost-only pass, so that the run ends exactly
      // where a call of that many iterations leaves it.  (Passing over rather than leaving the loop: a loop exit or a jump
      // of `it` costs the headline kernel 16 bytes of scratch, this an LDS read per iteration)
      if (do_iteration && uni(conv_state()->stop)) continue;

      // ---- hmc momentum resample (src/orcdchomp_mod.cpp:2755-2768) ----------
      if (do_iteration && bp->use_hmc && bp->use_momentum && next_resample < bp->max_resamples
          && bp->hmc_iters[(size_t) run * bp->max_resamples + next_resample] == it)
      {
         phase_hmc<real, GS16, BLOCK, WGS>(kp, pack_it(next_resample, it));
         leapfrog_first = 1;
         next_resample++;
      }

      double cost_lane = 0.0;
      for (int tk=0; ; tk++)
      {
         bp = fresh_kernarg<real>(kp);
         if (!(tk < bp->n_tiles)) break;
         const int ts = (tk == 0) ? 0 : bp->tile_first + (tk - 1) * bp->tile_rest;
         const int te = (tk == bp->n_tiles - 1) ? bp->m : bp->tile_first + tk * bp->tile_rest;
         // (the tile's end as the phases take it, with the iteration's bits for their rotation: formed here, behind an empty asm,
         // so that no part of it is a loop invariant the compiler would carry across the calls)
         int itv = it;
         __asm__ volatile("" : "+s"(itv));
         const int tep = pack_it(te, itv);
         // ORC_STAGGER_MODE=9 (a timing experiment, wrong results): only the first tile is walked and a pause stands in for a
         // barrier across workgroups -- what an iteration of ONE run would take with its tiles on as many CUs
         // (scripts/single_run_latency.py, profiles/r04_single_run_ceiling.txt)
         if (bp->stagger_mode == 9 && tk > 0) { if (tk == 1) for (int k=0; k<bp->stagger_sleeps; k++) __builtin_amdgcn_s_sleep(10); continue; }
#ifndef ORC_ABLATE_FK
         // a wavefront without a waypoint in the tile (20 per wavefront: the second of a 128-thread workgroup in each of its tiles of 14)
         // only joins the phase's barrier: it saves the call's ~120 scalar registers moved through the vector pipe
         // (the FK groups go to the last logical wavefronts, wave_roles.h: it is the first ones that have nothing to walk.  Without a
         // rotation the logical wavefront is the hardware's; under ORC_WAVE_ROTATE every wavefront makes the call and the idle ones
         // find nothing to walk inside it: forming the rotation here cost the kernel function a spilled register)
         if (!bp->ms.fk_split && !bp->wave_rotate && orc::fk_wave_idle(uni((int)(threadIdx.x >> 6)), BLOCK, 1, te - ts + 2)) __syncthreads();
         else phase_fk<real, TREE, GS16, BLOCK, WGS>(kp, ts, tep);      // (skipping the call for the wavefronts without a waypoint in the tile -- their share of the callee-saved registers -- measured nothing: profiles/r04_ab_experiments.txt)
#ifdef ORC_ABLATE_FKTWICE      // timing experiments: the FK phase twice (what a 2x slower FK would cost)
         phase_fk<real, TREE, GS16, BLOCK, WGS>(kp, ts, tep);
#endif
#endif
#ifndef ORC_ABLATE_COST
         // the pass of an iteration inside the kernel function itself: a kernel has no callee-saved registers to
         // preserve (as a call the many-sphere pass saved and restored 67 of them per tile and wavefront: 2 x 198 GB
         // of scratch traffic per launch of BASELINE configs[4], most of what the HBM counters saw)
         // The 16-lane pass and the FK phase stay calls: inside the kernel function they measured slower (the FK phase's hoisted loop
         // invariants spill to scratch; profiles/r04_ab_experiments.txt, profiles/r05_ab_experiments.txt)
         if (do_iteration && !GS16) cost_lane = phase_cost_body<real, TREE, GS16, BLOCK, KIND, true>(kp, ts, tep, cost_lane);
         else
         cost_lane = do_iteration ? phase_cost<real, TREE, GS16, BLOCK, KIND, true, WGS>(kp, ts, tep, cost_lane)
                                  : phase_cost<real, TREE, GS16, BLOCK, KIND, false, WGS>(kp, ts, tep, cost_lane);
         bp = fresh_kernarg<real>(kp);
         if (tk == 0 && bp->free_start) cost_lane = phase_cost_start<real, TREE, GS16, BLOCK, WGS>(kp, pack_it(do_iteration ? 1 : 0, it), cost_lane);
#endif
      } // tiles

      // update and costs of an iteration in one call (phase_update_costs) for the two lean update modes.  The general mode keeps
      // its two calls: fused, its frame is larger than the update's alone (NOTES/call-overhead.md), and that frame lies on the
      // deepest call chain of the kernel.  The cost-only pass that ends a call has no update in front of it
      PassCosts pc;
      bp = fresh_kernarg<real>(kp);
      const bool lean = bp->solve_mode == 2 && bp->n <= 64 && !bp->lim_generic && bp->Gdbg == nullptr;      // (workgroup-uniform)
      if (do_iteration)
      {
         int num_limadjs;
         if (!lean) num_limadjs = uni(phase_update<real, TREE, GS16, BLOCK, WGS, 0>(kp, it, leapfrog_first));
         else
         {
            const UpdateCosts uc = (bp->n_tsrs == 0) ? phase_update_costs<real, TREE, GS16, BLOCK, WGS, 1>(kp, it, leapfrog_first, cost_lane)
                                                     : phase_update_costs<real, TREE, GS16, BLOCK, WGS, 2>(kp, it, leapfrog_first, cost_lane);
            num_limadjs = uni(uc.num_limadjs);
            pc.obs = uc.obs; pc.smooth = uc.smooth;
         }
         bp = fresh_kernarg<real>(kp);
         if (bp->use_momentum) leapfrog_first = 0;
         // "ran too many joint limit fixes! aborting ..." (chomp.c:651-655): cd_chomp_iterate returns
         // before the smoothness cost, mod::iterate throws before the quaternion renormalisation and
         // the log line; the trajectory keeps what the limit rounds made of it (workgroup-uniform)
         if (!(num_limadjs < 1000)) { status = -1; break; }
      }
      if (!do_iteration || !lean)
      {
         pc = phase_costs<real, GS16, BLOCK, WGS>(kp, pack_it(do_iteration ? 1 : 0, it), cost_lane);
         bp = fresh_kernarg<real>(kp);
      }
      pc.obs = unir(pc.obs); pc.smooth = unir(pc.smooth);

      if (threadIdx.x == 0 && bp->trace && do_iteration)      // (wave-uniform values: any one thread)
      {
         double * tr = bp->trace + ((size_t) run * bp->n_iter + it) * 3;
         tr[0] = pc.obs + pc.smooth; tr[1] = pc.obs; tr[2] = pc.smooth;
      }
      done_obs = pc.obs; done_smooth = pc.smooth; have_costs = 1;
      if (do_iteration) iters_done++;

   }

   phase_finish<real, GS16, BLOCK, WGS>(kp, status, iters_done, leapfrog_first, have_costs, done_obs, done_smooth);
}

// straight-line seeding of every run (src/orcdchomp_mod.cpp:2417-2464):
// traj[i][j] = s_j + (g_j - s_j) * i / (n_points-1), rows 0 and n_points-1 included,
// then quaternion normalisation per row when floating.
template <typename real>
__global__ void seed_traj_kernel(real * traj, const double * starts, const double * goals,
   int n_runs, int n_points, int n, int floating)
{
   const long total = (long) n_runs * n_points;
   for (long idx = blockIdx.x * (long) blockDim.x + threadIdx.x; idx < total; idx += (long) gridDim.x * blockDim.x)
   {
      const int run = (int)(idx / n_points);
      const int i = (int)(idx - (long) run * n_points);
      double row[ORC_MAX_JOINTS + 7];
      for (int j=0; j<n; j++)
      {
         const double s = starts[(size_t) run*n + j];
         const double g = goals[(size_t) run*n + j];
         row[j] = s + (g - s) * i / (n_points - 1);
      }
      if (floating)
      {
         // the sum of squares as written (no fused multiply-add: the rows of a seed are compared bit for bit)
         const double len = ::sqrt(__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(row[3], row[3]), __dmul_rn(row[4], row[4])), __dmul_rn(row[5], row[5])), __dmul_rn(row[6], row[6])));
         const double inv = 1.0 / len;
         row[3] *= inv; row[4] *= inv; row[5] *= inv; row[6] *= inv;
      }
      for (int j=0; j<n; j++) traj[((size_t) run * n_points + i) * n + j] = (real) row[j];
   }
}

} // namespace

// ---------------------------------------------------------------------------
// host-side launch wrappers (launch.h)
template <typename real, bool TREE, bool GS16, int BLOCK, int KIND = 0, int WGS = 0>
static hipError_t launch_iterate_tt(const DevBatch<real> & b, size_t lds, hipStream_t stream)
{
   // the attribute is per device (and per kernel instantiation)
   static std::atomic<unsigned long long> attr_set{0ull};
   int dev = 0;
   if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;
   if (!((attr_set.load() >> dev) & 1ull))
   {
      hipError_t e = hipFuncSetAttribute((const void *) chomp_iterate_kernel<real, TREE, GS16, BLOCK, KIND, WGS>,
         hipFuncAttributeMaxDynamicSharedMemorySize, 160*1024 - 256);
      if (e != hipSuccess) return e;
      attr_set.fetch_or(1ull << dev);
   }
   hipLaunchKernelGGL((chomp_iterate_kernel<real, TREE, GS16, BLOCK, KIND, WGS>), dim3(b.n_runs), dim3(BLOCK), lds, stream, b);
   return hipGetLastError();
}

// The row of kernel_table.h that the plan names (its variant mask -- the ORC_VAR_ bits of dev_types.h --, its block size, the
// precision) launches; a plan that names no row of this build is refused.
template <typename real>
static hipError_t launch_iterate_t(const DevBatch<real> & b, size_t lds, hipStream_t stream, int variant, int block)
{
   const orc::KernelKey key = orc::kernel_of(variant, block, (int) sizeof(real));
#define ORC_LAUNCH_ROW(BYTES, TREE, GS16, BLOCK, KIND, WGS) \
   if constexpr (sizeof(real) == BYTES && orc::kernel_compiled(orc::KernelKey{ BYTES, TREE, GS16, BLOCK, KIND, WGS })) \
      if (key == orc::KernelKey{ BYTES, TREE, GS16, BLOCK, KIND, WGS }) return launch_iterate_tt<real, TREE, GS16, BLOCK, KIND, WGS>(b, lds, stream);
   ORC_ITERATE_KERNELS(ORC_LAUNCH_ROW)
#undef ORC_LAUNCH_ROW
   return hipErrorInvalidValue;
}

hipError_t orc_launch_iterate(const DevBatch<double> & b, size_t lds, hipStream_t stream, int variant, int block)
{ return launch_iterate_t<double>(b, lds, stream, variant, block); }
hipError_t orc_launch_iterate(const DevBatch<float> & b, size_t lds, hipStream_t stream, int variant, int block)
{ return launch_iterate_t<float>(b, lds, stream, variant, block); }

template <typename real>
hipError_t orc_launch_seed(real * traj, const double * starts, const double * goals, int n_runs, int n_points, int n, int floating, hipStream_t stream)
{
   const long total = (long) n_runs * n_points;
   int blocks = (int)((total + 255) / 256); if (blocks > 4096) blocks = 4096; if (blocks < 1) blocks = 1;
   hipLaunchKernelGGL(seed_traj_kernel<real>, dim3(blocks), dim3(256), 0, stream, traj, starts, goals, n_runs, n_points, n, floating);
   return hipGetLastError();
}
template hipError_t orc_launch_seed<double>(double *, const double *, const double *, int, int, int, int, hipStream_t);
template hipError_t orc_launch_seed<float>(float *, const double *, const double *, int, int, int, int, hipStream_t);
