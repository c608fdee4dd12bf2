// stages.h -- `create` of a batch, stage by stage: pure host functions over plain structs.
//
// BatchShard::construct (batch.cpp) reads the switches once, calls the stages in this order, uploads what they
// return and keeps their results:  fold_joint_tree -> fold_robot -> fold_tsrs -> fold_scenes -> pack_metric ->
// plan_iterate  (fold.cpp, plan.cpp).  None of them touches the device; what one stage needs of another it gets by value.
#pragma once
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "dev_types.h"
#include "wave_roles.h"
#include "host_math.h"

namespace orc {

struct Robot                      // what the path reads from an OpenRAVE::RobotBase
{
   std::string name;
   int n_links = 0;
   std::vector<int> parent;
   std::vector<Pose> pose_parent_joint;
   std::vector<int> joint_type;
   std::vector<double> axis;      // [n_links][3]
   std::vector<int> dof_index;
   int n_dof = 0;
   std::vector<double> limit_lower, limit_upper;
   std::vector<double> limit_vel;   // GetDOFVelocityLimits, used by the retimer of gettraj (default 1)
   struct Sphere { int link; double pos[3]; double radius; int body = 0; };   // struct sphere, src/orcdchomp_kdata.h:33-39; body: 0 the robot's own, 1 + k a sphere of the k-th grabbed body (robot_for_run)
   std::vector<Sphere> spheres;   // XML order
   // what the TSR constraints address (`con_tsr 'all link NAME'`, `'all manipee NAME'`, src/orcdchomp_mod.cpp:1957-1976)
   std::vector<std::string> link_names;        // GetLink(name); empty: links are addressed as "link<i>"
   struct Manip { std::string name; int link; Pose tool; };   // GetEndEffectorTransform = link transform o tool
   std::vector<Manip> manips;
   int active_manip = 0;                       // GetActiveManipulator
   std::vector<std::pair<int, int>> adjacent;  // link pairs the robot description declares adjacent (<adjacent> tags)
   bool self_check = true;                     // the sphere-pair stand-in for CheckSelfCollision in gettraj's re-check (orc_robot_set_self_check)
   // kinbodies the robot holds, in the order they were grabbed (RobotBase::Grab / GetGrabbed, src/orcdchomp_mod.cpp:2168-2171):
   // the body is rigid with `link` from the moment of the grab, `rel` = T_w_link^-1 o T_w_body at that moment
   // touch_link / touch_body: what the body's spheres overlapped AT THE MOMENT OF THE GRAB (Environment::grab; taken anew when
   // set_kinbody_transform re-anchors it): links of the robot, by its own spheres, and bodies the robot held already.
   // OpenRAVE's CheckSelfCollision leaves a grabbed body out against exactly those (and against the grabbing link).
   struct Grab { std::string body; int link; Xform rel; std::vector<unsigned char> touch_link; std::vector<std::string> touch_body; };
   std::vector<Grab> grabbed;
   // state
   Pose transform;
   std::vector<double> dof_values;
   std::vector<int> active_dofs;
   bool does_affect(int dof, int link) const;
   // link pairs a self-collision check skips [n_links][n_links]: the same link, parent and child, the pairs the robot
   // description declares adjacent, and links whose spheres already overlap with all dofs at zero (KinBody computes
   // its non-adjacent links from the initial configuration the same way)
   std::vector<unsigned char> self_pairs_excluded() const;
   // ... sphere by sphere for a run's list (the robot's spheres, then those of the bodies it holds, `spheres` as robot_for_run
   // leaves them, the robot in the configuration of `create`): [n][n], 1 = the pair is never tested
   std::vector<unsigned char> run_self_pairs_excluded(int n_own) const;
   // world frames of all links for the given state
   void fk(const Pose & base, const std::vector<double> & q, std::vector<Xform> & frames) const;
};

struct Sdf                        // struct sdf, src/orcdchomp_mod.cpp:148-153
{
   std::string kinbody_name;
   Pose pose;                     // grid wrt kinbody frame
   Grid grid;
   // device copies per device ordinal, created on demand; batches that read a copy share its
   // ownership, so removefield while a run exists does not pull the cells from under it
   std::map<int, std::shared_ptr<void>> dev64, dev32;
};

// The obstacles of a batch's runs (orc_batch_create_scenes): scenes of at most ORC_MAX_SDFS field placements, every run
// in one of them.  orc_batch_create is the one-scene case: the module's fields where their kinbodies stand, every run in
// scene 0 (Environment::current_scene).
struct ScenePlacement
{
   std::shared_ptr<Sdf> sdf;      // the module's field (shared: removefield does not pull it from under a batch)
   Pose pose_world_kinbody;       // where its kinbody stands for this scene: the field is at pose_world_kinbody o sdf->pose
};
struct SceneTable
{
   std::vector<std::vector<ScenePlacement>> scenes;   // in the order of the best-of-N loop: a tie goes to the earlier field
   std::vector<int> scene_of_run;                     // [n_runs]
   int max_fields() const;                            // fields of the largest scene
};

// a TSR hard constraint on every moving point (`con_tsr all ...` or `everyn_tsr`; struct tsr,
// src/orcdchomp_mod.h:80-87, struct run_contsr, src/orcdchomp_mod.cpp:873-885)
struct TsrSpec
{
   int ee_link = -1;
   Pose tool;                 // end effector in the link frame (identity for `link NAME`)
   Pose T0w, Twe;
   double Bw[6][2];
   int point = -1;            // -1: every moving point (`con_tsr all`, `everyn_tsr`); >= 0: that moving point only (`start_tsr`: 0)
};

struct BatchParams
{
   std::vector<TsrSpec> tsrs; // in the reference's order of addition: start_tsr, everyn_tsr, then the con_tsrs (mod.cpp:2570-2612)
   int free_start = 0;        // `start_tsr`: the start point is a variable (m = n_points - 1, no start boundary in the metric)
   int n_points = 101;
   int floating_base = 0;
   double lambda = 10.0;
   int derivative = 1;
   int use_momentum = 0;
   int use_hmc = 0;
   double hmc_resample_lambda = 0.02;
   double epsilon = 0.1, epsilon_self = 0.04, obs_factor = 200.0, obs_factor_self = 10.0;
   int precision = 64;
   int workgroup_threads = 0;   // 0: the module's setting (orc_set_workgroup_threads); `create` asks for 512 for its single run
   int workgroups_per_cu = 0;   // 0: the module's setting (orc_set_workgroups_per_cu)
};

// The ORC_* diagnostics switches of the environment (NOTES/switches.md), read once per `create` (BatchShard::construct)
// and handed to the stages; a shard's later calls go by what its `create` read.  (`hmc_room` and `hmc_plan_sync` alone are
// a call's: HmcPlanner::plan reads them again, the overflow test sets ORC_HMC_ROOM between `create` and `iterate`.)
struct Switches
{
   struct Int { bool set = false; int value = 0; };      // a switch with a number: is it set, and atoi of its text
   bool debug_plan = false, phase_timers = false, debug_state = false, hmc_device = false, hmc_host = false, hmc_plan_sync = false;
   bool no_jt_scan = false, no_placement = false, no_static_lanes = false, pairs_chain64_only = false, no_pairs = false;
   bool no_kind = false, no_fk_split = false, no_semisep = false, no_scan_solve = false, pcr_full = false, no_short128 = false;
   bool no_band_toeplitz = false, tsr_dense = false;
   bool t_staged_off = false;                             // ORC_T_STAGED=0
   int lim_generic = 0, stagger_mode = 0, stagger_sleeps = 10, scan_max_m = 1 << 30, wgs128 = 8;
   int wave_rotate = 0;      // ORC_WAVE_ROTATE (wave_roles.h): rotation of the logical thread index; values outside 0 .. WAVE_ROTATE_MAX are refused at create
   Int block_threads, tile_m, pcr_lds, ag_lds, wgs, g_lds, t_lds, hmc_room;
   static Switches read();
};

// ---- the robot -----------------------------------------------------------------------------------------------------
// The optimized joints (links whose joint moves with an active dof) as a tree, walked depth first with save / load slots
// for the branch points' frames.
struct JointTree
{
   std::vector<int> jlink, jcol;              // link and optimizer column of optimized joint k
   std::vector<int> link2joint;               // optimized joint of a link, -1: none
   std::vector<int> jparent;                  // nearest optimized joint above k, -1: the base
   std::vector<std::vector<int>> children;    // ... in the order they are walked (the subtree that needs the most slots last)
   std::vector<int> roots;
   std::vector<int> order, pos_in_order;      // the walk: joint at position p; position of joint k
   std::vector<int> load_slot, save_slot;     // per joint: -2 a root, -1 the frame just computed / nothing to save, else the slot
   std::vector<Mat3> canon;                   // per joint: its canonical rotation C, C e_z = axis (below); built once with the tree
   int nj() const { return (int) jlink.size(); }
   // C of optimized joint k; the identity for -1 (the base, fixed or floating)
   const Mat3 & canonical(int k) const;
   // nearest optimized-joint ancestor-or-self of a link (-1: rigid with the base)
   int attach_of(const Robot & robot, int link) const;
};
JointTree fold_joint_tree(const Robot & robot, bool floating_base);
// The canonical form of a joint's moved frame: F' = F C with the constant rotation C, C e_z = axis, so that the FK walk turns
// every joint about z (fk.h).  A signed permutation for +- a coordinate axis (the fold's products then stay exact), else built
// in extended precision, orthonormal to rounding, the free turn about z fixed by the axis alone.
Mat3 canonical_rotation(const double axis[3]);
// frozen local transforms of the robot's current configuration.  Everything that is folded into the device model is a
// product of link-local transforms, so no frame is ever inverted (the base rotation need not be orthonormal)
Xform local_moved(const Robot & robot, int li);
// joint frame of link li (before its own motion) relative to the moved frame of link `from_link` (-1: the base frame);
// every joint in between is frozen
Xform fixed_between(const Robot & robot, int from_link, int li);
// a point of link `li` expressed in the moved frame of link `from_link` (-1: base)
void point_in(const Robot & robot, int from_link, int li, const double * pin, double * pout);

// lane placement of a robot's active spheres (place_spheres_on_row): a pure function of the robot (geometry, limits,
// frozen dof values), the active dofs, floating base and epsilon_self -- kept by the module, shared by the shards
struct PlacementCache { std::map<std::string, std::vector<int>> & placed; std::recursive_mutex & mutex; };
// the key holds everything the placement is a function of (the frozen dofs by their bit patterns)
std::string placement_key(const Robot & robot, const BatchParams & params, int n_static);

template <typename real>
struct FoldedModel
{
   std::unique_ptr<DevModel<real>> model;
   ModelScalars scalars;                       // the model's scalars (carried in the kernarg block): nj, lanes Sa, S, GS, Sa_real, ...
   std::vector<int> device_sphere_order;       // XML index of device sphere k
   std::vector<int> slot_xml;                  // XML index of the sphere in lane/slot q of the active block, -1: empty
   int pair_entries = 0;                       // entries of the staged self-collision pair list (rounds x 32; 0: the kernel family does not use one)
   int variant = 0;                            // the robot's part of the kernel variant mask (ORC_VAR_ bits of dev_types.h)
};
// `asked_block`: the workgroup shape the caller asked for (the module's setting, else the parameters'; 0: none)
template <typename real>
FoldedModel<real> fold_robot(const Robot & robot, const BatchParams & params, int n, const JointTree & tree, int asked_block,
   const Switches & sw, PlacementCache cache);

// ---- TSR hard constraints, folded onto the device's joint order (csrc/tsr.h) ------------------------------------------
struct TsrDims
{
   int n_tsrs = 0;
   int cons_k = 0;            // constrained rows in all
   int blocks = 0;            // (constraint, point) blocks of the system
   int kmax = 0;              // most constrained rows on one point
   size_t ws_stride = 0;      // reals of workspace per run
};
template <typename real>
struct FoldedTsrs : TsrDims { std::vector<DevTsr<real>> tsrs; };
template <typename real>
FoldedTsrs<real> fold_tsrs(const Robot & robot, const BatchParams & params, const JointTree & tree, int m, int n);

// ---- the scene table --------------------------------------------------------------------------------------------------
// rooted fields (mod.cpp:2348-2369), scene by scene: descriptors [n_scenes][n_sdfs] (n_sdfs: the fields of the largest scene,
// what the LDS carve-up holds), the same in cell units [n_scenes][sdfc_stride], every scene's slice padded to whole batches of
// four plus four and zeroed (the many-sphere cost path loads a batch unconditionally), the field count of every scene
struct SceneDims { int n_scenes = 1, n_sdfs = 0, sdfc_stride = 0; };
template <typename real>
struct FoldedScenes : SceneDims
{
   std::vector<DevSdf<real>> sdfs;
   std::vector<DevSdfCell<real>> cells;
   std::vector<int> scene_nsdf;
   bool one_aligned = false;                   // every scene: one field with the world's axes
   // the (scene, field) slots of the scenes this shard's runs are in: their `data` is the caller's to fill with the grid's device copy
   struct GridSlot { int scene, field; Sdf * sdf; };
   std::vector<GridSlot> grids;
};
// `offsets_24bit`: the kernel family forms its cell offsets with 24-bit multiplies (the many-sphere pass, cost_generic.h)
template <typename real>
FoldedScenes<real> fold_scenes(const SceneTable & table, int run0, int n_runs, bool offsets_24bit);

// ---- the metric -------------------------------------------------------------------------------------------------------
struct MetricDims
{
   // A^-1: 0 cyclic reduction (tridiagonal), 1 the dense inverse, 2 the closed-form Toeplitz inverse through two wave scans
   // per column (derivative 1, ca tridiag(-1,2,-1)), 3 the band inverse through its rank-D generators (derivative 2..4)
   int solve_mode = 0;
   int pcr_rows = 0, pcr_sym = 0;              // rows of m reals of the table area; mode 0: the compact table is in use
   // mode 3: the band is one Toeplitz row away from the D rows at either end, with no coupling to the end points
   int band_toeplitz = 0;
   double band_c64[ORC_SS_MAX_RANK + 1] = { 0.0 };
};
struct MetricTables : MetricDims
{
   std::vector<double> pcr;                    // the table to upload (empty: none) ...
   bool pcr_as_doubles = false;                // ... entry by entry as reals, or (mode 3) as the doubles they are into the area of pcr_rows x m reals
   std::vector<double> metric64;               // fp32 runs of derivative >= 2: Aband, beta_s, beta_g in double (empty otherwise)
   std::vector<double> Ainv;                   // the dense inverse where the run needs one and the metric came without (empty otherwise)
};
MetricTables pack_metric(const Metric & metric, const BatchParams & params, int m, size_t real_bytes, const Switches & sw);

// ---- the launch plan --------------------------------------------------------------------------------------------------
// What the planner reads: the robot, the run parameters and the MODULE's settings -- never the batch (a run's bits must not
// depend on what shares its batch): no run count, no run offset, no pointer.
struct PlanInput
{
   int variant = 0;                            // the variant bits known so far (robot and scenes)
   int m = 0, n = 0, nj = 0, Sa = 0, S = 0, GS = 0, n_sdfs = 0, n_tsrs = 0, tsr_kmax = 0, pcr_rows = 0, pair_entries = 0;
   int use_momentum = 0, free_start = 0, derivative = 1, solve_mode = 0;
   size_t real_bytes = 8, sdf_bytes = 0;       // sizeof(real), sizeof(DevSdf<real>)
   bool overlapping = false;                   // the module's launches overlap (orc_set_num_streams >= 2)
   int module_threads = 0, module_per_cu = 0;  // orc_set_workgroup_threads / orc_set_workgroups_per_cu of the module (0: not set)
   int params_threads = 0, params_per_cu = 0;  // ... of the run's parameters
};
struct IteratePlan
{
   int variant = 0;                            // the final kernel variant mask (with ORC_VAR_WGS4)
   int block = 256;                            // threads per workgroup of the iterate kernel
   int per_cu = 0;                             // resident workgroups per CU the plan's share of the LDS is sized for (the kernel's registers must hold as many)
   int tile_m = 0, n_tiles = 1, tile_first = 0, tile_rest = 0;   // tiles of an iteration: the first of tile_first moving waypoints, the others of tile_rest
   size_t lds_bytes = 0;
   int lds_flags = 0, pcr_in_lds = 0, ag_in_lds = 1, g_in_lds = 1, t_in_lds = 1;
   LdsLayout lay = {};                         // the LDS carve-up of this plan
   int tsr_structured = 0, tsr_wcap = 0, tsr_nmax = 0;      // the constraint step's structured solve fits the axis tile buffer
   int workgroups_per_cu() const { return (int)((160*1024) / ((lds_bytes + 1279) / 1280 * 1280)); }
};
IteratePlan plan_iterate(const PlanInput & in, const Switches & sw);

} // namespace orc
