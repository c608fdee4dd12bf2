// batch.h -- a batch of CHOMP runs as the host layer holds it: the shard of its runs on one device, the batch over the shards, and
// the small structs their calls take (batch.cpp, verdict.cpp, clearance.cpp, config_clearance.cpp, penetration.cpp, project.cpp,
// project_clear.cpp, multistart.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <vector>
#include "stages.h"      // Robot, Sdf, SceneTable, TsrSpec, BatchParams; the stages of `create`
#include "devbuf.h"      // DeviceGuard, hip_check, DevBuf, dev_alloc, upload
#include "hmc.h"         // HmcPlan, PlanStore, HmcPlanner: the momentum-resampling plan of HMC runs
#include "verdict.h"     // VerdictInputs, the sample clock, the free functions of the collision verdict
#include "tsr_form.h"    // TsrForm, tsr_form: the constraint step's form, the iterate kernel's own decision
#include "multistart.h"  // SelectCriterion, SelectResult, PerturbPlan, RespawnPlan: what the multi-start calls pass each other
#include "deal.h"        // DealColumn, deal_gather, deal_scatter: the queries of a single-row call dealt to the shards

template <typename real> struct DevVerdictWalk;      // verdict_device.h
template <typename real> struct DevVerdictPlanned;
template <typename real> struct DevPenetration;      // penetration_device.h

namespace orc {

// Which runs a device-planned collision verdict examines, and what it does about the samples nobody walks (the fields of the
// same names in DevVerdictPlan, verdict_device.h).  The default is orc_batch_collision_verdict_device's: every run, the
// samples behind a contact counted, a run that is too long fails the call.
struct VerdictScope
{
   int which = -1;                            // -1 every run; 0 the runs of `examine`; 1 the candidates (run_candidate.h)
   const unsigned char * examine = nullptr;   // which 0: a byte per run of the BATCH, nonzero: examine it (a shard takes its slice)
   bool count_rest = true;                    // false: n_samples of an examined run is not exact and nobody counts to 2^30
   bool long_marks_run = false;               // true: a run that is too long reports n_samples ORC_VERDICT_TOO_LONG and the call succeeds
};

// the convergence stop of a batch's runs (orc_batch_set_convergence; dev_types.h DevBatch::conv_*): patience 0 is off
struct ConvergenceSpec
{
   double rtol = 0.0;
   int patience = 0;
   double obs_max = HUGE_VAL;
   // rejects a NaN or non-positive rtol and a NaN obs_max when the stop is on (throws)
   void validate() const;
};

// where a penetration call's results go (penetration.cpp): cost [n_q][2], grad [n_q][n], clear [n_q][2], key [n_q][2]
// (config_device.h); any may be NULL
struct PenetrationOut
{
   double * cost = nullptr, * grad = nullptr, * clear = nullptr;
   unsigned int * key = nullptr;
};
// what the calls with margins reject of them (penetration.cpp; who: the call's name in what it throws)
void margins_check(const char * who, double margin_field, double margin_self);
// key [count] of a single-row call (config_device.h) as the boundary returns it: the XML sphere, and the field or the other
// sphere of a pair; -1 and -1 without an item (config_clearance.cpp; sphere, other: [count] or NULL)
void unpack_keys(const unsigned int * key, size_t count, int * sphere, int * other);

// the parameters of a projection onto TSRs (project.cpp; or_cdchomp_amd/project.py is the rule); lower, upper [n] or NULL
struct ProjectSpec
{
   int max_steps = 30;
   double tol = 1e-6, mu = 1e-8, step_cap = 0.5;
   const double * lower = nullptr, * upper = nullptr;
};
// where the results of the two TSR calls go: h [n_q][6], jac [n_q][6][n] (the evaluation); rows [n_q][n], resid, steps, status
// [n_q] (the projection); any may be NULL
struct ProjectOut
{
   double * h = nullptr, * jac = nullptr, * rows = nullptr, * resid = nullptr;
   int * steps = nullptr, * status = nullptr;
   ProjectOut from(size_t first, int n) const;
};

// the parameters of a projection onto TSRs and out of contact (project_clear.cpp; or_cdchomp_amd/project_clear.py is the rule)
struct ProjectClearSpec
{
   ProjectSpec project;          // max_steps, tol, mu, step_cap, lower, upper: as the projection's
   double push_cap = 0.2, margin_field = 0.02, margin_self = 0.0, slack = 2e-3;
};
// where its results go: rows [n_q][n], resid [n_q], clear [n_q][2], steps, status [n_q]; none is NULL
struct ProjectClearOut
{
   double * rows = nullptr, * resid = nullptr, * clear = nullptr;
   int * steps = nullptr, * status = nullptr;
};

class Module;

// a contiguous block of the runs of a batch on ONE device: n_runs independent runs sharing robot,
// fields and parameters (struct run, src/orcdchomp_mod.cpp:887-966, once per run in the reference)
class BatchShard
{
public:
   BatchShard(Module * mod, int device, hipStream_t stream, const Robot & robot, const BatchParams & p, int n_runs,
      const double * starts, const double * goals, const double * basegoals, const unsigned int * seeds,
      std::shared_ptr<const SceneTable> scenes, int run0);
   ~BatchShard();
   BatchShard(const BatchShard &) = delete;
   BatchShard & operator=(const BatchShard &) = delete;
   // iterations [iter_begin, iter_begin + n_iter) of an iterate call (r->iter restarts at 0 in every
   // call, src/orcdchomp_mod.cpp:2752: the hmc schedule compares against it), then the cost-only pass
   // `carry`: the launch continues an iterate call (runs that left their limits earlier in the call stay out)
   void iterate_async(int n_iter, int iter_begin = 0, bool final_eval = true, bool carry = false);
   void sync_begin(double * costs_out, int * status_out, int * iters_out);   // enqueue the copies
   void sync_end();                                                          // wait for them
   void gettraj(double * out);
   void get_plan(double out[9]) const;      // kernel variant bits, threads per workgroup, LDS bytes, tile, solve mode, workgroups per CU, tiles, lanes per waypoint, first tile
   void get_tsr_plan(double out[11]) const; // constraints, rows in all, structured solve or not, N at its largest; tsr_form's fields (width -1: the dense step); m
   void get_state(const std::string & which, double * out);
   void get_trace(double * out);
   void set_noise(const double * noise, int n_blocks) { hmc_->set_noise(noise, n_blocks); }      // caller-supplied blocks (host streams only)
   void set_traj(const double * traj);          // [n_runs][n_points][n] host -> device (warm start)
   // multi-start (multistart.cpp, multistart_kernels.hip)
   // perturb: T[moving] += scale * A^-1 xi(seed of the run), clamped to the limits;
   // gen = the generators of A^-1, U [rank][m] then V [rank][m] (Batch::perturb builds them once for all shards)
   void perturb(double scale, const unsigned int * seeds, const std::vector<double> & gen, int rank);
   // the winners among this shard's runs (LOCAL runs); group [n_runs] is this shard's slice.  collision_free reads the keys the
   // last collision_verdict_planned kept on the device, by_margin the minima the last `clearance` kept there
   SelectResult select(int n_groups, const int * group, const SelectCriterion & c);
   // respawn (orc_batch_respawn).  This shard's groups as a CSR over its LOCAL runs (group_offs [n_groups + 1], members ascending per group, every run in one
   // group): ranks every group, makes every run that does not survive a copy of its source or the straight line, perturbs those
   // runs when scale > 0 (seeds, gen, rank: as in perturb).  mode 1, 2: the keys of the collision_verdict_planned made just
   // before.  One synchronisation, at the end; source_out [n_runs] (local runs, -1: the line) and n_survivors_out [n_groups]
   // are what comes back
   void respawn(int n_groups, const std::vector<int> & group_offs, const std::vector<int> & members, int column, int mode, int keep,
      double scale, const unsigned int * seeds, const std::vector<double> & gen, int rank, int * source_out, int * n_survivors_out);
   // per-run lambda, epsilon, obs_factor, obs_factor_self of this shard's runs (orc_batch_set_run_params): table [n_runs][4] doubles,
   // validated by Batch::set_run_params, converted to the batch's precision here and uploaded on the shard's stream (so that launches
   // enqueued before keep the old values); NULL: the later launches read no table
   void set_run_params(const double * table);
   void get_run_params(double * out);       // [n_runs][4]: what the device holds, or the shared values when there is no table
   // rows[k] (local runs) of the trajectory array as doubles: out [rows.size()][n_points][n]
   void gettraj_rows(const std::vector<int> & rows, double * out);
   const Metric & metric() const { return metric_; }
   // (verdict.cpp) first contact of every run's trajectory with a field, on the device (Module::batch_collision_verdict plans the samples)
   void collision_verdict(const std::vector<int> & offs, const std::vector<int> & seg, const std::vector<double> & u,
                          const VerdictInputs & in, unsigned long long * key_out, double * depth_out);
   // the same verdict with the retiming and the samples planned on the device (verdict_kernels.hip): nothing but vmax
   // [n - col0] and the pair tables goes up, and what of key / depth / time / n_samples [n_runs] is not NULL comes back; the
   // keys stay on the device for select_best.  Returns false when a run has too many samples (nothing is written then).
   // scope: the runs that are examined (its `examine` is this shard's slice); a run that is not has the key ORC_VERDICT_NONE
   bool collision_verdict_planned(const VerdictInputs & in, unsigned long long * key_out, double * depth_out, double * time_out,
                                  int * n_samples_out, const VerdictScope & scope = VerdictScope());
   // (clearance.cpp) the clearance of this shard's runs (clearance_kernels.hip; scope.which -1, 0, 1 as for the verdict, the other
   // fields of the scope are not read): the two minima of every run stay on the device for `select`, and what of clear /
   // time [n_runs][2], key [n_runs][2] and n_samples [n_runs] is not NULL comes back
   void clearance(const VerdictInputs & in, const VerdictScope & scope, int max_samples, double * clear_out, double * time_out,
                  unsigned long long * key_out, int * n_samples_out);
   // (config_clearance.cpp) the clearance of n_q single rows against the scenes of this shard's runs (config_kernels.hip):
   // configs [n_q][n] with run_of_q [n_q] (LOCAL runs); or configs NULL, waypoints of the device's trajectories: run_of_q and
   // point_of_q [n_q], or both NULL and n_q = n_runs * n_points, every waypoint in storage order.  What of clear [n_q][2] and
   // key [n_q][2] (config_device.h) is not NULL comes back; nothing is kept on the device
   void config_clearance(const VerdictInputs & in, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
                         double * clear_out, unsigned int * key_out);
   int config_chunk() const;                 // the queries a workgroup of that kernel takes: the walk's rule for `chunk` with this kernel's LDS
   // (path_clearance.cpp) the clearance of n_q paths against the scenes of this shard's runs (path_kernels.hip): paths
   // [n_q][n_rows][n] with run_of_q [n_q] (LOCAL runs, NULL: run 0); or paths NULL and n_rows 2, the segments between the
   // waypoints from_of_q and to_of_q [n_q] of the device's trajectories.  What of clear, time, key [n_q][2] (path_device.h) and
   // n_samples [n_q] is not NULL comes back; nothing is kept on the device
   void path_clearance(const VerdictInputs & in, int n_q, const int * run_of_q, const int * from_of_q, const int * to_of_q, int n_rows,
                       const double * paths, int max_samples, double * clear_out, double * time_out, unsigned long long * key_out, int * n_samples_out);
   // (penetration.cpp) the penetration cost and its gradient of the same queries (penetration_kernels.hip), with the two minima
   // and keys of config_clearance; nothing is kept on the device
   void config_penetration(const VerdictInputs & in, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
                           double margin_field, double margin_self, const PenetrationOut & out);
   int penetration_chunk() const;            // the queries a workgroup of that kernel takes
   // (project.cpp) the constraints `specs` (ee_link resolved, one point each) folded with `robot` as `create` folds a batch's, and
   // at n_q rows configs [n_q][n] with tsr_of_q [n_q] (NULL: specs[0]): their value and Jacobian (ps NULL), or the projection
   // onto them (project_kernels.hip); nothing is kept on the device
   void project_tsr(const Robot & robot, const std::vector<TsrSpec> & specs, int n_q, const int * tsr_of_q, const double * configs,
                    const ProjectSpec * ps, const ProjectOut & out);
   // (project_clear.cpp) the projection of n_q rows onto `specs` and out of contact with the scenes of this shard's runs
   // (run_of_q: LOCAL runs, NULL: run 0): rounds of penetration_kernel and project_clear_step_kernel on the shard's stream
   // (project_clear_kernels.hip); nothing is kept on the device
   void project_tsr_clear(const Robot & robot, const VerdictInputs & in, const std::vector<TsrSpec> & specs, int n_q, const int * tsr_of_q,
                          const int * run_of_q, const double * configs, const ProjectClearSpec & ps, const ProjectClearOut & out);
   int project_state_in_lds(int kmax) const; // 1: a lane's state of that kernel (kmax 3 or 6 rows) lives in LDS for this batch, 0: in the call's workspace
   void get_phase_cycles(long long * out);   // [n_runs][8], diagnostics (ORC_PHASE_TIMERS=1)
   void get_wave_hwid(unsigned int * out);   // [n_runs][8][2], diagnostics (ORC_PHASE_TIMERS=1): DevBatch::wave_hwid of the last launch
   // kernel timing: completed event pairs are added to the module's totals (all of them when `wait`)
   void harvest_events(bool wait);

   int n_runs, n_points, n, m;
   BatchParams params;
   ConvergenceSpec conv;           // sticky for the later iterate calls (Batch::set_convergence)
   int last_n_iter = 0;
   int device;
   std::string robot_name;
   std::vector<int> adofindices;
   std::vector<int> device_sphere_order;    // XML index of device sphere k
   std::vector<int> slot_xml;               // XML index of the sphere in lane/slot q of the active block, -1: empty
private:
   template <typename real> void build_device(const Robot & robot);     // the stages of stages.h, and the uploads of what they return
   template <typename real> std::shared_ptr<void> grid_on_device(Sdf & s);      // the device's copy of a field's grid, shared by the shards
   template <typename real> void seed_runs(const Robot & robot, const double * starts, const double * goals, const double * basegoals);
   template <typename real> void launch(int n_iter, bool final_eval, bool carry, const HmcPlan & hmc);
   // generators, limits and seeds of a perturbation go up and perturb_kernel is launched (source_of_run: a respawn's plan, or NULL); no wait
   struct PerturbUpload { DevBuf gen, seeds; };
   void launch_perturb(double scale, const unsigned int * seeds, const std::vector<double> & gen, int rank, const int * source_of_run, PerturbUpload & up);
   // what the verdicts and the clearance put on the device (verdict.cpp): the tables of DevVerdictWalk and, for a device-planned
   // walk, of DevVerdictPlanned, which the handles keep until the kernel has run
   struct VerdictTables { DevBuf xml, pairs, rsum, inact, depth, vmax, examine; };
   template <typename real> void verdict_walk_args(const VerdictInputs & in, const std::function<size_t(int)> & lds_bytes, VerdictTables & t, DevVerdictWalk<real> & w);
   template <typename real> size_t verdict_planned_args(const char * who, const char * tag, size_t (*kernel_lds)(int, int, int, int, int, size_t, int), const VerdictInputs & in,
      const VerdictScope & scope, VerdictTables & t, DevVerdictPlanned<real> & v);
   template <typename real> void collision_verdict_typed(const std::vector<int> & offs, const std::vector<int> & seg, const std::vector<double> & u,
      const VerdictInputs & in, unsigned long long * key_out, double * depth_out);
   template <typename real> bool collision_verdict_planned_typed(const VerdictInputs & in, unsigned long long * key_out, double * depth_out,
      double * time_out, int * n_samples_out, const VerdictScope & scope);
   template <typename real> void clearance_typed(const VerdictInputs & in, const VerdictScope & scope, int max_samples, double * clear_out,
      double * time_out, unsigned long long * key_out, int * n_samples_out);
   template <typename real> void config_clearance_typed(const VerdictInputs & in, int n_q, const int * run_of_q, const int * point_of_q,
      const double * configs, double * clear_out, unsigned int * key_out);
   template <typename real> void path_clearance_typed(const VerdictInputs & in, int n_q, const int * run_of_q, const int * from_of_q, const int * to_of_q,
      int n_rows, const double * paths, int max_samples, double * clear_out, double * time_out, unsigned long long * key_out, int * n_samples_out);
   template <typename real> void config_penetration_typed(const VerdictInputs & in, int n_q, const int * run_of_q, const int * point_of_q,
      const double * configs, double margin_field, double margin_self, const PenetrationOut & out);
   // what a launch of penetration_kernel needs beside its queries and outputs: the walk's tables (verdict_walk_args) and the
   // pairs by sphere go up, `v` gets them and its chunk; returns the launch's LDS bytes (throws when the robot does not fit)
   struct PenetrationTables { VerdictTables walk; DevBuf pair_offs, pair_list; std::vector<int> host_offs, host_list; };
   template <typename real> size_t penetration_setup(const VerdictInputs & in, PenetrationTables & t, DevPenetration<real> & v);
   template <typename real> void project_tsr_clear_typed(const Robot & robot, const VerdictInputs & in, const std::vector<TsrSpec> & specs, int n_q,
      const int * tsr_of_q, const int * run_of_q, const double * configs, const ProjectClearSpec & ps, const ProjectClearOut & out);
   template <typename real> void project_tsr_typed(const Robot & robot, const std::vector<TsrSpec> & specs, int n_q, const int * tsr_of_q,
      const double * configs, const ProjectSpec * ps, const ProjectOut & out);
   void construct(const Robot & robot, const double * starts, const double * goals, const double * basegoals,
      const unsigned int * seeds);
   Module * mod_;
   hipStream_t stream_ = nullptr;   // the stream all work of this shard is issued on
   Switches sw_;                    // the environment's switches as `create` found them
   std::vector<std::shared_ptr<void>> sdf_refs_;   // the field copies the device descriptors point at
   std::shared_ptr<const SceneTable> scenes_;      // the batch's scenes; this shard holds runs [run0_, run0_ + n_runs) of its scene_of_run
   int run0_ = 0;
   std::vector<std::pair<hipEvent_t, hipEvent_t>> pending_events_;
   Metric metric_;
   // what the stages of `create` left (stages.h)
   ModelScalars ms_ = {};           // the device model's scalars (carried in the kernarg block)
   TsrDims tsr_;
   SceneDims scn_;
   MetricDims met_;
   IteratePlan plan_;
   // device buffers of the shard (typed by params.precision: a cast where they are used)
   DevBuf d_model_, d_sdfs_, d_sdfc_, d_scene_of_run_, d_scene_nsdf_;
   DevBuf d_traj_, d_AG_, d_G_, d_Gcost_;
   DevBuf d_costs_, d_trace_; size_t trace_cap_ = 0;
   DevBuf d_conv_prev_, d_conv_streak_;      // [n_runs] the convergence stop's state between the launches of a call
   DevBuf d_status_, d_iters_done_, d_leap_, d_phase_, d_hwid_;
   DevBuf d_run_params_; bool run_params_on_ = false;      // [n_runs] RunParams<real>; kept allocated while off (launches in flight may read it)
   DevBuf d_vkey_;                           // [n_runs] the keys of the last collision_verdict_planned
   DevBuf d_clear_, d_clear_ns_;             // [n_runs][2] doubles, [n_runs] ints: the minima and the sample counts of the last `clearance`
   DevBuf d_Aband_, d_beta_s_, d_beta_g_, d_metric64_, d_pcr_, d_Ainv_, d_jl_lo_, d_jl_hi_;
   // TSR hard constraints (csrc/tsr.h): the device copies of the constraints, the per-run workspace
   DevBuf d_tsrs_, d_tsr_ws_, d_tsr_err_;
   std::vector<double> jl_lo_, jl_hi_;
   std::unique_ptr<HmcPlanner> hmc_;         // the momentum-resampling plan of the runs (hmc.h), made at the end of `construct`
};

// A batch as the boundary sees it: its runs are cut into contiguous blocks, one BatchShard per
// entry of the module's device list (no collective, the caller's arrays are the
// gather).  One device: one shard.
class Batch
{
public:
   Batch(Module * mod, const std::vector<int> & devices, const Robot & robot, const BatchParams & p, int n_runs,
      const double * starts, const double * goals, const double * basegoals, const unsigned int * seeds,
      std::shared_ptr<const SceneTable> scenes);
   ~Batch();
   void iterate_async(int n_iter, int iter_begin = 0, bool final_eval = true, bool carry = false);
   void sync(double * costs_out, int * status_out, int * iters_out = nullptr);
   void gettraj(double * out);
   void get_plan(double out[9]);            // the plan of the first shard (all shards of a batch plan alike)
   void get_tsr_plan(double out[11]);       // ... and what the constraint step will run
   void get_state(const std::string & which, double * out);
   void get_trace(double * out);
   void set_noise(const double * noise, int n_blocks);
   void set_traj(const double * traj);
   // multi-start (multistart.cpp): orc_batch_perturb / _select_best / _select_clear / _respawn / _gettraj_runs (include/orcdchomp_amd.h
   // has the contract)
   void perturb(double sigma, const unsigned int * seeds);
   // throws for a bad sigma and for the batches orc_batch_perturb rejects, whatever sigma is
   PerturbPlan perturb_plan(double sigma) const;
   // respawn (orc_batch_respawn): respawn_plan checks every argument and builds the shards' group tables without any device
   // work (throws); respawn then runs on every shard that has a group.  The verdict, for mode 1 and 2, is taken between the two
   RespawnPlan respawn_plan(int cost_column, int n_groups, const int * group_of_run, int collision_mode, int keep, double sigma,
      const unsigned int * seeds) const;
   void respawn(const RespawnPlan & plan, const unsigned int * seeds, int * source_of_run_out, int * n_survivors_out);
   std::vector<int> select_groups(int n_groups, const int * group_of_run) const;   // the validated group of every run (NULL: contiguous equal blocks); throws
   // every shard's winners merged (merge_winners), with the batch's runs; the verdict or the clearance the criterion reads was
   // made just before and never left the device (validate a column 0..2 with select_column first)
   SelectResult select(int n_groups, const std::vector<int> & group, const SelectCriterion & c);
   static void select_column(int column);   // throws unless 0, 1 or 2
   // per-run parameters: each array [n_runs] or NULL (the value of `params`); all NULL switches the table off.  Throws and changes
   // nothing on a NaN or infinite entry or a lambda or epsilon <= 0
   void set_run_params(const double * lambda, const double * epsilon, const double * obs_factor, const double * obs_factor_self);
   void get_run_params(double * out);       // [n_runs][4]
   void gettraj_runs(const int * runs, int n_sel, double * out);
   bool iterated = false;            // an iterate call has been made: the device's costs and status are a call's results
   void collision_verdict(const std::vector<int> & offs, const std::vector<int> & seg, const std::vector<double> & u,
                          const VerdictInputs & in, unsigned long long * key_out, double * depth_out);
   // every shard plans and walks its own runs; outputs [n_runs] or NULL; throws when a run has too many samples (unless
   // scope.long_marks_run).  scope.which 1 on a batch that has not been iterated throws select_best's message
   void collision_verdict_planned(const VerdictInputs & in, unsigned long long * key_out, double * depth_out, double * time_out,
                                  int * n_samples_out, const VerdictScope & scope = VerdictScope());
   // the checks of a device-planned walk's scope that the verdict and the clearance share (verdict.cpp; throws)
   void verdict_scope_check(const char * who, int which, const unsigned char * examine, const char * unmasked, const char * other) const;
   // (clearance.cpp) orc_batch_clearance / orc_batch_select_clear.  clearance_check throws for what those calls reject of which,
   // examine and max_samples, before any device work; `clearance`: every shard walks its slice, outputs as BatchShard's, over
   // the batch's runs
   void clearance_check(int which, const unsigned char * examine, int max_samples) const;
   void clearance(const VerdictInputs & in, int which, const unsigned char * examine, int max_samples, double * clear_out, double * time_out,
                  unsigned long long * key_out, int * n_samples_out);
   // The queries of a single-row call dealt to the shards (batch.cpp, deal.h).  Per shard: the queries whose run (run_of_q, NULL:
   // run 0) it owns, in their order, with the run rebased; the input columns `ins` gathered; call(shard, count, run, in, out) with
   // the columns' data in their order (NULL for a NULL column); the output columns `outs` scattered back to the caller's order.
   // Nothing is copied when one shard owns every run, nor in the profile form (`profile`: query q is waypoint q in storage
   // order, n_points per run, and a shard's queries are a contiguous slice of the caller's arrays; run is NULL then)
   using DealCall = std::function<void(size_t, int, const int *, const std::vector<void *> &, const std::vector<void *> &)>;
   void deal_by_run(int n_q, const int * run_of_q, bool profile, const std::vector<DealColumn> & ins, const std::vector<DealColumn> & outs, const DealCall & call);
   // (config_clearance.cpp) orc_batch_config_clearance / orc_batch_waypoint_clearance.  config_clearance_check throws for what
   // those calls reject, before any device work; `config_clearance`: every shard takes the queries whose run it owns, in their
   // order, and the results go back to the caller's order; outputs [n_q][2] or NULL
   void config_clearance_check(bool waypoints, int n_q, const int * run_of_q, const int * point_of_q, const double * configs) const;
   void config_clearance(const VerdictInputs & in, bool waypoints, int n_q, const int * run_of_q, const int * point_of_q,
                         const double * configs, double * clear_out, unsigned int * key_out);
   // (path_clearance.cpp) orc_batch_path_clearance / orc_batch_waypoint_segment_clearance.  path_clearance_check throws for what
   // those calls reject, before any device work (waypoints: n_rows and paths are not read); `path_clearance`: every shard takes
   // the queries whose run it owns, in their order, and the results go back to the caller's order; outputs [n_q][2], n_samples
   // [n_q], or NULL
   void path_clearance_check(bool waypoints, int n_q, const int * run_of_q, const int * from_of_q, const int * to_of_q, int n_rows,
                             const double * paths, int max_samples) const;
   void path_clearance(const VerdictInputs & in, bool waypoints, int n_q, const int * run_of_q, const int * from_of_q, const int * to_of_q,
                       int n_rows, const double * paths, int max_samples, double * clear_out, double * time_out, unsigned long long * key_out,
                       int * n_samples_out);
   // (penetration.cpp) orc_batch_config_penetration / orc_batch_waypoint_penetration: the queries dealt by run (the caller has
   // made config_clearance_check and margins_check)
   void config_penetration(const VerdictInputs & in, bool waypoints, int n_q, const int * run_of_q, const int * point_of_q,
                           const double * configs, double margin_field, double margin_self, const PenetrationOut & out);
   // (project.cpp) orc_batch_config_tsr / orc_batch_project_tsr: every shard takes an even contiguous slice of the queries (the
   // caller, Module::project_check, has checked the arguments)
   void project_tsr(const Robot & robot, const std::vector<TsrSpec> & specs, int n_q, const int * tsr_of_q, const double * configs,
                    const ProjectSpec * ps, const ProjectOut & out);
   // (project_clear.cpp) orc_batch_project_tsr_clear: a row goes to the shard that owns its run (the caller,
   // Module::batch_project_tsr_clear, has checked the arguments)
   void project_tsr_clear(const Robot & robot, const VerdictInputs & in, const std::vector<TsrSpec> & specs, int n_q, const int * tsr_of_q,
                          const int * run_of_q, const double * configs, const ProjectClearSpec & ps, const ProjectClearOut & out);
   // the runs the verdict inside select_best and respawn examines (orc_batch_set_verdict_scope): 0 every run, 1 the candidates;
   // kept until it is set again
   int verdict_scope = 0;
   void set_verdict_scope(int scope);        // throws unless 0 or 1
   VerdictScope selection_scope() const;     // what that verdict is taken with
   void get_phase_cycles(long long * out);
   void get_wave_hwid(unsigned int * out);
   // the convergence stop of every shard's runs for the later iterate calls (validated: throws and changes nothing on a bad spec)
   void set_convergence(const ConvergenceSpec & c);
   const ConvergenceSpec & convergence() const { return shards[0]->conv; }
   // the per-iteration log of create's dat_filename (src/orcdchomp_mod.cpp:2306-2310, 2811-2818)
   void open_dat(const std::string & pattern);
   void write_dat(int iter_begin, int n_iter, const int * iters_done, double t_begin, double t_end);

   int n_runs, n_points, n, m;
   BatchParams params;
   int last_n_iter = 0;
   std::string robot_name;
   std::vector<int> adofindices;
   std::vector<int> device_sphere_order;
   std::vector<int> slot_xml;
   std::vector<Robot::Sphere> run_spheres;   // the spheres create collected (robot + held bodies): what the XML indices count through
   std::vector<unsigned char> run_self_excl; // [n][n] pairs of them the re-check's self-collision leg never tests (Robot::run_self_pairs_excluded, taken at create)
   std::vector<std::unique_ptr<BatchShard>> shards;
   std::vector<int> offs;            // first run of every shard, then n_runs
   std::shared_ptr<const SceneTable> scenes;   // the runs' obstacles as create placed them
   bool per_run_scenes = false;      // created with a scene table (orc_batch_create_scenes): gettraj's re-check walks the run's scene
   bool has_dat() const { return !dat_.empty(); }
private:
   void for_shards(const std::function<void(size_t)> & body, bool threads);
   std::vector<FILE *> dat_;         // one per run (a single run: the reference's fp_dat)
};

} // namespace orc
