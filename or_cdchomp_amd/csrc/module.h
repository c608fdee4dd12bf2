// module.h -- host side of the MI355X-native orcdchomp module.
//
// Mirrors class mod of the reference (src/orcdchomp_mod.h:38-90): the module owns
// the list of signed distance fields and the runs, and exposes the same commands
// through SendCommand.  OpenRAVE's environment (robots, kinbodies, transforms) is
// third party; the pieces of it the hot path reads are held in `env` (env.h).
#pragma once
#include <hip/hip_runtime.h>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "env.h"         // Environment, KinBody
#include "batch.h"       // Batch, BatchShard, VerdictScope, ConvergenceSpec

namespace orc {

class Module
{
public:
   explicit Module(int device);
   explicit Module(const std::vector<int> & devices);     // batches are sharded over these (repeats allowed)
   ~Module();
   // the SendCommand surface (src/orcdchomp_mod.h:58-66); throws std::runtime_error
   // with the reference's message strings
   std::string send_command(const std::string & cmd);

   // the environment stand-ins: robots, kinbodies, grabs, the fields (env.h)
   Environment env;

   // lane placement of a robot's active spheres (place_spheres_on_row): a pure function of the robot
   // (geometry, limits, frozen dof values), the active dofs, floating base and epsilon_self
   std::map<std::string, std::vector<int>> placement_cache;
   // the shards of a batch are built on host threads of their own (Batch::Batch): the placement cache and the fields'
   // device copies (Sdf::dev64 / dev32) are taken under this
   std::recursive_mutex env_mutex;

   // batches
   int create_batch(const std::string & robot, const BatchParams & p, int n_runs,
      const double * starts, const double * goals, const double * basegoals, const unsigned int * seeds,
      const std::vector<int> * devices_override = nullptr, std::shared_ptr<const SceneTable> scenes = nullptr);
   Batch & batch(int id);
   void destroy_batch(int id);
   // collision verdict of all runs of a batch (gettraj's re-check, batched on the device; verdict.cpp): per run
   // collides (0/1), time of the first contact on the retimed trajectory, XML sphere, field, depth
   void batch_collision_verdict(int id, int * collides, double * time, int * sphere, int * field, double * depth, bool self_check = true);
   // the same verdict planned on the device (no trajectory is read back); every output may be NULL: the keys stay on the
   // device for Batch::select and BatchShard::respawn (multistart.cpp).  n_samples: the samples of every run's retimed trajectory
   void batch_collision_verdict_device(int id, int * collides, double * time, int * sphere, int * field, double * depth, int * n_samples,
      const VerdictScope & scope = VerdictScope());
   // ... of a subset of the runs (orc_batch_collision_verdict_subset): which 0 the runs with a nonzero byte in examine [n_runs],
   // which 1 the candidates; a run that is not examined reports collides -1, one that is too long -2; n_samples NULL: the
   // samples behind a contact are not counted
   void batch_collision_verdict_subset(int id, int which, const unsigned char * examine, int * collides, double * time, int * sphere,
      int * field, double * depth, int * n_samples);
   // (clearance.cpp) orc_batch_clearance: per run the smallest gap to a field [0] and between two spheres of a pair [1] over the
   // samples the verdict looks at, with time, XML sphere and field / other sphere; which 0 examine, 1 the candidates, 2 every run
   void batch_clearance(int id, int which, const unsigned char * examine, int max_samples, double * clearance, double * time, int * sphere,
      int * other, int * n_samples);
   // (config_clearance.cpp) orc_batch_config_clearance / orc_batch_waypoint_clearance: the two minima of a single row, n_q rows
   // that are uploaded (configs [n_q][n]) or waypoints of the device's trajectories (waypoints: configs is not read); run_of_q
   // names the run whose scene a query is tested against; outputs [n_q][2], any may be NULL
   void batch_config_clearance(int id, bool waypoints, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
      double * clearance, int * sphere, int * other);
   // (path_clearance.cpp) orc_batch_path_clearance / orc_batch_waypoint_segment_clearance: what batch_clearance reports for a run
   // that holds the path, n_q paths that are uploaded (paths [n_q][n_rows][n]) or segments between two waypoints of the device's
   // trajectories (waypoints: n_rows and paths are not read); outputs [n_q][2] and n_samples [n_q], any may be NULL
   void batch_path_clearance(int id, bool waypoints, int n_q, const int * run_of_q, const int * from_of_q, const int * to_of_q, int n_rows,
      const double * paths, int max_samples, double * clearance, double * time, int * sphere, int * other, int * n_samples);
   // (penetration.cpp) orc_batch_config_penetration / orc_batch_waypoint_penetration: the same queries; per query the penetration
   // cost of the two legs at the two margins [n_q][2], its gradient with respect to the row [n_q][n], and the outputs above
   void batch_config_penetration(int id, bool waypoints, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
      double margin_field, double margin_self, double * cost, double * grad, double * clearance, int * sphere, int * other);
   // (project.cpp) orc_batch_config_tsr: the enforced entries of a TSR's xyzrpy value [n_q][6] and their Jacobian rows [n_q][6][n]
   // (or NULL) at n_q rows, tsrs[tsr_of_q[q]] at row q (tsr_of_q NULL: tsrs[0]; ee_link -1: the active manipulator);
   // orc_batch_project_tsr: the rows projected onto their TSRs on the device.  project_check throws for what both reject
   void batch_config_tsr(int id, const std::vector<TsrSpec> & tsrs, int n_q, const int * tsr_of_q, const double * configs, double * h_out,
      double * jac_out);
   void batch_project_tsr(int id, const std::vector<TsrSpec> & tsrs, int n_q, const int * tsr_of_q, const double * configs, const ProjectSpec & ps,
      double * rows_out, double * resid_out, int * steps_out, int * status_out);
   std::vector<TsrSpec> project_check(const char * who, const Batch & b, const std::vector<TsrSpec> & tsrs, int n_q, const int * tsr_of_q,
      const double * configs) const;
   void project_spec_check(const char * who, const Batch & b, const ProjectSpec & ps) const;      // ... and of a projection's parameters
   // (project_clear.cpp) orc_batch_project_tsr_clear: the rows projected onto their TSRs and moved out of contact with the scenes of
   // their runs at once (or_cdchomp_amd/project_clear.py is the rule); rejects what the projection and the penetration call reject
   void batch_project_tsr_clear(int id, const std::vector<TsrSpec> & tsrs, int n_q, const int * tsr_of_q, const int * run_of_q,
      const double * configs, const ProjectClearSpec & ps, const ProjectClearOut & out);
   // (multistart.cpp) orc_batch_select_best[_by], _respawn, _select_clear: each checks every argument on the host, then takes the
   // verdict with Batch::selection_scope() (collision_free; collision_mode 1, 2) or the clearance, then selects or respawns on the device
   void batch_select_best(int id, int cost_column, int n_groups, const int * group_of_run, bool collision_free, int * best_run, double * best_cost,
      int * n_eligible);
   void batch_respawn(int id, int cost_column, int n_groups, const int * group_of_run, int collision_mode, int keep, double sigma,
      const unsigned int * seeds, int * source_of_run, int * n_survivors);
   // orc_batch_select_clear: the clearance of the candidates, then per group the best run among those that clear `margin`
   void batch_select_clear(int id, int cost_column, int n_groups, const int * group_of_run, double margin, int max_samples,
      int * best_run, double * best_cost, double * best_clearance, int * n_eligible, int * n_samples);

   // orc_scene_merge_fields / the mergefields command: the fields of `fields` (each where field_poses [n][7] puts its kinbody;
   // NULL: where it stands) resampled on the device into one grid with the axes of `target`, a kinbody without a field, and
   // registered as that kinbody's field; bounds [6] in the target's frame or NULL (merge_grid_dims, merge_kernels.hip)
   void merge_fields(const std::string & target, const std::vector<std::string> & fields, const double * field_poses, double cell,
      const double * bounds);

   hipStream_t stream = nullptr;     // orc_set_stream: the stream of the first device's work (NULL: its default stream)
   int device;                       // first entry of `devices`
   std::vector<int> devices;
   // optional pool of streams per device: shards are bound round-robin to one of them at creation so
   // that independent batches overlap on the GPU (the tail of one launch fills with the next)
   std::map<int, std::vector<hipStream_t>> stream_pool;
   std::map<int, size_t> next_pool_stream;
   int num_streams = 0;
   int workgroup_threads = 0;       // 0: the planner's choice; 192 or 256: the workgroup shape of every batch created from now on
   int workgroups_per_cu = 0;       // 0: the kernels' own register budget; 4: four 256-thread workgroups per CU where a kernel is built for it
   void set_num_streams(int n);
   hipStream_t pick_stream(int device, bool distinct);
   // a high-priority stream per device for the hmc plan of a call (hmc_kernels.hip): its wavefronts are dispatched ahead
   // of the iterate launches queued on the other streams instead of behind them
   hipStream_t plan_stream(int device);
   // The momentum-resampling plan of an iterate call (noise [n_runs][cap][m n], resample iterations [n_runs][cap]) is written and
   // read inside that one call, so the batches that run on one stream share one pair of buffers: the stream orders their
   // calls.  (A buffer per batch held 1.8 GB for every config-4 batch a caller had created ahead of time.)
   struct PlanBuffers { PlanStore store; std::mutex enqueue; };
   PlanBuffers & plan_buffers(int device, hipStream_t stream);
   // kernel timing (HIP events on the shards' streams), harvested from the shards
   void time_collect();
   double kernel_ms_total = 0.0;
   int kernel_launches = 0;
   // The pool of timing events and the totals are shared by all shards, and the shards of one batch may
   // launch from host threads of their own (Batch::for_shards): everything below takes timing_mutex_.
   hipEvent_t acquire_event(int device);                       // a pooled event of `device`, or a new one (the device must be current)
   void release_event(int device, hipEvent_t ev);
   void add_kernel_time(double ms);
   std::string last_error;
   std::string last_reply;
   std::string last_collision_details;   // what the reference logs with RAVELOG_ERROR in gettraj

private:
   std::string cmd_computedistancefield(const std::vector<std::string> & argv);
   std::string cmd_addfield_fromobsarray(const std::vector<std::string> & argv);
   std::string cmd_removefield(const std::vector<std::string> & argv);
   std::string cmd_mergefields(const std::vector<std::string> & argv);
   std::string cmd_create(const std::vector<std::string> & argv, bool batch);
   std::string cmd_iterate(const std::vector<std::string> & argv, bool batch);
   std::string cmd_gettraj(const std::vector<std::string> & argv, bool batch);
   std::string cmd_destroy(const std::vector<std::string> & argv);
   std::map<int, std::unique_ptr<Batch>> batches_;
   int next_batch_id_ = 1;
   std::map<int, std::vector<hipEvent_t>> event_pool_;
   std::map<int, hipStream_t> plan_streams_;
   std::map<std::pair<int, hipStream_t>, PlanBuffers> plan_buffers_;
   std::mutex timing_mutex_;
};

} // namespace orc
