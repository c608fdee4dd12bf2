/* orcdchomp_amd.h -- C ABI of the MI355X-native CHOMP hot path.
 *
 * Drop-in boundary for the path  computedistancefield -> create -> iterate ->
 * gettraj -> destroy  of the orcdchomp OpenRAVE module (personalrobotics/or_cdchomp).
 * Plain C: pointers and sizes only, no C++/torch types.  Every entry point names
 * the reference interface it replaces (paths relative to /root/reference).
 *
 * Conventions
 *   - all functions return 0 on success, non-zero on error; the message of the
 *     last error of a module is available through orc_last_error() and uses the
 *     reference's own exception strings.  1 = the call failed
 *     (message set), 2 = no module was passed.  A null pointer where an array, a
 *     name or a struct is required, an unknown handle, a short buffer or a
 *     malformed robot description is such an error, not a fault; pointers
 *     documented as optional may be NULL.
 *   - pose = 7 doubles [x y z qx qy qz qw]           (src/libcd/kin.c:42-52)
 *   - grids are C ordered [x][y][z] doubles            (src/libcd/grid.c:31-32)
 *   - trajectories are run-major: traj[run][waypoint][dof]
 *   - handles returned as text by create are opaque strings, as in the reference
 *     ("%p" there, an integer id here; src/orcdchomp_mod.cpp:2670-2674).
 */
#ifndef ORCDCHOMP_AMD_H
#define ORCDCHOMP_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orc_module orc_module;

/* ---- module lifetime ---------------------------------------------------------
 * replaces the plugin entry points CreateInterfaceValidated / DestroyPlugin
 * (src/orcdchomp.cpp:50-74) and the mod constructor/destructor
 * (src/orcdchomp_mod.h:45-75).  device = HIP device ordinal (one process per GPU). */
orc_module * orc_module_new(int device);
/* one module over several GPUs of the node, inside one process: every batch is cut into contiguous
 * blocks of runs, one per entry of `devices` (an ordinal may repeat: its blocks then run on streams
 * of their own), each block iterates on its device and copies its results straight into the
 * caller's arrays -- the host-side gather; no collective.  Fields and the robot model
 * are replicated to every device at create.  orc_module_new(d) is the list {d}. */
orc_module * orc_module_new_multi(const int * devices, int n_devices);
void orc_module_free(orc_module * mod);
const char * orc_last_error(const orc_module * mod);
/* HIP stream all kernels and copies of this module are issued on (a hipStream_t,
 * e.g. torch.cuda.current_stream().cuda_stream); NULL = the default stream. */
int orc_set_stream(orc_module * mod, void * hip_stream);
/* give the module a pool of n internal streams per device: batches created afterwards are bound to
 * them round-robin, so launches of independent batches overlap on the GPU (0 = back to one stream).
 * Fails while batches exist: they hold the streams they were bound to. */
int orc_set_num_streams(orc_module * mod, int n);

/* ---- SendCommand -------------------------------------------------------------
 * replaces ModuleBase::SendCommand -> orcwrap_call (src/orcwrap.cpp:37-69) ->
 * mod::computedistancefield / addfield_fromobsarray / removefield / create /
 * iterate / gettraj / destroy (src/orcdchomp_mod.h:58-66).  Same command names,
 * same argv grammar (shell-style quoting, src/libcd/util_shparse.c), same textual
 * returns.  out receives the reply (NUL terminated, truncated to out_cap).
 * Batch extensions (additive): createbatch, iteratebatch, gettrajbatch; and
 * mergefields kinbody NAME fields 'A B C' cell F [bounds 'x0 y0 z0 x1 y1 z1'] (orc_scene_merge_fields with every source
 * where it stands; reply "").
 * create ... dat_filename PATH writes the reference's per-iteration log "%d %f %f %f %f\n"
 * (iteration, seconds, cost_total, cost_obs, cost_smooth; mod.cpp:2306-2310, 2811-2818); the seconds
 * are wall seconds since the iterate call began (the reference: thread CPU seconds), a fused launch's
 * interval divided evenly over its iterations.  createbatch takes a pattern with %d = run index, and
 * `devices 'i j ...'` to shard one batch over GPUs (see orc_module_new_multi).  iterate / iteratebatch
 * take `converge_rtol F`, `converge_patience N` and `converge_obs F`: the convergence stop of
 * orc_batch_set_convergence for that call only (tokens not given keep the batch's setting, patience
 * defaults to 1); a run that converges reports status 1, and only status -1 throws. */
int orc_send_command(orc_module * mod, const char * cmd, char * out, size_t out_cap);
/* size in bytes (without NUL) of the full reply of the last successful command */
size_t orc_last_reply_size(const orc_module * mod);
/* copy of the full reply of the last successful command (for replies larger than out_cap) */
int orc_last_reply(const orc_module * mod, char * out, size_t out_cap);

/* ---- environment stand-ins ---------------------------------------------------
 * The reference reads robots and bodies from the OpenRAVE environment
 * (e->GetRobot / e->GetKinBody, src/orcdchomp_mod.cpp:1894,336).  OpenRAVE is
 * third party; these calls hand the same information over explicitly. */

/* kinematic tree, links in topological order (parent index < own index):
 *   link frame = parent link frame o pose_parent_joint o motion(axis, q[dof])
 * joint_type 0 fixed, 1 revolute, 2 prismatic.  Spheres in <orcdchomp><spheres>
 * XML order (src/orcdchomp_kdata.cpp:79-94, struct sphere src/orcdchomp_kdata.h:33-39). */
typedef struct orc_robot_desc
{
   int n_links;
   const int * parent;               /* [n_links], -1 for the root */
   const double * pose_parent_joint; /* [n_links][7] */
   const int * joint_type;           /* [n_links] */
   const double * axis;              /* [n_links][3] unit, in the joint frame */
   const int * dof_index;            /* [n_links] robot dof, -1 for fixed */
   int n_dof;
   const double * limit_lower;       /* [n_dof]  (GetDOFLimits, mod.cpp:2639) */
   const double * limit_upper;       /* [n_dof] */
   int n_spheres;
   const int * sphere_link;          /* [n_spheres] link index */
   const double * sphere_pos;        /* [n_spheres][3] in the link frame */
   const double * sphere_radius;     /* [n_spheres] */
} orc_robot_desc;

int orc_env_add_robot(orc_module * mod, const char * name, const orc_robot_desc * desc);
int orc_robot_set_transform(orc_module * mod, const char * name, const double pose[7]);      /* robot->SetTransform */
int orc_robot_set_dof_values(orc_module * mod, const char * name, const double * values, int n); /* SetDOFValues */
int orc_robot_set_active_dofs(orc_module * mod, const char * name, const int * indices, int n); /* SetActiveDOFs */
/* GetDOFVelocityLimits: used by the linear retimer of gettraj (default 1 for every dof) */
int orc_robot_set_velocity_limits(orc_module * mod, const char * name, const double * limits, int n);

/* Workgroup shape of the iterate kernel for the batches created from now on: 0 = the planner's choice
 * (256 threads, three workgroups per CU for the WAM), 192 = three wavefronts, four workgroups per CU:
 * 1024 runs are then resident at once on 256 CUs and ONE launch of 1024 runs ends ~10 % earlier; large
 * or overlapping batches are ~5 % slower with it; 512 = eight wavefronts on one run, one run per CU, the
 * whole trajectory in one tile: the latency shape for batches smaller than the chip (one run: 34 k
 * instead of 22 k iterations/s, 256 runs: 5.4 M instead of 4.2 M).  The single-run `create` command uses
 * 512 unless a shape is set here.  128 = two wavefronts on a run, up to eight runs per CU (fp64 fixed-base chains with at
 * most 16 active spheres): what the planner gives runs with TSR constraints -- whose elimination is the work of two
 * wavefronts -- when the module's launches overlap (orc_set_num_streams >= 2): +18 %.  The shape never depends on the batch
 * itself, so that a run's result does not depend on what shares its batch (trajectories are bit-identical across shapes;
 * robots with 17 .. 32 active spheres have the 256- and 512-thread shapes and fall back to the many-sphere kernels at 192). */
int orc_set_workgroup_threads(orc_module * mod, int threads);
/* Register budget of the batches created from now on: 0 (default) the planner's choice, 3 the kernels' own (three 256-thread
 * workgroups per CU at 168 registers for fp64), 4: four per CU at 128 registers with smaller tiles, where a kernel is built
 * for it (fp64 robots on a fixed-base chain with at most 16 active spheres -- the WAM of the BASELINE configurations -- or
 * with 17 .. 32: the robot that holds something; others, and runs too long for the smaller share of the LDS, keep their
 * default).  The planner's choice is a function of the robot, the run parameters and this module's settings, never of the
 * batch: four per CU for runs with TSR constraints and for the 17 .. 32-sphere family (faster whatever the launch pattern)
 * and, when the module's launches overlap (orc_set_num_streams >= 2), for every fixed-base chain (+3-5 %; one launch of
 * <= 1024 runs at a time is 3 % faster at three).  Trajectories are bit-identical either way. */
int orc_set_workgroups_per_cu(orc_module * mod, int workgroups);

/* What the TSR constraints of `create` address on the robot (src/orcdchomp_mod.cpp:1957-1976):
 * GetLink(name) for `con_tsr 'all link NAME'`; GetManipulators() / GetActiveManipulator() and their
 * GetEndEffectorTransform() (= end-effector link transform o tool_pose) for `'all manipee NAME'`,
 * `'all'` and `everyn_tsr`.  The first manipulator added is the active one. */
int orc_robot_set_link_names(orc_module * mod, const char * name, const char * const * names, int n);
int orc_robot_add_manipulator(orc_module * mod, const char * name, const char * manip, int ee_link, const double tool_pose[7]);
int orc_robot_set_active_manipulator(orc_module * mod, const char * name, const char * manip);
/* Pairs of links the robot description declares adjacent (OpenRAVE robot files: <adjacent>linkA linkB</adjacent>;
 * KinBody::GetAdjacentLinks): RobotBase::CheckSelfCollision, which the re-check of mod::gettraj calls
 * (src/orcdchomp_mod.cpp:2998-2999), never tests them.  link_pairs [n_pairs][2] link indices. */
int orc_robot_set_adjacent_links(orc_module * mod, const char * name, const int * link_pairs, int n_pairs);
/* The self-collision leg of the re-check is a stand-in: OpenRAVE tests the links' meshes, this library the bounding
 * spheres of the optimizer's model, which are fatter (a trajectory whose meshes clear each other by less than the spheres'
 * slack is "in collision" here and returned by the reference), and "adjacent in the initial configuration" is taken with
 * all dofs at zero.  enabled = 0 leaves that leg out for this robot (gettraj, gettrajbatch ... verdict,
 * orc_batch_collision_verdict); `gettraj ... no_self_collision_check` does the same for one call.  Default 1. */
int orc_robot_set_self_check(orc_module * mod, const char * name, int enabled);

/* a kinbody made of oriented boxes (InitFromBoxes-style); box_poses [n_boxes][7]
 * in the kinbody frame, half_extents [n_boxes][3] */
int orc_env_add_kinbody_boxes(orc_module * mod, const char * name, int n_boxes,
   const double * box_poses, const double * half_extents);
/* a kinbody given as a triangle mesh (KinBody::InitFromTrimesh; the reference's own scene is meshes, scripts/test_wam7.py:23-28):
 * vertices [n_tri][3][3] in the kinbody frame.  computedistancefield sweeps its cube against the triangles (the collision
 * query of src/orcdchomp_mod.cpp:462-531; a mesh is a surface, the flood fill of 540-548 closes its inside; touching counts as
 * a collision so that a closed mesh gives a closed shell of cells).  Called for an existing kinbody of boxes the triangles are
 * added to it. */
int orc_env_add_kinbody_trimesh(orc_module * mod, const char * name, int n_tri, const double * vertices);
/* KinBody::SetTransform.  A kinbody the robot holds is moved there and rides with its link from there on (the grab's
 * relative transform is taken anew; passing the pose orc_body_get_transform returns changes nothing) */
int orc_kinbody_set_transform(orc_module * mod, const char * name, const double pose[7]);
int orc_kinbody_enable(orc_module * mod, const char * name, int enabled);
/* KinBody::GetTransform of a robot or kinbody; a kinbody the robot holds is where its link carries it now */
int orc_body_get_transform(orc_module * mod, const char * name, double pose_out[7]);

/* ---- grabbed bodies ----------------------------------------------------------
 * mod::create collects the spheres of the robot AND of every kinbody the robot is grabbing
 * (src/orcdchomp_mod.cpp:2168-2300: r->robot->GetGrabbed(), the body's <orcdchomp> kdata, the link
 * r->robot->IsGrabbing(k)); carrying an object is the planner's normal use.  The stand-ins for what the
 * reference asks OpenRAVE: */
/* the <orcdchomp><spheres> data of a kinbody (src/orcdchomp_kdata.cpp:79-94; the stand-in's kinbodies have one
 * link, so the sphere's link attribute is that link): sphere_pos [n_spheres][3] in the kinbody frame */
int orc_kinbody_set_spheres(orc_module * mod, const char * name, int n_spheres, const double * sphere_pos,
   const double * sphere_radius);
/* RobotBase::Grab(body, link): from now on the kinbody is rigid with robot link `link` at its current relative
 * transform (orc_robot_set_dof_values / orc_robot_set_transform carry it along) and a `create` for this robot
 * adds the body's spheres to the run: each rides on `link` at T_w_rlink^-1 o T_w_klink o pos
 * (src/orcdchomp_mod.cpp:2200-2208), active when an active dof moves `link` (2265-2291); the run's sphere list is the
 * last grabbed body's spheres first and the robot's last, as the head insertion of 2273-2290 leaves it.  XML
 * sphere indices reported by the collision verdict count through the robot's spheres, then the held bodies' in the
 * order they were grabbed.  A held body (or the robot) without spheres makes `create` fail with the reference's
 * "no spheres! kinbody does not have a <orcdchomp> tag defined?" (2262-2263).  The re-check of gettraj includes the
 * spheres a run was created with (the reference's note at 2992-2996).  A run keeps the spheres it was created with. */
int orc_robot_grab(orc_module * mod, const char * robot, const char * kinbody, int link);
/* RobotBase::Release(body) / ReleaseAllGrabbed(): the body stays where the link left it */
int orc_robot_release(orc_module * mod, const char * robot, const char * kinbody);
int orc_robot_release_all(orc_module * mod, const char * robot);

/* ---- SDF access --------------------------------------------------------------
 * the module's field list (struct sdf, src/orcdchomp_mod.cpp:148-153) */
int orc_scene_add_sdf(orc_module * mod, const char * kinbody, const int sizes[3], const double lengths[3],
   const double pose_kinbody_gsdf[7], const double * sdf_data);
/* copy out a computed field: sizes[3], lengths[3], pose[7] (grid wrt kinbody), data (may be NULL to query sizes) */
int orc_scene_get_sdf(orc_module * mod, const char * kinbody, int sizes[3], double lengths[3], double pose[7],
   double * data, size_t data_cap);

/* The fields of n_fields placed kinbodies baked into ONE field whose axes are the target kinbody's, on the device: the layout
 * becomes an ordinary module field, so a scene of that one placement is under the cap of ORC_MAX_SDFS whatever n_fields is
 * (there is no limit of eight here) and, with the target standing at the identity, runs the one-field kernels.
 *   field_kinbodies [n_fields]: kinbodies with a field, in the order of the best-of-N field loop; one may repeat.
 *   field_poses [n_fields][7] (x y z qx qy qz qw): the world pose to use for every source kinbody, or NULL: every kinbody
 *     where it stands now.  Poses are used as given (pose_apply's expanded quaternion; nothing is normalised).
 *   cell: the edge of the merged grid's cubic cells.  bounds [6] = lo[3], hi[3] in the target kinbody's frame, or NULL: the
 *     box around the eight corners of every source's box.  sizes[d] = max(2, ceil((hi[d] - lo[d]) / cell)), lengths[d] =
 *     sizes[d] cell, and the field's pose in the target kinbody's frame is (lo, identity quaternion): orc_host_merge_grid.
 * Every cell holds what the best-of-N loop finds at the cell's CENTRE: the smallest value, by strict <, that the reference's
 * interpolation (cd_grid_double_interp, src/libcd/grid.c:386-454, HUGE_VAL poisoning included) gives among the sources that
 * contain the centre; a cell no source covers holds +inf, which every cost family reads as "no field here".  That is the one
 * difference from a scene of the n_fields placements: the values are resampled at cell centres and interpolated from there
 * (merged_grid_dims and merged_field of or_cdchomp_amd/module.py are the specification, orc_host_merge_fields the host twin
 * the device agrees with bit for bit).
 * The target must be an existing kinbody without a field (one of zero boxes is the intended target).  The field is a
 * snapshot: moving a source afterwards does not change it, moving the target moves it, as with any field.  The host copy is
 * read back once; the kernel's output buffer stays as the field's fp64 copy on the module's (first) device.
 * Rejected with a nonzero return and a message, before any device work, the module unchanged: n_fields < 1; an unknown
 * kinbody, or a source without a field; the target among the sources, or a target that already has a field; a non-finite or
 * non-positive cell; non-finite poses or bounds, or lo >= hi; a quaternion of zero norm; a grid of 2^31 bytes or more
 * ("signed distance field too large for this build!", here and not at create). */
int orc_scene_merge_fields(orc_module * mod, const char * target_kinbody, int n_fields, const char * const * field_kinbodies,
   const double * field_poses, double cell, const double * bounds);

/* ---- kernel-level batch API --------------------------------------------------
 * what the command layer calls; one batch = n_runs independent CHOMP runs that
 * share robot, fields and parameters (struct run, src/orcdchomp_mod.cpp:887-966;
 * cd_chomp, src/libcd/chomp.h:38-101).  A single `create` is a batch of 1.
 * (The fields may differ per run: orc_batch_create_scenes; so may the seed trajectories: orc_batch_perturb; and
 * lambda, epsilon, obs_factor and obs_factor_self: orc_batch_set_run_params.) */
typedef struct orc_batch_params
{
   int n_points;               /* default 101        (mod.cpp:1840) */
   int floating_base;          /*                    (mod.cpp:1843,1928) */
   double lambda;              /* default 10         (mod.cpp:1824) */
   int derivative;             /* D, default 1       (mod.cpp:1826) */
   int use_momentum;           /*                    (mod.cpp:1825) */
   int use_hmc;                /*                    (mod.cpp:1873) */
   double hmc_resample_lambda; /* default 0.02       (mod.cpp:1875) */
   double epsilon;             /* default 0.1        (mod.cpp:1845) */
   double epsilon_self;        /* default 0.04       (mod.cpp:1846) */
   double obs_factor;          /* default 200        (mod.cpp:1847) */
   double obs_factor_self;     /* default 10         (mod.cpp:1848) */
   int precision;              /* 64 (default) or 32: arithmetic type of the device path */
} orc_batch_params;
void orc_batch_params_default(orc_batch_params * p);

/* replaces mod::create (src/orcdchomp_mod.cpp:1800-2688) for n_runs runs at once.
 * starts: [n_runs][n_adof] or NULL (= the robot's current active dof values, as the
 * reference does); goals: [n_runs][n_adof]; basegoals: [n_runs][7] or NULL;
 * seeds: [n_runs] or NULL (0).  *batch_id receives the handle. */
int orc_batch_create(orc_module * mod, const char * robot, const orc_batch_params * params, int n_runs,
   const double * starts, const double * goals, const double * basegoals, const unsigned int * seeds,
   int * batch_id);
/* orc_batch_create with obstacles per run: a scene is an ordered list of at most ORC_MAX_SDFS (8) field
 * placements, and every run is optimized against the scene scene_of_run[run] names.  A placement is a
 * kinbody whose field exists in the module (computedistancefield, addfield_fromobsarray,
 * orc_scene_add_sdf) and the kinbody's world pose to use for it: the field then stands at
 * pose_world_kinbody o (the field's pose in the kinbody frame).  Scenes are given in CSR form: scene s
 * holds the placements [scene_begin[s], scene_begin[s+1]) of field_kinbodies / field_poses, in the
 * order of the best-of-N field loop (a tie goes to the earlier field).  A scene may be empty (no
 * obstacle cost) and may place one kinbody's field more than once; the scenes share the device
 * copies of the grids.  field_poses [scene_begin[n_scenes]][7] (x y z qx qy qz qw) or NULL: every
 * kinbody where it stands now.  The rest of the batch API works unchanged; the collision verdict
 * (orc_batch_collision_verdict, gettrajbatch ... verdict, the re-check of gettraj) tests every run
 * against its own scene, and a reported field index is the placement's position in that scene.
 * A malformed table (n_scenes < 1, scene_begin not starting at 0 or decreasing, a scene of more
 * than ORC_MAX_SDFS fields, an unknown kinbody or one without a field, a scene_of_run entry outside
 * [0, n_scenes)) is rejected with a nonzero return; the module stays usable. */
int orc_batch_create_scenes(orc_module * mod, const char * robot, const orc_batch_params * params, int n_runs,
   const double * starts, const double * goals, const double * basegoals, const unsigned int * seeds,
   int n_scenes, const int * scene_begin, const char * const * field_kinbodies, const double * field_poses,
   const int * scene_of_run, int * batch_id);
/* replaces mod::iterate (src/orcdchomp_mod.cpp:2690-2852): n_iter iterations of
 * cd_chomp_iterate (src/libcd/chomp.c:430-683) for every run, then the final
 * cost evaluation.  costs_out [n_runs][3] = total, obs, smooth (may be NULL);
 * status_out [n_runs]: 0 ok, -1 "Resulting trajectory is outside of joint limits!", 1 the run
 * converged and stopped early (orc_batch_set_convergence; not an error). */
int orc_batch_iterate(orc_module * mod, int batch_id, int n_iter, double * costs_out, int * status_out);
/* A run that leaves its joint limits stops iterating for the rest of THAT call (the reference throws
 * out of mod::iterate, src/orcdchomp_mod.cpp:2799-2803) and reports status -1 and the costs of its
 * last complete iteration; the run stays usable and a later call iterates it again, as in the
 * reference.  A run that converged (status 1) made k+1 <= n_iter iterations and reports the final
 * costs of a call of k+1 iterations.  Iterations each run completed in the last call: iters_out [n_runs]. */
int orc_batch_iterations_done(orc_module * mod, int batch_id, int * iters_out);
/* Convergence stop for the batch's later iterate calls (orc_batch_iterate, _iterate_async, the
 * iterate / iteratebatch commands), on the device, per run.  With tot_k = obs_k + smooth_k the costs
 * of iteration k (the trace's row k), iteration k is settled when it has a predecessor k-1 in the
 * same call, |tot_{k-1} - tot_k| <= rtol |tot_{k-1}| and obs_k <= obs_max.  A streak counter starts
 * at 0 in every call, counts settled iterations and drops to 0 on an unsettled one; the run stops
 * after completing the first iteration at which it reaches patience, with status 1.  A stopped run
 * is exactly a run whose call had n_iter = k+1 (trajectory, final costs, "AG", iterations done); its
 * trace rows from k+1 on are NaN.  A run that leaves its joint limits first reports -1 as before.
 * patience <= 0 switches the stop off (the default).  A NaN or non-positive rtol or a NaN obs_max
 * is rejected with a nonzero return; the batch keeps its previous setting.  obs_max: +inf for none.
 * HMC runs: the call's momentum resamples are planned for all n_iter iterations, so after a stop the
 * random stream is where a full-length call leaves it (as after a run that left its limits). */
int orc_batch_set_convergence(orc_module * mod, int batch_id, double rtol, int patience, double obs_max);
/* Per-run lambda, epsilon, obs_factor and obs_factor_self: a portfolio of parameter sets in one batch.  Each array is
 * [n_runs], or NULL: every run takes the value the batch was created with.  The call REPLACES the whole table (it does not
 * merge with an earlier call); all four NULL switches the feature off, the kernels then read no table.  It applies to every
 * iterate call enqueued after it (orc_batch_iterate, _iterate_async, the iterate / iteratebatch commands, every launch of a
 * call that launches once per iteration -- max_time, trajs_fileformstr -- and the final cost-only pass); an
 * orc_batch_iterate_async enqueued before it finishes with the old values (the upload follows it on the shard's stream).  It
 * may be called between iterate calls: a schedule, such as annealing obs_factor, is a sequence of calls.
 * The values are converted to the batch's precision once on the host, as create converts orc_batch_params; the kernels pick
 * the run's record or the batch's own once per phase and share all code after that, so a run with per-run values p is bit
 * for bit the same run in a batch created with p as its parameters: trajectory, costs, trace, status, iterations done, "AG".
 * A run's result depends on its own four values only, never on its position, its neighbours or the shard that holds it (a
 * module over several devices slices the table by shard, as it slices scene_of_run).
 * Rejected with a nonzero return and a message, the previous table kept and the module usable: an unknown batch; a NaN or
 * infinite entry in any array; a lambda or epsilon entry <= 0 (the kernels form 1/lambda and 1/epsilon).
 * Read-back: orc_batch_get_state(..., "run_params", ...) gives [n_runs][4] doubles in the order lambda, epsilon, obs_factor,
 * obs_factor_self: what the device holds (a precision 32 batch returns them float-rounded; a batch without a table returns
 * the shared values, rounded alike).
 * Deliberately NOT per run: epsilon_self feeds the fold (sphere placement on the 16-lane row, the pair list's order and its
 * always-evaluated rounds), the fold decides the plan, and a plan must not depend on the run; hmc_resample_lambda is planned
 * by another kernel (or the host) for the whole call; n_points, derivative, use_momentum, use_hmc and precision all shape
 * the plan. */
int orc_batch_set_run_params(orc_module * mod, int batch_id,
   const double * lambda, const double * epsilon,
   const double * obs_factor, const double * obs_factor_self);
/* asynchronous form for measurement: enqueue only, results stay on the device */
int orc_batch_iterate_async(orc_module * mod, int batch_id, int n_iter);
int orc_batch_sync(orc_module * mod, int batch_id, double * costs_out, int * status_out);
/* per-iteration cost trace of the last iterate call: [n_runs][n_iter][3] (total, obs, smooth as the
 * reference logs them, mod.cpp:2798); rows of iterations an aborted (status -1) or converged
 * (status 1) run did not make are NaN */
int orc_batch_get_trace(orc_module * mod, int batch_id, double * trace_out, size_t cap_doubles);
/* momentum noise for HMC resampling supplied by the caller instead of the module's
 * own mt19937 stream: noise [n_runs][n_blocks][m][n] (used in resample order) */
int orc_batch_set_noise(orc_module * mod, int batch_id, const double * noise, int n_blocks);
/* replaces the waypoint export of mod::gettraj (src/orcdchomp_mod.cpp:2897-2903):
 * traj_out [n_runs][n_points][n] */
int orc_batch_gettraj(orc_module * mod, int batch_id, double * traj_out, size_t cap_doubles);
/* replaces the collision re-check of mod::gettraj (src/orcdchomp_mod.cpp:2958-3006) for all runs of
 * a batch at once, on the device: every run's trajectory is retimed at the dof velocity limits and
 * sampled every 0.04 rad of C-space distance like the reference's loop; a sample collides when an
 * active sphere penetrates a field (the optimizer's own model; OpenRAVE's mesh checker is third
 * party) or, the reference's `|| CheckSelfCollision` (src/orcdchomp_mod.cpp:2998-2999), when two spheres on
 * links that may collide overlap (not the same link, not parent and child, not links whose spheres already
 * overlap with all dofs at zero: the sphere model's stand-in for OpenRAVE's adjacent links).  Per run (any
 * output may be NULL): collides 0/1, time of the first contact, XML index of the sphere, index of the field
 * (a pair of spheres: -2 - the XML index of the other sphere), penetration depth in metres. */
int orc_batch_collision_verdict(orc_module * mod, int batch_id, int * collides_out, double * time_out,
                                int * sphere_out, int * field_out, double * depth_out);
/* The same verdict with the retiming and the sample planning done by the kernel that walks the samples: no trajectory
 * is read back and no sample list is uploaded; what goes to the device is the velocity limits and the tables of the
 * self-collision leg, which do not depend on the trajectories.  The outputs are those of orc_batch_collision_verdict,
 * bit for bit (the planning arithmetic is the host's, in double for precision 32 batches too: the specification is
 * verdict_samples of or_cdchomp_amd/module.py, the host's own planner is orc_host_verdict_samples), with the robot's
 * self-check setting; n_samples_out [n_runs]: the samples of every run's retimed trajectory, all of them also when the
 * walk stops at a contact.  Only collides_out is required.  A run of 2^30 samples or more (C-space length / 0.04)
 * fails the call with "trajectory too long for the batched collision verdict!" before anything of it is walked.  A
 * batch over several devices: every shard plans and walks its own runs. */
int orc_batch_collision_verdict_device(orc_module * mod, int batch_id, int * collides_out, double * time_out,
                                       int * sphere_out, int * field_out, double * depth_out, int * n_samples_out);
/* orc_batch_collision_verdict_device asked about some of the runs only: the workgroup of a run that is not examined returns
 * before it stages or walks anything, so the call costs what the examined runs cost.  It replaces "the verdict of every run,
 * then look at the ones that matter": after an iterate call the runs that left their joint limits (status -1) end far outside
 * them, their retimed trajectories are by far the longest of the batch, and no selection rule can pick them.
 *   which 0: examine [n_runs] bytes, nonzero: examine the run.  NULL is rejected.
 *   which 1: the candidates -- the runs whose status of the last iterate call is 0 or 1 and whose total cost is finite, the
 *     eligibility of orc_batch_select_best without its verdict (`candidates` of or_cdchomp_amd/module.py), decided on the
 *     device from what that call left there.  examine must be NULL; a batch that has not been iterated is rejected as
 *     orc_batch_select_best rejects it.
 * An examined run: the outputs of orc_batch_collision_verdict_device, bit for bit.  A run that is not examined: collides -1
 * and n_samples -1, and time -1, sphere -1, field -1, depth 0 as a run without a contact reports them.  An examined run of
 * 2^30 samples or more: collides -2 and n_samples -2, otherwise like a run that is not examined, AND THE CALL SUCCEEDS: one
 * hopeless run no longer takes the verdict of the others with it (`verdict_subset` of module.py is the specification of
 * all three).  n_samples_out == NULL: the samples behind a first contact are not counted -- one lane steps through them by
 * repeated addition, up to 2^30 times -- and "too long" is then what is decided before anything is walked (C-space length
 * / 0.04 >= 2^30); the other outputs do not change.  Only collides_out is required.  Several devices: every shard takes its
 * slice of examine, a shard without a run to examine does nothing.
 * Rejected with a nonzero return and a message before any device work, the module usable: any other `which`; a NULL examine
 * with which 0 or an examine with which 1; collides_out == NULL; an unknown batch; which 1 on a batch never iterated. */
int orc_batch_collision_verdict_subset(orc_module * mod, int batch_id, int which, const unsigned char * examine,
                                       int * collides_out, double * time_out, int * sphere_out, int * field_out,
                                       double * depth_out, int * n_samples_out);
/* Which runs the verdict inside orc_batch_select_best[_by] (require_collision_free) and orc_batch_respawn (collision_mode 1
 * and 2) examines.  scope 0, the default: every run, orc_batch_collision_verdict_device's call in every respect.  scope 1:
 * the candidates (which 1 above), the samples behind a contact not counted, and the call fails with "trajectory too long
 * for the batched collision verdict!" only when a CANDIDATE is too long.  The documented results of those calls do not
 * depend on the scope: a run that is no candidate was never eligible and never a survivor, whatever its verdict.  Any other
 * scope is rejected and the setting kept; it persists until it is set again, like orc_batch_set_convergence. */
int orc_batch_set_verdict_scope(orc_module * mod, int batch_id, int scope);
/* optimizer state read-back for tests: which = "G", "AG", "T" ([n_runs][m][n]); "phase" ([n_runs][8] cycle counters with
 * ORC_PHASE_TIMERS=1); "waves" ([n_runs][8][2], with ORC_PHASE_TIMERS=1: the hardware-ID register and the XCC-ID register of
 * every wavefront of the run's workgroup as read at the start of the last launch, 4294967295 for a wavefront the workgroup does
 * not have; HW_ID holds the wave slot in bits 0-3, the SIMD in 4-5, the CU in 8-11, the shader array in 12, the shader engine
 * in 13-15; the second number holds the XCC in bits 0-3 and, in bits 8.., the logical wavefront the hardware wavefront is in
 * the launch's last iteration, ORC_WAVE_ROTATE); "plan" (8 numbers: kernel variant bits -- 512 = the dense pair-list family, 1 = a tree --, threads per
 * workgroup, LDS bytes per workgroup, tile, solve mode (2 closed-form scans, 3 band-inverse generators, 1 dense), workgroups
 * per CU, tiles, lanes per waypoint; a ninth, the moving waypoints of the first tile, when cap_doubles >= 9);
 * "run_params" ([n_runs][4]: lambda, epsilon, obs_factor, obs_factor_self as the device holds them, orc_batch_set_run_params);
 * "config_chunk" (1 number: the consecutive queries a workgroup of orc_batch_config_clearance's kernel takes for this batch);
 * "penetration_chunk" (1 number: the same of orc_batch_config_penetration's kernel);
 * "project_state" (2 numbers: 1 when a lane's state of orc_batch_project_tsr's kernel lives in LDS for this batch, 0 when it
 * lives in the call's workspace, for TSRs of up to 3 and of up to 6 enforced rows);
 * "tsr_plan" (11 numbers: constraints, constrained rows in all (cons_k), 1 when the constraint step is solved point by point
 * (tsr_structured), n_max (tsr_nmax), then orc_host_tsr_form's six for this batch, the first of them -1 when every step is the
 * dense one, and m, the moving waypoints: n_points - 2, or n_points - 1 with start_tsr) */
int orc_batch_get_state(orc_module * mod, int batch_id, const char * which, double * out, size_t cap_doubles);
int orc_batch_dims(orc_module * mod, int batch_id, int * n_runs, int * n_points, int * n);
/* overwrite the trajectories of a batch (warm start; what `create starttraj` does for one run,
 * src/orcdchomp_mod.cpp:2375-2416): traj [n_runs][n_points][n] */
int orc_batch_set_traj(orc_module * mod, int batch_id, const double * traj, size_t count_doubles);
/* ---- multi-start: K runs per planning problem from different seed trajectories, the best one kept -----------------
 * The reference has no multi-start (its seed is the straight line, src/orcdchomp_mod.cpp:2417-2464, so K runs of one
 * problem without hmc are K identical runs); these three calls diversify the seeds, reduce the results and fetch the
 * winners on the device.  They compose with per-run scenes and the convergence stop: one batch can hold P problems x K
 * starts, each run stopping on its own, and hand back P trajectories. */
/* Adds a smooth random displacement to the moving waypoints of every run; after create (or orc_batch_set_traj), before
 * iterate.  For run r, with m moving waypoints and n columns:  xi = the first m n unit Gaussians of a fresh GSL stream
 * seeded seeds[r], in [waypoint][dof] order -- exactly what orc_host_gsl_stream(seeds[r], 1.0, m n, ...) returns; seed 0
 * is GSL's 4357; the stream is the call's own, the batch's hmc stream is not advanced.  delta = sigma c A^-1 xi, column
 * by column, with A the batch's smoothness metric (what orc_host_metric(m, derivative, dt = 1/(n_points-1), ...)
 * describes) and c = 1 / |row mid of A^-1|_2, mid = m / 2 (integer division, 0-based moving row): sigma is the standard
 * deviation, in dof units, of the displacement of the middle waypoint, and the displacement tapers to zero at the fixed
 * ends (the scale of A cancels).  Then T[moving] += delta and every entry is clamped to [limit_lower, limit_upper] of
 * its dof.  The arithmetic is in double for precision 32 batches too; the result is stored in the batch's precision.
 * A run's result depends on its seed, sigma and the batch's parameters only, never on its position in the batch or on
 * the shard that holds it.  sigma == 0 on a batch the call accepts returns before any device work and changes no bit
 * (the rejections below are checked first, so they do not depend on sigma).  The call leaves no other state behind: a
 * perturbed batch is the same batch as one given those trajectories through orc_batch_set_traj.
 * Rejected with a nonzero return and a message, the batch unchanged and the module usable: a NaN, negative or infinite
 * sigma; seeds == NULL; an unknown batch; a floating-base batch (quaternion columns); a batch whose start point is free
 * (start_tsr); derivative > 4 or any metric for which the device has only the dense inverse (orc_host_metric_semisep_rank
 * gives 0 for a derivative >= 2); a run whose m n Gaussians (doubles) do not fit the LDS of one CU
 * (m n > 20 136: 8 m n + 2496 bytes of generator state against 160 KB - 256). */
int orc_batch_perturb(orc_module * mod, int batch_id, double sigma, const unsigned int * seeds);
/* The best run of every group of a batch, after an iterate call.  group_of_run [n_runs] with entries in [0, n_groups)
 * (anything else is rejected), or NULL: n_groups contiguous equal blocks of runs (n_runs % n_groups != 0 is then
 * rejected).  A run is eligible when its status from the last iterate call is 0 or 1, its total cost (costs[run][0] of
 * that call) is finite and, with require_collision_free != 0, the batch's collision verdict for its current trajectory
 * says it does not collide -- the verdict orc_batch_collision_verdict gives, with the robot's self-check setting, taken
 * by orc_batch_collision_verdict_device's kernel.  Per
 * group the eligible run of lowest total cost wins, a tie goes to the lowest run index: best_run_out [n_groups] (-1 for a
 * group without an eligible run), best_cost_out [n_groups] (+inf there), n_eligible_out [n_groups] the group's eligible
 * runs; any output may be NULL.  A batch that has never been iterated is rejected (orc_batch_iterate with 0 iterations
 * makes the costs valid).  The reduction is a segmented arg-min on the device over the costs and status an iterate call
 * left there: only n_groups triples leave it (a module over several devices: every shard reduces its runs and the host
 * merges n_shards x n_groups candidates by the same rule; groups may span shards).  With require_collision_free the
 * verdict plans its samples on the device and its keys stay there, where the reduction reads them: the velocity limits
 * and the tables of the self-collision leg go up, no trajectory leaves the device either way.  What stays on the host is
 * the construction of those tables, which does not depend on the trajectories.  The arguments are checked before the
 * verdict is taken: a rejected call costs no kernel. */
int orc_batch_select_best(orc_module * mod, int batch_id, int n_groups, const int * group_of_run, int require_collision_free,
   int * best_run_out, double * best_cost_out, int * n_eligible_out);
/* orc_batch_select_best with the cost that is minimised chosen by the caller: cost_column 0 total, 1 obs, 2 smooth (any other
 * value is rejected before any device work).  costs[run][0] and [1] contain obs_factor, so the total is not comparable between
 * runs of different weights (orc_batch_set_run_params); the smoothness cost is.  Eligibility is exactly
 * orc_batch_select_best's -- status 0 or 1, a finite TOTAL cost, the verdict if asked -- whatever the column; only the key
 * changes: per group the eligible run with the lowest costs[run][cost_column] wins, a tie goes to the lowest run index, and
 * best_cost_out is that column's value (+inf for a group without an eligible run).  orc_batch_select_best is the column-0
 * case; several devices merge by the same rule. */
int orc_batch_select_best_by(orc_module * mod, int batch_id, int cost_column, int n_groups,
   const int * group_of_run, int require_collision_free,
   int * best_run_out, double * best_cost_out, int * n_eligible_out);
/* Successive halving between two iterate calls: every group keeps its best `keep` runs, and every other run of the group
 * becomes a freshly perturbed copy of one of them; a group with nothing worth keeping restarts from the straight line.
 * cost_column, n_groups and group_of_run (NULL: contiguous equal blocks) mean what they mean in orc_batch_select_best_by.
 * collision_mode 0 ignores the collision verdict, 1 requires a collision-free run, 2 prefers one.  The rule is respawn_plan
 * of or_cdchomp_amd/module.py:
 *   Candidates: a run whose status of the last iterate call is 0 or 1 and whose TOTAL cost is finite; with mode 1 a run that
 *     collides is not a candidate (orc_batch_select_best's eligibility); with mode 2 it stays one but ranks behind every
 *     collision-free candidate.  Modes 1 and 2 take the verdict of the current trajectories as orc_batch_select_best does
 *     (orc_batch_collision_verdict_device's kernel; the keys stay on the device).
 *   Order: a group's candidates ascending by (collides -- mode 2 only --, costs[run][cost_column] with -0 equal to +0, run
 *     index).  The first min(keep, candidates) are the group's survivors: n_survivors_out [n_groups].
 *   Sources: source_of_run_out [n_runs].  A survivor's source is its own index.  The other runs of the group, candidates or
 *     not, in ascending run index: the j-th of them (from 0) gets the survivor of rank j mod n_survivors, so the best
 *     survivor receives the most copies.  In a group without a survivor every run's source is -1, the straight line.
 *   A survivor: no bit of it changes (trajectory, "AG", leapfrog_first).
 *   Source s != r: the moving rows [1, n_points-1) of run r become those of run s; BOTH END ROWS OF r STAY, so the call is
 *     meant for groups whose runs share start and goal.  "AG" and leapfrog_first of r become those of s.
 *   Source -1: moving row i becomes s + (g - s) * i / (n_points - 1) column by column, s and g the run's own stored first
 *     and last rows widened to double, evaluated in double in that order and rounded once to the batch's precision (the
 *     statement create seeds with); "AG" = 0 and leapfrog_first = 1, as create leaves them.
 *   Perturbation: with sigma > 0 every run that is not a survivor then receives exactly the displacement
 *     orc_batch_perturb(sigma, seeds) would add to it on its new trajectory (seeds[r], the same scale, the clamp to the
 *     joint limits); survivors receive none.  sigma == 0 clones only; seeds may then be NULL.
 * Nothing else of a run changes: its scene, its orc_batch_set_run_params record (a clone continues under its OWN parameter
 * set), its hmc stream, costs, status, trace and iterations done stay.  The costs on the device now describe trajectories
 * that no longer exist, so the batch counts as not iterated: orc_batch_select_best[_by] and a second orc_batch_respawn are
 * refused until the next iterate call (orc_batch_iterate with 0 iterations is enough).
 * On the device: the host sorts the runs by group (a counting sort of n_runs ints) and uploads that table and the seeds; one
 * workgroup per group ranks its members by counting, without atomics; one kernel copies, one perturbs.  The three run on
 * the shard's stream behind one another with one synchronisation at the end (the verdict of modes 1 and 2 is
 * orc_batch_collision_verdict_device's call in front of them); n_runs + n_groups ints come back and no trajectory crosses
 * the link.  A module over several devices: every shard works on the groups it holds.  Outputs may be NULL.
 * Rejected with a nonzero return and a message, before any device work, the batch unchanged bit for bit and the module
 * usable: an unknown batch; a batch that has not been iterated since create or the last respawn; cost_column outside 0..2;
 * collision_mode outside 0..2; keep < 1; n_groups < 1, a group_of_run entry outside [0, n_groups), or a NULL group_of_run
 * with n_runs % n_groups != 0; a NaN, negative or infinite sigma; seeds == NULL with sigma > 0; every batch
 * orc_batch_perturb rejects (floating base, start_tsr, a metric with the dense inverse only, m n > 20 136), whatever sigma
 * is; a group whose runs lie on more than one shard of a module over several devices (no copy crosses devices); a group of
 * more than 4 096 runs (the ranking kernel stages a group's keys in the LDS of one workgroup). */
int orc_batch_respawn(orc_module * mod, int batch_id, int cost_column, int n_groups, const int * group_of_run,
   int collision_mode, int keep, double sigma, const unsigned int * seeds,
   int * source_of_run_out, int * n_survivors_out);
/* ---- clearance: how far a run stays away, where the verdict only says whether it touches -----------------------------
 * The walk of orc_batch_collision_verdict_device without its stop at the first contact: the same retiming, the same samples
 * (verdict_samples of or_cdchomp_amd/module.py), the same FK and field lookup in the batch's precision, with the robot's
 * self-check setting.  Over every sample of a run two minima are kept:
 *   [0] fields: value - radius, over the live active spheres and every field of the run's scene that contains the sphere's
 *       centre.  A +inf value (a poisoned cell, a merged field's "no field here") is never the minimum, a NaN is ignored.
 *   [1] self: distance - (r_a + r_b), over the pairs of the verdict's self-collision leg (none with the self check off).
 * They are the subtractions the verdict compares to zero: min(clearance) < 0 exactly when the verdict says the run collides,
 * and then min(clearance) <= -depth.  Where a minimum is attained more than once the item of the lowest key counts
 * (sample, XML sphere, field -- or sample, XML sphere a, XML sphere b); the reduction is deterministic (an integer minimum
 * over the keys at the minimum, no floating-point atomic), so a run's outputs depend on its trajectory only, not on its
 * batch, its shard or a schedule.
 *   which 0: examine [n_runs] bytes, nonzero: examine the run (NULL is rejected).  which 1: the candidates, as
 *   orc_batch_collision_verdict_subset's which 1 (examine must be NULL; a batch never iterated is rejected).  which 2: every
 *   run (examine must be NULL).
 * The walk cannot stop early, so it is bounded by the caller: a run with duration > 0 and (C-space length / 0.04 >=
 * max_samples or a step that does not advance the clock) is TOO LONG, decided before anything of it is walked
 * (`clearance_too_long` of module.py).  max_samples lies in [1, 2^20]; a run the rule passes has at most max_samples + 2
 * samples.  A run of 2^20 samples occupies one workgroup for 16 384 chunks of 64 samples: measured once on an MI355X, alone
 * in a batch of one, 0.31 s (NOTES/clearance.md); the default of the Python layer is 65 536.
 * Outputs, clearance_out [n_runs][2] and n_samples_out [n_runs] required, the others may be NULL:
 *   an examined run: clearance_out the two minima widened to double from the batch's precision; time_out [n_runs][2] the time
 *     of each on the retimed trajectory; sphere_out [n_runs][2] the XML index of the sphere (of sphere a); other_out
 *     [n_runs][2] the index of the field, or the XML index of sphere b; n_samples_out the samples walked.  A minimum over
 *     nothing (no sample, no field that contains a sphere, no pairs) is +inf with time -1.0, sphere -1 and other -1.
 *   a run that is not examined: clearance NaN, time -1, sphere -1, other -1, n_samples -1; its workgroup returns before it
 *     stages anything.
 *   a run that is too long: the same with n_samples -2, AND THE CALL SUCCEEDS.
 * Several devices: every shard takes its slice, as the subset verdict does.
 * Rejected with a nonzero return and a message before any device work, the batch unchanged and the module usable: an unknown
 * batch; which outside 0..2; a NULL examine with which 0 or an examine with which 1 or 2; clearance_out or n_samples_out
 * NULL; max_samples outside [1, 2^20]; which 1 on a batch never iterated. */
int orc_batch_clearance(orc_module * mod, int batch_id, int which, const unsigned char * examine, int max_samples,
   double * clearance_out /* [n_runs][2]: fields, self */, double * time_out /* [n_runs][2] */,
   int * sphere_out /* [n_runs][2] */, int * other_out /* [n_runs][2]: field index; XML index of sphere b */,
   int * n_samples_out /* [n_runs] */);
/* The clearance of single configurations, on the device: the per-sample body of orc_batch_clearance's walk -- FK, every live
 * active sphere against every field of a scene, the self-collision pairs -- without a trajectory and a sample clock around it.
 * A configuration is one row of the batch's trajectories, n columns as orc_batch_dims reports (a floating base: columns 0..6
 * the pose, its quaternion renormalised as the walk renormalises a sample's); a precision-32 batch narrows the row to float
 * on upload, as orc_batch_set_traj does.  Query q is tested against the scene of run run_of_q[q] (NULL: run 0 for every
 * query) with what orc_batch_clearance would use at this moment: the batch's robot model, held bodies, live mask and pair
 * tables, and the robot's self-check setting.
 * orc_batch_config_clearance uploads configs [n_q][n].  orc_batch_waypoint_clearance reads T[run_of_q[q]][point_of_q[q]] of
 * the device's trajectories and uploads the two index arrays only; with both NULL, n_q must be n_runs * n_points and the
 * queries are every waypoint in storage order, the profile [n_runs][n_points].
 * Per query, any output may be NULL:
 *   clearance_out [n_q][2]: [0] the smallest value - radius over the live active spheres and the fields that contain them,
 *     [1] the smallest distance - (r_a + r_b) over the pairs; the subtractions of orc_batch_clearance, widened to double.  A
 *     trajectory with exactly one sample (0 < C-space length < 0.04) has the clearance of its first row, bit for bit.
 *   sphere_out / other_out [n_q][2]: XML sphere and field, XML spheres a and b, of the item of lowest key (sphere << 16 |
 *     other) among those that attain the minimum.
 *   A minimum over nothing (an empty scene, a configuration outside every field, the self check off) is +inf with -1, -1; a
 *   NaN gap is never a minimum.  A row with a non-finite entry is not evaluated: NaN and -1, -1 on both legs.
 * A query's answer depends on its row and its run only: not on its place in the list, on n_q, on the shard or on a schedule
 * (each query is reduced by one wavefront with shuffles; no atomic).  The calls leave no state: trajectories, momentum, costs,
 * status, verdict keys and the minima orc_batch_select_clear cached are untouched.  They are ordered on the shards' streams
 * like orc_batch_clearance: after orc_batch_iterate_async they see the trajectories that launch leaves.  Several devices: every
 * shard takes the queries whose run it owns; a list may interleave shards freely.
 * Rejected with a nonzero return and a message before any device work, the batch unchanged and the module usable: an unknown
 * batch; n_q < 1 or n_q > 2^22; configs NULL; a run_of_q entry outside [0, n_runs); a point_of_q entry outside [0, n_points);
 * exactly one of run_of_q / point_of_q NULL; both NULL with n_q != n_runs * n_points. */
int orc_batch_config_clearance(orc_module * mod, int batch_id, int n_q, const int * run_of_q,
   const double * configs /* [n_q][n] */, double * clearance_out /* [n_q][2] */, int * sphere_out, int * other_out /* [n_q][2] each */);
int orc_batch_waypoint_clearance(orc_module * mod, int batch_id, int n_q, const int * run_of_q, const int * point_of_q,
   double * clearance_out, int * sphere_out, int * other_out);
/* The clearance of given paths and of segments between waypoints, on the device: what orc_batch_clearance reports for a run
 * that holds the path as its trajectory, for paths that are no run's.  Query q returns clearance, time, sphere, other and
 * n_samples of that hypothetical run BIT FOR BIT, the run living in a batch with the same robot, held bodies, live mask, pair
 * tables and self-check setting, the same precision and velocity limits, and the scene of run run_of_q[q] (NULL: run 0 for
 * every query).  The batch's own n_points plays no part.
 * orc_batch_path_clearance uploads paths [n_q][n_rows][n], rows as orc_batch_set_traj takes them and narrowed to float for a
 * precision-32 batch as it narrows them; n_rows lies in [2, 4096].  Two rows are a segment: its answer is that of a 3-point run
 * holding [a, b, b], which has the same samples.  orc_batch_waypoint_segment_clearance takes the segment from
 * T[run_of_q[q]][from_of_q[q]] to T[run_of_q[q]][to_of_q[q]] of the device's trajectories and uploads the three index arrays
 * only; from > to is the reverse direction, from == to has no sample; it returns what orc_batch_path_clearance returns for
 * those two rows, bit for bit.
 * Retiming and samples are orc_batch_clearance's (verdict_samples of or_cdchomp_amd/module.py: a sample every 0.04 of C-space
 * length, the clock advanced by repeated addition while time < duration).  THE END ROW IS NOT A SAMPLE, exactly as the goal of a
 * run is not: ask orc_batch_config_clearance about it.  The too-long rule is orc_batch_clearance's with this call's max_samples
 * (in [1, 2^20]; `clearance_too_long` of module.py): such a query reports NaN, time -1, -1 / -1 and n_samples -2, AND THE CALL
 * SUCCEEDS.  A path of zero length has no sample: +inf, time -1, -1 / -1, n_samples 0.  Non-finite entries are decided by the
 * same rules as they stand: a NaN entry leaves one sample (or none) whose NaN gaps are never a minimum -- the spheres the entry
 * does not move still count --, an infinite entry makes the query too long; no memory is indexed by a value derived from one.
 * Outputs as orc_batch_clearance's with n_q in place of n_runs; clearance_out and n_samples_out required, the others may be
 * NULL.
 * The samples of all queries are packed: a workgroup walks 64 consecutive samples of the call (fewer for a robot whose rows do
 * not fit the LDS), whichever queries they belong to, so short segments share chunks.  They lie in a workspace of 2^21
 * samples (96 MiB at most, allocated at the size a call needs and freed at its end); a call with more is cut into rounds of
 * consecutive queries by the host.  A query's answer depends on its rows and its run only: not on its place in the list, on
 * n_q, on what shares a chunk with it, on the shard or on the rounds (a sample is reduced by one wavefront with shuffles, a
 * query by one wavefront over its samples in order; no atomic, ties to the lowest key as in orc_batch_clearance).  The calls
 * leave no state and are ordered on the shards' streams like orc_batch_clearance; the host waits once in their middle for the
 * sample counts.  Several devices: every shard takes the queries whose run it owns; a list may interleave shards freely.
 * Rejected with a nonzero return and a message before any device work, the batch unchanged and the module usable: an unknown
 * batch; n_q < 1 or n_q > 2^22; n_rows < 2 or n_rows > 4096; paths, clearance_out or n_samples_out NULL; max_samples outside
 * [1, 2^20]; a run_of_q entry outside [0, n_runs); from_of_q or to_of_q NULL, or an entry of theirs outside [0, n_points). */
int orc_batch_path_clearance(orc_module * mod, int batch_id, int n_q, const int * run_of_q /* NULL: run 0 */,
   int n_rows, const double * paths /* [n_q][n_rows][n] */, int max_samples,
   double * clearance_out /* [n_q][2] */, double * time_out /* [n_q][2] */,
   int * sphere_out, int * other_out /* [n_q][2] each */, int * n_samples_out /* [n_q] */);
int orc_batch_waypoint_segment_clearance(orc_module * mod, int batch_id, int n_q, const int * run_of_q,
   const int * from_of_q, const int * to_of_q, int max_samples,
   double * clearance_out, double * time_out, int * sphere_out, int * other_out, int * n_samples_out);
/* Which way is out: the penetration cost of single configurations and its gradient, on the device.  The queries, their rows,
 * runs and waypoints are those of the two clearance calls above, and so are the rules for n_q, run_of_q, point_of_q and configs.
 * With gap the quantity those calls take the minimum of, per query:
 *   cost_out [n_q][2]: [0] 1/2 sum max(0, margin_field - gap)^2 over the live active spheres and the fields that contain them,
 *     [1] 1/2 sum max(0, margin_self - gap)^2 over the pairs.  An item whose gap is not below its margin adds nothing: a
 *     poisoned (+inf) value, a NaN, a sphere outside a field.  The margins are rounded to the batch's precision.
 *   grad_out [n_q][n]: d(cost[0] + cost[1]) / d row[c], what a finite difference of the cost over the caller's row measures.  A
 *     field's slope is that of the cell the lookup interpolates in.  An inactive sphere is a constant; a pair whose centres
 *     coincide adds to the cost and not to the gradient.  A floating base: columns 0..2 take the force, columns 3..6 the
 *     derivative through the renormalisation of the quaternion (a factor 1 / |quaternion| of the caller's row); the 0.01 by
 *     which the optimizer scales its base block is not applied.
 *   clearance_out, sphere_out, other_out [n_q][2]: orc_batch_config_clearance's, bit for bit.
 * A row with a non-finite entry: NaN costs, NaN gradient, NaN minima and -1, -1.  Any output may be NULL.
 * As with the clearance calls, a query's answer depends on its row, its run and the margins only (every sum has a fixed order;
 * no atomic), the calls leave no state, and they are ordered on the shards' streams.  Rejected in addition to what those calls
 * reject: a margin that is negative, infinite or NaN. */
int orc_batch_config_penetration(orc_module * mod, int batch_id, int n_q, const int * run_of_q, const double * configs /* [n_q][n] */,
   double margin_field, double margin_self, double * cost_out /* [n_q][2] */, double * grad_out /* [n_q][n] */,
   double * clearance_out /* [n_q][2] */, int * sphere_out, int * other_out /* [n_q][2] each */);
int orc_batch_waypoint_penetration(orc_module * mod, int batch_id, int n_q, const int * run_of_q, const int * point_of_q,
   double margin_field, double margin_self, double * cost_out, double * grad_out, double * clearance_out, int * sphere_out, int * other_out);
/* ---- task space regions at single configurations: batched inverse kinematics for goals -----------------------------
 * "The hand at this pose" as configurations.  A TSR is what con_tsr, everyn_tsr and start_tsr of `create` take (struct tsr,
 * src/orcdchomp_mod.h:80-87), with the end effector it is about: */
typedef struct orc_tsr
{
   int ee_link;        /* link index; -1: the robot's active manipulator (its link and tool; `tool` below is ignored) */
   double tool[7];     /* end effector in the link frame */
   double T0w[7], Twe[7];
   double Bw[6][2];    /* x y z roll pitch yaw; a row is enforced iff Bw[i] == {0,0}, exactly as create's con_tsr (mod.cpp:2466-2480) */
} orc_tsr;
/* The value and the Jacobian of TSRs at given configurations, on the device; stateless.  Row q is configs[q] (the batch's
 * columns: 7 of a floating base, whose quaternion is used as given, then the active dofs) with tsrs[tsr_of_q[q]], or tsrs[0]
 * when tsr_of_q is NULL.  h_out [n_q][6]: the k enforced entries of the TSR's xyzrpy value in con_tsr's order (that of the Bw rows: x y z
 * roll pitch yaw), jac_out [n_q][6][n] (or NULL) their Jacobian rows; rows from k on are
 * zero.  These are the h and J the constraint step of iterate sees for a trajectory row: the same device function
 * (tsr_eval_point), the batch's model -- robot, base pose, active dofs, precision -- as `create` folded it.  A row with a
 * non-finite entry has NaN in its k rows.
 * Rejected with a nonzero return and a message before any device work, the module usable: an unknown batch; n_q < 1 or
 * n_q > 2^22; n_tsr < 1; a tsr_of_q entry outside [0, n_tsr); NULL tsrs, configs or h_out; an ee_link outside the robot's
 * links; ee_link -1 on a robot without a manipulator; a TSR with no enforced row or a non-finite pose; a robot whose
 * active dofs are no longer the batch's. */
int orc_batch_config_tsr(orc_module * mod, int batch_id, int n_tsr, const orc_tsr * tsrs, int n_q, const int * tsr_of_q /* NULL: tsr 0 */,
   const double * configs /* [n_q][n] */, double * h_out /* [n_q][6] */, double * jac_out /* [n_q][6][n] or NULL */);
/* Projects every row onto its TSR, the whole iteration on the device (one lane per row).  At iterate q with r = max_i |h_i|:
 * r <= tol: done, status 0.  Otherwise (J J^T + mu I_k) y = h by Cholesky in the order of the rows, dq = -J^T y, shortened to
 * step_cap in the 2-norm, q <- clip(q + dq, lower, upper) (lower, upper [n] or NULL: no box).  Status 1: a pivot that is not
 * positive and finite, or a step that moves no entry; 2: out of steps; 3: a row with a non-finite entry (every output of the
 * row NaN, 0 steps).  A row that is not done comes back as the visited iterate of smallest r, never worse than the input; a
 * row within tol, and every row when max_steps is 0, comes back bit for bit with 0 steps, and so does every entry that a
 * projection leaves where it was (a dof that does not move the link), in a precision-32 batch too.  resid_out is r of the returned
 * row.  The arithmetic is in the batch's precision, the outputs are doubles; or_cdchomp_amd/project.py is the rule.
 * A row's answer depends on the row, its TSR and the parameters only: not on its place, on n_q, or on the shard.
 * Rejected as above, and: a NULL output; a NaN or non-positive tol or step_cap; a NaN or negative mu; max_steps outside
 * [0, 256]; lower[c] > upper[c]; a floating-base batch (the update of a quaternion column is not defined here). */
int orc_batch_project_tsr(orc_module * mod, int batch_id, int n_tsr, const orc_tsr * tsrs, int n_q, const int * tsr_of_q,
   const double * configs, const double * lower, const double * upper /* [n] each or NULL */, int max_steps, double tol, double mu,
   double step_cap, double * configs_out /* [n_q][n] */, double * resid_out /* [n_q] */, int * steps_out, int * status_out);
/* Projects every row onto its TSR and moves it out of contact at once, on the device; or_cdchomp_amd/project_clear.py is the
 * rule.  Row q is tested against the scene of run run_of_q[q] as orc_batch_config_penetration tests it.  Per round
 * it = 0 .. max_steps the penetration cost U = cost[0] + cost[1], its gradient g and the two clearances are taken at the
 * iterate at the margins (margin_field + slack, margin_self + slack), and h, J and r = max_i |h_i| as orc_batch_project_tsr
 * takes them.  The iterate is `on` when r <= tol and `clear` when clearance[0] >= margin_field and clearance[1] >= margin_self
 * (a NaN is never clear).  Its key is class 0 (on and clear), class 1 (on, compared by U) or class 2 (anything else, compared
 * by r): the lower class wins, within a class the smaller value, a NaN is never better and anything beats a NaN, the earlier
 * iterate keeps a tie; the best iterate is what comes back.  On and clear: status 0.  it == max_steps: status 2.  Otherwise
 * one step: A = J J^T + mu I_k factored by orc_batch_project_tsr's Cholesky, dq = -J^T A^-1 h; where U is finite and positive
 * and g finite, g_N = g - J^T A^-1 (J g), s = g_N . g_N, and where s is finite and positive p = -(2U / s) g_N, shortened to
 * push_cap in the 2-norm, is added to dq; dq is shortened to step_cap, q <- clip(q + dq, lower, upper).  Status 1: a pivot that
 * is not positive and finite, or a step that moves no entry; 3: a row with a non-finite entry (every output of the row NaN, 0
 * steps).  A row that starts on its TSR and clear, and every row when max_steps is 0, comes back bit for bit with 0 steps, and so
 * does every entry the loop leaves where it was, in a precision-32 batch too.  resid_out is r and clearance_out [n_q][2] the
 * clearance of the returned row; steps_out counts the steps taken.  The arithmetic is in the batch's precision, the outputs
 * are doubles.  One launch of orc_batch_config_penetration's kernel and one of the step kernel per round, on the stream of the
 * shard that owns the row's run.
 * A row's answer depends on the row, its TSR, its run and the parameters only: not on its place, on n_q, or on the shard.
 * Rejected with a nonzero return and a message before any device work, the module usable: everything orc_batch_project_tsr
 * rejects (a floating-base batch included; clearance_out may not be NULL either); everything orc_batch_config_penetration
 * rejects about run_of_q and the margins; a NaN or non-positive push_cap; a NaN, negative or infinite slack. */
int orc_batch_project_tsr_clear(orc_module * mod, int batch_id, int n_tsr, const orc_tsr * tsrs, int n_q, const int * tsr_of_q,
   const int * run_of_q /* NULL: run 0 */, const double * configs, const double * lower, const double * upper, int max_steps,
   double tol, double mu, double step_cap, double push_cap, double margin_field, double margin_self, double slack,
   double * configs_out, double * resid_out, double * clearance_out /* [n_q][2] */, int * steps_out, int * status_out);
/* The best run of every group among those that keep a margin.  n_groups and group_of_run as in orc_batch_select_best.  A run
 * is eligible when all three hold: it is a candidate (status 0 or 1 and a finite total cost); it was walked, i.e. is not too
 * long for max_samples; fmin(clearance[0], clearance[1]) >= margin.  margin 0 is orc_batch_select_best_by's
 * require_collision_free.  cost_column 0..2: orc_batch_select_best_by's key and tie rule.  cost_column 3: the largest
 * clearance wins, a tie goes to the lowest run index, and best_cost_out is -clearance, so "lowest wins" holds for every
 * column.  best_run_out [n_groups] (-1 for a group without an eligible run), best_cost_out [n_groups] (+inf there),
 * best_clearance_out [n_groups] the winner's fmin of the two minima (NaN there), n_eligible_out [n_groups]; n_samples_out
 * [n_runs] as orc_batch_clearance(which 1) reports it; any output may be NULL.  `select_clear` of module.py is the rule.
 * On the device: the clearance kernel runs over the candidates only, the minima stay there, a segmented arg-min reads them;
 * n_groups rows come back, and n_samples_out if asked for.  Several devices: every shard reduces its runs and the host merges
 * n_shards x n_groups candidates by the same rule; groups may span shards.
 * Rejected with a nonzero return and a message before any device work, the batch unchanged and the module usable: an unknown
 * batch; a batch never iterated; cost_column outside 0..3; a NaN margin (+-inf are accepted); max_samples outside [1, 2^20];
 * n_groups < 1, a group_of_run entry outside [0, n_groups), or a NULL group_of_run with n_runs % n_groups != 0. */
int orc_batch_select_clear(orc_module * mod, int batch_id, int cost_column, int n_groups, const int * group_of_run,
   double margin, int max_samples,
   int * best_run_out, double * best_cost_out, double * best_clearance_out, int * n_eligible_out, int * n_samples_out);
/* The rows runs[0 .. n_sel) of what orc_batch_gettraj returns, gathered on the device and copied as n_sel n_points n
 * doubles: traj_out [n_sel][n_points][n].  An entry -1 (what orc_batch_select_best reports for a group without an
 * eligible run) gives a row of NaN; duplicates are allowed; runs that live on different shards work.  Any other entry
 * outside [0, n_runs), a NULL array or a short buffer is an error, found before anything is written to traj_out. */
int orc_batch_gettraj_runs(orc_module * mod, int batch_id, const int * runs, int n_sel, double * traj_out, size_t cap_doubles);
/* the collision report the last gettraj produced (the reference logs it, mod.cpp:3000) */
const char * orc_last_collision_details(const orc_module * mod);
/* replaces mod::destroy (src/orcdchomp_mod.cpp:3013-3066) */
int orc_batch_destroy(orc_module * mod, int batch_id);

/* ---- measurement -------------------------------------------------------------
 * average device time (ms) of the iterate kernel launches since the last reset,
 * measured with HIP events on the module's stream; count of launches */
int orc_kernel_time(orc_module * mod, double * total_ms, int * launches, int reset);

/* ---- host utilities (no GPU needed) -------------------------------------------
 * the host-side numerics of the path, callable on their own */
/* occupancy (0.0 free, HUGE_VAL obstacle) -> signed distance field, positive outside:
 * replaces cd_grid_double_bin_sdf (src/libcd/grid.c:637-687) */
int orc_host_bin_sdf(const int sizes[3], const double lengths[3], const double * occupancy, double * sdf_out);
/* flood fill from cell `start`, 1.0 -> 0.0, axis neighbours: replaces cd_grid_flood_fill with
 * replace_1_to_0 (src/libcd/grid_flood.c:30-111, src/orcdchomp_mod.cpp:160-168); in place */
int orc_host_flood_fill(const int sizes[3], double * cells, size_t start);
/* occupancy the way computedistancefield forms it (src/orcdchomp_mod.cpp:462-531): a cube of
 * half-extent cube_extent swept over the cell centres of a grid rooted at pose_world_gsdf against
 * oriented boxes given in the world (box_world_poses [n_boxes][7], half_extents [n_boxes][3]; the
 * stand-in for OpenRAVE's CheckCollision): occupancy_out gets HUGE_VAL where it touches, 1.0 elsewhere */
int orc_host_voxelize_boxes(const int sizes[3], const double lengths[3], const double pose_world_gsdf[7], double cube_extent,
   int n_boxes, const double * box_world_poses, const double * half_extents, double * occupancy_out);
/* ... and of a triangle mesh (world_vertices [n_tri][3][3]): HUGE_VAL where the cube touches a triangle */
int orc_host_voxelize_trimesh(const int sizes[3], const double lengths[3], const double pose_world_gsdf[7], double cube_extent,
   int n_tri, const double * world_vertices, double * occupancy_out);
/* the grid orc_scene_merge_fields merges into: source_lengths [n_sources][3] and source_poses [n_sources][7], every source
 * grid's box and its pose in the TARGET KINBODY's frame; cell and bounds as there (with bounds the sources are not read and
 * n_sources may be 0).  pose_out is the merged grid's pose in the target kinbody's frame.  Nonzero on what that call rejects */
int orc_host_merge_grid(int n_sources, const double * source_lengths, const double * source_poses, double cell, const double * bounds,
   int sizes_out[3], double lengths_out[3], double pose_out[7]);
/* the host twin of the merge kernel: the grid (sizes, lengths) rooted at pose_world_gsdf filled from n_sources grids given by
 * source_sizes [n][3], source_lengths [n][3], source_poses [n][7] (every source GRID's world pose) and source_data [n]
 * (C ordered cells); data_out [sizes[0] sizes[1] sizes[2]].  Same function, same operations as the device: bit for bit */
int orc_host_merge_fields(int n_sources, const int * source_sizes, const double * source_lengths, const double * source_poses,
   const double * const * source_data, const int sizes[3], const double lengths[3], const double pose_world_gsdf[7], double * data_out);
/* tokenizer of the command grammar: replaces cd_util_shparse (src/libcd/util_shparse.c:37-128).
 * tokens are written NUL-separated into out; returns the token count or -1 if out is too small */
int orc_host_shparse(const char * in, char * out, size_t out_cap);
/* smoothness metric of cd_chomp_init (src/libcd/chomp.c:239-340, 393-403) in the form the
 * kernels use: dense A [m][m], endpoint couplings beta_s/beta_g [m], kappa[3] = kss ksg kgg
 * (trC), and A^-1 applied to rhs [m][ncols] by what the device uses: the cyclic-reduction tables (D=1), the
 * generators of the band inverse (2 <= D <= 4: rank-D semiseparable form, D prefix and D suffix scans
 * per column; replaces the dense dgetrf/dgetri inverse of src/libcd/chomp.c:393-403) or the dense
 * inverse (D > 4); any output may be NULL */
int orc_host_metric(int m, int derivative, double dt, double * A_out, double * beta_s_out, double * beta_g_out,
   double kappa_out[3], const double * rhs, int ncols, double * solve_out);
/* the same with the start point a variable (`start_tsr`: inits[0] == NULL, src/orcdchomp_mod.cpp:2572) */
int orc_host_metric_free_start(int m, int derivative, double dt, double * A_out, double * beta_s_out, double * beta_g_out,
   double kappa_out[3], const double * rhs, int ncols, double * solve_out);
/* rank of the semiseparable form of A^-1 the device applies for this metric (0: none -- derivative 1 has its closed
 * form, derivative > 4 the dense inverse); -1 on bad arguments */
int orc_host_metric_semisep_rank(int m, int derivative, double dt, int free_start);
/* which form of the structured constraint solve the iterate kernel takes for `threads` per workgroup, m moving waypoints, n
 * columns and n_max = n + (most constrained rows on one point): the kernel's own decision (csrc/tsr_form.h).  out: lanes per
 * row of the register form (16, 32; 0: the one-wavefront LDS form), registers per lane, 1 for the augmented block, the meet
 * form (tsr_meet_regs<2>, <4>; 0: tsr_meet), the substitution form's two template numbers.  Nonzero on bad arguments */
int orc_host_tsr_form(int threads, int m, int n, int n_max, int out[6]);
/* GSL's default generator restated (src/orcdchomp_mod.cpp:2303-2304,2763,2767): n gaussians with
 * the given sigma from seed, then one uniform; out_gauss[n], out_uniform[1] */
int orc_host_gsl_stream(unsigned long seed, double sigma, int n, double * out_gauss, double * out_uniform);
/* the sample plan of the collision verdict for one trajectory [n_points][n], by the functions orc_batch_collision_verdict
 * runs: retimed at vmax [n - col0] (an entry <= 0 counts as 1) over the columns col0 .. n-1, a sample every 0.04 of
 * C-space distance; per sample the segment it lies on, the position on the segment and its time.  n_samples_out gets
 * their number; the arrays (any may be NULL) are filled when cap holds them all, otherwise the return is nonzero */
int orc_host_verdict_samples(const double * traj, int n_points, int n, int col0, const double * vmax, int cap,
   int * seg_out, double * u_out, double * time_out, int * n_samples_out);

#ifdef __cplusplus
}
#endif
#endif
