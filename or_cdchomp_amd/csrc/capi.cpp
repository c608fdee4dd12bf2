// capi.cpp -- the extern "C" boundary declared in include/orcdchomp_amd.h.
#include "../../include/orcdchomp_amd.h"
#include "module.h"
#include <cstring>
#include <new>
#include <stdexcept>

struct orc_module
{
   orc::Module * impl;
   std::string last_error;
};

namespace {
std::string g_new_error;

template <typename F>
int guarded(orc_module * mod, F f)
{
   if (!mod) return 2;
   // every entry point asserts the module's (first) device for the calling thread: modules on
   // different GPUs may share a process, and callers may come from any thread
   try { orc::DeviceGuard guard(mod->impl->device); f(); mod->last_error.clear(); return 0; }
   catch (const std::exception & e) { mod->last_error = e.what(); return 1; }
   catch (...) { mod->last_error = "unknown error"; return 1; }
}

// a C caller's mistakes come back as error codes, never as a fault inside the library
void need(const void * p, const char * what)
{
   if (!p) throw std::runtime_error(std::string("null argument: ") + what);
}
const char * str(const char * s, const char * what) { need(s, what); return s; }

orc::BatchParams to_params(const orc_batch_params & p)
{
   orc::BatchParams q;
   q.n_points = p.n_points; q.floating_base = p.floating_base; q.lambda = p.lambda;
   q.derivative = p.derivative; q.use_momentum = p.use_momentum; q.use_hmc = p.use_hmc;
   q.hmc_resample_lambda = p.hmc_resample_lambda; q.epsilon = p.epsilon; q.epsilon_self = p.epsilon_self;
   q.obs_factor = p.obs_factor; q.obs_factor_self = p.obs_factor_self; q.precision = p.precision;
   return q;
}

// the same validation the create command performs (mod.cpp:2091-2097); no_fields: the call plans with the module's field list and
// that list is empty (orc_batch_create_scenes brings its fields in the scene table and passes false)
void check_create(const orc::BatchParams & q, int n_runs, const double * goals, const double * basegoals, bool no_fields)
{
   if (!goals) throw std::runtime_error("Did not pass either adofgoal or starttraj!");
   if (q.floating_base && !basegoals) throw std::runtime_error("Passed floating_base with no basegoal!");
   if (!q.floating_base && basegoals) throw std::runtime_error("Passed basegoal with no floating_base!");
   if (no_fields) throw std::runtime_error("No signed distance fields have yet been computed!");
   if (q.lambda < 0.01) throw std::runtime_error("lambda must be >=0.01!");
   if (q.n_points < 3) throw std::runtime_error("n_points must be >=3!");
   if (n_runs < 1) throw std::runtime_error("n_runs must be >=1!");
}
}

extern "C" {

orc_module * orc_module_new(int device)
{
   try
   {
      orc_module * m = new orc_module;
      m->impl = new orc::Module(device);
      return m;
   }
   catch (const std::exception & e) { g_new_error = e.what(); return nullptr; }
}

orc_module * orc_module_new_multi(const int * devices, int n_devices)
{
   try
   {
      if (!devices || n_devices < 1) throw std::runtime_error("orcdchomp_amd: empty device list");
      orc_module * m = new orc_module;
      m->impl = new orc::Module(std::vector<int>(devices, devices + n_devices));
      return m;
   }
   catch (const std::exception & e) { g_new_error = e.what(); return nullptr; }
}

void orc_module_free(orc_module * mod)
{
   if (!mod) return;
   delete mod->impl;
   delete mod;
}

const char * orc_last_error(const orc_module * mod)
{
   if (!mod) return g_new_error.c_str();
   return mod->last_error.c_str();
}

int orc_set_stream(orc_module * mod, void * hip_stream)
{
   return guarded(mod, [&] { mod->impl->stream = (hipStream_t) hip_stream; });
}

int orc_set_num_streams(orc_module * mod, int n)
{
   return guarded(mod, [&] { mod->impl->set_num_streams(n < 0 ? 0 : n); });
}

int orc_send_command(orc_module * mod, const char * cmd, char * out, size_t out_cap)
{
   return guarded(mod, [&] {
      mod->impl->last_reply = mod->impl->send_command(cmd ? cmd : "");
      if (out && out_cap)
      {
         const size_t k = std::min(out_cap - 1, mod->impl->last_reply.size());
         std::memcpy(out, mod->impl->last_reply.data(), k);
         out[k] = 0;
      }
   });
}

size_t orc_last_reply_size(const orc_module * mod) { return mod ? mod->impl->last_reply.size() : 0; }

int orc_last_reply(const orc_module * mod, char * out, size_t out_cap)
{
   if (!mod || !out || !out_cap) return 2;
   const size_t k = std::min(out_cap - 1, mod->impl->last_reply.size());
   std::memcpy(out, mod->impl->last_reply.data(), k);
   out[k] = 0;
   return 0;
}

int orc_env_add_robot(orc_module * mod, const char * name, const orc_robot_desc * d)
{
   return guarded(mod, [&] {
      need(name, "name"); need(d, "robot description");
      if (d->n_links < 1 || d->n_dof < 0 || d->n_spheres < 0) throw std::runtime_error("bad robot description: counts!");
      need(d->parent, "parent"); need(d->pose_parent_joint, "pose_parent_joint"); need(d->joint_type, "joint_type");
      need(d->axis, "axis"); need(d->dof_index, "dof_index");
      if (d->n_dof) { need(d->limit_lower, "limit_lower"); need(d->limit_upper, "limit_upper"); }
      if (d->n_spheres) { need(d->sphere_link, "sphere_link"); need(d->sphere_pos, "sphere_pos"); need(d->sphere_radius, "sphere_radius"); }
      for (int i=0; i<d->n_links; i++)
      {
         const int jt = d->joint_type[i], dof = d->dof_index[i];
         if (jt < 0 || jt > 2) throw std::runtime_error("bad robot description: joint type (0 fixed, 1 revolute, 2 prismatic)!");
         if (jt == 0 ? dof != -1 : (dof < 0 || dof >= d->n_dof)) throw std::runtime_error("bad robot description: dof index of a joint!");
         const double * a = d->axis + 3*i;
         const double a2 = a[0]*a[0] + a[1]*a[1] + a[2]*a[2];
         if (jt != 0 && !(a2 > 0.0 && a2 < 1e300)) throw std::runtime_error("bad robot description: joint axis!");
      }
      orc::Robot r;
      r.name = name;
      r.n_links = d->n_links;
      r.parent.assign(d->parent, d->parent + d->n_links);
      for (int i=0; i<d->n_links; i++)
      {
         if (r.parent[i] >= i) throw std::runtime_error("links must be in topological order!");
         r.pose_parent_joint.push_back(orc::Pose(d->pose_parent_joint + 7*i));
      }
      r.joint_type.assign(d->joint_type, d->joint_type + d->n_links);
      r.axis.assign(d->axis, d->axis + 3*d->n_links);
      r.dof_index.assign(d->dof_index, d->dof_index + d->n_links);
      r.n_dof = d->n_dof;
      r.limit_lower.assign(d->limit_lower, d->limit_lower + d->n_dof);
      r.limit_upper.assign(d->limit_upper, d->limit_upper + d->n_dof);
      for (int s=0; s<d->n_spheres; s++)
      {
         orc::Robot::Sphere sp;
         sp.link = d->sphere_link[s];
         if (sp.link < 0 || sp.link >= d->n_links) throw std::runtime_error("link in <orcdchomp> does not exist.");
         for (int k=0; k<3; k++) sp.pos[k] = d->sphere_pos[3*s+k];
         sp.radius = d->sphere_radius[s];
         if (!(sp.radius > 0.0 && sp.radius < 1e300)) throw std::runtime_error("bad robot description: sphere radius!");
         r.spheres.push_back(sp);
      }
      r.dof_values.assign(d->n_dof, 0.0);
      for (int i=0; i<d->n_dof; i++) r.active_dofs.push_back(i);
      mod->impl->env.add_robot(r);
   });
}

int orc_robot_set_transform(orc_module * mod, const char * name, const double pose[7])
{
   return guarded(mod, [&] { need(pose, "pose"); mod->impl->env.robot(str(name, "name")).transform = orc::Pose(pose); });
}

int orc_robot_set_dof_values(orc_module * mod, const char * name, const double * values, int n)
{
   return guarded(mod, [&] {
      orc::Robot & r = mod->impl->env.robot(str(name, "name"));
      if (n != r.n_dof) throw std::runtime_error("wrong number of dof values!");
      if (n) need(values, "values");
      r.dof_values.assign(values, values + n);
   });
}

int orc_robot_set_active_dofs(orc_module * mod, const char * name, const int * indices, int n)
{
   return guarded(mod, [&] {
      orc::Robot & r = mod->impl->env.robot(str(name, "name"));
      if (n < 0) throw std::runtime_error("bad dof index!");
      if (n) need(indices, "indices");
      for (int i=0; i<n; i++) if (indices[i] < 0 || indices[i] >= r.n_dof) throw std::runtime_error("bad dof index!");
      r.active_dofs.assign(indices, indices + n);
   });
}

int orc_robot_set_velocity_limits(orc_module * mod, const char * name, const double * limits, int n)
{
   return guarded(mod, [&] {
      orc::Robot & r = mod->impl->env.robot(str(name, "name"));
      if (n != r.n_dof) throw std::runtime_error("wrong number of velocity limits!");
      if (n) need(limits, "limits");
      r.limit_vel.assign(limits, limits + n);
   });
}

int orc_set_workgroup_threads(orc_module * mod, int threads)
{
   return guarded(mod, [&] {
      if (threads != 0 && threads != 128 && threads != 192 && threads != 256 && threads != 512)
         throw std::runtime_error("workgroup threads must be 0 (default), 128, 192, 256 or 512!");
      mod->impl->workgroup_threads = threads;
   });
}

int orc_set_workgroups_per_cu(orc_module * mod, int workgroups)
{
   return guarded(mod, [&] {
      if (workgroups != 0 && workgroups != 3 && workgroups != 4) throw std::runtime_error("workgroups per CU must be 0 (the planner's choice), 3 or 4!");
      mod->impl->workgroups_per_cu = workgroups;
   });
}

int orc_robot_set_link_names(orc_module * mod, const char * name, const char * const * names, int n)
{
   return guarded(mod, [&] {
      orc::Robot & r = mod->impl->env.robot(str(name, "name"));
      if (n != r.n_links) throw std::runtime_error("wrong number of link names!");
      need(names, "names");
      for (int i=0; i<n; i++) need(names[i], "a link name");
      r.link_names.assign(names, names + n);
   });
}

int orc_robot_add_manipulator(orc_module * mod, const char * name, const char * manip, int ee_link, const double tool_pose[7])
{
   return guarded(mod, [&] {
      orc::Robot & r = mod->impl->env.robot(str(name, "name"));
      if (ee_link < 0 || ee_link >= r.n_links) throw std::runtime_error("manipulator end-effector link out of range!");
      orc::Robot::Manip m;
      m.name = str(manip, "manipulator name"); m.link = ee_link;
      if (tool_pose) m.tool = orc::Pose(tool_pose);
      r.manips.push_back(m);
   });
}

int orc_robot_set_adjacent_links(orc_module * mod, const char * name, const int * link_pairs, int n_pairs)
{
   return guarded(mod, [&] {
      orc::Robot & r = mod->impl->env.robot(str(name, "name"));
      if (n_pairs < 0 || (n_pairs > 0 && !link_pairs)) throw std::runtime_error("bad adjacent link list!");
      r.adjacent.clear();
      for (int k=0; k<n_pairs; k++)
      {
         const int a = link_pairs[2*k], b = link_pairs[2*k+1];
         if (a < 0 || a >= r.n_links || b < 0 || b >= r.n_links) throw std::runtime_error("adjacent link out of range!");
         r.adjacent.push_back(std::make_pair(a, b));
      }
   });
}

int orc_robot_set_self_check(orc_module * mod, const char * name, int enabled)
{
   return guarded(mod, [&] { mod->impl->env.robot(str(name, "name")).self_check = enabled != 0; });
}

int orc_robot_set_active_manipulator(orc_module * mod, const char * name, const char * manip)
{
   return guarded(mod, [&] {
      orc::Robot & r = mod->impl->env.robot(str(name, "name"));
      for (size_t k=0; k<r.manips.size(); k++)
         if (r.manips[k].name == str(manip, "manipulator name")) { r.active_manip = (int) k; return; }
      throw std::runtime_error("manipulator not found!");
   });
}

int orc_env_add_kinbody_boxes(orc_module * mod, const char * name, int n_boxes, const double * box_poses, const double * half_extents)
{
   return guarded(mod, [&] {
      need(name, "name");
      if (n_boxes < 0) throw std::runtime_error("bad number of boxes!");
      if (n_boxes) { need(box_poses, "box_poses"); need(half_extents, "half_extents"); }
      orc::KinBody k;
      k.name = name;
      for (int i=0; i<n_boxes; i++)
      {
         orc::KinBody::B b;
         b.pose = orc::Pose(box_poses + 7*i);
         for (int q=0; q<3; q++) b.half[q] = half_extents[3*i+q];
         k.boxes.push_back(b);
      }
      mod->impl->env.add_kinbody(k);
   });
}

int orc_env_add_kinbody_trimesh(orc_module * mod, const char * name, int n_tri, const double * vertices)
{
   return guarded(mod, [&] {
      if (n_tri < 1) throw std::runtime_error("a mesh needs at least one triangle!");
      need(vertices, "vertices");
      if (n_tri > (1 << 26)) throw std::runtime_error("too many triangles in one mesh (at most 2^26)!");
      for (size_t i=0; i<9*(size_t) n_tri; i++) if (!std::isfinite(vertices[i])) throw std::runtime_error("mesh vertices must be finite numbers!");
      const std::string nm = str(name, "name");
      if (mod->impl->env.has_body(nm))
      {
         // a kinbody of boxes gets its mesh geometry added (a body may have both kinds); a robot of that name is an error.
         // A body whose distance field exists already keeps the field of its OLD geometry (computedistancefield refuses a second
         // one: "We already have an sdf for this kinbody!"), so new geometry for it is an error here, not a stale field later
         if (mod->impl->env.find_sdf(nm)) throw std::runtime_error("that kinbody has a distance field already: removefield first!");
         orc::KinBody & k = mod->impl->env.kinbody(nm);
         k.tris.insert(k.tris.end(), vertices, vertices + 9*(size_t) n_tri);
         return;
      }
      orc::KinBody k;
      k.name = nm;
      k.tris.assign(vertices, vertices + 9*(size_t) n_tri);
      mod->impl->env.add_kinbody(k);
   });
}

int orc_kinbody_set_transform(orc_module * mod, const char * name, const double pose[7])
{
   return guarded(mod, [&] { need(pose, "pose"); mod->impl->env.set_kinbody_transform(str(name, "name"), orc::Pose(pose)); });
}

int orc_kinbody_set_spheres(orc_module * mod, const char * name, int n_spheres, const double * sphere_pos, const double * sphere_radius)
{
   return guarded(mod, [&] {
      orc::KinBody & k = mod->impl->env.kinbody(str(name, "name"));
      if (n_spheres < 0) throw std::runtime_error("bad number of spheres!");
      if (n_spheres) { need(sphere_pos, "sphere_pos"); need(sphere_radius, "sphere_radius"); }
      k.spheres.clear();
      for (int i=0; i<n_spheres; i++)
      {
         orc::Robot::Sphere sp;
         sp.link = 0; sp.radius = sphere_radius[i];
         for (int q=0; q<3; q++) sp.pos[q] = sphere_pos[3*i+q];
         k.spheres.push_back(sp);
      }
      mod->impl->env.refresh_grab_contacts(k.name);      // (a held body's contacts were taken with its old spheres)
   });
}

int orc_robot_grab(orc_module * mod, const char * robot, const char * kinbody, int link)
{
   return guarded(mod, [&] { mod->impl->env.grab(str(robot, "robot"), str(kinbody, "kinbody"), link); });
}

int orc_robot_release(orc_module * mod, const char * robot, const char * kinbody)
{
   return guarded(mod, [&] { mod->impl->env.release(str(robot, "robot"), str(kinbody, "kinbody")); });
}

int orc_robot_release_all(orc_module * mod, const char * robot)
{
   return guarded(mod, [&] { mod->impl->env.release_all(str(robot, "robot")); });
}

int orc_body_get_transform(orc_module * mod, const char * name, double pose_out[7])
{
   return guarded(mod, [&] {
      need(pose_out, "pose_out");
      if (!mod->impl->env.has_body(str(name, "name"))) throw std::runtime_error("Could not find kinbody with that name!");
      const orc::Pose p = mod->impl->env.body_transform(name);
      for (int i=0; i<7; i++) pose_out[i] = p.v[i];
   });
}

int orc_kinbody_enable(orc_module * mod, const char * name, int enabled)
{
   return guarded(mod, [&] { mod->impl->env.kinbody(str(name, "name")).enabled = enabled != 0; });
}

int orc_scene_add_sdf(orc_module * mod, const char * kinbody, const int sizes[3], const double lengths[3],
   const double pose[7], const double * data)
{
   return guarded(mod, [&] {
      need(kinbody, "kinbody"); need(sizes, "sizes"); need(lengths, "lengths"); need(pose, "pose"); need(data, "data");
      if (!mod->impl->env.has_body(kinbody)) throw std::runtime_error("Could not find kinbody with that name!");
      for (int i=0; i<3; i++) if (sizes[i] < 2 || !(lengths[i] > 0.0)) throw std::runtime_error("sdf grids need at least 2 cells per dimension and positive lengths!");
      orc::Grid g;
      for (int i=0; i<3; i++) { g.sizes[i] = sizes[i]; g.lengths[i] = lengths[i]; }
      g.data.assign(data, data + g.ncells());
      mod->impl->env.add_sdf(kinbody, g, orc::Pose(pose));
   });
}

int orc_scene_get_sdf(orc_module * mod, const char * kinbody, int sizes[3], double lengths[3], double pose[7],
   double * data, size_t data_cap)
{
   return guarded(mod, [&] {
      need(kinbody, "kinbody"); need(sizes, "sizes"); need(lengths, "lengths"); need(pose, "pose");
      orc::Sdf * s = mod->impl->env.find_sdf(kinbody);
      if (!s) throw std::runtime_error("No sdf for that kinbody!");
      for (int i=0; i<3; i++) { sizes[i] = s->grid.sizes[i]; lengths[i] = s->grid.lengths[i]; }
      for (int i=0; i<7; i++) pose[i] = s->pose.v[i];
      if (data)
      {
         if (data_cap < s->grid.ncells()) throw std::runtime_error("buffer too small!");
         std::memcpy(data, s->grid.data.data(), s->grid.ncells() * sizeof(double));
      }
   });
}

int orc_scene_merge_fields(orc_module * mod, const char * target_kinbody, int n_fields, const char * const * field_kinbodies,
   const double * field_poses, double cell, const double * bounds)
{
   return guarded(mod, [&] {
      need(target_kinbody, "target_kinbody");
      if (n_fields < 1) throw std::runtime_error("n_fields must be >=1!");
      need(field_kinbodies, "field_kinbodies");
      std::vector<std::string> names;
      for (int k=0; k<n_fields; k++) names.push_back(str(field_kinbodies[k], "field_kinbodies entry"));
      mod->impl->merge_fields(target_kinbody, names, field_poses, cell, bounds);
   });
}

void orc_batch_params_default(orc_batch_params * p)
{
   if (!p) return;
   orc::BatchParams d;
   p->n_points = d.n_points; p->floating_base = d.floating_base; p->lambda = d.lambda;
   p->derivative = d.derivative; p->use_momentum = d.use_momentum; p->use_hmc = d.use_hmc;
   p->hmc_resample_lambda = d.hmc_resample_lambda; p->epsilon = d.epsilon; p->epsilon_self = d.epsilon_self;
   p->obs_factor = d.obs_factor; p->obs_factor_self = d.obs_factor_self; p->precision = d.precision;
}

int orc_batch_create(orc_module * mod, const char * robot, const orc_batch_params * p, int n_runs,
   const double * starts, const double * goals, const double * basegoals, const unsigned int * seeds, int * batch_id)
{
   return guarded(mod, [&] {
      need(robot, "robot"); need(p, "params"); need(batch_id, "batch_id");
      const orc::BatchParams q = to_params(*p);
      check_create(q, n_runs, goals, basegoals, mod->impl->env.sdfs.empty());
      *batch_id = mod->impl->create_batch(robot, q, n_runs, starts, goals, basegoals, seeds);
   });
}

int orc_batch_create_scenes(orc_module * mod, const char * robot, const orc_batch_params * p, int n_runs,
   const double * starts, const double * goals, const double * basegoals, const unsigned int * seeds,
   int n_scenes, const int * scene_begin, const char * const * field_kinbodies, const double * field_poses,
   const int * scene_of_run, int * batch_id)
{
   return guarded(mod, [&] {
      need(robot, "robot"); need(p, "params"); need(batch_id, "batch_id");
      const orc::BatchParams q = to_params(*p);
      check_create(q, n_runs, goals, basegoals, false);
      // the scene table
      if (n_scenes < 1) throw std::runtime_error("n_scenes must be >=1!");
      need(scene_begin, "scene_begin"); need(scene_of_run, "scene_of_run");
      if (scene_begin[0] != 0) throw std::runtime_error("scene_begin[0] must be 0!");
      for (int sc=0; sc<n_scenes; sc++)
      {
         if (scene_begin[sc+1] < scene_begin[sc]) throw std::runtime_error("scene_begin must be non-decreasing!");
         if (scene_begin[sc+1] - scene_begin[sc] > ORC_MAX_SDFS) throw std::runtime_error("too many signed distance fields for this build!");
      }
      const int n_fields = scene_begin[n_scenes];
      if (n_fields > 0) need(field_kinbodies, "field_kinbodies");
      std::shared_ptr<orc::SceneTable> t = std::make_shared<orc::SceneTable>();
      t->scenes.resize(n_scenes);
      for (int sc=0; sc<n_scenes; sc++)
         for (int k=scene_begin[sc]; k<scene_begin[sc+1]; k++)
         {
            const std::string name = str(field_kinbodies[k], "field_kinbodies entry");
            if (!mod->impl->env.has_body(name)) throw std::runtime_error("Kinbody " + name + " of a scene does not exist!");
            std::shared_ptr<orc::Sdf> field;
            for (const auto & f : mod->impl->env.sdfs) if (f->kinbody_name == name) field = f;
            if (!field) throw std::runtime_error("Kinbody " + name + " of a scene has no signed distance field!");
            orc::Pose pose;
            if (field_poses) for (int j=0; j<7; j++) pose.v[j] = field_poses[(size_t) k*7 + j];
            else pose = mod->impl->env.body_transform(name);
            t->scenes[sc].push_back({ field, pose });
         }
      t->scene_of_run.assign(scene_of_run, scene_of_run + n_runs);
      for (int sc : t->scene_of_run)
         if (sc < 0 || sc >= n_scenes) throw std::runtime_error("scene_of_run entries must lie in [0, n_scenes)!");
      *batch_id = mod->impl->create_batch(robot, q, n_runs, starts, goals, basegoals, seeds, nullptr, t);
   });
}

int orc_batch_iterate(orc_module * mod, int id, int n_iter, double * costs_out, int * status_out)
{
   return guarded(mod, [&] {
      orc::Batch & b = mod->impl->batch(id);
      b.iterate_async(n_iter);
      b.sync(costs_out, status_out);
   });
}

int orc_batch_set_convergence(orc_module * mod, int id, double rtol, int patience, double obs_max)
{
   return guarded(mod, [&] {
      orc::ConvergenceSpec c;
      c.rtol = rtol; c.patience = patience; c.obs_max = obs_max;
      mod->impl->batch(id).set_convergence(c);
   });
}

int orc_batch_iterate_async(orc_module * mod, int id, int n_iter)
{
   return guarded(mod, [&] { mod->impl->batch(id).iterate_async(n_iter); });
}

int orc_batch_sync(orc_module * mod, int id, double * costs_out, int * status_out)
{
   return guarded(mod, [&] { mod->impl->batch(id).sync(costs_out, status_out); });
}

int orc_batch_iterations_done(orc_module * mod, int id, int * iters_out)
{
   return guarded(mod, [&] { mod->impl->batch(id).sync(nullptr, nullptr, iters_out); });
}

int orc_batch_get_trace(orc_module * mod, int id, double * out, size_t cap)
{
   return guarded(mod, [&] {
      orc::Batch & b = mod->impl->batch(id);
      need(out, "out");
      if (cap < (size_t) b.n_runs * b.last_n_iter * 3) throw std::runtime_error("buffer too small!");
      b.get_trace(out);
   });
}

int orc_batch_set_noise(orc_module * mod, int id, const double * noise, int n_blocks)
{
   return guarded(mod, [&] {
      if (n_blocks < 0 || (n_blocks > 0 && !noise)) throw std::runtime_error("bad noise blocks!");
      mod->impl->batch(id).set_noise(noise, n_blocks);
   });
}

int orc_batch_gettraj(orc_module * mod, int id, double * out, size_t cap)
{
   return guarded(mod, [&] {
      orc::Batch & b = mod->impl->batch(id);
      need(out, "out");
      if (cap < (size_t) b.n_runs * b.n_points * b.n) throw std::runtime_error("buffer too small!");
      b.gettraj(out);
   });
}

int orc_batch_collision_verdict(orc_module * mod, int id, int * collides_out, double * time_out, int * sphere_out,
   int * field_out, double * depth_out)
{
   return guarded(mod, [&] {
      need(collides_out, "collides_out");
      mod->impl->batch_collision_verdict(id, collides_out, time_out, sphere_out, field_out, depth_out);
   });
}

int orc_batch_collision_verdict_device(orc_module * mod, int id, int * collides_out, double * time_out, int * sphere_out,
   int * field_out, double * depth_out, int * n_samples_out)
{
   return guarded(mod, [&] {
      need(collides_out, "collides_out");
      mod->impl->batch_collision_verdict_device(id, collides_out, time_out, sphere_out, field_out, depth_out, n_samples_out);
   });
}

int orc_batch_collision_verdict_subset(orc_module * mod, int id, int which, const unsigned char * examine, int * collides_out,
   double * time_out, int * sphere_out, int * field_out, double * depth_out, int * n_samples_out)
{
   return guarded(mod, [&] {
      need(collides_out, "collides_out");
      mod->impl->batch_collision_verdict_subset(id, which, examine, collides_out, time_out, sphere_out, field_out, depth_out, n_samples_out);
   });
}

int orc_batch_set_verdict_scope(orc_module * mod, int id, int scope)
{
   return guarded(mod, [&] { mod->impl->batch(id).set_verdict_scope(scope); });
}

int orc_batch_get_state(orc_module * mod, int id, const char * which, double * out, size_t cap)
{
   return guarded(mod, [&] {
      orc::Batch & b = mod->impl->batch(id);
      need(which, "which"); need(out, "out");
      if (std::string(which) == "phase")
      {
         if (cap < (size_t) b.n_runs * 8) throw std::runtime_error("buffer too small!");
         std::vector<long long> tmp((size_t) b.n_runs * 8);
         b.get_phase_cycles(tmp.data());
         for (size_t i=0; i<tmp.size(); i++) out[i] = (double) tmp[i];
         return;
      }
      if (std::string(which) == "waves")
      {
         if (cap < (size_t) b.n_runs * 16) throw std::runtime_error("buffer too small!");
         std::vector<unsigned int> tmp((size_t) b.n_runs * 16);
         b.get_wave_hwid(tmp.data());
         for (size_t i=0; i<tmp.size(); i++) out[i] = (double) tmp[i];
         return;
      }
      if (std::string(which) == "plan")
      {
         if (cap < 8) throw std::runtime_error("buffer too small!");
         double plan[9];
         b.get_plan(plan);
         std::copy(plan, plan + (cap < 9 ? 8 : 9), out);      // (the first tile's size: appended, read when there is room)
         return;
      }
      if (std::string(which) == "tsr_plan")      // which form of the constraint step this batch runs (tsr_form.h)
      {
         if (cap < 11) throw std::runtime_error("buffer too small!");
         b.get_tsr_plan(out);
         return;
      }
      if (std::string(which) == "config_chunk")      // the queries a workgroup of config_clearance_kernel takes for this batch
      {
         if (cap < 1) throw std::runtime_error("buffer too small!");
         out[0] = (double) b.shards[0]->config_chunk();
         return;
      }
      if (std::string(which) == "penetration_chunk")      // ... of penetration_kernel
      {
         if (cap < 1) throw std::runtime_error("buffer too small!");
         out[0] = (double) b.shards[0]->penetration_chunk();
         return;
      }
      if (std::string(which) == "project_state")      // where a lane's state of project_tsr_kernel lives: [0] up to 3 enforced rows, [1] up to 6
      {
         if (cap < 2) throw std::runtime_error("buffer too small!");
         out[0] = (double) b.shards[0]->project_state_in_lds(3); out[1] = (double) b.shards[0]->project_state_in_lds(6);
         return;
      }
      if (std::string(which) == "run_params")
      {
         if (cap < (size_t) b.n_runs * 4) throw std::runtime_error("buffer too small!");
         b.get_run_params(out);
         return;
      }
      if (cap < (size_t) b.n_runs * b.m * b.n) throw std::runtime_error("buffer too small!");
      b.get_state(which, out);
   });
}

int orc_batch_dims(orc_module * mod, int id, int * n_runs, int * n_points, int * n)
{
   return guarded(mod, [&] {
      orc::Batch & b = mod->impl->batch(id);
      if (n_runs) *n_runs = b.n_runs;
      if (n_points) *n_points = b.n_points;
      if (n) *n = b.n;
   });
}

int orc_batch_set_traj(orc_module * mod, int id, const double * traj, size_t count)
{
   return guarded(mod, [&] {
      orc::Batch & b = mod->impl->batch(id);
      need(traj, "traj");
      if (count != (size_t) b.n_runs * b.n_points * b.n) throw std::runtime_error("wrong trajectory size!");
      b.set_traj(traj);
   });
}

int orc_batch_perturb(orc_module * mod, int id, double sigma, const unsigned int * seeds)
{
   return guarded(mod, [&] { mod->impl->batch(id).perturb(sigma, seeds); });
}

int orc_batch_select_best(orc_module * mod, int id, int n_groups, const int * group_of_run, int require_collision_free,
   int * best_run_out, double * best_cost_out, int * n_eligible_out)
{
   return orc_batch_select_best_by(mod, id, 0, n_groups, group_of_run, require_collision_free, best_run_out, best_cost_out, n_eligible_out);
}

int orc_batch_select_best_by(orc_module * mod, int id, int cost_column, int n_groups, const int * group_of_run, int require_collision_free,
   int * best_run_out, double * best_cost_out, int * n_eligible_out)
{
   return guarded(mod, [&] {
      mod->impl->batch_select_best(id, cost_column, n_groups, group_of_run, require_collision_free != 0, best_run_out, best_cost_out, n_eligible_out);
   });
}

int orc_batch_clearance(orc_module * mod, int id, int which, const unsigned char * examine, int max_samples, double * clearance_out,
   double * time_out, int * sphere_out, int * other_out, int * n_samples_out)
{
   return guarded(mod, [&] {
      mod->impl->batch(id);      // (an unknown batch first)
      need(clearance_out, "clearance_out"); need(n_samples_out, "n_samples_out");
      mod->impl->batch_clearance(id, which, examine, max_samples, clearance_out, time_out, sphere_out, other_out, n_samples_out);
   });
}

int orc_batch_config_clearance(orc_module * mod, int id, int n_q, const int * run_of_q, const double * configs, double * clearance_out,
   int * sphere_out, int * other_out)
{
   return guarded(mod, [&] { mod->impl->batch_config_clearance(id, false, n_q, run_of_q, nullptr, configs, clearance_out, sphere_out, other_out); });
}

int orc_batch_waypoint_clearance(orc_module * mod, int id, int n_q, const int * run_of_q, const int * point_of_q, double * clearance_out,
   int * sphere_out, int * other_out)
{
   return guarded(mod, [&] { mod->impl->batch_config_clearance(id, true, n_q, run_of_q, point_of_q, nullptr, clearance_out, sphere_out, other_out); });
}

int orc_batch_path_clearance(orc_module * mod, int id, int n_q, const int * run_of_q, int n_rows, const double * paths, int max_samples,
   double * clearance_out, double * time_out, int * sphere_out, int * other_out, int * n_samples_out)
{
   return guarded(mod, [&] {
      mod->impl->batch(id);      // (an unknown batch first)
      need(clearance_out, "clearance_out"); need(n_samples_out, "n_samples_out");
      mod->impl->batch_path_clearance(id, false, n_q, run_of_q, nullptr, nullptr, n_rows, paths, max_samples, clearance_out, time_out, sphere_out,
         other_out, n_samples_out);
   });
}

int orc_batch_waypoint_segment_clearance(orc_module * mod, int id, int n_q, const int * run_of_q, const int * from_of_q, const int * to_of_q,
   int max_samples, double * clearance_out, double * time_out, int * sphere_out, int * other_out, int * n_samples_out)
{
   return guarded(mod, [&] {
      mod->impl->batch(id);      // (an unknown batch first)
      need(clearance_out, "clearance_out"); need(n_samples_out, "n_samples_out");
      mod->impl->batch_path_clearance(id, true, n_q, run_of_q, from_of_q, to_of_q, 2, nullptr, max_samples, clearance_out, time_out, sphere_out,
         other_out, n_samples_out);
   });
}

int orc_batch_config_penetration(orc_module * mod, int id, int n_q, const int * run_of_q, const double * configs, double margin_field,
   double margin_self, double * cost_out, double * grad_out, double * clearance_out, int * sphere_out, int * other_out)
{
   return guarded(mod, [&] {
      mod->impl->batch_config_penetration(id, false, n_q, run_of_q, nullptr, configs, margin_field, margin_self, cost_out, grad_out, clearance_out,
         sphere_out, other_out);
   });
}

int orc_batch_waypoint_penetration(orc_module * mod, int id, int n_q, const int * run_of_q, const int * point_of_q, double margin_field,
   double margin_self, double * cost_out, double * grad_out, double * clearance_out, int * sphere_out, int * other_out)
{
   return guarded(mod, [&] {
      mod->impl->batch_config_penetration(id, true, n_q, run_of_q, point_of_q, nullptr, margin_field, margin_self, cost_out, grad_out, clearance_out,
         sphere_out, other_out);
   });
}

namespace {
// the caller's TSRs as the host layer holds them (ee_link -1, the active manipulator, is resolved by Module::project_check)
std::vector<orc::TsrSpec> to_tsrs(int n_tsr, const orc_tsr * tsrs)
{
   if (n_tsr < 1) throw std::runtime_error("n_tsr must be >= 1!");
   need(tsrs, "tsrs");
   std::vector<orc::TsrSpec> out(n_tsr);
   for (int t=0; t<n_tsr; t++)
   {
      out[t].ee_link = tsrs[t].ee_link;
      out[t].tool = orc::Pose(tsrs[t].tool); out[t].T0w = orc::Pose(tsrs[t].T0w); out[t].Twe = orc::Pose(tsrs[t].Twe);
      for (int r=0; r<6; r++) { out[t].Bw[r][0] = tsrs[t].Bw[r][0]; out[t].Bw[r][1] = tsrs[t].Bw[r][1]; }
   }
   return out;
}
}

int orc_batch_config_tsr(orc_module * mod, int id, int n_tsr, const orc_tsr * tsrs, int n_q, const int * tsr_of_q, const double * configs,
   double * h_out, double * jac_out)
{
   return guarded(mod, [&] {
      mod->impl->batch(id);      // (an unknown batch first)
      mod->impl->batch_config_tsr(id, to_tsrs(n_tsr, tsrs), n_q, tsr_of_q, configs, h_out, jac_out);
   });
}

int orc_batch_project_tsr(orc_module * mod, int id, int n_tsr, const orc_tsr * tsrs, int n_q, const int * tsr_of_q, const double * configs,
   const double * lower, const double * upper, int max_steps, double tol, double mu, double step_cap, double * configs_out,
   double * resid_out, int * steps_out, int * status_out)
{
   return guarded(mod, [&] {
      mod->impl->batch(id);
      orc::ProjectSpec ps;
      ps.max_steps = max_steps; ps.tol = tol; ps.mu = mu; ps.step_cap = step_cap; ps.lower = lower; ps.upper = upper;
      mod->impl->batch_project_tsr(id, to_tsrs(n_tsr, tsrs), n_q, tsr_of_q, configs, ps, configs_out, resid_out, steps_out, status_out);
   });
}

int orc_batch_project_tsr_clear(orc_module * mod, int id, int n_tsr, const orc_tsr * tsrs, int n_q, const int * tsr_of_q, const int * run_of_q,
   const double * configs, const double * lower, const double * upper, int max_steps, double tol, double mu, double step_cap, double push_cap,
   double margin_field, double margin_self, double slack, double * configs_out, double * resid_out, double * clearance_out, int * steps_out,
   int * status_out)
{
   return guarded(mod, [&] {
      mod->impl->batch(id);
      orc::ProjectClearSpec ps;
      ps.project.max_steps = max_steps; ps.project.tol = tol; ps.project.mu = mu; ps.project.step_cap = step_cap;
      ps.project.lower = lower; ps.project.upper = upper;
      ps.push_cap = push_cap; ps.margin_field = margin_field; ps.margin_self = margin_self; ps.slack = slack;
      orc::ProjectClearOut out;
      out.rows = configs_out; out.resid = resid_out; out.clear = clearance_out; out.steps = steps_out; out.status = status_out;
      mod->impl->batch_project_tsr_clear(id, to_tsrs(n_tsr, tsrs), n_q, tsr_of_q, run_of_q, configs, ps, out);
   });
}

int orc_batch_select_clear(orc_module * mod, int id, int cost_column, int n_groups, const int * group_of_run, double margin, int max_samples,
   int * best_run_out, double * best_cost_out, double * best_clearance_out, int * n_eligible_out, int * n_samples_out)
{
   return guarded(mod, [&] {
      mod->impl->batch_select_clear(id, cost_column, n_groups, group_of_run, margin, max_samples, best_run_out, best_cost_out,
         best_clearance_out, n_eligible_out, n_samples_out);
   });
}

int orc_batch_respawn(orc_module * mod, int id, int cost_column, int n_groups, const int * group_of_run, int collision_mode, int keep,
   double sigma, const unsigned int * seeds, int * source_of_run_out, int * n_survivors_out)
{
   return guarded(mod, [&] {
      mod->impl->batch_respawn(id, cost_column, n_groups, group_of_run, collision_mode, keep, sigma, seeds, source_of_run_out, n_survivors_out);
   });
}

int orc_batch_set_run_params(orc_module * mod, int id, const double * lambda, const double * epsilon,
   const double * obs_factor, const double * obs_factor_self)
{
   return guarded(mod, [&] { mod->impl->batch(id).set_run_params(lambda, epsilon, obs_factor, obs_factor_self); });
}

int orc_batch_gettraj_runs(orc_module * mod, int id, const int * runs, int n_sel, double * out, size_t cap)
{
   return guarded(mod, [&] {
      orc::Batch & b = mod->impl->batch(id);
      need(runs, "runs"); need(out, "out");
      if (n_sel < 0) throw std::runtime_error("gettraj_runs: n_sel must be >=0!");
      if (cap < (size_t) n_sel * b.n_points * b.n) throw std::runtime_error("buffer too small!");
      b.gettraj_runs(runs, n_sel, out);
   });
}

const char * orc_last_collision_details(const orc_module * mod)
{
   return mod ? mod->impl->last_collision_details.c_str() : "";
}

int orc_batch_destroy(orc_module * mod, int id)
{
   return guarded(mod, [&] { mod->impl->destroy_batch(id); });
}

int orc_kernel_time(orc_module * mod, double * total_ms, int * launches, int reset)
{
   return guarded(mod, [&] {
      mod->impl->time_collect();
      if (total_ms) *total_ms = mod->impl->kernel_ms_total;
      if (launches) *launches = mod->impl->kernel_launches;
      if (reset) { mod->impl->kernel_ms_total = 0.0; mod->impl->kernel_launches = 0; }
   });
}

int orc_host_bin_sdf(const int sizes[3], const double lengths[3], const double * occupancy, double * sdf_out)
{
   try
   {
      orc::Grid occ, sdf;
      for (int i=0; i<3; i++) { occ.sizes[i] = sizes[i]; occ.lengths[i] = lengths[i]; }
      occ.data.assign(occupancy, occupancy + occ.ncells());
      orc::grid_bin_sdf(occ, sdf);
      std::memcpy(sdf_out, sdf.data.data(), sdf.ncells() * sizeof(double));
      return 0;
   }
   catch (...) { return 1; }
}

int orc_host_flood_fill(const int sizes[3], double * cells, size_t start)
{
   try
   {
      orc::Grid g;
      for (int i=0; i<3; i++) { g.sizes[i] = sizes[i]; g.lengths[i] = 1.0; }
      g.data.assign(cells, cells + g.ncells());
      orc::grid_flood_1_to_0(g, start);
      std::memcpy(cells, g.data.data(), g.ncells() * sizeof(double));
      return 0;
   }
   catch (...) { return 1; }
}

int orc_host_voxelize_boxes(const int sizes[3], const double lengths[3], const double pose_world_gsdf[7], double cube_extent,
   int n_boxes, const double * box_world_poses, const double * half_extents, double * occupancy_out)
{
   try
   {
      orc::Grid g;
      for (int i=0; i<3; i++) { g.sizes[i] = sizes[i]; g.lengths[i] = lengths[i]; }
      std::vector<orc::Box> boxes(n_boxes);
      for (int k=0; k<n_boxes; k++)
      {
         boxes[k].world = orc::xform_from_pose(orc::Pose(box_world_poses + 7*k));
         for (int q=0; q<3; q++) boxes[k].half[q] = half_extents[3*k+q];
      }
      orc::voxelize_boxes(g, orc::Pose(pose_world_gsdf), cube_extent, boxes);
      std::memcpy(occupancy_out, g.data.data(), g.ncells() * sizeof(double));
      return 0;
   }
   catch (...) { return 1; }
}

int orc_host_voxelize_trimesh(const int sizes[3], const double lengths[3], const double pose_world_gsdf[7], double cube_extent,
   int n_tri, const double * world_vertices, double * occupancy_out)
{
   try
   {
      if (!sizes || !lengths || !pose_world_gsdf || !occupancy_out || (n_tri > 0 && !world_vertices) || n_tri > (1 << 26)) return 1;
      for (int i=0; i<3; i++) if (sizes[i] < 1 || !(lengths[i] > 0.0)) return 1;
      if (!(cube_extent > 0.0)) return 1;
      orc::Grid g;
      for (int i=0; i<3; i++) { g.sizes[i] = sizes[i]; g.lengths[i] = lengths[i]; }
      const std::vector<double> tris(world_vertices, world_vertices + 9*(size_t)(n_tri > 0 ? n_tri : 0));
      orc::voxelize_boxes(g, orc::Pose(pose_world_gsdf), cube_extent, std::vector<orc::Box>(), tris);
      std::memcpy(occupancy_out, g.data.data(), g.ncells() * sizeof(double));
      return 0;
   }
   catch (...) { return 1; }
}

int orc_host_merge_grid(int n_sources, const double * source_lengths, const double * source_poses, double cell, const double * bounds,
   int sizes_out[3], double lengths_out[3], double pose_out[7])
{
   if (n_sources < 0 || !sizes_out || !lengths_out || !pose_out) return 1;
   if (n_sources > 0 && (!source_lengths || !source_poses)) return 1;
   try
   {
      std::vector<orc::MergeBox> boxes(n_sources);
      for (int k=0; k<n_sources; k++)
      {
         for (int d=0; d<3; d++) boxes[k].lengths[d] = source_lengths[3*k+d];
         boxes[k].pose = orc::Pose(source_poses + 7*k);
      }
      orc::Pose pose;
      orc::merge_grid_dims(boxes, cell, bounds, sizes_out, lengths_out, pose);
      for (int i=0; i<7; i++) pose_out[i] = pose.v[i];
      return 0;
   }
   catch (...) { return 1; }
}

int orc_host_merge_fields(int n_sources, const int * source_sizes, const double * source_lengths, const double * source_poses,
   const double * const * source_data, const int sizes[3], const double lengths[3], const double pose_world_gsdf[7], double * data_out)
{
   if (n_sources < 0 || !sizes || !lengths || !pose_world_gsdf || !data_out) return 1;
   if (n_sources > 0 && (!source_sizes || !source_lengths || !source_poses || !source_data)) return 1;
   for (int d=0; d<3; d++) if (sizes[d] < 1 || !(lengths[d] > 0.0)) return 1;
   try
   {
      std::vector<OrcMergeSource> table;
      for (int k=0; k<n_sources; k++)
      {
         if (!source_data[k]) return 1;
         for (int d=0; d<3; d++) if (source_sizes[3*k+d] < 2 || !(source_lengths[3*k+d] > 0.0)) return 1;
         table.push_back(orc::merge_affine(orc::Pose(pose_world_gsdf), orc::Pose(source_poses + 7*k), source_sizes + 3*k, source_lengths + 3*k,
                                           source_data[k]));
      }
      orc::Grid g;
      for (int d=0; d<3; d++) { g.sizes[d] = sizes[d]; g.lengths[d] = lengths[d]; }
      orc::merge_fields_host(table, g);
      std::memcpy(data_out, g.data.data(), g.ncells() * sizeof(double));
      return 0;
   }
   catch (...) { return 1; }
}

int orc_host_shparse(const char * in, char * out, size_t out_cap)
{
   const std::vector<std::string> toks = orc::shparse(in ? in : "");
   size_t need = 0;
   for (const std::string & t : toks) need += t.size() + 1;
   if (need > out_cap) return -1;
   size_t off = 0;
   for (const std::string & t : toks) { std::memcpy(out + off, t.c_str(), t.size() + 1); off += t.size() + 1; }
   return (int) toks.size();
}

static int host_metric_impl(bool free_start, int m, int derivative, double dt, double * A_out, double * beta_s_out, double * beta_g_out,
   double kappa_out[3], const double * rhs, int ncols, double * solve_out)
{
   try
   {
      orc::Metric M;
      orc::build_metric(m, derivative, dt, M, free_start);
      if (A_out) std::memcpy(A_out, M.Adense.data(), (size_t) m*m*sizeof(double));
      if (beta_s_out) std::memcpy(beta_s_out, M.beta_s.data(), m*sizeof(double));
      if (beta_g_out) std::memcpy(beta_g_out, M.beta_g.data(), m*sizeof(double));
      if (kappa_out) { kappa_out[0] = M.kss; kappa_out[1] = M.ksg; kappa_out[2] = M.kgg; }
      if (rhs && solve_out) orc::metric_solve(M, rhs, ncols, solve_out);
      return 0;
   }
   catch (...) { return 1; }
}

int orc_host_metric(int m, int derivative, double dt, double * A_out, double * beta_s_out, double * beta_g_out,
   double kappa_out[3], const double * rhs, int ncols, double * solve_out)
{
   return host_metric_impl(false, m, derivative, dt, A_out, beta_s_out, beta_g_out, kappa_out, rhs, ncols, solve_out);
}
int orc_host_metric_free_start(int m, int derivative, double dt, double * A_out, double * beta_s_out, double * beta_g_out,
   double kappa_out[3], const double * rhs, int ncols, double * solve_out)
{
   return host_metric_impl(true, m, derivative, dt, A_out, beta_s_out, beta_g_out, kappa_out, rhs, ncols, solve_out);
}

int orc_host_metric_semisep_rank(int m, int derivative, double dt, int free_start)
{
   try
   {
      if (m < 1 || derivative < 1) return -1;
      orc::Metric M;
      orc::build_metric(m, derivative, dt, M, free_start != 0);
      return M.ss_rank;
   }
   catch (...) { return -1; }
}

int orc_host_tsr_form(int threads, int m, int n, int n_max, int out[6])
{
   if (!out || threads < 1 || m < 1 || n < 1 || n_max <= n) return 1;
   const TsrForm f = tsr_form(threads, m, n, n_max);
   out[0] = f.width; out[1] = f.regs; out[2] = f.aug; out[3] = f.meet; out[4] = f.subst_w; out[5] = f.subst_u;
   return 0;
}

int orc_host_verdict_samples(const double * traj, int n_points, int n, int col0, const double * vmax, int cap,
   int * seg_out, double * u_out, double * time_out, int * n_samples_out)
{
   try
   {
      if (!traj || !vmax || n_points < 2 || n < 1 || col0 < 0 || col0 >= n) return 1;
      std::vector<int> seg; std::vector<double> u, times;
      orc::host_verdict_samples(traj, n_points, n, col0, std::vector<double>(vmax, vmax + (n - col0)), seg, u, times);
      if (seg.size() > (size_t) 0x7fffffff) return 1;
      if (n_samples_out) *n_samples_out = (int) seg.size();
      if (cap < 0 || seg.size() > (size_t) cap) return 1;
      if (seg_out) std::copy(seg.begin(), seg.end(), seg_out);
      if (u_out) std::copy(u.begin(), u.end(), u_out);
      if (time_out) std::copy(times.begin(), times.end(), time_out);
      return 0;
   }
   catch (...) { return 1; }
}

int orc_host_gsl_stream(unsigned long seed, double sigma, int n, double * out_gauss, double * out_uniform)
{
   orc::GslRng r(seed);
   for (int i=0; i<n; i++) out_gauss[i] = r.gaussian(sigma);
   if (out_uniform) out_uniform[0] = r.uniform();
   return 0;
}

} // extern "C"
