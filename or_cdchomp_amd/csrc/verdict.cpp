// verdict.cpp -- host side of the collision verdict: gettraj's re-check of one run, and the batched verdicts of
// Module, Batch and BatchShard, which plan the samples here or leave that to the device and launch verdict_kernels.hip; and what
// the clearance (clearance.cpp) shares with the device-planned verdict: the checks of a scope and the kernel arguments of a
// planned walk.
#include "module.h"
#include "verdict_device.h"
#include "query_upload.h"      // walk_chunk
#include <cstdlib>
#include <sstream>
#include <stdexcept>

namespace orc {

void host_verdict_samples(const double * traj, int n_points, int n, int col0, const std::vector<double> & vmax,
   std::vector<int> & seg_out, std::vector<double> & u_out, std::vector<double> & time_out)
{
   const std::vector<double> dtm = retime_linear(traj, n_points, n, col0, vmax);
   for (SampleClock c(traj, n_points, n, col0, dtm); c.sample(); c.step()) { seg_out.push_back(c.seg); u_out.push_back(c.u); time_out.push_back(c.time); }
}

// the pairs of the verdict's self-collision leg (`|| CheckSelfCollision`, mod.cpp:2998-2999): spheres on links that may
// collide, in XML order; an end is a slot of the device's position row or an inactive sphere's world position
static void verdict_self_pairs(const Robot & rob, const Batch & b, bool self_check, VerdictInputs & in)
{
   if ((int) rob.spheres.size() > 128) throw std::runtime_error("too many spheres for the batched collision verdict!");
   if (!self_check || !rob.self_check) return;
   const std::vector<unsigned char> & excl = b.run_self_excl;      // sphere by sphere, taken at create (held bodies: Robot::run_self_pairs_excluded)
   const int ns = (int) rob.spheres.size();
   std::vector<int> end_of(ns, 0);
   std::vector<Xform> frames;
   rob.fk(rob.transform, rob.dof_values, frames);
   for (int si=0; si<ns; si++)
   {
      int slot = -1;
      for (size_t q=0; q<b.slot_xml.size(); q++) if (b.slot_xml[q] == si) slot = (int) q;
      if (slot >= 0) { end_of[si] = slot; continue; }
      end_of[si] = -1 - (int)(in.inact_pos.size() / 3);
      double r[3];
      mat3_vec(frames[rob.spheres[si].link].R, rob.spheres[si].pos, r);
      for (int q=0; q<3; q++) in.inact_pos.push_back(r[q] + frames[rob.spheres[si].link].t[q]);
   }
   for (int a=0; a<ns; a++)
      for (int c=a+1; c<ns; c++)
      {
         if (excl[(size_t) a * ns + c]) continue;
         in.pairs.push_back(end_of[a]); in.pairs.push_back(end_of[c]); in.pairs.push_back(a); in.pairs.push_back(c);
         in.rsum.push_back(rob.spheres[a].radius + rob.spheres[c].radius);
      }
}

// the robot with the spheres of the batch's runs: its own and those of the bodies it held at create (mod.cpp:2992-2996)
static Robot verdict_robot(Robot rob, const Batch & b) { rob.spheres = b.run_spheres; return rob; }

VerdictInputs verdict_inputs(const Robot & robot, const Batch & b, bool self_check, bool tables)
{
   VerdictInputs in;
   in.col0 = b.params.floating_base ? 7 : 0;
   for (int a : b.adofindices) in.vmax.push_back(a < (int) robot.limit_vel.size() ? robot.limit_vel[a] : 1.0);
   if (tables) verdict_self_pairs(verdict_robot(robot, b), b, self_check, in);
   return in;
}

// The reference samples the timed trajectory every 0.04 rad of C-space distance and asks
// OpenRAVE for environment/self collisions (mod.cpp:2958-3006).  Here the verdict comes from
// the model the optimizer itself uses: a configuration collides when an active sphere
// penetrates a signed distance field (interpolated field value below the sphere radius).
bool host_recheck(const Environment & env, const Batch & b, const double * traj, const std::vector<double> & dtm, bool self_check, std::string & details_out)
{
   const int col0 = b.params.floating_base ? 7 : 0;
   const Robot rob = verdict_robot(env.robot(b.robot_name), b);
   std::vector<Xform> frames;
   std::vector<double> q = rob.dof_values;
   bool collides = false; std::ostringstream details;
   for (SampleClock clock(traj, b.n_points, b.n, col0, dtm); !collides && clock.sample(); clock.step())
   {
      const int seg = clock.seg; const double u = clock.u, time = clock.time;
      Pose base = rob.transform;
      if (col0)
      {
         for (int j=0; j<7; j++) base.v[j] = traj[(size_t) seg*b.n+j] + (traj[(size_t)(seg+1)*b.n+j] - traj[(size_t) seg*b.n+j]) * u;
         pose_normalize(base);
      }
      for (size_t a=0; a<b.adofindices.size(); a++)
      {
         const double a0 = traj[(size_t) seg*b.n+col0+a], a1 = traj[(size_t)(seg+1)*b.n+col0+a];
         q[b.adofindices[a]] = a0 + (a1 - a0) * u;
      }
      rob.fk(base, q, frames);
      for (size_t si=0; si<rob.spheres.size() && !collides; si++)
      {
         const Robot::Sphere & sp = rob.spheres[si];
         bool active = col0 != 0;
         for (size_t a=0; a<b.adofindices.size() && !active; a++) active = rob.does_affect(b.adofindices[a], sp.link);
         if (!active) continue;
         double pw[3];
         mat3_vec(frames[sp.link].R, sp.pos, pw);
         for (int k=0; k<3; k++) pw[k] += frames[sp.link].t[k];
         // the module's fields where their kinbodies stand now; a batch with per-run scenes: the placements of run 0's scene
         const size_t n_fields = b.per_run_scenes ? b.scenes->scenes[b.scenes->scene_of_run[0]].size() : env.sdfs.size();
         for (size_t fi=0; fi<n_fields; fi++)
         {
            const ScenePlacement * pl = b.per_run_scenes ? &b.scenes->scenes[b.scenes->scene_of_run[0]][fi] : nullptr;
            const Sdf & f = pl ? *pl->sdf : *env.sdfs[fi];
            const Pose pose_world_gsdf = pose_compose(pl ? pl->pose_world_kinbody : env.body_transform(f.kinbody_name), f.pose);
            double pg[3], val;
            pose_apply(pose_invert(pose_world_gsdf), pw, pg);
            if (grid_interp(f.grid, pg, &val)) continue;
            if (val - sp.radius < 0.0)
            {
               collides = true;
               details << "Collision at t=" << time << ": sphere " << si << " of " << b.robot_name
                       << " is " << (sp.radius - val) << " m inside the field of " << f.kinbody_name << "\n";
               break;
            }
         }
      }
      // ... || CheckSelfCollision (mod.cpp:2998-2999): two spheres on links that may collide overlap
      for (size_t a=0; a<rob.spheres.size() && !collides && self_check && rob.self_check; a++)
         for (size_t c=a+1; c<rob.spheres.size(); c++)
         {
            const Robot::Sphere & sa = rob.spheres[a], & sc = rob.spheres[c];
            if (b.run_self_excl[a * rob.spheres.size() + c]) continue;
            double pa[3], pc[3], d2 = 0.0;
            mat3_vec(frames[sa.link].R, sa.pos, pa);
            mat3_vec(frames[sc.link].R, sc.pos, pc);
            for (int k=0; k<3; k++) { const double d = (pa[k] + frames[sa.link].t[k]) - (pc[k] + frames[sc.link].t[k]); d2 += d*d; }
            const double dist = std::sqrt(d2), rs = sa.radius + sc.radius;
            if (dist - rs < 0.0)
            {
               collides = true;
               details << "Collision at t=" << time << ": spheres " << a << " and " << c << " of " << b.robot_name
                       << " overlap by " << (rs - dist) << " m\n";
               break;
            }
         }
   }
   details_out = details.str();
   return collides;
}

// key: sample << 32 | pair bit << 31 | XML sphere << 16 | field (or, for a pair, the other sphere), into run k's entries of
// the outputs that are not NULL
static void verdict_decode(unsigned long long key, int k, int * collides, int * sphere, int * field)
{
   const bool hit = key != ORC_VERDICT_NONE;
   const bool self = hit && ((key >> 31) & 1ull);
   if (collides) collides[k] = hit ? 1 : 0;
   if (sphere) sphere[k] = hit ? (int)((key >> 16) & 0x7fffull) : -1;
   if (field) field[k] = hit ? (self ? -2 - (int)(key & 0xffffull) : (int)(key & 0xffffull)) : -1;      // a pair: -2 - the other sphere
}

void Module::batch_collision_verdict(int id, int * collides, double * time, int * sphere, int * field, double * depth, bool self_check)
{
   Batch & b = batch(id);
   const VerdictInputs in = verdict_inputs(env.robot(b.robot_name), b, self_check);
   std::vector<double> traj((size_t) b.n_runs * b.n_points * b.n);
   b.gettraj(traj.data());
   std::vector<int> offs(b.n_runs + 1, 0), seg;
   std::vector<double> u, times;
   for (int k=0; k<b.n_runs; k++)
   {
      host_verdict_samples(&traj[(size_t) k * b.n_points * b.n], b.n_points, b.n, in.col0, in.vmax, seg, u, times);
      if (seg.size() >= ((size_t) 1 << 31) - 1) throw std::runtime_error("trajectory too long for the batched collision verdict!");      // (the running total is an int on both sides)
      offs[k+1] = (int) seg.size();
      if (offs[k+1] - offs[k] >= (1 << 30)) throw std::runtime_error("trajectory too long for the batched collision verdict!");
   }
   std::vector<unsigned long long> key(b.n_runs); std::vector<double> dep(b.n_runs);
   b.collision_verdict(offs, seg, u, in, key.data(), dep.data());
   if (getenv("ORC_DEBUG_VERDICT"))
      for (int k=0; k<b.n_runs; k++) fprintf(stderr, "verdict run %d key %016llx samples %d\n", k, key[k], offs[k+1] - offs[k]);
   for (int k=0; k<b.n_runs; k++)
   {
      const bool hit = key[k] != ORC_VERDICT_NONE;
      verdict_decode(key[k], k, collides, sphere, field);
      if (time) time[k] = hit ? times[(size_t) offs[k] + (size_t)(key[k] >> 32)] : -1.0;
      if (depth) depth[k] = hit ? dep[k] : 0.0;
   }
}

// The verdict above with the planning left to the device (verdict_kernels.hip): what goes up is vmax and the pair tables,
// what comes back is what the caller asks for.
void Module::batch_collision_verdict_device(int id, int * collides, double * time, int * sphere, int * field, double * depth, int * n_samples,
   const VerdictScope & scope)
{
   Batch & b = batch(id);
   const VerdictInputs in = verdict_inputs(env.robot(b.robot_name), b, true);
   const bool want_key = collides || sphere || field;
   std::vector<unsigned long long> key(want_key ? b.n_runs : 0);
   b.collision_verdict_planned(in, want_key ? key.data() : nullptr, depth, time, n_samples, scope);
   for (int k=0; k<(int) key.size(); k++) verdict_decode(key[k], k, collides, sphere, field);
}

// ... of the runs the caller names.  The kernel tells a run it did not examine (ORC_VERDICT_SKIPPED) and one it found too long
// (ORC_VERDICT_TOO_LONG) in n_samples, whether or not the caller takes that array; both have the key of a run without a
// contact, so time, sphere, field and depth are already what such a run reports.
void Module::batch_collision_verdict_subset(int id, int which, const unsigned char * examine, int * collides, double * time, int * sphere,
   int * field, double * depth, int * n_samples)
{
   Batch & b = batch(id);
   if (which != 0 && which != 1) throw std::runtime_error("collision verdict: which is 0 (the runs of examine) or 1 (the candidates)!");
   VerdictScope scope;
   scope.which = which; scope.examine = examine;
   scope.count_rest = n_samples != nullptr;
   scope.long_marks_run = true;
   std::vector<int> ns(b.n_runs);
   batch_collision_verdict_device(id, collides, time, sphere, field, depth, ns.data(), scope);
   for (int k=0; k<b.n_runs; k++)
   {
      if (ns[k] < 0 && collides) collides[k] = ns[k];
      if (n_samples) n_samples[k] = ns[k];
   }
}

void Batch::collision_verdict(const std::vector<int> & soffs, const std::vector<int> & seg, const std::vector<double> & u,
   const VerdictInputs & in, unsigned long long * key_out, double * depth_out)
{
   for_shards([&](size_t k) {
      const int r0 = offs[k], r1 = offs[k+1];
      std::vector<int> so(r1 - r0 + 1);
      for (int r=r0; r<=r1; r++) so[r - r0] = soffs[r] - soffs[r0];
      const std::vector<int> sg(seg.begin() + soffs[r0], seg.begin() + soffs[r1]);
      const std::vector<double> su(u.begin() + soffs[r0], u.begin() + soffs[r1]);
      shards[k]->collision_verdict(so, sg, su, in, key_out + r0, depth_out + r0);
   }, true);
}

// what a device-planned walk rejects of its scope, the verdict's or the clearance's (`who`), before any device work; `unmasked`
// names the values of which that go without examine.  `other`: NULL, or what the caller found wrong with another argument,
// which ranks behind a wrong mask and before the batch's state
void Batch::verdict_scope_check(const char * who, int which, const unsigned char * examine, const char * unmasked, const char * other) const
{
   if (which == 0 && !examine) throw std::runtime_error(std::string(who) + ": which 0 needs examine [n_runs]!");
   if (which > 0 && examine) throw std::runtime_error(std::string(who) + ": " + unmasked + " no examine!");      // (the verdict's 1; the clearance's 1 and 2; not the verdict's -1, as before)
   if (other) throw std::runtime_error(other);
   if (which == 1 && !iterated) throw std::runtime_error("select_best: the batch has not been iterated (orc_batch_iterate with 0 iterations makes its costs valid)!");
}

void Batch::collision_verdict_planned(const VerdictInputs & in, unsigned long long * key_out, double * depth_out, double * time_out,
   int * n_samples_out, const VerdictScope & scope)
{
   // (scope.which is -1, 0 or 1: the callers' own values, Module::batch_collision_verdict_subset checks the C caller's)
   verdict_scope_check("collision verdict", scope.which, scope.examine, "which 1 (the candidates) takes", nullptr);
   std::vector<int> ok(shards.size(), 1);
   for_shards([&](size_t k) {
      const int r0 = offs[k];
      VerdictScope mine = scope;      // (every shard takes its slice of the caller's bytes)
      if (mine.examine) mine.examine += r0;
      ok[k] = shards[k]->collision_verdict_planned(in, key_out ? key_out + r0 : nullptr, depth_out ? depth_out + r0 : nullptr,
         time_out ? time_out + r0 : nullptr, n_samples_out ? n_samples_out + r0 : nullptr, mine) ? 1 : 0;
   }, true);
   for (int v : ok) if (!v) throw std::runtime_error("trajectory too long for the batched collision verdict!");
}

// What the two verdicts share: the tables that the walk reads (verdict_walk.h) go up, the depths are zeroed and `w` is
// filled, but for key_out.  The chunk is walk_chunk's (query_upload.h) for the kernel's dynamic LDS, lds_bytes(chunk).
template <typename real>
void BatchShard::verdict_walk_args(const VerdictInputs & in, const std::function<size_t(int)> & lds_bytes, VerdictTables & t, DevVerdictWalk<real> & w)
{
   hipStream_t st = stream_;
   t.xml.reset(dev_alloc<int>(slot_xml.size())); t.pairs.reset(dev_alloc<int>(in.pairs.size())); t.depth.reset(dev_alloc<double>(n_runs));
   hip_check(hipMemcpyAsync(t.xml.as<void>(), slot_xml.data(), slot_xml.size()*sizeof(int), hipMemcpyHostToDevice, st), "verdict xml");
   hip_check(hipMemcpyAsync(t.pairs.as<void>(), in.pairs.data(), in.pairs.size()*sizeof(int), hipMemcpyHostToDevice, st), "verdict pairs");
   hip_check(hipMemsetAsync(t.depth.as<void>(), 0, n_runs*sizeof(double), st), "verdict depth");
   t.rsum.reset(upload<real>(in.rsum, st)); t.inact.reset(upload<real>(in.inact_pos, st));
   const int chunk = walk_chunk(lds_bytes);
   w.model = d_model_.as<const DevModel<real>>(); w.sdfs = d_sdfs_.as<const DevSdf<real>>(); w.n_sdfs = scn_.n_sdfs;
   w.scene_of_run = d_scene_of_run_.as<int>(); w.scene_nsdf = d_scene_nsdf_.as<int>();
   w.n_runs = n_runs; w.n_points = n_points; w.n = n; w.chunk = chunk; w.traj = d_traj_.as<const real>();
   w.slot_xml = t.xml.as<int>();
   w.n_pairs = (int) in.rsum.size(); w.pairs = t.pairs.as<int>(); w.pair_rsum = t.rsum.as<const real>(); w.inact_pos = t.inact.as<const real>();
   w.depth_out = t.depth.as<double>();
}

template void BatchShard::verdict_walk_args<double>(const VerdictInputs &, const std::function<size_t(int)> &, VerdictTables &, DevVerdictWalk<double> &);      // (config_clearance.cpp calls them)
template void BatchShard::verdict_walk_args<float>(const VerdictInputs &, const std::function<size_t(int)> &, VerdictTables &, DevVerdictWalk<float> &);

// first contact of every run's trajectory with a field, in the run's precision
template <typename real>
void BatchShard::collision_verdict_typed(const std::vector<int> & offs, const std::vector<int> & seg, const std::vector<double> & u,
   const VerdictInputs & in, unsigned long long * key_out, double * depth_out)
{
   hipStream_t st = stream_;
   hip_check(hipStreamSynchronize(st), "verdict: pending work");
   const size_t ns = seg.size();
   const auto lds_bytes = [this](int chunk) { return orc_verdict_lds_bytes(n, ms_.Sa, ms_.Sa_real, ms_.nj, sizeof(real), chunk); };
   VerdictTables t;
   DevVerdict<real> v;
   verdict_walk_args<real>(in, lds_bytes, t, v);
   DevBuf d_offs, d_seg, d_key, d_u;
   d_offs.reset(dev_alloc<int>(offs.size())); d_seg.reset(dev_alloc<int>(ns)); d_key.reset(dev_alloc<unsigned long long>(n_runs));
   hip_check(hipMemcpyAsync(d_offs.as<void>(), offs.data(), offs.size()*sizeof(int), hipMemcpyHostToDevice, st), "verdict offs");
   hip_check(hipMemcpyAsync(d_seg.as<void>(), seg.data(), ns*sizeof(int), hipMemcpyHostToDevice, st), "verdict seg");
   d_u.reset(upload<real>(u, st));
   v.offs = d_offs.as<int>(); v.seg = d_seg.as<int>(); v.u = d_u.as<const real>(); v.key_out = d_key.as<unsigned long long>();
   hip_check(orc_launch_verdict(v, lds_bytes(v.chunk), st, plan_.variant & ORC_VAR_TREE), "collision_verdict_kernel launch");
   hip_check(hipMemcpyAsync(key_out, d_key.as<void>(), n_runs*sizeof(unsigned long long), hipMemcpyDeviceToHost, st), "verdict keys");
   hip_check(hipMemcpyAsync(depth_out, t.depth.as<void>(), n_runs*sizeof(double), hipMemcpyDeviceToHost, st), "verdict depth");
   hip_check(hipStreamSynchronize(st), "verdict sync");
}

void BatchShard::collision_verdict(const std::vector<int> & offs, const std::vector<int> & seg, const std::vector<double> & u,
   const VerdictInputs & in, unsigned long long * key_out, double * depth_out)
{
   DeviceGuard guard(device);
   if (params.precision == 64) collision_verdict_typed<double>(offs, seg, u, in, key_out, depth_out);
   else collision_verdict_typed<float>(offs, seg, u, in, key_out, depth_out);
}

// What the two device-planned walks share (verdict_planned.h; `who`, `tag`: the verdict or the clearance, for its messages): the
// walk's tables and vmax go up, the scope becomes the kernel's pointers, and `v` is filled but for n_samples_out.  Returns the
// kernel's dynamic LDS by the kernel's own formula: the plan's arrays sit there too, and grow with n_points.
template <typename real>
size_t BatchShard::verdict_planned_args(const char * who, const char * tag, size_t (*kernel_lds)(int, int, int, int, int, size_t, int), const VerdictInputs & in,
   const VerdictScope & scope, VerdictTables & t, DevVerdictPlanned<real> & v)
{
   hipStream_t st = stream_;
   hip_check(hipStreamSynchronize(st), (std::string(tag) + ": pending work").c_str());
   if (n_points < 2 || (int) in.vmax.size() != n - in.col0) throw std::runtime_error(std::string(who) + ": bad trajectory dimensions!");
   const auto lds_bytes = [&](int chunk) { return kernel_lds(n_points, n, ms_.Sa, ms_.Sa_real, ms_.nj, sizeof(real), chunk); };
   verdict_walk_args<real>(in, lds_bytes, t, v);
   const size_t lds = lds_bytes(v.chunk);
   if (lds > ORC_VERDICT_LDS_LIMIT) throw std::runtime_error("trajectory too long for the batched collision verdict!");
   t.vmax.reset(upload<double>(in.vmax, st));
   v.col0 = in.col0; v.vmax = t.vmax.as<const double>();
   v.examine = nullptr; v.cand_status = nullptr; v.cand_costs = nullptr;
   if (scope.which == 0)
   {
      t.examine.reset(dev_alloc<unsigned char>(n_runs));
      hip_check(hipMemcpyAsync(t.examine.as<void>(), scope.examine, n_runs, hipMemcpyHostToDevice, st), (std::string(tag) + " runs").c_str());
      v.examine = t.examine.as<unsigned char>();
   }
   else if (scope.which == 1) { v.cand_status = d_status_.as<int>(); v.cand_costs = d_costs_.as<double>(); }      // (what the last iterate call left)
   return lds;
}

template size_t BatchShard::verdict_planned_args<double>(const char *, const char *, size_t (*)(int, int, int, int, int, size_t, int), const VerdictInputs &, const VerdictScope &, VerdictTables &, DevVerdictPlanned<double> &);      // (clearance.cpp calls them)
template size_t BatchShard::verdict_planned_args<float>(const char *, const char *, size_t (*)(int, int, int, int, int, size_t, int), const VerdictInputs &, const VerdictScope &, VerdictTables &, DevVerdictPlanned<float> &);

// ... with the samples planned by the kernel itself: the trajectories stay where they are
template <typename real>
bool BatchShard::collision_verdict_planned_typed(const VerdictInputs & in, unsigned long long * key_out, double * depth_out, double * time_out,
   int * n_samples_out, const VerdictScope & scope)
{
   hipStream_t st = stream_;
   VerdictTables t;
   DevVerdictPlan<real> v;
   const size_t lds = verdict_planned_args<real>("collision verdict", "verdict", orc_verdict_planned_lds_bytes, in, scope, t, v);
   DevBuf d_time, d_ns, d_flag;
   d_time.reset(dev_alloc<double>(n_runs)); d_ns.reset(dev_alloc<int>(n_runs)); d_flag.reset(dev_alloc<int>(1));
   if (!d_vkey_) d_vkey_.reset(dev_alloc<unsigned long long>(n_runs));
   hip_check(hipMemsetAsync(d_flag.as<void>(), 0, sizeof(int), st), "verdict flag");
   v.key_out = d_vkey_.as<unsigned long long>(); v.time_out = d_time.as<double>();
   v.n_samples_out = d_ns.as<int>(); v.too_long = d_flag.as<int>();
   v.count_rest = scope.count_rest ? 1 : 0; v.long_marks_run = scope.long_marks_run ? 1 : 0;
   hip_check(orc_launch_verdict_planned(v, lds, st, plan_.variant & ORC_VAR_TREE), "collision_verdict_planned_kernel launch");
   int too_long = 0;
   hip_check(hipMemcpyAsync(&too_long, d_flag.as<void>(), sizeof(int), hipMemcpyDeviceToHost, st), "verdict flag");
   hip_check(hipStreamSynchronize(st), "verdict sync");
   if (too_long) return false;
   if (key_out) hip_check(hipMemcpyAsync(key_out, d_vkey_.as<void>(), n_runs*sizeof(unsigned long long), hipMemcpyDeviceToHost, st), "verdict keys");
   if (depth_out) hip_check(hipMemcpyAsync(depth_out, t.depth.as<void>(), n_runs*sizeof(double), hipMemcpyDeviceToHost, st), "verdict depth");
   if (time_out) hip_check(hipMemcpyAsync(time_out, d_time.as<void>(), n_runs*sizeof(double), hipMemcpyDeviceToHost, st), "verdict time");
   if (n_samples_out) hip_check(hipMemcpyAsync(n_samples_out, d_ns.as<void>(), n_runs*sizeof(int), hipMemcpyDeviceToHost, st), "verdict samples");
   hip_check(hipStreamSynchronize(st), "verdict sync");
   return true;
}

bool BatchShard::collision_verdict_planned(const VerdictInputs & in, unsigned long long * key_out, double * depth_out, double * time_out,
   int * n_samples_out, const VerdictScope & scope)
{
   DeviceGuard guard(device);
   if (params.precision == 64) return collision_verdict_planned_typed<double>(in, key_out, depth_out, time_out, n_samples_out, scope);
   return collision_verdict_planned_typed<float>(in, key_out, depth_out, time_out, n_samples_out, scope);
}

} // namespace orc
