// module.cpp -- the module's device plumbing (event pool, stream pool, plan streams and buffers, timing totals) and its batches.
// (The SendCommand layer: commands.cpp; the environment: env.cpp; the collision verdicts: verdict.cpp.)
#include "module.h"
#include "merge_launch.h"
#include <cmath>
#include <stdexcept>

namespace orc {

Module::Module(int dev) : Module(std::vector<int>(1, dev)) {}

Module::Module(const std::vector<int> & devs) : device(devs.empty() ? 0 : devs[0]), devices(devs)
{
   int count = 0;
   hipError_t e = hipGetDeviceCount(&count);
   if (e != hipSuccess || count <= 0)
      throw std::runtime_error("orcdchomp_amd: no HIP device available (the MI355X path has no CPU fallback)");
   if (devices.empty()) throw std::runtime_error("orcdchomp_amd: empty device list");
   for (int d : devices) if (d < 0 || d >= count) throw std::runtime_error("orcdchomp_amd: bad device ordinal");
   hip_check(hipSetDevice(device), "hipSetDevice");
}

Module::~Module()
{
   batches_.clear();
   env.sdfs.clear();
   for (auto & kv : event_pool_)
   {
      DeviceGuard guard(kv.first);
      for (hipEvent_t ev : kv.second) (void) hipEventDestroy(ev);
   }
   for (auto & kv : stream_pool)
   {
      DeviceGuard guard(kv.first);
      for (hipStream_t st : kv.second) (void) hipStreamDestroy(st);
   }
   for (auto & kv : plan_streams_)
   {
      DeviceGuard guard(kv.first);
      (void) hipStreamDestroy(kv.second);
   }
}

hipEvent_t Module::acquire_event(int dev)
{
   {
      std::lock_guard<std::mutex> lock(timing_mutex_);
      std::vector<hipEvent_t> & pool = event_pool_[dev];
      if (!pool.empty()) { hipEvent_t ev = pool.back(); pool.pop_back(); return ev; }
   }
   hipEvent_t ev;
   hip_check(hipEventCreate(&ev), "hipEventCreate");
   return ev;
}

void Module::release_event(int dev, hipEvent_t ev)
{
   std::lock_guard<std::mutex> lock(timing_mutex_);
   event_pool_[dev].push_back(ev);
}

void Module::add_kernel_time(double ms)
{
   std::lock_guard<std::mutex> lock(timing_mutex_);
   kernel_ms_total += ms;
   kernel_launches++;
}

// a pool of n streams on every device of the module; live batches hold the streams they were bound
// to, so the pool only changes while no batch exists
void Module::set_num_streams(int n)
{
   if (!batches_.empty())
      throw std::runtime_error("orc_set_num_streams: destroy the existing batches first (they hold the pool's streams)");
   for (auto & kv : stream_pool)
   {
      DeviceGuard guard(kv.first);
      for (hipStream_t st : kv.second) (void) hipStreamDestroy(st);
   }
   stream_pool.clear();
   next_pool_stream.clear();
   num_streams = n;
}

// the stream a new shard on `dev` is bound to: round-robin over the device's pool when there is one
// (created on first use), else the module's stream on the first device and the default stream
// elsewhere.  `distinct`: the shard shares its device with another shard of the same batch and must
// not queue behind it.
hipStream_t Module::pick_stream(int dev, bool distinct)
{
   int want = num_streams;
   if (distinct && want < 2)
   {
      int same = 0;
      for (int d : devices) if (d == dev) same++;
      want = same > 2 ? same : 2;
   }
   if (want <= 0) return dev == device ? stream : nullptr;
   std::vector<hipStream_t> & pool = stream_pool[dev];
   if ((int) pool.size() < want)
   {
      DeviceGuard guard(dev);
      while ((int) pool.size() < want)
      {
         hipStream_t st;
         hip_check(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
         pool.push_back(st);
      }
   }
   return pool[next_pool_stream[dev]++ % pool.size()];
}

hipStream_t Module::plan_stream(int dev)
{
   std::lock_guard<std::mutex> lock(timing_mutex_);
   auto it = plan_streams_.find(dev);
   if (it != plan_streams_.end()) return it->second;
   DeviceGuard guard(dev);
   int least = 0, greatest = 0;
   hip_check(hipDeviceGetStreamPriorityRange(&least, &greatest), "hipDeviceGetStreamPriorityRange");
   hipStream_t st;
   hip_check(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest), "hipStreamCreateWithPriority");
   plan_streams_[dev] = st;
   return st;
}

Module::PlanBuffers & Module::plan_buffers(int dev, hipStream_t stream)
{
   std::lock_guard<std::mutex> lock(timing_mutex_);
   return plan_buffers_[std::make_pair(dev, stream)];      // (references to a map's elements stay valid)
}

void Module::time_collect()
{
   for (auto & kv : batches_)
      for (auto & sh : kv.second->shards) sh->harvest_events(false);
}

int Module::create_batch(const std::string & rname, const BatchParams & p, int n_runs,
   const double * starts, const double * goals, const double * basegoals, const unsigned int * seeds,
   const std::vector<int> * devices_override, std::shared_ptr<const SceneTable> scenes)
{
   const bool per_run_scenes = scenes != nullptr;
   if (!scenes) scenes = env.current_scene(n_runs);
   if ((int) scenes->scene_of_run.size() != n_runs) throw std::runtime_error("scene_of_run must have an entry for every run!");
   const Robot r = env.robot_for_run(rname);
   if (devices_override)
   {
      int count = 0;
      hip_check(hipGetDeviceCount(&count), "hipGetDeviceCount");
      for (int d : *devices_override) if (d < 0 || d >= count) throw std::runtime_error("orcdchomp_amd: bad device ordinal");
   }
   std::unique_ptr<Batch> b(new Batch(this, devices_override ? *devices_override : devices, r, p, n_runs, starts, goals, basegoals, seeds, scenes));
   b->per_run_scenes = per_run_scenes;
   b->run_spheres = r.spheres;
   b->run_self_excl = r.run_self_pairs_excluded((int) env.robot(rname).spheres.size());
   const int id = next_batch_id_++;
   batches_[id] = std::move(b);
   return id;
}

// orc_scene_merge_fields.  Everything that can be refused is refused before the first device call, and the field list
// changes in the last statement: a call that fails leaves the module as it was.
void Module::merge_fields(const std::string & target, const std::vector<std::string> & fields, const double * field_poses,
   double cell, const double * bounds)
{
   std::lock_guard<std::recursive_mutex> env_lock(env_mutex);
   auto need_pose = [](const Pose & p) {
      for (int i=0; i<7; i++) if (!std::isfinite(p.v[i])) throw std::runtime_error("poses and bounds must be finite numbers!");
      if (p.v[3] == 0.0 && p.v[4] == 0.0 && p.v[5] == 0.0 && p.v[6] == 0.0) throw std::runtime_error("a pose's quaternion has zero norm!");
   };
   if (fields.empty()) throw std::runtime_error("n_fields must be >=1!");
   env.kinbody(target);                                     // "Could not find kinbody with that name!"
   if (env.find_sdf(target)) throw std::runtime_error("We already have an sdf for this kinbody!");
   if (!std::isfinite(cell) || !(cell > 0.0)) throw std::runtime_error("cell must be a positive finite number!");
   const Pose pose_world_target = env.body_transform(target);
   need_pose(pose_world_target);
   std::vector<std::shared_ptr<Sdf>> src;
   std::vector<Pose> pose_world_gsrc;
   std::vector<MergeBox> boxes;
   const Pose pose_target_world = pose_invert(pose_world_target);
   for (size_t k=0; k<fields.size(); k++)
   {
      const std::string & name = fields[k];
      if (!env.has_body(name)) throw std::runtime_error("Could not find kinbody with that name!");
      if (name == target) throw std::runtime_error("the target kinbody is among the fields to merge!");
      std::shared_ptr<Sdf> field;
      for (const auto & f : env.sdfs) if (f->kinbody_name == name) field = f;
      if (!field) throw std::runtime_error("Kinbody " + name + " has no signed distance field!");
      const Pose pose_world_kinbody = field_poses ? Pose(field_poses + 7*k) : env.body_transform(name);
      need_pose(pose_world_kinbody);
      need_pose(field->pose);
      const Pose pw = pose_compose(pose_world_kinbody, field->pose);
      MergeBox b;
      for (int d=0; d<3; d++) b.lengths[d] = field->grid.lengths[d];
      b.pose = pose_compose(pose_target_world, pw);
      src.push_back(field); pose_world_gsrc.push_back(pw); boxes.push_back(b);
   }
   Grid g;
   Pose pose_kinbody_gsdf;
   merge_grid_dims(boxes, cell, bounds, g.sizes, g.lengths, pose_kinbody_gsdf);      // (with the other refusals: bounds, 2^31 bytes)
   const Pose pose_world_gsdf = pose_compose(pose_world_target, pose_kinbody_gsdf);

   // ---- the device: the sources' fp64 copies (shared with the batches, made on demand as BatchShard::grid_on_device makes
   // them), the table, one kernel, one read-back
   DeviceGuard guard(device);
   std::vector<OrcMergeSource> table;
   for (size_t k=0; k<src.size(); k++)
   {
      Sdf & s = *src[k];
      std::shared_ptr<void> & buf = s.dev64[device];
      if (!buf)
      {
         const size_t bytes = s.grid.ncells() * sizeof(double);
         std::shared_ptr<void> fresh = device_buffer(device, bytes);
         hip_check(hipMemcpy(fresh.get(), s.grid.data.data(), bytes, hipMemcpyHostToDevice), "sdf upload");
         buf = fresh;
      }
      table.push_back(merge_affine(pose_world_gsdf, pose_world_gsrc[k], s.grid.sizes, s.grid.lengths, (const double *) buf.get()));
   }
   const size_t nc = g.ncells();
   std::shared_ptr<void> out = device_buffer(device, nc * sizeof(double));
   std::shared_ptr<void> dtable = device_buffer(device, table.size() * sizeof(OrcMergeSource));
   g.data.resize(nc);
   hip_check(hipMemcpyAsync(dtable.get(), table.data(), table.size() * sizeof(OrcMergeSource), hipMemcpyHostToDevice, stream), "merge table upload");
   hip_check(orc_launch_merge_fields((double *) out.get(), g.sizes, g.lengths, (const OrcMergeSource *) dtable.get(), (int) table.size(), stream),
             "merge_fields_kernel");
   hip_check(hipMemcpyAsync(g.data.data(), out.get(), nc * sizeof(double), hipMemcpyDeviceToHost, stream), "merged field read-back");
   hip_check(hipStreamSynchronize(stream), "merge sync");
   env.add_sdf(target, g, pose_kinbody_gsdf);
   env.find_sdf(target)->dev64[device] = out;               // the kernel's buffer is the field's fp64 copy here: no re-upload
}

Batch & Module::batch(int id)
{
   auto it = batches_.find(id);
   if (it == batches_.end()) throw std::runtime_error("you must pass a created run!");
   return *it->second;
}

void Module::destroy_batch(int id)
{
   auto it = batches_.find(id);
   if (it == batches_.end()) throw std::runtime_error("you must pass a created run!");
   batches_.erase(it);
}

} // namespace orc
