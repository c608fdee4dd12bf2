// module.cpp -- the module's device plumbing (event pool, stream pool, plan streams and buffers, timing totals) and its batches.
// (The SendCommand layer: commands.cpp; the environment: env.cpp; the collision verdicts: verdict.cpp.)
#include "module.h"
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
