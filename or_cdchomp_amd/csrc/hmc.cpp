// hmc.cpp -- the momentum-resampling plan of a shard's HMC runs (hmc.h): one owner of the streams, the plan's device memory, the
// overflow flag and the three ways a call's plan is made.
#include "module.h"
#include "launch.h"
#include <algorithm>
#include <functional>
#include <stdexcept>
#include <thread>

namespace orc {

void PlanStore::reserve(size_t icount, size_t nbytes, const hipStream_t * drain)
{
   if (icount <= iters_count && nbytes <= noise_bytes) return;
   if (drain) hip_check(hipStreamSynchronize(*drain), "hmc buffers: pending work");      // (an earlier launch may still read them)
   if (icount > iters_count) { iters.reset(); iters_count = 0; iters.reset(dev_alloc<int>(icount)); iters_count = icount; }
   if (nbytes > noise_bytes)
   {
      noise.reset(); noise_bytes = 0;
      void * p = nullptr;
      hip_check(hipMalloc(&p, nbytes), "noise");
      noise.reset(p); noise_bytes = nbytes;
   }
}

// runs [0, count) split over the host cores (the per-run noise streams are independent)
static void parallel_for_runs(int count, const std::function<void(int, int)> & body)
{
   unsigned hw = std::thread::hardware_concurrency();
   int nt = (int) std::min<unsigned>(hw ? hw : 1u, 16u);      // containers often grant far fewer cores than they list
   if (count < 64 || nt < 2) { body(0, count); return; }
   nt = std::min(nt, count / 16);
   std::vector<std::thread> pool;
   for (int t=0; t<nt; t++)
   {
      const int lo = (int)((long long) count * t / nt), hi = (int)((long long) count * (t+1) / nt);
      pool.emplace_back([&body, lo, hi]() { body(lo, hi); });
   }
   for (std::thread & th : pool) th.join();
}

HmcPlanner::HmcPlanner(Module * mod, int device, hipStream_t st, int n_runs, size_t mn, int precision, double lambda, bool use_hmc,
   const Switches & sw, const unsigned int * seeds)
   : mod_(mod), device_(device), stream_(st), n_runs_(n_runs), mn_(mn), precision_(precision), lambda_(lambda), use_hmc_(use_hmc)
{
   on_device_ = use_hmc && (n_runs >= 256 || sw.hmc_device) && !sw.hmc_host;
   if (on_device_)
   {
      d_mt_.reset(dev_alloc<uint32_t>((size_t) 625 * n_runs));
      d_next_.reset(dev_alloc<int>(n_runs)); d_overflow_.reset(dev_alloc<int>(1));
      DevBuf d_seeds;
      if (seeds)
      {
         d_seeds.reset(dev_alloc<unsigned int>(n_runs));
         hip_check(hipMemcpyAsync(d_seeds.as<void>(), seeds, n_runs*sizeof(unsigned int), hipMemcpyHostToDevice, st), "seeds");
      }
      hip_check(orc_launch_hmc_seed(d_mt_.as<uint32_t>(), d_next_.as<int>(), d_seeds.as<unsigned int>(), n_runs, st), "hmc seed");
      hip_check(hipStreamSynchronize(st), "hmc seed sync");
      hip_check(hipMemsetAsync(d_overflow_.as<void>(), 0, sizeof(int), st), "hmc overflow");
      hip_check(hipStreamSynchronize(st), "hmc overflow");
      // (the plan's buffers are the first iterate call's to allocate: Module::PlanBuffers)
   }
   else
   {
      host_.rng.resize(use_hmc ? n_runs : 0);
      for (int k=0; k<(int) host_.rng.size(); k++) host_.rng[k].set(seeds ? seeds[k] : 0);
   }
   host_.next.assign(n_runs, 0);
   host_.ext_used.assign(n_runs, 0);
}

HmcPlanner::~HmcPlanner()
{
   DeviceGuard guard(device_);
   for (int k=0; k<2; k++) if (ev_[k]) (void) hipEventDestroy(ev_[k]);
}

void HmcPlanner::check_usable() const
{
   if (unusable_) throw std::runtime_error("hmc: an earlier iterate call of this batch ran out of room for its momentum resamples; destroy the batch and create it again!");
}

void HmcPlanner::set_noise(const double * noise, int n_blocks)
{
   if (on_device_) throw std::runtime_error("caller-supplied noise needs the host noise streams (ORC_HMC_HOST=1, or fewer than 256 runs)!");
   host_.ext_blocks = n_blocks;
   host_.ext.assign(noise, noise + (size_t) n_runs_ * n_blocks * mn_);
}

// Resamples of the iterations [iter_begin, iter_begin + n_iter) of an iterate call; the kernel gets their positions relative to
// iter_begin (src/orcdchomp_mod.cpp:2755-2768; r->iter restarts at 0 on every call, 2752).
HmcPlan HmcPlanner::plan(int iter_begin, int n_iter, std::unique_lock<std::mutex> & enqueue)
{
   if (iter_begin == 0) std::fill(host_.ext_used.begin(), host_.ext_used.end(), 0);
   if (!use_hmc_ || n_iter <= 0) return HmcPlan();
   if (!on_device_) return plan_from_host_streams(iter_begin, n_iter);
   // The plan's buffers belong to the stream (Module::plan_buffers): the plan and the launch that reads it go into the stream
   // as one piece -- another shard on the same stream, launched from another host thread, must not get its plan in between.
   enqueue = std::unique_lock<std::mutex>(mod_->plan_buffers(device_, stream_).enqueue);
   // (the two switches of the plan are a call's, not a create's: the overflow test sets ORC_HMC_ROOM between the two)
   const Switches now = Switches::read();
   return now.hmc_plan_sync ? plan_with_host_wait(iter_begin, n_iter, now) : plan_on_plan_stream(iter_begin, n_iter, now);
}

// The plan of the call runs on the device's high-priority plan stream, ordered between the shard's earlier work and the iterate launch by
// events: the host does not wait for it (queued on the shard's own stream it sat behind the other stream's iterate launch for ~14 ms of
// a config-4 step, and the host with it).  A run that needs more than the room below raises the overflow flag, which the call's sync reports as
// an error.  The buffers are the stream's, shared by every batch that runs on it.
HmcPlan HmcPlanner::plan_on_plan_stream(int iter_begin, int n_iter, const Switches & now)
{
   // room for the resamples of a call: Poisson(n_iter lambda) + 8 standard deviations + 6 (a run draws more than that in a call with
   // probability ~1e-12); ORC_HMC_ROOM: the tests', too little on purpose
   const double mean = n_iter * lambda_;
   const int cap = now.hmc_room.set ? now.hmc_room.value : (int) std::ceil(mean + 8.0 * std::sqrt(mean) + 6.0);
   PlanStore & shared = mod_->plan_buffers(device_, stream_).store;
   shared.reserve((size_t) n_runs_ * cap, noise_bytes((size_t) n_runs_ * cap), &stream_);
   hipStream_t ps = mod_->plan_stream(device_);
   for (int k=0; k<2; k++) if (!ev_[k]) hip_check(hipEventCreateWithFlags(&ev_[k], hipEventDisableTiming), "hipEventCreate");
   overflow_armed_ = true;
   hip_check(hipEventRecord(ev_[0], stream_), "hipEventRecord");
   hip_check(hipStreamWaitEvent(ps, ev_[0], 0), "hipStreamWaitEvent");
   // (the flag is cleared where it is read, sync_begin: calls queued without a sync in between add to it)
   const hipError_t e = orc_launch_hmc_plan(d_mt_.as<uint32_t>(), d_next_.as<int>(), n_runs_, iter_begin, iter_begin + n_iter, cap, mn_, lambda_,
      precision_, shared.noise.as<void>(), shared.iters.as<int>(), d_overflow_.as<int>(), ps);
   hip_check(e, "hmc plan");
   hip_check(hipEventRecord(ev_[1], ps), "hipEventRecord");
   hip_check(hipStreamWaitEvent(stream_, ev_[1], 0), "hipStreamWaitEvent");
   return HmcPlan{ shared.iters.as<int>(), shared.noise.as<void>(), cap };
}

// ORC_HMC_PLAN_SYNC (round 2's way): the plan on the shard's own stream, in buffers of its own, and the host waits for it; a
// run with more resamples than `cap` makes the call start over with twice the room.  The first room is ORC_HMC_ROOM when set.
HmcPlan HmcPlanner::plan_with_host_wait(int iter_begin, int n_iter, const Switches & now)
{
   int cap = now.hmc_room.set ? now.hmc_room.value : 6 + (int) std::ceil(n_iter * lambda_ * 3.0);
   const size_t mt_bytes = (size_t) 625 * n_runs_ * sizeof(uint32_t), next_bytes = n_runs_ * sizeof(int);
   if (!d_mt_bak_) { d_mt_bak_.reset(dev_alloc<uint32_t>((size_t) 625 * n_runs_)); d_next_bak_.reset(dev_alloc<int>(n_runs_)); }
   for (;;)
   {
      own_.reserve((size_t) n_runs_ * cap, noise_bytes((size_t) n_runs_ * cap), nullptr);
      hip_check(hipMemcpyAsync(d_mt_bak_.as<void>(), d_mt_.as<void>(), mt_bytes, hipMemcpyDeviceToDevice, stream_), "hmc backup");
      hip_check(hipMemcpyAsync(d_next_bak_.as<void>(), d_next_.as<void>(), next_bytes, hipMemcpyDeviceToDevice, stream_), "hmc backup");
      hip_check(hipMemsetAsync(d_overflow_.as<void>(), 0, sizeof(int), stream_), "hmc overflow");
      const hipError_t e = orc_launch_hmc_plan(d_mt_.as<uint32_t>(), d_next_.as<int>(), n_runs_, iter_begin, iter_begin + n_iter, cap, mn_, lambda_,
         precision_, own_.noise.as<void>(), own_.iters.as<int>(), d_overflow_.as<int>(), stream_);
      hip_check(e, "hmc plan");
      int over = 0;
      hip_check(hipMemcpyAsync(&over, d_overflow_.as<void>(), sizeof(int), hipMemcpyDeviceToHost, stream_), "hmc overflow");
      hip_check(hipStreamSynchronize(stream_), "hmc plan sync");
      if (!over) return HmcPlan{ own_.iters.as<int>(), own_.noise.as<void>(), cap };
      hip_check(hipMemcpyAsync(d_mt_.as<void>(), d_mt_bak_.as<void>(), mt_bytes, hipMemcpyDeviceToDevice, stream_), "hmc restore");
      hip_check(hipMemcpyAsync(d_next_.as<void>(), d_next_bak_.as<void>(), next_bytes, hipMemcpyDeviceToDevice, stream_), "hmc restore");
      cap *= 2;
   }
}

// the host's GslRng streams (and the caller's blocks): drawn on the host's cores, then uploaded as [n_runs][maxr] and
// [n_runs][maxr][m n] with maxr the most resamples a run has in this call
HmcPlan HmcPlanner::plan_from_host_streams(int iter_begin, int n_iter)
{
   std::vector<std::vector<int>> iters(n_runs_);
   std::vector<std::vector<double>> noise(n_runs_);
   parallel_for_runs(n_runs_, [&](int lo, int hi) { host_.draw(lo, hi, iter_begin, iter_begin + n_iter, mn_, lambda_, iters, noise); });
   int maxr = 0;
   for (int k=0; k<n_runs_; k++) maxr = std::max(maxr, (int) iters[k].size());
   if (maxr == 0) return HmcPlan();
   std::vector<int> flat((size_t) n_runs_ * maxr, -1);
   for (int k=0; k<n_runs_; k++) for (size_t r=0; r<iters[k].size(); r++) flat[(size_t) k*maxr + r] = iters[k][r];
   const size_t ncount = (size_t) n_runs_ * maxr * mn_;
   own_.reserve(flat.size(), noise_bytes((size_t) n_runs_ * maxr), nullptr);
   hip_check(hipMemcpyAsync(own_.iters.as<void>(), flat.data(), flat.size()*sizeof(int), hipMemcpyHostToDevice, stream_), "hmc iters");
   std::vector<double> buf64(precision_ == 64 ? ncount : 0, 0.0);
   std::vector<float> buf32(precision_ == 64 ? 0 : ncount, 0.f);
   if (precision_ == 64)
      parallel_for_runs(n_runs_, [&](int k_lo, int k_hi) {
         for (int k=k_lo; k<k_hi; k++) std::copy(noise[k].begin(), noise[k].end(), buf64.begin() + (size_t) k*maxr*mn_);
      });
   else
      for (int k=0; k<n_runs_; k++)
         for (size_t e=0; e<noise[k].size(); e++) buf32[(size_t) k*maxr*mn_ + e] = (float) noise[k][e];
   const void * buf = precision_ == 64 ? (const void *) buf64.data() : (const void *) buf32.data();
   hip_check(hipMemcpyAsync(own_.noise.as<void>(), buf, noise_bytes((size_t) n_runs_ * maxr), hipMemcpyHostToDevice, stream_), "noise");
   hip_check(hipStreamSynchronize(stream_), "noise sync");
   return HmcPlan{ own_.iters.as<int>(), own_.noise.as<void>(), maxr };
}

void HmcPlanner::sync_begin()
{
   if (!overflow_armed_) return;
   hip_check(hipMemcpyAsync(&overflow_host_, d_overflow_.as<void>(), sizeof(int), hipMemcpyDeviceToHost, stream_), "hmc overflow");
   hip_check(hipMemsetAsync(d_overflow_.as<void>(), 0, sizeof(int), stream_), "hmc overflow");
}

void HmcPlanner::sync_end()
{
   if (!(overflow_armed_ && overflow_host_)) return;
   // the iterate kernel has run with a cut schedule and the generators have moved on: nothing to go back to
   overflow_host_ = 0;
   unusable_ = true;
   throw std::runtime_error("hmc: a run drew more momentum resamples in one iterate call than the plan has room for (probability ~1e-12 per run and call); "
                            "the batch is not usable any more: destroy it, create it again and iterate with fewer iterations per call!");
}

} // namespace orc
