// hmc.h -- the momentum-resampling plan of HMC runs, host side (hmc.cpp): which iterations of an iterate call resample a run's
// momentum, and with what noise (src/orcdchomp_mod.cpp:2303-2304, 2634-2635, 2755-2768).  HostNoiseStreams, in front, uses
// nothing of HIP or the module.
#pragma once
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>
#include "host_math.h"      // GslRng
#include "devbuf.h"         // DevBuf
#include "stages.h"         // Switches

namespace orc {

// The streams of a shard's runs in host GslRng objects (src/orcdchomp_mod.cpp:948-952) and the blocks a caller supplied in their place
// ([n_runs][ext_blocks][m n]).  `next` persists over the calls while the iteration counter restarts at 0 in each (mod.cpp:2752).
struct HostNoiseStreams
{
   std::vector<GslRng> rng;
   std::vector<int> next, ext_used;      // next resample iteration; supplied blocks consumed by the current iterate call
   std::vector<double> ext; int ext_blocks = 0;
   // Runs [lo, hi), iterations [iter_begin, iter_end): appends to iters[k] the resample iterations relative to iter_begin and to noise[k]
   // their m n values each (the scale uses the call's own counter, mod.cpp:2757).  A supplied block replaces what the stream drew, and
   // the stream is advanced all the same.  No HIP call; the runs are independent of each other.
   void draw(int lo, int hi, int iter_begin, int iter_end, size_t mn, double lambda, std::vector<std::vector<int>> & iters,
      std::vector<std::vector<double>> & noise)
   {
      for (int k=lo; k<hi; k++)
      {
         int & used_ext = ext_used[k];
         for (int it=iter_begin; it<iter_end; it++)
         {
            if (it != next[k]) continue;
            const double alpha = 100.0 * std::exp(0.02 * it);
            const double sigma = 1.0 / std::sqrt(alpha);
            const size_t off = noise[k].size();
            noise[k].resize(off + mn);
            for (size_t e=0; e<mn; e++) noise[k][off+e] = rng[k].gaussian(sigma);
            if (ext_blocks > 0 && used_ext < ext_blocks)
               std::memcpy(&noise[k][off], &ext[((size_t) k * ext_blocks + used_ext) * mn], mn*sizeof(double));
            used_ext++;
            iters[k].push_back(it - iter_begin);
            next[k] += 1 + (int)(-std::log(rng[k].uniform()) / lambda);
         }
      }
   }
};

// what the iterate launch reads of a call's plan: iterations [n_runs][max_resamples] (-1: none), noise [n_runs][max_resamples][m n] in
// the batch's precision.  Empty: the call resamples nothing
struct HmcPlan { const int * iters = nullptr; const void * noise = nullptr; int max_resamples = 0; };

// The device memory of a plan: it grows only, frees before it allocates, and first waits for `*drain` when the caller names a
// stream whose pending work may still read it.
struct PlanStore
{
   DevBuf iters, noise;
   size_t iters_count = 0, noise_bytes = 0;
   void reserve(size_t icount, size_t nbytes, const hipStream_t * drain);
};

class Module;

// The plan of one shard's runs.  The streams live on the device for large batches (hmc_kernels.hip: one wavefront per run draws the plan
// of a call), in host GslRng objects otherwise (and whenever the caller supplies the noise: set_noise).
class HmcPlanner
{
public:
   HmcPlanner(Module * mod, int device, hipStream_t stream, int n_runs, size_t mn, int precision, double lambda, bool use_hmc,
      const Switches & sw, const unsigned int * seeds);
   ~HmcPlanner();
   void check_usable() const;      // throws once an overflow has cut the runs' schedules short
   // The plan of the iterations [iter_begin, iter_begin + n_iter), enqueued in front of the launch that reads it.  `enqueue` takes the
   // lock of the stream's plan buffers where the streams are the device's: hold it through that launch
   HmcPlan plan(int iter_begin, int n_iter, std::unique_lock<std::mutex> & enqueue);
   void sync_begin();              // enqueues the copy of the overflow flag and its clearing
   void sync_end();                // after the stream's wait: throws, and marks the batch, when a call ran out of room
   void set_noise(const double * noise, int n_blocks);
private:
   HmcPlan plan_on_plan_stream(int iter_begin, int n_iter, const Switches & now);
   HmcPlan plan_with_host_wait(int iter_begin, int n_iter, const Switches & now);
   HmcPlan plan_from_host_streams(int iter_begin, int n_iter);
   size_t noise_bytes(size_t resamples) const { return resamples * mn_ * (precision_ == 64 ? 8 : 4); }
   Module * mod_;
   int device_;
   hipStream_t stream_;
   int n_runs_;
   size_t mn_;
   int precision_;
   double lambda_;
   bool use_hmc_, on_device_ = false;
   PlanStore own_;                 // the host streams' and the synchronous plan's; the plan stream's is the module's (Module::plan_buffers)
   HostNoiseStreams host_;
   // on the device: mt19937 state [625][n_runs], next resample iteration [n_runs]; their backups are the synchronous plan's
   DevBuf d_mt_, d_next_, d_mt_bak_, d_next_bak_, d_overflow_;
   hipEvent_t ev_[2] = { nullptr, nullptr };       // iterate stream -> plan stream -> iterate stream
   int overflow_host_ = 0; bool overflow_armed_ = false;      // the plan's overflow flag, read (and cleared) with the results of a call
   bool unusable_ = false;
};

} // namespace orc
