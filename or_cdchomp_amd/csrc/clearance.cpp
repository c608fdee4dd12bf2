// clearance.cpp -- host side of the clearance of a batch's runs and of the selection by margin (orc_batch_clearance,
// orc_batch_select_clear): the checks of their arguments, the launches of clearance_kernels.hip and of the selection kernels
// of multistart_kernels.hip on every shard, and the merge of the shards' winners.  The tables the walk reads are the collision
// verdict's (verdict.cpp: verdict_inputs, BatchShard::verdict_walk_args).
#include "module.h"
#include "clearance_device.h"
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace orc {

void Batch::clearance_check(int which, const unsigned char * examine, int max_samples) const
{
   if (which < 0 || which > 2) throw std::runtime_error("clearance: which is 0 (the runs of examine), 1 (the candidates) or 2 (every run)!");
   if (which == 0 && !examine) throw std::runtime_error("clearance: which 0 needs examine [n_runs]!");
   if (which != 0 && examine) throw std::runtime_error("clearance: which 1 (the candidates) and 2 (every run) take no examine!");
   if (max_samples < 1 || max_samples > ORC_CLEARANCE_MAX_SAMPLES) throw std::runtime_error("clearance: max_samples must lie in [1, 1048576]!");
   if (which == 1 && !iterated) throw std::runtime_error("select_best: the batch has not been iterated (orc_batch_iterate with 0 iterations makes its costs valid)!");
}

// key: sample << 32 | XML sphere << 16 | field, or the other sphere of a pair
static void clearance_decode(const std::vector<unsigned long long> & key, int * sphere, int * other)
{
   for (size_t q=0; q<key.size(); q++)
   {
      const bool has = key[q] != ORC_VERDICT_NONE;
      if (sphere) sphere[q] = has ? (int)((key[q] >> 16) & 0xffffull) : -1;
      if (other) other[q] = has ? (int)(key[q] & 0xffffull) : -1;
   }
}

void Module::batch_clearance(int id, int which, const unsigned char * examine, int max_samples, double * clearance, double * time, int * sphere,
   int * other, int * n_samples)
{
   Batch & b = batch(id);
   b.clearance_check(which, examine, max_samples);
   const VerdictInputs in = verdict_inputs(env.robot(b.robot_name), b, true);
   std::vector<unsigned long long> key((sphere || other) ? (size_t) b.n_runs * 2 : 0);
   b.clearance(in, which, examine, max_samples, clearance, time, key.empty() ? nullptr : key.data(), n_samples);
   clearance_decode(key, sphere, other);
}

void Module::batch_select_clear(int id, int cost_column, int n_groups, const int * group_of_run, double margin, int max_samples,
   int * best_run, double * best_cost, double * best_clearance, int * n_eligible, int * n_samples)
{
   Batch & b = batch(id);
   // every argument first, on the host: a rejected call costs no kernel
   if (cost_column < 0 || cost_column > 3) throw std::runtime_error("select_clear: cost_column must be 0 (total), 1 (obs), 2 (smooth) or 3 (clearance)!");
   if (std::isnan(margin)) throw std::runtime_error("select_clear: margin is NaN!");
   const std::vector<int> group = b.select_groups(n_groups, group_of_run);
   b.clearance_check(1, nullptr, max_samples);
   const VerdictInputs in = verdict_inputs(env.robot(b.robot_name), b, true);
   b.clearance(in, 1, nullptr, max_samples, nullptr, nullptr, nullptr, n_samples);      // (the minima stay on the device)
   b.select_clear(n_groups, group, cost_column, margin, best_run, best_cost, best_clearance, n_eligible);
}

void Batch::clearance(const VerdictInputs & in, int which, const unsigned char * examine, int max_samples, double * clear_out, double * time_out,
   unsigned long long * key_out, int * n_samples_out)
{
   clearance_check(which, examine, max_samples);
   for_shards([&](size_t k) {
      const size_t r0 = (size_t) offs[k];
      VerdictScope mine;      // (every shard takes its slice of the caller's bytes)
      mine.which = which == 2 ? -1 : which;
      mine.examine = examine ? examine + r0 : nullptr;
      shards[k]->clearance(in, mine, max_samples, clear_out ? clear_out + 2*r0 : nullptr, time_out ? time_out + 2*r0 : nullptr,
         key_out ? key_out + 2*r0 : nullptr, n_samples_out ? n_samples_out + r0 : nullptr);
   }, true);
}

template <typename real>
void BatchShard::clearance_typed(const VerdictInputs & in, const VerdictScope & scope, int max_samples, double * clear_out, double * time_out,
   unsigned long long * key_out, int * n_samples_out)
{
   hipStream_t st = stream_;
   hip_check(hipStreamSynchronize(st), "clearance: pending work");
   if (n_points < 2 || (int) in.vmax.size() != n - in.col0) throw std::runtime_error("clearance: bad trajectory dimensions!");
   const auto lds_bytes = [this](int chunk) { return orc_clearance_lds_bytes(n_points, n, ms_.Sa, ms_.Sa_real, ms_.nj, sizeof(real), chunk); };
   VerdictTables t;
   DevClearance<real> v;
   verdict_walk_args<real>(in, lds_bytes, t, v);
   const size_t lds = lds_bytes(v.chunk);
   if (lds > 160*1024 - 256) throw std::runtime_error("trajectory too long for the batched collision verdict!");
   DevBuf d_time, d_key, d_vmax, d_examine;
   const size_t n2 = (size_t) n_runs * 2;
   d_time.reset(dev_alloc<double>(n2)); d_key.reset(dev_alloc<unsigned long long>(n2));
   if (!d_clear_) { d_clear_.reset(dev_alloc<double>(n2)); d_clear_ns_.reset(dev_alloc<int>(n_runs)); }
   d_vmax.reset(upload<double>(in.vmax, st));
   v.key_out = nullptr; v.depth_out = nullptr;      // (the walk's outputs of the verdict: not written here)
   v.col0 = in.col0; v.vmax = d_vmax.as<const double>(); v.max_samples = max_samples;
   v.examine = nullptr; v.cand_status = nullptr; v.cand_costs = nullptr;
   if (scope.which == 0)
   {
      d_examine.reset(dev_alloc<unsigned char>(n_runs));
      hip_check(hipMemcpyAsync(d_examine.as<void>(), scope.examine, n_runs, hipMemcpyHostToDevice, st), "clearance runs");
      v.examine = d_examine.as<unsigned char>();
   }
   else if (scope.which == 1) { v.cand_status = d_status_.as<int>(); v.cand_costs = d_costs_.as<double>(); }      // (what the last iterate call left)
   v.clear_out = d_clear_.as<double>(); v.ckey_out = d_key.as<unsigned long long>(); v.ctime_out = d_time.as<double>();
   v.n_samples_out = d_clear_ns_.as<int>();
   hip_check(orc_launch_clearance(v, lds, st, plan_.variant & ORC_VAR_TREE), "clearance_kernel launch");
   if (clear_out) hip_check(hipMemcpyAsync(clear_out, d_clear_.as<void>(), n2*sizeof(double), hipMemcpyDeviceToHost, st), "clearance minima");
   if (time_out) hip_check(hipMemcpyAsync(time_out, d_time.as<void>(), n2*sizeof(double), hipMemcpyDeviceToHost, st), "clearance times");
   if (key_out) hip_check(hipMemcpyAsync(key_out, d_key.as<void>(), n2*sizeof(unsigned long long), hipMemcpyDeviceToHost, st), "clearance keys");
   if (n_samples_out) hip_check(hipMemcpyAsync(n_samples_out, d_clear_ns_.as<void>(), n_runs*sizeof(int), hipMemcpyDeviceToHost, st), "clearance samples");
   hip_check(hipStreamSynchronize(st), "clearance sync");
}

void BatchShard::clearance(const VerdictInputs & in, const VerdictScope & scope, int max_samples, double * clear_out, double * time_out,
   unsigned long long * key_out, int * n_samples_out)
{
   DeviceGuard guard(device);
   if (params.precision == 64) clearance_typed<double>(in, scope, max_samples, clear_out, time_out, key_out, n_samples_out);
   else clearance_typed<float>(in, scope, max_samples, clear_out, time_out, key_out, n_samples_out);
}

void BatchShard::select_clear(int n_groups, const int * group, int column, double margin, unsigned long long * key_out, int * best_out,
   double * best_clear_out, int * count_out)
{
   DeviceGuard guard(device);
   hipStream_t st = stream_;
   if (!d_clear_) throw std::runtime_error("select_clear: no clearance on the device!");
   DevBuf group_buf, key_buf, best_buf, count_buf, clear_buf;
   group_buf.reset(dev_alloc<int>(n_runs)); key_buf.reset(dev_alloc<unsigned long long>(n_groups));
   best_buf.reset(dev_alloc<int>(n_groups)); count_buf.reset(dev_alloc<int>(n_groups)); clear_buf.reset(dev_alloc<double>(n_groups));
   int * d_group = group_buf.as<int>(), * d_best = best_buf.as<int>(), * d_count = count_buf.as<int>();
   unsigned long long * d_key = key_buf.as<unsigned long long>();
   hip_check(hipMemcpyAsync(d_group, group, n_runs*sizeof(int), hipMemcpyHostToDevice, st), "select groups");
   hip_check(hipMemsetAsync(d_key, 0xff, n_groups*sizeof(unsigned long long), st), "select keys");
   hip_check(hipMemsetAsync(d_best, 0x7f, n_groups*sizeof(int), st), "select runs");      // (0x7f7f7f7f: above every run index)
   hip_check(hipMemsetAsync(d_count, 0, n_groups*sizeof(int), st), "select counts");
   hip_check(orc_launch_select_clear(d_costs_.as<double>(), d_status_.as<int>(), d_clear_.as<double>(), d_clear_ns_.as<int>(), d_group, n_runs, n_groups,
      column, margin, d_key, d_count, d_best, clear_buf.as<double>(), st), "select_clear kernels launch");
   hip_check(hipMemcpyAsync(key_out, d_key, n_groups*sizeof(unsigned long long), hipMemcpyDeviceToHost, st), "select keys");
   hip_check(hipMemcpyAsync(best_out, d_best, n_groups*sizeof(int), hipMemcpyDeviceToHost, st), "select runs");
   hip_check(hipMemcpyAsync(count_out, d_count, n_groups*sizeof(int), hipMemcpyDeviceToHost, st), "select counts");
   hip_check(hipMemcpyAsync(best_clear_out, clear_buf.as<void>(), n_groups*sizeof(double), hipMemcpyDeviceToHost, st), "select clearance");
   hip_check(hipStreamSynchronize(st), "select sync");
}

void Batch::select_clear(int n_groups, const std::vector<int> & group, int column, double margin, int * best_run_out, double * best_cost_out,
   double * best_clear_out, int * n_eligible_out)
{
   const size_t S = shards.size();
   std::vector<unsigned long long> key(S * n_groups);
   std::vector<int> best(S * n_groups), count(S * n_groups);
   std::vector<double> clear(S * n_groups);
   for_shards([&](size_t k) {
      shards[k]->select_clear(n_groups, group.data() + offs[k], column, margin, key.data() + k * n_groups, best.data() + k * n_groups,
                              clear.data() + k * n_groups, count.data() + k * n_groups);
   }, true);
   // the merge of n_shards x n_groups candidates: the lower key, then the lower run (the shards hold ascending runs)
   for (int g=0; g<n_groups; g++)
   {
      unsigned long long bk = ~0ull; int br = -1, cnt = 0; double bc = std::nan("");
      for (size_t k=0; k<S; k++)
      {
         const size_t q = k * n_groups + g;
         cnt += count[q];
         if (count[q] > 0 && key[q] < bk) { bk = key[q]; br = offs[k] + best[q]; bc = clear[q]; }
      }
      if (best_run_out) best_run_out[g] = br;
      if (n_eligible_out) n_eligible_out[g] = cnt;
      if (best_clear_out) best_clear_out[g] = bc;
      if (best_cost_out)
      {
         double cost = HUGE_VAL;
         if (br >= 0)
         {
            const unsigned long long bits = (bk >> 63) ? (bk & 0x7fffffffffffffffull) : ~bk;      // (cost_key of multistart_kernels.hip, undone)
            std::memcpy(&cost, &bits, sizeof(double));
         }
         best_cost_out[g] = cost;
      }
   }
}

} // namespace orc
