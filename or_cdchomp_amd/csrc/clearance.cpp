// clearance.cpp -- host side of the clearance of a batch's runs (orc_batch_clearance; the selection by margin that reads it is
// multistart.cpp's): the checks of its arguments and the launches of clearance_kernels.hip on every shard.  What it shares with
// the device-planned collision verdict is verdict.cpp's: verdict_inputs, Batch::verdict_scope_check and
// BatchShard::verdict_planned_args, which puts the tables, vmax and the scope on the device.
#include "module.h"
#include "clearance_device.h"
#include <stdexcept>

namespace orc {

void Batch::clearance_check(int which, const unsigned char * examine, int max_samples) const
{
   if (which < 0 || which > 2) throw std::runtime_error("clearance: which is 0 (the runs of examine), 1 (the candidates) or 2 (every run)!");
   const bool cap_ok = max_samples >= 1 && max_samples <= ORC_CLEARANCE_MAX_SAMPLES;
   verdict_scope_check("clearance", which, examine, "which 1 (the candidates) and 2 (every run) take", cap_ok ? nullptr : "clearance: max_samples must lie in [1, 1048576]!");
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
   VerdictTables t;
   DevClearance<real> v;
   const size_t lds = verdict_planned_args<real>("clearance", "clearance", orc_clearance_lds_bytes, in, scope, t, v);
   DevBuf d_time, d_key;
   const size_t n2 = (size_t) n_runs * 2;
   d_time.reset(dev_alloc<double>(n2)); d_key.reset(dev_alloc<unsigned long long>(n2));
   if (!d_clear_) { d_clear_.reset(dev_alloc<double>(n2)); d_clear_ns_.reset(dev_alloc<int>(n_runs)); }
   v.key_out = nullptr; v.depth_out = nullptr;      // (the walk's outputs of the verdict: not written here)
   v.max_samples = max_samples;
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

} // namespace orc
