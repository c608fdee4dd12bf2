// config_clearance.cpp -- host side of the clearance of given configurations and of waypoints (orc_batch_config_clearance,
// orc_batch_waypoint_clearance): the checks of their arguments in one place, the queries dealt to the shards that own their
// runs, the launches of config_kernels.hip.  The inputs are the clearance's (clearance.cpp): verdict_inputs with the self
// check as the robot has it, and BatchShard::verdict_walk_args for the tables; vmax plays no part.  Nothing is kept: no
// trajectory, cost, status or key is written, and the minima of the last `clearance` (d_clear_) stay as they are.
#include "module.h"
#include "config_device.h"
#include <cmath>
#include <stdexcept>

namespace orc {

void Batch::config_clearance_check(bool waypoints, int n_q, const int * run_of_q, const int * point_of_q, const double * configs) const
{
   const char * who = waypoints ? "waypoint clearance" : "config clearance";
   if (n_q < 1 || n_q > ORC_CONFIG_MAX_Q) throw std::runtime_error(std::string(who) + ": n_q must lie in [1, 4194304]!");
   if (!waypoints && !configs) throw std::runtime_error(std::string(who) + ": configs [n_q][n] is NULL!");
   if (waypoints && (run_of_q == nullptr) != (point_of_q == nullptr))
      throw std::runtime_error(std::string(who) + ": run_of_q and point_of_q are both given or both NULL!");
   if (waypoints && !run_of_q && (long long) n_q != (long long) n_runs * n_points)
      throw std::runtime_error(std::string(who) + ": without run_of_q and point_of_q, n_q must be n_runs * n_points!");
   for (int q=0; run_of_q && q<n_q; q++)
      if (run_of_q[q] < 0 || run_of_q[q] >= n_runs) throw std::runtime_error(std::string(who) + ": a run_of_q entry lies outside [0, n_runs)!");
   for (int q=0; waypoints && point_of_q && q<n_q; q++)
      if (point_of_q[q] < 0 || point_of_q[q] >= n_points) throw std::runtime_error(std::string(who) + ": a point_of_q entry lies outside [0, n_points)!");
}

void Module::batch_config_clearance(int id, bool waypoints, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
   double * clearance, int * sphere, int * other)
{
   Batch & b = batch(id);
   b.config_clearance_check(waypoints, n_q, run_of_q, point_of_q, configs);
   const VerdictInputs in = verdict_inputs(env.robot(b.robot_name), b, true);
   std::vector<unsigned int> key((sphere || other) ? (size_t) n_q * 2 : 0);
   b.config_clearance(in, waypoints, n_q, run_of_q, point_of_q, configs, clearance, key.empty() ? nullptr : key.data());
   // key: XML sphere << 16 | field, or the other sphere of a pair
   for (size_t q=0; q<key.size(); q++)
   {
      const bool has = key[q] != ORC_CONFIG_NONE;
      if (sphere) sphere[q] = has ? (int)(key[q] >> 16) : -1;
      if (other) other[q] = has ? (int)(key[q] & 0xffffu) : -1;
   }
}

void Batch::config_clearance(const VerdictInputs & in, bool waypoints, int n_q, const int * run_of_q, const int * point_of_q,
   const double * configs, double * clear_out, unsigned int * key_out)
{
   config_clearance_check(waypoints, n_q, run_of_q, point_of_q, configs);
   if (shards.size() == 1)      // one shard owns every run: the gather below would be the identity, and copies n_q rows to say so
   {
      shards[0]->config_clearance(in, n_q, run_of_q, point_of_q, waypoints ? nullptr : configs, clear_out, key_out);
      return;
   }
   if (waypoints && !run_of_q)      // every waypoint in storage order: a shard's queries are its slice
   {
      for_shards([&](size_t k) {
         const size_t w0 = (size_t) offs[k] * n_points;
         shards[k]->config_clearance(in, (offs[k+1] - offs[k]) * n_points, nullptr, nullptr, nullptr, clear_out ? clear_out + 2*w0 : nullptr,
            key_out ? key_out + 2*w0 : nullptr);
      }, true);
      return;
   }
   for_shards([&](size_t k) {
      const int r0 = offs[k], r1 = offs[k+1];
      // the queries whose run this shard owns, in their order, with the run rebased to the shard
      std::vector<int> at, run, point;
      std::vector<double> rows;
      for (int q=0; q<n_q; q++)
      {
         const int r = run_of_q ? run_of_q[q] : 0;
         if (r < r0 || r >= r1) continue;
         at.push_back(q); run.push_back(r - r0);
         if (waypoints) point.push_back(point_of_q[q]);
         else rows.insert(rows.end(), configs + (size_t) q*n, configs + (size_t)(q+1)*n);
      }
      if (at.empty()) return;
      const size_t cnt = at.size();
      std::vector<double> clr(clear_out ? cnt*2 : 0);
      std::vector<unsigned int> key(key_out ? cnt*2 : 0);
      shards[k]->config_clearance(in, (int) cnt, run.data(), waypoints ? point.data() : nullptr, waypoints ? nullptr : rows.data(),
         clear_out ? clr.data() : nullptr, key_out ? key.data() : nullptr);
      for (size_t i=0; i<cnt; i++)      // (a query belongs to one shard: the shards' threads write disjoint entries)
         for (int leg=0; leg<2; leg++)
         {
            if (clear_out) clear_out[(size_t) at[i]*2 + leg] = clr[i*2 + leg];
            if (key_out) key_out[(size_t) at[i]*2 + leg] = key[i*2 + leg];
         }
   }, true);
}

// (BatchShard::verdict_walk_args's choice, which the launch below takes; here for whoever wants to know it without a launch)
int BatchShard::config_chunk() const
{
   const size_t real_size = params.precision == 64 ? sizeof(double) : sizeof(float);
   int chunk = 64;
   while (chunk > 4 && orc_config_clearance_lds_bytes(n, ms_.Sa, ms_.Sa_real, ms_.nj, real_size, chunk) > ORC_VERDICT_LDS_LIMIT) chunk -= 4;
   return chunk;
}

template <typename real>
void BatchShard::config_clearance_typed(const VerdictInputs & in, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
   double * clear_out, unsigned int * key_out)
{
   hipStream_t st = stream_;
   const auto lds_bytes = [this](int chunk) { return orc_config_clearance_lds_bytes(n, ms_.Sa, ms_.Sa_real, ms_.nj, sizeof(real), chunk); };
   VerdictTables t;
   DevConfigClearance<real> v;
   verdict_walk_args<real>(in, lds_bytes, t, v);
   const size_t lds = lds_bytes(v.chunk);
   if (lds > ORC_VERDICT_LDS_LIMIT) throw std::runtime_error("config clearance: the robot does not fit the kernel's shared memory!");
   DevBuf d_run, d_point, d_cfg, d_clr, d_key;
   const size_t n2 = (size_t) n_q * 2;
   v.key_out = nullptr; v.depth_out = nullptr;      // (the walk's outputs of the verdict: not written here)
   v.n_q = n_q; v.run_of_q = nullptr; v.point_of_q = nullptr; v.configs = nullptr;
   if (run_of_q)
   {
      d_run.reset(dev_alloc<int>(n_q));
      hip_check(hipMemcpyAsync(d_run.as<void>(), run_of_q, (size_t) n_q*sizeof(int), hipMemcpyHostToDevice, st), "config clearance runs");
      v.run_of_q = d_run.as<int>();
   }
   if (point_of_q)
   {
      d_point.reset(dev_alloc<int>(n_q));
      hip_check(hipMemcpyAsync(d_point.as<void>(), point_of_q, (size_t) n_q*sizeof(int), hipMemcpyHostToDevice, st), "config clearance points");
      v.point_of_q = d_point.as<int>();
   }
   std::vector<real> narrowed;      // (a precision-32 batch: narrowed as set_traj narrows; it lives until the copy is done)
   if (configs)
   {
      const size_t count = (size_t) n_q * n;
      d_cfg.reset(dev_alloc<real>(count));
      const void * src = configs;
      if (sizeof(real) != sizeof(double)) { narrowed.assign(configs, configs + count); src = narrowed.data(); }
      hip_check(hipMemcpyAsync(d_cfg.as<void>(), src, count*sizeof(real), hipMemcpyHostToDevice, st), "config clearance rows");
      v.configs = d_cfg.as<const real>();
   }
   d_clr.reset(dev_alloc<double>(n2)); d_key.reset(dev_alloc<unsigned int>(n2));
   v.clear_out = d_clr.as<double>(); v.ckey_out = d_key.as<unsigned int>();
   hip_check(orc_launch_config_clearance(v, lds, st, plan_.variant & ORC_VAR_TREE), "config_clearance_kernel launch");
   if (clear_out) hip_check(hipMemcpyAsync(clear_out, d_clr.as<void>(), n2*sizeof(double), hipMemcpyDeviceToHost, st), "config clearance minima");
   if (key_out) hip_check(hipMemcpyAsync(key_out, d_key.as<void>(), n2*sizeof(unsigned int), hipMemcpyDeviceToHost, st), "config clearance keys");
   hip_check(hipStreamSynchronize(st), "config clearance sync");
}

void BatchShard::config_clearance(const VerdictInputs & in, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
   double * clear_out, unsigned int * key_out)
{
   DeviceGuard guard(device);
   if (params.precision == 64) config_clearance_typed<double>(in, n_q, run_of_q, point_of_q, configs, clear_out, key_out);
   else config_clearance_typed<float>(in, n_q, run_of_q, point_of_q, configs, clear_out, key_out);
}

} // namespace orc
