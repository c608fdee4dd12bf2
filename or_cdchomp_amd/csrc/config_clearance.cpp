// config_clearance.cpp -- host side of the clearance of given configurations and of waypoints (orc_batch_config_clearance,
// orc_batch_waypoint_clearance): the checks of their arguments in one place, the queries dealt to the shards that own their
// runs (Batch::deal_by_run), the launches of config_kernels.hip.  The inputs are the clearance's (clearance.cpp): verdict_inputs with the self
// check as the robot has it, and BatchShard::verdict_walk_args for the tables; vmax plays no part.  Nothing is kept: no
// trajectory, cost, status or key is written, and the minima of the last `clearance` (d_clear_) stay as they are.
#include "module.h"
#include "config_device.h"
#include "query_upload.h"
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
   unpack_keys(key.data(), key.size(), sphere, other);
}

// key: XML sphere << 16 | field, or the other sphere of a pair; -1 and -1 without one
void unpack_keys(const unsigned int * key, size_t count, int * sphere, int * other)
{
   for (size_t q=0; q<count; q++)
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
   deal_by_run(n_q, run_of_q, waypoints && !run_of_q, { deal_in(waypoints ? point_of_q : nullptr, 1), deal_in(waypoints ? nullptr : configs, n) },
      { deal_out(clear_out, 2), deal_out(key_out, 2) },
      [&](size_t k, int cnt, const int * run, const std::vector<void *> & in_col, const std::vector<void *> & out_col) {
         shards[k]->config_clearance(in, cnt, run, (const int *) in_col[0], (const double *) in_col[1], (double *) out_col[0], (unsigned int *) out_col[1]);
      });
}

// (the choice of the launch below; here for whoever wants to know it without a launch)
int BatchShard::config_chunk() const
{
   const size_t real_size = params.precision == 64 ? sizeof(double) : sizeof(float);
   return walk_chunk([&](int chunk) { return orc_config_clearance_lds_bytes(n, ms_.Sa, ms_.Sa_real, ms_.nj, real_size, chunk); });
}

template <typename real>
void BatchShard::config_clearance_typed(const VerdictInputs & in, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
   double * clear_out, unsigned int * key_out)
{
   const auto lds_bytes = [this](int chunk) { return orc_config_clearance_lds_bytes(n, ms_.Sa, ms_.Sa_real, ms_.nj, sizeof(real), chunk); };
   VerdictTables t;
   DevConfigClearance<real> v;
   verdict_walk_args<real>(in, lds_bytes, t, v);
   const size_t lds = lds_bytes(v.chunk);
   if (lds > ORC_VERDICT_LDS_LIMIT) throw std::runtime_error("config clearance: the robot does not fit the kernel's shared memory!");
   QueryUpload<real> up(stream_, "config clearance");
   const size_t n2 = (size_t) n_q * 2;
   v.key_out = nullptr; v.depth_out = nullptr;      // (the walk's outputs of the verdict: not written here)
   v.n_q = n_q; v.run_of_q = up.ints(run_of_q, n_q, "runs"); v.point_of_q = up.ints(point_of_q, n_q, "points");
   v.configs = configs ? up.rows(configs, (size_t) n_q * n) : nullptr;
   v.clear_out = up.template alloc<double>(n2); v.ckey_out = up.template alloc<unsigned int>(n2);
   hip_check(orc_launch_config_clearance(v, lds, up.st, plan_.variant & ORC_VAR_TREE), "config_clearance_kernel launch");
   up.down(clear_out, v.clear_out, n2*sizeof(double), "minima");
   up.down(key_out, v.ckey_out, n2*sizeof(unsigned int), "keys");
   up.sync();
}

void BatchShard::config_clearance(const VerdictInputs & in, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
   double * clear_out, unsigned int * key_out)
{
   DeviceGuard guard(device);
   if (params.precision == 64) config_clearance_typed<double>(in, n_q, run_of_q, point_of_q, configs, clear_out, key_out);
   else config_clearance_typed<float>(in, n_q, run_of_q, point_of_q, configs, clear_out, key_out);
}

} // namespace orc
