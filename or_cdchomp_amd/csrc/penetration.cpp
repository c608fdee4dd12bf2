// penetration.cpp -- host side of the penetration cost of given configurations and of waypoints (orc_batch_config_penetration,
// orc_batch_waypoint_penetration): the argument checks of the two clearance calls (Batch::config_clearance_check) and the
// margins', the queries dealt to the shards that own their runs as config_clearance.cpp deals them, the pairs by sphere, the
// launches of penetration_kernels.hip.  The inputs are the clearance's: verdict_inputs with the self check as the robot has it,
// BatchShard::verdict_walk_args for the tables.  Nothing is kept on the device.
#include "module.h"
#include "penetration_device.h"
#include <cmath>
#include <stdexcept>

namespace orc {

// the caller's arrays from query `first` on (a NULL stays NULL)
PenetrationOut PenetrationOut::from(size_t first, int n) const
{
   PenetrationOut o;
   o.cost = cost ? cost + 2*first : nullptr; o.grad = grad ? grad + (size_t) n*first : nullptr;
   o.clear = clear ? clear + 2*first : nullptr; o.key = key ? key + 2*first : nullptr;
   return o;
}

void Module::batch_config_penetration(int id, bool waypoints, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
   double margin_field, double margin_self, double * cost, double * grad, double * clearance, int * sphere, int * other)
{
   Batch & b = batch(id);
   b.config_clearance_check(waypoints, n_q, run_of_q, point_of_q, configs);
   if (!(margin_field >= 0.0) || !(margin_self >= 0.0) || std::isinf(margin_field) || std::isinf(margin_self))
      throw std::runtime_error(std::string(waypoints ? "waypoint" : "config") + " penetration: the margins are finite and not negative!");
   const VerdictInputs in = verdict_inputs(env.robot(b.robot_name), b, true);
   std::vector<unsigned int> key((sphere || other) ? (size_t) n_q * 2 : 0);
   PenetrationOut out;
   out.cost = cost; out.grad = grad; out.clear = clearance; out.key = key.empty() ? nullptr : key.data();
   b.config_penetration(in, waypoints, n_q, run_of_q, point_of_q, configs, margin_field, margin_self, out);
   for (size_t q=0; q<key.size(); q++)      // key: XML sphere << 16 | field, or the other sphere of a pair
   {
      const bool has = key[q] != ORC_CONFIG_NONE;
      if (sphere) sphere[q] = has ? (int)(key[q] >> 16) : -1;
      if (other) other[q] = has ? (int)(key[q] & 0xffffu) : -1;
   }
}

void Batch::config_penetration(const VerdictInputs & in, bool waypoints, int n_q, const int * run_of_q, const int * point_of_q,
   const double * configs, double margin_field, double margin_self, const PenetrationOut & out)
{
   if (shards.size() == 1)      // one shard owns every run
   {
      shards[0]->config_penetration(in, n_q, run_of_q, point_of_q, waypoints ? nullptr : configs, margin_field, margin_self, out);
      return;
   }
   if (waypoints && !run_of_q)      // every waypoint in storage order: a shard's queries are its slice
   {
      for_shards([&](size_t k) {
         shards[k]->config_penetration(in, (offs[k+1] - offs[k]) * n_points, nullptr, nullptr, nullptr, margin_field, margin_self,
            out.from((size_t) offs[k] * n_points, n));
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
      std::vector<double> cst(out.cost ? cnt*2 : 0), grd(out.grad ? cnt*n : 0), clr(out.clear ? cnt*2 : 0);
      std::vector<unsigned int> key(out.key ? cnt*2 : 0);
      PenetrationOut mine;
      mine.cost = out.cost ? cst.data() : nullptr; mine.grad = out.grad ? grd.data() : nullptr;
      mine.clear = out.clear ? clr.data() : nullptr; mine.key = out.key ? key.data() : nullptr;
      shards[k]->config_penetration(in, (int) cnt, run.data(), waypoints ? point.data() : nullptr, waypoints ? nullptr : rows.data(),
         margin_field, margin_self, mine);
      for (size_t i=0; i<cnt; i++)      // (a query belongs to one shard: the shards' threads write disjoint entries)
      {
         const size_t q = (size_t) at[i];
         for (int leg=0; leg<2; leg++)
         {
            if (out.cost) out.cost[q*2 + leg] = cst[i*2 + leg];
            if (out.clear) out.clear[q*2 + leg] = clr[i*2 + leg];
            if (out.key) out.key[q*2 + leg] = key[i*2 + leg];
         }
         if (out.grad) std::copy(grd.begin() + i*n, grd.begin() + (i+1)*n, out.grad + q*n);
      }
   }, true);
}

// (the walk's rule for `chunk` with this kernel's LDS, which the launch below takes)
int BatchShard::penetration_chunk() const
{
   const size_t real_size = params.precision == 64 ? sizeof(double) : sizeof(float);
   int chunk = 64;
   while (chunk > 4 && orc_penetration_lds_bytes(n, ms_.Sa, ms_.Sa_real, ms_.nj, real_size, chunk) > ORC_VERDICT_LDS_LIMIT) chunk -= 4;
   return chunk;
}

// The pairs by sphere (DevPenetration::sph_pair_offs, sph_pair_list): every slot's entries ascending by pair.  The pair's owner
// is its end a, or its end b when a is an inactive sphere; a pair of two inactive spheres is listed once, with the first live slot.
static void pairs_by_sphere(const std::vector<int> & pairs, int Sa, unsigned long long live_mask, std::vector<int> & offs, std::vector<int> & list)
{
   const int n_pairs = (int)(pairs.size() / 4);
   if (n_pairs >= (1 << 28)) throw std::runtime_error("penetration: too many pairs!");
   int first_live = -1;
   for (int s=Sa-1; s>=0; s--) if ((live_mask >> s) & 1ull) first_live = s;
   std::vector<std::vector<int>> of(Sa);
   for (int pi=0; pi<n_pairs; pi++)
   {
      const int ea = pairs[pi*4+0], eb = pairs[pi*4+1];
      if (ea >= Sa || eb >= Sa) throw std::runtime_error("penetration: a pair names a slot outside the position row!");
      if (ea >= 0) of[ea].push_back(pi << 3 | 4 | 0);
      if (eb >= 0) of[eb].push_back(pi << 3 | (ea < 0 ? 4 : 0) | 1);
      if (ea < 0 && eb < 0 && first_live >= 0) of[first_live].push_back(pi << 3 | 4 | 2);
   }
   offs.assign(Sa + 1, 0); list.clear();
   for (int s=0; s<Sa; s++)
   {
      list.insert(list.end(), of[s].begin(), of[s].end());
      offs[s+1] = (int) list.size();
   }
}

// the part of a launch that does not depend on the queries (project_clear.cpp launches the kernel once per round after one set-up)
template <typename real>
size_t BatchShard::penetration_setup(const VerdictInputs & in, PenetrationTables & t, DevPenetration<real> & v)
{
   hipStream_t st = stream_;
   const auto lds_bytes = [this](int chunk) { return orc_penetration_lds_bytes(n, ms_.Sa, ms_.Sa_real, ms_.nj, sizeof(real), chunk); };
   verdict_walk_args<real>(in, lds_bytes, t.walk, v);
   const size_t lds = lds_bytes(v.chunk);
   if (lds > ORC_VERDICT_LDS_LIMIT) throw std::runtime_error("penetration: the robot does not fit the kernel's shared memory!");
   v.key_out = nullptr; v.depth_out = nullptr;      // (the walk's outputs of the verdict: not written here)
   std::vector<int> & poffs = t.host_offs, & plist = t.host_list;      // (they live until the caller has synchronised)
   pairs_by_sphere(in.pairs, ms_.Sa, ms_.live_mask, poffs, plist);
   t.pair_offs.reset(dev_alloc<int>(poffs.size())); t.pair_list.reset(dev_alloc<int>(plist.size() + 1));
   hip_check(hipMemcpyAsync(t.pair_offs.as<void>(), poffs.data(), poffs.size()*sizeof(int), hipMemcpyHostToDevice, st), "penetration pair offsets");
   if (!plist.empty()) hip_check(hipMemcpyAsync(t.pair_list.as<void>(), plist.data(), plist.size()*sizeof(int), hipMemcpyHostToDevice, st), "penetration pair list");
   v.sph_pair_offs = t.pair_offs.as<int>(); v.sph_pair_list = t.pair_list.as<int>();
   return lds;
}
template size_t BatchShard::penetration_setup<double>(const VerdictInputs &, PenetrationTables &, DevPenetration<double> &);      // (project_clear.cpp calls them)
template size_t BatchShard::penetration_setup<float>(const VerdictInputs &, PenetrationTables &, DevPenetration<float> &);

template <typename real>
void BatchShard::config_penetration_typed(const VerdictInputs & in, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
   double margin_field, double margin_self, const PenetrationOut & out)
{
   hipStream_t st = stream_;
   PenetrationTables t;
   DevPenetration<real> v;
   const size_t lds = penetration_setup<real>(in, t, v);
   DevBuf d_run, d_point, d_cfg, d_cost, d_grad, d_clr, d_key;
   const size_t n2 = (size_t) n_q * 2, ng = (size_t) n_q * n;
   v.n_q = n_q; v.run_of_q = nullptr; v.point_of_q = nullptr; v.configs = nullptr;
   v.margin_field = (real) margin_field; v.margin_self = (real) margin_self;
   if (run_of_q)
   {
      d_run.reset(dev_alloc<int>(n_q));
      hip_check(hipMemcpyAsync(d_run.as<void>(), run_of_q, (size_t) n_q*sizeof(int), hipMemcpyHostToDevice, st), "penetration runs");
      v.run_of_q = d_run.as<int>();
   }
   if (point_of_q)
   {
      d_point.reset(dev_alloc<int>(n_q));
      hip_check(hipMemcpyAsync(d_point.as<void>(), point_of_q, (size_t) n_q*sizeof(int), hipMemcpyHostToDevice, st), "penetration points");
      v.point_of_q = d_point.as<int>();
   }
   std::vector<real> narrowed;      // (a precision-32 batch: narrowed as set_traj narrows; it lives until the copy is done)
   if (configs)
   {
      const size_t count = (size_t) n_q * n;
      d_cfg.reset(dev_alloc<real>(count));
      const void * src = configs;
      if (sizeof(real) != sizeof(double)) { narrowed.assign(configs, configs + count); src = narrowed.data(); }
      hip_check(hipMemcpyAsync(d_cfg.as<void>(), src, count*sizeof(real), hipMemcpyHostToDevice, st), "penetration rows");
      v.configs = d_cfg.as<const real>();
   }
   d_cost.reset(dev_alloc<double>(n2)); d_grad.reset(dev_alloc<double>(ng)); d_clr.reset(dev_alloc<double>(n2)); d_key.reset(dev_alloc<unsigned int>(n2));
   hip_check(hipMemsetAsync(d_grad.as<void>(), 0, ng*sizeof(double), st), "penetration gradient");
   v.cost_out = d_cost.as<double>(); v.grad_out = d_grad.as<double>(); v.clear_out = d_clr.as<double>(); v.ckey_out = d_key.as<unsigned int>();
   hip_check(orc_launch_penetration(v, lds, st, plan_.variant & ORC_VAR_TREE), "penetration_kernel launch");
   if (out.cost) hip_check(hipMemcpyAsync(out.cost, d_cost.as<void>(), n2*sizeof(double), hipMemcpyDeviceToHost, st), "penetration costs");
   if (out.grad) hip_check(hipMemcpyAsync(out.grad, d_grad.as<void>(), ng*sizeof(double), hipMemcpyDeviceToHost, st), "penetration gradients");
   if (out.clear) hip_check(hipMemcpyAsync(out.clear, d_clr.as<void>(), n2*sizeof(double), hipMemcpyDeviceToHost, st), "penetration minima");
   if (out.key) hip_check(hipMemcpyAsync(out.key, d_key.as<void>(), n2*sizeof(unsigned int), hipMemcpyDeviceToHost, st), "penetration keys");
   hip_check(hipStreamSynchronize(st), "penetration sync");
}

void BatchShard::config_penetration(const VerdictInputs & in, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
   double margin_field, double margin_self, const PenetrationOut & out)
{
   DeviceGuard guard(device);
   if (params.precision == 64) config_penetration_typed<double>(in, n_q, run_of_q, point_of_q, configs, margin_field, margin_self, out);
   else config_penetration_typed<float>(in, n_q, run_of_q, point_of_q, configs, margin_field, margin_self, out);
}

} // namespace orc
