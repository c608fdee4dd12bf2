// penetration.cpp -- host side of the penetration cost of given configurations and of waypoints (orc_batch_config_penetration,
// orc_batch_waypoint_penetration): the argument checks of the two clearance calls (Batch::config_clearance_check) and the
// margins', the queries dealt to the shards that own their runs (Batch::deal_by_run), the pairs by sphere, the launches of
// penetration_kernels.hip.  The inputs are the clearance's: verdict_inputs with the self check as the robot has it,
// BatchShard::verdict_walk_args for the tables.  Nothing is kept on the device.
#include "module.h"
#include "penetration_device.h"
#include "query_upload.h"
#include <cmath>
#include <stdexcept>

namespace orc {

// what the calls with margins reject of them (who: the call's name in what it throws)
void margins_check(const char * who, double margin_field, double margin_self)
{
   if (!(margin_field >= 0.0) || !(margin_self >= 0.0) || std::isinf(margin_field) || std::isinf(margin_self))
      throw std::runtime_error(std::string(who) + ": the margins are finite and not negative!");
}

void Module::batch_config_penetration(int id, bool waypoints, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
   double margin_field, double margin_self, double * cost, double * grad, double * clearance, int * sphere, int * other)
{
   Batch & b = batch(id);
   b.config_clearance_check(waypoints, n_q, run_of_q, point_of_q, configs);
   margins_check(waypoints ? "waypoint penetration" : "config penetration", margin_field, margin_self);
   const VerdictInputs in = verdict_inputs(env.robot(b.robot_name), b, true);
   std::vector<unsigned int> key((sphere || other) ? (size_t) n_q * 2 : 0);
   PenetrationOut out;
   out.cost = cost; out.grad = grad; out.clear = clearance; out.key = key.empty() ? nullptr : key.data();
   b.config_penetration(in, waypoints, n_q, run_of_q, point_of_q, configs, margin_field, margin_self, out);
   unpack_keys(key.data(), key.size(), sphere, other);
}

void Batch::config_penetration(const VerdictInputs & in, bool waypoints, int n_q, const int * run_of_q, const int * point_of_q,
   const double * configs, double margin_field, double margin_self, const PenetrationOut & out)
{
   deal_by_run(n_q, run_of_q, waypoints && !run_of_q, { deal_in(waypoints ? point_of_q : nullptr, 1), deal_in(waypoints ? nullptr : configs, n) },
      { deal_out(out.cost, 2), deal_out(out.grad, n), deal_out(out.clear, 2), deal_out(out.key, 2) },
      [&](size_t k, int cnt, const int * run, const std::vector<void *> & in_col, const std::vector<void *> & out_col) {
         PenetrationOut mine;
         mine.cost = (double *) out_col[0]; mine.grad = (double *) out_col[1]; mine.clear = (double *) out_col[2]; mine.key = (unsigned int *) out_col[3];
         shards[k]->config_penetration(in, cnt, run, (const int *) in_col[0], (const double *) in_col[1], margin_field, margin_self, mine);
      });
}

// (the choice of the launch below)
int BatchShard::penetration_chunk() const
{
   const size_t real_size = params.precision == 64 ? sizeof(double) : sizeof(float);
   return walk_chunk([&](int chunk) { return orc_penetration_lds_bytes(n, ms_.Sa, ms_.Sa_real, ms_.nj, real_size, chunk); });
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
   PenetrationTables t;
   DevPenetration<real> v;
   const size_t lds = penetration_setup<real>(in, t, v);
   QueryUpload<real> up(stream_, "penetration");
   const size_t n2 = (size_t) n_q * 2, ng = (size_t) n_q * n;
   v.n_q = n_q; v.run_of_q = up.ints(run_of_q, n_q, "runs"); v.point_of_q = up.ints(point_of_q, n_q, "points");
   v.configs = configs ? up.rows(configs, ng) : nullptr;
   v.margin_field = (real) margin_field; v.margin_self = (real) margin_self;
   v.cost_out = up.template alloc<double>(n2); v.grad_out = up.template alloc<double>(ng);
   v.clear_out = up.template alloc<double>(n2); v.ckey_out = up.template alloc<unsigned int>(n2);
   up.zero(v.grad_out, ng*sizeof(double), "gradient");
   hip_check(orc_launch_penetration(v, lds, up.st, plan_.variant & ORC_VAR_TREE), "penetration_kernel launch");
   up.down(out.cost, v.cost_out, n2*sizeof(double), "costs");
   up.down(out.grad, v.grad_out, ng*sizeof(double), "gradients");
   up.down(out.clear, v.clear_out, n2*sizeof(double), "minima");
   up.down(out.key, v.ckey_out, n2*sizeof(unsigned int), "keys");
   up.sync();
}

void BatchShard::config_penetration(const VerdictInputs & in, int n_q, const int * run_of_q, const int * point_of_q, const double * configs,
   double margin_field, double margin_self, const PenetrationOut & out)
{
   DeviceGuard guard(device);
   if (params.precision == 64) config_penetration_typed<double>(in, n_q, run_of_q, point_of_q, configs, margin_field, margin_self, out);
   else config_penetration_typed<float>(in, n_q, run_of_q, point_of_q, configs, margin_field, margin_self, out);
}

} // namespace orc
