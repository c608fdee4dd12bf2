// multistart.cpp -- host side of the multi-start calls (multistart.h): the perturbation of a batch's seeds, the best run per group
// by one selection (orc_batch_select_best[_by], orc_batch_select_clear), the respawn of the losing runs and the gather of the
// winners' rows, on the shard, over the shards, and the calls of the module that take a verdict or a clearance first.
#include "module.h"
#include "launch.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace orc {

// ================================================================ BatchShard ===
void BatchShard::launch_perturb(double scale, const unsigned int * seeds, const std::vector<double> & gen, int rank, const int * source_of_run, PerturbUpload & up)
{
   hipStream_t st = stream_;
   // one upload: the generators, then the limits of the columns
   std::vector<double> host(gen);
   host.insert(host.end(), jl_lo_.begin(), jl_lo_.end());
   host.insert(host.end(), jl_hi_.begin(), jl_hi_.end());
   up.gen.reset(dev_alloc<double>(host.size()));
   up.seeds.reset(dev_alloc<unsigned int>(n_runs));
   hip_check(hipMemcpyAsync(up.gen.as<void>(), host.data(), host.size()*sizeof(double), hipMemcpyHostToDevice, st), "perturb generators");
   hip_check(hipMemcpyAsync(up.seeds.as<void>(), seeds, n_runs*sizeof(unsigned int), hipMemcpyHostToDevice, st), "perturb seeds");
   const double * U = up.gen.as<double>(), * V = U + (size_t) rank * m, * lo = U + (size_t) 2 * rank * m, * hi = lo + n;
   const hipError_t e = orc_launch_perturb(d_traj_.as<void>(), params.precision, n_runs, n_points, n, m, up.seeds.as<unsigned int>(), rank, U, V,
      scale, lo, hi, orc_perturb_lds_bytes(m, n), source_of_run, st);
   hip_check(e, "perturb_kernel launch");
}

void BatchShard::perturb(double scale, const unsigned int * seeds, const std::vector<double> & gen, int rank)
{
   DeviceGuard guard(device);
   PerturbUpload up;
   launch_perturb(scale, seeds, gen, rank, nullptr, up);
   hip_check(hipStreamSynchronize(stream_), "perturb sync");
}

void BatchShard::respawn(int n_groups, const std::vector<int> & group_offs, const std::vector<int> & members, int column, int mode, int keep,
   double scale, const unsigned int * seeds, const std::vector<double> & gen, int rank, int * source_out, int * n_survivors_out)
{
   DeviceGuard guard(device);
   hipStream_t st = stream_;
   if (mode != 0 && !d_vkey_) throw std::runtime_error("respawn: no collision verdict on the device!");
   int max_group = 0;
   for (int g=0; g<n_groups; g++) max_group = std::max(max_group, group_offs[g+1] - group_offs[g]);
   // one upload of ints (the group table, then the members); launch_perturb makes the one of doubles
   std::vector<int> table(group_offs);
   table.insert(table.end(), members.begin(), members.end());
   DevBuf d_table, d_out;
   PerturbUpload up;
   d_table.reset(dev_alloc<int>(table.size()));
   d_out.reset(dev_alloc<int>((size_t) n_runs + n_groups));      // source_of_run, then n_survivors
   hip_check(hipMemcpyAsync(d_table.as<void>(), table.data(), table.size()*sizeof(int), hipMemcpyHostToDevice, st), "respawn groups");
   int * d_source = d_out.as<int>(), * d_nsurv = d_source + n_runs;
   const int * d_offs = d_table.as<int>(), * d_members = d_offs + group_offs.size();
   hip_check(orc_launch_respawn_rank(d_costs_.as<double>(), d_status_.as<int>(), mode ? d_vkey_.as<unsigned long long>() : nullptr, mode, column, keep,
      n_groups, d_offs, d_members, max_group, d_source, d_nsurv, st), "respawn_rank_kernel launch");
   hip_check(orc_launch_respawn_copy(d_traj_.as<void>(), d_AG_.as<void>(), params.precision, d_leap_.as<int>(), d_source, n_runs, n_points, n, m, st),
      "respawn_copy_kernel launch");
   if (scale > 0.0) launch_perturb(scale, seeds, gen, rank, d_source, up);
   std::vector<int> back((size_t) n_runs + n_groups);
   hip_check(hipMemcpyAsync(back.data(), d_out.as<void>(), back.size()*sizeof(int), hipMemcpyDeviceToHost, st), "respawn plan");
   hip_check(hipStreamSynchronize(st), "respawn sync");
   std::copy(back.begin(), back.begin() + n_runs, source_out);
   std::copy(back.begin() + n_runs, back.end(), n_survivors_out);
}

SelectResult BatchShard::select(int n_groups, const int * group, const SelectCriterion & c)
{
   DeviceGuard guard(device);
   hipStream_t st = stream_;
   if (c.collision_free && !d_vkey_) throw std::runtime_error("select_best: no collision verdict on the device!");
   if (c.by_margin && !d_clear_) throw std::runtime_error("select_clear: no clearance on the device!");
   const size_t G = (size_t) n_groups;
   DevBuf d_group, d_out;      // d_out: keys, clearances (8 bytes a group), then runs, counts (4 bytes a group)
   d_group.reset(dev_alloc<int>(n_runs)); d_out.reset(dev_alloc<unsigned long long>(3 * G));
   unsigned long long * d_key = d_out.as<unsigned long long>();
   double * d_best_clear = (double *)(d_key + G);
   int * d_best = (int *)(d_key + 2 * G), * d_count = d_best + G;
   hip_check(hipMemcpyAsync(d_group.as<void>(), group, n_runs*sizeof(int), hipMemcpyHostToDevice, st), "select groups");
   hip_check(hipMemsetAsync(d_key, 0xff, 2 * G * sizeof(unsigned long long), st), "select keys");      // (above every key; as a clearance: NaN)
   hip_check(hipMemsetAsync(d_best, 0x7f, G * sizeof(int), st), "select runs");      // (0x7f7f7f7f: above every run index)
   hip_check(hipMemsetAsync(d_count, 0, G * sizeof(int), st), "select counts");
   const SelectRule rule = { d_costs_.as<double>(), d_status_.as<int>(), c.collision_free ? d_vkey_.as<unsigned long long>() : nullptr,
      c.by_margin ? d_clear_.as<double>() : nullptr, c.by_margin ? d_clear_ns_.as<int>() : nullptr, c.margin, c.column };
   hip_check(orc_launch_select(rule, d_group.as<int>(), n_runs, n_groups, d_key, d_count, d_best, d_best_clear, st), "select kernels launch");
   std::vector<unsigned long long> back(3 * G);
   hip_check(hipMemcpyAsync(back.data(), d_out.as<void>(), back.size()*sizeof(unsigned long long), hipMemcpyDeviceToHost, st), "select results");
   hip_check(hipStreamSynchronize(st), "select sync");
   SelectResult out(G);
   const int * ints = (const int *)(back.data() + 2 * G);
   std::copy(back.begin(), back.begin() + G, out.key.begin());
   std::memcpy(out.clear.data(), back.data() + G, G * sizeof(double));
   std::copy(ints, ints + G, out.run.begin());
   std::copy(ints + G, ints + 2 * G, out.count.begin());
   return out;
}

void BatchShard::gettraj_rows(const std::vector<int> & rows, double * out)
{
   if (rows.empty()) return;
   DeviceGuard guard(device);
   hipStream_t st = stream_;
   const size_t row_len = (size_t) n_points * n;
   DevBuf d_rows, d_out;
   d_rows.reset(dev_alloc<int>(rows.size())); d_out.reset(dev_alloc<double>(rows.size() * row_len));
   hip_check(hipMemcpyAsync(d_rows.as<void>(), rows.data(), rows.size()*sizeof(int), hipMemcpyHostToDevice, st), "gather rows");
   hip_check(orc_launch_gather_rows(d_traj_.as<void>(), params.precision, d_rows.as<int>(), (int) rows.size(), row_len, d_out.as<double>(), st), "gather_rows_kernel launch");
   hip_check(hipMemcpyAsync(out, d_out.as<void>(), rows.size()*row_len*sizeof(double), hipMemcpyDeviceToHost, st), "gather download");
   hip_check(hipStreamSynchronize(st), "gather sync");
}

// ================================================================ Batch ===
PerturbPlan Batch::perturb_plan(double sigma) const
{
   if (!(sigma >= 0.0) || !std::isfinite(sigma)) throw std::runtime_error("perturb: sigma must be a finite number >= 0!");
   if (params.floating_base) throw std::runtime_error("perturb: floating-base batches (quaternion columns) are not supported!");
   if (params.free_start) throw std::runtime_error("perturb: batches with a free start point (start_tsr) are not supported!");
   const Metric & M = shards[0]->metric();
   const int D = M.D;
   if (D > ORC_SS_MAX_RANK || (D >= 2 && M.ss_rank != D))
      throw std::runtime_error("perturb: the device has only the dense inverse of this batch's metric (derivative > 4, or too few waypoints for it)!");
   if ((size_t) m * n > ORC_PERTURB_MAX_MN)
      throw std::runtime_error("perturb: the run's m x n Gaussians do not fit the LDS of one CU (m n <= " + std::to_string(ORC_PERTURB_MAX_MN) + ")!");
   PerturbPlan plan;
   plan.D = D;
   if (sigma == 0.0) return plan;
   // the generators of A^-1: U [D][m], then V [D][m]
   std::vector<double> & gen = plan.gen;
   gen.assign((size_t) 2 * D * m, 0.0);
   if (D == 1)
   {
      // A = a tridiag(-1, 2, -1) (both ends fixed): Ainv[i][j] = (i+1) (m-j) / ((m+1) a) for i <= j
      const double a = M.Aband[(size_t) 1*m + 0] / 2.0;
      for (int i=0; i<m; i++)
      {
         const double diag = M.Aband[(size_t) 1*m + i], lo = i > 0 ? M.Aband[(size_t) 0*m + i] : -a, hi = i < m-1 ? M.Aband[(size_t) 2*m + i] : -a;
         if (!(a > 0.0) || std::fabs(diag - 2.0*a) > 1e-12*a || std::fabs(lo + a) > 1e-12*a || std::fabs(hi + a) > 1e-12*a)
            throw std::runtime_error("perturb: the device has only the dense inverse of this batch's metric!");
         gen[i] = (double)(i + 1);
         gen[(size_t) m + i] = (double)(m - i) / ((double)(m + 1) * a);
      }
   }
   else
   {
      std::copy(M.ssU.begin(), M.ssU.end(), gen.begin());
      std::copy(M.ssV.begin(), M.ssV.end(), gen.begin() + (size_t) D * m);
   }
   // c = 1 / |row mid of A^-1|_2: sigma is the standard deviation of the middle waypoint's displacement
   std::vector<double> e(m, 0.0), row(m, 0.0);
   e[m / 2] = 1.0;
   metric_solve(M, e.data(), 1, row.data());
   double s2 = 0.0;
   for (int i=0; i<m; i++) s2 += row[i] * row[i];
   if (!(s2 > 0.0) || !std::isfinite(s2)) throw std::runtime_error("perturb: the metric's inverse has no middle row!");
   const double c = 1.0 / std::sqrt(s2);
   plan.scale = sigma * c;
   return plan;
}

void Batch::perturb(double sigma, const unsigned int * seeds)
{
   if (!(sigma >= 0.0) || !std::isfinite(sigma)) throw std::runtime_error("perturb: sigma must be a finite number >= 0!");
   if (!seeds) throw std::runtime_error("null argument: seeds");
   const PerturbPlan plan = perturb_plan(sigma);
   if (sigma == 0.0) return;
   for_shards([&](size_t k) { shards[k]->perturb(plan.scale, seeds + offs[k], plan.gen, plan.D); }, true);
}

std::vector<int> Batch::select_groups(int n_groups, const int * group_of_run) const
{
   if (!iterated) throw std::runtime_error("select_best: the batch has not been iterated (orc_batch_iterate with 0 iterations makes its costs valid)!");
   if (n_groups < 1) throw std::runtime_error("select_best: n_groups must be >=1!");
   std::vector<int> group(n_runs);
   if (group_of_run)
   {
      for (int r=0; r<n_runs; r++)
      {
         if (group_of_run[r] < 0 || group_of_run[r] >= n_groups) throw std::runtime_error("select_best: group_of_run entries must lie in [0, n_groups)!");
         group[r] = group_of_run[r];
      }
   }
   else
   {
      if (n_runs % n_groups) throw std::runtime_error("select_best: n_runs is not a multiple of n_groups (pass group_of_run)!");
      for (int r=0; r<n_runs; r++) group[r] = r / (n_runs / n_groups);
   }
   return group;
}

void Batch::select_column(int column)
{
   if (column < 0 || column > 2) throw std::runtime_error("select_best_by: cost_column must be 0 (total), 1 (obs) or 2 (smooth)!");
}

SelectResult Batch::select(int n_groups, const std::vector<int> & group, const SelectCriterion & c)
{
   std::vector<SelectResult> won(shards.size());
   for_shards([&](size_t k) { won[k] = shards[k]->select(n_groups, group.data() + offs[k], c); }, true);
   return merge_winners(won, offs, n_groups);
}

RespawnPlan Batch::respawn_plan(int cost_column, int n_groups, const int * group_of_run, int collision_mode, int keep, double sigma,
   const unsigned int * seeds) const
{
   if (!iterated) throw std::runtime_error("respawn: the batch has not been iterated since it was created or respawned (orc_batch_iterate with 0 iterations makes its costs valid)!");
   select_column(cost_column);
   if (collision_mode < 0 || collision_mode > 2) throw std::runtime_error("respawn: collision_mode must be 0 (ignore), 1 (require) or 2 (prefer)!");
   if (keep < 1) throw std::runtime_error("respawn: keep must be >=1!");
   const std::vector<int> group = select_groups(n_groups, group_of_run);
   RespawnPlan plan;
   plan.perturb = perturb_plan(sigma);
   if (sigma > 0.0 && !seeds) throw std::runtime_error("null argument: seeds (respawn with sigma > 0)");
   plan.column = cost_column; plan.mode = collision_mode; plan.keep = keep; plan.n_groups = n_groups;
   plan.shards = group_csr_by_shard(group, n_groups, offs);
   return plan;
}

void Batch::respawn(const RespawnPlan & plan, const unsigned int * seeds, int * source_of_run_out, int * n_survivors_out)
{
   std::vector<int> source(n_runs, -1), nsurv(plan.n_groups, 0);
   iterated = false;      // whatever happens from here on: the device's costs no longer describe its trajectories
   for_shards([&](size_t k) {
      const GroupCsr & sh = plan.shards[k];
      if (sh.groups.empty()) return;
      std::vector<int> ns(sh.groups.size());
      shards[k]->respawn((int) sh.groups.size(), sh.group_offs, sh.members, plan.column, plan.mode, plan.keep, plan.perturb.scale,
         seeds ? seeds + offs[k] : nullptr, plan.perturb.gen, plan.perturb.D, source.data() + offs[k], ns.data());
      for (int r=offs[k]; r<offs[k+1]; r++) if (source[r] >= 0) source[r] += offs[k];
      for (size_t q=0; q<sh.groups.size(); q++) nsurv[sh.groups[q]] = ns[q];
   }, true);
   if (source_of_run_out) std::copy(source.begin(), source.end(), source_of_run_out);
   if (n_survivors_out) std::copy(nsurv.begin(), nsurv.end(), n_survivors_out);
}

void Batch::gettraj_runs(const int * runs, int n_sel, double * out)
{
   const size_t row_len = (size_t) n_points * n;
   const size_t S = shards.size();
   std::vector<std::vector<int>> rows(S), where(S);      // per shard: local runs, and the rows of `out` they go to
   for (int q=0; q<n_sel; q++)      // (before anything is written: a rejected call leaves `out` alone)
      if (runs[q] < -1 || runs[q] >= n_runs) throw std::runtime_error("gettraj_runs: a run index is out of range (-1: a row of NaN)!");
   for (int q=0; q<n_sel; q++)
   {
      const int r = runs[q];
      if (r == -1) { for (size_t e=0; e<row_len; e++) out[(size_t) q * row_len + e] = std::nan(""); continue; }
      size_t k = 0;
      while (r >= offs[k+1]) k++;
      rows[k].push_back(r - offs[k]); where[k].push_back(q);
   }
   for_shards([&](size_t k) {
      std::vector<double> tmp(rows[k].size() * row_len);
      shards[k]->gettraj_rows(rows[k], tmp.data());
      for (size_t j=0; j<rows[k].size(); j++)
         std::memcpy(out + (size_t) where[k][j] * row_len, &tmp[j * row_len], row_len * sizeof(double));
   }, true);
}

// ================================================================ Module ===
// what a selection reports of its groups: every output may be NULL
static void report_winners(const SelectResult & w, int * best_run, double * best_cost, double * best_clear, int * n_eligible)
{
   for (size_t g=0; g<w.run.size(); g++)
   {
      if (best_run) best_run[g] = w.run[g];
      if (best_cost) best_cost[g] = w.cost(g);
      if (best_clear) best_clear[g] = w.clear[g];
      if (n_eligible) n_eligible[g] = w.count[g];
   }
}

void Module::batch_select_best(int id, int cost_column, int n_groups, const int * group_of_run, bool collision_free, int * best_run, double * best_cost,
   int * n_eligible)
{
   Batch & b = batch(id);
   Batch::select_column(cost_column);      // (the arguments first: the verdict below walks every trajectory)
   const std::vector<int> group = b.select_groups(n_groups, group_of_run);
   // the verdict's keys stay on the device, where the selection reads them
   if (collision_free) batch_collision_verdict_device(id, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, b.selection_scope());
   const SelectCriterion c = { collision_free, false, 0.0, cost_column };
   report_winners(b.select(n_groups, group, c), best_run, best_cost, nullptr, n_eligible);
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
   const SelectCriterion c = { false, true, margin, cost_column };
   report_winners(b.select(n_groups, group, c), best_run, best_cost, best_clearance, n_eligible);
}

void Module::batch_respawn(int id, int cost_column, int n_groups, const int * group_of_run, int collision_mode, int keep, double sigma,
   const unsigned int * seeds, int * source_of_run, int * n_survivors)
{
   Batch & b = batch(id);
   // every argument first, on the host: a rejected call costs no kernel and changes no bit
   const RespawnPlan plan = b.respawn_plan(cost_column, n_groups, group_of_run, collision_mode, keep, sigma, seeds);
   // the verdict of the current trajectories; its keys stay on the device, where the ranking reads them
   if (collision_mode != 0) batch_collision_verdict_device(id, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, b.selection_scope());
   b.respawn(plan, seeds, source_of_run, n_survivors);
}

} // namespace orc
