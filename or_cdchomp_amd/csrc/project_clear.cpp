// project_clear.cpp -- host side of the projection onto TSRs and out of contact (orc_batch_project_tsr_clear): the argument
// checks of the projection (Module::project_check, Module::project_spec_check) and of the penetration call
// (Batch::config_clearance_check, the margins), the rows dealt to the shards that own their runs as penetration.cpp deals them,
// and per shard one upload, one set-up of the penetration tables (BatchShard::penetration_setup), then max_steps + 1 rounds of
// two launches on the shard's stream -- penetration_kernel as it stands on the iterates, project_clear_step_kernel
// (project_clear_kernels.hip) -- with no synchronisation in between, and one download.  Every ORC_PROJECT_CLEAR_POLL rounds (4
// when the environment does not say) the host reads the count of rows that go on and stops at 0; a finished row is frozen, so
// no answer depends on that interval.  Nothing is kept on the device.
#include "module.h"
#include "penetration_device.h"
#include "project_clear_device.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>

namespace orc {

void Module::batch_project_tsr_clear(int id, const std::vector<TsrSpec> & tsrs, int n_q, const int * tsr_of_q, const int * run_of_q,
   const double * configs, const ProjectClearSpec & ps, const ProjectClearOut & out)
{
   Batch & b = batch(id);
   const std::vector<TsrSpec> specs = project_check("project tsr clear", b, tsrs, n_q, tsr_of_q, configs);
   if (!out.rows || !out.resid || !out.clear || !out.steps || !out.status)
      throw std::runtime_error("project tsr clear: configs_out, resid_out, clearance_out, steps_out and status_out are required!");
   project_spec_check("project tsr clear", b, ps.project);
   b.config_clearance_check(false, n_q, run_of_q, nullptr, configs);
   if (!(ps.margin_field >= 0.0) || !(ps.margin_self >= 0.0) || std::isinf(ps.margin_field) || std::isinf(ps.margin_self))
      throw std::runtime_error("project tsr clear: the margins are finite and not negative!");
   if (!(ps.push_cap > 0.0)) throw std::runtime_error("project tsr clear: push_cap must be a positive number!");
   if (!(ps.slack >= 0.0) || std::isinf(ps.slack)) throw std::runtime_error("project tsr clear: slack must be a finite number >= 0!");
   const VerdictInputs in = verdict_inputs(env.robot(b.robot_name), b, true);
   b.project_tsr_clear(env.robot(b.robot_name), in, specs, n_q, tsr_of_q, run_of_q, configs, ps, out);
}

void Batch::project_tsr_clear(const Robot & robot, const VerdictInputs & in, const std::vector<TsrSpec> & specs, int n_q, const int * tsr_of_q,
   const int * run_of_q, const double * configs, const ProjectClearSpec & ps, const ProjectClearOut & out)
{
   if (shards.size() == 1)      // one shard owns every run
   {
      shards[0]->project_tsr_clear(robot, in, specs, n_q, tsr_of_q, run_of_q, configs, ps, out);
      return;
   }
   for_shards([&](size_t k) {
      const int r0 = offs[k], r1 = offs[k+1];
      // the rows whose run this shard owns, in their order, with the run rebased to the shard
      std::vector<int> at, run, of;
      std::vector<double> rows;
      for (int q=0; q<n_q; q++)
      {
         const int r = run_of_q ? run_of_q[q] : 0;
         if (r < r0 || r >= r1) continue;
         at.push_back(q); run.push_back(r - r0);
         if (tsr_of_q) of.push_back(tsr_of_q[q]);
         rows.insert(rows.end(), configs + (size_t) q*n, configs + (size_t)(q+1)*n);
      }
      if (at.empty()) return;
      const size_t cnt = at.size();
      std::vector<double> row(cnt*n), res(cnt), clr(cnt*2);
      std::vector<int> stp(cnt), sta(cnt);
      ProjectClearOut mine;
      mine.rows = row.data(); mine.resid = res.data(); mine.clear = clr.data(); mine.steps = stp.data(); mine.status = sta.data();
      shards[k]->project_tsr_clear(robot, in, specs, (int) cnt, tsr_of_q ? of.data() : nullptr, run.data(), rows.data(), ps, mine);
      for (size_t i=0; i<cnt; i++)      // (a row belongs to one shard: the shards' threads write disjoint entries)
      {
         const size_t q = (size_t) at[i];
         std::copy(row.begin() + i*n, row.begin() + (i+1)*n, out.rows + q*n);
         out.resid[q] = res[i]; out.clear[q*2] = clr[i*2]; out.clear[q*2 + 1] = clr[i*2 + 1];
         out.steps[q] = stp[i]; out.status[q] = sta[i];
      }
   }, true);
}

// every how many rounds the host looks at the count of rows that go on
static int project_clear_poll()
{
   const char * e = getenv("ORC_PROJECT_CLEAR_POLL");
   const int v = e ? atoi(e) : 4;
   return v >= 1 ? v : 4;
}

template <typename real>
void BatchShard::project_tsr_clear_typed(const Robot & robot, const VerdictInputs & in, const std::vector<TsrSpec> & specs, int n_q,
   const int * tsr_of_q, const int * run_of_q, const double * configs, const ProjectClearSpec & pcs, const ProjectClearOut & out)
{
   hipStream_t st = stream_;
   const ProjectSpec & ps = pcs.project;
   // the constraints on the device's joint order: project.cpp's path
   const JointTree tree = fold_joint_tree(robot, params.floating_base != 0);
   if (tree.nj() != ms_.nj) throw std::runtime_error("project tsr clear: the robot's joint tree is not the one the batch was created with!");
   BatchParams one = params;
   one.tsrs = specs;
   const FoldedTsrs<real> ft = fold_tsrs<real>(robot, one, tree, 1, n);
   int kmax = 3;
   for (const DevTsr<real> & t : ft.tsrs) if (t.k > 3) kmax = 6;
   const int rounds = ps.max_steps + 1;
   const size_t count = (size_t) n_q * n, n2 = (size_t) n_q * 2;

   // ---- one upload: the rows, the constraints, tsr_of_q, run_of_q, the box
   DevProjectClear<real> v;
   std::memset(&v, 0, sizeof(v));
   v.model = d_model_.as<const DevModel<real>>();
   v.n_q = n_q; v.n = n; v.max_steps = ps.max_steps;
   v.stride = orc_project_stride(n, kmax);
   v.tol = (real) ps.tol; v.mu = (real) ps.mu; v.step_cap = (real) ps.step_cap; v.push_cap = (real) pcs.push_cap;
   v.margin_field = pcs.margin_field; v.margin_self = pcs.margin_self;
   DevBuf d_tsrs, d_of, d_run, d_cur, d_start, d_given, d_lo, d_hi, d_ws, d_aws, d_cost, d_grad, d_clr, d_key;
   DevBuf d_done, d_cls, d_val, d_count, d_rows, d_resid, d_clear, d_steps, d_status;
   d_tsrs.reset(dev_alloc<DevTsr<real>>(ft.tsrs.size()));
   hip_check(hipMemcpyAsync(d_tsrs.as<void>(), ft.tsrs.data(), ft.tsrs.size()*sizeof(DevTsr<real>), hipMemcpyHostToDevice, st), "project clear tsrs");
   v.tsrs = d_tsrs.as<const DevTsr<real>>();
   if (tsr_of_q)
   {
      d_of.reset(dev_alloc<int>(n_q));
      hip_check(hipMemcpyAsync(d_of.as<void>(), tsr_of_q, (size_t) n_q*sizeof(int), hipMemcpyHostToDevice, st), "project clear tsr_of_q");
      v.tsr_of_q = d_of.as<int>();
   }
   if (run_of_q)
   {
      d_run.reset(dev_alloc<int>(n_q));
      hip_check(hipMemcpyAsync(d_run.as<void>(), run_of_q, (size_t) n_q*sizeof(int), hipMemcpyHostToDevice, st), "project clear runs");
   }
   std::vector<real> narrowed;      // (a precision-32 batch: narrowed as set_traj narrows; it lives until the copy is done)
   d_cur.reset(dev_alloc<real>(count)); d_start.reset(dev_alloc<real>(count));
   d_given.reset(dev_alloc<double>(count)); d_rows.reset(dev_alloc<double>(count));
   {
      const void * src = configs;
      if (sizeof(real) != sizeof(double)) { narrowed.assign(configs, configs + count); src = narrowed.data(); }
      hip_check(hipMemcpyAsync(d_cur.as<void>(), src, count*sizeof(real), hipMemcpyHostToDevice, st), "project clear rows");
      hip_check(hipMemcpyAsync(d_start.as<void>(), d_cur.as<void>(), count*sizeof(real), hipMemcpyDeviceToDevice, st), "project clear start");
      hip_check(hipMemcpyAsync(d_given.as<void>(), configs, count*sizeof(double), hipMemcpyHostToDevice, st), "project clear given");
      // (the answer of a row that never improves on its input is the input: the caller's own doubles)
      hip_check(hipMemcpyAsync(d_rows.as<void>(), d_given.as<void>(), count*sizeof(double), hipMemcpyDeviceToDevice, st), "project clear rows out");
   }
   v.cur = d_cur.as<real>(); v.start = d_start.as<const real>(); v.given = d_given.as<const double>(); v.rows_out = d_rows.as<double>();
   std::vector<real> lo(n), hi(n);
   for (int c=0; c<n; c++)
   {
      lo[c] = ps.lower ? (real) ps.lower[c] : -std::numeric_limits<real>::infinity();
      hi[c] = ps.upper ? (real) ps.upper[c] : std::numeric_limits<real>::infinity();
      // (precision 32: a limit that rounds outwards is taken one step inwards, so that a clipped row lies inside the caller's box)
      if (ps.lower && (double) lo[c] < ps.lower[c]) lo[c] = std::nextafter(lo[c], std::numeric_limits<real>::infinity());
      if (ps.upper && (double) hi[c] > ps.upper[c]) hi[c] = std::nextafter(hi[c], -std::numeric_limits<real>::infinity());
   }
   d_lo.reset(dev_alloc<real>(n)); d_hi.reset(dev_alloc<real>(n));
   hip_check(hipMemcpyAsync(d_lo.as<void>(), lo.data(), n*sizeof(real), hipMemcpyHostToDevice, st), "project clear lower");
   hip_check(hipMemcpyAsync(d_hi.as<void>(), hi.data(), n*sizeof(real), hipMemcpyHostToDevice, st), "project clear upper");
   v.lower = d_lo.as<const real>(); v.upper = d_hi.as<const real>();
   // a lane's state within a launch: in LDS when a workgroup's states fit, else in a workspace of the call
   if ((size_t) ORC_PROJECT_LANES * v.stride * sizeof(real) > ORC_PROJECT_LDS_BYTES)
   {
      d_ws.reset(dev_alloc<real>((size_t) n_q * v.stride));
      v.ws = d_ws.as<real>();
   }
   d_aws.reset(dev_alloc<real>((size_t) ms_.nj * 6 * n_q));
   v.aws = d_aws.as<real>();

   // ---- one set-up of the penetration tables; the kernel evaluates the iterates where they stand, at the margins + slack
   PenetrationTables pt;
   DevPenetration<real> pv;
   const size_t pen_lds = penetration_setup<real>(in, pt, pv);
   pv.n_q = n_q; pv.run_of_q = run_of_q ? d_run.as<int>() : nullptr; pv.point_of_q = nullptr; pv.configs = d_cur.as<const real>();
   pv.margin_field = (real)(pcs.margin_field + pcs.slack); pv.margin_self = (real)(pcs.margin_self + pcs.slack);
   d_cost.reset(dev_alloc<double>(n2)); d_grad.reset(dev_alloc<double>(count)); d_clr.reset(dev_alloc<double>(n2)); d_key.reset(dev_alloc<unsigned int>(n2));
   hip_check(hipMemsetAsync(d_grad.as<void>(), 0, count*sizeof(double), st), "project clear gradient");      // (a column no joint owns stays zero in every round)
   pv.cost_out = d_cost.as<double>(); pv.grad_out = d_grad.as<double>(); pv.clear_out = d_clr.as<double>(); pv.ckey_out = d_key.as<unsigned int>();
   v.cost = d_cost.as<const double>(); v.grad = d_grad.as<const double>(); v.clear = d_clr.as<const double>();

   // ---- the rows' state between the rounds
   d_done.reset(dev_alloc<int>(n_q)); d_cls.reset(dev_alloc<int>(n_q)); d_val.reset(dev_alloc<real>(n_q)); d_count.reset(dev_alloc<int>(rounds));
   d_resid.reset(dev_alloc<double>(n_q)); d_clear.reset(dev_alloc<double>(n2)); d_steps.reset(dev_alloc<int>(n_q)); d_status.reset(dev_alloc<int>(n_q));
   hip_check(hipMemsetAsync(d_done.as<void>(), 0, (size_t) n_q*sizeof(int), st), "project clear flags");
   hip_check(hipMemsetAsync(d_count.as<void>(), 0, (size_t) rounds*sizeof(int), st), "project clear counts");
   v.done = d_done.as<int>(); v.best_cls = d_cls.as<int>(); v.best_val = d_val.as<real>(); v.count = d_count.as<int>();
   v.resid_out = d_resid.as<double>(); v.clear_out = d_clear.as<double>(); v.steps_out = d_steps.as<int>(); v.status_out = d_status.as<int>();

   // ---- the rounds
   const int poll = project_clear_poll();
   const int is_tree = plan_.variant & ORC_VAR_TREE;
   for (int it=0; it<rounds; it++)
   {
      hip_check(orc_launch_penetration(pv, pen_lds, st, is_tree), "penetration_kernel launch");
      v.it = it;
      hip_check(orc_launch_project_clear_step(v, kmax, st), "project_clear_step_kernel launch");
      if ((it + 1) % poll == 0 && it + 1 < rounds)
      {
         int going = 0;
         hip_check(hipMemcpyAsync(&going, d_count.as<int>() + it, sizeof(int), hipMemcpyDeviceToHost, st), "project clear count");
         hip_check(hipStreamSynchronize(st), "project clear poll");
         if (going == 0) break;
      }
   }
   // ---- one download
   hip_check(hipMemcpyAsync(out.rows, d_rows.as<void>(), count*sizeof(double), hipMemcpyDeviceToHost, st), "project clear rows");
   hip_check(hipMemcpyAsync(out.resid, d_resid.as<void>(), (size_t) n_q*sizeof(double), hipMemcpyDeviceToHost, st), "project clear residuals");
   hip_check(hipMemcpyAsync(out.clear, d_clear.as<void>(), n2*sizeof(double), hipMemcpyDeviceToHost, st), "project clear clearances");
   hip_check(hipMemcpyAsync(out.steps, d_steps.as<void>(), (size_t) n_q*sizeof(int), hipMemcpyDeviceToHost, st), "project clear steps");
   hip_check(hipMemcpyAsync(out.status, d_status.as<void>(), (size_t) n_q*sizeof(int), hipMemcpyDeviceToHost, st), "project clear statuses");
   hip_check(hipStreamSynchronize(st), "project clear sync");
}

void BatchShard::project_tsr_clear(const Robot & robot, const VerdictInputs & in, const std::vector<TsrSpec> & specs, int n_q, const int * tsr_of_q,
   const int * run_of_q, const double * configs, const ProjectClearSpec & ps, const ProjectClearOut & out)
{
   DeviceGuard guard(device);
   if (params.precision == 64) project_tsr_clear_typed<double>(robot, in, specs, n_q, tsr_of_q, run_of_q, configs, ps, out);
   else project_tsr_clear_typed<float>(robot, in, specs, n_q, tsr_of_q, run_of_q, configs, ps, out);
}

} // namespace orc
