// project_clear.cpp -- host side of the projection onto TSRs and out of contact (orc_batch_project_tsr_clear): the argument
// checks of the projection (Module::project_check, Module::project_spec_check) and of the penetration call
// (Batch::config_clearance_check, margins_check), the rows dealt to the shards that own their runs (Batch::deal_by_run),
// and per shard one upload (QueryUpload), one set-up of the penetration tables (BatchShard::penetration_setup), then max_steps + 1 rounds of
// two launches on the shard's stream -- penetration_kernel as it stands on the iterates, project_clear_step_kernel
// (project_clear_kernels.hip) -- with no synchronisation in between, and one download.  Every ORC_PROJECT_CLEAR_POLL rounds (4
// when the environment does not say) the host reads the count of rows that go on and stops at 0; a finished row is frozen, so
// no answer depends on that interval.  Nothing is kept on the device.
#include "module.h"
#include "penetration_device.h"
#include "project_clear_device.h"
#include "query_upload.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
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
   margins_check("project tsr clear", ps.margin_field, ps.margin_self);
   if (!(ps.push_cap > 0.0)) throw std::runtime_error("project tsr clear: push_cap must be a positive number!");
   if (!(ps.slack >= 0.0) || std::isinf(ps.slack)) throw std::runtime_error("project tsr clear: slack must be a finite number >= 0!");
   const VerdictInputs in = verdict_inputs(env.robot(b.robot_name), b, true);
   b.project_tsr_clear(env.robot(b.robot_name), in, specs, n_q, tsr_of_q, run_of_q, configs, ps, out);
}

void Batch::project_tsr_clear(const Robot & robot, const VerdictInputs & in, const std::vector<TsrSpec> & specs, int n_q, const int * tsr_of_q,
   const int * run_of_q, const double * configs, const ProjectClearSpec & ps, const ProjectClearOut & out)
{
   deal_by_run(n_q, run_of_q, false, { deal_in(tsr_of_q, 1), deal_in(configs, n) },
      { deal_out(out.rows, n), deal_out(out.resid, 1), deal_out(out.clear, 2), deal_out(out.steps, 1), deal_out(out.status, 1) },
      [&](size_t k, int cnt, const int * run, const std::vector<void *> & in_col, const std::vector<void *> & out_col) {
         ProjectClearOut mine;
         mine.rows = (double *) out_col[0]; mine.resid = (double *) out_col[1]; mine.clear = (double *) out_col[2];
         mine.steps = (int *) out_col[3]; mine.status = (int *) out_col[4];
         shards[k]->project_tsr_clear(robot, in, specs, cnt, (const int *) in_col[0], run, (const double *) in_col[1], ps, mine);
      });
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
   const ProjectSpec & ps = pcs.project;
   QueryUpload<real> up(stream_, "project clear");
   hipStream_t st = up.st;
   const int rounds = ps.max_steps + 1;
   const size_t count = (size_t) n_q * n, n2 = (size_t) n_q * 2;

   // ---- one upload: the constraints, tsr_of_q, run_of_q, the rows, the box
   int kmax;
   DevProjectClear<real> v;
   std::memset(&v, 0, sizeof(v));
   v.tsrs = up.constraints("project tsr clear", robot, params, ms_.nj, n, specs, kmax);
   v.model = d_model_.as<const DevModel<real>>();
   v.n_q = n_q; v.n = n; v.max_steps = ps.max_steps;
   v.stride = orc_project_stride(n, kmax);
   v.tol = (real) ps.tol; v.mu = (real) ps.mu; v.step_cap = (real) ps.step_cap; v.push_cap = (real) pcs.push_cap;
   v.margin_field = pcs.margin_field; v.margin_self = pcs.margin_self;
   v.tsr_of_q = up.ints(tsr_of_q, n_q, "tsr_of_q");
   const int * d_run = up.ints(run_of_q, n_q, "runs");
   v.cur = up.rows(configs, count);
   real * d_start = up.template alloc<real>(count);
   double * d_given = up.template alloc<double>(count);
   v.rows_out = up.template alloc<double>(count);
   up.check(hipMemcpyAsync(d_start, v.cur, count*sizeof(real), hipMemcpyDeviceToDevice, st), "start");
   up.up(d_given, configs, count*sizeof(double), "given");
   // (the answer of a row that never improves on its input is the input: the caller's own doubles)
   up.check(hipMemcpyAsync(v.rows_out, d_given, count*sizeof(double), hipMemcpyDeviceToDevice, st), "rows out");
   v.start = d_start; v.given = d_given;
   up.box(ps.lower, ps.upper, n, v.lower, v.upper);
   v.ws = up.lane_state(n_q, n, kmax);
   v.aws = up.template alloc<real>((size_t) ms_.nj * 6 * n_q);

   // ---- one set-up of the penetration tables; the kernel evaluates the iterates where they stand, at the margins + slack
   PenetrationTables pt;
   DevPenetration<real> pv;
   const size_t pen_lds = penetration_setup<real>(in, pt, pv);
   pv.n_q = n_q; pv.run_of_q = d_run; pv.point_of_q = nullptr; pv.configs = v.cur;
   pv.margin_field = (real)(pcs.margin_field + pcs.slack); pv.margin_self = (real)(pcs.margin_self + pcs.slack);
   pv.cost_out = up.template alloc<double>(n2); pv.grad_out = up.template alloc<double>(count);
   pv.clear_out = up.template alloc<double>(n2); pv.ckey_out = up.template alloc<unsigned int>(n2);
   up.zero(pv.grad_out, count*sizeof(double), "gradient");      // (a column no joint owns stays zero in every round)
   v.cost = pv.cost_out; v.grad = pv.grad_out; v.clear = pv.clear_out;

   // ---- the rows' state between the rounds
   v.done = up.template alloc<int>(n_q); v.best_cls = up.template alloc<int>(n_q); v.best_val = up.template alloc<real>(n_q);
   v.count = up.template alloc<int>(rounds);
   v.resid_out = up.template alloc<double>(n_q); v.clear_out = up.template alloc<double>(n2);
   v.steps_out = up.template alloc<int>(n_q); v.status_out = up.template alloc<int>(n_q);
   up.zero(v.done, (size_t) n_q*sizeof(int), "flags");
   up.zero(v.count, (size_t) rounds*sizeof(int), "counts");

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
         up.down(&going, v.count + it, sizeof(int), "count");
         up.sync("poll");
         if (going == 0) break;
      }
   }
   // ---- one download
   up.down(out.rows, v.rows_out, count*sizeof(double), "rows");
   up.down(out.resid, v.resid_out, (size_t) n_q*sizeof(double), "residuals");
   up.down(out.clear, v.clear_out, n2*sizeof(double), "clearances");
   up.down(out.steps, v.steps_out, (size_t) n_q*sizeof(int), "steps");
   up.down(out.status, v.status_out, (size_t) n_q*sizeof(int), "statuses");
   up.sync();
}

void BatchShard::project_tsr_clear(const Robot & robot, const VerdictInputs & in, const std::vector<TsrSpec> & specs, int n_q, const int * tsr_of_q,
   const int * run_of_q, const double * configs, const ProjectClearSpec & ps, const ProjectClearOut & out)
{
   DeviceGuard guard(device);
   if (params.precision == 64) project_tsr_clear_typed<double>(robot, in, specs, n_q, tsr_of_q, run_of_q, configs, ps, out);
   else project_tsr_clear_typed<float>(robot, in, specs, n_q, tsr_of_q, run_of_q, configs, ps, out);
}

} // namespace orc
