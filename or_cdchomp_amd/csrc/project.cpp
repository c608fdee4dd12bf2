// project.cpp -- host side of the TSR calls on single configurations (orc_batch_config_tsr, orc_batch_project_tsr): the checks of
// their arguments, the constraints folded with the batch's robot and joint tree through fold_tsrs (one constraint on one point
// each), the queries dealt to the shards in even contiguous slices (a row names no run: any split does), the launches of
// project_kernels.hip.  The model is the one `create` put on the device; nothing is kept there after the call.
#include "module.h"
#include "project_device.h"
#include "query_upload.h"
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace orc {

ProjectOut ProjectOut::from(size_t first, int n) const
{
   ProjectOut o;
   o.h = h ? h + 6*first : nullptr; o.jac = jac ? jac + (size_t) 6*n*first : nullptr;
   o.rows = rows ? rows + (size_t) n*first : nullptr; o.resid = resid ? resid + first : nullptr;
   o.steps = steps ? steps + first : nullptr; o.status = status ? status + first : nullptr;
   return o;
}

// what both calls reject, before any device work; returns the constraints with `ee_link -1` resolved to the active manipulator
std::vector<TsrSpec> Module::project_check(const char * who, const Batch & b, const std::vector<TsrSpec> & tsrs, int n_q, const int * tsr_of_q,
   const double * configs) const
{
   const std::string w = std::string(who) + ": ";
   const int n_tsr = (int) tsrs.size();
   if (n_tsr < 1) throw std::runtime_error(w + "n_tsr must be >= 1!");
   if (n_q < 1 || n_q > ORC_PROJECT_MAX_Q) throw std::runtime_error(w + "n_q must lie in [1, 4194304]!");
   if (!configs) throw std::runtime_error(w + "configs [n_q][n] is NULL!");
   for (int q=0; tsr_of_q && q<n_q; q++)
      if (tsr_of_q[q] < 0 || tsr_of_q[q] >= n_tsr) throw std::runtime_error(w + "a tsr_of_q entry lies outside [0, n_tsr)!");
   const Robot & robot = env.robot(b.robot_name);
   if (robot.active_dofs != b.adofindices) throw std::runtime_error(w + "the robot's active dofs are not those the batch was created with!");
   std::vector<TsrSpec> out = tsrs;
   for (TsrSpec & t : out)
   {
      if (t.ee_link == -1)
      {
         if (robot.manips.empty()) throw std::runtime_error(w + "ee_link -1 names the active manipulator, and the robot has none!");
         t.ee_link = robot.manips[robot.active_manip].link; t.tool = robot.manips[robot.active_manip].tool;
      }
      if (t.ee_link < 0 || t.ee_link >= robot.n_links) throw std::runtime_error(w + "ee_link lies outside the robot's links!");
      int k = 0;
      for (int r=0; r<6; r++) k += (t.Bw[r][0] == 0.0 && t.Bw[r][1] == 0.0) ? 1 : 0;
      if (k == 0) throw std::runtime_error(w + "a TSR enforces no row (every Bw row has a range)!");
      for (int e=0; e<7; e++)
         if (!std::isfinite(t.tool.v[e]) || !std::isfinite(t.T0w.v[e]) || !std::isfinite(t.Twe.v[e])) throw std::runtime_error(w + "a TSR's poses must be finite numbers!");
      t.point = 0;      // (fold_tsrs: one constraint on one point)
   }
   return out;
}

// what the projections reject of their parameters (orc_batch_project_tsr, orc_batch_project_tsr_clear), before any device work
void Module::project_spec_check(const char * who, const Batch & b, const ProjectSpec & ps) const
{
   const std::string w = std::string(who) + ": ";
   if (!(ps.tol > 0.0)) throw std::runtime_error(w + "tol must be a positive number!");
   if (!(ps.step_cap > 0.0)) throw std::runtime_error(w + "step_cap must be a positive number!");
   if (!(ps.mu >= 0.0)) throw std::runtime_error(w + "mu must be a number >= 0!");
   if (ps.max_steps < 0 || ps.max_steps > ORC_PROJECT_MAX_STEPS) throw std::runtime_error(w + "max_steps must lie in [0, 256]!");
   for (int c=0; c<b.n; c++)
   {
      const double lo = ps.lower ? ps.lower[c] : -HUGE_VAL, hi = ps.upper ? ps.upper[c] : HUGE_VAL;
      if (std::isnan(lo) || std::isnan(hi) || lo > hi) throw std::runtime_error(w + "lower[c] <= upper[c] must hold for every column!");
   }
   if (b.params.floating_base) throw std::runtime_error(w + "a floating-base batch is not projected (its quaternion columns have no update rule here)!");
}

void Module::batch_config_tsr(int id, const std::vector<TsrSpec> & tsrs, int n_q, const int * tsr_of_q, const double * configs,
   double * h_out, double * jac_out)
{
   Batch & b = batch(id);
   const std::vector<TsrSpec> specs = project_check("config tsr", b, tsrs, n_q, tsr_of_q, configs);
   if (!h_out) throw std::runtime_error("config tsr: h_out [n_q][6] is NULL!");
   ProjectOut out;
   out.h = h_out; out.jac = jac_out;
   b.project_tsr(env.robot(b.robot_name), specs, n_q, tsr_of_q, configs, nullptr, out);
}

void Module::batch_project_tsr(int id, const std::vector<TsrSpec> & tsrs, int n_q, const int * tsr_of_q, const double * configs,
   const ProjectSpec & ps, double * rows_out, double * resid_out, int * steps_out, int * status_out)
{
   Batch & b = batch(id);
   const std::vector<TsrSpec> specs = project_check("project tsr", b, tsrs, n_q, tsr_of_q, configs);
   if (!rows_out || !resid_out || !steps_out || !status_out) throw std::runtime_error("project tsr: configs_out, resid_out, steps_out and status_out are required!");
   project_spec_check("project tsr", b, ps);
   ProjectOut out;
   out.rows = rows_out; out.resid = resid_out; out.steps = steps_out; out.status = status_out;
   b.project_tsr(env.robot(b.robot_name), specs, n_q, tsr_of_q, configs, &ps, out);
}

void Batch::project_tsr(const Robot & robot, const std::vector<TsrSpec> & specs, int n_q, const int * tsr_of_q, const double * configs,
   const ProjectSpec * ps, const ProjectOut & out)
{
   // shard k takes the queries [n_q k / S, n_q (k + 1) / S): slices of the caller's arrays, nothing is gathered
   const size_t S = shards.size();
   for_shards([&](size_t k) {
      const size_t q0 = (size_t) n_q * k / S, q1 = (size_t) n_q * (k + 1) / S;
      if (q1 == q0) return;
      shards[k]->project_tsr(robot, specs, (int)(q1 - q0), tsr_of_q ? tsr_of_q + q0 : nullptr, configs + q0 * n, ps, out.from(q0, n));
   }, true);
}

template <typename real>
void BatchShard::project_tsr_typed(const Robot & robot, const std::vector<TsrSpec> & specs, int n_q, const int * tsr_of_q, const double * configs,
   const ProjectSpec * ps, const ProjectOut & out)
{
   QueryUpload<real> up(stream_, "project");
   int kmax;
   DevProject<real> v;
   std::memset(&v, 0, sizeof(v));
   v.tsrs = up.constraints("project tsr", robot, params, ms_.nj, n, specs, kmax);
   v.model = d_model_.as<const DevModel<real>>();
   v.n_q = n_q; v.n = n; v.max_steps = ps ? ps->max_steps : -1;
   v.stride = orc_project_stride(n, kmax);
   v.tsr_of_q = up.ints(tsr_of_q, n_q, "tsr_of_q");
   const size_t count = (size_t) n_q * n;
   v.configs = up.rows(configs, count);
   v.ws = up.lane_state(n_q, n, kmax);
   v.aws = up.template alloc<real>((size_t) ms_.nj * 6 * n_q);
   if (ps)
   {
      v.tol = (real) ps->tol; v.mu = (real) ps->mu; v.step_cap = (real) ps->step_cap;
      up.box(ps->lower, ps->upper, n, v.lower, v.upper);
      v.rows_out = up.template alloc<double>(count); v.resid_out = up.template alloc<double>(n_q);
      v.steps_out = up.template alloc<int>(n_q); v.status_out = up.template alloc<int>(n_q);
      // (the answer of a row that never improves on its input is the input: the caller's own doubles)
      up.up(v.rows_out, configs, count*sizeof(double), "rows out");
   }
   else
   {
      v.h_out = up.template alloc<double>((size_t) n_q * 6); v.jac_out = up.template alloc<double>(count * 6);
      hip_check(hipMemsetAsync(v.h_out, 0, (size_t) n_q*6*sizeof(double), up.st), "config tsr h");
      hip_check(hipMemsetAsync(v.jac_out, 0, count*6*sizeof(double), up.st), "config tsr jac");
   }
   hip_check(orc_launch_project(v, kmax, up.st), "project_tsr_kernel launch");
   if (out.h) hip_check(hipMemcpyAsync(out.h, v.h_out, (size_t) n_q*6*sizeof(double), hipMemcpyDeviceToHost, up.st), "config tsr h");
   if (out.jac) hip_check(hipMemcpyAsync(out.jac, v.jac_out, count*6*sizeof(double), hipMemcpyDeviceToHost, up.st), "config tsr jac");
   up.down(out.rows, v.rows_out, count*sizeof(double), "rows");
   up.down(out.resid, v.resid_out, (size_t) n_q*sizeof(double), "residuals");
   up.down(out.steps, v.steps_out, (size_t) n_q*sizeof(int), "steps");
   up.down(out.status, v.status_out, (size_t) n_q*sizeof(int), "statuses");
   up.sync();
}

void BatchShard::project_tsr(const Robot & robot, const std::vector<TsrSpec> & specs, int n_q, const int * tsr_of_q, const double * configs,
   const ProjectSpec * ps, const ProjectOut & out)
{
   DeviceGuard guard(device);
   if (params.precision == 64) project_tsr_typed<double>(robot, specs, n_q, tsr_of_q, configs, ps, out);
   else project_tsr_typed<float>(robot, specs, n_q, tsr_of_q, configs, ps, out);
}

// where a lane's state lives for this batch's model and `kmax` enforced rows: 1 in LDS, 0 in the call's workspace
int BatchShard::project_state_in_lds(int kmax) const
{
   return project_state_fits_lds(n, kmax, params.precision == 64 ? sizeof(double) : sizeof(float)) ? 1 : 0;
}

} // namespace orc
