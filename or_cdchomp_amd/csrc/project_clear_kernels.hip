// project_clear_kernels.hip -- one round of the projection of configurations onto TSRs and out of contact
// (orc_batch_project_tsr_clear): project_tsr_kernel's sibling.  The rule is or_cdchomp_amd/project_clear.py.
//
// A launch is one round for every row that is still active, after penetration_kernel has written the cost, the gradient and
// the clearance of the rows' iterates.  One lane = one row: the lane evaluates h and J at its iterate (tsr_eval_point), forms
// the iterate's key and keeps the better one, and, unless the row is finished, takes the step: the k x k system
// A = J J^T + mu I in registers (k <= 6, every index known at compile time), factored once by Cholesky and solved twice, for the
// task step -J^T A^-1 h and for the push -(2U / s) g_N with g_N = g - J^T A^-1 (J g).  There is no barrier and no exchange between
// lanes; what a row carries from round to round is in global memory (project_clear_device.h), so a row's answer is its lane's
// alone: nothing of it depends on its place in the list, on what shares its wavefront, on the shard, or on how often the host
// looks at the count.
//
// Within a launch a lane's state -- h, J [KMAX][n], the iterate, the gradient -- is indexed by loop counters and lives in
// memory, not in registers: in LDS when a workgroup's 64 states fit ORC_PROJECT_LDS_BYTES, else in the call's workspace, as the
// sibling's.  The residual, the factor, the solve and the clipped move are the sibling's text (project_step.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include "dev_types.h"
#include "project_clear_device.h"

#pragma clang fp contract(fast)
namespace {

#include "sdf_lookup.h"
#include "fk.h"
#include "tsr_point.h"
#include "project_step.h"

template <typename real>
__device__ __forceinline__ bool clear_finite(real x) { return M<real>::fabs_(x) < M<real>::inf(); }

template <typename real, int KMAX>
__global__ __launch_bounds__(ORC_PROJECT_LANES)
void project_clear_step_kernel(DevProjectClear<real> v)
{
   extern __shared__ __align__(16) unsigned char smem_raw[];
   const int q = blockIdx.x * ORC_PROJECT_LANES + threadIdx.x;
   if (q >= v.n_q) return;      // (a lane without a row idles: nothing below waits for it)
   if (v.done[q]) return;       // (a frozen row)
   const DevModel<real> & gm = *v.model;
   const int n = v.n, it = v.it;
   const ProjectLane<real> S = project_lane<real, KMAX>(v.ws, smem_raw, q, v.stride, n);
   real * hs = S.hs, * J = S.J, * cur = S.cur, * g = S.own;
   const DevTsr<real> & ts = v.tsrs[v.tsr_of_q ? v.tsr_of_q[q] : 0];
   const int k = ts.k;          // (1 .. KMAX: the host chose KMAX by the call's constraints)
   const double nan = __longlong_as_double(0x7ff8000000000000LL);

   bool bad = false;
   for (int c=0; c<n; c++)
   {
      const real x = v.cur[(size_t) q*n + c];
      cur[c] = x;
      bad = bad || !clear_finite<real>(x);
   }
   if (it == 0)
   {
      v.steps_out[q] = 0;
      if (bad)      // a row with a non-finite entry is not evaluated
      {
         for (int c=0; c<n; c++) v.rows_out[(size_t) q*n + c] = nan;
         v.resid_out[q] = nan; v.clear_out[(size_t) q*2] = nan; v.clear_out[(size_t) q*2 + 1] = nan;
         v.status_out[q] = ORC_PROJECT_NOT_FINITE;
         v.done[q] = 1;
         return;
      }
      v.status_out[q] = ORC_PROJECT_OUT_OF_STEPS;
   }
   // ---- the iterate's key
   tsr_eval_point<real>(gm, ts, cur, n, hs, J, v.aws, v.n_q, q);
   real h[KMAX];
   const real r = project_residual<real, KMAX>(hs, k, h);
   const real U = (real) v.cost[(size_t) q*2] + (real) v.cost[(size_t) q*2 + 1];
   const double clr0 = v.clear[(size_t) q*2], clr1 = v.clear[(size_t) q*2 + 1];
   const bool on = r <= v.tol;
   const bool clear = (clr0 >= v.margin_field) && (clr1 >= v.margin_self);      // (a NaN is never clear)
   const int cls = (on && clear) ? ORC_CLEAR_ON_AND_CLEAR : (on ? ORC_CLEAR_ON : ORC_CLEAR_OFF);
   const real val = (cls == ORC_CLEAR_ON_AND_CLEAR) ? (real)0 : ((cls == ORC_CLEAR_ON) ? U : r);
   // the lower class wins; within a class the smaller value, a NaN is never better and anything beats a NaN; a tie stays
   bool better = (it == 0);
   if (!better)
   {
      const int bc = v.best_cls[q];
      const real bv = v.best_val[q];
      better = (cls < bc) || (cls == bc && (val == val) && !(bv <= val));
   }
   if (better)
   {
      v.best_cls[q] = cls; v.best_val[q] = val;
      v.resid_out[q] = (double) r; v.clear_out[(size_t) q*2] = clr0; v.clear_out[(size_t) q*2 + 1] = clr1;
      // an entry the loop left where it was is the caller's own double (in a precision-32 batch its double is not the float's)
      if (it > 0)
         for (int c=0; c<n; c++)
            v.rows_out[(size_t) q*n + c] = (cur[c] == v.start[(size_t) q*n + c]) ? v.given[(size_t) q*n + c] : (double) cur[c];
   }
   if (cls == ORC_CLEAR_ON_AND_CLEAR) { v.status_out[q] = ORC_PROJECT_DONE; v.done[q] = 1; return; }
   if (it == v.max_steps) { v.done[q] = 1; return; }
   // ---- the step: A = J J^T + mu I, factored once and solved twice
   real L[KMAX][KMAX], y[KMAX];
   if (!project_factor<real, KMAX>(J, n, k, v.mu, L)) { v.status_out[q] = ORC_PROJECT_STALLED; v.done[q] = 1; return; }
   project_solve<real, KMAX>(L, h, y);
   // the push, in the null space of J: only from a cost that is finite and positive and a gradient that is finite
   bool push = clear_finite<real>(U) && (U > (real)0);
   for (int c=0; c<n; c++)
   {
      const real x = (real) v.grad[(size_t) q*n + c];
      g[c] = x;
      push = push && clear_finite<real>(x);
   }
   real pscale = 0;
   if (push)
   {
      real w[KMAX], z[KMAX];
#pragma unroll
      for (int i=0; i<KMAX; i++) w[i] = 0;
      for (int c=0; c<n; c++)
      {
         const real gc = g[c];
#pragma unroll
         for (int i=0; i<KMAX; i++) w[i] += ((i < k) ? J[i*n + c] : (real)0) * gc;
      }
      project_solve<real, KMAX>(L, w, z);
      real s = 0;
      for (int c=0; c<n; c++)
      {
         real t = 0;
#pragma unroll
         for (int i=0; i<KMAX; i++) t += ((i < k) ? J[i*n + c] : (real)0) * z[i];
         const real gn = g[c] - t;
         g[c] = gn;
         s += gn * gn;
      }
      push = clear_finite<real>(s) && (s > (real)0);
      if (push)
      {
         const real coef = ((real)2 * U) / s;
         real pp = 0;
         for (int c=0; c<n; c++)
         {
            const real p = -(coef * g[c]);
            g[c] = p;
            pp += p * p;
         }
         const real plen = M<real>::sqrt_(pp);
         pscale = (plen > v.push_cap) ? v.push_cap / plen : (real)1;
      }
   }
   const bool moved = project_move<real, KMAX>(J, cur, n, k, y, push ? g : nullptr, pscale, v.step_cap, v.lower, v.upper);
   if (!moved) { v.status_out[q] = ORC_PROJECT_STALLED; v.done[q] = 1; return; }
   for (int c=0; c<n; c++) v.cur[(size_t) q*n + c] = cur[c];
   v.steps_out[q] += 1;
   atomicAdd(v.count + it, 1);      // (an integer sum: the order of the lanes does not show in it)
}

} // namespace

template <typename real>
static hipError_t launch_project_clear_t(const DevProjectClear<real> & v, int kmax, hipStream_t stream)
{
   if (v.max_steps < 0 || v.it < 0 || v.it > v.max_steps) return hipErrorInvalidValue;
   if (!v.cur || !v.start || !v.given || !v.lower || !v.upper || !v.cost || !v.grad || !v.clear) return hipErrorInvalidValue;
   if (!v.done || !v.best_cls || !v.best_val || !v.count || !v.rows_out || !v.resid_out || !v.clear_out || !v.steps_out || !v.status_out)
      return hipErrorInvalidValue;
   return launch_project_kernels<DevProjectClear<real>, project_clear_step_kernel<real, 3>, project_clear_step_kernel<real, 6>>(v, kmax, stream);
}
hipError_t orc_launch_project_clear_step(const DevProjectClear<double> & v, int kmax, hipStream_t stream) { return launch_project_clear_t<double>(v, kmax, stream); }
hipError_t orc_launch_project_clear_step(const DevProjectClear<float> & v, int kmax, hipStream_t stream) { return launch_project_clear_t<float>(v, kmax, stream); }
