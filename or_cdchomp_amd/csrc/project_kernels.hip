// project_kernels.hip -- the value and Jacobian of TSRs at given configurations (orc_batch_config_tsr) and the projection of
// configurations onto TSRs (orc_batch_project_tsr): tsr_eval_point (tsr_point.h), the function the iterate kernel's constraint
// step evaluates a trajectory row with, in a loop of its own.
//
// One lane = one query, from the row to the answer: the lane evaluates h and J at its iterate, forms the k x k system
// (J J^T + mu I) y = h in registers (k <= 6, every index known at compile time), solves it by Cholesky, steps by -J^T y, and
// goes round until |h| is within the tolerance, the step fails or the steps run out.  Lanes take different numbers of rounds;
// there is no barrier and no exchange between lanes, so a query's answer is its lane's alone: nothing of it depends on its
// place in the list, on what shares its wavefront, or on the shard.  The rule is or_cdchomp_amd/project.py.
//
// A lane's state -- h, J [KMAX][n], the current row, the best row -- is indexed by loop counters and lives in memory, not in
// registers: in LDS when a workgroup's 64 states fit ORC_PROJECT_LDS_BYTES, else in the call's workspace (DevProject::ws).
// tsr_eval_point reaches both through generic pointers; its own workspace of joint axes (aws) is global memory by its text.
// The step -- residual, factor, solve, clipped move -- is project_step.h, which project_clear_kernels.hip shares.
#include <hip/hip_runtime.h>
#include <math.h>
#include "dev_types.h"
#include "project_device.h"

#pragma clang fp contract(fast)
namespace {

#include "sdf_lookup.h"
#include "fk.h"
#include "tsr_point.h"
#include "project_step.h"

template <typename real>
__device__ __forceinline__ double project_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// KMAX: the most rows a lane's constraint enforces (3 or 6, tsr_eval_point's own two shapes); a lane with k < KMAX rows
// carries the others as the identity: A[i][i] = 1, h[i] = 0, which leaves y[i] = 0 exactly and the k x k part untouched
template <typename real, int KMAX>
__global__ __launch_bounds__(ORC_PROJECT_LANES)
void project_tsr_kernel(DevProject<real> v)
{
   extern __shared__ __align__(16) unsigned char smem_raw[];
   const int q = blockIdx.x * ORC_PROJECT_LANES + threadIdx.x;
   if (q >= v.n_q) return;      // (a lane without a query idles: nothing below waits for it)
   const DevModel<real> & gm = *v.model;
   const int n = v.n;
   const ProjectLane<real> S = project_lane<real, KMAX>(v.ws, smem_raw, q, v.stride, n);
   real * hs = S.hs, * J = S.J, * cur = S.cur, * best = S.own;
   const DevTsr<real> & ts = v.tsrs[v.tsr_of_q ? v.tsr_of_q[q] : 0];
   const int k = ts.k;          // (1 .. KMAX: the host chose KMAX by the call's constraints)
   const bool evaluate_only = v.max_steps < 0;

   bool bad = false;
   for (int c=0; c<n; c++)
   {
      const real x = v.configs[(size_t) q*n + c];
      cur[c] = x; best[c] = x;
      bad = bad || !(M<real>::fabs_(x) < M<real>::inf());
   }
   if (bad)      // a row with a non-finite entry is not evaluated
   {
      const double nan = project_nan<real>();
      if (evaluate_only)
      {
         for (int i=0; i<k; i++) v.h_out[(size_t) q*6 + i] = nan;
         for (int e=0; e<k*n; e++) v.jac_out[(size_t) q*6*n + e] = nan;
         return;
      }
      for (int c=0; c<n; c++) v.rows_out[(size_t) q*n + c] = nan;
      v.resid_out[q] = nan; v.steps_out[q] = 0; v.status_out[q] = ORC_PROJECT_NOT_FINITE;
      return;
   }
   if (evaluate_only)
   {
      tsr_eval_point<real>(gm, ts, cur, n, hs, J, v.aws, v.n_q, q);
      for (int i=0; i<k; i++) v.h_out[(size_t) q*6 + i] = (double) hs[i];
      for (int e=0; e<k*n; e++) v.jac_out[(size_t) q*6*n + e] = (double) J[e];      // (rows of n entries in both)
      return;
   }

   const real tol = v.tol, mu = v.mu, cap = v.step_cap;
   const int max_steps = v.max_steps;
   int steps = 0, status = ORC_PROJECT_OUT_OF_STEPS, best_it = 0;
   real best_r = 0;
   for (int it=0; ; it++)
   {
      tsr_eval_point<real>(gm, ts, cur, n, hs, J, v.aws, v.n_q, q);
      real h[KMAX];
      const real r = project_residual<real, KMAX>(hs, k, h);
      // the visited iterate of smallest r (a NaN is never better, and anything is better than a NaN)
      if (it == 0 || ((r == r) && !(best_r <= r)))
      {
         best_r = r; best_it = it;
         if (it > 0) for (int c=0; c<n; c++) best[c] = cur[c];
      }
      if (r <= tol) { status = ORC_PROJECT_DONE; break; }
      if (it == max_steps) break;
      real L[KMAX][KMAX], y[KMAX];
      if (!project_factor<real, KMAX>(J, n, k, mu, L)) { status = ORC_PROJECT_STALLED; break; }
      project_solve<real, KMAX>(L, h, y);
      const bool moved = project_move<real, KMAX>(J, cur, n, k, y, nullptr, (real)0, cap, v.lower, v.upper);
      if (!moved) { status = ORC_PROJECT_STALLED; break; }
      steps++;
   }
   // A row whose best iterate is the input itself keeps what the caller put there, the input's own bits; and so does an entry
   // the projection left where it was (a dof that does not move the link: in a precision-32 batch its double is not the float's)
   if (best_it > 0)
      for (int c=0; c<n; c++)
         if (best[c] != v.configs[(size_t) q*n + c]) v.rows_out[(size_t) q*n + c] = (double) best[c];
   v.resid_out[q] = (double) best_r; v.steps_out[q] = steps; v.status_out[q] = status;
}

} // namespace

template <typename real>
static hipError_t launch_project_t(const DevProject<real> & v, int kmax, hipStream_t stream)
{
   if (!v.configs) return hipErrorInvalidValue;
   if (v.max_steps < 0 ? (!v.h_out || !v.jac_out) : (!v.lower || !v.upper || !v.rows_out || !v.resid_out || !v.steps_out || !v.status_out))
      return hipErrorInvalidValue;
   return launch_project_kernels<DevProject<real>, project_tsr_kernel<real, 3>, project_tsr_kernel<real, 6>>(v, kmax, stream);
}
hipError_t orc_launch_project(const DevProject<double> & v, int kmax, hipStream_t stream) { return launch_project_t<double>(v, kmax, stream); }
hipError_t orc_launch_project(const DevProject<float> & v, int kmax, hipStream_t stream) { return launch_project_t<float>(v, kmax, stream); }
