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
#include <hip/hip_runtime.h>
#include <math.h>
#include "dev_types.h"
#include "project_device.h"

#pragma clang fp contract(fast)
namespace {

#include "sdf_lookup.h"
#include "fk.h"
#include "tsr_point.h"

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
   real * st = v.ws ? v.ws + (size_t) q * v.stride : (real *) smem_raw + (size_t) threadIdx.x * v.stride;
   real * hs = st, * J = st + KMAX, * cur = J + KMAX*n, * best = cur + n;
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
      real r = 0;      // max |h_i|; a NaN entry makes it NaN
#pragma unroll
      for (int i=0; i<KMAX; i++)
      {
         h[i] = (i < k) ? hs[i] : (real)0;
         const real a = M<real>::fabs_(h[i]);
         r = (a > r || a != a) ? a : r;
      }
      // the visited iterate of smallest r (a NaN is never better, and anything is better than a NaN)
      if (it == 0 || ((r == r) && !(best_r <= r)))
      {
         best_r = r; best_it = it;
         if (it > 0) for (int c=0; c<n; c++) best[c] = cur[c];
      }
      if (r <= tol) { status = ORC_PROJECT_DONE; break; }
      if (it == max_steps) break;
      // A = J J^T + mu I, the lower triangle, every sum in the order of the columns
      real A[KMAX][KMAX];
#pragma unroll
      for (int i=0; i<KMAX; i++)
#pragma unroll
         for (int j=0; j<KMAX; j++) A[i][j] = 0;
      for (int c=0; c<n; c++)
      {
         real jc[KMAX];
#pragma unroll
         for (int i=0; i<KMAX; i++) jc[i] = (i < k) ? J[i*n + c] : (real)0;
#pragma unroll
         for (int i=0; i<KMAX; i++)
#pragma unroll
            for (int j=0; j<=i; j++) A[i][j] += jc[i] * jc[j];
      }
#pragma unroll
      for (int i=0; i<KMAX; i++) A[i][i] = (i < k) ? A[i][i] + mu : (real)1;
      // Cholesky row by row: L L^T = A.  A pivot that is not positive and finite ends the row's projection
      real L[KMAX][KMAX];
      bool ok = true;
#pragma unroll
      for (int i=0; i<KMAX; i++)
#pragma unroll
         for (int j=0; j<=i; j++)
         {
            real s = A[i][j];
#pragma unroll
            for (int p=0; p<j; p++) s -= L[i][p] * L[j][p];
            if (j == i)
            {
               const bool good = (s > (real)0) && (s < M<real>::inf());
               ok = ok && good;
               L[i][i] = M<real>::sqrt_(good ? s : (real)1);
            }
            else L[i][j] = s / L[j][j];
         }
      if (!ok) { status = ORC_PROJECT_STALLED; break; }
      real y[KMAX];
#pragma unroll
      for (int i=0; i<KMAX; i++)      // L z = h
      {
         real s = h[i];
#pragma unroll
         for (int p=0; p<i; p++) s -= L[i][p] * y[p];
         y[i] = s / L[i][i];
      }
#pragma unroll
      for (int i=KMAX-1; i>=0; i--)   // L^T y = z
      {
         real s = y[i];
#pragma unroll
         for (int p=i+1; p<KMAX; p++) s -= L[p][i] * y[p];
         y[i] = s / L[i][i];
      }
      // dq = -J^T y, kept in J's first row (column c of J is read before entry c is written, and J is dead after the step)
      real nn = 0;
      for (int c=0; c<n; c++)
      {
         real d = 0;
#pragma unroll
         for (int i=0; i<KMAX; i++) d += ((i < k) ? J[i*n + c] : (real)0) * y[i];
         d = -d;
         J[c] = d;
         nn += d * d;
      }
      const real len = M<real>::sqrt_(nn);
      const real scale = (len > cap) ? cap / len : (real)1;
      bool moved = false;
      for (int c=0; c<n; c++)
      {
         const real x = cur[c];
         real nx = x + J[c] * scale;
         const real lo = v.lower[c], hi = v.upper[c];
         nx = (nx < lo) ? lo : nx;
         nx = (nx > hi) ? hi : nx;
         moved = moved || (nx != x);
         cur[c] = nx;
      }
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
   if (kmax != 3 && kmax != 6) return hipErrorInvalidValue;
   if (v.n_q < 1 || v.n_q > ORC_PROJECT_MAX_Q || v.n < 1 || v.max_steps > ORC_PROJECT_MAX_STEPS) return hipErrorInvalidValue;
   if (v.stride < orc_project_stride(v.n, kmax)) return hipErrorInvalidValue;
   if (!v.model || !v.tsrs || !v.configs || !v.aws) return hipErrorInvalidValue;
   if (v.max_steps < 0 ? (!v.h_out || !v.jac_out) : (!v.lower || !v.upper || !v.rows_out || !v.resid_out || !v.steps_out || !v.status_out))
      return hipErrorInvalidValue;
   const size_t lds = v.ws ? 0 : (size_t) ORC_PROJECT_LANES * v.stride * sizeof(real);
   if (lds > ORC_PROJECT_LDS_BYTES) return hipErrorInvalidValue;
   const int blocks = (v.n_q + ORC_PROJECT_LANES - 1) / ORC_PROJECT_LANES;
   if (kmax == 3) hipLaunchKernelGGL((project_tsr_kernel<real, 3>), dim3(blocks), dim3(ORC_PROJECT_LANES), lds, stream, v);
   else hipLaunchKernelGGL((project_tsr_kernel<real, 6>), dim3(blocks), dim3(ORC_PROJECT_LANES), lds, stream, v);
   return hipGetLastError();
}
hipError_t orc_launch_project(const DevProject<double> & v, int kmax, hipStream_t stream) { return launch_project_t<double>(v, kmax, stream); }
hipError_t orc_launch_project(const DevProject<float> & v, int kmax, hipStream_t stream) { return launch_project_t<float>(v, kmax, stream); }
