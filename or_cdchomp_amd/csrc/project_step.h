// project_step.h -- the step of the projection onto a TSR that project_tsr_kernel (project_kernels.hip) and
// project_clear_step_kernel (project_clear_kernels.hip) take: one lane = one row, the k x k system A = J J^T + mu I in registers
// (k <= KMAX, every index known at compile time), factored by Cholesky, solved, and the clipped move.  The rules are
// or_cdchomp_amd/project.py and or_cdchomp_amd/project_clear.py.
//
// Included inside the including file's namespace after tsr_point.h, with its contraction in force.  Where no iterate of the
// clear projection is pushed, its rows are the projection's bit for bit because this text is compiled into both kernels: every
// sum has the order of the columns, and a lane with k < KMAX rows carries the others as the identity (A[i][i] = 1, h[i] = 0),
// which leaves y[i] = 0 exactly and the k x k part untouched.
#pragma once

// A lane's state is indexed by loop counters and lives in memory, not in registers: `stride` reals at ws + q stride, or in
// LDS at lane x stride when ws is NULL (project_device.h).  h [KMAX], J [KMAX][n], the iterate [n], then n reals of the kernel's own
template <typename real>
struct ProjectLane
{
   real * hs, * J, * cur, * own;
};

template <typename real, int KMAX>
__device__ __forceinline__ ProjectLane<real> project_lane(real * ws, unsigned char * smem_raw, int q, int stride, int n)
{
   real * st = ws ? ws + (size_t) q * stride : (real *) smem_raw + (size_t) threadIdx.x * stride;
   ProjectLane<real> s;
   s.hs = st; s.J = st + KMAX; s.cur = s.J + KMAX*n; s.own = s.cur + n;
   return s;
}

// h: the k enforced rows of hs, zero behind them.  Returns max |h_i|; a NaN entry makes it NaN
template <typename real, int KMAX>
__device__ __forceinline__ real project_residual(const real * hs, int k, real (&h)[KMAX])
{
   real r = 0;
#pragma unroll
   for (int i=0; i<KMAX; i++)
   {
      h[i] = (i < k) ? hs[i] : (real)0;
      const real a = M<real>::fabs_(h[i]);
      r = (a > r || a != a) ? a : r;
   }
   return r;
}

// L L^T = J J^T + mu I, the lower triangle (nothing above the diagonal is written or read).  False: a pivot is not positive
// and finite, which ends the row's projection
template <typename real, int KMAX>
__device__ __forceinline__ bool project_factor(const real * J, int n, int k, real mu, real (&L)[KMAX][KMAX])
{
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
   // Cholesky row by row
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
   return ok;
}

// y = (L L^T)^-1 b: L z = b by rows ascending, L^T y = z by rows descending
template <typename real, int KMAX>
__device__ __forceinline__ void project_solve(const real (&L)[KMAX][KMAX], const real (&b)[KMAX], real (&y)[KMAX])
{
#pragma unroll
   for (int i=0; i<KMAX; i++)
   {
      real s = b[i];
#pragma unroll
      for (int p=0; p<i; p++) s -= L[i][p] * y[p];
      y[i] = s / L[i][i];
   }
#pragma unroll
   for (int i=KMAX-1; i>=0; i--)
   {
      real s = y[i];
#pragma unroll
      for (int p=i+1; p<KMAX; p++) s -= L[p][i] * y[p];
      y[i] = s / L[i][i];
   }
}

// The move: dq = -J^T y, plus pscale x push where `push` is not NULL, capped at length `cap`, and the iterate clipped to the box.
// dq is kept in J's first row (column c of J is read before entry c is written, and J is dead after the step).  False: no
// entry of the iterate moved
template <typename real, int KMAX>
__device__ __forceinline__ bool project_move(real * J, real * cur, int n, int k, const real (&y)[KMAX], const real * push, real pscale, real cap,
   const real * lower, const real * upper)
{
   real nn = 0;
   for (int c=0; c<n; c++)
   {
      real d = 0;
#pragma unroll
      for (int i=0; i<KMAX; i++) d += ((i < k) ? J[i*n + c] : (real)0) * y[i];
      d = -d;
      if (push) d += push[c] * pscale;
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
      const real lo = lower[c], hi = upper[c];
      nx = (nx < lo) ? lo : nx;
      nx = (nx > hi) ? hi : nx;
      moved = moved || (nx != x);
      cur[c] = nx;
   }
   return moved;
}

// What both launchers check of their arguments, and the launch of the instantiation for kmax (3 when no constraint of the call
// enforces more rows, else 6): host code
template <typename Args, void (*K3)(Args), void (*K6)(Args)>
static hipError_t launch_project_kernels(const Args & v, int kmax, hipStream_t stream)
{
   if (kmax != 3 && kmax != 6) return hipErrorInvalidValue;
   if (v.n_q < 1 || v.n_q > ORC_PROJECT_MAX_Q || v.n < 1 || v.max_steps > ORC_PROJECT_MAX_STEPS) return hipErrorInvalidValue;
   if (v.stride < orc_project_stride(v.n, kmax)) return hipErrorInvalidValue;
   if (!v.model || !v.tsrs || !v.aws) return hipErrorInvalidValue;
   const size_t lds = v.ws ? 0 : (size_t) ORC_PROJECT_LANES * v.stride * sizeof(*v.aws);
   if (lds > ORC_PROJECT_LDS_BYTES) return hipErrorInvalidValue;
   const int blocks = (v.n_q + ORC_PROJECT_LANES - 1) / ORC_PROJECT_LANES;
   if (kmax == 3) hipLaunchKernelGGL(K3, dim3(blocks), dim3(ORC_PROJECT_LANES), lds, stream, v);
   else hipLaunchKernelGGL(K6, dim3(blocks), dim3(ORC_PROJECT_LANES), lds, stream, v);
   return hipGetLastError();
}
