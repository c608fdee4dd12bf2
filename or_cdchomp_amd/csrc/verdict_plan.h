// verdict_plan.h -- the plan of a run's samples on the device: the host's arithmetic (verdict.h retime_linear, SampleClock),
// rounding for rounding, as the planner wavefront of the planned walk (verdict_planned.h: collision_verdict_planned_kernel and
// clearance_kernel) runs it.  module.py verdict_samples is its specification: doubles for either
// precision, no fused multiply-add, the sums in index order, time advanced by repeated addition.
//
// Included inside the including file's namespace after <hip/hip_runtime.h> and <math.h>, with `#pragma clang fp contract(off)`
// in force: a contraction here changes the samples.
#pragma once

#define ORC_VD_MAX_SAMPLES (1 << 30)        // the sample index sits above bit 32 of the key, under ORC_VERDICT_NONE

// segment i (rows i-1 and i): its time at the largest velocity the limits allow, and its length
template <typename real>
__device__ __forceinline__ void plan_segment(const real * traj, int i, int n, int col0, const double * vmax, double & dtm, double & len)
{
   double dt = 0.0, d2 = 0.0;
   for (int j=col0; j<n; j++)
   {
      const double lo = (double) traj[(size_t)(i-1)*n + j], hi = (double) traj[(size_t) i*n + j];
      const double v = vmax[j-col0] > 0.0 ? vmax[j-col0] : 1.0;
      const double c = ::fabs(hi - lo) / v;
      dt = dt < c ? c : dt;                  // std::max(dt, c): a NaN candidate is ignored
      const double d = lo - hi;
      d2 += d*d;
   }
   dtm = dt; len = ::sqrt(d2);
}

// in: tstart[i] = length of segment i; out: tstart[i] = time at which segment i ends (tstart[0] = 0, tstart[np-1] = duration)
__device__ __forceinline__ void plan_totals(int np, const double * dtm, double * tstart, double & total_dist, double & duration)
{
   double td = 0.0, du = 0.0;
   tstart[0] = 0.0;
   for (int i=1; i<np; i++)
   {
      td += tstart[i];
      du += dtm[i];
      tstart[i] = du;
   }
   total_dist = td; duration = du;
}

__device__ __forceinline__ double plan_step_time(double total_dist, double duration)
{
   return total_dist > 0.0 ? duration * 0.04 / total_dist : duration + 1.0;
}

// A run of `cap` samples or more is too long, and so is one whose step does not advance the clock (an underflow: the walk
// would never end).  Decided before anything is walked; a run this passes has at most cap + 2 samples.
__device__ __forceinline__ bool plan_too_long(double total_dist, double step_time, double duration, int cap)
{
   return duration > 0.0 && (total_dist / 0.04 >= (double) cap || step_time <= 0.0);
}

// the next samples' times, `cap` at most; returns their number
__device__ __forceinline__ int plan_times(double & time, double step_time, double duration, double * out, int cap)
{
   int k = 0;
   while (k < cap && time < duration) { out[k++] = time; time += step_time; }
   return k;
}

// the samples nobody walks
__device__ __forceinline__ int plan_count_rest(double time, double step_time, double duration, int have)
{
   while (have < ORC_VD_MAX_SAMPLES && time < duration) { time += step_time; have++; }
   return have;
}

// segment of a sample and its position on it
__device__ __forceinline__ int plan_locate(double time, int np, const double * dtm, const double * tstart, double & u)
{
   int lo = 0, hi = np - 2;                  // the largest s in 1 .. np-2 with tstart[s] < time (tstart does not decrease), or 0
   while (lo < hi)
   {
      const int mid = (lo + hi + 1) >> 1;
      if (tstart[mid] < time) lo = mid; else hi = mid - 1;
   }
   const double d = dtm[lo+1];
   u = d > 0.0 ? (time - tstart[lo]) / d : 0.0;
   return lo;
}
