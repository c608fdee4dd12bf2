// verdict.h -- host side of the collision verdict (verdict.cpp): the retiming and the sample clock that gettraj's re-check and the
// host-planned verdict share, then what the verdicts take from a batch.  Down to SampleClock nothing needs HIP or the module.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace orc {
struct Robot; class Batch; class Environment;

// LinearTrajectoryRetimer stand-in (reference: RetimeActiveDOFTrajectory(..., "LinearTrajectoryRetimer"),
// src/orcdchomp_mod.cpp:2905-2911): each segment is traversed at the largest constant velocity the dof velocity limits allow.
inline std::vector<double> retime_linear(const double * traj, int n_points, int n, int col0, const std::vector<double> & vmax)
{
   std::vector<double> dtm(n_points, 0.0);
   for (int i=1; i<n_points; i++)
      for (int j=col0; j<n; j++)
      {
         const double v = vmax[j-col0] > 0.0 ? vmax[j-col0] : 1.0;
         dtm[i] = std::max(dtm[i], std::fabs(traj[(size_t) i*n+j] - traj[(size_t)(i-1)*n+j]) / v);
      }
   return dtm;
}

// Samples of a retimed trajectory [n_points][n] every 0.04 rad of C-space distance, the grid of the reference's re-check
// (src/orcdchomp_mod.cpp:2958-3006): `for (SampleClock c(...); c.sample(); c.step())` visits every sample with the segment it
// lies on, the position on it and its time.  Every rounding here is the verdict's (NOTES/verdict-on-device.md): keep the order.
struct SampleClock
{
   int seg = 0; double u = 0.0, time = 0.0;
   SampleClock(const double * traj, int n_points, int n, int col0, const std::vector<double> & dtm) : dtm_(dtm.data()), last_seg_(n_points - 2)
   {
      double total_dist = 0.0;
      for (int i=0; i+1<n_points; i++)
      {
         double d2 = 0.0;
         for (int j=col0; j<n; j++) { const double d = traj[(size_t) i*n+j] - traj[(size_t)(i+1)*n+j]; d2 += d*d; }
         total_dist += std::sqrt(d2);
         duration_ += dtm[i+1];
      }
      step_time_ = total_dist > 0.0 ? duration_ * 0.04 / total_dist : duration_ + 1.0;
   }
   bool sample()      // false: the trajectory is over; true: seg and u are those of `time`
   {
      if (!(time < duration_)) return false;
      while (seg < last_seg_ && tseg0_ + dtm_[seg+1] < time) { tseg0_ += dtm_[seg+1]; seg++; }
      u = dtm_[seg+1] > 0.0 ? (time - tseg0_) / dtm_[seg+1] : 0.0;
      return true;
   }
   void step() { time += step_time_; }      // (added up, never k * step_time)
private:
   const double * dtm_; int last_seg_;
   double duration_ = 0.0, step_time_ = 0.0, tseg0_ = 0.0;
};

// the collision verdict's plan of one trajectory (retime_linear, then the clock's samples): appended to the outputs (orc_host_verdict_samples)
void host_verdict_samples(const double * traj, int n_points, int n, int col0, const std::vector<double> & vmax,
   std::vector<int> & seg_out, std::vector<double> & u_out, std::vector<double> & time_out);

// what the verdicts take from a batch: the first retimed column, the velocity limits of the batch's columns and the tables of
// the self-collision leg (verdict_device.h: pairs, pair_rsum, inact_pos)
struct VerdictInputs
{
   int col0;
   std::vector<double> vmax;
   std::vector<int> pairs;
   std::vector<double> rsum, inact_pos;
};
// tables false: the pair tables, which only the kernels read, stay empty (gettraj's re-check walks the spheres itself)
VerdictInputs verdict_inputs(const Robot & robot, const Batch & b, bool self_check, bool tables = true);
// gettraj's re-check of run 0 of `b` on the host, dtm being retime_linear's: true when a sample is in contact, with the line the reference logs
bool host_recheck(const Environment & env, const Batch & b, const double * traj, const std::vector<double> & dtm, bool self_check, std::string & details);

} // namespace orc
