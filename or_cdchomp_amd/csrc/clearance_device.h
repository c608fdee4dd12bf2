// clearance_device.h -- the clearance of a batch's runs (clearance_kernels.hip), as clearance.cpp launches it.  The selection by
// margin that reads it is orc_launch_select's (launch.h).
#pragma once
#include <hip/hip_runtime.h>
#include "verdict_device.h"

// The device-planned walk (DevVerdictPlanned, verdict_planned.h) without the verdict's stop at the first contact: over every
// sample of an examined run the smallest `value - radius` of a live active sphere in a field of the run's scene, and the
// smallest `distance - radius sum` of a pair of the self-collision leg.  key_out and depth_out of the walk are not used;
// n_samples_out: the samples walked.
template <typename real>
struct DevClearance : DevVerdictPlanned<real>
{
   int max_samples;            // a run with C-space length / 0.04 >= max_samples is too long: nothing of it is walked
   // per run two minima, [0] over the fields and [1] over the pairs: the value widened to double (+inf: nothing to take a
   // minimum of; NaN: the run was not walked), its key and its time on the retimed trajectory (-1 without a key).
   //   key [0]: sample << 32 | XML sphere << 16 | field      key [1]: sample << 32 | XML sphere a << 16 | XML sphere b
   // the lowest key among the items that attain the minimum; ORC_VERDICT_NONE without one
   double * clear_out;              // [n_runs][2]
   unsigned long long * ckey_out;   // [n_runs][2]
   double * ctime_out;              // [n_runs][2]
};

#define ORC_CLEARANCE_MAX_SAMPLES (1 << 20)

hipError_t orc_launch_clearance(const DevClearance<double> & v, size_t lds, hipStream_t stream, int tree);
hipError_t orc_launch_clearance(const DevClearance<float> & v, size_t lds, hipStream_t stream, int tree);
size_t orc_clearance_lds_bytes(int n_points, int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk);
