// merge_launch.h -- the launch wrapper of merge_kernels.hip, as the host layer calls it.
#pragma once
#include <hip/hip_runtime.h>
#include "merge_interp.h"

// the merged grid of `n_src` sources (a device table of OrcMergeSource whose data pointers are device memory) into `out`
// (device memory, sizes[0] sizes[1] sizes[2] doubles); enqueue only
hipError_t orc_launch_merge_fields(double * out, const int sizes[3], const double lengths[3], const OrcMergeSource * sources, int n_src,
   hipStream_t stream);
