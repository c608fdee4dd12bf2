// launch.h -- the launch wrappers of chomp_kernel.hip, as batch.cpp calls them (one name per wrapper, overloaded by precision).
#pragma once
#include <hip/hip_runtime.h>
#include "dev_types.h"

// the row of kernel_table.h that (variant, block, precision) names; hipErrorInvalidValue when the library holds no such kernel
hipError_t orc_launch_iterate(const DevBatch<double> & b, size_t lds, hipStream_t stream, int variant, int block);
hipError_t orc_launch_iterate(const DevBatch<float> & b, size_t lds, hipStream_t stream, int variant, int block);
// straight-line seed trajectories (instantiated for double and float)
template <typename real>
hipError_t orc_launch_seed(real * traj, const double * starts, const double * goals, int n_runs, int n_points, int n, int floating, hipStream_t stream);
