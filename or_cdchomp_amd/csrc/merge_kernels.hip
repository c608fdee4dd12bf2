// merge_kernels.hip -- the fields of any number of placed kinbodies resampled into one grid (orc_scene_merge_fields).
//
// One thread per cell of the target grid, 256 threads per workgroup, a 64-bit cell index as in voxelize_kernel; z is the
// fastest index, so a wavefront stores 64 consecutive doubles.  Every cell is orc_merge_cell of merge_interp.h, the function
// the host twin (merge_fields_host, host_math.cpp) calls: the best-of-N field loop at the cell's centre through the
// reference's interpolation, with its divisions.  Contraction into fused multiply-adds is off for this file as for the
// host's, so device and host agree bit for bit.
// The sources come as a table in device memory indexed by the loop's source number, which is the same in every lane: the
// record (affine, sizes, lengths, data pointer) is read with scalar loads.  A lane whose centre lies outside a source's box
// leaves orc_grid_interp before it reads a cell; the reads of the others are a gather of up to four cells of 8 bytes each
// around the centre's image, neighbours in z for neighbouring lanes when the two grids are aligned.
#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)

#include "merge_launch.h"

namespace {

struct MergeTarget { int size[3]; int pad_; double length[3]; };

__global__ __launch_bounds__(256) void merge_fields_kernel(double * __restrict__ out, MergeTarget g,
   const OrcMergeSource * __restrict__ sources, int n_src)
{
   const long count = (long) g.size[0] * g.size[1] * g.size[2];
   const long idx = blockIdx.x * (long) blockDim.x + threadIdx.x;
   if (idx >= count) return;
   out[idx] = orc_merge_cell(g.size, g.length, idx, sources, n_src);
}

} // namespace

hipError_t orc_launch_merge_fields(double * out, const int sizes[3], const double lengths[3], const OrcMergeSource * sources, int n_src,
   hipStream_t stream)
{
   MergeTarget g;
   for (int d=0; d<3; d++) { g.size[d] = sizes[d]; g.length[d] = lengths[d]; }
   g.pad_ = 0;
   const long count = (long) sizes[0] * sizes[1] * sizes[2];
   if (count < 1 || count >= (long) 1 << 28 || n_src < 0) return hipErrorInvalidValue;      // (2^31 bytes: refused by the caller already)
   hipLaunchKernelGGL(merge_fields_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, out, g, sources, n_src);
   return hipGetLastError();
}
