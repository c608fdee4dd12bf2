// merge_interp.h -- the reference's grid interpolation and one cell of a merged field (orc_scene_merge_fields), for the host
// and for the device.
//
// cd_grid_double_interp (/root/reference src/libcd/grid.c:386-454) operation for operation: the reference's divisions, not the
// reciprocals the iterate kernel's lookup folds on the host (sdf_lookup.h), its HUGE_VAL poisoning, its choice of the inward
// neighbour in the edge cells.  One definition for the host path (host_math.cpp: grid_interp, merge_fields_host) and the
// device kernel (merge_kernels.hip): the same operations in the same order, no contraction into fused multiply-adds in either
// file, so the two agree bit for bit (the vox_tri.h pattern).
#pragma once
#include <math.h>

#ifndef ORC_HD
#if defined(__HIPCC__)
#define ORC_HD __host__ __device__
#else
#define ORC_HD
#endif
#endif

// (the device reads the cells as global memory: a pointer that comes out of a table would otherwise cost flat loads)
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(1))) double * orc_grid_cells;
#else
typedef const double * orc_grid_cells;
#endif

// returns 1 when p lies outside the grid (sizes [3], lengths [3], data C order [x][y][z]; every size >= 2).  The bounds test is
// written so that a NaN coordinate counts as outside (`x < 0 || x > 1` would let it through to an index); no read leaves the
// grid for any input.
ORC_HD inline int orc_grid_interp(const int * sizes, const double * lengths, const double * cells, const double * p, double * value)
{
   const orc_grid_cells data = (orc_grid_cells) cells;
   int sub[3];
   for (int d=0; d<3; d++)
   {
      const double x = p[d] / lengths[d];
      if (!(x >= 0.0 && x <= 1.0)) return 1;
      int s = (int) ::floor(x * sizes[d]);
      if (s == sizes[d]) s--;
      sub[d] = s;
   }
   const size_t stride[3] = { (size_t) sizes[1] * sizes[2], (size_t) sizes[2], 1 };
   const size_t index = sub[0]*stride[0] + sub[1]*stride[1] + sub[2];
   double v = data[index];
   if (v == HUGE_VAL) { *value = HUGE_VAL; return 0; }
   for (int d=2; d>=0; d--)
   {
      const double center = (0.5 + sub[d]) / sizes[d] * lengths[d];
      bool prev;
      if (sub[d] == 0) prev = false;
      else if (sub[d] == sizes[d]-1) prev = true;
      else prev = p[d] < center;
      const double after = prev ? data[index] : data[index + stride[d]];
      const double before = prev ? data[index - stride[d]] : data[index];
      if (after == HUGE_VAL || before == HUGE_VAL) { *value = HUGE_VAL; return 0; }
      double diff = after;
      diff -= before;
      v += diff * sizes[d] / lengths[d] * (p[d] - center);
   }
   *value = v;
   return 0;
}

// one source of a merge as the kernel reads it: the affine from the target grid's frame to the source grid's frame
// (p_src = A p_tgt + t, composed once on the host in double: merge_affine of host_math.cpp), and the source grid
struct OrcMergeSource
{
   double A[9];         // row major
   double t[3];
   double length[3];
   int size[3];
   int pad_;
   const double * data; // host twin: host memory; kernel: the field's fp64 copy on the device
};

// cell `idx` (C order, z fastest) of the merged grid: the best-of-N field loop (src/orcdchomp_mod.cpp:1170-1190: strict <, so a
// poisoned value never wins) evaluated at the cell's centre, the centre as voxelize_kernel and Grid::center form it.  A cell no
// source covers is HUGE_VAL.
ORC_HD inline double orc_merge_cell(const int * tsizes, const double * tlengths, long idx, const OrcMergeSource * src, int n_src)
{
   long rem = idx; double c[3];
   for (int d=2; d>=0; d--)
   {
      const int sub = (int)(rem % tsizes[d]);
      rem /= tsizes[d];
      c[d] = (0.5 + sub) / tsizes[d];
   }
   for (int d=0; d<3; d++) c[d] *= tlengths[d];
   double best = HUGE_VAL;
   for (int k=0; k<n_src; k++)
   {
      const OrcMergeSource & s = src[k];
      double p[3], val;
      for (int i=0; i<3; i++) p[i] = (s.A[i*3+0]*c[0] + s.A[i*3+1]*c[1] + s.A[i*3+2]*c[2]) + s.t[i];
      if (orc_grid_interp(s.size, s.length, s.data, p, &val)) continue;
      if (val < best) best = val;
   }
   return best;
}
