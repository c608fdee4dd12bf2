// query_upload.h -- what a single-row call puts on a shard's device for its queries (config_clearance.cpp, penetration.cpp,
// project.cpp, project_clear.cpp): the rows in the batch's precision, the optional int arrays, the box, the constraints of the
// call, the lanes' workspace.  One QueryUpload per call: it owns the device memory and the host copies the asynchronous
// uploads read, so it lives until the call has synchronised.
#pragma once
#include <cmath>
#include <deque>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>
#include "stages.h"
#include "devbuf.h"
#include "verdict_device.h"      // ORC_VERDICT_LDS_LIMIT
#include "project_device.h"

namespace orc {

// the queries a workgroup of a walk's kernel takes: 64, or what the LDS of a CU holds of this robot's rows, positions and
// joint frames behind what the kernel itself keeps there (lds_bytes(chunk): the kernel's dynamic LDS)
template <typename LdsBytes>
int walk_chunk(const LdsBytes & lds_bytes)
{
   int chunk = 64;
   while (chunk > 4 && lds_bytes(chunk) > ORC_VERDICT_LDS_LIMIT) chunk -= 4;
   return chunk;
}

// where a lane's state of the projection kernels lives for n columns and `kmax` enforced rows: in LDS when a workgroup's
// states fit, else in a workspace of the call
inline bool project_state_fits_lds(int n, int kmax, size_t real_size)
{
   return (size_t) ORC_PROJECT_LANES * orc_project_stride(n, kmax) * real_size <= ORC_PROJECT_LDS_BYTES;
}

template <typename real>
struct QueryUpload
{
   // tag: the call's name in the labels of its HIP calls ("<tag> rows")
   QueryUpload(hipStream_t stream, const char * tag) : st(stream), tag(tag) {}

   template <typename T> T * alloc(size_t count)
   {
      bufs.emplace_back();
      bufs.back().reset(dev_alloc<T>(count));
      return bufs.back().template as<T>();
   }
   void up(void * dst, const void * src, size_t bytes, const char * what) { check(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st), what); }
   void down(void * dst, const void * src, size_t bytes, const char * what) { if (dst) check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st), what); }      // (a NULL output is not wanted)
   void zero(void * dst, size_t bytes, const char * what) { check(hipMemsetAsync(dst, 0, bytes, st), what); }
   void sync(const char * what = "sync") { check(hipStreamSynchronize(st), what); }
   void check(hipError_t e, const char * what) { if (e != hipSuccess) hip_check(e, (tag + " " + what).c_str()); }

   // rows as `real` (a precision-32 batch: narrowed as set_traj narrows)
   real * rows(const double * src, size_t count)
   {
      real * d = alloc<real>(count);
      const void * from = src;
      if (sizeof(real) != sizeof(double)) { narrowed.assign(src, src + count); from = narrowed.data(); }
      up(d, from, count*sizeof(real), "rows");
      return d;
   }
   // an optional int array: NULL stays NULL
   const int * ints(const int * src, size_t count, const char * what)
   {
      if (!src) return nullptr;
      int * d = alloc<int>(count);
      up(d, src, count*sizeof(int), what);
      return d;
   }
   // the box as `real`, -inf / +inf without one.  Precision 32: a limit that rounds outwards is taken one step inwards, so that
   // a clipped row lies inside the caller's box
   void box(const double * lower, const double * upper, int n, const real * & d_lower, const real * & d_upper)
   {
      const real inf = std::numeric_limits<real>::infinity();
      lo.resize(n); hi.resize(n);
      for (int c=0; c<n; c++)
      {
         lo[c] = lower ? (real) lower[c] : -inf;
         hi[c] = upper ? (real) upper[c] : inf;
         if (lower && (double) lo[c] < lower[c]) lo[c] = std::nextafter(lo[c], inf);
         if (upper && (double) hi[c] > upper[c]) hi[c] = std::nextafter(hi[c], -inf);
      }
      real * dl = alloc<real>(n), * dh = alloc<real>(n);
      up(dl, lo.data(), n*sizeof(real), "lower");
      up(dh, hi.data(), n*sizeof(real), "upper");
      d_lower = dl; d_upper = dh;
   }
   // the constraints of a call on the device's joint order, folded as `create` folds a batch's for a trajectory of one moving
   // point; kmax: 3 when none enforces more rows, else 6.  (who: the call's name in what it throws)
   const DevTsr<real> * constraints(const char * who, const Robot & robot, const BatchParams & params, int nj, int n, const std::vector<TsrSpec> & specs, int & kmax)
   {
      const JointTree tree = fold_joint_tree(robot, params.floating_base != 0);
      if (tree.nj() != nj) throw std::runtime_error(std::string(who) + ": the robot's joint tree is not the one the batch was created with!");
      BatchParams one = params;
      one.tsrs = specs;
      folded = fold_tsrs<real>(robot, one, tree, 1, n).tsrs;
      kmax = 3;
      for (const DevTsr<real> & t : folded) if (t.k > 3) kmax = 6;
      DevTsr<real> * d = alloc<DevTsr<real>>(folded.size());
      up(d, folded.data(), folded.size()*sizeof(DevTsr<real>), "tsrs");
      return d;
   }
   // the lanes' state of a projection kernel: NULL when it lives in LDS, else the call's workspace
   real * lane_state(int n_q, int n, int kmax)
   {
      return project_state_fits_lds(n, kmax, sizeof(real)) ? nullptr : alloc<real>((size_t) n_q * orc_project_stride(n, kmax));
   }

   hipStream_t st;
   std::string tag;
private:
   std::deque<DevBuf> bufs;
   std::vector<real> narrowed, lo, hi;
   std::vector<DevTsr<real>> folded;
};

} // namespace orc
