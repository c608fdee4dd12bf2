// penetration_kernels.hip -- the penetration cost of given configurations and of waypoints, with its gradient
// (orc_batch_config_penetration, orc_batch_waypoint_penetration): config_clearance_kernel's sibling.  Per query, one stateless
// evaluation: U_f over the spheres and fields, U_s over the pairs, d(U_f + U_s)/d row, and the two minima and keys of the sibling.
//
// Staging, the copy of the rows, verdict_renormalise and verdict_fk are the sibling's (config_query_prologue of config_query.h,
// with one real per query of its own in the LDS header), and the wavefront that ran FK for a query evaluates it alone.  Its
// lanes change roles twice:
//   lane = sphere slot   the slot's fields in scene order, then the slot's pairs in list order (the pairs by sphere: a CSR the
//                        host builds from the pair table).  The lane ends with its sphere's total force f = dU/dp and its
//                        share of the two costs.
//   lane = joint         the sum of (p x C f, f) over the spheres the joint moves (DevModel::sph_affects), slot by slot through
//                        lane reads, contracted with the axis and anchor verdict_fk left in ax_s.
//   every lane           butterfly sums of the costs and, for a floating base, of the wrench.
// The two minima and their keys are the sibling's to the bit.  They are taken by the sibling's own loop (config_tests of
// config_query.h, lanes striding over the items), not from the gaps the cost pass forms: the lookup is compiled with contraction
// allowed, and where its slope is live (here, for the force) the compiler fuses and vectorises its sums differently than where it
// is dead (there) -- in fp32 the two gaps differ in the last bit.  A second lookup per item is the price of the same bits.
// Every sum has a fixed order that depends on the robot alone, and there is no atomic: a query's answer depends on its row, its
// run and the margins only.
//
// C: the base frame of a fixed robot is applied as the matrix the host made of its pose, which is a rotation only as far as
// the pose's quaternion is a unit one.  With Rb that matrix, a revolute joint moves a sphere by Rb (a_l x r_l) = C (a x r),
// C = Rb Rb^T / det Rb, for the world axis a and lever r: the joint's entry is a . (r x C f).  For a rotation C is the identity
// (a floating base: the renormalised quaternion's).
#include <hip/hip_runtime.h>
#include <math.h>
#include <atomic>
#include "dev_types.h"
#include "penetration_device.h"

#pragma clang fp contract(fast)
namespace {

#include "sdf_lookup.h"
#include "fk.h"
#include "verdict_walk.h"
#include "wave.h"           // wave_sum, read_lane; config_query.h's wave_min
#include "config_query.h"

// lane = sphere slot: the slot's items of query s.  f: dU/dp of the sphere, cost [2] the lane's share of U_f and U_s
template <typename real>
__device__ __forceinline__ void pen_sphere(const DevPenetration<real> & v, const DevSdf<real> * sdfs, int n_fields, int s, int slot,
   const VerdictLds<real> & L, const real p[3], real f[3], real cost[2])
{
   const real radius = L.srad_s[slot];
   for (int i=0; i<n_fields; i++)
   {
      const DevSdf<real> & F = sdfs[i];
      real gp[3], gg[3], val;
#pragma unroll
      for (int k=0; k<3; k++)
         gp[k] = F.Rgw[k*3+0]*p[0] + F.Rgw[k*3+1]*p[1] + F.Rgw[k*3+2]*p[2] + F.tgw[k];
      if (sdf_lookup(F, gp, val, gg)) continue;                 // outside this field
      const real gap = val - radius;
      if (gap < v.margin_field)      // (not +inf, a poisoned value; not a NaN)
      {
         const real d = v.margin_field - gap;
         cost[0] += (real)0.5 * d * d;
#pragma unroll
         for (int c=0; c<3; c++) f[c] -= d * (F.Rgw[0*3+c]*gg[0] + F.Rgw[1*3+c]*gg[1] + F.Rgw[2*3+c]*gg[2]);      // the slope, into the world
      }
   }
   for (int e=v.sph_pair_offs[slot]; e<v.sph_pair_offs[slot+1]; e++)
   {
      const int w = v.sph_pair_list[e];
      const int pi = w >> 3, role = w & 3;
      const bool owner = (w & 4) != 0;
      const int ea = v.pairs[pi*4+0], eb = v.pairs[pi*4+1];
      const real * pa = (ea >= 0) ? L.pos_s + s*L.pstr + ea*3 : v.inact_pos + (-1 - ea)*3;
      const real * pb = (eb >= 0) ? L.pos_s + s*L.pstr + eb*3 : v.inact_pos + (-1 - eb)*3;
      const real dx = pa[0]-pb[0], dy = pa[1]-pb[1], dz = pa[2]-pb[2];
      const real dist = M<real>::sqrt_(dx*dx + dy*dy + dz*dz);
      const real rs = v.pair_rsum[pi];
      const real gap = dist - rs;
      if (gap < v.margin_self)
      {
         const real d = v.margin_self - gap;
         if (owner) cost[1] += (real)0.5 * d * d;
         if (role < 2 && dist != (real)0)      // the gap's slope is +-(pa - pb)/dist; coincident centres have none
         {
            const real sc = ((role == 0) ? -d : d) / dist;
            f[0] += sc * dx; f[1] += sc * dy; f[2] += sc * dz;
         }
      }
   }
}

template <typename real, bool TREE>
__global__ __launch_bounds__(ORC_BLOCK)
void penetration_kernel(DevPenetration<real> v)
{
   extern __shared__ __align__(16) unsigned char smem_raw[];
   const DevModel<real> & gmod = *v.model;
   const int lane = threadIdx.x & 63, n = v.n;
   real * qinv_s = (real *)(smem_raw + config_query_header_bytes(v.chunk, 0));      // [chunk] a floating base: 1 / |quaternion| of the caller's row
   const ConfigQuery<real> Q = config_query_prologue<real, TREE>(v, smem_raw, sizeof(real), [qinv_s](int s, const real * row, const ModelView<real> & mod) {
      qinv_s[s] = mod.floating ? (real)1 / M<real>::sqrt_(row[3]*row[3] + row[4]*row[4] + row[5]*row[5] + row[6]*row[6]) : (real)1;
   });
   const VerdictLds<real> & L = Q.L;
   const ModelView<real> & mod = Q.mod;
   // C (top of the file), row major; symmetric
   real C[9] = { (real)1, (real)0, (real)0, (real)0, (real)1, (real)0, (real)0, (real)0, (real)1 };
   if (!mod.floating)
   {
      const real * B = L.base_s;
      const real det = B[0]*(B[4]*B[8] - B[5]*B[7]) - B[1]*(B[3]*B[8] - B[5]*B[6]) + B[2]*(B[3]*B[7] - B[4]*B[6]);
      const real inv_det = (real)1 / det;
#pragma unroll
      for (int r=0; r<3; r++)
#pragma unroll
         for (int c=0; c<3; c++) C[r*3+c] = (B[r*3+0]*B[c*3+0] + B[r*3+1]*B[c*3+1] + B[r*3+2]*B[c*3+2]) * inv_det;
   }
   const int Sa = mod.Sa, nj = mod.nj;
   const bool live = (lane < Sa) && ((mod.live_mask >> lane) & 1ull);
   const double nan = __longlong_as_double(0x7ff8000000000000LL);
   for (int s=Q.s_begin; s<Q.s_end; s++)
   {
      const size_t q = (size_t)(Q.q0 + s);
      if (Q.bad_s[s])      // (wave-uniform)
      {
         if (lane < 2)
         {
            v.clear_out[q*2 + lane] = nan;
            v.ckey_out[q*2 + lane] = ORC_CONFIG_NONE;
            v.cost_out[q*2 + lane] = nan;
         }
         for (int c=lane; c<n; c+=64) v.grad_out[q*n + c] = nan;
         continue;
      }
      const DevSdf<real> * sdfs; int n_fields;
      verdict_scene<real>(v, __builtin_amdgcn_readfirstlane(Q.run_s[s]), sdfs, n_fields);
      ConfigMin<real> best[2];      // [0] fields, [1] pairs
      for (int leg=0; leg<2; leg++) { best[leg].val = M<real>::inf(); best[leg].key = ORC_CONFIG_NONE; }
      config_tests<real>(v, mod, sdfs, n_fields, s, lane, L, best[0], best[1]);
      // ---- lane = sphere slot
      real p[3] = { (real)0, (real)0, (real)0 }, f[3] = { (real)0, (real)0, (real)0 }, cost[2] = { (real)0, (real)0 };
      if (live)
      {
#pragma unroll
         for (int k=0; k<3; k++) p[k] = L.pos_s[s*L.pstr + lane*3 + k];
         pen_sphere<real>(v, sdfs, n_fields, s, lane, L, p, f, cost);
      }
      for (int leg=0; leg<2; leg++)
      {
         config_report<real>(best[leg], lane, v.clear_out + q*2 + leg, v.ckey_out + q*2 + leg);
         const real total = wave_sum<real>(cost[leg]);
         if (lane == 0) v.cost_out[q*2 + leg] = (double) total;
      }
      // the sphere's wrench about the world's origin: (p x C f, f)
      real w6[6];
      {
         const real cf0 = C[0]*f[0] + C[1]*f[1] + C[2]*f[2], cf1 = C[3]*f[0] + C[4]*f[1] + C[5]*f[2], cf2 = C[6]*f[0] + C[7]*f[1] + C[8]*f[2];
         w6[0] = p[1]*cf2 - p[2]*cf1;
         w6[1] = p[2]*cf0 - p[0]*cf2;
         w6[2] = p[0]*cf1 - p[1]*cf0;
         w6[3] = f[0]; w6[4] = f[1]; w6[5] = f[2];
      }
      // ---- lane = joint: the spheres it moves, in slot order
      real W[6] = { (real)0, (real)0, (real)0, (real)0, (real)0, (real)0 };
      for (int o=0; o<Sa; o++)      // (o is uniform: every lane reads lane o)
      {
         const unsigned long long aff = ((mod.live_mask >> o) & 1ull) ? gmod.sph_affects[o] : 0ull;
         const bool mine = (aff >> lane) & 1ull;
#pragma unroll
         for (int k=0; k<6; k++)
         {
            const real x = read_lane(w6[k], o);
            W[k] += mine ? x : (real)0;
         }
      }
      if (lane < nj)
      {
         const int pk = L.jctl_s[2*lane];
         const real * ax = L.ax_s + s*L.astr + lane*6;
         // the joint's entry: a . (tau - an x C F) for a revolute joint, a . F for a prismatic one
         const real F0 = C[0]*W[3] + C[1]*W[4] + C[2]*W[5], F1 = C[3]*W[3] + C[4]*W[4] + C[5]*W[5], F2 = C[6]*W[3] + C[7]*W[4] + C[8]*W[5];
         const real c0 = W[0] - (ax[4]*F2 - ax[5]*F1);
         const real c1 = W[1] - (ax[5]*F0 - ax[3]*F2);
         const real c2 = W[2] - (ax[3]*F1 - ax[4]*F0);
         const real crev = ax[0]*c0 + ax[1]*c1 + ax[2]*c2;
         const real cpri = ax[0]*W[3] + ax[1]*W[4] + ax[2]*W[5];
         v.grad_out[q*n + ((pk >> 24) & 127)] = (double)(((pk & 3) == 1) ? crev : cpri);
      }
      // ---- a floating base: the wrench of all spheres on the pose.  Its translation takes the force; its unit quaternion u takes
      // e_c . (tau - x x F) (cost_generic.h has the four e_c), which is tangent to the unit sphere, so the renormalisation
      // u = r/|r| of the caller's row only scales it by 1/|r|
      if (mod.floating)      // (uniform)
      {
         real T[6];
#pragma unroll
         for (int k=0; k<6; k++) T[k] = wave_sum<real>(w6[k]);
         if (lane == 0)
         {
            const real * row = L.rows_s + s*n;
            const real x = row[0], y = row[1], z = row[2];
            const real qx = 2*row[3], qy = 2*row[4], qz = 2*row[5], qw = 2*row[6];
            const real tq0 = T[0] - (y*T[5] - z*T[4]);
            const real tq1 = T[1] - (z*T[3] - x*T[5]);
            const real tq2 = T[2] - (x*T[4] - y*T[3]);
            const real inv = qinv_s[s];
            double * g = v.grad_out + q*n;
            g[0] = (double) T[3]; g[1] = (double) T[4]; g[2] = (double) T[5];
            g[3] = (double)(( qw*tq0 + qz*tq1 - qy*tq2) * inv);
            g[4] = (double)((-qz*tq0 + qw*tq1 + qx*tq2) * inv);
            g[5] = (double)(( qy*tq0 - qx*tq1 + qw*tq2) * inv);
            g[6] = (double)((-qx*tq0 - qy*tq1 - qz*tq2) * inv);
         }
      }
   }
}

} // namespace

template <typename real>
static hipError_t launch_penetration_t(const DevPenetration<real> & v, size_t lds, hipStream_t stream, int tree)
{
   if (!v.sph_pair_offs || !v.sph_pair_list || !v.cost_out || !v.grad_out || !v.clear_out || !v.ckey_out) return hipErrorInvalidValue;
   return launch_config_query<DevPenetration<real>, penetration_kernel<real, true>, penetration_kernel<real, false>>(v, lds, stream, tree);
}
hipError_t orc_launch_penetration(const DevPenetration<double> & v, size_t lds, hipStream_t stream, int tree) { return launch_penetration_t<double>(v, lds, stream, tree); }
hipError_t orc_launch_penetration(const DevPenetration<float> & v, size_t lds, hipStream_t stream, int tree) { return launch_penetration_t<float>(v, lds, stream, tree); }

// dynamic LDS of penetration_kernel: the queries' header with one real per query, then what the walk holds
size_t orc_penetration_lds_bytes(int n, int Sa, int Sa_real, int nj, size_t real_size, int chunk) { return config_query_lds_bytes(n, Sa, Sa_real, nj, real_size, chunk, real_size); }
