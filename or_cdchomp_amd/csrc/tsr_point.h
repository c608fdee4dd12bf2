// tsr_point.h -- con_tsr at one row: the value and the Jacobian of a TSR's enabled rows (tsr_eval_point), with the pose
// helpers it is made of.  The constraint step of the iterate kernel (tsr.h) evaluates every constrained trajectory row
// with it, the projection kernel (project_kernels.hip) single configurations.  Needs M<real> (sdf_lookup.h), sincos_joint
// (fk.h) and DevModel / DevTsr (dev_types.h) in front of it.
#pragma once

template <typename real> struct TM;
template <> struct TM<double>
{
   static __device__ __forceinline__ double atan2_(double y, double x) { return ::atan2(y, x); }
   static __device__ __forceinline__ double asin_(double x) { return ::asin(x); }
};
template <> struct TM<float>
{
   static __device__ __forceinline__ float atan2_(float y, float x) { return ::atan2f(y, x); }
   static __device__ __forceinline__ float asin_(float x) { return ::asinf(x); }
};

// the expanded quaternion rotation of kin.c:160-172
template <typename real>
__device__ __forceinline__ void t_quat_rotate(real qx, real qy, real qz, real qw, real x, real y, real z, real out[3])
{
   const real qx2 = qx*qx, qy2 = qy*qy, qz2 = qz*qz, qw2 = qw*qw;
   const real qxqy = qx*qy, qxqz = qx*qz, qxqw = qx*qw, qyqz = qy*qz, qyqw = qy*qw, qzqw = qz*qw;
   out[0] = x*(qx2-qy2-qz2+qw2) + 2*y*(qxqy-qzqw) + 2*z*(qxqz+qyqw);
   out[1] = 2*x*(qxqy+qzqw) + y*(-qx2+qy2-qz2+qw2) + 2*z*(qyqz-qxqw);
   out[2] = 2*x*(qxqz-qyqw) + 2*y*(qyqz+qxqw) + z*(-qx2-qy2+qz2+qw2);
}
// cd_kin_pose_compose, kin.c:136-178
template <typename real>
__device__ __forceinline__ void t_pose_compose(const real ab[7], const real bc[7], real ac[7])
{
   const real ax = ab[3], ay = ab[4], az = ab[5], aw = ab[6];
   const real bx = bc[3], by = bc[4], bz = bc[5], bw = bc[6];
   real rot[3];
   ac[3] = aw*bx + ax*bw + ay*bz - az*by;
   ac[4] = aw*by - ax*bz + ay*bw + az*bx;
   ac[5] = aw*bz + ax*by - ay*bx + az*bw;
   ac[6] = aw*bw - ax*bx - ay*by - az*bz;
   t_quat_rotate(ax, ay, az, aw, bc[0], bc[1], bc[2], rot);
   ac[0] = rot[0] + ab[0]; ac[1] = rot[1] + ab[1]; ac[2] = rot[2] + ab[2];
}
// cd_kin_quat_to_R, kin.c:348-370
template <typename real>
__device__ __forceinline__ void t_quat_to_R(const real q[4], real R[9])
{
   const real xx = q[0]*q[0], xy = q[0]*q[1], xz = q[0]*q[2], xw = q[0]*q[3];
   const real yy = q[1]*q[1], yz = q[1]*q[2], yw = q[1]*q[3], zz = q[2]*q[2], zw = q[2]*q[3];
   R[0] = 1 - 2*(yy+zz); R[1] = 2*(xy-zw);     R[2] = 2*(xz+yw);
   R[3] = 2*(xy+zw);     R[4] = 1 - 2*(xx+zz); R[5] = 2*(yz-xw);
   R[6] = 2*(xz-yw);     R[7] = 2*(yz+xw);     R[8] = 1 - 2*(xx+yy);
}
// cd_kin_quat_from_R, kin.c:418-459 (R row major): the largest of the four squared components is taken from the
// diagonal (ties go to the later one, as the reference's cascade of comparisons does), the other three from the
// sums and differences of the off-diagonal pairs
template <typename real>
__device__ __forceinline__ void t_quat_from_R(const real R[9], real quat[4])
{
   const real d4[4] = { 1 + R[0] - R[4] - R[8], 1 - R[0] + R[4] - R[8], 1 - R[0] - R[4] + R[8], 1 + R[0] + R[4] + R[8] };   // 4 x^2, 4 y^2, 4 z^2, 4 w^2
   // 4 x y, 4 x z, 4 y z, 4 w x, 4 w y, 4 w z
   const real pr[6] = { R[3] + R[1], R[2] + R[6], R[7] + R[5], R[7] - R[5], R[2] - R[6], R[3] - R[1] };
   int big = 0;
#pragma unroll
   for (int k=1; k<4; k++) if (d4[k] >= d4[big]) big = k;
   real dbig = d4[0];
#pragma unroll
   for (int k=1; k<4; k++) dbig = (big == k) ? d4[k] : dbig;
   const real qbig = M<real>::sqrt_((real)0.25 * dbig);
   const real v4 = (real)0.25 / qbig;
   // product of components a and b (a < b): index into pr
#pragma unroll
   for (int c=0; c<4; c++)
   {
      // pair (min(big, c), max(big, c)) -> (0,1) 0, (0,2) 1, (1,2) 2, (0,3) 3, (1,3) 4, (2,3) 5
      real v = 0;
#pragma unroll
      for (int o=0; o<4; o++)
      {
         if (o == c) continue;
         const int lo = o < c ? o : c, hi = o < c ? c : o;
         const int idx = (hi == 3) ? 3 + lo : lo + hi - 1;
         v = (big == o) ? pr[idx] : v;
      }
      quat[c] = (big == c) ? qbig : v4 * v;
   }
}
// cd_kin_pose_to_xyzypr, kin.c:615-646: yaw, pitch, roll of the quaternion; at the poles (|sin pitch| > 0.99998) the yaw
// takes the whole rotation about the vertical
template <typename real>
__device__ __forceinline__ void t_pose_to_xyzypr(const real pose[7], real o[6])
{
   const real qx = pose[3], qy = pose[4], qz = pose[5], qw = pose[6];
   const real quarter_turn = (real) 1.5707963267948966192313216916398;
   o[0] = pose[0]; o[1] = pose[1]; o[2] = pose[2];
   const real half_sinp = qw*qy - qz*qx;
   if (M<real>::fabs_(half_sinp) > (real)0.49999)
   {
      const real sgn = half_sinp > 0 ? (real)1 : (real)(-1);
      o[3] = (real)(-2) * sgn * TM<real>::atan2_(qx, qw); o[4] = sgn * quarter_turn; o[5] = 0;
      return;
   }
   o[3] = TM<real>::atan2_(2*(qw*qz + qx*qy), 1 - 2*(qy*qy + qz*qz));
   o[4] = TM<real>::asin_(2*half_sinp);
   o[5] = TM<real>::atan2_(2*(qw*qx + qy*qz), 1 - 2*(qx*qx + qy*qy));
}
// cd_kin_pose_to_xyzypr_J, kin.c:682-717: the derivative of the above by the pose.  An angle atan2(s, c) has the
// gradient (c grad s - s grad c) / (c^2 + s^2); the pitch asin(a) has grad a / sqrt(1 - a^2).
template <typename real>
__device__ __forceinline__ void t_xyzypr_J(const real pose[7], real J[6][7])
{
   const real qx = pose[3], qy = pose[4], qz = pose[5], qw = pose[6];
#pragma unroll
   for (int i=0; i<6; i++)
#pragma unroll
      for (int j=0; j<7; j++) J[i][j] = 0;
   J[0][0] = 1; J[1][1] = 1; J[2][2] = 1;
   auto angle_row = [](real s, real c, const real gs[4], const real gc[4], real * row) {
      const real inv = (real)1 / (c*c + s*s);
      const real wc = c * inv, ws = s * inv;
#pragma unroll
      for (int k=0; k<4; k++) row[k] = wc * gs[k] - ws * gc[k];
   };
   {  // yaw: s = 2 (qw qz + qx qy), c = 1 - 2 (qy^2 + qz^2); gradients by (qx, qy, qz, qw)
      const real gs[4] = { 2*qy, 2*qx, 2*qw, 2*qz }, gc[4] = { 0, (real)(-4)*qy, (real)(-4)*qz, 0 };
      angle_row(2*(qw*qz + qx*qy), 1 - 2*(qy*qy + qz*qz), gs, gc, &J[3][3]);
   }
   {  // pitch: asin(a), a = 2 (qw qy - qz qx)
      const real a = 2 * (qw*qy - qz*qx);
      const real ia2 = (real)2 / M<real>::sqrt_(1 - a*a);
      J[4][3] = -ia2*qz; J[4][4] = ia2*qw; J[4][5] = -ia2*qx; J[4][6] = ia2*qy;
   }
   {  // roll: s = 2 (qw qx + qy qz), c = 1 - 2 (qx^2 + qy^2)
      const real gs[4] = { 2*qw, 2*qz, 2*qy, 2*qx }, gc[4] = { (real)(-4)*qx, (real)(-4)*qy, 0, 0 };
      angle_row(2*(qw*qx + qy*qz), 1 - 2*(qx*qx + qy*qy), gs, gc, &J[5][3]);
   }
}
// a frame walking the joints of the end effector's chain (the build's own kinematic model, the one
// fk.h walks for the spheres): cur <- cur o (Rfix, tfix); world axis and anchor; cur <- cur o motion(q)
template <typename real>
struct TFrame { real R[9], t[3]; };
template <typename real, typename JT>
__device__ __forceinline__ void t_apply_joint(const JT & J, real q, TFrame<real> & cur, real axis_w[3], real anchor[3])
{
   real Rj[9], tj[3];
   real Rf[9], tf[3], ax[3];
#pragma unroll
   for (int e=0; e<9; e++) Rf[e] = J.Rfix[e];
#pragma unroll
   for (int e=0; e<3; e++) { tf[e] = J.tfix[e]; ax[e] = J.axis[e]; }
#pragma unroll
   for (int r=0; r<3; r++)
   {
#pragma unroll
      for (int c=0; c<3; c++) Rj[3*r+c] = cur.R[3*r+0]*Rf[0*3+c] + cur.R[3*r+1]*Rf[1*3+c] + cur.R[3*r+2]*Rf[2*3+c];
      tj[r] = cur.R[3*r+0]*tf[0] + cur.R[3*r+1]*tf[1] + cur.R[3*r+2]*tf[2] + cur.t[r];
   }
#pragma unroll
   for (int r=0; r<3; r++)
   {
      axis_w[r] = Rj[3*r+0]*ax[0] + Rj[3*r+1]*ax[1] + Rj[3*r+2]*ax[2];
      anchor[r] = tj[r];
   }
   if (J.type == 1)
   {
      real sn, cs;
      sincos_joint(q, &sn, &cs);      // (fk.h: the short kernel the FK phase uses, ~1 ulp: the library call carries a large-argument path several times its length)
      const real v = (real)1 - cs;
      const real a0 = ax[0], a1 = ax[1], a2 = ax[2];
      real Rm[9];
      Rm[0] = cs + a0*a0*v;    Rm[1] = a0*a1*v - a2*sn; Rm[2] = a0*a2*v + a1*sn;
      Rm[3] = a1*a0*v + a2*sn; Rm[4] = cs + a1*a1*v;    Rm[5] = a1*a2*v - a0*sn;
      Rm[6] = a2*a0*v - a1*sn; Rm[7] = a2*a1*v + a0*sn; Rm[8] = cs + a2*a2*v;
#pragma unroll
      for (int r=0; r<3; r++)
#pragma unroll
         for (int c=0; c<3; c++) cur.R[3*r+c] = Rj[3*r+0]*Rm[0*3+c] + Rj[3*r+1]*Rm[1*3+c] + Rj[3*r+2]*Rm[2*3+c];
#pragma unroll
      for (int r=0; r<3; r++) cur.t[r] = tj[r];
   }
   else
   {
#pragma unroll
      for (int e=0; e<9; e++) cur.R[e] = Rj[e];
#pragma unroll
      for (int r=0; r<3; r++) cur.t[r] = tj[r] + q*axis_w[r];
   }
}

// con_tsr (src/orcdchomp_mod.cpp:1330-1497) at one trajectory row: h[k] and J[k][n] of the enabled rows.
// One lane = one point.  Everything a lane keeps is indexed at compile time (registers: a table indexed by a loop counter is
// a table in scratch memory, 2.4 KB of it per lane until round 4), the joints' constants come by scalar loads, and only the
// enabled rows of the chain of Jacobians are formed -- row `row` of
//    B = (xyzypr-Jacobian . pose-Jacobian-inverse)(pose) . spatial transform(table_world)        (mod.cpp:1466-1480)
// with the sums in the order the full 6 x 7 . 7 x 6 . 6 x 6 products take them (their other terms are exact zeros).
// KMAX: the most rows a lane holds (3 or 6: six rows of B next to the walk's frames do not fit the register budget).
// aws: [nj][6][astride] workspace in global memory, this lane's column `slot`: the world axis and anchor of every joint of the chain,
// written by the walk and read back when the rows of B are known (round 6).  Until then the chain was walked TWICE -- the rows
// of B need the end effector's pose, the Jacobian columns the joints' axes -- with the first walk's base frame and the second walk's
// temporaries alive next to B: 596 bytes of scratch per lane, 194 stores and 476 loads per call at the 128-register budget, a third
// of the constrained lines' HBM traffic (profiles/r06_tsr1_summary.json before / after).
template <typename real, int KMAX>
__device__ __forceinline__ void tsr_eval_point_k(const DevModel<real> & gm, const DevTsr<real> & ts, const real * point, int n, real * hrow, real * Jrows,
   real * aws, int astride, int slot)
{
   typedef const __attribute__((address_space(4))) DevJoint<real> JointC;
   JointC * joints = (JointC *) gm.joints;
   const int nj = __builtin_amdgcn_readfirstlane(gm.nj);
   TFrame<real> cur;
   if (gm.floating)
   {
      const real q[4] = { point[3], point[4], point[5], point[6] };
      t_quat_to_R(q, cur.R);
      cur.t[0] = point[0]; cur.t[1] = point[1]; cur.t[2] = point[2];
   }
   else
   {
#pragma unroll
      for (int e=0; e<9; e++) cur.R[e] = gm.base_R[e];
#pragma unroll
      for (int e=0; e<3; e++) cur.t[e] = gm.base_t[e];
   }
   // the end-effector link's frame: walk its chain (every joint's world axis and anchor go to the workspace), then the fixed
   // transform to the link
   typedef __attribute__((address_space(1))) real * GlobalW;
   GlobalW awg = (GlobalW) aws + slot;
   real aw[3], an[3];
   for (int j=0; j<nj; j++)
      if ((ts.chain_mask >> j) & 1u)
      {
         t_apply_joint<real>(joints[j], point[joints[j].col], cur, aw, an);
#pragma unroll
         for (int q=0; q<3; q++) { awg[(size_t)(j*6 + q) * astride] = aw[q]; awg[(size_t)(j*6 + 3 + q) * astride] = an[q]; }
      }
   real Rl[9], tl[3];
#pragma unroll
   for (int r=0; r<3; r++)
   {
#pragma unroll
      for (int c=0; c<3; c++) Rl[3*r+c] = cur.R[3*r+0]*ts.Xl_R[0*3+c] + cur.R[3*r+1]*ts.Xl_R[1*3+c] + cur.R[3*r+2]*ts.Xl_R[2*3+c];
      tl[r] = cur.R[3*r+0]*ts.Xl_t[0] + cur.R[3*r+1]*ts.Xl_t[1] + cur.R[3*r+2]*ts.Xl_t[2] + cur.t[r];
   }
   real pose_link[7], pose_ee[7], pose_obj[7], P[7], xyzypr[6], tool[7], ee_obj[7], tw[7];
#pragma unroll
   for (int e=0; e<7; e++) { tool[e] = ts.tool[e]; ee_obj[e] = ts.ee_obj[e]; tw[e] = ts.table_world[e]; }
   pose_link[0] = tl[0]; pose_link[1] = tl[1]; pose_link[2] = tl[2];
   t_quat_from_R(Rl, pose_link+3);
   t_pose_compose(pose_link, tool, pose_ee);                 // GetEndEffectorTransform (mod.cpp:1382-1394)
   t_pose_compose(pose_ee, ee_obj, pose_obj);                // mod.cpp:1396-1398
   t_pose_compose(tw, pose_obj, P);                          // mod.cpp:1400-1404: the object in the TSR's frame
   t_pose_to_xyzypr(P, xyzypr);
   // the enabled rows, three bits each (xyzypr order: x y z yaw pitch roll <- Bw rows x y z roll pitch yaw)
   unsigned int rowpack = 0; int k = 0;
#pragma unroll
   for (int tsri=0; tsri<6; tsri++) if (ts.enabled[tsri]) { rowpack |= (unsigned int)(tsri<3?tsri:8-tsri) << (3*k); k++; }
   // what the rows of B are made of
   real R[9], rxR[9];                           // spatial transform of table_world: [R 0; [r]x R  R]   (spatial.c:71-102)
   t_quat_to_R(tw+3, R);
   {
      const real rx[9] = { 0, -tw[2], tw[1],  tw[2], 0, -tw[0],  -tw[1], tw[0], 0 };
#pragma unroll
      for (int i=0; i<3; i++)
#pragma unroll
         for (int j=0; j<3; j++) { real s = 0; for (int q=0; q<3; q++) s += rx[3*i+q] * R[3*q+j]; rxR[3*i+j] = s; }
   }
   real Jx[6][7];
   t_xyzypr_J(P, Jx);                           // rows 3..5, columns 3..6 are what is not 0 or 1 (kin.c:682-717)
   const real x = P[0], y = P[1], z = P[2];
   const real qxd2 = (real)0.5*P[3], qyd2 = (real)0.5*P[4], qzd2 = (real)0.5*P[5], qwd2 = (real)0.5*P[6];
   // pose-Jacobian-inverse (spatial.c:339-375): rows 0..2 = [[r]x | I], rows 3..6 = the quaternion part, columns 0..2
   const real Jiq[4][3] = { { qwd2, qzd2, -qyd2 }, { -qzd2, qwd2, qxd2 }, { qyd2, -qxd2, qwd2 }, { -qxd2, -qyd2, -qzd2 } };
   real B[KMAX][6];
#pragma unroll
   for (int ki=0; ki<KMAX; ki++)
   {
#pragma unroll
      for (int j=0; j<6; j++) B[ki][j] = 0;
      if (ki < k)
      {
         const int row = (rowpack >> (3*ki)) & 7u;
         real hv = xyzypr[0];
#pragma unroll
         for (int e=1; e<6; e++) hv = (row == e) ? xyzypr[e] : hv;
         hrow[ki] = hv;
         real a[6];
         if (row < 3)
         {
            a[0] = (row == 0) ? (real)0 : ((row == 1) ? -z : y);
            a[1] = (row == 0) ? z : ((row == 1) ? (real)0 : -x);
            a[2] = (row == 0) ? -y : ((row == 1) ? x : (real)0);
            a[3] = (row == 0) ? (real)1 : (real)0; a[4] = (row == 1) ? (real)1 : (real)0; a[5] = (row == 2) ? (real)1 : (real)0;
         }
         else
         {
            real g[4];
#pragma unroll
            for (int q=0; q<4; q++) g[q] = (row == 3) ? Jx[3][3+q] : ((row == 4) ? Jx[4][3+q] : Jx[5][3+q]);
#pragma unroll
            for (int c=0; c<3; c++) { real s = 0; for (int q=0; q<4; q++) s += g[q] * Jiq[q][c]; a[c] = s; }
            a[3] = 0; a[4] = 0; a[5] = 0;
         }
#pragma unroll
         for (int j=0; j<3; j++)
         {
            real s = 0;
#pragma unroll
            for (int i=0; i<3; i++) s += a[i] * R[3*i+j];
#pragma unroll
            for (int i=0; i<3; i++) s += a[3+i] * rxR[3*i+j];
            B[ki][j] = s;
            real u = 0;
#pragma unroll
            for (int i=0; i<3; i++) u += a[3+i] * R[3*i+j];
            B[ki][3+j] = u;
         }
      }
   }
   for (int e=0; e<k*n; e++) Jrows[e] = 0;
   // . spatial Jacobian, column by column (mod.cpp:1432-1464, 1481-1491)
   if (gm.floating)
   {
      // cd_spatial_pose_jac(point), spatial.c:295-337: the first seven columns
      const real px = point[0], py = point[1], pz = point[2];
      const real qx = 2*point[3], qy = 2*point[4], qz = 2*point[5], qw = 2*point[6];
      const real Jsp[6][7] = {
         { 0, 0, 0,  qw, -qz,  qy, -qx },
         { 0, 0, 0,  qz,  qw, -qx, -qy },
         { 0, 0, 0, -qy,  qx,  qw, -qz },
         { 1, 0, 0, -pz*qz - py*qy, -pz*qw + py*qx,  pz*qx + py*qw,  pz*qy - py*qz },
         { 0, 1, 0,  pz*qw + px*qy, -pz*qz - px*qx,  pz*qy - px*qw, -pz*qx + px*qz },
         { 0, 0, 1, -py*qw + px*qz,  py*qz + px*qw, -py*qy - px*qx,  py*qx - px*qy } };
#pragma unroll
      for (int c=0; c<7; c++)
#pragma unroll
         for (int ki=0; ki<KMAX; ki++) if (ki < k)
         {
            real s = 0;
#pragma unroll
            for (int q=0; q<6; q++) s += B[ki][q] * Jsp[q][c];
            Jrows[ki*n + c] = s;
         }
   }
   for (int j=0; j<nj; j++)
      if ((ts.chain_mask >> j) & 1u)
      {
         JointC & J = joints[j];
         const int col = J.col;
#pragma unroll
         for (int q=0; q<3; q++) { aw[q] = awg[(size_t)(j*6 + q) * astride]; an[q] = awg[(size_t)(j*6 + 3 + q) * astride]; }
         real col6[6];
         if (J.type == 1)
         {
            // angular part: the axis; linear part: velocity of the link's point at the world origin, axis x (0 - anchor)
            col6[0] = aw[0]; col6[1] = aw[1]; col6[2] = aw[2];
            col6[3] = aw[1]*(-an[2]) - aw[2]*(-an[1]);
            col6[4] = aw[2]*(-an[0]) - aw[0]*(-an[2]);
            col6[5] = aw[0]*(-an[1]) - aw[1]*(-an[0]);
         }
         else { col6[0] = 0; col6[1] = 0; col6[2] = 0; col6[3] = aw[0]; col6[4] = aw[1]; col6[5] = aw[2]; }
#pragma unroll
         for (int ki=0; ki<KMAX; ki++) if (ki < k)
         {
            real s = 0;
#pragma unroll
            for (int q=0; q<6; q++) s += B[ki][q] * col6[q];
            Jrows[ki*n + col] = s;
         }
      }
}
template <typename real>
__device__ void tsr_eval_point(const DevModel<real> & gm, const DevTsr<real> & ts, const real * point, int n, real * hrow, real * Jrows,
   real * aws, int astride, int slot)
{
   if (ts.k <= 3) tsr_eval_point_k<real, 3>(gm, ts, point, n, hrow, Jrows, aws, astride, slot);
   else tsr_eval_point_k<real, 6>(gm, ts, point, n, hrow, Jrows, aws, astride, slot);
}
