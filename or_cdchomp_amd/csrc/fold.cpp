// fold.cpp -- the folds of `create` (stages.h): the robot into DevModel, the TSR constraints into DevTsr, the scene table into
// DevSdf / DevSdfCell rows, the metric into its device tables.  Host arithmetic only; BatchShard::construct uploads the results.
#include "stages.h"
#include "kernel_table.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <stdexcept>

namespace orc {

Switches Switches::read()
{
   Switches s;
   auto on = [](const char * name) { return getenv(name) != nullptr; };
   auto num = [](const char * name) { Int v; if (const char * e = getenv(name)) { v.set = true; v.value = atoi(e); } return v; };
   auto num_or = [&num](const char * name, int otherwise) { const Int v = num(name); return v.set ? v.value : otherwise; };
   s.debug_plan = on("ORC_DEBUG_PLAN"); s.phase_timers = on("ORC_PHASE_TIMERS"); s.debug_state = on("ORC_DEBUG_STATE");
   s.hmc_device = on("ORC_HMC_DEVICE"); s.hmc_host = on("ORC_HMC_HOST"); s.hmc_plan_sync = on("ORC_HMC_PLAN_SYNC");
   s.no_jt_scan = on("ORC_NO_JT_SCAN"); s.no_placement = on("ORC_NO_PLACEMENT"); s.no_static_lanes = on("ORC_NO_STATIC_LANES");
   s.pairs_chain64_only = on("ORC_PAIRS_CHAIN64_ONLY"); s.no_pairs = on("ORC_NO_PAIRS"); s.no_kind = on("ORC_NO_KIND");
   s.no_fk_split = on("ORC_NO_FK_SPLIT"); s.no_semisep = on("ORC_NO_SEMISEP"); s.no_scan_solve = on("ORC_NO_SCAN_SOLVE");
   s.pcr_full = on("ORC_PCR_FULL"); s.no_short128 = on("ORC_NO_SHORT128"); s.no_band_toeplitz = on("ORC_NO_BAND_TOEPLITZ");
   s.tsr_dense = on("ORC_TSR_DENSE");
   const Int staged = num("ORC_T_STAGED");
   s.t_staged_off = staged.set && staged.value == 0;
   s.lim_generic = num_or("ORC_LIM_GENERIC", 0); s.stagger_mode = num_or("ORC_STAGGER_MODE", 0); s.stagger_sleeps = num_or("ORC_STAGGER_SLEEPS", 10);
   s.wave_rotate = num_or("ORC_WAVE_ROTATE", 0);
   s.scan_max_m = num_or("ORC_SCAN_MAX_M", 1 << 30); s.wgs128 = num_or("ORC_WGS128", 8);
   s.block_threads = num("ORC_BLOCK_THREADS"); s.tile_m = num("ORC_TILE_M"); s.pcr_lds = num("ORC_PCR_LDS"); s.ag_lds = num("ORC_AG_LDS");
   s.wgs = num("ORC_WGS"); s.g_lds = num("ORC_G_LDS"); s.t_lds = num("ORC_T_LDS"); s.hmc_room = num("ORC_HMC_ROOM");
   return s;
}

// ================================================================ the joint tree ===
int JointTree::attach_of(const Robot & robot, int link) const
{
   for (int li=link; li>=0; li=robot.parent[li]) if (link2joint[li] >= 0) return link2joint[li];
   return -1;
}

JointTree fold_joint_tree(const Robot & robot, bool floating_base)
{
   JointTree T;
   const int n_adof = (int) robot.active_dofs.size();
   const int col0 = floating_base ? 7 : 0;
   // optimized joints = links whose joint moves with an active dof
   T.link2joint.assign(robot.n_links, -1);
   for (int li=0; li<robot.n_links; li++)
   {
      if (robot.joint_type[li] == 0) continue;
      for (int j=0; j<n_adof; j++)
         if (robot.active_dofs[j] == robot.dof_index[li])
         {
            for (int lk : T.jlink)
               if (robot.dof_index[lk] == robot.dof_index[li])
                  throw std::runtime_error("two joints share one active dof (mimic joints are not supported)!");
            T.link2joint[li] = (int) T.jlink.size();
            T.jlink.push_back(li); T.jcol.push_back(col0 + j);
         }
   }
   const int nj = T.nj();
   if (nj > ORC_MAX_JOINTS) throw std::runtime_error("too many active joints for this build!");
   for (int k=0; k<nj; k++) T.canon.push_back(canonical_rotation(&robot.axis[3*T.jlink[k]]));
   T.jparent.resize(nj);
   for (int k=0; k<nj; k++)
   {
      const int pl = robot.parent[T.jlink[k]];
      T.jparent[k] = (pl >= 0) ? T.attach_of(robot, pl) : -1;
   }
   // depth-first order over the joint tree with save/restore slots for branch points
   T.children.resize(nj);
   for (int k=0; k<nj; k++) { if (T.jparent[k] < 0) T.roots.push_back(k); else T.children[T.jparent[k]].push_back(k); }
   T.load_slot.assign(nj, -1); T.save_slot.assign(nj, -1);
   // A branch point's frame is kept in a slot while all of its subtrees but the last are walked; the last takes it out of
   // the slot.  Walking the subtree that needs the most slots last (a stable sort: robots whose subtrees need the same
   // keep their order) bounds the slots by the tree's Strahler number, <= log2(joints + 1): four for any tree of 30.
   std::vector<int> need(nj, 0);
   std::function<int(int)> slots_needed = [&](int k) -> int
   {
      std::vector<int> & ch = T.children[k];
      for (int c : ch) slots_needed(c);
      std::stable_sort(ch.begin(), ch.end(), [&](int a, int b) { return need[a] < need[b]; });
      int v = 0;
      for (size_t c=0; c<ch.size(); c++) v = std::max(v, need[ch[c]] + ((c + 1 < ch.size()) ? 1 : 0));
      return need[k] = v;
   };
   for (int rk : T.roots) slots_needed(rk);
   int open_slots = 0;
   std::function<void(int)> visit = [&](int k)
   {
      T.order.push_back(k);
      const size_t nc = T.children[k].size();
      if (nc > 1)
      {
         if (open_slots >= ORC_MAX_SAVE) throw std::runtime_error("kinematic tree branches too deeply for this build!");
         T.save_slot[k] = open_slots++;
      }
      for (size_t c=0; c<nc; c++)
      {
         if (nc > 1 && c + 1 == nc) open_slots--;
         T.load_slot[T.children[k][c]] = (c == 0) ? -1 : T.save_slot[k];
         visit(T.children[k][c]);
      }
   };
   for (int rk : T.roots) { T.load_slot[rk] = -2; visit(rk); }
   T.pos_in_order.resize(nj);
   for (int k=0; k<nj; k++) T.pos_in_order[T.order[k]] = k;
   return T;
}

Xform local_moved(const Robot & robot, int li)
{
   Xform x = xform_from_pose(robot.pose_parent_joint[li]);
   if (robot.joint_type[li] == 1)
   {
      Xform rot; rot.R = axis_angle(&robot.axis[3*li], robot.dof_values[robot.dof_index[li]]);
      rot.t[0] = rot.t[1] = rot.t[2] = 0.0;
      x = xform_mul(x, rot);
   }
   else if (robot.joint_type[li] == 2)
   {
      double aw[3];
      mat3_vec(x.R, &robot.axis[3*li], aw);
      for (int q=0; q<3; q++) x.t[q] += robot.dof_values[robot.dof_index[li]] * aw[q];
   }
   return x;
}

Xform fixed_between(const Robot & robot, int from_link, int li)
{
   Xform x = xform_from_pose(robot.pose_parent_joint[li]);
   for (int cur=robot.parent[li]; cur!=from_link && cur>=0; cur=robot.parent[cur])
      x = xform_mul(local_moved(robot, cur), x);
   return x;
}

void point_in(const Robot & robot, int from_link, int li, const double * pin, double * pout)
{
   double pt[3] = { pin[0], pin[1], pin[2] };
   for (int cur=li; cur!=from_link && cur>=0; cur=robot.parent[cur])
   {
      const Xform x = local_moved(robot, cur);
      double r[3];
      mat3_vec(x.R, pt, r);
      for (int q=0; q<3; q++) pt[q] = r[q] + x.t[q];
   }
   pout[0] = pt[0]; pout[1] = pt[1]; pout[2] = pt[2];
}

// ================================================================ canonical joint frames ===
// The FK walk (fk.h) turns every joint about z.  The fold re-expresses the moved frame F_j of every optimized joint as
// F'_j = F_j C_j with a constant rotation C_j, C_j e_z = axis_j (C = I for the base):
//    Rfix'_j = C_parent^T Rfix_j C_j,   tfix'_j = C_parent^T tfix_j,   axis'_j = (0, 0, 1),
// and everything that is stored in a joint's moved frame (sphere centres, the TSR's link frame) is multiplied by C_j^T on the
// host.  World quantities -- sphere centres, joint axes, anchors, the end effector's pose -- are what they were.
Mat3 canonical_rotation(const double axis[3])
{
   Mat3 C;
   for (int q=0; q<9; q++) C.m[q] = 0.0;
   // +- a coordinate axis: a signed permutation of determinant +1, so that the fold's products stay exact
   // (columns: +x (y z x), -x (z y -x), +y (z x y), -y (x z -y), +z (x y z), -z (x -y -z))
   for (int q=0; q<3; q++)
      if (std::fabs(axis[q]) == 1.0 && axis[(q+1)%3] == 0.0 && axis[(q+2)%3] == 0.0)
      {
         const bool neg = axis[q] < 0.0;
         const int c0 = neg ? (q == 2 ? 0 : (q+2)%3) : (q+1)%3, c1 = neg ? (q == 2 ? 1 : (q+1)%3) : (q+2)%3;
         C.m[c0*3+0] = 1.0; C.m[c1*3+1] = (neg && q == 2) ? -1.0 : 1.0; C.m[q*3+2] = axis[q];
         return C;
      }
   // a general axis, in extended precision: z = the axis; x = the coordinate axis along which the axis has its smallest component
   // (the first of equals), made orthogonal to z; y = z x x.  One more Gram-Schmidt pass, then rounded.
   long double z[3] = { axis[0], axis[1], axis[2] }, x[3] = { 0.0L, 0.0L, 0.0L }, y[3];
   auto dot = [](const long double * a, const long double * b) { return a[0]*b[0] + a[1]*b[1] + a[2]*b[2]; };
   auto unit = [&dot](long double * a) { const long double n = std::sqrt(dot(a, a)); for (int q=0; q<3; q++) a[q] /= n; };
   if (!(dot(z, z) > 0.0L)) throw std::runtime_error("a joint axis of zero length!");
   unit(z);
   int least = 0;
   for (int q=1; q<3; q++) if (std::fabs(z[q]) < std::fabs(z[least])) least = q;
   x[least] = 1.0L;
   for (int pass=0; pass<2; pass++)
   {
      const long double xz = dot(x, z);
      for (int q=0; q<3; q++) x[q] -= xz * z[q];
      unit(x);
   }
   y[0] = z[1]*x[2] - z[2]*x[1]; y[1] = z[2]*x[0] - z[0]*x[2]; y[2] = z[0]*x[1] - z[1]*x[0];
   unit(y);
   for (int q=0; q<3; q++) { C.m[q*3+0] = (double) x[q]; C.m[q*3+1] = (double) y[q]; C.m[q*3+2] = (double) z[q]; }
   return C;
}

namespace { const Mat3 IDENTITY3 = { { 1.0, 0.0, 0.0,  0.0, 1.0, 0.0,  0.0, 0.0, 1.0 } }; }
const Mat3 & JointTree::canonical(int k) const { return (k >= 0) ? canon[k] : IDENTITY3; }

namespace {
// C^T v and C^T R D, summed in extended precision and rounded once (a signed permutation leaves every entry as it was)
void canon_vec(const Mat3 & C, const double v[3], double out[3])
{
   for (int c=0; c<3; c++) out[c] = (double)((long double) C.m[0*3+c]*v[0] + (long double) C.m[1*3+c]*v[1] + (long double) C.m[2*3+c]*v[2]);
}
Mat3 canon_mat(const Mat3 & C, const Mat3 & R, const Mat3 & D)
{
   long double RD[9];
   for (int r=0; r<3; r++) for (int c=0; c<3; c++)
      RD[r*3+c] = (long double) R.m[r*3+0]*D.m[0*3+c] + (long double) R.m[r*3+1]*D.m[1*3+c] + (long double) R.m[r*3+2]*D.m[2*3+c];
   Mat3 out;
   for (int r=0; r<3; r++) for (int c=0; c<3; c++)
      out.m[r*3+c] = (double)((long double) C.m[0*3+r]*RD[0*3+c] + (long double) C.m[1*3+r]*RD[1*3+c] + (long double) C.m[2*3+r]*RD[2*3+c]);
   return out;
}
}

// ================================================================ lanes of the self-collision term ===
namespace {

// how often a pair of the given spheres (XML indices) is within self-collision range: fixed-seed configurations of the active
// dofs inside their limits, the other dofs frozen where the robot has them.  freq[a*Sa + b] for a < b; pairs of one link: 0.
// (`next`: the caller's generator; the placement search goes on with it)
template <typename Rng>
void pair_range_frequencies(const Robot & robot, double eps_self, const std::vector<int> & xml, Rng & next, std::vector<double> & freq)
{
   const int Sa = (int) xml.size();
   const int n_adof = (int) robot.active_dofs.size();
   const int n_samples = 384;
   freq.assign((size_t) Sa * Sa, 0.0);
   std::vector<double> q = robot.dof_values;
   std::vector<Xform> frames;
   std::vector<double> pw((size_t) Sa * 3);
   Pose origin;                                  // the base pose moves all spheres alike
   for (int it=0; it<n_samples; it++)
   {
      for (int j=0; j<n_adof; j++)
      {
         const int d = robot.active_dofs[j];
         double lo = robot.limit_lower[d], hi = robot.limit_upper[d];
         if (!(lo > -1e30)) lo = -3.14159265358979;
         if (!(hi < 1e30)) hi = 3.14159265358979;
         q[d] = lo + (hi - lo) * next();
      }
      robot.fk(origin, q, frames);
      for (int s=0; s<Sa; s++)
      {
         const Robot::Sphere & sp = robot.spheres[xml[s]];
         double r[3];
         mat3_vec(frames[sp.link].R, sp.pos, r);
         for (int k=0; k<3; k++) pw[(size_t) s*3+k] = r[k] + frames[sp.link].t[k];
      }
      for (int a=0; a<Sa; a++) for (int b=a+1; b<Sa; b++)
      {
         const Robot::Sphere & sa = robot.spheres[xml[a]], & sb = robot.spheres[xml[b]];
         if (sa.link == sb.link) continue;
         double d2 = 0;
         for (int k=0; k<3; k++) { const double d = pw[(size_t) a*3+k] - pw[(size_t) b*3+k]; d2 += d*d; }
         const double R = sa.radius + sb.radius + eps_self;
         if (d2 <= R*R) freq[(size_t) a*Sa+b] += 1.0 / n_samples;
      }
   }
}

// The dense self-collision pair list of the 32-lane kernel family (cost_pairs.h, DevModel::pr_*).  `xml`: the spheres on the
// lanes of a waypoint's group, the n_active active ones first, then inactive ones carried on free lanes.  Every pair that can
// count (different links, not both inactive) gets one entry; entries are handed out in the order of how often the pair is within
// range, each to the earliest round that has a lane left (the last lane of a round never holds a pair: its force is an
// exact zero, which the unused gather entries of a sphere point at) and in which both of its spheres still have a gather
// entry free on the side the pair gives them (ORC_PAIR_DEG adding, ORC_PAIR_DEG subtracting): the pair is turned round
// when that helps.  A pure function of the robot, the active dofs and eps_self (like the placement of the 16-lane rows):
// the order in which a sphere's pair forces are added up must not depend on what shares the batch.
// Returns the rounds in use, 0 when the list does not fit ORC_PAIR_ROUNDS.
struct PairTable { int rounds = 0, hot = 0; std::vector<int> ab, gat; std::vector<double> rsum; unsigned long long deg[2] = { 0ull, 0ull }; int n_pairs = 0; double expected_rounds = 0.0; };
PairTable build_pair_table(const Robot & robot, double eps_self, const std::vector<int> & xml, int n_active, int GS, bool debug)
{
   PairTable T;
   const int L = (int) xml.size();
   unsigned long long rng = 0x9E3779B97F4A7C15ull;
   auto next = [&rng]() { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (double)(rng >> 11) * (1.0 / 9007199254740992.0); };
   std::vector<double> freq;
   pair_range_frequencies(robot, eps_self, xml, next, freq);
   struct Cand { int a, b; double f; };
   std::vector<Cand> cand;
   for (int a=0; a<L; a++) for (int b=a+1; b<L; b++)
   {
      if (robot.spheres[xml[a]].link == robot.spheres[xml[b]].link) continue;      // src/orcdchomp_mod.cpp:1255-1256
      if (a >= n_active && b >= n_active) continue;                                 // two spheres that stand still
      cand.push_back({ a, b, freq[(size_t) a*L + b] });
   }
   std::stable_sort(cand.begin(), cand.end(), [](const Cand & x, const Cand & y) { return x.f > y.f; });
   const int per_round = GS - 1;
   std::vector<int> used(ORC_PAIR_ROUNDS, 0);
   std::vector<int> plus((size_t) ORC_PAIR_ROUNDS * GS, 0), minus((size_t) ORC_PAIR_ROUNDS * GS, 0);
   T.ab.assign((size_t) ORC_PAIR_ROUNDS * 32, 0); T.gat.assign((size_t) ORC_PAIR_ROUNDS * 32 * 2, 0); T.rsum.assign((size_t) ORC_PAIR_ROUNDS * 32, 0.0);
   // gather entries: word 0 adding, word 1 subtracting, a byte each; all of them start at the round's last lane
   for (size_t e=0; e<T.gat.size(); e++) { const int z = (GS - 1) * 4; T.gat[e] = z | (z << 8) | (z << 16) | (z << 24); }
   std::vector<double> none(ORC_PAIR_ROUNDS, 1.0);      // probability that no pair of the round is within range (two waypoints per wavefront: squared below)
   for (const Cand & c : cand)
   {
      int r = 0, first = c.a, second = c.b;
      for (; r<ORC_PAIR_ROUNDS; r++)
      {
         if (used[r] >= per_round) continue;
         const bool fwd = plus[(size_t) r*GS + c.a] < ORC_PAIR_DEG && minus[(size_t) r*GS + c.b] < ORC_PAIR_DEG;
         const bool rev = plus[(size_t) r*GS + c.b] < ORC_PAIR_DEG && minus[(size_t) r*GS + c.a] < ORC_PAIR_DEG;
         if (!fwd && !rev) continue;
         // the orientation that leaves the spheres' sides more evenly used
         const int load_f = plus[(size_t) r*GS + c.a] + minus[(size_t) r*GS + c.b], load_r = plus[(size_t) r*GS + c.b] + minus[(size_t) r*GS + c.a];
         if (!fwd || (rev && load_r < load_f)) { first = c.b; second = c.a; }
         break;
      }
      if (r == ORC_PAIR_ROUNDS) return PairTable();
      const int k = used[r]++;
      const size_t e = (size_t) r*32 + k;
      T.ab[e] = first | (second << 8);
      T.rsum[e] = robot.spheres[xml[first]].radius + robot.spheres[xml[second]].radius;
      int & gp = T.gat[((size_t) r*32 + first)*2 + 0];  const int np_ = plus[(size_t) r*GS + first]++;
      gp = (int)(((unsigned int) gp & ~(0xffu << (8*np_))) | ((unsigned int)(k*4) << (8*np_)));
      int & gm = T.gat[((size_t) r*32 + second)*2 + 1]; const int nm_ = minus[(size_t) r*GS + second]++;
      gm = (int)(((unsigned int) gm & ~(0xffu << (8*nm_))) | ((unsigned int)(k*4) << (8*nm_)));
      none[r] *= (1.0 - c.f);
      if (c.f > 0.95 && r + 1 > T.hot) T.hot = r + 1;
      if (r + 1 > T.rounds) T.rounds = r + 1;
      T.n_pairs++;
   }
   for (int r=0; r<T.rounds; r++)
   {
      int dp = 0, dm = 0;
      for (int q=0; q<GS; q++) { dp = std::max(dp, plus[(size_t) r*GS + q]); dm = std::max(dm, minus[(size_t) r*GS + q]); }
      T.deg[r >> 3] |= (unsigned long long)(dp | (dm << 4)) << (8*(r & 7));
      T.expected_rounds += 1.0 - std::pow(none[r], 64 / GS);
   }
   if (debug)
   {
      fprintf(stderr, "orc pair list: %d pairs of %d lanes in %d rounds of %d, %d of them always evaluated; expected force evaluations per wavefront pass %.2f; pairs per round", T.n_pairs, L, T.rounds, per_round, T.hot, T.expected_rounds);
      for (int r=0; r<T.rounds; r++) fprintf(stderr, " %d", used[r]);
      fprintf(stderr, "\n");
   }
   return T;
}

// Placement of the active spheres (given by XML index, sorted by joint) on the 16 lanes of a DPP
// row.  Rotation K of the self-collision term costs its force evaluation whenever some pair of
// spheres K lanes apart is within range in any of the four waypoints of a wavefront; pairs are
// within range mostly for structural reasons (neighbouring links, a hand's fingers), so their
// frequencies are estimated from fixed-seed configurations of the active dofs inside their limits
// (the other dofs frozen where the robot has them) and a seeded annealing run looks for the
// placement with the fewest expected evaluations.  Returns slot[k] for the k-th sphere; the
// identity when nothing better than the sorted order is found.  The placement fixes the order in
// which a sphere's pair forces are added up, so it must not depend on what shares the batch: it is a
// pure function of the robot (geometry, limits, frozen dof values), the active dofs and eps_self.
// Every pair is visited exactly once whatever the placement.
std::vector<int> place_spheres_on_row(const Robot & robot, double eps_self, const std::vector<int> & xml, bool debug)
{
   const int Sa = (int) xml.size();
   std::vector<int> ident(Sa);
   for (int s=0; s<Sa; s++) ident[s] = s;
   if (Sa > 16) return ident;
   unsigned long long rng = 0x9E3779B97F4A7C15ull;
   auto next = [&rng]() { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (double)(rng >> 11) * (1.0 / 9007199254740992.0); };
   // frequencies of "within range" per pair
   std::vector<double> freq;
   pair_range_frequencies(robot, eps_self, xml, next, freq);
   struct Pair { int a, b; double keep; };      // keep = probability that none of 4 waypoints has the pair in range
   std::vector<Pair> pairs;
   for (int a=0; a<Sa; a++) for (int b=a+1; b<Sa; b++)
      if (freq[(size_t) a*Sa+b] > 0.0)
      {
         const double f = freq[(size_t) a*Sa+b];
         pairs.push_back({ a, b, (1-f)*(1-f)*(1-f)*(1-f) });
      }
   auto cost = [&](const std::vector<int> & slot) {
      double none[9];
      for (int K=0; K<9; K++) none[K] = 1.0;
      for (const Pair & p : pairs)
      {
         int d = slot[p.a] - slot[p.b]; if (d < 0) d = -d; if (d > 8) d = 16 - d;
         none[d] *= p.keep;
      }
      double c = 0;
      for (int K=1; K<=8; K++) c += 1.0 - none[K];
      return c;
   };
   const double c_ident = cost(ident);
   std::vector<int> best = ident; double c_best = c_ident;
   for (int restart=0; restart<16; restart++)
   {
      // random start: a shuffle of the 16 slots
      int slots[16];
      for (int k=0; k<16; k++) slots[k] = k;
      for (int k=15; k>0; k--) { const int j = (int)(next() * (k+1)); std::swap(slots[k], slots[j]); }
      std::vector<int> cur(slots, slots + Sa);
      double c_cur = cost(cur), T = 0.5;
      for (int it=0; it<8000; it++, T *= 0.9993)
      {
         std::vector<int> cand = cur;
         const int i = (int)(next() * Sa);
         const int target = (int)(next() * 16);                 // a slot: swap with its owner, or move there if free
         int owner = -1;
         for (int k=0; k<Sa; k++) if (cand[k] == target) owner = k;
         if (owner >= 0) std::swap(cand[i], cand[owner]); else cand[i] = target;
         const double c = cost(cand);
         if (c < c_cur || next() < std::exp((c_cur - c) / T)) { cur.swap(cand); c_cur = c; }
         if (c_cur < c_best) { c_best = c_cur; best = cur; }
      }
   }
   if (debug)
   {
      fprintf(stderr, "orc placement: expected force evaluations per wavefront pass %.2f sorted -> %.2f placed; slots", c_ident, c_best);
      for (int s=0; s<Sa; s++) fprintf(stderr, " %d", best[s]);
      fprintf(stderr, "\n");
   }
   return (c_best < c_ident - 0.25) ? best : ident;
}

struct SphRef { int xml; int attach_pos; };    // attach_pos: -1 base, else position in DFS order

// where the spheres of a waypoint sit in its lane group
struct Lanes
{
   bool pairs = false;              // the 32-lane family with the dense pair list
   PairTable ptab;
   bool placed = false;             // the spheres are placed on the 16 lanes of a DPP row
   int n_static = 0;                // inactive spheres carried on free lanes
   int lanes = 0;                   // lanes of the active block
   std::vector<int> slot_of;        // lane of sorted sphere s (the active ones, then the static ones)
};

std::vector<int> xml_of_lanes(const std::vector<SphRef> & act, const std::vector<SphRef> & inact, int n_static)
{
   std::vector<int> xml_of(act.size() + n_static);
   for (size_t s=0; s<act.size(); s++) xml_of[s] = act[s].xml;
   for (int s=0; s<n_static; s++) xml_of[act.size() + s] = inact[s].xml;
   return xml_of;
}

// Lanes of the DPP row.  The self-collision term walks the row in rotations 1..8 and evaluates
// the forces of a rotation only when some pair at that lane distance is in range, so the spheres
// are placed on the 16 lanes such that the pairs that are usually in range share few distances
// (place_spheres_on_row).  Everything indexed by lane (pos, radius, link, affects) is in slot
// order; FK and the J^T ranges keep the order sorted by joint and go through slot_of.
// Inactive spheres on free lanes of the row (DevModel::static_*): as many as fit, in XML order; the rest
// stay in the loop over inactive spheres.  (The J^T code drops a static lane's force with the lanes past
// the active spheres of the placed, scanned layout: only then.)
Lanes choose_lanes(const Robot & robot, const BatchParams & params, const std::vector<SphRef> & act, const std::vector<SphRef> & inact,
   int GS, bool tree, int jt_scan, bool fp64, int asked_block, const Switches & sw, PlacementCache cache)
{
   Lanes L;
   const int Sa = (int) act.size();
   if (GS == 16 && Sa >= 4 && jt_scan != 0 && !sw.no_placement && !sw.no_static_lanes)
      L.n_static = std::min((int) inact.size(), 16 - Sa);
   // 17 .. 32 active spheres on a chain, fp64 (the robot that holds something): the 32-lane family with the dense
   // self-collision pair list (cost_pairs.h).  The spheres keep their sorted order; inactive ones ride on the free lanes.
   // Round 6: trees whose joints move contiguous ranges of the sorted spheres (jt_scan 2: a WAM with its finger dofs active) and
   // fp32 runs take the family too (256-thread workgroups; the latency shape stays an fp64 chain's)
   const bool pair_chain64 = fp64 && !tree && jt_scan == 1;
   const bool pair_other = GS == 32 && ((tree && jt_scan == 2) || (!tree && jt_scan == 1)) && !sw.pairs_chain64_only;
   // (the family is a function of the robot and the run, not of the latency shape asked for -- 512 threads, what the single-run
   // `create` asks for: where the family has no such kernel, a tree or an fp32 run, the planner drops the request, so that a run alone
   // has the bits it has inside a batch.  Any other shape asked for is binding: a robot whose pair-list family has no kernel of it
   // stays on the many-sphere family)
   const int pair_variant = robot_variant(tree, GS, params.floating_base != 0, jt_scan, false, 0, true, sw.no_kind);
   const bool pair_shape = asked_block == 0 || asked_block == 512 || kernel_exists(kernel_of(pair_variant, asked_block, fp64 ? 8 : 4));
   if ((pair_chain64 || pair_other) && GS == 32 && !params.free_start && pair_shape
       && !sw.no_pairs && !sw.no_kind && !sw.block_threads.set)
   {
      const int ns = sw.no_static_lanes ? 0 : std::min((int) inact.size(), GS - Sa);
      L.ptab = build_pair_table(robot, params.epsilon_self, xml_of_lanes(act, inact, ns), Sa, GS, sw.debug_plan);
      if (L.ptab.rounds > 0) { L.pairs = true; L.n_static = ns; }
   }
   L.slot_of.resize(Sa + L.n_static);
   for (int s=0; s<Sa+L.n_static; s++) L.slot_of[s] = s;
   L.lanes = Sa;
   if (GS == 16 && Sa >= 4 && !L.pairs && !sw.no_placement)
   {
      const std::string key = placement_key(robot, params, L.n_static);
      std::lock_guard<std::recursive_mutex> lock(cache.mutex);
      auto hit = cache.placed.find(key);
      if (hit == cache.placed.end() || (int) hit->second.size() != Sa + L.n_static)
         hit = cache.placed.insert_or_assign(key, place_spheres_on_row(robot, params.epsilon_self, xml_of_lanes(act, inact, L.n_static), sw.debug_plan)).first;
      const std::vector<int> & placed = hit->second;
      bool ident = true;
      for (int s=0; s<Sa+L.n_static; s++) if (placed[s] != s) ident = false;
      if (!ident || L.n_static > 0) { L.slot_of = placed; L.lanes = 16; L.placed = true; }
   }
   return L;
}

// the joints' records in the order of the walk: fixed transform from the parent joint's moved frame, axis, slots
template <typename real>
void fold_joints(DevModel<real> & M, const Robot & robot, const JointTree & T)
{
   for (int k=0; k<T.nj(); k++)
   {
      const int jk = T.order[k];
      DevJoint<real> & J = M.joints[k];
      const int li = T.jlink[jk];
      // from-frame: the moved frame of the parent optimized joint's link (or the base)
      const Xform fix = fixed_between(robot, (T.jparent[jk] < 0) ? -1 : T.jlink[T.jparent[jk]], li);
      // ... both in their canonical form (above): the joint turns about z of its own frame
      const Mat3 & Cp = T.canonical(T.jparent[jk]);
      const Mat3 Rc = canon_mat(Cp, fix.R, T.canonical(jk));
      double tc[3];
      canon_vec(Cp, fix.t, tc);
      for (int q=0; q<9; q++) J.Rfix[q] = (real) Rc.m[q];
      for (int q=0; q<3; q++) { J.tfix[q] = (real) tc[q]; J.axis[q] = (real)((q == 2) ? 1 : 0); }
      J.type = robot.joint_type[li];
      J.col = T.jcol[jk];
      J.load_slot = T.load_slot[jk];
      J.save_slot = T.save_slot[jk];
      if (T.save_slot[jk] >= 0 || T.load_slot[jk] >= 0 || (T.load_slot[jk] == -2 && k > 0)) M.tree = 1;
      J.sph_begin = 0; J.sph_end = 0;
   }
}

// the active spheres in device order (sorted by the joint they ride on), the joints' sphere ranges and packed words, and
// which spheres a joint moves as a range of the device order (J^T through wrench suffix sums: DevModel::jt_scan)
template <typename real>
void fold_active_spheres(DevModel<real> & M, const Robot & robot, const JointTree & T, const std::vector<SphRef> & act,
   std::vector<int> & device_sphere_order)
{
   const int nj = T.nj(), Sa = (int) act.size();
   for (int s=0; s<Sa; s++)
   {
      const Robot::Sphere & sp = robot.spheres[act[s].xml];
      const int ap = act[s].attach_pos;
      // position in the attach frame (frozen intermediate joints folded in), the frame in its canonical form
      double pt[3], pl[3];
      point_in(robot, (ap < 0) ? -1 : T.jlink[T.order[ap]], sp.link, sp.pos, pt);
      canon_vec(T.canonical((ap < 0) ? -1 : T.order[ap]), pt, pl);
      for (int q=0; q<3; q++) M.sph_pos[s][q] = (real) pl[q];
      M.sph_radius[s] = (real) sp.radius;
      M.sph_link[s] = sp.link;
      unsigned long long aff = 0ull;
      if (ap >= 0) for (int jk=T.order[ap]; jk>=0; jk=T.jparent[jk]) aff |= (1ull << T.pos_in_order[jk]);
      M.sph_affects[s] = aff;
      if (ap < 0) { if (M.base_sph_end == 0) M.base_sph_begin = s; M.base_sph_end = s+1; }
      else
      {
         DevJoint<real> & J = M.joints[ap];
         if (J.sph_end == 0 && J.sph_begin == 0) J.sph_begin = s;
         J.sph_end = s+1;
      }
      device_sphere_order.push_back(act[s].xml);
   }
   for (int k=0; k<nj; k++)
   {
      DevJoint<real> & J = M.joints[k];
      J.packed = (J.type & 3) | ((J.sph_begin & 255) << 8) | ((J.sph_end & 255) << 16) | ((J.col & 127) << 24);
      J.packed2 = ((J.load_slot + 2) & 15) | (((J.save_slot + 2) & 15) << 4);
      M.jpacked[k] = J.packed; M.jpacked2[k] = J.packed2;
   }
   M.jt_scan = 1;
   for (int k=0; k<nj; k++)
   {
      DevJoint<real> & J = M.joints[k];
      int first = -1, last = -1, count = 0;
      for (int s=0; s<Sa; s++)
         if ((M.sph_affects[s] >> k) & 1ull) { if (first < 0) first = s; last = s; count++; }
      J.aff_begin = (count > 0) ? first : Sa;
      J.aff_end = (count > 0) ? last + 1 : Sa;
      if (count > 0 && last - first + 1 != count) { M.jt_scan = 0; break; }
      if (count > 0 && J.aff_end != Sa) M.jt_scan = 2;
   }
}

// everything indexed by lane goes to slot order; the inactive spheres ride on free lanes or stay in their loop; the pair list
template <typename real>
void fold_lanes(DevModel<real> & M, const Robot & robot, const Lanes & L, const std::vector<SphRef> & act, const std::vector<SphRef> & inact,
   std::vector<int> & device_sphere_order, std::vector<int> & slot_xml)
{
   const int Sa = (int) act.size();
   int lanes = L.lanes, n_static = L.n_static;
   {
      std::vector<real> rad(Sa); std::vector<int> link(Sa); std::vector<unsigned long long> aff(Sa);
      for (int s=0; s<Sa; s++) { rad[s] = M.sph_radius[s]; link[s] = M.sph_link[s]; aff[s] = M.sph_affects[s]; }
      for (int q=0; q<lanes; q++) { M.sph_radius[q] = (real) 0; M.sph_link[q] = -1000 - q; M.sph_affects[q] = 0ull; }
      M.live_mask = 0ull; M.placed = L.placed ? 1 : 0;
      for (int s=0; s<Sa; s++)
      {
         const int q = L.slot_of[s];
         M.slot_of[s] = q; M.sph_radius[q] = rad[s]; M.sph_link[q] = link[s]; M.sph_affects[q] = aff[s];
         M.live_mask |= (1ull << q);
      }
   }
   if (L.pairs) lanes = Sa + n_static;
   if (!L.placed && !L.pairs) n_static = 0;
   if (L.placed)
   {
      // entries past the active spheres: the slots without an active sphere, in order (static or empty: their wrench is zero)
      int next = Sa;
      for (int q=0; q<16 && next<16; q++) if (!((M.live_mask >> q) & 1ull)) M.slot_of[next++] = q;
   }
   M.n_static = n_static; M.static_mask = 0ull;
   M.Sa_real = Sa; M.Sa = lanes; M.S = lanes + (int) inact.size() - n_static;
   slot_xml.assign(lanes, -1);
   for (int s=0; s<Sa; s++) slot_xml[L.slot_of[s]] = act[s].xml;
   std::vector<Xform> frames;
   robot.fk(robot.transform, robot.dof_values, frames);
   for (int s=0; s<(int) inact.size(); s++)
   {
      const Robot::Sphere & sp = robot.spheres[inact[s].xml];
      const Xform & lf = frames[sp.link];
      double pw[3];
      mat3_vec(lf.R, sp.pos, pw);                                    // mod.cpp:2332-2345
      if (s < n_static)
      {
         const int q = L.slot_of[Sa + s];
         M.static_slot[s] = q; M.static_mask |= (1ull << q);
         for (int k=0; k<3; k++) M.static_pos[s][k] = (real)(pw[k] + lf.t[k]);
         M.sph_radius[q] = (real) sp.radius; M.sph_link[q] = sp.link; M.sph_affects[q] = 0ull;
      }
      else
      {
         const int r = s - n_static;
         for (int q=0; q<3; q++) M.sph_inactive_pos[r][q] = (real)(pw[q] + lf.t[q]);
         M.sph_radius[lanes+r] = (real) sp.radius;
         M.sph_link[lanes+r] = sp.link;
      }
      device_sphere_order.push_back(inact[s].xml);
   }
   M.pr_rounds = L.pairs ? L.ptab.rounds : 0;
   M.pr_hot = L.pairs ? L.ptab.hot : 0;
   if (L.pairs)
      for (size_t e=0; e<(size_t) ORC_PAIR_ROUNDS * 32; e++)
      { M.pr_ab[e] = L.ptab.ab[e]; M.pr_gat[2*e] = L.ptab.gat[2*e]; M.pr_gat[2*e+1] = L.ptab.gat[2*e+1]; M.pr_rsum[e] = (real) L.ptab.rsum[e]; }
}

// the FK walk's records (DevFkJoint): fixed transform (the axis is z), control word and the first four spheres of the link; and the cut
// of the walk.  A chain that then branches: joints 0 .. c are each other's parents, c has several children and everything
// after c hangs below it.  The walk is cut at the child of c that balances [0, cut) against (chain + [cut, nj)).
template <typename real>
void fold_fk_walk(DevModel<real> & M, const JointTree & T, const Switches & sw)
{
   const int nj = T.nj();
   for (int k=0; k<nj; k++)
   {
      const DevJoint<real> & J = M.joints[k];
      DevFkJoint<real> & F = M.fkj[k];
      for (int q=0; q<9; q++) F.Rfix[q] = J.Rfix[q];
      for (int q=0; q<3; q++) F.tfix[q] = J.tfix[q];
      const int count = J.sph_end - J.sph_begin;
      F.ctl = (count & 255) | ((J.sph_begin & 255) << 8) | (((J.load_slot + 2) & 15) << 16) | (((J.save_slot + 2) & 15) << 20)
            | ((J.type == 1 ? 1 : 0) << 24) | ((J.col & 127) << 25);
      for (int u=0; u<4; u++)
      {
         const int sidx = (u < count) ? J.sph_begin + u : 0;
         for (int q=0; q<3; q++) F.sph[u][q] = (u < count) ? M.sph_pos[sidx][q] : (real) 0;
         F.slot[u] = (u < count) ? M.slot_of[sidx] : 0;
      }
   }
   M.fk_split = 0; M.fk_nanc = 0; M.fk_b_begin = nj;
   if (T.roots.size() == 1 && nj >= 8 && !sw.no_fk_split)
   {
      std::vector<int> ppos(nj);                       // parent of the k-th joint of the walk, as a position of the walk
      for (int k=0; k<nj; k++) ppos[k] = (T.jparent[T.order[k]] < 0) ? -1 : T.pos_in_order[T.jparent[T.order[k]]];
      int c = 0;
      while (c + 1 < nj && T.children[T.order[c]].size() == 1) c++;       // the chain in front of the first branching joint
      bool chain = true;
      for (int k=1; k<=c; k++) if (ppos[k] != k - 1) chain = false;
      const std::vector<int> & branches = T.children[T.order[c]];
      if (chain && branches.size() >= 2)
      {
         int best = -1, best_len = nj;
         for (size_t ci=1; ci<branches.size(); ci++)
         {
            const int cut = T.pos_in_order[branches[ci]];
            const int len = std::max(cut, (c + 1) + (nj - cut));
            if (len < best_len) { best_len = len; best = cut; }
         }
         if (best > 0 && 4 * best_len <= 3 * nj) { M.fk_split = 1; M.fk_nanc = c + 1; M.fk_b_begin = best; }
      }
   }
   if (sw.debug_plan && M.fk_split)
      fprintf(stderr, "orc fk: the walk is cut in two: joints [0, %d) | chain [0, %d) + joints [%d, %d)\n", M.fk_b_begin, M.fk_nanc, M.fk_b_begin, nj);
}

} // namespace

std::string placement_key(const Robot & robot, const BatchParams & params, int n_static)
{
   std::string key = robot.name + (params.floating_base ? "|f|" : "|a|") + std::to_string(params.epsilon_self) + "|s" + std::to_string(n_static);
   for (int d : robot.active_dofs) key += "," + std::to_string(d);
   key += "|";
   for (int d=0; d<robot.n_dof; d++)
   {
      bool act = false;
      for (int a : robot.active_dofs) if (a == d) act = true;
      unsigned long long bits = 0; const double v = act ? 0.0 : robot.dof_values[d];
      std::memcpy(&bits, &v, sizeof(bits));
      key += std::to_string(bits) + ",";
   }
   // ... and the spheres themselves: the same robot holding a body is another row of spheres
   unsigned long long h = 1469598103934665603ull;
   auto mix = [&h](const void * p, size_t nb) { const unsigned char * c = (const unsigned char *) p; for (size_t i=0; i<nb; i++) { h ^= c[i]; h *= 1099511628211ull; } };
   for (const Robot::Sphere & sp : robot.spheres) { mix(&sp.link, sizeof(sp.link)); mix(sp.pos, sizeof(sp.pos)); mix(&sp.radius, sizeof(sp.radius)); }
   return key + "|h" + std::to_string(h);
}

// ================================================================ the robot ===
// Fold the robot into the device model: only optimized joints remain, every other
// joint is frozen at its current value inside the fixed transforms; active spheres are
// sorted by the joint they ride on (SURVEY 8a T2 for the active/inactive split).
template <typename real>
FoldedModel<real> fold_robot(const Robot & robot, const BatchParams & params, int n, const JointTree & T, int asked_block,
   const Switches & sw, PlacementCache cache)
{
   FoldedModel<real> out;
   out.model.reset(new DevModel<real>);
   DevModel<real> & M = *out.model;
   const int n_adof = (int) robot.active_dofs.size(), nj = T.nj();
   const Xform xbase = xform_from_pose(robot.transform);
   std::memset(&M, 0, sizeof(M));
   M.nj = nj; M.n = n; M.floating = params.floating_base;
   for (int k=0; k<9; k++) M.base_R[k] = (real) xbase.R.m[k];
   for (int k=0; k<3; k++) M.base_t[k] = (real) xbase.t[k];

   // spheres: active first (device order = by joint in DFS order), then inactive
   std::vector<SphRef> act, inact;
   for (int si=0; si<(int) robot.spheres.size(); si++)
   {
      bool active = params.floating_base != 0;
      for (int j=0; j<n_adof && !active; j++)
         if (robot.does_affect(robot.active_dofs[j], robot.spheres[si].link)) active = true;
      const int at = T.attach_of(robot, robot.spheres[si].link);
      SphRef s; s.xml = si; s.attach_pos = (at < 0) ? -1 : T.pos_in_order[at];
      (active ? act : inact).push_back(s);
   }
   if (act.empty()) throw std::runtime_error("robot active dofs must have at least one sphere!");
   std::stable_sort(act.begin(), act.end(), [](const SphRef & a, const SphRef & b) { return a.attach_pos < b.attach_pos; });
   const int Sa = (int) act.size(), S = Sa + (int) inact.size();
   if (S > ORC_MAX_SPHERES) throw std::runtime_error("too many spheres for this build!");
   M.Sa = Sa; M.S = S;
   int GS = 1; while (GS < Sa) GS <<= 1;
   M.GS = GS;
   M.base_sph_begin = 0; M.base_sph_end = 0;
   fold_joints(M, robot, T);
   fold_active_spheres(M, robot, T, act, out.device_sphere_order);
   if (sw.no_jt_scan) M.jt_scan = 0;      // experiments: per-joint reductions
   const Lanes L = choose_lanes(robot, params, act, inact, M.GS, M.tree != 0, M.jt_scan, sizeof(real) == 8, asked_block, sw, cache);
   fold_lanes(M, robot, L, act, inact, out.device_sphere_order, out.slot_xml);
   fold_fk_walk(M, T, sw);

   const bool pairs = L.pairs;
   out.variant = robot_variant(M.tree != 0, M.GS, M.floating != 0, M.jt_scan, M.placed != 0, nj, pairs, sw.no_kind);
   out.pair_entries = pairs ? L.ptab.rounds * M.GS : 0;

   ModelScalars & ms = out.scalars;
   ms = ModelScalars();
   ms.nj = M.nj; ms.floating = M.floating; ms.tree = M.tree; ms.Sa = M.Sa; ms.S = M.S; ms.Sa_real = M.Sa_real; ms.placed = M.placed;
   ms.GS = M.GS; ms.base_sph_begin = M.base_sph_begin; ms.base_sph_end = M.base_sph_end; ms.jt_scan = M.jt_scan; ms.n_static = M.n_static;
   ms.live_mask = M.live_mask; ms.static_mask = M.static_mask;
   ms.fk_split = M.fk_split; ms.fk_nanc = M.fk_nanc; ms.fk_b_begin = M.fk_b_begin; ms.pr_rounds = M.pr_rounds;
   ms.pr_deg[0] = pairs ? L.ptab.deg[0] : 0ull; ms.pr_deg[1] = pairs ? L.ptab.deg[1] : 0ull; ms.pr_hot = M.pr_hot; ms.pad2_ = 0;
   return out;
}
template FoldedModel<double> fold_robot<double>(const Robot &, const BatchParams &, int, const JointTree &, int, const Switches &, PlacementCache);
template FoldedModel<float> fold_robot<float>(const Robot &, const BatchParams &, int, const JointTree &, int, const Switches &, PlacementCache);

// ================================================================ TSR constraints ===
template <typename real>
FoldedTsrs<real> fold_tsrs(const Robot & robot, const BatchParams & params, const JointTree & tree, int m, int n)
{
   FoldedTsrs<real> out;
   const int n_tsrs = out.n_tsrs = (int) params.tsrs.size();
   if (n_tsrs == 0) return out;
   std::vector<DevTsr<real>> & ht = out.tsrs;
   ht.resize(n_tsrs);
   for (int c=0; c<n_tsrs; c++)
   {
      const TsrSpec & sp = params.tsrs[c];
      DevTsr<real> & T = ht[c];
      std::memset(&T, 0, sizeof(T));
      const int at = tree.attach_of(robot, sp.ee_link);
      for (int jk=at; jk>=0; jk=tree.jparent[jk]) T.chain_mask |= (1u << tree.pos_in_order[jk]);
      // the link's frame in the moved frame of its last chain joint's link (the base frame for -1)
      Xform x; for (int q=0; q<9; q++) x.R.m[q] = (q % 4 == 0) ? 1.0 : 0.0;
      x.t[0] = x.t[1] = x.t[2] = 0.0;
      const int from_link = (at < 0) ? -1 : tree.jlink[at];
      for (int cur=sp.ee_link; cur!=from_link && cur>=0; cur=robot.parent[cur]) x = xform_mul(local_moved(robot, cur), x);
      // (the walk's frame of that joint is canonical; the constraint reads the link's true pose)
      const Mat3 & Ca = tree.canonical(at);
      const Mat3 Rc = canon_mat(Ca, x.R, tree.canonical(-1));
      double tc[3];
      canon_vec(Ca, x.t, tc);
      for (int q=0; q<9; q++) T.Xl_R[q] = (real) Rc.m[q];
      for (int q=0; q<3; q++) T.Xl_t[q] = (real) tc[q];
      const Pose tw = pose_invert(sp.T0w), eo = pose_invert(sp.Twe);
      for (int q=0; q<7; q++) { T.tool[q] = (real) sp.tool.v[q]; T.table_world[q] = (real) tw.v[q]; T.ee_obj[q] = (real) eo.v[q]; }
      T.k = 0;
      for (int q=0; q<6; q++)      // src/orcdchomp_mod.cpp:2466-2480
      {
         T.enabled[q] = (sp.Bw[q][0] == 0.0 && sp.Bw[q][1] == 0.0) ? 1 : 0;
         T.k += T.enabled[q];
      }
      if (T.k == 0) throw std::runtime_error("TSR constraint with no fixed dimension (every Bw row has a range)!");
   }
   // rows in the reference's list order: the last constraint added comes first (src/libcd/chomp.c:231-232,418-424)
   int base = 0, blocks = 0;
   for (int c=n_tsrs-1; c>=0; c--)
   {
      ht[c].point = params.tsrs[c].point;
      ht[c].npts = (ht[c].point < 0) ? m : 1;
      if (ht[c].point >= m) throw std::runtime_error("TSR constraint on a point the trajectory does not have!");
      ht[c].row_base = base; base += ht[c].k * ht[c].npts;
      ht[c].blk_base = blocks; blocks += ht[c].npts;
   }
   out.cons_k = base; out.blocks = blocks;
   out.ws_stride = (size_t) 2*base + (size_t) base * n + (size_t) blocks * n + (size_t) base * base
                 + (size_t) m * n * (n + 1)            // delta rows of the structured solve (tsr.h)
                 + (size_t) blocks * tree.nj() * 6;    // the joints' world axes and anchors of every (constraint, point) block (tsr_eval_point)
   for (int i=0; i<m; i++)
   {
      int ki = 0;
      for (int c=0; c<n_tsrs; c++) if (ht[c].npts == m || ht[c].point == i) ki += ht[c].k;
      out.kmax = std::max(out.kmax, ki);
   }
   return out;
}
template FoldedTsrs<double> fold_tsrs<double>(const Robot &, const BatchParams &, const JointTree &, int, int);
template FoldedTsrs<float> fold_tsrs<float>(const Robot &, const BatchParams &, const JointTree &, int, int);

// ================================================================ the scene table ===
namespace {
// one field placement as the kernels read it: the descriptor, and the same in cell units (folded in double precision)
template <typename real>
void fold_field(const ScenePlacement & placement, DevSdf<real> & hsi, DevSdfCell<real> & hci)
{
   const Sdf & s = *placement.sdf;
   const Pose pose_world_gsdf = pose_compose(placement.pose_world_kinbody, s.pose);
   const Pose pose_gsdf_world = pose_invert(pose_world_gsdf);
   const Mat3 Rgw = pose_rotation_expanded(pose_gsdf_world);
   const Mat3 Rwg = pose_rotation_expanded(pose_world_gsdf);
   for (int q=0; q<9; q++) { hsi.Rgw[q] = (real) Rgw.m[q]; hsi.Rwg[q] = (real) Rwg.m[q]; }
   hsi.rot_identity = 1;
   for (int q=0; q<9; q++)
      if (Rgw.m[q] != ((q % 4 == 0) ? 1.0 : 0.0) || Rwg.m[q] != ((q % 4 == 0) ? 1.0 : 0.0)) hsi.rot_identity = 0;
   for (int q=0; q<3; q++)
   {
      hsi.tgw[q] = (real) pose_gsdf_world.v[q];
      hsi.size[q] = s.grid.sizes[q];
      hsi.length[q] = (real) s.grid.lengths[q];
      hsi.inv_length[q] = (real)(1.0 / s.grid.lengths[q]);
      hsi.cell[q] = (real)(s.grid.lengths[q] / s.grid.sizes[q]);
      hsi.size_over_len[q] = (real)(s.grid.sizes[q] / s.grid.lengths[q]);
   }
   for (int r=0; r<3; r++)
   {
      const double sol = s.grid.sizes[r] / s.grid.lengths[r];
      for (int c=0; c<3; c++)
      {
         hci.M[r*3+c] = (real)(sol * Rgw.m[r*3+c]);
         hci.W[c*3+r] = (real)(Rwg.m[c*3+r] * sol);
      }
      hci.t[r] = (real)(sol * pose_gsdf_world.v[r]);
      hci.fsize[r] = (real) s.grid.sizes[r];
      hci.fsize_m1[r] = (real)(s.grid.sizes[r] - 1);
   }
   hci.stride_b[0] = s.grid.sizes[1] * s.grid.sizes[2] * (int) sizeof(real);
   hci.stride_b[1] = s.grid.sizes[2] * (int) sizeof(real);
   hci.stride_r[0] = (real) hci.stride_b[0]; hci.stride_r[1] = (real) hci.stride_b[1]; hci.stride_r[2] = (real) sizeof(real);
}
}

template <typename real>
FoldedScenes<real> fold_scenes(const SceneTable & table, int run0, int n_runs, bool offsets_24bit)
{
   FoldedScenes<real> out;
   out.n_scenes = (int) table.scenes.size();
   out.n_sdfs = table.max_fields();
   if (out.n_sdfs > ORC_MAX_SDFS) throw std::runtime_error("too many signed distance fields for this build!");
   out.sdfc_stride = ((out.n_sdfs + 3) / 4) * 4 + 4;
   out.sdfs.resize((size_t) out.n_scenes * out.n_sdfs);
   out.cells.resize((size_t) out.n_scenes * out.sdfc_stride);
   std::memset(out.cells.data(), 0, out.cells.size() * sizeof(DevSdfCell<real>));
   out.scene_nsdf.resize(out.n_scenes);
   // the grids of the scenes this shard's runs are in come to its device (once per device: the copies are shared)
   std::vector<unsigned char> used(out.n_scenes, 0);
   for (int k=0; k<n_runs; k++) used[table.scene_of_run[run0 + k]] = 1;
   out.one_aligned = out.n_scenes > 0;
   for (int sc=0; sc<out.n_scenes; sc++)
   {
      const std::vector<ScenePlacement> & fields = table.scenes[sc];
      out.scene_nsdf[sc] = (int) fields.size();
      if (fields.size() != 1) out.one_aligned = false;
      for (int f=0; f<(int) fields.size(); f++)
      {
         Sdf & s = *fields[f].sdf;
         DevSdf<real> & hsi = out.sdfs[(size_t) sc * out.n_sdfs + f];
         DevSdfCell<real> & hci = out.cells[(size_t) sc * out.sdfc_stride + f];
         if (used[sc]) out.grids.push_back({ sc, f, &s });
         fold_field(fields[f], hsi, hci);
         if (!hsi.rot_identity) out.one_aligned = false;
         if (s.grid.ncells() * sizeof(real) >= (size_t) 1 << 31) throw std::runtime_error("signed distance field too large for this build!");
         // the many-sphere pass forms its cell offsets with 24-bit multiplies (cost_generic.h: signed, both operands below 2^23)
         if (offsets_24bit && (hci.stride_b[0] >= (1 << 23) || std::max(s.grid.sizes[0], std::max(s.grid.sizes[1], s.grid.sizes[2])) >= (1 << 23)))
            throw std::runtime_error("signed distance field too large for this build (a y-z plane of 8 MB or more with a robot of more than 16 active spheres)!");
      }
   }
   return out;
}
template FoldedScenes<double> fold_scenes<double>(const SceneTable &, int, int, bool);
template FoldedScenes<float> fold_scenes<float>(const SceneTable &, int, int, bool);

// ================================================================ the metric ===
MetricTables pack_metric(const Metric & metric, const BatchParams & params, int m, size_t real_bytes, const Switches & sw)
{
   MetricTables out;
   if (real_bytes == 4 && params.derivative >= 2)
   {
      out.metric64 = metric.Aband;
      out.metric64.insert(out.metric64.end(), metric.beta_s.begin(), metric.beta_s.end());
      out.metric64.insert(out.metric64.end(), metric.beta_g.begin(), metric.beta_g.end());
   }
   // A^-1: closed-form Toeplitz inverse through two wave scans per column when the metric is
   // ca tridiag(-1,2,-1) (derivative 1), else cyclic reduction (tridiagonal) or the dense inverse
   out.solve_mode = (params.derivative == 1) ? 0 : 1;
   // derivative 2..4: the band inverse through its rank-D generators, D prefix and D suffix wave scans per column (the dense
   // inverse stays for a metric whose generators the host's check rejects, and as ORC_NO_SEMISEP=1 for A/B runs)
   if (metric.ss_rank > 0 && !sw.no_semisep) out.solve_mode = 3;
   // (any length since round 6: beyond 256 moving waypoints the scans read a lane's rows twice instead of holding them in registers;
   // ORC_SCAN_MAX_M=256 brings the cyclic reduction back for such runs, for A/B)
   if (params.derivative == 1 && m <= sw.scan_max_m && metric.Aband.size() == (size_t) 3*m
       && (m < 2 || metric.Aband[(size_t) 1*m] == -2.0 * metric.Aband[(size_t) 2*m]) && !sw.no_scan_solve)
      out.solve_mode = 2;
   if (!metric.pcr.empty() && out.solve_mode == 0)
   {
      if (metric.pcr_sym && !sw.pcr_full)
      {
         // compact table: the rows towards i-s of every level, then the inverse diagonal
         for (int l=0; l<metric.pcr_levels; l++)
            out.pcr.insert(out.pcr.end(), metric.pcr.begin() + (size_t)(2*l)*m, metric.pcr.begin() + (size_t)(2*l+1)*m);
         out.pcr.insert(out.pcr.end(), metric.pcr.begin() + (size_t)(2*metric.pcr_levels)*m, metric.pcr.end());
         out.pcr_rows = metric.pcr_levels + 1; out.pcr_sym = 1;
      }
      else
      {
         out.pcr = metric.pcr;
         out.pcr_rows = 2*metric.pcr_levels + 1; out.pcr_sym = 0;
      }
   }
   if (out.solve_mode == 3)
   {
      // The metric's tables of a higher derivative, one array of doubles (also for fp32 runs: the scans and the band rows are
      // taken in double) that travels like the cyclic-reduction tables of derivative 1 -- staged in LDS when the plan has room,
      // read through L2 otherwise: U [D][m], V [D][m] (generators of the band inverse), then the D rows at either end of the band
      // with their couplings to the end points, [2D][2D+3] = A[i][i-D..i+D], beta_s[i], beta_g[i] (the rows between are one
      // Toeplitz row, kernarg scalars: DevBatch::band_c)
      const int D = metric.ss_rank;
      std::vector<double> & tab = out.pcr;
      tab = metric.ssU;
      tab.insert(tab.end(), metric.ssV.begin(), metric.ssV.end());
      for (int e=0; e<2*D; e++)
      {
         const int i = (e < D) ? e : m - 2*D + e;
         for (int k=-D; k<=D; k++) tab.push_back((i+k >= 0 && i+k < m) ? metric.Aband[(size_t)(k+D)*m + i] : 0.0);
         tab.push_back(metric.beta_s[i]); tab.push_back(metric.beta_g[i]);
      }
      const size_t per = sizeof(double) / real_bytes;                       // reals per table entry
      out.pcr_rows = (int)((tab.size() * per + (size_t) m - 1) / (size_t) m);
      tab.resize(((size_t) out.pcr_rows * m + per - 1) / per, 0.0);
      out.pcr_as_doubles = true; out.pcr_sym = 0;
   }
   if (metric.Ainv.empty() && (!params.tsrs.empty() || out.solve_mode == 1))
   {
      // the constraint step multiplies by entries of the dense inverse (src/libcd/chomp.c:567-575,592-599)
      out.Ainv = metric.Adense;
      invert_matrix(out.Ainv, m);
   }
   // a higher derivative: is the band one Toeplitz row away from the D rows at either end, with no coupling to the end points?
   const int D = metric.D;
   if (out.solve_mode == 3 && D >= 2 && D <= ORC_SS_MAX_RANK && m >= 2*D + 1 && !sw.no_band_toeplitz)
   {
      bool ok = true;
      for (int i=D; i<m-D && ok; i++)
      {
         for (int k=-D; k<=D; k++)
            if (metric.Aband[(size_t)(k+D)*m + i] != metric.Aband[(size_t)(std::abs(k)+D)*m + D]) ok = false;
         if (metric.beta_s[i] != 0.0 || metric.beta_g[i] != 0.0) ok = false;
      }
      if (ok)
      {
         out.band_toeplitz = 1;
         for (int k=0; k<=D; k++) out.band_c64[k] = metric.Aband[(size_t)(k+D)*m + D];
      }
   }
   return out;
}

} // namespace orc
