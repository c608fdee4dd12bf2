// fk_canonical_driver.cpp -- the fold's canonical joint records, composed on the host (tests/test_host_fk_canonical.py).
//
// Compiled by a host compiler with csrc/fold.cpp, env.cpp and host_math.cpp: no HIP, no device.  Reads one robot, its state and a
// list of configurations from the file named on the command line (numbers as C99 hexadecimal floats), folds the robot as `create`
// does (fold_joint_tree, fold_robot<double>, fold_tsrs<double>) and walks the folded records the way fk.h does -- frame o (Rfix,
// tfix), then a turn about z or a shift along z -- in plain double arithmetic.  Prints
//    C <walk position> <link> <9 entries of C_j> <3 of the robot's axis>          the canonical rotation of every optimized joint
//    J <config> <link> <R[9]> <t[3]>                                              the link's TRUE frame: walked frame o C_j^T
//    S <config> <xml index> <p[3]>                                                the centre of every active sphere in the world
//    E <config> <R[9]> <t[3]>                                                     the constrained link's frame as tsr_point.h forms it
// for the test to hold against RobotModel.link_frames.
#include "stages.h"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

using namespace orc;

namespace {
struct Reader
{
   std::ifstream in;
   explicit Reader(const char * path) : in(path) { if (!in) throw std::runtime_error("cannot read the input file"); }
   double num() { std::string tok; if (!(in >> tok)) throw std::runtime_error("input ends early"); return strtod(tok.c_str(), nullptr); }
   int integer() { return (int) num(); }
};
struct Frame { double R[9], t[3]; };

Frame apply(const Frame & f, const double * R, const double * t)
{
   Frame o;
   for (int r=0; r<3; r++)
   {
      for (int c=0; c<3; c++) o.R[3*r+c] = f.R[3*r+0]*R[0*3+c] + f.R[3*r+1]*R[1*3+c] + f.R[3*r+2]*R[2*3+c];
      o.t[r] = f.R[3*r+0]*t[0] + f.R[3*r+1]*t[1] + f.R[3*r+2]*t[2] + f.t[r];
   }
   return o;
}
void print_frame(const Frame & f)
{
   for (int q=0; q<9; q++) printf(" %a", f.R[q]);
   for (int q=0; q<3; q++) printf(" %a", f.t[q]);
   printf("\n");
}
}

int main(int argc, char ** argv)
{
   if (argc != 2) { fprintf(stderr, "usage: fk_canonical_driver <input>\n"); return 2; }
   try
   {
      Reader rd(argv[1]);
      Robot robot;
      robot.name = "canonical";
      robot.n_links = rd.integer(); robot.n_dof = rd.integer();
      const int n_spheres = rd.integer(), floating = rd.integer(), n_active = rd.integer(), n_configs = rd.integer(), ee_link = rd.integer();
      for (int li=0; li<robot.n_links; li++)
      {
         robot.parent.push_back(rd.integer()); robot.joint_type.push_back(rd.integer()); robot.dof_index.push_back(rd.integer());
         double p[7]; for (int q=0; q<7; q++) p[q] = rd.num();
         robot.pose_parent_joint.push_back(Pose(p));
         for (int q=0; q<3; q++) robot.axis.push_back(rd.num());
      }
      for (int d=0; d<robot.n_dof; d++) { robot.limit_lower.push_back(rd.num()); robot.limit_upper.push_back(rd.num()); }
      { double p[7]; for (int q=0; q<7; q++) p[q] = rd.num(); robot.transform = Pose(p); }
      for (int d=0; d<robot.n_dof; d++) robot.dof_values.push_back(rd.num());
      for (int a=0; a<n_active; a++) robot.active_dofs.push_back(rd.integer());
      for (int s=0; s<n_spheres; s++)
      {
         Robot::Sphere sp; sp.link = rd.integer();
         for (int q=0; q<3; q++) sp.pos[q] = rd.num();
         sp.radius = rd.num();
         robot.spheres.push_back(sp);
      }
      const int n = (floating ? 7 : 0) + n_active;
      std::vector<double> configs((size_t) n_configs * n);
      for (double & v : configs) v = rd.num();

      BatchParams params;
      params.floating_base = floating;
      TsrSpec ts; ts.ee_link = ee_link;
      for (int q=0; q<6; q++) ts.Bw[q][0] = ts.Bw[q][1] = 0.0;
      params.tsrs.push_back(ts);
      Switches sw; sw.no_placement = true;      // (the lanes are not this test's business; the annealing run takes its time)
      std::map<std::string, std::vector<int>> placed; std::recursive_mutex mutex;
      const JointTree T = fold_joint_tree(robot, floating != 0);
      const FoldedModel<double> fm = fold_robot<double>(robot, params, n, T, 0, sw, PlacementCache{ placed, mutex });
      const FoldedTsrs<double> ft = fold_tsrs<double>(robot, params, T, 1, n);
      const DevModel<double> & M = *fm.model;
      const int nj = T.nj();
      for (int k=0; k<nj; k++)
      {
         const int li = T.jlink[T.order[k]];
         const Mat3 C = T.canonical(T.order[k]);
         printf("C %d %d", k, li);
         for (int q=0; q<9; q++) printf(" %a", C.m[q]);
         for (int q=0; q<3; q++) printf(" %a", robot.axis[3*li+q]);
         printf("\n");
         if (M.joints[k].axis[0] != 0.0 || M.joints[k].axis[1] != 0.0 || M.joints[k].axis[2] != 1.0) throw std::runtime_error("a record's axis is not z");
      }
      for (int cfg=0; cfg<n_configs; cfg++)
      {
         const double * row = &configs[(size_t) cfg * n];
         Frame base;
         if (floating)
         {
            const double q[4] = { row[3], row[4], row[5], row[6] };
            const Mat3 R = quat_to_R(q);
            for (int e=0; e<9; e++) base.R[e] = R.m[e];
            for (int e=0; e<3; e++) base.t[e] = row[e];
         }
         else
         {
            for (int e=0; e<9; e++) base.R[e] = M.base_R[e];
            for (int e=0; e<3; e++) base.t[e] = M.base_t[e];
         }
         std::vector<Frame> moved(nj);
         for (int k=0; k<nj; k++)
         {
            const DevJoint<double> & J = M.joints[k];
            const int jp = T.jparent[T.order[k]];
            Frame f = apply((jp < 0) ? base : moved[T.pos_in_order[jp]], J.Rfix, J.tfix);
            const double q = row[J.col];
            if (J.type == 1)
            {
               const double s = std::sin(q), c = std::cos(q);
               for (int r=0; r<3; r++)
               {
                  const double r0 = f.R[3*r+0], r1 = f.R[3*r+1];
                  f.R[3*r+0] = r0*c + s*r1; f.R[3*r+1] = r1*c - s*r0;
               }
            }
            else for (int r=0; r<3; r++) f.t[r] += q * f.R[3*r+2];
            moved[k] = f;
            // the link's true frame: F = F' C^T
            const Mat3 C = T.canonical(T.order[k]);
            double Ct[9]; const double zero[3] = { 0.0, 0.0, 0.0 };
            for (int r=0; r<3; r++) for (int c=0; c<3; c++) Ct[3*r+c] = C.m[3*c+r];
            printf("J %d %d", cfg, T.jlink[T.order[k]]);
            print_frame(apply(f, Ct, zero));
         }
         for (int s=0; s<M.Sa_real; s++)
         {
            int k_at = -1;
            for (int k=0; k<nj; k++) if (s >= M.joints[k].sph_begin && s < M.joints[k].sph_end) k_at = k;
            const Frame & f = (k_at < 0) ? base : moved[k_at];
            printf("S %d %d", cfg, fm.device_sphere_order[s]);
            for (int r=0; r<3; r++) printf(" %a", f.R[3*r+0]*M.sph_pos[s][0] + f.R[3*r+1]*M.sph_pos[s][1] + f.R[3*r+2]*M.sph_pos[s][2] + f.t[r]);
            printf("\n");
         }
         const int at = T.attach_of(robot, ee_link);
         printf("E %d", cfg);
         print_frame(apply((at < 0) ? base : moved[T.pos_in_order[at]], ft.tsrs[0].Xl_R, ft.tsrs[0].Xl_t));
      }
   }
   catch (const std::exception & e) { fprintf(stderr, "fk_canonical_driver: %s\n", e.what()); return 1; }
   return 0;
}
