// trajdoc.cpp -- trajectory documents written, read and sampled (trajdoc.h).
// Reference: src/orcdchomp_mod.cpp:2375-2416 (starttraj), 2899-3008 (gettraj).
#include "trajdoc.h"
#include "host_math.h"
#include <algorithm>
#include <cstdlib>
#include <iomanip>
#include <limits>
#include <sstream>

namespace orc {

std::string serialize_traj(const std::string & robot, const std::vector<int> & adofs,
   const double * traj, int n_points, int n, int col0, const std::vector<double> & deltatime)
{
   std::ostringstream o;
   const int nd = n - col0;
   o << std::setprecision(std::numeric_limits<double>::max_digits10);
   o << "<trajectory>\n<configuration>\n<group name=\"joint_values " << robot;
   for (int a : adofs) o << " " << a;
   o << "\" offset=\"0\" dof=\"" << nd << "\" interpolation=\"linear\"/>\n";
   o << "<group name=\"deltatime\" offset=\"" << nd << "\" dof=\"1\" interpolation=\"\"/>\n";
   if (col0)
   {
      // floating base: the second trajectory of src/orcdchomp_mod.cpp:2912-2956 merged in: the base pose of every
      // waypoint as `affine_transform <robot> <DOF_Transform>` (x y z, then the quaternion in OpenRAVE's order
      // w x y z) and its finite-difference velocities over the waypoint's deltatime as `affine_velocities`
      const int dof_transform = 1 | 2 | 4 | 32;      // OpenRAVE::DOF_XYZ | DOF_RotationQuat
      o << "<group name=\"affine_transform " << robot << " " << dof_transform << "\" offset=\"" << nd + 1 << "\" dof=\"7\" interpolation=\"linear\"/>\n";
      o << "<group name=\"affine_velocities " << robot << " " << dof_transform << "\" offset=\"" << nd + 8 << "\" dof=\"7\" interpolation=\"next\"/>\n";
   }
   o << "</configuration>\n<data count=\"" << n_points << "\">\n";
   static const int order[7] = { 0, 1, 2, 6, 3, 4, 5 };      // libcd x y z qx qy qz qw -> x y z qw qx qy qz
   for (int i=0; i<n_points; i++)
   {
      for (int j=col0; j<n; j++) o << traj[(size_t) i*n+j] << " ";
      o << deltatime[i];
      if (col0)
      {
         for (int k=0; k<7; k++) o << " " << traj[(size_t) i*n + order[k]];
         for (int k=0; k<7; k++)
            o << " " << ((i > 0) ? (traj[(size_t) i*n + order[k]] - traj[(size_t)(i-1)*n + order[k]]) / deltatime[i] : 0.0);
      }
      if (i+1 < n_points) o << " ";
   }
   o << "\n</data>\n</trajectory>\n";
   return o.str();
}

bool parse_traj(const std::string & text, TrajDoc & doc)
{
   const size_t c0 = text.find("<data count=\"");
   if (c0 == std::string::npos) return false;
   doc.count = std::atoi(text.c_str() + c0 + 13);
   const size_t d0 = text.find('>', c0), d1 = text.find("</data>", c0);
   if (d0 == std::string::npos || d1 == std::string::npos || doc.count < 1) return false;
   std::istringstream is(text.substr(d0+1, d1-d0-1));
   double v;
   while (is >> v) doc.vals.push_back(v);
   if (doc.vals.empty() || doc.vals.size() % (size_t) doc.count) return false;
   doc.width = (int)(doc.vals.size() / doc.count);
   bool any_group = false;
   for (size_t g=text.find("<group name=\""); g!=std::string::npos && g<c0; g=text.find("<group name=\"", g+1))
   {
      const size_t n0 = g + 13, n1 = text.find('"', n0);
      const size_t o0 = text.find("offset=\"", n1), f0 = text.find("dof=\"", n1);
      if (n1 == std::string::npos || o0 == std::string::npos || f0 == std::string::npos) return false;
      const std::string name = text.substr(n0, n1 - n0);
      const int off = std::atoi(text.c_str() + o0 + 8), dof = std::atoi(text.c_str() + f0 + 5);
      if (off < 0 || dof < 1 || off + dof > doc.width) return false;
      any_group = true;
      if (name.compare(0, 12, "joint_values") == 0) { doc.joint_off = off; doc.joint_dof = dof; }
      else if (name == "deltatime") doc.dt_off = off;
      else if (name.compare(0, 16, "affine_transform") == 0 && dof == 7) doc.base_off = off;
   }
   if (!any_group) { doc.joint_off = 0; doc.joint_dof = doc.width - 1; doc.dt_off = doc.width - 1; }
   return doc.joint_dof >= 1 && doc.dt_off >= 0;
}

void sample_starttraj(const TrajDoc & doc, int n_points, bool floating_base, std::vector<double> & sampled)
{
   const int dof = doc.joint_dof, count = doc.count, c0 = floating_base ? 7 : 0, nn = c0 + dof;
   std::vector<double> tcum(count, 0.0);
   for (int k=1; k<count; k++) tcum[k] = tcum[k-1] + doc.vals[(size_t) k*doc.width + doc.dt_off];
   const double duration = tcum[count-1];
   sampled.resize((size_t) n_points * nn);
   int seg = 0;
   for (int k=0; k<n_points; k++)
   {
      // untimed documents (all deltatimes zero) are sampled uniformly over the waypoint index
      const double t = duration > 0.0 ? k * duration / (n_points - 1) : (double) k * (count - 1) / (n_points - 1);
      double u = 0.0;
      if (duration > 0.0)
      {
         while (seg < count-2 && tcum[seg+1] < t) seg++;
         const double dt = tcum[seg+1] - tcum[seg];
         u = (count > 1 && dt > 0.0) ? (t - tcum[seg]) / dt : 0.0;
      }
      else { seg = std::min((int) t, count-2); if (seg < 0) seg = 0; u = t - seg; }
      if (count == 1) { seg = 0; u = 0.0; }
      int s0 = seg, s1 = std::min(seg+1, count-1);
      // at (and past) the end a trajectory is its last waypoint (OpenRAVE's Sample), also when the last segments take no time
      if (duration > 0.0 && (k == n_points-1 || t >= duration)) { s0 = s1 = count-1; u = 0.0; }
      const double * r0 = &doc.vals[(size_t) s0*doc.width], * r1 = &doc.vals[(size_t) s1*doc.width];
      double * row = &sampled[(size_t) k*nn];
      if (floating_base)
      {
         // the base: OpenRAVE's x y z qw qx qy qz, into libcd's order, normalised (mod.cpp:2389-2399)
         double vec[7];
         for (int j=0; j<7; j++) vec[j] = r0[doc.base_off+j] + (r1[doc.base_off+j] - r0[doc.base_off+j]) * u;
         Pose bp;
         bp.v[0] = vec[0]; bp.v[1] = vec[1]; bp.v[2] = vec[2]; bp.v[3] = vec[4]; bp.v[4] = vec[5]; bp.v[5] = vec[6]; bp.v[6] = vec[3];
         pose_normalize(bp);
         for (int j=0; j<7; j++) row[j] = bp.v[j];
      }
      for (int j=0; j<dof; j++) row[c0+j] = r0[doc.joint_off+j] + (r1[doc.joint_off+j] - r0[doc.joint_off+j]) * u;
   }
}

// conversions of a printf pattern: the number of integer conversions (%d, %i, %u with flags and a width), or -1
// when the pattern holds any other conversion (a caller's pattern is never handed to printf with one)
int count_int_conversions(const std::string & pattern)
{
   int count = 0;
   for (size_t k=0; k<pattern.size(); k++)
   {
      if (pattern[k] != '%') continue;
      if (k + 1 < pattern.size() && pattern[k+1] == '%') { k++; continue; }
      size_t q = k + 1;
      while (q < pattern.size() && (pattern[q] == '0' || pattern[q] == '-' || pattern[q] == '+' || pattern[q] == ' ')) q++;
      while (q < pattern.size() && pattern[q] >= '0' && pattern[q] <= '9') q++;
      if (q >= pattern.size() || (pattern[q] != 'd' && pattern[q] != 'i' && pattern[q] != 'u')) return -1;
      count++; k = q;
   }
   return count;
}

} // namespace orc
