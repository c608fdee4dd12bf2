// trajdoc.h -- OpenRAVE-style trajectory documents: what gettraj writes, what `create starttraj` reads and samples, and the check of
// a caller's printf pattern for the files they go to.  Host arithmetic only (no HIP).
#pragma once
#include <string>
#include <vector>

namespace orc {

// an OpenRAVE-style trajectory document holding the waypoints of one run
// (stands in for t->serialize(sout), src/orcdchomp_mod.cpp:3008).  One row per waypoint:
// the joint values followed by the deltatime to reach it from the previous waypoint.
std::string serialize_traj(const std::string & robot, const std::vector<int> & adofs,
   const double * traj, int n_points, int n, int col0, const std::vector<double> & deltatime);

// reads a trajectory document: the rows of its <data> block and where its groups sit in a row.  A document without
// a <configuration> block (the bare form the tests also pass) is joint values followed by one deltatime.
struct TrajDoc
{
   int count = 0, width = 0;
   std::vector<double> vals;                       // [count][width]
   int joint_off = 0, joint_dof = 0, dt_off = -1, base_off = -1;
};
bool parse_traj(const std::string & text, TrajDoc & doc);
// initialisation from a passed trajectory (src/orcdchomp_mod.cpp:2375-2416): sampled at i * duration / (n_points-1), linear
// interpolation between its waypoints; sampled [n_points][(floating_base ? 7 : 0) + joint_dof], the base in libcd's order
void sample_starttraj(const TrajDoc & doc, int n_points, bool floating_base, std::vector<double> & sampled);

int count_int_conversions(const std::string & pattern);   // integer conversions of a printf pattern, -1: it holds another kind

} // namespace orc
