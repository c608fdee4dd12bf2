// env.h -- the environment stand-ins: robots, kinbodies, grabs and the list of signed distance fields.
//
// OpenRAVE's environment (robots, kinbodies, transforms) is third party; the pieces of it the commands and the hot path read
// are held here explicitly.  Host arithmetic only: no HIP in here, so env.cpp builds and runs without a device.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "stages.h"      // Robot, Sdf, SceneTable

namespace orc {

struct KinBody                    // a kinbody of oriented boxes (InitFromBoxes style) and / or triangles (a mesh: KinBody::InitFromTrimesh, the .iv files of the reference's scene)
{
   std::string name;
   Pose transform;
   bool enabled = true;
   struct B { Pose pose; double half[3]; };
   std::vector<B> boxes;
   std::vector<double> tris;      // 9 doubles per triangle, in the kinbody frame
   // <orcdchomp><spheres> of the kinbody (src/orcdchomp_kdata.cpp:79-94), in its own frame (one link): what create
   // reads from a body the robot holds (src/orcdchomp_mod.cpp:2173-2211); `link` is unused
   std::vector<Robot::Sphere> spheres;
};

class Environment
{
public:
   void add_robot(const Robot & r);
   Robot & robot(const std::string & name);
   const Robot & robot(const std::string & name) const { return const_cast<Environment *>(this)->robot(name); }
   void add_kinbody(const KinBody & k);
   KinBody & kinbody(const std::string & name);
   bool has_body(const std::string & name) const;
   Pose body_transform(const std::string & name) const;   // robot or kinbody (a held kinbody: where its link carries it now)
   // RobotBase::Grab(body, link) / Release(body) / ReleaseAllGrabbed()
   void grab(const std::string & robot, const std::string & body, int link);
   void release(const std::string & robot, const std::string & body);
   void note_grab_contacts(Robot & r, Robot::Grab & g);      // fills touch_link / touch_body from the robot's state now
   void refresh_grab_contacts(const std::string & body);     // ... again, for a body that is held (its spheres were redefined)
   void set_kinbody_transform(const std::string & body, const Pose & pose);      // (a held body is re-anchored to its link)
   void release_all(const std::string & robot);
   // the robot as create collects its spheres (src/orcdchomp_mod.cpp:2148-2300): its own in XML order, then those of
   // every held body in GetGrabbed() order, each on the link that holds the body at T_w_rlink^-1 o T_w_klink o pos
   Robot robot_for_run(const std::string & name);

   // fields
   void add_sdf(const std::string & kinbody, const Grid & sdf, const Pose & pose_kinbody_gsdf);
   Sdf * find_sdf(const std::string & kinbody);
   void remove_sdf(const std::string & kinbody);      // (device copies live on while a batch still reads them)
   std::vector<std::shared_ptr<Sdf>> sdfs;
   // the module's fields where their kinbodies stand now, every one of `n_runs` runs in it (what orc_batch_create plans with)
   std::shared_ptr<SceneTable> current_scene(int n_runs);

   // computedistancefield's grid around a body (src/orcdchomp_mod.cpp:377-409): the AABB of its enabled geometry with the body at
   // the world origin, padded, in cubes of 2 cube_extent; g: sizes, lengths and every cell 1.0 (free); pose_gsdf: the grid in the
   // body's frame
   void field_grid(const std::string & kinbody, double cube_extent, double aabb_padding, Grid & g, Pose & pose_gsdf);
   // what that field is built from: the boxes and triangles (9 doubles each) of every enabled kinbody, in world coordinates
   void world_geometry(std::vector<Box> & boxes, std::vector<double> & tris);

private:
   std::map<std::string, Robot> robots_;
   std::map<std::string, KinBody> kinbodies_;
};

} // namespace orc
