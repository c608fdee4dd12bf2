// env.cpp -- the environment stand-ins: the Robot:: methods of stages.h, robots and kinbodies, grab / release / re-anchor, the
// field list, and the geometry computedistancefield reads.  Host arithmetic only (no HIP call, no device).
#include "env.h"
#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace orc {

// ================================================================ Robot ===
bool Robot::does_affect(int dof, int link) const
{
   for (int li=link; li>=0; li=parent[li])
      if (joint_type[li] != 0 && dof_index[li] == dof) return true;
   return false;
}

std::vector<unsigned char> Robot::self_pairs_excluded() const
{
   const int nl = n_links;
   std::vector<unsigned char> excl((size_t) nl * nl, 0);
   for (int a=0; a<nl; a++)
   {
      excl[(size_t) a*nl + a] = 1;
      if (parent[a] >= 0) { excl[(size_t) a*nl + parent[a]] = 1; excl[(size_t) parent[a]*nl + a] = 1; }
   }
   for (const auto & pr : adjacent) { excl[(size_t) pr.first*nl + pr.second] = 1; excl[(size_t) pr.second*nl + pr.first] = 1; }
   std::vector<Xform> frames;
   fk(Pose(), std::vector<double>(n_dof > 0 ? n_dof : 1, 0.0), frames);
   std::vector<double> pw(spheres.size() * 3);
   for (size_t a=0; a<spheres.size(); a++)
   {
      double r[3];
      mat3_vec(frames[spheres[a].link].R, spheres[a].pos, r);
      for (int k=0; k<3; k++) pw[a*3+k] = r[k] + frames[spheres[a].link].t[k];
   }
   for (size_t a=0; a<spheres.size(); a++)
      for (size_t b=a+1; b<spheres.size(); b++)
      {
         double d2 = 0.0;
         for (int k=0; k<3; k++) { const double d = pw[a*3+k] - pw[b*3+k]; d2 += d*d; }
         if (std::sqrt(d2) - (spheres[a].radius + spheres[b].radius) < 0.0)
         {
            excl[(size_t) spheres[a].link*nl + spheres[b].link] = 1;
            excl[(size_t) spheres[b].link*nl + spheres[a].link] = 1;
         }
      }
   return excl;
}

// The re-check's self-collision leg for a robot that holds bodies.  OpenRAVE's CheckSelfCollision tests the robot's links
// against each other (minus adjacent links: self_pairs_excluded, from the ROBOT's own spheres) and every grabbed body against the
// links it was NOT touching when it was grabbed (the grabbing link is always left out).  For the sphere model: a pair of the
// robot's own spheres follows the link rule; two spheres of one held body are one rigid body; a held body's sphere against
// anything else is left out when both ride on the same link, or when the body overlapped that link's own spheres (or that other
// body) at the moment of the grab (Grab::touch_link / touch_body, recorded by Environment::grab -- not in the configuration the run
// is created in: a body that has come to touch a link since the grab is reported against it).
std::vector<unsigned char> Robot::run_self_pairs_excluded(int n_own) const
{
   const int ns = (int) spheres.size();
   std::vector<unsigned char> excl((size_t) ns * ns, 0);
   Robot own = *this;
   own.spheres.resize(n_own);
   const std::vector<unsigned char> link_excl = own.self_pairs_excluded();
   auto body_touches_link = [&](int body, int link) {
      const Grab & g = grabbed[body - 1];
      return link == g.link || (link < (int) g.touch_link.size() && g.touch_link[link] != 0);
   };
   auto bodies_touch = [&](int ba, int bb) {
      const Grab & ga = grabbed[ba - 1], & gb = grabbed[bb - 1];
      for (const std::string & nm : ga.touch_body) if (nm == gb.body) return true;
      for (const std::string & nm : gb.touch_body) if (nm == ga.body) return true;
      return false;
   };
   for (int a=0; a<ns; a++)
      for (int b=a+1; b<ns; b++)
      {
         const int ba = spheres[a].body, bb = spheres[b].body;
         bool ex;
         if (ba == 0 && bb == 0) ex = link_excl[(size_t) spheres[a].link * n_links + spheres[b].link] != 0;
         else if (ba == bb) ex = true;
         else if (ba == 0) ex = body_touches_link(bb, spheres[a].link);
         else if (bb == 0) ex = body_touches_link(ba, spheres[b].link);
         else ex = bodies_touch(ba, bb);
         excl[(size_t) a*ns + b] = excl[(size_t) b*ns + a] = ex ? 1 : 0;
      }
   for (int a=0; a<ns; a++) excl[(size_t) a*ns + a] = 1;
   return excl;
}

void Robot::fk(const Pose & base, const std::vector<double> & q, std::vector<Xform> & frames) const
{
   frames.resize(n_links);
   const Xform xb = xform_from_pose(base);
   for (int li=0; li<n_links; li++)
   {
      const Xform & from = (parent[li] < 0) ? xb : frames[parent[li]];
      Xform xj = xform_mul(from, xform_from_pose(pose_parent_joint[li]));
      if (joint_type[li] == 1)
      {
         Xform rot; rot.R = axis_angle(&axis[3*li], q[dof_index[li]]); rot.t[0] = rot.t[1] = rot.t[2] = 0.0;
         xj = xform_mul(xj, rot);
      }
      else if (joint_type[li] == 2)
      {
         double aw[3];
         mat3_vec(xj.R, &axis[3*li], aw);
         for (int k=0; k<3; k++) xj.t[k] += q[dof_index[li]] * aw[k];
      }
      frames[li] = xj;
   }
}

// ========================================================== Environment ===
void Environment::add_robot(const Robot & r)
{
   if (has_body(r.name)) throw std::runtime_error("a body with that name already exists!");
   robots_[r.name] = r;
}

Robot & Environment::robot(const std::string & name)
{
   auto it = robots_.find(name);
   if (it == robots_.end()) throw std::runtime_error("Could not find robot with that name!");
   return it->second;
}

void Environment::add_kinbody(const KinBody & k)
{
   if (has_body(k.name)) throw std::runtime_error("a body with that name already exists!");
   kinbodies_[k.name] = k;
}

KinBody & Environment::kinbody(const std::string & name)
{
   auto it = kinbodies_.find(name);
   if (it == kinbodies_.end()) throw std::runtime_error("Could not find kinbody with that name!");
   return it->second;
}

bool Environment::has_body(const std::string & name) const
{
   return robots_.count(name) || kinbodies_.count(name);
}

Pose Environment::body_transform(const std::string & name) const
{
   auto r = robots_.find(name);
   if (r != robots_.end()) return r->second.transform;
   auto k = kinbodies_.find(name);
   if (k != kinbodies_.end())
   {
      // a held body moves with the link that holds it (OpenRAVE updates grabbed bodies with the robot's state)
      for (const auto & kv : robots_)
         for (const Robot::Grab & g : kv.second.grabbed)
            if (g.body == name)
            {
               std::vector<Xform> frames;
               kv.second.fk(kv.second.transform, kv.second.dof_values, frames);
               const Xform now = xform_mul(frames[g.link], g.rel);
               return pose_from_dR(now.t, now.R);
            }
      return k->second.transform;
   }
   throw std::runtime_error("KinBody " + name + " referenced by active signed distance field does not exist!\n");
}

void Environment::grab(const std::string & rname, const std::string & body, int link)
{
   Robot & r = robot(rname);
   KinBody & k = kinbody(body);
   if (link < 0 || link >= r.n_links) throw std::runtime_error("grabbing link out of range!");
   for (const auto & kv : robots_)
      for (const Robot::Grab & g : kv.second.grabbed)
         if (g.body == body) throw std::runtime_error("that kinbody is already grabbed!");
   std::vector<Xform> frames;
   r.fk(r.transform, r.dof_values, frames);
   Robot::Grab g;
   g.body = body; g.link = link;
   g.rel = xform_mul(xform_inverse(frames[link]), xform_from_pose(k.transform));
   note_grab_contacts(r, g);
   r.grabbed.push_back(g);
}

// What a body overlaps at the moment it is grabbed (or re-anchored): the robot's links, by the robot's own <orcdchomp> spheres
// against the body's, and the bodies the robot holds already.  RobotBase::Grab records the links in collision with the body and
// CheckSelfCollision ignores them afterwards (third party; src/orcdchomp_mod.cpp:2998-2999 calls it).
void Environment::note_grab_contacts(Robot & r, Robot::Grab & g)
{
   g.touch_link.assign(r.n_links, 0);
   g.touch_body.clear();
   const KinBody & k = kinbody(g.body);
   std::vector<Xform> frames;
   r.fk(r.transform, r.dof_values, frames);
   auto world = [&](const Xform & x, const double pos[3], double out[3]) {
      mat3_vec(x.R, pos, out);
      for (int q=0; q<3; q++) out[q] += x.t[q];
   };
   const Xform xb = xform_mul(frames[g.link], g.rel);
   std::vector<double> pb(k.spheres.size() * 3);
   for (size_t a=0; a<k.spheres.size(); a++) world(xb, k.spheres[a].pos, &pb[a*3]);
   auto overlap = [](const double * p, double rp, const double * q, double rq) {
      double d2 = 0.0;
      for (int c=0; c<3; c++) { const double d = p[c] - q[c]; d2 += d*d; }
      return std::sqrt(d2) - (rp + rq) < 0.0;
   };
   for (const Robot::Sphere & sp : r.spheres)
   {
      double pw[3];
      world(frames[sp.link], sp.pos, pw);
      for (size_t a=0; a<k.spheres.size(); a++)
         if (overlap(pw, sp.radius, &pb[a*3], k.spheres[a].radius)) { g.touch_link[sp.link] = 1; break; }
   }
   for (const Robot::Grab & other : r.grabbed)
   {
      if (other.body == g.body) continue;
      const KinBody & ko = kinbody(other.body);
      const Xform xo = xform_mul(frames[other.link], other.rel);
      bool hit = false;
      for (size_t a=0; a<ko.spheres.size() && !hit; a++)
      {
         double po[3];
         world(xo, ko.spheres[a].pos, po);
         for (size_t c=0; c<k.spheres.size() && !hit; c++)
            if (overlap(po, ko.spheres[a].radius, &pb[c*3], k.spheres[c].radius)) hit = true;
      }
      if (hit) g.touch_body.push_back(other.body);
   }
}

// SetTransform of a kinbody.  A body the robot holds is moved where the caller says and rides with its link from THERE
// (the grab's relative transform is taken anew): a binding that copies every body's pose before a command passes a held
// body's current pose, which changes nothing.
void Environment::set_kinbody_transform(const std::string & body, const Pose & pose)
{
   KinBody & k = kinbody(body);
   k.transform = pose;
   for (auto & kv : robots_)
      for (Robot::Grab & g : kv.second.grabbed)
         if (g.body == body)
         {
            std::vector<Xform> frames;
            kv.second.fk(kv.second.transform, kv.second.dof_values, frames);
            g.rel = xform_mul(xform_inverse(frames[g.link]), xform_from_pose(pose));
            note_grab_contacts(kv.second, g);      // (a new anchoring is a new grab: what it touches is taken from here)
         }
}

void Environment::refresh_grab_contacts(const std::string & body)
{
   for (auto & kv : robots_)
      for (Robot::Grab & g : kv.second.grabbed)
         if (g.body == body) note_grab_contacts(kv.second, g);
}

void Environment::release(const std::string & rname, const std::string & body)
{
   Robot & r = robot(rname);
   for (size_t i=0; i<r.grabbed.size(); i++)
      if (r.grabbed[i].body == body)
      {
         kinbody(body).transform = body_transform(body);      // the body stays where the link left it
         r.grabbed.erase(r.grabbed.begin() + i);
         return;
      }
   throw std::runtime_error("the robot is not grabbing that kinbody!");
}

void Environment::release_all(const std::string & rname)
{
   Robot & r = robot(rname);
   while (!r.grabbed.empty()) release(rname, r.grabbed.back().body);
}

Robot Environment::robot_for_run(const std::string & rname)
{
   Robot eff = robot(rname);
   // a body without spheres, the robot itself included (src/orcdchomp_mod.cpp:2262-2263)
   if (eff.spheres.empty()) throw std::runtime_error("no spheres! kinbody does not have a <orcdchomp> tag defined?");
   int body_index = 0;
   for (const Robot::Grab & g : eff.grabbed)
   {
      body_index++;
      const KinBody & k = kinbody(g.body);
      if (k.spheres.empty()) throw std::runtime_error("no spheres! kinbody does not have a <orcdchomp> tag defined?");
      for (const Robot::Sphere & ks : k.spheres)
      {
         // T_w_rlink^-1 o T_w_klink o pos (mod.cpp:2200-2208); the held body is rigid with its link, so the product of
         // the first two is what the grab recorded
         Robot::Sphere sp;
         sp.link = g.link; sp.radius = ks.radius; sp.body = body_index;
         mat3_vec(g.rel.R, ks.pos, sp.pos);
         for (int q=0; q<3; q++) sp.pos[q] += g.rel.t[q];
         eff.spheres.push_back(sp);
      }
   }
   return eff;
}

Sdf * Environment::find_sdf(const std::string & kinbody)
{
   for (auto & s : sdfs) if (s->kinbody_name == kinbody) return s.get();
   return nullptr;
}

void Environment::add_sdf(const std::string & kb, const Grid & g, const Pose & pose)
{
   if (find_sdf(kb)) throw std::runtime_error("We already have an sdf for this kinbody!");
   for (int d=0; d<3; d++)
      if (g.sizes[d] < 2) throw std::runtime_error("sdf grids need at least 2 cells per dimension!");
   std::shared_ptr<Sdf> s = std::make_shared<Sdf>();
   s->kinbody_name = kb;
   s->pose = pose;
   s->grid = g;
   sdfs.push_back(std::move(s));
}

int SceneTable::max_fields() const
{
   size_t f = 0;
   for (const auto & sc : scenes) f = std::max(f, sc.size());
   return (int) f;
}

std::shared_ptr<SceneTable> Environment::current_scene(int n_runs)
{
   std::shared_ptr<SceneTable> t = std::make_shared<SceneTable>();
   t->scenes.resize(1);
   for (const auto & s : sdfs) t->scenes[0].push_back({ s, body_transform(s->kinbody_name) });
   t->scene_of_run.assign(std::max(n_runs, 0), 0);
   return t;
}

void Environment::remove_sdf(const std::string & kb)
{
   for (size_t k=0; k<sdfs.size(); k++)
      if (sdfs[k]->kinbody_name == kb)
      {
         sdfs.erase(sdfs.begin() + k);      // device copies live on while a batch still reads them
         return;
      }
   throw std::runtime_error("No sdf for that kinbody!");
}

// src/orcdchomp_mod.cpp:377-409
void Environment::field_grid(const std::string & kb, double cube_extent, double aabb_padding, Grid & g, Pose & pose_gsdf)
{
   // AABB of the enabled geometry with the body at the world origin (mod.cpp:377-381, 88-140)
   double amin[3] = {0,0,0}, amax[3] = {0,0,0};
   bool init = false;
   if (kinbodies_.count(kb))
   {
      const KinBody & k = kinbodies_[kb];
      if (k.enabled) for (size_t v=0; v<k.tris.size()/3; v++)      // (a mesh: the box around its vertices)
         for (int r=0; r<3; r++)
         {
            const double c = k.tris[3*v + r];
            if (!init) { amin[r] = c; amax[r] = c; }
            else { if (amin[r] > c) amin[r] = c; if (amax[r] < c) amax[r] = c; }
            if (r == 2) init = true;
         }
      if (k.enabled) for (const KinBody::B & bx : k.boxes)
      {
         const Xform x = xform_from_pose(bx.pose);
         double ext[3];
         for (int r=0; r<3; r++)
            ext[r] = std::fabs(x.R.m[r*3+0])*bx.half[0] + std::fabs(x.R.m[r*3+1])*bx.half[1] + std::fabs(x.R.m[r*3+2])*bx.half[2];
         if (ext[0] == 0 && ext[1] == 0 && ext[2] == 0) continue;
         for (int r=0; r<3; r++)
         {
            const double lo = x.t[r] - ext[r], hi = x.t[r] + ext[r];
            if (!init) { amin[r] = lo; amax[r] = hi; }
            else { if (amin[r] > lo) amin[r] = lo; if (amax[r] < hi) amax[r] = hi; }
         }
         init = true;
      }
   }
   double apos[3], aext[3];
   for (int r=0; r<3; r++)
   {
      if (init) { apos[r] = 0.5 * (amin[r] + amax[r]); aext[r] = amax[r] - apos[r]; }
      else { apos[r] = 0.0; aext[r] = 0.0; }      // identity transform translation (mod.cpp:131-134)
   }

   for (int r=0; r<3; r++)
   {
      g.sizes[r] = (int) std::ceil((aext[r] + aabb_padding) / cube_extent);      // mod.cpp:391
      g.lengths[r] = g.sizes[r] * 2.0 * cube_extent;                              // mod.cpp:403
   }
   for (int r=0; r<3; r++)
      if (g.sizes[r] < 2) throw std::runtime_error("Not enough memory for distance field!");
   pose_gsdf = Pose();
   for (int r=0; r<3; r++) pose_gsdf.v[r] = apos[r] - 0.5 * g.lengths[r];         // mod.cpp:407-409
   g.data.assign(g.ncells(), 1.0);
}

// (mod.cpp:462-531 asks OpenRAVE's CheckCollision, which sees every enabled body of the world)
void Environment::world_geometry(std::vector<Box> & boxes, std::vector<double> & tris)
{
   for (auto & kv : kinbodies_)
   {
      const KinBody & k = kv.second;
      if (!k.enabled) continue;
      const Xform xk = xform_from_pose(body_transform(kv.first));      // (a held body is where its link is NOW)
      for (size_t v=0; v<k.tris.size()/3; v++)
      {
         double w[3];
         mat3_vec(xk.R, &k.tris[3*v], w);
         for (int r=0; r<3; r++) tris.push_back(w[r] + xk.t[r]);
      }
      for (const KinBody::B & bx : k.boxes)
      {
         Box b;
         b.world = xform_mul(xk, xform_from_pose(bx.pose));
         for (int r=0; r<3; r++) b.half[r] = bx.half[r];
         boxes.push_back(b);
      }
   }
}

} // namespace orc
