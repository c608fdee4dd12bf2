// commands.cpp -- the SendCommand layer: the command grammar of the reference, argument loop by argument loop.
// Reference: src/orcdchomp_mod.cpp (commands), src/orcwrap.cpp (argv adaptor).
#include "module.h"
#include "launch.h"
#include "trajdoc.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>

namespace orc {

// a field is built on the GPU for large grids (or ORC_SDF_DEVICE=1), on the host otherwise (ORC_SDF_DEVICE=0 forces the host);
// both give the same cells bit for bit
static bool sdf_on_device(size_t ncells)
{
   const char * env = getenv("ORC_SDF_DEVICE");
   return env ? (atoi(env) != 0) : (ncells >= (size_t) 1 << 18);
}

// occupancy -> signed distance field
static void bin_sdf_any(const Grid & occ, Grid & sdf, hipStream_t st)
{
   if (!sdf_on_device(occ.ncells())) { grid_bin_sdf(occ, sdf); return; }
   sdf = occ;
   hip_check(orc_sdf_from_occupancy_device(occ.data.data(), sdf.data.data(), occ.sizes, occ.lengths, st), "sdf build");
}

namespace {

std::vector<double> parse_vector(const std::string & s)
{
   std::vector<double> out;
   for (const std::string & tok : shparse(s)) out.push_back(std::atof(tok.c_str()));
   return out;
}

void bad_arguments() { throw std::runtime_error("Bad arguments!"); }

void * parse_pointer(const std::string & s)
{
   void * p = nullptr;
   if (std::sscanf(s.c_str(), "%p", &p) != 1) return nullptr;
   return p;
}

// the TSR tokens of `create` that name no link: the active manipulator's end effector, or the token's own message
void on_active_manip(TsrSpec & t, const Robot & rb, const char * msg)
{
   if (rb.manips.empty()) throw std::runtime_error(msg);
   t.ee_link = rb.manips[rb.active_manip].link; t.tool = rb.manips[rb.active_manip].tool;
}

} // namespace

std::string Module::send_command(const std::string & cmd)
{
   // orcwrap_call (src/orcwrap.cpp:37-69): tokenise; argv[0] is the command name
   std::vector<std::string> argv = shparse(cmd);
   if (argv.empty()) throw std::runtime_error("empty command!");
   const std::string name = argv[0];
   if (name == "computedistancefield") return cmd_computedistancefield(argv);
   if (name == "addfield_fromobsarray") return cmd_addfield_fromobsarray(argv);
   if (name == "removefield") return cmd_removefield(argv);
   if (name == "mergefields") return cmd_mergefields(argv);
   if (name == "create") return cmd_create(argv, false);
   if (name == "createbatch") return cmd_create(argv, true);
   if (name == "iterate") return cmd_iterate(argv, false);
   if (name == "iteratebatch") return cmd_iterate(argv, true);
   if (name == "gettraj") return cmd_gettraj(argv, false);
   if (name == "gettrajbatch") return cmd_gettraj(argv, true);
   if (name == "destroy") return cmd_destroy(argv);
   if (name == "viewspheres" || name == "viewfields")
      throw std::runtime_error("command " + name + " needs an OpenRAVE viewer and is not part of this build");
   throw std::runtime_error("unknown command " + name);
}

// src/orcdchomp_mod.cpp:297-589
std::string Module::cmd_computedistancefield(const std::vector<std::string> & argv)
{
   std::string kb;
   double cube_extent = 0.02, aabb_padding = 0.2;
   std::string cache_filename;
   bool have_cache = false, require_cache = false;
   const int argc = (int) argv.size();
   int i;
   for (i=1; i<argc; i++)
   {
      if (argv[i] == "kinbody" && i+1 < argc)
      {
         if (!kb.empty()) throw std::runtime_error("Only one kinbody can be passed!");
         kb = argv[++i];
         if (!env.has_body(kb)) throw std::runtime_error("Could not find kinbody with that name!");
      }
      else if (argv[i] == "aabb_padding" && i+1 < argc) aabb_padding = std::atof(argv[++i].c_str());
      else if (argv[i] == "cube_extent" && i+1 < argc) cube_extent = std::atof(argv[++i].c_str());
      else if (argv[i] == "cache_filename" && i+1 < argc) { cache_filename = argv[++i]; have_cache = true; }
      else if (argv[i] == "require_cache") require_cache = true;
      else break;
   }
   if (i < argc) bad_arguments();
   if (kb.empty()) throw std::runtime_error("Did not pass all required args!");
   if (env.find_sdf(kb)) throw std::runtime_error("We already have an sdf for this kinbody!");

   Grid g;
   Pose pose_gsdf;
   env.field_grid(kb, cube_extent, aabb_padding, g, pose_gsdf);

   bool loaded = false;
   if (have_cache)
   {
      // raw doubles, C order, no header; validated by size only (mod.cpp:416-444)
      std::ifstream fp(cache_filename.c_str(), std::ios::binary | std::ios::ate);
      if (fp)
      {
         const std::streamoff sz = fp.tellg();
         if ((size_t) sz == g.ncells() * sizeof(double))
         {
            fp.seekg(0);
            fp.read((char *) g.data.data(), sz);
            loaded = (bool) fp;
         }
      }
   }
   if (!loaded)
   {
      if (require_cache) throw std::runtime_error("Field not found from cache, but require_cache flag set!");
      // occupancy by sweeping a cube of half-extent cube_extent over the cell centres
      // (mod.cpp:462-531; OpenRAVE's CheckCollision replaced by a box-box test)
      const Pose pose_world_gsdf = pose_compose(env.body_transform(kb), pose_gsdf);
      std::vector<Box> obstacles;
      std::vector<double> tris;                                            // 9 doubles per triangle, world coordinates
      env.world_geometry(obstacles, tris);
      // voxelize -> flood fill from cell 0 (reachable 1.0 -> 0.0, the rest becomes obstacle,
      // mod.cpp:540-548) -> signed distance field (mod.cpp:560): on the GPU for large grids
      // (or ORC_SDF_DEVICE=1), on the host otherwise; both give the same cells bit for bit
      if (sdf_on_device(g.ncells()))
      {
         DeviceGuard guard(device);
         std::vector<double> bx;                       // per box: R[9] t[3] half[3]
         for (const Box & b : obstacles)
         {
            bx.insert(bx.end(), b.world.R.m, b.world.R.m + 9);
            bx.insert(bx.end(), b.world.t, b.world.t + 3);
            bx.insert(bx.end(), b.half, b.half + 3);
         }
         const Xform xg = xform_from_pose(pose_world_gsdf);
         double gx[12];
         for (int q=0; q<9; q++) gx[q] = xg.R.m[q];
         for (int q=0; q<3; q++) gx[9+q] = xg.t[q];
         hip_check(orc_sdf_build_device(g.sizes, g.lengths, gx, pose_world_gsdf.v, cube_extent, (int) obstacles.size(), bx.data(), (int)(tris.size() / 9), tris.data(),
                                        g.data.data(), stream), "sdf build");
      }
      else
      {
         voxelize_boxes(g, pose_world_gsdf, cube_extent, obstacles, tris);
         grid_flood_1_to_0(g, 0);                                                   // mod.cpp:540-548
         const size_t nc = g.ncells();
         for (size_t idx=0; idx<nc; idx++) if (g.data[idx] == 1.0) g.data[idx] = HUGE_VAL;
         Grid sdf;
         grid_bin_sdf(g, sdf);                                                      // mod.cpp:560
         g = sdf;
      }
      if (have_cache)
      {
         std::ofstream fp(cache_filename.c_str(), std::ios::binary);
         fp.write((const char *) g.data.data(), g.ncells() * sizeof(double));
      }
   }
   env.add_sdf(kb, g, pose_gsdf);
   return "";
}

// src/orcdchomp_mod.cpp:592-722
std::string Module::cmd_addfield_fromobsarray(const std::vector<std::string> & argv)
{
   std::string kb;
   double * obsarray = nullptr;
   int sizes[3] = {0,0,0};
   double lengths[3] = {0,0,0};
   Pose pose;
   const int argc = (int) argv.size();
   int i;
   for (i=1; i<argc; i++)
   {
      if (argv[i] == "kinbody" && i+1 < argc)
      {
         if (!kb.empty()) throw std::runtime_error("Only one kinbody can be passed!");
         kb = argv[++i];
         if (!env.has_body(kb)) throw std::runtime_error("Could not find kinbody with that name!");
      }
      else if (argv[i] == "obsarray" && i+1 < argc) obsarray = (double *) parse_pointer(argv[++i]);
      else if (argv[i] == "sizes" && i+1 < argc)
      {
         std::vector<std::string> t = shparse(argv[++i]);
         if (t.size() != 3) throw std::runtime_error("sizes must be length 3!");
         for (int j=0; j<3; j++) sizes[j] = std::atoi(t[j].c_str());
      }
      else if (argv[i] == "lengths" && i+1 < argc)
      {
         std::vector<double> t = parse_vector(argv[++i]);
         if (t.size() != 3) throw std::runtime_error("lengths must be length 3!");
         for (int j=0; j<3; j++) lengths[j] = t[j];
      }
      else if (argv[i] == "pose" && i+1 < argc)
      {
         std::vector<double> t = parse_vector(argv[++i]);
         if (t.size() != 7) throw std::runtime_error("pose must be length 7!");
         for (int j=0; j<7; j++) pose.v[j] = t[j];
      }
      else break;
   }
   if (i < argc) bad_arguments();
   if (kb.empty()) throw std::runtime_error("Did not pass a kinbody!");
   if (!obsarray) throw std::runtime_error("Did not pass an obsarray!");
   for (int j=0; j<3; j++) if (sizes[j] <= 0) throw std::runtime_error("Didn't pass non-zero sizes!");
   for (int j=0; j<3; j++) if (lengths[j] <= 0.0) throw std::runtime_error("Didn't pass non-zero lengths!");
   pose_normalize(pose);
   if (env.find_sdf(kb)) throw std::runtime_error("We already have an sdf for this kinbody!");
   Grid occ;
   for (int j=0; j<3; j++) { occ.sizes[j] = sizes[j]; occ.lengths[j] = lengths[j]; }
   // the reference takes ownership of the malloc'd array (mod.cpp:702-704); this build
   // copies it and leaves ownership with the caller (no cross-allocator free)
   occ.data.assign(obsarray, obsarray + occ.ncells());
   Grid sdf;
   bin_sdf_any(occ, sdf, stream);
   env.add_sdf(kb, sdf, pose);
   return "";
}

// src/orcdchomp_mod.cpp:799-847
std::string Module::cmd_removefield(const std::vector<std::string> & argv)
{
   std::string kb;
   const int argc = (int) argv.size();
   int i;
   for (i=1; i<argc; i++)
   {
      if (argv[i] == "kinbody" && i+1 < argc)
      {
         if (!kb.empty()) throw std::runtime_error("Only one kinbody can be passed!");
         kb = argv[++i];
      }
      else break;
   }
   if (i < argc) bad_arguments();
   if (kb.empty()) throw std::runtime_error("Did not pass a kinbody!");
   env.remove_sdf(kb);
   return "";
}

// additive: mergefields kinbody NAME fields 'A B C' cell F [bounds 'x0 y0 z0 x1 y1 z1'] -- orc_scene_merge_fields with every
// source where its kinbody stands now
std::string Module::cmd_mergefields(const std::vector<std::string> & argv)
{
   std::string kb;
   std::vector<std::string> fields;
   std::vector<double> bounds;
   double cell = 0.0;
   bool have_fields = false, have_cell = false, have_bounds = false;
   const int argc = (int) argv.size();
   int i;
   for (i=1; i<argc; i++)
   {
      if (argv[i] == "kinbody" && i+1 < argc)
      {
         if (!kb.empty()) throw std::runtime_error("Only one kinbody can be passed!");
         kb = argv[++i];
      }
      else if (argv[i] == "fields" && i+1 < argc) { fields = shparse(argv[++i]); have_fields = true; }
      else if (argv[i] == "cell" && i+1 < argc) { cell = std::atof(argv[++i].c_str()); have_cell = true; }
      else if (argv[i] == "bounds" && i+1 < argc)
      {
         bounds = parse_vector(argv[++i]);
         if (bounds.size() != 6) throw std::runtime_error("bounds must be length 6!");
         have_bounds = true;
      }
      else break;
   }
   if (i < argc) bad_arguments();
   if (kb.empty() || !have_fields || !have_cell) throw std::runtime_error("Did not pass all required args!");
   merge_fields(kb, fields, nullptr, cell, have_bounds ? bounds.data() : nullptr);
   return "";
}

// tsr_create_parse, src/orcdchomp_mod.cpp:3068-3111: "manipindex bodyandlink" + T0w (rotation column
// by column, then translation) + Twe (the same) + Bw [6][2]; 38 fields
static bool parse_tsr(const std::string & str, TsrSpec & t)
{
   // the wire format of a TSR (tsr_create_parse, src/orcdchomp_mod.cpp:3068-3111): manipulator index, "body link"
   // word, then 36 numbers: T0w and Twe as a rotation column by column followed by the translation, Bw row by row
   std::istringstream in(str);
   int manipindex; std::string bodyandlink;
   if (!(in >> manipindex >> bodyandlink) || bodyandlink.size() > 31) return false;
   double num[36];
   for (double & v : num) if (!(in >> v)) return false;
   Pose * frames[2] = { &t.T0w, &t.Twe };
   for (int f=0; f<2; f++)
   {
      const double * block = num + 12*f;
      Mat3 R;
      for (int col=0; col<3; col++) for (int row=0; row<3; row++) R.m[3*row+col] = block[3*col+row];
      *frames[f] = pose_from_dR(block + 9, R);
   }
   for (int k=0; k<12; k++) t.Bw[k/2][k%2] = num[24+k];
   return true;
}

// src/orcdchomp_mod.cpp:1800-2688 (argument grammar 1888-2085)
std::string Module::cmd_create(const std::vector<std::string> & argv, bool batchmode)
{
   std::string rname;
   std::vector<double> adofgoal, basegoal;
   bool have_adofgoal = false, have_basegoal = false, have_starttraj = false;
   std::string starttraj;
   BatchParams p;
   unsigned int seed = 0;
   int n_runs = 1;
   std::string dat_filename;
   std::vector<int> devs; bool have_devs = false;
   std::vector<TsrSpec> con_tsrs, everyn_tsr, start_tsr;
   const double * goals_ptr = nullptr, * starts_ptr = nullptr, * basegoals_ptr = nullptr;
   const unsigned int * seeds_ptr = nullptr;
   const int argc = (int) argv.size();
   int i;
   for (i=1; i<argc; i++)
   {
      const std::string & a = argv[i];
      if (a == "robot" && i+1 < argc)
      {
         if (!rname.empty()) throw std::runtime_error("Only one robot can be passed!");
         rname = argv[++i];
         env.robot(rname);
      }
      else if (a == "adofgoal" && i+1 < argc)
      {
         if (have_adofgoal) throw std::runtime_error("Only one adofgoal can be passed!");
         if (have_starttraj) throw std::runtime_error("Cannot pass both adofgoal and starttraj!");
         adofgoal = parse_vector(argv[++i]); have_adofgoal = true;
      }
      else if (a == "basegoal" && i+1 < argc)
      {
         if (have_basegoal) throw std::runtime_error("Only one basegoal can be passed!");
         basegoal = parse_vector(argv[++i]);
         if (basegoal.size() != 7) throw std::runtime_error("basegoal argument must be length 7!");
         have_basegoal = true;
      }
      else if (a == "floating_base") p.floating_base = 1;
      else if (a == "lambda" && i+1 < argc) p.lambda = std::atof(argv[++i].c_str());
      else if (a == "n_points" && i+1 < argc) p.n_points = std::atoi(argv[++i].c_str());
      else if (a == "derivative" && i+1 < argc) p.derivative = std::atoi(argv[++i].c_str());
      else if (a == "use_momentum") p.use_momentum = 1;
      else if (a == "use_hmc") p.use_hmc = 1;
      else if (a == "hmc_resample_lambda" && i+1 < argc) p.hmc_resample_lambda = std::atof(argv[++i].c_str());
      else if (a == "seed" && i+1 < argc) std::sscanf(argv[++i].c_str(), "%u", &seed);
      else if (a == "epsilon" && i+1 < argc) p.epsilon = std::atof(argv[++i].c_str());
      else if (a == "epsilon_self" && i+1 < argc) p.epsilon_self = std::atof(argv[++i].c_str());
      else if (a == "obs_factor" && i+1 < argc) p.obs_factor = std::atof(argv[++i].c_str());
      else if (a == "obs_factor_self" && i+1 < argc) p.obs_factor_self = std::atof(argv[++i].c_str());
      else if (a == "no_report_cost") { /* emitted by the python layer, ignored */ }
      else if (a == "dat_filename" && i+1 < argc) dat_filename = argv[++i];
      else if (a == "starttraj" && i+1 < argc)
      {
         if (have_starttraj) throw std::runtime_error("Only one starttraj can be passed!");
         if (have_adofgoal) throw std::runtime_error("Cannot pass both adofgoal and starttraj!");
         starttraj = argv[++i]; have_starttraj = true;
      }
      else if (a == "con_tsr" && i+2 < argc)
      {
         // src/orcdchomp_mod.cpp:1930-1987: TYPE | TYPE manipee NAME | TYPE link NAME, then the TSR
         if (rname.empty()) throw std::runtime_error("You must pass robot before any con_tsrs!");
         Robot & rb = env.robot(rname);
         const std::vector<std::string> head = shparse(argv[++i]);
         if (head.size() != 1 && head.size() != 3) throw std::runtime_error("con_tsr first argument must be length 1 or 3!");
         if (head[0] != "all") throw std::runtime_error("con_tsr first arg must be start, end, or all!");
         TsrSpec t;
         if (head.size() != 3) on_active_manip(t, rb, "con_tsr manip not found!");
         else if (head[1] == "manipee")
         {
            size_t ui = 0;
            for (; ui<rb.manips.size(); ui++) if (rb.manips[ui].name == head[2]) break;
            if (!(ui < rb.manips.size())) throw std::runtime_error("con_tsr manip not found!");
            t.ee_link = rb.manips[ui].link; t.tool = rb.manips[ui].tool;
         }
         else if (head[1] == "link")
         {
            for (int li=0; li<rb.n_links; li++)
               if ((li < (int) rb.link_names.size() ? rb.link_names[li] : "link" + std::to_string(li)) == head[2]) t.ee_link = li;
            if (t.ee_link < 0) throw std::runtime_error("con_tsr link not found!");
         }
         else throw std::runtime_error("con_tsr first arg must be empty, manipee, or link!");
         if (!parse_tsr(argv[++i], t)) throw std::runtime_error("Cannot parse constraint TSR!");
         con_tsrs.push_back(t);
      }
      else if (a == "everyn_tsr" && i+1 < argc)
      {
         // src/orcdchomp_mod.cpp:1993-1997; applied to the active manipulator's end effector (mod.cpp:1548)
         if (rname.empty()) throw std::runtime_error("You must pass robot before any con_tsrs!");
         Robot & rb = env.robot(rname);
         TsrSpec t;
         if (!parse_tsr(argv[++i], t)) throw std::runtime_error("Cannot parse everyn_tsr TSR!");
         on_active_manip(t, rb, "everyn_tsr needs an active manipulator!");
         everyn_tsr.clear(); everyn_tsr.push_back(t);
      }
      else if (a == "start_tsr" && i+1 < argc)
      {
         // src/orcdchomp_mod.cpp:1988-1992: the start point becomes a variable held on this TSR by a hard
         // constraint (m = n_points-1; mod.cpp:2316-2323, 2570-2576); the active manipulator's end effector (mod.cpp:1704)
         if (rname.empty()) throw std::runtime_error("You must pass robot before any con_tsrs!");
         Robot & rb = env.robot(rname);
         TsrSpec t;
         if (!parse_tsr(argv[++i], t)) throw std::runtime_error("Cannot parse start_tsr TSR!");
         on_active_manip(t, rb, "start_tsr needs an active manipulator!");
         t.point = 0;
         start_tsr.clear(); start_tsr.push_back(t);
      }
      else if ((a == "start_cost" || a == "ee_force" || a == "ee_force_at" || a == "ee_torque_weights") && i+1 < argc)
         throw std::runtime_error("argument " + a + " is outside the scope of this build (SURVEY.md section 2)");
      else if (batchmode && a == "n_runs" && i+1 < argc) n_runs = std::atoi(argv[++i].c_str());
      else if (batchmode && a == "adofgoals" && i+1 < argc) goals_ptr = (const double *) parse_pointer(argv[++i]);
      else if (batchmode && a == "adofstarts" && i+1 < argc) starts_ptr = (const double *) parse_pointer(argv[++i]);
      else if (batchmode && a == "basegoals" && i+1 < argc) basegoals_ptr = (const double *) parse_pointer(argv[++i]);
      else if (batchmode && a == "seeds" && i+1 < argc) seeds_ptr = (const unsigned int *) parse_pointer(argv[++i]);
      else if (batchmode && a == "precision" && i+1 < argc) p.precision = std::atoi(argv[++i].c_str());
      else if (batchmode && a == "devices" && i+1 < argc)
      {
         for (const std::string & t : shparse(argv[++i])) devs.push_back(std::atoi(t.c_str()));
         if (devs.empty()) throw std::runtime_error("devices must name at least one device!");
         have_devs = true;
      }
      else break;
   }
   if (i < argc) bad_arguments();
   if (rname.empty()) throw std::runtime_error("Did not pass a robot!");
   if (!batchmode)
   {
      if (!have_adofgoal && !have_starttraj) throw std::runtime_error("Did not pass either adofgoal or starttraj!");
      if (p.floating_base && !have_basegoal && !have_starttraj) throw std::runtime_error("Passed floating_base with no basegoal!");
      if (!p.floating_base && have_basegoal) throw std::runtime_error("Passed basegoal with no floating_base!");
   }
   else
   {
      if (!goals_ptr) throw std::runtime_error("Did not pass either adofgoal or starttraj!");
      if (p.floating_base && !basegoals_ptr) throw std::runtime_error("Passed floating_base with no basegoal!");
      if (!p.floating_base && basegoals_ptr) throw std::runtime_error("Passed basegoal with no floating_base!");
      if (n_runs < 1) throw std::runtime_error("n_runs must be >=1!");
   }
   if (env.sdfs.empty()) throw std::runtime_error("No signed distance fields have yet been computed!");
   if (p.lambda < 0.01) throw std::runtime_error("lambda must be >=0.01!");
   if (p.n_points < 3) throw std::runtime_error("n_points must be >=3!");
   // a single run (the reference's `create`) gets the latency shape: eight wavefronts on the one run
   // (its trajectory is the one it has in a batch, bit for bit; its cost sums are grouped differently)
   if (!batchmode) p.workgroup_threads = 512;
   // the constraints in the reference's order of addition (src/orcdchomp_mod.cpp:2582-2612)
   if (p.floating_base && !start_tsr.empty()) throw std::runtime_error("floating_base and start_tsr together is not yet implemented!");   // mod.cpp:2100
   p.free_start = start_tsr.empty() ? 0 : 1;
   p.tsrs = start_tsr;
   p.tsrs.insert(p.tsrs.end(), everyn_tsr.begin(), everyn_tsr.end());
   p.tsrs.insert(p.tsrs.end(), con_tsrs.begin(), con_tsrs.end());
   Robot & r = env.robot(rname);
   // initialisation from a passed trajectory (src/orcdchomp_mod.cpp:2375-2416): sampled at
   // i * duration / (n_points-1), linear interpolation between its waypoints
   std::vector<double> sampled;
   if (!batchmode && have_starttraj)
   {
      TrajDoc doc;
      if (!parse_traj(starttraj, doc)) throw std::runtime_error("Cannot parse starttraj!");
      const int dof = doc.joint_dof, c0 = p.floating_base ? 7 : 0, nn = c0 + dof;
      if (dof != (int) r.active_dofs.size()) throw std::runtime_error("size of adofgoal does not match active dofs!");
      if (p.floating_base && doc.base_off < 0) throw std::runtime_error("starttraj with floating_base needs an affine_transform group!");
      sample_starttraj(doc, p.n_points, p.floating_base != 0, sampled);
      adofgoal.assign(sampled.end() - dof, sampled.end());
      if (p.floating_base) { basegoal.assign(sampled.end() - nn, sampled.end() - dof); have_basegoal = true; }
   }
   if (!batchmode && adofgoal.size() != r.active_dofs.size())
      throw std::runtime_error("size of adofgoal does not match active dofs!");
   int id;
   if (!batchmode)
   {
      id = create_batch(rname, p, 1, nullptr, adofgoal.data(), have_basegoal ? basegoal.data() : nullptr, &seed);
      if (have_starttraj) batch(id).set_traj(sampled.data());
   }
   else
      id = create_batch(rname, p, n_runs, starts_ptr, goals_ptr, basegoals_ptr, seeds_ptr, have_devs ? &devs : nullptr);
   if (!dat_filename.empty())
   {
      try { batch(id).open_dat(dat_filename); }
      catch (...) { destroy_batch(id); throw; }
   }
   std::ostringstream o;
   o << id;
   return o.str();
}

namespace {
int parse_run(const std::vector<std::string> & argv, int & i, int & run, const char * dup_msg)
{
   if (run != 0) throw std::runtime_error(dup_msg);
   int v = 0;
   if (std::sscanf(argv[++i].c_str(), "%d", &v) != 1 || v <= 0) throw std::runtime_error("Could not parse r!");
   run = v;
   return v;
}

double parse_conv_double(const std::string & s, const char * what)
{
   char * end = nullptr;
   const double v = std::strtod(s.c_str(), &end);
   if (end == s.c_str() || *end) throw std::runtime_error(std::string("Could not parse ") + what + "!");
   return v;
}

// puts a batch's convergence stop back as it was when the iterate call began (converge_* tokens hold for one call)
struct ConvergenceRestore
{
   Batch & b;
   ConvergenceSpec saved;
   explicit ConvergenceRestore(Batch & batch) : b(batch), saved(batch.convergence()) {}
   ~ConvergenceRestore() { try { b.set_convergence(saved); } catch (...) {} }
};
}

// src/orcdchomp_mod.cpp:2690-2852
std::string Module::cmd_iterate(const std::vector<std::string> & argv, bool batchmode)
{
   int run = 0, n_iter = 1;
   double max_time = HUGE_VAL;
   std::string fileform;
   bool have_fileform = false;
   double * costs_ptr = nullptr; int * status_ptr = nullptr;
   // the convergence stop for this call only (converge_*: the batch's own setting, overridden token by token)
   bool have_rtol = false, have_obs = false, have_patience = false;
   ConvergenceSpec call_conv;
   const int argc = (int) argv.size();
   int i;
   for (i=1; i<argc; i++)
   {
      if (argv[i] == "run" && i+1 < argc) parse_run(argv, i, run, "Only one r can be passed!");
      else if (argv[i] == "n_iter" && i+1 < argc) n_iter = std::atoi(argv[++i].c_str());
      else if (argv[i] == "converge_rtol" && i+1 < argc) { call_conv.rtol = parse_conv_double(argv[++i], "converge_rtol"); have_rtol = true; }
      else if (argv[i] == "converge_obs" && i+1 < argc) { call_conv.obs_max = parse_conv_double(argv[++i], "converge_obs"); have_obs = true; }
      else if (argv[i] == "converge_patience" && i+1 < argc)
      {
         char * end = nullptr;
         const long v = std::strtol(argv[++i].c_str(), &end, 10);
         if (end == argv[i].c_str() || *end) throw std::runtime_error("Could not parse converge_patience!");
         call_conv.patience = (int) std::max(-1L, std::min(v, 1L << 30));
         have_patience = true;
      }
      else if (argv[i] == "max_time" && i+1 < argc) max_time = std::atof(argv[++i].c_str());
      else if (argv[i] == "trajs_fileformstr" && i+1 < argc) { fileform = argv[++i]; have_fileform = true; }
      else if (batchmode && argv[i] == "costs" && i+1 < argc) costs_ptr = (double *) parse_pointer(argv[++i]);
      else if (batchmode && argv[i] == "status" && i+1 < argc) status_ptr = (int *) parse_pointer(argv[++i]);
      else break;
   }
   if (i < argc) bad_arguments();
   if (!run) throw std::runtime_error("you must pass a created run!");
   if (n_iter < 0) throw std::runtime_error("n_iter must be >=0!");
   Batch & b = batch(run);
   std::unique_ptr<ConvergenceRestore> conv_restore;
   if (have_rtol || have_obs || have_patience)
   {
      // tokens not given keep the batch's setting; the stop is on (patience 1) unless converge_patience says otherwise
      const ConvergenceSpec cur = b.convergence();
      ConvergenceSpec c = cur;
      if (have_rtol) c.rtol = call_conv.rtol;
      if (have_obs) c.obs_max = call_conv.obs_max;
      c.patience = have_patience ? call_conv.patience : (cur.patience > 0 ? cur.patience : 1);
      conv_restore.reset(new ConvergenceRestore(b));
      b.set_convergence(c);
   }
   const bool conv_on = b.convergence().patience > 0;
   std::vector<double> costs((size_t) b.n_runs * 3, 0.0);
   std::vector<int> status(b.n_runs, 0), iters(b.n_runs, 0);
   if (have_fileform && b.params.floating_base)
      throw std::runtime_error("Error: trajs_fileformstr and floating_base combined is not yet implemented!");
   // the pattern goes to printf with (iteration) for one run as in the reference (mod.cpp:2783-2784), with
   // (iteration, run) for a batch: those integer conversions and no other.  One run may also pass a constant name (no
   // conversion: every iteration overwrites the file, which is what the reference's sprintf makes of it)
   if (have_fileform)
   {
      const int nconv = count_int_conversions(fileform);
      if (b.n_runs > 1 ? nconv != 2 : (nconv != 0 && nconv != 1)) bad_arguments();
   }
   // seconds since the call began, without the time spent writing trajectory dumps (mod.cpp:2748-2750,
   // 2781-2795: the reference stops its clock around the dump)
   auto t_last = std::chrono::steady_clock::now();
   double ticks = 0.0;
   auto clock_now = [&]() {
      const auto now = std::chrono::steady_clock::now();
      ticks += std::chrono::duration<double>(now - t_last).count();
      t_last = now;
      return ticks;
   };
   if (!have_fileform && max_time == HUGE_VAL)
   {
      b.iterate_async(n_iter);
      b.sync(costs.data(), status.data(), iters.data());
      if (b.has_dat()) b.write_dat(0, n_iter, iters.data(), 0.0, clock_now());
   }
   else
   {
      // the trajectory dump before each iteration and the time limit need the host between
      // iterations: one iteration per launch, the cost-only pass once at the end (mod.cpp:2830).
      // r->iter restarts at 0 in every iterate call while hmc_resample_iter persists (mod.cpp:2752,
      // 2755): the launches pass their position in the call on to the hmc schedule.
      std::vector<double> traj((size_t) b.n_runs * b.n_points * b.n);
      std::vector<int> st1(b.n_runs, 0);
      bool aborted = false;
      for (int it=0; it<n_iter; it++)
      {
         if (have_fileform)
         {
            clock_now();
            for (int k=0; k<b.n_runs; k++)
            {
               if (k == 0) b.gettraj(traj.data());
               char fname[1024];
               // one run: the reference's file name; a batch: the pattern takes (iteration, run)
               std::snprintf(fname, sizeof(fname), fileform.c_str(), it, k);
               std::ofstream f(fname);
               f << serialize_traj(b.robot_name, b.adofindices, &traj[(size_t) k * b.n_points * b.n], b.n_points, b.n, 0,
                                   std::vector<double>(b.n_points, 0.0));
            }
            t_last = std::chrono::steady_clock::now();        // the dump is off the clock
         }
         const double t_begin = ticks;
         const std::vector<int> before = (it > 0) ? iters : std::vector<int>(b.n_runs, 0);
         b.iterate_async(1, it, false, it > 0);                // (runs that left their limits earlier in the call stay out)
         b.sync(costs.data(), st1.data(), iters.data());       // iterations made accumulate over the launches of the call
         const double t_end = clock_now();
         if (b.has_dat())
         {
            std::vector<int> made(b.n_runs);
            for (int k=0; k<b.n_runs; k++) made[k] = iters[k] - before[k];
            b.write_dat(it, 1, made.data(), t_begin, t_end);
         }
         // status 1: the run converged (it makes no more iterations in this call but takes the final cost-only pass)
         for (int k=0; k<b.n_runs; k++) if (st1[k] != 0) { status[k] = st1[k]; if (st1[k] == -1) aborted = true; }
         // a single run stops where the reference throws; a batch goes on for its other runs
         if (aborted && b.n_runs == 1) break;
         if (t_end > max_time) break;
         if (conv_on && std::all_of(status.begin(), status.end(), [](int v) { return v != 0; })) break;      // nothing left to iterate
      }
      if (!(aborted && b.n_runs == 1))
      {
         b.iterate_async(0, 0, true, n_iter > 0);              // cd_chomp_iterate(c, 0, ...) (mod.cpp:2830)
         b.sync(costs.data(), st1.data(), nullptr);
      }
   }
   if (costs_ptr) std::memcpy(costs_ptr, costs.data(), costs.size() * sizeof(double));
   if (status_ptr) std::memcpy(status_ptr, status.data(), status.size() * sizeof(int));
   if (!batchmode)
      for (int k=0; k<b.n_runs; k++)
         if (status[k] == -1) throw std::runtime_error("Resulting trajectory is outside of joint limits!");
   std::ostringstream o;
   o << costs[0];                                                   // sout << cost_total (mod.cpp:2849)
   return o.str();
}

// src/orcdchomp_mod.cpp:2854-3011
std::string Module::cmd_gettraj(const std::vector<std::string> & argv, bool batchmode)
{
   int run = 0;
   bool no_collision_check = false, no_collision_exception = false, no_collision_details = false, no_self_check = false;
   double * out_ptr = nullptr;
   int * verdict_ptr = nullptr;
   const int argc = (int) argv.size();
   int i;
   for (i=1; i<argc; i++)
   {
      if (argv[i] == "run" && i+1 < argc) parse_run(argv, i, run, "Only one r can be passed!");
      else if (argv[i] == "no_collision_check") no_collision_check = true;
      else if (argv[i] == "no_collision_exception") no_collision_exception = true;
      else if (argv[i] == "no_collision_details") no_collision_details = true;
      else if (argv[i] == "no_self_collision_check") no_self_check = true;      // additive: the field leg of the re-check alone
      else if (batchmode && argv[i] == "out" && i+1 < argc) out_ptr = (double *) parse_pointer(argv[++i]);
      else if (batchmode && argv[i] == "verdict" && i+1 < argc) verdict_ptr = (int *) parse_pointer(argv[++i]);
      else break;
   }
   if (i < argc) bad_arguments();
   if (!run) throw std::runtime_error("you must pass a created run!");
   Batch & b = batch(run);
   std::vector<double> traj((size_t) b.n_runs * b.n_points * b.n);
   b.gettraj(traj.data());
   if (batchmode)
   {
      if (!out_ptr) throw std::runtime_error("gettrajbatch needs out %p!");
      std::memcpy(out_ptr, traj.data(), traj.size() * sizeof(double));
      if (verdict_ptr) batch_collision_verdict(run, verdict_ptr, nullptr, nullptr, nullptr, nullptr, !no_self_check);
      return "";
   }
   const VerdictInputs in = verdict_inputs(env.robot(b.robot_name), b, false, false);      // col0 and vmax: the kernels' pair tables are not built
   // timing (mod.cpp:2905-2911)
   const std::vector<double> dtm = retime_linear(traj.data(), b.n_points, b.n, in.col0, in.vmax);
   if (!no_collision_check)
   {
      std::string details;
      const bool collides = host_recheck(env, b, traj.data(), dtm, !no_self_check, details);
      last_collision_details = no_collision_details ? std::string() : details;
      if (collides && !no_collision_exception) throw std::runtime_error("Resulting trajectory is in collision!");
   }
   // active dof columns only (mod.cpp:2899-2903)
   return serialize_traj(b.robot_name, b.adofindices, traj.data(), b.n_points, b.n, in.col0, dtm);
}

// src/orcdchomp_mod.cpp:3013-3037
std::string Module::cmd_destroy(const std::vector<std::string> & argv)
{
   int run = 0;
   const int argc = (int) argv.size();
   int i;
   for (i=1; i<argc; i++)
   {
      if (argv[i] == "run" && i+1 < argc) parse_run(argv, i, run, "Only one run can be passed!");
      else break;
   }
   if (i < argc) bad_arguments();
   if (!run) throw std::runtime_error("you must pass a created run!");
   destroy_batch(run);
   return "";
}

} // namespace orc
