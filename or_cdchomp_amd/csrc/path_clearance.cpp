// path_clearance.cpp -- host side of the clearance of given paths and of segments between waypoints (orc_batch_path_clearance,
// orc_batch_waypoint_segment_clearance): the checks of their arguments in one place, the queries dealt to the shards that own
// their runs (Batch::deal_by_run), the launches of path_kernels.hip.  The inputs are the clearance's (clearance.cpp):
// verdict_inputs with the self check as the robot has it, BatchShard::verdict_walk_args for the tables, and vmax for the
// retiming.  Nothing is kept: no trajectory, cost, status or key is written, and the minima of the last `clearance` (d_clear_)
// stay as they are.
//
// The samples of a call's queries lie in a workspace of a fixed number of entries (ORC_PATH_WORKSPACE of path_device.h; the
// environment's ORC_PATH_WORKSPACE=<entries> shrinks it).  The sample counts come back from the device once -- the cut needs
// them, whichever form the rows came in -- and the host cuts the call into rounds of consecutive queries whose samples fit.
#include "module.h"
#include "path_device.h"
#include "query_upload.h"
#include <cstdlib>
#include <stdexcept>

namespace orc {

void Batch::path_clearance_check(bool waypoints, int n_q, const int * run_of_q, const int * from_of_q, const int * to_of_q, int n_rows,
   const double * paths, int max_samples) const
{
   const char * who = waypoints ? "waypoint segment clearance" : "path clearance";
   if (n_q < 1 || n_q > ORC_PATH_MAX_Q) throw std::runtime_error(std::string(who) + ": n_q must lie in [1, 4194304]!");
   if (!waypoints && (n_rows < 2 || n_rows > ORC_PATH_MAX_ROWS)) throw std::runtime_error(std::string(who) + ": n_rows must lie in [2, 4096]!");
   if (!waypoints && !paths) throw std::runtime_error(std::string(who) + ": paths [n_q][n_rows][n] is NULL!");
   if (waypoints && (!from_of_q || !to_of_q)) throw std::runtime_error(std::string(who) + ": from_of_q or to_of_q is NULL!");
   if (max_samples < 1 || max_samples > (1 << 20)) throw std::runtime_error(std::string(who) + ": max_samples must lie in [1, 1048576]!");
   for (int q=0; run_of_q && q<n_q; q++)
      if (run_of_q[q] < 0 || run_of_q[q] >= n_runs) throw std::runtime_error(std::string(who) + ": a run_of_q entry lies outside [0, n_runs)!");
   for (int q=0; waypoints && q<n_q; q++)
      if (from_of_q[q] < 0 || from_of_q[q] >= n_points || to_of_q[q] < 0 || to_of_q[q] >= n_points)
         throw std::runtime_error(std::string(who) + ": a from_of_q or to_of_q entry lies outside [0, n_points)!");
}

void Module::batch_path_clearance(int id, bool waypoints, int n_q, const int * run_of_q, const int * from_of_q, const int * to_of_q, int n_rows,
   const double * paths, int max_samples, double * clearance, double * time, int * sphere, int * other, int * n_samples)
{
   Batch & b = batch(id);
   b.path_clearance_check(waypoints, n_q, run_of_q, from_of_q, to_of_q, n_rows, paths, max_samples);
   const VerdictInputs in = verdict_inputs(env.robot(b.robot_name), b, true);
   std::vector<unsigned long long> key((sphere || other) ? (size_t) n_q * 2 : 0);
   b.path_clearance(in, waypoints, n_q, run_of_q, from_of_q, to_of_q, waypoints ? 2 : n_rows, paths, max_samples, clearance, time,
      key.empty() ? nullptr : key.data(), n_samples);
   // key: sample << 32 | XML sphere << 16 | field, or the other sphere of a pair
   for (size_t q=0; q<key.size(); q++)
   {
      const bool has = key[q] != ORC_VERDICT_NONE;
      if (sphere) sphere[q] = has ? (int)((key[q] >> 16) & 0xffffull) : -1;
      if (other) other[q] = has ? (int)(key[q] & 0xffffull) : -1;
   }
}

void Batch::path_clearance(const VerdictInputs & in, bool waypoints, int n_q, const int * run_of_q, const int * from_of_q, const int * to_of_q,
   int n_rows, const double * paths, int max_samples, double * clear_out, double * time_out, unsigned long long * key_out, int * n_samples_out)
{
   path_clearance_check(waypoints, n_q, run_of_q, from_of_q, to_of_q, n_rows, paths, max_samples);
   deal_by_run(n_q, run_of_q, false,
      { deal_in(waypoints ? from_of_q : nullptr, 1), deal_in(waypoints ? to_of_q : nullptr, 1), deal_in(waypoints ? nullptr : paths, (size_t) n_rows * n) },
      { deal_out(clear_out, 2), deal_out(time_out, 2), deal_out(key_out, 2), deal_out(n_samples_out, 1) },
      [&](size_t k, int cnt, const int * run, const std::vector<void *> & in_col, const std::vector<void *> & out_col) {
         shards[k]->path_clearance(in, cnt, run, (const int *) in_col[0], (const int *) in_col[1], n_rows, (const double *) in_col[2], max_samples,
            (double *) out_col[0], (double *) out_col[1], (unsigned long long *) out_col[2], (int *) out_col[3]);
      });
}

// entries of the workspace: the environment may shrink it
static int path_workspace()
{
   const char * e = getenv("ORC_PATH_WORKSPACE");
   const long v = e ? atol(e) : 0;
   return (v >= 1 && v < ORC_PATH_WORKSPACE) ? (int) v : ORC_PATH_WORKSPACE;
}

template <typename real>
void BatchShard::path_clearance_typed(const VerdictInputs & in, int n_q, const int * run_of_q, const int * from_of_q, const int * to_of_q, int n_rows,
   const double * paths, int max_samples, double * clear_out, double * time_out, unsigned long long * key_out, int * n_samples_out)
{
   if ((int) in.vmax.size() != n - in.col0) throw std::runtime_error("path clearance: bad trajectory dimensions!");
   const auto lds_bytes = [this](int chunk) { return orc_path_walk_lds_bytes(n, ms_.Sa, ms_.Sa_real, ms_.nj, sizeof(real), chunk); };
   VerdictTables t;
   DevPathClearance<real> v;
   verdict_walk_args<real>(in, lds_bytes, t, v);
   const size_t lds = lds_bytes(v.chunk);
   if (lds > ORC_VERDICT_LDS_LIMIT) throw std::runtime_error("path clearance: the robot does not fit the kernel's shared memory!");
   QueryUpload<real> up(stream_, "path clearance");
   const int tree = plan_.variant & ORC_VAR_TREE;
   const size_t n2 = (size_t) n_q * 2;
   t.vmax.reset(upload<double>(in.vmax, up.st));
   v.key_out = nullptr; v.depth_out = nullptr;      // (the walk's outputs of the verdict: not written here)
   v.col0 = in.col0; v.vmax = t.vmax.as<const double>(); v.max_samples = max_samples;
   v.n_q = n_q; v.n_rows = n_rows;
   v.run_of_q = up.ints(run_of_q, n_q, "runs"); v.from_of_q = up.ints(from_of_q, n_q, "from"); v.to_of_q = up.ints(to_of_q, n_q, "to");
   v.paths = paths ? up.rows(paths, (size_t) n_q * n_rows * n) : nullptr;
   // one allocation for the arrays per query and, below, one for the workspace: `carve` hands out its parts, 256-byte aligned
   const auto padded = [](size_t bytes) { return (bytes + 255) & ~(size_t) 255; };
   const auto carve = [&padded](unsigned char * & at, size_t bytes) { unsigned char * part = at; at += padded(bytes); return (void *) part; };
   unsigned char * per_q = up.template alloc<unsigned char>(3*padded((size_t) n_q * sizeof(int)) + 3*padded(n2 * sizeof(double)));
   int * d_offs = (int *) carve(per_q, (size_t) n_q * sizeof(int));
   v.count = (int *) carve(per_q, (size_t) n_q * sizeof(int)); v.offs = d_offs; v.n_entries = 0;
   v.e_query = nullptr; v.e_seg = nullptr; v.e_u = nullptr; v.e_time = nullptr; v.e_gap = nullptr; v.e_key = nullptr;
   v.clear_out = (double *) carve(per_q, n2 * sizeof(double)); v.ckey_out = (unsigned long long *) carve(per_q, n2 * sizeof(unsigned long long));
   v.ctime_out = (double *) carve(per_q, n2 * sizeof(double)); v.n_samples_out = (int *) carve(per_q, (size_t) n_q * sizeof(int));

   // ---- the sample counts, and the rounds they cut the call into
   hip_check(orc_launch_path_count(v, up.st), "path_count_kernel launch");
   std::vector<int> count(n_q), offs(n_q);
   up.down(count.data(), v.count, (size_t) n_q * sizeof(int), "counts");
   up.sync("counts sync");
   const int budget = path_workspace();
   struct Round { int q0, q1, entries; };
   std::vector<Round> rounds;
   Round r{ 0, 0, 0 };
   int most = 0;
   for (int q=0; q<n_q; q++)
   {
      const int c = count[q] > 0 ? count[q] : 0;
      if (c > budget) throw std::runtime_error("path clearance: ORC_PATH_WORKSPACE holds fewer samples than one of the queries has!");
      if (r.entries + c > budget) { rounds.push_back(r); r = Round{ q, q, 0 }; }
      offs[q] = r.entries;
      r.entries += c; r.q1 = q + 1;
      most = r.entries > most ? r.entries : most;
   }
   rounds.push_back(r);
   up.up(d_offs, offs.data(), (size_t) n_q * sizeof(int), "offsets");
   if (most)
   {
      const size_t ints = (size_t) most * sizeof(int), reals = (size_t) most * sizeof(double);      // (48 bytes an entry)
      unsigned char * ws = up.template alloc<unsigned char>(2*padded(ints) + 2*padded(reals) + padded(2*reals) + padded(2*ints));
      v.e_query = (int *) carve(ws, ints); v.e_seg = (int *) carve(ws, ints);
      v.e_u = (double *) carve(ws, reals); v.e_time = (double *) carve(ws, reals);
      v.e_gap = (double *) carve(ws, 2*reals); v.e_key = (unsigned int *) carve(ws, 2*ints);
   }
   for (const Round & rd : rounds)
   {
      DevPathClearance<real> w = v;      // the round's slice of the per-query arrays
      const size_t q0 = (size_t) rd.q0;
      w.n_q = rd.q1 - rd.q0; w.n_entries = rd.entries;
      if (v.run_of_q) w.run_of_q = v.run_of_q + q0;
      if (v.from_of_q) { w.from_of_q = v.from_of_q + q0; w.to_of_q = v.to_of_q + q0; }
      if (v.paths) w.paths = v.paths + q0 * n_rows * n;
      w.count = v.count + q0; w.offs = v.offs + q0;
      w.clear_out = v.clear_out + q0*2; w.ckey_out = v.ckey_out + q0*2; w.ctime_out = v.ctime_out + q0*2; w.n_samples_out = v.n_samples_out + q0;
      hip_check(orc_launch_path_round(w, lds, up.st, tree), "path clearance round launch");
   }
   up.down(clear_out, v.clear_out, n2*sizeof(double), "minima");
   up.down(time_out, v.ctime_out, n2*sizeof(double), "times");
   up.down(key_out, v.ckey_out, n2*sizeof(unsigned long long), "keys");
   up.down(n_samples_out, v.n_samples_out, (size_t) n_q * sizeof(int), "samples");
   up.sync();
}

void BatchShard::path_clearance(const VerdictInputs & in, int n_q, const int * run_of_q, const int * from_of_q, const int * to_of_q, int n_rows,
   const double * paths, int max_samples, double * clear_out, double * time_out, unsigned long long * key_out, int * n_samples_out)
{
   DeviceGuard guard(device);
   if (params.precision == 64) path_clearance_typed<double>(in, n_q, run_of_q, from_of_q, to_of_q, n_rows, paths, max_samples, clear_out, time_out, key_out, n_samples_out);
   else path_clearance_typed<float>(in, n_q, run_of_q, from_of_q, to_of_q, n_rows, paths, max_samples, clear_out, time_out, key_out, n_samples_out);
}

} // namespace orc
