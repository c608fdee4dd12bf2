// batch.cpp -- a batch of independent CHOMP runs on one GPU (its collision verdicts: verdict.cpp).
// Host side of struct run / cd_chomp (src/orcdchomp_mod.cpp:887-966, 2104-2674;
// src/libcd/chomp.h:38-101): uploads what the stages of `create` fold and plan (stages.h), keeps
// the per-run state in HBM (run-major), launches the fused kernel (the hmc resamples of a call: hmc.cpp).
#include "module.h"
#include "kernel_table.h"
#include "launch.h"
#include "trajdoc.h"      // count_int_conversions
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <thread>
#include <exception>

namespace orc {

BatchShard::BatchShard(Module * mod, int dev, hipStream_t stream, const Robot & robot, const BatchParams & p, int nruns,
   const double * starts, const double * goals, const double * basegoals, const unsigned int * seeds,
   std::shared_ptr<const SceneTable> scenes, int run0)
   : n_runs(nruns), params(p), device(dev), mod_(mod), stream_(stream), scenes_(std::move(scenes)), run0_(run0)
{
   DeviceGuard guard(device);
   construct(robot, starts, goals, basegoals, seeds);      // (a failed construction holds device memory in handles only: they free it)
}

void BatchShard::construct(const Robot & robot, const double * starts, const double * goals, const double * basegoals,
   const unsigned int * seeds)
{
   sw_ = Switches::read();
   if (sw_.wave_rotate < 0 || sw_.wave_rotate > orc::WAVE_ROTATE_MAX) throw std::runtime_error("ORC_WAVE_ROTATE must be 0, 1 or 2!");
   const BatchParams & p = params;
   if (p.precision != 64 && p.precision != 32) throw std::runtime_error("precision must be 32 or 64!");
   const int n_adof = (int) robot.active_dofs.size();
   n_points = p.n_points;
   m = n_points - 2 + (p.free_start ? 1 : 0);                     // mod.cpp:2315-2316
   n = (p.floating_base ? 7 : 0) + n_adof;                        // mod.cpp:2104-2105
   robot_name = robot.name;
   adofindices = robot.active_dofs;
   if (n > ORC_MAX_JOINTS + 7) throw std::runtime_error("too many optimizer dofs for this build!");
   if (m < 1) throw std::runtime_error("n_points must be >=3!");
   if (m > ORC_MAX_POINTS) throw std::runtime_error("n_points is beyond what this build plans for (at most " + std::to_string(ORC_MAX_POINTS + 2) + ")!");
   if ((double) n_runs * n_points * n * 8.0 > 64e9) throw std::runtime_error("the batch's trajectories exceed 64 GB!");

   // joint limits (mod.cpp:2639-2660)
   jl_lo_.assign(n, -HUGE_VAL); jl_hi_.assign(n, HUGE_VAL);
   for (int j=0; j<n_adof; j++)
   {
      jl_lo_[(p.floating_base ? 7 : 0) + j] = robot.limit_lower[robot.active_dofs[j]];
      jl_hi_[(p.floating_base ? 7 : 0) + j] = robot.limit_upper[robot.active_dofs[j]];
   }

   build_metric(m, p.derivative, 1.0/(n_points-1), metric_, p.free_start != 0);       // dt: mod.cpp:2567

   if (p.precision == 64) { build_device<double>(robot); seed_runs<double>(robot, starts, goals, basegoals); }
   else { build_device<float>(robot); seed_runs<float>(robot, starts, goals, basegoals); }
   hmc_.reset(new HmcPlanner(mod_, device, stream_, n_runs, (size_t) m * n, p.precision, p.hmc_resample_lambda, p.use_hmc != 0, sw_, seeds));
}

// endpoints of every run, the straight-line seed on the device (mod.cpp:2417-2464) and the runs' state
template <typename real>
void BatchShard::seed_runs(const Robot & robot, const double * starts, const double * goals, const double * basegoals)
{
   const BatchParams & p = params;
   const int n_adof = (int) robot.active_dofs.size();
   std::vector<double> s((size_t) n_runs * n), g((size_t) n_runs * n);
   for (int k=0; k<n_runs; k++)
   {
      double * sk = &s[(size_t) k*n]; double * gk = &g[(size_t) k*n];
      int c0 = 0;
      if (p.floating_base)
      {
         for (int j=0; j<7; j++) { sk[j] = robot.transform.v[j]; gk[j] = basegoals[(size_t) k*7+j]; }
         c0 = 7;
      }
      for (int j=0; j<n_adof; j++)
      {
         sk[c0+j] = starts ? starts[(size_t) k*n_adof+j] : robot.dof_values[robot.active_dofs[j]];
         gk[c0+j] = goals[(size_t) k*n_adof+j];
      }
   }
   hipStream_t st = stream_;
   DevBuf d_s, d_g;
   d_s.reset(dev_alloc<double>(s.size())); d_g.reset(dev_alloc<double>(g.size()));
   hip_check(hipMemcpyAsync(d_s.as<void>(), s.data(), s.size()*sizeof(double), hipMemcpyHostToDevice, st), "starts");
   hip_check(hipMemcpyAsync(d_g.as<void>(), g.data(), g.size()*sizeof(double), hipMemcpyHostToDevice, st), "goals");
   const size_t tcount = (size_t) n_runs * n_points * n, mcount = (size_t) n_runs * m * n;
   d_traj_.reset(dev_alloc<real>(tcount)); d_AG_.reset(dev_alloc<real>(mcount)); d_G_.reset(dev_alloc<real>(mcount));
   hip_check(hipMemsetAsync(d_AG_.as<void>(), 0, mcount*sizeof(real), st), "memset");       // zero momentum, chomp.c:114-115
   hip_check(hipMemsetAsync(d_G_.as<void>(), 0, mcount*sizeof(real), st), "memset");
   hip_check(orc_launch_seed(d_traj_.as<real>(), d_s.as<double>(), d_g.as<double>(), n_runs, n_points, n, p.floating_base, st), "seed");
   d_costs_.reset(dev_alloc<double>((size_t) n_runs * 3));
   d_status_.reset(dev_alloc<int>(n_runs));
   d_iters_done_.reset(dev_alloc<int>(n_runs));
   d_leap_.reset(dev_alloc<int>(n_runs));
   d_conv_prev_.reset(dev_alloc<double>(n_runs));
   d_conv_streak_.reset(dev_alloc<int>(n_runs));
   hip_check(hipMemsetAsync(d_conv_prev_.as<void>(), 0, n_runs*sizeof(double), st), "memset");
   hip_check(hipMemsetAsync(d_conv_streak_.as<void>(), 0, n_runs*sizeof(int), st), "memset");
   hip_check(hipMemsetAsync(d_costs_.as<void>(), 0, (size_t) n_runs*3*sizeof(double), st), "memset");
   hip_check(hipMemsetAsync(d_status_.as<void>(), 0, n_runs*sizeof(int), st), "memset");
   hip_check(hipMemsetAsync(d_iters_done_.as<void>(), 0, n_runs*sizeof(int), st), "memset");
   std::vector<int> ones(n_runs, 1);                              // leapfrog_first = 1, chomp.c:80
   hip_check(hipMemcpyAsync(d_leap_.as<void>(), ones.data(), n_runs*sizeof(int), hipMemcpyHostToDevice, st), "leap");
   hip_check(hipStreamSynchronize(st), "sync");
   if (sw_.phase_timers)
   {
      d_phase_.reset(dev_alloc<long long>((size_t) n_runs * 8));
      d_hwid_.reset(dev_alloc<unsigned int>((size_t) n_runs * 16));
      hip_check(hipMemset(d_hwid_.as<void>(), 0xff, (size_t) n_runs * 16 * sizeof(unsigned int)), "memset");      // (all ones: a wavefront the workgroup does not have)
   }
}

BatchShard::~BatchShard()
{
   DeviceGuard guard(device);
   (void) hipStreamSynchronize(stream_);
   try { harvest_events(true); } catch (...) {}
   for (auto & ev : pending_events_) { mod_->release_event(device, ev.first); mod_->release_event(device, ev.second); }
   // (the device buffers, the hmc plan and the shard's share of the fields' copies go with their handles)
}

// kernel timing: a launch is bracketed by two events on the shard's stream
void BatchShard::harvest_events(bool wait)
{
   DeviceGuard guard(device);
   size_t kept = 0;
   for (auto & ev : pending_events_)
   {
      if (!wait && hipEventQuery(ev.second) != hipSuccess) { pending_events_[kept++] = ev; continue; }
      hip_check(hipEventSynchronize(ev.second), "hipEventSynchronize");
      float ms = 0.f;
      hip_check(hipEventElapsedTime(&ms, ev.first, ev.second), "hipEventElapsedTime");
      mod_->add_kernel_time(ms);
      mod_->release_event(device, ev.first);
      mod_->release_event(device, ev.second);
   }
   pending_events_.resize(kept);
}

// the device's copy of a field's grid in the run's precision (once per device: the shards share the copies)
template <typename real>
std::shared_ptr<void> BatchShard::grid_on_device(Sdf & s)
{
   std::lock_guard<std::recursive_mutex> env_lock(mod_->env_mutex);
   std::shared_ptr<void> & buf = (sizeof(real) == 8 ? s.dev64 : s.dev32)[device];
   if (!buf)
   {
      const size_t nc = s.grid.ncells();
      std::vector<real> converted;                  // (fp64: the grid as it is)
      const void * src = s.grid.data.data();
      if (sizeof(real) != sizeof(double)) { converted.assign(s.grid.data.begin(), s.grid.data.end()); src = converted.data(); }
      buf = device_buffer(device, nc*sizeof(real));
      hip_check(hipMemcpy(buf.get(), src, nc*sizeof(real), hipMemcpyHostToDevice), "sdf upload");
   }
   return buf;
}

// `create` on the device: the stages of stages.h in order, each followed by the upload of what it returned.
template <typename real>
void BatchShard::build_device(const Robot & robot)
{
   hipStream_t st = stream_;
   const JointTree tree = fold_joint_tree(robot, params.floating_base != 0);
   const int asked_block = mod_->workgroup_threads ? mod_->workgroup_threads : params.workgroup_threads;
   FoldedModel<real> fm = fold_robot<real>(robot, params, n, tree, asked_block, sw_, PlacementCache{ mod_->placement_cache, mod_->env_mutex });
   device_sphere_order = std::move(fm.device_sphere_order); slot_xml = std::move(fm.slot_xml);
   ms_ = fm.scalars;

   const FoldedTsrs<real> ft = fold_tsrs<real>(robot, params, tree, m, n);
   tsr_ = ft;
   if (tsr_.n_tsrs > 0)
   {
      const double gbytes = (double) tsr_.ws_stride * n_runs * sizeof(real) / 1e9;
      if (tsr_.cons_k > 2048 || gbytes > 64.0)
         throw std::runtime_error("TSR constraints: the constraint system is too large for this build (" + std::to_string(tsr_.cons_k)
                                  + " rows, " + std::to_string(gbytes) + " GB of workspace)!");
      d_tsrs_.reset(dev_alloc<DevTsr<real>>(tsr_.n_tsrs));
      hip_check(hipMemcpy(d_tsrs_.as<void>(), ft.tsrs.data(), ft.tsrs.size()*sizeof(DevTsr<real>), hipMemcpyHostToDevice), "tsrs");
      d_tsr_ws_.reset(dev_alloc<real>(tsr_.ws_stride * n_runs));
      d_tsr_err_.reset(dev_alloc<int>(n_runs));
      hip_check(hipMemset(d_tsr_err_.as<void>(), 0, sizeof(int) * n_runs), "tsr err");
   }
   d_model_.reset(dev_alloc<DevModel<real>>(1));
   hip_check(hipMemcpyAsync(d_model_.as<void>(), fm.model.get(), sizeof(DevModel<real>), hipMemcpyHostToDevice, st), "model");
   hip_check(hipStreamSynchronize(st), "model sync");

   FoldedScenes<real> fs = fold_scenes<real>(*scenes_, run0_, n_runs, ms_.GS != 16 && !(fm.variant & ORC_VAR_PAIRS));
   scn_ = fs;
   for (const auto & g : fs.grids)
   {
      const std::shared_ptr<void> buf = grid_on_device<real>(*g.sdf);
      fs.sdfs[(size_t) g.scene * fs.n_sdfs + g.field].data = fs.cells[(size_t) g.scene * fs.sdfc_stride + g.field].data = (const real *) buf.get();
      sdf_refs_.push_back(buf);
   }
   d_sdfc_.reset(dev_alloc<DevSdfCell<real>>(fs.cells.size()));
   hip_check(hipMemcpy(d_sdfc_.as<void>(), fs.cells.data(), fs.cells.size()*sizeof(DevSdfCell<real>), hipMemcpyHostToDevice), "sdfs (cell units)");
   d_sdfs_.reset(dev_alloc<DevSdf<real>>(fs.sdfs.size()));
   hip_check(hipMemcpy(d_sdfs_.as<void>(), fs.sdfs.data(), fs.sdfs.size()*sizeof(DevSdf<real>), hipMemcpyHostToDevice), "sdfs");
   d_scene_nsdf_.reset(dev_alloc<int>(fs.n_scenes));
   hip_check(hipMemcpy(d_scene_nsdf_.as<void>(), fs.scene_nsdf.data(), fs.n_scenes*sizeof(int), hipMemcpyHostToDevice), "scene field counts");
   d_scene_of_run_.reset(dev_alloc<int>(n_runs));
   hip_check(hipMemcpy(d_scene_of_run_.as<void>(), scenes_->scene_of_run.data() + run0_, n_runs*sizeof(int), hipMemcpyHostToDevice), "scene of run");

   MetricTables mt = pack_metric(metric_, params, m, sizeof(real), sw_);
   met_ = mt;
   d_Aband_.reset(upload<real>(metric_.Aband, st));
   d_beta_s_.reset(upload<real>(metric_.beta_s, st));
   d_beta_g_.reset(upload<real>(metric_.beta_g, st));
   if (!mt.metric64.empty()) d_metric64_.reset(upload<double>(mt.metric64, st));
   if (!mt.pcr.empty() && !mt.pcr_as_doubles) d_pcr_.reset(upload<real>(mt.pcr, st));
   if (!mt.pcr.empty() && mt.pcr_as_doubles)
   {
      // (as bytes: for an fp32 run every entry takes two reals of the table area)
      const size_t bytes = (size_t) mt.pcr_rows * m * sizeof(real);
      d_pcr_.reset(dev_alloc<real>((size_t) mt.pcr_rows * m));
      hip_check(hipMemsetAsync(d_pcr_.as<void>(), 0, bytes, st), "metric tables");
      hip_check(hipMemcpyAsync(d_pcr_.as<void>(), mt.pcr.data(), std::min(bytes, mt.pcr.size() * sizeof(double)), hipMemcpyHostToDevice, st), "metric tables");
      hip_check(hipStreamSynchronize(st), "metric tables sync");
   }
   if (!mt.Ainv.empty()) metric_.Ainv = std::move(mt.Ainv);
   if (!metric_.Ainv.empty()) d_Ainv_.reset(upload<real>(metric_.Ainv, st));
   d_jl_lo_.reset(upload<real>(jl_lo_, st));
   d_jl_hi_.reset(upload<real>(jl_hi_, st));

   PlanInput in;
   // one field with the world's axes in every scene: known at compile time (phase_cost KIND)
   in.variant = scene_variant(fm.variant, fs.one_aligned, ms_.S == ms_.Sa);
   in.m = m; in.n = n; in.nj = ms_.nj; in.Sa = ms_.Sa; in.S = ms_.S; in.GS = ms_.GS;
   in.n_sdfs = scn_.n_sdfs; in.n_tsrs = tsr_.n_tsrs; in.tsr_kmax = tsr_.kmax; in.pcr_rows = met_.pcr_rows; in.pair_entries = fm.pair_entries;
   in.use_momentum = params.use_momentum; in.free_start = params.free_start; in.derivative = params.derivative; in.solve_mode = met_.solve_mode;
   in.real_bytes = sizeof(real); in.sdf_bytes = sizeof(DevSdf<real>);
   in.overlapping = mod_->num_streams >= 2;
   in.module_threads = mod_->workgroup_threads; in.module_per_cu = mod_->workgroups_per_cu;
   in.params_threads = params.workgroup_threads; in.params_per_cu = params.workgroups_per_cu;
   plan_ = plan_iterate(in, sw_);
}

template <typename real>
void BatchShard::launch(int n_iter, bool final_eval, bool carry, const HmcPlan & hmc)
{
   const IteratePlan & P = plan_;
   DevBatch<real> b;
   std::memset(&b, 0, sizeof(b));
   b.model = d_model_.as<const DevModel<real>>();
   b.sdfs = d_sdfs_.as<const DevSdf<real>>();
   b.sdfc = d_sdfc_.as<const DevSdfCell<real>>();
   b.n_sdfs = scn_.n_sdfs;
   b.scene_of_run = d_scene_of_run_.as<int>(); b.scene_nsdf = d_scene_nsdf_.as<int>(); b.n_scenes = scn_.n_scenes; b.sdfc_stride = scn_.sdfc_stride;
   b.n_runs = n_runs; b.n_points = m + 2; b.np_global = n_points; b.free_start = params.free_start; b.m = m; b.n = n;
   if (params.free_start && P.tile_first < 2)
      throw std::runtime_error("start_tsr: the first tile must hold the two points after the start point!");
   b.tile_m = P.tile_m;
   b.n_tiles = P.n_tiles; b.tile_first = P.tile_first; b.tile_rest = P.tile_rest;
   if (!P.g_in_lds && !d_Gcost_) d_Gcost_.reset(dev_alloc<real>((size_t) n_runs * m * n));
   b.traj = d_traj_.as<real>(); b.AG = d_AG_.as<real>(); b.Gcost = d_Gcost_.as<real>();
   b.Gdbg = sw_.debug_state ? d_G_.as<real>() : nullptr;
   b.g_in_lds = P.g_in_lds; b.lds_flags = P.lds_flags; b.t_in_lds = P.t_in_lds; b.t_staged = (P.lds_flags & ORC_LDS_T_STAGED) ? 1 : 0;
   b.ms = ms_;
   b.lay = P.lay;
   b.costs = d_costs_.as<double>(); b.trace = d_trace_.as<double>(); b.status = d_status_.as<int>(); b.iters_done = d_iters_done_.as<int>();
   b.leapfrog_first = d_leap_.as<int>();
   const double dt = 1.0/(n_points-1);
   b.dt = (real) dt;
   b.inv_2dt = (real)(1.0/(2.0*dt));
   b.inv_dt2 = (real)(1.0/(dt*dt));
   b.inv_m = (real)(1.0/m);
   b.shared = run_params_record<real>(params.lambda, params.epsilon, params.obs_factor, params.obs_factor_self);
   b.epsilon_self = (real) params.epsilon_self; b.inv_epsilon_self = (real)1 / b.epsilon_self;
   b.run_params = run_params_on_ ? d_run_params_.as<const RunParams<real>>() : nullptr;
   b.use_momentum = params.use_momentum; b.use_hmc = params.use_hmc && hmc.max_resamples > 0;
   b.D = (params.derivative == 1 && params.free_start) ? -1 : params.derivative;
   b.Aband = d_Aband_.as<const real>(); b.beta_s = d_beta_s_.as<const real>(); b.beta_g = d_beta_g_.as<const real>();
   b.metric64 = d_metric64_.as<const double>();
   b.kss = metric_.kss; b.ksg = metric_.ksg; b.kgg = metric_.kgg;
   b.solve_mode = met_.solve_mode;
   b.pcr_levels = metric_.pcr_levels;
   b.pcr = d_pcr_.as<const real>(); b.Ainv = d_Ainv_.as<const real>();
   b.ss_rank = (met_.solve_mode == 3) ? metric_.ss_rank : 0;
   b.jl_lo = d_jl_lo_.as<const real>(); b.jl_hi = d_jl_hi_.as<const real>();
   b.hmc_iters = hmc.iters; b.noise = (const real *) hmc.noise; b.max_resamples = hmc.max_resamples;
   if (m >= (1 << ORC_IT_SHIFT) || hmc.max_resamples >= (1 << ORC_IT_SHIFT)) throw std::runtime_error("too many waypoints or resamples for the phase arguments!");
   b.n_iter = n_iter; b.final_eval = final_eval ? 1 : 0; b.carry_status = carry ? 1 : 0;
   b.conv_patience = conv.patience > 0 ? conv.patience : 0;
   b.conv_rtol = conv.rtol; b.conv_obs_max = conv.obs_max;
   b.conv_prev = d_conv_prev_.as<double>(); b.conv_streak = d_conv_streak_.as<int>();      // (a launch that starts a call does not read them)
   b.phase_cycles = d_phase_.as<long long>(); b.wave_hwid = d_hwid_.as<unsigned int>();
   b.pcr_in_lds = P.pcr_in_lds; b.pcr_sym = met_.pcr_sym; b.pcr_rows = met_.pcr_rows; b.ag_in_lds = P.ag_in_lds;
   b.stagger_mode = sw_.stagger_mode; b.stagger_sleeps = sw_.stagger_sleeps; b.lim_generic = sw_.lim_generic;
   b.wave_rotate = sw_.wave_rotate;
   b.band_toeplitz = met_.band_toeplitz;
   for (int k=0; k<=ORC_SS_MAX_RANK; k++) { b.band_c64[k] = met_.band_c64[k]; b.band_c[k] = (real) met_.band_c64[k]; }
   if (params.derivative == 1 && m >= 2)
   {
      b.a_diag = (real) metric_.Adense[(size_t) 1*m + 1];
      b.a_off = (real) metric_.Adense[(size_t) 1*m + 0];
   }
   else if (params.derivative == 1)
   {
      b.a_diag = (real) metric_.Adense[0];
      b.a_off = (real) metric_.beta_s[0];
   }
   b.tsrs = d_tsrs_.as<const DevTsr<real>>(); b.n_tsrs = tsr_.n_tsrs; b.cons_k = tsr_.cons_k; b.tsr_blocks = tsr_.blocks;
   b.tsr_structured = P.tsr_structured; b.tsr_wcap = P.tsr_wcap; b.tsr_nmax = P.tsr_nmax;
   b.tsr_ws = d_tsr_ws_.as<real>(); b.tsr_ws_stride = tsr_.ws_stride; b.tsr_err = d_tsr_err_.as<int>();
   hipEvent_t ev[2] = { mod_->acquire_event(device), mod_->acquire_event(device) };
   hip_check(hipEventRecord(ev[0], stream_), "hipEventRecord");
   hipError_t e = orc_launch_iterate(b, P.lds_bytes, stream_, P.variant, P.block);
   hip_check(e, "chomp_iterate_kernel launch");
   hip_check(hipEventRecord(ev[1], stream_), "hipEventRecord");
   pending_events_.push_back(std::make_pair(ev[0], ev[1]));
}

void BatchShard::iterate_async(int n_iter, int iter_begin, bool final_eval, bool carry)
{
   if (n_iter < 0) throw std::runtime_error("n_iter must be >=0!");
   hmc_->check_usable();
   DeviceGuard guard(device);
   last_n_iter = n_iter;
   const size_t tneed = (size_t) n_runs * (n_iter ? n_iter : 1) * 3;
   if (tneed > trace_cap_)
   {
      hip_check(hipStreamSynchronize(stream_), "sync");
      d_trace_.reset(); d_trace_.reset(dev_alloc<double>(tneed)); trace_cap_ = tneed;
   }
   // (the lock of the stream's plan buffers, where the plan takes it, is held through the launch that reads them)
   std::unique_lock<std::mutex> plan_lock;
   const HmcPlan hmc = hmc_->plan(iter_begin, n_iter, plan_lock);
   if (params.precision == 64) launch<double>(n_iter, final_eval, carry, hmc); else launch<float>(n_iter, final_eval, carry, hmc);
}

void BatchShard::sync_begin(double * costs_out, int * status_out, int * iters_out)
{
   DeviceGuard guard(device);
   hipStream_t st = stream_;
   if (costs_out) hip_check(hipMemcpyAsync(costs_out, d_costs_.as<void>(), (size_t) n_runs*3*sizeof(double), hipMemcpyDeviceToHost, st), "costs");
   if (status_out) hip_check(hipMemcpyAsync(status_out, d_status_.as<void>(), n_runs*sizeof(int), hipMemcpyDeviceToHost, st), "status");
   if (iters_out) hip_check(hipMemcpyAsync(iters_out, d_iters_done_.as<void>(), n_runs*sizeof(int), hipMemcpyDeviceToHost, st), "iters_done");
   hmc_->sync_begin();
}

void BatchShard::sync_end()
{
   DeviceGuard guard(device);
   hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
   harvest_events(false);
   hmc_->sync_end();
}

namespace {
void download(void * d, size_t count, int precision, double * out, hipStream_t st)
{
   if (precision == 64)
   {
      hip_check(hipMemcpyAsync(out, d, count*sizeof(double), hipMemcpyDeviceToHost, st), "download");
      hip_check(hipStreamSynchronize(st), "sync");
   }
   else
   {
      std::vector<float> tmp(count);
      hip_check(hipMemcpyAsync(tmp.data(), d, count*sizeof(float), hipMemcpyDeviceToHost, st), "download");
      hip_check(hipStreamSynchronize(st), "sync");
      for (size_t i=0; i<count; i++) out[i] = tmp[i];
   }
}
}

void BatchShard::gettraj(double * out)
{
   DeviceGuard guard(device);
   download(d_traj_.as<void>(), (size_t) n_runs * n_points * n, params.precision, out, stream_);
}

void BatchShard::get_plan(double out[9]) const
{
   out[0] = plan_.variant; out[1] = plan_.block; out[2] = (double) plan_.lds_bytes; out[3] = plan_.tile_m; out[4] = met_.solve_mode;
   out[5] = (double) plan_.workgroups_per_cu(); out[6] = plan_.n_tiles; out[7] = ms_.GS;
   out[8] = plan_.tile_first;
}

void BatchShard::get_tsr_plan(double out[11]) const
{
   // the decision phase_tsr makes from the same four numbers (tsr_form.h); without the structured solve every step is tsr_dense_step
   const TsrForm f = tsr_form(plan_.block, m, n, plan_.tsr_nmax);
   const bool st = plan_.tsr_structured != 0;
   out[0] = tsr_.n_tsrs; out[1] = tsr_.cons_k; out[2] = plan_.tsr_structured; out[3] = plan_.tsr_nmax;
   out[4] = st ? f.width : -1; out[5] = st ? f.regs : 0; out[6] = st ? f.aug : 0; out[7] = st ? f.meet : 0;
   out[8] = st ? f.subst_w : 0; out[9] = st ? f.subst_u : 0;
   out[10] = m;
}

void BatchShard::get_state(const std::string & which, double * out)
{
   DeviceGuard guard(device);
   const size_t mcount = (size_t) n_runs * m * n;
   if (which == "G") download(d_G_.as<void>(), mcount, params.precision, out, stream_);
   else if (which == "AG") download(d_AG_.as<void>(), mcount, params.precision, out, stream_);
   else if (which == "T")
   {
      std::vector<double> full((size_t) n_runs * n_points * n);
      gettraj(full.data());
      for (int k=0; k<n_runs; k++)
         std::memcpy(out + (size_t) k*m*n, &full[((size_t) k*n_points + (params.free_start ? 0 : 1))*n], (size_t) m*n*sizeof(double));
   }
   else throw std::runtime_error("unknown state name");
}

void BatchShard::get_trace(double * out)
{
   DeviceGuard guard(device);
   hip_check(hipMemcpyAsync(out, d_trace_.as<void>(), (size_t) n_runs * last_n_iter * 3 * sizeof(double), hipMemcpyDeviceToHost, stream_), "trace");
   hip_check(hipStreamSynchronize(stream_), "sync");
}

void BatchShard::get_phase_cycles(long long * out)
{
   DeviceGuard guard(device);
   if (!d_phase_) throw std::runtime_error("phase timers are off (set ORC_PHASE_TIMERS=1 before create)");
   hip_check(hipMemcpy(out, d_phase_.as<void>(), (size_t) n_runs*8*sizeof(long long), hipMemcpyDeviceToHost), "phase");
}

void BatchShard::get_wave_hwid(unsigned int * out)
{
   DeviceGuard guard(device);
   if (!d_hwid_) throw std::runtime_error("wave placement is recorded with the phase timers (set ORC_PHASE_TIMERS=1 before create)");
   hip_check(hipMemcpy(out, d_hwid_.as<void>(), (size_t) n_runs*16*sizeof(unsigned int), hipMemcpyDeviceToHost), "waves");
}

void BatchShard::set_traj(const double * traj)
{
   DeviceGuard guard(device);
   const size_t count = (size_t) n_runs * n_points * n;
   if (params.precision == 64)
      hip_check(hipMemcpyAsync(d_traj_.as<void>(), traj, count*sizeof(double), hipMemcpyHostToDevice, stream_), "set_traj");
   else
   {
      std::vector<float> tmp(traj, traj + count);
      hip_check(hipMemcpyAsync(d_traj_.as<void>(), tmp.data(), count*sizeof(float), hipMemcpyHostToDevice, stream_), "set_traj");
   }
   hip_check(hipStreamSynchronize(stream_), "set_traj sync");
}

// ---- per-run parameters ---------------------------------------------------------------------------------------------
namespace {
template <typename real>
void upload_run_params(const double * table, int n_runs, void * d, hipStream_t st)
{
   // the conversion `launch` makes of the shared values: (real) of the caller's double, once
   std::vector<RunParams<real>> rec(n_runs);
   for (int k=0; k<n_runs; k++) rec[k] = run_params_record<real>(table[4*k], table[4*k + 1], table[4*k + 2], table[4*k + 3]);
   hip_check(hipMemcpyAsync(d, rec.data(), rec.size()*sizeof(RunParams<real>), hipMemcpyHostToDevice, st), "run params");
   hip_check(hipStreamSynchronize(st), "run params sync");
}
}

void BatchShard::set_run_params(const double * table)
{
   // the kernarg block of a launch carries the table's address or NULL by value: launches already enqueued are not touched by
   // the switch, and the copy below follows them on the stream
   if (!table) { run_params_on_ = false; return; }
   DeviceGuard guard(device);
   const size_t rsize = (params.precision == 64) ? sizeof(RunParams<double>) : sizeof(RunParams<float>);
   if (!d_run_params_) d_run_params_.reset(dev_alloc<char>((size_t) n_runs * rsize));
   if (params.precision == 64) upload_run_params<double>(table, n_runs, d_run_params_.as<void>(), stream_);
   else upload_run_params<float>(table, n_runs, d_run_params_.as<void>(), stream_);
   run_params_on_ = true;
}

void BatchShard::get_run_params(double * out)
{
   if (run_params_on_)
   {
      DeviceGuard guard(device);
      // (a record is eight reals: the four parameters, 1/epsilon, padding)
      constexpr size_t W = sizeof(RunParams<double>) / sizeof(double);
      static_assert(W == sizeof(RunParams<float>) / sizeof(float), "RunParams");
      std::vector<double> rec((size_t) n_runs * W);
      download(d_run_params_.as<void>(), rec.size(), params.precision, rec.data(), stream_);
      for (int k=0; k<n_runs; k++) std::copy(rec.begin() + k*W, rec.begin() + k*W + 4, out + (size_t) 4*k);
      return;
   }
   const double shared[4] = { params.lambda, params.epsilon, params.obs_factor, params.obs_factor_self };
   for (int k=0; k<n_runs; k++)
      for (int c=0; c<4; c++) out[4*k + c] = (params.precision == 64) ? shared[c] : (double)(float) shared[c];
}

// ================================================================ Batch ===
// the runs of a batch in contiguous blocks over the module's devices: no collective,
// every shard copies its block straight into the caller's arrays (the host-side gather)
Batch::Batch(Module * mod, const std::vector<int> & devices, const Robot & robot, const BatchParams & p, int nruns,
   const double * starts, const double * goals, const double * basegoals, const unsigned int * seeds,
   std::shared_ptr<const SceneTable> scene_table)
   : n_runs(nruns), params(p), scenes(std::move(scene_table))
{
   const int n_adof = (int) robot.active_dofs.size();
   int world = (int) devices.size();
   if (world < 1) throw std::runtime_error("a batch needs at least one device!");
   if (world > n_runs) world = n_runs;
   offs.assign(world + 1, 0);
   for (int r=0; r<world; r++)
   {
      // the first n_runs % world shards get one extra run (or_cdchomp_amd/sharding.py: shard_bounds)
      const int base = n_runs / world, extra = n_runs % world;
      offs[r+1] = offs[r] + base + (r < extra ? 1 : 0);
   }
   std::vector<hipStream_t> streams(world);
   for (int r=0; r<world; r++)
   {
      bool repeated = false;                      // a device listed twice: its shards get streams of their own
      for (int q=0; q<world; q++) if (q != r && devices[q] == devices[r]) repeated = true;
      streams[r] = mod->pick_stream(devices[r], repeated);
   }
   // one host thread per shard builds it on its device (model fold, uploads, seed kernel); what the shards share in the
   // module (the placement cache, the fields' device copies, the event pool) is behind its mutexes
   shards.resize(world);
   for_shards([&](size_t r) {
      const size_t lo = (size_t) offs[r];
      shards[r].reset(new BatchShard(mod, devices[r], streams[r], robot, p, offs[r+1] - offs[r],
         starts ? starts + lo * n_adof : nullptr, goals + lo * n_adof, basegoals ? basegoals + lo * 7 : nullptr,
         seeds ? seeds + lo : nullptr, scenes, (int) lo));
   }, true);
   const BatchShard & s0 = *shards[0];
   n_points = s0.n_points; n = s0.n; m = s0.m;
   robot_name = s0.robot_name; adofindices = s0.adofindices;
   device_sphere_order = s0.device_sphere_order; slot_xml = s0.slot_xml;
}

Batch::~Batch()
{
   for (FILE * f : dat_) if (f) std::fclose(f);
}

// body(k) for every shard; on host threads when the bodies block (each asserts its own device)
void Batch::for_shards(const std::function<void(size_t)> & body, bool threads)
{
   if (!threads || shards.size() < 2) { for (size_t k=0; k<shards.size(); k++) body(k); return; }
   std::vector<std::thread> pool;
   std::vector<std::exception_ptr> errs(shards.size());
   for (size_t k=0; k<shards.size(); k++)
      pool.emplace_back([&body, &errs, k]() { try { body(k); } catch (...) { errs[k] = std::current_exception(); } });
   for (std::thread & th : pool) th.join();
   for (std::exception_ptr & e : errs) if (e) std::rethrow_exception(e);
}

void Batch::deal_by_run(int n_q, const int * run_of_q, bool profile, const std::vector<DealColumn> & ins, const std::vector<DealColumn> & outs,
   const DealCall & call)
{
   // the caller's own arrays from query `first` on (a NULL stays NULL)
   const auto from = [](const std::vector<DealColumn> & cols, size_t first) {
      std::vector<void *> p;
      for (const DealColumn & c : cols) p.push_back(c.data ? (unsigned char *) c.data + first*c.bytes() : nullptr);
      return p;
   };
   if (shards.size() == 1)      // one shard owns every run: the gather would be the identity, and copy n_q rows to say so
   {
      call(0, n_q, run_of_q, from(ins, 0), from(outs, 0));
      return;
   }
   for_shards([&](size_t k) {
      if (profile)      // every waypoint in storage order: a shard's queries are its slice
      {
         const size_t w0 = (size_t) offs[k] * n_points;
         call(k, (offs[k+1] - offs[k]) * n_points, nullptr, from(ins, w0), from(outs, w0));
         return;
      }
      const Deal d = deal_gather(n_q, run_of_q, offs[k], offs[k+1], ins, outs);
      if (d.at.empty()) return;
      call(k, (int) d.at.size(), d.run.data(), d.in_ptr, d.out_ptr);
      deal_scatter(d, outs);
   }, true);
}

void Batch::iterate_async(int n_iter, int iter_begin, bool final_eval, bool carry)
{
   if (n_iter < 0) throw std::runtime_error("n_iter must be >=0!");
   last_n_iter = n_iter;
   iterated = true;
   // one host thread per shard: each asserts its device and launches there (the hmc plan of a shard may wait for its device)
   for_shards([&](size_t k) { shards[k]->iterate_async(n_iter, iter_begin, final_eval, carry); }, true);
}

void ConvergenceSpec::validate() const
{
   if (patience <= 0) return;
   if (!(rtol > 0.0)) throw std::runtime_error("convergence: rtol must be a number > 0!");
   if (std::isnan(obs_max)) throw std::runtime_error("convergence: obs_max must not be NaN!");
}

void Batch::set_convergence(const ConvergenceSpec & c)
{
   c.validate();
   ConvergenceSpec v = c;
   if (v.patience <= 0) v = ConvergenceSpec();
   for (auto & s : shards) s->conv = v;
}

void Batch::set_verdict_scope(int scope)
{
   if (scope != 0 && scope != 1) throw std::runtime_error("set_verdict_scope: scope is 0 (all runs) or 1 (the candidates)!");
   verdict_scope = scope;
}

// With scope 1 the selection's verdict asks about the candidates only -- a run that is none was never eligible -- and, as
// nobody reads n_samples there, does not count the samples behind a contact; a candidate that is too long fails the call as
// before.
VerdictScope Batch::selection_scope() const
{
   VerdictScope s;
   if (verdict_scope == 1) { s.which = 1; s.count_rest = false; }
   return s;
}

void Batch::sync(double * costs_out, int * status_out, int * iters_out)
{
   // the host-side gather: every shard copies its block straight into the caller's arrays
   for_shards([&](size_t k) {
      shards[k]->sync_begin(costs_out ? costs_out + (size_t) offs[k]*3 : nullptr, status_out ? status_out + offs[k] : nullptr,
                            iters_out ? iters_out + offs[k] : nullptr);
      shards[k]->sync_end();
   }, true);
}

void Batch::gettraj(double * out)
{
   for_shards([&](size_t k) { shards[k]->gettraj(out + (size_t) offs[k] * n_points * n); }, true);
}

void Batch::get_plan(double out[9]) { shards[0]->get_plan(out); }
void Batch::get_tsr_plan(double out[11]) { shards[0]->get_tsr_plan(out); }

void Batch::get_state(const std::string & which, double * out)
{
   for_shards([&](size_t k) { shards[k]->get_state(which, out + (size_t) offs[k] * m * n); }, true);
}

void Batch::get_trace(double * out)
{
   for_shards([&](size_t k) { shards[k]->get_trace(out + (size_t) offs[k] * last_n_iter * 3); }, true);
}

void Batch::set_noise(const double * noise, int n_blocks)
{
   for (size_t k=0; k<shards.size(); k++) shards[k]->set_noise(noise + (size_t) offs[k] * n_blocks * m * n, n_blocks);
}

void Batch::set_traj(const double * traj)
{
   for_shards([&](size_t k) { shards[k]->set_traj(traj + (size_t) offs[k] * n_points * n); }, true);
}

void Batch::set_run_params(const double * lambda, const double * epsilon, const double * obs_factor, const double * obs_factor_self)
{
   const double * arr[4] = { lambda, epsilon, obs_factor, obs_factor_self };
   static const char * const name[4] = { "lambda", "epsilon", "obs_factor", "obs_factor_self" };
   if (!lambda && !epsilon && !obs_factor && !obs_factor_self)
   {
      for (auto & s : shards) s->set_run_params(nullptr);
      return;
   }
   const double shared[4] = { params.lambda, params.epsilon, params.obs_factor, params.obs_factor_self };
   std::vector<double> table((size_t) n_runs * 4);
   for (int c=0; c<4; c++)
      for (int r=0; r<n_runs; r++)
      {
         const double v = arr[c] ? arr[c][r] : shared[c];
         if (!std::isfinite(v)) throw std::runtime_error(std::string("set_run_params: ") + name[c] + " of run " + std::to_string(r) + " is not a finite number!");
         // (the kernels form 1/lambda and 1/epsilon)
         if (c < 2 && !(v > 0.0)) throw std::runtime_error(std::string("set_run_params: ") + name[c] + " of run " + std::to_string(r) + " must be > 0!");
         table[(size_t) 4*r + c] = v;
      }
   // every shard takes its slice, as it took its slice of scene_of_run
   for_shards([&](size_t k) { shards[k]->set_run_params(table.data() + (size_t) offs[k] * 4); }, true);
}

void Batch::get_run_params(double * out)
{
   for_shards([&](size_t k) { shards[k]->get_run_params(out + (size_t) offs[k] * 4); }, true);
}

void Batch::get_phase_cycles(long long * out)
{
   for (size_t k=0; k<shards.size(); k++) shards[k]->get_phase_cycles(out + (size_t) offs[k] * 8);
}

void Batch::get_wave_hwid(unsigned int * out)
{
   for (size_t k=0; k<shards.size(); k++) shards[k]->get_wave_hwid(out + (size_t) offs[k] * 16);
}

// create's dat_filename (src/orcdchomp_mod.cpp:2306-2310): one file per run; a batch of several
// runs takes a printf pattern with one %d (the run index)
void Batch::open_dat(const std::string & pattern)
{
   // one run: the name as it is (src/orcdchomp_mod.cpp:2306-2310); a batch: a pattern with exactly one integer
   // conversion, the run index
   if (n_runs > 1 && count_int_conversions(pattern) != 1) throw std::runtime_error("Bad arguments!");
   for (int k=0; k<n_runs; k++)
   {
      char name[1024];
      if (n_runs > 1) std::snprintf(name, sizeof(name), pattern.c_str(), k);
      else std::snprintf(name, sizeof(name), "%s", pattern.c_str());
      FILE * f = std::fopen(name, "w");
      if (!f) throw std::runtime_error("could not open dat_filename for writing!");
      dat_.push_back(f);
   }
}

// "%d %f %f %f %f\n" = iteration, seconds, cost_total, cost_obs, cost_smooth (mod.cpp:2811-2818) for
// the iterations [iter_begin, iter_begin + iters_done) a launch completed, from the launch's trace.
// The reference's second column is the thread CPU time since the iterate call began; the fused kernel
// has no per-iteration host clock, so the launch's wall interval [t_begin, t_end] (seconds since the
// call began) is divided evenly over its iterations.
void Batch::write_dat(int iter_begin, int n_iter, const int * iters_done, double t_begin, double t_end)
{
   if (dat_.empty() || n_iter <= 0) return;
   std::vector<double> tr((size_t) n_runs * n_iter * 3);
   get_trace(tr.data());
   for (int k=0; k<n_runs; k++)
   {
      const int done = iters_done ? iters_done[k] : n_iter;
      for (int it=0; it<done; it++)
      {
         const double * row = &tr[((size_t) k * n_iter + it) * 3];
         std::fprintf(dat_[k], "%d %f %f %f %f\n", iter_begin + it, t_begin + (t_end - t_begin) * (it + 1) / n_iter, row[0], row[1], row[2]);
      }
      std::fflush(dat_[k]);
   }
}

} // namespace orc
