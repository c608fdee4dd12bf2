"""-m gpu: the other BASELINE.json configurations at oracle-sized scale:
floating base + momentum + hmc (config 4), multi-SDF 30-dof tree in fp64 and fp32
(config 5), higher-order smoothness (derivative 2, dense A^-1 fallback)."""
import numpy as np
import pytest

import common
from or_cdchomp_amd import robots, scenes

pytestmark = pytest.mark.gpu


def _mk_module():
    import or_cdchomp_amd
    return or_cdchomp_amd.Module(0)


@pytest.mark.parametrize("device_streams", [False, True])
def test_floating_base_momentum_hmc(oracle, monkeypatch, device_streams):
    """config 4 shape: base pose columns 0..6, all spheres active, hmc resampling from the
    module's own mt19937 stream (seed = run index), quaternion renormalisation per iteration.
    The streams of a batch live on the host (small batches) or on the device (hmc_kernels.hip,
    batches of 256 runs and more; forced here): both reproduce the oracle's GSL streams"""
    if device_streams:
        monkeypatch.setenv("ORC_HMC_DEVICE", "1")
    else:
        monkeypatch.setenv("ORC_HMC_HOST", "1")
    mod = _mk_module()
    model = common.setup_product_wam(mod)
    prob = common.tabletop_problem(oracle)
    _, base, dofvals, adofs = common.wam_state()
    n_runs, n_points, n_iter = 4, 60, 40
    rng = np.random.default_rng(20250103)
    goals = common.wam_goals(n_runs, seed=20250103)
    basegoals = np.tile(np.asarray(base), (n_runs, 1))
    basegoals[:, :3] += rng.uniform(-0.3, 0.3, size=(n_runs, 3))
    seeds = np.arange(n_runs, dtype=np.uint32)
    kw = dict(n_points=n_points, lambda_=100.0, obs_factor=500.0, floating_base=1, use_momentum=1,
              use_hmc=1, hmc_resample_lambda=0.02)
    bid = mod.batch_create(model.name, goals, basegoals=basegoals, seeds=seeds, **kw)
    seed_traj = mod.batch_gettraj(bid)
    costs, status = mod.batch_iterate(bid, n_iter)
    traj = mod.batch_gettraj(bid)
    trace = mod.batch_trace(bid, n_iter)
    rob = oracle.OraRobot(model)
    errs = []
    for k in range(n_runs):
        p = oracle.default_params(seed=int(seeds[k]), **kw)
        run = oracle.OraRun(rob, base, dofvals, adofs, goals[k], [prob["sdf"]], [prob["pose"]], p, basegoal=basegoals[k])
        assert run.n == 14 and run.Sa == 16
        assert np.array_equal(seed_traj[k], run.traj())
        st, ocosts, otr = run.iterate(n_iter, trace=True)
        assert st == 0 and status[k] == 0
        errs.append(common.rel_l2(traj[k], run.traj()))
        assert np.allclose(costs[k], ocosts, rtol=1e-6, atol=0), (costs[k], ocosts)
        assert np.allclose(trace[k], otr, rtol=1e-6, atol=0)
        run.destroy()
    assert max(errs) <= 1e-6, errs
    # a second iterate call: r->iter restarts at 0 while hmc_resample_iter persists
    costs2, _ = mod.batch_iterate(bid, 10)
    mod.batch_destroy(bid)
    print("floating/hmc worst rel L2 %.3e" % max(errs))


def _hmc_batch(mod, model, n_runs, seed0, n_points=40):
    _, base, _, _ = common.wam_state()
    goals = common.wam_goals(n_runs, seed=20250103 + seed0)
    basegoals = np.tile(np.asarray(base), (n_runs, 1))
    seeds = np.arange(n_runs, dtype=np.uint32) + seed0
    kw = dict(n_points=n_points, lambda_=100.0, obs_factor=500.0, floating_base=1, use_momentum=1, use_hmc=1, hmc_resample_lambda=0.05)
    return mod.batch_create(model.name, goals, basegoals=basegoals, seeds=seeds, **kw)


def test_hmc_plan_out_of_room_leaves_the_batch_unusable(monkeypatch):
    """a run that draws more momentum resamples in one call than the plan has room for: the call reports it, and the
    batch -- whose kernel ran with a cut schedule -- refuses further calls instead of going on from an inconsistent state
    (ORC_HMC_ROOM: room for one resample per run and call, where 60 iterations at lambda 0.05 draw three on average)"""
    import os
    if os.environ.get("ORC_HMC_PLAN_SYNC"):
        pytest.skip("the synchronous plan (round 2's way, scripts/test_toggles.sh) retries with more room instead")
    monkeypatch.setenv("ORC_HMC_DEVICE", "1")
    mod = _mk_module()
    model = common.setup_product_wam(mod)
    good = _hmc_batch(mod, model, 8, 0)
    bad = _hmc_batch(mod, model, 8, 100)
    monkeypatch.setenv("ORC_HMC_ROOM", "1")
    with pytest.raises(RuntimeError, match="not usable any more"):
        mod.batch_iterate(bad, 60)
    monkeypatch.delenv("ORC_HMC_ROOM")
    with pytest.raises(RuntimeError, match="create it again"):
        mod.batch_iterate(bad, 5)
    mod.batch_destroy(bad)
    costs, status = mod.batch_iterate(good, 60)          # the flag was the other batch's: this one runs
    assert np.all(np.isfinite(costs))
    mod.batch_destroy(good)


def test_hmc_batches_of_one_stream_share_the_plan_buffers(monkeypatch):
    """the noise of an iterate call is written and read inside the call, so the batches of a stream share one buffer
    (Module::plan_buffers): calls of two batches queued back to back without a sync give what each gives alone"""
    monkeypatch.setenv("ORC_HMC_DEVICE", "1")
    alone = []
    for seed0, n_runs in ((0, 8), (100, 12)):
        mod = _mk_module()
        model = common.setup_product_wam(mod)
        bid = _hmc_batch(mod, model, n_runs, seed0)
        mod.batch_iterate(bid, 30)
        alone.append(mod.batch_gettraj(bid))
    mod = _mk_module()
    mod.set_num_streams(1)
    model = common.setup_product_wam(mod)
    a = _hmc_batch(mod, model, 8, 0)
    b = _hmc_batch(mod, model, 12, 100)
    mod.batch_iterate_async(a, 30)
    mod.batch_iterate_async(b, 30)
    mod.batch_sync(a); mod.batch_sync(b)
    assert np.array_equal(mod.batch_gettraj(a), alone[0])
    assert np.array_equal(mod.batch_gettraj(b), alone[1])


def _replay_host_noise(oracle, seeds, n_iter, mn, lam):
    """the blocks the host planner draws for one iterate call of n_iter iterations, per run in resample order: at a
    resample iteration `it` m n Gaussians of sigma 1/sqrt(100 exp(0.02 it)), then one uniform u, and the next resample
    at it + 1 + int(-log(u)/lambda); the first is at iteration 0 (src/orcdchomp_mod.cpp:2755-2768)"""
    import ctypes as C
    L = oracle.lib()
    blocks = []
    for seed in seeds:
        r = oracle.Rng()
        L.ora_rng_set(C.byref(r), int(seed))
        mine, nxt = [], 0
        for it in range(n_iter):
            if it != nxt:
                continue
            sigma = 1.0 / np.sqrt(100.0 * np.exp(0.02 * it))
            mine.append(np.array([L.ora_ran_gaussian(C.byref(r), sigma) for _ in range(mn)]))
            nxt += 1 + int(-np.log(L.ora_rng_uniform(C.byref(r))) / lam)
        blocks.append(mine)
    return blocks


@pytest.mark.parametrize("precision", [64, 32])
def test_caller_supplied_noise_replays_the_host_streams(oracle, monkeypatch, precision):
    """orc_batch_set_noise: a batch given the blocks its own streams would draw (replayed with the oracle's generator)
    computes what the batch on its streams computes, bit for bit; so does one given the first block only (the later
    resamples fall back to the stream, which was advanced all the same); the negated blocks give something else (they
    are read).  Seeds 0..3 draw 4, 4, 4 and 3 resamples in the 12 iterations.  fp32 is compared with the fp32 batch on its
    own streams: the host planner's (float) conversion of either source"""
    monkeypatch.setenv("ORC_HMC_HOST", "1")
    mod = _mk_module()
    model = common.setup_product_wam(mod)
    _, base, _, _ = common.wam_state()
    n_runs, n_points, n_iter, lam = 4, 12, 12, 0.3
    goals = common.wam_goals(n_runs, seed=20250103)
    basegoals = np.tile(np.asarray(base), (n_runs, 1))
    seeds = np.arange(n_runs, dtype=np.uint32)
    kw = dict(n_points=n_points, lambda_=100.0, obs_factor=500.0, floating_base=1, use_momentum=1, use_hmc=1,
              hmc_resample_lambda=lam, precision=precision)

    def run(noise=None):
        bid = mod.batch_create(model.name, goals, basegoals=basegoals, seeds=seeds, **kw)
        if noise is not None:
            mod.batch_set_noise(bid, noise)
        costs, status = mod.batch_iterate(bid, n_iter)
        out = (mod.batch_gettraj(bid), costs, status)
        mod.batch_destroy(bid)
        return out

    mn = (n_points - 2) * 14
    blocks = _replay_host_noise(oracle, seeds, n_iter, mn, lam)
    counts = [len(b) for b in blocks]
    print("resamples per run:", counts)
    assert min(counts) >= 2, counts
    noise = np.zeros((n_runs, max(counts), mn))
    for k, mine in enumerate(blocks):
        noise[k, :len(mine)] = mine
    a = run()
    assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1]))
    for name, given in (("all blocks", noise), ("the first block", noise[:, :1])):
        got = run(given)
        assert np.array_equal(got[0], a[0]) and np.array_equal(got[1], a[1]) and np.array_equal(got[2], a[2]), name
    d = run(-noise)
    assert not np.array_equal(d[0], a[0])
    monkeypatch.delenv("ORC_HMC_HOST")
    monkeypatch.setenv("ORC_HMC_DEVICE", "1")
    bid = mod.batch_create(model.name, goals, basegoals=basegoals, seeds=seeds, **kw)
    with pytest.raises(RuntimeError, match="caller-supplied noise needs the host noise streams"):
        mod.batch_set_noise(bid, noise)
    mod.batch_destroy(bid)


def test_synchronous_hmc_plan_retries_with_more_room(oracle, monkeypatch):
    """ORC_HMC_PLAN_SYNC draws the plan on the shard's stream and waits; a run that needs more room than the call began
    with makes it back the generators up, double the room and draw again.  With ORC_HMC_ROOM=1 as the first room the
    retry runs twice in the first call (of seeds 0..7, run 0 draws three resamples in 20 iterations at lambda 0.05 and
    run 6 two: asserted below by replaying the streams), and two calls give bit for bit what the plan stream's way
    gives.  What the test cannot see is whether the first room really was 1: were ORC_HMC_ROOM ignored under
    ORC_HMC_PLAN_SYNC again (as it was before hmc.cpp), the results would be the same and the retry not reached"""
    counts = [len(b) for b in _replay_host_noise(oracle, np.arange(8), 20, 14 * 14, 0.05)]
    assert counts[0] == 3 and counts[6] == 2, counts          # more than a room of one, and of two: the loop doubles twice
    monkeypatch.setenv("ORC_HMC_DEVICE", "1")
    legs = []
    for sync in (False, True):
        mod = _mk_module()
        model = common.setup_product_wam(mod)
        bid = _hmc_batch(mod, model, 8, 0, n_points=16)
        if sync:
            monkeypatch.setenv("ORC_HMC_PLAN_SYNC", "1")
            monkeypatch.setenv("ORC_HMC_ROOM", "1")
        out = []
        for n_iter in (20, 6):
            costs, status = mod.batch_iterate(bid, n_iter)
            out.append((mod.batch_gettraj(bid), costs, status))
        mod.batch_destroy(bid)
        legs.append(out)
    for plain, retried in zip(*legs):
        assert np.all(np.isfinite(plain[1]))
        for x, y in zip(plain, retried):
            assert np.array_equal(x, y)


def _tree_scene(mod, oracle, cube_extent):
    """four box kinbodies with their own fields (config 5), returned for the oracle as well"""
    rng = np.random.default_rng(20250104)
    grids, poses = [], []
    for name, (boxes, pose) in scenes.random_boxes(rng).items():
        mod.add_kinbody_boxes(name, boxes, transform=pose)
        mod.SendCommand("computedistancefield kinbody %s cube_extent %f aabb_padding 0.15" % (name, cube_extent))
        data, lengths, gpose = mod.get_sdf(name)
        grids.append(oracle.OraGrid(data, lengths))
        # pose_world_gsdf = kinbody pose o grid pose (reference src/orcdchomp_mod.cpp:2359-2367)
        out = np.zeros(7)
        oracle.lib().ora_kin_pose_compose(oracle.dp(oracle.f64(pose)), oracle.dp(oracle.f64(gpose)), oracle.dp(out))
        poses.append(out)
    return grids, poses


@pytest.mark.parametrize("precision,tol", [(64, 1e-6), (32, 1e-3)])
def test_tree30_multi_sdf(oracle, precision, tol):
    mod = _mk_module()
    model = robots.tree30()
    base = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    dofvals = np.zeros(model.n_dof)
    adofs = list(range(model.n_dof))
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    grids, poses = _tree_scene(mod, oracle, 0.02)
    n_runs, n_points, n_iter = 3, 40, 20
    rng = np.random.default_rng(5)
    goals = rng.uniform(-0.8, 0.8, size=(n_runs, model.n_dof))
    kw = dict(n_points=n_points, lambda_=200.0, obs_factor=100.0)
    bid = mod.batch_create(model.name, goals, precision=precision, **kw)
    costs, status = mod.batch_iterate(bid, n_iter)
    traj = mod.batch_gettraj(bid)
    mod.batch_destroy(bid)
    rob = oracle.OraRobot(model)
    errs = []
    for k in range(n_runs):
        run = oracle.OraRun(rob, base, dofvals, adofs, goals[k], grids, poses, oracle.default_params(**kw))
        assert run.n == 30 and run.Sa == 60
        st, ocosts = run.iterate(n_iter)
        assert st == 0 and status[k] == 0
        errs.append(common.rel_l2(traj[k], run.traj()))
        assert np.allclose(costs[k], ocosts, rtol=max(tol, 1e-6) * (100 if precision == 32 else 1), atol=0), (costs[k], ocosts)
        run.destroy()
    assert max(errs) <= tol, errs
    print("tree30 fp%d worst rel L2 %.3e" % (precision, max(errs)))


@pytest.mark.parametrize("precision,tol", [(64, 1e-6), (32, 1e-3)])
def test_tree30_floating_base_arms_crossing(oracle, precision, tol):
    """the many-sphere path with a floating base and a strong self-collision term, the two arms folded across each
    other so that many pairs of the 60 spheres come within range: fp32 nominates the pairs on the matrix cores
    (csrc/self_mfma.h) and repeats the reference's range test on them, fp64 walks the rotations of the wavefront"""
    mod = _mk_module()
    model = robots.tree30()
    base = [0.1, -0.2, 0.3, 0.0, 0.0, 0.0, 1.0]
    dofvals = np.zeros(model.n_dof)
    adofs = list(range(model.n_dof))
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    grids, poses = _tree_scene(mod, oracle, 0.02)
    n_runs, n_points, n_iter = 3, 30, 12
    rng = np.random.default_rng(7)
    goals = rng.uniform(-0.4, 0.4, size=(n_runs, model.n_dof))
    goals[:, 2:5] = [0.9, 1.2, -0.6]; goals[:, 16:19] = [-0.9, 1.2, 0.6]        # both arms swing in front of the torso
    basegoals = np.tile(np.asarray(base), (n_runs, 1)); basegoals[:, :3] += rng.uniform(-0.2, 0.2, size=(n_runs, 3))
    kw = dict(n_points=n_points, lambda_=400.0, obs_factor=50.0, obs_factor_self=40.0, epsilon_self=0.08, floating_base=1)
    bid = mod.batch_create(model.name, goals, basegoals=basegoals, precision=precision, **kw)
    costs, status = mod.batch_iterate(bid, n_iter)
    traj = mod.batch_gettraj(bid)
    mod.batch_destroy(bid)
    rob = oracle.OraRobot(model)
    errs = []
    for k in range(n_runs):
        run = oracle.OraRun(rob, base, dofvals, adofs, goals[k], grids, poses, oracle.default_params(**kw), basegoal=basegoals[k])
        assert run.n == 37
        st, ocosts = run.iterate(n_iter)
        assert st == 0 and status[k] == 0
        errs.append(common.rel_l2(traj[k], run.traj()))
        assert ocosts[1] > 0.0                                  # the obstacle + self-collision cost is really there
        assert np.allclose(costs[k], ocosts, rtol=max(tol, 1e-6) * (100 if precision == 32 else 1), atol=0), (costs[k], ocosts)
        run.destroy()
    assert max(errs) <= tol, errs
    print("tree30 floating, arms crossing, fp%d worst rel L2 %.3e" % (precision, max(errs)))


def test_derivative_2(oracle):
    """D=2: pentadiagonal metric, dense A^-1 fallback on the device"""
    mod = _mk_module()
    model = common.setup_product_wam(mod)
    prob = common.tabletop_problem(oracle)
    _, base, dofvals, adofs = common.wam_state()
    goals = common.wam_goals(2, seed=3)
    kw = dict(n_points=40, lambda_=1000.0, obs_factor=100.0, D=2)
    bid = mod.batch_create(model.name, goals, derivative=2, n_points=40, lambda_=1000.0, obs_factor=100.0)
    costs, status = mod.batch_iterate(bid, 10)
    traj = mod.batch_gettraj(bid)
    rob = oracle.OraRobot(model)
    for k in range(2):
        run = oracle.OraRun(rob, base, dofvals, adofs, goals[k], [prob["sdf"]], [prob["pose"]], oracle.default_params(**kw))
        st, ocosts = run.iterate(10)
        assert st == status[k]
        assert common.rel_l2(traj[k], run.traj()) <= 1e-6
        assert np.allclose(costs[k], ocosts, rtol=1e-6, atol=0)
        run.destroy()


def test_joint_limit_status(oracle):
    """runs the reference would abort with 'Resulting trajectory is outside of joint limits!'
    are flagged per run (status -1), the rest of the batch is unaffected"""
    mod = _mk_module()
    model = common.setup_product_wam(mod)
    prob = common.tabletop_problem(oracle)
    _, base, dofvals, adofs = common.wam_state()
    goals = common.wam_goals(256, seed=20250101)
    kw = dict(n_points=100, lambda_=100.0, obs_factor=500.0)
    bid = mod.batch_create(model.name, goals, **kw)
    costs, status = mod.batch_iterate(bid, 100)
    traj = mod.batch_gettraj(bid)
    ora = lambda g: oracle.batch_run(oracle.OraRobot(model), base, dofvals, adofs, g, [prob["sdf"]], [prob["pose"]],
                                     oracle.default_params(**kw), 100)
    ores = ora(goals)
    otraj, ocosts, ostatus = ores[:3]
    assert (ostatus == -1).sum() > 0, "the workload is expected to contain diverging runs"
    # A diverging run is chaotic shortly before it fails, so the verdict may flip for a few.  What the oracle says about
    # itself (scripts/chaos_ratio.py, profiles/r04_chaos_ratio.txt): its own status agrees with its status under a one-ulp
    # change of the goal for 99.4-99.6 % of config 2's runs, and so does the HIP path's (99.4 % of 2048 runs; 97 % was the
    # bar until round 3).  Every run whose status differs must be one the oracle itself cannot reproduce.
    amp, stable = common.amplification(ora, goals, ores)
    agree = (status == ostatus)
    assert agree.mean() >= 0.98, agree.mean()
    for k in np.flatnonzero(~agree):
        assert amp[k] >= 1e-9 or not stable[k], (k, status[k], ostatus[k], amp[k])
    ok = (status == 0) & (ostatus == 0)
    errs = np.array([common.rel_l2(traj[k], otraj[k]) for k in range(len(goals))])
    assert np.median(errs[ok]) <= 1e-9
    well = ok & (amp < 1e-9) & stable
    assert well.sum() >= 0.8 * ok.sum()
    assert errs[well].max() <= 1e-6, np.sort(errs[well])[-8:]
    # the others are the runs about to diverge (cost exploding, limits hit every iteration): chaotic in the reference
    # algorithm itself, shown by the oracle alone (one-ulp changes of the goal); the HIP path is held to that conditioning
    ill = ok & ~well
    assert (errs[ill] <= np.maximum(1e-6, common.CHAOS_FACTOR * amp[ill])).all(), (errs[ill], amp[ill])
    print("joint-limit workload: status agreement %.4f, %d well-conditioned runs worst %.2e, %d ill-conditioned worst ratio %.1f"
          % (agree.mean(), well.sum(), errs[well].max(), ill.sum(), (errs[ill] / np.maximum(amp[ill], 1e-300)).max() if ill.any() else 0.0))
    from or_cdchomp_amd import bindings
    k = int(np.where(status == -1)[0][0])
    with pytest.raises(RuntimeError, match="Resulting trajectory is outside of joint limits!"):
        bindings.runchomp(mod, robot=model.name, n_iter=100, lambda_=100.0, obs_factor=500.0, n_points=100,
                          adofgoal=list(goals[k]))


def test_wam_with_finger_dofs_tree_row_kernel(oracle):
    """arm + the three finger joints optimized: a branching joint tree with <= 16 active spheres,
    i.e. the DPP-row cost phase with saved FK frames, and J^T from wrench range sums (the spheres a
    finger joint moves are a range of the row that does not end at the last sphere)"""
    mod = _mk_module()
    model = common.setup_product_wam(mod)
    prob = common.tabletop_problem(oracle)
    _, base, dofvals, _ = common.wam_state()
    adofs = list(range(10))
    mod.set_active_dofs(model.name, adofs)
    n_runs, n_points, n_iter = 6, 70, 30
    rng = np.random.default_rng(77)
    lo = np.asarray(model.limit_lower[:10]) + 0.1
    hi = np.asarray(model.limit_upper[:10]) - 0.1
    goals = rng.uniform(lo, hi, size=(n_runs, 10))
    kw = dict(n_points=n_points, lambda_=100.0, obs_factor=300.0)
    bid = mod.batch_create(model.name, goals, **kw)
    costs, status = mod.batch_iterate(bid, n_iter)
    traj = mod.batch_gettraj(bid)
    mod.batch_destroy(bid)
    rob = oracle.OraRobot(model)
    errs = []
    for k in range(n_runs):
        run = oracle.OraRun(rob, base, dofvals, adofs, goals[k], [prob["sdf"]], [prob["pose"]], oracle.default_params(**kw))
        assert run.n == 10 and run.Sa == 15
        st, ocosts = run.iterate(n_iter)
        assert st == status[k]
        if st == 0:
            errs.append(common.rel_l2(traj[k], run.traj()))
            assert np.allclose(costs[k], ocosts, rtol=1e-6, atol=0), (costs[k], ocosts)
        run.destroy()
    assert errs and max(errs) <= 1e-6, errs
    print("wam + fingers (tree, 15 spheres) worst rel L2 %.3e" % max(errs))


def test_two_link_arm_single_tile(oracle):
    """a 2-dof arm with 3 spheres: the whole trajectory is one tile (FK in two passes of 64
    waypoints), the sparse joint-limit rounds run with 128 rows per slice, most row lanes are empty"""
    mod = _mk_module()
    model = robots.RobotModel("twolink")
    R = robots.JOINT_REVOLUTE
    model.add_link("base")
    model.add_link("upper", "base", (0, 0, 0.8), joint=R, axis=(0, 1, 0), limits=(-1.2, 1.2))
    model.add_link("fore", "upper", (0.4, 0, 0), joint=R, axis=(0, 1, 0), limits=(-2.0, 0.3))
    model.add_sphere("upper", (0.2, 0, 0), 0.07)
    model.add_sphere("fore", (0.15, 0, 0), 0.06)
    model.add_sphere("fore", (0.35, 0, 0), 0.05)
    base = [-0.9, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    dofvals = np.array([-1.0, 0.2])
    adofs = [0, 1]
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    prob = common.tabletop_problem(oracle)
    n_runs, n_points, n_iter = 5, 100, 60
    goals = np.random.default_rng(9).uniform([0.2, -1.9], [1.1, 0.2], size=(n_runs, 2))
    kw = dict(n_points=n_points, lambda_=20.0, obs_factor=200.0)
    bid = mod.batch_create(model.name, goals, **kw)
    costs, status = mod.batch_iterate(bid, n_iter)
    traj = mod.batch_gettraj(bid)
    mod.batch_destroy(bid)
    rob = oracle.OraRobot(model)
    errs = []
    for k in range(n_runs):
        run = oracle.OraRun(rob, base, dofvals, adofs, goals[k], [prob["sdf"]], [prob["pose"]], oracle.default_params(**kw))
        assert run.n == 2 and run.Sa == 3
        st, ocosts = run.iterate(n_iter)
        assert st == status[k]
        if st == 0:
            errs.append(common.rel_l2(traj[k], run.traj()))
            assert np.allclose(costs[k], ocosts, rtol=1e-6, atol=0), (costs[k], ocosts)
        run.destroy()
    assert errs and max(errs) <= 1e-6, errs
    print("two-link arm worst rel L2 %.3e" % max(errs))


def test_ten_link_chain_two_waypoints_per_wavefront(oracle):
    """a 10-dof serial chain with 20 spheres: the generic cost path with 32 lanes per waypoint (two
    waypoints share a wavefront; the J^T suffix scan spans two DPP rows per waypoint)"""
    mod = _mk_module()
    model = robots.RobotModel("chain10")
    R = robots.JOINT_REVOLUTE
    model.add_link("base")
    prev = "base"
    for i in range(10):
        nm = "c%d" % i
        model.add_link(nm, prev, (0, 0, 0.12 if i else 0.5), joint=R, axis=(0, 0, 1) if i % 2 == 0 else (0, 1, 0), limits=(-1.8, 1.8))
        model.add_sphere(nm, (0, 0, 0.03), 0.045)
        model.add_sphere(nm, (0, 0, 0.09), 0.045)
        prev = nm
    base = [-0.9, 0.1, 0.0, 0.0, 0.0, 0.0, 1.0]
    dofvals = np.zeros(10); dofvals[1] = 0.9; dofvals[3] = 0.7
    adofs = list(range(10))
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    prob = common.tabletop_problem(oracle)
    n_runs, n_points, n_iter = 5, 50, 25
    goals = np.random.default_rng(12).uniform(-1.2, 1.2, size=(n_runs, 10))
    kw = dict(n_points=n_points, lambda_=150.0, obs_factor=200.0)
    bid = mod.batch_create(model.name, goals, **kw)
    costs, status = mod.batch_iterate(bid, n_iter)
    traj = mod.batch_gettraj(bid)
    mod.batch_destroy(bid)
    rob = oracle.OraRobot(model)
    errs = []
    for k in range(n_runs):
        run = oracle.OraRun(rob, base, dofvals, adofs, goals[k], [prob["sdf"]], [prob["pose"]], oracle.default_params(**kw))
        assert run.n == 10 and run.Sa == 20
        st, ocosts = run.iterate(n_iter)
        assert st == status[k]
        if st == 0:
            errs.append(common.rel_l2(traj[k], run.traj()))
            assert np.allclose(costs[k], ocosts, rtol=1e-6, atol=0), (costs[k], ocosts)
        run.destroy()
    assert errs and max(errs) <= 1e-6, errs
    print("10-link chain (20 spheres, 32 lanes per waypoint) worst rel L2 %.3e" % max(errs))


@pytest.mark.parametrize("n_points,momentum", [(300, 0), (520, 0), (300, 1)])
def test_long_trajectory_scan_solve(oracle, n_points, momentum, monkeypatch):
    """more than 256 moving waypoints (round 6): the closed-form scans with a lane's rows read twice instead of held in registers, in the
    metric solve and in the joint-limit rounds (goals at the limits: rounds are made), against the oracle; and against the cyclic
    reduction such runs took until then (ORC_SCAN_MAX_M=256) to rounding"""
    model0, base, dofvals, adofs = common.wam_state()
    lo, hi = np.array(model0.limit_lower)[:7], np.array(model0.limit_upper)[:7]
    rng = np.random.default_rng(n_points)
    n_runs = 6
    goals = common.wam_goals(n_runs, seed=3)
    goals[:3, :2] = np.where(rng.uniform(size=(3, 2)) < 0.5, lo[:2] + 0.005, hi[:2] - 0.005)
    kw = dict(n_points=n_points, lambda_=40.0 * n_points / 100.0, obs_factor=500.0, use_momentum=momentum)
    n_iter = 12
    out = {}
    switched = common.plan_switches_active()
    for name, env in (("scan", None), ("pcr", "256")):
        if env:
            monkeypatch.setenv("ORC_SCAN_MAX_M", env)
        mod = _mk_module()
        model = common.setup_product_wam(mod)
        bid = mod.batch_create(model.name, goals, **kw)
        plan = mod.batch_plan(bid)
        assert switched or plan["solve_mode"] == (0 if env else 2), plan
        costs, status = mod.batch_iterate(bid, n_iter)
        out[name] = (mod.batch_gettraj(bid), costs, status)
        mod.batch_destroy(bid)
        mod.close()
    monkeypatch.delenv("ORC_SCAN_MAX_M", raising=False)
    prob = common.tabletop_problem(oracle)
    ora = lambda g: oracle.batch_run(oracle.OraRobot(model), base, dofvals, adofs, g, [prob["sdf"]], [prob["pose"]], oracle.default_params(**kw), n_iter)
    res = ora(goals)
    amp, stable = common.amplification(ora, goals, res)
    traj, costs, status = out["scan"]
    well = (res[2] == 0) & (status == 0) & (amp < 1e-9) & stable
    assert well.sum() >= 4, (amp, res[2], status)
    for k in np.flatnonzero(well):
        assert common.rel_l2(traj[k], res[0][k]) <= 1e-6, k
        assert np.allclose(costs[k], res[1][k], rtol=1e-6, atol=0), k
    assert np.array_equal(out["scan"][2], out["pcr"][2])
    assert max(common.rel_l2(out["scan"][0][k], out["pcr"][0][k]) for k in np.flatnonzero(well)) <= 1e-9
