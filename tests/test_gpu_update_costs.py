"""-m gpu: the update and the costs of an iteration made in one phase call (csrc/chomp_kernel.hip phase_update_costs), against the
oracle, on the smallest shape on which the lean update, the joint-limit rounds and the cost sums all run: the WAM of config 2
with 20 waypoints (18 moving ones, one tile), 8 runs, 6 iterations.  What the fused call must keep of the two calls it
replaces: the per-iteration trace (total, obs, smooth), the abort rule of chomp.c:651-655 (no costs, no trace row and no
renormalisation in the iteration that gives up), the stand-alone cost-only pass that ends a call, the convergence stop,
the quaternion renormalisation of a floating base, the row copy of `start_tsr`, and a call made of several launches."""
import numpy as np
import pytest

import common
import or_cdchomp_amd
from or_cdchomp_amd import robots
from test_gpu_convergence import check_stop, same, wam_maker

pytestmark = pytest.mark.gpu

N_RUNS, N_POINTS, N_ITER = 8, 20, 6
KW = dict(n_points=N_POINTS, lambda_=100.0, obs_factor=500.0)      # config 2's parameters
TOL = 1e-6                                                          # the project's bound against the oracle (fp64)
INF = float("inf")


@pytest.fixture(scope="module")
def wam():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    yield mod, model
    mod.close()


@pytest.fixture(scope="module")
def scene(oracle):
    """what every oracle run of the tabletop takes, built once"""
    model, base, dofvals, adofs = common.wam_state()
    prob = common.tabletop_problem(oracle)
    return dict(O=oracle, rob=oracle.OraRobot(model), base=base, dofvals=dofvals, adofs=adofs, grids=[prob["sdf"]], poses=[prob["pose"]])


def oracle_runs(scene, goals, kw, n_iter=N_ITER, base=None, basegoals=None, seeds=None, start_tsr=None):
    """every run by the oracle with its trace: status [n], iterations made [n], costs [n][3], trace [n][n_iter][3]
    (the rows of iterations not made NaN, as the product reports them), trajectories, limit rounds of the last iteration"""
    O = scene["O"]
    okw = dict(kw)
    if "derivative" in okw:
        okw["D"] = okw.pop("derivative")
    okw.pop("precision", None)
    st, it, costs, trace, traj = [], [], [], [], []
    for k, g in enumerate(goals):
        p = O.default_params(start_tsr=start_tsr, **(dict(okw, seed=int(seeds[k])) if seeds is not None else okw))
        run = O.OraRun(scene["rob"], scene["base"] if base is None else base, scene["dofvals"], scene["adofs"], g, scene["grids"],
                       scene["poses"], p, basegoal=None if basegoals is None else basegoals[k])
        s, c, tr = run.iterate(n_iter, trace=True)
        made = run.iter()
        tr = tr.copy(); tr[made:] = np.nan
        st.append(s); it.append(made); costs.append(c); trace.append(tr); traj.append(run.traj().copy())
        run.destroy()
    return np.array(st), np.array(it), np.array(costs), np.array(trace), traj


def limit_rounds(scene, goals, kw, n_iter=N_ITER):
    """joint-limit rounds the oracle makes over the iterations of every run"""
    O = scene["O"]
    total = 0
    for g in goals:
        run = O.OraRun(scene["rob"], scene["base"], scene["dofvals"], scene["adofs"], g, scene["grids"], scene["poses"], O.default_params(**kw))
        for _ in range(n_iter):
            run.iterate(1)
            total += run.chomp().last_num_limadjs
        run.destroy()
    return total


def product(mod, bid, n_iter=N_ITER):
    costs, status = mod.batch_iterate(bid, n_iter)
    return dict(costs=costs, status=status, iters=mod.batch_iterations_done(bid), trace=mod.batch_trace(bid, n_iter), traj=mod.batch_gettraj(bid))


def assert_trace(got, want, made, tol=TOL):
    """rows [0, made) within the bound, the rows from `made` on NaN"""
    print("trace rows %d: worst relative difference %.3e (bound %.1e)" % (made, np.max(np.abs(got[:made] / want[:made] - 1.0), initial=0.0), tol))
    assert np.allclose(got[:made], want[:made], rtol=tol, atol=0), (got[:made], want[:made])
    assert np.isnan(got[made:]).all()


def test_plain(wam, scene):
    """trace, final costs and trajectories on the well-conditioned runs; the workload makes joint-limit rounds"""
    mod, model = wam
    goals = common.wam_goals(N_RUNS)
    assert limit_rounds(scene, goals, KW) > 0, "the workload is expected to make joint-limit rounds"
    bid = mod.batch_create(model.name, goals, **KW)
    p = product(mod, bid)
    mod.batch_destroy(bid)
    ost, oit, ocosts, otrace, otraj = oracle_runs(scene, goals, KW)
    assert np.array_equal(p["status"], ost) and (ost == 0).all() and np.array_equal(p["iters"], oit)
    O = scene["O"]
    ora = lambda g: O.batch_run(scene["rob"], scene["base"], scene["dofvals"], scene["adofs"], g, scene["grids"], scene["poses"],
                                O.default_params(**KW), N_ITER)
    amp, stable = common.amplification(ora, goals, (otraj, ocosts, ost))
    well = (amp < 1e-9) & stable
    assert well.sum() >= 0.8 * N_RUNS, (amp, stable)
    for k in np.flatnonzero(well):
        assert_trace(p["trace"][k], otrace[k], N_ITER)
        assert np.allclose(p["costs"][k], ocosts[k], rtol=TOL, atol=0), (p["costs"][k], ocosts[k])
        err = common.rel_l2(p["traj"][k], otraj[k])
        assert err <= TOL, (k, err)


def corner_goals(model):
    """every joint of the goal at its lower or its upper limit"""
    lo, hi = np.asarray(model.limit_lower[:7]), np.asarray(model.limit_upper[:7])
    pick = np.random.default_rng(20250101).integers(0, 2, size=(N_RUNS, 7))
    return np.where(pick, hi, lo)


def test_aborted_runs(wam, scene):
    """goals at the joint limits and a long step (lambda 10): six of the eight runs give up in the limit rounds of iterations
    1 .. 4 (the oracle's verdict is the same under one-ulp changes of the goals).  The iteration that gives up writes no trace row"""
    mod, model = wam
    kw = dict(KW, lambda_=10.0)
    goals = corner_goals(model)
    ost, oit, ocosts, otrace, otraj = oracle_runs(scene, goals, kw)
    assert (ost == -1).sum() >= 2 and (ost == 0).sum() >= 1, ost
    bid = mod.batch_create(model.name, goals, **kw)
    p = product(mod, bid)
    mod.batch_destroy(bid)
    assert np.array_equal(p["status"], ost), (p["status"], ost)
    assert np.array_equal(p["iters"], oit), (p["iters"], oit)
    for k in range(N_RUNS):
        assert_trace(p["trace"][k], otrace[k], int(oit[k]))
        if ost[k] == -1 and oit[k] > 0:
            assert np.array_equal(p["costs"][k], p["trace"][k, oit[k] - 1])      # the costs of the last complete iteration


def test_cost_only_pass_equals_a_following_n_iter_0_call(wam, scene):
    """the cost-only pass that ends a call is the stand-alone phase_costs: a following call of no iterations makes the same
    pass on the same trajectory"""
    mod, model = wam
    goals = common.wam_goals(N_RUNS)
    bid = mod.batch_create(model.name, goals, **KW)
    costs6, status6 = mod.batch_iterate(bid, N_ITER)
    traj6 = mod.batch_gettraj(bid)
    costs0, status0 = mod.batch_iterate(bid, 0)
    traj0 = mod.batch_gettraj(bid)
    mod.batch_destroy(bid)
    assert (status6 == 0).all() and (status0 == 0).all()
    assert same(costs0, costs6) and same(traj0, traj6)
    _, _, ocosts, _, _ = oracle_runs(scene, goals, KW)
    assert np.allclose(costs0, ocosts, rtol=TOL, atol=0)


def test_convergence_stop(wam):
    """the stop rule runs at the end of the fused call: iterations, status, trace and costs of the stopped runs follow
    convergence_stop on the trace of the same runs without the criterion, and equal a fresh call of that many iterations
    (the comparison of tests/test_gpu_convergence.py; patience 1, the first rtol at which some runs stop and some do not)"""
    mod, model = wam
    goals = common.wam_goals(N_RUNS)
    make = lambda idx: mod.batch_create(model.name, goals[idx], **KW)
    check_stop(mod, make, N_RUNS, N_ITER, (np.geomspace(3e-3, 3e-2, 5), 1, INF), max_groups=3)


def test_floating_base_momentum_hmc(wam, scene):
    """config 4's options on four runs: the trace of one call against the oracle, and, call by call of one iteration, unit
    quaternions in every row after every iteration (the renormalisation follows the sums inside the fused call)"""
    mod, model = wam
    n_runs = 4
    rng = np.random.default_rng(20250103)
    goals = common.wam_goals(n_runs, seed=20250103)
    basegoals = np.tile(np.asarray(scene["base"], dtype=np.float64), (n_runs, 1))
    basegoals[:, :3] += rng.uniform(-0.3, 0.3, size=(n_runs, 3))
    seeds = np.arange(n_runs, dtype=np.uint32)
    kw = dict(KW, floating_base=1, use_momentum=1, use_hmc=1, hmc_resample_lambda=0.02)
    bid = mod.batch_create(model.name, goals, basegoals=basegoals, seeds=seeds, **kw)
    p = product(mod, bid)
    mod.batch_destroy(bid)
    ost, oit, ocosts, otrace, otraj = oracle_runs(scene, goals, kw, basegoals=basegoals, seeds=seeds)
    assert (ost == 0).all() and (p["status"] == 0).all()
    for k in range(n_runs):
        assert_trace(p["trace"][k], otrace[k], N_ITER)
        assert common.rel_l2(p["traj"][k], otraj[k]) <= TOL
    bid = mod.batch_create(model.name, goals, basegoals=basegoals, seeds=seeds, **kw)
    for it in range(N_ITER):
        mod.batch_iterate(bid, 1)
        q = mod.batch_gettraj(bid)[:, :, 3:7]
        # a quaternion scaled by 1/|q| in double has a norm within a few ulp of 1
        assert np.abs(np.linalg.norm(q, axis=2) - 1.0).max() <= 1e-15, (it, np.abs(np.linalg.norm(q, axis=2) - 1.0).max())
    mod.batch_destroy(bid)


def test_start_tsr(scene):
    """`start_tsr` (free_start): the row in front of the start point is copied after the sums, as in the stand-alone pass"""
    O = scene["O"]
    s2 = np.sqrt(0.5)
    base = [-1.0, 0.0, 1.0, 0.0, s2, 0.0, s2]
    mod = or_cdchomp_amd.Module(0)
    model, _, dofvals, adofs = common.wam_state()
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    from or_cdchomp_amd import scenes
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    tool = [0, 0, 0.16, 0, 0, 0, 1]
    R, t, _, _ = scene["rob"].fk(base, dofvals)
    li = model.link_names.index("handbase")
    Ree, tee = R[li], t[li] + R[li] @ np.array(tool[:3])
    Bw = [[0, 0], [0, 0], [0, 0], [-3, 3], [-3, 3], [-3, 3]]      # hand position fixed, orientation free
    tsr = robots.Tsr(T0w_R=Ree, T0w_d=tee, Bw=Bw)
    goals = np.ascontiguousarray(np.array(robots.WAM_START)[None, :] + 0.3 * np.random.default_rng(11).uniform(-1, 1, size=(N_RUNS, 7)))
    bid = int(mod.SendCommand("createbatch robot %s n_runs %d adofgoals 0x%x n_points %d lambda 100 obs_factor 200 start_tsr '%s'"
                              % (model.name, N_RUNS, goals.ctypes.data, N_POINTS, tsr.serialize())))
    p = product(mod, bid)
    mod.batch_destroy(bid)
    mod.close()
    kw = dict(n_points=N_POINTS, lambda_=100.0, obs_factor=200.0)
    ost, oit, ocosts, otrace, otraj = oracle_runs(scene, goals, kw, base=base, start_tsr=(li, tool, O.pose_from_dR(tee, Ree), [0, 0, 0, 0, 0, 0, 1], Bw))
    assert np.array_equal(p["status"], ost) and np.array_equal(p["iters"], oit) and (ost == 0).all()
    for k in range(N_RUNS):
        assert_trace(p["trace"][k], otrace[k], N_ITER)
        assert common.rel_l2(p["traj"][k], otraj[k]) <= TOL


def test_derivative_2(wam, scene):
    """`derivative 2`: the general update mode and the band form of the smoothness cost inside the fused call"""
    mod, model = wam
    goals = common.wam_goals(N_RUNS)
    kw = dict(KW, derivative=2)
    bid = mod.batch_create(model.name, goals, **kw)
    p = product(mod, bid)
    mod.batch_destroy(bid)
    ost, oit, ocosts, otrace, otraj = oracle_runs(scene, goals, kw)
    assert np.array_equal(p["status"], ost) and np.array_equal(p["iters"], oit)
    for k in range(N_RUNS):
        assert_trace(p["trace"][k], otrace[k], int(oit[k]))


def test_fp32(wam, scene):
    """one fp32 batch: the trace at 1e-3"""
    mod, model = wam
    goals = common.wam_goals(N_RUNS)
    bid = mod.batch_create(model.name, goals, precision=32, **KW)
    p = product(mod, bid)
    mod.batch_destroy(bid)
    ost, oit, ocosts, otrace, otraj = oracle_runs(scene, goals, KW)
    assert np.array_equal(p["status"], ost) and np.array_equal(p["iters"], oit)
    for k in range(N_RUNS):
        assert_trace(p["trace"][k], otrace[k], N_ITER, tol=1e-3)


def test_two_launches_of_one_call(wam, scene, tmp_path):
    """a call made of several launches (iterate ... max_time: one iteration per launch, each but the first continuing the call
    with the runs' status carried over): the log lines the launches write one after the other (create's dat_filename: iteration,
    seconds, total, obs, smooth) are the lines of the same call made by one launch, and the oracle's trace to the log's six
    decimals; costs, status and trajectories are those of the one launch, bit for bit"""
    mod, model = wam
    goals = np.ascontiguousarray(common.wam_goals(N_RUNS))
    out = {}
    for name, more in (("one", ""), ("many", " max_time 1e9")):
        bid = int(mod.SendCommand("createbatch robot %s n_runs %d adofgoals 0x%x n_points %d lambda 100 obs_factor 500 dat_filename '%s'"
                                  % (model.name, N_RUNS, goals.ctypes.data, N_POINTS, str(tmp_path / (name + "%d.dat")))))
        costs = np.zeros((N_RUNS, 3)); status = np.zeros(N_RUNS, dtype=np.int32)
        mod.SendCommand("iteratebatch run %d n_iter %d%s costs 0x%x status 0x%x" % (bid, N_ITER, more, costs.ctypes.data, status.ctypes.data))
        out[name] = dict(costs=costs, status=status, traj=mod.batch_gettraj(bid))
        mod.batch_destroy(bid)
    _, _, _, otrace, _ = oracle_runs(scene, goals, KW)
    for key in ("costs", "status", "traj"):
        assert same(out["one"][key], out["many"][key]), key
    for k in range(N_RUNS):
        rows = {name: [ln.split() for ln in open(str(tmp_path / ("%s%d.dat" % (name, k)))).read().splitlines()] for name in out}
        assert [int(r[0]) for r in rows["many"]] == list(range(N_ITER))
        assert [r[2:] for r in rows["many"]] == [r[2:] for r in rows["one"]], k
        got = np.array([[float(v) for v in r[2:]] for r in rows["many"]])
        assert np.allclose(got, otrace[k], rtol=TOL, atol=6e-7)                  # %f keeps six decimals
