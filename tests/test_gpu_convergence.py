"""-m gpu: the convergence stop (orc_batch_set_convergence, Module.batch_set_convergence, the converge_* tokens of iterate /
iteratebatch).  The device must stop every run exactly where or_cdchomp_amd.module.convergence_stop says, applied to the
trace of the same runs iterated without the criterion; a stopped run must be bit for bit a run whose call had that many
iterations; every kernel family and both launch paths go through the same rule."""
import numpy as np
import pytest

import common
import or_cdchomp_amd
from or_cdchomp_amd import robots
from or_cdchomp_amd.module import convergence_stop

pytestmark = pytest.mark.gpu

KW = dict(n_points=100, lambda_=100.0, obs_factor=500.0)
INF = float("inf")


def same(a, b):
    """bit-identical arrays (NaN rows included)"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def agstate(mod, bid, m):
    """the "AG" read-back with m moving rows"""
    n_runs, _, n = mod.batch_dims(bid)
    out = np.zeros((n_runs, m, n))
    mod._check(mod._lib.orc_batch_get_state(mod._h, bid, b"AG", out.ctypes.data_as(or_cdchomp_amd._capi.c_double_p), out.size))
    return out


def run(mod, make, idx, n_iter, crit=None, m=None):
    """create the runs `idx` (make(idx) -> batch id), optionally set the criterion, iterate n_iter, read everything back"""
    bid = make(idx)
    if crit is not None:
        mod.batch_set_convergence(bid, *crit)
    costs, status = mod.batch_iterate(bid, n_iter)
    n_points = mod.batch_dims(bid)[1]
    out = dict(costs=costs, status=status, iters=mod.batch_iterations_done(bid), trace=mod.batch_trace(bid, n_iter),
               traj=mod.batch_gettraj(bid), ag=agstate(mod, bid, m if m is not None else n_points - 2))
    mod.batch_destroy(bid)
    return out


def check_stop(mod, make, n_runs, n_iter, crit, equiv=True, m=None, max_groups=None):
    """tests 2 and 3 of the feature: the stop iteration and status follow convergence_stop of the trace without the
    criterion, the trace before the stop is that trace bit for bit and NaN after it; a stopped run equals a fresh run of
    the same composition... iterated exactly as often (bits of trajectory, costs, AG, iterations, status 0)"""
    idx = np.arange(n_runs)
    a = run(mod, make, idx, n_iter, m=m)
    # crit = (rtol or a list of them, patience, obs_max): the first rtol at which the workload holds runs that stop and runs
    # that do not, so that the test cannot pass vacuously (the traces of `a` are deterministic)
    rtols, patience, obs_max = crit
    for rtol in np.atleast_1d(rtols):
        iters, stopped = convergence_stop(a["trace"], float(rtol), patience, obs_max)
        if stopped.any() and (~stopped).any():
            break
    assert stopped.any() and (~stopped).any(), ("the workload must hold runs that stop and runs that do not", stopped.sum())
    crit = (float(rtol), patience, obs_max)
    b = run(mod, make, idx, n_iter, crit=crit, m=m)
    assert np.array_equal(b["iters"], iters)
    want = np.where(stopped, 1, a["status"])
    assert np.array_equal(b["status"], want), (b["status"], want)
    assert set(np.unique(b["status"])) <= {-1, 0, 1}
    for k in range(n_runs):
        assert same(b["trace"][k, :iters[k]], a["trace"][k, :iters[k]]), k
        assert np.isnan(b["trace"][k, iters[k]:]).all(), k
    # runs that did not stop are the runs of the call without the criterion
    keep = ~stopped
    for key in ("costs", "traj", "iters", "status"):
        assert same(b[key][keep], a[key][keep]), key
    if not equiv:
        return a, b, iters, stopped
    groups = sorted(set(iters[stopped].tolist()))
    if max_groups is not None and len(groups) > max_groups:
        groups = [groups[int(round(j))] for j in np.linspace(0, len(groups) - 1, max_groups)]
    for cnt in groups:
        sel = np.flatnonzero(stopped & (iters == cnt))
        f = run(mod, make, sel, int(cnt), m=m)
        assert (f["status"] == 0).all() and (f["iters"] == cnt).all(), cnt
        for key in ("traj", "costs", "ag"):
            assert same(f[key], b[key][sel]), (cnt, key)
    return a, b, iters, stopped


# ---- the WAM tabletop: exact stop iteration, equivalence, the oracle --------------------------------------------------

@pytest.fixture(scope="module")
def wam():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    yield mod, model
    mod.close()


def wam_maker(mod, model, goals, **kw):
    return lambda idx: mod.batch_create(model.name, goals[idx], **dict(KW, **kw))


def test_wam_stop_iteration_and_equivalence(wam):
    mod, model = wam
    goals = common.wam_goals(256, seed=20250101)
    check_stop(mod, wam_maker(mod, model, goals), 256, 300, (1e-3, 3, INF))


def test_wam_obs_max(wam):
    """obs_max = 0: on the tabletop no run's obstacle cost is exactly zero, so none stops and every run is the run without
    the criterion; then the median of the final obstacle costs, at which some runs stop and some do not"""
    mod, model = wam
    goals = common.wam_goals(256, seed=20250101)
    make = wam_maker(mod, model, goals)
    idx = np.arange(256)
    a = run(mod, make, idx, 300)
    b = run(mod, make, idx, 300, crit=(1e-3, 3, 0.0))
    iters, stopped = convergence_stop(a["trace"], 1e-3, 3, 0.0)
    assert np.array_equal(b["iters"], iters) and np.array_equal(b["status"], np.where(stopped, 1, a["status"]))
    for key in ("costs", "traj", "trace"):
        assert same(b[key][~stopped], a[key][~stopped]), key
    made = a["iters"]
    last_obs = a["trace"][idx, np.maximum(made - 1, 0), 1]
    check_stop(mod, make, 256, 300, (1e-3, 3, float(np.median(last_obs[made > 0]))), max_groups=12)


def test_wam_stopped_runs_match_the_oracle(wam, oracle):
    """16 well-conditioned stopped runs against the oracle iterated as often as the run was (1e-6 relative L2)"""
    mod, model = wam
    goals = common.wam_goals(64, seed=77)
    bid = mod.batch_create(model.name, goals, **KW)
    mod.batch_set_convergence(bid, 1e-3, 3)
    costs, status = mod.batch_iterate(bid, 300)
    iters = mod.batch_iterations_done(bid)
    traj = mod.batch_gettraj(bid)
    mod.batch_destroy(bid)
    prob = common.tabletop_problem(oracle)
    _, base, dofvals, adofs = common.wam_state()
    rob = oracle.OraRobot(model)
    checked = 0
    for k in np.flatnonzero(status == 1):
        if checked == 16:
            break
        ora = lambda g: oracle.batch_run(rob, base, dofvals, adofs, g, [prob["sdf"]], [prob["pose"]],
                                         oracle.default_params(**KW), int(iters[k]))
        res = ora(goals[[k]])
        amp, stable = common.amplification(ora, goals[[k]], res)
        if res[2][0] != 0 or not stable[0] or amp[0] >= 1e-9:
            continue
        assert common.rel_l2(traj[k], res[0][0]) <= 1e-6, (k, common.rel_l2(traj[k], res[0][0]))
        assert np.allclose(costs[k], res[1][0], rtol=1e-6, atol=0), (k, costs[k], res[1][0])
        checked += 1
    assert checked == 16, checked


# ---- every kernel family through the same loop -----------------------------------------------------------------------

def test_family_fp32(wam):
    mod, model = wam
    goals = common.wam_goals(64, seed=5)
    check_stop(mod, wam_maker(mod, model, goals, precision=32), 64, 150, (1e-3, 3, INF), max_groups=6)


def test_family_derivative2(wam):
    mod, model = wam
    goals = common.wam_goals(64, seed=6)
    check_stop(mod, wam_maker(mod, model, goals, derivative=2), 64, 150, (np.geomspace(1e-3, 1e-1, 25), 3, INF), max_groups=6)


def test_family_momentum(wam):
    mod, model = wam
    goals = common.wam_goals(64, seed=7)
    check_stop(mod, wam_maker(mod, model, goals, use_momentum=1), 64, 150, (1e-3, 3, INF), max_groups=6)


def test_family_momentum_hmc(wam):
    """the resamples of a call are planned for all its iterations: only the trace prefix and the stop iteration"""
    mod, model = wam
    goals = common.wam_goals(64, seed=8)
    seeds = np.arange(64, dtype=np.uint32)
    make = lambda idx: mod.batch_create(model.name, goals[idx], seeds=seeds[idx],
                                        **dict(KW, use_momentum=1, use_hmc=1, hmc_resample_lambda=0.05))
    check_stop(mod, make, 64, 150, (1e-3, 3, INF), equiv=False)


@pytest.mark.parametrize("threads", [512, 192])
def test_family_workgroup_shapes(threads):
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    mod.set_workgroup_threads(threads)
    goals = common.wam_goals(48, seed=9)
    make = wam_maker(mod, model, goals)
    bid = make(np.arange(2))
    assert mod.batch_plan(bid)["threads"] == threads or common.plan_switches_active()
    mod.batch_destroy(bid)
    check_stop(mod, make, 48, 150, (1e-3, 3, INF), max_groups=6)
    mod.close()


def test_family_held4():
    mod = or_cdchomp_amd.Module(0)
    model, _, _ = common.setup_product_wam_held4(mod)
    goals = common.wam_goals(48, seed=10)
    check_stop(mod, wam_maker(mod, model, goals), 48, 150, (1e-3, 3, INF), max_groups=6)
    mod.close()


def test_family_tree30():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_tree30(mod)
    goals = common.config5_goals(48)
    make = lambda idx: mod.batch_create(model.name, goals[idx], **common.CONFIG5_KW)
    check_stop(mod, make, 48, 120, ([1e-3, 1e-4, 1e-5, 1e-6, 1e-7], 3, INF), max_groups=6)
    mod.close()


def test_family_con_tsr():
    mod = or_cdchomp_amd.Module(0)
    s2 = np.sqrt(0.5)
    base = [-1.0, 0.0, 1.0, 0.0, s2, 0.0, s2]
    model, _, dofvals, adofs = common.wam_state()
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    from or_cdchomp_amd import scenes
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    R, t = model.link_frames(base, dofvals)
    li = model.link_names.index("wam7")
    tsr = robots.Tsr(T0w_R=R[li], T0w_d=t[li], Bw=[[-1, 1], [-1, 1], [0, 0], [0, 0], [0, 0], [-3, 3]])
    rng = np.random.default_rng(3)
    goals = np.array(robots.WAM_START)[None, :] + 0.4 * rng.uniform(-1, 1, size=(32, 7))

    def make(idx):
        g = np.ascontiguousarray(goals[idx])
        return int(mod.SendCommand("createbatch robot %s n_runs %d adofgoals 0x%x n_points 40 lambda 100 obs_factor 200 "
                                   "con_tsr 'all link wam7' '%s'" % (model.name, len(idx), g.ctypes.data, tsr.serialize())))
    check_stop(mod, make, 32, 80, (1e-4, 2, INF), max_groups=6)
    mod.close()


# ---- launch paths and the command layer ------------------------------------------------------------------------------

def test_per_iteration_launches_match_the_fused_call(wam, tmp_path):
    """iteratebatch ... trajs_fileformstr (one launch per iteration) with the criterion: the fused call's iterations,
    status, costs and trajectories; the call's converge_* tokens do not stay on the batch"""
    mod, model = wam
    goals = common.wam_goals(32, seed=12)
    a = mod.batch_create(model.name, goals, **KW)
    b = mod.batch_create(model.name, goals, **KW)
    res = []
    for bid, extra in ((a, ""), (b, " trajs_fileformstr '%s'" % str(tmp_path / "t_%d_%d.txt"))):
        costs = np.zeros((32, 3)); st = np.full(32, 9, dtype=np.int32)
        mod.SendCommand("iteratebatch run %d n_iter 150 costs 0x%x status 0x%x converge_rtol 1e-3 converge_patience 3%s"
                        % (bid, costs.ctypes.data, st.ctypes.data, extra))
        res.append(dict(costs=costs, status=st, iters=mod.batch_iterations_done(bid), traj=mod.batch_gettraj(bid)))
    assert (res[0]["status"] == 1).any() and (res[0]["status"] == 0).any()
    for key in ("costs", "status", "iters", "traj"):
        assert same(res[0][key], res[1][key]), key
    # the next call of the batch runs without the criterion again
    _, st = mod.batch_iterate(a, 5)
    assert (st != 1).all() and (mod.batch_iterations_done(a)[st == 0] == 5).all()
    mod.batch_destroy(a); mod.batch_destroy(b)


def test_shards_match_one_batch(wam):
    """createbatch ... devices '0 0': the runs of both shards stop exactly where the one-shard batch's do"""
    mod, model = wam
    goals = np.ascontiguousarray(common.wam_goals(40, seed=13))
    one = mod.batch_create(model.name, goals, **KW)
    two = int(mod.SendCommand("createbatch robot %s n_runs 40 adofgoals 0x%x n_points 100 lambda 100 obs_factor 500 devices '0 0'"
                              % (model.name, goals.ctypes.data)))
    out = []
    for bid in (one, two):
        mod.batch_set_convergence(bid, 1e-3, 3)
        costs, status = mod.batch_iterate(bid, 200)
        out.append(dict(costs=costs, status=status, iters=mod.batch_iterations_done(bid), traj=mod.batch_gettraj(bid),
                        trace=mod.batch_trace(bid, 200)))
        mod.batch_destroy(bid)
    assert (out[0]["status"] == 1).any() and (out[0]["status"] == 0).any()
    assert (out[1]["status"][:20] == 1).any() and (out[1]["status"][20:] == 1).any()
    for key in out[0]:
        assert same(out[0][key], out[1][key]), key


def test_single_run_commands(wam, tmp_path):
    """create / iterate ... converge_rtol: the cost text comes back without an exception when the run converges; the fused
    and the per-iteration forms stop where convergence_stop of the run's own trace says"""
    mod, model = wam
    goals = common.wam_goals(16, seed=14)
    bid = mod.batch_create(model.name, goals, **KW)
    _, st = mod.batch_iterate(bid, 300)
    iters, stopped = convergence_stop(mod.batch_trace(bid, 300), 1e-3, 3)
    mod.batch_destroy(bid)
    k = int(np.flatnonzero(stopped & (st == 0))[0])
    goal = " ".join(repr(float(v)) for v in goals[k])
    create = "create robot %s adofgoal '%s' n_points 100 lambda 100 obs_factor 500" % (model.name, goal)
    r = int(mod.SendCommand(create))
    mod.SendCommand("iterate run %d n_iter 300" % r)
    want, _ = convergence_stop(mod.batch_trace(r, 300)[0], 1e-3, 3)
    mod.SendCommand("destroy run %d" % r)
    texts, made = [], []
    for extra in ("", " trajs_fileformstr '%s'" % str(tmp_path / "one_%d.txt")):
        r = int(mod.SendCommand(create))
        texts.append(mod.SendCommand("iterate run %d n_iter 300 converge_rtol 1e-3 converge_patience 3%s" % (r, extra)))
        made.append(int(mod.batch_iterations_done(r)[0]))
        mod.SendCommand("destroy run %d" % r)
    assert made[0] == made[1] == want and want < 300, (made, want)
    assert texts[0] == texts[1] and np.isfinite(float(texts[0]))


def test_bad_arguments_leave_the_module_usable(wam):
    mod, model = wam
    goals = common.wam_goals(4, seed=15)
    bid = mod.batch_create(model.name, goals, **KW)
    for rtol, patience, obs_max in ((0.0, 3, INF), (-1e-3, 3, INF), (float("nan"), 3, INF), (1e-3, 3, float("nan"))):
        with pytest.raises(RuntimeError, match="convergence"):
            mod.batch_set_convergence(bid, rtol, patience, obs_max)
    for tokens in ("converge_rtol 0", "converge_rtol -1", "converge_rtol nan", "converge_rtol 1e-3 converge_obs nan",
                   "converge_patience 3", "converge_rtol abc"):
        with pytest.raises(RuntimeError):
            mod.SendCommand("iteratebatch run %d n_iter 5 %s" % (bid, tokens))
    # patience 0 switches it off without asking for a valid rtol
    mod.batch_set_convergence(bid, 0.0, 0)
    costs, status = mod.batch_iterate(bid, 5)
    assert (status == 0).all() and (mod.batch_iterations_done(bid) == 5).all() and np.isfinite(costs).all()
    mod.batch_destroy(bid)
    bid = mod.batch_create(model.name, goals, **KW)
    _, status = mod.batch_iterate(bid, 5)
    assert (status == 0).all()
    mod.batch_destroy(bid)
