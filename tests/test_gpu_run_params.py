"""-m gpu: per-run optimizer parameters (orc_batch_set_run_params, orc_batch_select_best_by and their Module methods): a portfolio of
lambda / epsilon / obs_factor / obs_factor_self sets in one batch.  A run with per-run values p is held, bit for bit, to the same
run in a batch created with p as its shared parameters, in every kernel family and at every read site; the mixed batch is held to
the oracle run with each set; the read-back to run_params_table and the selection to select_best(..., column=)."""
import numpy as np
import pytest

import common
import or_cdchomp_amd
from or_cdchomp_amd import robots, scenes as scene_lib
from or_cdchomp_amd.module import run_params_table, select_best

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
# every set differs from every other in all four values: a swapped column cannot pass
SETS = [dict(lambda_=100.0, obs_factor=500.0, obs_factor_self=10.0, epsilon=0.10),
        dict(lambda_=50.0, obs_factor=200.0, obs_factor_self=10.0, epsilon=0.10),
        dict(lambda_=200.0, obs_factor=1000.0, obs_factor_self=5.0, epsilon=0.06),
        dict(lambda_=400.0, obs_factor=500.0, obs_factor_self=20.0, epsilon=0.14)]
NS = len(SETS)
KEYS = ("traj", "costs", "status", "iters", "trace", "AG")


def table(set_of_run):
    """the four arrays of batch_set_run_params for runs that take the sets `set_of_run`"""
    return {k: np.array([SETS[s][k] for s in set_of_run]) for k in SETS[0]}


def mixed_goals(goals):
    """run r of a mixed batch is goal r // 4 with set r % 4"""
    return np.repeat(np.asarray(goals), NS, axis=0), np.arange(len(goals) * NS) % NS


def results(mod, bid, n_iter):
    costs, status = mod.batch_iterate(bid, n_iter)
    return dict(costs=costs, status=status, traj=mod.batch_gettraj(bid), iters=mod.batch_iterations_done(bid),
                trace=mod.batch_trace(bid, n_iter), AG=mod.batch_state(bid, "AG"))


def assert_same(a, b, what=""):
    for key in KEYS:
        assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)


def rows(res, idx):
    return {k: res[k][idx] for k in KEYS}


@pytest.fixture(scope="module")
def wam():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    yield mod, model
    mod.close()


GOALS = common.wam_goals(8, seed=11)


# ---- 1. a mixed batch is the separate batches, bit for bit ---------------------------------------------------------

def _wam_case(**kw):
    def make():
        mod = or_cdchomp_amd.Module(0)
        model = common.setup_product_wam(mod)
        return mod, GOALS, lambda goals, pset, seeds=None: mod.batch_create(model.name, goals, seeds=seeds, **dict(kw, **pset))
    return make


def _two_fields():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    mod.SendCommand("computedistancefield kinbody mug")
    return mod, GOALS, lambda goals, pset, seeds=None: mod.batch_create(model.name, goals, **dict(n_points=100, **pset))


def _held4():
    mod = or_cdchomp_amd.Module(0)
    model, _, _ = common.setup_product_wam_held4(mod)
    return mod, GOALS[:4], lambda goals, pset, seeds=None: mod.batch_create(model.name, goals, **dict(n_points=100, **pset))


def _tree():
    mod = or_cdchomp_amd.Module(0)
    model = robots.tree30()
    mod.add_robot(model, transform=[0.0] * 6 + [1.0], dof_values=np.zeros(model.n_dof), active_dofs=list(range(model.n_dof)))
    for name, (boxes, pose) in scene_lib.random_boxes(np.random.default_rng(20250104)).items():
        mod.add_kinbody_boxes(name, boxes, transform=pose)
        mod.SendCommand("computedistancefield kinbody %s cube_extent 0.02 aabb_padding 0.15" % name)
    goals = np.random.default_rng(5).uniform(-0.8, 0.8, size=(4, model.n_dof))
    return mod, goals, lambda g, pset, seeds=None: mod.batch_create(model.name, g, precision=32, **dict(n_points=40, **pset))


def _con_tsr():
    """the WAM with its elbow height held on every point (`con_tsr`), created through the createbatch command"""
    mod = or_cdchomp_amd.Module(0)
    model, _, dofvals, adofs = common.wam_state()
    s2 = float(np.sqrt(0.5))
    base = [-1.0, 0.0, 1.0, 0.0, s2, 0.0, s2]
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    scene_lib.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    R, t = model.link_frames(base, dofvals)
    elbow = model.link_names.index("wam4")
    goals = np.ascontiguousarray(np.array(robots.WAM_START)[None, :] + 0.3 * np.random.default_rng(11).uniform(-1, 1, size=(4, 7)))
    tsr = robots.Tsr(T0w_R=R[elbow], T0w_d=t[elbow], Bw=[[-1, 1], [-1, 1], [0, 0], [-3, 3], [-3, 3], [-3, 3]])

    def create(g, pset, seeds=None):
        g = np.ascontiguousarray(g, dtype=np.float64)
        cmd = "createbatch robot %s n_runs %d adofgoals 0x%x n_points 30 lambda %r obs_factor %r obs_factor_self %r epsilon %r" % (
            model.name, len(g), g.ctypes.data, pset["lambda_"], pset["obs_factor"], pset["obs_factor_self"], pset["epsilon"])
        cmd += " con_tsr 'all link wam4' '%s'" % tsr.serialize()
        return int(mod.SendCommand(cmd))
    return mod, goals, create


CASES = {
    "wam-fp64-100": _wam_case(n_points=100),                    # the two-tile, four-per-CU headline kernel
    "wam-fp64-30": _wam_case(n_points=30),                      # the 128-thread shape
    "wam-fp32": _wam_case(n_points=100, precision=32),
    "wam-two-fields": _two_fields,                              # the general, not one-field, kernel
    "wam-derivative-2": _wam_case(n_points=100, derivative=2),  # the band-metric solve
    "wam-momentum-hmc": _wam_case(n_points=100, use_momentum=1, use_hmc=1),      # lambda in the leapfrog factors
    "held4": _held4,                                            # the pair-list family
    "tree30-fp32-40": _tree,                                    # the many-sphere family
    "con-tsr": _con_tsr,                                        # tsr.h's 1/lambda
}


@pytest.mark.parametrize("case", list(CASES))
def test_a_mixed_batch_is_the_separate_batches(case):
    """created with P0 shared, then all four arrays set: run 4 g + s equals run g of a batch created with set s, bit for bit"""
    mod, goals, create = CASES[case]()
    try:
        n_iter = 20
        run_goals, set_of_run = mixed_goals(goals)
        seeds = (np.arange(len(run_goals), dtype=np.uint32) * 31 + 7) if case == "wam-momentum-hmc" else None
        bid = create(run_goals, SETS[0], seeds)
        mod.batch_set_run_params(bid, **table(set_of_run))
        mixed = results(mod, bid, n_iter)
        mod.batch_destroy(bid)
        sep = []
        for s in range(NS):
            bid = create(goals, SETS[s], None if seeds is None else seeds[s::NS])
            sep.append(results(mod, bid, n_iter))
            mod.batch_destroy(bid)
            assert_same(rows(mixed, np.arange(len(goals)) * NS + s), sep[s], (case, s))
        # the sets are told apart (a table that is ignored gives four equal trajectories per goal)
        for a in range(NS):
            for b in range(a + 1, NS):
                assert any(not np.array_equal(sep[a]["traj"][g], sep[b]["traj"][g], equal_nan=True) for g in range(len(goals))), (case, a, b)
        assert np.isfinite(mixed["traj"]).all(), case
    finally:
        mod.close()


# ---- 2. against the oracle -----------------------------------------------------------------------------------------

def test_the_mixed_batch_matches_the_oracle(wam, oracle):
    """WAM fp64, 100 points, 60 iterations: the runs of every set against oracle.batch_run with that set's parameters, by the
    rules of test_gpu_scenes.check_against_oracle; at least 24 of the 32 runs well-conditioned and within 1e-6"""
    from test_gpu_scenes import check_against_oracle
    mod, model = wam
    n_iter = 60
    run_goals, set_of_run = mixed_goals(GOALS)
    bid = mod.batch_create(model.name, run_goals, n_points=100, **SETS[0])
    mod.batch_set_run_params(bid, **table(set_of_run))
    got = results(mod, bid, n_iter)
    mod.batch_destroy(bid)
    data, lengths, gpose = mod.get_sdf("table")
    grid = oracle.OraGrid(data, lengths)
    pose = np.zeros(7)
    oracle.lib().ora_kin_pose_compose(oracle.dp(oracle.f64(mod.body_transform("table"))), oracle.dp(oracle.f64(gpose)), oracle.dp(pose))
    _, base, dofvals, adofs = common.wam_state()
    rob = oracle.OraRobot(model)
    n_well, traced = 0, []
    for s in range(NS):
        params = lambda: oracle.default_params(n_points=100, **SETS[s])
        ora = lambda g: oracle.batch_run(rob, base, dofvals, adofs, g, [grid], [pose], params(), n_iter)
        idx = np.arange(len(GOALS)) * NS + s
        nw, res, well = check_against_oracle(oracle, got, idx, ora, GOALS)
        print("set %d: %d of %d runs well-conditioned and within 1e-6; oracle status %s" % (s, nw, len(GOALS), res[2].tolist()))
        n_well += nw
        # the per-iteration trace of three well-conditioned runs, of three different sets
        if s > 0 and len(traced) < 3 and well.any():
            j = int(np.flatnonzero(well)[min(s, well.sum() - 1)])
            run = oracle.OraRun(rob, base, dofvals, adofs, GOALS[j], [grid], [pose], params())
            st, _, otr = run.iterate(n_iter, trace=True)
            run.destroy()
            assert st == 0
            assert np.allclose(got["trace"][idx[j]], otr, rtol=1e-6, atol=0), (s, j)
            traced.append((s, j))
    assert len(traced) == 3, traced
    assert n_well >= 24, n_well


# ---- 3. off is off -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [64, 32])
def test_off_is_off(wam, precision):
    """a table of the create values, and an all-None call after a real table, both give the untouched batch; the plan stays"""
    mod, model = wam
    run_goals, set_of_run = mixed_goals(GOALS[:4])
    kw = dict(n_points=100, precision=precision, **SETS[2])
    bid = mod.batch_create(model.name, run_goals, **kw)
    plan = mod.batch_plan(bid)
    plain = results(mod, bid, 20)
    mod.batch_destroy(bid)

    bid = mod.batch_create(model.name, run_goals, **kw)
    mod.batch_set_run_params(bid, **{k: np.full(len(run_goals), v) for k, v in SETS[2].items()})
    assert mod.batch_plan(bid) == plan
    assert_same(results(mod, bid, 20), plain, "a table of the shared values")
    mod.batch_destroy(bid)

    bid = mod.batch_create(model.name, run_goals, **kw)
    mod.batch_set_run_params(bid, **table(set_of_run))
    assert not np.array_equal(mod.batch_state(bid, "run_params"), run_params_table(SETS[2], len(run_goals), precision))
    mod.batch_set_run_params(bid)
    assert mod.batch_plan(bid) == plan
    assert np.array_equal(mod.batch_state(bid, "run_params"), run_params_table(SETS[2], len(run_goals), precision))
    assert_same(results(mod, bid, 20), plain, "switched off again")
    mod.batch_destroy(bid)


# ---- 4. between calls, and ordering ---------------------------------------------------------------------------------

def test_between_calls_and_ordering(wam):
    """iterate 10 with P0, set P2 for all runs, iterate 10: a P0 batch's trajectories after 10 handed to a P2 batch, iterated 10
    (plain runs: the trajectory is the whole state).  The same with iterate_async: a call enqueued before the set keeps P0"""
    mod, model = wam
    goals = GOALS
    a = mod.batch_create(model.name, goals, n_points=100, **SETS[0])
    mod.batch_iterate(a, 10)
    b = mod.batch_create(model.name, goals, n_points=100, **SETS[2])
    mod.batch_set_traj(b, mod.batch_gettraj(a))
    want = results(mod, b, 10)
    mod.batch_destroy(a); mod.batch_destroy(b)
    p2 = {k: np.full(len(goals), v) for k, v in SETS[2].items()}

    bid = mod.batch_create(model.name, goals, n_points=100, **SETS[0])
    mod.batch_iterate(bid, 10)
    mod.batch_set_run_params(bid, **p2)
    got = results(mod, bid, 10)
    mod.batch_destroy(bid)
    assert_same(got, want, "iterate, set, iterate")

    bid = mod.batch_create(model.name, goals, n_points=100, **SETS[0])
    mod.batch_iterate_async(bid, 10)
    mod.batch_set_run_params(bid, **p2)
    mod.batch_iterate_async(bid, 10)
    costs, status = mod.batch_sync(bid)
    got = dict(costs=costs, status=status, traj=mod.batch_gettraj(bid), iters=mod.batch_iterations_done(bid),
               trace=mod.batch_trace(bid, 10), AG=mod.batch_state(bid, "AG"))
    mod.batch_destroy(bid)
    assert_same(got, want, "iterate_async, set, iterate_async, sync")
    # P0 for all twenty iterations is another result: the second call did read the table
    bid = mod.batch_create(model.name, goals, n_points=100, **SETS[0])
    mod.batch_iterate(bid, 10)
    other = results(mod, bid, 10)
    mod.batch_destroy(bid)
    assert not np.array_equal(other["traj"], want["traj"], equal_nan=True)


# ---- 5. shards -----------------------------------------------------------------------------------------------------

def test_shards(wam):
    """Module([0, 0]) with a 10-run mixed batch (an uneven cut of the table) equals the single-device batch bit for bit, and so
    does the selection by the smoothness cost over groups that span the cut"""
    mod, model = wam
    run_goals, set_of_run = mixed_goals(GOALS)
    run_goals, set_of_run = run_goals[:10], set_of_run[:10]
    groups = np.arange(10) % 3                                   # every group has runs on both sides of the cut
    out = []
    mod2 = or_cdchomp_amd.Module([0, 0])
    try:
        model2 = common.setup_product_wam(mod2)
        for m, name in ((mod, model.name), (mod2, model2.name)):
            bid = m.batch_create(name, run_goals, n_points=100, **SETS[0])
            m.batch_set_run_params(bid, **table(set_of_run))
            res = results(m, bid, 20)
            res["rp"] = m.batch_state(bid, "run_params")
            res["sel"] = [m.batch_select_best(bid, groups=groups, collision_free=cf, by=by) for cf in (False, True) for by in ("smooth", "obs")]
            m.batch_destroy(bid)
            out.append(res)
    finally:
        mod2.close()
    assert_same(out[0], out[1], "two shards")
    assert np.array_equal(out[0]["rp"], out[1]["rp"])
    assert np.array_equal(out[0]["rp"], run_params_table(SETS[0], 10, 64, **table(set_of_run)))
    for a, b in zip(out[0]["sel"], out[1]["sel"]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    assert (out[0]["sel"][0][0] >= 0).all()


# ---- 6. selection by column ----------------------------------------------------------------------------------------

def test_selection_by_column(wam):
    """groups are the goals, four runs each (group 0: four times the same run, a tie in every column); a ninth group is empty.
    by = smooth / obs / total against the pure select_best(..., column=) on the read-back costs"""
    mod, model = wam
    run_goals, set_of_run = mixed_goals(GOALS)
    set_of_run = set_of_run.copy()
    set_of_run[:NS] = 1
    groups = np.arange(len(run_goals)) // NS
    n_groups = len(GOALS) + 1
    bid = mod.batch_create(model.name, run_goals, n_points=100, **SETS[0])
    mod.batch_set_run_params(bid, **table(set_of_run))
    costs, status = mod.batch_iterate(bid, 30)
    collides = mod.batch_collision_verdict(bid, on_device=True)["collides"]
    winners = {}
    for cf in (False, True):
        for column, by in enumerate(("total", "obs", "smooth")):
            got = mod.batch_select_best(bid, groups=groups, n_groups=n_groups, collision_free=cf, by=by)
            want = select_best(costs, status, collides if cf else None, groups, n_groups, column=column)
            for x, y in zip(got, want):
                assert np.array_equal(x, y), (cf, by, x, y)
            assert got[0][-1] == -1 and got[1][-1] == INF and got[2][-1] == 0
            winners[cf, by] = got[0]
        # by="total" is orc_batch_select_best itself
        for x, y in zip(mod.batch_select_best(bid, groups=groups, n_groups=n_groups, collision_free=cf),
                        mod.batch_select_best(bid, groups=groups, n_groups=n_groups, collision_free=cf, by="total")):
            assert np.array_equal(x, y)
    mod.batch_destroy(bid)
    assert status[0] in (0, 1) and np.array_equal(costs[0], costs[1]) and np.array_equal(costs[0], costs[3])
    for by in ("total", "obs", "smooth"):
        assert winners[False, by][0] == 0                         # the tie goes to the lowest index
    assert any(not np.array_equal(winners[False, "total"], winners[False, by]) for by in ("obs", "smooth")), "the column must matter"


# ---- 7. read-back and rejections -----------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [64, 32])
def test_read_back_and_rejections(wam, precision):
    mod, model = wam
    run_goals, set_of_run = mixed_goals(GOALS[:4])
    n_runs = len(run_goals)
    kw = dict(n_points=100, precision=precision)
    bid = mod.batch_create(model.name, run_goals, **dict(kw, **SETS[0]))
    assert np.array_equal(mod.batch_state(bid, "run_params"), run_params_table(SETS[0], n_runs, precision))
    tab = table(set_of_run)
    mod.batch_set_run_params(bid, **tab)
    want = run_params_table(SETS[0], n_runs, precision, **tab)
    assert np.array_equal(mod.batch_state(bid, "run_params"), want)
    # a scalar goes to every run, None is the shared value; the call replaces the table, it does not merge
    mod.batch_set_run_params(bid, epsilon=0.07, obs_factor_self=tab["obs_factor_self"])
    assert np.array_equal(mod.batch_state(bid, "run_params"),
                          run_params_table(SETS[0], n_runs, precision, epsilon=0.07, obs_factor_self=tab["obs_factor_self"]))
    mod.batch_set_run_params(bid, **tab)
    mod.batch_iterate(bid, 5)

    def bad(k, v):
        arr = tab[k].copy()
        arr[n_runs // 2] = v
        return dict(tab, **{k: arr})
    rejected = [bad("lambda_", NAN), bad("obs_factor", NAN), bad("epsilon", INF), bad("obs_factor_self", -INF),
                bad("lambda_", 0.0), bad("epsilon", -1.0)]
    for args in rejected:
        with pytest.raises(RuntimeError) as e:
            mod.batch_set_run_params(bid, **args)
        assert str(e.value), "a message"
        with pytest.raises(ValueError):
            run_params_table(SETS[0], n_runs, precision, **args)
        assert np.array_equal(mod.batch_state(bid, "run_params"), want)
    lib, h = mod._lib, mod._h
    assert lib.orc_batch_set_run_params(h, 987654, None, None, None, None) != 0 and lib.orc_last_error(h)
    groups = np.arange(n_runs, dtype=np.int32) // NS
    best = np.full(4, 77, dtype=np.int32)
    from or_cdchomp_amd._capi import c_int_p
    for column in (3, -1):
        assert lib.orc_batch_select_best_by(h, bid, column, 4, groups.ctypes.data_as(c_int_p), 0, best.ctypes.data_as(c_int_p), None, None) != 0
        assert b"cost_column" in lib.orc_last_error(h) and (best == 77).all()
    assert lib.orc_batch_select_best_by(h, 987654, 2, 4, groups.ctypes.data_as(c_int_p), 0, None, None, None) != 0
    assert np.array_equal(mod.batch_state(bid, "run_params"), want)
    # one more iterate call still runs with the table that was kept
    got = results(mod, bid, 5)
    mod.batch_destroy(bid)
    ref = mod.batch_create(model.name, run_goals, **dict(kw, **SETS[0]))
    mod.batch_set_run_params(ref, **tab)
    mod.batch_iterate(ref, 5)
    assert_same(got, results(mod, ref, 5), "after the rejected calls")
    mod.batch_destroy(ref)
