"""-m gpu: the device-planned collision verdict asked about a subset of the runs (orc_batch_collision_verdict_subset,
Module.batch_collision_verdict(on_device=True, runs=...)) and the scope of the verdict inside the selection calls
(orc_batch_set_verdict_scope).  The yardstick is the all-runs verdict of the same batch, orc_batch_collision_verdict_device,
which tests/test_gpu_verdict_device.py holds to the host-planned one: an examined run must report its bits, every other run
what or_cdchomp_amd.module.verdict_subset says, and the selection calls must not notice the scope."""
import numpy as np
import pytest

import common
import or_cdchomp_amd
from or_cdchomp_amd import _capi, robots
from or_cdchomp_amd.module import candidates, contiguous_groups, respawn_plan, select_best, verdict_subset
from test_gpu_verdict_device import KW, check_workload, same, set_wam_vmax, wam_goals_with_table

pytestmark = pytest.mark.gpu

KW40 = dict(KW, n_points=40)
KEYS = ("collides", "time", "sphere", "field", "depth", "n_samples")
TOO_LONG = "trajectory too long for the batched collision verdict!"


def assert_verdicts_equal(got, want, what=""):
    assert sorted(got) == sorted(want) == sorted(KEYS), (what, sorted(got), sorted(want))
    for key in KEYS:
        assert got[key].dtype == want[key].dtype, (what, key)
        if got[key].dtype == np.float64:
            assert same(got[key], want[key]), (what, key, np.flatnonzero(got[key] != want[key]), got[key], want[key])
        else:
            assert np.array_equal(got[key], want[key]), (what, key, np.flatnonzero(got[key] != want[key]), got[key], want[key])


def masks_of(n_runs):
    half = np.zeros(n_runs, dtype=bool); half[n_runs // 2:] = True
    only0 = np.zeros(n_runs, dtype=bool); only0[0] = True
    last = np.zeros(n_runs, dtype=bool); last[-1] = True
    return {"all ones": np.ones(n_runs, dtype=bool), "all zeros": np.zeros(n_runs, dtype=bool),
            "alternating": np.arange(n_runs) % 2 == 0, "only run 0": only0, "only the last run": last,
            "random": np.random.default_rng(20251018).random(n_runs) < 0.5,
            "the second half": half}      # (two shards: the first has no run to examine; "only run 0": the second has none)


def check_masks(mod, bid, full):
    """every mask's subset verdict is verdict_subset of the all-runs verdict, bit for bit"""
    n_runs = len(full["collides"])
    for name, mask in masks_of(n_runs).items():
        got = mod.batch_collision_verdict(bid, on_device=True, runs=mask)
        assert_verdicts_equal(got, verdict_subset(full, mask), name)
        assert np.array_equal(got["collides"] == -1, ~mask), name
    # 0-1 integers are a mask too
    ints = masks_of(n_runs)["random"].astype(np.int64)
    assert_verdicts_equal(mod.batch_collision_verdict(bid, on_device=True, runs=ints), verdict_subset(full, ints), "ints")
    # and the all-runs call still gives what it gave: the subset calls left nothing behind
    assert_verdicts_equal(mod.batch_collision_verdict(bid, on_device=True), full, "again")


# ---- 1. a mask's verdict is the full verdict of its runs ----------------------------------------------------------------

@pytest.mark.parametrize("precision", [64, 32])
def test_mask_equals_the_full_verdict(precision):
    """the WAM at the tabletop after 10 iterations, one run replaced by a trajectory whose contact lies beyond the first
    chunk of samples (check_workload asserts both outcomes and that late contact)"""
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    vmax = set_wam_vmax(mod, model)
    goals = wam_goals_with_table(32, seed=79)
    bid = mod.batch_create(model.name, goals, **dict(KW40, precision=precision))
    host, full, traj = check_workload(mod, bid, vmax, 0, 10)
    check_masks(mod, bid, full)
    mod.batch_destroy(bid)
    mod.close()


def test_mask_tree_robot():
    """the TREE instantiation: the 30-dof tree among config 5's bodies (tests/test_gpu_verdict_device.py test_tree_robot)"""
    mod = or_cdchomp_amd.Module(0)
    model = robots.tree30()
    mod.add_robot(model, transform=[0.0] * 6 + [1.0], dof_values=np.zeros(model.n_dof), active_dofs=list(range(model.n_dof)))
    for name, (boxes, pose) in common.config5_bodies().items():
        if name != "box2":
            mod.add_kinbody_boxes(name, boxes, transform=pose)
            mod.SendCommand("computedistancefield kinbody %s cube_extent %f aabb_padding %f" % (name, common.CONFIG5_CUBE, common.CONFIG5_PADDING))
    vmax = np.linspace(0.5, 2.0, model.n_dof)
    mod.set_velocity_limits(model.name, vmax)
    bid = mod.batch_create(model.name, common.config5_goals(48), **dict(common.CONFIG5_KW, n_points=60))
    assert mod.batch_plan(bid)["variant"] & 1, "the robot must be a tree"
    host, full, traj = check_workload(mod, bid, vmax, 0, 5)
    check_masks(mod, bid, full)
    mod.batch_destroy(bid)
    mod.close()


def test_mask_scene_batch():
    """per-run scenes, the empty scene among them: a skipped run's workgroup returns before it looks its scene up"""
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    mod.SendCommand("computedistancefield kinbody mug")
    vmax = set_wam_vmax(mod, model)
    shift = np.array([0.03, -0.04, 0.02, 0.0, 0.0, 0.0, 1.0])
    scenes = [[("table", None), ("mug", None)], [("table", shift), ("mug", shift)], [("mug", None), ("table", None)], []]
    n_runs = 32
    goals = wam_goals_with_table(n_runs, seed=78, k_table=8)
    scene_of_run = (np.arange(n_runs) % len(scenes)).astype(np.int32)
    bid = mod.batch_create(model.name, goals, scenes=scenes, scene_of_run=scene_of_run, **KW40)
    host, full, traj = check_workload(mod, bid, vmax, 0, 10, pick=n_runs - 4)
    assert (scene_of_run == 3).any()
    check_masks(mod, bid, full)
    mod.batch_destroy(bid)
    mod.close()


@pytest.fixture(scope="module")
def wam():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    vmax = set_wam_vmax(mod, model)
    yield mod, model, vmax
    mod.close()


@pytest.fixture(scope="module")
def wam2():
    """the same scene on a module of two in-process shards on one card"""
    mod = or_cdchomp_amd.Module([0, 0])
    model = common.setup_product_wam(mod)
    vmax = set_wam_vmax(mod, model)
    yield mod, model, vmax
    mod.close()


def test_mask_two_shards(wam2):
    """every shard takes its slice of the mask; "the second half" and "only run 0" leave one shard with nothing to examine"""
    mod, model, vmax = wam2
    goals = wam_goals_with_table(32, seed=79)
    bid = mod.batch_create(model.name, goals, **KW40)
    host, full, traj = check_workload(mod, bid, vmax, 0, 10)
    check_masks(mod, bid, full)
    mod.batch_destroy(bid)


# ---- 2. without the count ---------------------------------------------------------------------------------------------

def raw_subset(mod, bid, which, examine, n_runs, count=True, collides=True):
    """the C call itself; returns (rc, dict)"""
    col = np.full(n_runs, 77, dtype=np.int32); sph = np.full(n_runs, 77, dtype=np.int32); fld = np.full(n_runs, 77, dtype=np.int32)
    tim = np.full(n_runs, 77.0); dep = np.full(n_runs, 77.0); cnt = np.full(n_runs, 77, dtype=np.int32)
    ip, dp = _capi.c_int_p, _capi.c_double_p
    ex = None if examine is None else np.ascontiguousarray(examine, dtype=np.uint8)
    rc = mod._lib.orc_batch_collision_verdict_subset(
        mod._h, bid, which, None if ex is None else ex.ctypes.data_as(_capi.c_ubyte_p),
        col.ctypes.data_as(ip) if collides else None, tim.ctypes.data_as(dp), sph.ctypes.data_as(ip), fld.ctypes.data_as(ip),
        dep.ctypes.data_as(dp), cnt.ctypes.data_as(ip) if count else None)
    return rc, dict(collides=col, time=tim, sphere=sph, field=fld, depth=dep, n_samples=cnt)


def test_without_the_count(wam):
    """n_samples_out == NULL: the samples behind a contact are not counted, and nothing else changes"""
    mod, model, vmax = wam
    n_runs = 24
    bid = mod.batch_create(model.name, wam_goals_with_table(n_runs, seed=84), **KW40)
    mod.batch_iterate(bid, 10)
    full = mod.batch_collision_verdict(bid, on_device=True)
    hit = full["collides"] == 1
    assert hit.any() and not hit.all()
    # the count is only work where samples lie behind a contact
    assert (full["n_samples"][hit] > 1).any()
    for name, mask in masks_of(n_runs).items():
        rc, counted = raw_subset(mod, bid, 0, mask, n_runs, count=True)
        assert rc == 0
        assert_verdicts_equal(counted, verdict_subset(full, mask), name)
        rc, plain = raw_subset(mod, bid, 0, mask, n_runs, count=False)
        assert rc == 0
        assert (plain["n_samples"] == 77).all(), "a NULL output is not written"
        assert_verdicts_equal(dict(plain, n_samples=counted["n_samples"]), counted, name)
        # the same through Module.batch_collision_verdict(count=False): no n_samples in the dict, the rest bit for bit
        py = mod.batch_collision_verdict(bid, on_device=True, runs=mask, count=False)
        assert "n_samples" not in py
        assert_verdicts_equal(dict(py, n_samples=counted["n_samples"]), counted, name)
    with pytest.raises(ValueError):
        mod.batch_collision_verdict(bid, on_device=True, count=False)      # (the all-runs verdict always counts)
    mod.batch_destroy(bid)


# ---- 3 .. 5. the candidates ---------------------------------------------------------------------------------------------
# Config 2's keywords (lambda 100, obs_factor 500) at n_points 40 on 32 runs in 4 groups of 8, every fourth run (1, 5, 9, ...)
# at lambda 50 through batch_set_run_params, 100 iterations.  The goals' seed and the lambda were picked with the oracle on
# the CPU (oracle_py.batch_run of these goals at lambda 100 and at lambda 50, n_points 40): at lambda 50 a run takes steps
# twice as long, and runs 1, 5, 13, 17, 25 and 29 leave their joint limits (status -1); at lambda 100 only runs 9 and 13 do,
# which are at lambda 50 here.  The last four goals lie in the table top: runs 28, 30 and 31 stay inside their limits at
# lambda 100 and end in a contact, the colliding candidates.  The tests assert what they need of this on the statuses and
# the verdict the device returns.
P_RUNS, P_GROUPS = 32, 4
P_SEED = 90
P_LAMBDA = np.where(np.arange(P_RUNS) % 4 == 1, 50.0, 100.0)


def portfolio(mod, model):
    """a fresh batch in that state (the same bits every time); returns (bid, costs, status)"""
    goals = wam_goals_with_table(P_RUNS, seed=P_SEED)
    bid = mod.batch_create(model.name, goals, **KW40)
    mod.batch_set_run_params(bid, lambda_=P_LAMBDA)
    costs, status = mod.batch_iterate(bid, 100)
    return bid, costs, status


def portfolio_premise(costs, status, full):
    cand = candidates(costs, status)
    assert (status == -1).any(), "a run must have left its limits"
    assert (status == 0).any(), "a run must have stayed inside"
    assert (cand & (full["collides"] == 1)).any(), "a candidate must collide"
    assert (cand & (full["collides"] == 0)).any(), "a candidate must be free"
    return cand


def test_candidates(wam):
    mod, model, vmax = wam
    bid, costs, status = portfolio(mod, model)
    full = mod.batch_collision_verdict(bid, on_device=True)
    cand = portfolio_premise(costs, status, full)
    print("status -1: %d, candidates: %d, colliding candidates: %d; n_samples of status -1 runs up to %d, of candidates up to %d"
          % ((status == -1).sum(), cand.sum(), (cand & (full["collides"] == 1)).sum(), full["n_samples"][status == -1].max(),
             full["n_samples"][cand].max()))
    got = mod.batch_collision_verdict(bid, on_device=True, runs="candidates")
    assert_verdicts_equal(got, verdict_subset(full, cand), "candidates")
    # the skip set is exactly the non-candidates
    assert np.array_equal(got["collides"] == -1, ~cand) and np.array_equal(got["n_samples"] == -1, ~cand)
    assert (got["collides"][status == -1] == -1).all()
    # a mask the caller computed gives the same
    assert_verdicts_equal(mod.batch_collision_verdict(bid, on_device=True, runs=cand), got, "the caller's mask")
    mod.batch_destroy(bid)


def test_a_too_long_run_no_longer_sinks_the_batch(wam):
    mod, model, vmax = wam
    bid, costs, status = portfolio(mod, model)
    full = mod.batch_collision_verdict(bid, on_device=True)
    cand = portfolio_premise(costs, status, full)
    groups = contiguous_groups(P_RUNS, P_GROUPS)
    before = {by: mod.batch_select_best(bid, n_groups=P_GROUPS, collision_free=True, by=by) for by in ("total", "smooth")}
    for by, column in (("total", 0), ("smooth", 2)):
        want = select_best(costs, status, full["collides"], groups, P_GROUPS, column=column)
        assert np.array_equal(before[by][0], want[0]) and same(before[by][1], want[1]) and np.array_equal(before[by][2], want[2])
    assert (before["total"][0] >= 0).any()
    # one run that left its limits gets a middle waypoint 1e9 rad out: 2e9 / 0.04 samples, decided before anything is walked
    victim = int(np.flatnonzero(status == -1)[0])
    traj = mod.batch_gettraj(bid)
    traj[victim, traj.shape[1] // 2, 0] = 1e9
    mod.batch_set_traj(bid, traj)
    costs2, status2 = mod.batch_sync(bid)
    assert np.array_equal(status2, status) and same(costs2, costs), "set_traj leaves costs and status alone"
    # premises: today's calls fail
    with pytest.raises(RuntimeError, match="trajectory too long"):
        mod.batch_collision_verdict(bid, on_device=True)
    assert mod._lib.orc_last_error(mod._h).decode() == TOO_LONG
    for by in ("total", "smooth"):
        with pytest.raises(RuntimeError, match="trajectory too long"):
            mod.batch_select_best(bid, n_groups=P_GROUPS, collision_free=True, by=by)
    # asked about every run by mask, the call succeeds and only that run says so
    ones = np.ones(P_RUNS, dtype=bool)
    got = mod.batch_collision_verdict(bid, on_device=True, runs=ones)
    want = verdict_subset(full, ones)
    want["collides"][victim] = -2; want["n_samples"][victim] = -2
    want["time"][victim] = -1.0; want["sphere"][victim] = -1; want["field"][victim] = -1; want["depth"][victim] = 0.0
    assert_verdicts_equal(got, want, "every run, one of them too long")
    rc, plain = raw_subset(mod, bid, 0, ones, P_RUNS, count=False)
    assert rc == 0
    assert_verdicts_equal(dict(plain, n_samples=want["n_samples"]), want, "... without the count")
    # it is no candidate: the candidates' verdict is what it was
    assert_verdicts_equal(mod.batch_collision_verdict(bid, on_device=True, runs="candidates"), verdict_subset(full, cand), "candidates")
    # the selection under scope "candidates" returns what it returned before the replacement
    mod.batch_set_verdict_scope(bid, "candidates")
    for by in ("total", "smooth"):
        got = mod.batch_select_best(bid, n_groups=P_GROUPS, collision_free=True, by=by)
        assert np.array_equal(got[0], before[by][0]) and same(got[1], before[by][1]) and np.array_equal(got[2], before[by][2]), by
    # a rejected setting changes nothing
    assert mod._lib.orc_batch_set_verdict_scope(mod._h, bid, 2) != 0
    got = mod.batch_select_best(bid, n_groups=P_GROUPS, collision_free=True)
    assert np.array_equal(got[0], before["total"][0])
    # back under "all" the call fails again: the setting is a setting
    mod.batch_set_verdict_scope(bid, "all")
    with pytest.raises(RuntimeError, match="trajectory too long"):
        mod.batch_select_best(bid, n_groups=P_GROUPS, collision_free=True)
    with pytest.raises(RuntimeError, match="trajectory too long"):
        mod.batch_respawn(bid, 2, 0.0, None, n_groups=P_GROUPS, collision="require")
    mod.batch_set_verdict_scope(bid, "candidates")
    src, cnt = mod.batch_respawn(bid, 2, 0.0, None, n_groups=P_GROUPS, collision="require")
    want = respawn_plan(costs, status, full["collides"], groups, P_GROUPS, 2, mode=1)
    assert np.array_equal(src, want[0]) and np.array_equal(cnt, want[1])
    assert src[victim] != victim
    mod.batch_destroy(bid)


def test_a_too_long_candidate_still_fails_the_selection(wam):
    """scope "candidates" fails with today's message when a CANDIDATE is too long; the subset call marks that run alone"""
    mod, model, vmax = wam
    bid, costs, status = portfolio(mod, model)
    full = mod.batch_collision_verdict(bid, on_device=True)
    cand = portfolio_premise(costs, status, full)
    victim = int(np.flatnonzero(cand)[0])
    traj = mod.batch_gettraj(bid)
    traj[victim, traj.shape[1] // 2, 0] = 1e9
    mod.batch_set_traj(bid, traj)
    mod.batch_set_verdict_scope(bid, "candidates")
    with pytest.raises(RuntimeError, match="trajectory too long"):
        mod.batch_select_best(bid, n_groups=P_GROUPS, collision_free=True)
    got = mod.batch_collision_verdict(bid, on_device=True, runs="candidates")
    want = verdict_subset(full, cand)
    want["collides"][victim] = -2; want["n_samples"][victim] = -2
    want["time"][victim] = -1.0; want["sphere"][victim] = -1; want["field"][victim] = -1; want["depth"][victim] = 0.0
    assert_verdicts_equal(got, want, "a candidate that is too long")
    mod.batch_destroy(bid)


@pytest.mark.parametrize("shards", [1, 2])
def test_scope_changes_nothing_else(wam, wam2, shards):
    mod, model, vmax = wam if shards == 1 else wam2
    bid, costs, status = portfolio(mod, model)
    full = mod.batch_collision_verdict(bid, on_device=True)
    portfolio_premise(costs, status, full)
    contiguous = contiguous_groups(P_RUNS, P_GROUPS)
    shuffled = np.random.default_rng(6).permutation(contiguous).astype(np.int32)      # (groups that span the shards)
    for grp in (contiguous, shuffled, None):
        for by, column in (("total", 0), ("smooth", 2)):
            res = {}
            for scope in ("all", "candidates"):
                mod.batch_set_verdict_scope(bid, scope)
                res[scope] = mod.batch_select_best(bid, groups=grp, n_groups=P_GROUPS, collision_free=True, by=by)
            a, c = res["all"], res["candidates"]
            assert np.array_equal(a[0], c[0]) and same(a[1], c[1]) and np.array_equal(a[2], c[2]), (grp, by)
            want = select_best(costs, status, full["collides"], contiguous if grp is None else grp, P_GROUPS, column=column)
            assert np.array_equal(c[0], want[0]) and same(c[1], want[1]) and np.array_equal(c[2], want[2]), (grp, by)
    mod.batch_destroy(bid)
    # both respawn modes, each on a fresh batch of the same bits
    for collision, mode in (("require", 1), ("prefer", 2)):
        plans = {}
        for scope in ("all", "candidates"):
            bid, c2, s2 = portfolio(mod, model)
            assert same(c2, costs) and np.array_equal(s2, status), "the batch must be reproducible"
            mod.batch_set_verdict_scope(bid, scope)
            plans[scope] = mod.batch_respawn(bid, 2, 0.0, None, n_groups=P_GROUPS, collision=collision)
            after = mod.batch_gettraj(bid)
            plans[scope] = plans[scope] + (after,)
            mod.batch_destroy(bid)
        a, c = plans["all"], plans["candidates"]
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and same(a[2], c[2]), collision
        want = respawn_plan(costs, status, full["collides"], contiguous, P_GROUPS, 2, mode=mode)
        assert np.array_equal(c[0], want[0]) and np.array_equal(c[1], want[1]), collision


# ---- 6. rejections --------------------------------------------------------------------------------------------------------

def test_rejected_calls(wam):
    mod, model, vmax = wam
    lib, h = mod._lib, mod._h
    n_runs = 6
    bid = mod.batch_create(model.name, wam_goals_with_table(n_runs, seed=85, k_table=2), **KW40)
    ones = np.ones(n_runs, dtype=np.uint8)

    def rejected(rc_out, text=None):
        rc, out = rc_out
        assert rc != 0
        msg = lib.orc_last_error(h).decode()
        assert msg and (text is None or text in msg), msg
        assert all((out[k] == 77).all() for k in out), "a rejected call writes nothing"

    rejected(raw_subset(mod, bid, 2, ones, n_runs), "which")
    rejected(raw_subset(mod, bid, -1, ones, n_runs), "which")
    rejected(raw_subset(mod, bid, 0, None, n_runs), "examine")
    rejected(raw_subset(mod, bid, 1, ones, n_runs), "examine")
    rejected(raw_subset(mod, bid, 0, ones, n_runs, collides=False), "collides_out")
    rejected(raw_subset(mod, bid + 1000, 0, ones, n_runs))
    # the candidates of a batch that has not been iterated: select_best's message
    rejected(raw_subset(mod, bid, 1, None, n_runs), "select_best: the batch has not been iterated")
    with pytest.raises(RuntimeError, match="has not been iterated"):
        mod.batch_collision_verdict(bid, on_device=True, runs="candidates")
    assert lib.orc_batch_select_best(h, bid, 1, None, 0, None, None, None) != 0
    select_msg = lib.orc_last_error(h).decode()
    raw_subset(mod, bid, 1, None, n_runs)
    assert lib.orc_last_error(h).decode() == select_msg
    for scope in (2, -1):
        assert lib.orc_batch_set_verdict_scope(h, bid, scope) != 0
        assert "scope" in lib.orc_last_error(h).decode()
    assert lib.orc_batch_set_verdict_scope(h, bid + 1000, 1) != 0
    with pytest.raises(ValueError):
        mod.batch_set_verdict_scope(bid, "some")
    with pytest.raises(ValueError):
        mod.batch_collision_verdict(bid, on_device=True, runs="all")
    with pytest.raises(ValueError):
        mod.batch_collision_verdict(bid, on_device=True, runs=np.ones(n_runs + 1))
    with pytest.raises(ValueError):
        mod.batch_collision_verdict(bid, runs=np.ones(n_runs))      # (the host-planned verdict has no subset)
    # the module is usable: a mask needs no iterate call, the candidates need one (0 iterations are enough)
    full = mod.batch_collision_verdict(bid, on_device=True)
    rc, got = raw_subset(mod, bid, 0, ones, n_runs)
    assert rc == 0
    assert_verdicts_equal(got, full, "after the rejections")
    costs, status = mod.batch_iterate(bid, 0)
    assert_verdicts_equal(mod.batch_collision_verdict(bid, on_device=True, runs="candidates"),
                          verdict_subset(full, candidates(costs, status)), "candidates after iterate 0")
    for scope in (1, 0):
        assert lib.orc_batch_set_verdict_scope(h, bid, scope) == 0
    mod.batch_destroy(bid)
