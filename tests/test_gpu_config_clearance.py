"""-m gpu: the clearance of given configurations and of waypoints (orc_batch_config_clearance, orc_batch_waypoint_clearance;
Module.batch_config_clearance, Module.batch_waypoint_clearance).

The exact yardstick is orc_batch_clearance: a trajectory with exactly one sample (tests/config_clearance.py; the premise is
checked in tests/test_host_config_clearance.py) has the clearance of its first row, so the new calls must return that run's
clearance bits, sphere and other -- with no tolerance, in fp64 and in fp32.  Beside it: the restatement of tests/clearance.py,
and the independence of a query's answer from its place in the list, its chunk and its shard."""
import numpy as np
import pytest

import clearance as CL
import common
import config_clearance as CC
import or_cdchomp_amd
from or_cdchomp_amd import _capi, robots, scenes
from test_gpu_clearance import bits, product_field
from test_gpu_verdict_device import KW, same, set_wam_vmax, wam_goals_with_table

pytestmark = pytest.mark.gpu

OUT = ("clearance", "sphere", "other")
KW4 = dict(KW, n_points=4)
SHIFT = np.array([0.03, -0.04, 0.02, 0.0, 0.0, 0.0, 1.0])


def assert_same(got, want, what=""):
    """bit for bit, the three outputs of two results (dicts of arrays of one shape)"""
    for key in OUT:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        if key == "clearance":
            assert np.array_equal(bits(a), bits(b)), (what, key, a, b)
        else:
            assert a.dtype == np.int32 and np.array_equal(a, b), (what, key, a, b)


def pick(res, idx):
    return {key: np.asarray(res[key])[idx] for key in OUT}


def yardstick(mod, bid, configs, col0=0, what=""):
    """one run per configuration: the run's one-sample trajectory goes up, and batch_clearance of the batch is what both new
    calls must return.  Returns batch_clearance's result."""
    n_runs, n_points, _ = mod.batch_dims(bid)
    assert n_runs == len(configs)
    mod.batch_set_traj(bid, CC.one_sample_batch(configs, n_points, col0))
    ref = mod.batch_clearance(bid)
    assert (ref["n_samples"] == 1).all(), (what, ref["n_samples"])
    assert_same(mod.batch_config_clearance(bid, configs, runs=np.arange(n_runs)), ref, what + ": configurations")
    first = mod.batch_waypoint_clearance(bid, points=0)
    assert first["clearance"].shape == (n_runs, 1, 2)
    assert_same(pick(first, (slice(None), 0)), ref, what + ": waypoint 0")
    return ref


@pytest.fixture(scope="module")
def wam(oracle):
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    vmax = set_wam_vmax(mod, model)
    _, base, dofvals, adofs = common.wam_state()
    field = product_field(oracle, mod, "table")
    tab = CL.Tables(oracle, model, base, dofvals, adofs, [field])
    yield dict(mod=mod, model=model, vmax=vmax, field=field, tab=tab)
    mod.close()


@pytest.fixture(scope="module")
def wam2():
    """the same scene on a module of two in-process shards on one card"""
    mod = or_cdchomp_amd.Module([0, 0])
    model = common.setup_product_wam(mod)
    set_wam_vmax(mod, model)
    yield dict(mod=mod, model=model)
    mod.close()


# ---- 1. the WAM and the table ---------------------------------------------------------------------------------------------

def test_wam_and_table(wam):
    mod, model = wam["mod"], wam["model"]
    fixed = CC.wam_fixed()
    configs = np.array(list(fixed.values()))
    bid = mod.batch_create(model.name, common.wam_goals(len(configs), seed=1), **KW4)
    ref = yardstick(mod, bid, configs, what="wam")
    got = mod.batch_config_clearance(bid, configs, runs=np.arange(len(configs)))
    for k, name in enumerate(fixed):
        res = CL.restate(wam["tab"], CC.one_sample(configs[k])[:2], wam["vmax"], 0, [wam["field"]])
        assert res["n_samples"] == 1 and not CL.set_aside(res, [wam["field"]]), name
        print("%-14s %+.9f %+.9f  spheres %s others %s" % (name, got["clearance"][k, 0], got["clearance"][k, 1], got["sphere"][k], got["other"][k]))
        for leg, (gap, key) in enumerate(((res["fgap"], res["fkey"]), (res["pgap"], res["pkey"]))):
            if not len(gap):
                assert np.isposinf(got["clearance"][k, leg]) and got["sphere"][k, leg] == -1 and got["other"][k, leg] == -1, (name, leg)
                continue
            c = res["clearance"][leg]
            tol = 1e-12 + 1e-9 * abs(c)
            assert abs(got["clearance"][k, leg] - c) <= tol, (name, leg, got["clearance"][k, leg], c)
            near = np.flatnonzero(gap <= c + tol)
            assert any(key[i, 1] == got["sphere"][k, leg] and key[i, 2] == got["other"][k, leg] for i in near), (name, leg, got["sphere"][k], got["other"][k])
    names = list(fixed)
    assert ref["clearance"][names.index("in the table"), 0] < 0.0
    assert ref["clearance"][names.index("folded"), 1] < 0.0
    assert np.isposinf(ref["clearance"][names.index("away"), 0]) and ref["sphere"][names.index("away"), 0] == -1
    # one row, one int for all, None for run 0
    one = mod.batch_config_clearance(bid, configs[1])
    assert_same(one, pick(got, slice(1, 2)), "a single row, run 0")
    assert_same(mod.batch_config_clearance(bid, configs, runs=3), mod.batch_config_clearance(bid, configs, runs=np.full(len(configs), 3)), "one run for all")
    mod.batch_destroy(bid)


# ---- 2. chunk and wavefront edges, independence of position -------------------------------------------------------------------

def tree_module():
    mod = or_cdchomp_amd.Module(0)
    model = robots.tree30()
    mod.add_robot(model, transform=[0.0] * 6 + [1.0], dof_values=np.zeros(model.n_dof), active_dofs=list(range(model.n_dof)))
    names = []
    for name, (boxes, pose) in common.config5_bodies().items():
        if name != "box2":
            mod.add_kinbody_boxes(name, boxes, transform=pose)
            mod.SendCommand("computedistancefield kinbody %s cube_extent %f aabb_padding %f" % (name, common.CONFIG5_CUBE, common.CONFIG5_PADDING))
            names.append(name)
    vmax = np.linspace(0.5, 2.0, model.n_dof)
    mod.set_velocity_limits(model.name, vmax)
    return mod, model, names


def check_positions(mod, bid, pool, n_runs, chunk, what):
    alone = {key: [] for key in OUT}
    for c in range(len(pool)):
        for r in range(n_runs):
            res = mod.batch_config_clearance(bid, pool[c], runs=r)
            for key in OUT:
                alone[key].append(res[key][0])
    alone = {key: np.array(alone[key]).reshape(len(pool), n_runs, 2) for key in OUT}
    assert len(np.unique(bits(alone["clearance"]).reshape(-1, 2), axis=0)) > len(pool), "the answers must tell configurations and scenes apart"
    for length in CC.lengths(chunk):
        ci, ri = CC.draw(length, len(pool), n_runs, seed=length)
        got = mod.batch_config_clearance(bid, pool[ci], runs=ri)
        assert_same(got, pick(alone, (ci, ri)), "%s: %d queries" % (what, length))


def test_positions_wam(wam):
    mod, model = wam["mod"], wam["model"]
    bid = mod.batch_create(model.name, common.wam_goals(2, seed=2), scenes=[[("table", None)], [("table", SHIFT)]],
                           scene_of_run=np.array([0, 1], dtype=np.int32), **KW4)
    chunk = mod.batch_config_chunk(bid)
    assert chunk == 64
    check_positions(mod, bid, CC.wam_pool(), 2, chunk, "wam")
    mod.batch_destroy(bid)


def test_positions_tree():
    mod, model, names = tree_module()
    sc = [[(nm, None) for nm in names], [(names[0], SHIFT), (names[2], None)]]
    bid = mod.batch_create(model.name, common.config5_goals(2), scenes=sc, scene_of_run=np.array([0, 1], dtype=np.int32),
                           **dict(common.CONFIG5_KW, n_points=4))
    assert mod.batch_plan(bid)["variant"] & 1, "the robot must be a tree"
    chunk = mod.batch_config_chunk(bid)
    print("tree: chunk", chunk)
    assert 4 <= chunk <= 64 and chunk % 4 == 0
    check_positions(mod, bid, CC.tree_pool(), 2, chunk, "tree")
    mod.batch_destroy(bid)
    mod.close()


# ---- 3. the profile ---------------------------------------------------------------------------------------------------------------

def test_profile(wam):
    mod, model = wam["mod"], wam["model"]
    n_runs, n_points = 6, 12
    bid = mod.batch_create(model.name, wam_goals_with_table(n_runs, seed=91, k_table=2), **dict(KW, n_points=n_points))
    mod.batch_iterate(bid, 10)
    traj = mod.batch_gettraj(bid)
    prof = mod.batch_waypoint_clearance(bid)
    assert prof["clearance"].shape == (n_runs, n_points, 2) and prof["sphere"].shape == (n_runs, n_points, 2)
    cfg = mod.batch_config_clearance(bid, traj.reshape(-1, traj.shape[2]), runs=np.repeat(np.arange(n_runs), n_points))
    assert_same({key: cfg[key].reshape(n_runs, n_points, 2) for key in OUT}, prof, "profile against the rows of gettraj")
    ends = mod.batch_waypoint_clearance(bid, points=(0, -1))
    assert_same(ends, pick(prof, (slice(None), [0, n_points - 1])), "starts and goals")
    runs, points = np.array([5, 0, 3, 3]), np.array([11, 0, 4, 4])
    assert_same(mod.batch_waypoint_clearance(bid, runs=runs, points=points), pick(prof, (runs, points)), "named waypoints")
    full = mod.batch_clearance(bid)
    walked = np.flatnonzero(full["n_samples"] > 0)      # (no samples: a minimum over nothing)
    assert len(walked) >= n_runs - 1
    for r in walked:
        assert (full["clearance"][r] <= prof["clearance"][r, 0]).all(), (r, full["clearance"][r], prof["clearance"][r, 0])
    assert (prof["clearance"][:, :, 0] < 0).any() and (prof["clearance"][:, :, 0] > 0).any(), "both outcomes must occur"
    mod.batch_destroy(bid)


# ---- 4. variants ------------------------------------------------------------------------------------------------------------------

def test_floating_base():
    mod = or_cdchomp_amd.Module(0)
    model, base, dofvals, adofs = common.wam_state()
    base = np.asarray(base, dtype=np.float64)
    base[0] -= 0.2
    mod.add_robot(model, transform=list(base), dof_values=dofvals, active_dofs=adofs)
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    set_wam_vmax(mod, model)
    configs = CC.floating_configs(base)
    assert (np.abs(np.linalg.norm(configs[:, 3:7], axis=1) - 1.0) > 0.05).sum() >= 4, "the quaternions must not be of unit length"
    bid = mod.batch_create(model.name, common.wam_goals(len(configs), seed=3), basegoals=np.tile(base, (len(configs), 1)),
                           **dict(KW4, floating_base=1))
    assert mod.batch_dims(bid)[2] == 14
    ref = yardstick(mod, bid, configs, col0=7, what="floating base")
    assert np.isfinite(ref["clearance"][:, 1]).all() and len(np.unique(bits(ref["clearance"]), axis=0)) == len(configs)
    mod.batch_destroy(bid)
    mod.close()


def test_tree_robot():
    mod, model, names = tree_module()
    configs = CC.tree_pool()
    bid = mod.batch_create(model.name, common.config5_goals(len(configs)), **dict(common.CONFIG5_KW, n_points=4))
    assert mod.batch_plan(bid)["variant"] & 1, "the robot must be a tree"
    ref = yardstick(mod, bid, configs, what="tree")
    print("tree: fields at the minima", sorted(set(ref["other"][:, 0].tolist())), "clearances", ref["clearance"].min(axis=0))
    assert np.isfinite(ref["clearance"][:, 1]).all()
    mod.batch_destroy(bid)
    mod.close()


def test_held_body():
    mod = or_cdchomp_amd.Module(0)
    model, hand, pose = common.setup_product_wam_held4(mod)
    set_wam_vmax(mod, model)
    configs = CC.held_configs()
    bid = mod.batch_create(model.name, common.wam_goals(len(configs), seed=4), **KW4)
    ref = yardstick(mod, bid, configs, what="held body")
    print("held body: spheres at the minima", ref["sphere"].tolist())
    assert np.isin(ref["sphere"], [16, 17, 18, 19]).any(), "the held spheres must appear among the answers"
    mod.batch_destroy(bid)
    mod.close()


def test_self_check_off_and_on_again():
    mod = or_cdchomp_amd.Module(0)
    model, base, dofvals, adofs = common.wam_state()
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    mod.add_kinbody_boxes("far", [([0, 0, 0, 0, 0, 0, 1], [0.05, 0.05, 0.05])], transform=[5, 5, 5, 0, 0, 0, 1])
    mod.SendCommand("computedistancefield kinbody far")
    set_wam_vmax(mod, model)
    configs = CC.folding_configs()
    bid = mod.batch_create(model.name, configs, **dict(n_points=4, lambda_=100.0, obs_factor=0.0, obs_factor_self=0.0))
    on = yardstick(mod, bid, configs, what="self check on")
    assert (on["clearance"][:, 1] < 0).any() and (on["clearance"][:, 1] > 0).any() and np.isposinf(on["clearance"][:, 0]).all()
    mod.set_self_check(model.name, False)
    off = yardstick(mod, bid, configs, what="self check off")
    assert np.isposinf(off["clearance"]).all() and (off["sphere"] == -1).all() and (off["other"] == -1).all()
    mod.set_self_check(model.name, True)
    assert_same(yardstick(mod, bid, configs, what="self check on again"), on, "on again")
    mod.batch_destroy(bid)
    mod.close()


def test_precision_32(wam):
    mod, model = wam["mod"], wam["model"]
    configs = CC.wam_pool()
    bid = mod.batch_create(model.name, common.wam_goals(len(configs), seed=5), **dict(KW4, precision=32))
    ref = yardstick(mod, bid, configs, what="precision 32")
    traj = mod.batch_gettraj(bid)
    assert same(traj, traj.astype(np.float32)) and not same(traj[:, 0], configs), "a precision 32 batch holds floats"
    assert_same(mod.batch_config_clearance(bid, traj[:, 0], runs=np.arange(len(configs))), ref, "the narrowed rows")
    assert same(ref["clearance"], ref["clearance"].astype(np.float32)), "the minima are floats, widened"
    assert (ref["clearance"][:, 0] < 0).any()
    mod.batch_destroy(bid)


# ---- 5. per-run scenes ------------------------------------------------------------------------------------------------------------

def test_per_run_scenes():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    mod.SendCommand("computedistancefield kinbody mug")
    set_wam_vmax(mod, model)
    mod.add_kinbody_boxes("merged", [], transform=[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    mod.merge_fields("merged", [("table", None), ("mug", None)], 0.04)
    sc = [[("table", None), ("mug", None)], [("table", SHIFT), ("mug", SHIFT)], [("merged", None)], []]
    pool = CC.wam_pool()
    goals = common.wam_goals(4, seed=6)
    bid = mod.batch_create(model.name, goals, scenes=sc, scene_of_run=np.arange(4, dtype=np.int32), **KW4)
    got = mod.batch_config_clearance(bid, np.repeat(pool, 4, axis=0), runs=np.tile(np.arange(4), len(pool)))
    got = {key: got[key].reshape(len(pool), 4, 2) for key in OUT}
    assert np.isposinf(got["clearance"][:, 3, 0]).all() and (got["sphere"][:, 3, 0] == -1).all() and (got["other"][:, 3, 0] == -1).all()
    assert np.isfinite(got["clearance"][:, 3, 1]).all(), "the empty scene still has the robot itself"
    for s in range(3):
        single = mod.batch_create(model.name, goals[:1], scenes=[sc[s]], scene_of_run=np.zeros(1, dtype=np.int32), **KW4)
        assert_same(mod.batch_config_clearance(single, pool), pick(got, (slice(None), s)), "scene %d" % s)
        mod.batch_destroy(single)
    assert not np.array_equal(bits(got["clearance"][:, 0, 0]), bits(got["clearance"][:, 1, 0])), "the shifted scene must answer differently"
    mod.batch_destroy(bid)
    mod.close()


# ---- 6. two shards ----------------------------------------------------------------------------------------------------------------

def test_two_shards(wam, wam2):
    pool = CC.wam_pool()
    ci = np.arange(21) % len(pool)
    ri = np.array([0, 2, 1, 3] * 6)[:21]      # runs 0, 1: the first shard; 2, 3: the second
    wr, wp = np.array([0, 2, 1, 3, 3, 0]), np.array([0, 1, 2, 3, 0, 1])
    res = []
    for m_ in (wam, wam2):
        mod, model = m_["mod"], m_["model"]
        bid = mod.batch_create(model.name, common.wam_goals(4, seed=7), scenes=[[("table", None)], [("table", SHIFT)]],
                               scene_of_run=np.array([0, 1, 1, 0], dtype=np.int32), **KW4)
        mod.batch_set_traj(bid, CC.one_sample_batch(pool[:4]))
        res.append((mod.batch_config_clearance(bid, pool[ci], runs=ri), mod.batch_waypoint_clearance(bid, runs=wr, points=wp),
                    mod.batch_waypoint_clearance(bid), mod.batch_waypoint_clearance(bid, points=(0, -1))))
        mod.batch_destroy(bid)
    for one, two, what in zip(res[0], res[1], ("configurations", "named waypoints", "profile", "starts and goals")):
        assert_same(two, one, "two shards: " + what)


# ---- 7. no state ----------------------------------------------------------------------------------------------------------------

def test_the_calls_leave_no_state(wam):
    mod, model = wam["mod"], wam["model"]
    kw = dict(KW, n_points=16)
    goals = wam_goals_with_table(4, seed=92, k_table=1)
    asked, twin = mod.batch_create(model.name, goals, **kw), mod.batch_create(model.name, goals, **kw)
    for bid in (asked, twin):
        mod.batch_iterate(bid, 5)
    before = mod.batch_select_clear(asked, n_groups=2, margin=-np.inf, by="clearance")
    prof = mod.batch_waypoint_clearance(asked)
    mod.batch_config_clearance(asked, CC.wam_pool(), runs=np.arange(8) % 4)
    mod.batch_waypoint_clearance(asked, points=(0, -1))
    after = mod.batch_select_clear(asked, n_groups=2, margin=-np.inf, by="clearance")
    for a, b in zip(before, after):
        assert np.array_equal(a, b, equal_nan=True)
    assert same(mod.batch_gettraj(asked), mod.batch_gettraj(twin))
    out = [mod.batch_iterate(bid, 5) for bid in (asked, twin)]
    assert same(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), "costs and status"
    assert same(mod.batch_gettraj(asked), mod.batch_gettraj(twin)), "trajectories"
    assert not same(mod.batch_waypoint_clearance(asked)["clearance"], prof["clearance"]), "the profile follows the trajectories"
    mod.batch_destroy(asked); mod.batch_destroy(twin)


# ---- 8. rejected calls ------------------------------------------------------------------------------------------------------------

def test_rejected_calls(wam):
    mod, model = wam["mod"], wam["model"]
    lib, h = mod._lib, mod._h
    dp, ip = _capi.c_double_p, _capi.c_int_p
    n_runs, n_points = 3, 4
    pool = CC.wam_pool()[:3]
    bid = mod.batch_create(model.name, common.wam_goals(n_runs, seed=8), **KW4)
    mod.batch_set_traj(bid, CC.one_sample_batch(pool))
    traj = mod.batch_gettraj(bid)
    want = mod.batch_config_clearance(bid, pool, runs=np.arange(3))
    clr = np.full((n_runs * n_points, 2), 7.0); sph = np.full((n_runs * n_points, 2), 7, dtype=np.int32); oth = sph.copy()
    cfg = np.ascontiguousarray(pool); run = np.arange(3, dtype=np.int32); pt = np.zeros(3, dtype=np.int32)
    arr = lambda *v: np.array(v, dtype=np.int32)
    config = lambda b, n_q, r, c: lib.orc_batch_config_clearance(h, b, n_q, None if r is None else r.ctypes.data_as(ip),
                                                                 None if c is None else c.ctypes.data_as(dp), clr.ctypes.data_as(dp),
                                                                 sph.ctypes.data_as(ip), oth.ctypes.data_as(ip))
    waypoint = lambda b, n_q, r, p: lib.orc_batch_waypoint_clearance(h, b, n_q, None if r is None else r.ctypes.data_as(ip),
                                                                     None if p is None else p.ctypes.data_as(ip), clr.ctypes.data_as(dp),
                                                                     sph.ctypes.data_as(ip), oth.ctypes.data_as(ip))
    cases = {
        "config: unknown batch": lambda: config(bid + 1000, 3, run, cfg), "waypoint: unknown batch": lambda: waypoint(bid + 1000, 3, run, pt),
        "config: n_q 0": lambda: config(bid, 0, run, cfg), "config: n_q 2^22 + 1": lambda: config(bid, (1 << 22) + 1, None, cfg),
        "waypoint: n_q 0": lambda: waypoint(bid, 0, run, pt), "waypoint: n_q 2^22 + 1": lambda: waypoint(bid, (1 << 22) + 1, None, None),
        "config: no configs": lambda: config(bid, 3, run, None),
        "config: run -1": lambda: config(bid, 3, arr(0, -1, 2), cfg), "config: run n_runs": lambda: config(bid, 3, arr(0, 1, n_runs), cfg),
        "waypoint: run -1": lambda: waypoint(bid, 3, arr(-1, 1, 2), pt), "waypoint: run n_runs": lambda: waypoint(bid, 3, arr(0, n_runs, 2), pt),
        "waypoint: point -1": lambda: waypoint(bid, 3, run, arr(0, 0, -1)), "waypoint: point n_points": lambda: waypoint(bid, 3, run, arr(n_points, 0, 0)),
        "waypoint: runs without points": lambda: waypoint(bid, 3, run, None), "waypoint: points without runs": lambda: waypoint(bid, 3, None, pt),
        "waypoint: the profile with a wrong n_q": lambda: waypoint(bid, n_runs * n_points - 1, None, None),
    }
    for name, call in cases.items():
        assert call() == 1, name
        assert lib.orc_last_error(h).decode(), name
        assert (clr == 7.0).all() and (sph == 7).all() and (oth == 7).all(), name
        assert same(mod.batch_gettraj(bid), traj), name
        assert config(bid, 3, run, cfg) == 0, name      # the next valid call succeeds
        assert np.array_equal(bits(clr[:3]), bits(want["clearance"])) and np.array_equal(sph[:3], want["sphere"]) and np.array_equal(oth[:3], want["other"]), name
        clr[:] = 7.0; sph[:] = 7; oth[:] = 7
    # any output may be NULL
    assert lib.orc_batch_config_clearance(h, bid, 3, None, cfg.ctypes.data_as(dp), None, None, None) == 0
    assert lib.orc_batch_waypoint_clearance(h, bid, n_runs * n_points, None, None, None, sph.ctypes.data_as(ip), None) == 0
    # a non-finite entry: that query alone is not evaluated
    for poison in (np.nan, np.inf, -np.inf):
        bad = pool.copy(); bad[1, 5] = poison
        got = mod.batch_config_clearance(bid, bad, runs=np.arange(3))
        assert np.isnan(got["clearance"][1]).all() and (got["sphere"][1] == -1).all() and (got["other"][1] == -1).all(), poison
        assert_same(pick(got, [0, 2]), pick(want, [0, 2]), "beside a poisoned row")
    assert_same(mod.batch_config_clearance(bid, pool, runs=np.arange(3)), want, "after the poisoned rows")
    # the Python layer's own checks
    for call in (lambda: mod.batch_config_clearance(bid, pool[:, :6]), lambda: mod.batch_config_clearance(bid, pool, runs=[0, 1]),
                 lambda: mod.batch_config_clearance(bid, pool, runs=n_runs), lambda: mod.batch_waypoint_clearance(bid, runs=[0, 1]),
                 lambda: mod.batch_waypoint_clearance(bid, points=n_points), lambda: mod.batch_waypoint_clearance(bid, runs=[0, 1], points=[0]),
                 lambda: mod.batch_waypoint_clearance(bid, points=[0.5])):
        with pytest.raises(ValueError):
            call()
    mod.batch_destroy(bid)
