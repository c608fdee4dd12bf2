"""-m gpu: the clearance of given paths and of segments between waypoints (orc_batch_path_clearance,
orc_batch_waypoint_segment_clearance; Module.batch_path_clearance, Module.batch_waypoint_segment_clearance).

The exact yardstick is orc_batch_clearance: a batch of one run per path, given the paths by batch_set_traj -- for a segment
[a, b] the three-point trajectory [a, b, b], which has the same samples (tests/test_host_path_clearance.py checks that
premise).  The new calls must return that run's five outputs with no tolerance, in fp64 and in fp32, whatever shares a chunk
with a query, in whatever order, shard or round it is asked."""
import os
import subprocess
import sys

import numpy as np
import pytest

import common
import config_clearance as CC
import or_cdchomp_amd
import path_clearance as PC
from or_cdchomp_amd import _capi, scenes
from test_gpu_config_clearance import SHIFT, tree_module
from test_gpu_verdict_device import KW, same, set_wam_vmax, wam_goals_with_table

pytestmark = pytest.mark.gpu

KEYS = PC.KEYS
KW4 = dict(KW, n_points=4)


def assert_same(got, want, what=""):
    """bit for bit, the five outputs of two results (dicts of arrays of one shape); NaN minima on a bit view"""
    for key in KEYS:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, key, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (what, key, np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1)), a, b)


def pick(res, idx):
    return {key: np.asarray(res[key])[idx] for key in KEYS}


def yardstick(mod, create, paths, max_samples=65536):
    """batch_clearance of a batch of one run per path that holds the paths: create(n_runs, n_points) makes the batch"""
    paths = np.asarray(paths, dtype=np.float64)
    trajs = PC.abb(paths) if paths.shape[1] == 2 else paths
    bid = create(len(trajs), trajs.shape[1])
    mod.batch_set_traj(bid, trajs)
    ref = mod.batch_clearance(bid, max_samples=max_samples)
    mod.batch_destroy(bid)
    return ref


@pytest.fixture(scope="module")
def wam():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    set_wam_vmax(mod, model)
    create = lambda n_runs, n_points, **kw: mod.batch_create(model.name, common.wam_goals(n_runs, seed=1), **dict(KW, n_points=n_points, **kw))
    yield dict(mod=mod, model=model, create=create)
    mod.close()


@pytest.fixture(scope="module")
def wam2():
    """the same scene on a module of two in-process shards on one card"""
    mod = or_cdchomp_amd.Module([0, 0])
    model = common.setup_product_wam(mod)
    set_wam_vmax(mod, model)
    yield dict(mod=mod, model=model)
    mod.close()


@pytest.fixture(scope="module")
def chunks(wam):
    """the segments that meet the chunk's edges, their yardstick, and the new call's answer in the order as built"""
    mod = wam["mod"]
    segs, counts = PC.chunk_segments()
    ref = yardstick(mod, wam["create"], segs)
    bid = wam["create"](1, 4)
    got = mod.batch_path_clearance(bid, segs)
    yield dict(segs=segs, counts=counts, ref=ref, got=got, bid=bid)
    mod.batch_destroy(bid)


# ---- 1. paths against batch_clearance ------------------------------------------------------------------------------------------

def test_paths_of_the_wam(wam):
    mod = wam["mod"]
    paths, counts = PC.wam_paths()
    names = list(paths)
    P = np.array([paths[nm] for nm in names])
    bid = wam["create"](3, 8)      # (the asked batch's own shape plays no part)
    for cap, col in ((65536, 0), (PC.CAP, 1)):
        ref = yardstick(mod, wam["create"], P, max_samples=cap)
        got = mod.batch_path_clearance(bid, P, max_samples=cap)
        for k, nm in enumerate(names):
            print("cap %5d  %-28s n %4d  %+.9f %+.9f  t %s  spheres %s others %s" % (cap, nm, got["n_samples"][k], got["clearance"][k, 0],
                  got["clearance"][k, 1], got["time"][k], got["sphere"][k], got["other"][k]))
        assert ref["n_samples"].tolist() == [counts[nm][col] for nm in names], "the yardstick has the intended samples"
        assert_same(got, ref, "max_samples %d" % cap)
        for k in range(len(names)):
            assert_same(mod.batch_path_clearance(bid, P[k], max_samples=cap), pick(ref, slice(k, k + 1)), "alone: " + names[k])
    ix = names.index
    assert (ref["n_samples"][[ix("dips: from above"), ix("too long under the cap")]] == -2).all() and np.isnan(ref["clearance"][ix("dips: from above")]).all()
    ref = yardstick(mod, wam["create"], P)
    assert (ref["clearance"][ix("clear: about the start")] > 0).all() and ref["clearance"][ix("clear: away from the table"), 0] > 0
    assert (ref["clearance"][[ix("dips: from above"), ix("dips: along the top")], 0] < 0).all()
    assert ref["clearance"][ix("self contact"), 1] < 0
    z = ix("zero length")
    assert np.isposinf(ref["clearance"][z]).all() and (ref["time"][z] == -1).all() and (ref["sphere"][z] == -1).all() and (ref["other"][z] == -1).all()
    assert np.isnan(ref["clearance"][ix("an infinite entry")]).all() and not np.isnan(ref["clearance"][ix("a NaN entry")]).any()
    mod.batch_destroy(bid)


# ---- 2. segments at the chunk's edges, in three orders ---------------------------------------------------------------------

def test_segments_at_the_chunk_edges(wam, chunks):
    mod, segs, ref = wam["mod"], chunks["segs"], chunks["ref"]
    assert ref["n_samples"].tolist() == chunks["counts"].tolist()
    assert len(np.unique(ref["clearance"], axis=0)) >= 20, "the answers must tell the segments apart"
    for k, order in enumerate(PC.chunk_orders(chunks["counts"])):
        got = mod.batch_path_clearance(chunks["bid"], segs[order])
        assert_same(got, pick(ref, order), "order %d against the yardstick" % k)
        back = np.argsort(order)
        assert_same(pick(got, back), chunks["got"], "order %d against the order as built" % k)
    # the same segments as two rows of longer storage: runs=... of one int
    assert_same(mod.batch_path_clearance(chunks["bid"], segs, runs=0), chunks["got"], "run 0 named")


# ---- 3. rounds ---------------------------------------------------------------------------------------------------------------

def test_rounds(chunks, tmp_path):
    out = str(tmp_path / "rounds.npz")
    env = dict(os.environ, ORC_PATH_WORKSPACE="132")
    subprocess.run([sys.executable, os.path.abspath(PC.__file__), out], env=env, check=True, timeout=300)
    res = np.load(out)
    assert_same({k: res[k] for k in KEYS}, chunks["got"], "a workspace of 132 entries")
    assert_same({k: res["again_" + k] for k in KEYS}, chunks["got"], "... asked again")
    assert "ORC_PATH_WORKSPACE" in str(res["refused"]), "a workspace below the longest query is refused: the switch is read"


# ---- 4. variants -------------------------------------------------------------------------------------------------------------

def check_variant(mod, create, paths, what, runs=None, **create_kw):
    """paths and, of their first and last rows, segments: the new call on a batch of another shape against the yardstick"""
    bid = create(1 if runs is None else int(np.max(runs)) + 1, 6)
    out = None
    for form, P in (("paths", paths), ("segments", paths[:, [0, -1]])):
        ref = yardstick(mod, create, P)
        got = mod.batch_path_clearance(bid, P, runs=runs)
        assert (ref["n_samples"] >= (2 if form == "paths" else 1)).all(), (what, form, ref["n_samples"])
        assert_same(got, ref, "%s: %s" % (what, form))
        out = out or ref
    mod.batch_destroy(bid)
    return out


def test_floating_base():
    mod = or_cdchomp_amd.Module(0)
    model, base, dofvals, adofs = common.wam_state()
    base = np.asarray(base, dtype=np.float64)
    base[0] -= 0.2
    mod.add_robot(model, transform=list(base), dof_values=dofvals, active_dofs=adofs)
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    set_wam_vmax(mod, model)
    paths = PC.local_paths(CC.floating_configs(base), 7, seed=len("floating"))
    create = lambda n_runs, n_points: mod.batch_create(model.name, common.wam_goals(n_runs, seed=3), basegoals=np.tile(base, (n_runs, 1)),
                                                       **dict(KW, n_points=n_points, floating_base=1))
    ref = check_variant(mod, create, paths, "floating base")
    assert np.isfinite(ref["clearance"][:, 1]).all() and len(np.unique(ref["clearance"], axis=0)) == len(paths)
    mod.close()


def test_tree_robot():
    mod, model, names = tree_module()
    paths = PC.local_paths(CC.tree_pool(), seed=len("tree"))
    create = lambda n_runs, n_points: mod.batch_create(model.name, common.config5_goals(n_runs), **dict(common.CONFIG5_KW, n_points=n_points))
    bid = create(1, 4)
    assert mod.batch_plan(bid)["variant"] & 1, "the robot must be a tree"
    mod.batch_destroy(bid)
    ref = check_variant(mod, create, paths, "tree")
    print("tree: fields at the minima", sorted(set(ref["other"][:, 0].tolist())), "clearances", ref["clearance"].min(axis=0))
    assert np.isfinite(ref["clearance"][:, 1]).all()
    mod.close()


def test_held_body():
    mod = or_cdchomp_amd.Module(0)
    model, hand, pose = common.setup_product_wam_held4(mod)
    set_wam_vmax(mod, model)
    paths = PC.local_paths(CC.held_configs(), seed=len("held"))
    create = lambda n_runs, n_points: mod.batch_create(model.name, common.wam_goals(n_runs, seed=4), **dict(KW, n_points=n_points))
    ref = check_variant(mod, create, paths, "held body")
    print("held body: spheres at the minima", ref["sphere"].tolist())
    assert np.isin(ref["sphere"], [16, 17, 18, 19]).any(), "the held spheres must appear among the answers"
    mod.close()


def test_precision_32(wam):
    mod, model = wam["mod"], wam["model"]
    paths = PC.local_paths(CC.wam_pool(), seed=len("pool"))
    assert not same(paths, paths.astype(np.float32)), "the rows are doubles that no float holds"
    create = lambda n_runs, n_points: wam["create"](n_runs, n_points, precision=32)
    ref = check_variant(mod, create, paths, "precision 32")
    assert same(ref["clearance"], ref["clearance"].astype(np.float32)), "the minima are floats, widened"
    bid = create(1, 4)
    narrowed = paths.astype(np.float32).astype(np.float64)
    assert_same(mod.batch_path_clearance(bid, narrowed), ref, "the narrowed rows")
    mod.batch_destroy(bid)
    ref64 = yardstick(mod, wam["create"], paths)
    assert not same(ref64["clearance"], ref["clearance"]), "the two precisions answer differently"


def test_self_check_off_and_on_again():
    mod = or_cdchomp_amd.Module(0)
    model, base, dofvals, adofs = common.wam_state()
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    mod.add_kinbody_boxes("far", [([0, 0, 0, 0, 0, 0, 1], [0.05, 0.05, 0.05])], transform=[5, 5, 5, 0, 0, 0, 1])
    mod.SendCommand("computedistancefield kinbody far")
    set_wam_vmax(mod, model)
    paths = PC.local_paths(CC.folding_configs(), seed=len("folding"))
    create = lambda n_runs, n_points: mod.batch_create(model.name, np.tile(CC.folding_configs()[0], (n_runs, 1)),
                                                       **dict(n_points=n_points, lambda_=100.0, obs_factor=0.0, obs_factor_self=0.0))
    on = check_variant(mod, create, paths, "self check on")
    assert (on["clearance"][:, 1] < 0).any() and (on["clearance"][:, 1] > 0).any() and np.isposinf(on["clearance"][:, 0]).all()
    mod.set_self_check(model.name, False)
    off = check_variant(mod, create, paths, "self check off")
    assert np.isposinf(off["clearance"]).all() and (off["sphere"] == -1).all() and (off["other"] == -1).all() and (off["time"] == -1).all()
    assert (off["n_samples"] == on["n_samples"]).all()
    mod.set_self_check(model.name, True)
    assert_same(check_variant(mod, create, paths, "self check on again"), on, "on again")
    mod.close()


def test_per_run_scenes():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    mod.SendCommand("computedistancefield kinbody mug")
    set_wam_vmax(mod, model)
    sc = [[("table", None), ("mug", None)], [("table", SHIFT), ("mug", SHIFT)], [("table", None)], []]
    paths = PC.local_paths(CC.wam_pool(), seed=len("scenes"))
    run_of_q = np.array([0, 1, 2, 3, 3, 1, 0, 2], dtype=np.int32)
    goals = common.wam_goals(8, seed=6)
    # the yardstick: run q of a per-run-scenes batch sees the scene that query q names
    create = lambda n_runs, n_points: mod.batch_create(model.name, goals[:n_runs], scenes=sc, scene_of_run=run_of_q[:n_runs], **dict(KW, n_points=n_points))
    bid = mod.batch_create(model.name, goals[:4], scenes=sc, scene_of_run=np.arange(4, dtype=np.int32), **KW4)
    for form, P in (("paths", paths), ("segments", paths[:, [0, -1]])):
        ref = yardstick(mod, create, P)
        assert_same(mod.batch_path_clearance(bid, P, runs=run_of_q), ref, "per-run scenes: " + form)
    empty = run_of_q == 3
    assert np.isposinf(ref["clearance"][empty, 0]).all() and np.isfinite(ref["clearance"][empty, 1]).all(), "the empty scene still has the robot itself"
    one = mod.batch_path_clearance(bid, paths, runs=0); two = mod.batch_path_clearance(bid, paths, runs=1)
    assert not same(one["clearance"][:, 0], two["clearance"][:, 0]), "the shifted scene must answer differently"
    mod.batch_destroy(bid)
    mod.close()


# ---- 5. the waypoint form ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [64, 32])
def test_waypoint_segments(wam, precision):
    mod, model = wam["mod"], wam["model"]
    n_runs, n_points = 4, 12
    bid = mod.batch_create(model.name, wam_goals_with_table(n_runs, seed=91, k_table=2), **dict(KW, n_points=n_points, precision=precision))
    mod.batch_iterate(bid, 10)
    traj = mod.batch_gettraj(bid)
    runs, frm, to = PC.waypoint_pairs(n_runs, n_points)
    got = mod.batch_waypoint_segment_clearance(bid, runs, frm, to)
    rows = np.stack([traj[runs, frm], traj[runs, to]], axis=1)
    want = mod.batch_path_clearance(bid, rows, runs=runs)
    print("waypoint segments, precision", precision, "samples", got["n_samples"].tolist(), "clearance", got["clearance"][:, 0].tolist())
    assert_same(got, want, "against the rows of gettraj")
    assert (got["n_samples"][frm == to] == 0).all() and np.isposinf(got["clearance"][frm == to]).all()
    assert (got["n_samples"][frm != to] > 0).all()
    assert (got["clearance"][:, 0] < 0).any() and (got["clearance"][:, 0] > 0).any(), "both outcomes must occur"
    # one int stands for all
    assert_same(mod.batch_waypoint_segment_clearance(bid, 1, frm, to), mod.batch_path_clearance(bid, np.stack([traj[1, frm], traj[1, to]], axis=1), runs=1),
                "one run for all")
    mod.batch_destroy(bid)


# ---- 6. two shards -------------------------------------------------------------------------------------------------------------

def test_two_shards(wam, wam2):
    paths = PC.local_paths(CC.wam_pool(), seed=len("shards"))
    ci = np.arange(21) % len(paths)
    ri = np.array([0, 2, 1, 3, 2, 0, 3, 1, 1] * 3)[:21]      # runs 0, 1: the first shard; 2, 3: the second
    wr, wf, wt = np.array([0, 2, 1, 3, 3, 0]), np.array([0, 1, 2, 3, 0, 1]), np.array([3, 0, 2, 1, 2, 3])
    res = []
    for m_ in (wam, wam2):
        mod, model = m_["mod"], m_["model"]
        bid = mod.batch_create(model.name, common.wam_goals(4, seed=7), scenes=[[("table", None)], [("table", SHIFT)]],
                               scene_of_run=np.array([0, 1, 1, 0], dtype=np.int32), **KW4)
        res.append((mod.batch_path_clearance(bid, paths[ci], runs=ri), mod.batch_path_clearance(bid, paths[ci][:, [0, -1]], runs=ri),
                    mod.batch_waypoint_segment_clearance(bid, wr, wf, wt)))
        mod.batch_destroy(bid)
    for one, two, what in zip(res[0], res[1], ("paths", "segments", "waypoint segments")):
        assert_same(two, one, "two shards: " + what)
    assert ci[0] == ci[8] and (ri[0], ri[8]) == (0, 1)
    assert not same(res[0][0]["clearance"][0, 0], res[0][0]["clearance"][8, 0]), "the two scenes answer differently"


# ---- 7. no state ---------------------------------------------------------------------------------------------------------------

def test_the_calls_leave_no_state(wam):
    mod, model = wam["mod"], wam["model"]
    kw = dict(KW, n_points=16)
    goals = wam_goals_with_table(4, seed=92, k_table=1)
    asked, twin = mod.batch_create(model.name, goals, **kw), mod.batch_create(model.name, goals, **kw)
    for bid in (asked, twin):
        mod.batch_iterate(bid, 5)
    state = lambda bid: [mod.batch_state(bid, w) for w in ("T", "G", "AG")]
    before = state(asked)
    sel = mod.batch_select_clear(asked, n_groups=2, margin=-np.inf, by="clearance")
    best = mod.batch_select_best(asked, n_groups=2)
    runs, frm, to = PC.waypoint_pairs(4, 16)
    first = mod.batch_waypoint_segment_clearance(asked, runs, frm, to)
    mod.batch_path_clearance(asked, PC.local_paths(CC.wam_pool()), runs=np.arange(8) % 4)
    for a, b in zip(before, state(asked)):
        assert same(a, b), "trajectories, gradients and momentum"
    for a, b in zip(sel, mod.batch_select_clear(asked, n_groups=2, margin=-np.inf, by="clearance")):
        assert np.array_equal(a, b, equal_nan=True)
    for a, b in zip(best, mod.batch_select_best(asked, n_groups=2)):
        assert np.array_equal(a, b, equal_nan=True), "the verdict keys"
    assert same(mod.batch_gettraj(asked), mod.batch_gettraj(twin))
    out = [mod.batch_iterate(bid, 5) for bid in (asked, twin)]
    assert same(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), "costs and status"
    assert same(mod.batch_gettraj(asked), mod.batch_gettraj(twin)), "trajectories"
    assert not same(mod.batch_waypoint_segment_clearance(asked, runs, frm, to)["clearance"], first["clearance"]), "the segments follow the trajectories"
    mod.batch_destroy(asked); mod.batch_destroy(twin)


# ---- 8. rejected calls ---------------------------------------------------------------------------------------------------------

def test_rejected_calls(wam):
    mod, model = wam["mod"], wam["model"]
    lib, h = mod._lib, mod._h
    dp, ip = _capi.c_double_p, _capi.c_int_p
    n_runs, n_points, n_q = 3, 4, 3
    paths = np.ascontiguousarray(PC.local_paths(CC.wam_pool()[:3]))
    bid = mod.batch_create(model.name, common.wam_goals(n_runs, seed=8), **KW4)
    traj = mod.batch_gettraj(bid)
    want = mod.batch_path_clearance(bid, paths, runs=np.arange(3))
    clr = np.full((n_q, 2), 7.0); tim = np.full((n_q, 2), 7.0)
    sph = np.full((n_q, 2), 7, dtype=np.int32); oth = sph.copy(); cnt = np.full(n_q, 7, dtype=np.int32)
    run = np.arange(3, dtype=np.int32); pf = np.zeros(3, dtype=np.int32); pt = np.full(3, 2, dtype=np.int32)
    arr = lambda *v: np.array(v, dtype=np.int32)
    p_ = lambda a, t: None if a is None else a.ctypes.data_as(t)

    def path(b, nq, r, n_rows, p, cap, c=clr, ns=cnt):
        return lib.orc_batch_path_clearance(h, b, nq, p_(r, ip), n_rows, p_(p, dp), cap, p_(c, dp), p_(tim, dp), p_(sph, ip), p_(oth, ip), p_(ns, ip))

    def segment(b, nq, r, f, t, cap, c=clr, ns=cnt):
        return lib.orc_batch_waypoint_segment_clearance(h, b, nq, p_(r, ip), p_(f, ip), p_(t, ip), cap, p_(c, dp), p_(tim, dp), p_(sph, ip), p_(oth, ip),
                                                        p_(ns, ip))
    cases = {
        "path: unknown batch": lambda: path(bid + 1000, 3, run, 3, paths, 64), "segment: unknown batch": lambda: segment(bid + 1000, 3, run, pf, pt, 64),
        "path: n_q 0": lambda: path(bid, 0, run, 3, paths, 64), "path: n_q 2^22 + 1": lambda: path(bid, (1 << 22) + 1, None, 3, paths, 64),
        "segment: n_q 0": lambda: segment(bid, 0, run, pf, pt, 64), "segment: n_q 2^22 + 1": lambda: segment(bid, (1 << 22) + 1, None, pf, pt, 64),
        "path: n_rows 1": lambda: path(bid, 3, run, 1, paths, 64), "path: n_rows 4097": lambda: path(bid, 3, run, 4097, paths, 64),
        "path: no paths": lambda: path(bid, 3, run, 3, None, 64),
        "path: no clearance_out": lambda: path(bid, 3, run, 3, paths, 64, c=None), "path: no n_samples_out": lambda: path(bid, 3, run, 3, paths, 64, ns=None),
        "segment: no clearance_out": lambda: segment(bid, 3, run, pf, pt, 64, c=None), "segment: no n_samples_out": lambda: segment(bid, 3, run, pf, pt, 64, ns=None),
        "path: max_samples 0": lambda: path(bid, 3, run, 3, paths, 0), "path: max_samples 2^20 + 1": lambda: path(bid, 3, run, 3, paths, (1 << 20) + 1),
        "segment: max_samples 0": lambda: segment(bid, 3, run, pf, pt, 0), "segment: max_samples 2^20 + 1": lambda: segment(bid, 3, run, pf, pt, (1 << 20) + 1),
        "path: run -1": lambda: path(bid, 3, arr(0, -1, 2), 3, paths, 64), "path: run n_runs": lambda: path(bid, 3, arr(0, 1, n_runs), 3, paths, 64),
        "segment: run -1": lambda: segment(bid, 3, arr(-1, 1, 2), pf, pt, 64), "segment: run n_runs": lambda: segment(bid, 3, arr(0, n_runs, 2), pf, pt, 64),
        "segment: from -1": lambda: segment(bid, 3, run, arr(0, 0, -1), pt, 64), "segment: from n_points": lambda: segment(bid, 3, run, arr(n_points, 0, 0), pt, 64),
        "segment: to -1": lambda: segment(bid, 3, run, pf, arr(0, -1, 0), 64), "segment: to n_points": lambda: segment(bid, 3, run, pf, arr(0, 0, n_points), 64),
        "segment: no from": lambda: segment(bid, 3, run, None, pt, 64), "segment: no to": lambda: segment(bid, 3, run, pf, None, 64),
    }
    for name, call in cases.items():
        assert call() == 1, name
        assert lib.orc_last_error(h).decode(), name
        assert (clr == 7.0).all() and (tim == 7.0).all() and (sph == 7).all() and (oth == 7).all() and (cnt == 7).all(), name
        assert same(mod.batch_gettraj(bid), traj), name
        assert path(bid, 3, run, 3, paths, 65536) == 0, name      # the next valid call succeeds
        assert_same(dict(clearance=clr, time=tim, sphere=sph, other=oth, n_samples=cnt), want, name)
        clr[:] = 7.0; tim[:] = 7.0; sph[:] = 7; oth[:] = 7; cnt[:] = 7
    # the optional outputs may be NULL
    assert lib.orc_batch_path_clearance(h, bid, 3, None, 3, p_(paths, dp), 64, p_(clr, dp), None, None, None, p_(cnt, ip)) == 0
    assert lib.orc_batch_waypoint_segment_clearance(h, bid, 3, None, p_(pf, ip), p_(pt, ip), 64, p_(clr, dp), None, None, None, p_(cnt, ip)) == 0
    # the Python layer's own checks
    for call in (lambda: mod.batch_path_clearance(bid, paths[:, :, :6]), lambda: mod.batch_path_clearance(bid, paths, runs=[0, 1]),
                 lambda: mod.batch_waypoint_segment_clearance(bid, [0, 1], [0, 1, 2], [1, 2, 3])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError):
        mod.batch_path_clearance(bid, paths, runs=n_runs)
    assert_same(mod.batch_path_clearance(bid, paths, runs=np.arange(3)), want, "after the rejected calls")
    mod.batch_destroy(bid)
