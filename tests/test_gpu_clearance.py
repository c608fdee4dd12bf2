"""-m gpu: the clearance of a batch's runs (orc_batch_clearance, Module.batch_clearance) and the selection by margin
(orc_batch_select_clear, Module.batch_select_clear).  The yardstick is the restatement of tests/clearance.py on the doubles
batch_gettraj returns, which tests/test_host_clearance.py pins to the oracle's re-check; the selection is held to
or_cdchomp_amd.module.select_clear and, at margin 0, to orc_batch_select_best_by with require_collision_free."""
import ctypes as C

import numpy as np
import pytest

import clearance as CL
import common
import or_cdchomp_amd
from or_cdchomp_amd import _capi, robots, scenes
from or_cdchomp_amd.module import candidates, clearance_too_long, contiguous_groups, select_clear
from test_gpu_verdict_device import KW, same, set_wam_vmax, wam_goals_with_table
from test_gpu_verdict_subset import masks_of

pytestmark = pytest.mark.gpu

KEYS = ("clearance", "time", "sphere", "other", "n_samples")
# precision 32: the existing fp32 verdict's depth against the restated first contact's (fp32_depth_error below, which
# test_precision_32 prints again) on the 10 colliding runs of that test's batch measured 7.829e-08 m as the largest absolute
# difference (NOTES/clearance.md); a minimum ranges over many more items than one contact, so four times that is allowed
FP32_DEPTH_ERR = 7.829e-08
FP32_TOL = 4.0 * FP32_DEPTH_ERR


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def compose(O, a, b):
    out = np.zeros(7)
    O.lib().ora_kin_pose_compose(O.dp(O.f64(a)), O.dp(O.f64(b)), O.dp(out))
    return out


def product_field(O, mod, name, kpose=None):
    """the module's field of `name` as the restatement reads it, the kinbody where it stands or at kpose"""
    data, lengths, gpose = mod.get_sdf(name)
    return CL.Field(O, data, lengths, compose(O, mod.body_transform(name) if kpose is None else kpose, gpose))


def assert_rows_equal(got, want, rows, what=""):
    """bit for bit, the rows `rows` of two results"""
    for key in KEYS:
        a, b = np.asarray(got[key])[rows], np.asarray(want[key])[rows]
        if a.dtype == np.float64:
            assert np.array_equal(bits(a), bits(b)), (what, key, a, b)
        else:
            assert np.array_equal(a, b), (what, key, a, b)


def assert_not_walked(got, rows, mark, what=""):
    rows = np.asarray(rows)
    assert np.isnan(got["clearance"][rows]).all() and (got["time"][rows] == -1.0).all(), what
    assert (got["sphere"][rows] == -1).all() and (got["other"][rows] == -1).all() and (got["n_samples"][rows] == mark).all(), what


def assert_run(got, k, res, tol, what=""):
    """run k of a device result against its restatement: n_samples equal; each minimum within tol(restated minimum); its key
    one of the items whose restated gap lies within that tolerance of the restated minimum -- the item, where the minimum is
    that clear -- and its time that item's, bit for bit"""
    assert got["n_samples"][k] == res["n_samples"], (what, k, got["n_samples"][k], res["n_samples"])
    n_tied = 0
    for leg, (gap, key, tm) in enumerate(((res["fgap"], res["fkey"], res["ftime"]), (res["pgap"], res["pkey"], res["ptime"]))):
        if not len(gap):
            assert np.isposinf(got["clearance"][k, leg]) and (got["sphere"][k, leg], got["other"][k, leg], got["time"][k, leg]) == (-1, -1, -1.0), (what, k, leg)
            continue
        t = tol(res["clearance"][leg])
        assert abs(got["clearance"][k, leg] - res["clearance"][leg]) <= t, (what, k, leg, got["clearance"][k], res["clearance"])
        near = np.flatnonzero(gap <= res["clearance"][leg] + t)
        n_tied += len(near) > 1
        hit = [i for i in near if key[i, 1] == got["sphere"][k, leg] and key[i, 2] == got["other"][k, leg] and bits(tm[i]) == bits(got["time"][k, leg])]
        assert hit, (what, k, leg, got["sphere"][k], got["other"][k], got["time"][k], res["sphere"], res["other"], res["time"])
    return n_tied


def assert_run_fp64(got, k, res, what=""):
    """fp64: np.isclose's rtol 1e-9 and atol 1e-12, the figures the verdict's depth is held to.  Where the restated minimum is
    the only item within that tolerance of itself this is "keys equal, times bit-identical"; a pair of spheres that no active
    joint moves against each other has the same gap at every sample but for the last bits, and there no restatement can say
    which sample the device's own rounding makes the lowest"""
    return assert_run(got, k, res, lambda c: 1e-12 + 1e-9 * abs(c), what)


def assert_run_fp32(got, k, res, what=""):
    """precision 32: the restatement in double on the batch's float trajectories, FP32_TOL for the minima and for the key as "one of them" """
    return assert_run(got, k, res, lambda c: FP32_TOL, what)


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
    vmax = set_wam_vmax(mod, model)
    yield dict(mod=mod, model=model, vmax=vmax)
    mod.close()


# ---- 1. chunk edges -----------------------------------------------------------------------------------------------------

def test_chunk_edges(wam):
    mod, model = wam["mod"], wam["model"]
    runs = CL.synthetic_runs(robots.WAM_START)
    bid = mod.batch_create(model.name, common.wam_goals(len(runs), seed=1), **dict(KW, n_points=CL.SYNTH_POINTS))
    mod.batch_set_traj(bid, runs)
    assert same(mod.batch_gettraj(bid), runs)
    got = mod.batch_clearance(bid)
    for k, name in enumerate(CL.SYNTH_NAMES):
        res = CL.restate(wam["tab"], runs[k], wam["vmax"], 0, [wam["field"]])
        assert not CL.set_aside(res, [wam["field"]]), name
        print("%-20s samples %4d clearance %+.6f %+.6f at samples %s" % (name, res["n_samples"], got["clearance"][k, 0], got["clearance"][k, 1],
              [int(np.searchsorted(res["times"], t)) if t >= 0 else -1 for t in got["time"][k]]))
        assert_run_fp64(got, k, res, name)
    z = CL.SYNTH_NAMES.index("zero length")
    assert got["n_samples"][z] == 0 and np.isposinf(got["clearance"][z]).all() and (got["time"][z] == -1.0).all()
    assert (got["sphere"][z] == -1).all() and (got["other"][z] == -1).all()
    assert_rows_equal(got, {key: np.roll(got[key], 1, axis=0) for key in KEYS}, [CL.SYNTH_NAMES.index("twin b")], "twins")
    p = CL.SYNTH_NAMES.index("penetrates")
    assert got["clearance"][p, 0] < 0.0
    mod.batch_destroy(bid)


# ---- 2 .. the batch after an iterate call --------------------------------------------------------------------------------
N_RUNS, N_ITER, CAP = 24, 40, 4096
KW30 = dict(KW, n_points=30)
SEED = 91      # (the oracle on the CPU, these goals, 40 iterations: run 0 leaves its joint limits)


def iterate_batch(mod, model, goals=None):
    goals = wam_goals_with_table(N_RUNS, seed=SEED) if goals is None else goals
    bid = mod.batch_create(model.name, goals, **KW30)
    costs, status = mod.batch_iterate(bid, N_ITER)
    return bid, costs, status


@pytest.fixture(scope="module")
def iterated(wam):
    """the batch of tests 2, 3, 5 .. 9, its all-runs clearance and the restatement of every run the cap lets through"""
    mod, model, vmax = wam["mod"], wam["model"], wam["vmax"]
    bid, costs, status = iterate_batch(mod, model)
    traj = mod.batch_gettraj(bid)
    full = mod.batch_clearance(bid, max_samples=CAP)
    long_ = np.array([clearance_too_long(traj[k], vmax, 0, CAP) for k in range(N_RUNS)])
    res = [None if long_[k] else CL.restate(wam["tab"], traj[k], vmax, 0, [wam["field"]]) for k in range(N_RUNS)]
    aside = np.array([r is not None and CL.set_aside(r, [wam["field"]]) for r in res])
    yield dict(bid=bid, costs=costs, status=status, traj=traj, full=full, long=long_, res=res, aside=aside)
    mod.batch_destroy(bid)


def test_after_an_iterate_call(wam, iterated):
    it = iterated
    status, full = it["status"], it["full"]
    assert (status == -1).any(), "a run must have left its limits"
    assert not it["long"][status != -1].any(), "only a run that left its limits is too long"
    print("status -1: %s, too long for %d: %s, set aside by the face premise: %d" % (np.flatnonzero(status == -1).tolist(), CAP,
          np.flatnonzero(it["long"]).tolist(), int(it["aside"].sum())))
    assert it["aside"].sum() <= 1
    if it["long"].any():
        assert_not_walked(full, np.flatnonzero(it["long"]), -2, "too long")
    for k in np.flatnonzero(~it["long"] & ~it["aside"]):
        assert_run_fp64(full, k, it["res"][k], "iterated")
    walked = full["n_samples"] >= 0
    assert (full["clearance"][walked].min(axis=1) < 0).any() and (full["clearance"][walked].min(axis=1) > 0).any(), "both outcomes must occur"


# ---- 3. exact relations to the verdict -----------------------------------------------------------------------------------

def test_relations_to_the_verdict(wam, iterated):
    mod, it = wam["mod"], iterated
    full = it["full"]
    verdict = mod.batch_collision_verdict(it["bid"], on_device=True, runs=np.ones(N_RUNS, dtype=bool))
    both = np.flatnonzero((full["n_samples"] >= 0) & (verdict["collides"] >= 0))
    assert len(both) >= N_RUNS - 4
    low = np.fmin(full["clearance"][:, 0], full["clearance"][:, 1])
    n_equal = 0
    for k in both:
        assert (low[k] < 0) == (verdict["collides"][k] == 1), k
        assert full["n_samples"][k] == verdict["n_samples"][k], k
        if verdict["collides"][k] == 1:
            assert low[k] <= -verdict["depth"][k], (k, low[k], verdict["depth"][k])
            res = it["res"][k]
            fc = CL.first_contact(res)
            if not it["aside"][k] and fc is not None and -fc[3] == min(res["clearance"]):      # the first contact is the deepest
                assert low[k] == -verdict["depth"][k], (k, low[k], verdict["depth"][k])
                n_equal += 1
    assert (verdict["collides"][both] == 1).any() and (verdict["collides"][both] == 0).any()
    print("colliding runs %d, of them with the first contact the deepest %d" % ((verdict["collides"][both] == 1).sum(), n_equal))


# ---- 4. variants -----------------------------------------------------------------------------------------------------------

def check_variant(mod, bid, tab, vmax, col0, fields_of_run, check=assert_run_fp64, n_iter=5, self_check=True, **kw):
    """iterate a little, then every run against its restatement; returns (device result, restatements)"""
    if n_iter:
        mod.batch_iterate(bid, n_iter)
    traj = mod.batch_gettraj(bid)
    got = mod.batch_clearance(bid, **kw)
    out, n_aside, n_tied = [], 0, 0
    for k in range(len(traj)):
        res = CL.restate(tab, traj[k], vmax, col0, fields_of_run(k), self_check=self_check)
        out.append(res)
        if CL.set_aside(res, fields_of_run(k)):
            n_aside += 1
            continue
        n_tied += check(got, k, res)
    print("set aside by the face premise: %d of %d; minima with another item within the tolerance: %d" % (n_aside, len(traj), n_tied))
    assert n_aside <= 1
    return got, out


def test_floating_base(oracle):
    """columns 0..6 are the base pose; the robot stands 20 cm further from the table (tests/test_gpu_verdict_device.py)"""
    mod = or_cdchomp_amd.Module(0)
    model, base, dofvals, adofs = common.wam_state()
    base = np.asarray(base, dtype=np.float64)
    base[0] -= 0.2
    mod.add_robot(model, transform=list(base), dof_values=dofvals, active_dofs=adofs)
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    vmax = set_wam_vmax(mod, model)
    n_runs = 8
    goals = wam_goals_with_table(n_runs, seed=77, k_table=2)
    basegoals = np.tile(base, (n_runs, 1))
    basegoals[:, :3] += [0.04, -0.03, 0.02]
    basegoals[:, 3:] += [0.05, 0.0, 0.03, 0.0]
    basegoals[:, 3:] /= np.linalg.norm(basegoals[:, 3:], axis=1)[:, None]
    bid = mod.batch_create(model.name, goals, basegoals=basegoals, **dict(KW, n_points=16, floating_base=1))
    assert mod.batch_dims(bid)[2] == 14
    field = product_field(oracle, mod, "table")
    tab = CL.Tables(oracle, model, base, dofvals, adofs, [field], floating=True)
    assert tab.active.all(), "with a floating base every sphere is active"
    check_variant(mod, bid, tab, vmax, 7, lambda k: [field])
    mod.batch_destroy(bid)
    mod.close()


def test_tree_robot(oracle):
    """the TREE instantiation: the 30-dof tree among three of config 5's bodies"""
    mod = or_cdchomp_amd.Module(0)
    model = robots.tree30()
    base, dofvals, adofs = [0.0] * 6 + [1.0], np.zeros(model.n_dof), list(range(model.n_dof))
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    names = []
    for name, (boxes, pose) in common.config5_bodies().items():
        if name != "box2":
            mod.add_kinbody_boxes(name, boxes, transform=pose)
            mod.SendCommand("computedistancefield kinbody %s cube_extent %f aabb_padding %f" % (name, common.CONFIG5_CUBE, common.CONFIG5_PADDING))
            names.append(name)
    vmax = np.linspace(0.5, 2.0, model.n_dof)
    mod.set_velocity_limits(model.name, vmax)
    bid = mod.batch_create(model.name, common.config5_goals(8), **dict(common.CONFIG5_KW, n_points=16))
    assert mod.batch_plan(bid)["variant"] & 1, "the robot must be a tree"
    fields = [product_field(oracle, mod, nm) for nm in names]
    tab = CL.Tables(oracle, model, base, dofvals, adofs, fields)
    got, res = check_variant(mod, bid, tab, vmax, 0, lambda k: fields, n_iter=3)
    print("fields at the minima:", sorted(set(got["other"][:, 0].tolist())))
    mod.batch_destroy(bid)
    mod.close()


def test_scene_batch_with_a_merged_field(oracle):
    """per-run scenes: the table and the mug, the two shifted, the empty scene, and the two merged into one field whose cells
    outside both sources hold +inf"""
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    mod.SendCommand("computedistancefield kinbody mug")
    vmax = set_wam_vmax(mod, model)
    mod.add_kinbody_boxes("merged", [], transform=[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    mod.merge_fields("merged", [("table", None), ("mug", None)], 0.04)
    shift = np.array([0.03, -0.04, 0.02, 0.0, 0.0, 0.0, 1.0])
    sc = [[("table", None), ("mug", None)], [("table", shift), ("mug", shift)], [("merged", None)], []]
    merged = product_field(oracle, mod, "merged")
    assert np.isposinf(merged.grid.data).any(), "the merged field must have cells without a source"
    fields = [[product_field(oracle, mod, "table"), product_field(oracle, mod, "mug")],
              [product_field(oracle, mod, "table", shift), product_field(oracle, mod, "mug", shift)], [merged], []]
    n_runs = 12
    goals = wam_goals_with_table(n_runs, seed=78, k_table=4)
    scene_of_run = (np.arange(n_runs) % len(sc)).astype(np.int32)
    bid = mod.batch_create(model.name, goals, scenes=sc, scene_of_run=scene_of_run, **dict(KW, n_points=16))
    _, base, dofvals, adofs = common.wam_state()
    tab = CL.Tables(oracle, model, base, dofvals, adofs, fields[0])
    got, res = check_variant(mod, bid, tab, vmax, 0, lambda k: fields[scene_of_run[k]])
    empty = np.flatnonzero(scene_of_run == 3)
    assert np.isposinf(got["clearance"][empty, 0]).all() and (got["other"][empty, 0] == -1).all(), "the empty scene has no field"
    assert np.isfinite(got["clearance"][empty, 1]).all()
    mod.batch_destroy(bid)
    mod.close()


def test_held_body(oracle):
    """the WAM with a four-sphere box in its hand: 19 active spheres, XML indices 16..19 the held ones"""
    mod = or_cdchomp_amd.Module(0)
    model, hand, pose = common.setup_product_wam_held4(mod)
    vmax = set_wam_vmax(mod, model)
    bid = mod.batch_create(model.name, wam_goals_with_table(8, seed=79, k_table=2), **dict(KW, n_points=16))
    _, base, dofvals, adofs = common.wam_state()
    field = product_field(oracle, mod, "table")
    tab = CL.Tables(oracle, model, base, dofvals, adofs, [field], held=[(hand, pose, common.HELD4_POS, common.HELD4_RAD)])
    assert tab.S == 20 and tab.active.sum() == 19
    got, res = check_variant(mod, bid, tab, vmax, 0, lambda k: [field])
    print("spheres at the field minima:", got["sphere"][:, 0].tolist())
    mod.batch_destroy(bid)
    mod.close()


def test_self_check_on_and_off(oracle):
    """the arm folds until the hand reaches the shoulder, far from any field: with the self check off there are no pairs"""
    mod = or_cdchomp_amd.Module(0)
    model, base, dofvals, adofs = common.wam_state()
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    mod.add_kinbody_boxes("far", [([0, 0, 0, 0, 0, 0, 1], [0.05, 0.05, 0.05])], transform=[5, 5, 5, 0, 0, 0, 1])
    mod.SendCommand("computedistancefield kinbody far")
    vmax = set_wam_vmax(mod, model)
    n_runs = 8
    goals = np.tile(np.asarray(robots.WAM_START), (n_runs, 1))
    goals[:, 3] = np.linspace(2.3, 3.05, n_runs)
    bid = mod.batch_create(model.name, goals, **dict(n_points=16, lambda_=100.0, obs_factor=0.0, obs_factor_self=0.0))
    field = product_field(oracle, mod, "far")
    tab = CL.Tables(oracle, model, base, dofvals, adofs, [field])
    on, _ = check_variant(mod, bid, tab, vmax, 0, lambda k: [field], n_iter=0)
    assert (on["clearance"][:, 1] < 0).any() and (on["clearance"][:, 1] > 0).any()
    assert np.isposinf(on["clearance"][:, 0]).all(), "nothing but the robot itself is near"
    mod.set_self_check(model.name, False)
    off, _ = check_variant(mod, bid, tab, vmax, 0, lambda k: [field], n_iter=0, self_check=False)
    assert np.isposinf(off["clearance"][:, 1]).all() and (off["sphere"][:, 1] == -1).all() and (off["time"][:, 1] == -1.0).all()
    assert np.array_equal(off["n_samples"], on["n_samples"])
    mod.set_self_check(model.name, True)
    assert_rows_equal(mod.batch_clearance(bid), on, np.arange(n_runs), "on again")
    mod.batch_destroy(bid)
    mod.close()


def fp32_depth_error(mod, bid, tab, field, vmax):
    """how FP32_DEPTH_ERR was measured: the fp32 verdict's depth against the restated first contact's (double, on the batch's
    float trajectories), the largest absolute difference over the colliding runs whose contact is the same item"""
    verdict = mod.batch_collision_verdict(bid, on_device=True, runs=np.ones(mod.batch_dims(bid)[0], dtype=bool))
    traj = mod.batch_gettraj(bid)
    worst, n = 0.0, 0
    for k in np.flatnonzero(verdict["collides"] == 1):
        fc = CL.first_contact(CL.restate(tab, traj[k], vmax, 0, [field]))
        if fc is not None and bits(fc[0]) == bits(verdict["time"][k]) and fc[1:3] == (verdict["sphere"][k], verdict["field"][k]):
            worst = max(worst, abs(fc[3] - verdict["depth"][k])); n += 1
    return worst, n


def test_precision_32(wam):
    """a precision 32 batch against the restatement in double on its float trajectories"""
    mod, model, vmax = wam["mod"], wam["model"], wam["vmax"]
    bid = mod.batch_create(model.name, wam_goals_with_table(12, seed=SEED, k_table=3), **dict(KW, n_points=20, precision=32))
    mod.batch_iterate(bid, 10)
    worst, n = fp32_depth_error(mod, bid, wam["tab"], wam["field"], vmax)
    print("fp32 verdict depth against the restatement: max abs difference %.3e over %d colliding runs (FP32_DEPTH_ERR %.3e)" % (worst, n, FP32_DEPTH_ERR))
    assert n >= 1 and FP32_TOL > 0.0
    got, res = check_variant(mod, bid, wam["tab"], vmax, 0, lambda k: [wam["field"]], check=assert_run_fp32, n_iter=0)
    traj = mod.batch_gettraj(bid)
    assert same(traj, traj.astype(np.float32)), "a precision 32 batch holds floats"
    assert (got["clearance"][:, 0] < 0).any()
    mod.batch_destroy(bid)


# ---- 5. subsets --------------------------------------------------------------------------------------------------------------

def test_subsets(wam, iterated):
    mod, it = wam["mod"], iterated
    full = it["full"]
    for name, mask in masks_of(N_RUNS).items():
        got = mod.batch_clearance(it["bid"], runs=mask, max_samples=CAP)
        assert_rows_equal(got, full, np.flatnonzero(mask), name)
        if (~mask).any():
            assert_not_walked(got, np.flatnonzero(~mask), -1, name)
    cand = candidates(it["costs"], it["status"])
    assert cand.any() and not cand.all()
    got = mod.batch_clearance(it["bid"], runs="candidates", max_samples=CAP)
    assert_rows_equal(got, full, np.flatnonzero(cand), "candidates")
    assert_not_walked(got, np.flatnonzero(~cand), -1, "candidates")
    assert_rows_equal(mod.batch_clearance(it["bid"], max_samples=CAP), full, np.arange(N_RUNS), "again")


# ---- 6. independence ---------------------------------------------------------------------------------------------------------

def test_a_run_does_not_depend_on_its_batch_or_shard(wam, wam2, iterated):
    it = iterated
    for m_, order, what in ((wam, np.arange(N_RUNS)[::-1], "reversed"), (wam2, np.arange(N_RUNS), "two shards")):
        mod, model = m_["mod"], m_["model"]
        bid = mod.batch_create(model.name, wam_goals_with_table(N_RUNS, seed=SEED)[order], **KW30)
        mod.batch_set_traj(bid, it["traj"][order])
        got = mod.batch_clearance(bid, max_samples=CAP)
        mod.batch_destroy(bid)
        assert_rows_equal({key: got[key][np.argsort(order)] for key in KEYS}, it["full"], np.arange(N_RUNS), what)


# ---- 7. select_clear -----------------------------------------------------------------------------------------------------------
N_GROUPS = 4
BY = ("total", "obs", "smooth", "clearance")


def assert_selection(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert np.array_equal(bits(got[1]), bits(want[1])), (what, got[1], want[1])
    assert np.array_equal(bits(got[2]), bits(want[2])), (what, got[2], want[2])
    assert np.array_equal(got[3], want[3]), (what, got[3], want[3])


def test_select_clear(wam, wam2, iterated):
    mod, it = wam["mod"], iterated
    bid, costs, status = it["bid"], it["costs"], it["status"]
    cand = candidates(costs, status)
    part = mod.batch_clearance(bid, runs="candidates", max_samples=CAP)
    low = np.fmin(part["clearance"][:, 0], part["clearance"][:, 1])
    contiguous = contiguous_groups(N_RUNS, N_GROUPS)
    shuffled = np.random.default_rng(5).permutation(contiguous).astype(np.int32)
    # a margin between two clearances of one group, chosen so that the group's winner by total cost does not clear it
    free = [g for g in range(N_GROUPS) if (cand & (contiguous == g) & (low >= 0)).sum() >= 2]
    assert free, "a group needs two free candidates"
    g0 = free[0]
    members = np.flatnonzero(cand & (contiguous == g0) & (low >= 0))
    winner = members[np.argmin(costs[members, 0])]
    others = members[low[members] > low[winner]]
    assert len(others), "the free winner of the group must not be its clearest run"
    between = 0.5 * (low[winner] + low[others].min())
    for margin in (-np.inf, 0.0, between, np.inf):
        for column, by in enumerate(BY):
            for grp in (contiguous, shuffled, None):
                got = mod.batch_select_clear(bid, groups=grp, n_groups=N_GROUPS, margin=margin, by=by, max_samples=CAP)
                want = select_clear(costs, status, part["clearance"], part["n_samples"], contiguous if grp is None else grp, N_GROUPS, margin, column)
                assert_selection(got[:4], want, (margin, by))
                assert np.array_equal(got[4], part["n_samples"])
        if margin == np.inf:
            assert (got[0] == -1).all() and np.isposinf(got[1]).all() and np.isnan(got[2]).all() and (got[3] == 0).all()
    at0 = mod.batch_select_clear(bid, n_groups=N_GROUPS, margin=0.0, by="total", max_samples=CAP)
    flip = mod.batch_select_clear(bid, n_groups=N_GROUPS, margin=between, by="total", max_samples=CAP)
    assert at0[0][g0] == winner and flip[0][g0] != winner and flip[0][g0] >= 0, "the margin must flip the group's winner"
    # margin 0 is require_collision_free
    mod.batch_set_verdict_scope(bid, "candidates")      # (a run that left its limits may be too long for the all-runs verdict)
    for column, by in enumerate(BY[:3]):
        for grp in (contiguous, shuffled):
            got = mod.batch_select_clear(bid, groups=grp, n_groups=N_GROUPS, margin=0.0, by=by, max_samples=CAP)
            ref = mod.batch_select_best(bid, groups=grp, n_groups=N_GROUPS, collision_free=True, by=by)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(bits(got[1]), bits(ref[1])) and np.array_equal(got[3], ref[2]), by
    mod.batch_set_verdict_scope(bid, "all")
    # one shard against two, with groups that span the shards
    mod2 = wam2["mod"]
    bid2, costs2, status2 = iterate_batch(mod2, wam2["model"])
    assert np.array_equal(bits(costs2), bits(costs)) and np.array_equal(status2, status)
    assert len(np.intersect1d(shuffled[:N_RUNS // 2], shuffled[N_RUNS // 2:])) > 0, "groups must span the shards"
    for margin in (0.0, between):
        for by in BY:
            one = mod.batch_select_clear(bid, groups=shuffled, n_groups=N_GROUPS, margin=margin, by=by, max_samples=CAP)
            two = mod2.batch_select_clear(bid2, groups=shuffled, n_groups=N_GROUPS, margin=margin, by=by, max_samples=CAP)
            assert_selection(two[:4], one[:4], (margin, by, "two shards"))
            assert np.array_equal(two[4], one[4])
    mod2.batch_destroy(bid2)


# ---- 8. rejected calls ----------------------------------------------------------------------------------------------------------

def test_rejected_calls(wam, iterated):
    mod, model, it = wam["mod"], wam["model"], iterated
    lib, h, bid = mod._lib, mod._h, it["bid"]
    dp, ip, up = _capi.c_double_p, _capi.c_int_p, _capi.c_ubyte_p
    clr = np.full((N_RUNS, 2), 7.0); ns = np.full(N_RUNS, 7, dtype=np.int32)
    ex = np.ones(N_RUNS, dtype=np.uint8); grp = contiguous_groups(N_RUNS, N_GROUPS).astype(np.int32)
    best = np.full(N_GROUPS, 7, dtype=np.int32)
    fresh = mod.batch_create(model.name, wam_goals_with_table(N_RUNS, seed=SEED), **KW30)      # never iterated
    cp, npp, exp, gp, bp = clr.ctypes.data_as(dp), ns.ctypes.data_as(ip), ex.ctypes.data_as(up), grp.ctypes.data_as(ip), best.ctypes.data_as(ip)
    bad_grp = grp.copy(); bad_grp[3] = N_GROUPS
    nan, d = float("nan"), C.c_double
    clearance = lambda b, which, e, cap, c=cp, n=npp: lib.orc_batch_clearance(h, b, which, e, cap, c, None, None, None, n)
    select = lambda b, col, ng, g, margin, cap: lib.orc_batch_select_clear(h, b, col, ng, g, d(margin), cap, bp, None, None, None, None)
    cases = {
        "unknown batch": lambda: clearance(bid + 1000, 2, None, 64),
        "which -1": lambda: clearance(bid, -1, None, 64), "which 3": lambda: clearance(bid, 3, None, 64),
        "which 0 without a mask": lambda: clearance(bid, 0, None, 64), "which 1 with a mask": lambda: clearance(bid, 1, exp, 64),
        "which 2 with a mask": lambda: clearance(bid, 2, exp, 64),
        "no clearance_out": lambda: clearance(bid, 2, None, 64, c=None), "no n_samples_out": lambda: clearance(bid, 2, None, 64, n=None),
        "max_samples 0": lambda: clearance(bid, 2, None, 0), "max_samples 2^20 + 1": lambda: clearance(bid, 2, None, (1 << 20) + 1),
        "candidates of a batch never iterated": lambda: clearance(fresh, 1, None, 64),
        "select: unknown batch": lambda: select(bid + 1000, 0, N_GROUPS, gp, 0.0, 64),
        "select: column -1": lambda: select(bid, -1, N_GROUPS, gp, 0.0, 64), "select: column 4": lambda: select(bid, 4, N_GROUPS, gp, 0.0, 64),
        "select: NaN margin": lambda: select(bid, 0, N_GROUPS, gp, nan, 64),
        "select: max_samples 0": lambda: select(bid, 0, N_GROUPS, gp, 0.0, 0), "select: max_samples 2^20 + 1": lambda: select(bid, 0, N_GROUPS, gp, 0.0, (1 << 20) + 1),
        "select: n_groups 0": lambda: select(bid, 0, 0, gp, 0.0, 64), "select: a group out of range": lambda: select(bid, 0, N_GROUPS, bad_grp.ctypes.data_as(ip), 0.0, 64),
        "select: n_runs % n_groups": lambda: select(bid, 0, 5, None, 0.0, 64),
        "select: a batch never iterated": lambda: select(fresh, 0, N_GROUPS, gp, 0.0, 64),
    }
    for name, call in cases.items():
        assert call() != 0, name
        assert lib.orc_last_error(h).decode(), name
        assert (clr == 7.0).all() and (ns == 7).all() and (best == 7).all(), name
        assert same(mod.batch_gettraj(bid), it["traj"]), name
        assert clearance(bid, 2, None, CAP) == 0, name
        assert np.array_equal(ns, it["full"]["n_samples"]) and np.array_equal(bits(clr), bits(it["full"]["clearance"])), name
        clr[:] = 7.0; ns[:] = 7
    assert select(bid, 3, N_GROUPS, gp, float("inf"), 64) == 0 and select(bid, 3, N_GROUPS, gp, float("-inf"), 64) == 0, "an infinite margin is accepted"
    mod.batch_destroy(fresh)


# ---- 9. too long -----------------------------------------------------------------------------------------------------------------

def test_too_long_runs_are_marked_and_the_call_returns(wam, iterated):
    mod, it = wam["mod"], iterated
    cap = 8
    long8 = np.array([clearance_too_long(it["traj"][k], wam["vmax"], 0, cap) for k in range(N_RUNS)])
    assert long8.sum() >= N_RUNS // 2, "most runs have more than a few samples"
    got = mod.batch_clearance(it["bid"], max_samples=cap)
    assert_not_walked(got, np.flatnonzero(long8), -2, "cap 8")
    if (~long8).any():
        assert_rows_equal(got, it["full"], np.flatnonzero(~long8), "cap 8: the short runs")
        assert (got["n_samples"][~long8] <= cap + 2).all()
    sel = mod.batch_select_clear(it["bid"], n_groups=N_GROUPS, margin=-np.inf, by="total", max_samples=cap)
    cand = candidates(it["costs"], it["status"])
    assert np.array_equal(sel[4][cand], np.where(long8, -2, it["full"]["n_samples"])[cand]) and (sel[4][~cand] == -1).all()
    want = select_clear(it["costs"], it["status"], got["clearance"], sel[4], contiguous_groups(N_RUNS, N_GROUPS), N_GROUPS, -np.inf, 0)
    assert_selection(sel[:4], want, "cap 8")
    assert sel[3].sum() == (cand & ~long8).sum(), "a run that is too long is not eligible"
