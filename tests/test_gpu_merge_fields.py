"""-m gpu: merged fields (orc_scene_merge_fields, Module.merge_fields, the mergefields command, scenes.merged_scenes).  The
kernel against the host twin bit for bit; more than ORC_MAX_SDFS sources; which kernel a merged scene runs; batches over a
merged field against the oracle on that grid; the kernel's buffer kept as the field's device copy; the rejections."""
import numpy as np
import pytest

import common
import merge_common as mc
import or_cdchomp_amd
from or_cdchomp_amd import bindings, scenes as scene_lib
from or_cdchomp_amd.module import pose_invert
from test_gpu_scenes import compose, mug_tilted, wam_scenes

pytestmark = pytest.mark.gpu

IDENT = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
KW = dict(n_points=30, lambda_=100.0, obs_factor=500.0)
N_ITER = 10
ORC_VAR_ONE_FIELD = 32
TURNED = [0.0, 0.0, 0.0, 0.0, 0.0, float(np.sin(0.15)), float(np.cos(0.15))]      # 0.3 rad about z


def empty_kinbody(mod, name, pose=IDENT):
    mod.add_kinbody_boxes(name, [], transform=pose)


def run_batch(mod, robot, goals, scenes, n_iter=N_ITER, **kw):
    bid = mod.batch_create(robot, goals, scenes=scenes, scene_of_run=np.zeros(len(goals), dtype=np.int32), **kw)
    costs, status = mod.batch_iterate(bid, n_iter)
    out = dict(costs=costs, status=status, traj=mod.batch_gettraj(bid), plan=mod.batch_plan(bid))
    mod.batch_destroy(bid)
    return out


def same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("costs", "status", "traj"))


# ---- device against host twin ------------------------------------------------------------------------------------------

def test_device_is_the_host_twin_bit_for_bit():
    sources, sizes, lengths, tpose = mc.three_sources()
    mod = or_cdchomp_amd.Module(0)
    fields = []
    for k, (data, slen, spose) in enumerate(sources):
        # the field's pose in its kinbody is the identity, so the grid's world pose is the kinbody's, exactly
        empty_kinbody(mod, "src%d" % k, spose if k != 1 else IDENT)
        mod.add_sdf("src%d" % k, data, slen, IDENT)
        fields.append(("src%d" % k, None if k != 1 else spose))       # (both forms: where it stands, and a pose given)
    empty_kinbody(mod, "merged", tpose)
    # bounds that end half a cell short of the 17 x 13 x 11 box: ceil gives those sizes whatever the division rounds to
    bounds = [0.0, 0.0, 0.0] + [(s - 0.5) * mc.CELL for s in sizes]
    mod.merge_fields("merged", fields, mc.CELL, bounds)
    got, glen, gpose = mod.get_sdf("merged")
    assert got.shape == tuple(sizes) == (17, 13, 11) and got.size == 2431
    assert list(glen) == [s * mc.CELL for s in sizes] and list(gpose) == IDENT
    want = mc.host_merge_fields(sources, sizes, list(glen), tpose)
    n_inf = int(np.isposinf(want).sum())
    assert 0 < n_inf < want.size and not np.isnan(want).any()
    assert np.array_equal(np.isposinf(got), np.isposinf(want))
    assert got.tobytes() == want.tobytes()
    mod.close()


# ---- the cap, the kernel choice, the oracle -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wam():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    mod.SendCommand("computedistancefield kinbody mug")
    yield dict(mod=mod, model=model, goals=common.wam_goals(8, seed=11))
    mod.close()


def test_twelve_fields_pass_the_cap_of_eight(wam):
    mod, model, goals = wam["mod"], wam["model"], wam["goals"]
    names = []
    for k in range(12):
        name = "shelf%d" % k
        pos = [0.35 + 0.12 * (k % 4), -0.3 + 0.2 * (k // 4), 0.9 + 0.05 * (k % 3)]
        mod.add_kinbody_boxes(name, [(IDENT, [0.04, 0.04, 0.04])], transform=pos + [0.0, 0.0, 0.0, 1.0])
        mod.SendCommand("computedistancefield kinbody %s cube_extent 0.04" % name)
        names.append(name)
    twelve = [(nm, None) for nm in names]
    with pytest.raises(RuntimeError, match="too many signed distance fields"):
        mod.batch_create(model.name, goals, scenes=[twelve], scene_of_run=np.zeros(len(goals), dtype=np.int32), **KW)
    empty_kinbody(mod, "merged12")
    mod.merge_fields("merged12", twelve, 0.04)
    data, _, _ = mod.get_sdf("merged12")
    assert np.isfinite(data).any() and float(data[np.isfinite(data)].min()) < 0.04      # a centre within a cell of a box
    got = run_batch(mod, model.name, goals, [[("merged12", None)]], **KW)
    assert np.isfinite(got["costs"]).all() and np.isin(got["status"], (0, -1)).all()
    if not common.plan_switches_active():
        assert got["plan"]["variant"] & ORC_VAR_ONE_FIELD
    # the twelve kinbodies stay out of the later tests' way: they are sources of explicit scenes only
    for nm in names + ["merged12"]:
        mod.SendCommand("removefield kinbody %s" % nm)


@pytest.fixture(scope="module")
def merged_pair(wam, oracle):
    """the table and the tilted mug merged with cell 0.04 into a target at the identity and into one turned 0.3 rad"""
    mod = wam["mod"]
    pair = [("table", None), ("mug", mug_tilted(oracle))]
    out = {}
    for name, kpose in (("merged", IDENT), ("merged_turned", TURNED)):
        empty_kinbody(mod, name, kpose)
        mod.merge_fields(name, pair, 0.04)
        data, lengths, gpose = mod.get_sdf(name)
        got = run_batch(mod, wam["model"].name, wam["goals"], [[(name, None)]], **KW)
        out[name] = dict(data=data, lengths=lengths, gpose=gpose, kpose=kpose, wpose=compose(oracle, kpose, gpose), got=got)
    return out


def test_kernel_choice_follows_the_targets_axes(merged_pair):
    assert list(merged_pair["merged"]["gpose"][3:]) == [0.0, 0.0, 0.0, 1.0]
    assert list(merged_pair["merged_turned"]["gpose"][3:]) == [0.0, 0.0, 0.0, 1.0]      # (the grid's axes are the kinbody's)
    if not common.plan_switches_active():      # (an ORC_* experiment switch: the plan is the switch's)
        assert merged_pair["merged"]["got"]["plan"]["variant"] & ORC_VAR_ONE_FIELD
        assert merged_pair["merged_turned"]["got"]["plan"]["variant"] & ORC_VAR_ONE_FIELD == 0


@pytest.mark.parametrize("name", ["merged", "merged_turned"])
def test_batches_over_the_merged_field_match_the_oracle_on_it(wam, merged_pair, oracle, name):
    """every run against the oracle given get_sdf(name) as its single grid: max(1e-6, CHAOS_FACTOR amp) in relative L2,
    costs to 1e-6 where amp < 1e-9, equal status where the oracle's is stable; no run is set aside"""
    m = merged_pair[name]
    goals = wam["goals"]
    _, base, dofvals, adofs = common.wam_state()
    rob = oracle.OraRobot(wam["model"])
    grid = oracle.OraGrid(m["data"], m["lengths"])
    ora = lambda g: oracle.batch_run(rob, base, dofvals, adofs, g, [grid], [m["wpose"]], oracle.default_params(**KW), N_ITER)
    res = ora(goals)
    amp, stable = common.amplification(ora, goals, res)
    otraj, ocosts, ost = res[0], res[1], res[2]
    got = m["got"]
    assert np.isfinite(got["costs"]).all() and np.isfinite(ocosts).all()
    for k in range(len(goals)):
        err = common.rel_l2(got["traj"][k], otraj[k])
        bar = max(1e-6, common.CHAOS_FACTOR * amp[k])
        print("%s run %d: rel L2 %.3e (bar %.3e, amp %.3e), status %d / %d" % (name, k, err, bar, amp[k], got["status"][k], ost[k]))
        assert err <= bar, (k, err, bar)
        if amp[k] < 1e-9:
            assert np.allclose(got["costs"][k], ocosts[k], rtol=1e-6, atol=0), (k, got["costs"][k], ocosts[k])
        if stable[k]:
            assert got["status"][k] == ost[k], (k, got["status"][k], ost[k])
    # at least one run's path crosses +inf cells of the merged grid: the spheres of the oracle's trajectory, in the grid's frame
    assert np.isposinf(m["data"]).any()
    qi = np.asarray(pose_invert(m["wpose"]))
    crossing = 0
    for k in range(len(goals)):
        run = oracle.OraRun(rob, base, dofvals, adofs, goals[k], [grid], [m["wpose"]], oracle.default_params(**KW))
        run.set_traj(otraj[k])
        _, _, P = run.eval_obstacle()
        run.destroy()
        x = (P.reshape(-1, 3) @ mc.rotation(qi[3:]).T + qi[:3]) / np.asarray(m["lengths"])
        inside = ((x >= 0) & (x <= 1)).all(axis=1)
        idx = np.minimum(np.floor(x[inside] * np.asarray(m["data"].shape)).astype(int), np.asarray(m["data"].shape) - 1)
        crossing += int(np.isposinf(m["data"][idx[:, 0], idx[:, 1], idx[:, 2]]).any())
    assert crossing >= 1


def test_kernel_buffer_is_the_fields_device_copy(wam, merged_pair):
    """a batch over the merged field reads the kernel's output buffer, kept as the field's fp64 copy; the same data re-added
    with add_sdf to a second empty kinbody at the same pose is an upload of the host copy: the same bits"""
    mod = wam["mod"]
    for name in ("merged", "merged_turned"):
        m = merged_pair[name]
        twin = name + "_twin"
        empty_kinbody(mod, twin, m["kpose"])
        mod.add_sdf(twin, m["data"], m["lengths"], m["gpose"])
        again = run_batch(mod, wam["model"].name, wam["goals"], [[(twin, None)]], **KW)
        assert same_bits(again, m["got"]), name
        assert again["plan"] == m["got"]["plan"]
        mod.SendCommand("removefield kinbody %s" % twin)


def test_merged_scenes_in_one_batch(wam, oracle):
    """three two-field scenes merged and run in one batch: every run is the run of a one-scene batch over its scene's field"""
    mod, model, goals = wam["mod"], wam["model"], wam["goals"]
    scenes = wam_scenes(oracle)[:3]
    assert all(len(sc) == 2 for sc in scenes)
    merged = scene_lib.merged_scenes(mod, scenes + [[]], 0.04, prefix="baked")
    assert merged == [[("baked0", None)], [("baked1", None)], [("baked2", None)], []]
    merged = merged[:3]
    n_runs = len(goals) * 3
    scene_of_run = np.arange(n_runs) % 3
    run_goals = goals[np.arange(n_runs) // 3]
    bid = mod.batch_create(model.name, run_goals, scenes=merged, scene_of_run=scene_of_run, **KW)
    costs, status = mod.batch_iterate(bid, N_ITER)
    traj = mod.batch_gettraj(bid)
    plan = mod.batch_plan(bid)
    mod.batch_destroy(bid)
    if not common.plan_switches_active():
        assert plan["variant"] & ORC_VAR_ONE_FIELD
    # the scenes are told apart: (b) is (a) shifted as a whole -- the same cells at another pose --, (c) has other cells
    baked = [mod.get_sdf("baked%d" % s) for s in range(3)]
    assert list(baked[0][2]) != list(baked[1][2]) and baked[0][0].tobytes() != baked[2][0].tobytes()
    assert costs[scene_of_run == 0].tobytes() != costs[scene_of_run == 1].tobytes()
    for s in range(3):
        idx = np.flatnonzero(scene_of_run == s)
        one = run_batch(mod, model.name, run_goals[idx], [merged[s]], **KW)
        assert one["traj"].tobytes() == traj[idx].tobytes(), s
        assert one["costs"].tobytes() == costs[idx].tobytes() and one["status"].tobytes() == status[idx].tobytes(), s
    for s in range(3):
        mod.SendCommand("removefield kinbody baked%d" % s)


# ---- errors and the command ---------------------------------------------------------------------------------------------

def test_every_rejection_and_the_module_afterwards(wam):
    mod, model, goals = wam["mod"], wam["model"], wam["goals"]
    empty_kinbody(mod, "bare")                       # a kinbody without a field
    empty_kinbody(mod, "target")
    nan, inf = float("nan"), float("inf")
    pair = [("table", None), ("mug", None)]
    bad_pose = lambda v: [("table", None), ("mug", v)]
    cases = [
        (("target", [], 0.04, None), "n_fields must be >=1"),
        (("target", [("nobody", None)], 0.04, None), "Could not find kinbody"),
        (("nobody", pair, 0.04, None), "Could not find kinbody"),
        (("target", [("table", None), ("bare", None)], 0.04, None), "has no signed distance field"),
        (("target", [("table", None), ("target", None)], 0.04, None), "target kinbody is among"),
        (("table", [("mug", None)], 0.04, None), "already have an sdf"),
        (("target", pair, 0.0, None), "cell must be"),
        (("target", pair, -0.04, None), "cell must be"),
        (("target", pair, nan, None), "cell must be"),
        (("target", pair, inf, None), "cell must be"),
        (("target", bad_pose([0.0, nan, 0.0, 0.0, 0.0, 0.0, 1.0]), 0.04, None), "finite"),
        (("target", bad_pose([0.0, 0.0, inf, 0.0, 0.0, 0.0, 1.0]), 0.04, None), "finite"),
        (("target", bad_pose([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]), 0.04, None), "zero norm"),
        (("target", pair, 0.04, [0.0, 0.0, 0.0, 1.0, nan, 1.0]), "finite"),
        (("target", pair, 0.04, [0.0, 0.0, 0.0, 1.0, 0.0, 1.0]), "lo < hi"),
        (("target", pair, 0.04, [0.0, 0.0, 2.0, 1.0, 1.0, 1.0]), "lo < hi"),
        (("target", pair, 1e-4, None), "signed distance field too large for this build!"),
        (("target", pair, 1e-9, [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]), "signed distance field too large for this build!"),
    ]
    for args, message in cases:
        with pytest.raises(RuntimeError, match=message):
            mod.merge_fields(*args)
        with pytest.raises(RuntimeError, match="No sdf for that kinbody"):      # no state changed: the target has no field
            mod.get_sdf("target" if args[0] != "nobody" else "bare")
    # a robot is no target
    with pytest.raises(RuntimeError, match="Could not find kinbody"):
        mod.merge_fields(model.name, pair, 0.04)
    table_before = mod.get_sdf("table")[0].tobytes()
    # ... and the module still merges and runs a batch
    mod.merge_fields("target", pair, 0.04)
    got = run_batch(mod, model.name, goals, [[("target", None)]], **KW)
    assert np.isfinite(got["costs"]).all()
    assert mod.get_sdf("table")[0].tobytes() == table_before
    # the field is a snapshot: moving a source afterwards changes no cell of it
    snap = mod.get_sdf("target")[0].tobytes()
    mod.set_kinbody_transform("mug", [0.3, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    assert mod.get_sdf("target")[0].tobytes() == snap
    mod.set_kinbody_transform("mug", IDENT)
    with pytest.raises(RuntimeError, match="already have an sdf"):
        mod.merge_fields("target", pair, 0.04)
    mod.SendCommand("removefield kinbody target")


def test_command_gives_the_grid_of_the_call(wam):
    mod = wam["mod"]
    bounds = [-0.3, -0.4, 0.5, 0.5, 0.4, 1.1]
    for k, bd in enumerate((None, bounds)):
        a, b = "by_call%d" % k, "by_command%d" % k
        empty_kinbody(mod, a); empty_kinbody(mod, b)
        mod.merge_fields(a, [("table", None), ("mug", None)], 0.037, bd)
        cmd = "mergefields kinbody %s fields 'table mug' cell 0.037" % b
        if bd is not None:
            cmd += " bounds '%s'" % " ".join(repr(v) for v in bd)
        assert mod.SendCommand(cmd) == ""
        da, la, pa = mod.get_sdf(a)
        db, lb, pb = mod.get_sdf(b)
        assert da.shape == db.shape and da.tobytes() == db.tobytes() and list(la) == list(lb) and list(pa) == list(pb)
        mod.SendCommand("removefield kinbody %s" % a)
        mod.SendCommand("removefield kinbody %s" % b)
    # the keyword front end emits the same command
    empty_kinbody(mod, "by_binding")
    bound = bindings.bind(mod)
    assert bound.mergefields(kinbody="by_binding", fields=["table", "mug"], cell=0.037, bounds=bounds) == ""
    empty_kinbody(mod, "by_call")
    mod.merge_fields("by_call", [("table", None), ("mug", None)], 0.037, bounds)
    assert mod.get_sdf("by_binding")[0].tobytes() == mod.get_sdf("by_call")[0].tobytes()
    for nm in ("by_binding", "by_call"):
        mod.SendCommand("removefield kinbody %s" % nm)
    empty_kinbody(mod, "cmd_target")
    for cmd in ("mergefields kinbody cmd_target fields 'table mug' cell 0.04 nonsense",
                "mergefields kinbody cmd_target fields 'table mug' cell",
                "mergefields kinbody cmd_target fields 'table mug' cell 0.04 bounds",
                "mergefields cell 0.04 extra 1"):
        with pytest.raises(RuntimeError, match="Bad arguments!"):
            mod.SendCommand(cmd)
    with pytest.raises(RuntimeError, match="Did not pass all required args!"):
        mod.SendCommand("mergefields kinbody cmd_target fields 'table mug'")
    with pytest.raises(RuntimeError, match="bounds must be length 6!"):
        mod.SendCommand("mergefields kinbody cmd_target fields 'table mug' cell 0.04 bounds '0 0 0 1 1'")
    # the error texts are those of the C call
    empty_kinbody(mod, "cmd_bare")
    with pytest.raises(RuntimeError, match="Kinbody cmd_bare has no signed distance field!"):
        mod.SendCommand("mergefields kinbody cmd_target fields 'table cmd_bare' cell 0.04")
    with pytest.raises(RuntimeError, match="cell must be a positive finite number!"):
        mod.SendCommand("mergefields kinbody cmd_target fields 'table mug' cell -1")
