"""-m gpu: per-run scenes (orc_batch_create_scenes, Module.batch_create(scenes=..., scene_of_run=...)): one batch of CHOMP runs over
several obstacle layouts.  Every scene's runs are checked against the oracle run on that scene's grids and world poses; a batch of
one scene that is the module's fields as they stand is the plain batch bit for bit; runs do not depend on what shares the batch."""
import re

import numpy as np
import pytest

import common
import or_cdchomp_amd
from or_cdchomp_amd import robots, scenes as scene_lib

pytestmark = pytest.mark.gpu

KW = dict(n_points=100, lambda_=100.0, obs_factor=500.0)
N_ITER = 100
IDENT = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
FAR = np.array([100.0, 100.0, 100.0, 0.0, 0.0, 0.0, 1.0])     # a field no sphere reaches: the oracle's stand-in for an empty scene


def compose(oracle, a, b):
    out = np.zeros(7)
    oracle.lib().ora_kin_pose_compose(oracle.dp(oracle.f64(a)), oracle.dp(oracle.f64(b)), oracle.dp(out))
    return out


def mug_tilted(oracle):
    """the mug kinbody turned 0.5 rad about a horizontal axis through its centre: its field is not axis-aligned"""
    ax = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    rot = np.concatenate([[0.0, 0.0, 0.0], ax * np.sin(0.25), [np.cos(0.25)]])
    c = np.array(scene_lib.tabletop_boxes()["mug"][0][0][:3])
    return compose(oracle, np.concatenate([c, [0, 0, 0, 1]]), compose(oracle, rot, np.concatenate([-c, [0, 0, 0, 1]])))


def wam_scenes(oracle):
    shift = np.array([0.03, -0.04, 0.02, 0.0, 0.0, 0.0, 1.0])
    return [
        [("table", None), ("mug", None)],                 # (a) where they stand
        [("table", shift), ("mug", shift)],               # (b) both shifted by a few cm
        [("table", None), ("mug", mug_tilted(oracle))],   # (c) the mug tilted
        [("table", IDENT)],                               # (d) table only
        [],                                               # (e) empty
    ]


class Fields:
    """the module's fields as the oracle takes them: grid, and the field's pose in its kinbody's frame"""

    def __init__(self, mod, oracle, names):
        self.grid, self.gpose = {}, {}
        for name in names:
            data, lengths, gpose = mod.get_sdf(name)
            self.grid[name] = oracle.OraGrid(data, lengths)
            self.gpose[name] = np.asarray(gpose, dtype=np.float64)

    def oracle_scene(self, mod, oracle, scene):
        """(grids, world poses) of a scene for the oracle; an empty scene gets one field far out of reach (no cost, no contact)"""
        if not scene:
            name = next(iter(self.grid))
            return [self.grid[name]], [FAR]
        grids, poses = [], []
        for name, pose in scene:
            kpose = mod.body_transform(name) if pose is None else pose
            grids.append(self.grid[name])
            poses.append(compose(oracle, kpose, self.gpose[name]))
        return grids, poses


def wam_module(devices=0):
    mod = or_cdchomp_amd.Module(devices)
    model = common.setup_product_wam(mod)
    mod.SendCommand("computedistancefield kinbody mug")
    return mod, model


def run_batch(mod, robot, goals, n_iter, **kw):
    bid = mod.batch_create(robot, goals, **kw)
    costs, status = mod.batch_iterate(bid, n_iter)
    out = dict(costs=costs, status=status, traj=mod.batch_gettraj(bid), trace=mod.batch_trace(bid, n_iter), plan=mod.batch_plan(bid))
    mod.batch_destroy(bid)
    return out


def check_against_oracle(oracle, got, idx, ora, goals, tol=1e-6, cost_rtol=1e-6):
    """the runs `idx` of `got` against `ora(goals)` (the oracle on their scene), well-conditioned runs to the bars of
    test_gpu_configs / test_gpu_held4; returns the number of well-conditioned runs"""
    res = ora(goals)
    amp, stable = common.amplification(ora, goals, res)
    otraj, ocosts, ost = res[0], res[1], res[2]
    st = got["status"][idx]
    well = (ost == 0) & (st == 0) & (amp < 1e-9) & stable
    for j in np.flatnonzero(well):
        k = idx[j]
        assert common.rel_l2(got["traj"][k], otraj[j]) <= tol, (k, common.rel_l2(got["traj"][k], otraj[j]))
        assert np.allclose(got["costs"][k], ocosts[j], rtol=cost_rtol, atol=0), (k, got["costs"][k], ocosts[j])
    # a status that differs belongs to a run the oracle itself moves under a one-ulp change of its goal
    assert all(amp[j] >= 1e-9 or not stable[j] for j in np.flatnonzero(ost != st)), (ost, st, amp)
    return int(well.sum()), res, well


@pytest.fixture(scope="module")
def wam5(oracle):
    mod, model = wam_module()
    fields = Fields(mod, oracle, ["table", "mug"])
    scenes = wam_scenes(oracle)
    goals = common.wam_goals(8, seed=11)
    n_runs = len(goals) * len(scenes)
    scene_of_run = np.arange(n_runs) % len(scenes)
    run_goals = goals[np.arange(n_runs) // len(scenes)]
    got = run_batch(mod, model.name, run_goals, N_ITER, scenes=scenes, scene_of_run=scene_of_run, **KW)
    yield dict(mod=mod, model=model, fields=fields, scenes=scenes, goals=goals, run_goals=run_goals, scene_of_run=scene_of_run, got=got)
    mod.close()


def test_wam_five_scenes_match_the_oracle(wam5, oracle):
    """five obstacle layouts in one batch, each goal once in every scene (interleaved): status, costs, trace and trajectories
    of every scene's runs against the oracle on that scene"""
    w = wam5; mod = w["mod"]
    _, base, dofvals, adofs = common.wam_state()
    rob = oracle.OraRobot(w["model"])
    otrajs, ostat = {}, {}
    n_well = 0
    for s, scene in enumerate(w["scenes"]):
        grids, poses = w["fields"].oracle_scene(mod, oracle, scene)
        ora = lambda g: oracle.batch_run(rob, base, dofvals, adofs, g, grids, poses, oracle.default_params(**KW), N_ITER)
        idx = np.flatnonzero(w["scene_of_run"] == s)
        nw, res, well = check_against_oracle(oracle, w["got"], idx, ora, w["run_goals"][idx])
        n_well += nw
        otrajs[s], ostat[s] = res[0], res[2]
        # the per-iteration trace of the well-conditioned runs
        for j in np.flatnonzero(well)[:3]:
            k = idx[j]
            run = oracle.OraRun(rob, base, dofvals, adofs, w["run_goals"][k], grids, poses, oracle.default_params(**KW))
            st, _, otr = run.iterate(N_ITER, trace=True)
            run.destroy()
            assert st == 0
            assert np.allclose(w["got"]["trace"][k], otr, rtol=1e-6, atol=0), k
    assert n_well >= 12, n_well
    # the scenes are told apart: the oracle's trajectories of one goal differ between (a) and (b), and between (a) and (e)
    both = [g for g in range(len(w["goals"])) if ostat[0][g] == 0 and ostat[1][g] == 0 and ostat[4][g] == 0]
    assert len(both) >= 3, ostat
    for g in both:
        assert common.rel_l2(otrajs[1][g], otrajs[0][g]) > 1e-4, g
        assert common.rel_l2(otrajs[4][g], otrajs[0][g]) > 1e-4, g
    print("five scenes: %d of %d runs well-conditioned and within 1e-6 of the oracle" % (n_well, len(w["run_goals"])))


@pytest.mark.parametrize("precision", [64, 32])
def test_one_scene_is_the_plain_batch(wam5, precision):
    """one scene that is the module's fields where they stand, every run in it: the plain batch bit for bit, the same plan"""
    w = wam5; mod = w["mod"]
    goals = common.wam_goals(16, seed=23)
    kw = dict(KW, precision=precision)
    plain = run_batch(mod, w["model"].name, goals, 50, **kw)
    one = [[("table", None), ("mug", None)]]
    sc = run_batch(mod, w["model"].name, goals, 50, scenes=one, scene_of_run=np.zeros(len(goals), dtype=np.int32), **kw)
    for key in ("traj", "costs", "status", "trace"):
        assert np.array_equal(plain[key], sc[key], equal_nan=True), key
    assert plain["plan"] == sc["plan"]


def test_runs_are_independent_of_the_batch(wam5):
    """a permuted subset with the same scene table reproduces the full batch's rows bit for bit; so do in-process shards"""
    w = wam5; mod = w["mod"]
    n_runs = len(w["run_goals"])
    pick = np.random.default_rng(9).permutation(n_runs)[:23]
    sub = run_batch(mod, w["model"].name, w["run_goals"][pick], N_ITER, scenes=w["scenes"], scene_of_run=w["scene_of_run"][pick], **KW)
    for key in ("traj", "costs", "status", "trace"):
        assert np.array_equal(sub[key], w["got"][key][pick], equal_nan=True), key
    mod2, model2 = wam_module([0, 0])
    try:
        sh = run_batch(mod2, model2.name, w["run_goals"], N_ITER, scenes=w["scenes"], scene_of_run=w["scene_of_run"], **KW)
    finally:
        mod2.close()
    for key in ("traj", "costs", "status", "trace"):
        assert np.array_equal(sh[key], w["got"][key], equal_nan=True), key


@pytest.mark.parametrize("precision,tol", [(64, 1e-6), (32, 1e-3)])
def test_tree30_two_scenes_of_four_and_two_fields(oracle, precision, tol):
    """the many-sphere path (descriptors loaded four at a time) with scenes of 4 and 2 fields, rearranged and moved"""
    mod = or_cdchomp_amd.Module(0)
    model = robots.tree30()
    base = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    dofvals = np.zeros(model.n_dof)
    adofs = list(range(model.n_dof))
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    rng = np.random.default_rng(20250104)
    names = []
    for name, (boxes, pose) in scene_lib.random_boxes(rng).items():
        mod.add_kinbody_boxes(name, boxes, transform=pose)
        mod.SendCommand("computedistancefield kinbody %s cube_extent 0.02 aabb_padding 0.15" % name)
        names.append(name)
    fields = Fields(mod, oracle, names)
    prng = np.random.default_rng(77)

    def moved(name):
        p = np.asarray(mod.body_transform(name), dtype=np.float64).copy()
        p[:3] += prng.uniform(-0.15, 0.15, 3)
        return p

    scenes = [[(names[2], None), (names[0], moved(names[0])), (names[3], None), (names[1], moved(names[1]))],
              [(names[1], moved(names[1])), (names[2], moved(names[2]))]]
    n_runs, n_iter = 4, 20
    goals = np.random.default_rng(5).uniform(-0.8, 0.8, size=(n_runs, model.n_dof))
    scene_of_run = np.array([0, 1, 1, 0])
    kw = dict(n_points=40, lambda_=200.0, obs_factor=100.0)
    got = run_batch(mod, model.name, goals, n_iter, scenes=scenes, scene_of_run=scene_of_run, precision=precision, **kw)
    rob = oracle.OraRobot(model)
    errs = []
    for k in range(n_runs):
        grids, poses = fields.oracle_scene(mod, oracle, scenes[scene_of_run[k]])
        run = oracle.OraRun(rob, base, dofvals, adofs, goals[k], grids, poses, oracle.default_params(**kw))
        st, ocosts = run.iterate(n_iter)
        assert st == 0 and got["status"][k] == 0
        errs.append(common.rel_l2(got["traj"][k], run.traj()))
        assert np.allclose(got["costs"][k], ocosts, rtol=1e-6 * (100 if precision == 32 else 1), atol=0), (k, got["costs"][k], ocosts)
        run.destroy()
    mod.close()
    assert max(errs) <= tol, errs


def test_held4_pair_list_two_scenes(oracle):
    """the 17-32 sphere family (dense pair list) with two scenes, fp64"""
    mod = or_cdchomp_amd.Module(0)
    model, hand, pose = common.setup_product_wam_held4(mod)
    mod.SendCommand("computedistancefield kinbody mug")
    fields = Fields(mod, oracle, ["table", "mug"])
    scenes = [[("table", None), ("mug", None)], [("mug", mug_tilted(oracle)), ("table", np.array([0.0, 0.05, -0.03, 0, 0, 0, 1]))]]
    goals = common.wam_goals(6, seed=31)
    run_goals = np.repeat(goals, 2, axis=0)
    scene_of_run = np.tile([0, 1], len(goals))
    kw = dict(common.CONFIG2_KW)
    got = run_batch(mod, model.name, run_goals, N_ITER, scenes=scenes, scene_of_run=scene_of_run, **kw)
    assert got["plan"]["variant"] & 512, got["plan"]
    _, base, dofvals, adofs = common.wam_state()
    rob = oracle.OraRobot(model, grabbed=[(hand, pose, common.HELD4_POS, common.HELD4_RAD)])
    n_well = 0
    for s, scene in enumerate(scenes):
        grids, poses = fields.oracle_scene(mod, oracle, scene)
        ora = lambda g: oracle.batch_run(rob, base, dofvals, adofs, g, grids, poses, oracle.default_params(**kw), N_ITER)
        idx = np.flatnonzero(scene_of_run == s)
        n_well += check_against_oracle(oracle, got, idx, ora, run_goals[idx])[0]
    mod.close()
    assert n_well >= 4, n_well


def test_floating_base_momentum_hmc_two_scenes(oracle, monkeypatch):
    """momentum + hmc resampling, seeded, over two scenes: the per-run noise is indexed by run, not by scene"""
    monkeypatch.setenv("ORC_HMC_HOST", "1")
    mod, model = wam_module()
    fields = Fields(mod, oracle, ["table", "mug"])
    _, base, dofvals, adofs = common.wam_state()
    n_runs, n_iter = 4, 40
    rng = np.random.default_rng(20250103)
    goals = common.wam_goals(n_runs, seed=20250103)
    basegoals = np.tile(np.asarray(base), (n_runs, 1))
    basegoals[:, :3] += rng.uniform(-0.3, 0.3, size=(n_runs, 3))
    seeds = np.arange(n_runs, dtype=np.uint32) + 3
    kw = dict(n_points=60, lambda_=100.0, obs_factor=500.0, floating_base=1, use_momentum=1, use_hmc=1, hmc_resample_lambda=0.02)
    scenes = [[("mug", None)], [("table", None), ("mug", np.array([-0.1, 0.05, 0.0, 0, 0, 0, 1]))]]
    scene_of_run = np.array([1, 0, 0, 1])
    bid = mod.batch_create(model.name, goals, basegoals=basegoals, seeds=seeds, scenes=scenes, scene_of_run=scene_of_run, **kw)
    costs, status = mod.batch_iterate(bid, n_iter)
    traj = mod.batch_gettraj(bid)
    trace = mod.batch_trace(bid, n_iter)
    mod.batch_destroy(bid)
    rob = oracle.OraRobot(model)
    errs = []
    for k in range(n_runs):
        grids, poses = fields.oracle_scene(mod, oracle, scenes[scene_of_run[k]])
        run = oracle.OraRun(rob, base, dofvals, adofs, goals[k], grids, poses, oracle.default_params(seed=int(seeds[k]), **kw),
                            basegoal=basegoals[k])
        st, ocosts, otr = run.iterate(n_iter, trace=True)
        assert st == 0 and status[k] == 0
        errs.append(common.rel_l2(traj[k], run.traj()))
        assert np.allclose(costs[k], ocosts, rtol=1e-6, atol=0), (k, costs[k], ocosts)
        assert np.allclose(trace[k], otr, rtol=1e-6, atol=0), k
        run.destroy()
    mod.close()
    assert max(errs) <= 1e-6, errs


# a straight trajectory of the WAM from its start that runs into the tabletop in scene (a) and is clear of everything
# when the scene is empty (found with the oracle's re-check)
VERDICT_GOAL = [-2.071754164281878, -1.0001200749348211, 1.6268821121145431, 1.4122157370445974, -4.114053875005685,
                -0.2006191792905785, -0.12150247078316267]


def test_collision_verdict_per_scene(wam5, oracle):
    """every run's straight trajectory against its own scene: the device verdict (orc_batch_collision_verdict and
    gettrajbatch ... verdict) matches the oracle's re-check on that scene; gettraj's host re-check walks the run's scene"""
    w = wam5; mod = w["mod"]; model = w["model"]
    _, base, dofvals, adofs = common.wam_state()
    vmax = np.ones(model.n_dof)
    mod.set_velocity_limits(model.name, vmax)
    kw = dict(n_points=40, lambda_=100.0, obs_factor=500.0)
    start = np.asarray(robots.WAM_START)
    goal = np.asarray(VERDICT_GOAL)
    straight = start[None, :] + np.linspace(0.0, 1.0, kw["n_points"])[:, None] * (goal - start)[None, :]
    # the scenes of test 1 and the two fields in the other order (a field index that is not the module's)
    scenes = w["scenes"] + [[("mug", None), ("table", None)]]
    n_runs = 2 * len(scenes)
    scene_of_run = np.arange(n_runs) % len(scenes)
    goals = np.tile(goal, (n_runs, 1))
    bid = mod.batch_create(model.name, goals, scenes=scenes, scene_of_run=scene_of_run, **kw)
    mod.batch_set_traj(bid, np.tile(straight, (n_runs, 1, 1)))
    got = mod.batch_collision_verdict(bid)
    out = np.zeros((n_runs, kw["n_points"], 7)); ver = np.zeros(n_runs, dtype=np.int32)
    mod.SendCommand("gettrajbatch run %d out 0x%x verdict 0x%x" % (bid, out.ctypes.data, ver.ctypes.data))
    mod.batch_destroy(bid)
    assert np.array_equal(ver, got["collides"])
    rob = oracle.OraRobot(model)
    for k in range(n_runs):
        grids, poses = w["fields"].oracle_scene(mod, oracle, scenes[scene_of_run[k]])
        orun = oracle.OraRun(rob, base, dofvals, adofs, goal, grids, poses, oracle.default_params(**kw))
        orun.set_traj(straight)
        want = orun.collision_recheck(vmax[:7])
        orun.destroy()
        assert want["collides"] == got["collides"][k], (k, want, {q: got[q][k] for q in got})
        if want["collides"]:
            assert want["sphere"] == got["sphere"][k] and want["field"] == got["field"][k], (k, want, got["sphere"][k], got["field"][k])
            assert np.isclose(want["time"], got["time"][k], rtol=1e-12, atol=1e-15)
            assert np.isclose(want["depth"], got["depth"][k], rtol=1e-9, atol=1e-12)
    assert got["collides"][0] == 1 and got["collides"][4] == 0
    # gettraj of a one-run scene batch: collides in scene (a), not in scene (e)
    for s, collides in ((0, True), (4, False)):
        bid = mod.batch_create(model.name, goal, scenes=[scenes[s]], scene_of_run=[0], **kw)
        mod.batch_set_traj(bid, straight[None])
        if collides:
            with pytest.raises(RuntimeError, match="Resulting trajectory is in collision!"):
                mod.SendCommand("gettraj run %d" % bid)
            assert re.search(r"inside the field of table", mod.last_collision_details()), mod.last_collision_details()
        else:
            mod.SendCommand("gettraj run %d" % bid)
            assert mod.last_collision_details() == ""
        mod.batch_destroy(bid)


def test_malformed_scene_tables_are_rejected(wam5):
    """each malformed table fails with a message; the module stays usable"""
    w = wam5; mod = w["mod"]; robot = w["model"].name
    lib = mod._lib
    from or_cdchomp_amd import _capi
    import ctypes as C
    p = mod.batch_params(n_points=20)
    goals = common.wam_goals(2, seed=3)
    gp = goals.ctypes.data_as(_capi.c_double_p)

    def create(n_scenes, begin, names, scene_of_run):
        b = np.ascontiguousarray(begin, dtype=np.int32)
        s = np.ascontiguousarray(scene_of_run, dtype=np.int32)
        cn = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
        bid = C.c_int(0)
        rc = lib.orc_batch_create_scenes(mod._h, robot.encode(), C.byref(p), 2, None, gp, None, None, n_scenes,
                                         b.ctypes.data_as(_capi.c_int_p), cn, None, s.ctypes.data_as(_capi.c_int_p), C.byref(bid))
        msg = lib.orc_last_error(mod._h).decode() if rc != 0 else ""
        return rc, bid.value, msg

    mod.add_kinbody_boxes("nofield", [([0, 0, 0, 0, 0, 0, 1], [0.05, 0.05, 0.05])], transform=[3, 3, 3, 0, 0, 0, 1])
    bad = [
        ((0, [0], [], [0, 0]), "n_scenes"),
        ((1, [1, 1], ["table"], [0, 0]), "scene_begin"),
        ((2, [0, 1, 0], ["table"], [0, 0]), "scene_begin"),
        ((1, [0, 9], ["table"] * 9, [0, 0]), "too many signed distance fields"),
        ((1, [0, 1], ["nosuchbody"], [0, 0]), "nosuchbody"),
        ((1, [0, 1], ["nofield"], [0, 0]), "nofield"),
        ((2, [0, 1, 1], ["table"], [0, 2]), "scene_of_run"),
        ((2, [0, 1, 1], ["table"], [-1, 0]), "scene_of_run"),
    ]
    for args, what in bad:
        rc, _, msg = create(*args)
        assert rc != 0 and what in msg, (args, rc, msg)
        rc, bid, msg = create(2, [0, 2, 2], ["table", "table"], [1, 0])
        assert rc == 0, msg
        mod.batch_iterate(bid, 2)
        mod.batch_destroy(bid)
    with pytest.raises(RuntimeError, match="too many signed distance fields"):
        mod.batch_create(robot, goals, scenes=[[("mug", None)] * 9], scene_of_run=[0, 0], n_points=20)
