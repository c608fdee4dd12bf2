"""-m gpu: the plan of every case of a matrix equals the one recorded before `create` was split into stages.

tests/golden/plans_parent.json holds the nine numbers of Module.batch_plan for each case below, recorded on an MI355X with
the library of the commit BEFORE BatchShard::build_device was cut into fold_joint_tree / fold_robot / fold_tsrs /
fold_scenes / pack_metric / plan_iterate (csrc/fold.cpp, csrc/plan.cpp).  The planner's contract is that a plan is a
function of the robot, the run parameters and the module's settings: a case that gets other numbers now has been planned
differently, whatever its results look like.  `cases()` is also what the bit-for-bit comparison of the two libraries
walked (NOTES/stages.md)."""
import json
import os

import numpy as np
import pytest

import common
import or_cdchomp_amd
from or_cdchomp_amd import robots, scenes as scene_lib

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plans_parent.json")
BENCH_CONFIGS = (2, 3, 4, 5, "tsr1", "tsr3", "held4", "d2", "d3")


def _bench(config, streams=0, threads=0, per_cu=0, batch=64):
    """a workload of bench.py (a smaller batch: the plan does not read the batch)"""
    def make():
        import bench
        mod = or_cdchomp_amd.Module(0)
        if streams:
            mod.set_num_streams(streams)
        mod.set_workgroup_threads(threads)
        mod.set_workgroups_per_cu(per_cu)
        w = bench.Workload(config, 0, 1, batch)
        w.setup(mod)
        return mod, w.create(mod, 0, 0), w
    return make


def _wam(streams=0, threads=0, per_cu=0, n_runs=16, **kw):
    def make():
        mod = or_cdchomp_amd.Module(0)
        if streams:
            mod.set_num_streams(streams)
        mod.set_workgroup_threads(threads)
        mod.set_workgroups_per_cu(per_cu)
        model = common.setup_product_wam(mod)
        return mod, mod.batch_create(model.name, common.wam_goals(n_runs), **dict(common.CONFIG2_KW, **kw)), None
    return make


def _tree(precision, **kw):
    def make():
        mod = or_cdchomp_amd.Module(0)
        model = robots.tree30()
        mod.add_robot(model, transform=[0.0] * 6 + [1.0], dof_values=np.zeros(model.n_dof), active_dofs=list(range(model.n_dof)))
        for name, (boxes, pose) in scene_lib.random_boxes(np.random.default_rng(20250104)).items():
            mod.add_kinbody_boxes(name, boxes, transform=pose)
            mod.SendCommand("computedistancefield kinbody %s cube_extent 0.02 aabb_padding 0.15" % name)
        goals = np.random.default_rng(5).uniform(-0.8, 0.8, size=(8, model.n_dof))
        return mod, mod.batch_create(model.name, goals, precision=precision, **dict(dict(n_points=40, lambda_=200.0, obs_factor=100.0), **kw)), None
    return make


def _wam_tsr(start, con, n_points=30, streams=0, momentum=False):
    """the WAM with its hand held on a TSR at the start point (`start_tsr`) and / or its elbow height on every point (`con_tsr`)"""
    def make():
        mod = or_cdchomp_amd.Module(0)
        if streams:
            mod.set_num_streams(streams)
        model, _, dofvals, adofs = common.wam_state()
        s2 = float(np.sqrt(0.5))
        base = [-1.0, 0.0, 1.0, 0.0, s2, 0.0, s2]
        mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
        scene_lib.add_tabletop(mod)
        mod.SendCommand("computedistancefield kinbody table")
        R, t = model.link_frames(base, dofvals)
        hand, elbow = model.link_names.index("handbase"), model.link_names.index("wam4")
        goals = np.ascontiguousarray(np.array(robots.WAM_START)[None, :] + 0.3 * np.random.default_rng(11).uniform(-1, 1, size=(4, 7)))
        cmd = "createbatch robot %s n_runs 4 adofgoals 0x%x n_points %d lambda 100 obs_factor 200" % (model.name, goals.ctypes.data, n_points)
        if start:
            tsr = robots.Tsr(T0w_R=R[hand], T0w_d=t[hand] + R[hand] @ np.array([0, 0, 0.16]), Bw=[[0, 0], [0, 0], [0, 0], [-3, 3], [-3, 3], [-3, 3]])
            cmd += " start_tsr '%s'" % tsr.serialize()
        if con:
            tsr = robots.Tsr(T0w_R=R[elbow], T0w_d=t[elbow], Bw=[[-1, 1], [-1, 1], [0, 0], [-3, 3], [-3, 3], [-3, 3]])
            cmd += " con_tsr 'all link wam4' '%s'" % tsr.serialize()
        if momentum:
            cmd += " use_momentum"
        return mod, int(mod.SendCommand(cmd)), goals
    return make


def _two_fields(per_run):
    """the WAM over the table's and the mug's fields: the module's own scene, or three scenes of two, two and one field"""
    def make():
        mod = or_cdchomp_amd.Module(0)
        model = common.setup_product_wam(mod)
        mod.SendCommand("computedistancefield kinbody mug")
        goals = common.wam_goals(12, seed=11)
        if not per_run:
            return mod, mod.batch_create(model.name, goals, **common.CONFIG2_KW), None
        shift = np.array([0.03, -0.04, 0.02, 0.0, 0.0, 0.0, 1.0])
        table = [[("table", None), ("mug", None)], [("table", shift), ("mug", shift)], [("table", None)]]
        return mod, mod.batch_create(model.name, goals, scenes=table, scene_of_run=np.arange(12) % 3, **common.CONFIG2_KW), None
    return make


def _random_robot(seed):
    """the batch test_gpu_random_robots.test_random_robot_matches_oracle creates for `seed` (its draws, in its order)"""
    def make():
        import test_gpu_random_robots as rr
        rng = np.random.default_rng(5000 + seed)
        model, _ = rr.random_robot(seed)
        n_dof = model.n_dof
        if rng.uniform() < 0.35 and n_dof > 3:
            adofs = sorted(rng.choice(n_dof, size=int(rng.integers(2, n_dof)), replace=False).tolist())
        else:
            adofs = list(range(n_dof))
        lo = np.array([max(model.limit_lower[d], -1.5) for d in range(n_dof)])
        hi = np.array([min(model.limit_upper[d], 1.5) for d in range(n_dof)])
        dofvals = rng.uniform(0.5 * lo, 0.5 * hi)
        which = ("table", 2, 4, "table")[int(rng.integers(0, 4))]
        base = ([-0.55, 0.05, 0.75] if which == "table" else [0.05, -0.1, 0.35]) + list(rr._random_quat(rng, 0.7))
        floating = bool(rng.uniform() < 0.25)
        precision = 32 if rng.uniform() < 0.25 else 64
        momentum = bool(rng.uniform() < 0.3)
        second_order = bool(rng.uniform() < 0.12)
        hmc = momentum and bool(rng.uniform() < 0.4)
        long_traj = bool(rng.uniform() < 0.1)
        n_runs = (3, 3, 3, 40, 300)[int(rng.integers(0, 5))]
        n_points = int(rng.integers(100, 230)) if long_traj else int(rng.integers(5, 72))
        int(rng.integers(6, 16))                              # (the test's n_iter)
        kw = dict(n_points=n_points, lambda_=float(rng.uniform(120.0, 400.0)), obs_factor=float(rng.uniform(20.0, 200.0)),
                  obs_factor_self=float(rng.uniform(2.0, 20.0)), epsilon=float(rng.uniform(0.06, 0.14)),
                  epsilon_self=float(rng.uniform(0.02, 0.08)))
        if momentum:
            kw["use_momentum"] = 1
        if second_order:
            kw["derivative"] = 2
        if hmc:
            kw["use_hmc"] = 1
            kw["hmc_resample_lambda"] = float(rng.uniform(0.02, 0.3))
        seeds = rng.integers(0, 1000, size=n_runs).astype(np.uint32)
        if floating:
            kw["floating_base"] = 1
        shards = int(rng.integers(2, 4)) if rng.uniform() < 0.15 else 1
        mod = or_cdchomp_amd.Module([0] * shards if shards > 1 else 0)
        mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
        if which == "table":
            scene_lib.add_tabletop(mod)
            mod.SendCommand("computedistancefield kinbody table")
        else:
            for name, (boxes, pose) in scene_lib.random_boxes(np.random.default_rng(20250104), n_bodies=which).items():
                mod.add_kinbody_boxes(name, boxes, transform=pose)
                mod.SendCommand("computedistancefield kinbody %s cube_extent 0.02 aabb_padding 0.15" % name)
        threads = (0, 0, 192, 512)[int(rng.integers(0, 4))]
        per_cu = 4 if rng.uniform() < 0.3 and threads == 0 else 0
        mod.set_workgroup_threads(threads)
        if rng.uniform() < 0.2:
            mod.set_num_streams(2)
        mod.set_workgroups_per_cu(per_cu)
        goals = rng.uniform(0.7 * lo[adofs], 0.7 * hi[adofs], size=(n_runs, len(adofs)))
        basegoals = None
        if floating:
            basegoals = np.tile(np.asarray(base), (n_runs, 1)); basegoals[:, :3] += rng.uniform(-0.2, 0.2, size=(n_runs, 3))
        return mod, mod.batch_create(model.name, goals, basegoals=basegoals, seeds=seeds, precision=precision, **kw), None
    return make


def cases():
    """{name: make}; make() -> (module, batch id, what has to stay alive as long as the batch)"""
    out = {}
    for c in BENCH_CONFIGS:
        out["bench %s" % c] = _bench(c, batch=256 if c == 4 else 64)
        out["bench %s, two streams" % c] = _bench(c, streams=2, batch=256 if c == 4 else 64)
    out["bench 2, one stream"] = _bench(2, streams=1)
    out["bench held4, 512 threads"] = _bench("held4", threads=512, batch=4)
    out["bench tsr1, four per CU asked"] = _bench("tsr1", per_cu=4)
    out["start_tsr"] = _wam_tsr(True, False)
    out["start_tsr, con_tsr, momentum"] = _wam_tsr(True, True, momentum=True)
    for n_points in (400, 640):
        out["con_tsr, %d waypoints, two streams" % n_points] = _wam_tsr(False, True, n_points=n_points, streams=2)
    out["wam fp32"] = _wam(precision=32)
    out["wam fp32, derivative 2"] = _wam(precision=32, derivative=2)
    out["tree fp32"] = _tree(32)
    out["tree fp64"] = _tree(64)
    out["tree fp64, 200 waypoints, momentum"] = _tree(64, n_points=200, use_momentum=1)
    for n_points in (8, 32, 34, 300, 640):
        out["wam, %d waypoints" % n_points] = _wam(n_points=n_points)
        out["wam, %d waypoints, two streams" % n_points] = _wam(n_points=n_points, streams=2)
    out["wam, momentum, 640 waypoints"] = _wam(n_points=640, use_momentum=1)
    for threads in (192, 512):
        out["wam, %d threads" % threads] = _wam(threads=threads)
    out["wam, four per CU asked"] = _wam(per_cu=4)
    out["wam, 192 threads, two streams"] = _wam(threads=192, streams=2)
    out["wam, two fields"] = _two_fields(False)
    out["wam, scenes of two fields and one"] = _two_fields(True)
    for seed in range(8):
        out["random robot %d" % seed] = _random_robot(seed)
    return out


def plan_of(make):
    """the nine numbers, or the refusal's text (a random robot whose active dofs move no sphere)"""
    try:
        mod, bid, keep = make()
    except RuntimeError as e:
        return str(e)
    plan = mod.batch_plan(bid)
    mod.batch_destroy(bid)
    mod.close()
    return plan


@pytest.mark.parametrize("name", sorted(cases()))
def test_plan_is_the_parents(name):
    if common.plan_switches_active():
        pytest.skip("an experiment switch is set: the planner's own choice is what this test reads")
    golden = json.load(open(GOLDEN))
    assert name in golden, "no recorded plan for this case"
    assert plan_of(cases()[name]) == golden[name]
