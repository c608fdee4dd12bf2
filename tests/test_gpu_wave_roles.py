"""-m gpu: every value of ORC_WAVE_ROTATE gives the bits of 0.

The phases of the iterate kernel hand their work out by a logical thread index, the hardware index rotated by whole wavefronts
(csrc/wave_roles.h).  A run's results are a function of the logical index alone, so the trajectories, the costs (the wavefronts'
partial sums are added in logical order), the status, the iterations made, the trace and the momentum AG of a batch must not
depend on the rotation -- bit for bit, in every kernel family.  The switch is read at `create`, so one module serves all values.

Six iterations: more than the four wavefronts of a workgroup, so that value 2 (a rotation per iteration) wraps.  Value 1 takes
the rotation from bits 8.. of the workgroup index: the short-trajectory cases have 520 runs and the headline plan is also run
with 1024, so that it rotates by every amount.  That the switch reaches the kernels at all is read back: with ORC_PHASE_TIMERS=1
every hardware wavefront records the logical wavefront it was in the launch's last iteration (the "waves" state)."""
import numpy as np
import pytest

import common
import or_cdchomp_amd
from or_cdchomp_amd import robots, scenes as scene_lib

pytestmark = pytest.mark.gpu

N_ITER = 6
ROTATIONS = (1, 2)
# rows of common.wam_goals(256) for the headline case: all but row 2 leave their joint limits within six iterations and are
# brought back by 2 .. 14 projection rounds (asserted below through the phase counters)
HEADLINE_ROWS = (0, 1, 2, 3, 4, 5, 6, 7)


def _outputs(mod, bid, n_iter=N_ITER, phase=False):
    costs, status = mod.batch_iterate(bid, n_iter)
    out = dict(costs=costs, status=status, iters=mod.batch_iterations_done(bid), trace=mod.batch_trace(bid, n_iter),
               traj=mod.batch_gettraj(bid), AG=mod.batch_state(bid, "AG"), plan=mod.batch_plan(bid))
    if phase:
        ph = np.zeros((costs.shape[0], 8))
        mod._check(mod._lib.orc_batch_get_state(mod._h, bid, b"phase", ph.ctypes.data_as(or_cdchomp_amd._capi.c_double_p), ph.size))
        out["rounds"] = ph[:, 6]
        raw = np.zeros((costs.shape[0], 8, 2))
        mod._check(mod._lib.orc_batch_get_state(mod._h, bid, b"waves", raw.ctypes.data_as(or_cdchomp_amd._capi.c_double_p), raw.size))
        out["logical_wave"] = raw[:, :out["plan"]["threads"] // 64, 1].astype(np.int64) >> 8
    mod.batch_destroy(bid)
    return out


def _same_bits(a, b, what):
    for key in ("traj", "costs", "status", "iters", "trace", "AG", "rounds"):
        if key in a:
            assert np.array_equal(a[key], b[key], equal_nan=True), "%s: %s differs" % (what, key)
    assert a["plan"] == b["plan"], what


def _expected_logical_wave(value, n_runs, waves, n_iter=N_ITER):
    """csrc/wave_roles.h wave_rot and logical_tid, restated: [n_runs][waves] in the launch's last iteration"""
    run = np.arange(n_runs)[:, None]
    rot = (((run >> 8) & 7) + (((n_iter - 1) & 7) if value >= 2 else 0)) % waves if value else 0 * run
    return (np.arange(waves)[None, :] + rot) % waves


def _all_rotations(monkeypatch, mod, create, phase=False):
    """the outputs of the batch `create()` makes without a rotation, checked against those under every value of the switch"""
    monkeypatch.delenv("ORC_WAVE_ROTATE", raising=False)
    base = _outputs(mod, create(), phase=phase)
    assert np.isfinite(base["traj"]).all()
    for value in ROTATIONS:
        monkeypatch.setenv("ORC_WAVE_ROTATE", str(value))
        out = _outputs(mod, create(), phase=phase)
        lw = out.pop("logical_wave", None)
        if lw is not None:
            assert np.array_equal(lw, _expected_logical_wave(value, *lw.shape)), "ORC_WAVE_ROTATE=%d did not reach the kernel" % value
        _same_bits(base, out, "ORC_WAVE_ROTATE=%d" % value)
    lw = base.pop("logical_wave", None)
    if lw is not None:
        assert np.array_equal(lw, _expected_logical_wave(0, *lw.shape))
    monkeypatch.delenv("ORC_WAVE_ROTATE")
    return base


def test_headline_plan_with_joint_limit_rounds(monkeypatch):
    """the WAM of config 2, 100 waypoints, launches that overlap: the tiles of 50 + 48 and the two-waypoint cost round exist only here"""
    headline = not common.plan_switches_active()
    monkeypatch.setenv("ORC_PHASE_TIMERS", "1")
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    mod.set_num_streams(2)
    goals = np.ascontiguousarray(common.wam_goals(256)[list(HEADLINE_ROWS)])
    base = _all_rotations(monkeypatch, mod, lambda: mod.batch_create(model.name, goals, **common.CONFIG2_KW), phase=True)
    if headline:
        plan = base["plan"]
        assert plan["threads"] == 256 and plan["workgroups_per_cu"] == 4 and plan["tiles"] == 2 and plan["tile_first"] == 50, plan
    assert (base["iters"] == N_ITER).all() and (base["status"] == 0).all()
    assert (base["rounds"] > 0).any(), "no run made a joint-limit round: %s" % base["rounds"]
    mod.close()


def test_headline_plan_with_every_rotation_by_workgroup(monkeypatch):
    """the same plan with 1024 runs: value 1 rotates workgroups 256 apart by 0, 1, 2 and 3 wavefronts"""
    monkeypatch.setenv("ORC_PHASE_TIMERS", "1")
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    mod.set_num_streams(2)
    goals = common.wam_goals(1024)
    base = _all_rotations(monkeypatch, mod, lambda: mod.batch_create(model.name, goals, **common.CONFIG2_KW), phase=True)
    assert (base["rounds"] > 0).any()
    mod.close()


def test_a_value_outside_the_table_is_refused(monkeypatch):
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    for value in ("3", "-1"):
        monkeypatch.setenv("ORC_WAVE_ROTATE", value)
        with pytest.raises(RuntimeError, match="ORC_WAVE_ROTATE"):
            mod.batch_create(model.name, common.wam_goals(4), **common.CONFIG2_KW)
    monkeypatch.delenv("ORC_WAVE_ROTATE")
    mod.close()


@pytest.mark.parametrize("threads", [128, 192, 512])
def test_short_trajectories_at_other_workgroup_sizes(monkeypatch, threads):
    monkeypatch.setenv("ORC_PHASE_TIMERS", "1")
    mod = or_cdchomp_amd.Module(0)
    mod.set_workgroup_threads(threads)
    model = common.setup_product_wam(mod)
    goals = common.wam_goals(520)
    base = _all_rotations(monkeypatch, mod, lambda: mod.batch_create(model.name, goals, **dict(common.CONFIG2_KW, n_points=20)), phase=True)
    if not common.plan_switches_active():
        assert base["plan"]["threads"] == threads, base["plan"]
    mod.close()


def test_held_body_pair_list(monkeypatch):
    """15 + 4 active spheres: the 32-lane family with the dense pair list (cost_pairs.h)"""
    mod = or_cdchomp_amd.Module(0)
    model, _, _ = common.setup_product_wam_held4(mod)
    goals = common.wam_goals(4, seed=3)
    _all_rotations(monkeypatch, mod, lambda: mod.batch_create(model.name, goals, **dict(common.CONFIG2_KW, n_points=40)))
    mod.close()


def test_fp32_tree_generic_pass(monkeypatch):
    """the 30-dof tree in fp32: the many-sphere pass (cost_generic.h), inlined into the kernel function"""
    mod = or_cdchomp_amd.Module(0)
    model = robots.tree30()
    mod.add_robot(model, transform=[0.0] * 6 + [1.0], dof_values=np.zeros(model.n_dof), active_dofs=list(range(model.n_dof)))
    for name, (boxes, pose) in scene_lib.random_boxes(np.random.default_rng(20250104)).items():
        mod.add_kinbody_boxes(name, boxes, transform=pose)
        mod.SendCommand("computedistancefield kinbody %s cube_extent 0.02 aabb_padding 0.15" % name)
    goals = np.random.default_rng(5).uniform(-0.8, 0.8, size=(8, model.n_dof))
    _all_rotations(monkeypatch, mod, lambda: mod.batch_create(model.name, goals, precision=32, n_points=40, lambda_=200.0, obs_factor=100.0))
    mod.close()


def test_floating_base_momentum_hmc(monkeypatch):
    """n = 14 with the quaternion renormalisation, momentum carried between iterations, resamples inside the six iterations
    (asserted: the momentum differs from that of the same runs without hmc)"""
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    goals, basegoals, seeds, kw = common.config4_problem(n_runs=8)
    kw = dict(kw, n_points=40, hmc_resample_lambda=0.5)
    base = _all_rotations(monkeypatch, mod, lambda: mod.batch_create(model.name, goals, basegoals=basegoals, seeds=seeds, **kw))
    plain = _outputs(mod, mod.batch_create(model.name, goals, basegoals=basegoals, seeds=seeds, **dict(kw, use_hmc=0)))
    resampled = [k for k in range(len(goals)) if not np.array_equal(base["AG"][k], plain["AG"][k])]
    assert len(resampled) >= 4, "too few runs resampled their momentum within %d iterations: %s" % (N_ITER, resampled)
    mod.close()


def test_one_tsr_row(monkeypatch):
    """the elbow's height held on every point (`con_tsr`): one constrained row per waypoint (tsr.h)"""
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
    cmd = ("createbatch robot %s n_runs 4 adofgoals 0x%x n_points 30 lambda 100 obs_factor 200 con_tsr 'all link wam4' '%s'"
           % (model.name, goals.ctypes.data, tsr.serialize()))
    _all_rotations(monkeypatch, mod, lambda: int(mod.SendCommand(cmd)))
    mod.close()


def test_derivative_2(monkeypatch):
    """the penta-diagonal metric: the band passes and the solve through the inverse's generators"""
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    goals = common.wam_goals(8, seed=7)
    _all_rotations(monkeypatch, mod, lambda: mod.batch_create(model.name, goals, **dict(common.CONFIG2_KW, n_points=30, derivative=2)))
    mod.close()
