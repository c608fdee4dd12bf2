"""-m "not gpu": the projection onto a TSR without a GPU.  The premises tests/test_gpu_project_tsr.py leans on, checked with the
oracle alone (P1 .. P5 below), the step rule of or_cdchomp_amd.project in isolation, and the two calls' place in the C ABI."""
import os
import re

import numpy as np
import pytest

import common
import project as PJ
from or_cdchomp_amd import _capi, project, robots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = {"unit": PJ.unit_base(), "default": list(robots.WAM_BASE_POSE)}
ROWS = {"six": PJ.BW6, "three": PJ.BW3}


@pytest.fixture(scope="module")
def sequences(oracle):
    """the restatement's run on the P1 inputs, for both bases and both TSRs: (base, rows) -> (case, result, history)"""
    out = {}
    for bname, base in BASES.items():
        for rname, Bw in ROWS.items():
            case = PJ.wam_case(oracle, base, Bw)
            hist = []
            res = case["ora"].project(case["seeds"], history=hist, lower=case["lower"], upper=case["upper"], tol=PJ.TOL)
            out[(bname, rname)] = (case, res, hist)
    return out


# ---- the premises ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bname", list(BASES))
@pytest.mark.parametrize("rname", list(ROWS))
def test_p1_the_chosen_inputs_converge(sequences, bname, rname):
    case, (rows, resid, steps, status), _ = sequences[(bname, rname)]
    assert (status == project.DONE).all(), status
    assert (resid <= PJ.TOL).all()
    assert ((rows >= case["lower"]) & (rows <= case["upper"])).all()
    if rname == "six":
        assert set(steps.tolist()) <= {3, 4}, steps      # (the three-row TSR leaves a null space to wander in: one row takes 26)
    print(bname, rname, "steps", np.bincount(steps))


@pytest.mark.parametrize("bname", list(BASES))
@pytest.mark.parametrize("rname", list(ROWS))
def test_p2_no_residual_next_to_the_tolerance(sequences, bname, rname):
    """what the device's rounding could flip: a residual within a relative 1e-3 of tol (if one is: change that seed, not tol)"""
    _, _, hist = sequences[(bname, rname)]
    r = np.concatenate([h[2] for h in hist])
    assert np.isfinite(r).all()
    rel = np.abs(r - PJ.TOL) / PJ.TOL
    print(bname, rname, "closest residual to tol, relative: %.3g" % rel.min())
    assert rel.min() > 1e-3


@pytest.mark.parametrize("bname", list(BASES))
def test_p3_away_from_the_angle_singularities(sequences, bname):
    """|pitch| <= 1.2 and |yaw|, |roll| <= 2.5 in the TSR's frame at q* and at every visited iterate: clear of 1/sqrt(1 - a^2)
    and of the wrap at +-pi"""
    case, _, hist = sequences[(bname, "six")]
    h_star, _ = case["ora"].evaluate(case["qstar"])
    angles = [np.abs(h_star[:, 3:])] + [np.abs(case["ora"].evaluate(it, idx)[0][:, 3:]) for idx, it, _ in hist]
    worst = np.concatenate(angles).max(axis=0)      # roll, pitch, yaw
    print(bname, "largest |roll|, |pitch|, |yaw|:", worst)
    assert worst[1] <= 1.2 and worst[0] <= 2.5 and worst[2] <= 2.5


def test_p4_wide_seeds_do_not_all_converge(oracle):
    case = PJ.wam_case(oracle, PJ.unit_base(), PJ.BW6, spread=1.0)
    rows, resid, steps, status = case["ora"].project(case["seeds"], lower=case["lower"], upper=case["upper"], tol=PJ.TOL)
    out = np.flatnonzero(status == project.OUT_OF_STEPS)
    print("rows out of steps:", out.tolist())
    assert 1 <= len(out) < PJ.N_TARGETS and (steps[out] == 30).all()
    assert (status[status != project.OUT_OF_STEPS] == project.DONE).all()
    case["ora"].destroy()


def test_p5_an_unreachable_target(oracle):
    model, _, dofvals, adofs = common.wam_state()
    lo, hi = PJ.wam_limits()
    ora = PJ.OracleTsrs(oracle, model, PJ.unit_base(), dofvals, adofs, "handbase", PJ.TOOL, [robots.Tsr(Bw=PJ.BW6, **PJ.UNREACHABLE)])
    hist = []
    rows, resid, steps, status = ora.project(np.array([robots.WAM_START]), history=hist, lower=lo, upper=hi, tol=PJ.TOL)
    visited = np.array([h[2][0] for h in hist])
    print("unreachable: residual %.3f from %.3f" % (resid[0], visited[0]))
    assert status[0] == project.OUT_OF_STEPS and steps[0] == 30
    assert resid[0] == visited.min() and resid[0] < visited[0]
    assert np.isfinite(rows).all() and np.isfinite(resid).all()
    assert np.abs(ora.evaluate(rows)[0]).max() == resid[0]
    ora.destroy()


# ---- the step rule in isolation ----------------------------------------------------------------------------------------------

def linear(Jm, target):
    """evaluate of the linear constraint h = J (q - target)"""
    Jm = np.asarray(Jm, dtype=np.float64); target = np.asarray(target, dtype=np.float64)
    return lambda rows: (((rows - target) @ Jm.T), np.broadcast_to(Jm, (len(rows),) + Jm.shape))


def test_a_step_is_the_regularised_least_norm_solution():
    rng = np.random.default_rng(3)
    Jm = rng.normal(size=(3, 5)); q = rng.normal(size=(2, 5)); h = rng.normal(size=(2, 3)) * 0.01
    new, ok, moved = project.project_step(q, h, np.broadcast_to(Jm, (2, 3, 5)), mu=1e-8, step_cap=10.0)
    want = q - (Jm.T @ np.linalg.solve(Jm @ Jm.T + 1e-8 * np.eye(3), h.T)).T
    assert ok.all() and moved.all() and np.abs(new - want).max() < 1e-13
    # rows from k on are carried as the identity: they change nothing
    pad_h = np.concatenate([h, np.full((2, 3), 7.0)], axis=1)
    pad_J = np.concatenate([np.broadcast_to(Jm, (2, 3, 5)), np.full((2, 3, 5), 9.0)], axis=1)
    assert np.array_equal(project.project_step(q, pad_h, pad_J, mu=1e-8, step_cap=10.0, k=[3, 3])[0], new)


def test_the_cap_on_the_step():
    Jm = np.eye(2, 4)
    new, ok, moved = project.project_step(np.zeros((1, 4)), [[3.0, 4.0]], Jm[None], mu=0.0, step_cap=0.5)
    assert ok[0] and moved[0] and np.allclose(new[0], [-0.3, -0.4, 0.0, 0.0], rtol=1e-15, atol=0)
    new, _, _ = project.project_step(np.zeros((1, 4)), [[0.03, 0.04]], Jm[None], mu=0.0, step_cap=0.5)
    assert np.array_equal(new[0], [-0.03, -0.04, 0.0, 0.0])      # a step within the cap is not scaled


def test_the_clip():
    Jm = np.eye(2, 3)
    new, ok, moved = project.project_step([[0.0, 0.0, 0.0]], [[-0.2, 0.2]], Jm[None], lower=[-1, -0.05, -1], upper=[0.1, 1, 1], mu=0.0)
    assert np.array_equal(new[0], [0.1, -0.05, 0.0]) and moved[0]
    # a step that the box takes back entirely moves no entry
    new, ok, moved = project.project_step([[0.1, -0.05, 0.0]], [[-0.2, 0.2]], Jm[None], lower=[-1, -0.05, -1], upper=[0.1, 1, 1], mu=0.0)
    assert ok[0] and not moved[0]
    out = project.project(linear(Jm, [0.3, -0.3, 0.0]), [[0.1, -0.05, 0.0]], lower=[-1, -0.05, -1], upper=[0.1, 1, 1], mu=0.0)
    assert out[3][0] == project.STALLED and out[2][0] == 0 and np.array_equal(out[0][0], [0.1, -0.05, 0.0])


def test_a_singular_system_without_mu_stalls():
    Jm = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])      # two identical rows: J J^T is singular
    rows = np.array([[0.5, 0.2, -0.1]])
    new, ok, moved = project.project_step(rows, [[0.5, 0.5]], Jm[None], mu=0.0)
    assert not ok[0] and np.array_equal(new, rows)
    out = project.project(linear(Jm, [0.0, 0.0, 0.0]), rows, mu=0.0)
    assert out[3][0] == project.STALLED and out[2][0] == 0 and np.array_equal(out[0], rows) and out[1][0] == 0.5
    # with mu the same system steps
    assert project.project(linear(Jm, [0.0, 0.0, 0.0]), rows, mu=1e-8)[3][0] == project.DONE
    # a pivot that is not finite
    assert not project.project_step(rows, [[0.5, 0.5]], np.array([[[np.inf, 0, 0], [0, 1, 0]]]), mu=0.0)[1][0]


def test_a_row_within_tol_comes_back_bit_for_bit():
    Jm = np.eye(2, 3)
    rows = np.array([[1e-7 / 3, -2e-7 / 3, 0.123456789], [0.5, 0.0, 0.0]])
    out, resid, steps, status = project.project(linear(Jm, [0, 0, 0]), rows, tol=1e-6, dtype=np.float32)
    assert status[0] == project.DONE and steps[0] == 0 and np.array_equal(out[0], rows[0]) and out.dtype == np.float64
    assert status[1] == project.DONE and steps[1] == 1


def test_max_steps_zero_is_the_evaluation_alone():
    Jm = np.eye(2, 3)
    rows = np.array([[0.25, -0.5, 1.0 / 3], [1e-8, 0.0, 0.7]])
    out, resid, steps, status = project.project(linear(Jm, [0, 0, 0]), rows, max_steps=0)
    assert np.array_equal(out, rows) and np.array_equal(resid, [0.5, 1e-8]) and (steps == 0).all()
    assert status.tolist() == [project.OUT_OF_STEPS, project.DONE]


def test_a_non_finite_row():
    Jm = np.eye(2, 3)
    rows = np.array([[0.5, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0]])
    seen = []

    def evaluate(r):
        seen.append(r.copy())
        return linear(Jm, [0, 0, 0])(r)

    out, resid, steps, status = project.project(evaluate, rows)
    assert status.tolist() == [project.DONE, project.NOT_FINITE, project.NOT_FINITE]
    assert np.isnan(out[1:]).all() and np.isnan(resid[1:]).all() and (steps[1:] == 0).all()
    assert all(np.isfinite(r).all() for r in seen), "a non-finite row is never evaluated"
    alone = project.project(linear(Jm, [0, 0, 0]), rows[:1])
    assert np.array_equal(alone[0][0], out[0]) and alone[1][0] == resid[0]


def test_the_best_visited_iterate_comes_back():
    """a constraint whose step overshoots: r goes 1, 3, 9, ...; the input is the best and comes back"""
    evaluate = lambda rows: (rows[:, :1].copy(), np.full((len(rows), 1, 1), -0.25))      # dq = -J h / J^2 = +4 h: away
    out, resid, steps, status = project.project(evaluate, [[1.0]], max_steps=3, step_cap=100.0, mu=0.0)
    assert status[0] == project.OUT_OF_STEPS and steps[0] == 3 and out[0, 0] == 1.0 and resid[0] == 1.0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------

def test_the_calls_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "orcdchomp_amd.h")).read()
    bound = {name for name, _, _ in _capi.SYMBOLS}
    for name in ("orc_batch_config_tsr", "orc_batch_project_tsr"):
        assert re.search(r"\bint %s\(" % name, header) and name in bound
    assert "typedef struct orc_tsr" in header
    import ctypes as C
    assert C.sizeof(_capi.Tsr) == 8 + 8 * (7 * 3 + 12)      # int + padding, three poses, Bw [6][2]


def test_pose_from_dr_is_the_oracles(oracle):
    rng = np.random.default_rng(5)
    for _ in range(20):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        R = PJ.rot(q); d = rng.normal(size=3)
        assert np.array_equal(robots.pose_from_dR(d, R), oracle.pose_from_dR(d, R))
