"""not gpu: the rule of the projection onto a TSR and out of contact (or_cdchomp_amd/project_clear.py) -- the premises of
tests/test_gpu_project_clear.py on the 15 goals in contact, the properties of the step, the key and the loop, and the C symbol.

Premises, with the committed rule's own numbers (fp64, tests/project_clear.PARAMS, inside the WAM's limits):
  six rows (BW6)    rows 0 and 14 of the 15 finish, in 9 and 13 steps; the other 13 run out of steps
  three rows (BW3)  rows 0, 2, 3, 8, 10, 11, 12, 14 finish, in 5, 6, 4, 10, 32, 6, 8, 8 steps
  closest decisions over all visited iterates of all 15 rows: |r - tol| / tol 6.6e-3 (BW6), 6.3e-2 (BW3); |clearance - margin|
  7.1e-4 m (BW6), 1.2e-4 m (BW3) -- no row had to be dropped from the compared set.
  Plain projection (project.project) finishes all 15 at status 0 and clears none.  With BW3 every row comes back bit for bit; with
  BW6 rows 6 and 11 start at r = 1.107e-6 and 1.039e-6, just off the tolerance (the default base's matrix is not a rotation, and
  the TSR's frame is made with the exact one), take one step of 2e-6 and 2e-4 and stay in contact; the other 13 come back bit
  for bit."""
import os
import re

import numpy as np
import pytest

import common
import project_clear as PC
from or_cdchomp_amd import _capi, project, project_clear

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fifteen(oracle):
    """the 15 rows under BW6 and BW3: name -> dict(R, out, hist, plain)"""
    w = PC.world(oracle)
    rows = PC.contact_rows(w)
    res = {"w": w, "rows": rows}
    for name, Bw in PC.BWS.items():
        R = PC.Restated(oracle, w, PC.tsrs_of(w, rows, Bw), np.arange(len(rows)))
        hist = []
        out = R.run(rows, history=hist)
        plain = R.ora.project(rows, lower=w["lower"], upper=w["upper"], tol=PC.PARAMS["tol"])
        res[name] = dict(R=R, out=out, hist=hist, plain=plain)
    yield res
    for name in PC.BWS:
        res[name]["R"].destroy()


def test_the_fifteen_goals_are_the_ones_in_contact(fifteen):
    assert np.flatnonzero(PC.in_contact(fifteen["w"], common.wam_goals(48))).tolist() == PC.CONTACT_48


@pytest.mark.parametrize("name", list(PC.BWS))
def test_which_rows_finish_and_in_how_many_steps(fifteen, name):
    c = fifteen[name]
    rows, resid, clr, steps, status = c["out"]
    print(name, "status", status.tolist(), "steps", steps.tolist())
    done = np.flatnonzero(status == project.DONE)
    assert done.tolist() == sorted(PC.FINISH[name]) and [int(steps[q]) for q in done] == [PC.FINISH[name][q] for q in done]
    rest = np.setdiff1d(np.arange(15), done)
    assert (status[rest] == project.OUT_OF_STEPS).all() and (steps[rest] == PC.PARAMS["max_steps"]).all()
    # every finished row: the oracle's max |h| <= tol and the restated clearance >= margin
    r = c["R"].residual(rows); cl = c["R"].clearance(rows)
    assert (r[done] <= PC.PARAMS["tol"]).all() and (cl[done] >= np.asarray(PC.PARAMS["margin"])).all()
    assert np.array_equal(r, resid) and np.array_equal(cl, clr), "resid and clearance are the returned row's"
    # no row is worse than its input
    c0, v0 = c["R"].keys(fifteen["rows"]); c1, v1 = c["R"].keys(rows)
    assert PC.not_worse(c1, v1, c0, v0, 0.0).all()


@pytest.mark.parametrize("name", list(PC.BWS))
def test_plain_projection_finishes_all_and_clears_none(fifteen, name):
    rows, resid, steps, status = fifteen[name]["plain"]
    assert (status == project.DONE).all()
    assert PC.in_contact(fifteen["w"], rows).all(), "none is clear"
    stepped = np.flatnonzero(steps > 0).tolist()
    assert stepped == ([6, 11] if name == "BW6" else []), stepped      # (the module's docstring)
    keep = np.setdiff1d(np.arange(15), stepped)
    assert rows[keep].tobytes() == fifteen["rows"][keep].tobytes()


@pytest.mark.parametrize("name", list(PC.BWS))
def test_no_decision_of_a_compared_row_lies_in_a_band(fifteen, name):
    dr, dc = PC.decisions(fifteen[name]["hist"])
    print(name, "closest |r - tol| / tol %.2e, closest |clearance - margin| %.2e m (all 15 rows)" % (dr.min(), dc.min()))
    compared = sorted(PC.FINISH[name])
    assert len(compared) >= (2 if name == "BW6" else 6)
    assert (dr[compared] >= 1e-3).all() and (dc[compared] >= 1e-6).all()


# ---- the step ------------------------------------------------------------------------------------------------------------------

def random_system(q=24, K=6, n=7, seed=3):
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-1, 1, (q, n)); h = 0.1 * rng.standard_normal((q, K)); J = rng.standard_normal((q, K, n))
    g = rng.standard_normal((q, n)); cost = np.abs(rng.standard_normal((q, 2))) * 1e-3
    k = rng.integers(1, K + 1, q)
    return rows, h, J, cost, g, k


def test_the_push_lies_in_the_null_space_of_J_up_to_the_damping():
    """J g_N = J g - (A - mu I) A^-1 J g = mu A^-1 (J g): J p is held to -(2U / s) shrink mu z, and is small against p"""
    rows, h, J, cost, g, k = random_system()
    mu = 1e-8
    d = {}
    project_clear.clear_step(rows, h, J, cost, g, mu=mu, k=k, detail=d)
    assert d["pushed"].all() and np.abs(d["push"]).max() > 1e-3
    on = np.arange(6)[None, :] < k[:, None]
    Jk = np.where(on[:, :, None], J, 0.0)
    Jp = np.einsum("qkn,qn->qk", Jk, d["push"])
    gN = g - np.einsum("qkn,qk->qn", Jk, d["z"])
    coef = np.abs(d["push"]).max(axis=1) / np.abs(gN).max(axis=1)      # (2U / s) shrink, from the step itself
    want = -coef[:, None] * mu * d["z"]
    scale = coef * np.abs(Jk).sum(axis=(1, 2)) * np.abs(g).max(axis=1)
    assert (np.abs(Jp - want).max(axis=1) <= 1e-13 * scale).all()
    assert (np.abs(Jp).max(axis=1) <= 1e-6 * np.abs(d["push"]).max(axis=1)).all()
    # the push descends: p . g < 0, and its length is capped
    assert ((d["push"] * g).sum(axis=1) < 0).all() and (np.sqrt((d["push"] ** 2).sum(axis=1)) <= 0.2 * (1 + 1e-15)).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_step_without_cost_is_project_steps_bit_for_bit(dtype):
    rows, h, J, cost, g, k = random_system()
    lo = np.full(7, -0.9); hi = np.full(7, 0.95)
    for c in (np.zeros_like(cost), np.full_like(cost, np.nan), -cost):      # (U = 0, not finite, negative: no push)
        got = project_clear.clear_step(rows, h, J, c, g, lo, hi, k=k, dtype=dtype)
        want = project.project_step(rows, h, J, lo, hi, k=k, dtype=dtype)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    bad = g.copy(); bad[::2, 3] = np.inf      # a gradient that is not finite: no push either
    got = project_clear.clear_step(rows, h, J, cost, bad, lo, hi, k=k, dtype=dtype)
    want = project.project_step(rows, h, J, lo, hi, k=k, dtype=dtype)
    assert got[0][::2].tobytes() == want[0][::2].tobytes() and (got[0][1::2] != want[0][1::2]).any()


def test_the_order_of_the_key():
    nan = np.nan
    tol, m = 1e-6, (0.02, 0.0)
    cls, val = project_clear.key_of(np.array([1e-7, 1e-7, 1e-7, 1e-3, nan, 1e-7]), np.array([0.0, 3.0, 3.0, 0.0, 1.0, 1.0]),
                                    np.array([[0.03, 0.1], [0.01, 0.1], [0.03, -0.1], [0.03, 0.1], [0.03, 0.1], [nan, 0.1]]), tol, m)
    assert cls.tolist() == [0, 1, 1, 2, 2, 1] and val[0] == 0 and val[1] == 3.0 and val[3] == 1e-3 and np.isnan(val[4]) and val[5] == 1.0
    better = lambda a, b: bool(project_clear.key_better(np.array([a[0]]), np.array([a[1]]), np.array([b[0]]), np.array([b[1]]))[0])
    assert better((0, 0.0), (1, 0.0)) and better((1, 5.0), (2, 1e-9)) and not better((2, 1e-9), (1, 5.0))
    assert better((1, 1.0), (1, 2.0)) and not better((1, 2.0), (1, 1.0)) and not better((1, 1.0), (1, 1.0))      # the earlier keeps a tie
    assert not better((2, nan), (2, 1.0)) and better((2, 1.0), (2, nan)) and not better((2, nan), (2, nan))
    assert better((1, nan), (2, 1.0)), "the lower class wins"


# ---- the loop on small hand-made evaluations ---------------------------------------------------------------------------------

def plane(n=4, wall=0.3):
    """a TSR that holds x[0] at 0 and leaves the rest free; a wall that wants x[1] >= wall: gap = x[1] - wall + margin"""
    def tsr(rows):
        J = np.zeros((len(rows), 1, n)); J[:, 0, 0] = 1.0
        return rows[:, :1].copy(), J

    def pen(rows, margin):
        gap = rows[:, 1] - wall
        d = np.maximum(0.0, margin[0] - gap)
        grad = np.zeros((len(rows), n)); grad[:, 1] = -d
        return dict(cost=np.stack([0.5 * d * d, np.zeros(len(rows))], axis=1), grad=grad, clearance=np.stack([gap, np.full(len(rows), np.inf)], axis=1))
    return tsr, pen


def test_the_loop_on_a_plane_and_a_wall():
    tsr, pen = plane()
    rows = np.array([[0.2, 0.0, 0.7, 0.1 + 2.0 ** -30], [0.0, 0.5, 0.3, 0.2], [1e-7, 0.31, 0.3, 0.2]])
    out, resid, clr, steps, status = project_clear.project_clear(tsr, pen, rows, margin=(0.0, 0.0))
    assert status.tolist() == [0, 0, 0] and steps.tolist()[1:] == [0, 0] and steps[0] >= 1
    assert abs(out[0, 0]) <= 1e-6 and out[0, 1] >= 0.3 and clr[0, 0] >= 0.0 and resid[0] == abs(out[0, 0])
    assert out[0, 2:].tobytes() == rows[0, 2:].tobytes(), "the entries no step moved are the caller's doubles"
    assert out[1:].tobytes() == rows[1:].tobytes(), "a row that starts on its TSR and clear comes back bit for bit"
    for dtype in (np.float64, np.float32):
        z = project_clear.project_clear(tsr, pen, rows, margin=(0.0, 0.0), max_steps=0, dtype=dtype)
        assert z[0].tobytes() == rows.tobytes() and (z[3] == 0).all() and z[4].tolist() == [2, 0, 0]
        o32 = project_clear.project_clear(tsr, pen, rows, margin=(0.0, 0.0), dtype=dtype, tol=1e-4)
        assert o32[0][0, 2:].tobytes() == rows[0, 2:].tobytes() and o32[4][0] == 0
    # the best iterate by the key: with one step allowed the row is off the TSR before and after, and the smaller r wins
    one = project_clear.project_clear(tsr, pen, rows[:1], margin=(0.0, 0.0), max_steps=1, step_cap=0.05)
    assert one[4][0] == project.OUT_OF_STEPS and one[3][0] == 1 and one[1][0] < 0.2


def test_status_1_and_status_3():
    tsr, pen = plane()
    rows = np.array([[0.2, 0.0, 0.7, 0.1]])
    # a step that moves no entry: the box is the row
    out = project_clear.project_clear(tsr, pen, rows, margin=(0.0, 0.0), lower=rows[0], upper=rows[0])
    assert out[4][0] == project.STALLED and out[3][0] == 0 and out[0].tobytes() == rows.tobytes()
    # a pivot that is not positive: J = 0 without damping
    flat = lambda r: (r[:, :1].copy(), np.zeros((len(r), 1, 4)))
    out = project_clear.project_clear(flat, pen, rows, margin=(0.0, 0.0), mu=0.0)
    assert out[4][0] == project.STALLED and out[3][0] == 0
    # a row with a non-finite entry
    bad = np.array([[0.2, np.nan, 0.7, 0.1], [0.0, 0.5, 0.3, 0.2], [np.inf, 0.5, 0.3, 0.2]])
    out = project_clear.project_clear(tsr, pen, bad, margin=(0.0, 0.0))
    assert out[4].tolist() == [3, 0, 3] and out[3].tolist() == [0, 0, 0]
    for q in (0, 2):
        assert np.isnan(out[0][q]).all() and np.isnan(out[1][q]) and np.isnan(out[2][q]).all()
    assert out[0][1].tobytes() == bad[1].tobytes()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_symbol_and_null_module():
    header = open(os.path.join(ROOT, "include", "orcdchomp_amd.h")).read()
    name = "orc_batch_project_tsr_clear"
    args = ["orc_module * mod", "int batch_id", "int n_tsr", "const orc_tsr * tsrs", "int n_q", "const int * tsr_of_q", "const int * run_of_q",
            "const double * configs", "const double * lower", "const double * upper", "int max_steps", "double tol", "double mu", "double step_cap",
            "double push_cap", "double margin_field", "double margin_self", "double slack", "double * configs_out", "double * resid_out",
            "double * clearance_out", "int * steps_out", "int * status_out"]
    m = re.search(r"int %s\((.*?)\);" % name, header, re.S)
    assert m, name
    assert [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")] == args
    assert "or_cdchomp_amd/project_clear.py" in header
    assert name in [s[0] for s in _capi.SYMBOLS] and hasattr(_capi.lib(), name)
    assert len([s for s in _capi.SYMBOLS if s[0] == name][0][2]) == len(args)
    lib = _capi.lib()
    dp, ip = _capi.c_double_p, _capi.c_int_p
    cfg = np.zeros((3, 7)); ro = np.full((3, 7), 7.0); rs = np.full(3, 7.0); cl = np.full((3, 2), 7.0)
    st = np.full(3, 7, dtype=np.int32); ss = np.full(3, 7, dtype=np.int32)
    rec = (_capi.Tsr * 1)()
    want = lib.orc_batch_project_tsr(None, 1, 1, rec, 3, None, cfg.ctypes.data_as(dp), None, None, 30, 1e-6, 1e-8, 0.5, ro.ctypes.data_as(dp),
                                     rs.ctypes.data_as(dp), st.ctypes.data_as(ip), ss.ctypes.data_as(ip))
    assert want != 0
    assert lib.orc_batch_project_tsr_clear(None, 1, 1, rec, 3, None, None, cfg.ctypes.data_as(dp), None, None, 40, 1e-6, 1e-8, 0.5, 0.2, 0.02, 0.0, 2e-3,
                                           ro.ctypes.data_as(dp), rs.ctypes.data_as(dp), cl.ctypes.data_as(dp), st.ctypes.data_as(ip),
                                           ss.ctypes.data_as(ip)) == want
    assert (ro == 7.0).all() and (rs == 7.0).all() and (cl == 7.0).all() and (st == 7).all() and (ss == 7).all(), "a NULL module writes nothing"
