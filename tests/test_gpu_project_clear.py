"""-m gpu: the projection onto TSRs and out of contact on the device (orc_batch_project_tsr_clear;
Module.batch_project_tsr_clear) against the restatement of tests/project_clear.py: project_clear.project_clear around the
oracle's eval_contsr and the restated penetration.  The premises -- which of the 15 goals in contact finish, in how many steps,
and that no decision of a compared row lies near the tolerance or a margin -- are tests/test_host_project_clear.py's.

The bounds are measured ones (NOTES/project-clear.md): ten times the largest difference seen on an MI355X over the comparisons
of this file that share the bound, rounded up to a power of ten.  A row that runs all 40 steps amplifies rounding and is not
compared row for row; its reported residual and clearance are still held to the oracle's at the row it returns."""
import os

import numpy as np
import pytest

import clearance as CL
import common
import or_cdchomp_amd
import penetration as PN
import project as PJ
import project_clear as PC
from or_cdchomp_amd import _capi, project, project_clear, robots, scenes
from test_gpu_clearance import product_field

pytestmark = pytest.mark.gpu

# measured on an MI355X, the largest over this file's comparisons.  The single step against the rule's: 5.12e-13 over the rows
# whose gradient the null-space projection cancels by less than 1e3 (3.11e-15 with three rows), 3.43e-9 over all (test_one_round
# says why).  The whole loop's compared rows against the restatement's: 4.44e-15.  resid_out against the oracle's max |h| and
# clearance_out against the restated clearance at the returned row: 4.79e-16 and 3.19e-16 in fp64, 1.07e-7 and 8.20e-8 in
# precision 32; they are held to the bounds tests/test_gpu_project_tsr.py measured for h against eval_contsr
BOUND_STEP = 1e-11
BOUND_STEP_ILL = 1e-7
BOUND_ROWS = 1e-13
BOUND_64 = 1e-13
BOUND_32 = 1e-5
KW = dict(n_points=4, lambda_=100.0, obs_factor=200.0)
SCENES = dict(scenes=[[("table", None)], [("table", PN.SHIFT)]], scene_of_run=np.array([0, 1], dtype=np.int32))
N = 15


@pytest.fixture(scope="module")
def wam(oracle):
    """the WAM on its default base over the table, with a batch of each precision whose run 1 sees the table at PN.SHIFT, and
    the restatement's answers on the 15 rows: dict(mod, w, rows, b64, b32, BW6, BW3)"""
    w = PC.world(oracle)
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    assert np.array_equal(mod.get_sdf("table")[0], w["prob"]["sdf"].data)
    w["table"] = product_field(oracle, mod, "table")
    w["shifted"] = product_field(oracle, mod, "table", kpose=PN.compose(oracle, PN.SHIFT, mod.body_transform("table")))
    w["tab"] = CL.Tables(oracle, model, w["base"], w["dofvals"], w["adofs"], [w["table"]])
    goals = common.wam_goals(2, seed=3)
    rows = PC.contact_rows(w)
    out = dict(mod=mod, model=model, w=w, rows=rows, b64=mod.batch_create(model.name, goals, **dict(KW, **SCENES)),
               b32=mod.batch_create(model.name, goals, precision=32, **dict(KW, **SCENES)))
    for name, Bw in PC.BWS.items():
        tsrs = PC.tsrs_of(w, rows, Bw)
        R = PC.Restated(oracle, w, tsrs, np.arange(N))
        out[name] = dict(tsrs=tsrs, R=R, want=R.run(rows))
    yield out
    for name in PC.BWS:
        out[name]["R"].destroy()
    mod.close()


def call(wam, name, rows, bid=None, tsr_of=None, **kw):
    tsr_of = np.arange(N) if tsr_of is None else tsr_of
    return wam["mod"].batch_project_tsr_clear(wam["b64"] if bid is None else bid, wam[name]["tsrs"], rows, tsr_of=tsr_of, **kw)


OUT = ("configs", "resid", "clearance", "steps", "status")


def same(a, b, what, idx=None, jdx=None):
    for key in OUT:
        x = np.asarray(a[key]) if idx is None else np.asarray(a[key])[idx]
        y = np.asarray(b[key]) if jdx is None else np.asarray(b[key])[jdx]
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (what, key)


def reported_is_the_returned_rows(R, res, bound, what):
    """for every row: the oracle's residual and the restated clearance at the returned row against resid_out and clearance_out"""
    r = R.residual(res["configs"]); c = R.clearance(res["configs"])
    fin = np.isfinite(c)
    assert np.array_equal(fin, np.isfinite(res["clearance"])) and np.array_equal(c[~fin], res["clearance"][~fin])
    er = float(np.abs(r - res["resid"]).max()); ec = float(np.abs(c[fin] - res["clearance"][fin]).max())
    print("%s: resid_out against the oracle's %.2e, clearance_out against the restated %.2e" % (what, er, ec))
    assert er <= bound and ec <= bound, (what, er, ec)
    return r, c


# ---- 1. one round --------------------------------------------------------------------------------------------------------------

def conditioning(R, rows):
    """|g| / |g_N| of the rule's step at rows: how much of the gradient the projection into J's null space cancels.  The push
    is g_N stretched to 2U / |g_N| (or to push_cap), so a rounding error of g_N's entries grows by this ratio"""
    idx = np.arange(len(rows))
    h, J = R.ora.evaluate(rows, idx)
    pen = R.pen(rows, tuple(np.asarray(PC.PARAMS["margin"]) + PC.PARAMS["slack"]), idx)
    d = {}
    project_clear.clear_step(rows, h, J, pen["cost"], pen["grad"], k=R.k, detail=d)
    Jk = np.where((np.arange(6)[None, :] < R.k[:, None])[:, :, None], J, 0.0)
    gN = pen["grad"] - np.einsum("qkc,qk->qc", Jk, d["z"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d["pushed"], np.linalg.norm(pen["grad"], axis=1) / np.linalg.norm(gN, axis=1), 1.0)


@pytest.mark.parametrize("name", list(PC.BWS))
def test_one_round(wam, name):
    """Measured on an MI355X, the largest difference of a returned step from the rule's: 3.11e-15 with BW3.  With BW6 3.43e-9, at
    one bent row (row 9) whose gradient lies in the row space of J up to 1e-7 of its length: g_N is what a cancellation leaves,
    and the push stretches it to push_cap.  The rule's own fp64 step differs from its long double step by 8.8e-10 at that row
    (by at most 1.4e-12 at the others): the difference is the rule's rounding, not the kernel's.  A row whose ratio
    |g| / |g_N| is below 1e3 is held to BOUND_STEP, every row to BOUND_STEP_ILL."""
    R = wam[name]["R"]
    worst, worst_well, won = 0.0, 0.0, 0
    for what, rows in (("the 15 rows", wam["rows"]), ("the 15 rows bent", PC.bent_rows(wam["w"]))):
        want = R.run(rows, max_steps=1)
        got = call(wam, name, rows, max_steps=1)
        assert np.array_equal(got["status"], want[4]) and np.array_equal(got["steps"], want[3]), (what, got["status"], want[4])
        assert (want[3] == 1).sum() >= 13, "the rows must take the step"
        wins = (want[0] != rows).any(axis=1)      # the step's iterate is the better one: it is what comes back
        assert np.array_equal(wins, (got["configs"] != rows).any(axis=1)), what
        err = np.abs(got["configs"] - want[0]).max(axis=1)
        well = wins & (conditioning(R, rows) < 1e3)
        print("%s, %s: %d rows return their step (%d of them well conditioned); difference from the rule's step per row %s"
              % (name, what, wins.sum(), well.sum(), np.array2string(np.where(wins, err, 0.0), precision=2)))
        worst = max(worst, float(err[wins].max()) if wins.any() else 0.0); won += int(wins.sum())
        worst_well = max(worst_well, float(err[well].max()) if well.any() else 0.0)
        assert got["configs"][~wins].tobytes() == rows[~wins].tobytes(), what + ": a row whose step loses comes back bit for bit"
        reported_is_the_returned_rows(R, got, BOUND_64, "%s, %s" % (name, what))
    assert won >= 15
    print("%s: largest difference from the rule's step %.2e, over the well conditioned rows %.2e" % (name, worst, worst_well))
    assert worst_well <= BOUND_STEP and worst <= BOUND_STEP_ILL, (worst_well, worst)


# ---- 2. the whole loop ---------------------------------------------------------------------------------------------------------

def whole_loop(wam, name, got, R, want, rows, what):
    compared = sorted(PC.FINISH[name])
    print("%s: status %s steps %s; the restatement's %s %s" % (what, got["status"].tolist(), got["steps"].tolist(), want[4].tolist(), want[3].tolist()))
    assert np.array_equal(got["status"][compared], want[4][compared]) and np.array_equal(got["steps"][compared], want[3][compared])
    assert (got["status"][compared] == project.DONE).all() and [int(s) for s in got["steps"][compared]] == [PC.FINISH[name][q] for q in compared]
    err = float(np.abs(got["configs"] - want[0])[compared].max())
    print("%s: compared rows against the restatement's, largest difference %.2e" % (what, err))
    assert err <= BOUND_ROWS, err
    r, c = reported_is_the_returned_rows(R, got, BOUND_64, what)
    done = got["status"] == project.DONE
    assert (r[done] <= PC.PARAMS["tol"] + BOUND_64).all() and (c[done] >= np.asarray(PC.PARAMS["margin"]) - BOUND_64).all()
    # the key of the returned row is never worse than the key of the input
    c0, v0 = R.keys(rows); c1, v1 = R.keys(got["configs"])
    assert PC.not_worse(c1, v1, c0, v0, BOUND_64).all(), (c0, v0, c1, v1)
    assert ((got["configs"] >= wam["w"]["lower"]) & (got["configs"] <= wam["w"]["upper"])).all()


@pytest.mark.parametrize("name", list(PC.BWS))
def test_the_whole_loop(wam, name):
    got = call(wam, name, wam["rows"])
    whole_loop(wam, name, got, wam[name]["R"], wam[name]["want"], wam["rows"], name)
    assert (got["status"] == project.OUT_OF_STEPS).any() and (got["steps"].max() == PC.PARAMS["max_steps"])


def test_three_and_six_rows_in_one_call(oracle, wam):
    """tsr_of mixes BW3 and BW6: the call runs the kernel of six rows, a row of three carries the others as the identity"""
    tsrs = wam["BW6"]["tsrs"] + wam["BW3"]["tsrs"]
    of = np.concatenate([np.arange(N), N + np.arange(N)])
    rows = np.concatenate([wam["rows"], wam["rows"]])
    got = wam["mod"].batch_project_tsr_clear(wam["b64"], tsrs, rows, tsr_of=of)
    for name, part in (("BW6", slice(0, N)), ("BW3", slice(N, 2 * N))):
        sub = {key: got[key][part] for key in OUT}
        whole_loop(wam, name, sub, wam[name]["R"], wam[name]["want"], wam["rows"], "mixed, " + name)
        alone = call(wam, name, wam["rows"])
        print("mixed, %s: bit for bit with the call of its own: %s" % (name, all(sub[k].tobytes() == alone[k].tobytes() for k in OUT)))


# ---- 3. the fixed point --------------------------------------------------------------------------------------------------------

def test_the_fixed_point(wam):
    mod, w = wam["mod"], wam["w"]
    goals = common.wam_goals(48)
    clear = ~PC.in_contact(w, goals, margin=(0.03, 0.01))      # (well clear of the margins in either precision)
    rows = goals[clear][:N]
    assert len(rows) == N
    tsrs = PC.tsrs_of(w, rows, PJ.BW3)
    assert (rows.astype(np.float32).astype(np.float64) != rows).all()
    for bid, tol in ((wam["b64"], PC.PARAMS["tol"]), (wam["b32"], 1e-4)):
        res = mod.batch_project_tsr_clear(bid, tsrs, rows, tsr_of=np.arange(N), tol=tol)
        assert res["configs"].tobytes() == rows.tobytes() and (res["steps"] == 0).all() and (res["status"] == project.DONE).all()
        assert (res["resid"] <= tol).all() and (res["clearance"] >= np.asarray(PC.PARAMS["margin"])).all()
        # max_steps 0: every row comes back bit for bit, the rows in contact too
        both = np.concatenate([rows[:5], wam["rows"]])
        res = mod.batch_project_tsr_clear(bid, tsrs[:5] + wam["BW3"]["tsrs"], both, tsr_of=np.arange(5 + N), tol=tol, max_steps=0)
        assert res["configs"].tobytes() == both.tobytes() and (res["steps"] == 0).all()
        assert res["status"].tolist() == [project.DONE] * 5 + [project.OUT_OF_STEPS] * N
        want = mod.batch_config_clearance(bid, both)["clearance"]
        assert res["clearance"].tobytes() == want.tobytes()
        h = mod.batch_config_tsr(bid, tsrs[:5] + wam["BW3"]["tsrs"], both, tsr_of=np.arange(5 + N))["h"]
        assert np.array_equal(res["resid"], np.abs(h).max(axis=1))


def test_a_row_with_a_nan(wam):
    rows = wam["rows"].copy()
    clean = call(wam, "BW3", rows)
    rows[3, 2] = np.nan; rows[6, 0] = np.inf
    res = call(wam, "BW3", rows)
    for q in (3, 6):
        assert np.isnan(res["configs"][q]).all() and np.isnan(res["resid"][q]) and np.isnan(res["clearance"][q]).all()
        assert res["steps"][q] == 0 and res["status"][q] == project.NOT_FINITE
    keep = [q for q in range(N) if q not in (3, 6)]
    same(res, clean, "the rows beside a non-finite one", keep, keep)


# ---- 4. independence -----------------------------------------------------------------------------------------------------------

def test_independent_of_the_place_in_the_list(wam):
    alone = [call(wam, "BW3", wam["rows"][i:i + 1], tsr_of=np.array([i])) for i in range(N)]
    assert len({int(a["steps"][0]) for a in alone}) >= 4, "rows of different step counts must share a wavefront"
    rng = np.random.default_rng(7)
    for length in (1, 63, 64, 65, 3 * 64 + 7):
        of = rng.integers(0, N, size=length)
        for pos in sorted({0, length // 2, length - 1}):
            of[pos] = (5 + pos) % N
        res = call(wam, "BW3", wam["rows"][of], tsr_of=of)
        for q in range(length):
            same(res, alone[of[q]], "a list of %d, position %d" % (length, q), slice(q, q + 1))


def test_two_shards_and_the_poll_interval(wam):
    of = np.arange(65) % N
    runs = (np.arange(65) // 3 % 2).astype(np.int32)
    one = call(wam, "BW3", wam["rows"][of], tsr_of=of, runs=runs)
    assert "ORC_PROJECT_CLEAR_POLL" not in os.environ
    os.environ["ORC_PROJECT_CLEAR_POLL"] = "1"
    try:
        same(call(wam, "BW3", wam["rows"][of], tsr_of=of, runs=runs), one, "a poll interval of 1 against 4")
    finally:
        del os.environ["ORC_PROJECT_CLEAR_POLL"]
    two = or_cdchomp_amd.Module([0, 0])
    model = common.setup_product_wam(two)
    bid = two.batch_create(model.name, common.wam_goals(2, seed=3), **dict(KW, **SCENES))
    same(two.batch_project_tsr_clear(bid, wam["BW3"]["tsrs"], wam["rows"][of], tsr_of=of, runs=runs), one, "two shards")
    same(two.batch_project_tsr_clear(bid, wam["BW3"]["tsrs"][3:4], wam["rows"][3:4], runs=1), one, "two shards, one row", None, slice(3, 4))
    two.close()


# ---- 5. per-run scenes ---------------------------------------------------------------------------------------------------------

def test_per_run_scenes(oracle, wam):
    w = wam["w"]
    rows = np.concatenate([wam["rows"], wam["rows"]])
    of = np.concatenate([np.arange(N), np.arange(N)])
    runs = np.repeat(np.arange(2, dtype=np.int32), N)
    got = call(wam, "BW3", rows, tsr_of=of, runs=runs)
    same(got, call(wam, "BW3", wam["rows"]), "run 0 is the call without runs", slice(0, N))
    same(got, call(wam, "BW3", wam["rows"], runs=1), "run 1", slice(N, 2 * N))
    assert got["configs"][:N].tobytes() != got["configs"][N:].tobytes(), "the shifted scene must answer differently"
    R = PC.Restated(oracle, w, wam["BW3"]["tsrs"], of, fields_of=[[w["table"]]] * N + [[w["shifted"]]] * N)
    r, c = reported_is_the_returned_rows(R, got, BOUND_64, "per-run scenes")
    done = got["status"] == project.DONE
    assert done[N:].any() and (r[done] <= PC.PARAMS["tol"] + BOUND_64).all() and (c[done] >= np.asarray(PC.PARAMS["margin"]) - BOUND_64).all()
    c0, v0 = R.keys(rows); c1, v1 = R.keys(got["configs"])
    assert PC.not_worse(c1, v1, c0, v0, BOUND_64).all()
    R.destroy()


# ---- 6. precision 32 -----------------------------------------------------------------------------------------------------------

def test_precision_32(wam):
    w = wam["w"]
    R = wam["BW3"]["R"]
    rows = wam["rows"]
    # a box that clips: a three-hundredth of a radian outside the rows' own span, at doubles no float holds
    lower = np.maximum(w["lower"], rows.min(axis=0) - 1.0 / 300.0); upper = np.minimum(w["upper"], rows.max(axis=0) + 1.0 / 300.0)
    assert (lower.astype(np.float32).astype(np.float64) != lower).all() and (upper.astype(np.float32).astype(np.float64) != upper).all()
    got = wam["mod"].batch_project_tsr_clear(wam["b32"], wam["BW3"]["tsrs"], rows, tsr_of=np.arange(N), tol=1e-4, lower=lower, upper=upper)
    print("precision 32: status %s steps %s" % (got["status"].tolist(), got["steps"].tolist()))
    r, c = reported_is_the_returned_rows(R, got, BOUND_32, "precision 32")
    done = got["status"] == project.DONE
    assert done.sum() >= 4
    assert (r[done] <= 1e-4 + BOUND_32).all() and (c[done] >= np.asarray(PC.PARAMS["margin"]) - BOUND_32).all()
    assert ((got["configs"] >= lower) & (got["configs"] <= upper)).all(), "a clipped row lies inside the box"
    # one bent row in a box of its own, a three-thousandth of a radian wide: the row is off its TSR, every step towards it is clipped,
    # and the better iterate that comes back sits on the box
    bent = PC.bent_rows(w)[:1]
    lo1 = bent[0] - 1.0 / 3000.0; hi1 = bent[0] + 1.0 / 3000.0
    one = wam["mod"].batch_project_tsr_clear(wam["b32"], wam["BW3"]["tsrs"][:1], bent, tol=1e-4, lower=lo1, upper=hi1)
    at_box = (np.abs(one["configs"] - lo1) < 1e-6) | (np.abs(one["configs"] - hi1) < 1e-6)
    print("precision 32, one bent row in a tight box: status %d steps %d, %d entries sit on the box" % (one["status"][0], one["steps"][0], at_box.sum()))
    assert one["steps"][0] >= 1 and at_box.sum() >= 1
    assert ((one["configs"] >= lo1) & (one["configs"] <= hi1)).all(), "a clipped row lies inside the box"
    # (an untouched dof as the caller's double: test_the_fixed_point for whole rows, test_tree_robot for single columns)


# ---- 7. the 30-dof tree --------------------------------------------------------------------------------------------------------

def test_tree_robot(oracle):
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_tree30(mod)
    case = PJ.tree_case(oracle)
    names, grids, poses = common.config5_oracle_fields(oracle)
    fields = [CL.Field(oracle, g, None, p) for g, p in zip(grids, poses)]
    tab = CL.Tables(oracle, model, case["base"], case["dofvals"], case["adofs"], fields)
    n_t = len(case["tsrs"])
    margin = np.asarray(PC.PARAMS["margin"]); at = tuple(margin + PC.PARAMS["slack"])
    states = set()
    # the TSRs of the case with three rows: in precision 32 a workgroup's states of three rows fit the LDS, all others live in the workspace
    Rs, ds = PJ.target_frames(model, case["base"], case["dofvals"], case["adofs"], "L6", PJ.IDENT, case["qstar"])
    three_rows = PJ.tsrs_at(Rs, ds, PJ.BW3)
    ora3 = PJ.OracleTsrs(oracle, model, case["base"], case["dofvals"], case["adofs"], "L6", PJ.IDENT, three_rows, tsr_of=np.arange(n_t))
    six = dict(tsrs=case["tsrs"], ora=case["ora"], k=6)
    for precision, bound, tol, tc in ((64, BOUND_64, PC.PARAMS["tol"], six), (32, BOUND_32, 1e-4, six), (32, BOUND_32, 1e-4, dict(tsrs=three_rows, ora=ora3, k=3))):
        bid = mod.batch_create(model.name, common.config5_goals(2), **dict(common.CONFIG5_KW, n_points=4, precision=precision))
        state = mod.batch_project_state(bid)[0 if tc["k"] == 3 else 1]
        states.add((precision, tc["k"], state))
        seeds = case["seeds"]
        res = mod.batch_project_tsr_clear(bid, tc["tsrs"], seeds, tsr_of=np.arange(n_t), link="L6", tol=tol)
        pen0 = mod.batch_config_penetration(bid, seeds, margin=at)
        print("tree, precision %d, %d rows (state in %s): status %s steps %s; cost at the seeds %s" % (precision, tc["k"], state, res["status"].tolist(), res["steps"].tolist(),
              np.array2string(pen0["cost"].sum(axis=1), precision=2)))
        h = tc["ora"].evaluate(res["configs"], np.arange(n_t))[0]
        clr = np.array([PN.restate(tab, q, 0, fields, PC.PARAMS["margin"])["clearance"] for q in res["configs"]])
        done = res["status"] == project.DONE
        assert done.any()
        assert (np.abs(h).max(axis=1)[done] <= tol + bound).all() and (clr[done] >= margin - bound).all()
        assert np.abs(np.abs(h).max(axis=1) - res["resid"]).max() <= bound and np.abs(clr - res["clearance"]).max() <= bound
        assert (res["steps"] > 0).all()
        # a dof that moves neither the link nor a sphere within the margins has a zero Jacobian column and a zero gradient entry:
        # the step leaves it where it was.  `still`: the dofs whose restated gradient entry is zero, at margins a centimetre
        # wider, at every iterate the rule visits in three steps; the device's three steps leave them bit for bit
        hist = []

        def pen(rows, m):
            out = [PN.restate(tab, q, 0, fields, m) for q in rows]
            return {key: np.array([o[key] for o in out]) for key in ("cost", "grad", "clearance")}

        project_clear.project_clear(tc["ora"].evaluate, lambda rows, m, index: pen(rows, m), seeds, k=tc["k"], indexed=True, tol=tol, max_steps=3,
                                    dtype=np.float64 if precision == 64 else np.float32, history=hist)
        still = np.tile(~case["moving"], (n_t, 1))
        for index, iterates, _, _, _ in hist:
            still[index] &= pen(iterates.astype(np.float64), (at[0] + 0.01, at[1] + 0.01))["grad"] == 0
        three = mod.batch_project_tsr_clear(bid, tc["tsrs"], seeds, tsr_of=np.arange(n_t), link="L6", tol=tol, max_steps=3)
        print("tree, precision %d: %d of %d entries are still; three steps: status %s steps %s" % (precision, still.sum(), still.size,
              three["status"].tolist(), three["steps"].tolist()))
        assert still.sum() >= n_t * 8 and (three["steps"] == 3).all()
        assert np.array_equal(three["configs"][still].view(np.uint64), seeds[still].view(np.uint64)), "those dofs come back bit for bit"
        assert (seeds[still].astype(np.float32).astype(np.float64) != seeds[still]).all()
        assert (three["configs"][:, case["moving"]] != seeds[:, case["moving"]]).any()
        mod.batch_destroy(bid)
    assert states == {(64, 6, "global"), (32, 6, "global"), (32, 3, "lds")}, states
    ora3.destroy()
    case["ora"].destroy()
    mod.close()


# ---- 8. nothing to clear -------------------------------------------------------------------------------------------------------

# 16 goals of common.wam_goals(48) that are not in contact and whose bent rows the rule keeps clear on their way back to the
# goal's hand pose (chosen with or_cdchomp_amd/project_clear.py on the host; the test asserts it on the rule's trace)
CLEAR_16 = [3, 4, 5, 7, 10, 11, 12, 14, 16, 18, 20, 21, 25, 27, 28, 29]


@pytest.mark.parametrize("name, precision", [("BW3", 64), ("BW6", 64), ("BW3", 32)])
def test_nothing_to_clear_is_the_projection(oracle, wam, name, precision):
    """Rows off their TSRs that no visited iterate brings into contact, margins (0, 0) and slack 0: no cost, no push, every
    clearance at the margins, so the clear projection is the projection.  The two kernels take their step from one text
    (project_step.h): the rows, residuals, steps and statuses agree bit for bit."""
    mod, w = wam["mod"], wam["w"]
    assert not set(CLEAR_16) & set(PC.CONTACT_48)
    goals = common.wam_goals(48)[CLEAR_16]
    rows = np.clip(goals + PC.BENT * np.random.default_rng(21).standard_normal(goals.shape), w["lower"], w["upper"])
    tsrs = PC.tsrs_of(w, goals, PC.BWS[name])
    p = dict(tol=PC.PARAMS["tol"] if precision == 64 else 1e-4, mu=PC.PARAMS["mu"], step_cap=PC.PARAMS["step_cap"], max_steps=30)
    # the premise, on the rule's trace
    R = PC.Restated(oracle, w, tsrs, np.arange(len(rows)))
    hist = []
    rule = R.run(rows, history=hist, dtype=np.float64 if precision == 64 else np.float32, margin=(0.0, 0.0), slack=0.0, **p)
    R.destroy()
    lowest = min(float(clr.min()) for _, _, _, _, clr in hist)
    print("%s, precision %d: the rule visits %d rounds, steps %s; largest cost %g, lowest clearance %.4f"
          % (name, precision, len(hist), rule[3].tolist(), max(float(U.max()) for _, _, _, U, _ in hist), lowest))
    assert (rule[3] >= 2).all(), "every row must take steps"
    for _, _, _, U, clr in hist:
        assert (U == 0).all() and (clr >= 0).all(), "no visited iterate has a cost, and every clearance is at or above the margins"
    bid = wam["b64"] if precision == 64 else wam["b32"]
    want = mod.batch_project_tsr(bid, tsrs, rows, tsr_of=np.arange(len(rows)), **p)
    got = mod.batch_project_tsr_clear(bid, tsrs, rows, tsr_of=np.arange(len(rows)), margin=(0.0, 0.0), slack=0.0, **p)
    print("%s, precision %d: steps %s status %s" % (name, precision, got["steps"].tolist(), got["status"].tolist()))
    assert (want[2] >= 1).all() and (want[3] == project.DONE).all()
    for key, x in zip(("configs", "resid", "steps", "status"), want):
        y = got[key]
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (name, precision, key, x, y)


@pytest.mark.parametrize("name", list(PC.BWS))
def test_a_pivot_that_is_not_positive_stalls_the_row(wam, name):
    """A TSR on the robot's base link, which no joint moves, and mu 0: J is zero, A = J J^T is zero, and the first pivot of its
    factor is not positive.  Both projections stop the row at once: a singular system, no step, the row as it came."""
    mod, bid = wam["mod"], wam["b64"]
    rows = wam["rows"][:3]
    link = wam["model"].link_names[0]
    tsrs = [robots.Tsr(T0w_d=(0.3, -0.2, 1.5), Bw=PC.BWS[name])]
    ev = mod.batch_config_tsr(bid, tsrs, rows, link=link)
    r = np.abs(ev["h"]).max(axis=1)
    assert (ev["jac"] == 0).all() and (r > 1e-3).all(), "the premise: no joint moves the link, and it is off the TSR"
    p = dict(link=link, mu=0.0, tol=PC.PARAMS["tol"], step_cap=PC.PARAMS["step_cap"], max_steps=30)
    out, resid, steps, status = mod.batch_project_tsr(bid, tsrs, rows, **p)
    got = mod.batch_project_tsr_clear(bid, tsrs, rows, **p)
    for what, o, rs, st, ss in (("project", out, resid, steps, status), ("clear", got["configs"], got["resid"], got["steps"], got["status"])):
        assert (ss == project.STALLED).all() and (st == 0).all(), (what, ss, st)
        assert o.tobytes() == rows.tobytes() and np.array_equal(rs, r), what


# ---- 9. rejections -------------------------------------------------------------------------------------------------------------

def test_rejections(wam):
    mod, bid = wam["mod"], wam["b64"]
    lib, h = mod._lib, mod._h
    tsrs = wam["BW3"]["tsrs"]
    rec, _ = mod._tsr_records(bid, tsrs[:2], None, None)
    cf = np.ascontiguousarray(wam["rows"][:3]); of = np.array([0, 1, 0], dtype=np.int32); rq = np.array([0, 1, 0], dtype=np.int32)
    n = cf.shape[1]
    ro = np.zeros((3, n)); rs = np.zeros(3); cl = np.zeros((3, 2)); st = np.zeros(3, dtype=np.int32); ss = np.zeros(3, dtype=np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(_capi.c_double_p)
    ip = lambda a: None if a is None else a.ctypes.data_as(_capi.c_int_p)

    def proj(bid=bid, n_tsr=2, rec=rec, n_q=3, of=of, rq=rq, cf=cf, lo=None, hi=None, max_steps=40, tol=1e-6, mu=1e-8, cap=0.5, push=0.2, mf=0.02,
             ms=0.0, slack=2e-3, ro=ro, rs=rs, cl=cl, st=st, ss=ss):
        return lib.orc_batch_project_tsr_clear(h, bid, n_tsr, rec, n_q, ip(of), ip(rq), dp(cf), dp(lo), dp(hi), max_steps, tol, mu, cap, push, mf, ms,
                                               slack, dp(ro), dp(rs), dp(cl), ip(st), ip(ss))

    def good():
        assert proj() == 0 and np.abs(ro).max() > 0 and set(ss.tolist()) <= {0, 2}

    def other_link(link):
        r, _ = mod._tsr_records(bid, tsrs[:2], None, None)
        r[1].ee_link = link
        return r

    def bad_pose():
        r, _ = mod._tsr_records(bid, tsrs[:2], None, None)
        r[0].T0w[1] = float("nan")
        return r

    loose = mod._tsr_records(bid, [tsrs[0], robots.Tsr(Bw=[[-1, 1]] * 3 + [[-3, 3]] * 3)], None, None)[0]
    nan, inf = float("nan"), float("inf")
    lo = wam["w"]["lower"].copy(); hi = wam["w"]["upper"].copy()
    crossed = lo.copy(); crossed[4] = hi[4] + 0.1
    W = "project tsr clear: "
    good()
    cases = [(dict(bid=bid + 999), "you must pass a created run"), (dict(n_q=0), W + "n_q must lie"), (dict(n_q=-4), W + "n_q must lie"), (dict(n_tsr=0), "n_tsr must be >= 1"),
             (dict(of=np.array([0, 2, 0], dtype=np.int32)), W + "a tsr_of_q entry"), (dict(of=np.array([0, -1, 0], dtype=np.int32)), W + "a tsr_of_q entry"),
             (dict(rec=None), "tsrs"), (dict(cf=None), W + "configs [n_q][n] is NULL"),
             (dict(rec=other_link(len(wam["model"].link_names))), W + "ee_link lies outside"), (dict(rec=other_link(-2)), W + "ee_link lies outside"),
             (dict(rec=loose), W + "a TSR enforces no row"), (dict(rec=bad_pose()), W + "a TSR's poses must be finite"),
             (dict(ro=None), W + "configs_out, resid_out, clearance_out, steps_out and status_out are required"), (dict(rs=None), W + "configs_out"),
             (dict(cl=None), W + "configs_out"), (dict(st=None), W + "configs_out"), (dict(ss=None), W + "configs_out"),
             (dict(tol=nan), W + "tol must be a positive number"), (dict(tol=0.0), W + "tol"), (dict(tol=-1e-6), W + "tol"),
             (dict(cap=nan), W + "step_cap must be a positive number"), (dict(cap=0.0), W + "step_cap"), (dict(cap=-0.5), W + "step_cap"),
             (dict(mu=nan), W + "mu must be a number >= 0"), (dict(mu=-1e-8), W + "mu"),
             (dict(max_steps=-1), W + "max_steps must lie in [0, 256]"), (dict(max_steps=257), W + "max_steps"),
             (dict(lo=crossed, hi=hi), W + "lower[c] <= upper[c] must hold"),
             (dict(rq=np.array([0, 2, 0], dtype=np.int32)), "a run_of_q entry lies outside"), (dict(rq=np.array([0, -1, 0], dtype=np.int32)), "a run_of_q entry"),
             (dict(mf=nan), W + "the margins are finite and not negative"), (dict(mf=-0.01), W + "the margins"), (dict(ms=inf), W + "the margins"),
             (dict(ms=-1.0), W + "the margins"), (dict(mf=inf), W + "the margins"),
             (dict(push=nan), W + "push_cap must be a positive number"), (dict(push=0.0), W + "push_cap"), (dict(push=-0.2), W + "push_cap"),
             (dict(slack=nan), W + "slack must be a finite number >= 0"), (dict(slack=-1e-3), W + "slack"), (dict(slack=inf), W + "slack")]
    for kw, text in cases:
        assert proj(**kw) != 0, kw
        msg = lib.orc_last_error(h).decode()
        assert text in msg, (kw, msg)
        good()
    assert proj(max_steps=256, mu=0.0, lo=lo, hi=hi, slack=0.0, mf=0.0) == 0 and proj(max_steps=0) == 0 and proj(of=None, rq=None) == 0


def test_a_floating_base_batch_and_a_robot_without_a_manipulator_are_rejected(oracle, wam):
    mod = or_cdchomp_amd.Module(0)
    base = np.asarray(PJ.unit_base(), dtype=np.float64)
    model, _, dofvals, adofs = common.wam_state()
    mod.add_robot(model, transform=list(base), dof_values=dofvals, active_dofs=adofs)
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    bid = mod.batch_create(model.name, common.wam_goals(1, seed=3), basegoals=base[None, :], floating_base=1, **KW)
    rows = np.concatenate([np.tile(base, (2, 1)), wam["rows"][:2]], axis=1)
    with pytest.raises(RuntimeError, match="project tsr clear: a floating-base batch is not projected"):
        mod.batch_project_tsr_clear(bid, wam["BW3"]["tsrs"][:2], rows, tsr_of=np.arange(2), lower=None, upper=None)
    assert mod.batch_config_tsr(bid, wam["BW3"]["tsrs"][:2], rows[:1])["h"].shape == (1, 6)
    mod.close()
    mod = or_cdchomp_amd.Module(0)
    tree = common.setup_product_tree30(mod)
    case = PJ.tree_case(oracle)
    bid = mod.batch_create(tree.name, common.config5_goals(1), **dict(common.CONFIG5_KW, n_points=4))
    with pytest.raises(RuntimeError, match="project tsr clear: ee_link -1 names the active manipulator"):
        mod.batch_project_tsr_clear(bid, case["tsrs"], case["seeds"][:1])
    case["ora"].destroy()
    mod.close()
