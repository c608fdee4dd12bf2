"""-m gpu: the value and Jacobian of TSRs at configurations (orc_batch_config_tsr) and the projection onto them
(orc_batch_project_tsr) on the device, against the oracle's con_tsr and the restatement of tests/project.py (project.project
around the oracle).  The premises -- that the chosen inputs converge, away from the tolerance and from the angle singularities --
are tests/test_host_project.py's.

The bounds of the comparison with the oracle are measured ones (NOTES/project-tsr.md): ten times the largest absolute difference
seen on an MI355X over every comparison of this file, rounded up to a power of ten; the margin is for other cards and the ~1 ulp
sincos of the device."""
import ctypes as C

import numpy as np
import pytest

import common
import project as PJ
import or_cdchomp_amd
from or_cdchomp_amd import _capi, project, robots, scenes

pytestmark = pytest.mark.gpu

# measured on an MI355X, the largest over this file's comparisons: h and J against eval_contsr 1.33e-15 (fp64) and 4.37e-7
# (precision 32); projected rows against the restatement's 9.44e-16 on the WAM's P1 inputs, 4.55e-15 on the tree
BOUND_64 = 1e-13
BOUND_32 = 1e-5
BOUND_ROWS = 1e-14
BOUND_ROWS_TREE = 1e-13
KW = dict(n_points=4, lambda_=100.0, obs_factor=200.0)
BOTH = np.concatenate([np.arange(PJ.N_TARGETS), np.arange(PJ.N_TARGETS)])      # the TSR of the 32 q* and of the 32 seeds


def setup(mod, base, floating=False):
    model, _, dofvals, adofs = common.wam_state()
    mod.add_robot(model, transform=list(base), dof_values=dofvals, active_dofs=adofs)
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    return model


@pytest.fixture(scope="module")
def wam():
    """the WAM on the unit base with a batch of each precision: dict(mod, model, b64, b32)"""
    mod = or_cdchomp_amd.Module(0)
    model = setup(mod, PJ.unit_base())
    goals = common.wam_goals(2, seed=3)
    out = dict(mod=mod, model=model, b64=mod.batch_create(model.name, goals, **KW), b32=mod.batch_create(model.name, goals, precision=32, **KW))
    yield out
    mod.close()


@pytest.fixture(scope="module")
def p1(oracle):
    """the P1 inputs with the restatement's answer: dict(case, rows, resid, steps, status)"""
    case = PJ.wam_case(oracle, PJ.unit_base(), PJ.BW6)
    res = case["ora"].project(case["seeds"], lower=case["lower"], upper=case["upper"], tol=PJ.TOL)
    return dict(case=case, res=res)


def same(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x = np.asarray(x); y = np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), what


# ---- 1. value and Jacobian against the oracle --------------------------------------------------------------------------------

VARIANTS = {"six rows": dict(Bw=PJ.BW6), "three rows": dict(Bw=PJ.BW3), "one row": dict(Bw=PJ.BW1),
            "link wam7": dict(Bw=PJ.BW6, link="wam7", tool=PJ.IDENT), "Twe": dict(Bw=PJ.BW6, twe=PJ.TWE)}


def against_oracle(mod, bid, case, rows, tsr_of, bound, what, **address):
    dev = mod.batch_config_tsr(bid, case["tsrs"], rows, tsr_of=tsr_of, **address)
    h, J = case["ora"].evaluate(rows, tsr_of)
    k = case["ora"].ks(tsr_of)
    assert np.array_equal(dev["k"], k)
    err_h = float(np.abs(dev["h"] - h).max()); err_J = float(np.abs(dev["jac"] - J).max())
    print("%s: largest difference from eval_contsr: h %.2e, jac %.2e (|h| up to %.2f, |jac| up to %.2f)"
          % (what, err_h, err_J, np.abs(h).max(), np.abs(J).max()))
    assert np.abs(h).max() > 1e-3 and np.abs(J).max() > 0.1, "the comparison must be about something"
    for q in range(len(rows)):      # rows from k on are zero
        assert not dev["h"][q, k[q]:].any() and not dev["jac"][q, k[q]:].any()
    assert max(err_h, err_J) <= bound, (what, err_h, err_J)
    return dev


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_value_and_jacobian_match_the_oracle(oracle, wam, variant):
    v = dict(VARIANTS[variant])
    address = dict(link=v["link"]) if "link" in v else {}
    case = PJ.wam_case(oracle, PJ.unit_base(), v["Bw"], v.get("link", "handbase"), v.get("tool", PJ.TOOL), v.get("twe", PJ.IDENT))
    rows = np.concatenate([case["qstar"], case["seeds"]])
    d64 = against_oracle(wam["mod"], wam["b64"], case, rows, BOTH, BOUND_64, variant + ", fp64", **address)
    against_oracle(wam["mod"], wam["b32"], case, rows, BOTH, BOUND_32, variant + ", precision 32", **address)
    if variant == "six rows":      # the three ways to name the active manipulator's end effector are one
        for other in (dict(manip="arm"), dict(link="handbase")):
            res = wam["mod"].batch_config_tsr(wam["b64"], case["tsrs"], rows, tsr_of=BOTH, **other)
            if "manip" in other:
                same([res["h"], res["jac"]], [d64["h"], d64["jac"]], "manip arm is the active manipulator")
            else:      # the link's own frame: without the tool the value differs
                assert np.abs(res["h"] - d64["h"]).max() > 0.1
    case["ora"].destroy()


def test_the_default_base(oracle):
    """the WAM's default base, whose matrix is not a rotation: value and Jacobian are the oracle's all the same"""
    mod = or_cdchomp_amd.Module(0)
    base = list(robots.WAM_BASE_POSE)
    model = setup(mod, base)
    bid = mod.batch_create(model.name, common.wam_goals(1, seed=3), **KW)
    case = PJ.wam_case(oracle, base, PJ.BW6)
    against_oracle(mod, bid, case, np.concatenate([case["qstar"], case["seeds"]]), BOTH, BOUND_64, "default base, fp64")
    case["ora"].destroy()
    mod.close()


def test_jacobian_is_the_derivative_of_the_value(wam, p1):
    """central differences of the call's own h (unit base: with the default base the reference's Jacobian is not the exact
    derivative); step and tolerance of test_oracle_tsr_jacobian_is_the_derivative_of_its_value"""
    case = p1["case"]
    pick = np.arange(0, PJ.N_TARGETS, 4)
    rows = case["seeds"][pick]
    eps = 1e-6
    n = rows.shape[1]
    moved = np.repeat(rows, 2 * n, axis=0).reshape(len(rows), n, 2, n)
    for j in range(n):
        moved[:, j, 0, j] += eps; moved[:, j, 1, j] -= eps
    mod, bid = wam["mod"], wam["b64"]
    at = mod.batch_config_tsr(bid, case["tsrs"], rows, tsr_of=pick)
    h = mod.batch_config_tsr(bid, case["tsrs"], moved.reshape(-1, n), tsr_of=np.repeat(pick, 2 * n))["h"].reshape(len(rows), n, 2, 6)
    d = (h[:, :, 0] - h[:, :, 1]) / (2 * eps)                      # [row][j][6]
    worst = float(np.abs(np.swapaxes(d, 1, 2) - at["jac"]).max())
    print("jac against central differences of h: largest difference %.2e" % worst)
    assert np.allclose(at["jac"], np.swapaxes(d, 1, 2), rtol=1e-5, atol=2e-6)


def test_a_floating_base_batch_is_evaluated(oracle):
    mod = or_cdchomp_amd.Module(0)
    base = np.asarray(PJ.unit_base(), dtype=np.float64)
    model = setup(mod, base)
    _, _, dofvals, adofs = common.wam_state()
    bid = mod.batch_create(model.name, common.wam_goals(1, seed=3), basegoals=base[None, :], floating_base=1, **KW)
    assert mod.batch_dims(bid)[2] == 14
    qstar, seeds = PJ.p1_inputs()
    rows = np.zeros((6, 14))
    for i in range(6):
        quat = robots.quat_mul(list(base[3:]), robots.quat_from_axis_angle((0.3, -1.0, 0.5), 0.1 * i))
        rows[i] = list(base[:3] + [0.02 * i, -0.01 * i, 0.015 * i]) + list(quat) + list(seeds[i])
    Rs, ds = PJ.target_frames(model, base, dofvals, adofs, "handbase", PJ.TOOL, qstar[:6])
    tsrs = PJ.tsrs_at(Rs, ds, PJ.BW6)
    ora = PJ.OracleTsrs(oracle, model, list(base), dofvals, adofs, "handbase", PJ.TOOL, tsrs, tsr_of=np.arange(6), floating=True)
    dev = against_oracle(mod, bid, dict(tsrs=tsrs, ora=ora), rows, np.arange(6), BOUND_64, "floating base, fp64")
    assert np.abs(dev["jac"][:, :, :7]).max() > 0.1
    with pytest.raises(RuntimeError, match="floating"):
        mod.batch_project_tsr(bid, tsrs, rows, tsr_of=np.arange(6), lower=None, upper=None)
    assert mod.batch_config_tsr(bid, tsrs, rows[:1])["h"].shape == (1, 6)
    ora.destroy()
    mod.close()


# ---- 2. bit for bit across placement -----------------------------------------------------------------------------------------

def answers(mod, bid, tsrs, rows, tsr_of, lower, upper, **kw):
    ev = mod.batch_config_tsr(bid, tsrs, rows, tsr_of=tsr_of)
    pr = mod.batch_project_tsr(bid, tsrs, rows, tsr_of=tsr_of, lower=lower, upper=upper, tol=PJ.TOL, **kw)
    return [ev["h"], ev["jac"]] + list(pr)


def at(res, i):
    return [r[i] for r in res]


def check_positions(mod, bid, tsrs, seeds, lower, upper, lengths, what):
    n_t = len(tsrs)
    alone = [answers(mod, bid, [tsrs[i]], seeds[i:i + 1], None, lower, upper) for i in range(n_t)]
    rng = np.random.default_rng(7)
    for length in lengths:
        of = rng.integers(0, n_t, size=length)
        for pos in sorted({0, length // 2, length - 1}):
            of[pos] = (5 + pos) % n_t
        res = answers(mod, bid, tsrs, seeds[of], of, lower, upper)
        for q in range(length):
            same(at(res, q), at(alone[of[q]], 0), "%s: a list of %d, position %d" % (what, length, q))
        # the TSRs in another order, tsr_of permuted with them
        perm = rng.permutation(n_t)
        inv = np.argsort(perm)
        again = answers(mod, bid, [tsrs[p] for p in perm], seeds[of], inv[of], lower, upper)
        same(again, res, "%s: permuted TSRs, a list of %d" % (what, length))
    return alone


def test_bit_for_bit_across_positions_and_lengths(wam, p1):
    case = p1["case"]
    alone = check_positions(wam["mod"], wam["b64"], case["tsrs"], case["seeds"], case["lower"], case["upper"], (1, 63, 64, 65, 129), "wam")
    assert len({int(a[4][0]) for a in alone}) >= 2, "rows of different step counts must share a wavefront"
    check_positions(wam["mod"], wam["b32"], case["tsrs"], case["seeds"], case["lower"], case["upper"], (65,), "wam, precision 32")


def test_bit_for_bit_on_two_shards(wam, p1):
    case = p1["case"]
    two = or_cdchomp_amd.Module([0, 0])
    model = setup(two, PJ.unit_base())
    bid = two.batch_create(model.name, common.wam_goals(2, seed=3), **KW)
    of = np.arange(65) % PJ.N_TARGETS
    one = answers(wam["mod"], wam["b64"], case["tsrs"], case["seeds"][of], of, case["lower"], case["upper"])
    other = answers(two, bid, case["tsrs"], case["seeds"][of], of, case["lower"], case["upper"])
    same(other, one, "two shards")
    same(answers(two, bid, case["tsrs"][3:4], case["seeds"][3:4], None, case["lower"], case["upper"]), at(one, slice(3, 4)), "two shards, one query")
    two.close()


# ---- 3. the projection -------------------------------------------------------------------------------------------------------

def test_projection_of_the_p1_inputs(wam, p1):
    case = p1["case"]
    want_rows, want_resid, want_steps, want_status = p1["res"]
    mod = wam["mod"]
    of = np.arange(PJ.N_TARGETS)
    rows, resid, steps, status = mod.batch_project_tsr(wam["b64"], case["tsrs"], case["seeds"], tsr_of=of, tol=PJ.TOL)      # (the robot's limits by default)
    assert (status == project.DONE).all(), status
    assert np.array_equal(steps, want_steps), (steps, want_steps)
    err = float(np.abs(rows - want_rows).max())
    h = case["ora"].evaluate(rows, of)[0]
    print("projected rows against the restatement's: largest difference %.2e; steps %s; oracle residual up to %.2e, device's %.2e"
          % (err, np.bincount(steps).tolist(), np.abs(h).max(), resid.max()))
    assert err <= BOUND_ROWS
    assert np.abs(h).max() <= PJ.TOL + BOUND_64      # independent of any restatement
    assert (resid <= PJ.TOL).all() and np.abs(resid - np.abs(h).max(axis=1)).max() <= BOUND_64
    assert ((rows >= case["lower"]) & (rows <= case["upper"])).all()
    assert np.abs(rows - case["seeds"]).max() > 0.05 and np.abs(rows - case["qstar"]).max() > 1e-3, "another solution than q*, not the seed"


def test_wide_seeds_have_the_restatements_statuses(oracle, wam):
    case = PJ.wam_case(oracle, PJ.unit_base(), PJ.BW6, spread=1.0)
    want = case["ora"].project(case["seeds"], lower=case["lower"], upper=case["upper"], tol=PJ.TOL)
    rows, resid, steps, status = wam["mod"].batch_project_tsr(wam["b64"], case["tsrs"], case["seeds"], tsr_of=np.arange(PJ.N_TARGETS), tol=PJ.TOL)
    print("wide seeds: statuses", status.tolist(), "steps", steps.tolist(), "restatement's steps", want[2].tolist())
    assert np.array_equal(status, want[3])
    assert (status == project.OUT_OF_STEPS).any() and (status == project.DONE).any()
    # a row that is not done is never worse than its input
    r0 = np.abs(case["ora"].evaluate(case["seeds"], np.arange(PJ.N_TARGETS))[0]).max(axis=1)
    assert (resid <= r0 + BOUND_64).all()
    case["ora"].destroy()


def test_an_unreachable_target(wam):
    mod = wam["mod"]
    far = [robots.Tsr(Bw=PJ.BW6, **PJ.UNREACHABLE)]
    start = np.array([robots.WAM_START])
    r0 = np.abs(mod.batch_config_tsr(wam["b64"], far, start)["h"]).max()
    rows, resid, steps, status = mod.batch_project_tsr(wam["b64"], far, start)
    print("unreachable: residual %.3f from %.3f in %d steps" % (resid[0], r0, steps[0]))
    assert status[0] == project.OUT_OF_STEPS and steps[0] == 30
    assert resid[0] <= r0 and np.isfinite(rows).all() and np.isfinite(resid).all()
    assert np.abs(mod.batch_config_tsr(wam["b64"], far, rows)["h"]).max() == resid[0]


def test_projection_in_precision_32(wam, p1):
    case = p1["case"]
    of = np.arange(PJ.N_TARGETS)
    rows, resid, steps, status = wam["mod"].batch_project_tsr(wam["b32"], case["tsrs"], case["seeds"], tsr_of=of, tol=1e-4)
    h = case["ora"].evaluate(rows, of)[0]
    print("precision 32: steps %s, oracle residual up to %.2e, device's %.2e" % (np.bincount(steps).tolist(), np.abs(h).max(), resid.max()))
    assert (status == project.DONE).all(), status
    assert np.abs(h).max() <= 1e-4 + BOUND_32
    assert ((rows >= case["lower"]) & (rows <= case["upper"])).all()      # (the limits as the device rounds them lie inside... or on them)


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------

def test_max_steps_zero_is_the_evaluation(wam, p1):
    case = p1["case"]
    of = np.arange(PJ.N_TARGETS)
    for bid in (wam["b64"], wam["b32"]):
        rows, resid, steps, status = wam["mod"].batch_project_tsr(bid, case["tsrs"], case["seeds"], tsr_of=of, max_steps=0)
        assert rows.tobytes() == case["seeds"].tobytes() and (steps == 0).all() and (status == project.OUT_OF_STEPS).all()
        h = wam["mod"].batch_config_tsr(bid, case["tsrs"], case["seeds"], tsr_of=of)["h"]
        assert np.array_equal(resid, np.abs(h).max(axis=1))


def test_a_row_within_tol_comes_back_bit_for_bit(wam, p1):
    case = p1["case"]
    of = np.arange(PJ.N_TARGETS)
    for bid, tol in ((wam["b64"], PJ.TOL), (wam["b32"], 1e-4)):
        rows, resid, steps, status = wam["mod"].batch_project_tsr(bid, case["tsrs"], case["qstar"], tsr_of=of, tol=tol)
        assert rows.tobytes() == case["qstar"].tobytes() and (steps == 0).all() and (status == project.DONE).all() and (resid <= tol).all()


def test_a_row_with_a_nan(wam, p1):
    case = p1["case"]
    mod, bid = wam["mod"], wam["b64"]
    of = np.arange(8)
    clean = answers(mod, bid, case["tsrs"], case["seeds"][:8], of, case["lower"], case["upper"])
    seeds = case["seeds"][:8].copy()
    seeds[3, 2] = np.nan; seeds[6, 0] = np.inf
    res = answers(mod, bid, case["tsrs"], seeds, of, case["lower"], case["upper"])
    for q in (3, 6):
        assert np.isnan(res[0][q]).all() and np.isnan(res[1][q]).all()      # (six rows: all of h and jac)
        assert np.isnan(res[2][q]).all() and np.isnan(res[3][q]) and res[4][q] == 0 and res[5][q] == project.NOT_FINITE
    keep = [q for q in range(8) if q not in (3, 6)]
    same(at(res, keep), at(clean, keep), "the rows beside a non-finite one")


def test_a_box_that_excludes_the_solution(oracle, wam, p1):
    case = p1["case"]
    of = np.arange(PJ.N_TARGETS)
    lower = case["lower"].copy(); upper = case["upper"].copy()
    # the elbow kept 0.3 below every q*: no other solution of the redundant arm lies inside either (the restatement's residuals
    # stay above 0.1; the wrist columns would let some rows in)
    upper[3] = case["qstar"][:, 3].min() - 0.3
    assert upper[3] > lower[3] + 1.0
    seeds = np.minimum(case["seeds"], upper)
    want = case["ora"].project(seeds, lower=lower, upper=upper, tol=PJ.TOL)
    rows, resid, steps, status = wam["mod"].batch_project_tsr(wam["b64"], case["tsrs"], seeds, tsr_of=of, lower=lower, upper=upper, tol=PJ.TOL)
    print("narrowed box: statuses", np.bincount(status, minlength=4).tolist(), "restatement's", np.bincount(want[3], minlength=4).tolist())
    assert ((rows >= lower) & (rows <= upper)).all()
    assert set(status.tolist()) <= {project.STALLED, project.OUT_OF_STEPS}
    assert np.array_equal(status, want[3])


# ---- 5. the 30-dof tree ------------------------------------------------------------------------------------------------------

def test_tree_robot(oracle):
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_tree30(mod)
    case = PJ.tree_case(oracle)
    for precision, bound in ((64, BOUND_64), (32, BOUND_32)):
        bid = mod.batch_create(model.name, common.config5_goals(2), **dict(common.CONFIG5_KW, n_points=4, precision=precision))
        assert mod.batch_plan(bid)["variant"] & 1, "the robot must be a tree"
        print("tree, precision %d: a lane's state lives in %s" % (precision, mod.batch_project_state(bid)))
        n_t = len(case["tsrs"])
        of = np.concatenate([np.arange(n_t), np.arange(n_t)])
        rows = np.concatenate([case["qstar"], case["seeds"]])
        dev = against_oracle(mod, bid, case, rows, of, bound, "tree, precision %d" % precision, link="L6")
        still = ~case["moving"]
        assert case["moving"].sum() == 9 and not dev["jac"][:, :, still].any(), "a dof that does not move the link has a zero column"
        assert (np.abs(dev["jac"][:, :, case["moving"]]).max(axis=(0, 1)) > 0).all()
        lower = np.asarray(model.limit_lower); upper = np.asarray(model.limit_upper)
        out = mod.batch_project_tsr(bid, case["tsrs"], case["seeds"], tsr_of=np.arange(n_t), link="L6", tol=PJ.TOL if precision == 64 else 1e-4)
        assert out[0][:, still].tobytes() == case["seeds"][:, still].tobytes(), "those dofs come back bit for bit"
        assert (out[3] == project.DONE).all() and (out[2] > 0).all(), (out[2], out[3])
        h = case["ora"].evaluate(out[0], np.arange(n_t))[0]
        assert np.abs(h).max() <= (PJ.TOL if precision == 64 else 1e-4) + bound
        assert ((out[0] >= lower) & (out[0] <= upper)).all()
        if precision == 64:
            want = case["ora"].project(case["seeds"], lower=lower, upper=upper, tol=PJ.TOL)
            print("tree: steps", out[2].tolist(), "restatement's", want[2].tolist(), "rows differ by %.2e" % np.abs(out[0] - want[0]).max())
            assert np.array_equal(out[3], want[3]) and np.array_equal(out[2], want[2])
            assert np.abs(out[0] - want[0]).max() <= BOUND_ROWS_TREE
            # placement: a list on either side of a wavefront, permuted TSRs
            alone = [mod.batch_project_tsr(bid, [case["tsrs"][i]], case["seeds"][i:i + 1], link="L6") for i in range(n_t)]
            of65 = np.arange(65) % n_t
            res = mod.batch_project_tsr(bid, case["tsrs"], case["seeds"][of65], tsr_of=of65, link="L6")
            for q in range(65):
                same(at(res, q), at(alone[of65[q]], 0), "tree: a list of 65, position %d" % q)
        mod.batch_destroy(bid)
    # a robot without a manipulator has no default end effector
    bid = mod.batch_create(model.name, common.config5_goals(1), **dict(common.CONFIG5_KW, n_points=4))
    with pytest.raises(RuntimeError, match="manipulator"):
        mod.batch_config_tsr(bid, case["tsrs"], case["seeds"][:1])
    assert np.isfinite(mod.batch_config_tsr(bid, case["tsrs"], case["seeds"][:1], link="L6")["h"]).all()
    case["ora"].destroy()
    mod.close()


# ---- 6. clearance=True -------------------------------------------------------------------------------------------------------

def test_clearance_of_the_results(wam, p1):
    case = p1["case"]
    mod, bid = wam["mod"], wam["b64"]
    of = np.arange(PJ.N_TARGETS)
    runs = np.arange(PJ.N_TARGETS, dtype=np.int32) % 2
    res = mod.batch_project_tsr(bid, case["tsrs"], case["seeds"], tsr_of=of, clearance=True, runs=runs)
    assert len(res) == 5
    same(res[:4], mod.batch_project_tsr(bid, case["tsrs"], case["seeds"], tsr_of=of), "the projection beside its clearance")
    want = mod.batch_config_clearance(bid, res[0], runs=runs)
    assert set(res[4]) == set(want) == {"clearance", "sphere", "other"}
    same([res[4][key] for key in sorted(want)], [want[key] for key in sorted(want)], "clearance=True")
    assert np.isfinite(res[4]["clearance"][:, 0]).any()


# ---- 7. rejections -----------------------------------------------------------------------------------------------------------

def test_rejections(wam, p1):
    case = p1["case"]
    mod, bid = wam["mod"], wam["b64"]
    lib, h = mod._lib, mod._h
    rec, _ = mod._tsr_records(bid, case["tsrs"][:2], None, None)
    cf = np.ascontiguousarray(case["seeds"][:3]); of = np.array([0, 1, 0], dtype=np.int32)
    n = cf.shape[1]
    hh = np.zeros((3, 6)); jj = np.zeros((3, 6, n))
    ro = np.zeros((3, n)); rs = np.zeros(3); st = np.zeros(3, dtype=np.int32); ss = np.zeros(3, dtype=np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(_capi.c_double_p)
    ip = lambda a: None if a is None else a.ctypes.data_as(_capi.c_int_p)

    def config(bid=bid, n_tsr=2, rec=rec, n_q=3, of=of, cf=cf, hh=hh, jj=jj):
        return lib.orc_batch_config_tsr(h, bid, n_tsr, rec, n_q, ip(of), dp(cf), dp(hh), dp(jj))

    def proj(bid=bid, n_tsr=2, rec=rec, n_q=3, of=of, cf=cf, lo=None, hi=None, max_steps=30, tol=1e-6, mu=1e-8, cap=0.5, ro=ro, rs=rs, st=st, ss=ss):
        return lib.orc_batch_project_tsr(h, bid, n_tsr, rec, n_q, ip(of), dp(cf), dp(lo), dp(hi), max_steps, tol, mu, cap, dp(ro), dp(rs), ip(st), ip(ss))

    def good():
        assert config() == 0 and proj() == 0 and np.abs(hh).max() > 0 and (ss == project.DONE).all()

    def other_link(link):
        r, _ = mod._tsr_records(bid, case["tsrs"][:2], None, None)
        r[1].ee_link = link
        return r

    loose = mod._tsr_records(bid, [case["tsrs"][0], robots.Tsr(Bw=[[-1, 1]] * 3 + [[-3, 3]] * 3)], None, None)[0]
    bad_of = np.array([0, 2, 0], dtype=np.int32); neg_of = np.array([0, -1, 0], dtype=np.int32)
    good()
    both = [dict(bid=bid + 999), dict(n_q=0), dict(n_q=-4), dict(n_tsr=0), dict(of=bad_of), dict(of=neg_of), dict(rec=None), dict(cf=None),
            dict(rec=other_link(len(wam["model"].link_names))), dict(rec=other_link(-2)), dict(rec=loose)]
    for kw in both + [dict(hh=None)]:
        assert config(**kw) != 0, kw
        assert lib.orc_last_error(h), kw
        good()
    nan = float("nan")
    lo = case["lower"].copy(); hi = case["upper"].copy()
    crossed = lo.copy(); crossed[4] = hi[4] + 0.1
    only = both + [dict(ro=None), dict(rs=None), dict(st=None), dict(ss=None), dict(tol=nan), dict(tol=0.0), dict(tol=-1e-6), dict(cap=nan),
                   dict(cap=0.0), dict(cap=-0.5), dict(mu=nan), dict(mu=-1e-8), dict(max_steps=-1), dict(max_steps=257), dict(lo=crossed, hi=hi)]
    for kw in only:
        assert proj(**kw) != 0, kw
        assert lib.orc_last_error(h), kw
        good()
    assert proj(max_steps=256, mu=0.0, lo=lo, hi=hi) == 0 and proj(max_steps=0) == 0 and config(jj=None) == 0 and config(of=None) == 0
