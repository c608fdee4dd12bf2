"""The inputs of tests/test_gpu_first_iteration_tsr.py, checked on the oracle alone (no GPU): one constrained iteration near rounding
only says something if the constraint is violated and acts, no joint-limit round is made, the system is well conditioned and the
oracle itself sits at rounding distance from the reference step.  And the two solvers behind that reference, and the function that
says which form of the step a batch runs (csrc/tsr_form.h) against a second statement of the rule, over its whole domain.
NOTES/first-iteration.md has the figures."""
import ctypes
import fractions

import numpy as np
import pytest

import common
import first_iteration as fi
import first_iteration_tsr as ft


@pytest.mark.parametrize("case", ft.CASES, ids=lambda c: c.id)
def test_inputs_of_the_constrained_step(oracle, case):
    ref = ft.reference(case, oracle)
    print("%s: m %d, draws %s, max |h| %.2e, constraint share %.2f .. %.2f, cond(J A^-1 J^T) %.1e, e_ref %.1e (%s), set aside %d of %d" % (
        case.id, ref["m"], ref["draws"], min(ref["h_max"]), min(ref["share"]), max(ref["share"]), max(ref["cond"]), max(ref["e_ref"]),
        "rational" if case.exact else "long double", ref["aside"].sum(), ref["aside"].size))
    # the joint-limit rounds stay out of it
    assert max(ref["rounds"]) == 0, ref["rounds"]
    # the bent rows violate the constraint
    assert min(ref["h_max"]) > 1e-2, ref["h_max"]
    # ... and the constraint's part of the step is no small correction of it
    assert min(ref["share"]) >= 0.3, ref["share"]
    assert max(ref["cond"]) < 1e7, ref["cond"]
    # the oracle's own step against the reference step of its own h, J, AG and A
    assert max(ref["e_ref"]) < 1e-12, ref["e_ref"]
    if case.precision == 32:
        # a comparison of costs in float: no piece of the obstacle cost is empty (first_iteration's cases ask for 20 sphere-waypoints in
        # each; the WAM's goals near its start leave 2 to 8 inside an obstacle, the chain has 56 and more in each)
        print("  d<0 %d, 0<=d<eps %d, d>=eps %d, outside %d" % tuple(ref["counts"][key] for key in ("inside", "near", "far", "outside")))
        assert min(ref["counts"].values()) >= 1, ref["counts"]
        assert ref["aside"].mean() <= 0.10, (ref["aside"].sum(), ref["aside"].size)
        for key in ("s_AG", "s_dT", "s_cost"):
            print("  %s %.1e .. %.1e" % (key, min(ref[key]), max(ref[key])))
            assert 0.0 < min(ref[key]) and max(ref[key]) < 1e-3, (key, ref[key])


def _random_system(seed, m=5, n=3, k=2):
    rng = np.random.default_rng(seed)
    A = np.diag(np.full(m, 2.0)) - np.diag(np.ones(m - 1), 1) - np.diag(np.ones(m - 1), -1)
    A *= rng.integers(3, 9) / 4.0
    blocks = [(i, rng.normal(size=k), rng.normal(size=(k, n))) for i in range(m)]
    blocks.append((0, rng.normal(size=1), rng.normal(size=(1, n))))      # a second constraint on the first point
    return A, blocks, rng.normal(size=(m, n)), 100.0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_exact_step_leaves_no_residual(seed):
    """A delta - J^T x = 0 and J delta = h' hold exactly in rational arithmetic, and the step is -AG/lambda - delta"""
    F = fractions.Fraction
    A, blocks, AG, lam = _random_system(seed)
    m, n = AG.shape
    step, delta, x, hp = ft.exact_step(A, 1, blocks, AG, lam)
    at = 0
    JTx = [[F(0)] * n for _ in range(m)]
    for i, h, J in blocks:
        for a in range(len(h)):
            assert sum(F(float(J[a, q])) * delta[i][q] for q in range(n)) == hp[at]
            assert hp[at] == F(float(h[a])) - sum(F(float(J[a, q])) * F(float(AG[i, q])) for q in range(n)) / F(lam)
            for q in range(n):
                JTx[i][q] += F(float(J[a, q])) * x[at]
            at += 1
    for r in range(m):
        for q in range(n):
            assert sum(F(float(A[r, j])) * delta[j][q] for j in range(m)) == JTx[r][q]
            assert step[r, q] == float(-F(float(AG[r, q])) / F(lam) - delta[r][q])


@pytest.mark.parametrize("case", [ft.BY_ID[i] for i in ("wam-k3-m5", "wam-k1-m10", "wam-start-k3-con-k3-p10", "chain13-k3-m10")], ids=lambda c: c.id)
def test_exact_step_against_numpy(oracle, case):
    """the rational step of the oracle's own inputs against the dense KKT system by numpy.linalg.solve: within 8 cond eps; and the
    long-double step, the reference of the cases too long for fractions, within 8 cond 2^-63 of the rational one"""
    ref = ft.reference(case, oracle)
    if np.finfo(np.longdouble).nmant < 63:
        pytest.fail("numpy.longdouble has %d bits of mantissa here: the long-double reference needs 63" % np.finfo(np.longdouble).nmant)
    A, lam = ref["A"], ref["lambda"]
    m = A.shape[0]
    for k in range(2):
        blocks, AG = ref["blocks"][k], ref["AG"][k]
        n = AG.shape[1]
        K = sum(len(h) for _, h, _ in blocks)
        kkt = np.zeros((m * n + K, m * n + K)); rhs = np.zeros(m * n + K)
        kkt[:m * n, :m * n] = np.kron(A, np.eye(n))
        at = m * n
        for i, h, J in blocks:
            for a in range(len(h)):
                kkt[at, i * n:(i + 1) * n] = J[a]; kkt[i * n:(i + 1) * n, at] = -J[a]
                rhs[at] = h[a] - J[a] @ AG[i] / lam
                at += 1
        cond = np.linalg.cond(kkt)
        want = -AG / lam - np.linalg.solve(kkt, rhs)[:m * n].reshape(m, n)
        exact = ft.exact_step(A, 1, blocks, AG, lam)[0]
        ld = ft.float_step(ref["Ainv_ld"], blocks, AG, lam, np.longdouble)[0].astype(np.float64)
        err, err_ld = common.rel_l2(want, exact), common.rel_l2(ld, exact)
        print("%s run %d: numpy's KKT solve vs exact %.1e (cond %.1e), long double vs exact %.1e" % (case.id, k, err, cond, err_ld))
        assert err <= 8.0 * cond * 2.0 ** -52
        assert err_ld <= max(8.0 * cond * 2.0 ** -63, 2.0 ** -52)      # (the comparison itself is made in double)


def test_form_function_over_its_domain():
    """orc_host_tsr_form -- the kernel's own ladders (csrc/tsr_form.h) -- against the rule written down a second time
    (first_iteration_tsr.form_expected), for every workgroup size, 1..40 moving waypoints, 1..31 columns and 1..18 constrained rows;
    the forms that are reached; and the rung nothing reaches"""
    from or_cdchomp_amd import _capi
    lib = _capi.lib()
    out = (ctypes.c_int * 6)()
    seen = {}
    for BLOCK in (64, 128, 192, 256, 512):
        for m in list(range(1, 12)) + [32, 40]:
            for n in range(1, 32):
                for k in range(1, 19):
                    assert lib.orc_host_tsr_form(BLOCK, m, n, n + k, out) == 0
                    got = tuple(out)
                    assert got == ft.form_expected(BLOCK, m, n, n + k), (BLOCK, m, n, k, got)
                    seen.setdefault(got, (BLOCK, m, n, k))
    for form, at in sorted(seen.items()):
        print("width %2d regs %2d aug %d meet %d subst <%d, %d>: first at BLOCK %d m %d n %d k %d" % (form + at))
    # 16 lanes and 2 registers WITHOUT the augmented block is not reached: N <= 8 with k >= 1 gives n <= 7 and N + n + 1 <= 16
    assert not [f for f in seen if f[:3] == (16, 2, 0)]
    # every other elimination and every meet is reached (the two are chosen independently: the meet and the substitution by n alone),
    # and the cases of first_iteration_tsr name each of them
    elims = set(f[:3] for f in seen)
    assert elims == {(0, 0, 0), (16, 2, 1), (16, 3, 0), (16, 4, 0), (32, 8, 0), (32, 10, 0), (32, 12, 0)}, sorted(elims)
    assert set(f[3:] for f in seen if f[0]) == {(2, 8, 1), (4, 16, 4), (0, 0, 1)}
    named = set((c.form.get("width"), c.form.get("regs", 0), c.form.get("aug", 0)) for c in ft.CASES)
    assert elims <= named, sorted(elims - named)
    assert set(f[3:] for f in seen if f[0]) == set((c.form["meet"],) + c.form["subst"] for c in ft.CASES if c.form.get("width", 0) > 0)
    assert lib.orc_host_tsr_form(128, 10, 7, 7, out) != 0      # (no constrained row: not a constraint step)


@pytest.mark.parametrize("case", ft.CASES, ids=lambda c: c.id)
def test_the_case_table_names_the_form_of_the_rule(case):
    """the form a case asserts on the device is the one the rule gives for its n, m and rows at 128 and 256 threads (the planner's
    two shapes for such runs): a case cannot pass by asserting the wrong form on both sides"""
    if case.form.get("width", 0) <= 0:
        return
    n = {"wam": 7, "floating": 14, "tree30": 30}.get(case.robot) or int(case.robot[5:])
    per_point = {}
    m = case.n_points - 2 + (1 if ft.free_start(case) else 0)
    for con in case.cons:
        for i in ([0] if con.kind == "start" else range(m)):
            per_point[i] = per_point.get(i, 0) + ft.n_rows(con)
    Nm = n + max(per_point.values())
    assert case.form.get("n_max", Nm) == Nm
    for BLOCK in (128, 256):
        w, regs, aug, meet, sw, su = ft.form_expected(BLOCK, m, n, Nm)
        assert (case.form["width"], case.form["regs"], case.form.get("aug", 0), case.form["meet"], case.form["subst"]) == (w, regs, aug, meet, (sw, su))
