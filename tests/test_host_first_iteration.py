"""The inputs of tests/test_gpu_first_iteration.py, checked on the oracle alone (no GPU): a one-iteration comparison near rounding
only says something if every piece of the cost is populated, self collision and curvature act, no joint-limit round is made, and the
waypoints next to a switch of the field lookup -- where a rounding-level change of a sphere centre moves a gradient row at order one
-- are few and known.  And the exact rational solve of part C against numpy.linalg.solve.  NOTES/first-iteration.md has the figures."""
import fractions

import numpy as np
import pytest

import common
import first_iteration as fi


@pytest.mark.parametrize("case", fi.ALL_CASES, ids=lambda c: c.id)
def test_inputs_populate_every_branch(oracle, case):
    ref = fi.reference(case, oracle)
    counts = ref["counts"]
    print("%s: d<0 %d, 0<=d<eps %d, d>=eps %d, outside %d; set aside %d of %d at delta %.1e; self collision moves %.0f %% of the rows; "
          "largest second difference %.2e" % (case.id, counts["inside"], counts["near"], counts["far"], counts["outside"],
                                              ref["aside"].sum(), ref["aside"].size, ref["delta"], 100.0 * ref["self_share"], min(ref["max_acc"])))
    # every piece of the obstacle cost
    assert min(counts.values()) >= 20, counts
    # self collision acts: the gradient without it differs in at least 5 % of the rows
    assert ref["self_share"] >= 0.05, ref["self_share"]
    # curvature acts: no run's sphere accelerations are all zero (a straight line's are)
    assert min(ref["max_acc"]) > 0.0
    # the joint-limit rounds stay out of it
    assert max(ref["rounds"]) == 0, ref["rounds"]
    for k in range(case.n_runs):
        assert not np.array_equal(ref["T0"][k][1:-1], np.linspace(ref["T0"][k][0], ref["T0"][k][-1], case.n_points)[1:-1])
    # waypoints next to a lookup switch: at most 10 % in fp32, none in fp64 (change the case's seed, not the cap)
    share = ref["aside"].mean()
    assert share <= (0.10 if case.precision == 32 else 0.0), (ref["aside"].sum(), ref["aside"].size)
    if case.precision == 32:
        # `s` is the movement of the oracle's rows under a relative 2^-24 change of the waypoints.  Rounding moved them by 3e-7 .. 9e-5
        # of the largest row in every case measured; a lookup that switches under the perturbation moves a row by 1e-2 and more, and
        # would widen the device's tolerance: such a draw has to go (change the seed)
        for key in ("s_G", "s_AG", "s_dT", "s_cost"):
            print("  %s %.1e .. %.1e" % (key, min(ref[key]), max(ref[key])))
            assert 0.0 < min(ref[key]) and max(ref[key]) < 1e-3, (key, ref[key])


@pytest.mark.parametrize("D", [2, 3, 4])
def test_semisep_threshold(D):
    """the smallest run whose generators the host accepts (csrc/host_math.cpp build_semisep: m >= 2 D + 2), as part C assumes it"""
    from or_cdchomp_amd import _capi
    lib = _capi.lib()
    m = fi.SEMISEP_MIN_M(D)
    assert lib.orc_host_metric_semisep_rank(m, D, 1.0 / (m + 1), 0) == D
    assert lib.orc_host_metric_semisep_rank(m - 1, D, 1.0 / m, 0) == 0


@pytest.mark.parametrize("case", fi.SOLVE_CASES[:6], ids=lambda c: c.id)
def test_exact_solve_against_numpy(oracle, case):
    """derivative 1 is well conditioned (cond 4e2 .. 3e4): LAPACK's solve is within a few cond(A) eps of the rational one"""
    ref = fi.reference(case, oracle)
    A = ref["A"]
    cond = np.linalg.cond(A)
    for k in range(2):
        x = fi.exact_band_solve(A, ref["G"][k], 1)
        err = common.rel_l2(np.linalg.solve(A, ref["G"][k]), x)
        print("%s run %d: numpy vs exact %.1e, cond %.1e; the oracle's AG vs exact %.1e" % (case.id, k, err, cond, common.rel_l2(ref["AG"][k], x)))
        assert err <= 8.0 * cond * 2.0 ** -52
        assert common.rel_l2(ref["AG"][k], x) <= 8.0 * cond * 2.0 ** -52


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_exact_solve_leaves_no_residual(D):
    """A x - G is exactly zero in rational arithmetic, for a symmetric positive definite band matrix of doubles"""
    rng = np.random.default_rng(D)
    m = 11
    K = np.zeros((m + D, m))
    for q in range(D + 1):
        K[np.arange(m) + q, np.arange(m)] = rng.integers(1, 9, size=m) / 8.0
    A = K.T @ K
    G = rng.normal(size=(m, 3))
    x = fi.exact_band_solve(A, G, D, rounded=False)
    F = fractions.Fraction
    for i in range(m):
        for c in range(3):
            assert sum(F(float(A[i, j])) * x[j][c] for j in range(m)) == F(float(G[i, c]))
    assert common.rel_l2(fi.exact_band_solve(A, G, D), np.linalg.solve(A, G)) < 1e-10
