"""CPU: the specifications of the multi-start calls (or_cdchomp_amd.module.select_best and seed_perturbation, what the
-m gpu tests in test_gpu_multistart.py hold orc_batch_select_best and orc_batch_perturb to) and the three symbols."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from or_cdchomp_amd import _capi
from or_cdchomp_amd.module import contiguous_groups, seed_perturbation, select_best

INF = float("inf")
NAN = float("nan")


# ---- select_best -----------------------------------------------------------------------------------------------------

def test_lowest_cost_wins_and_a_tie_goes_to_the_lower_index():
    costs = [5.0, 3.0, 3.0, 4.0, 2.0, 2.0]
    run, cost, cnt = select_best(costs, [0] * 6, [0] * 6, [0, 0, 0, 0, 1, 1], 2)
    assert run.tolist() == [1, 4] and cost.tolist() == [3.0, 2.0] and cnt.tolist() == [4, 2]
    assert run.dtype == np.int32 and cnt.dtype == np.int32
    # the same costs with the groups interleaved: the tie is by run index, not by position in the group's list
    run, cost, cnt = select_best([3.0, 2.0, 3.0, 2.0], [0] * 4, None, [1, 0, 1, 0], 2)
    assert run.tolist() == [1, 0] and cost.tolist() == [2.0, 3.0] and cnt.tolist() == [2, 2]


def test_status_minus_one_is_excluded_and_converged_runs_count():
    run, cost, cnt = select_best([1.0, 2.0, 3.0], [-1, 1, 0], [0, 0, 0], [0, 0, 0], 1)
    assert run.tolist() == [1] and cost.tolist() == [2.0] and cnt.tolist() == [2]
    # rows of (total, obs, smooth) as batch_iterate returns them: the total counts
    run, cost, cnt = select_best([[4.0, 0.0, 4.0], [3.0, 3.0, 0.0]], [0, 0], None, [0, 0], 1)
    assert run.tolist() == [1] and cost.tolist() == [3.0]


def test_nan_and_infinite_costs_are_excluded():
    run, cost, cnt = select_best([NAN, INF, -INF, 7.0], [0, 0, 0, 0], None, [0, 0, 0, 0], 1)
    assert run.tolist() == [3] and cost.tolist() == [7.0] and cnt.tolist() == [1]


def test_a_colliding_run_is_excluded_only_when_asked():
    costs, status, col, grp = [1.0, 2.0, 3.0, 4.0], [0, 0, 0, 0], [1, 0, 1, 0], [0, 0, 1, 1]
    run, cost, cnt = select_best(costs, status, col, grp, 2)
    assert run.tolist() == [1, 3] and cost.tolist() == [2.0, 4.0] and cnt.tolist() == [1, 1]
    run, cost, cnt = select_best(costs, status, None, grp, 2)
    assert run.tolist() == [0, 2] and cost.tolist() == [1.0, 3.0] and cnt.tolist() == [2, 2]


def test_an_empty_group():
    # group 1 has no run at all, group 2 only runs that are not eligible
    run, cost, cnt = select_best([1.0, 2.0, 3.0], [0, -1, 0], [0, 0, 1], [0, 2, 2], 3)
    assert run.tolist() == [0, -1, -1]
    assert cost.tolist() == [1.0, INF, INF]
    assert cnt.tolist() == [1, 0, 0]


def test_arbitrary_and_contiguous_groups_agree():
    rng = np.random.default_rng(3)
    n_runs, n_groups = 48, 6
    costs = rng.integers(0, 6, n_runs).astype(np.float64)          # many ties
    status = rng.choice([-1, 0, 1], n_runs)
    col = rng.integers(0, 2, n_runs)
    grp = contiguous_groups(n_runs, n_groups)
    assert grp.tolist() == [r // 8 for r in range(n_runs)]
    a = select_best(costs, status, col, grp, n_groups)
    # the same partition with the groups renamed: the winners are the same runs under the new names
    name = rng.permutation(n_groups)
    b = select_best(costs, status, col, name[grp], n_groups)
    for x, y in zip(a, b):
        assert np.array_equal(x, y[name])
    # ... and with the runs shuffled: the winner is the lowest ORIGINAL index among the group's best only through the
    # shuffled order, so compare costs and counts, and the winner's cost
    perm = rng.permutation(n_runs)
    c = select_best(costs[perm], status[perm], col[perm], grp[perm], n_groups)
    assert np.array_equal(c[1], a[1]) and np.array_equal(c[2], a[2])
    for g in range(n_groups):
        if c[0][g] >= 0:
            assert grp[perm][c[0][g]] == g and costs[perm][c[0][g]] == a[1][g]
            ties = [r for r in range(n_runs) if grp[perm][r] == g and costs[perm][r] == a[1][g] and status[perm][r] >= 0 and col[perm][r] == 0]
            assert c[0][g] == min(ties)


def test_bad_groups():
    with pytest.raises(ValueError):
        select_best([1.0, 2.0], [0, 0], None, [0, 2], 2)
    with pytest.raises(ValueError):
        select_best([1.0, 2.0], [0, 0], None, [0, -1], 2)
    with pytest.raises(ValueError):
        select_best([1.0, 2.0], [0, 0], None, [0], 1)
    with pytest.raises(ValueError):
        contiguous_groups(10, 3)


# ---- seed_perturbation -----------------------------------------------------------------------------------------------

def host_metric(m, derivative, dt):
    A = np.zeros((m, m))
    assert _capi.lib().orc_host_metric(m, derivative, dt, A.ctypes.data_as(_capi.c_double_p), None, None, None, None, 0, None) == 0
    return A


@pytest.mark.parametrize("derivative", [1, 2, 3])
def test_definition(derivative):
    """delta = sigma c A^-1 xi with the library's own stream and metric, against a dense solve in numpy"""
    m, n, dt, sigma, seed = 30, 3, 1.0 / 31, 0.25, 12345
    base = np.linspace(0.0, 1.0, m * n).reshape(m, n)
    out = seed_perturbation(m, n, derivative, dt, sigma, seed, -INF, INF, base)
    assert out.shape == (m, n)                                 # moving rows only: the fixed ends have no displacement
    xi = np.zeros(m * n)
    _capi.lib().orc_host_gsl_stream(seed, 1.0, m * n, xi.ctypes.data_as(_capi.c_double_p), None)
    Ainv = np.linalg.inv(host_metric(m, derivative, dt))
    want = sigma / np.linalg.norm(Ainv[m // 2]) * (Ainv @ xi.reshape(m, n))
    # (the dense inverse in double is good to cond(A) eps: ~1e-9 of the result for derivative 3 at m = 30)
    assert np.linalg.norm((out - base) - want) <= 1e-7 * np.linalg.norm(want)
    assert np.linalg.norm(want) > 0.1
    # seed 0 is GSL's 4357; another seed is another displacement
    assert np.array_equal(seed_perturbation(m, n, derivative, dt, sigma, 0, -INF, INF, base),
                          seed_perturbation(m, n, derivative, dt, sigma, 4357, -INF, INF, base))
    assert not np.array_equal(seed_perturbation(m, n, derivative, dt, sigma, 1, -INF, INF, base), out)
    # the scale of the metric cancels: dt only enters through A's scale when both ends are fixed
    other = seed_perturbation(m, n, derivative, 2.0 * dt, sigma, seed, -INF, INF, base)
    assert np.linalg.norm(other - out) <= 1e-9 * np.linalg.norm(out - base)


def test_sigma_zero_is_the_identity():
    base = np.random.default_rng(1).normal(size=(12, 4))
    out = seed_perturbation(12, 4, 1, 0.1, 0.0, 7, -0.001, 0.001, base)      # (not even clamped: no bit changes)
    assert np.array_equal(out.view(np.int64), base.view(np.int64))
    for bad in (-1.0, NAN, INF):
        with pytest.raises(ValueError):
            seed_perturbation(12, 4, 1, 0.1, bad, 7, -1, 1, base)


@pytest.mark.parametrize("derivative", [1, 2])
def test_sigma_is_the_standard_deviation_of_the_middle_waypoint(derivative):
    """N = 1000 seeds x 2 columns = 2000 independent samples of delta[mid, j]: the sample standard deviation of a Gaussian
    has the relative standard error 1 / sqrt(2 N) = 1.58 %; the bound is five of them, 7.9 %."""
    m, n, sigma, seeds = 21, 2, 0.3, 1000
    N = seeds * n
    bound = 5.0 / math.sqrt(2.0 * N)
    base = np.zeros((m, n))
    d = np.stack([seed_perturbation(m, n, derivative, 1.0 / (m + 1), sigma, 1000 + s, -INF, INF, base) for s in range(seeds)])
    mid = m // 2
    sd = d[:, mid, :].reshape(-1).std(ddof=1)
    print("derivative %d: std of delta[mid] %.5f for sigma %.5f (relative error %.4f, bound %.4f)" % (derivative, sd, sigma, sd / sigma - 1, bound))
    assert abs(sd / sigma - 1.0) <= bound
    # the displacement is largest in the middle and tapers towards the fixed ends
    rows = d.transpose(1, 0, 2).reshape(m, -1).std(axis=1, ddof=1)
    assert abs(int(np.argmax(rows)) - mid) <= 1, rows
    assert rows[0] < 0.5 * rows[mid] and rows[-1] < 0.5 * rows[mid]
    assert abs(d.mean()) <= 5.0 * sigma / math.sqrt(N)         # zero mean (every entry's deviation is at most sigma)


def test_clamping():
    m, n, sigma = 40, 3, 0.5
    base = np.zeros((m, n))
    lo, hi = np.array([-0.1, -0.2, -0.05]), np.array([0.1, 0.05, 0.3])
    free = seed_perturbation(m, n, 1, 1.0 / (m + 1), sigma, 99, -INF, INF, base)
    out = seed_perturbation(m, n, 1, 1.0 / (m + 1), sigma, 99, lo, hi, base)
    below, above = free < lo, free > hi
    assert below.any() and above.any() and (~below & ~above).any()
    assert (out >= lo).all() and (out <= hi).all()
    assert np.array_equal(out[below], np.broadcast_to(lo, (m, n))[below])
    assert np.array_equal(out[above], np.broadcast_to(hi, (m, n))[above])
    assert np.array_equal(out[~below & ~above], free[~below & ~above])


# ---- the C ABI -------------------------------------------------------------------------------------------------------

PROTOTYPES = [
    "int orc_batch_perturb(orc_module * mod, int batch_id, double sigma, const unsigned int * seeds);",
    "int orc_batch_select_best(orc_module * mod, int batch_id, int n_groups, const int * group_of_run, int require_collision_free,",
    "int orc_batch_gettraj_runs(orc_module * mod, int batch_id, const int * runs, int n_sel, double * traj_out, size_t cap_doubles);",
]


def test_symbols_are_in_the_c_abi():
    names = [s[0] for s in _capi.SYMBOLS]
    raw = C.CDLL(_capi.LIB_PATH)
    for name in ("orc_batch_perturb", "orc_batch_select_best", "orc_batch_gettraj_runs"):
        assert name in names
        assert getattr(raw, name) is not None                  # (AttributeError: the built library lacks the symbol)
    root = os.path.dirname(os.path.dirname(os.path.abspath(_capi.__file__)))
    with open(os.path.join(root, "include", "orcdchomp_amd.h")) as f:
        header = f.read()
    for proto in PROTOTYPES:
        assert proto in header
    # without a module the calls report "no module" like every other entry point
    lib = _capi.lib()
    assert lib.orc_batch_perturb(None, 1, 0.1, None) == 2
    assert lib.orc_batch_select_best(None, 1, 1, None, 0, None, None, None) == 2
    assert lib.orc_batch_gettraj_runs(None, 1, None, 0, None, 0) == 2
