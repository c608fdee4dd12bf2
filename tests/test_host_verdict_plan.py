"""CPU: the sample plan of the collision verdict.  or_cdchomp_amd.module.verdict_samples (what the -m gpu tests in
test_gpu_verdict_device.py hold the device-planned verdict to) against orc_host_verdict_samples, the functions the
host-planned orc_batch_collision_verdict runs, bit for bit; and the two symbols."""
import ctypes as C
import os

import numpy as np
import pytest

from or_cdchomp_amd import _capi
from or_cdchomp_amd.module import verdict_samples

NAN = float("nan")
INF = float("inf")
CAP = 1 << 16


def host_samples(traj, vmax, col0=0, cap=CAP):
    """(return code, seg, u, time, n_samples) of orc_host_verdict_samples"""
    T = np.ascontiguousarray(traj, dtype=np.float64)
    vm = np.ascontiguousarray(vmax, dtype=np.float64)
    seg = np.zeros(max(cap, 1), dtype=np.int32); u = np.full(max(cap, 1), -7.0); tim = np.full(max(cap, 1), -7.0)
    cnt = C.c_int(-1)
    rc = _capi.lib().orc_host_verdict_samples(T.ctypes.data_as(_capi.c_double_p), T.shape[0], T.shape[1], col0,
                                              vm.ctypes.data_as(_capi.c_double_p), cap, seg.ctypes.data_as(_capi.c_int_p),
                                              u.ctypes.data_as(_capi.c_double_p), tim.ctypes.data_as(_capi.c_double_p), C.byref(cnt))
    k = max(cnt.value, 0) if rc == 0 else 0
    return rc, seg[:k], u[:k], tim[:k], cnt.value


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def agree(traj, vmax, col0=0):
    """both planners on one trajectory; returns the sample count"""
    rc, hseg, hu, htime, hcnt = host_samples(traj, vmax, col0)
    assert rc == 0
    seg, u, time = verdict_samples(traj, vmax, col0)
    assert seg.dtype == np.int32 and u.dtype == np.float64 and time.dtype == np.float64
    assert len(seg) == hcnt == len(hseg), (len(seg), hcnt)
    assert np.array_equal(seg, hseg)
    assert same_bits(u, hu)
    assert same_bits(time, htime)
    return hcnt


def random_traj(rng, n_points, n, scale=0.05):
    """a random walk: segments of about scale sqrt(n) rad"""
    return np.cumsum(rng.normal(scale=scale, size=(n_points, n)), axis=0)


@pytest.mark.parametrize("n,col0", [(1, 0), (7, 0), (14, 7)])
@pytest.mark.parametrize("n_points", [3, 4, 100, 300])
def test_specification_equals_the_host_planner(n_points, n, col0):
    rng = np.random.default_rng(1000 * n_points + n)
    total = spread = 0
    for trial in range(6):
        T = random_traj(rng, n_points, n, scale=[0.05, 0.3, 0.004][trial % 3])
        vmax = rng.uniform(0.2, 3.0, size=n - col0)
        if trial >= 3:                                      # zero and negative limits count as 1
            vmax[rng.integers(0, n - col0)] = 0.0
            vmax[rng.integers(0, n - col0)] = -2.0
        cnt = agree(T, vmax, col0)
        total += cnt
        seg, u, time = verdict_samples(T, vmax, col0)
        if cnt:
            assert seg[0] == 0 and u[0] == 0.0 and time[0] == 0.0
            assert (np.diff(seg) >= 0).all() and seg.max() <= n_points - 2
            assert (u >= 0.0).all() and (u <= 1.0 + 1e-9).all()
            spread = max(spread, len(np.unique(seg)))
    assert total > 6, "the workload must have samples"
    assert spread >= min(n_points - 1, 50), "the samples of the longest trajectories must spread over the segments"


@pytest.mark.parametrize("n,col0", [(1, 0), (7, 0), (14, 7)])
def test_repeated_waypoints(n, col0):
    """segments of zero time (dtm == 0): in front, in the middle, at the end, several in a row"""
    rng = np.random.default_rng(7 + n)
    for n_points in (4, 100):
        T = random_traj(rng, n_points, n, scale=0.2)
        T[1] = T[0]
        T[-1] = T[-2]
        if n_points > 10:
            T[40:44] = T[39]
            T[70, col0:] = T[69, col0:]                     # (only the retimed columns repeat)
        vmax = rng.uniform(0.5, 2.0, size=n - col0)
        assert agree(T, vmax, col0) > 2


@pytest.mark.parametrize("n,col0,n_points", [(1, 0, 3), (7, 0, 100), (14, 7, 4)])
def test_degenerate_trajectories(n, col0, n_points):
    rng = np.random.default_rng(11)
    vmax = rng.uniform(0.5, 2.0, size=n - col0)
    # all points equal: total_dist == 0 and duration == 0, no sample
    T = np.tile(rng.normal(size=n), (n_points, 1))
    assert agree(T, vmax, col0) == 0
    if col0:
        # ... the base columns are not retimed: moving them alone changes nothing
        T2 = T.copy(); T2[:, :col0] += rng.normal(size=(n_points, col0))
        assert agree(T2, vmax, col0) == 0
    # a NaN entry: the lengths of its segments are NaN (total_dist > 0 is false, one step covers everything) while the
    # retiming ignores the NaN candidate; one sample when another column moves, none when nothing else does
    T = random_traj(rng, n_points, n, scale=0.2)
    T[n_points // 2, n - 1] = NAN
    cnt = agree(T, vmax, col0)
    assert cnt == (1 if n - col0 > 1 or n_points > 3 else 0), cnt
    T = np.tile(rng.normal(size=n), (n_points, 1))
    T[n_points // 2, n - 1] = NAN
    assert agree(T, vmax, col0) == 0
    # an inf entry: an infinite duration and an infinite length; the step is NaN and the clock stops after one sample
    T = random_traj(rng, n_points, n, scale=0.2)
    T[n_points // 2, col0] = INF
    assert agree(T, vmax, col0) == 1
    T[n_points // 2, col0] = -INF
    assert agree(T, vmax, col0) == 1
    # inf in two neighbouring points of one column: inf - inf, a NaN candidate between them
    T[n_points // 2 - 1, col0] = -INF
    assert agree(T, vmax, col0) == 1


def test_a_known_plan():
    """one dof at 1 rad/s over 0 -> 0.1 -> 0.1 -> 0.3: 0.3 rad, a sample every 0.04 s"""
    T = np.array([[0.0], [0.1], [0.1], [0.3]])
    seg, u, time = verdict_samples(T, [1.0])
    assert agree(T, [1.0]) == len(seg) == 8
    assert np.allclose(time, 0.04 * np.arange(8), rtol=1e-12)
    assert seg.tolist() == [0, 0, 0, 2, 2, 2, 2, 2]         # the segment of zero time holds no sample
    assert np.allclose(u[3:], (time[3:] - 0.1) / 0.2, rtol=1e-12)
    # half the velocity limit: twice the times, the same places
    seg2, u2, time2 = verdict_samples(T, [0.5])
    assert np.array_equal(seg2, seg) and np.allclose(time2, 2 * time, rtol=1e-12) and np.allclose(u2, u, rtol=1e-9)


def test_a_small_cap_is_rejected():
    rng = np.random.default_rng(3)
    T = random_traj(rng, 100, 7)
    vmax = np.ones(7)
    rc, seg, u, tim, cnt = host_samples(T, vmax)
    assert rc == 0 and cnt > 10
    rc2, _, _, _, cnt2 = host_samples(T, vmax, cap=cnt - 1)
    assert rc2 != 0 and cnt2 == cnt, "a short buffer is refused and the count is still reported"
    assert host_samples(T, vmax, cap=cnt)[0] == 0
    # the arrays are optional
    c = C.c_int(0)
    assert _capi.lib().orc_host_verdict_samples(T.ctypes.data_as(_capi.c_double_p), 100, 7, 0, vmax.ctypes.data_as(_capi.c_double_p),
                                                cnt, None, None, None, C.byref(c)) == 0 and c.value == cnt
    # bad dimensions
    assert _capi.lib().orc_host_verdict_samples(T.ctypes.data_as(_capi.c_double_p), 1, 7, 0, vmax.ctypes.data_as(_capi.c_double_p),
                                                cnt, None, None, None, None) != 0
    assert _capi.lib().orc_host_verdict_samples(None, 100, 7, 0, vmax.ctypes.data_as(_capi.c_double_p), cnt, None, None, None, None) != 0
    with pytest.raises(ValueError):
        verdict_samples(T, np.ones(6))
    with pytest.raises(ValueError):
        verdict_samples(T[:1], np.ones(7))


PROTOTYPES = [
    "int orc_batch_collision_verdict_device(orc_module * mod, int batch_id, int * collides_out, double * time_out,",
    "int orc_host_verdict_samples(const double * traj, int n_points, int n, int col0, const double * vmax, int cap,",
]


def test_symbols_are_in_the_c_abi():
    names = [s[0] for s in _capi.SYMBOLS]
    raw = C.CDLL(_capi.LIB_PATH)
    for name in ("orc_batch_collision_verdict_device", "orc_host_verdict_samples"):
        assert name in names
        assert getattr(raw, name) is not None                  # (AttributeError: the built library lacks the symbol)
    root = os.path.dirname(os.path.dirname(os.path.abspath(_capi.__file__)))
    with open(os.path.join(root, "include", "orcdchomp_amd.h")) as f:
        header = f.read()
    for proto in PROTOTYPES:
        assert proto in header
    # without a module the call reports what its sibling reports
    lib = _capi.lib()
    col = np.zeros(1, dtype=np.int32)
    cp = col.ctypes.data_as(_capi.c_int_p)
    want = lib.orc_batch_collision_verdict(None, 1, cp, None, None, None, None)
    assert want != 0
    assert lib.orc_batch_collision_verdict_device(None, 1, cp, None, None, None, None, None) == want
