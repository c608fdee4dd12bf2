"""not gpu: the specification functions of the subset verdict (or_cdchomp_amd.module.candidates, verdict_subset) on hand-made
arrays, and the two calls' place in the C ABI (orc_batch_collision_verdict_subset, orc_batch_set_verdict_scope)."""
import ctypes as C
import os

import numpy as np
import pytest

from or_cdchomp_amd import _capi
from or_cdchomp_amd.module import (VERDICT_SKIPPED, VERDICT_TOO_LONG, candidates, contiguous_groups, respawn_plan, select_best,
                                   verdict_subset)

INF, NAN = float("inf"), float("nan")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_candidates_is_status_and_a_finite_total():
    #                     0     1     2     3     4     5     6     7     8
    status = np.array([0, 1, -1, 0, 1, 0, -1, 0, 2], dtype=np.int32)
    total = np.array([1.0, 2.0, 3.0, NAN, INF, -INF, NAN, -0.0, 1.0])
    want = np.array([True, True, False, False, False, False, False, True, False])
    got = candidates(total, status)
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    # rows as batch_iterate returns them: the TOTAL column decides, whatever the others hold
    rows = np.stack([total, np.full(9, NAN), np.full(9, INF)], axis=1)
    assert np.array_equal(candidates(rows, status), want)
    rows = np.stack([np.full(9, NAN), total, total], axis=1)
    assert not candidates(rows, status).any()
    assert candidates(np.zeros(0), np.zeros(0, dtype=np.int32)).shape == (0,)
    with pytest.raises(ValueError):
        candidates(total, status[:-1])


def test_candidates_is_what_the_selection_rules_use():
    """select_best's eligibility without a verdict and respawn_plan's mode-0 candidates are `candidates`"""
    rng = np.random.default_rng(7)
    n = 48
    status = rng.integers(-1, 2, n).astype(np.int32)
    costs = rng.uniform(-1.0, 5.0, (n, 3))
    costs[rng.integers(0, n, 6), 0] = NAN
    costs[rng.integers(0, n, 6), 0] = INF
    costs[3, 0] = -0.0
    cand = candidates(costs, status)
    assert cand.any() and not cand.all()
    each = np.arange(n, dtype=np.int32)
    best, cost, cnt = select_best(costs, status, None, each, n)
    assert np.array_equal(cnt, cand.astype(np.int32)) and np.array_equal(best >= 0, cand)
    source, n_surv = respawn_plan(costs, status, None, each, n, keep=1, mode=0)
    assert np.array_equal(n_surv, cand.astype(np.int32)) and np.array_equal(source == each, cand)
    # a colliding candidate stays one for the verdict's scope: the scope is decided before the verdict is known
    col = np.ones(n, dtype=np.int32)
    assert select_best(costs, status, col, contiguous_groups(n, 1), 1)[2][0] == 0 and cand.sum() > 0


def full_verdict():
    return dict(collides=np.array([1, 0, 1, 0, 0], dtype=np.int32),
                time=np.array([0.25, -1.0, 0.0, -1.0, -1.0]),
                sphere=np.array([7, -1, 0, -1, -1], dtype=np.int32),
                field=np.array([0, -1, -5, -1, -1], dtype=np.int32),
                depth=np.array([0.0125, 0.0, -0.0, 0.0, 0.0]),      # (-0.0: an examined run keeps its BITS)
                n_samples=np.array([300, 12, 64, 0, 1], dtype=np.int32))


def test_verdict_subset_keeps_examined_runs_and_blanks_the_others():
    full = full_verdict()
    mask = np.array([1, 0, 1, 1, 0])
    got = verdict_subset(full, mask)
    assert sorted(got) == sorted(full)
    for key in full:
        assert got[key].dtype == full[key].dtype, key
        assert got[key] is not full[key]
    assert got["collides"].tolist() == [1, VERDICT_SKIPPED, 1, 0, VERDICT_SKIPPED]
    assert got["n_samples"].tolist() == [300, VERDICT_SKIPPED, 64, 0, VERDICT_SKIPPED]
    assert got["sphere"].tolist() == [7, -1, 0, -1, -1] and got["field"].tolist() == [0, -1, -5, -1, -1]
    assert np.array_equal(bits(got["time"]), bits([0.25, -1.0, 0.0, -1.0, -1.0]))
    assert np.array_equal(bits(got["depth"]), bits([0.0125, 0.0, -0.0, 0.0, 0.0]))
    assert np.signbit(got["depth"][2]) and not np.signbit(got["depth"][1]), "-0.0 survives where examined, a skipped run's depth is +0"
    # the input is not touched
    again = full_verdict()
    for key in full:
        assert np.array_equal(bits(full[key]) if full[key].dtype == np.float64 else full[key],
                              bits(again[key]) if again[key].dtype == np.float64 else again[key])


def test_verdict_subset_masks():
    full = full_verdict()
    everything = verdict_subset(full, np.ones(5, dtype=bool))
    for key in full:
        assert np.array_equal(everything[key], full[key]) and np.array_equal(np.signbit(everything["depth"]), np.signbit(full["depth"]))
    nothing = verdict_subset(full, np.zeros(5, dtype=np.uint8))
    assert (nothing["collides"] == -1).all() and (nothing["n_samples"] == -1).all() and (nothing["time"] == -1.0).all()
    assert (nothing["sphere"] == -1).all() and (nothing["field"] == -1).all()
    assert np.array_equal(bits(nothing["depth"]), np.zeros(5, dtype=np.int64))
    # any nonzero entry means "examine", also a negative one or a float
    assert verdict_subset(full, [2, 0, -1, 0.5, 0])["collides"].tolist() == [1, -1, 1, 0, -1]
    # the host-planned verdict's dict has no n_samples: the keys of the input are the keys of the output
    host = {k: v for k, v in full.items() if k != "n_samples"}
    assert sorted(verdict_subset(host, [1, 0, 0, 0, 0])) == sorted(host)
    with pytest.raises(ValueError):
        verdict_subset(full, [1, 0, 1])
    with pytest.raises(ValueError):
        verdict_subset(dict(full, other=np.zeros(5)), np.ones(5))
    assert VERDICT_SKIPPED == -1 and VERDICT_TOO_LONG == -2


def test_candidates_feed_verdict_subset():
    full = full_verdict()
    status = np.array([0, -1, 1, 0, -1], dtype=np.int32)
    costs = np.array([[1.0, 0, 0], [2.0, 0, 0], [-0.0, 0, 0], [NAN, 0, 0], [INF, 0, 0]])
    got = verdict_subset(full, candidates(costs, status))
    assert got["collides"].tolist() == [1, -1, 1, -1, -1]


PROTOTYPES = [
    "int orc_batch_collision_verdict_subset(orc_module * mod, int batch_id, int which, const unsigned char * examine,",
    "int orc_batch_set_verdict_scope(orc_module * mod, int batch_id, int scope);",
]


def test_symbols_are_exported_and_declared():
    names = [s[0] for s in _capi.SYMBOLS]
    raw = C.CDLL(_capi.LIB_PATH)
    for name in ("orc_batch_collision_verdict_subset", "orc_batch_set_verdict_scope"):
        assert name in names
        assert getattr(raw, name) is not None                  # (AttributeError: the built library lacks the symbol)
    root = os.path.dirname(os.path.dirname(os.path.abspath(_capi.__file__)))
    with open(os.path.join(root, "include", "orcdchomp_amd.h")) as f:
        header = f.read()
    for proto in PROTOTYPES:
        assert proto in header
    # without a module the calls report what their sibling reports, and touch nothing
    lib = _capi.lib()
    col = np.full(1, 5, dtype=np.int32)
    cp = col.ctypes.data_as(_capi.c_int_p)
    want = lib.orc_batch_collision_verdict_device(None, 1, cp, None, None, None, None, None)
    assert want != 0
    ex = np.ones(1, dtype=np.uint8)
    assert lib.orc_batch_collision_verdict_subset(None, 1, 0, ex.ctypes.data_as(_capi.c_ubyte_p), cp, None, None, None, None, None) == want
    assert lib.orc_batch_set_verdict_scope(None, 1, 1) == want
    assert col[0] == 5
