"""-m "not gpu": the premises of tests/test_gpu_path_clearance.py, without a GPU.  The two calls' place in the C ABI; for every
segment those tests build, verdict_samples([a, b]) equals verdict_samples([a, b, b]) in all three arrays, so the three-point
batch is a yardstick for a segment; and the paths have the sample counts the tests intend."""
import os
import re

import numpy as np

import common
import config_clearance as CC
import path_clearance as PC
from or_cdchomp_amd import _capi
from or_cdchomp_amd.module import clearance_too_long, verdict_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_VMAX = np.linspace(0.5, 2.0, 30)


def n_samples(path, vmax, col0, cap):
    """what orc_batch_clearance must report as n_samples for a run that holds the path"""
    if clearance_too_long(path, vmax, col0, cap):
        return -2
    return len(verdict_samples(path, vmax, col0)[0])


def assert_segment_premise(seg, vmax, col0, what):
    two, three = verdict_samples(seg, vmax, col0), verdict_samples(PC.abb(seg[None])[0], vmax, col0)
    for a, b in zip(two, three):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what
    for cap in (PC.CAP, 65536):
        assert clearance_too_long(seg, vmax, col0, cap) == clearance_too_long(PC.abb(seg[None])[0], vmax, col0, cap), what
    return len(two[0])


def test_symbols_and_null_module():
    header = open(os.path.join(ROOT, "include", "orcdchomp_amd.h")).read()
    tail = ["int max_samples", "double * clearance_out", "double * time_out", "int * sphere_out", "int * other_out", "int * n_samples_out"]
    for name, args in (("orc_batch_path_clearance", ["orc_module * mod", "int batch_id", "int n_q", "const int * run_of_q", "int n_rows",
                                                     "const double * paths"] + tail),
                       ("orc_batch_waypoint_segment_clearance", ["orc_module * mod", "int batch_id", "int n_q", "const int * run_of_q",
                                                                 "const int * from_of_q", "const int * to_of_q"] + tail)):
        m = re.search(r"int %s\((.*?)\);" % name, header, re.S)
        assert m, name
        assert [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")] == args
        assert name in [s[0] for s in _capi.SYMBOLS] and hasattr(_capi.lib(), name)
    lib = _capi.lib()
    dp, ip = _capi.c_double_p, _capi.c_int_p
    clr = np.full((3, 2), 7.0); cnt = np.full(3, 7, dtype=np.int32); paths = np.zeros((3, 2, 7)); idx = np.zeros(3, dtype=np.int32)
    want = lib.orc_batch_clearance(None, 1, 2, None, 64, clr.ctypes.data_as(dp), None, None, None, cnt.ctypes.data_as(ip))
    assert lib.orc_batch_path_clearance(None, 1, 3, None, 2, paths.ctypes.data_as(dp), 64, clr.ctypes.data_as(dp), None, None, None,
                                        cnt.ctypes.data_as(ip)) == want
    assert lib.orc_batch_waypoint_segment_clearance(None, 1, 3, idx.ctypes.data_as(ip), idx.ctypes.data_as(ip), idx.ctypes.data_as(ip), 64,
                                                    clr.ctypes.data_as(dp), None, None, None, cnt.ctypes.data_as(ip)) == want
    assert (clr == 7.0).all() and (cnt == 7).all(), "a NULL module writes nothing"


def test_the_wam_paths_have_the_intended_samples():
    paths, counts = PC.wam_paths()
    assert len(paths) == 10 and all(p.shape == (5, 7) for p in paths.values())
    for name, path in paths.items():
        got = (n_samples(path, PC.WAM_VMAX, 0, 65536), n_samples(path, PC.WAM_VMAX, 0, PC.CAP))
        print("%-28s samples %4d, under the cap %3d" % (name, got[0], got[1]))
        for want, have in zip(counts[name], got):
            assert want is None or want == have, (name, counts[name], got)
        assert got[0] <= 200, name
    ns = {name: n_samples(p, PC.WAM_VMAX, 0, 65536) for name, p in paths.items()}
    assert ns["dips: from above"] > 64, "one path spans two chunks"
    assert all(ns[name] > 1 for name in ("clear: about the start", "clear: away from the table", "dips: along the top", "self contact"))
    assert all(n_samples(paths[name], PC.WAM_VMAX, 0, PC.CAP) > 1 for name in ("clear: about the start", "dips: along the top", "self contact")), \
        "the cap leaves short paths walked"


def test_the_chunk_segments():
    segs, counts = PC.chunk_segments()
    assert segs.shape == (26, 2, 7) and sorted(counts.tolist()) == sorted([3] * 20 + list(PC.SPECIAL))
    for vmax in (np.ones(7), PC.WAM_VMAX):
        for q, seg in enumerate(segs):
            assert assert_segment_premise(seg, vmax, 0, q) == counts[q], (q, counts[q])
    # in the order as built: chunks of 64 with several whole queries, with a tail and a head, and one query over three chunks
    first = np.concatenate([[0], np.cumsum(counts)])
    chunk_of = lambda e: e // 64
    whole = [q for q in range(26) if chunk_of(first[q]) == chunk_of(first[q + 1] - 1)]
    split = [q for q in range(26) if chunk_of(first[q]) != chunk_of(first[q + 1] - 1)]
    assert len(whole) >= 15 and len(split) >= 3
    big = int(np.flatnonzero(counts == 130)[0])
    assert chunk_of(first[big + 1] - 1) - chunk_of(first[big]) >= 2
    orders = PC.chunk_orders(counts)
    assert len(orders) == 3 and orders[1][0] == big and orders[2][-1] == big
    for order in orders:
        assert sorted(order.tolist()) == list(range(26))
    # the rounds' test: a workspace of 132 entries holds the longest query, and the list needs several rounds
    assert counts.max() <= 132 < counts.sum() // 2


def test_the_variants_segments_and_paths():
    _, base, _, _ = common.wam_state()
    base = np.asarray(base, dtype=np.float64); base[0] -= 0.2
    sets = [("pool", CC.wam_pool(), PC.WAM_VMAX, 0), ("tree", CC.tree_pool(), TREE_VMAX, 0), ("floating", CC.floating_configs(base), PC.WAM_VMAX, 7),
            ("held", CC.held_configs(), PC.WAM_VMAX, 0), ("folding", CC.folding_configs(), PC.WAM_VMAX, 0)]
    for name, configs, vmax, col0 in sets:
        paths = PC.local_paths(configs, col0, seed=len(name))
        assert 4 <= len(paths) <= 8
        for q, path in enumerate(paths):
            assert np.array_equal(path[0], configs[q])
            ns = n_samples(path, vmax, col0, 65536)
            assert 2 <= ns <= 64, (name, q, ns)
            # a precision-32 batch holds the narrowed rows, and its plan is made on them widened
            narrowed = path.astype(np.float32).astype(np.float64)
            assert not np.array_equal(narrowed, path) and 2 <= n_samples(narrowed, vmax, col0, 65536) <= 64
            # as segments (first and last row) the premise holds too
            assert_segment_premise(path[[0, -1]], vmax, col0, (name, q))
            assert_segment_premise(narrowed[[0, -1]], vmax, col0, (name, q, "fp32"))
        if col0:
            assert (np.abs(np.linalg.norm(paths[:, :, 3:7], axis=2) - 1.0) > 0.05).sum() >= 4, "the quaternions must not be of unit length"


def test_waypoint_pairs():
    runs, frm, to = PC.waypoint_pairs(4, 12)
    assert len(runs) == len(frm) == len(to) == 10
    assert (frm > to).any() and (frm == to).any() and (np.abs(frm - to) == 1).any()
    assert any(f == 0 and t == 11 for f, t in zip(frm, to))
    assert ((frm >= 0) & (frm < 12) & (to >= 0) & (to < 12) & (runs >= 0) & (runs < 4)).all()
