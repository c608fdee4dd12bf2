"""CPU: merged fields (orc_scene_merge_fields).  The specification (merged_grid_dims and merged_field of
or_cdchomp_amd/module.py), the library's host twin (orc_host_merge_grid, orc_host_merge_fields: what the -m gpu tests of
test_gpu_merge_fields.py hold the kernel to, bit for bit) and the three symbols."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import merge_common as mc
from or_cdchomp_amd import _capi
from or_cdchomp_amd.module import grid_interp, merged_field, merged_grid_dims, pose_apply, pose_invert

INF = np.inf
IDENT = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]


def test_symbols_are_in_the_c_abi():
    names = ("orc_host_merge_grid", "orc_host_merge_fields", "orc_scene_merge_fields")
    bound = [s[0] for s in _capi.SYMBOLS]
    raw = C.CDLL(_capi.LIB_PATH)
    root = os.path.dirname(os.path.dirname(os.path.abspath(_capi.__file__)))
    with open(os.path.join(root, "include", "orcdchomp_amd.h")) as f:
        header = f.read()
    for name in names:
        assert name in bound
        assert getattr(raw, name) is not None                    # (AttributeError: the built library lacks the symbol)
        assert re.search(r"^int %s\(" % name, header, re.M), name
    for word in ("resampled at cell centres", "holds +inf", "no limit of eight", "before any device work"):
        assert word in header, word
    # without a module the call reports "no module" like every other entry point
    assert _capi.lib().orc_scene_merge_fields(None, b"merged", 0, None, None, 0.04, None) == 2


# ---- sizing --------------------------------------------------------------------------------------------------------------

def sizing_cases():
    rng = np.random.default_rng(20261)
    cases = []
    for k in range(12):
        n = int(rng.integers(1, 5))
        boxes = []
        for _ in range(n):
            q = mc.random_quat(rng) if k % 4 else np.array([0.0, 0.0, 0.0, 1.0])
            if k % 5 == 1:
                q = q * 1.3                                  # a quaternion that is not of unit length is used as it is
            boxes.append((list(rng.uniform(0.1, 1.2, size=3)), list(rng.uniform(-2.0, 2.0, size=3)) + list(q)))
        cell = float(rng.uniform(0.01, 0.11))
        bounds = None
        if k % 3 == 2:
            lo = rng.uniform(-1.0, 0.0, size=3)
            bounds = list(lo) + list(lo + rng.uniform(0.2, 1.5, size=3))
        cases.append((boxes, cell, bounds))
    # an extent below two cells: every size is the minimum, 2
    cases.append(([([0.5, 0.5, 0.5], IDENT)], 0.1, [0.0, 0.0, 0.0, 0.05, 0.12, 0.19]))
    # a box of whole cells, and one that exceeds them by one part in 2^40
    cases.append(([([0.5, 0.25, 0.125], IDENT)], 2.0 ** -5, None))
    cases.append(([([0.5 + 2.0 ** -40, 0.25, 0.125], IDENT)], 2.0 ** -5, None))
    return cases


def test_host_merge_grid_is_merged_grid_dims():
    seen_min = seen_rot = seen_bounds = 0
    for boxes, cell, bounds in sizing_cases():
        sizes, lengths, pose = merged_grid_dims(boxes, cell, bounds)
        rc, hs, hl, hp = mc.host_merge_grid(boxes, cell, bounds)
        assert rc == 0
        assert hs == sizes and hl == lengths and hp == pose, (boxes, cell, bounds)      # exactly: the same doubles
        assert pose[3:] == [0.0, 0.0, 0.0, 1.0] and all(s >= 2 for s in sizes)
        assert lengths == [s * cell for s in sizes]
        seen_min += sizes == [2, 2, 2]
        seen_rot += any(b[1][3] != 0.0 for b in boxes)
        seen_bounds += bounds is not None
    assert seen_min >= 1 and seen_rot >= 6 and seen_bounds >= 4
    # the hand-made ones
    assert merged_grid_dims([([0.5, 0.25, 0.125], IDENT)], 2.0 ** -5)[0] == [16, 8, 4]
    assert merged_grid_dims([([0.5 + 2.0 ** -40, 0.25, 0.125], IDENT)], 2.0 ** -5)[0] == [17, 8, 4]
    # with bounds the sources are not read
    assert mc.host_merge_grid([], 0.1, [0, 0, 0, 1, 1, 1])[:2] == (0, [10, 10, 10])


def test_what_the_sizing_rejects():
    box = [([0.5, 0.5, 0.5], IDENT)]
    bad = [
        (box, 0.0, None), (box, -0.1, None), (box, math.nan, None), (box, math.inf, None),
        (box, 0.1, [0, 0, 0, 1, 1, math.nan]), (box, 0.1, [0, 0, 0, 1, 1, math.inf]),
        (box, 0.1, [0, 0, 0, 1, 0, 1]), (box, 0.1, [0, 0, 2, 1, 1, 1]),
        ([([0.5, 0.5, 0.5], [0, 0, math.nan, 0, 0, 0, 1])], 0.1, None),
        ([([0.5, 0.5, 0.5], [0, 0, 0, 0, 0, 0, 0])], 0.1, None),           # a quaternion of zero norm: a box without extent
        ([], 0.1, None),
        (box, 1e-4, [0, 0, 0, 1, 1, 1]),                                   # 10^12 cells: 2^31 bytes and more
        (box, 1e-9, [0, 0, 0, 1, 1, 1]),                                   # cell counts that do not fit an int
    ]
    for boxes, cell, bounds in bad:
        assert mc.host_merge_grid(boxes, cell, bounds)[0] != 0, (boxes, cell, bounds)
        with pytest.raises(ValueError):
            merged_grid_dims(boxes, cell, bounds)
    # one cell less than 2^31 bytes is accepted, 2^31 bytes are not: 2^28 doubles
    assert mc.host_merge_grid([], 1.0, [0, 0, 0, 1023, 512, 512])[0] == 0
    assert mc.host_merge_grid([], 1.0, [0, 0, 0, 1024, 512, 512])[0] != 0
    assert merged_grid_dims([], 1.0, [0, 0, 0, 1023, 512, 512])[0] == [1023, 512, 512]


# ---- the host twin against an independent reading ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def case():
    sources, sizes, lengths, pose = mc.three_sources()
    return dict(sources=sources, sizes=sizes, lengths=lengths, pose=pose,
                host=mc.host_merge_fields(sources, sizes, lengths, pose))


def test_precondition_no_centre_on_a_discontinuity(case):
    """The bound of the next test compares two roundings of the same point.  It needs every centre on the same side of every
    discontinuity of the interpolation in both: the boundary faces of a source (the issue's precondition), and the faces
    between a source's cells -- crossing one changes the cell whose differences along the OTHER axes are taken, and whether a
    neighbour is +inf (across the planes through the cell centres the interpolation is continuous).  From the
    specification alone; the seed of merge_common.three_sources is chosen so that both counts are 0."""
    n_boundary, n_face = mc.near_discontinuity(case["sources"], case["sizes"], case["lengths"], case["pose"], eps=1e-9)
    assert n_boundary == 0
    assert n_face == 0


def test_host_twin_against_the_oracles_interpolation(case, oracle):
    """inf exactly where the specification has inf; elsewhere within 1e-12 (1 + s) metres, s the steepest neighbour difference
    over cell size in the sources: a few roundings of coordinates of a few metres move the point by about 1e-15 m, the
    value by s times that, and the bound leaves three orders over it (derived, not measured)."""
    sources, sizes, lengths, pose = case["sources"], case["sizes"], case["lengths"], case["pose"]
    want = mc.merged_field_over_oracle(oracle, sources, sizes, lengths, pose)
    got = case["host"]
    assert got.shape == tuple(sizes) and not np.isnan(got).any()
    n_inf = int(np.isinf(want).sum())
    covered = np.zeros(int(np.prod(sizes)), dtype=bool)
    for _, slen, spose in sources:
        x = mc.source_points(spose, sizes, lengths, pose) / np.asarray(slen)
        inside = ((x >= 0) & (x <= 1)).all(axis=1)
        assert 0 < inside.sum() < inside.size                      # the target lies partly outside every source
        covered |= inside
    # cells no source covers, and covered cells that are +inf through the sources' own +inf cells
    assert (~covered).sum() > 100 and covered.sum() > 500 and n_inf > (~covered).sum()
    assert np.array_equal(np.isinf(got), np.isinf(want))
    assert (got[np.isinf(got)] > 0).all()
    fin = np.isfinite(want)
    s = mc.steepest(sources)
    assert 0.5 < s < 50.0, s                                       # a distance field's slope is about 1; the +inf cells' neighbours aside
    err = float(np.abs(got[fin] - want[fin]).max())
    print("host twin against the oracle's interpolation: max |diff| %.3e m, s %.3f, bound %.3e" % (err, s, 1e-12 * (1 + s)))
    assert err <= 1e-12 * (1 + s), (err, s)
    # ... and the pure-Python specification reads the same cells
    spec = merged_field(sources, sizes, lengths, pose)
    assert np.array_equal(np.isinf(spec), np.isinf(want))
    assert float(np.abs(spec[fin] - want[fin]).max()) <= 1e-12 * (1 + s)


def test_grid_interp_of_the_specification_is_the_oracles(case, oracle):
    data, slen, _ = case["sources"][0]
    grid = oracle.OraGrid(data, slen)
    rng = np.random.default_rng(5)
    pts = rng.uniform(-0.05, 1.05, size=(400, 3)) * np.asarray(slen)
    pts[:8] = [[0, 0, 0], slen, [slen[0], 0, 0], [0, slen[1], slen[2]], 0.5 * np.asarray(slen), [math.nan, 0.1, 0.1],
               [0.1, -1e-300, 0.1], [0.1, 0.1, slen[2] * (1 + 2.0 ** -52)]]
    for p in pts:
        s_out, s_val = grid_interp(data, slen, p)
        if np.isnan(p).any():
            assert s_out                                            # (the reference's own test lets a NaN through: not asked)
            continue
        o_out, o_val = grid.interp(p)
        assert bool(o_out) == s_out, p
        if not s_out:
            assert o_val == s_val, (p, o_val, s_val)


# ---- exact cases ---------------------------------------------------------------------------------------------------------

def test_identity_onto_the_own_lattice_is_the_source():
    rng = np.random.default_rng(7)
    for ssz in mc.SOURCE_SIZES:
        data, slen = mc.random_sdf(rng, ssz, n_inf=0)
        got = mc.host_merge_fields([(data, slen, IDENT)], ssz, slen, IDENT)
        assert got.tobytes() == data.tobytes()
        # a shifted pose shared by both changes nothing either when the shift is a few exact binary digits
        shift = [0.5, -0.25, 2.0, 0.0, 0.0, 0.0, 1.0]
        assert mc.host_merge_fields([(data, slen, shift)], ssz, slen, shift).tobytes() == data.tobytes()


def test_whole_cell_crop_is_the_cropped_block():
    rng = np.random.default_rng(8)
    cell = 2.0 ** -5
    ssz = (8, 16, 4)
    data, slen = mc.random_sdf(rng, ssz, cell=cell, n_inf=0)
    lo, hi = (2, 4, 1), (6, 12, 3)
    bounds = [l * cell for l in lo] + [h * cell for h in hi]
    sizes, lengths, pose = merged_grid_dims([(list(slen), IDENT)], cell, bounds)
    assert sizes == [4, 8, 2] and pose[:3] == bounds[:3]
    assert mc.host_merge_grid([(list(slen), IDENT)], cell, bounds) == (0, sizes, lengths, pose)
    got = mc.host_merge_fields([(data, slen, IDENT)], sizes, lengths, pose)
    want = np.ascontiguousarray(data[2:6, 4:12, 1:3])
    assert got.tobytes() == want.tobytes()
    # (interior cells only: the source's edge cells take their neighbour inwards, which at a centre adds 0 times it)
    full = merged_grid_dims([(list(slen), IDENT)], cell)
    assert full[0] == list(ssz) and full[2] == IDENT
    assert mc.host_merge_fields([(data, slen, IDENT)], full[0], full[1], full[2]).tobytes() == data.tobytes()


# ---- order and coverage --------------------------------------------------------------------------------------------------

def test_order_reach_and_coverage(case):
    sources, sizes, lengths, pose = case["sources"], case["sizes"], case["lengths"], case["pose"]
    base = case["host"]
    # swapping two sources changes no cell (the minimum does not depend on the order; a tie holds the same double)
    for perm in ([1, 0, 2], [2, 1, 0], [1, 2, 0]):
        assert mc.host_merge_fields([sources[k] for k in perm], sizes, lengths, pose).tobytes() == base.tobytes()
    # a source moved out of reach changes no cell
    far = (sources[0][0], sources[0][1], np.concatenate([[50.0, -60.0, 70.0], sources[0][2][3:]]))
    two = mc.host_merge_fields(sources[1:], sizes, lengths, pose)
    assert mc.host_merge_fields([far] + list(sources[1:]), sizes, lengths, pose).tobytes() == two.tobytes()
    assert two.tobytes() != base.tobytes()
    # a target outside every source is all +inf
    away = np.concatenate([[40.0, 40.0, 40.0], pose[3:]])
    out = mc.host_merge_fields(sources, sizes, lengths, away)
    assert np.isposinf(out).all()
    # no source at all: the same
    assert np.isposinf(mc.host_merge_fields([], [3, 2, 4], [0.3, 0.2, 0.4], IDENT)).all()


def test_pose_helpers_of_the_specification():
    rng = np.random.default_rng(9)
    for _ in range(20):
        pose = list(rng.uniform(-2, 2, size=3)) + list(mc.random_quat(rng))
        p = rng.uniform(-1, 1, size=3)
        w = pose_apply(pose, p)
        assert np.allclose(w, mc.rotation(pose[3:]) @ p + pose[:3], rtol=0, atol=1e-14)
        assert np.allclose(pose_apply(pose_invert(pose), w), p, rtol=0, atol=1e-13)
    assert pose_apply(IDENT, [0.1, 0.2, 0.3]) == [0.1, 0.2, 0.3]
