"""not gpu: the oracle against the reference's own code (grid.c, grid_flood.c) on randomised scenes beyond the
committed golden grid vectors.  What the reference makes of these scenes is recorded in
tests/golden/ref_random_scenes.npz (tests/golden/make_ref_random_golden.py); where oracle/_ref/libcd_ref.so is
built, the live library is also held to that record."""
import ctypes as C
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_random_scenes.npz")
SEEDS = [0, 1, 2]
FIELDS = ("sdf", "err", "val", "grad", "idx")


class CdGrid(C.Structure):          # struct cd_grid, reference src/libcd/grid.h:29-41
    _fields_ = [("n", C.c_int), ("sizes", C.POINTER(C.c_int)), ("ncells", C.c_size_t),
                ("cell_size", C.c_int), ("data", C.c_void_p), ("lengths", C.POINTER(C.c_double))]


def prepare(R):
    R.cd_grid_double_interp.argtypes = [C.POINTER(CdGrid), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    R.cd_grid_double_grad.argtypes = [C.POINTER(CdGrid), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    R.cd_grid_lookup_index.argtypes = [C.POINTER(CdGrid), C.POINTER(C.c_double), C.POINTER(C.c_size_t)]
    return R


def _ref_grid(R, data, lengths):
    data = np.ascontiguousarray(data, dtype=np.float64)
    sizes = (C.c_int * 3)(*data.shape)
    gp = C.POINTER(CdGrid)()
    init = C.c_double(0.0)
    R.cd_grid_create_sizearray(C.byref(gp), C.byref(init), 8, 3, sizes)
    C.memmove(gp.contents.data, data.ctypes.data, data.nbytes)
    for i in range(3):
        gp.contents.lengths[i] = lengths[i]
    return gp


def scene(seed):
    """occupancy (inf = obstacle), cell lengths and 400 probe points of one randomised scene"""
    rng = np.random.default_rng(seed)
    shape = tuple(int(v) for v in rng.integers(5, 20, size=3))
    lengths = rng.uniform(0.3, 2.0, size=3)
    occ = np.where(rng.uniform(size=shape) < 0.06, np.inf, 0.0)
    occ.flat[0] = 0.0
    pts = rng.uniform(-0.05, 1.05, size=(400, 3)) * lengths
    return occ, lengths, pts


def reference_outputs(R, seed):
    """what the reference's own code makes of scene(seed): cd_grid_double_bin_sdf, and at every probe point the
    error code of cd_grid_double_interp, with its value, cd_grid_double_grad and cd_grid_lookup_index where it is 0"""
    occ, lengths, pts = scene(seed)
    gp = _ref_grid(R, occ, lengths)
    out = C.POINTER(CdGrid)()
    assert R.cd_grid_double_bin_sdf(C.byref(out), gp) == 0
    sdf = np.ctypeslib.as_array(C.cast(out.contents.data, C.POINTER(C.c_double)), shape=occ.shape).copy()
    n = len(pts)
    err, val, grad, idx = np.zeros(n, np.int32), np.zeros(n), np.zeros((n, 3)), np.zeros(n, np.uint64)
    for i, p in enumerate(pts):
        p = np.ascontiguousarray(p)
        v = C.c_double(); g = np.zeros(3); ix = C.c_size_t()
        err[i] = R.cd_grid_double_interp(out, p.ctypes.data_as(C.POINTER(C.c_double)), C.byref(v))
        if err[i] == 0:
            val[i] = v.value
            R.cd_grid_double_grad(out, p.ctypes.data_as(C.POINTER(C.c_double)), g.ctypes.data_as(C.POINTER(C.c_double)))
            grad[i] = g
            R.cd_grid_lookup_index(out, p.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ix))
            idx[i] = ix.value
    return dict(sdf=sdf, err=err, val=val, grad=grad, idx=idx)


@pytest.fixture(scope="module")
def recorded():
    return np.load(GOLDEN)


@pytest.mark.parametrize("seed", SEEDS)
def test_sdf_pipeline_random_scenes(oracle, recorded, seed):
    want = {k: recorded["%s_%d" % (k, seed)] for k in FIELDS}
    R = oracle.ref()
    if R is not None:                     # the reference's own code is built here: it still makes what was recorded
        live = reference_outputs(prepare(R), seed)
        for k in FIELDS:
            assert np.array_equal(live[k], want[k]), k
    occ, lengths, pts = scene(seed)
    og = oracle.OraGrid(occ, lengths)
    sdf = og.bin_sdf()
    assert np.array_equal(sdf.data, want["sdf"])
    for i, p in enumerate(pts):
        p = np.ascontiguousarray(p)
        oe, ov = sdf.interp(p)
        assert oe == want["err"][i]
        if oe == 0:
            assert ov == want["val"][i]
            _, og_ = sdf.grad(p)
            assert np.array_equal(want["grad"][i], og_)
            oidx = C.c_size_t()
            oracle.lib().ora_grid_lookup_index(sdf.ptr, oracle.dp(p), C.byref(oidx))
            assert want["idx"][i] == oidx.value
