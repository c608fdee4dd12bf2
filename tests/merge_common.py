"""Shared builders for test_host_merge_fields.py and test_gpu_merge_fields.py: the three-source case, the library's host
calls as numpy functions, and the independent reading of the specification over the oracle's grid interpolation."""
import ctypes as C

import numpy as np

from or_cdchomp_amd import _capi

INF = np.inf
CELL = 0.05
SOURCE_SIZES = ((9, 7, 8), (6, 10, 5), (12, 5, 7))
TARGET_SIZES = (17, 13, 11)
SEED = 20260


def _dp(a):
    return a.ctypes.data_as(_capi.c_double_p)


def _ip(a):
    return a.ctypes.data_as(_capi.c_int_p)


def host_merge_grid(boxes, cell, bounds=None):
    """orc_host_merge_grid: (rc, sizes, lengths, pose)"""
    lens = np.ascontiguousarray([b[0] for b in boxes], dtype=np.float64).reshape(-1, 3)
    poses = np.ascontiguousarray([b[1] for b in boxes], dtype=np.float64).reshape(-1, 7)
    bd = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.float64)
    sizes = np.zeros(3, dtype=np.int32); lengths = np.zeros(3); pose = np.zeros(7)
    rc = _capi.lib().orc_host_merge_grid(len(boxes), _dp(lens) if len(boxes) else None, _dp(poses) if len(boxes) else None,
                                         float(cell), None if bd is None else _dp(bd), _ip(sizes), _dp(lengths), _dp(pose))
    return rc, [int(s) for s in sizes], [float(v) for v in lengths], [float(v) for v in pose]


def host_merge_fields(sources, sizes, lengths, pose_world_gsdf):
    """orc_host_merge_fields over sources [(data, lengths, pose_world_gsrc)]: data [sizes]"""
    datas = [np.ascontiguousarray(s[0], dtype=np.float64) for s in sources]
    ssz = np.ascontiguousarray([d.shape for d in datas], dtype=np.int32).reshape(-1, 3)
    slen = np.ascontiguousarray([s[1] for s in sources], dtype=np.float64).reshape(-1, 3)
    spose = np.ascontiguousarray([s[2] for s in sources], dtype=np.float64).reshape(-1, 7)
    ptrs = (_capi.c_double_p * max(len(datas), 1))(*[_dp(d) for d in datas])
    out = np.full(tuple(int(s) for s in sizes), np.nan)
    rc = _capi.lib().orc_host_merge_fields(len(datas), _ip(ssz), _dp(slen), _dp(spose), ptrs,
                                           _ip(np.ascontiguousarray(sizes, dtype=np.int32)),
                                           _dp(np.ascontiguousarray(lengths, dtype=np.float64)),
                                           _dp(np.ascontiguousarray(pose_world_gsdf, dtype=np.float64)), _dp(out))
    assert rc == 0
    return out


def random_sdf(rng, sizes, cell=CELL, n_inf=4):
    """a true distance field: orc_host_bin_sdf of a seeded random occupancy, then a few cells overwritten with +inf"""
    occ = np.where(rng.random(sizes) < 0.12, INF, 0.0)
    occ[0, 0, 0] = 0.0; occ[-1, -1, -1] = INF                     # (both kinds of cell exist)
    lengths = np.asarray(sizes, dtype=np.float64) * cell
    sdf = np.zeros(sizes)
    rc = _capi.lib().orc_host_bin_sdf(_ip(np.asarray(sizes, dtype=np.int32)), _dp(lengths), _dp(np.ascontiguousarray(occ)), _dp(sdf))
    assert rc == 0 and np.isfinite(sdf).all()
    for _ in range(n_inf):
        sdf[tuple(int(rng.integers(0, s)) for s in sizes)] = INF
    return sdf, lengths


def rotation(q):
    """the matrix pose_apply turns a point with (the expanded quaternion products)"""
    qx, qy, qz, qw = q
    return np.array([[qx*qx - qy*qy - qz*qz + qw*qw, 2*(qx*qy - qz*qw), 2*(qx*qz + qy*qw)],
                     [2*(qx*qy + qz*qw), -qx*qx + qy*qy - qz*qz + qw*qw, 2*(qy*qz - qx*qw)],
                     [2*(qx*qz - qy*qw), 2*(qy*qz + qx*qw), -qx*qx - qy*qy + qz*qz + qw*qw]])


def random_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def three_sources(seed=SEED):
    """The three-source case: true distance fields of 9x7x8, 6x10x5 and 12x5x7 cells of 0.05 m with a few +inf cells, at
    seeded generic rotations and offsets, and a target of 17x13x11 cells of 0.05 m (2431: no multiple of 64 or 256) at a
    seeded world pose that lies partly outside every source.  Returns (sources [(data, lengths, pose_world_gsrc)], sizes,
    lengths, pose_world_gsdf)."""
    rng = np.random.default_rng(seed)
    sizes = list(TARGET_SIZES)
    lengths = [s * CELL for s in sizes]
    tq = random_quat(rng)
    tpose = np.concatenate([rng.uniform(-1.5, 1.5, size=3), tq])
    sources = []
    for ssz in SOURCE_SIZES:
        data, slen = random_sdf(rng, ssz)
        q = random_quat(rng)
        # the source's centre lies inside the target's box; the source is smaller than the target, so part of the target is
        # outside it, and turned against it, so part of it is outside the target
        centre_t = rng.uniform(0.3, 0.7, size=3) * np.asarray(lengths)
        centre_w = rotation(tq) @ centre_t + tpose[:3]
        t = centre_w - rotation(q) @ (0.5 * slen)
        sources.append((data, slen, np.concatenate([t, q])))
    return sources, sizes, lengths, tpose


def cell_centres(sizes, lengths):
    """[n][3] cell centres in the grid's frame, C order, as the voxelizer forms them"""
    ax = [(0.5 + np.arange(sizes[d])) / sizes[d] * lengths[d] for d in range(3)]
    g = np.meshgrid(ax[0], ax[1], ax[2], indexing="ij")
    return np.stack([a.reshape(-1) for a in g], axis=1)


def source_points(src_pose, sizes, lengths, pose_world_gsdf):
    """the target's cell centres in a source grid's frame, by the two steps of the specification, in numpy"""
    p_w = cell_centres(sizes, lengths) @ rotation(pose_world_gsdf[3:]).T + np.asarray(pose_world_gsdf[:3])
    qi = np.array([-src_pose[3], -src_pose[4], -src_pose[5], src_pose[6]])
    ti = -(rotation(qi) @ np.asarray(src_pose[:3]))
    return p_w @ rotation(qi).T + ti


def merged_field_over_oracle(oracle, sources, sizes, lengths, pose_world_gsdf):
    """merged_field of or_cdchomp_amd/module.py read independently: numpy for the points, the oracle's grid interpolation
    (OraGrid.interp) for the values, the strict-< loop over the sources in order"""
    n = int(np.prod(sizes))
    best = np.full(n, INF)
    for data, slen, spose in sources:
        grid = oracle.OraGrid(data, slen)
        pts = source_points(spose, sizes, lengths, pose_world_gsdf)
        for i in range(n):
            outside, val = grid.interp(pts[i])
            if not outside and val < best[i]:
                best[i] = val
    return best.reshape(sizes)


def steepest(sources):
    """the largest difference of two finite neighbouring cells over the cell size, over all sources"""
    s = 0.0
    for data, slen, _ in sources:
        for d in range(3):
            diff = np.abs(np.diff(data, axis=d))
            diff = diff[np.isfinite(diff)]
            s = max(s, float(diff.max()) / (slen[d] / data.shape[d]))
    return s


def near_discontinuity(sources, sizes, lengths, pose_world_gsdf, eps=1e-9):
    """(centres within eps, normalised to the source's length, of a boundary face of a source; centres within eps, in cells,
    of a face between two cells of a source that contains them) -- from the specification alone"""
    n_boundary = n_face = 0
    for data, slen, spose in sources:
        x = source_points(spose, sizes, lengths, pose_world_gsdf) / np.asarray(slen)
        n_boundary += int(((np.abs(x) < eps) | (np.abs(x - 1.0) < eps)).any(axis=1).sum())
        inside = ((x >= 0.0) & (x <= 1.0)).all(axis=1)
        u = x[inside] * np.asarray(data.shape)
        n_face += int((np.abs(u - np.round(u)) < eps).any(axis=1).sum())
    return n_boundary, n_face
