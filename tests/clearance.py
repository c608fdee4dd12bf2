"""TEST INFRASTRUCTURE: the clearance of a trajectory restated on the host from the oracle's pieces, for
tests/test_host_clearance.py and tests/test_gpu_clearance.py.

Per trajectory, from the doubles batch_gettraj returns: the samples of or_cdchomp_amd.module.verdict_samples, the link frames
of OraRobot.fk, the run's sphere list, active flags and self_excluded of an OraRun, ora_kin's pose composition into every
field's frame and OraGrid.interp for the value.  The result is what orc_batch_clearance reports of the run -- the two minima,
their keys and times, n_samples -- and every item behind them, with the distance of its point from the nearest cell face of
its field: the field value jumps at cell faces, so a minimum that sits on one cannot be held to a restatement."""
import numpy as np

from or_cdchomp_amd.module import verdict_samples

FACE_EPS = 1e-7          # cells: an item this close to a cell face "can switch" cells under a rounding difference


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2*(y*y + z*z), 2*(x*y - z*w), 2*(x*z + y*w)], [2*(x*y + z*w), 1 - 2*(x*x + z*z), 2*(y*z - x*w)],
                     [2*(x*z - y*w), 2*(y*z + x*w), 1 - 2*(x*x + y*y)]])


class Field:
    """a field as the restatement reads it: an OraGrid, its pose in the world, the largest jump between adjacent cells"""

    def __init__(self, O, data, lengths, pose_world_gsdf):
        self.grid = data if isinstance(data, O.OraGrid) else O.OraGrid(data, lengths)
        self.pose = O.f64(pose_world_gsdf)
        self.inv = np.zeros(7)
        O.lib().ora_kin_pose_invert(O.dp(self.pose), O.dp(self.inv))
        d = self.grid.data
        self.sizes = np.array(d.shape, dtype=np.float64)
        self.lengths = np.array([self.grid.g.lengths[i] for i in range(3)])
        jump = 0.0
        for ax in range(3):
            a = np.moveaxis(d, ax, 0)
            lo, hi = a[:-1], a[1:]
            ok = np.isfinite(lo) & np.isfinite(hi)
            if ok.any():
                jump = max(jump, float(np.abs(hi[ok] - lo[ok]).max()))
        self.jump = jump


class Tables:
    """the run's spheres in XML order (the robot's, then those of the bodies it holds): link, position on the link, radius,
    active flag; and the pairs the self-collision leg never tests.  held: the grabbed tuples of OraRobot."""

    def __init__(self, O, model, base, dofvals, adofs, fields, held=(), floating=False):
        self.O = O
        self.base = O.f64(base); self.dofvals = O.f64(dofvals); self.adofs = list(adofs)
        self.robot = O.OraRobot(model, grabbed=list(held))
        goal = self.dofvals[self.adofs]
        run = O.OraRun(self.robot, self.base, self.dofvals, self.adofs, goal, [f.grid for f in fields], [f.pose for f in fields],
                       O.default_params(n_points=4, floating_base=1 if floating else 0), basegoal=self.base if floating else None)
        a = model.arrays()
        link = list(a["sphere_link"]); pos = [p for p in a["sphere_pos"]]; rad = list(a["sphere_radius"])
        R, t, _, _ = self.robot.fk(self.base, self.dofvals)
        for hl, kpose, kpos, krad in [h[:4] for h in held]:
            for p, r in zip(np.asarray(kpos, dtype=np.float64).reshape(-1, 3), krad):
                world = _rot(kpose[3:7]) @ p + np.asarray(kpose[:3], dtype=np.float64)
                link.append(int(hl)); pos.append(np.linalg.inv(R[hl]) @ (world - t[hl])); rad.append(float(r))      # (the WAM's base quaternion is not a unit one: no transpose)
        self.link = np.asarray(link, dtype=np.int64); self.pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
        self.rad = np.asarray(rad, dtype=np.float64)
        self.S = run.S
        assert self.S == len(self.rad)
        order = list(run.sphere_order())
        self.active = np.zeros(self.S, dtype=bool); self.active[order[:run.Sa]] = True
        excl = run.self_excluded()
        self.pairs = [(a_, b_) for a_ in range(self.S) for b_ in range(a_ + 1, self.S) if not excl[a_, b_]]
        run.destroy()


def restate(tab, traj, vmax, col0, fields, self_check=True):
    """one trajectory [n_points][n] of doubles against `fields` (the run's scene, in its order).  Returns a dict:
    clearance [2], time [2], sphere [2], other [2], n_samples as orc_batch_clearance reports them; and the items: fgap, fkey
    [items][3] (sample, sphere, field), fface (cells from the nearest face), ftime; pgap, pkey [items][3] (sample, a, b), ptime."""
    O = tab.O
    T = np.asarray(traj, dtype=np.float64)
    seg, u, times = verdict_samples(T, vmax, col0)
    fgap, fkey, fface, ftime, pgap, pkey, ptime = [], [], [], [], [], [], []
    act = np.flatnonzero(tab.active)
    pa = np.array([p[0] for p in tab.pairs], dtype=np.int64); pb = np.array([p[1] for p in tab.pairs], dtype=np.int64)
    rsum = tab.rad[pa] + tab.rad[pb] if len(pa) else np.zeros(0)
    pg = np.zeros(3)
    for k in range(len(seg)):
        a0, a1 = T[seg[k]], T[seg[k] + 1]
        row = a0 + (a1 - a0) * u[k]
        base = tab.base
        if col0:
            base = np.ascontiguousarray(row[:7])
            O.lib().ora_kin_pose_normalize(O.dp(base))
        q = tab.dofvals.copy()
        q[tab.adofs] = row[col0:]
        R, t, _, _ = tab.robot.fk(base, q)
        pw = np.einsum("sij,sj->si", R[tab.link], tab.pos) + t[tab.link]
        for si in act:
            p = np.ascontiguousarray(pw[si])
            for fi, f in enumerate(fields):
                O.lib().ora_kin_pose_compos(O.dp(f.inv), O.dp(p), O.dp(pg))
                err, val = f.grid.interp(pg)
                if err or not np.isfinite(val):      # outside this field; a poisoned value, a NaN: never the minimum
                    continue
                x = pg / f.lengths * f.sizes
                fgap.append(val - tab.rad[si]); fkey.append((k, int(si), fi)); ftime.append(times[k])
                fface.append(float(np.abs(x - np.round(x)).min()))
        if self_check and len(pa):
            d = pw[pa] - pw[pb]
            dist = np.sqrt(d[:, 0]*d[:, 0] + d[:, 1]*d[:, 1] + d[:, 2]*d[:, 2])
            pgap.extend(dist - rsum); pkey.extend((k, int(a_), int(b_)) for a_, b_ in zip(pa, pb)); ptime.extend([times[k]] * len(pa))
    out = dict(n_samples=len(seg), fgap=np.asarray(fgap, dtype=np.float64), fkey=np.asarray(fkey, dtype=np.int64).reshape(-1, 3),
               fface=np.asarray(fface, dtype=np.float64), ftime=np.asarray(ftime, dtype=np.float64),
               pgap=np.asarray(pgap, dtype=np.float64), pkey=np.asarray(pkey, dtype=np.int64).reshape(-1, 3),
               ptime=np.asarray(ptime, dtype=np.float64), times=times)
    clear = np.full(2, np.inf); tim = np.full(2, -1.0); sph = np.full(2, -1, dtype=np.int32); oth = np.full(2, -1, dtype=np.int32)
    for leg, (gap, key, tm) in enumerate(((out["fgap"], out["fkey"], out["ftime"]), (out["pgap"], out["pkey"], out["ptime"]))):
        ok = np.flatnonzero(~np.isnan(gap))
        if len(ok):
            i = ok[int(np.argmin(gap[ok]))]      # (the first of equal minima: the items are in key order)
            clear[leg] = gap[i]; tim[leg] = tm[i]; sph[leg] = key[i, 1]; oth[leg] = key[i, 2]
    out.update(clearance=clear, time=tim, sphere=sph, other=oth)
    return out


def set_aside(res, fields):
    """the face premise: an item that can switch cells has a gap below the run's minimum plus the largest jump between two
    adjacent cells of its field -- the run's minimum may be another number on the device, rightly"""
    if not len(res["fgap"]):
        return False
    jump = np.array([f.jump for f in fields])[res["fkey"][:, 2]]
    can = res["fface"] < FACE_EPS
    return bool((can & (res["fgap"] < res["clearance"][0] + jump)).any())


def first_contact(res):
    """the first item with a negative gap in the verdict's order -- sample by sample the fields first (sphere, then field),
    then the pairs -- as (time, sphere, field or -2 - other sphere, depth), or None"""
    fneg = np.flatnonzero(res["fgap"] < 0.0); pneg = np.flatnonzero(res["pgap"] < 0.0)
    fs = res["fkey"][fneg[0], 0] if len(fneg) else None
    ps = res["pkey"][pneg[0], 0] if len(pneg) else None
    if fs is None and ps is None:
        return None
    if ps is None or (fs is not None and fs <= ps):
        i = fneg[0]
        return float(res["ftime"][i]), int(res["fkey"][i, 1]), int(res["fkey"][i, 2]), float(-res["fgap"][i])
    i = pneg[0]
    return float(res["ptime"][i]), int(res["pkey"][i, 1]), -2 - int(res["pkey"][i, 2]), float(-res["pgap"][i])


# ---- the synthetic trajectories of the chunk-edge test (tests/test_gpu_clearance.py; their premises: tests/test_host_clearance.py)
CHUNK = 64                                         # samples the kernel walks at a time (the WAM's rows fit the LDS)
IN_TABLE = [1.2, -0.2, 0.0, 0.3, 0.0, 0.0, 0.0]    # the forearm in the table top (tests/test_gpu_verdict_device.py)
SYNTH_POINTS = 12
SYNTH_NAMES = ("short", "zigzag", "chunk multiple", "min at sample 0", "min at last sample", "zero length", "twin a", "twin b",
               "penetrates", "through and out")


def zigzag(a, b, n_points, total_len):
    """n_points rows going back and forth on the line a -> b in n_points - 1 equal segments of C-space length
    total_len / (n_points - 1): the polyline's length is total_len"""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    d = total_len / (n_points - 1) / float(np.linalg.norm(b - a))
    assert d <= 1.0
    s = np.array([d * (i % 2) for i in range(n_points)])
    return a[None, :] + s[:, None] * (b - a)[None, :]


def line(a, b, n_points=SYNTH_POINTS):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return a[None, :] + np.linspace(0.0, 1.0, n_points)[:, None] * (b - a)[None, :]


def synthetic_runs(start):
    """[10][SYNTH_POINTS][7]: the cases of SYNTH_NAMES, from the WAM's start configuration"""
    start = np.asarray(start, dtype=np.float64)
    table = np.asarray(IN_TABLE)
    near = start + 0.15 * (table - start)                                        # a centimetre and a half above the table
    wrist = start + np.array([0, 0, 0, 0, 0.3, 0.2, 0.3])
    turn = start + np.array([0, 0, 0, 0, -0.5, 0.2, 0.4])
    far = start + np.array([0, 0, 0, 0, -2.6, 0, 0])
    runs = [line(start, wrist),                                                  # 0.47 rad: a dozen samples
            zigzag(start, turn, SYNTH_POINTS, 2.5 * CHUNK * 0.04),                # between two and three chunks
            zigzag(start, turn, SYNTH_POINTS, (2 * CHUNK - 0.5) * 0.04),          # 128 samples: two full chunks
            line(near, start),
            line(far, near),                                                      # 66 samples: the last one is the second of a chunk
            np.tile(start, (SYNTH_POINTS, 1)),
            line(start, turn), line(start, turn),
            line(start, table),
            line(start, start + 1.6 * (table - start))]
    return np.array(runs)
