"""TEST INFRASTRUCTURE: the penetration cost of a configuration and its gradient restated on the host from the oracle's pieces,
for tests/test_host_penetration.py and tests/test_gpu_penetration.py.

Per row: the link frames, joint axes and anchors of OraRobot.fk, the spheres, active flags and pairs of clearance.Tables, the
items of clearance.restate (every active sphere against every field that contains it; every pair), OraGrid.interp for a
field's value and OraGrid.grad for its slope.  U_f = 1/2 sum max(0, m_f - gap)^2 over the field items, U_s the same over the
pairs with m_s, and the gradient of U_f + U_s with respect to the row by the chain rule, joint by joint.

The base of a fixed robot need not be a rotation (the WAM's quaternion has length 1.0000046): with Rb its matrix, the spheres
are p = Rb (chain) + tb, and a revolute joint moves one by Rb (a_l x r_l) = C (a x r) with C = Rb Rb^T / det Rb and a, r the
world axis and lever of OraRobot.fk -- so the joint's entry is a . (r x C f).  C is the identity for a rotation."""
import numpy as np

import clearance as CL
import config_clearance as CC

H = 1e-6                 # the finite-difference step of the tests
FACE_EPS_32 = 1e-4       # cells: the face premise for a precision-32 batch
MARGINS = ((0.0, 0.0), (0.02, 0.0), (0.05, 0.05))      # (fields, self) of the tests; [1] is the calls' default
# The margins at which cost and gradient are held to the restatement, relative to the row's largest entry.  The self margin of
# the third stays below 0.0154, the gap of the WAM's pairs that no column moves: their forces cancel in every column, and what is
# left of them in a gradient is rounding (and the 1e-5 by which the base's matrix is not a rotation) of summands a million
# times larger -- 3e-8 in the restatement itself for "away" at (0.05, 0.05).  A row with nothing else in contact then has no
# largest entry for an error to be relative to; the absolute checks (central differences, zero cost, bit for bit) keep 0.05.
RESTATED = ((0.0, 0.0), (0.02, 0.0), (0.05, 0.01))
SHIFT = np.array([0.03, -0.04, 0.02, 0.0, 0.0, 0.0, 1.0])      # where the second scene of the per-run tests puts the table
CPU_STEPS = [2, 1, 3, 4, 5, 2, 3]      # push_out's steps on named_rows() against the restatement, margins (0.02, 0), slack 2e-3, cap 0.2


def compose(O, a, b):
    out = np.zeros(7)
    O.lib().ora_kin_pose_compose(O.dp(O.f64(a)), O.dp(O.f64(b)), O.dp(out))
    return out


def floating_base():
    """the base pose of the floating-base tests (tests/test_gpu_config_clearance.py: the WAM a little nearer the table)"""
    import common
    base = np.asarray(common.wam_state()[1], dtype=np.float64).copy()
    base[0] -= 0.2
    return base


def named_rows():
    """the seven rows of the push-out table: name -> WAM configuration"""
    f = CC.wam_fixed()
    s, t = f["start"], f["in the table"]
    fold = CC.folding_configs()
    return {"in the table": t, "near": f["near"], "a = 0.3": s + 0.3 * (t - s), "a = 0.4": s + 0.4 * (t - s), "a = 0.5": s + 0.5 * (t - s),
            "folding 0": fold[0], "folding 1": fold[1]}


def wam_rows():
    """the WAM pool of tests/config_clearance.py and the seven named rows: name -> configuration"""
    rows = {("pool %d" % k): q for k, q in enumerate(CC.wam_pool())}
    for k, name in enumerate(CC.wam_fixed()):
        rows[name] = rows.pop("pool %d" % k)
    rows.update(named_rows())
    return rows


def _joint_links(tab, model_arrays):
    """per column behind col0: the links whose joint the column's dof drives"""
    jt, di = model_arrays["joint_type"], model_arrays["dof_index"]
    return [[li for li in range(len(jt)) if jt[li] != 0 and di[li] == d] for d in tab.adofs]


def _ancestors(parent, link):
    out = set()
    while link >= 0:
        out.add(link); link = parent[link]
    return out


def restate(tab, row, col0, fields, margin, self_check=True):
    """one row [n] against `fields`.  Returns a dict: cost [2], grad [n], clearance [2], sphere [2], other [2] as the device
    call reports them, and the items behind them: fgap, fkey [items][2] (sphere, field), fface (cells from the nearest cell
    face OR half-cell plane, where the lookup's neighbour switches), pgap, pkey [items][2]."""
    O = tab.O
    a = tab.robot._keep
    parent = a["parent"]
    row = np.asarray(row, dtype=np.float64)
    n = len(row)
    base = tab.base
    if col0:
        base = np.array(row[:7])      # (a copy: the caller's row keeps its quaternion's length)
        O.lib().ora_kin_pose_normalize(O.dp(base))
    q = tab.dofvals.copy()
    q[tab.adofs] = row[col0:]
    R, t, ax, an = tab.robot.fk(base, q)
    pw = np.einsum("sij,sj->si", R[tab.link], tab.pos) + t[tab.link]
    S = tab.S
    force = np.zeros((S, 3))
    m_f, m_s = float(margin[0]), float(margin[1])
    cost = np.zeros(2)
    fgap, fkey, fface, pgap, pkey = [], [], [], [], []
    pg = np.zeros(3)
    for si in np.flatnonzero(tab.active):
        p = np.ascontiguousarray(pw[si])
        for fi, f in enumerate(fields):
            O.lib().ora_kin_pose_compos(O.dp(f.inv), O.dp(p), O.dp(pg))
            err, val = f.grid.interp(pg)
            if err or not np.isfinite(val):
                continue
            gap = val - tab.rad[si]
            x = pg / f.lengths * f.sizes
            fgap.append(gap); fkey.append((int(si), fi))
            fface.append(float(min(np.abs(x - np.round(x)).min(), np.abs(x - 0.5 - np.round(x - 0.5)).min())))
            if gap < m_f:
                d = m_f - gap
                cost[0] += 0.5 * d * d
                err, gg = f.grid.grad(pg)
                assert not err
                force[si] += -d * (CL._rot(f.inv[3:7]).T @ gg)
    if self_check:
        for (sa, sb) in tab.pairs:
            dv = pw[sa] - pw[sb]
            dist = np.sqrt(dv[0]*dv[0] + dv[1]*dv[1] + dv[2]*dv[2])
            gap = dist - (tab.rad[sa] + tab.rad[sb])
            pgap.append(gap); pkey.append((int(sa), int(sb)))
            if gap < m_s:
                d = m_s - gap
                cost[1] += 0.5 * d * d
                if dist != 0.0:
                    if tab.active[sa]:
                        force[sa] += -d * dv / dist
                    if tab.active[sb]:
                        force[sb] += d * dv / dist
    grad = np.zeros(n)
    Rb = CL._rot(base[3:7])
    C = Rb @ Rb.T / np.linalg.det(Rb)
    links = _joint_links(tab, a)
    for si in np.flatnonzero(tab.active):
        if not force[si].any():
            continue
        anc = _ancestors(parent, int(tab.link[si]))
        for c, ls in enumerate(links):
            for lj in ls:
                if lj not in anc:
                    continue
                if a["joint_type"][lj] == 1:
                    grad[col0 + c] += ax[lj] @ np.cross(pw[si] - an[lj], C @ force[si])
                else:
                    grad[col0 + c] += ax[lj] @ force[si]
    if col0:
        F = force[tab.active].sum(axis=0)
        tau = np.cross(pw[tab.active], force[tab.active]).sum(axis=0)
        tq = tau - np.cross(base[:3], F)
        qx, qy, qz, qw = 2.0 * base[3:7]
        gu = np.array([qw*tq[0] + qz*tq[1] - qy*tq[2], -qz*tq[0] + qw*tq[1] + qx*tq[2], qy*tq[0] - qx*tq[1] + qw*tq[2],
                       -qx*tq[0] - qy*tq[1] - qz*tq[2]])
        grad[:3] = F
        grad[3:7] = gu / np.linalg.norm(row[3:7])      # (gu is tangent to the unit sphere: the renormalisation only scales it)
    out = dict(cost=cost, grad=grad, fgap=np.asarray(fgap), fkey=np.asarray(fkey, dtype=np.int64).reshape(-1, 2), fface=np.asarray(fface),
               pgap=np.asarray(pgap), pkey=np.asarray(pkey, dtype=np.int64).reshape(-1, 2))
    clear = np.full(2, np.inf); sph = np.full(2, -1, dtype=np.int32); oth = np.full(2, -1, dtype=np.int32)
    for leg, (gap, key) in enumerate(((out["fgap"], out["fkey"]), (out["pgap"], out["pkey"]))):
        if len(gap):
            i = int(np.argmin(gap))
            clear[leg] = gap[i]; sph[leg] = key[i, 0]; oth[leg] = key[i, 1]
    out.update(clearance=clear, sphere=sph, other=oth)
    return out


def evaluator(tab, col0, fields, self_check=True):
    """the restatement in the shape push_out takes: evaluate(rows, margin) -> dict of cost, grad, clearance"""
    def evaluate(rows, margin):
        res = [restate(tab, r, col0, fields, margin, self_check) for r in np.asarray(rows, dtype=np.float64).reshape(-1, len(tab.adofs) + col0)]
        return {key: np.array([r[key] for r in res]) for key in ("cost", "grad", "clearance", "sphere", "other")}
    return evaluate


def central_differences(cost_of, row, h=H):
    """[n]: (U(row + h e_c) - U(row - h e_c)) / 2h with U = cost_of(rows [k][n]) -> [k] evaluated in one call"""
    row = np.asarray(row, dtype=np.float64)
    n = len(row)
    rows = np.tile(row, (2 * n, 1))
    for c in range(n):
        rows[2*c, c] += h; rows[2*c + 1, c] -= h
    U = np.asarray(cost_of(rows), dtype=np.float64).reshape(2 * n)
    return (U[0::2] - U[1::2]) / (2.0 * h)


def fd_rows(row, h=H):
    """the 2n rows central_differences evaluates"""
    row = np.asarray(row, dtype=np.float64)
    rows = np.tile(row, (2 * len(row), 1))
    for c in range(len(row)):
        rows[2*c, c] += h; rows[2*c + 1, c] -= h
    return rows


def single_item_rows(tab, col0, fields, rows, margin):
    """bool [len(rows)]: exactly one item violates, a field item"""
    res = [restate(tab, q, col0, fields, margin) for q in rows]
    return np.array([(r["fgap"] < margin[0]).sum() == 1 and (r["pgap"] < margin[1]).sum() == 0 for r in res])


def contributing_face_distance(res, margin):
    """the smallest fface among the field items that contribute at `margin` (inf: none contributes)"""
    on = res["fgap"] < margin[0]
    return float(res["fface"][on].min()) if on.any() else np.inf
