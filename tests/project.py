"""Shared inputs and the restatement of the TSR projection tests (tests/test_host_project.py, tests/test_gpu_project_tsr.py).

The restatement is or_cdchomp_amd.project.project with evaluate = the oracle's eval_contsr: the value and Jacobian of con_tsr,
held to a second restatement and to its own finite differences in tests/test_oracle_random_robots.py."""
import numpy as np

import common
from or_cdchomp_amd import project, robots

TOOL = [0.0, 0.0, 0.16, 0.0, 0.0, 0.0, 1.0]      # the WAM's manipulator `arm`: handbase with this tool
IDENT = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
BW6 = [[0, 0]] * 6                                                          # all six rows
BW3 = [[-1, 1], [-1, 1], [0, 0], [0, 0], [0, 0], [-3, 3]]                   # z, roll, pitch (test_con_tsr_all_matches_oracle)
BW1 = [[0, 0], [-1, 1], [-1, 1], [-3, 3], [-3, 3], [-3, 3]]                 # x only
TOL = 1e-6
N_TARGETS = 32
TWE = [0.03, -0.02, 0.05] + list(robots.quat_from_axis_angle((0.2, 1.0, -0.4), 0.5))      # a Twe that is not the identity


def unit_base():
    """the base of tests/test_gpu_tsr.py: a rotation (the WAM's default base matrix is not one)"""
    s2 = np.sqrt(0.5)
    return [-1.0, 0.0, 1.0, 0.0, s2, 0.0, s2]


def wam_limits():
    model = robots.wam7()
    return np.asarray(model.limit_lower[:7], dtype=np.float64), np.asarray(model.limit_upper[:7], dtype=np.float64)


def p1_inputs(spread=0.2):
    """(q* [32][7], seeds [32][7]): q* = clip(WAM_START + 0.4 u, limits -+ 0.05), seeds = clip(q* + spread u', limits), default_rng(11)"""
    lo, hi = wam_limits()
    rng = np.random.default_rng(11)
    u = rng.uniform(-1.0, 1.0, size=(N_TARGETS, 7))
    v = rng.uniform(-1.0, 1.0, size=(N_TARGETS, 7))
    qstar = np.clip(np.asarray(robots.WAM_START)[None, :] + 0.4 * u, lo + 0.05, hi - 0.05)
    return qstar, np.clip(qstar + spread * v, lo, hi)


def rot(q):
    x, y, z, w = q
    return np.array([[1 - 2*(y*y + z*z), 2*(x*y - z*w), 2*(x*z + y*w)],
                     [2*(x*y + z*w), 1 - 2*(x*x + z*z), 2*(y*z - x*w)],
                     [2*(x*z - y*w), 2*(y*z + x*w), 1 - 2*(x*x + y*y)]])


def hom(R, t):
    H = np.eye(4); H[:3, :3] = R; H[:3, 3] = t
    return H


def target_frames(model, base, dofvals, adofs, link, tool, rows, twe=IDENT):
    """(R [q][3][3], d [q][3]) of T0w for which the end effector (link o tool) at every row sits at the TSR's origin:
    T0w = link o tool o Twe^-1"""
    li = model.link_names.index(link)
    Rs, ds = [], []
    for q in np.atleast_2d(rows):
        dv = np.array(dofvals, dtype=np.float64); dv[adofs] = q
        R, t = model.link_frames(base, dv)
        H = hom(R[li], t[li]) @ hom(rot(tool[3:]), tool[:3]) @ np.linalg.inv(hom(rot(twe[3:]), twe[:3]))
        Rs.append(H[:3, :3]); ds.append(H[:3, 3])
    return np.array(Rs), np.array(ds)


def tsrs_at(Rs, ds, Bw, twe=IDENT):
    """robots.Tsr objects at those frames"""
    return [robots.Tsr(T0w_R=R, T0w_d=d, Twe_R=rot(twe[3:]), Twe_d=twe[:3], Bw=Bw) for R, d in zip(Rs, ds)]


class OracleTsrs:
    """the oracle's con_tsr of a list of robots.Tsr on one robot state: evaluate(rows, index) -> (h [q][k], J [q][k][n]) with
    tsr_of[index] the constraint of a row.  One oracle run per constraint (a run's constraint 0)."""

    def __init__(self, O, model, base, dofvals, adofs, link, tool, tsrs, tsr_of=None, floating=False):
        self.O = O
        rob = O.OraRobot(model)
        self.keep = rob
        li = model.link_names.index(link)
        kw = dict(n_points=4)
        if floating:
            kw["floating_base"] = 1
        goal = np.asarray(dofvals, dtype=np.float64)[adofs]
        # (a run needs a field to exist; con_tsr never looks at it: eight cells a hundred metres away)
        self.grid = O.OraGrid(np.ones((2, 2, 2)), [0.1, 0.1, 0.1])
        far = [[100.0, 100.0, 100.0, 0.0, 0.0, 0.0, 1.0]]
        self.runs = []
        self.k = []
        for t in tsrs:
            run = O.OraRun(rob, base, dofvals, adofs, goal, [self.grid], far, O.default_params(**kw), basegoal=base if floating else None)
            T0w, Twe = t.poses()
            self.k.append(run.add_contsr(li, tool, T0w, Twe, t.Bw))
            self.runs.append(run)
        self.tsr_of = np.zeros(0, dtype=np.int64) if tsr_of is None else np.asarray(tsr_of)
        self.n = self.runs[0].n

    def of(self, index):
        return self.tsr_of[index] if len(self.tsr_of) else np.zeros(len(index), dtype=np.int64)

    def evaluate(self, rows, index=None):
        """h and J zero-padded to six rows, so that rows of different k stack"""
        rows = np.atleast_2d(rows)
        index = np.arange(len(rows)) if index is None else index
        which = self.of(index)
        h = np.zeros((len(rows), 6)); J = np.zeros((len(rows), 6, self.n))
        for i, (q, w) in enumerate(zip(rows, which)):
            hi, Ji = self.runs[w].eval_contsr(0, q)
            h[i, :len(hi)] = hi; J[i, :len(hi)] = Ji
        return h, J

    def ks(self, index):
        return np.asarray(self.k)[self.of(index)]

    def project(self, rows, history=None, **kw):
        """the restatement: project.project around evaluate"""
        return project.project(self.evaluate, rows, k=self.ks(np.arange(len(np.atleast_2d(rows)))), indexed=True, history=history, **kw)

    def destroy(self):
        for r in self.runs:
            r.destroy()


def wam_case(O, base, Bw=BW6, link="handbase", tool=TOOL, twe=IDENT, spread=0.2):
    """the P1 inputs on the WAM with `base`: dict(model, dofvals, adofs, qstar, seeds, tsrs, ora, lower, upper)"""
    model, _, dofvals, adofs = common.wam_state()
    qstar, seeds = p1_inputs(spread)
    Rs, ds = target_frames(model, base, dofvals, adofs, link, tool, qstar, twe)
    tsrs = tsrs_at(Rs, ds, Bw, twe)
    ora = OracleTsrs(O, model, base, dofvals, adofs, link, tool, tsrs, tsr_of=np.arange(N_TARGETS))
    lo, hi = wam_limits()
    return dict(model=model, dofvals=dofvals, adofs=adofs, qstar=qstar, seeds=seeds, tsrs=tsrs, ora=ora, lower=lo, upper=hi)


UNREACHABLE = dict(T0w_R=np.eye(3), T0w_d=[3.0, 0.0, 1.0])      # P5: a target three metres away


def tree_case(O):
    """the 30-dof tree of tests/config_clearance.py with a TSR on link L6 of the left branch: the torso's two dofs and L0 .. L6
    move it, nothing else does.  dict(model, base, dofvals, adofs, qstar, seeds, tsrs, ora, moving)"""
    model = robots.tree30()
    base = [0.0] * 6 + [1.0]
    dofvals = np.zeros(model.n_dof); adofs = list(range(model.n_dof))
    rng = np.random.default_rng(12)
    qstar = rng.uniform(-0.6, 0.6, size=(6, model.n_dof))
    seeds = qstar + 0.15 * rng.uniform(-1.0, 1.0, size=qstar.shape)
    Rs, ds = target_frames(model, base, dofvals, adofs, "L6", IDENT, qstar)
    tsrs = tsrs_at(Rs, ds, BW6)
    ora = OracleTsrs(O, model, base, dofvals, adofs, "L6", IDENT, tsrs, tsr_of=np.arange(len(qstar)))
    moving = np.zeros(model.n_dof, dtype=bool)
    li = model.link_names.index("L6")
    while li >= 0:
        if model.dof_index[li] >= 0:
            moving[model.dof_index[li]] = True
        li = model.parent[li]
    return dict(model=model, base=base, dofvals=dofvals, adofs=adofs, qstar=qstar, seeds=seeds, tsrs=tsrs, ora=ora, moving=moving)
