"""Robots for the canonical joint frames of the FK walk (csrc/fold.cpp canonical_rotation, csrc/fk.h): the cases, their inputs and
the oracle's side (no GPU).  Shared by tests/test_gpu_fk_canonical.py (the device against the oracle) and
tests/test_host_fk_canonical.py (the conditions on the inputs, on the oracle alone).  NOTES/fk-canonical.md has the figures.

Every case is a small batch of straight-line seeds next to the tabletop: 4 .. 8 runs of 8 .. 12 waypoints, one iteration.  The
seeds are the first (in steps of 7) whose goals give the oracle no joint-limit round on that iteration -- the WAM starts 0.1 from a
limit, and the reference keeps its workspace in G and AG while it makes such rounds --, no sphere next to a switch, and in every
run a gradient entry above G_FLOOR (a run whose spheres are all out of reach has a gradient of rounding noise: nothing to compare)."""
import collections

import numpy as np

import common
from or_cdchomp_amd import robots

Case = collections.namedtuple("Case", "id robot n_runs n_points seed floating tsr held")

CASES = [
    Case("general3", "general3", 6, 10, 1, False, False, False),          # three axes in general position, fixed rotations that are no identity
    Case("prismatic-middle", "prismatic", 6, 9, 9, False, False, False),  # ... the middle joint prismatic
    Case("negative-axes", "signed", 8, 8, 3, False, False, False),        # -x, +y, -z: the signed permutations, no reflection
    Case("fork-general", "fork", 4, 12, 4, False, False, False),          # a frame saved and loaded; six spheres on one link (count > 4)
    Case("floating2", "floating2", 4, 10, 5, True, False, False),         # floating base and two joints
    Case("wam-tsr", "wam", 4, 8, 468, False, True, False),                  # con_tsr on wam7, one row: the true link frame reaches the constraint
    Case("wam-held4", "wam", 4, 8, 14, False, False, True),                # the WAM holding the four-sphere box
]
KW = dict(lambda_=150.0, obs_factor=120.0, obs_factor_self=15.0, epsilon=0.2, epsilon_self=0.06)
WAM_KW = dict(lambda_=100.0, obs_factor=500.0)
BASE = [-0.55, 0.05, 0.75]             # next to the table, where tests/test_gpu_random_robots.py stands its robots
SWITCH = 1e-6                          # no sphere this close to a switch of the field lookup (in cells) or of the cost (in metres)
G_FLOOR = 1e-4                         # every run's largest gradient entry is above this
TSR_LINK = "wam7"
TSR_BW = [[-1, 1], [-1, 1], [0, 0], [-3, 3], [-3, 3], [-3, 3]]      # the height of the link: one row


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _quat(rng):
    return robots.quat_from_axis_angle(tuple(_unit(rng.normal(size=3))), float(rng.uniform(0.3, 1.2)))


def _off_axis_sphere(model, link, axis, rng, radius=0.05):
    """a sphere that is not on the joint's axis: 0.06 .. 0.1 away from it"""
    a = _unit(axis)
    side = _unit(np.cross(a, _unit(rng.normal(size=3))))
    model.add_sphere(link, tuple(float(rng.uniform(0.02, 0.12)) * a + float(rng.uniform(0.06, 0.1)) * side), radius)


def build_robot(name):
    """the RobotModel of a case (the WAM: common.wam_state)"""
    rng = np.random.default_rng([31, sum(ord(c) for c in name)])
    model = robots.RobotModel("canon_" + name)
    R, P = robots.JOINT_REVOLUTE, robots.JOINT_PRISMATIC
    model.add_link("b")

    def joint(nm, parent, axis, kind=R, quat=None):
        model.add_link(nm, parent, tuple(rng.uniform(-0.05, 0.05, size=2)) + (float(rng.uniform(0.12, 0.2)),), _quat(rng) if quat is None else quat,
                       joint=kind, axis=tuple(axis), limits=(-0.25, 0.25) if kind == P else (-2.2, 2.2))
        _off_axis_sphere(model, nm, axis, rng)

    if name in ("general3", "prismatic"):
        for j in range(3):
            joint("j%d" % j, "b" if j == 0 else "j%d" % (j - 1), _unit(rng.normal(size=3)), P if (name == "prismatic" and j == 1) else R)
    elif name == "signed":
        for j, axis in enumerate(((-1, 0, 0), (0, 1, 0), (0, 0, -1))):
            joint("j%d" % j, "b" if j == 0 else "j%d" % (j - 1), axis)
    elif name == "fork":
        joint("j0", "b", _unit(rng.normal(size=3)))
        joint("j1", "j0", (0, 1, 0))
        for side in "lr":
            joint(side + "0", "j1", _unit(rng.normal(size=3)))
            joint(side + "1", side + "0", _unit(rng.normal(size=3)))
        for _ in range(5):                       # six spheres on l1: past the four of the joint's record
            _off_axis_sphere(model, "l1", model.axis[model.link_names.index("l1")], rng, radius=0.035)
    elif name == "floating2":
        model.add_sphere("b", (0.02, -0.03, 0.05), 0.07)
        joint("j0", "b", _unit(rng.normal(size=3)))
        joint("j1", "j0", _unit(rng.normal(size=3)))
    else:
        raise KeyError(name)
    return model


_PROBLEMS = {}


def problem(case, oracle):
    """dict(model, rob, base, dofvals, adofs, goals, basegoals, grids, poses, radius, kw, grabbed)"""
    if case.id in _PROBLEMS:
        return _PROBLEMS[case.id]
    rng = np.random.default_rng([57, case.seed])
    table = common.tabletop_problem(oracle)
    grabbed, basegoals = [], None
    if case.robot == "wam":
        model, base, dofvals, adofs = common.wam_state()
        goals = common.wam_goals(case.n_runs, seed=100 + case.seed)
        kw = dict(WAM_KW)
        if case.held:
            grabbed = [(model.link_names.index("handbase"), common.held4_pose(model), common.HELD4_POS, common.HELD4_RAD)]
    else:
        model = build_robot(case.robot)
        base = BASE + list(_quat(rng))
        adofs = list(range(model.n_dof))
        lo = np.maximum(model.limit_lower, -1.4); hi = np.minimum(model.limit_upper, 1.4)
        dofvals = rng.uniform(0.6 * lo, 0.6 * hi)
        goals = rng.uniform(0.6 * lo, 0.6 * hi, size=(case.n_runs, model.n_dof))      # (well inside the limits: no joint-limit round on the first step)
        kw = dict(KW)
        if case.floating:
            kw["floating_base"] = 1
            basegoals = np.tile(np.asarray(base), (case.n_runs, 1)); basegoals[:, :3] += rng.uniform(-0.2, 0.2, size=(case.n_runs, 3))
    rob = oracle.OraRobot(model, grabbed=grabbed)
    radius = np.concatenate([model.arrays()["sphere_radius"]] + [np.asarray(g[3], dtype=np.float64) for g in grabbed])
    _PROBLEMS[case.id] = dict(model=model, rob=rob, base=base, dofvals=np.asarray(dofvals), adofs=adofs, goals=np.ascontiguousarray(goals),
                              basegoals=basegoals, grids=[table["sdf"]], poses=[table["pose"]], radius=radius, kw=kw, grabbed=grabbed)
    return _PROBLEMS[case.id]


def tsr_frame(pr, oracle):
    """(link index, R, t) of the constrained link where the robot stands"""
    li = pr["model"].link_names.index(TSR_LINK)
    R, t, _, _ = pr["rob"].fk(pr["base"], pr["dofvals"])
    return li, R[li], t[li]


def make_run(case, oracle, k):
    pr = problem(case, oracle)
    run = oracle.OraRun(pr["rob"], pr["base"], pr["dofvals"], pr["adofs"], pr["goals"][k], pr["grids"], pr["poses"],
                        oracle.default_params(n_points=case.n_points, **pr["kw"]), basegoal=None if pr["basegoals"] is None else pr["basegoals"][k])
    if case.tsr:
        li, R, t = tsr_frame(pr, oracle)
        assert run.add_contsr(li, [0, 0, 0, 0, 0, 0, 1], oracle.pose_from_dR(t, R), [0, 0, 0, 0, 0, 0, 1], TSR_BW) == 1
    return run


def switches(case, oracle, P, radius, epsilon):
    """over every sphere-waypoint of one run (P [n_points][Sa][3]): how many are within SWITCH of a switch of the field lookup (a cell
    face, a cell centre or the field's box, in cells), of dist = 0 or of dist = epsilon; and how many are inside the field at all"""
    pr = problem(case, oracle)
    L = oracle.lib()
    out = dict(face=0, zero=0, eps=0, in_field=0, in_reach=0, total=0)
    g_point = np.zeros(3)
    for grid, pose in zip(pr["grids"], pr["poses"]):
        inv = np.zeros(7)
        L.ora_kin_pose_invert(oracle.dp(oracle.f64(pose)), oracle.dp(inv))
        sizes = np.array([grid.g.sizes[d] for d in range(3)], dtype=np.float64)
        lengths = np.array([grid.g.lengths[d] for d in range(3)])
        for i in range(P.shape[0]):
            for s in range(P.shape[1]):
                L.ora_kin_pose_compos(oracle.dp(inv), oracle.dp(np.ascontiguousarray(P[i, s])), oracle.dp(g_point))
                gc = g_point / lengths * sizes
                out["total"] += 1
                if ((gc > -1.0) & (gc < sizes + 1.0)).all():
                    out["face"] += int((np.abs(gc - np.round(2.0 * gc) / 2.0) < SWITCH).any())
                err, v = grid.interp(g_point)
                if err:
                    continue
                d = v - radius[s]
                out["in_field"] += 1
                out["in_reach"] += int(d < epsilon)
                out["zero"] += int(abs(d) < SWITCH)
                out["eps"] += int(abs(d - epsilon) < SWITCH)
    return out


_REFERENCES = {}


def reference(case, oracle):
    """the oracle's side, computed once: per run the seed T0, G and AG of one iteration, the costs, the joint-limit rounds of that
    iteration (the reference keeps its workspace in G and AG while it makes them: a case must have none) and the switch counts; for the TSR case h of every row of the seed"""
    if case.id in _REFERENCES:
        return _REFERENCES[case.id]
    pr = problem(case, oracle)
    out = dict(T0=[], G=[], AG=[], trace=[], h=[], counts=[], rounds=[])
    for k in range(case.n_runs):
        run = make_run(case, oracle, k)
        T0 = run.traj().copy()
        P = run.eval_obstacle()[2].copy()
        out["counts"].append(switches(case, oracle, P, pr["radius"][run.sphere_order()[:run.Sa]], float(oracle.default_params(**pr["kw"]).epsilon)))
        if case.tsr:
            out["h"].append(np.array([run.eval_contsr(0, T0[i])[0] for i in range(case.n_points)]))
        st, _, tr = run.iterate(1, trace=True)
        assert st == 0
        # (the reference's final cost-only pass rescales the stale G by 1/m once more: tests/test_gpu_parity.py)
        out["G"].append(run.mat("G", run.m, run.n) * run.m); out["AG"].append(run.mat("AG", run.m, run.n).copy())
        out["T0"].append(T0); out["trace"].append(tr[0].copy()); out["rounds"].append(int(run.chomp().last_num_limadjs))
        run.destroy()
    for key in ("T0", "G", "AG", "trace"):
        out[key] = np.array(out[key])
    _REFERENCES[case.id] = out
    return out


def setup_product(case, mod, oracle):
    """the case's robot and the tabletop on the product module; returns the robot's name"""
    from or_cdchomp_amd import scenes
    if case.robot == "wam":
        return (common.setup_product_wam_held4(mod)[0] if case.held else common.setup_product_wam(mod)).name
    pr = problem(case, oracle)
    mod.add_robot(pr["model"], transform=pr["base"], dof_values=pr["dofvals"], active_dofs=pr["adofs"])
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    return pr["model"].name
