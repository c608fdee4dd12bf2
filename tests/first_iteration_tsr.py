"""One CONSTRAINED iteration from a bent trajectory: the cases of the TSR step (csrc/tsr.h phase_tsr), the form of the step each must
run, the oracle's side, and the exact solve of the step (no GPU).

Shared by tests/test_host_first_iteration_tsr.py (the conditions on the inputs, the solvers, the form function's table) and
tests/test_gpu_first_iteration_tsr.py (the device against the oracle and against the exact solve of its own inputs).  The rules for
the inputs are first_iteration's: the straight seed plus bend() bumps, rounded to float for both sides in fp32, a run's bumps drawn
again until the oracle makes no joint-limit round and T1 stays STEP_MARGIN inside the limits.  A constraint's frame is its end
effector's pose at the start configuration.  NOTES/first-iteration.md has the case table and the figures.

The step (oracle/ora_chomp.c:358-408): h' = h - 1/lambda J AG_i per constrained point, (J A^-1 J^T) x = h', and
T1 - T0 = -AG/lambda - A^-1 J^T x.  As a KKT system: A delta - J^T x = 0, J delta = h'."""
import collections
import fractions

import numpy as np

import common
import first_iteration as fi
from or_cdchomp_amd import robots

TsrCase = collections.namedtuple("TsrCase", "id robot n_points precision kw env amp seed n_runs cons form exact")
Con = collections.namedtuple("Con", "kind link tool Bw")      # kind: "con" (`con_tsr 'all ...'`), "everyn" (`everyn_tsr`), "start" (`start_tsr`)

ZERO = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
ARM_TOOL = (0.0, 0.0, 0.16, 0.0, 0.0, 0.0, 1.0)              # the WAM's manipulator "arm": handbase, 0.16 m along the arm
LEFT_TOOL = (0.0, 0.0, 0.15, 0.0, 0.0, 0.0, 1.0)             # the tree's "left": the tip of L13
FREE, FIX = [-3.0, 3.0], [0.0, 0.0]
LIN = [-1.0, 1.0]
BW = {                                                        # enforced rows of x y z roll pitch yaw
    "z": [LIN, LIN, FIX, FREE, FREE, FREE],
    "x": [FIX, LIN, LIN, FREE, FREE, FREE],
    "xyz": [FIX, FIX, FIX, FREE, FREE, FREE],
    "z-roll-pitch": [LIN, LIN, FIX, FIX, FIX, FREE],
    "yz-roll": [LIN, FIX, FIX, FIX, FREE, FREE],
    "yz-roll-pitch": [LIN, FIX, FIX, FIX, FIX, FREE],
    "all6": [FIX] * 6,
}
WAM_KW = fi.WAM_KW
CHAIN_KW = dict(lambda_=200.0, obs_factor=100.0)
TREE_KW = fi.TREE_KW
EXACT_MAX_M = 14             # the rational solve is kept to this many moving waypoints (a few seconds per case at most)

# what Module.batch_tsr_plan must say (csrc/tsr_form.h)
F16_2A = dict(width=16, regs=2, aug=1)
F16_3 = dict(width=16, regs=3, aug=0)
F16_4 = dict(width=16, regs=4, aug=0)
MEET2 = dict(meet=2, subst=(8, 1))
MEET4 = dict(meet=4, subst=(16, 4))
MEET0 = dict(meet=0, subst=(0, 1))
THOMAS = dict(structured=1, width=0)
DENSE = dict(structured=0, width=-1)


def _case(id, robot, m, cons, form, precision=64, env=(), amp=0.2, seed=1, n_runs=4, n_points=None, **kw):
    n_points = m + 2 if n_points is None else n_points
    m = n_points - 2 + (1 if any(c.kind == "start" for c in cons) else 0)
    exact = precision == 64 and m <= EXACT_MAX_M
    return TsrCase(id, robot, n_points, precision, tuple(sorted(kw.items())), tuple(env), amp, seed, n_runs, tuple(cons), form, exact)


def _wam(rows):
    return Con("con", "wam7", ZERO, rows)


W3 = [_wam("z-roll-pitch")]
DENSE_ENV = (("ORC_TSR_DENSE", "1"),)
CASES = [_case("wam-k3-m%d" % m, "wam", m, W3, dict(F16_3, **MEET2), **WAM_KW) for m in (4, 5, 10, 32)]
CASES += [
    _case("wam-k1-m3", "wam", 3, [_wam("z")], dict(THOMAS, n_max=8), **WAM_KW),
    _case("wam-k3-m3", "wam", 3, W3, DENSE, **WAM_KW),              # (the block of 10 rows does not fit the tile buffer of three waypoints)
    _case("wam-k1-m5", "wam", 5, [_wam("z")], dict(F16_2A, **MEET2), **WAM_KW),
    _case("wam-k1-m10", "wam", 10, [_wam("z")], dict(F16_2A, **MEET2), **WAM_KW),
    _case("wam-everyn-k1-con-k1-m10", "wam", 10, [Con("everyn", "handbase", ARM_TOOL, "z"), Con("con", "wam4", ZERO, "x")],
          dict(F16_3, n_max=9, **MEET2), **WAM_KW),
    _case("wam-k6-m10", "wam", 10, [_wam("all6")], dict(F16_4, n_max=13, **MEET2), n_runs=2, **WAM_KW),      # (K = 60: 2 s per exact solve)
    _case("floating-k1-m14", "floating", 14, [_wam("z")], dict(F16_4, n_max=15, **MEET4), floating_base=1, **WAM_KW),
    _case("wam-start-k3-p10", "wam", None, [Con("start", "handbase", ARM_TOOL, "xyz")], dict(F16_3, n_max=10, **MEET2), n_points=10, **WAM_KW),
    _case("wam-start-k3-con-k3-p10", "wam", None, [Con("start", "handbase", ARM_TOOL, "xyz"), _wam("yz-roll")],
          dict(F16_4, n_max=13, **MEET2), n_points=10, **WAM_KW),
    _case("chain13-k3-m10", "chain13", 10, [Con("con", "l12", ZERO, "yz-roll")], dict(width=32, regs=8, n_max=16, **MEET4), **CHAIN_KW),
    _case("chain17-k3-m10", "chain17", 10, [Con("con", "l16", ZERO, "yz-roll")], dict(width=32, regs=10, n_max=20, **MEET0), **CHAIN_KW),
    _case("chain21-k3-m11", "chain21", 11, [Con("con", "l20", ZERO, "yz-roll")], dict(width=32, regs=12, n_max=24, **MEET0), **CHAIN_KW),
    _case("chain22-k3-m12", "chain22", 12, [Con("con", "l21", ZERO, "yz-roll")], dict(THOMAS, n_max=25), **CHAIN_KW),
    _case("chain24-k1-m11", "chain24", 11, [Con("con", "l23", ZERO, "z")], dict(THOMAS, n_max=25), **CHAIN_KW),
    _case("chain30-k3-m18", "chain30", 18, [Con("con", "l29", ZERO, "yz-roll")], dict(THOMAS, n_max=33), **CHAIN_KW),      # Wd = 64
    _case("chain30-k4-m18", "chain30", 18, [Con("con", "l29", ZERO, "yz-roll-pitch")], DENSE, **CHAIN_KW),                # Wd = 65
    _case("tree30-k3-m18", "tree30", 18, [Con("con", "L13", LEFT_TOOL, "xyz")], DENSE, amp=0.4, **TREE_KW),                # (Wd = 64, but two tiles: no room)
    _case("wam-k3-m10-dense", "wam", 10, W3, DENSE, env=DENSE_ENV, **WAM_KW),
    _case("wam-k3-m10-derivative2", "wam", 10, W3, DENSE, n_runs=2, derivative=2, **WAM_KW),                  # (1.2 s per exact solve)
    _case("wam-k3-m32-global", "wam", 32, W3, dict(F16_3, **MEET2), env=(("ORC_T_LDS", "0"), ("ORC_G_LDS", "0")), **WAM_KW),
    _case("wam-k3-m10-momentum", "wam", 10, W3, dict(F16_3, **MEET2), use_momentum=1, **WAM_KW),
    _case("wam-k3-m5-fp32", "wam", 5, W3, dict(F16_3, **MEET2), 32, **WAM_KW),
    _case("wam-k3-m32-fp32", "wam", 32, W3, dict(F16_3, **MEET2), 32, **WAM_KW),
    _case("chain13-k3-m10-fp32", "chain13", 10, [Con("con", "l12", ZERO, "yz-roll")], dict(width=32, regs=8, n_max=16, **MEET4), 32, **CHAIN_KW),
    _case("wam-k3-m10-dense-fp32", "wam", 10, W3, DENSE, 32, env=DENSE_ENV, **WAM_KW),
]
BY_ID = {c.id: c for c in CASES}
EXACT_CASES = [c for c in CASES if c.exact]
# the two builds of the step on the same inputs: (structured, dense by choice)
TWINS = [("wam-k3-m10", "wam-k3-m10-dense")]


def n_rows(con):
    return sum(1 for lo, hi in BW[con.Bw] if lo == 0.0 and hi == 0.0)


def free_start(case):
    return any(c.kind == "start" for c in case.cons)


def moving(case):
    """the rows of the trajectory that are variables"""
    return slice(0, case.n_points - 1) if free_start(case) else slice(1, case.n_points - 1)


# ---- the problems ----------------------------------------------------------------------------------------------------
def chain(n_dof):
    """tests/test_gpu_tsr.py's chain of n_dof revolute joints"""
    from test_gpu_tsr import _chain
    return _chain(n_dof)


# the chain rises through the table top: every piece of the obstacle cost is populated (spheres inside, within epsilon, beyond it
# and outside the field: 58 / 83 / 56 / 427 sphere-waypoints of chain13's four runs).  At tests/test_gpu_tsr.py's base, z 0.9, the
# chain is outside the field, and standing ON the table (z 0.58) no sphere is inside or beyond epsilon and the cost is carried by
# the lowest links' spheres, which hardly move: their velocity is a difference of two nearly equal positions
CHAIN_BASE = [0.3, 0.0, 0.34, 0.0, 0.0, 0.0, 1.0]
GOAL_SPREAD = 0.25           # of the WAM's goals around its start configuration, per joint
_PROBLEMS = {}


def problem(robot, oracle):
    """first_iteration.problem's dict, for the chains too"""
    if robot in _PROBLEMS:
        return _PROBLEMS[robot]
    if robot.startswith("chain"):
        n_dof = int(robot[5:])
        model = chain(n_dof)
        rng = np.random.default_rng(100 + n_dof)
        dofvals = 0.4 * rng.uniform(-1, 1, size=n_dof)
        goals = np.ascontiguousarray(dofvals[None, :] + 0.25 * rng.uniform(-1, 1, size=(4, n_dof)))
        table = common.tabletop_problem(oracle)
        pr = dict(model=model, rob=oracle.OraRobot(model), base=CHAIN_BASE, dofvals=dofvals, adofs=list(range(n_dof)), goals=goals, basegoals=None,
                  grids=[table["sdf"]], poses=[table["pose"]], radius=model.arrays()["sphere_radius"], grabbed=[])
    else:
        # first_iteration's scene; goals near the start configuration, as tests/test_gpu_tsr.py draws them: a constraint held at the
        # start's frame and a goal across the workspace make a first step that leaves the joint limits whatever the bumps are
        pr = dict(fi.problem(robot, oracle))
        rng = np.random.default_rng(3)
        if robot == "tree30":
            pr["goals"] = rng.uniform(-0.4, 0.4, size=(4, pr["model"].n_dof))
        else:
            pr["goals"] = np.array(robots.WAM_START)[None, :] + GOAL_SPREAD * rng.uniform(-1, 1, size=(4, 7))
        if robot == "floating":
            pr["basegoals"] = np.tile(np.asarray(pr["base"], dtype=np.float64), (4, 1))
            pr["basegoals"][:, :3] += rng.uniform(-0.1, 0.1, size=(4, 3))
    _PROBLEMS[robot] = pr
    return pr


def setup_product(robot, mod):
    """the same scene on the product module; returns the robot's name"""
    if robot.startswith("chain"):
        from or_cdchomp_amd import scenes
        n_dof = int(robot[5:])
        model = chain(n_dof)
        rng = np.random.default_rng(100 + n_dof)
        mod.add_robot(model, transform=CHAIN_BASE, dof_values=0.4 * rng.uniform(-1, 1, size=n_dof), active_dofs=list(range(n_dof)))
        scenes.add_tabletop(mod)
        mod.SendCommand("computedistancefield kinbody table")
        return model.name
    name = fi.setup_product(robot, mod)
    if robot == "tree30":
        mod.add_manipulator(name, "left", robots.tree30().link_names.index("L13"), list(LEFT_TOOL))
    return name


def frame(con, pr):
    """the end effector's pose at the start configuration: (link index, rotation, translation)"""
    model = pr["model"]
    li = model.link_names.index(con.link)
    dofvals = np.asarray(pr["dofvals"], dtype=np.float64)
    R, t, _, _ = pr["rob"].fk(pr["base"], dofvals)
    assert tuple(con.tool[3:]) == (0.0, 0.0, 0.0, 1.0)
    return li, R[li], t[li] + R[li] @ np.asarray(con.tool[:3])


def tsr_of(con, pr):
    _, R, d = frame(con, pr)
    return robots.Tsr(T0w_R=R, T0w_d=d, Bw=BW[con.Bw])


def _contsr_args(con, pr, oracle):
    li, R, d = frame(con, pr)
    return li, list(con.tool), oracle.pose_from_dR(d, R), list(ZERO), BW[con.Bw]


def make_run(case, oracle, k, evaluator=False):
    """the oracle's run k with its constraints in the product's order (`everyn_tsr` first, then the `con_tsr`s); evaluator: the start
    point's constraint as an ordinary one, so that eval_contsr reaches every constraint of the case (in the case's order)"""
    pr = problem(case.robot, oracle)
    start = [c for c in case.cons if c.kind == "start"]
    more = {}
    if start and not evaluator:
        more["start_tsr"] = _contsr_args(start[0], pr, oracle)
    run = oracle.OraRun(pr["rob"], pr["base"], pr["dofvals"], pr["adofs"], pr["goals"][k], pr["grids"], pr["poses"],
                        oracle.default_params(**fi.oracle_kw(case), **more), basegoal=None if pr["basegoals"] is None else pr["basegoals"][k])
    order = list(case.cons) if evaluator else [c for c in case.cons if c.kind == "everyn"] + [c for c in case.cons if c.kind == "con"]
    for con in order:
        assert run.add_contsr(*_contsr_args(con, pr, oracle)) == n_rows(con)
    return run


def create_command(case, name, goals, basegoals, pr):
    """`createbatch ...` as the reference's python layer issues it; goals (and basegoals) must outlive the call"""
    kw = dict(case.kw)
    cmd = "createbatch robot %s n_runs %d adofgoals 0x%x n_points %d lambda %r obs_factor %r" % (
        name, case.n_runs, goals.ctypes.data, case.n_points, kw.pop("lambda_"), kw.pop("obs_factor"))
    if basegoals is not None:
        cmd += " basegoals 0x%x" % basegoals.ctypes.data
    for flag in ("floating_base", "use_momentum"):
        if kw.pop(flag, 0):
            cmd += " " + flag
    for key in ("derivative", "obs_factor_self", "epsilon_self"):
        if key in kw:
            cmd += " %s %r" % (key, kw.pop(key))
    assert not kw, kw
    if case.precision == 32:
        cmd += " precision 32"
    for con in case.cons:
        tsr = tsr_of(con, pr).serialize()
        if con.kind == "everyn":
            cmd += " everyn_tsr '%s'" % tsr
        elif con.kind == "start":
            cmd += " start_tsr '%s'" % tsr
        else:
            manip = [mp for mp in (("arm", "handbase", ARM_TOOL), ("left", "L13", LEFT_TOOL)) if mp[1] == con.link and mp[2] == con.tool]
            cmd += " con_tsr '%s' '%s'" % ("all manipee %s" % manip[0][0] if manip else "all link %s" % con.link, tsr)
    return cmd


def blocks_of(case, eval_hJ):
    """the (constraint, point) blocks of the system: [(point i of 0..m-1, h [k], J [k][n])]; eval_hJ(constraint index, trajectory row)"""
    m = case.n_points - 2 + (1 if free_start(case) else 0)
    row0 = 0 if free_start(case) else 1
    out = []
    for c, con in enumerate(case.cons):
        for i in ([0] if con.kind == "start" else range(m)):
            h, J = eval_hJ(c, i + row0)
            out.append((i, np.asarray(h, dtype=np.float64), np.asarray(J, dtype=np.float64)))
    return out


# ---- the step, three times: rational, long double, double ----------------------------------------------------------------
def exact_step(A, D, blocks, AG, lam):
    """T1 - T0 of the moving rows in rational arithmetic from doubles taken exactly: the metric A [m][m] (band D), the blocks' h and J,
    AG [m][n] and lambda.  The Schur form: A^-1 by exact_band_solve on the identity, then the K x K system (J A^-1 J^T) x = h' by
    elimination with the first nonzero pivot.  Returns (step [m][n] rounded to double, the fractions delta [m][n], x [K] and h' [K])"""
    F = fractions.Fraction
    A = np.asarray(A, dtype=np.float64)
    m = A.shape[0]
    n = AG.shape[1]
    Ainv = fi.exact_band_solve(A, np.eye(m), D, rounded=False)
    il = 1 / F(float(lam))
    AGf = [[F(float(v)) for v in row] for row in AG]
    Jf = [[[F(float(v)) for v in row] for row in J] for _, _, J in blocks]
    rows = []                # (block, row of the block)
    hp = []
    for b, (i, h, J) in enumerate(blocks):
        for a in range(len(h)):
            rows.append((b, a))
            hp.append(F(float(h[a])) - il * sum(Jf[b][a][q] * AGf[i][q] for q in range(n)))
    K = len(rows)
    JJ = {}
    M = [[None] * K for _ in range(K)]
    for r, (b1, a1) in enumerate(rows):
        for c in range(r, K):
            b2, a2 = rows[c]
            key = (b1, a1, b2, a2)
            if key not in JJ:
                JJ[key] = sum(u * v for u, v in zip(Jf[b1][a1], Jf[b2][a2]))
            M[r][c] = Ainv[blocks[b1][0]][blocks[b2][0]] * JJ[key]
            M[c][r] = Ainv[blocks[b2][0]][blocks[b1][0]] * JJ[key]
    x = solve_fractions(M, hp)
    delta = [[F(0)] * n for _ in range(m)]
    for b, (i, h, J) in enumerate(blocks):
        base = rows.index((b, 0))
        v = [sum(Jf[b][a][q] * x[base + a] for a in range(len(h))) for q in range(n)]
        for r in range(m):
            w = Ainv[r][i]
            if w != 0:
                for q in range(n):
                    delta[r][q] += w * v[q]
    step = np.array([[float(-il * AGf[r][q] - delta[r][q]) for q in range(n)] for r in range(m)])
    return step, delta, x, hp


def solve_fractions(M, rhs):
    """M x = rhs for fractions.Fraction entries, exactly.  The rows are brought to integers over one common denominator and
    eliminated without fractions (Bareiss: every division is exact, no gcd is taken), which is some twenty times faster than
    eliminating the fractions themselves; the back substitution returns fractions"""
    import math
    F = fractions.Fraction
    K = len(rhs)
    rows = [list(row) + [rhs[r]] for r, row in enumerate(M)]
    den = math.lcm(*[v.denominator for row in rows for v in row])
    U = [[int(v * den) for v in row] for row in rows]
    prev = 1
    for c in range(K - 1):
        p = next(r for r in range(c, K) if U[r][c] != 0)
        U[c], U[p] = U[p], U[c]
        Uc = U[c]
        piv = Uc[c]
        for r in range(c + 1, K):
            Ur = U[r]
            f = Ur[c]
            U[r] = [0] * (c + 1) + [(piv * Ur[q] - f * Uc[q]) // prev for q in range(c + 1, K + 1)]
        prev = piv
    assert U[K - 1][K - 1] != 0
    x = [None] * K
    for r in range(K - 1, -1, -1):
        acc = F(U[r][K])
        for q in range(r + 1, K):
            acc -= U[r][q] * x[q]
        x[r] = acc / U[r][r]
    return x


def float_step(Ainv, blocks, AG, lam, dtype=np.float64):
    """the same step in floating point of `dtype` (np.longdouble: 64 bits of mantissa on x86, the reference where the rational solve is
    too slow) from an inverse metric of that type.  Returns (step [m][n], delta [m][n], cond of J A^-1 J^T in double)"""
    Ainv = np.asarray(Ainv, dtype=dtype)
    AG = np.asarray(AG, dtype=dtype)
    lam = dtype(lam)
    J = [np.asarray(b[2], dtype=dtype) for b in blocks]
    hp = np.concatenate([np.asarray(h, dtype=dtype) - (Jb @ AG[i]) / lam for (i, h, _), Jb in zip(blocks, J)])
    pts = np.concatenate([[i] * len(h) for i, h, _ in blocks]).astype(int)
    Jall = np.vstack(J)
    M = Ainv[np.ix_(pts, pts)] * (Jall @ Jall.T)
    x = solve_pivoting(M, hp)
    delta = np.zeros(AG.shape, dtype=dtype)
    at = 0
    for (i, h, _), Jb in zip(blocks, J):
        delta += np.outer(Ainv[:, i], Jb.T @ x[at:at + len(h)])
        at += len(h)
    return -AG / lam - delta, delta, float(np.linalg.cond(M.astype(np.float64)))


def solve_pivoting(M, rhs):
    """Gaussian elimination with partial pivoting in the arrays' own type (numpy.linalg has no long double)"""
    M = np.array(M); x = np.array(rhs)
    K = len(x)
    for c in range(K):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if p != c:
            M[[c, p]] = M[[p, c]]; x[[c, p]] = x[[p, c]]
        f = M[c + 1:, c] / M[c, c]
        M[c + 1:, c:] -= np.outer(f, M[c, c:])
        x[c + 1:] -= f * x[c]
    for c in range(K - 1, -1, -1):
        x[c] = (x[c] - M[c, c + 1:] @ x[c + 1:]) / M[c, c]
    return x


def invert_longdouble(A):
    """A^-1 in long double: numpy's inverse refined by two Newton steps X (2 I - A X)"""
    A = np.asarray(A, dtype=np.longdouble)
    X = np.linalg.inv(A.astype(np.float64)).astype(np.longdouble)
    eye2 = 2 * np.eye(len(A), dtype=np.longdouble)
    for _ in range(3):
        X = X @ (eye2 - A @ X)
    return X


def normalized(case, T):
    """a floating base's pose columns after an iteration (oracle/ora_run.c:914-916, ora_kin_pose_normalize): the quaternion at unit length"""
    if not dict(case.kw).get("floating_base"):
        return T
    T = np.array(T, dtype=np.float64)
    T[..., 3:7] /= np.sqrt((T[..., 3:7] ** 2).sum(axis=-1))[..., None]
    return T


def reference_step(case, ref, blocks, AG, T0m):
    """T1 - T0 of the moving rows T0m for `blocks` and AG by the best reference the case affords: rational up to EXACT_MAX_M moving
    waypoints, else long double; with a floating base the rows' quaternions are then brought to unit length, as the run does"""
    if case.exact:
        step = exact_step(ref["A"], dict(case.kw).get("derivative", 1), blocks, AG, ref["lambda"])[0]
    else:
        step = float_step(ref["Ainv_ld"], blocks, AG, ref["lambda"], np.longdouble)[0].astype(np.float64)
    return normalized(case, T0m + step) - T0m


# ---- the oracle's side ---------------------------------------------------------------------------------------------------
_REFERENCES = {}


def iterate_once(run, T0):
    """first_iteration._iterate_once with the status returned: a draw whose joint-limit rounds do not end (status -1) is drawn again"""
    run.set_traj(T0)
    st, costs, tr = run.iterate(1, trace=True)
    m, n = run.m, run.n
    return dict(status=st, G=run.mat("G", m, n) * m, AG=run.mat("AG", m, n).copy(), T1=run.traj().copy(), trace=tr[0].copy(),
                rounds=int(run.chomp().last_num_limadjs))


def reference(case, oracle):
    """the oracle's side of a case, computed once: per run T0, G, AG, T1, trace, rounds, the blocks (h, J at the rows of T0), the
    constraint part of the step and its share, cond(J A^-1 J^T), e_ref (the oracle's step against the reference step of its own
    inputs); A, Ainv; for an fp32 case `s` as first_iteration.reference measures it -- with the constraint in place -- and the
    set-aside waypoints"""
    if case.id in _REFERENCES:
        return _REFERENCES[case.id]
    pr = problem(case.robot, oracle)
    prng = np.random.default_rng(2000 + case.seed)
    mv = moving(case)
    out = dict(T0=[], G=[], AG=[], T1=[], trace=[], rounds=[], blocks=[], share=[], cond=[], e_ref=[], h_max=[], draws=[],
               s_AG=[], s_dT=[], s_cost=[])
    runs_P = []
    moved = []
    for k in range(case.n_runs):
        run = make_run(case, oracle, k)
        lower, upper = fi._limits(run)
        seed_traj = run.traj().copy()
        if k == 0:
            out["A"] = run.mat("A", run.m, run.m).copy(); out["Ainv"] = run.mat("Ainv", run.m, run.m).copy()
            out["lambda"] = float(run.chomp().lambda_); out["epsilon"] = float(oracle.default_params(**fi.oracle_kw(case)).epsilon)
            out["Ainv_ld"] = invert_longdouble(out["A"])
            out["m"] = run.m
        run.destroy()
        for attempt in range(fi.MAX_DRAWS):
            T0 = fi.bend(seed_traj, lower, upper, case.amp, np.random.default_rng([case.seed, k, attempt]))
            if free_start(case):
                # the start point is a variable held on the TSR: it is moved off it like any other row (bend() keeps the end rows)
                T0[0] += 0.5 * case.amp * np.random.default_rng([case.seed, k, attempt, 1]).normal(size=T0.shape[1])
                T0[0] = np.minimum(np.maximum(T0[0], lower + fi.CLIP), upper - fi.CLIP)
            if case.precision == 32:
                T0 = T0.astype(np.float32).astype(np.float64)
            prun = make_run(case, oracle, k)
            base = iterate_once(prun, T0)
            prun.destroy()
            if base["status"] == 0 and base["rounds"] == 0 and np.minimum(base["T1"] - lower, upper - base["T1"])[mv].min() > fi.STEP_MARGIN:
                break
        else:
            raise AssertionError("%s run %d: no draw of %d keeps the first step inside the limits" % (case.id, k, fi.MAX_DRAWS))
        out["draws"].append(attempt + 1)
        for key in ("G", "AG", "T1", "trace", "rounds"):
            out[key].append(base[key])
        out["T0"].append(T0)
        ev = make_run(case, oracle, k, evaluator=True)
        blocks = blocks_of(case, lambda c, row: ev.eval_contsr(c, T0[row]))
        if case.precision == 32:
            ev.set_traj(T0)
            P = ev.eval_obstacle()[2].copy()
            runs_P.append((P, pr["radius"][ev.sphere_order()[:ev.Sa]]))
        ev.destroy()
        out["blocks"].append(blocks)
        out["h_max"].append(max(float(np.abs(h).max()) for _, h, _ in blocks))
        step = (base["T1"] - T0)[mv]
        _, delta, cond = float_step(out["Ainv"], blocks, base["AG"], out["lambda"])
        out["share"].append(float(np.linalg.norm(delta) / np.linalg.norm(step)))
        out["cond"].append(cond)
        out["e_ref"].append(common.rel_l2(step, reference_step(case, out, blocks, base["AG"], T0[mv])))
        if case.precision == 32:
            movs = []
            for draw in range(3):
                Tp = T0.copy()
                Tp[mv] *= 1.0 + np.where(prng.uniform(size=Tp[mv].shape) < 0.5, -1.0, 1.0) * 2.0 ** -24
                prun = make_run(case, oracle, k)
                movs.append((iterate_once(prun, Tp), Tp))
                prun.destroy()
            moved.append(movs)
    for key in ("T0", "G", "AG", "T1", "trace"):
        out[key] = np.array(out[key])
    out["aside"] = np.zeros((case.n_runs, out["m"]), dtype=bool)
    if case.precision == 32:
        out["counts"], out["aside"], out["delta"] = fi._inputs_report(case, oracle, pr, runs_P, out["epsilon"])
        for k in range(case.n_runs):
            sAG = sdT = sc = 0.0
            for mvd, Tp in moved[k]:
                sAG = max(sAG, fi.row_err(mvd["AG"], out["AG"][k]))
                sdT = max(sdT, fi.row_err((mvd["T1"] - Tp)[mv], (out["T1"][k] - out["T0"][k])[mv]))
                sc = max(sc, float(np.abs(mvd["trace"] / out["trace"][k] - 1.0).max()))
            out["s_AG"].append(sAG); out["s_dT"].append(sdT); out["s_cost"].append(sc)
    _REFERENCES[case.id] = out
    return out


# ---- the form function's domain ------------------------------------------------------------------------------------------
def form_expected(BLOCK, m, n, Nm):
    """the rule of csrc/tsr_form.h written down a second time, from the issue's description of phase_tsr: (width, regs, aug, meet,
    subst_w, subst_u).  The host test holds orc_host_tsr_form to it over the whole domain"""
    k = Nm - n
    if BLOCK < 128 or m < 4 or n > 23 or Nm > 24 or k > 16:
        return (0, 0, 0, 0, 0, 0)
    if Nm <= 15:
        width = 16
        regs, aug = (2, int(Nm + n + 1 <= 16)) if Nm <= 8 else (3, 0) if Nm <= 12 else (4, 0)
    else:
        width, aug = 32, 0
        regs = 8 if Nm <= 16 else 10 if Nm <= 20 else 12
    meet = (2, 8, 1) if n <= 7 else (4, 16, 4) if n <= 15 else (0, 0, 1)
    return (width, regs, aug) + meet
