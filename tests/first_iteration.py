"""One iteration from a bent trajectory: the cases, their inputs and the oracle's side of the comparison (no GPU).

Shared by tests/test_host_first_iteration.py (the conditions on the inputs, on the oracle alone) and
tests/test_gpu_first_iteration.py (the device against the oracle).  NOTES/first-iteration.md has the case table and the
measured figures.

A case's trajectories are the straight-line seed plus seeded smooth bumps amp/k N(0,1) sin(k pi s), k = 1..3, per column,
the moving rows clipped 0.02 inside the joint limits; an fp32 case rounds them to float, for the oracle too.  A run's bumps are
drawn again until the oracle's first step makes no joint-limit round (reference())."""
import collections
import fractions

import numpy as np

import common
from or_cdchomp_amd import robots

Case = collections.namedtuple("Case", "id robot n_points precision kw env amp seed n_runs")

WAM_KW = dict(lambda_=100.0, obs_factor=500.0)
TREE_KW = dict(lambda_=400.0, obs_factor=50.0, obs_factor_self=40.0, epsilon_self=0.08)
CLIP = 0.02              # the moving rows stay this far inside the joint limits: no joint-limit round is made
NEAR = 0.08              # a sphere within epsilon + NEAR of an obstacle counts for the set-aside rule
FP32_MARGIN = 16.0       # the kernel rounds at every step of a chain, the experiment behind `s` once at its head (not derived)
FP64_TOL = 1e-10
MAX_DRAWS = 64           # of a run's bumps, until the first step stays inside the limits
STEP_MARGIN = 1e-3       # ... by this much, so that the fp32 step stays inside as well


def _case(id, robot, n_points, precision=64, env=(), amp=0.4, seed=1, n_runs=8, **kw):
    return Case(id, robot, n_points, precision, tuple(sorted(kw.items())), tuple(env), amp, seed, n_runs)


# ---- parts A and B: the cost families -------------------------------------------------------------------------------
COST_CASES = [_case("chain16-p%d-fp%d" % (p, prec), "wam", p, prec, **WAM_KW)
              for p, prec in ((7, 64), (34, 64), (100, 64), (101, 64), (7, 32), (34, 32))]
COST_CASES += [
    _case("chain16-general-p34-fp64", "wam_mug", 34, **WAM_KW),
    _case("tree16-p34-fp64", "wam_fingers", 34, n_runs=6, lambda_=100.0, obs_factor=300.0),
    _case("pairs-chain-p34-fp64", "held4", 34, **WAM_KW),
    _case("pairs-chain-p34-fp32", "held4", 34, 32, **WAM_KW),
    _case("pairs-tree-p34-fp64", "held4_fingers", 34, **WAM_KW),
    _case("pairs-tree-p34-fp32", "held4_fingers", 34, 32, **WAM_KW),
    _case("many-p20-fp64", "tree30", 20, n_runs=4, amp=0.25, **TREE_KW),
    _case("many-p20-fp32", "tree30", 20, 32, n_runs=4, amp=0.25, **TREE_KW),
    _case("floating-p34-fp64", "floating", 34, n_runs=4, use_momentum=1, floating_base=1, **WAM_KW),
    _case("chain16-global-p34-fp64", "wam", 34, env=(("ORC_T_LDS", "0"), ("ORC_G_LDS", "0")), **WAM_KW),
]

# ---- part C: the metric solves (WAM, 4 runs) ------------------------------------------------------------------------
SEMISEP_MIN_M = lambda D: 2 * D + 2          # build_semisep refuses m < 2 D + 2 (csrc/host_math.cpp): the dense inverse below
SOLVE_CASES = [_case("scan-p%d" % p, "wam", p, n_runs=4, **WAM_KW) for p in (66, 67, 258, 259)]
SOLVE_CASES += [_case("pcr-p%d" % p, "wam", p, n_runs=4, env=(("ORC_NO_SCAN_SOLVE", "1"),), **WAM_KW) for p in (34, 67)]
for _D in (2, 3, 4):
    _pts = [100, 66, 67] + ([130] if _D == 2 else []) + [SEMISEP_MIN_M(_D) + 2, SEMISEP_MIN_M(_D) + 1]
    SOLVE_CASES += [_case("band%d-p%d" % (_D, p), "wam", p, n_runs=4, derivative=_D, **WAM_KW) for p in _pts]
SOLVE_CASES += [_case("band2-p34-fp32", "wam", 34, 32, n_runs=4, derivative=2, **WAM_KW)]
LEAN_CASES = SOLVE_CASES[:4]                 # the scan solve without the switch: the lean update path

ALL_CASES = COST_CASES + SOLVE_CASES


def solve_mode_expected(case):
    """what `plan` must say: 2 the Toeplitz scans, 0 cyclic reduction, 3 the band generators, 1 the dense inverse"""
    kw = dict(case.kw)
    D = kw.get("derivative", 1)
    if D == 1:
        return 0 if ("ORC_NO_SCAN_SOLVE", "1") in case.env else 2
    return 3 if case.n_points - 2 >= SEMISEP_MIN_M(D) else 1


# ---- the problems: what the oracle needs, built without a GPU ----------------------------------------------------------
def _finger_goals(n_runs, seed):
    arm = common.wam_goals(n_runs, seed=seed)
    fingers = np.random.default_rng(seed + 7).uniform(0.2, 2.2, size=(n_runs, 3))
    return np.ascontiguousarray(np.hstack([arm, fingers]))


def box_field(oracle, name, aabb_padding):
    """a tabletop body's field as `computedistancefield kinbody <name> aabb_padding ...` builds it (common.tabletop_problem's recipe)"""
    from or_cdchomp_amd import scenes
    boxes = scenes.tabletop_boxes()
    bpose, bhalf = boxes[name][0]
    lo = [bpose[i] - bhalf[i] for i in range(3)]
    hi = [bpose[i] + bhalf[i] for i in range(3)]
    apos = [0.5 * (lo[i] + hi[i]) for i in range(3)]
    aext = [hi[i] - apos[i] for i in range(3)]
    sizes, lengths, pose = common.grid_dims(apos, aext, 0.02, aabb_padding)
    world = [(b[0][:3], b[1]) for nm in boxes for b in boxes[nm]]
    occ = common.voxelize_axis_aligned(sizes, lengths, pose[:3], world, 0.02)
    g = oracle.OraGrid(occ, lengths)
    g.flood_fill(0)
    g.data[g.data == 1.0] = common.HUGE
    return g.bin_sdf(), pose


_PROBLEMS = {}


def problem(robot, oracle):
    """dict(model, rob, base, dofvals, adofs, goals, basegoals, grids, poses, radius [S])"""
    if robot in _PROBLEMS:
        return _PROBLEMS[robot]
    grabbed = []
    basegoals = None
    if robot == "tree30":
        model = robots.tree30()
        base = [0.0] * 6 + [1.0]
        dofvals = np.zeros(model.n_dof)
        adofs = list(range(model.n_dof))
        _, grids, poses = common.config5_oracle_fields(oracle, 0.02, 0.15)
        goals = np.random.default_rng(7).uniform(-0.4, 0.4, size=(4, model.n_dof))
        goals[:, 2:5] = [0.9, 1.2, -0.6]; goals[:, 16:19] = [-0.9, 1.2, 0.6]       # both arms swing in front of the torso
    else:
        model, base, dofvals, adofs = common.wam_state()
        table = common.tabletop_problem(oracle)
        grids, poses = [table["sdf"]], [table["pose"]]
        goals = common.wam_goals(8, seed=11)
        if robot == "wam_mug":
            mug, mpose = box_field(oracle, "mug", 0.15)
            grids.append(mug); poses.append(mpose)
        if robot in ("held4", "held4_fingers"):
            grabbed = [(model.link_names.index("handbase"), common.held4_pose(model), common.HELD4_POS, common.HELD4_RAD)]
        if robot == "held4_fingers":
            adofs = list(range(10))
            goals = _finger_goals(8, 11)
        if robot == "wam_fingers":
            adofs = list(range(10))
            lo = np.asarray(model.limit_lower[:10]) + 0.1
            hi = np.asarray(model.limit_upper[:10]) - 0.1
            goals = np.random.default_rng(77).uniform(lo, hi, size=(6, 10))
        if robot == "floating":
            goals, basegoals, _, _ = common.config4_problem(4)
    rob = oracle.OraRobot(model, grabbed=grabbed)
    radius = np.concatenate([model.arrays()["sphere_radius"]] + [np.asarray(g[3], dtype=np.float64) for g in grabbed])
    _PROBLEMS[robot] = dict(model=model, rob=rob, base=base, dofvals=dofvals, adofs=adofs, goals=np.asarray(goals),
                            basegoals=basegoals, grids=grids, poses=poses, radius=radius, grabbed=grabbed)
    return _PROBLEMS[robot]


def setup_product(robot, mod):
    """the same scene on the product module; returns the robot's name"""
    if robot == "tree30":
        return common.setup_product_tree30(mod, 0.02, 0.15).name
    if robot in ("held4", "held4_fingers"):
        model = common.setup_product_wam_held4(mod)[0]
    else:
        model = common.setup_product_wam(mod)
    if robot == "wam_mug":
        mod.SendCommand("computedistancefield kinbody mug aabb_padding 0.15")
    if robot in ("held4_fingers", "wam_fingers"):
        mod.set_active_dofs(model.name, list(range(10)))
    return model.name


def oracle_kw(case, **more):
    kw = dict(case.kw, n_points=case.n_points, **more)
    if "derivative" in kw:
        kw["D"] = kw.pop("derivative")
    return kw


def make_run(case, oracle, k, **more):
    pr = problem(case.robot, oracle)
    return oracle.OraRun(pr["rob"], pr["base"], pr["dofvals"], pr["adofs"], pr["goals"][k], pr["grids"], pr["poses"],
                         oracle.default_params(**oracle_kw(case, **more)),
                         basegoal=None if pr["basegoals"] is None else pr["basegoals"][k])


def bend(seed_traj, lower, upper, amp, rng):
    """the straight line plus amp/k N(0,1) sin(k pi s), k = 1..3, per column; moving rows clipped CLIP inside the limits, end rows kept"""
    n_points, n = seed_traj.shape
    s = np.linspace(0.0, 1.0, n_points)
    out = seed_traj.copy()
    z = rng.normal(size=(3, n))
    for k in (1, 2, 3):
        out += (amp / k) * np.sin(k * np.pi * s)[:, None] * z[k - 1][None, :]
    out[1:-1] = np.minimum(np.maximum(out[1:-1], lower + CLIP), upper - CLIP)
    out[0] = seed_traj[0]; out[-1] = seed_traj[-1]
    return out


def _limits(run):
    c = run.chomp()
    return (np.ctypeslib.as_array(c.jlimit_lower, shape=(run.n,)).copy(), np.ctypeslib.as_array(c.jlimit_upper, shape=(run.n,)).copy())


def _iterate_once(run, T0):
    run.set_traj(T0)
    st, costs, tr = run.iterate(1, trace=True)
    assert st == 0
    m, n = run.m, run.n
    # the reference's final cost-only pass rescales the stale G by 1/m once more (tests/test_gpu_parity.py): G x m is the
    # gradient the solve saw
    return dict(G=run.mat("G", m, n) * m, AG=run.mat("AG", m, n).copy(), T1=run.traj().copy(), trace=tr[0].copy(),
                rounds=int(run.chomp().last_num_limadjs))


def row_err(a, b):
    """the largest movement of a row over the largest row norm"""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b, axis=-1).max() / max(np.linalg.norm(b, axis=-1).max(), 1e-300))


def joints_on_chain(pr, floating):
    """the longest chain of optimized joints between the base and a sphere (the floating base counts as one)"""
    a = pr["model"].arrays()
    best = 0
    for li in set(int(l) for l in a["sphere_link"]):
        cnt = 0
        while li >= 0:
            cnt += int(a["joint_type"][li] != 0 and int(a["dof_index"][li]) in pr["adofs"])
            li = int(a["parent"][li])
        best = max(best, cnt)
    return best + (1 if floating else 0)


def delta_cells(case, pr, reach):
    """how close (in cells) a sphere centre may come to a switch of the field lookup before its waypoint is set aside: the centre's
    rounding error -- joints on the chain x unit roundoff x reach -- in cells, times 8.  fp64 keeps 1e-9 where the formula gives
    less (2e-13 for the WAM): the wider band only asks more of the inputs."""
    u = 2.0 ** -24 if case.precision == 32 else 2.0 ** -53
    cell = min(float(g.g.lengths[i]) / g.g.sizes[i] for g in pr["grids"] for i in range(3))
    d = 8.0 * joints_on_chain(pr, bool(dict(case.kw).get("floating_base"))) * u * reach / cell
    return d if case.precision == 32 else max(d, 1e-9)


def _inputs_report(case, oracle, pr, runs_P, epsilon):
    """branch counts over every sphere-waypoint and the set-aside waypoints [n_runs][m]"""
    L = oracle.lib()
    inv = []
    for pose in pr["poses"]:
        out = np.zeros(7)
        L.ora_kin_pose_invert(oracle.dp(oracle.f64(pose)), oracle.dp(out))
        inv.append(out)
    reach = max(float(np.linalg.norm(P - np.asarray(pr["base"][:3]), axis=-1).max()) for P, _ in runs_P)
    delta = delta_cells(case, pr, reach)
    counts = dict(inside=0, near=0, far=0, outside=0)
    aside = []
    g_point = np.zeros(3)
    for P, rad in runs_P:
        n_points, Sa, _ = P.shape
        mask = np.zeros(n_points, dtype=bool)
        for i in range(n_points):
            for s in range(Sa):
                best = np.inf
                found = False
                flag = False
                pos = np.ascontiguousarray(P[i, s])
                for f, grid in enumerate(pr["grids"]):
                    L.ora_kin_pose_compos(oracle.dp(inv[f]), oracle.dp(pos), oracle.dp(g_point))
                    sizes = np.array([grid.g.sizes[d] for d in range(3)], dtype=np.float64)
                    gc = g_point / np.array([grid.g.lengths[d] for d in range(3)]) * sizes
                    err, v = grid.interp(g_point)
                    on_face = bool(((gc > -delta) & (gc < sizes + delta)).all() and ((np.abs(gc) < delta) | (np.abs(gc - sizes) < delta)).any())
                    if err:
                        flag |= on_face
                        continue
                    found = True
                    best = min(best, v)
                    if v - rad[s] < epsilon + NEAR:
                        flag |= on_face or bool((np.abs(gc - np.round(2.0 * gc) / 2.0) < delta).any())
                mask[i] |= flag
                d = best - rad[s]
                counts["outside" if not found else "inside" if d < 0 else "near" if d < epsilon else "far"] += 1
        aside.append(mask[1:-1])
    return counts, np.array(aside), delta


_REFERENCES = {}


def reference(case, oracle):
    """the oracle's side of a case, computed once: per run T0, G, AG, T1, trace and A, Ainv; the conditions on the inputs; for an
    fp32 case `s`, the largest movement of the oracle's rows under relative +-2^-24 changes of the moving waypoints"""
    if case.id in _REFERENCES:
        return _REFERENCES[case.id]
    pr = problem(case.robot, oracle)
    prng = np.random.default_rng(1000 + case.seed)
    out = dict(T0=[], G=[], AG=[], T1=[], trace=[], rounds=[], G_noself=[], max_acc=[], s_G=[], s_AG=[], s_dT=[], s_cost=[])
    runs_P = []
    for k in range(case.n_runs):
        run = make_run(case, oracle, k)
        lower, upper = _limits(run)
        seed_traj = run.traj().copy()
        for attempt in range(MAX_DRAWS):
            # a draw whose first step leaves the limits (a row clipped to CLIP inside them moves out easily) is drawn again: the
            # joint-limit rounds are not this comparison's business, on either side
            T0 = bend(seed_traj, lower, upper, case.amp, np.random.default_rng([case.seed, k, attempt]))
            if case.precision == 32:
                T0 = T0.astype(np.float32).astype(np.float64)
            prun = make_run(case, oracle, k)
            probe = _iterate_once(prun, T0)
            prun.destroy()
            if probe["rounds"] == 0 and np.minimum(probe["T1"] - lower, upper - probe["T1"])[1:-1].min() > STEP_MARGIN:
                break
        else:
            raise AssertionError("%s run %d: no draw of %d keeps the first step inside the limits" % (case.id, k, MAX_DRAWS))
        run.destroy()
        run = make_run(case, oracle, k)
        run.set_traj(T0)
        P = run.eval_obstacle()[2].copy()
        runs_P.append((P, pr["radius"][run.sphere_order()[:run.Sa]]))
        out["max_acc"].append(float(np.abs(P[2:] - 2.0 * P[1:-1] + P[:-2]).max()))
        if k == 0:
            out["A"] = run.mat("A", run.m, run.m).copy(); out["Ainv"] = run.mat("Ainv", run.m, run.m).copy()
            out["lambda"] = float(run.chomp().lambda_); out["epsilon"] = float(oracle.default_params(**oracle_kw(case)).epsilon)
        base = _iterate_once(run, T0)
        run.destroy()
        for key in ("G", "AG", "T1", "trace", "rounds"):
            out[key].append(base[key])
        out["T0"].append(T0)
        noself = make_run(case, oracle, k, obs_factor_self=0.0)
        out["G_noself"].append(_iterate_once(noself, T0)["G"])
        noself.destroy()
        if case.precision == 32:
            movs = []
            for draw in range(3):
                Tp = T0.copy()
                Tp[1:-1] *= 1.0 + np.where(prng.uniform(size=Tp[1:-1].shape) < 0.5, -1.0, 1.0) * 2.0 ** -24
                prun = make_run(case, oracle, k)
                movs.append((_iterate_once(prun, Tp), Tp))
                prun.destroy()
            out.setdefault("_moved", []).append(movs)
    counts, aside, delta = _inputs_report(case, oracle, pr, runs_P, out["epsilon"])
    out["counts"] = counts; out["aside"] = aside; out["delta"] = delta
    for k in range(case.n_runs):
        if case.precision != 32:
            continue
        keep = ~aside[k]
        sG = sAG = sdT = sc = 0.0
        for moved, Tp in out["_moved"][k]:
            sG = max(sG, float(np.linalg.norm((moved["G"] - out["G"][k])[keep], axis=-1).max() / np.linalg.norm(out["G"][k], axis=-1).max()))
            sAG = max(sAG, row_err(moved["AG"], out["AG"][k]))
            sdT = max(sdT, row_err((moved["T1"] - Tp)[1:-1], (out["T1"][k] - out["T0"][k])[1:-1]))
            sc = max(sc, float(np.abs(moved["trace"] / out["trace"][k] - 1.0).max()))
        out["s_G"].append(sG); out["s_AG"].append(sAG); out["s_dT"].append(sdT); out["s_cost"].append(sc)
    out.pop("_moved", None)
    for key in ("T0", "G", "AG", "T1", "trace", "G_noself"):
        out[key] = np.array(out[key])
    out["self_share"] = float((np.abs(out["G"] - out["G_noself"]).max(axis=-1) > 0).mean())
    _REFERENCES[case.id] = out
    return out


# ---- the exact solve --------------------------------------------------------------------------------------------------
def exact_band_solve(A, G, D, rounded=True):
    """A x = G in rational arithmetic: band elimination without pivoting (A symmetric positive definite, zero outside D
    diagonals either side) on fractions.Fraction; A [m][m] and G [m][cols] doubles, taken exactly.  Returns x rounded to double (or the fractions themselves)."""
    F = fractions.Fraction
    A = np.asarray(A, dtype=np.float64); G = np.asarray(G, dtype=np.float64)
    m = A.shape[0]
    off = np.abs(np.subtract.outer(np.arange(m), np.arange(m))) > D
    assert not A[off].any(), "the metric has entries outside its band"
    cols = G.shape[1]
    rows = [[F(float(A[i, j])) if j < m else F(0) for j in range(i, i + D + 1)] for i in range(m)]      # rows[i][q] = A[i][i+q], the upper band
    x = [[F(float(v)) for v in G[i]] for i in range(m)]
    for k in range(m):
        piv = rows[k][0]
        assert piv > 0
        for q in range(1, min(D, m - 1 - k) + 1):          # row i = k + q; by symmetry of the reduced matrix A[i][k] = rows[k][q]
            f = rows[k][q] / piv
            if f == 0:
                continue
            ri, rk, xi, xk = rows[k + q], rows[k], x[k + q], x[k]
            for p in range(q, D + 1):                       # column j = k + p >= i
                ri[p - q] -= f * rk[p]
            for c in range(cols):
                xi[c] -= f * xk[c]
    for k in range(m - 1, -1, -1):
        rk, xk = rows[k], x[k]
        for c in range(cols):
            acc = xk[c]
            for q in range(1, min(D, m - 1 - k) + 1):
                acc -= rk[q] * x[k + q][c]
            xk[c] = acc / rk[0]
    return np.array([[float(v) for v in row] for row in x]) if rounded else x
