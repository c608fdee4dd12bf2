"""-m gpu: ONE iteration of every kernel family against the oracle, from bent trajectories, held near rounding.

The other GPU comparisons run tens of iterations and allow for what an optimizer amplifies (1e-6 in fp64, 1e-3 in fp32).  One
iteration from a controlled trajectory has nothing to amplify: the gradient G of every cost family (part A), what the product's own
update path leaves -- A^-1 G, the step, the costs, without the debug switch (part B) -- and the metric solves against an exact rational
solve of the device's own gradient (part C).  The cases, their inputs and the oracle's side are tests/first_iteration.py's;
tests/test_host_first_iteration.py checks the inputs; NOTES/first-iteration.md has the figures.

fp64 is held to 1e-10 relative L2 per run.  fp32 is held, row by row, to 16 s of the largest row, with s the movement of the ORACLE's
rows under relative 2^-24 changes of the waypoints (the input's own conditioning, three draws), and to the 1e-3 bar as well; the
waypoints next to a switch of the field lookup (first_iteration.reference()["aside"]) are set aside in fp32, none exist in fp64."""
import numpy as np
import pytest

import common
import first_iteration as fi
import or_cdchomp_amd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def products():
    """one module per scene, made when a case first asks for it"""
    mods = {}

    def get(robot):
        if robot not in mods:
            mod = or_cdchomp_amd.Module(0)
            mods[robot] = (mod, fi.setup_product(robot, mod))
        return mods[robot]
    yield get
    for mod, _ in mods.values():
        mod.close()


@pytest.fixture(scope="module")
def device_results():
    return {}


def _device(products, device_results, monkeypatch, oracle, case, switch):
    """one iteration of the case's batch on the device from the oracle's bent trajectories; with `switch` under ORC_DEBUG_STATE=1 (G
    readable, the general update path), without it the product's path.  Run once per module."""
    key = (case.id, switch)
    if key in device_results:
        return device_results[key]
    ref = fi.reference(case, oracle)
    pr = fi.problem(case.robot, oracle)
    mod, name = products(case.robot)
    with monkeypatch.context() as mp:
        for var, value in case.env:
            mp.setenv(var, value)
        if switch:
            mp.setenv("ORC_DEBUG_STATE", "1")
        else:
            mp.delenv("ORC_DEBUG_STATE", raising=False)
        extra = dict(precision=32) if case.precision == 32 else {}
        bid = mod.batch_create(name, pr["goals"][:case.n_runs], basegoals=None if pr["basegoals"] is None else pr["basegoals"][:case.n_runs],
                               n_points=case.n_points, **dict(case.kw), **extra)
    mod.batch_set_traj(bid, ref["T0"])
    assert np.array_equal(mod.batch_gettraj(bid), ref["T0"])
    costs, status = mod.batch_iterate(bid, 1)
    out = dict(status=status, AG=mod.batch_state(bid, "AG"), T1=mod.batch_gettraj(bid), trace=mod.batch_trace(bid, 1)[:, 0],
               plan=mod.batch_plan(bid), G=mod.batch_state(bid, "G") if switch else None)
    mod.batch_destroy(bid)
    device_results[key] = out
    return out


def _hold(what, case, k, got, want, s, keep=None, stored=None):
    """fp64: relative L2 of the run below 1e-10.  fp32: every kept row within 16 s of the largest row, and the kept rows within 1e-3.
    stored [rows][n]: the float values the rows were formed from by a subtraction in the test (T1 of T1 - T0): their storage rounding,
    2^-24 |value| per entry, is no error of the kernel and is allowed on top, row by row"""
    got = np.asarray(got, dtype=np.float64); want = np.asarray(want, dtype=np.float64)
    if case.precision == 64:
        err = common.rel_l2(got, want)
        print("%s %s run %d: rel L2 %.2e" % (case.id, what, k, err))
        assert err < fi.FP64_TOL, (what, case.id, k, err)
        return
    keep = np.ones(len(want), dtype=bool) if keep is None else keep
    top = np.linalg.norm(want, axis=-1).max()
    rows = np.linalg.norm(got - want, axis=-1)
    if stored is not None:
        rows = np.maximum(rows - np.linalg.norm(2.0 ** -24 * np.abs(stored), axis=-1), 0.0)
    err = float(rows[keep].max() / top)
    print("%s %s run %d: row error %.2e, s %.2e, err / s %.2f (%d rows set aside)" % (case.id, what, k, err, s, err / s, (~keep).sum()))
    assert err <= fi.FP32_MARGIN * s, (what, case.id, k, err, s, err / s)
    assert common.rel_l2(got[keep], want[keep]) <= 1e-3, (what, case.id, k)


def _hold_costs(case, k, got, want, s):
    rel = float(np.abs(got / want - 1.0).max())
    print("%s costs run %d: %.2e%s" % (case.id, k, rel, "" if case.precision == 64 else ", s %.2e, err / s %.2f" % (s, rel / s)))
    if case.precision == 64:
        assert np.allclose(got, want, rtol=1e-9, atol=0), (case.id, k, got, want)
    else:
        assert rel <= fi.FP32_MARGIN * s, (case.id, k, got, want, rel / s)


def _s(ref, key, k):
    return ref[key][k] if ref[key] else None


# ---- part A: the cost phase ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fi.COST_CASES, ids=lambda c: c.id)
def test_first_gradient(products, device_results, monkeypatch, oracle, case):
    """G of one iteration, per run, and the iteration's costs.  (Under the switch the update phase writes G out after G/m + A T + B on
    every path, whatever n and with TSR rows: chomp_kernel.hip phase_update_body.)"""
    ref = fi.reference(case, oracle)
    dev = _device(products, device_results, monkeypatch, oracle, case, True)
    assert (dev["status"] == 0).all()
    for k in range(case.n_runs):
        _hold("G", case, k, dev["G"][k], ref["G"][k], _s(ref, "s_G", k), ~ref["aside"][k])
        if case.precision == 64 or not ref["aside"][k].any():      # (the value jumps at a lookup switch as the gradient does)
            _hold_costs(case, k, dev["trace"][k], ref["trace"][k], _s(ref, "s_cost", k))


# ---- part B: the product's update path -------------------------------------------------------------------------------------
def _update_reference(ref, dev_switch, case, k):
    """the oracle's AG and T1 - T0 of run k; in fp32, with the set-aside rows of its G replaced by the device's own (a row next to a
    lookup switch may differ at order one, and A^-1 spreads it over every row of AG)"""
    AG = ref["AG"][k]
    if case.precision == 32 and ref["aside"][k].any():
        dG = np.zeros_like(ref["G"][k])
        dG[ref["aside"][k]] = (dev_switch["G"][k] - ref["G"][k])[ref["aside"][k]]
        AG = AG + ref["Ainv"] @ dG
    return AG, -AG / ref["lambda"]


@pytest.mark.parametrize("case", fi.COST_CASES, ids=lambda c: c.id)
def test_update_path_of_the_product(products, device_results, monkeypatch, oracle, case):
    """AG, T1 - T0 and the costs as the product's own update path leaves them (ORC_DEBUG_STATE unset: phase_update_costs<lean> where the
    plan allows it) against the oracle, and bit for bit what the batch under the switch gave: the switch changes only what is readable"""
    ref = fi.reference(case, oracle)
    with_switch = _device(products, device_results, monkeypatch, oracle, case, True)
    dev = _device(products, device_results, monkeypatch, oracle, case, False)
    assert (dev["status"] == 0).all()
    momentum = bool(dict(case.kw).get("use_momentum"))
    for k in range(case.n_runs):
        AG, dT = _update_reference(ref, with_switch, case, k)
        if momentum:
            AG, dT = ref["AG"][k], (ref["T1"][k] - ref["T0"][k])[1:-1]      # (AG is the momentum: 0.5 / lambda A^-1 G after the first step)
        _hold("AG", case, k, dev["AG"][k], AG, _s(ref, "s_AG", k))
        _hold("T1 - T0", case, k, (dev["T1"][k] - ref["T0"][k])[1:-1], dT, _s(ref, "s_dT", k), stored=dev["T1"][k][1:-1])
        assert np.array_equal(dev["T1"][k][[0, -1]], ref["T0"][k][[0, -1]])
        if case.precision == 64 or not ref["aside"][k].any():
            _hold_costs(case, k, dev["trace"][k], ref["trace"][k], _s(ref, "s_cost", k))
    assert np.array_equal(dev["T1"], with_switch["T1"])
    assert np.array_equal(dev["AG"], with_switch["AG"])
    assert np.array_equal(dev["trace"], with_switch["trace"])


# ---- part C: the metric solves ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fi.SOLVE_CASES, ids=lambda c: c.id)
def test_metric_solve_against_exact(products, device_results, monkeypatch, oracle, case):
    """the device's AG against the exact rational solution of A x = G_dev, the device's own gradient: the solve alone.  Held to
    max(1e-10, 4 e_ref) with e_ref the oracle's own AG against the exact solution of its own G (both are within cond(A) eps of it,
    DESIGN.md 4; 4 is the margin between two elimination orders).  fp32: 16 x 2^-24, AG is stored as float while the sums and scans
    run in double."""
    ref = fi.reference(case, oracle)
    dev = _device(products, device_results, monkeypatch, oracle, case, True)
    assert (dev["status"] == 0).all()
    D = dict(case.kw).get("derivative", 1)
    assert dev["plan"]["solve_mode"] == fi.solve_mode_expected(case), dev["plan"]
    n = ref["G"].shape[2]
    rhs = np.hstack([dev["G"][k] for k in range(case.n_runs)] + [ref["G"][k] for k in range(case.n_runs)])
    x = fi.exact_band_solve(ref["A"], rhs, D)
    e_ref = max(common.rel_l2(ref["AG"][k], x[:, (case.n_runs + k) * n:(case.n_runs + k + 1) * n]) for k in range(case.n_runs))
    e_dev = max(common.rel_l2(dev["AG"][k], x[:, k * n:(k + 1) * n]) for k in range(case.n_runs))
    tol = 16.0 * 2.0 ** -24 if case.precision == 32 else max(1e-10, 4.0 * e_ref)
    print("%s: device AG vs exact %.2e, the oracle's %.2e, bound %.2e, cond(A) %.1e" % (case.id, e_dev, e_ref, tol, np.linalg.cond(ref["A"])))
    assert e_dev <= tol, (case.id, e_dev, e_ref)
    if case.precision == 64:
        for k in range(case.n_runs):
            _hold("G", case, k, dev["G"][k], ref["G"][k], None)


@pytest.mark.parametrize("case", fi.LEAN_CASES, ids=lambda c: c.id)
def test_lean_scan_solve_equals_the_general_path(products, device_results, monkeypatch, oracle, case):
    """one or two rows per lane, rows in registers or read twice: the lean path's toeplitz_scan_solve leaves the bits of the general path's"""
    with_switch = _device(products, device_results, monkeypatch, oracle, case, True)
    dev = _device(products, device_results, monkeypatch, oracle, case, False)
    assert np.array_equal(dev["AG"], with_switch["AG"])
    assert np.array_equal(dev["T1"], with_switch["T1"])
    assert np.array_equal(dev["trace"], with_switch["trace"])
    ref = fi.reference(case, oracle)
    for k in range(case.n_runs):
        _hold("AG", case, k, dev["AG"][k], ref["AG"][k], None)
