"""-m gpu: ONE constrained iteration against the oracle and against an exact solve, from bent trajectories, held near rounding, in
every form the TSR step takes (csrc/tsr.h phase_tsr: the register eliminations in rows of 16 and 32 lanes, their three meets and
substitutions, the one-wavefront LDS form, the dense step) -- and the form that ran is asserted (Module.batch_tsr_plan).

tests/test_gpu_tsr.py runs 4 to 40 iterations at 1e-6; a step that is wrong at 1e-9 passes all of it.  Here fp64 is held to 1e-10
against the oracle, fp32 to 16 s with s the oracle's own movement under 2^-24 changes of the waypoints, the constraint in place; and
the solve alone -- the device's own h, J and AG through a rational solve of the KKT system -- to max(1e-10, 4 e_ref).  The cases,
their inputs and the references are tests/first_iteration_tsr.py's; tests/test_host_first_iteration_tsr.py checks them;
NOTES/first-iteration.md has the figures."""
import numpy as np
import pytest

import common
import first_iteration as fi
import first_iteration_tsr as ft
import or_cdchomp_amd
from test_gpu_first_iteration import _hold, _hold_costs, _s

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def products():
    """one module per robot, made when a case first asks for it"""
    mods = {}

    def get(robot):
        if robot not in mods:
            mod = or_cdchomp_amd.Module(0)
            mods[robot] = (mod, ft.setup_product(robot, mod))
        return mods[robot]
    yield get
    for mod, _ in mods.values():
        mod.close()


@pytest.fixture(scope="module")
def device_results():
    return {}


def _end_effector(con):
    """how batch_config_tsr addresses a constraint's end effector: the head of its `con_tsr '...'`"""
    if con.kind != "con":
        return {}                                                  # the active manipulator
    if tuple(con.tool) == ft.ZERO:
        return dict(link=con.link)
    return dict(manip={"handbase": "arm", "L13": "left"}[con.link])


def _device(products, device_results, monkeypatch, oracle, case, switch):
    """one iteration of the case's batch on the device from the oracle's bent trajectories, created through the command layer; with
    `switch` under ORC_DEBUG_STATE=1.  For a case with an exact comparison also the device's h and J at the rows of T0
    (batch_config_tsr).  Run once per module."""
    key = (case.id, switch)
    if key in device_results:
        return device_results[key]
    ref = ft.reference(case, oracle)
    pr = ft.problem(case.robot, oracle)
    mod, name = products(case.robot)
    goals = np.ascontiguousarray(pr["goals"][:case.n_runs], dtype=np.float64)
    basegoals = None if pr["basegoals"] is None else np.ascontiguousarray(pr["basegoals"][:case.n_runs], dtype=np.float64)
    with monkeypatch.context() as mp:
        for var, value in case.env:
            mp.setenv(var, value)
        if switch:
            mp.setenv("ORC_DEBUG_STATE", "1")
        else:
            mp.delenv("ORC_DEBUG_STATE", raising=False)
        bid = int(mod.SendCommand(ft.create_command(case, name, goals, basegoals, pr)))
    mod.batch_set_traj(bid, ref["T0"])
    assert np.array_equal(mod.batch_gettraj(bid), ref["T0"])
    costs, status = mod.batch_iterate(bid, 1)
    out = dict(status=status, AG=mod.batch_state(bid, "AG"), T1=mod.batch_gettraj(bid), trace=mod.batch_trace(bid, 1)[:, 0],
               tsr_plan=mod.batch_tsr_plan(bid), plan=mod.batch_plan(bid), G=mod.batch_state(bid, "G") if switch else None)
    if case.exact and not switch:
        rows = ref["T0"].reshape(-1, ref["T0"].shape[2])
        out["hJ"] = [mod.batch_config_tsr(bid, ft.tsr_of(con, pr), rows, **_end_effector(con)) for con in case.cons]
    mod.batch_destroy(bid)
    device_results[key] = out
    return out


def _assert_form(case, dev):
    plan = dev["tsr_plan"]
    want = dict(structured=1)
    want.update(case.form)
    got = {key: plan[key] for key in want}
    print("%s: %d threads, tsr_plan %s" % (case.id, dev["plan"]["threads"], plan))
    assert got == want, (case.id, plan)
    assert plan["n_tsrs"] == len(case.cons) and plan["cons_k"] == sum(len(h) for _, h, _ in ft.blocks_of(case, lambda c, row: (np.zeros(ft.n_rows(case.cons[c])), None)))


def _oracle_update(case, ref, with_switch, k):
    """the oracle's AG and T1 - T0 (moving rows) of run k; in fp32 with the set-aside rows of its G replaced by the device's own, as
    part B of tests/test_gpu_first_iteration.py does it: A^-1 spreads such a row over AG, and AG enters the constraint step twice"""
    mv = ft.moving(case)
    AG, dT = ref["AG"][k], (ref["T1"][k] - ref["T0"][k])[mv]
    if case.precision == 32 and ref["aside"][k].any():
        dG = np.zeros_like(ref["G"][k])
        dG[ref["aside"][k]] = (with_switch["G"][k] - ref["G"][k])[ref["aside"][k]]
        AG2 = AG + ref["Ainv"] @ dG
        dT = dT + ft.float_step(ref["Ainv"], ref["blocks"][k], AG2, ref["lambda"])[0] - ft.float_step(ref["Ainv"], ref["blocks"][k], AG, ref["lambda"])[0]
        AG = AG2
    return AG, dT


@pytest.mark.parametrize("case", ft.CASES, ids=lambda c: c.id)
def test_constrained_step_against_the_oracle(products, device_results, monkeypatch, oracle, case):
    """AG, T1 - T0 and the costs as the product's own path leaves them (ORC_DEBUG_STATE unset) against the oracle's add_contsr /
    start_tsr, set_traj and iterate(1); the form that ran; the rows that are no variables bit-equal to T0; and bit for bit what the
    batch under the switch gives.

    (wam-k3-m32-fp32 found the float rounding of the smoothness gradient's row, which A^-1 passed on to AG at 56 s; smooth_grad now
    forms the row in double: NOTES/first-iteration.md, "Found: the fp32 smoothness gradient".)"""
    ref = ft.reference(case, oracle)
    with_switch = _device(products, device_results, monkeypatch, oracle, case, True)
    dev = _device(products, device_results, monkeypatch, oracle, case, False)
    assert (dev["status"] == 0).all()
    _assert_form(case, dev)
    mv = ft.moving(case)
    fixed = [-1] if ft.free_start(case) else [0, -1]
    for k in range(case.n_runs):
        AG, dT = _oracle_update(case, ref, with_switch, k)
        if case.precision == 32:      # (not held here: part A of tests/test_gpu_first_iteration.py holds G; a row that stands out says where an AG comes from)
            rows = np.linalg.norm(with_switch["G"][k] - ref["G"][k], axis=-1) / np.linalg.norm(ref["G"][k], axis=-1).max()
            spread = fi.row_err(ref["AG"][k] + ref["Ainv"] @ (with_switch["G"][k] - ref["G"][k]), dev["AG"][k])
            print("%s G run %d: largest row error %.2e at row %d; the device's AG against A^-1 of its own G: %.2e" % (case.id, k, rows.max(), rows.argmax(), spread))
        _hold("AG", case, k, dev["AG"][k], AG, _s(ref, "s_AG", k))
        _hold("T1 - T0", case, k, (dev["T1"][k] - ref["T0"][k])[mv], dT, _s(ref, "s_dT", k), stored=dev["T1"][k][mv])
        assert np.array_equal(dev["T1"][k][fixed], ref["T0"][k][fixed])
        if case.precision == 64 or not ref["aside"][k].any():
            _hold_costs(case, k, dev["trace"][k], ref["trace"][k], _s(ref, "s_cost", k))
    assert np.array_equal(dev["T1"], with_switch["T1"])
    assert np.array_equal(dev["AG"], with_switch["AG"])
    assert np.array_equal(dev["trace"], with_switch["trace"])
    assert dev["tsr_plan"] == with_switch["tsr_plan"]


def _exact_comparison(case, ref, dev):
    """(largest error of the device's step against the exact step of its own h, J and AG, the bound)"""
    mv = ft.moving(case)
    n_rows_T = ref["T0"].shape[1]
    errs = []
    for k in range(case.n_runs):
        def hJ(c, row):
            rec, kk = dev["hJ"][c], ft.n_rows(case.cons[c])
            return rec["h"][k * n_rows_T + row][:kk], rec["jac"][k * n_rows_T + row][:kk]
        blocks = ft.blocks_of(case, hJ)
        want = ft.reference_step(case, ref, blocks, dev["AG"][k], ref["T0"][k][mv])
        errs.append(common.rel_l2((dev["T1"][k] - ref["T0"][k])[mv], want))
    return max(errs), max(fi.FP64_TOL, 4.0 * max(ref["e_ref"]))


@pytest.mark.parametrize("case", ft.EXACT_CASES, ids=lambda c: c.id)
def test_constrained_step_against_the_exact_solve(products, device_results, monkeypatch, oracle, case):
    """the solve and the move alone: the device's T1 - T0 against the rational solution of A delta - J^T x = 0, J delta = h' with the
    device's own h and J at the rows of T0 (batch_config_tsr), its own AG and the oracle's A; expected -AG/lambda - delta.  Held to
    max(1e-10, 4 e_ref), e_ref the oracle's own step against the exact step of its own inputs (part C's rule)"""
    ref = ft.reference(case, oracle)
    dev = _device(products, device_results, monkeypatch, oracle, case, False)
    assert (dev["status"] == 0).all()
    _assert_form(case, dev)
    e_dev, tol = _exact_comparison(case, ref, dev)
    print("%s: device step vs exact %.2e, the oracle's %.2e, bound %.2e, cond(J A^-1 J^T) %.1e" % (case.id, e_dev, max(ref["e_ref"]), tol, max(ref["cond"])))
    assert e_dev <= tol, (case.id, e_dev, ref["e_ref"])


@pytest.mark.parametrize("structured,dense", ft.TWINS)
def test_structured_and_dense_steps_agree(products, device_results, monkeypatch, oracle, structured, dense):
    """the two builds of the step from the same trajectories: each is held to the exact solve above; they agree within twice its bound"""
    a, b = ft.BY_ID[structured], ft.BY_ID[dense]
    ra, rb = ft.reference(a, oracle), ft.reference(b, oracle)
    assert np.array_equal(ra["T0"], rb["T0"])
    da = _device(products, device_results, monkeypatch, oracle, a, False)
    db = _device(products, device_results, monkeypatch, oracle, b, False)
    assert da["tsr_plan"]["width"] > 0 and db["tsr_plan"]["width"] == -1
    tol = 2.0 * max(fi.FP64_TOL, 4.0 * max(ra["e_ref"]), 4.0 * max(rb["e_ref"]))
    mv = ft.moving(a)
    for k in range(a.n_runs):
        err = common.rel_l2((da["T1"][k] - ra["T0"][k])[mv], (db["T1"][k] - rb["T0"][k])[mv])
        print("%s / %s run %d: %.2e" % (structured, dense, k, err))
        assert err <= tol, (k, err)
    assert np.array_equal(da["AG"], db["AG"])
