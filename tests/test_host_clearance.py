"""-m "not gpu": the specifications behind orc_batch_clearance and orc_batch_select_clear, without a GPU.  The restatement of
tests/clearance.py -- what the -m gpu tests of test_gpu_clearance.py hold the kernel to -- is itself pinned to the oracle's
re-check; select_clear and clearance_too_long of or_cdchomp_amd.module on hand-made inputs; the two calls' place in the C
ABI; and the premise of the synthetic trajectories of the GPU tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import clearance as CL
import common
from or_cdchomp_amd import _capi, robots
from or_cdchomp_amd.module import clearance_too_long, select_clear, verdict_samples

WAM_VMAX = [0.5, 1.0, 2.0, 1.0, 4.0, 1.0, 0.25]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def wam(oracle):
    prob = common.tabletop_problem(oracle)
    model, base, dofvals, adofs = common.wam_state()
    field = CL.Field(oracle, prob["sdf"], None, prob["pose"])
    return dict(model=model, base=base, dofvals=dofvals, adofs=adofs, field=field, prob=prob,
                tab=CL.Tables(oracle, model, base, dofvals, adofs, [field]))


def twelve_trajectories():
    """straight lines of the WAM: from its start to config 2's goals and into the table; with the arm turned away from the
    table, free ones and ones that fold the forearm onto the shoulder"""
    start = np.asarray(robots.WAM_START)
    back = np.array([-1.0, -1.8, 0.0, 2.0, 0.0, 0.2, 0.0])
    lines = [(start, g) for g in common.wam_goals(3, seed=20250101)]
    lines += [(start, np.asarray(CL.IN_TABLE)), (start, start + 1.6 * (np.asarray(CL.IN_TABLE) - start)),
              (start, start + np.array([0, 0, 0, 0, 0.3, 0.2, 0.3])),
              (back, back + np.array([0.5, 0, 0.3, 0, 1.0, 0, 0.5])), (back, back + np.array([-0.8, 0.3, 0.5, -0.6, -1.0, 0.4, 0.5])),
              (back, back + np.array([0.3, 0, 0, 0.2, 0, 0, 0]))]
    for j3, j2 in ((2.9, 0.0), (3.05, 0.2), (2.7, -0.2)):
        g = back.copy(); g[3] = j3; g[2] = j2
        lines.append((back, g))
    return [CL.line(a, b, 30) for a, b in lines]


def test_restatement_is_the_oracles_recheck(oracle, wam):
    """the first sample with a negative restated gap, in the verdict's order, is OraRun.collision_recheck's contact"""
    n_field = n_self = n_free = 0
    for T in twelve_trajectories():
        run = oracle.OraRun(wam["tab"].robot, wam["base"], wam["dofvals"], wam["adofs"], T[-1], [wam["field"].grid], [wam["field"].pose],
                            oracle.default_params(n_points=len(T)))
        run.set_traj(T)
        want = run.collision_recheck(WAM_VMAX)
        run.destroy()
        res = CL.restate(wam["tab"], T, WAM_VMAX, 0, [wam["field"]])
        got = CL.first_contact(res)
        if not want["collides"]:
            assert got is None and res["clearance"][0] >= 0.0 and res["clearance"][1] >= 0.0
            assert res["n_samples"] == want["samples"]
            n_free += 1
            continue
        assert got is not None
        time, sphere, field, depth = got
        assert np.float64(time).view(np.int64) == np.float64(want["time"]).view(np.int64)
        assert (sphere, field) == (want["sphere"], want["field"])
        assert np.isclose(depth, want["depth"], rtol=1e-9, atol=1e-12), (depth, want["depth"])
        assert min(res["clearance"]) <= -depth
        n_field += field >= 0; n_self += field <= -2
    print("contacts with the field %d, with the robot itself %d, free %d" % (n_field, n_self, n_free))
    assert n_field >= 2 and n_self >= 2 and n_free >= 2, "the twelve must cover the three outcomes"


# ---- select_clear -------------------------------------------------------------------------------------------------------

def test_select_clear_rule():
    inf, nan = np.inf, np.nan
    #                 total obs smooth
    costs = np.array([[5.0, 1.0, 4.0], [5.0, 2.0, 3.0], [3.0, 3.0, -0.0], [3.0, 3.0, 0.0], [1.0, 0.5, 0.5], [1.0, 0.5, 0.5],
                      [nan, 0.0, 0.0], [2.0, 1.0, 1.0], [2.0, 1.0, 1.0], [0.5, 0.1, 0.4]])
    status = np.array([0, 1, 0, 0, 0, -1, 0, 0, 0, 1])
    clear = np.array([[0.02, 0.05], [0.03, 0.01], [0.04, 0.04], [0.04, inf], [nan, nan], [0.5, 0.5], [0.5, 0.5], [0.1, 0.2], [-0.0, 0.3],
                      [nan, nan]])
    ns = np.array([10, 10, 10, 10, -1, 10, 10, 10, 10, -2])
    group = np.array([0, 0, 1, 1, 2, 2, 2, 3, 3, 3])
    # margin 0: run 4 was not walked, 5 left its limits, 6 has no finite cost, 9 is too long; -0 clears a margin of 0
    best, cost, bc, cnt = select_clear(costs, status, clear, ns, group, 5, 0.0, 0)
    assert best.tolist() == [0, 2, -1, 7, -1] and cnt.tolist() == [2, 2, 0, 2, 0]      # ties: the lower run; group 4 is empty
    assert cost.tolist()[:2] == [5.0, 3.0] and cost[2] == inf and cost[4] == inf and cost[3] == 2.0
    assert bc[0] == 0.02 and bc[1] == 0.04 and np.isnan(bc[2]) and bc[3] == 0.1 and np.isnan(bc[4])
    # smooth: -0 ties with +0, the lower run wins, and the cost that comes back is +0
    best, cost, bc, cnt = select_clear(costs, status, clear, ns, group, 5, 0.0, 2)
    assert best.tolist() == [1, 2, -1, 7, -1] and cost[1] == 0.0 and not np.signbit(cost[1]) and bc[0] == 0.01
    # column 3: the largest clearance, cost -clearance; a tie (0.04 and fmin(0.04, inf)) goes to the lower run
    best, cost, bc, cnt = select_clear(costs, status, clear, ns, group, 5, 0.0, 3)
    assert best.tolist() == [0, 2, -1, 7, -1] and cost.tolist()[:2] == [-0.02, -0.04] and cost[3] == -0.1
    # a margin between two clearances of group 0 flips its winner by column 2 and empties nothing else
    best, cost, bc, cnt = select_clear(costs, status, clear, ns, group, 5, 0.015, 2)
    assert best.tolist() == [0, 2, -1, 7, -1] and cnt.tolist() == [1, 2, 0, 1, 0]
    # -inf: every walked candidate (a negative clearance too); +inf: nobody here
    neg = clear.copy(); neg[0] = [-0.3, 0.1]
    best, cost, bc, cnt = select_clear(costs, status, neg, ns, group, 5, -inf, 0)
    assert best.tolist() == [0, 2, -1, 7, -1] and bc[0] == -0.3 and cnt.tolist() == [2, 2, 0, 2, 0]
    best, cost, bc, cnt = select_clear(costs, status, clear, ns, group, 5, inf, 0)
    assert best.tolist() == [-1] * 5 and np.isinf(cost).all() and np.isnan(bc).all() and cnt.tolist() == [0] * 5
    # a NaN clearance of a walked run (it cannot occur; the rule still says): fmin ignores it
    odd = clear.copy(); odd[7] = [nan, 0.2]
    assert select_clear(costs, status, odd, ns, group, 5, 0.15, 0)[0][3] == 7
    for bad in (dict(column=4), dict(margin=nan), dict(n_groups=3)):
        kw = dict(column=0, margin=0.0, n_groups=5); kw.update(bad)
        with pytest.raises(ValueError):
            select_clear(costs, status, clear, ns, group, kw["n_groups"], kw["margin"], kw["column"])


# ---- clearance_too_long -------------------------------------------------------------------------------------------------

def test_too_long_either_side_of_the_cap():
    start = np.asarray(robots.WAM_START)
    turn = start + np.array([0, 0, 0, 0, -4.0, 1.6, 3.2])      # (a set_traj trajectory: the limits do not bind it)
    for cap in (8, 64, 1000):
        for length, want in (((cap - 0.5) * 0.04, False), ((cap + 0.5) * 0.04, True)):
            T = CL.zigzag(start, turn, 12, length)
            assert clearance_too_long(T, WAM_VMAX, 0, cap) is want, (cap, length)
            n = len(verdict_samples(T, WAM_VMAX, 0)[0])
            assert (n <= cap + 2) if not want else (n >= cap), (cap, n)
    still = np.tile(start, (12, 1))
    assert clearance_too_long(still, WAM_VMAX, 0, 1) is False and len(verdict_samples(still, WAM_VMAX, 0)[0]) == 0
    with pytest.raises(ValueError):
        clearance_too_long(still, WAM_VMAX[:3], 0, 8)


def test_a_run_the_rule_passes_has_at_most_cap_plus_two_samples():
    rng = np.random.default_rng(20251019)
    passed = 0
    for k in range(1000):
        n_points = int(rng.integers(2, 9)); n = int(rng.integers(1, 5))
        cap = int(rng.integers(1, 200))
        scale = 10.0 ** rng.uniform(-3, 0.5)
        T = np.cumsum(rng.normal(size=(n_points, n)) * scale, axis=0)
        if rng.random() < 0.2:
            T[int(rng.integers(1, n_points))] = T[0]      # repeated rows: segments of no length
        vmax = rng.uniform(0.1, 4.0, n)
        if not clearance_too_long(T, vmax, 0, cap):
            passed += 1
            assert len(verdict_samples(T, vmax, 0)[0]) <= cap + 2, k
    assert 100 < passed < 900, passed


# ---- the C ABI ------------------------------------------------------------------------------------------------------------

PROTOTYPES = (
    "int orc_batch_clearance(orc_module * mod, int batch_id, int which, const unsigned char * examine, int max_samples,",
    "int orc_batch_select_clear(orc_module * mod, int batch_id, int cost_column, int n_groups, const int * group_of_run,\n"
    "   double margin, int max_samples,\n"
    "   int * best_run_out, double * best_cost_out, double * best_clearance_out, int * n_eligible_out, int * n_samples_out);",
)


def test_symbols_and_null_module():
    header = open(os.path.join(ROOT, "include", "orcdchomp_amd.h")).read()
    for proto in PROTOTYPES:
        assert proto in header, proto
    m = re.search(r"int orc_batch_clearance\((.*?)\);", header, re.S)
    args = re.sub(r"/\*.*?\*/", "", m.group(1))
    assert [a.strip() for a in args.split(",")] == [
        "orc_module * mod", "int batch_id", "int which", "const unsigned char * examine", "int max_samples", "double * clearance_out",
        "double * time_out", "int * sphere_out", "int * other_out", "int * n_samples_out"]
    names = [s[0] for s in _capi.SYMBOLS]
    lib = _capi.lib()
    for name in ("orc_batch_clearance", "orc_batch_select_clear"):
        assert name in names and hasattr(lib, name)
    col = np.full(4, 7, dtype=np.int32)
    want = lib.orc_batch_collision_verdict_device(None, 1, col.ctypes.data_as(_capi.c_int_p), None, None, None, None, None)
    clr = np.full((4, 2), 7.0); ns = np.full(4, 7, dtype=np.int32)
    assert lib.orc_batch_clearance(None, 1, 2, None, 64, clr.ctypes.data_as(_capi.c_double_p), None, None, None,
                                   ns.ctypes.data_as(_capi.c_int_p)) == want
    best = np.full(2, 7, dtype=np.int32)
    assert lib.orc_batch_select_clear(None, 1, 0, 2, None, C.c_double(0.0), 64, best.ctypes.data_as(_capi.c_int_p), None, None, None,
                                      ns.ctypes.data_as(_capi.c_int_p)) == want
    assert (clr == 7.0).all() and (ns == 7).all() and (best == 7).all(), "a NULL module writes nothing"


# ---- the premise of the synthetic GPU inputs ------------------------------------------------------------------------------

def test_synthetic_runs_keep_their_premises(wam):
    """what the chunk-edge test of test_gpu_clearance.py relies on: the sample counts, where the minima sit, and that the face
    premise sets no run aside"""
    runs = CL.synthetic_runs(robots.WAM_START)
    assert runs.shape == (len(CL.SYNTH_NAMES), CL.SYNTH_POINTS, 7)
    res = {nm: CL.restate(wam["tab"], T, WAM_VMAX, 0, [wam["field"]]) for nm, T in zip(CL.SYNTH_NAMES, runs)}
    for nm, r in res.items():
        assert not CL.set_aside(r, [wam["field"]]), nm
    sample_of = lambda r: int(r["fkey"][np.flatnonzero(r["fgap"] == r["clearance"][0])[0], 0])
    assert 0 < res["short"]["n_samples"] < CL.CHUNK
    assert 2 * CL.CHUNK < res["zigzag"]["n_samples"] < 3 * CL.CHUNK
    assert res["chunk multiple"]["n_samples"] == 2 * CL.CHUNK
    assert sample_of(res["min at sample 0"]) == 0 and res["min at sample 0"]["n_samples"] > 1
    last = res["min at last sample"]
    assert sample_of(last) == last["n_samples"] - 1 and last["n_samples"] > CL.CHUNK and last["n_samples"] % CL.CHUNK
    assert res["zero length"]["n_samples"] == 0 and np.isinf(res["zero length"]["clearance"]).all()
    assert np.array_equal(runs[6], runs[7])
    for nm in ("penetrates", "through and out"):
        r = res[nm]
        fc = CL.first_contact(r)
        assert r["clearance"][0] < 0.0 and fc is not None and r["time"][0] > fc[0] and -r["clearance"][0] > fc[3], nm
