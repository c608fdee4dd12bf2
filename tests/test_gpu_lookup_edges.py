"""-m gpu: every device form of the field lookup against the oracle AT its ties: cell faces, half-cell planes, the border layers,
x == length, one ulp outside, +inf in the cell or in a used or an unused neighbour, equal values in two fields.

The inputs lie on a dyadic lattice (tests/lookup_edges.py), so every quantity a decision hangs on is exact in fp64 and in fp32: no
waypoint is set aside, in either precision.  Part A asks the clearance and penetration calls (sdf_lookup) about single rows and
wants equality; part B runs one iteration of every form the iterate kernel looks fields up in -- each case names the variant bits
it expects of the planner and asserts them --; part C takes the many-sphere pass's 24-bit offsets to their limit and beyond.
tests/test_host_lookup_edges.py checks the inputs; NOTES/lookup-edges.md has the case table and the figures."""
import numpy as np
import pytest

import common
import first_iteration as fi
import lookup_edges as LE
import or_cdchomp_amd

pytestmark = pytest.mark.gpu

PEN_TOL = {64: 1e-10, 32: 1e-3}      # tests/test_gpu_penetration.py TOL: relative to the row's largest entry
FP32_ROW_TOL = 1e-3                  # the project's fp32 bar, here per row (LE.fp32_row_errors)


@pytest.fixture(scope="module")
def products():
    """one module per (scene, gantry), made when a case first asks for it"""
    mods = {}

    def get(scene, spheres):
        if (scene, spheres) not in mods:
            mod = or_cdchomp_amd.Module(0)
            mods[(scene, spheres)] = (mod, LE.setup_product(mod, scene, spheres))
        return mods[(scene, spheres)]
    yield get
    for mod, _ in mods.values():
        mod.close()


# ---- part A: single rows, exact -----------------------------------------------------------------------------------------------
def _ask(mod, name, rows, precision):
    """the four calls on `rows`: the two configuration calls, and the two waypoint calls on a batch whose trajectories are the rows"""
    P = LE.PART_A_POINTS
    n_runs = -(-len(rows) // P)
    padded = np.concatenate([rows, np.tile(rows[-1], (n_runs * P - len(rows), 1))]).reshape(n_runs, P, 3)
    bid = mod.batch_create(name, padded[:, -1], n_points=P, precision=precision, **LE.KW)
    out = dict(config_clearance=mod.batch_config_clearance(bid, rows, runs=0),
               config_penetration=mod.batch_config_penetration(bid, rows, runs=0, margin=LE.PART_A_MARGIN))
    mod.batch_set_traj(bid, padded)
    assert np.array_equal(mod.batch_gettraj(bid), padded)
    for key, res in (("waypoint_clearance", mod.batch_waypoint_clearance(bid)),
                     ("waypoint_penetration", mod.batch_waypoint_penetration(bid, margin=LE.PART_A_MARGIN))):
        out[key] = {k: v.reshape((n_runs * P,) + v.shape[2:])[:len(rows)] for k, v in res.items()}
    mod.batch_destroy(bid)
    return out


def _hold_rows(what, ref, got, precision, keep, exact):
    """the field leg: clearance, sphere and field EQUAL on the exact rows (close, with the same keys, on a row one ulp outside one field and
    inside another: no lattice point there); cost and gradient within PEN_TOL of the row's largest entry.  The self leg (the far sphere
    on the base, a square root) to 1e-6."""
    bad = []
    for k in np.flatnonzero(keep):
        same = got["sphere"][k, 0] == ref["sphere"][k, 0] and got["other"][k, 0] == ref["other"][k, 0]
        if exact[k]:
            same = same and got["clearance"][k, 0] == ref["clearance"][k, 0]
        else:
            same = same and abs(got["clearance"][k, 0] - ref["clearance"][k, 0]) <= 2.0 ** -20
        if not same:
            bad.append((ref["names"][k], got["clearance"][k, 0], ref["clearance"][k, 0], got["sphere"][k, 0], ref["sphere"][k, 0],
                        got["other"][k, 0], ref["other"][k, 0]))
    assert not bad, (what, len(bad), bad[:8])
    assert np.allclose(got["clearance"][keep, 1], ref["clearance"][keep, 1], rtol=1e-6, atol=0), what
    if "cost" not in got:
        return 0.0
    worst = 0.0
    for k in np.flatnonzero(keep):
        for key in ("cost", "grad"):
            scale = max(float(np.abs(ref[key][k]).max()), 1e-300)
            err = float(np.abs(got[key][k] - ref[key][k]).max()) / scale
            worst = max(worst, err)
            assert err <= PEN_TOL[precision], (what, ref["names"][k], key, err, got[key][k], ref[key][k])
    return worst


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("scene", ["a", "b", "c", "d"])
def test_single_rows_are_exact(products, oracle, scene, precision):
    """sdf_lookup through config_clearance, waypoint_clearance, config_penetration, waypoint_penetration: every class combination of
    every field, the poison cases, the ties between fields, one ulp outside every bound"""
    ref = LE.part_a_reference(oracle, scene, precision)
    mod, name = products(scene, 1)
    got = _ask(mod, name, ref["rows"], precision)
    rows = ref["rows"]
    exact = np.all(rows == np.round(rows / LE.Q) * LE.Q, axis=1) | np.isinf(ref["clearance"][:, 0])      # on the lattice, or in no field
    for key, res in got.items():
        worst = _hold_rows("%s fp%d %s" % (scene, precision, key), ref, res, precision, ref["asserted"], exact)
        print("scene %s fp%d %s: %d rows equal (%d of them off the lattice, held close)%s" % (
            scene, precision, key, len(rows), (~exact).sum(), "; cost and gradient within %.1e" % worst if "cost" in res else ""))


@pytest.mark.parametrize("precision", [64, 32])
def test_rounded_lengths(products, oracle, precision):
    """scene (e), 6 x 5 x 7 cells: sdf_lookup multiplies by a rounded 1 / length.  Quarter-cell points and a quarter cell either side of
    a bound are asserted; what the device does at the exact faces and at x == length is printed, not asserted"""
    ref = LE.part_a_reference(oracle, "e", precision)
    mod, name = products("e", 1)
    got = _ask(mod, name, ref["rows"], precision)
    exact = np.ones(len(ref["rows"]), dtype=bool)
    for key, res in got.items():
        _hold_rows("e fp%d %s" % (precision, key), ref, res, precision, ref["asserted"], exact)
    res = got["config_clearance"]
    rec = np.flatnonzero(~ref["asserted"])
    differ = [k for k in rec if not (res["clearance"][k, 0] == ref["clearance"][k, 0] and res["other"][k, 0] == ref["other"][k, 0])]
    print("scene e fp%d: %d quarter-cell rows equal; of %d rows on exact faces or bounds %d differ from the oracle" % (
        precision, ref["asserted"].sum(), len(rec), len(differ)))
    for k in differ:
        print("   %s: device %r, oracle %r" % (ref["names"][k], res["clearance"][k, 0], ref["clearance"][k, 0]))


# ---- part B: one iteration of every lookup form ----------------------------------------------------------------------------------
def _iterate(products, monkeypatch, oracle, case):
    """one iteration of the case's batch from the oracle's lattice trajectories under ORC_DEBUG_STATE=1 (G readable)"""
    ref = LE.reference(case, oracle)
    mod, name = products(case.scene, case.spheres)
    with monkeypatch.context() as mp:
        for var, value in case.env:
            mp.setenv(var, value)
        mp.setenv("ORC_DEBUG_STATE", "1")
        extra = dict(precision=32) if case.precision == 32 else {}
        bid = mod.batch_create(name, ref["goals"], n_points=LE.N_POINTS, **LE.KW, **extra)
    mod.batch_set_traj(bid, ref["T0"])
    assert np.array_equal(mod.batch_gettraj(bid), ref["T0"])
    costs, status = mod.batch_iterate(bid, 1)
    out = dict(status=status, G=mod.batch_state(bid, "G"), trace=mod.batch_trace(bid, 1)[:, 0], plan=mod.batch_plan(bid))
    mod.batch_destroy(bid)
    return ref, out


def _hold_iteration(case, ref, dev):
    assert (dev["status"] == 0).all()
    assert np.isfinite(dev["G"]).all(), "a non-finite gradient (a poisoned lookup through a zero scale?)"
    worst = worst_cost = 0.0
    for k in range(LE.N_RUNS):
        cost = float(np.abs(dev["trace"][k] / ref["trace"][k] - 1.0).max())
        worst_cost = max(worst_cost, cost)
        if case.precision == 64:
            err = common.rel_l2(dev["G"][k], ref["G"][k])
            print("%s run %d: G rel L2 %.2e, costs %.2e" % (case.id, k, err, cost))
            assert err < fi.FP64_TOL, (case.id, k, err)
            assert np.allclose(dev["trace"][k], ref["trace"][k], rtol=1e-9, atol=0), (case.id, k, dev["trace"][k], ref["trace"][k])
        else:
            rows = LE.fp32_row_errors(dev["G"][k], ref["G"][k])
            err = float(rows.max())
            print("%s run %d: G largest row error %.2e (row %d), costs %.2e" % (case.id, k, err, int(rows.argmax()), cost))
            assert err <= FP32_ROW_TOL, (case.id, k, int(rows.argmax()), err)
            assert cost <= FP32_ROW_TOL, (case.id, k, dev["trace"][k], ref["trace"][k])
        worst = max(worst, err)
    print("%s: variant %d, %d threads; G %.2e, costs %.2e at the most" % (case.id, dev["plan"]["variant"], dev["plan"]["threads"], worst, worst_cost))


@pytest.mark.parametrize("case", LE.CASES, ids=lambda c: c.id)
def test_one_iteration_at_the_ties(products, monkeypatch, oracle, case):
    """G and the costs of one iteration from lattice trajectories, in the form the case names: the plan's bits are asserted first"""
    ref, dev = _iterate(products, monkeypatch, oracle, case)
    if not common.plan_switches_active():
        assert dev["plan"]["variant"] & LE.VAR_MASK == case.bits, (case.id, dev["plan"], case.bits)
    _hold_iteration(case, ref, dev)


# ---- part C: the 24-bit offsets --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,accepted", LE.BIG_CASES, ids=[c.id for c, _ in LE.BIG_CASES])
def test_offsets_near_two_to_the_23(products, monkeypatch, oracle, case, accepted):
    """a y-z plane of 8 380 416 B (4 x 1024 x 1023 doubles) is accepted by the many-sphere pass and read right in its last x cells at
    the highest y and z; 1024 x 1024 doubles are refused there (for the 4-sphere robot too: it takes that pass), and accepted as floats,
    by the 16-lane row's fp64-formed offsets and by the pair list"""
    if not accepted:
        mod, name = products(case.scene, case.spheres)
        with pytest.raises(RuntimeError) as info:
            mod.batch_create(name, np.tile(LE.START, (2, 1)), n_points=LE.N_POINTS, **LE.KW)
        assert LE.REFUSAL in str(info.value), str(info.value)
        return
    ref, dev = _iterate(products, monkeypatch, oracle, case)
    if not common.plan_switches_active():
        assert dev["plan"]["variant"] & LE.VAR_MASK == case.bits, (case.id, dev["plan"], case.bits)
    _hold_iteration(case, ref, dev)


# ---- part D: the merge's interpolation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("scene", LE.MERGE_SCENES)
def test_merged_field_at_lattice_points(products, oracle, scene, parity):
    """orc_grid_interp of csrc/merge_interp.h: a scene's fields merged into a grid whose cell centres are their lattice points (faces,
    half-cell planes, bounds; +inf cells and neighbours; the ties of scene (c)) equal the oracle's best-of-N at those points, exactly"""
    want, _ = LE.merged_reference(oracle, scene, parity)
    mod, _ = products(scene, 1)
    target = "merged%d" % parity
    mod.add_kinbody_boxes(target, [], transform=LE.IDENT)
    mod.merge_fields(target, [(f.name, None) for f in LE.scene(scene)], LE.MERGE_CELL, LE.merge_bounds(scene, parity))
    got, glen, gpose = mod.get_sdf(target)
    mod.SendCommand("removefield kinbody %s" % target)      # (the module's other tests plan against the scene's own fields)
    assert got.shape == LE.MERGE_SIZES[scene] and list(gpose) == LE.merge_bounds(scene, parity)[:3] + [0.0, 0.0, 0.0, 1.0]
    differ = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    print("scene %s parity %d: %d cells, %d finite, %d differ" % (scene, parity, got.size, np.isfinite(want).sum(), len(differ)))
    assert len(differ) == 0, (scene, parity, [(tuple(c), got[tuple(c)], want[tuple(c)]) for c in differ[:8]])
