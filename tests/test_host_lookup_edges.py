"""The inputs of tests/test_gpu_lookup_edges.py, checked on the oracle alone (no GPU): a comparison at the ties of the field lookup
only says something if every class of lattice point occurs on every axis, the poison cases and the ties between fields are met, the
oracle itself takes the decision the lattice predicts, no limit round is made, the obstacle part carries the compared rows and no
waypoint has to be set aside.  NOTES/lookup-edges.md has the figures."""
import numpy as np
import pytest

import lookup_edges as LE

SHARED = [c for c in LE.CASES if c.precision == 64 and not c.env]      # (a case's precisions and switches share their inputs)


@pytest.mark.parametrize("case", SHARED, ids=lambda c: "%s-g%d" % (c.scene, c.spheres))
def test_inputs_meet_every_decision(oracle, case):
    ref = LE.reference(case, oracle)
    sv = ref["survey"]
    print("%s: lookups per class with the other two axes inside" % case.id)
    print("  %-10s %6s %6s %6s" % ("class", "x", "y", "z"))
    for cls in LE.CLASSES:
        print("  %-10s %6d %6d %6d" % ((cls,) + tuple(sv["table"][d][cls] for d in range(3))))
    print("  poison and ties: %s; most spheres inside one field at a waypoint: %d" % (dict(sv["kinds"]), sv["cap"]))
    # every class on every axis
    for d in range(3):
        for cls in LE.CLASSES:
            assert sv["table"][d][cls] >= LE.MIN_PER_CLASS, (case.id, d, cls, sv["table"][d][cls])
    # the poison cases, each at least twice; scene (c): the ties between the two fields
    for kind in ("cell", "used0", "used1", "used2", "unused"):
        assert sv["kinds"][kind] >= 2, (case.id, kind, sv["kinds"])
    if case.scene == "c":
        assert sv["kinds"]["tie"] >= 2, sv["kinds"]
    # the oracle's in / out code is the lattice's, at every lookup
    assert sv["agree"]
    # status 0, no limit round
    assert (ref["status"] == 0).all() and (ref["rounds"] == 0).all(), (ref["status"], ref["rounds"])
    # the caps on spheres inside a field at one waypoint
    assert sv["cap"] <= LE.INSIDE_CAP[case.spheres], sv["cap"]
    # the obstacle part carries every row a lookup contributes to (three quarters of all rows at least); the other rows are A T + B alone
    con = sv["contributing"][:, 1:-1]
    obs = np.linalg.norm(ref["G"] - ref["G_free"], axis=-1)
    share = obs / np.linalg.norm(ref["G"], axis=-1)
    print("  rows a lookup contributes to: %d of %d; their obstacle part over the row's norm: %.3f at the least" % (con.sum(), con.size, share[con].min()))
    assert con.mean() >= 0.6, con.mean()
    assert share[con].min() >= 0.5, share[con].min()
    # nothing is set aside: every sphere centre of every waypoint is a lattice point of every field, in float as well (trajectories()
    # asserts the rows; survey() asserts u Q == g for every lookup)
    assert np.array_equal(ref["T0"], ref["T0"].astype(np.float32).astype(np.float64))


def test_planted_points_are_what_they_claim():
    """a planted point's kind, from the data alone"""
    for name in LE.SCENE_NAMES:
        fs = LE.scene(name)
        kinds = set()
        for kind, fi, u in LE.planted(name):
            f = fs[fi]; N = f.data.shape
            c = [min(u[d] // 4, N[d] - 1) for d in range(3)]
            r = [u[d] - 4 * c[d] for d in range(3)]
            assert all(0 <= c[d] < N[d] and 0 <= r[d] <= 4 for d in range(3)), (name, kind, u)
            nb = [f.data[tuple(c[:d] + [c[d] + LE.used_side(c[d], N[d], r[d])] + c[d+1:])] for d in range(3)]
            if kind == "cell":
                assert np.isinf(f.data[tuple(c)])
            elif kind.startswith("used"):
                assert np.isfinite(f.data[tuple(c)]) and np.isinf(nb[int(kind[4])])
            elif kind == "unused":
                assert np.isfinite(f.data[tuple(c)]) and np.isfinite(nb).all()
                other = [f.data[tuple(c[:d] + [c[d] - LE.used_side(c[d], N[d], r[d])] + c[d+1:])] for d in range(3) if 0 <= c[d] - LE.used_side(c[d], N[d], r[d]) < N[d]]
                assert np.isinf(other).any()
            kinds.add(kind)
        assert {"cell", "used0", "used1", "used2", "unused"} <= kinds, (name, kinds)


def test_ties_of_scene_c(oracle):
    """at a planted tie the two fields give the same value and another gradient: only the strict `<` keeps the first field's"""
    grids, _ = LE.oracle_fields(oracle, "c")
    f0, f1 = LE.scene("c")
    for c0, a in LE.C_TIES:
        p = LE.to_world(f0, np.array(LE.lattice_of_cell(c0)) * LE.Q)
        (e0, v0), (e1, v1) = grids[0].interp(LE.to_field(f0, p)), grids[1].interp(LE.to_field(f1, p))
        g0, g1 = grids[0].grad(LE.to_field(f0, p))[1], grids[1].grad(LE.to_field(f1, p))[1]
        assert e0 == 0 and e1 == 0 and v0 == v1 == f0.data[tuple(c0)] and np.isfinite(v0)
        assert g0[0] != g1[0] and g1[0] == 64.0 * a * LE.VALUE


@pytest.mark.parametrize("scene", ["a", "b", "c", "d"])
def test_part_a_rows(oracle, scene):
    """every class combination of every field is a row; the restatement's verdict is the lattice's; a point one ulp outside a bound
    is outside in the field's frame in float as in double (the subtraction of the field's translation is exact there)"""
    fs = LE.scene(scene)
    finite = [f for f in fs if np.isfinite(f.data).any()]
    for precision in (64, 32):
        ref = LE.part_a_reference(oracle, scene, precision)
        assert len(ref["rows"]) >= len(LE.CLASSES) ** 3 * len(finite)
        real = np.float32 if precision == 32 else np.float64
        assert np.array_equal(ref["rows"], ref["rows"].astype(real).astype(np.float64))
        n_out = 0
        for name, q, clr, oth in zip(ref["names"], ref["rows"], ref["clearance"], ref["other"]):
            inside = []
            for f in fs:
                g = LE.to_field(f, q)
                g32 = (LE.rot(f.pose[3:7]).T.astype(real) @ q.astype(real) - (LE.rot(f.pose[3:7]).T @ np.asarray(f.pose[:3])).astype(real)).astype(np.float64)
                inside.append(bool(((g >= 0) & (g <= np.asarray(f.lengths))).all()))
                if "one ulp out" not in name or name.startswith(f.name + " "):
                    assert np.array_equal(g, g32), (name, g, g32)
                else:      # (another field, far from its bounds: the same verdict is all the row needs)
                    assert inside[-1] == bool(((g32 >= 0) & (g32 <= np.asarray(f.lengths))).all()), (name, g, g32)
            if "one ulp out" in name:
                n_out += 1
                assert not inside[[f.name for f in fs].index(name.split()[0])], name
            if not any(inside):
                assert clr[0] == np.inf and oth[0] == -1, name
        assert n_out == 6 * len(finite)
    print("scene %s: %d rows, %d with a finite clearance, %d with a cost" % (scene, len(ref["rows"]), np.isfinite(ref["clearance"][:, 0]).sum(),
                                                                              (ref["cost"][:, 0] > 0).sum()))
    assert np.isfinite(ref["clearance"][:, 0]).sum() >= 100 and (ref["cost"][:, 0] > 0).sum() >= 100


def test_rounded_lengths_of_scene_e(oracle):
    """scene (e): the oracle's own division p / length puts every lattice point of the 6 x 5 x 7 field in the cell the lattice names
    (so part B may aim at its faces); which of the points part A asserts and which it only records"""
    f = LE.scene("e")[0]
    grid = oracle.OraGrid(f.data, f.lengths)
    import ctypes
    N = f.data.shape
    for ax in range(3):
        for u_ax in range(0, 4 * N[ax] + 1):
            g = np.array([6.0, 6.0, 6.0]) * LE.Q
            g[ax] = u_ax * LE.Q
            idx = ctypes.c_size_t()
            assert oracle.lib().ora_grid_lookup_index(grid.ptr, oracle.dp(g), ctypes.byref(idx)) == 0
            sub = np.unravel_index(idx.value, N)[ax]
            assert sub == min(u_ax // 4, N[ax] - 1), (ax, u_ax, sub)
    asserted, recorded = LE.rounded_length_points()
    assert len(asserted) >= 30 and len(recorded) >= 30


@pytest.mark.parametrize("scene", LE.MERGE_SCENES)
def test_merge_points(oracle, scene):
    """the merged grids' cell centres are lattice points of the sources: between the two parities every class of the first field on
    every axis; finite cells, poisoned cells and ties are among them"""
    finite = 0
    met = [set() for _ in range(3)]
    for parity in (0, 1):
        want, m = LE.merged_reference(oracle, scene, parity)
        assert want.shape == LE.MERGE_SIZES[scene] and not np.isnan(want).any()
        finite += int(np.isfinite(want).sum())
        assert np.isposinf(want).any() and np.isfinite(want).any()
        for d in range(3):
            met[d] |= m[d]
    for d in range(3):
        assert met[d] == set(LE.CLASSES), (scene, d, set(LE.CLASSES) - met[d])
    print("scene %s: %d finite merged cells of %d" % (scene, finite, 2 * want.size))
