"""-m gpu: the penetration cost of configurations and of waypoints with its gradient (orc_batch_config_penetration,
orc_batch_waypoint_penetration; Module.batch_config_penetration, batch_waypoint_penetration, batch_push_out).

Three yardsticks.  The minima and keys are batch_config_clearance's, bit for bit.  Cost and gradient are held to the
restatement of tests/penetration.py (whose own gradient tests/test_host_penetration.py holds to central differences), and
the gradient to central differences of the call's own cost.  And a query's answer is held to itself across list positions,
chunks, shards and the waypoint form.  The premises (no contributing item near a cell face, the rows' coverage) are checked in
tests/test_host_penetration.py."""
import numpy as np
import pytest

import clearance as CL
import common
import config_clearance as CC
import or_cdchomp_amd
import penetration as PN
from or_cdchomp_amd import _capi, pushout, robots, scenes
from test_gpu_clearance import bits, product_field
from test_gpu_verdict_device import KW, same, set_wam_vmax

pytestmark = pytest.mark.gpu

OUT = ("cost", "grad", "clearance", "sphere", "other")
KW4 = dict(KW, n_points=4)
TOL = {64: 1e-10, 32: 1e-3}      # relative to the row's largest entry: test_seed_and_first_gradient's bar on G; the project's fp32 bar
FD_TOL = 1e-6                    # tests/test_host_penetration.py has the reasoning


def assert_same(got, want, what="", keys=OUT):
    """bit for bit, the outputs of two results (dicts of arrays of one shape)"""
    for key in keys:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.shape == b.shape, (what, key, a.shape, b.shape)
        if a.dtype == np.float64:
            assert np.array_equal(bits(a), bits(b)), (what, key, a, b)
        else:
            assert a.dtype == np.int32 and np.array_equal(a, b), (what, key, a, b)


def pick(res, idx):
    return {key: np.asarray(res[key])[idx] for key in OUT}


def check(mod, bid, tab, col0, fields_of_run, rows, runs, precision=64, what="", self_check=True):
    """the checks every case makes: at the three margins the minima against the parent's call and zero cost exactly where the
    parent's clearance keeps the margin; at the margins of PN.RESTATED cost and gradient against the restatement.  Returns the
    results by margin."""
    parent = mod.batch_config_clearance(bid, rows, runs=runs)
    real = np.float64 if precision == 64 else np.float32
    out = {}
    for margin in PN.MARGINS + PN.RESTATED[2:]:
        got = mod.batch_config_penetration(bid, rows, runs=runs, margin=margin)
        out[margin] = got
        assert_same(got, parent, what + ": minima", keys=("clearance", "sphere", "other"))
        assert got["cost"].shape == (len(rows), 2) and got["grad"].shape == rows.shape
        m = np.array([real(margin[0]), real(margin[1])], dtype=np.float64)      # (the margins in the batch's precision)
        assert np.array_equal(got["cost"] == 0.0, parent["clearance"] >= m), (what, margin, got["cost"], parent["clearance"])
        assert (got["cost"] >= 0.0).all() and np.isfinite(got["grad"]).all()
        if margin not in PN.RESTATED:
            continue
        worst = 0.0
        for k, q in enumerate(rows):
            q = np.asarray(q, dtype=real).astype(np.float64)
            res = PN.restate(tab, q, col0, fields_of_run[int(runs[k])], margin, self_check)
            for key in ("cost", "grad"):
                scale = max(float(np.abs(res[key]).max()), 1e-300)
                err = float(np.abs(got[key][k] - res[key]).max()) / scale
                worst = max(worst, err)
                assert err <= TOL[precision], (what, margin, k, key, err, got[key][k], res[key])
        print("%s margins %s: largest relative difference from the restatement %.2e; rows with a cost %d of %d" % (what, margin, worst,
              int((got["cost"].sum(axis=1) > 0).sum()), len(rows)))
    return out


def check_single_items(got, parent, margin, precision):
    """rows with exactly one violating item: U_f is 0.5 (m - c)^2 of the parent's clearance c, to 4 ulp of the batch's precision"""
    real = np.float64 if precision == 64 else np.float32
    m, c = real(margin[0]), parent["clearance"][:, 0].astype(real)
    d = (m - c).astype(real)
    want = (real(0.5) * d * d).astype(real)
    return np.abs(got["cost"][:, 0].astype(real) - want) <= 4 * np.spacing(want)


@pytest.fixture(scope="module")
def wam(oracle):
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    vmax = set_wam_vmax(mod, model)
    _, base, dofvals, adofs = common.wam_state()
    field = product_field(oracle, mod, "table")
    tab = CL.Tables(oracle, model, base, dofvals, adofs, [field])
    shifted = product_field(oracle, mod, "table", kpose=PN.compose(oracle, PN.SHIFT, mod.body_transform("table")))
    yield dict(mod=mod, model=model, vmax=vmax, field=field, shifted=shifted, tab=tab)
    mod.close()


@pytest.fixture(scope="module")
def wam_batch(wam):
    """one batch of two runs over two scenes, for the tests that only ask questions of it"""
    mod, model = wam["mod"], wam["model"]
    bid = mod.batch_create(model.name, common.wam_goals(2, seed=2), scenes=[[("table", None)], [("table", PN.SHIFT)]],
                           scene_of_run=np.array([0, 1], dtype=np.int32), **KW4)
    yield bid
    mod.batch_destroy(bid)


# ---- 1. the WAM and the table: minima, zero cost, one violating item, the restatement, both precisions ---------------------------

@pytest.mark.parametrize("precision", [64, 32])
def test_wam_and_table(wam, precision):
    mod, model = wam["mod"], wam["model"]
    names = list(PN.wam_rows())
    rows = np.array(list(PN.wam_rows().values()))
    bid = mod.batch_create(model.name, common.wam_goals(1, seed=1), **dict(KW4, precision=precision))
    runs = np.zeros(len(rows), dtype=np.int32)
    res = check(mod, bid, wam["tab"], 0, [[wam["field"]]], rows, runs, precision, "wam fp%d" % precision)
    parent = mod.batch_config_clearance(bid, rows, runs=runs)
    tight = PN.MARGINS[1]
    single = PN.single_item_rows(wam["tab"], 0, [wam["field"]], rows.astype(np.float32 if precision == 32 else np.float64).astype(np.float64), tight)
    assert single.any()
    ok = check_single_items(res[tight], parent, tight, precision)
    assert ok[single].all(), (np.array(names)[single], res[tight]["cost"][single], parent["clearance"][single])
    got = res[PN.MARGINS[2]]
    assert (got["cost"][names.index("in the table")] > 0).all() and got["cost"][names.index("folded"), 1] > 0
    assert got["cost"][names.index("away"), 0] == 0.0 and np.abs(got["grad"][names.index("away")]).max() < 1e-6, "outside the field; the rigid pairs alone"
    # one row, one int for all, None for run 0
    assert_same(mod.batch_config_penetration(bid, rows[4]), pick(res[tight], slice(4, 5)), "a single row, run 0")
    if precision == 32:
        assert same(got["cost"], got["cost"].astype(np.float32)) and same(got["grad"], got["grad"].astype(np.float32)), "floats, widened"
    mod.batch_destroy(bid)


# ---- 2. central differences of the call's own cost --------------------------------------------------------------------------------

def differences(mod, bid, rows, margin, run=0):
    worst = 0.0
    for q in rows:
        here = mod.batch_config_penetration(bid, q, runs=run, margin=margin)
        if not here["cost"].sum() > 0:
            assert (here["grad"] == 0).all()
            continue
        fd = PN.central_differences(lambda r: mod.batch_config_penetration(bid, r, runs=run, margin=margin)["cost"].sum(axis=1), q)
        err = float(np.abs(fd - here["grad"][0]).max())
        worst = max(worst, err)
        assert err <= FD_TOL, (margin, q, err, fd, here["grad"][0])
    return worst


def test_finite_differences_wam(wam, wam_batch):
    rows = np.array(list(PN.wam_rows().values()))
    for margin in PN.MARGINS[1:]:
        for run in (0, 1):
            print("wam, margins %s, run %d: largest difference from central differences %.2e" % (margin, run, differences(wam["mod"], wam_batch, rows, margin, run)))


# ---- 3. the variants ----------------------------------------------------------------------------------------------------------------

def test_floating_base(oracle):
    mod = or_cdchomp_amd.Module(0)
    model, _, dofvals, adofs = common.wam_state()
    base = PN.floating_base()
    mod.add_robot(model, transform=list(base), dof_values=dofvals, active_dofs=adofs)
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    set_wam_vmax(mod, model)
    field = product_field(oracle, mod, "table")
    tab = CL.Tables(oracle, model, base, dofvals, adofs, [field], floating=True)
    rows = CC.floating_configs(base)
    assert (np.abs(np.linalg.norm(rows[:, 3:7], axis=1) - 1.0) > 0.05).sum() >= 4, "the quaternions must not be of unit length"
    bid = mod.batch_create(model.name, common.wam_goals(1, seed=3), basegoals=base[None, :], **dict(KW4, floating_base=1))
    assert mod.batch_dims(bid)[2] == 14
    res = check(mod, bid, tab, 7, [[field]], rows, np.zeros(len(rows), dtype=np.int32), what="floating base")
    g = res[PN.MARGINS[2]]["grad"]
    assert np.abs(g[:, :3]).max() > 1e-2 and np.abs(g[:, 3:7]).max() > 1e-2 and np.abs(g[:, 7:]).max() > 1e-2
    for margin in PN.MARGINS[1:]:
        print("floating base, margins %s: largest difference from central differences %.2e" % (margin, differences(mod, bid, rows, margin)))
    # the same pose under another length of its quaternion: the gradient of the pose's four columns scales with 1 / length
    twice = rows.copy(); twice[:, 3:7] *= 2.0
    two = mod.batch_config_penetration(bid, twice, margin=PN.MARGINS[2])
    assert np.allclose(two["grad"][:, 3:7] * 2.0, g[:, 3:7], rtol=1e-9, atol=1e-13) and np.allclose(two["grad"][:, :3], g[:, :3], rtol=1e-9, atol=1e-13)
    mod.batch_destroy(bid)
    mod.close()


def test_floating_base_with_a_non_finite_row():
    """A floating base, one workgroup's worth of queries and one more, the last two with a non-finite entry (one in the pose's
    quaternion, one in a joint): FK runs on the harmless row with a unit quaternion in their place, they alone report NaN, and
    every other query answers as in the call without them, in both kernels."""
    mod = or_cdchomp_amd.Module(0)
    model, _, dofvals, adofs = common.wam_state()
    base = PN.floating_base()
    mod.add_robot(model, transform=list(base), dof_values=dofvals, active_dofs=adofs)
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    set_wam_vmax(mod, model)
    bid = mod.batch_create(model.name, common.wam_goals(1, seed=3), basegoals=base[None, :], **dict(KW4, floating_base=1))
    pool = CC.floating_configs(base)
    for chunk, ask in ((mod.batch_penetration_chunk(bid), lambda r: mod.batch_config_penetration(bid, r, margin=PN.MARGINS[2])),
                       (mod.batch_config_chunk(bid), lambda r: mod.batch_config_clearance(bid, r))):
        rows = pool[np.arange(chunk + 1) % len(pool)]
        want = ask(rows)
        keys = tuple(want)
        bad = rows.copy(); bad[chunk - 1, 4] = np.nan; bad[chunk, 9] = np.inf      # the last query of a workgroup, the first of the next
        got = ask(bad)
        for q in (chunk - 1, chunk):
            assert all(np.isnan(got[key][q]).all() for key in keys if got[key].dtype == np.float64), q
            assert (got["sphere"][q] == -1).all() and (got["other"][q] == -1).all(), q
        keep = np.arange(chunk - 1)
        assert_same({key: got[key][keep] for key in keys}, {key: want[key][keep] for key in keys}, "beside the non-finite rows", keys=keys)
        assert np.isfinite(want["clearance"][:, 1]).all()
    mod.batch_destroy(bid)
    mod.close()


def test_tree_robot(oracle):
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_tree30(mod)
    mod.set_velocity_limits(model.name, np.linspace(0.5, 2.0, model.n_dof))
    names = list(common.config5_bodies())
    fields = [product_field(oracle, mod, nm) for nm in names]
    assert len(fields) == 4
    tab = CL.Tables(oracle, model, [0.0] * 6 + [1.0], np.zeros(model.n_dof), list(range(model.n_dof)), fields)
    rows = CC.tree_pool()
    bid = mod.batch_create(model.name, common.config5_goals(2), **dict(common.CONFIG5_KW, n_points=4))
    assert mod.batch_plan(bid)["variant"] & 1, "the robot must be a tree"
    chunk = mod.batch_penetration_chunk(bid)
    print("tree: chunk", chunk, "of the clearance kernel", mod.batch_config_chunk(bid))
    assert 4 <= chunk <= 64 and chunk % 4 == 0
    res = check(mod, bid, tab, 0, [fields, fields], rows, np.arange(len(rows), dtype=np.int32) % 2, what="tree")
    assert len(set(res[PN.MARGINS[2]]["other"][:, 0].tolist()) - {-1}) >= 2, "more than one field must hold a minimum"
    check_positions(mod, bid, rows, 2, chunk, "tree", lengths=(1, 21, chunk + 1, 3 * chunk + 7))
    mod.batch_destroy(bid)
    mod.close()


def test_held_body(oracle):
    mod = or_cdchomp_amd.Module(0)
    model, hand, pose = common.setup_product_wam_held4(mod)
    set_wam_vmax(mod, model)
    _, base, dofvals, adofs = common.wam_state()
    field = product_field(oracle, mod, "table")
    tab = CL.Tables(oracle, model, base, dofvals, adofs, [field], held=[(hand, pose, common.HELD4_POS, common.HELD4_RAD)])
    rows = CC.held_configs()
    bid = mod.batch_create(model.name, common.wam_goals(1, seed=4), **KW4)
    res = check(mod, bid, tab, 0, [[field]], rows, np.zeros(len(rows), dtype=np.int32), what="held body")
    assert np.isin(res[PN.MARGINS[2]]["sphere"], [16, 17, 18, 19]).any(), "the held spheres must appear among the answers"
    mod.batch_destroy(bid)
    mod.close()


def test_self_check_off_and_on_again(oracle):
    mod = or_cdchomp_amd.Module(0)
    model, base, dofvals, adofs = common.wam_state()
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    mod.add_kinbody_boxes("far", [([0, 0, 0, 0, 0, 0, 1], [0.05, 0.05, 0.05])], transform=[5, 5, 5, 0, 0, 0, 1])
    mod.SendCommand("computedistancefield kinbody far")
    set_wam_vmax(mod, model)
    field = product_field(oracle, mod, "far")
    tab = CL.Tables(oracle, model, base, dofvals, adofs, [field])
    rows = CC.folding_configs()
    runs = np.zeros(len(rows), dtype=np.int32)
    bid = mod.batch_create(model.name, rows[:1], **dict(n_points=4, lambda_=100.0, obs_factor=0.0, obs_factor_self=0.0))
    on = check(mod, bid, tab, 0, [[field]], rows, runs, what="self check on")[PN.MARGINS[2]]
    assert (on["cost"][:, 1] > 0).all() and (on["cost"][:, 0] == 0).all() and (np.abs(on["grad"]).max(axis=1) > 0).sum() >= 2
    mod.set_self_check(model.name, False)
    off = check(mod, bid, tab, 0, [[field]], rows, runs, what="self check off", self_check=False)[PN.MARGINS[2]]
    assert (off["cost"] == 0).all() and (off["grad"] == 0).all() and np.isposinf(off["clearance"]).all()
    mod.set_self_check(model.name, True)
    assert_same(mod.batch_config_penetration(bid, rows, runs=runs, margin=PN.MARGINS[2]), on, "on again")
    mod.batch_destroy(bid)
    mod.close()


def test_per_run_scenes(wam):
    mod, model = wam["mod"], wam["model"]
    sc = [[("table", None)], [("table", PN.SHIFT)], []]
    pool = CC.wam_pool()
    goals = common.wam_goals(3, seed=6)
    bid = mod.batch_create(model.name, goals, scenes=sc, scene_of_run=np.arange(3, dtype=np.int32), **KW4)
    rows, runs = np.repeat(pool, 3, axis=0), np.tile(np.arange(3, dtype=np.int32), len(pool))
    res = check(mod, bid, wam["tab"], 0, [[wam["field"]], [wam["shifted"]], []], rows, runs, what="per-run scenes")[PN.MARGINS[2]]
    got = {key: res[key].reshape((len(pool), 3) + res[key].shape[1:]) for key in OUT}
    assert (got["cost"][:, 2, 0] == 0).all() and (got["cost"][:, 2, 1] > 0).all(), "the empty scene still has the robot itself"
    assert not np.array_equal(bits(got["cost"][:, 0, 0]), bits(got["cost"][:, 1, 0])), "the shifted scene must answer differently"
    for s in range(3):
        single = mod.batch_create(model.name, goals[:1], scenes=[sc[s]], scene_of_run=np.zeros(1, dtype=np.int32), **KW4)
        assert_same(mod.batch_config_penetration(single, pool, margin=PN.MARGINS[2]), pick(got, (slice(None), s)), "scene %d" % s)
        mod.batch_destroy(single)
    mod.batch_destroy(bid)


# ---- 4. bit for bit: list positions and lengths, two shards, the waypoint form ----------------------------------------------------

def check_positions(mod, bid, pool, n_runs, chunk, what, lengths=None, margin=PN.MARGINS[2]):
    alone = {key: [] for key in OUT}
    for c in range(len(pool)):
        for r in range(n_runs):
            res = mod.batch_config_penetration(bid, pool[c], runs=r, margin=margin)
            for key in OUT:
                alone[key].append(res[key][0])
    alone = {key: np.array(alone[key]).reshape((len(pool), n_runs) + np.shape(alone[key][0])) for key in OUT}
    assert len(np.unique(bits(alone["grad"]).reshape(len(pool) * n_runs, -1), axis=0)) > len(pool) // 2, "the answers must tell configurations and scenes apart"
    for length in (lengths or CC.lengths(chunk)):
        ci, ri = CC.draw(length, len(pool), n_runs, seed=length)
        got = mod.batch_config_penetration(bid, pool[ci], runs=ri, margin=margin)
        assert_same(got, pick(alone, (ci, ri)), "%s: %d queries" % (what, length))


def test_positions_wam(wam, wam_batch):
    chunk = wam["mod"].batch_penetration_chunk(wam_batch)
    print("wam: chunk", chunk)
    assert 4 <= chunk <= 64 and chunk % 4 == 0
    check_positions(wam["mod"], wam_batch, np.array(list(PN.wam_rows().values())), 2, chunk, "wam")


def test_waypoints_and_two_shards(wam):
    pool = np.array(list(PN.wam_rows().values()))
    ci = np.arange(21) % len(pool)
    ri = np.array([0, 2, 1, 3] * 6)[:21]      # runs 0, 1: the first shard; 2, 3: the second
    wr, wp = np.array([0, 2, 1, 3, 3, 0]), np.array([0, 1, 2, 3, 0, 1])
    two = or_cdchomp_amd.Module([0, 0])
    model2 = common.setup_product_wam(two)
    set_wam_vmax(two, model2)
    res = []
    for mod, model in ((wam["mod"], wam["model"]), (two, model2)):
        bid = mod.batch_create(model.name, common.wam_goals(4, seed=7), scenes=[[("table", None)], [("table", PN.SHIFT)]],
                               scene_of_run=np.array([0, 1, 1, 0], dtype=np.int32), **KW4)
        traj = np.tile(pool[:4, None, :], (1, 4, 1))
        traj[:, 1:] = pool[4:7][None, :, :]
        mod.batch_set_traj(bid, traj)
        prof = mod.batch_waypoint_penetration(bid, margin=PN.MARGINS[2])
        assert prof["cost"].shape == (4, 4, 2) and prof["grad"].shape == (4, 4, 7) and prof["sphere"].shape == (4, 4, 2)
        assert_same(prof, mod.batch_waypoint_clearance(bid), "profile: minima", keys=("clearance", "sphere", "other"))
        cfg = mod.batch_config_penetration(bid, traj.reshape(-1, 7), runs=np.repeat(np.arange(4), 4), margin=PN.MARGINS[2])
        assert_same({key: cfg[key].reshape((4, 4) + cfg[key].shape[1:]) for key in OUT}, prof, "the waypoint form against the config form")
        ends = mod.batch_waypoint_penetration(bid, points=(0, -1), margin=PN.MARGINS[2])
        assert_same(ends, pick(prof, (slice(None), [0, 3])), "starts and goals")
        named = mod.batch_waypoint_penetration(bid, runs=wr, points=wp, margin=PN.MARGINS[2])
        assert_same(named, pick(prof, (wr, wp)), "named waypoints")
        res.append((mod.batch_config_penetration(bid, pool[ci], runs=ri, margin=PN.MARGINS[2]), named, prof, ends))
        mod.batch_destroy(bid)
    for one, other, what in zip(res[0], res[1], ("configurations", "named waypoints", "profile", "starts and goals")):
        assert_same(other, one, "two shards: " + what)
    assert (res[0][2]["cost"][..., 0] > 0).any() and (res[0][2]["cost"][..., 0] == 0).any(), "both outcomes must occur"
    two.close()


def test_a_deal_with_absent_output_columns():
    """Two shards on one card, 4 runs, the 21 queries of test_waypoints_and_two_shards through the C ABI: an output the caller
    does not pass (NULL) is not dealt, and every output that is present equals the call with all of them, bit for bit."""
    pool = np.array(list(PN.wam_rows().values()))
    cf = np.ascontiguousarray(pool[np.arange(21) % len(pool)])
    ri = np.array([0, 2, 1, 3] * 6, dtype=np.int32)[:21]      # runs 0, 1: the first shard; 2, 3: the second
    two = or_cdchomp_amd.Module([0, 0])
    model = common.setup_product_wam(two)
    set_wam_vmax(two, model)
    bid = two.batch_create(model.name, common.wam_goals(4, seed=7), scenes=[[("table", None)], [("table", PN.SHIFT)]],
                           scene_of_run=np.array([0, 1, 1, 0], dtype=np.int32), **KW4)
    dp = lambda a: None if a is None else a.ctypes.data_as(_capi.c_double_p)
    ip = lambda a: None if a is None else a.ctypes.data_as(_capi.c_int_p)

    def call(absent=()):
        out = dict(cost=np.full((21, 2), -7.0), grad=np.full((21, 7), -7.0), clearance=np.full((21, 2), -7.0),
                   sphere=np.full((21, 2), -7, dtype=np.int32), other=np.full((21, 2), -7, dtype=np.int32))
        for key in absent:
            out[key] = None
        rc = two._lib.orc_batch_config_penetration(two._h, bid, 21, ip(ri), dp(cf), PN.MARGINS[2][0], PN.MARGINS[2][1], dp(out["cost"]),
                                                   dp(out["grad"]), dp(out["clearance"]), ip(out["sphere"]), ip(out["other"]))
        assert rc == 0, two._lib.orc_last_error(two._h).decode()
        return out

    full = call()
    assert_same(full, two.batch_config_penetration(bid, cf, runs=ri, margin=PN.MARGINS[2]), "the C call against the wrapper's")
    assert (full["cost"][:, 0] > 0).any() and (full["grad"] != 0).any() and (full["sphere"] >= 0).any()
    for absent in (("grad",), ("sphere", "other"), ("cost",), ("sphere",), ("cost", "grad", "clearance")):
        part = call(absent)
        assert_same(part, full, "without " + " and ".join(absent), keys=[key for key in OUT if key not in absent])
    two.close()


# ---- 5. no state, rejected calls -------------------------------------------------------------------------------------------------

def test_the_calls_leave_no_state(wam):
    mod, model = wam["mod"], wam["model"]
    kw = dict(KW, n_points=16)
    goals = common.wam_goals(4, seed=92); goals[-1] = CL.IN_TABLE
    asked, twin = mod.batch_create(model.name, goals, **kw), mod.batch_create(model.name, goals, **kw)
    for bid in (asked, twin):
        mod.batch_iterate(bid, 5)
    before = mod.batch_select_clear(asked, n_groups=2, margin=-np.inf, by="clearance")
    prof = mod.batch_waypoint_penetration(asked)
    mod.batch_config_penetration(asked, CC.wam_pool(), runs=np.arange(8) % 4)
    mod.batch_waypoint_penetration(asked, points=(0, -1))
    mod.batch_push_out(asked, CC.wam_pool()[:3], runs=np.arange(3), max_steps=3)
    after = mod.batch_select_clear(asked, n_groups=2, margin=-np.inf, by="clearance")
    for a, b in zip(before, after):
        assert np.array_equal(a, b, equal_nan=True)
    assert same(mod.batch_gettraj(asked), mod.batch_gettraj(twin))
    out = [mod.batch_iterate(bid, 5) for bid in (asked, twin)]
    assert same(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), "costs and status"
    assert same(mod.batch_gettraj(asked), mod.batch_gettraj(twin)), "trajectories"
    assert not same(mod.batch_waypoint_penetration(asked)["cost"], prof["cost"]), "the profile follows the trajectories"
    mod.batch_destroy(asked); mod.batch_destroy(twin)


def test_rejected_calls(wam):
    mod, model = wam["mod"], wam["model"]
    lib, h = mod._lib, mod._h
    dp, ip = _capi.c_double_p, _capi.c_int_p
    n_runs, n_points = 3, 4
    pool = CC.wam_pool()[[1, 2, 5]]
    bid = mod.batch_create(model.name, common.wam_goals(n_runs, seed=8), **KW4)
    mod.batch_set_traj(bid, CC.one_sample_batch(pool))
    traj = mod.batch_gettraj(bid)
    want = mod.batch_config_penetration(bid, pool, runs=np.arange(3))
    assert (want["cost"][:, 0] > 0).any()
    nq = n_runs * n_points
    cst = np.full((nq, 2), 7.0); grd = np.full((nq, 7), 7.0); clr = np.full((nq, 2), 7.0)
    sph = np.full((nq, 2), 7, dtype=np.int32); oth = sph.copy()
    cfg = np.ascontiguousarray(pool); run = np.arange(3, dtype=np.int32); pt = np.zeros(3, dtype=np.int32)
    arr = lambda *v: np.array(v, dtype=np.int32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
    outs = lambda: (ptr(cst, dp), ptr(grd, dp), ptr(clr, dp), ptr(sph, ip), ptr(oth, ip))
    config = lambda b, n_q, r, c, mf=0.02, ms=0.0: lib.orc_batch_config_penetration(h, b, n_q, ptr(r, ip), ptr(c, dp), mf, ms, *outs())
    waypoint = lambda b, n_q, r, p, mf=0.02, ms=0.0: lib.orc_batch_waypoint_penetration(h, b, n_q, ptr(r, ip), ptr(p, ip), mf, ms, *outs())
    cases = {
        "config: unknown batch": lambda: config(bid + 1000, 3, run, cfg), "waypoint: unknown batch": lambda: waypoint(bid + 1000, 3, run, pt),
        "config: n_q 0": lambda: config(bid, 0, run, cfg), "config: n_q 2^22 + 1": lambda: config(bid, (1 << 22) + 1, None, cfg),
        "waypoint: n_q 0": lambda: waypoint(bid, 0, run, pt), "waypoint: n_q 2^22 + 1": lambda: waypoint(bid, (1 << 22) + 1, None, None),
        "config: no configs": lambda: config(bid, 3, run, None),
        "config: run -1": lambda: config(bid, 3, arr(0, -1, 2), cfg), "config: run n_runs": lambda: config(bid, 3, arr(0, 1, n_runs), cfg),
        "waypoint: run -1": lambda: waypoint(bid, 3, arr(-1, 1, 2), pt), "waypoint: run n_runs": lambda: waypoint(bid, 3, arr(0, n_runs, 2), pt),
        "waypoint: point -1": lambda: waypoint(bid, 3, run, arr(0, 0, -1)), "waypoint: point n_points": lambda: waypoint(bid, 3, run, arr(n_points, 0, 0)),
        "waypoint: runs without points": lambda: waypoint(bid, 3, run, None), "waypoint: points without runs": lambda: waypoint(bid, 3, None, pt),
        "waypoint: the profile with a wrong n_q": lambda: waypoint(bid, nq - 1, None, None),
        "config: a negative margin": lambda: config(bid, 3, run, cfg, -1e-9, 0.0), "config: a NaN margin": lambda: config(bid, 3, run, cfg, 0.02, np.nan),
        "config: an infinite margin": lambda: config(bid, 3, run, cfg, np.inf, 0.0),
        "waypoint: a negative margin": lambda: waypoint(bid, 3, run, pt, 0.02, -0.5), "waypoint: a NaN margin": lambda: waypoint(bid, 3, run, pt, np.nan, 0.0),
    }
    for name, call in cases.items():
        assert call() == 1, name
        assert lib.orc_last_error(h).decode(), name
        assert (cst == 7.0).all() and (grd == 7.0).all() and (clr == 7.0).all() and (sph == 7).all() and (oth == 7).all(), name
        assert same(mod.batch_gettraj(bid), traj), name
        assert config(bid, 3, run, cfg) == 0, name      # the next valid call succeeds
        assert_same(dict(cost=cst[:3], grad=grd[:3], clearance=clr[:3], sphere=sph[:3], other=oth[:3]), want, name)
        cst[:] = 7.0; grd[:] = 7.0; clr[:] = 7.0; sph[:] = 7; oth[:] = 7
    # any output may be NULL
    assert lib.orc_batch_config_penetration(h, bid, 3, None, ptr(cfg, dp), 0.02, 0.0, None, None, None, None, None) == 0
    assert lib.orc_batch_waypoint_penetration(h, bid, nq, None, None, 0.02, 0.0, None, ptr(grd, dp), None, None, None) == 0
    assert same(grd[0], want["grad"][0]) and same(grd[n_points], want["grad"][1]), "the profile's first rows are the configurations"
    # a non-finite entry: that query alone is not evaluated
    for poison in (np.nan, np.inf, -np.inf):
        bad = pool.copy(); bad[1, 5] = poison
        got = mod.batch_config_penetration(bid, bad, runs=np.arange(3))
        assert np.isnan(got["cost"][1]).all() and np.isnan(got["grad"][1]).all() and np.isnan(got["clearance"][1]).all(), poison
        assert (got["sphere"][1] == -1).all() and (got["other"][1] == -1).all(), poison
        assert_same(pick(got, [0, 2]), pick(want, [0, 2]), "beside a poisoned row")
    assert_same(mod.batch_config_penetration(bid, pool, runs=np.arange(3)), want, "after the poisoned rows")
    # the Python layer's own checks
    for call in (lambda: mod.batch_config_penetration(bid, pool[:, :6]), lambda: mod.batch_config_penetration(bid, pool, runs=[0, 1]),
                 lambda: mod.batch_config_penetration(bid, pool, margin=(0.02, -1.0)), lambda: mod.batch_config_penetration(bid, pool, margin=(0.1, 0.1, 0.1)),
                 lambda: mod.batch_waypoint_penetration(bid, runs=[0, 1]), lambda: mod.batch_waypoint_penetration(bid, points=n_points),
                 lambda: mod.batch_waypoint_penetration(bid, margin=np.nan), lambda: mod.batch_push_out(bid, pool, runs=n_runs)):
        with pytest.raises(ValueError):
            call()
    mod.batch_destroy(bid)


# ---- 6. push-out on the device ----------------------------------------------------------------------------------------------------

def test_push_out_on_the_device(wam, wam_batch):
    mod = wam["mod"]
    wam7 = robots.wam7()
    lo, hi = np.asarray(wam7.limit_lower[:7]), np.asarray(wam7.limit_upper[:7])
    rows = PN.wam_rows()
    names = list(PN.named_rows()) + ["start", "away", "folded"]
    sent = np.array([rows[nm] for nm in names])
    margin = PN.MARGINS[1]
    cpu = pushout.push_out(PN.evaluator(wam["tab"], 0, [wam["field"]]), sent, margin, lower=lo, upper=hi)
    assert cpu[1][:7].tolist() == PN.CPU_STEPS
    out, steps, status = mod.batch_push_out(wam_batch, sent, runs=np.zeros(len(sent), dtype=np.int32), margin=margin, lower=lo, upper=hi)
    for k, nm in enumerate(names):
        print("%-14s status %d (host %d) steps %2d (host %2d) moved %.4f" % (nm, status[k], cpu[2][k], steps[k], cpu[1][k], np.linalg.norm(out[k] - sent[k])))
    assert np.array_equal(status, cpu[2]) and (np.abs(steps - cpu[1]) <= 1).all()
    assert (status[:7] == 0).all() and status[names.index("folded")] != 0
    assert (out >= lo).all() and (out <= hi).all()
    clear = mod.batch_config_clearance(wam_batch, out)["clearance"]
    assert (clear[status == 0] >= np.asarray(margin)).all(), clear
    for nm in ("start", "away"):
        k = names.index(nm)
        assert steps[k] == 0 and same(out[k], sent[k]), nm
    # rows of different runs: each is pushed out of its own scene
    both, _, st = mod.batch_push_out(wam_batch, np.repeat(sent[:3], 2, axis=0), runs=np.tile([0, 1], 3), margin=margin, lower=lo, upper=hi)
    assert (st == 0).all()
    c = mod.batch_config_clearance(wam_batch, both, runs=np.tile([0, 1], 3))["clearance"]
    assert (c >= np.asarray(margin)).all() and not same(both[0::2], both[1::2])
