"""-m gpu: multi-start batches (orc_batch_perturb, orc_batch_select_best, orc_batch_gettraj_runs and their Module methods)
on the WAM tabletop.  The device is held to the pure specifications of or_cdchomp_amd.module -- seed_perturbation (built
from the library's host utilities orc_host_gsl_stream and orc_host_metric) and select_best (numpy) -- and to its own other
entry points: a perturbed batch is the batch given those trajectories through orc_batch_set_traj, a run's displacement does
not depend on what shares its batch or shard, the gather is batch_gettraj's rows."""
import numpy as np
import pytest

import common
import or_cdchomp_amd
from or_cdchomp_amd import _capi, robots
from or_cdchomp_amd.module import contiguous_groups, seed_perturbation, select_best

pytestmark = pytest.mark.gpu

KW = dict(common.CONFIG2_KW)                     # n_points 100, lambda 100, obs_factor 500
INF = float("inf")
IN_TABLE = [1.2, -0.2, 0.0, 0.3, 0.0, 0.0, 0.0]    # a configuration with the forearm in the table top: every trajectory that ends (or passes) there collides


def same(a, b):
    """bit-identical arrays"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope="module")
def wam():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    yield mod, model
    mod.close()


@pytest.fixture(scope="module")
def wam2():
    """the same scene on a module of two in-process shards on one card"""
    mod = or_cdchomp_amd.Module([0, 0])
    model = common.setup_product_wam(mod)
    yield mod, model
    mod.close()


def limits(model):
    return np.asarray(model.limit_lower[:7], dtype=np.float64), np.asarray(model.limit_upper[:7], dtype=np.float64)


def spec_rows(model, line, sigma, seeds, derivative=1, lo=None, hi=None):
    """seed_perturbation for every run of a batch whose moving rows are `line` [n_runs][m][n]"""
    n_runs, m, n = line.shape
    llo, lhi = limits(model)
    lo = llo if lo is None else lo
    hi = lhi if hi is None else hi
    return np.stack([seed_perturbation(m, n, derivative, 1.0 / (m + 1), sigma, int(seeds[k]), lo, hi, line[k]) for k in range(n_runs)])


# ---- 1. perturbation parity ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_points,derivative,n_runs", [(100, 1, 64), (100, 2, 64), (100, 3, 64), (300, 1, 8), (300, 2, 8)])
def test_perturbation_matches_the_specification(wam, n_points, derivative, n_runs):
    """fp64: the displacement (device T minus the straight line) within 1e-10 relative L2 of the specification's, run by
    run -- the bar test_seed_and_first_gradient holds state read-backs to.  300 waypoints: a lane holds five rows.
    For derivative >= 2 the specification's solve (orc_host_metric) applies the same generators of A^-1 the device applies,
    serially: this test checks the device's draw, scans and order of summation, not the generators.  Those are checked
    against a dense inverse in tests/test_host_multistart.py::test_definition (m = 30, 1e-7) and by build_semisep's own
    check of every entry of the inverse at create."""
    mod, model = wam
    goals = common.wam_goals(n_runs, seed=31)
    seeds = np.arange(n_runs, dtype=np.uint32) * 7919 + 3
    seeds[1] = 0                                             # GSL's 4357
    sigma = 0.15
    bid = mod.batch_create(model.name, goals, **dict(KW, n_points=n_points, derivative=derivative))
    line = mod.batch_state(bid, "T")
    mod.batch_perturb(bid, sigma, seeds)
    got = mod.batch_state(bid, "T")
    mod.batch_destroy(bid)
    want = spec_rows(model, line, sigma, seeds, derivative)
    assert line.shape == (n_runs, n_points - 2, 7)
    worst = 0.0
    for k in range(n_runs):
        d_want = want[k] - line[k]
        assert np.abs(d_want[(n_points - 2) // 2]).max() > 0.01, "the workload must move the middle waypoint"
        err = common.rel_l2(got[k] - line[k], d_want)
        worst = max(worst, err)
        assert err <= 1e-10, (k, err)
    print("n_points %d derivative %d: worst relative L2 of the displacement %.3e" % (n_points, derivative, worst))
    assert same(mod_seed_0(model, line[1], sigma, derivative), want[1])


@pytest.mark.parametrize("n_points,derivative", [(32, 1), (100, 2)])
def test_perturbation_with_a_zero_word_in_the_stream(wam, n_points, derivative):
    """seeds whose fresh stream holds an output word of 0 inside the m n >= 210 values drawn (hmc_stream.ZERO_WORD_*: word 141,
    the second of its pair, and word 400, the first of its pair): gsl_rng_uniform_pos skips it, and the wavefront's chunk of 64
    pairs that meets it takes MtWave's one-at-a-time walk.  The specification and the bar of
    test_perturbation_matches_the_specification; that the specification's own stream skips the word as the oracle's does is
    tests/test_host_hmc_stream.py's"""
    import hmc_stream
    mod, model = wam
    seeds = np.array([hmc_stream.ZERO_WORD_SECOND[0], hmc_stream.ZERO_WORD_FIRST[0], 3, hmc_stream.ZERO_WORD_SECOND[0], hmc_stream.ZERO_WORD_FIRST[0]],
                     dtype=np.uint32)
    n_runs = len(seeds)
    goals = common.wam_goals(n_runs, seed=31)
    sigma = 0.15
    bid = mod.batch_create(model.name, goals, **dict(KW, n_points=n_points, derivative=derivative))
    line = mod.batch_state(bid, "T")
    mod.batch_perturb(bid, sigma, seeds)
    got = mod.batch_state(bid, "T")
    mod.batch_destroy(bid)
    assert line.shape == (n_runs, n_points - 2, 7) and (n_points - 2) * 7 >= 210
    want = spec_rows(model, line, sigma, seeds, derivative)
    worst = 0.0
    for k in range(n_runs):
        d_want = want[k] - line[k]
        assert np.abs(d_want[(n_points - 2) // 2]).max() > 0.01, "the workload must move the middle waypoint"
        err = common.rel_l2(got[k] - line[k], d_want)
        worst = max(worst, err)
        assert err <= 1e-10, (k, int(seeds[k]), err)
    print("zero-word seeds, n_points %d derivative %d: worst relative L2 of the displacement %.3e" % (n_points, derivative, worst))


def mod_seed_0(model, line, sigma, derivative):
    """the run seeded 0, by the specification with GSL's default seed spelled out"""
    m, n = line.shape
    lo, hi = limits(model)
    return seed_perturbation(m, n, derivative, 1.0 / (m + 1), sigma, 4357, lo, hi, line)


@pytest.mark.parametrize("derivative", [1, 2])
def test_perturbation_fp32(wam, derivative):
    """a precision 32 batch: the draw and the solve are in double, so every entry is the specification's rounded to float:
    one rounding plus a flipped tie, 2 float ulps"""
    mod, model = wam
    n_runs = 64
    goals = common.wam_goals(n_runs, seed=32)
    seeds = np.arange(n_runs, dtype=np.uint32) + 100
    bid = mod.batch_create(model.name, goals, **dict(KW, derivative=derivative, precision=32))
    line = mod.batch_state(bid, "T")
    mod.batch_perturb(bid, 0.15, seeds)
    got = mod.batch_state(bid, "T")
    mod.batch_destroy(bid)
    assert same(line, line.astype(np.float32)), "a precision 32 batch holds floats"
    want = spec_rows(model, line, 0.15, seeds, derivative).astype(np.float32)
    assert np.abs(want.astype(np.float64) - line).max() > 0.05, "the workload must be displaced"
    ulps = np.abs(got - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    print("derivative %d fp32: worst distance %.2f float ulps" % (derivative, ulps.max()))
    assert ulps.max() <= 2.0


def test_long_runs_and_the_lds_bound():
    """the 30-dof tree: 300 waypoints are 298 x 30 doubles of xi, 71.5 KB -- more than the 64 KB a kernel has without
    asking, so the launch opts in to a larger LDS share; 700 waypoints in fp32 are 20 940 entries, over the bound of
    20 136 (8 m n + 2496 <= 160 KB - 256), and are rejected with the batch unchanged"""
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_tree30(mod)
    n_runs, n = 3, model.n_dof
    goals = common.config5_goals(n_runs)
    seeds = np.array([5, 0, 123456789], dtype=np.uint32)
    lo, hi = np.asarray(model.limit_lower, dtype=np.float64), np.asarray(model.limit_upper, dtype=np.float64)
    n_points = 300
    assert (n_points - 2) * n * 8 + 2496 > 64 * 1024
    bid = mod.batch_create(model.name, goals, **dict(common.CONFIG5_KW, n_points=n_points))
    line = mod.batch_state(bid, "T")
    mod.batch_perturb(bid, 0.1, seeds)
    got = mod.batch_state(bid, "T")
    mod.batch_destroy(bid)
    for k in range(n_runs):
        want = seed_perturbation(n_points - 2, n, 1, 1.0 / (n_points - 1), 0.1, int(seeds[k]), lo, hi, line[k])
        assert np.abs(want - line[k]).max() > 0.05
        assert common.rel_l2(got[k] - line[k], want - line[k]) <= 1e-10, k
    n_points = 700
    assert (n_points - 2) * n > 20136
    bid = mod.batch_create(model.name, goals, **dict(common.CONFIG5_KW, n_points=n_points, precision=32))
    before = mod.batch_gettraj(bid)
    rc = mod._lib.orc_batch_perturb(mod._h, bid, 0.1, seeds.ctypes.data_as(_capi.c_uint_p))
    assert "LDS" in rejected(mod, rc)
    assert same(mod.batch_gettraj(bid), before)
    mod.batch_destroy(bid)
    mod.close()


# ---- 2. identity and limits ------------------------------------------------------------------------------------------

def test_sigma_zero_and_clamping(wam):
    mod, model = wam
    n_runs = 64
    goals = common.wam_goals(n_runs, seed=33)
    seeds = np.arange(n_runs, dtype=np.uint32) + 1
    bid = mod.batch_create(model.name, goals, **KW)
    line = mod.batch_state(bid, "T")
    full = mod.batch_gettraj(bid)
    mod.batch_perturb(bid, 0.0, seeds)
    assert same(mod.batch_gettraj(bid), full), "sigma = 0 changes no bit"
    sigma = 3.0
    mod.batch_perturb(bid, sigma, seeds)
    got = mod.batch_state(bid, "T")
    after = mod.batch_gettraj(bid)
    mod.batch_destroy(bid)
    lo, hi = limits(model)
    free = spec_rows(model, line, sigma, seeds, 1, -INF, INF)
    want = spec_rows(model, line, sigma, seeds, 1)
    below, above = free < lo, free > hi
    assert ((below | above).reshape(n_runs, -1).sum(axis=1) >= 1).all(), "the specification must clamp an entry of every run"
    assert (~(below | above)).any()
    assert (got >= lo).all() and (got <= hi).all()
    assert same(got[below], np.broadcast_to(lo, got.shape)[below])
    assert same(got[above], np.broadcast_to(hi, got.shape)[above])
    assert same(got[below | above], want[below | above])
    for k in range(n_runs):
        assert common.rel_l2(got[k] - line[k], want[k] - line[k]) <= 1e-10, k
    # the fixed ends are the fixed ends
    assert same(after[:, 0], full[:, 0]) and same(after[:, -1], full[:, -1])


# ---- 3. no hidden state ----------------------------------------------------------------------------------------------

def test_perturbed_batch_is_the_batch_given_those_trajectories(wam):
    mod, model = wam
    n_runs = 64
    goals = common.wam_goals(n_runs, seed=20250101)
    seeds = np.arange(n_runs, dtype=np.uint32) + 500
    a = mod.batch_create(model.name, goals, **KW)
    start = mod.batch_gettraj(a)
    mod.batch_perturb(a, 0.2, seeds)
    seeded = mod.batch_gettraj(a)
    assert not same(seeded, start)
    ca, sa = mod.batch_iterate(a, 100)
    ta, ia = mod.batch_gettraj(a), mod.batch_iterations_done(a)
    b = mod.batch_create(model.name, goals, **KW)
    mod.batch_set_traj(b, seeded)
    cb, sb = mod.batch_iterate(b, 100)
    tb, ib = mod.batch_gettraj(b), mod.batch_iterations_done(b)
    mod.batch_destroy(a); mod.batch_destroy(b)
    assert np.abs(ta - seeded).max() > 1e-3, "the runs must have moved"
    assert same(ta, tb) and same(ca, cb)
    assert np.array_equal(sa, sb) and np.array_equal(ia, ib)


# ---- 4. independence of composition ----------------------------------------------------------------------------------

def test_a_run_does_not_depend_on_its_batch_or_shard(wam, wam2):
    mod, model = wam
    mod2, _ = wam2
    n_runs = 50                                             # (two shards of 25)
    goals = common.wam_goals(n_runs, seed=34)
    goals[1] = goals[0]
    seeds = np.arange(n_runs, dtype=np.uint32) * 13 + 11
    seeds[1] = seeds[0]                                      # runs 0 and 1: one problem, one seed
    goals[3] = goals[2]                                      # runs 2 and 3: one problem, two seeds

    def perturbed(m_, idx, **kw):
        bid = m_.batch_create(model.name, goals[idx], **dict(KW, **kw))
        m_.batch_perturb(bid, 0.2, seeds[idx])
        t = m_.batch_gettraj(bid)
        m_.batch_destroy(bid)
        return t

    for kw in (dict(), dict(derivative=2)):
        everything = perturbed(mod, np.arange(n_runs), **kw)
        assert np.abs(everything[:, 49] - (everything[:, 0] + everything[:, -1]) / 2).max() > 0.05, "the workload must be displaced"
        sub = np.array([5, 17, 18, 40, 49, 0])
        assert same(perturbed(mod, sub, **kw), everything[sub])
        assert same(perturbed(mod2, np.arange(n_runs), **kw), everything)
        assert same(perturbed(mod2, sub, **kw), everything[sub])
        assert same(everything[0], everything[1])
        assert not same(everything[2], everything[3])
        assert np.abs(everything[2] - everything[3]).max() > 0.01


# ---- 5. selection ----------------------------------------------------------------------------------------------------

K = 8
N_PROBLEMS = 30          # config 2's own goals, K perturbed starts each; then a group that ends in the table and a group of identical runs
N_GROUPS = N_PROBLEMS + 2
N_RUNS = N_GROUPS * K
TIE_GOAL = 14 * K        # the one problem of the workload whose goal the straight line reaches without a contact


def multistart_workload():
    base = common.wam_goals(N_PROBLEMS + 1, seed=20250101)
    goals = np.repeat(base[:N_PROBLEMS], K, axis=0)
    goals = np.concatenate([goals, np.tile(IN_TABLE, (K, 1)), np.tile(base[N_PROBLEMS], (K, 1))])
    seeds = np.arange(N_RUNS, dtype=np.uint32) + 9000
    seeds[-K:] = 77                                          # the last group: K identical runs, a K-fold tie
    return goals, seeds


def check_selection(mod, bid, rng):
    """batch_select_best against select_best of the read-backs, for contiguous and shuffled groups, with and without the
    verdict; returns the read-backs and the four results"""
    costs, status = mod.batch_sync(bid)
    col = mod.batch_collision_verdict(bid)["collides"]
    contiguous = contiguous_groups(N_RUNS, N_GROUPS)
    shuffled = rng.permutation(contiguous).astype(np.int32)
    out = {}
    for name, grp in (("contiguous", contiguous), ("shuffled", shuffled), ("null", None)):
        for cf in (True, False):
            got = mod.batch_select_best(bid, groups=grp, n_groups=N_GROUPS, collision_free=cf)
            want = select_best(costs, status, col if cf else None, contiguous if grp is None else grp, N_GROUPS)
            assert np.array_equal(got[0], want[0]), (name, cf, got[0], want[0])
            assert same(got[1], want[1]), (name, cf)
            assert np.array_equal(got[2], want[2]), (name, cf)
            assert got[0].dtype == np.int32 and got[2].dtype == np.int32
            out[name, cf] = got
    # outputs are optional
    lib, best = mod._lib, np.zeros(N_GROUPS, dtype=np.int32)
    assert lib.orc_batch_select_best(mod._h, bid, N_GROUPS, None, 0, None, None, None) == 0
    assert lib.orc_batch_select_best(mod._h, bid, N_GROUPS, None, 1, best.ctypes.data_as(_capi.c_int_p), None, None) == 0
    assert np.array_equal(best, out["null", True][0])
    return costs, status, col, out


@pytest.mark.parametrize("shards", [1, 2])
def test_select_best_and_gather(wam, wam2, shards):
    mod, model = wam if shards == 1 else wam2
    rng = np.random.default_rng(5)
    goals, seeds = multistart_workload()
    bid = mod.batch_create(model.name, goals, **KW)
    mod.batch_perturb(bid, 0.3, seeds)
    mod.batch_iterate(bid, 100)
    costs, status, col, out = check_selection(mod, bid, rng)
    # the workload is not vacuous
    grp = contiguous_groups(N_RUNS, N_GROUPS)
    eligible_cf = ((status == 0) | (status == 1)) & np.isfinite(costs[:, 0]) & (col == 0)
    assert (status == -1).any(), "config 2's goals must give aborted runs"
    assert (col == 1).any() and (col == 0).any()
    assert col[-2 * K:-K].all(), "every run that ends in the table collides"
    on, off = out["contiguous", True], out["contiguous", False]
    assert (np.bincount(grp[eligible_cf], minlength=N_GROUPS) == 0).any() and (on[0] == -1).any()
    assert on[0][N_PROBLEMS] == -1 and on[1][N_PROBLEMS] == INF and on[2][N_PROBLEMS] == 0
    assert (on[0] != off[0]).any(), "the verdict must matter"      # (the group with a winner both ways, and another one: below)
    assert off[0][N_PROBLEMS] >= N_PROBLEMS * K
    assert (on[0] >= 0).sum() >= N_PROBLEMS // 2, "most problems must have a collision-free winner"
    # the tie: K identical runs, all eligible, the lowest index wins
    tie = np.arange(N_RUNS - K, N_RUNS)
    assert same(costs[tie], np.tile(costs[tie[0]], (K, 1))) and eligible_cf[tie].all(), (costs[tie], status[tie], col[tie])
    assert on[0][-1] == tie[0] and off[0][-1] == tie[0] and on[2][-1] == K
    # the perturbed starts of a problem are different runs
    assert len(np.unique(costs[:K, 0])) > 1

    # ---- 6. the gather
    full = mod.batch_gettraj(bid)
    assert same(mod.batch_gettraj_runs(bid, on[0]), np.where((on[0] >= 0)[:, None, None], full[np.maximum(on[0], 0)], np.nan))
    assert np.isnan(mod.batch_gettraj_runs(bid, on[0])[N_PROBLEMS]).all()
    assert same(mod.batch_gettraj_runs(bid, off[0]), full[off[0]])
    perm = rng.permutation(N_RUNS)
    assert same(mod.batch_gettraj_runs(bid, perm), full[perm])
    dup = np.array([3, 3, N_RUNS - 1, 0, 3, N_RUNS // 2, N_RUNS // 2 - 1, 0])
    assert same(mod.batch_gettraj_runs(bid, dup), full[dup])
    mixed = np.array([-1, 7, -1, N_RUNS - 1])
    got = mod.batch_gettraj_runs(bid, mixed)
    assert np.isnan(got[[0, 2]]).all() and same(got[[1, 3]], full[[7, N_RUNS - 1]])
    assert mod.batch_gettraj_runs(bid, []).shape == (0, KW["n_points"], 7)

    # ---- trajectories set through the table and evaluated with iterate(0): a certain collision, an empty group
    _, base, dofvals, _ = common.wam_state()
    start = np.asarray(dofvals[:7])
    through = start + np.linspace(0.0, 1.0, KW["n_points"])[:, None] * (np.asarray(IN_TABLE) - start)
    moved = full.copy()
    moved[:K] = through
    # the second group: its cheapest run goes through the table, the others are free of it but expensive (the wrist
    # roll alternates by 3 rad from waypoint to waypoint) -- a group with a winner both ways, and a different one
    moved[K] = through
    jitter = np.tile(start, (KW["n_points"], 1))
    jitter[1:-1:2, 6] += 1.5
    jitter[2:-1:2, 6] -= 1.5
    moved[K + 1:2 * K] = jitter
    mod.batch_set_traj(bid, moved)
    mod.batch_iterate(bid, 0)
    costs0, status0, col0, out0 = check_selection(mod, bid, rng)
    assert (status0 == 0).all() and col0[:K].all()
    assert out0["contiguous", True][0][0] == -1 and out0["contiguous", True][2][0] == 0
    assert out0["contiguous", False][0][0] == 0, "K identical runs: the first"
    assert col0[K] == 1 and not col0[K + 1:2 * K].any(), col0[K:2 * K]
    assert costs0[K, 0] < costs0[K + 1, 0], (costs0[K], costs0[K + 1])
    on0, off0 = out0["contiguous", True][0], out0["contiguous", False][0]
    assert off0[1] == K and on0[1] == K + 1
    assert ((on0 >= 0) & (off0 >= 0) & (on0 != off0)).any(), "a group must have a winner both ways, and a different one"
    mod.batch_destroy(bid)


def test_shards_agree(wam, wam2):
    """the two-shard module selects what the one-device module selects: groups that span the shards included"""
    res = []
    rng = np.random.default_rng(6)
    grp = rng.permutation(contiguous_groups(N_RUNS, N_GROUPS)).astype(np.int32)
    for mod, model in (wam, wam2):
        goals, seeds = multistart_workload()
        bid = mod.batch_create(model.name, goals, **KW)
        mod.batch_perturb(bid, 0.3, seeds)
        mod.batch_iterate(bid, 50)
        res.append([mod.batch_select_best(bid, groups=grp, n_groups=N_GROUPS, collision_free=cf) for cf in (True, False)])
        mod.batch_destroy(bid)
    for a, b in zip(*res):
        assert np.array_equal(a[0], b[0]) and same(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert (res[0][1][0] >= 0).all()


def test_an_exact_tie_across_the_shards(wam2):
    """four identical runs, two on each shard: every key the shards report is the same, so the winner is the merge's own
    rule (the lower key, then the lower run), for select_best and select_clear, one group and two interleaved ones"""
    mod, model = wam2
    goals, _ = multistart_workload()
    bid = mod.batch_create(model.name, np.tile(goals[TIE_GOAL], (4, 1)), **KW)
    costs, status = mod.batch_iterate(bid, 0)
    assert same(costs, np.tile(costs[0], (4, 1))) and (status == 0).all(), (costs, status)
    assert not mod.batch_collision_verdict(bid)["collides"].any()
    clear = mod.batch_clearance(bid)["clearance"]
    assert same(clear, np.tile(clear[0], (4, 1)))
    interleaved = np.array([1, 0, 1, 0], dtype=np.int32)
    for grp, runs, n_eligible in ((None, [0], [4]), (interleaved, [1, 0], [2, 2])):
        for column, by in enumerate(("total", "obs", "smooth")):
            for cf in (False, True):
                got = mod.batch_select_best(bid, groups=grp, n_groups=len(runs), collision_free=cf, by=by)
                assert np.array_equal(got[0], runs) and np.array_equal(got[2], n_eligible), (by, cf, got)
                assert same(got[1], np.full(len(runs), costs[0, column])), (by, cf, got)
        for by in ("total", "obs", "smooth", "clearance"):
            got = mod.batch_select_clear(bid, groups=grp, n_groups=len(runs), margin=-INF, by=by)
            assert np.array_equal(got[0], runs) and np.array_equal(got[3], n_eligible), (by, got)
            assert same(got[2], np.full(len(runs), clear[0].min())), (by, got)
    mod.batch_destroy(bid)


# ---- 7. errors -------------------------------------------------------------------------------------------------------

def rejected(mod, rc):
    assert rc == 1
    msg = mod._lib.orc_last_error(mod._h).decode()
    assert msg, "a rejected call leaves a message"
    return msg


def test_rejected_arguments(wam):
    mod, model = wam
    lib, h = mod._lib, mod._h
    n_runs = 12
    goals = common.wam_goals(n_runs, seed=35)
    seeds = np.arange(n_runs, dtype=np.uint32) + 1
    sp = seeds.ctypes.data_as(_capi.c_uint_p)
    bid = mod.batch_create(model.name, goals, **KW)
    before = mod.batch_gettraj(bid)
    for sigma in (float("nan"), -0.1, INF, -INF):
        assert "sigma" in rejected(mod, lib.orc_batch_perturb(h, bid, sigma, sp))
    assert "seeds" in rejected(mod, lib.orc_batch_perturb(h, bid, 0.1, None))
    rejected(mod, lib.orc_batch_perturb(h, bid + 1000, 0.1, sp))
    # select_best before any iterate call; then its arguments
    best = np.zeros(n_runs, dtype=np.int32)
    bp = best.ctypes.data_as(_capi.c_int_p)
    assert "iterated" in rejected(mod, lib.orc_batch_select_best(h, bid, 1, None, 0, bp, None, None))
    assert same(mod.batch_gettraj(bid), before), "a rejected call leaves the trajectories alone"
    mod.batch_perturb(bid, 0.1, seeds)                       # the next valid call succeeds
    after = mod.batch_gettraj(bid)
    assert not same(after, before)
    mod.batch_iterate(bid, 0)
    grp = np.zeros(n_runs, dtype=np.int32)
    for bad in (-1, 3):
        grp[5] = bad
        for cf in (0, 1):
            assert "group_of_run" in rejected(mod, lib.orc_batch_select_best(h, bid, 3, grp.ctypes.data_as(_capi.c_int_p), cf, bp, None, None))
    assert "multiple" in rejected(mod, lib.orc_batch_select_best(h, bid, 5, None, 0, bp, None, None))
    assert "n_groups" in rejected(mod, lib.orc_batch_select_best(h, bid, 0, None, 0, bp, None, None))
    rejected(mod, lib.orc_batch_select_best(h, bid + 1000, 1, None, 0, bp, None, None))
    assert mod.batch_select_best(bid, n_groups=3, collision_free=False)[2].sum() == n_runs
    # gettraj_runs
    out = np.zeros((2, KW["n_points"], 7))
    op = out.ctypes.data_as(_capi.c_double_p)
    for bad in (-2, n_runs):
        runs = np.array([-1, bad], dtype=np.int32)
        out[:] = 7.0
        assert "range" in rejected(mod, lib.orc_batch_gettraj_runs(h, bid, runs.ctypes.data_as(_capi.c_int_p), 2, op, out.size))
        assert (out == 7.0).all(), "a rejected call writes nothing (not even the NaN row of the -1 in front)"
    runs = np.array([0, 1], dtype=np.int32)
    rp = runs.ctypes.data_as(_capi.c_int_p)
    rejected(mod, lib.orc_batch_gettraj_runs(h, bid, None, 2, op, out.size))
    rejected(mod, lib.orc_batch_gettraj_runs(h, bid, rp, 2, None, out.size))
    assert "small" in rejected(mod, lib.orc_batch_gettraj_runs(h, bid, rp, 2, op, out.size - 1))
    rejected(mod, lib.orc_batch_gettraj_runs(h, bid + 1000, rp, 2, op, out.size))
    assert lib.orc_batch_gettraj_runs(h, bid, rp, 2, op, out.size) == 0
    assert same(out, after[:2])
    assert same(mod.batch_gettraj(bid), after)
    mod.batch_destroy(bid)


def test_rejected_batches(wam):
    """batches the perturbation is not defined for: rejected, the batch unchanged and usable"""
    mod, model = wam
    n_runs = 4
    goals = common.wam_goals(n_runs, seed=36)
    seeds = np.arange(n_runs, dtype=np.uint32) + 1
    _, base, dofvals, _ = common.wam_state()
    # the hand keeps its position while the start configuration moves (the start_tsr of test_gpu_tsr.py)
    R, t = model.link_frames(base, dofvals)
    li = model.link_names.index("handbase")
    tsr = robots.Tsr(T0w_R=R[li], T0w_d=t[li] + R[li] @ np.array([0.0, 0.0, 0.16]), Bw=[[0, 0]] * 3 + [[-3, 3]] * 3)
    near = np.array(robots.WAM_START)[None, :] + 0.3 * np.random.default_rng(11).uniform(-1, 1, size=(n_runs, 7))
    made = [
        ("floating", mod.batch_create(model.name, goals, basegoals=np.tile(base, (n_runs, 1)), **dict(KW, n_points=30, floating_base=1))),
        ("start_tsr", int(mod.SendCommand("createbatch robot %s n_runs %d adofgoals 0x%x n_points 30 lambda 100 obs_factor 200 start_tsr '%s'"
                                          % (model.name, n_runs, near.ctypes.data, tsr.serialize())))),
        ("dense", mod.batch_create(model.name, goals, **dict(KW, n_points=30, derivative=5))),
        ("dense", mod.batch_create(model.name, goals, **dict(KW, n_points=6, derivative=2))),      # too few waypoints for the generators
    ]
    for word, bid in made:
        before = mod.batch_gettraj(bid)
        rc = mod._lib.orc_batch_perturb(mod._h, bid, 0.1, seeds.ctypes.data_as(_capi.c_uint_p))
        assert word in rejected(mod, rc), word
        assert same(mod.batch_gettraj(bid), before)
        costs, status = mod.batch_iterate(bid, 2)             # the batch is usable
        assert np.isfinite(costs).all()
        mod.batch_destroy(bid)
    # ... and so is the module
    bid = mod.batch_create(model.name, goals, **dict(KW, derivative=4))
    before = mod.batch_gettraj(bid)
    mod.batch_perturb(bid, 0.1, seeds)
    assert not same(mod.batch_gettraj(bid), before)
    mod.batch_destroy(bid)
