"""-m gpu: orc_batch_respawn / Module.batch_respawn on the WAM tabletop.  The device's plan is held to the pure specification
or_cdchomp_amd.module.respawn_plan of the batch's own read-backs, and its trajectories to the module's other entry points: a
respawned batch is the batch given the sources' rows (or the straight line) through batch_set_traj and perturbed by
batch_perturb, with the survivors left as they were.  Every comparison is an integer or a bitwise equality."""
import numpy as np
import pytest

import common
import or_cdchomp_amd
from or_cdchomp_amd import _capi, robots
from or_cdchomp_amd.module import contiguous_groups, respawn_plan

pytestmark = pytest.mark.gpu

KW = dict(common.CONFIG2_KW)                     # n_points 100, lambda 100, obs_factor 500
IN_TABLE = [1.2, -0.2, 0.0, 0.3, 0.0, 0.0, 0.0]    # a configuration with the forearm in the table top
K = 8
N_PROBLEMS = 30          # config 2's own goals, K perturbed starts each; then a group that ends in the table and a group of identical runs
N_GROUPS = N_PROBLEMS + 2
N_RUNS = N_GROUPS * K
MODES = ("ignore", "require", "prefer")


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


def multistart_workload():
    """the workload of test_gpu_multistart.py: 32 groups of K = 8"""
    base = common.wam_goals(N_PROBLEMS + 1, seed=20250101)
    goals = np.repeat(base[:N_PROBLEMS], K, axis=0)
    goals = np.concatenate([goals, np.tile(IN_TABLE, (K, 1)), np.tile(base[N_PROBLEMS], (K, 1))])
    seeds = np.arange(N_RUNS, dtype=np.uint32) + 9000
    seeds[-K:] = 77                                          # the last group: K identical runs, a K-fold tie
    return goals, seeds


RESPAWN_SEEDS = (np.arange(N_RUNS, dtype=np.uint32) * 31 + 5).astype(np.uint32)


def build(mod, model, **kw):
    """the workload after its 100 iterations: a respawn consumes the batch, so every case builds its own"""
    goals, seeds = multistart_workload()
    bid = mod.batch_create(model.name, goals, **dict(KW, **kw))
    mod.batch_perturb(bid, 0.3, seeds)
    mod.batch_iterate(bid, 100)
    return bid


_READBACKS = {}


def readbacks(mod, model, **kw):
    """costs, status, verdict, trajectories and "AG" of build(**kw), read once and left unchanged (a batch built again
    holds the same bits: test_gpu_multistart.py::test_perturbed_batch_is_the_batch_given_those_trajectories)"""
    key = tuple(sorted(kw.items()))
    if key not in _READBACKS:
        bid = build(mod, model, **kw)
        costs, status = mod.batch_sync(bid)
        col = mod.batch_collision_verdict(bid)["collides"]
        out = dict(costs=costs, status=status, col=col, traj=mod.batch_gettraj(bid), AG=mod.batch_state(bid, "AG"))
        mod.batch_destroy(bid)
        for v in out.values():
            v.setflags(write=False)
        _READBACKS[key] = out
    return _READBACKS[key]


def candidates(rb, mode):
    ok = ((rb["status"] == 0) | (rb["status"] == 1)) & np.isfinite(rb["costs"][:, 0])
    return ok & (rb["col"] == 0) if mode == 1 else ok


def test_the_workload_is_not_vacuous(wam):
    mod, model = wam
    rb = readbacks(mod, model)
    costs, status, col = rb["costs"], rb["status"], rb["col"]
    assert (status == -1).any(), "config 2's goals must give aborted runs"
    assert (col == 1).any() and (col == 0).any()
    assert col[-2 * K:-K].all(), "every run that ends in the table collides"
    assert candidates(rb, 0)[-2 * K:-K].any(), "... so the group is empty under mode 1 only"
    tie = np.arange(N_RUNS - K, N_RUNS)
    assert same(costs[tie], np.tile(costs[tie[0]], (K, 1))) and candidates(rb, 1)[tie].all()
    assert len(np.unique(costs[:K, 0])) > 1
    grp = contiguous_groups(N_RUNS, N_GROUPS)
    per_group = np.bincount(grp[candidates(rb, 1)], minlength=N_GROUPS)
    assert (per_group == 0).any() and (per_group == K).any() and ((per_group > 0) & (per_group < K)).any()
    # mode 2 differs from mode 0 and from mode 1 somewhere
    plans = [respawn_plan(costs, status, col, grp, N_GROUPS, 3, mode=m)[0] for m in (0, 1, 2)]
    assert (plans[0] != plans[2]).any() and (plans[1] != plans[2]).any()


# ---- 1. the plan against the specification ---------------------------------------------------------------------------

@pytest.mark.parametrize("groups", ["contiguous", "shuffled", "null"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_plan_matches_the_specification(wam, mode, groups):
    mod, model = wam
    rb = readbacks(mod, model)
    contiguous = contiguous_groups(N_RUNS, N_GROUPS)
    grp = np.random.default_rng(5).permutation(contiguous).astype(np.int32) if groups == "shuffled" else contiguous
    for keep in (1, 3, K, K + 5):
        for column in (0, 2):
            bid = build(mod, model)
            src, cnt = mod.batch_respawn(bid, keep, 0.0, None, groups=None if groups == "null" else grp, n_groups=N_GROUPS,
                                         collision=MODES[mode], by=("total", "obs", "smooth")[column])
            costs, status = mod.batch_sync(bid)
            mod.batch_destroy(bid)
            assert same(costs, rb["costs"]) and np.array_equal(status, rb["status"]), "a respawn leaves costs and status"
            want = respawn_plan(rb["costs"], rb["status"], rb["col"], grp, N_GROUPS, keep, mode=mode, column=column)
            assert src.dtype == np.int32 and cnt.dtype == np.int32
            assert np.array_equal(src, want[0]), (keep, column, src, want[0])
            assert np.array_equal(cnt, want[1]), (keep, column, cnt, want[1])
            if groups != "shuffled":
                tie = np.arange(N_RUNS - K, N_RUNS)
                assert np.array_equal(np.flatnonzero(src[tie] == tie), np.arange(min(keep, K))), "the tie keeps its first `keep` indices"
                table = np.arange(N_RUNS - 2 * K, N_RUNS - K)
                if mode == 1:
                    assert (src[table] == -1).all() and cnt[N_PROBLEMS] == 0
                else:
                    assert (src[table] >= 0).any()


# ---- 2. large, uneven groups -----------------------------------------------------------------------------------------

def uneven_batch(mod, model, sizes, iters=20):
    n_runs = int(np.sum(sizes))
    goals = common.wam_goals(n_runs, seed=77)
    seeds = (np.arange(n_runs, dtype=np.uint32) * 7 + 1).astype(np.uint32)
    goals[10:40] = goals[10]; seeds[10:40] = seeds[10]      # a 30-fold tie inside the first group
    goals[3] = IN_TABLE
    bid = mod.batch_create(model.name, goals, **dict(KW, n_points=10))
    mod.batch_perturb(bid, 0.3, seeds)
    mod.batch_iterate(bid, iters)
    return bid, np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)


@pytest.mark.parametrize("keep", [1, 5, 70])
def test_large_uneven_groups(wam, keep):
    """one group of 300 runs (five passes of a wavefront's 64 lanes, the last one partial; with keep 70 the survivors fill
    more than one step of the final walk), then groups of 1, 63, 64 and 65 runs"""
    mod, model = wam
    sizes = [300, 1, 63, 64, 65]
    bid, grp = uneven_batch(mod, model, sizes)
    costs, status = mod.batch_sync(bid)
    col = mod.batch_collision_verdict(bid)["collides"]
    before = mod.batch_gettraj(bid)
    assert same(costs[10:40], np.tile(costs[10], (30, 1))), "the tie"
    assert col.any() and not col.all()
    src, cnt = mod.batch_respawn(bid, keep, 0.0, None, groups=grp, n_groups=len(sizes), collision="prefer")
    after = mod.batch_gettraj(bid)
    mod.batch_destroy(bid)
    want = respawn_plan(costs, status, col, grp, len(sizes), keep, mode=2)
    assert np.array_equal(src, want[0]) and np.array_equal(cnt, want[1])
    assert cnt[0] == min(keep, int(((status >= 0) & np.isfinite(costs[:, 0]))[:300].sum()))
    # sigma 0: copies only, and both ends of every run stay
    assert (src[:300] >= 0).all() and (src[:300] != np.arange(300)).sum() == 300 - cnt[0]
    assert same(after, spec_base(before, src))


def test_the_largest_group_and_one_run_more(wam):
    """4 096 runs in one group are ranked (the bound in the header); 4 097 are rejected before any device work"""
    mod, model = wam
    bid, _ = uneven_batch(mod, model, [4097], iters=5)
    costs, status = mod.batch_sync(bid)
    before = mod.batch_gettraj(bid)
    rc = mod._lib.orc_batch_respawn(mod._h, bid, 0, 1, None, 0, 100, 0.0, None, None, None)
    assert "4096" in rejected(mod, rc)
    assert same(mod.batch_gettraj(bid), before)
    grp = np.zeros(4097, dtype=np.int32); grp[-1] = 1
    src, cnt = mod.batch_respawn(bid, 100, 0.0, None, groups=grp, n_groups=2, collision="ignore")
    mod.batch_destroy(bid)
    want = respawn_plan(costs, status, None, grp, 2, 100, mode=0)
    assert np.array_equal(src, want[0]) and np.array_equal(cnt, want[1])
    assert cnt[0] == 100 and cnt[1] == 1


# ---- 3. the trajectories ---------------------------------------------------------------------------------------------

def spec_base(before, src):
    """what every run is before its perturbation: its own rows (a survivor), its source's moving rows, or the line"""
    n_points = before.shape[1]
    base = before.copy()
    for r, s in enumerate(src):
        if s >= 0:
            base[r, 1:-1] = before[s, 1:-1]
        else:
            first, last = before[r, 0], before[r, -1]
            for i in range(1, n_points - 1):
                base[r, i] = first + (last - first) * i / (n_points - 1)
    return base


@pytest.mark.parametrize("kw", [dict(), dict(precision=32), dict(derivative=2)], ids=["fp64", "fp32", "derivative2"])
def test_respawned_batch_is_the_batch_given_those_trajectories(wam, kw):
    mod, model = wam
    rb = readbacks(mod, model, **kw)
    before = rb["traj"]
    a = build(mod, model, **kw)
    src, cnt = mod.batch_respawn(a, 3, 0.3, RESPAWN_SEEDS, n_groups=N_GROUPS, collision="require")
    want = respawn_plan(rb["costs"], rb["status"], rb["col"], contiguous_groups(N_RUNS, N_GROUPS), N_GROUPS, 3, mode=1)
    assert np.array_equal(src, want[0]) and np.array_equal(cnt, want[1])
    survivor = src == np.arange(N_RUNS)
    clone = (src >= 0) & ~survivor
    assert survivor.any() and clone.any() and (src == -1).any()
    after = mod.batch_gettraj(a)
    assert same(after[survivor], before[survivor]), "not one bit of a survivor changes"
    # the second batch: the same runs, given the base trajectories, perturbed with the same seeds, the survivors put back
    b = build(mod, model, **kw)
    mod.batch_set_traj(b, spec_base(before, src))
    mod.batch_perturb(b, 0.3, RESPAWN_SEEDS)
    spliced = mod.batch_gettraj(b)
    assert not same(spliced[survivor], before[survivor]), "batch_perturb moves every run"
    spliced[survivor] = before[survivor]
    assert same(after, spliced)
    assert np.abs(after[~survivor] - spec_base(before, src)[~survivor]).max() > 0.05, "the other runs are displaced"
    mod.batch_set_traj(b, spliced)
    ca, sa = mod.batch_iterate(a, 20)
    cb, sb = mod.batch_iterate(b, 20)
    ta, tb = mod.batch_gettraj(a), mod.batch_gettraj(b)
    mod.batch_destroy(a); mod.batch_destroy(b)
    assert np.abs(ta - after).max() > 1e-3, "the runs must have moved"
    assert same(ta, tb) and same(ca, cb) and np.array_equal(sa, sb)


# ---- 4. momentum -----------------------------------------------------------------------------------------------------

def test_momentum_follows_the_source(wam):
    mod, model = wam
    kw = dict(use_momentum=1)
    rb = readbacks(mod, model, **kw)
    assert np.abs(rb["AG"]).max() > 0.0
    fresh = mod.batch_create(model.name, multistart_workload()[0], **dict(KW, **kw))
    AG0 = mod.batch_state(fresh, "AG")
    mod.batch_destroy(fresh)
    a = build(mod, model, **kw)
    src, cnt = mod.batch_respawn(a, 2, 0.0, None, n_groups=N_GROUPS, collision="require")
    survivor = src == np.arange(N_RUNS)
    clone = (src >= 0) & ~survivor
    line = src == -1
    assert survivor.any() and clone.any() and line.any()
    AG = mod.batch_state(a, "AG")
    assert same(AG[survivor], rb["AG"][survivor])
    assert same(AG[clone], rb["AG"][src[clone]])
    assert not same(AG[clone], rb["AG"][clone])
    assert same(AG[line], AG0[line])
    traj = mod.batch_gettraj(a)
    assert same(traj[clone][:, 1:-1], rb["traj"][src[clone]][:, 1:-1])
    # a clone is its source from here on: the same problem and scene, the same trajectory, momentum and leapfrog_first
    mod.batch_iterate(a, 10)
    later = mod.batch_gettraj(a)
    mod.batch_destroy(a)
    assert np.abs(later[clone] - traj[clone]).max() > 1e-6, "the runs must have moved"
    assert same(later[clone], later[src[clone]])
    # a restarted run is a run of a fresh batch (zero momentum, leapfrog_first 1) that was given its line.  (Not the fresh
    # batch's own line: create interpolates between the caller's start and goal, a respawn between the run's stored end
    # rows, and the stored last row is s + (g - s), which need not be g to the last bit.)
    fresh = mod.batch_create(model.name, multistart_workload()[0], **dict(KW, **kw))
    mod.batch_set_traj(fresh, traj)
    mod.batch_iterate(fresh, 10)
    want = mod.batch_gettraj(fresh)
    mod.batch_destroy(fresh)
    assert same(later[line], want[line])
    assert not same(later[clone], want[clone]), "... which a clone, with its source's momentum, is not"


# ---- 5. a respawn that has nothing to do -----------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(), dict(use_momentum=1)], ids=["plain", "momentum"])
def test_keep_at_the_group_size_changes_no_bit_of_a_group_of_candidates(wam, kw):
    """without momentum the workload has aborted runs, so some groups are respawned next to those that are left alone; with
    momentum (where leapfrog_first matters) every run of it is a candidate and the whole call must change nothing"""
    mod, model = wam
    rb = readbacks(mod, model, **kw)
    grp = contiguous_groups(N_RUNS, N_GROUPS)
    whole = np.bincount(grp[candidates(rb, 0)], minlength=N_GROUPS) == K
    assert whole.any() and (kw or not whole.all())
    a = build(mod, model, **kw)
    src, cnt = mod.batch_respawn(a, K, 0.3, RESPAWN_SEEDS, n_groups=N_GROUPS, collision="ignore")
    traj, AG = mod.batch_gettraj(a), mod.batch_state(a, "AG")
    mod.batch_iterate(a, 5)
    later = mod.batch_gettraj(a)
    mod.batch_destroy(a)
    b = build(mod, model, **kw)
    mod.batch_iterate(b, 5)
    untouched = mod.batch_gettraj(b)
    mod.batch_destroy(b)
    runs = whole[grp]
    assert np.array_equal(src[runs], np.arange(N_RUNS)[runs]) and (cnt[whole] == K).all()
    assert same(traj[runs], rb["traj"][runs]) and same(AG[runs], rb["AG"][runs])
    assert same(later[runs], untouched[runs]), "... nor does leapfrog_first"
    assert runs.all() or not same(traj[~runs], rb["traj"][~runs])


# ---- 6. shards -------------------------------------------------------------------------------------------------------

def test_two_shards_give_the_bits_of_one(wam, wam2):
    mod, model = wam
    mod2, _ = wam2
    res = []
    for m_ in (mod, mod2):
        bid = build(m_, model)
        src, cnt = m_.batch_respawn(bid, 3, 0.3, RESPAWN_SEEDS, n_groups=N_GROUPS, collision="prefer")
        res.append((src, cnt, m_.batch_gettraj(bid), m_.batch_state(bid, "AG")))
        m_.batch_destroy(bid)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert same(res[0][2], res[1][2]) and same(res[0][3], res[1][3])
    assert (res[0][0][N_RUNS // 2:] >= N_RUNS // 2).all(), "the second shard's sources are reported as runs of the batch"
    # a group that spans the boundary between the shards (runs 124 .. 131)
    bid = build(mod2, model)
    before = mod2.batch_gettraj(bid)
    grp = ((np.arange(N_RUNS) + 4) // K % N_GROUPS).astype(np.int32)
    rc = mod2._lib.orc_batch_respawn(mod2._h, bid, 0, N_GROUPS, grp.ctypes.data_as(_capi.c_int_p), 0, 3, 0.0, None, None, None)
    assert "shard" in rejected(mod2, rc)
    assert same(mod2.batch_gettraj(bid), before)
    # ... is no problem on one device
    rb = readbacks(mod, model)
    one = build(mod, model)
    src, cnt = mod.batch_respawn(one, 3, 0.0, None, groups=grp, n_groups=N_GROUPS, collision="ignore")
    mod.batch_destroy(one)
    want = respawn_plan(rb["costs"], rb["status"], None, grp, N_GROUPS, 3, mode=0)
    assert np.array_equal(src, want[0]) and np.array_equal(cnt, want[1])
    # the batch is usable: groups inside the shards
    src, cnt = mod2.batch_respawn(bid, 3, 0.0, None, n_groups=N_GROUPS, collision="ignore")
    mod2.batch_destroy(bid)
    want = respawn_plan(rb["costs"], rb["status"], None, contiguous_groups(N_RUNS, N_GROUPS), N_GROUPS, 3, mode=0)
    assert np.array_equal(src, want[0]) and np.array_equal(cnt, want[1])


# ---- 7. rejections ---------------------------------------------------------------------------------------------------

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
    mod.batch_perturb(bid, 0.2, seeds)
    before = mod.batch_gettraj(bid)
    src = np.zeros(n_runs, dtype=np.int32); cnt = np.zeros(n_runs, dtype=np.int32)
    out = (src.ctypes.data_as(_capi.c_int_p), cnt.ctypes.data_as(_capi.c_int_p))

    def call(bid_=None, column=0, n_groups=3, grp=None, mode=2, keep=2, sigma=0.1, seeds_=sp):
        return lib.orc_batch_respawn(h, bid if bid_ is None else bid_, column, n_groups,
                                     None if grp is None else grp.ctypes.data_as(_capi.c_int_p), mode, keep, sigma, seeds_, *out)

    assert "iterated" in rejected(mod, call())                # a batch that has not been iterated
    mod.batch_iterate(bid, 0)
    rejected(mod, call(bid_=bid + 1000))
    for column in (-1, 3):
        assert "cost_column" in rejected(mod, call(column=column))
    for mode in (-1, 3):
        assert "collision_mode" in rejected(mod, call(mode=mode))
    for keep in (0, -1):
        assert "keep" in rejected(mod, call(keep=keep))
    grp = np.zeros(n_runs, dtype=np.int32)
    for bad in (-1, 3):
        grp[5] = bad
        assert "group_of_run" in rejected(mod, call(grp=grp))
    assert "multiple" in rejected(mod, call(n_groups=5))
    assert "n_groups" in rejected(mod, call(n_groups=0))
    for sigma in (float("nan"), -0.1, float("inf"), -float("inf")):
        assert "sigma" in rejected(mod, call(sigma=sigma))
    assert "seeds" in rejected(mod, call(seeds_=None))
    assert same(mod.batch_gettraj(bid), before), "a rejected call leaves the trajectories alone"
    assert (src == 0).all() and (cnt == 0).all(), "... and its outputs"
    # the batch is still iterated and usable: the outputs may be NULL, sigma 0 needs no seeds
    assert lib.orc_batch_respawn(h, bid, 0, 3, None, 2, 2, 0.0, None, None, None) == 0
    # ... and now it is respawned: select_best and another respawn wait for an iterate call
    best = np.zeros(3, dtype=np.int32)
    bp = best.ctypes.data_as(_capi.c_int_p)
    assert "iterated" in rejected(mod, lib.orc_batch_select_best(h, bid, 3, None, 0, bp, None, None))
    assert "iterated" in rejected(mod, lib.orc_batch_select_best_by(h, bid, 2, 3, None, 0, bp, None, None))
    assert "iterated" in rejected(mod, call())
    mod.batch_iterate(bid, 0)
    assert lib.orc_batch_select_best(h, bid, 3, None, 0, bp, None, None) == 0
    assert call() == 0
    assert (cnt[:3] >= 1).all() and (cnt[:3] <= 2).all() and (src >= 0).all()
    mod.batch_destroy(bid)


def test_rejected_batches(wam):
    """the batches orc_batch_perturb rejects are rejected whatever sigma is: the batch unchanged and usable"""
    mod, model = wam
    n_runs = 4
    goals = common.wam_goals(n_runs, seed=36)
    seeds = np.arange(n_runs, dtype=np.uint32) + 1
    _, base, dofvals, _ = common.wam_state()
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
        mod.batch_iterate(bid, 2)
        before = mod.batch_gettraj(bid)
        for sigma in (0.0, 0.1):
            rc = mod._lib.orc_batch_respawn(mod._h, bid, 0, 1, None, 0, 1, sigma, seeds.ctypes.data_as(_capi.c_uint_p), None, None)
            assert word in rejected(mod, rc), word
        assert same(mod.batch_gettraj(bid), before)
        costs, status = mod.batch_iterate(bid, 2)             # the batch is usable
        assert np.isfinite(costs).all()
        mod.batch_destroy(bid)


def test_rejected_long_runs():
    """the 30-dof tree with 700 waypoints in fp32: 20 940 Gaussians per run, over the perturbation's LDS bound"""
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_tree30(mod)
    goals = common.config5_goals(3)
    bid = mod.batch_create(model.name, goals, **dict(common.CONFIG5_KW, n_points=700, precision=32))
    mod.batch_iterate(bid, 0)
    before = mod.batch_gettraj(bid)
    for sigma in (0.0, 0.1):
        rc = mod._lib.orc_batch_respawn(mod._h, bid, 0, 1, None, 0, 1, sigma, np.arange(3, dtype=np.uint32).ctypes.data_as(_capi.c_uint_p), None, None)
        assert "LDS" in rejected(mod, rc)
    assert same(mod.batch_gettraj(bid), before)
    mod.batch_destroy(bid)
    mod.close()
