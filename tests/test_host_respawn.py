"""CPU: the specification of orc_batch_respawn (or_cdchomp_amd.module.respawn_plan, what the -m gpu tests in
test_gpu_respawn.py hold the device's plan to) on hand-made and on random tables, and the symbol."""
import ctypes as C
import os

import numpy as np

from or_cdchomp_amd import _capi
from or_cdchomp_amd.module import cost_key, respawn_plan, select_best

INF = float("inf")
NAN = float("nan")


def plan(costs, status, collides, group, n_groups, keep, mode=2, column=0):
    src, cnt = respawn_plan(costs, status, collides, group, n_groups, keep, mode=mode, column=column)
    assert src.dtype == np.int32 and cnt.dtype == np.int32
    return src.tolist(), cnt.tolist()


# ---- hand-made tables ------------------------------------------------------------------------------------------------

def test_order_ties_and_the_round_robin_of_the_copies():
    #        run   0    1    2    3    4    5    6
    costs = [5.0, 3.0, 3.0, 4.0, 9.0, 1.0, 8.0]
    grp = [0] * 7
    # keep 2: the survivors are runs 5 (rank 0) and 1 (rank 1: the tie with run 2 goes to the lower index); the other runs
    # 0, 2, 3, 4, 6 in ascending order get ranks 0, 1, 0, 1, 0: the best survivor receives the most copies
    assert plan(costs, [0] * 7, None, grp, 1, 2, mode=0) == ([5, 1, 1, 5, 1, 5, 5], [2])
    assert plan(costs, [0] * 7, None, grp, 1, 1, mode=0) == ([5, 5, 5, 5, 5, 5, 5], [1])
    assert plan(costs, [0] * 7, None, grp, 1, 3, mode=0) == ([5, 1, 2, 1, 2, 5, 5], [3])
    # interleaved groups: the tie and the order are by run index, not by position in the group's list
    src, cnt = plan([3.0, 2.0, 3.0, 2.0, 1.0, 7.0], [0] * 6, None, [1, 0, 1, 0, 1, 0], 2, 1, mode=0)
    assert cnt == [1, 1] and src == [4, 1, 4, 1, 4, 1]


def test_minus_zero_ties_with_plus_zero():
    assert cost_key(-0.0) == cost_key(0.0)
    assert cost_key(-1.0) < cost_key(-0.0) < cost_key(5e-324) < cost_key(1.0) < cost_key(INF)
    assert cost_key(-INF) < cost_key(-1.0)
    # run 0 holds +0 and run 1 holds -0: a tie, so the lower index survives, whichever sign it carries
    assert plan([0.0, -0.0, 1.0], [0] * 3, None, [0] * 3, 1, 1, mode=0) == ([0, 0, 0], [1])
    assert plan([-0.0, 0.0, 1.0], [0] * 3, None, [0] * 3, 1, 1, mode=0) == ([0, 0, 0], [1])
    assert plan([1.0, 0.0, -0.0], [0] * 3, None, [0] * 3, 1, 1, mode=0) == ([1, 1, 1], [1])
    # a negative cost comes before both zeros: run 2 has rank 0, run 0 rank 1, and the only other run copies rank 0
    assert plan([0.0, -0.0, -1e-300], [0] * 3, None, [0] * 3, 1, 2, mode=0) == ([0, 2, 2], [2])


def test_keep_at_or_above_the_group_size():
    costs = [4.0, 2.0, 3.0]
    for keep in (3, 4, 1000):
        assert plan(costs, [0, 1, 0], None, [0] * 3, 1, keep, mode=0) == ([0, 1, 2], [3])
    # ... of which one run is no candidate: it becomes a copy of the best
    assert plan(costs, [0, 1, -1], None, [0] * 3, 1, 5, mode=0) == ([0, 1, 1], [2])


def test_a_non_candidate_is_never_a_source():
    #        run    0     1    2    3    4
    costs = [0.5, NAN, INF, 1.0, 2.0]
    status = [-1, 0, 0, 0, 1]
    # the cheapest run aborted, the next two have no finite total: runs 3 and 4 are all there is
    src, cnt = plan(costs, status, None, [0] * 5, 1, 4, mode=0)
    assert cnt == [2] and src == [3, 4, 3, 3, 4]
    # the TOTAL decides who is a candidate, whatever the column
    rows = [[INF, 0.0, 0.0], [5.0, 4.0, 1.0], [6.0, 1.0, 5.0]]
    assert plan(rows, [0] * 3, None, [0] * 3, 1, 1, mode=0, column=2) == ([1, 1, 1], [1])
    assert plan(rows, [0] * 3, None, [0] * 3, 1, 1, mode=0, column=1) == ([2, 2, 2], [1])


def test_mode_2_ranks_colliding_runs_last_and_mode_1_drops_them():
    costs = [1.0, 2.0, 3.0, 4.0]
    col = [1, 0, 1, 0]
    st = [0] * 4
    assert plan(costs, st, col, [0] * 4, 1, 3, mode=0) == ([0, 1, 2, 0], [3])
    assert plan(costs, st, None, [0] * 4, 1, 3, mode=0) == ([0, 1, 2, 0], [3])
    # mode 1: the candidates are runs 1 and 3
    assert plan(costs, st, col, [0] * 4, 1, 3, mode=1) == ([1, 1, 3, 3], [2])
    # mode 2: the order is 1, 3 (free), then 0, 2 (colliding)
    assert plan(costs, st, col, [0] * 4, 1, 3, mode=2) == ([0, 1, 1, 3], [3])
    assert plan(costs, st, col, [0] * 4, 1, 1, mode=2) == ([1, 1, 1, 1], [1])
    # every run collides: mode 2 still has survivors, mode 1 has none
    assert plan(costs, st, [1] * 4, [0] * 4, 1, 2, mode=2) == ([0, 1, 0, 1], [2])
    assert plan(costs, st, [1] * 4, [0] * 4, 1, 2, mode=1) == ([-1] * 4, [0])
    # mode 1's candidates are select_best's eligible runs, and its best survivor is select_best's winner
    best, _, cnt = select_best(costs, st, col, [0] * 4, 1)
    src, kept = plan(costs, st, col, [0] * 4, 1, 100, mode=1)
    assert kept == cnt.tolist() and src[best[0]] == best[0]


def test_a_group_without_a_survivor_is_minus_one_throughout():
    # group 0 has a survivor, group 1 has no run at all, group 2 only runs that are no candidates
    src, cnt = plan([1.0, 2.0, NAN, 3.0], [0, -1, 0, 0], [0, 0, 0, 1], [0, 2, 2, 2], 3, 2, mode=1)
    assert cnt == [1, 0, 0] and src == [0, -1, -1, -1]


def test_a_column_other_than_total():
    rows = [[9.0, 8.0, 1.0], [5.0, 2.0, 3.0], [7.0, 1.0, 6.0]]
    assert plan(rows, [0] * 3, None, [0] * 3, 1, 1, mode=0, column=0) == ([1, 1, 1], [1])
    assert plan(rows, [0] * 3, None, [0] * 3, 1, 1, mode=0, column=1) == ([2, 2, 2], [1])
    assert plan(rows, [0] * 3, None, [0] * 3, 1, 1, mode=0, column=2) == ([0, 0, 0], [1])
    assert plan(rows, [0] * 3, None, [0] * 3, 1, 2, mode=0, column=2) == ([0, 1, 0], [2])


def test_bad_arguments_raise():
    for kw in (dict(keep=0), dict(mode=3), dict(column=3)):
        args = dict(keep=1, mode=0, column=0)
        args.update(kw)
        try:
            respawn_plan([[1.0, 0.0, 1.0]], [0], None, [0], 1, args["keep"], mode=args["mode"], column=args["column"])
        except ValueError:
            continue
        raise AssertionError(kw)
    for call in (lambda: respawn_plan([1.0], [0], None, [0], 1, 1, mode=2),         # the verdict is needed
                 lambda: respawn_plan([1.0], [0], None, [1], 1, 1, mode=0),         # a group out of range
                 lambda: respawn_plan([1.0], [0], None, [0], 1, 1, mode=0, column=2)):      # a column of a total-only table
        try:
            call()
        except ValueError:
            continue
        raise AssertionError("accepted")


# ---- random tables ---------------------------------------------------------------------------------------------------

def test_invariants_on_random_tables():
    rng = np.random.default_rng(20251018)
    pool = np.array([0.0, -0.0, 1.0, 1.0, 2.0, -3.0, 0.5, INF, -INF, NAN, 7.0, 7.0])
    seen_empty = seen_full = seen_collider_kept = 0
    for trial in range(200):
        n_groups = int(rng.integers(1, 7))
        sizes = rng.integers(1, 81, n_groups)
        group = rng.permutation(np.repeat(np.arange(n_groups), sizes)).astype(np.int32)
        n_runs = group.size
        rows = np.stack([rng.choice(pool, n_runs), rng.choice(pool, n_runs), rng.choice(pool, n_runs)], axis=1)
        if trial % 3 == 0:
            rows[rng.random(n_runs) < 0.7, 0] = NAN         # groups without a candidate
        status = rng.choice([-1, 0, 1], n_runs)
        col = rng.integers(0, 2, n_runs)
        keep = int(rng.integers(1, 12))
        mode = trial % 3
        column = int(rng.integers(0, 3))
        src, cnt = respawn_plan(rows, status, col, group, n_groups, keep, mode=mode, column=column)
        cand = ((status == 0) | (status == 1)) & np.isfinite(rows[:, 0])
        if mode == 1:
            cand &= col == 0
        assert (cnt <= keep).all()
        assert np.array_equal(cnt, np.minimum(keep, np.bincount(group[cand], minlength=n_groups)))
        survivor = src == np.arange(n_runs)
        assert np.array_equal(np.bincount(group[survivor], minlength=n_groups), cnt)
        assert cand[survivor].all()
        for r in range(n_runs):
            g = group[r]
            if cnt[g] == 0:
                assert src[r] == -1
                continue
            # -1 appears exactly where the group has no survivor; every source is a survivor of the same group
            assert src[r] >= 0 and survivor[src[r]] and group[src[r]] == g
        for g in range(n_groups):
            mine = np.flatnonzero((group == g) & survivor)
            others = np.flatnonzero((group == g) & cand & ~survivor)
            if mine.size and others.size:
                key = lambda r: ((int(col[r]) if mode == 2 else 0), cost_key(rows[r, column]), r)
                assert max(key(r) for r in mine) < min(key(r) for r in others)
            # the best survivor receives the most copies: the counts fall by at most one from rank to rank
            if mine.size:
                ranked = sorted(mine, key=lambda r: ((int(col[r]) if mode == 2 else 0), cost_key(rows[r, column]), r))
                copies = [int(((src == r) & ~survivor).sum()) for r in ranked]
                assert all(a >= b for a, b in zip(copies, copies[1:])) and copies[0] - copies[-1] <= 1
        seen_empty += int((cnt == 0).any())
        seen_full += int((cnt == keep).any())
        seen_collider_kept += int(mode == 2 and (col[survivor] == 1).any())
    assert seen_empty >= 10 and seen_full >= 10 and seen_collider_kept >= 5, (seen_empty, seen_full, seen_collider_kept)


# ---- the C ABI -------------------------------------------------------------------------------------------------------

PROTOTYPE = """int orc_batch_respawn(orc_module * mod, int batch_id, int cost_column, int n_groups, const int * group_of_run,
   int collision_mode, int keep, double sigma, const unsigned int * seeds,
   int * source_of_run_out, int * n_survivors_out);"""


def test_symbol_is_in_the_c_abi():
    assert "orc_batch_respawn" in [s[0] for s in _capi.SYMBOLS]
    raw = C.CDLL(_capi.LIB_PATH)
    assert raw.orc_batch_respawn is not None                    # (AttributeError: the built library lacks the symbol)
    root = os.path.dirname(os.path.dirname(os.path.abspath(_capi.__file__)))
    with open(os.path.join(root, "include", "orcdchomp_amd.h")) as f:
        header = f.read()
    assert PROTOTYPE in header
    for word in ("4 096 runs", "share start and goal", "more than one shard"):
        assert word in header, word
    # without a module the call reports "no module" like every other entry point
    assert _capi.lib().orc_batch_respawn(None, 1, 0, 1, None, 2, 1, 0.0, None, None, None) == 2
