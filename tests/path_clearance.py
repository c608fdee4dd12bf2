"""TEST INFRASTRUCTURE: the paths and segments of tests/test_gpu_path_clearance.py, whose premises
tests/test_host_path_clearance.py checks without a GPU, and the child process of its test of the rounds.

The exact yardstick of orc_batch_path_clearance is orc_batch_clearance itself: a batch of one run per path, n_points the
path's rows, given the paths by batch_set_traj.  A segment [a, b] has the samples of the three-point trajectory [a, b, b]
(the second segment has no length and no duration), which is what a batch can hold."""
import os
import sys

if __name__ == "__main__":      # (the child process: the package lies beside this folder)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

import config_clearance as CC

STEP = 0.04            # C-space length between two samples of the verdict's plan
WAM_VMAX = CC.WAM_VMAX
CAP = 8                # the max_samples under which the long paths of wam_paths are too long


def abb(segments):
    """[n_q][2][n] -> [n_q][3][n]: the three-point trajectories [a, b, b] of the segments [a, b]"""
    s = np.asarray(segments, dtype=np.float64)
    return np.concatenate([s, s[:, 1:]], axis=1)


def wam_paths():
    """the ten 5-row paths of the WAM over the table, by name, with the sample count each must have at the default
    max_samples and under CAP (-2: too long)"""
    f = CC.wam_fixed()
    start, table, folded, away = f["start"], f["in the table"], f["folded"], f["away"]
    mid = table + 0.6 * (start - table)
    wrist = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.06])
    paths, counts = {}, {}

    def add(name, rows, n_default, n_cap):
        paths[name] = np.asarray(rows, dtype=np.float64); counts[name] = (n_default, n_cap)

    drift = np.array([0.02, -0.01, 0.02, 0.01, 0.03, 0.02, 0.03])
    add("clear: about the start", [start + k * drift for k in range(5)], 6, 6)
    add("clear: away from the table", [away + k * wrist for k in range(5)], 6, 6)
    add("dips: from above", [mid, table, table + wrist, table + 2 * wrist, mid], 84, -2)
    add("dips: along the top", [table - 2 * wrist, table - wrist, table, table + wrist, table + 2 * wrist], 6, 6)
    add("self contact", [folded - 2 * wrist, folded - wrist, folded, folded + wrist, folded + 2 * wrist], 6, 6)
    short = np.tile(start, (5, 1)); short[1:, 4] += 0.01
    add("length 0.01", short, 1, 1)
    add("zero length", np.tile(f["near"], (5, 1)), 0, 0)
    nan = np.array([start + k * drift for k in range(5)]); nan[1, 5] = np.nan      # (the one sample is a0 + (a1 - a0) * 0 on segment 0: row 1 reaches it)
    add("a NaN entry", nan, 1, 1)
    inf = np.array([start + k * drift for k in range(5)]); inf[3, 1] = np.inf
    add("an infinite entry", inf, -2, -2)
    add("too long under the cap", [start + k * 6.0 * drift for k in range(5)], 34, -2)
    return paths, counts


def move(q, dof, k):
    """the segment from q along one dof that has exactly k samples: its length is 0.04 (k - 0.5)"""
    b = np.asarray(q, dtype=np.float64).copy()
    b[dof] += STEP * (k - 0.5)
    return np.array([q, b])


SPECIAL = (1, 2, 63, 64, 65, 130)      # sample counts of the segments that meet the chunk's edges


def chunk_segments():
    """26 segments of the WAM and their sample counts: the six of SPECIAL, each behind three or four of 3 samples, so that
    chunks of 64 hold several whole queries, tails and heads of two, and the 130-sample one spans three"""
    pool = CC.wam_pool()
    segs, counts = [], []
    threes = [move(pool[i % len(pool)], (i * 3) % 7, 3) for i in range(20)]
    t = 0
    for j, k in enumerate(SPECIAL):
        segs.append(move(pool[(j + 2) % len(pool)], j % 7, k)); counts.append(k)
        for _ in range(4 if j < 2 else 3):
            segs.append(threes[t]); counts.append(3); t += 1
    assert t == 20
    return np.array(segs), np.array(counts)


def chunk_orders(counts):
    """three orders of the list: as built, the 130-sample query first, the 130-sample query last"""
    n = len(counts)
    big = int(np.flatnonzero(np.asarray(counts) == 130)[0])
    rest = [i for i in range(n) if i != big]
    rng = np.random.default_rng(5)
    shuffled = list(rng.permutation(rest))
    return [np.arange(n), np.array([big] + shuffled), np.array(shuffled[::-1] + [big])]


def local_paths(configs, col0=0, n_rows=3, seed=0, step=0.05):
    """one path per configuration: rows that drift from it by up to `step` per joint column and row (doubles that no float
    holds), the columns before col0 (a floating base's pose) moved a little too, its quaternion NOT of unit length"""
    rng = np.random.default_rng(seed)
    configs = np.asarray(configs, dtype=np.float64)
    out = np.zeros((len(configs), n_rows, configs.shape[1]))
    for q, c in enumerate(configs):
        row = c.copy()
        for i in range(n_rows):
            out[q, i] = row
            row = row.copy()
            row[col0:] += rng.uniform(-step, step, size=len(c) - col0)
            if col0:
                row[:3] += rng.uniform(-0.01, 0.01, size=3)
                row[3:7] *= rng.uniform(0.8, 1.25)
    return out


def waypoint_pairs(n_runs, n_points):
    """(run, from, to) of the waypoint form's queries: forwards, backwards, from == to, adjacent points, the whole run"""
    runs = np.array([0, 1, 2, 3, 0, 1, 2, 3, 1, 2]) % n_runs
    frm = np.array([0, n_points - 1, 4, 5, 6, 2, n_points - 2, 3, 0, 7])
    to = np.array([n_points - 1, 0, 4, 6, 5, 9, n_points - 1, 1, 1, 7])
    return runs.astype(np.int32), frm.astype(np.int32), to.astype(np.int32)


KEYS = ("clearance", "time", "sphere", "other", "n_samples")


def rounds_child(out_path):
    """the child process of the rounds' test: the list of chunk_segments under the ORC_PATH_WORKSPACE of its environment, the
    five outputs into out_path (.npz); then a workspace smaller than the longest query, which the call must refuse"""
    import common
    import or_cdchomp_amd
    from test_gpu_verdict_device import KW, set_wam_vmax

    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    set_wam_vmax(mod, model)
    bid = mod.batch_create(model.name, common.wam_goals(1, seed=1), **dict(KW, n_points=4))
    segs, _ = chunk_segments()
    res = mod.batch_path_clearance(bid, segs)
    os.environ["ORC_PATH_WORKSPACE"] = "100"
    refused = ""
    try:
        mod.batch_path_clearance(bid, segs)
    except RuntimeError as e:
        refused = str(e)
    os.environ["ORC_PATH_WORKSPACE"] = "132"
    again = mod.batch_path_clearance(bid, segs)
    np.savez(out_path, refused=np.array(refused), **{k: res[k] for k in KEYS}, **{"again_" + k: again[k] for k in KEYS})
    mod.batch_destroy(bid)
    mod.close()


if __name__ == "__main__":
    rounds_child(sys.argv[1])
