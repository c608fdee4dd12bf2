"""Clearance of given segments, measured on one card: orc_batch_path_clearance against the only way to the same answers
without it, a three-point batch of one run per segment that is created, given [a, b, b] by batch_set_traj, walked by
batch_clearance and destroyed.  Two workloads over config 2's scene (the WAM and the table):
  lines   the 1 024 straight lines from config 2's start to its goals
  edges   65 536 random edges of 0.2 rad inside the joint limits (5 samples each)
Per workload: the wall time of the new call, of the detour (create, upload, walk, destroy) and of the detour's walk alone;
a warm-up of 2 and REPS (default 7) timed repeats, the legs alternated, medians.  The two ways' answers are compared bit for
bit, and for `lines` the number of lines that are clear at margin 0 is counted.
Writes <out>/path_clearance.json (default out: profiles/) and prints one line.
   python scripts/bench_path_clearance.py [reps] [--out DIR]
   python scripts/bench_path_clearance.py --trace          one pass of the new call per workload, for a kernel trace
       (rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_path_clearance.py --trace)"""
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import common  # noqa: E402
import or_cdchomp_amd  # noqa: E402
from or_cdchomp_amd import robots  # noqa: E402

KW = dict(common.CONFIG2_KW)
KEYS = ("clearance", "time", "sphere", "other", "n_samples")
EDGE = 0.2


def option(name, default=None):
    if name in sys.argv:
        return sys.argv[sys.argv.index(name) + 1]
    return default


def workloads():
    start = np.asarray(robots.WAM_START, dtype=np.float64)
    goals = common.wam_goals(1024)
    lines = np.stack([np.tile(start, (len(goals), 1)), goals], axis=1)
    model = robots.wam7()
    lo, hi = np.asarray(model.limit_lower[:7]) + 0.1, np.asarray(model.limit_upper[:7]) - 0.1
    rng = np.random.default_rng(20261021)
    a = rng.uniform(lo, hi, size=(65536, 7))
    d = rng.normal(size=(65536, 7))
    b = a + EDGE * d / np.linalg.norm(d, axis=1, keepdims=True)
    return {"lines": lines, "edges": np.stack([a, b], axis=1)}


def detour(mod, name, segs):
    """the parent's way; returns (result, seconds of the walk alone)"""
    trajs = np.concatenate([segs, segs[:, 1:]], axis=1)
    bid = mod.batch_create(name, segs[:, 1], **dict(KW, n_points=3))
    mod.batch_set_traj(bid, trajs)
    t0 = time.perf_counter()
    res = mod.batch_clearance(bid)
    walk = time.perf_counter() - t0
    mod.batch_destroy(bid)
    return res, walk


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 7
    out_dir = option("--out", os.path.join(ROOT, "profiles"))
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    bid = mod.batch_create(model.name, common.wam_goals(1), **dict(KW, n_points=4))
    record = {}
    for name, segs in workloads().items():
        if "--trace" in sys.argv:
            mod.batch_path_clearance(bid, segs)
            continue
        t_new, t_old, t_walk = [], [], []
        for rep in range(reps + 2):
            t0 = time.perf_counter()
            new = mod.batch_path_clearance(bid, segs)
            t1 = time.perf_counter()
            old, walk = detour(mod, model.name, segs)
            t2 = time.perf_counter()
            if rep >= 2:
                t_new.append(t1 - t0); t_old.append(t2 - t1); t_walk.append(walk)
        same = all(np.asarray(new[k]).tobytes() == np.asarray(old[k]).tobytes() for k in KEYS)
        walked = new["n_samples"] >= 0
        clear = walked & (new["clearance"].min(axis=1) > 0.0)
        ms = lambda t: round(1e3 * float(np.median(t)), 3)
        record[name] = dict(n_q=len(segs), samples=int(new["n_samples"][walked].sum()), samples_per_query=[int(new["n_samples"].min()), int(new["n_samples"].max())],
                            new_ms=ms(t_new), detour_ms=ms(t_old), detour_walk_ms=ms(t_walk), new_ms_all=[round(1e3 * t, 3) for t in t_new],
                            detour_ms_all=[round(1e3 * t, 3) for t in t_old], same_bits=bool(same), clear_at_margin_0=int(clear.sum()),
                            too_long=int((~walked).sum()))
    mod.batch_destroy(bid)
    mod.close()
    if record:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "path_clearance.json"), "w") as f:
            json.dump(dict(reps=reps, **record), f, indent=1)
        print(json.dumps(record))


if __name__ == "__main__":
    main()
