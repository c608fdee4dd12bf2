"""orc_batch_clearance against orc_batch_collision_verdict_subset, measured on the WAM tabletop (NOTES/clearance.md):
  pairs   config 2's 1 024 runs after 100 iterations: batch_clearance(runs="candidates") against
          batch_collision_verdict(on_device=True, runs="candidates", count=False) of the same build, alternated, REPS pairs
          (default 12) after a warm-up of each, CALLS calls per timed window; once on the whole batch, where the verdict stops
          at a contact and the clearance cannot, and once with the colliding candidates masked out (the same mask for both),
          where both walk every sample.
  bound   one run of about 2^20 samples alone in a batch of one, max_samples 2^20: what the cap's upper end costs.
Both calls end in a device synchronise; the clock is the host's around them.  Prints one JSON line per leg.
   python scripts/bench_clearance.py [--reps N] [--calls N] [--skip-bound]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import common  # noqa: E402
import or_cdchomp_amd  # noqa: E402
from or_cdchomp_amd.module import candidates  # noqa: E402

WAM_VMAX = [0.5, 1.0, 2.0, 1.0, 4.0, 1.0, 0.25]


def timed(f, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        f()
    return (time.perf_counter() - t0) / calls * 1e3


def pairs(mod, bid, runs, reps, calls, what):
    clear = lambda: mod.batch_clearance(bid, runs=runs)
    verdict = lambda: mod.batch_collision_verdict(bid, on_device=True, runs=runs, count=False)
    clear(); verdict()
    tc, tv = [], []
    for r in range(reps):
        for leg in ((clear, tc), (verdict, tv)) if r % 2 == 0 else ((verdict, tv), (clear, tc)):
            leg[1].append(timed(leg[0], calls))
    c = clear()
    walked = c["n_samples"] >= 0
    print(json.dumps(dict(leg=what, runs_walked=int(walked.sum()), samples=int(c["n_samples"][walked].sum()), reps=reps, calls=calls,
                          clearance_ms=dict(median=float(np.median(tc)), min=min(tc), max=max(tc)),
                          verdict_ms=dict(median=float(np.median(tv)), min=min(tv), max=max(tv)),
                          ratio=float(np.median(tc) / np.median(tv)))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--skip-bound", action="store_true")
    args = ap.parse_args()
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    vmax = np.ones(model.n_dof); vmax[:7] = WAM_VMAX
    mod.set_velocity_limits(model.name, vmax)
    bid = mod.batch_create(model.name, common.wam_goals(1024), **common.CONFIG2_KW)
    costs, status = mod.batch_iterate(bid, 100)
    cand = candidates(costs, status)
    v = mod.batch_collision_verdict(bid, on_device=True, runs="candidates", count=False)
    print(json.dumps(dict(leg="batch", runs=1024, candidates=int(cand.sum()), colliding_candidates=int((v["collides"] == 1).sum()))), flush=True)
    pairs(mod, bid, "candidates", args.reps, args.calls, "whole batch (candidates)")
    pairs(mod, bid, cand & (v["collides"] == 0), args.reps, args.calls, "colliding candidates masked out")
    mod.batch_destroy(bid)
    if not args.skip_bound:
        n_points = 100
        start = np.asarray(common.wam_state()[2][:7])
        turn = start + np.array([0.0, 0.0, 0.0, 0.0, -1.0, 0.4, 0.8])
        seg = ((1 << 20) - 0.5) * 0.04 / (n_points - 1)      # rad per segment: set_traj takes what the joint limits would not
        s = np.array([seg / np.linalg.norm(turn - start) * (i % 2) for i in range(n_points)])
        traj = start[None, :] + s[:, None] * (turn - start)[None, :]
        bid = mod.batch_create(model.name, common.wam_goals(1), **common.CONFIG2_KW)
        mod.batch_set_traj(bid, traj[None])
        t0 = time.perf_counter()
        c = mod.batch_clearance(bid, max_samples=1 << 20)
        first = (time.perf_counter() - t0) * 1e3
        again = timed(lambda: mod.batch_clearance(bid, max_samples=1 << 20), 3)
        print(json.dumps(dict(leg="one run at the cap", n_samples=int(c["n_samples"][0]), first_ms=first, ms=again,
                              clearance=c["clearance"][0].tolist())), flush=True)
        mod.batch_destroy(bid)
    mod.close()


if __name__ == "__main__":
    main()
