"""orc_batch_clearance against orc_batch_collision_verdict_subset, measured on the WAM tabletop (NOTES/clearance.md):
  pairs   config 2's 1 024 runs after 100 iterations: batch_clearance(runs="candidates") against
          batch_collision_verdict(on_device=True, runs="candidates", count=False) of the same build, alternated, REPS pairs
          (default 12) after a warm-up of each, CALLS calls per timed window; once on the whole batch, where the verdict stops
          at a contact and the clearance cannot, and once with the colliding candidates masked out (the same mask for both),
          where both walk every sample.
  bound   one run of about 2^20 samples alone in a batch of one, max_samples 2^20: what the cap's upper end costs.
  parent  (--parent-lib FILE, and nothing else) batch_clearance of "the candidates" and of "candidates that do not collide" in
          child processes, this build and the parent's library (loaded through ORC_LIB) alternated, a warm-up round and ROUNDS
          rounds (default 5) of CALLS calls after a warm-up call: median and min .. max per build, and whether this build's
          median lies within the parent's range.  The record goes to profiles/clearance_<build>.json.
Both calls end in a device synchronise; the clock is the host's around them.  Prints one JSON line per leg.
   python scripts/bench_clearance.py [--reps N] [--calls N] [--skip-bound] [--parent-lib FILE [--rounds N]]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import common  # noqa: E402
import or_cdchomp_amd  # noqa: E402
from or_cdchomp_amd import _capi  # noqa: E402
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


def iterated_batch(mod):
    """config 2's 1 024 runs after 100 iterations: the batch, its candidates and their verdict"""
    model = common.setup_product_wam(mod)
    vmax = np.ones(model.n_dof); vmax[:7] = WAM_VMAX
    mod.set_velocity_limits(model.name, vmax)
    bid = mod.batch_create(model.name, common.wam_goals(1024), **common.CONFIG2_KW)
    costs, status = mod.batch_iterate(bid, 100)
    cand = candidates(costs, status)
    return model, bid, cand, mod.batch_collision_verdict(bid, on_device=True, runs="candidates", count=False)


def parent_child(args):
    """one build's leg of a round: batch_clearance of the candidates and of those that do not collide, ms per call"""
    mod = or_cdchomp_amd.Module(0)
    model, bid, cand, v = iterated_batch(mod)
    rec = dict(lib=os.path.basename(_capi.LIB_PATH))
    for key, runs in (("candidates_ms", "candidates"), ("clear_candidates_ms", cand & (v["collides"] == 0))):
        c = mod.batch_clearance(bid, runs=runs)
        rec[key] = timed(lambda: mod.batch_clearance(bid, runs=runs), args.calls)
        rec[key.replace("_ms", "_samples")] = int(c["n_samples"][c["n_samples"] >= 0].sum())
        rec[key.replace("_ms", "_bits")] = hashlib.sha256(c["clearance"].tobytes() + c["n_samples"].tobytes()).hexdigest()
    mod.batch_destroy(bid)
    mod.close()
    print("CLEARANCE_CHILD " + json.dumps(rec))


def parent_rounds(args):
    """this build and the parent's library alternated in child processes"""
    legs = dict(this=[], parent=[])
    for rnd in range(args.rounds + 1):
        for name in ("parent", "this"):
            env = dict(os.environ)
            env.pop("ORC_LIB", None)
            if name == "parent":
                env["ORC_LIB"] = os.path.abspath(args.parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls)], env=env, check=True,
                                 stdout=subprocess.PIPE, timeout=600).stdout.decode()
            rec = json.loads([ln for ln in out.splitlines() if ln.startswith("CLEARANCE_CHILD ")][-1][len("CLEARANCE_CHILD "):])
            if rnd:
                legs[name].append(rec)
    out = dict(build=_capi.csrc_hash(), runs=1024, rounds=args.rounds, calls=args.calls)
    for key in ("candidates", "clear_candidates"):
        assert len({r[key + "_bits"] for r in legs["this"] + legs["parent"]}) == 1, "the builds must report the same clearances"
        out[key + "_samples"] = legs["this"][0][key + "_samples"]
        for name, recs in legs.items():
            ms = [r[key + "_ms"] for r in recs]
            out["%s_%s_ms" % (name, key)] = dict(median=float(np.median(ms)), min=min(ms), max=max(ms), all=ms)
        p, t = out["parent_%s_ms" % key], out["this_%s_ms" % key]
        out[key + "_within_parent_range"] = bool(p["min"] <= t["median"] <= p["max"])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "clearance_%s.json" % out["build"]), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--skip-bound", action="store_true")
    ap.add_argument("--parent-lib", default="", help="the parent build's library: only the alternation against it is run")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return parent_child(args)
    if args.parent_lib:
        return parent_rounds(args)
    mod = or_cdchomp_amd.Module(0)
    model, bid, cand, v = iterated_batch(mod)
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
