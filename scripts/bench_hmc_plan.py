"""The host layer of the hmc plan and of perturb / select, this build against the parent's library (NOTES/hmc-plan.md).
Child processes alternated parent, this (the parent's library through ORC_LIB), a warm-up round and REPS timed rounds per leg:
  config4     bench.py --gpus 1 --config 4 --no-cpu-baseline --no-other-configs: CHOMP iterations/s of 4 096 hmc runs per step
              on two streams (the host must not wait for a step's plan)
  async       the same two batches in a process of this script: host time of one batch_iterate_async call of 100 iterations
              (plan and launch enqueued) and wall time of a step of both, medians of STEPS steps
  multistart  the 8 192-run block of scripts/bench_multistart.py: batch_perturb, and batch_select_best(collision_free=False) +
              batch_gettraj_runs after 100 iterations, batch_select_clear (whole, and less the batch_clearance of the candidates
              timed beside it) and batch_respawn (mode 0, keep 16 of 128), medians of five calls (NOTES/multistart-host.md)
  headline    (--headline N) bench.py's headline configuration, parent / this alternated N times
Writes profiles/hmc_plan_<build>.json (adding to the legs an earlier call left there) and prints one line.
   python scripts/bench_hmc_plan.py --parent-lib FILE [--reps 5] [--headline 2] [--legs config4,async,multistart]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

STEPS = 6
BENCH = ["--gpus", "1", "--no-cpu-baseline", "--no-other-configs"]


def med(xs):
    return float(np.median(xs))


def child_async():
    import common
    import or_cdchomp_amd
    mod = or_cdchomp_amd.Module(0)
    mod.set_num_streams(2)
    model = common.setup_product_wam(mod)
    goals, basegoals, seeds, kw = common.config4_problem(4096)
    bids = [mod.batch_create(model.name, goals, basegoals=basegoals, seeds=seeds, **kw) for _ in range(2)]
    host, step = [], []
    for s in range(STEPS + 1):
        t0 = time.perf_counter()
        for b in bids:
            t1 = time.perf_counter()
            mod.batch_iterate_async(b, 100)
            if s:
                host.append(time.perf_counter() - t1)
        for b in bids:
            mod.batch_sync(b)
        if s:
            step.append(time.perf_counter() - t0)
    mod.close()
    return dict(iterate_async_host_s=med(host), iterate_async_host_max_s=max(host), step_s=med(step))


def child_multistart():
    import common
    import or_cdchomp_amd
    import bench_multistart as ms
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    goals = np.repeat(common.wam_goals(ms.N_PROBLEMS, seed=20250101), ms.N_STARTS, axis=0)
    seeds = np.arange(ms.N_BLOCK, dtype=np.uint32) + 1
    bid = mod.batch_create(model.name, goals, **ms.KW)
    start = mod.batch_gettraj(bid)
    perturb, select = [], []
    for rnd in range(6):
        mod.batch_set_traj(bid, start)
        t0 = time.perf_counter()
        mod.batch_perturb(bid, ms.SIGMA, seeds)
        if rnd:
            perturb.append(time.perf_counter() - t0)
    mod.batch_iterate(bid, 100)
    for rnd in range(6):
        t0 = time.perf_counter()
        best, cost, cnt = mod.batch_select_best(bid, n_groups=ms.N_PROBLEMS, collision_free=False)
        rows = mod.batch_gettraj_runs(bid, best)
        if rnd:
            select.append(time.perf_counter() - t0)
    # the selection by margin: its time is the clearance walk of the candidates, so that walk alone is timed beside it
    mod.batch_set_verdict_scope(bid, "candidates")
    clear, walk = [], []
    for rnd in range(6):
        t0 = time.perf_counter()
        sel = mod.batch_select_clear(bid, n_groups=ms.N_PROBLEMS, margin=0.0)
        t1 = time.perf_counter()
        mod.batch_clearance(bid, runs="candidates")
        if rnd:
            clear.append(t1 - t0); walk.append(time.perf_counter() - t1)
    # the respawn last (it changes the runs): mode 0, no verdict in its time; iterate(0) makes the costs valid again
    respawn = []
    for rnd in range(6):
        t0 = time.perf_counter()
        source, kept = mod.batch_respawn(bid, 16, ms.SIGMA, seeds, n_groups=ms.N_PROBLEMS, collision="ignore")
        if rnd:
            respawn.append(time.perf_counter() - t0)
        mod.batch_iterate(bid, 0)
    mod.close()
    return dict(perturb_s=med(perturb), select_gettraj_s=med(select), select_clear_s=med(clear), clearance_s=med(walk),
                select_clear_less_clearance_s=med(clear) - med(walk), respawn_s=med(respawn),
                winners=[int(x) for x in best] + [int(x) for x in sel[0]] + [int(x) for x in source],
                rows_sum=float(np.nansum(rows)) + float(np.nansum(sel[2])))


def run_child(leg, parent_lib, bench_args=()):
    env = dict(os.environ)
    env.pop("ORC_LIB", None)
    if parent_lib:
        env["ORC_LIB"] = os.path.abspath(parent_lib)
    if leg in ("config4", "headline"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + BENCH + list(bench_args)
    else:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", leg]
    out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, timeout=900, cwd=ROOT).stdout.decode()
    line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
    rec = json.loads(line)
    return dict(value=rec["value"]) if leg in ("config4", "headline") else rec


def spread(xs):
    return dict(median=med(xs), min=float(min(xs)), max=float(max(xs)), all=[float(x) for x in xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--headline", type=int, default=0)
    ap.add_argument("--legs", default="config4,async,multistart")
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child_async() if args.child == "async" else child_multistart()))
        return
    from or_cdchomp_amd import _capi
    rec = dict(build=_capi.csrc_hash(), reps=args.reps, legs={})
    path = os.path.join(ROOT, "profiles", "hmc_plan_%s.json" % rec["build"])
    if os.path.exists(path):                                  # (legs taken in an earlier call of the same build are kept)
        with open(path) as f:
            rec = json.load(f)
    for leg in [x for x in args.legs.split(",") if x]:
        runs = dict(parent=[], this=[])
        bench_args = ("--config", "4", "--steps", "8", "--warmup", "2") if leg == "config4" else ()
        for rnd in range(args.reps + 1):
            for name in ("parent", "this"):
                print("%s round %d %s" % (leg, rnd, name), file=sys.stderr, flush=True)
                r = run_child(leg, args.parent_lib if name == "parent" else "", bench_args)
                if rnd:
                    runs[name].append(r)
        if leg == "multistart":
            assert all(r["winners"] == runs["this"][0]["winners"] and r["rows_sum"] == runs["this"][0]["rows_sum"] for r in runs["this"] + runs["parent"])
        keys = [k for k in runs["this"][0] if k == "value" or k.endswith("_s")]
        rec["legs"][leg] = {k: dict(parent=spread([r[k] for r in runs["parent"]]), this=spread([r[k] for r in runs["this"]])) for k in keys}
    if args.headline:
        order, vals = [], []
        for _ in range(args.headline):
            for name in ("parent", "this"):
                order.append(name)
                vals.append(run_child("headline", args.parent_lib if name == "parent" else "", ("--steps", "20", "--warmup", "5"))["value"])
        rec["headline"] = dict(order=order, values=vals)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(dict(build=rec["build"], headline=rec.get("headline"),
                          legs={leg: {k: (round(v["parent"]["median"], 6), round(v["this"]["median"], 6)) for k, v in d.items()} for leg, d in rec["legs"].items()})))


if __name__ == "__main__":
    main()
