"""Per-run parameters (orc_batch_set_run_params, orc_batch_select_best_by), measured on the WAM tabletop (config 2: n_points 100,
lambda 100, obs_factor 500, 100 iterations per call):
  read      config 2's 1 024 runs with a table that equals the shared values against no table: the cost of the read path
  split     128 goals x 8 parameter sets as ONE batch of 1 024 with a table against EIGHT batches of 128, one per set, on
            set_num_streams(4), enqueued and then synced: the wall time ratio
  gain      config 2's 1 024 goals, K = 16 runs per goal: the share of goals with an eligible collision-free run for 16 perturbed
            starts at one parameter set, a 16-set portfolio from the straight line, and 4 sets x 4 perturbed starts; winners by
            the smoothness cost (by="smooth": the one that compares across obs_factor)
in one process, the legs of a comparison alternated, a warm-up round and REPS (default 5) timed rounds, medians.
Writes profiles/run_params_<build>.json and prints one line.
   python scripts/bench_run_params.py [--reps N] [--skip-gain]"""
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
from or_cdchomp_amd import _capi  # noqa: E402

KW = dict(common.CONFIG2_KW)
SHARED = dict(lambda_=KW["lambda_"], epsilon=0.1, obs_factor=KW["obs_factor"], obs_factor_self=10.0)
N_ITER = 100
SIGMA = 0.3
# the portfolio of the tests, and eight / sixteen sets around config 2's own
SETS4 = [dict(lambda_=100.0, obs_factor=500.0, obs_factor_self=10.0, epsilon=0.10),
         dict(lambda_=50.0, obs_factor=200.0, obs_factor_self=10.0, epsilon=0.10),
         dict(lambda_=200.0, obs_factor=1000.0, obs_factor_self=5.0, epsilon=0.06),
         dict(lambda_=400.0, obs_factor=500.0, obs_factor_self=20.0, epsilon=0.14)]
SETS16 = [dict(lambda_=lam, obs_factor=of, obs_factor_self=10.0, epsilon=0.10)
          for lam in (50.0, 100.0, 200.0, 400.0) for of in (200.0, 500.0, 1000.0, 2000.0)]
SETS8 = SETS16[4:12]


def med(xs):
    return float(np.median(xs))


def arrays(sets, set_of_run):
    return {k: np.array([sets[s][k] for s in set_of_run]) for k in sets[0]}


def timed(mod, ids):
    """enqueue one iterate call on every batch, then sync them all: wall seconds"""
    t0 = time.perf_counter()
    for b in ids:
        mod.batch_iterate_async(b, N_ITER)
    for b in ids:
        mod.batch_sync(b, fetch=False)
    return time.perf_counter() - t0


def read_path(args, mod, model):
    goals = common.wam_goals(1024, seed=20250101)
    s = dict(off=[], on=[])
    bid = mod.batch_create(model.name, goals, **KW)
    start = mod.batch_gettraj(bid)
    for rnd in range(args.reps + 1):
        for leg in ("off", "on"):
            mod.batch_set_traj(bid, start)
            if leg == "on":
                mod.batch_set_run_params(bid, **{k: np.full(len(goals), v) for k, v in SHARED.items()})
            else:
                mod.batch_set_run_params(bid)
            dt = timed(mod, [bid])
            if rnd:
                s[leg].append(dt)
    mod.batch_destroy(bid)
    return dict(runs=len(goals), n_iter=N_ITER, off_s=med(s["off"]), on_s=med(s["on"]), on_over_off=med(s["on"]) / med(s["off"]),
                off_all=s["off"], on_all=s["on"])


def split(args, mod, model):
    goals = common.wam_goals(128, seed=20250101)
    ns = len(SETS8)
    s = dict(one=[], eight=[])
    mod.set_num_streams(4)
    for rnd in range(args.reps + 1):
        for leg in ("one", "eight"):
            if leg == "one":
                ids = [mod.batch_create(model.name, np.repeat(goals, ns, axis=0), **KW)]
                mod.batch_set_run_params(ids[0], **arrays(SETS8, np.arange(len(goals) * ns) % ns))
            else:
                ids = [mod.batch_create(model.name, goals, **dict(KW, **SETS8[k])) for k in range(ns)]
            mod.batch_sync(ids[0], fetch=False)
            dt = timed(mod, ids)
            if rnd:
                s[leg].append(dt)
            for b in ids:
                mod.batch_destroy(b)
    mod.set_num_streams(0)
    return dict(goals=len(goals), sets=ns, n_iter=N_ITER, one_batch_s=med(s["one"]), eight_batches_s=med(s["eight"]),
                eight_over_one=med(s["eight"]) / med(s["one"]), one_all=s["one"], eight_all=s["eight"])


def gain(mod, model, K=16):
    goals = common.wam_goals(1024, seed=20250101)
    P = len(goals)
    run_goals = np.repeat(goals, K, axis=0)
    seeds = np.arange(P * K, dtype=np.uint32) + 1

    def leg(sets, set_of_run, perturbed):
        bid = mod.batch_create(model.name, run_goals, **KW)
        if sets is not None:
            mod.batch_set_run_params(bid, **arrays(sets, set_of_run))
        line = mod.batch_gettraj(bid)
        if perturbed is not None:
            # (runs that keep the straight line: sigma 0 is not per run, so they are put back)
            mod.batch_perturb(bid, SIGMA, seeds)
            if not perturbed.all():
                traj = mod.batch_gettraj(bid)
                traj[~perturbed] = line[~perturbed]
                mod.batch_set_traj(bid, traj)
        _, status = mod.batch_iterate(bid, N_ITER)
        if (status == -1).any():
            # a run that left its limits is not eligible, but a step of a strong set can have thrown it so far that its retimed
            # trajectory has more samples than the verdict takes, and that fails the verdict of the whole batch: such runs get
            # their straight line back before the selection (costs and status stay the call's)
            traj = mod.batch_gettraj(bid)
            traj[status == -1] = line[status == -1]
            mod.batch_set_traj(bid, traj)
        best, cost, cnt = mod.batch_select_best(bid, n_groups=P, collision_free=True, by="smooth")
        mod.batch_destroy(bid)
        has = best >= 0
        rec = dict(share_with_winner=float(has.mean()), median_smooth_cost=med(cost[has]) if has.any() else None,
                   aborted_share=float((status == -1).mean()), eligible_share_of_runs=float(cnt.sum() / (P * K)))
        if sets is not None:
            rec["winning_set_histogram"] = np.bincount(set_of_run[best[has]], minlength=len(sets)).tolist()
        return rec, has

    k = np.arange(P * K) % K
    out = {}
    out["K16_perturbed_one_set"], has_a = leg(None, None, np.ones(P * K, dtype=bool))
    out["K16_portfolio_straight_line"], has_b = leg(SETS16, k, None)
    out["K4x4_sets_x_perturbed"], has_c = leg(SETS4, k % 4, (k // 4) > 0)      # per set: the straight line and three perturbed starts
    out["solved_by_portfolio_only"] = int((has_b & ~has_a).sum())
    out["solved_by_perturbation_only"] = int((has_a & ~has_b).sum())
    out["solved_by_4x4_only_vs_perturbation"] = int((has_c & ~has_a).sum())
    out["sigma"] = SIGMA
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-gain", action="store_true")
    args = ap.parse_args()
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    rec = dict(build=_capi.csrc_hash(), lib=os.path.basename(_capi.LIB_PATH), reps=args.reps)
    rec["read"] = read_path(args, mod, model)
    rec["split"] = split(args, mod, model)
    if not args.skip_gain:
        rec["gain"] = gain(mod, model)
    mod.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "run_params_%s.json" % rec["build"]), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(dict(build=rec["build"], read_on_over_off=round(rec["read"]["on_over_off"], 4),
                          eight_over_one=round(rec["split"]["eight_over_one"], 2),
                          gain={k: round(v["share_with_winner"], 3) for k, v in rec.get("gain", {}).items() if isinstance(v, dict)})))


if __name__ == "__main__":
    main()
