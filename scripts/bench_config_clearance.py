"""orc_batch_waypoint_clearance and orc_batch_config_clearance, measured on the WAM tabletop (NOTES/config-clearance.md):
  profile  config 2's 1 024 runs after 100 iterations: the whole profile (batch_waypoint_clearance(bid), 102 400 queries), the
           same rows uploaded (batch_config_clearance of batch_gettraj's rows) and batch_clearance(bid) of the same build, each
           with the configurations it evaluates (queries; samples walked), alternated: a warm-up of each, then REPS rounds
           (default 12) of one timed window per leg -- CALLS calls at least (default 5), and as many as fill 0.2 s --, the order
           rotating; medians with min .. max, and the time per evaluated configuration.
  goals    config 2's 1 024 goals with K = 16 perturbed starts at sigma 0.3 after 100 iterations (the setup of DESIGN.md's
           multi-start table): of the problems without a collision-free winner, how many have a goal row, and how many a start
           row, with a negative minimum.
All calls end in a device synchronise; the clock is the host's around them.  Prints one JSON line per leg.
   python scripts/bench_config_clearance.py [--reps N] [--calls N] [--skip-goals]"""
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

WAM_VMAX = [0.5, 1.0, 2.0, 1.0, 4.0, 1.0, 0.25]
K, SIGMA = 16, 0.3
WINDOW_S = 0.2


def timed(f, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        f()
    return (time.perf_counter() - t0) / calls * 1e3


def profile(mod, model, reps, calls):
    bid = mod.batch_create(model.name, common.wam_goals(1024), **common.CONFIG2_KW)
    mod.batch_iterate(bid, 100)
    n_runs, n_points, n = mod.batch_dims(bid)
    rows = mod.batch_gettraj(bid).reshape(-1, n)
    runs = np.repeat(np.arange(n_runs), n_points)
    legs = dict(waypoints=lambda: mod.batch_waypoint_clearance(bid), uploaded=lambda: mod.batch_config_clearance(bid, rows, runs=runs),
                clearance=lambda: mod.batch_clearance(bid))
    first = {name: f() for name, f in legs.items()}
    assert np.array_equal(first["waypoints"]["clearance"].reshape(-1, 2), first["uploaded"]["clearance"], equal_nan=True)
    ns = first["clearance"]["n_samples"]
    evaluated = dict(waypoints=n_runs * n_points, uploaded=n_runs * n_points, clearance=int(ns[ns >= 0].sum()))
    ms = {name: [] for name in legs}
    names = list(legs)
    # a window lasts WINDOW_S at least: a call of half a millisecond is timed some hundred times over
    n_calls = {name: max(calls, int(np.ceil(WINDOW_S * 1e3 / timed(legs[name], calls)))) for name in names}
    for r in range(reps):
        for name in names[r % 3:] + names[:r % 3]:
            ms[name].append(timed(legs[name], n_calls[name]))
    prof = first["waypoints"]["clearance"]
    out = dict(leg="profile", runs=n_runs, n_points=n_points, reps=reps, runs_walked=int((ns >= 0).sum()), longest_run_samples=int(ns.max()),
               waypoints_in_contact=int((np.fmin(prof[:, :, 0], prof[:, :, 1]) < 0).sum()))
    for name in names:
        med = float(np.median(ms[name]))
        out[name] = dict(configurations=evaluated[name], calls_per_window=n_calls[name], ms=dict(median=med, min=min(ms[name]), max=max(ms[name])),
                         ns_per_configuration=med * 1e6 / evaluated[name])
    # what the upload alone costs: batch_set_traj of the same rows moves the same bytes (and leaves the batch as it is)
    traj = rows.reshape(n_runs, n_points, n)
    mod.batch_set_traj(bid, traj)
    out["set_traj_of_the_same_rows_ms"] = timed(lambda: mod.batch_set_traj(bid, traj), 10)
    out["uploaded_bytes"] = int(rows.nbytes)
    print(json.dumps(out), flush=True)
    mod.batch_destroy(bid)


def goals(mod, model):
    g = common.wam_goals(1024, seed=20250101)
    P = len(g)
    bid = mod.batch_create(model.name, np.repeat(g, K, axis=0), **common.CONFIG2_KW)
    mod.batch_perturb(bid, SIGMA, np.arange(P * K, dtype=np.uint32) + 1)
    mod.batch_iterate(bid, 100)
    best, _, _ = mod.batch_select_best(bid, n_groups=P, collision_free=True)
    n_points = mod.batch_dims(bid)[1]
    first = np.arange(P) * K      # (a problem's runs share start and goal: the perturbation leaves the end rows)
    ends = mod.batch_waypoint_clearance(bid, runs=np.concatenate([first, first]), points=np.concatenate([np.zeros(P, dtype=int), np.full(P, n_points - 1)]))
    low = np.fmin(ends["clearance"][:, 0], ends["clearance"][:, 1])
    start_low, goal_low = low[:P], low[P:]
    none = best < 0
    print(json.dumps(dict(leg="goals", problems=P, K=K, sigma=SIGMA, without_winner=int(none.sum()),
                          without_winner_goal_in_contact=int((none & (goal_low < 0)).sum()),
                          without_winner_start_in_contact=int((none & (start_low < 0)).sum()),
                          goal_in_contact=int((goal_low < 0).sum()), start_in_contact=int((start_low < 0).sum()),
                          with_winner_goal_in_contact=int((~none & (goal_low < 0)).sum()),
                          goal_in_contact_by_field=int((ends["clearance"][P:, 0] < 0).sum()), goal_in_contact_by_self=int((ends["clearance"][P:, 1] < 0).sum()),
                          median_goal_gap_without_winner=float(np.median(goal_low[none])) if none.any() else None)), flush=True)
    mod.batch_destroy(bid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--skip-goals", action="store_true")
    args = ap.parse_args()
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    vmax = np.ones(model.n_dof); vmax[:7] = WAM_VMAX
    mod.set_velocity_limits(model.name, vmax)
    profile(mod, model, args.reps, args.calls)
    if not args.skip_goals:
        goals(mod, model)
    mod.close()


if __name__ == "__main__":
    main()
