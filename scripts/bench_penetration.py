"""orc_batch_waypoint_penetration and batch_push_out, measured on the WAM tabletop (NOTES/penetration.md):
  profile  config 2's 1 024 runs after 100 iterations: the whole profile by batch_waypoint_penetration(bid) (102 400 queries)
           beside batch_waypoint_clearance(bid) of the same build, alternated: a warm-up of each, then REPS rounds (default 12)
           of one timed window per leg -- CALLS calls at least (default 5), and as many as fill 0.2 s --, the order rotating;
           medians with min .. max, and the time per evaluated configuration.
  goals    config 2's 1 024 goals (the goals leg of scripts/bench_config_clearance.py): those in contact are pushed out by
           batch_push_out at margins (0.02, 0) inside the joint limits: how many get clear, how far they moved, how many end
           with status 1 or 2, the calls it took and the time.
All calls end in a device synchronise; the clock is the host's around them.  Prints one JSON line per leg.
   python scripts/bench_penetration.py [--reps N] [--calls N] [--skip-goals]"""
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
from or_cdchomp_amd import robots  # noqa: E402

WAM_VMAX = [0.5, 1.0, 2.0, 1.0, 4.0, 1.0, 0.25]
MARGIN = (0.02, 0.0)
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
    legs = dict(penetration=lambda: mod.batch_waypoint_penetration(bid, margin=MARGIN), clearance=lambda: mod.batch_waypoint_clearance(bid))
    first = {name: f() for name, f in legs.items()}
    assert np.array_equal(first["penetration"]["clearance"], first["clearance"]["clearance"], equal_nan=True)
    names = list(legs)
    ms = {name: [] for name in names}
    n_calls = {name: max(calls, int(np.ceil(WINDOW_S * 1e3 / timed(legs[name], calls)))) for name in names}
    for r in range(reps):
        for name in names[r % 2:] + names[:r % 2]:
            ms[name].append(timed(legs[name], n_calls[name]))
    cost = first["penetration"]["cost"]
    out = dict(leg="profile", runs=n_runs, n_points=n_points, reps=reps, margin=MARGIN, chunk=mod.batch_penetration_chunk(bid),
               clearance_chunk=mod.batch_config_chunk(bid), waypoints_with_a_cost=int((cost.sum(axis=-1) > 0).sum()))
    for name in names:
        med = float(np.median(ms[name]))
        out[name] = dict(configurations=n_runs * n_points, calls_per_window=n_calls[name], ms=dict(median=med, min=min(ms[name]), max=max(ms[name])),
                         ns_per_configuration=med * 1e6 / (n_runs * n_points))
    print(json.dumps(out), flush=True)
    mod.batch_destroy(bid)


def goals(mod, model):
    g = common.wam_goals(1024, seed=20250101)
    wam = robots.wam7()
    lo, hi = np.asarray(wam.limit_lower[:7]), np.asarray(wam.limit_upper[:7])
    bid = mod.batch_create(model.name, g[:1], **common.CONFIG2_KW)
    before = mod.batch_config_clearance(bid, g)["clearance"]
    hit = np.fmin(before[:, 0], before[:, 1]) < 0
    calls = [0]
    real = mod.batch_config_penetration

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)
    mod.batch_config_penetration = counted
    t0 = time.perf_counter()
    rows, steps, status = mod.batch_push_out(bid, g[hit], margin=MARGIN, lower=lo, upper=hi)
    seconds = time.perf_counter() - t0
    mod.batch_config_penetration = real
    after = mod.batch_config_clearance(bid, rows)["clearance"]
    ok = status == 0
    assert (after[ok] >= np.asarray(MARGIN)).all()
    moved = np.linalg.norm(rows - g[hit], axis=1)
    print(json.dumps(dict(leg="goals", goals=len(g), in_contact=int(hit.sum()), in_contact_by_field=int((before[:, 0] < 0).sum()),
                          in_contact_by_self=int((before[:, 1] < 0).sum()), margin=MARGIN, clear=int(ok.sum()), status_1=int((status == 1).sum()),
                          status_2=int((status == 2).sum()), moved_rad=dict(median=float(np.median(moved[ok])), max=float(moved[ok].max())),
                          steps=dict(median=float(np.median(steps[ok])), max=int(steps[ok].max())), device_calls=calls[0], seconds=seconds,
                          not_clear_by_field=int((~ok & (after[:, 0] < MARGIN[0])).sum()), not_clear_by_self=int((~ok & (after[:, 1] < MARGIN[1])).sum()))),
          flush=True)
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
