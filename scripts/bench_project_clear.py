"""orc_batch_project_tsr_clear measured on the WAM tabletop (NOTES/project-clear.md): a configuration on the TSR and clear of
contact for config 2's goals in contact.
  The goals of common.wam_goals(1024) in contact (batch_config_clearance < 0) x 16 seeds, the goal plus a Gaussian of sigma 0.3
  per joint, clipped to the joint limits; the TSR of a row sits at its goal's hand pose (manipulator `arm`).  Two workloads: all
  six rows enforced (BW6) and z, roll, pitch (BW3); the defaults of batch_project_tsr_clear.
  device    Module.batch_project_tsr_clear: one call, max_steps + 1 rounds of two launches
  host      the same rule (project_clear.project_clear) as a host loop around Module.batch_config_tsr and
            Module.batch_config_penetration of the same build
            both alternated: a warm-up of each, then REPS rounds (default 8) of one timed window per leg -- CALLS calls at least
            (default 3), and as many as fill 0.2 s --, the order rotating; medians with min .. max
  restated  project_clear.project_clear around the oracle's eval_contsr and the restated penetration on the CPU, over the first
            RESTATED_ROWS rows (default 1024), once
  goals     for how many of the goals in contact a seed ends on the TSR and clear at margins (0.02, 0): beside the figures of
            NOTES/project-tsr.md (projection alone 16, at sigma 1.0 66; push-out 408, which gives up the hand pose)
All device calls end in a synchronise; the clock is the host's around them.  Prints one JSON line per leg and workload.
   python scripts/bench_project_clear.py [--reps N] [--calls N] [--restated-rows N] [--sigma S] [--only BW6|BW3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import common  # noqa: E402
import project as PJ  # noqa: E402
import project_clear as PC  # noqa: E402
import or_cdchomp_amd  # noqa: E402
from or_cdchomp_amd import project_clear  # noqa: E402

SEEDS, SIGMA, WINDOW_S = 16, 0.3, 0.2


def timed(f, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        f()
    return (time.perf_counter() - t0) / calls * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--restated-rows", type=int, default=1024)
    ap.add_argument("--sigma", type=float, default=SIGMA)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    _, base, dofvals, adofs = common.wam_state()
    all_goals = common.wam_goals(1024)
    lo, hi = PJ.wam_limits()
    bid = mod.batch_create(model.name, all_goals[:1], **common.CONFIG2_KW)
    before = mod.batch_config_clearance(bid, all_goals)["clearance"]
    goals = all_goals[np.fmin(before[:, 0], before[:, 1]) < 0]
    Rs, ds = PJ.target_frames(model, base, dofvals, adofs, "handbase", PJ.TOOL, goals)
    rng = np.random.default_rng(1)
    of = np.repeat(np.arange(len(goals)), SEEDS).astype(np.int32)
    seeds = np.clip(goals[of] + args.sigma * rng.normal(size=(len(of), 7)), lo, hi)
    p = PC.PARAMS
    for name, Bw in PC.BWS.items():
        if args.only and name != args.only:
            continue
        tsrs = PJ.tsrs_at(Rs, ds, Bw)
        rec = mod.batch_tsr_records(bid, tsrs)
        ks = rec[1][of]

        def evaluate_tsr(rows, index):
            res = mod.batch_config_tsr(bid, rec, rows, tsr_of=of[index])
            return res["h"], res["jac"]

        def evaluate_pen(rows, margin, index):
            return mod.batch_config_penetration(bid, rows, margin=margin)

        legs = dict(device=lambda: mod.batch_project_tsr_clear(bid, rec, seeds, tsr_of=of, lower=lo, upper=hi),
                    host=lambda: project_clear.project_clear(evaluate_tsr, evaluate_pen, seeds, lower=lo, upper=hi, k=ks, indexed=True, **p))
        first = {leg: f() for leg, f in legs.items()}
        names = list(legs)
        ms = {leg: [] for leg in names}
        n_calls = {leg: max(args.calls, int(np.ceil(WINDOW_S * 1e3 / timed(legs[leg], args.calls)))) for leg in names}
        for r in range(args.reps):
            for leg in names[r % 2:] + names[:r % 2]:
                ms[leg].append(timed(legs[leg], n_calls[leg]))
        dev = first["device"]
        status, steps = dev["status"], dev["steps"]
        host = first["host"]
        both = (status == 0) & (host[4] == 0)
        out = dict(leg="timing", tsr=name, goals=len(goals), seeds=SEEDS, rows=len(of), sigma=args.sigma, reps=args.reps,
                   state=mod.batch_project_state(bid)[0 if name == "BW3" else 1], status=np.bincount(status, minlength=4).tolist(),
                   steps=dict(median=float(np.median(steps[status == 0])) if (status == 0).any() else None, max=int(steps.max())),
                   host_same_status=int((host[4] == status).sum()), host_same_steps=int((host[3] == steps).sum()),
                   host_rows_differ_by=float(np.abs(host[0] - dev["configs"])[both].max()) if both.any() else None)
        for leg in names:
            med = float(np.median(ms[leg]))
            out[leg] = dict(calls_per_window=n_calls[leg], ms=dict(median=med, min=min(ms[leg]), max=max(ms[leg])), us_per_row=med * 1e3 / len(of))
        print(json.dumps(out), flush=True)

        # the goals: a seed on the TSR and clear, checked by the stateless calls on the returned rows
        h = mod.batch_config_tsr(bid, rec, dev["configs"], tsr_of=of)["h"]
        clr = mod.batch_config_clearance(bid, dev["configs"])["clearance"]
        good = (np.abs(h).max(axis=1) <= p["tol"]) & (clr >= np.asarray(p["margin"])).all(axis=1)
        per_goal = good.reshape(len(goals), SEEDS)
        print(json.dumps(dict(leg="goals", tsr=name, in_contact=len(goals), margin=p["margin"], status_0_rows=int((status == 0).sum()),
                              rows_on_the_tsr_and_clear=int(good.sum()), goals_with_such_a_seed=int(per_goal.any(axis=1).sum()))), flush=True)

        # the restatement on the CPU, a subset
        nr = min(args.restated_rows, len(of))
        if nr > 0:
            from oracle import oracle_py as O
            O.build(ref=False)
            w = PC.world(O)
            R = PC.Restated(O, w, tsrs[:int(of[nr - 1]) + 1], of[:nr])
            t0 = time.perf_counter()
            want = R.run(seeds[:nr])
            seconds = time.perf_counter() - t0
            print(json.dumps(dict(leg="restated", tsr=name, rows=nr, seconds=seconds, us_per_row=seconds * 1e6 / nr,
                                  same_status=int((want[4] == status[:nr]).sum()), same_steps=int((want[3] == steps[:nr]).sum()))), flush=True)
            R.destroy()
    mod.batch_destroy(bid)
    mod.close()


if __name__ == "__main__":
    main()
