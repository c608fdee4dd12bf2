"""orc_batch_project_tsr measured on the WAM tabletop (NOTES/project-tsr.md): batched inverse kinematics for config 2's goals.
  1 024 target poses -- the hand poses (manipulator `arm`) at common.wam_goals(1024) -- x 16 seeds, the goal plus a Gaussian of
  sigma 0.3 per joint, clipped to the joint limits: 16 384 rows, six enforced rows each, the defaults of batch_project_tsr.
  device   Module.batch_project_tsr: one call, the whole iteration in one kernel
  host     the same step rule (project.project) as a host loop around Module.batch_config_tsr of the same build
           both alternated: a warm-up of each, then REPS rounds (default 8) of one timed window per leg -- CALLS calls at least
           (default 3), and as many as fill 0.2 s --, the order rotating; medians with min .. max
  oracle   project.project around the oracle's eval_contsr on the CPU, over the first ORACLE_TARGETS targets' rows, once
  contact  of the goals in contact (batch_config_clearance < 0), for how many at least one of the 16 projected seeds is done and
           clear at margins (0.02, 0): a figure beside push-out's (scripts/bench_penetration.py), not a criterion
All device calls end in a synchronise; the clock is the host's around them.  Prints one JSON line per leg.
   python scripts/bench_project_tsr.py [--reps N] [--calls N] [--oracle-targets N] [--sigma S]"""
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
import or_cdchomp_amd  # noqa: E402
from or_cdchomp_amd import project  # noqa: E402

SEEDS, SIGMA, MARGIN, WINDOW_S = 16, 0.3, (0.02, 0.0), 0.2


def timed(f, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        f()
    return (time.perf_counter() - t0) / calls * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--oracle-targets", type=int, default=64)
    ap.add_argument("--sigma", type=float, default=SIGMA)
    args = ap.parse_args()
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    _, base, dofvals, adofs = common.wam_state()
    goals = common.wam_goals(1024)
    lo, hi = PJ.wam_limits()
    Rs, ds = PJ.target_frames(model, base, dofvals, adofs, "handbase", PJ.TOOL, goals)
    tsrs = PJ.tsrs_at(Rs, ds, PJ.BW6)
    rng = np.random.default_rng(1)
    of = np.repeat(np.arange(len(goals)), SEEDS).astype(np.int32)
    seeds = np.clip(goals[of] + args.sigma * rng.normal(size=(len(of), 7)), lo, hi)
    bid = mod.batch_create(model.name, goals[:1], **common.CONFIG2_KW)
    rec = mod.batch_tsr_records(bid, tsrs)
    ks = rec[1][of]

    def evaluate(rows, index):
        res = mod.batch_config_tsr(bid, rec, rows, tsr_of=of[index])
        return res["h"], res["jac"]

    legs = dict(device=lambda: mod.batch_project_tsr(bid, rec, seeds, tsr_of=of, lower=lo, upper=hi),
                host=lambda: project.project(evaluate, seeds, lower=lo, upper=hi, k=ks, indexed=True))
    first = {name: f() for name, f in legs.items()}
    names = list(legs)
    ms = {name: [] for name in names}
    n_calls = {name: max(args.calls, int(np.ceil(WINDOW_S * 1e3 / timed(legs[name], args.calls)))) for name in names}
    for r in range(args.reps):
        for name in names[r % 2:] + names[:r % 2]:
            ms[name].append(timed(legs[name], n_calls[name]))
    rows, resid, steps, status = first["device"]
    out = dict(leg="timing", targets=len(goals), seeds=SEEDS, rows=len(of), sigma=args.sigma, reps=args.reps, state=mod.batch_project_state(bid),
               status=np.bincount(status, minlength=4).tolist(), steps=dict(median=float(np.median(steps[status == 0])), max=int(steps.max())),
               host_same_status=int((first["host"][3] == status).sum()), host_same_steps=int((first["host"][2] == steps).sum()),
               host_rows_differ_by=float(np.abs(first["host"][0] - rows)[status == 0].max()))
    for name in names:
        med = float(np.median(ms[name]))
        out[name] = dict(calls_per_window=n_calls[name], ms=dict(median=med, min=min(ms[name]), max=max(ms[name])), us_per_row=med * 1e3 / len(of))
    print(json.dumps(out), flush=True)

    # the oracle on the CPU, a subset
    from oracle import oracle_py as O
    O.build(ref=False)
    nt = min(args.oracle_targets, len(goals))
    sub = of < nt
    ora = PJ.OracleTsrs(O, model, base, dofvals, adofs, "handbase", PJ.TOOL, tsrs[:nt], tsr_of=of[sub])
    t0 = time.perf_counter()
    want = ora.project(seeds[sub], lower=lo, upper=hi)
    seconds = time.perf_counter() - t0
    print(json.dumps(dict(leg="oracle", targets=nt, rows=int(sub.sum()), seconds=seconds, us_per_row=seconds * 1e6 / int(sub.sum()),
                          same_status=int((want[3] == status[sub]).sum()), same_steps=int((want[2] == steps[sub]).sum()))), flush=True)
    ora.destroy()

    # the goals in contact: another solution for the same hand pose
    before = mod.batch_config_clearance(bid, goals)["clearance"]
    hit = np.fmin(before[:, 0], before[:, 1]) < 0
    clr = mod.batch_config_clearance(bid, rows)["clearance"]
    clear = (status == 0) & (clr >= np.asarray(MARGIN)).all(axis=1)
    per_goal = clear.reshape(len(goals), SEEDS)
    done_goal = (status == 0).reshape(len(goals), SEEDS)
    print(json.dumps(dict(leg="contact", goals=len(goals), in_contact=int(hit.sum()), margin=MARGIN,
                          with_a_clear_seed=int(per_goal[hit].any(axis=1).sum()), with_a_done_seed=int(done_goal[hit].any(axis=1).sum()),
                          clear_seeds_per_goal_in_contact=float(per_goal[hit].sum(axis=1).mean()),
                          goals_not_in_contact_with_a_clear_seed=int(per_goal[~hit].any(axis=1).sum()), not_in_contact=int((~hit).sum()))), flush=True)
    mod.batch_destroy(bid)
    mod.close()


if __name__ == "__main__":
    main()
