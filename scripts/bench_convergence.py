"""The convergence stop (orc_batch_set_convergence), measured: the same runs with a fixed n_iter and with the criterion
(rtol, patience; the same n_iter as the cap), on
  c3_block  one 8 192-run block of config 3 (WAM, n_points 100, one batch)
  c2        config 2's 1 024 runs as two batches of 512 on two streams (set_num_streams(2)), enqueued, then synced
in one process, the two legs alternated, a warm-up round and REPS (default 5) timed rounds, medians.  Per leg: wall time of
enqueue + sync, the sum of the iterations the runs made (iterations_done), the time per iteration made, and for the
criterion the share of runs that stopped and the histogram of their stop iterations (status 1; bins of 10 iterations).
Writes profiles/convergence_<build>.json and prints one line.
   python scripts/bench_convergence.py [reps] [n_iter] [rtol] [patience]"""
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

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N_ITER = int(sys.argv[2]) if len(sys.argv) > 2 else 200
RTOL = float(sys.argv[3]) if len(sys.argv) > 3 else 1e-4
PATIENCE = int(sys.argv[4]) if len(sys.argv) > 4 else 5
KW = dict(common.CONFIG2_KW)


def measure(mod, make):
    """legs 'fixed' and 'converge' alternated; returns {leg: record}"""
    rec = {}
    samples = {"fixed": [], "converge": []}
    for rnd in range(REPS + 1):
        for leg in ("fixed", "converge"):
            ids = make()
            if leg == "converge":
                for b in ids:
                    mod.batch_set_convergence(b, RTOL, PATIENCE)
            mod.batch_sync(ids[0], fetch=False)
            t0 = time.perf_counter()
            for b in ids:
                mod.batch_iterate_async(b, N_ITER)
            for b in ids:
                mod.batch_sync(b, fetch=False)
            dt = time.perf_counter() - t0
            iters = np.concatenate([mod.batch_iterations_done(b) for b in ids])
            status = np.concatenate([mod.batch_sync(b)[1] for b in ids])
            for b in ids:
                mod.batch_destroy(b)
            if rnd > 0:
                samples[leg].append((dt, int(iters.sum())))
            if rnd == REPS:
                stopped = status == 1
                hist, edges = np.histogram(iters[stopped], bins=np.arange(0, N_ITER + 11, 10))
                rec[leg] = dict(runs=int(len(iters)), stopped_share=float(stopped.mean()), aborted=int((status == -1).sum()),
                                stop_hist={"%d-%d" % (edges[i], edges[i + 1] - 1): int(h) for i, h in enumerate(hist) if h},
                                stop_iter_median=float(np.median(iters[stopped])) if stopped.any() else None)
    for leg, s in samples.items():
        dts = np.array([d for d, _ in s]); made = np.array([m for _, m in s])
        rec[leg].update(wall_s_median=float(np.median(dts)), wall_s=[float(d) for d in dts], iters_made=int(np.median(made)),
                        us_per_iter_made=float(np.median(dts / made) * 1e6), it_per_s_made=float(np.median(made / dts)))
    rec["wall_ratio"] = rec["converge"]["wall_s_median"] / rec["fixed"]["wall_s_median"]
    return rec


def main():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    goals3 = common.config3_goals(rank=0, world=8)
    c3 = measure(mod, lambda: [mod.batch_create(model.name, goals3, **KW)])
    mod.close()

    mod = or_cdchomp_amd.Module(0)
    mod.set_num_streams(2)
    model = common.setup_product_wam(mod)
    goals2 = common.wam_goals(1024, seed=20250101)
    c2 = measure(mod, lambda: [mod.batch_create(model.name, goals2[:512], **KW), mod.batch_create(model.name, goals2[512:], **KW)])
    mod.close()

    rec = dict(build=_capi.csrc_hash(), reps=REPS, n_iter=N_ITER, rtol=RTOL, patience=PATIENCE, c3_block=c3, c2_two_streams=c2)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "convergence_%s.json" % rec["build"]), "w") as f:
        json.dump(rec, f, indent=1)
    short = lambda r: dict(fixed_s=round(r["fixed"]["wall_s_median"], 4), converge_s=round(r["converge"]["wall_s_median"], 4),
                           ratio=round(r["wall_ratio"], 3), stopped=round(r["converge"]["stopped_share"], 3),
                           iters_made=(r["fixed"]["iters_made"], r["converge"]["iters_made"]),
                           us_per_iter=(round(r["fixed"]["us_per_iter_made"], 4), round(r["converge"]["us_per_iter_made"], 4)))
    print(json.dumps(dict(build=rec["build"], c3_block=short(c3), c2=short(c2))))


if __name__ == "__main__":
    main()
