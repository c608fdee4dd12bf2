"""Per-run scenes, measured: 1024 WAM runs (config 2 shapes, 100 iterations) as
  L1   one scene, the table alone (config 2 itself: the reference leg)
  L1b  one scene, table and mug where they stand (the field count of L2 in one scene)
  L2   64 scenes of 16 runs each, table and mug at seeded random poses, one batch (orc_batch_create_scenes)
  L3   the same 64 scenes as 64 batches of 16 runs (the kinbodies moved before every create), set_num_streams(4),
       all enqueued asynchronously, then synced
in one process, the legs alternated, a warm-up round and REPS (default 7) timed rounds, medians of the rates.  A rate counts the
iterations the runs actually made (iterations_done, as bench.py counts them) over the wall time of enqueue + sync.
Writes profiles/scenes_<build>.json and prints one line.   python scripts/bench_scenes.py [reps]"""
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

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
N_RUNS, N_SCENES, N_ITER = 1024, 64, 100
KW = dict(common.CONFIG2_KW)


def quat_z(a):
    return [0.0, 0.0, np.sin(a / 2), np.cos(a / 2)]


def random_scenes(seed=20261016):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N_SCENES):
        t = [rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 0.0, 0.0, 0.0, 0.0, 1.0]
        m = [rng.uniform(-0.35, 0.15), rng.uniform(-0.25, 0.15), 0.0] + quat_z(rng.uniform(-0.3, 0.3))
        out.append([("table", np.array(t)), ("mug", np.array(m))])
    return out


def wam_module(streams):
    mod = or_cdchomp_amd.Module(0)
    mod.set_num_streams(streams)
    model = common.setup_product_wam(mod)
    return mod, model


def main():
    # two modules in the process: L3's stream pool is a module setting (set before its batches exist)
    mod, model = wam_module(0)
    mod3, _ = wam_module(4)
    mod3.SendCommand("computedistancefield kinbody mug")
    goals = common.wam_goals(N_RUNS, seed=20250101)
    scenes = random_scenes()
    scene_of_run = np.arange(N_RUNS) // (N_RUNS // N_SCENES)

    # L1 is created before the mug has a field (config 2: the table's field alone)
    l1 = [[mod.batch_create(model.name, goals, **KW)] for _ in range(REPS + 1)]
    mod.SendCommand("computedistancefield kinbody mug")
    l1b = [[mod.batch_create(model.name, goals, **KW)] for _ in range(REPS + 1)]
    l2 = [[mod.batch_create(model.name, goals, scenes=scenes, scene_of_run=scene_of_run, **KW)] for _ in range(REPS + 1)]

    def make_l3():
        ids = []
        per = N_RUNS // N_SCENES
        for s, sc in enumerate(scenes):
            for name, pose in sc:
                mod3.set_kinbody_transform(name, pose)
            ids.append(mod3.batch_create(model.name, goals[s * per:(s + 1) * per], **KW))
        for name in ("table", "mug"):
            mod3.set_kinbody_transform(name, [0, 0, 0, 0, 0, 0, 1])
        return ids

    legs = {"L1": (mod, l1), "L1b": (mod, l1b), "L2": (mod, l2), "L3": (mod3, [make_l3() for _ in range(REPS + 1)])}
    rates = {k: [] for k in legs}
    for rnd in range(REPS + 1):
        for name, (m, batches) in legs.items():
            ids = batches[rnd]
            t0 = time.perf_counter()
            for b in ids:
                m.batch_iterate_async(b, N_ITER)
            for b in ids:
                m.batch_sync(b, fetch=False)
            dt = time.perf_counter() - t0
            made = float(sum(m.batch_iterations_done(b).sum() for b in ids))
            if rnd > 0:
                rates[name].append(made / dt)
    for m, batches in legs.values():
        for ids in batches:
            for b in ids:
                m.batch_destroy(b)
    mod.close(); mod3.close()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    rec = dict(build=_capi.csrc_hash(), reps=REPS, n_runs=N_RUNS, n_scenes=N_SCENES, n_iter=N_ITER,
               median_it_per_s=med, rates=rates,
               ratios={"L2/L1": med["L2"] / med["L1"], "L2/L1b": med["L2"] / med["L1b"], "L2/L3": med["L2"] / med["L3"]})
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "scenes_%s.json" % rec["build"]), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(dict(build=rec["build"], **{k: round(v / 1e6, 3) for k, v in med.items()},
                          **{k: round(v, 3) for k, v in rec["ratios"].items()})))


if __name__ == "__main__":
    main()
