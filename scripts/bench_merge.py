"""Merged fields, measured: 1024 WAM runs (config 2 shapes, 100 iterations), one launch at a time, as
  L1   one scene, the table alone                                  (config 2 itself)
  L1b  one scene, table and mug where they stand, two fields
  M1   that scene merged into one world-aligned field, cell = the sources' cell (0.04 m)
  L2   64 scenes of 16 runs, table and mug at seeded random poses  (bench_scenes.py's L2)
  M2   the same 64 scenes, each merged over the robot's reach box
  M2s  the same 64 scenes, each merged over the box around its sources (bounds None)
  M3   twelve box kinbodies with a field each, merged: the scene that does not run unmerged
in one process, the legs alternated, a warm-up round and REPS (default 7) timed rounds, medians of the rates (iterations the
runs made over the wall time of enqueue + sync, as bench_scenes.py counts them).  Then
  M4   wall time of one merge call (kernel, read-back, registration) and of the 64 of M2, against computedistancefield of one
       field of M1's grid size, on the host and on the device
  M5   fidelity: the final total cost of the 1024 goals merged against unmerged (L1b), at cell 0.04 and 0.02: median and
       maximum relative difference, and the share of runs with the same collision verdict.
Writes <out>/merge_<build>.json (default out: profiles/) and prints one line.
   python scripts/bench_merge.py [reps] [--out DIR]
   python scripts/bench_merge.py --trace          one pass of every leg and the merge calls, for a kernel trace
       (rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_merge.py --trace)
   python scripts/bench_merge.py --kernel-times DIR [--out DIR]
       reads that trace and adds kernel times and the merge kernel's bytes per second to the record"""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import common  # noqa: E402
import or_cdchomp_amd  # noqa: E402
from or_cdchomp_amd import _capi, scenes as scene_lib  # noqa: E402

N_RUNS, N_SCENES, N_ITER = 1024, 64, 100
KW = dict(common.CONFIG2_KW)
CELL = 0.04                                                   # computedistancefield's default cube_extent 0.02: cells of 0.04 m
IDENT = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
# the WAM's shoulder stands at (-1, 0, 1); the arm with its hand reaches 1.2 m
REACH = [-2.2, -1.2, -0.2, 0.2, 1.2, 2.2]
PAIR = [("table", None), ("mug", None)]


def random_scenes(seed=20261016):
    """the 64 scenes of bench_scenes.py (the same seed, the same draws)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N_SCENES):
        t = [rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 0.0, 0.0, 0.0, 0.0, 1.0]
        mx, my, a = rng.uniform(-0.35, 0.15), rng.uniform(-0.25, 0.15), rng.uniform(-0.3, 0.3)
        m = [mx, my, 0.0, 0.0, 0.0, np.sin(a / 2), np.cos(a / 2)]
        out.append([("table", np.array(t)), ("mug", np.array(m))])
    return out


def option(name, default=None):
    if name in sys.argv:
        return sys.argv[sys.argv.index(name) + 1]
    return default


def setup():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    mod.SendCommand("computedistancefield kinbody mug")
    shelf = []
    for k in range(12):
        name = "shelf%d" % k
        pos = [0.35 + 0.12 * (k % 4), -0.3 + 0.2 * (k // 4), 0.9 + 0.05 * (k % 3)]
        mod.add_kinbody_boxes(name, [(IDENT, [0.04, 0.04, 0.04])], transform=pos + [0.0, 0.0, 0.0, 1.0])
        mod.SendCommand("computedistancefield kinbody %s" % name)
        shelf.append((name, None))
    return mod, model, shelf


def merge_into(mod, name, fields, cell, bounds=None):
    mod.add_kinbody_boxes(name, [], transform=IDENT)
    t0 = time.perf_counter()
    mod.merge_fields(name, fields, cell, bounds)
    return time.perf_counter() - t0


def grid_bytes(mod, names):
    return int(sum(mod.get_sdf(nm)[0].size * 8 for nm in names))


def scene_tables(mod, shelf):
    """the scene list and scene_of_run of every leg; the merges are timed on the way (M4)"""
    scenes = random_scenes()
    per16 = np.arange(N_RUNS) // (N_RUNS // N_SCENES)
    zero = np.zeros(N_RUNS, dtype=np.int32)
    t = {}
    t["merge_m1_s"] = [merge_into(mod, "m1_%d" % k, PAIR, CELL) for k in range(8)][1:]      # (the first call uploads the sources)
    t0 = time.perf_counter()
    m2 = scene_lib.merged_scenes(mod, scenes, CELL, bounds=REACH, prefix="m2r")
    t["merge_64_reach_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    m2s = scene_lib.merged_scenes(mod, scenes, CELL, bounds=None, prefix="m2s")
    t["merge_64_sources_s"] = time.perf_counter() - t0
    t["merge_m3_s"] = merge_into(mod, "m3", shelf, CELL)
    legs = {
        "L1": ([[("table", None)]], zero), "L1b": ([PAIR], zero), "M1": ([[("m1_0", None)]], zero),
        "L2": (scenes, per16), "M2": (m2, per16), "M2s": (m2s, per16), "M3": ([[("m3", None)]], zero),
    }
    sizes = {
        "sources": {nm: list(mod.get_sdf(nm)[0].shape) for nm in ("table", "mug", "shelf0")},
        "M1": list(mod.get_sdf("m1_0")[0].shape), "M2": list(mod.get_sdf("m2r0")[0].shape),
        "M2s": list(mod.get_sdf("m2s0")[0].shape), "M3": list(mod.get_sdf("m3")[0].shape),
    }
    nbytes = {"L1": grid_bytes(mod, ["table"]), "L1b/L2": grid_bytes(mod, ["table", "mug"]), "M1": grid_bytes(mod, ["m1_0"]),
              "M2": grid_bytes(mod, ["m2r%d" % s for s in range(N_SCENES)]),
              "M2s": grid_bytes(mod, ["m2s%d" % s for s in range(N_SCENES)]), "M3": grid_bytes(mod, ["m3"]),
              "M3_sources": grid_bytes(mod, [nm for nm, _ in shelf])}
    return legs, t, sizes, nbytes


def computedistancefield_times(mod, sizes):
    """computedistancefield of one box kinbody whose grid has `sizes` cells (cube_extent 0.02, aabb_padding 0.2): the other
    route to a single field.  Seconds on the host path and on the device path."""
    half = [s * 0.02 - 0.2 - 0.005 for s in sizes]
    out = {}
    for leg, env in (("host", "0"), ("device", "1")):
        times = []
        for k in range(4):
            name = "cdf_%s%d" % (leg, k)
            mod.add_kinbody_boxes(name, [(IDENT, half)], transform=[5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 1.0])
            os.environ["ORC_SDF_DEVICE"] = env
            t0 = time.perf_counter()
            mod.SendCommand("computedistancefield kinbody %s" % name)
            times.append(time.perf_counter() - t0)
            assert list(mod.get_sdf(name)[0].shape) == list(sizes), (mod.get_sdf(name)[0].shape, sizes)
            mod.SendCommand("removefield kinbody %s" % name)
            mod.enable_kinbody(name, False)
        del os.environ["ORC_SDF_DEVICE"]
        out[leg] = times[1:]
    return out


def fidelity(mod, model, goals):
    """M5: the final total cost and the collision verdict of every goal, unmerged (L1b) and merged at two cell sizes"""
    zero = np.zeros(N_RUNS, dtype=np.int32)

    def run(scene):
        bid = mod.batch_create(model.name, goals, scenes=[scene], scene_of_run=zero, **KW)
        costs, status = mod.batch_iterate(bid, N_ITER)
        hit = mod.batch_collision_verdict(bid, on_device=True, runs="candidates")["collides"]      # (-1: no candidate)
        mod.batch_destroy(bid)
        return costs[:, 0], status, hit

    base, bstat, bhit = run(PAIR)
    out = {}

    def compare(c, st, hit, **extra):
        ok = np.isfinite(base) & np.isfinite(c) & (base != 0)
        rel = np.abs(c[ok] - base[ok]) / np.abs(base[ok])
        return dict(runs_compared=int(ok.sum()), median_rel_cost_diff=float(np.median(rel)), max_rel_cost_diff=float(rel.max()),
                    p90_rel_cost_diff=float(np.quantile(rel, 0.9)), same_verdict_share=float(np.mean(hit == bhit)),
                    same_status_share=float(np.mean(st == bstat)), colliding_unmerged=int((bhit == 1).sum()),
                    colliding_merged=int((hit == 1).sum()), **extra)

    # the yardstick for those differences: the same two-field scene, unmerged, with the mug moved by one millimetre
    c, st, hit = run([("table", None), ("mug", [0.001, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])])
    out["control_unmerged_mug_moved_1mm"] = compare(c, st, hit)
    for cell in (CELL, CELL / 2):
        name = "fid_%d" % round(cell * 1000)
        merge_into(mod, name, PAIR, cell)
        c, st, hit = run([(name, None)])
        out["cell_%g" % cell] = compare(c, st, hit, grid=list(mod.get_sdf(name)[0].shape))
    return out


def trace_pass():
    """what the kernel trace sees, in this order: the merges (M1 x3, M1 at half the cell, reach box, M3), then one warm-up and
    three launches of every leg, each on a fresh batch"""
    mod, model, shelf = setup()
    goals = common.wam_goals(N_RUNS, seed=20250101)
    for k in range(3):
        merge_into(mod, "t_m1_%d" % k, PAIR, CELL)
    merge_into(mod, "t_half", PAIR, CELL / 2)
    merge_into(mod, "t_reach", PAIR, CELL, REACH)
    merge_into(mod, "t_m3", shelf, CELL)
    legs, _, _, _ = scene_tables(mod, shelf)
    for name, (scenes, sor) in legs.items():
        for _ in range(4):               # (a fresh batch per launch, as the timed legs have: the first 100 iterations of a run)
            bid = mod.batch_create(model.name, goals, scenes=scenes, scene_of_run=sor, **KW)
            mod.batch_iterate_async(bid, N_ITER)
            mod.batch_sync(bid, fetch=False)
            mod.batch_destroy(bid)
    print("trace order: merges m1 m1 m1 half reach m3 | 8 m1, 64 reach, 64 sources, m3 | legs " + " ".join(legs))
    mod.close()


def kernel_times(trace_dir, out_dir):
    """kernel milliseconds from a rocprofv3 kernel trace of --trace, added to the newest record of out_dir"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    merges = [(e - s) / 1e6 for s, e, nm in rows if "merge_fields_kernel" in nm]
    iters = [(e - s) / 1e6 for s, e, nm in rows if "chomp_iterate_kernel" in nm]
    legs = ["L1", "L1b", "M1", "L2", "M2", "M2s", "M3"]
    if len(merges) != 6 + 8 + 64 + 64 + 1 or len(iters) != 4 * len(legs):
        raise SystemExit("the trace is not one of --trace: %d merge and %d iterate kernels" % (len(merges), len(iters)))
    rec_path = sorted(glob.glob(os.path.join(out_dir, "merge_*.json")), key=os.path.getmtime)[-1]
    rec = json.load(open(rec_path))
    kt = {"iterate_ms": {leg: float(np.median(iters[4 * k + 1:4 * k + 4])) for k, leg in enumerate(legs)},
          "merge_ms": {"m1": float(np.median(merges[1:3])), "m1_half_cell": merges[3], "reach_box": merges[4], "m3": merges[5],
                       "m2_reach_64_median": float(np.median(merges[14:78])), "m2_sources_64_median": float(np.median(merges[78:142]))}}
    src = rec["grid_bytes"]["L1b/L2"]

    def floor_bytes(shape, source_bytes):
        return int(np.prod(shape)) * 8 + source_bytes

    fb = {"m1": floor_bytes(rec["grid_sizes"]["M1"], src), "reach_box": floor_bytes(rec["grid_sizes"]["M2"], src),
          "m3": floor_bytes(rec["grid_sizes"]["M3"], rec["grid_bytes"]["M3_sources"])}
    kt["it_per_s_by_kernel_time"] = {leg: rec["iterations_made"][leg] / (kt["iterate_ms"][leg] * 1e-3) for leg in legs}
    kt["merge_floor_bytes"] = fb
    kt["merge_GB_per_s_of_floor"] = {k: fb[k] / (kt["merge_ms"][k] * 1e-3) / 1e9 for k in fb}
    rec["kernel_times"] = kt
    json.dump(rec, open(rec_path, "w"), indent=1)
    print(json.dumps(kt))


def main():
    out_dir = option("--out", os.path.join(ROOT, "profiles"))
    if "--trace" in sys.argv:
        return trace_pass()
    if "--kernel-times" in sys.argv:
        return kernel_times(option("--kernel-times"), out_dir)
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 7
    mod, model, shelf = setup()
    goals = common.wam_goals(N_RUNS, seed=20250101)
    legs, merge_s, sizes, nbytes = scene_tables(mod, shelf)
    batches = {name: [mod.batch_create(model.name, goals, scenes=sc, scene_of_run=sor, **KW) for _ in range(reps + 1)]
               for name, (sc, sor) in legs.items()}
    plans = {name: mod.batch_plan(ids[0])["variant"] for name, ids in batches.items()}
    rates = {k: [] for k in legs}
    made_by = {}
    for rnd in range(reps + 1):
        for name, ids in batches.items():
            b = ids[rnd]
            t0 = time.perf_counter()
            mod.batch_iterate_async(b, N_ITER)
            mod.batch_sync(b, fetch=False)
            dt = time.perf_counter() - t0
            made = float(mod.batch_iterations_done(b).sum())
            made_by[name] = made          # (the same every round: the batches of a leg are the same problem)
            if rnd > 0:
                rates[name].append(made / dt)
    for ids in batches.values():
        for b in ids:
            mod.batch_destroy(b)
    cdf = computedistancefield_times(mod, sizes["M1"])
    fid = fidelity(mod, model, goals)
    mod.close()
    med = {k: float(np.median(v)) for k, v in rates.items()}
    spread = {k: [float(min(v)), float(max(v))] for k, v in rates.items()}
    rec = dict(build=_capi.csrc_hash(), reps=reps, n_runs=N_RUNS, n_scenes=N_SCENES, n_iter=N_ITER, cell=CELL, reach_box=REACH,
               median_it_per_s=med, min_max_it_per_s=spread, rates=rates, iterations_made=made_by, variant=plans, grid_sizes=sizes, grid_bytes=nbytes,
               ratios={"M1/L1b": med["M1"] / med["L1b"], "M1/L1": med["M1"] / med["L1"], "M2/L2": med["M2"] / med["L2"],
                       "M2s/L2": med["M2s"] / med["L2"]},
               merge_call_s=dict(one_m1_median=float(np.median(merge_s["merge_m1_s"])), one_m1=merge_s["merge_m1_s"],
                                 m3=merge_s["merge_m3_s"], sixty_four_reach=merge_s["merge_64_reach_s"],
                                 sixty_four_sources=merge_s["merge_64_sources_s"]),
               computedistancefield_s=dict(host_median=float(np.median(cdf["host"])), device_median=float(np.median(cdf["device"])),
                                           host=cdf["host"], device=cdf["device"], grid=sizes["M1"]),
               fidelity=fid)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "merge_%s.json" % rec["build"]), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(dict(build=rec["build"], **{k: round(v / 1e6, 3) for k, v in med.items()},
                          **{k: round(v, 3) for k, v in rec["ratios"].items()},
                          merge_ms=round(rec["merge_call_s"]["one_m1_median"] * 1e3, 3),
                          cdf_host_ms=round(rec["computedistancefield_s"]["host_median"] * 1e3, 1),
                          cdf_device_ms=round(rec["computedistancefield_s"]["device_median"] * 1e3, 1), fidelity=fid)))


if __name__ == "__main__":
    main()
