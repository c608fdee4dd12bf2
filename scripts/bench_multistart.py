"""Multi-start batches (orc_batch_perturb, orc_batch_select_best, orc_batch_gettraj_runs), measured on the WAM tabletop:
  seeding   one 8 192-run block, n_points 100: wall time of batch_perturb against the route a caller has without it -- the
            same kind of displacement built on the host with numpy (Gaussians, the dense A^-1, clip) and uploaded with
            batch_set_traj (45 MB)
  result    the same block as 64 problems x 128 starts after 100 iterations: batch_select_best(collision_free=False) +
            batch_gettraj_runs against batch_sync + batch_gettraj of everything + numpy; and the time of
            batch_select_best(collision_free=True), whose verdict plans its samples on the device
  verdict   (--parent-lib FILE) the same block and iterations in child processes, this build and the parent's library
            (loaded through ORC_LIB) alternated, a warm-up and REPS rounds: wall time of batch_select_best(collision_free=
            True), of the host-planned and the device-planned batch_collision_verdict, and the bytes each moves over the
            host link.  --verdict-child is such a child; --verdict-trace runs one of each verdict and nothing else, for
            a kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/bench_multistart.py --verdict-trace)
  gain      config 2's 1 024 goals as K = 1 (unperturbed) and as K = 16 perturbed starts at several sigma, 100 iterations:
            the share of problems with an eligible collision-free winner and the winning cost against K = 1
in one process, the legs of a comparison alternated, a warm-up round and REPS (default 5) timed rounds, medians.
Writes profiles/multistart_<build>.json and prints one line.
   python scripts/bench_multistart.py [--reps N] [--host-only --out FILE] [--parent-record FILE] [--headline FILE]
                                      [--parent-lib FILE] [--kernel-stats FILE]
--host-only: only the host routes (what a library built from the commit before the three calls can run; with ORC_LIB set
to such a library the three symbols are not bound) written to FILE; --parent-record embeds such a file in the record;
--headline embeds a JSON file of bench.py headline values of this build and its parent, taken next to it."""
import argparse
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

NEW = ("orc_batch_perturb", "orc_batch_select_best", "orc_batch_gettraj_runs")
KW = dict(common.CONFIG2_KW)
N_BLOCK, N_PROBLEMS, N_STARTS = 8192, 64, 128
SIGMA = 0.3


def med(xs):
    return float(np.median(xs))


def host_inverse(m, dt):
    A = np.zeros((m, m))
    assert _capi.lib().orc_host_metric(m, 1, dt, A.ctypes.data_as(_capi.c_double_p), None, None, None, None, 0, None) == 0
    Ainv = np.linalg.inv(A)
    return Ainv / np.linalg.norm(Ainv[m // 2])


def host_seed(mod, bid, start, Ainv_c, lo, hi, rng):
    """the caller's route: displacements with numpy, the whole trajectory array over the host link"""
    t0 = time.perf_counter()
    n_runs, n_points, n = start.shape
    xi = rng.standard_normal((n_runs, n_points - 2, n))
    traj = start.copy()
    traj[:, 1:-1] += SIGMA * np.einsum("ij,rjc->ric", Ainv_c, xi, optimize=True)
    np.clip(traj[:, 1:-1], lo, hi, out=traj[:, 1:-1])
    t1 = time.perf_counter()
    mod.batch_set_traj(bid, traj)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, traj.nbytes


def host_select(mod, bid, group, n_groups):
    """the caller's route: costs, status and every trajectory to the host, the reduction in numpy"""
    t0 = time.perf_counter()
    costs, status = mod.batch_sync(bid)
    traj = mod.batch_gettraj(bid)
    c = np.where(((status == 0) | (status == 1)) & np.isfinite(costs[:, 0]), costs[:, 0], np.inf)
    order = np.lexsort((np.arange(len(c)), c, group))                 # by group, then cost, then run
    first = order[np.searchsorted(group[order], np.arange(n_groups))]
    best = np.where(np.isfinite(c[first]), first, -1)
    out = np.where((best >= 0)[:, None, None], traj[np.maximum(best, 0)], np.nan)
    return time.perf_counter() - t0, best, out, costs.nbytes + status.nbytes + traj.nbytes


def block(args, mod, model):
    goals = np.repeat(common.wam_goals(N_PROBLEMS, seed=20250101), N_STARTS, axis=0)
    seeds = np.arange(N_BLOCK, dtype=np.uint32) + 1
    group = np.repeat(np.arange(N_PROBLEMS, dtype=np.int32), N_STARTS)
    lo, hi = np.asarray(model.limit_lower[:7]), np.asarray(model.limit_upper[:7])
    bid = mod.batch_create(model.name, goals, **KW)
    start = mod.batch_gettraj(bid)
    Ainv_c = host_inverse(KW["n_points"] - 2, 1.0 / (KW["n_points"] - 1))
    rng = np.random.default_rng(1)
    s = dict(device=[], host_build=[], host_upload=[])
    for rnd in range(args.reps + 1):
        mod.batch_set_traj(bid, start)
        if not args.host_only:
            t0 = time.perf_counter()
            mod.batch_perturb(bid, SIGMA, seeds)                      # (returns after the device has finished)
            dt = time.perf_counter() - t0
            if rnd:
                s["device"].append(dt)
            mod.batch_set_traj(bid, start)
        tb, tu, nbytes = host_seed(mod, bid, start, Ainv_c, lo, hi, rng)
        if rnd:
            s["host_build"].append(tb); s["host_upload"].append(tu)
    seeding = dict(runs=N_BLOCK, n_points=KW["n_points"], sigma=SIGMA, host_bytes=int(nbytes),
                   host_build_s=med(s["host_build"]), host_upload_s=med(s["host_upload"]),
                   host_total_s=med(np.add(s["host_build"], s["host_upload"])),
                   host_total_all=[float(a + b) for a, b in zip(s["host_build"], s["host_upload"])])
    if not args.host_only:
        seeding.update(device_s=med(s["device"]), device_all=[float(x) for x in s["device"]], device_bytes=int(seeds.nbytes),
                       host_over_device=seeding["host_total_s"] / med(s["device"]))

    mod.batch_set_traj(bid, start)
    if not args.host_only:
        mod.batch_perturb(bid, SIGMA, seeds)
    else:
        host_seed(mod, bid, start, Ainv_c, lo, hi, np.random.default_rng(1))
    mod.batch_iterate(bid, 100)
    r = dict(device=[], host=[], device_cf=[])
    for rnd in range(args.reps + 1):
        if not args.host_only:
            t0 = time.perf_counter()
            best, cost, cnt = mod.batch_select_best(bid, n_groups=N_PROBLEMS, collision_free=False)
            rows = mod.batch_gettraj_runs(bid, best)
            dt = time.perf_counter() - t0
            if rnd:
                r["device"].append(dt)
        th, hbest, hrows, hbytes = host_select(mod, bid, group, N_PROBLEMS)
        if rnd:
            r["host"].append(th)
        if not args.host_only:
            assert np.array_equal(best, hbest) and np.array_equal(rows, hrows, equal_nan=True)
            if rnd:
                t0 = time.perf_counter()
                mod.batch_select_best(bid, n_groups=N_PROBLEMS, collision_free=True)
                r["device_cf"].append(time.perf_counter() - t0)
    result = dict(problems=N_PROBLEMS, starts=N_STARTS, host_s=med(r["host"]), host_all=[float(x) for x in r["host"]], host_bytes=int(hbytes))
    if not args.host_only:
        result.update(device_s=med(r["device"]), device_all=[float(x) for x in r["device"]],
                      device_bytes=int(rows.nbytes + best.nbytes + cost.nbytes + cnt.nbytes), host_over_device=result["host_s"] / med(r["device"]),
                      device_collision_free_s=med(r["device_cf"]), winners=int((best >= 0).sum()))
    mod.batch_destroy(bid)
    return seeding, result


def iterated_block(mod, model):
    """the 8 192-run block, perturbed and iterated 100 times"""
    goals = np.repeat(common.wam_goals(N_PROBLEMS, seed=20250101), N_STARTS, axis=0)
    bid = mod.batch_create(model.name, goals, **KW)
    mod.batch_perturb(bid, SIGMA, np.arange(N_BLOCK, dtype=np.uint32) + 1)
    mod.batch_iterate(bid, 100)
    return bid


def device_link_bytes(mod, bid, select):
    """bytes the device-planned verdict moves over the host link, counted from what the route copies: vmax, the slot table and
    the tables of the self-collision leg up (the WAM's 15 spheres: at most 105 pairs of four ints and a radius sum), the
    too-long flag down; then keys, depths, times and sample counts down -- or, for batch_select_best(collision_free=True),
    which leaves them on the device, the groups up and n_groups triples down.  Also returns the samples of all runs."""
    n_runs, n_points, n = mod.batch_dims(bid)
    samples = int(mod.batch_collision_verdict(bid, on_device=True)["n_samples"].sum())
    tables = n * 8 + 16 * 4 + 105 * (16 + 8) + 4
    if select:
        return tables + n_runs * 4 + N_PROBLEMS * (8 + 4 + 4), samples
    return tables + n_runs * (8 + 8 + 8 + 4), samples


def verdict_child(args):
    """one build's leg of a round: wall times of the three calls on the iterated block"""
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    bid = iterated_block(mod, model)
    rec = dict(lib=os.path.basename(_capi.LIB_PATH), select_cf_s=[], verdict_host_s=[], verdict_device_s=[])
    for rnd in range(2):                                     # (a warm-up, then the timed call)
        t0 = time.perf_counter()
        best = mod.batch_select_best(bid, n_groups=N_PROBLEMS, collision_free=True)
        rec["select_cf_s"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        host = mod.batch_collision_verdict(bid)
        rec["verdict_host_s"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        dev = mod.batch_collision_verdict(bid, on_device=True)
        rec["verdict_device_s"].append(time.perf_counter() - t0)
        assert all(np.array_equal(dev[k], host[k]) for k in host)
    rec = {k: (v[-1] if isinstance(v, list) else v) for k, v in rec.items()}
    rec.update(winners=[int(x) for x in best[0]], colliding=int(host["collides"].sum()))
    n_runs, n_points, n = mod.batch_dims(bid)
    rec["select_cf_bytes"], rec["samples"] = device_link_bytes(mod, bid, True)
    rec["verdict_device_bytes"] = device_link_bytes(mod, bid, False)[0]
    # the host-planned route: the trajectories down, 4 (n_runs + 1) + (4 + 8) samples up, keys and depths down
    rec["verdict_host_bytes"] = n_runs * n_points * n * 8 + 4 * (n_runs + 1) + 12 * rec["samples"] + n_runs * 16
    mod.batch_destroy(bid)
    mod.close()
    print("VERDICT_CHILD " + json.dumps(rec))


def verdict_trace():
    """one host-planned and one device-planned verdict of the iterated block, for a kernel trace"""
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    bid = iterated_block(mod, model)
    for _ in range(3):
        host = mod.batch_collision_verdict(bid)
        dev = mod.batch_collision_verdict(bid, on_device=True)
    assert all(np.array_equal(dev[k], host[k]) for k in host)
    mod.batch_destroy(bid)
    mod.close()


def verdict_rounds(args):
    """this build and the parent's library alternated in child processes"""
    legs = dict(this=[], parent=[])
    for rnd in range(args.reps + 1):
        for name in ("parent", "this"):
            env = dict(os.environ)
            env.pop("ORC_LIB", None)
            if name == "parent":
                env["ORC_LIB"] = os.path.abspath(args.parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--verdict-child"], env=env, check=True,
                                 stdout=subprocess.PIPE, timeout=600).stdout.decode()
            rec = json.loads([ln for ln in out.splitlines() if ln.startswith("VERDICT_CHILD ")][-1][len("VERDICT_CHILD "):])
            if rnd:
                legs[name].append(rec)
    assert all(r["winners"] == legs["this"][0]["winners"] for r in legs["this"] + legs["parent"]), "the builds must select the same runs"
    out = dict(runs=N_BLOCK, rounds=args.reps)
    for name, recs in legs.items():
        for key in ("select_cf_s", "verdict_host_s", "verdict_device_s"):
            out["%s_%s" % (name, key)] = med([r[key] for r in recs])
            out["%s_%s_all" % (name, key)] = [r[key] for r in recs]
    last = legs["this"][-1]
    out.update(samples=last["samples"], colliding=last["colliding"], select_cf_bytes=last["select_cf_bytes"],
               verdict_device_bytes=last["verdict_device_bytes"], verdict_host_bytes=last["verdict_host_bytes"],
               parent_over_this_select_cf=out["parent_select_cf_s"] / out["this_select_cf_s"])
    return out


def gain(mod, model, K=16, sigmas=(0.1, 0.3, 0.6)):
    goals = common.wam_goals(1024, seed=20250101)
    P = len(goals)
    out = {}

    def leg(k, sigma):
        bid = mod.batch_create(model.name, np.repeat(goals, k, axis=0), **KW)
        if sigma:
            mod.batch_perturb(bid, sigma, np.arange(P * k, dtype=np.uint32) + 1)
        _, status = mod.batch_iterate(bid, 100)
        best, cost, cnt = mod.batch_select_best(bid, n_groups=P, collision_free=True)
        _, cost_any, _ = mod.batch_select_best(bid, n_groups=P, collision_free=False)
        mod.batch_destroy(bid)
        return dict(best=best, cost=cost, cost_any=cost_any, aborted=float((status == -1).mean()), eligible_runs=float(cnt.sum() / (P * k)))

    one = leg(1, 0.0)
    has1 = one["best"] >= 0
    out["K1"] = dict(share_with_winner=float(has1.mean()), median_cost=med(one["cost"][has1]), aborted_share=one["aborted"])
    for sg in sigmas:
        many = leg(K, sg)
        has = many["best"] >= 0
        both = has & has1
        out["K%d_sigma%g" % (K, sg)] = dict(
            share_with_winner=float(has.mean()), gained=int((has & ~has1).sum()), lost=int((~has & has1).sum()),
            median_cost=med(many["cost"][has]), median_cost_ratio_to_K1=med(many["cost"][both] / one["cost"][both]),
            share_cheaper_than_K1=float((many["cost"][both] < one["cost"][both]).mean()),
            aborted_share=many["aborted"], eligible_share_of_runs=many["eligible_runs"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-record", default="")
    ap.add_argument("--headline", default="")
    ap.add_argument("--parent-lib", default="", help="the parent build's library: adds the verdict leg")
    ap.add_argument("--kernel-stats", default="", help="a JSON file of kernel durations from a trace of --verdict-trace, embedded")
    ap.add_argument("--verdict-child", action="store_true")
    ap.add_argument("--verdict-trace", action="store_true")
    args = ap.parse_args()
    if args.verdict_child:
        return verdict_child(args)
    if args.verdict_trace:
        return verdict_trace()
    if args.host_only:
        _capi.SYMBOLS = [s for s in _capi.SYMBOLS if s[0] not in NEW]
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    seeding, result = block(args, mod, model)
    rec = dict(build=_capi.csrc_hash(), lib=os.path.basename(_capi.LIB_PATH), reps=args.reps, seeding=seeding, result=result)
    if args.host_only:
        mod.close()
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps(dict(host_only=True, seeding_s=round(seeding["host_total_s"], 4), result_s=round(result["host_s"], 4))))
        return
    rec["gain"] = gain(mod, model)
    mod.close()
    if args.parent_lib:
        rec["verdict"] = verdict_rounds(args)
    if args.kernel_stats:
        with open(args.kernel_stats) as f:
            rec["verdict_kernels"] = json.load(f)
    if args.parent_record:
        with open(args.parent_record) as f:
            rec["parent_build"] = json.load(f)
    if args.headline:
        with open(args.headline) as f:
            rec["headline"] = json.load(f)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "multistart_%s.json" % rec["build"]), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(dict(build=rec["build"],
                          seeding=dict(device_s=round(seeding["device_s"], 5), host_s=round(seeding["host_total_s"], 4), ratio=round(seeding["host_over_device"], 1)),
                          result=dict(device_s=round(result["device_s"], 5), host_s=round(result["host_s"], 4), ratio=round(result["host_over_device"], 1),
                                      collision_free_s=round(result["device_collision_free_s"], 5)),
                          verdict={k: v for k, v in rec.get("verdict", {}).items() if not k.endswith("_all")},
                          gain={k: (round(v["share_with_winner"], 3), round(v["median_cost"], 3)) for k, v in rec["gain"].items()})))


if __name__ == "__main__":
    main()
