"""orc_batch_respawn (successive halving on the device), measured on the WAM tabletop:
  cost   one 8 192-run block as 64 problems x 128 starts after 100 iterations: wall time and bytes over the host link of one
         batch_respawn(keep 16, sigma 0.3, "prefer") against the route a caller has without it -- batch_sync, the verdict,
         batch_gettraj of everything, the plan in numpy, batch_set_traj of everything, batch_perturb of everything (which
         moves the survivors too).  The verdict is the same kernel on both routes, so both are also timed without it
         (collision "ignore"), and the verdict alone.  Each leg of a round is a child process (--cost-child device | host);
         with --parent-lib FILE the host leg loads the parent build's library through ORC_LIB: it uses only calls the
         parent has.
  gain   config 2's 1 024 goals x K = 16 at an equal budget of 100 iterations: straight; 50 + respawn + 50; 4 x 25 with
         three respawns; keep 4, collision "require" and "prefer", sigma 0.1, 0.3 and 0.6 (of the first perturbation and of
         every respawn).  Per leg the share of problems with a collision-free winner, the median smoothness cost of the
         winners, and the problems gained and lost against the straight leg.
  verdict-subset (--verdict-subset: these legs alone, written to profiles/verdict_subset_<build>.json)
         the same block after its 100 iterations: the device-planned verdict of every run on this build and on the parent's
         library (--parent-lib), the verdict of the candidates only (batch_collision_verdict(runs="candidates")),
         batch_respawn("prefer") under batch_set_verdict_scope "all" and "candidates", and from the all-runs call n_samples by
         the runs' status (runs, maximum, sum): where the verdict's time goes.  Each leg of a round is a child process
         (--verdict-child parent | this | candidates: the candidates' legs do not follow the all-runs verdict in one process)
         that first takes the verdict of a small batch as its own warm-up.
A warm-up and REPS (default 5) alternated rounds, medians.  Writes profiles/respawn_<build>.json and prints one line.
   python scripts/bench_respawn.py [--reps N] [--parent-lib FILE] [--headline FILE] [--gain-from FILE] [--verdict-subset]
--gain-from takes the gain table of an earlier record of this script over instead of measuring it again; --headline embeds a JSON file of bench.py headline values of this build and its parent, taken next to it."""
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

KW = dict(common.CONFIG2_KW)
N_BLOCK, N_PROBLEMS, N_STARTS = 8192, 64, 128
SIGMA, KEEP = 0.3, 16


def med(xs):
    return float(np.median(xs))


def host_plan(costs, status, col, group, n_groups, keep):
    """respawn_plan's mode 2 on total costs, vectorised (the caller's numpy); equal blocks only"""
    n_runs = len(status)
    cand = ((status == 0) | (status == 1)) & np.isfinite(costs[:, 0])
    order = np.lexsort((np.arange(n_runs), costs[:, 0] + 0.0, col != 0, ~cand, group))      # by group: candidates first, free first, cost, run
    size = n_runs // n_groups
    order = order.reshape(n_groups, size)
    n_surv = np.minimum(keep, cand.reshape(n_groups, size).sum(axis=1))
    source = np.full(n_runs, -1, dtype=np.int32)
    for g in range(n_groups):
        if n_surv[g] == 0:
            continue
        surv = order[g, :n_surv[g]]
        source[surv] = surv
        rest = np.setdiff1d(order[g], surv)                       # ascending run index
        source[rest] = surv[np.arange(len(rest)) % n_surv[g]]
    return source, n_surv.astype(np.int32)


def host_route(mod, bid, group, n_groups, keep, sigma, seeds, verdict=True):
    """what a caller of the parent build does: everything to the host, the plan there, everything back"""
    t0 = time.perf_counter()
    costs, status = mod.batch_sync(bid)
    col = mod.batch_collision_verdict(bid, on_device=True)["collides"] if verdict else np.zeros(len(status), dtype=np.int32)
    traj = mod.batch_gettraj(bid)
    source, n_surv = host_plan(costs, status, col, group, n_groups, keep)
    new = traj.copy()
    clone = source >= 0
    new[clone, 1:-1] = traj[source[clone], 1:-1]
    line = np.flatnonzero(source < 0)
    if len(line):
        w = (np.arange(traj.shape[1]) / (traj.shape[1] - 1))[None, :, None]
        new[line] = traj[line, :1] + (traj[line, -1:] - traj[line, :1]) * w
    mod.batch_set_traj(bid, new)
    mod.batch_perturb(bid, sigma, seeds)
    dt = time.perf_counter() - t0
    nbytes = costs.nbytes + status.nbytes + col.nbytes + traj.nbytes + new.nbytes + seeds.nbytes
    return dt, source, n_surv, int(nbytes)


def iterated_block(mod, model):
    goals = np.repeat(common.wam_goals(N_PROBLEMS, seed=20250101), N_STARTS, axis=0)
    bid = mod.batch_create(model.name, goals, **KW)
    mod.batch_perturb(bid, SIGMA, np.arange(N_BLOCK, dtype=np.uint32) + 1)
    mod.batch_iterate(bid, 100)
    return bid


def cost_child(which):
    """one leg of a round: the block, a warm-up call on a block of its own, the timed call"""
    if os.environ.get("ORC_LIB"):
        _capi.SYMBOLS = [s for s in _capi.SYMBOLS if s[0] not in NEW_SYMBOLS]
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    group = np.repeat(np.arange(N_PROBLEMS, dtype=np.int32), N_STARTS)
    seeds = np.arange(N_BLOCK, dtype=np.uint32) + 70001
    rec = dict(lib=os.path.basename(_capi.LIB_PATH), which=which)
    for collision in ("prefer", "ignore"):                      # ("ignore": the call without the verdict, which both routes share)
        tag = "" if collision == "prefer" else "ignore_"
        for rnd in range(2):
            bid = iterated_block(mod, model)
            if collision == "prefer" and rnd:
                t0 = time.perf_counter()
                mod.batch_collision_verdict(bid, on_device=True)
                rec["verdict_s"] = time.perf_counter() - t0
            if which == "device":
                t0 = time.perf_counter()
                source, n_surv = mod.batch_respawn(bid, KEEP, SIGMA, seeds, n_groups=N_PROBLEMS, collision=collision)
                rec[tag + "s"] = time.perf_counter() - t0
                # up: the group table (n_groups + 1 + n_runs ints), the seeds, the generators and limits; with the verdict its
                # vmax, slot table and self-collision tables up and its flag down (scripts/bench_multistart.py:
                # device_link_bytes); down: the plan
                n_runs, n_points, n = mod.batch_dims(bid)
                rec[tag + "bytes"] = int(4 * (N_PROBLEMS + 1 + n_runs) + 4 * n_runs + 8 * (2 * (n_points - 2) + 2 * n)
                                         + (n * 8 + 16 * 4 + 105 * (16 + 8) + 4 if collision == "prefer" else 0) + 4 * (n_runs + N_PROBLEMS))
            else:
                rec[tag + "s"], source, n_surv, rec[tag + "bytes"] = host_route(mod, bid, group, N_PROBLEMS, KEEP, SIGMA, seeds,
                                                                                verdict=collision == "prefer")
            mod.batch_destroy(bid)
        rec.update({tag + "source_sum": int(source.astype(np.int64).sum()), tag + "survivors": int(n_surv.sum()),
                    tag + "lines": int((source < 0).sum())})
    mod.close()
    print("COST_CHILD " + json.dumps(rec))


def cost_rounds(args):
    legs = dict(device=[], host=[])
    for rnd in range(args.reps + 1):
        for which in ("host", "device"):
            env = dict(os.environ)
            env.pop("ORC_LIB", None)
            if which == "host" and args.parent_lib:
                env["ORC_LIB"] = os.path.abspath(args.parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cost-child", which], env=env, check=True,
                                 stdout=subprocess.PIPE, timeout=600).stdout.decode()
            rec = json.loads([ln for ln in out.splitlines() if ln.startswith("COST_CHILD ")][-1][len("COST_CHILD "):])
            if rnd:
                legs[which].append(rec)
    d, h = legs["device"], legs["host"]
    for tag in ("", "ignore_"):
        assert all(r[tag + "source_sum"] == d[0][tag + "source_sum"] and r[tag + "survivors"] == d[0][tag + "survivors"] for r in d + h), \
            "the routes must plan alike"
    out = dict(runs=N_BLOCK, problems=N_PROBLEMS, starts=N_STARTS, keep=KEEP, sigma=SIGMA, rounds=args.reps, host_lib=h[0]["lib"],
               survivors=d[0]["survivors"], line_runs=d[0]["lines"], verdict_alone_s=med([r["verdict_s"] for r in d]))
    for tag in ("", "ignore_"):
        out.update({tag + "device_s": med([r[tag + "s"] for r in d]), tag + "device_all": [r[tag + "s"] for r in d],
                    tag + "device_bytes": d[0][tag + "bytes"],
                    tag + "host_s": med([r[tag + "s"] for r in h]), tag + "host_all": [r[tag + "s"] for r in h],
                    tag + "host_bytes": h[0][tag + "bytes"],
                    tag + "host_over_device": med([r[tag + "s"] for r in h]) / med([r[tag + "s"] for r in d])})
    return out


NEW_SYMBOLS = ("orc_batch_respawn", "orc_batch_collision_verdict_subset", "orc_batch_set_verdict_scope")      # what a parent's library may lack


def verdict_child(which):
    """One leg of a verdict-subset round, a process of its own so that no leg finds the block's pages or the allocator warm
    from another: `parent` (the library of ORC_LIB) and `this` take the all-runs verdict, then (`this`) one respawn under scope
    "all" on a fresh block; `candidates` takes the candidates' verdict with the count (n_samples returned), then without it (count=False: that
    second call follows the first on the same block), then one respawn under scope "candidates" on a fresh block."""
    if os.environ.get("ORC_LIB"):
        _capi.SYMBOLS = [s for s in _capi.SYMBOLS if s[0] not in NEW_SYMBOLS[1:]]
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    seeds = np.arange(N_BLOCK, dtype=np.uint32) + 70001
    rec = dict(lib=os.path.basename(_capi.LIB_PATH), which=which)
    small = mod.batch_create(model.name, common.wam_goals(8, seed=3), **KW)      # (the kernel's first launch of the process)
    mod.batch_collision_verdict(small, on_device=True)
    mod.batch_destroy(small)
    bid = iterated_block(mod, model)
    costs, status = mod.batch_sync(bid)
    rec["status_counts"] = {str(st): int((status == st).sum()) for st in sorted(set(status.tolist()))}
    if which in ("parent", "this"):
        t0 = time.perf_counter()
        full = mod.batch_collision_verdict(bid, on_device=True)
        rec["all_s"] = time.perf_counter() - t0
        ns = full["n_samples"].astype(np.int64)
        rec["by_status"] = {str(st): dict(runs=int((status == st).sum()), max=int(ns[status == st].max()), sum=int(ns[status == st].sum()),
                                          median=float(np.median(ns[status == st])), colliding=int(full["collides"][status == st].sum()))
                            for st in sorted(set(status.tolist()))}
        rec["colliding"] = int(full["collides"].sum())
        rec["collides_sum_of_run_index"] = int(np.flatnonzero(full["collides"]).sum())
        scope = "all"
        if which == "this":      # (the respawn of either scope on a block of its own)
            mod.batch_destroy(bid)
            bid = iterated_block(mod, model)
    else:
        from or_cdchomp_amd.module import candidates
        cand = candidates(costs, status)
        t0 = time.perf_counter()
        part = mod.batch_collision_verdict(bid, on_device=True, runs="candidates")
        rec["candidates_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        plain = mod.batch_collision_verdict(bid, on_device=True, runs="candidates", count=False)
        rec["candidates_nocount_s"] = time.perf_counter() - t0
        assert np.array_equal(part["collides"] == -1, ~cand) and np.array_equal(plain["collides"], part["collides"])
        rec["candidates"] = int(cand.sum())
        rec["colliding_candidates"] = int((part["collides"] == 1).sum())
        rec["collides_sum_of_run_index"] = int(np.flatnonzero(part["collides"] == 1).sum())
        mod.batch_destroy(bid)
        bid = iterated_block(mod, model)
        scope = "candidates"
    if which != "parent":
        mod.batch_set_verdict_scope(bid, scope)
        t0 = time.perf_counter()
        source, n_surv = mod.batch_respawn(bid, KEEP, SIGMA, seeds, n_groups=N_PROBLEMS, collision="prefer")
        rec["respawn_s"] = time.perf_counter() - t0
        rec["source_sum"] = int(source.astype(np.int64).sum()); rec["survivors"] = int(n_surv.sum())
    mod.batch_destroy(bid)
    mod.close()
    print("VERDICT_CHILD " + json.dumps(rec))


def verdict_rounds(args):
    legs = dict(this=[], parent=[], candidates=[])
    for rnd in range(args.reps + 1):
        for which in ("parent", "this", "candidates"):
            if which == "parent" and not args.parent_lib:
                continue
            env = dict(os.environ)
            env.pop("ORC_LIB", None)
            if which == "parent":
                env["ORC_LIB"] = os.path.abspath(args.parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--verdict-child", which], env=env, check=True,
                                 stdout=subprocess.PIPE, timeout=600).stdout.decode()
            rec = json.loads([ln for ln in out.splitlines() if ln.startswith("VERDICT_CHILD ")][-1][len("VERDICT_CHILD "):])
            print("round %d %s: %s" % (rnd, which, {k: round(v, 4) for k, v in rec.items() if k.endswith("_s")}), file=sys.stderr, flush=True)
            if rnd:
                legs[which].append(rec)
    t, p, c = legs["this"], legs["parent"], legs["candidates"]
    assert all(r["status_counts"] == t[0]["status_counts"] for r in t + p + c), "every leg must see the same block"
    assert all(r["by_status"] == t[0]["by_status"] and r["colliding"] == t[0]["colliding"] for r in t + p), "every all-runs leg must give the same verdict"
    assert all(r["source_sum"] == t[0]["source_sum"] and r["survivors"] == t[0]["survivors"] for r in t + c), "the scope must not change the plan"
    out = dict(runs=N_BLOCK, problems=N_PROBLEMS, starts=N_STARTS, keep=KEEP, sigma=SIGMA, rounds=args.reps,
               candidates=c[0]["candidates"], colliding_candidates=c[0]["colliding_candidates"], survivors=t[0]["survivors"],
               colliding=t[0]["colliding"], n_samples_by_status=t[0]["by_status"])

    def leg(name, recs, key):
        out[name + "_s"] = med([r[key] for r in recs]); out[name + "_rounds"] = [r[key] for r in recs]
    leg("all", t, "all_s"); leg("respawn_all", t, "respawn_s")
    leg("candidates", c, "candidates_s"); leg("candidates_nocount", c, "candidates_nocount_s"); leg("respawn_candidates", c, "respawn_s")
    if p:
        out["parent_lib"] = p[0]["lib"]
        leg("parent_all", p, "all_s")
    out["candidates_over_all"] = out["candidates_s"] / out["all_s"]
    out["respawn_candidates_over_all"] = out["respawn_candidates_s"] / out["respawn_all_s"]
    return out


def gain(mod, model, K=16, keep=4, sigmas=(0.1, 0.3, 0.6)):
    goals = np.repeat(common.wam_goals(1024, seed=20250101), K, axis=0)
    P, n_runs = 1024, 1024 * K
    out = {}

    def leg(sigma, schedule, collision):
        bid = mod.batch_create(model.name, goals, **KW)
        mod.batch_perturb(bid, sigma, np.arange(n_runs, dtype=np.uint32) + 1)
        survivors, lines = [], []
        for k, n_iter in enumerate(schedule):
            if k:
                src, cnt = mod.batch_respawn(bid, keep, sigma, np.arange(n_runs, dtype=np.uint32) + 1 + 100003 * k, n_groups=P,
                                             collision=collision, by="smooth")
                survivors.append(int(cnt.sum())); lines.append(int((src < 0).sum()))
            costs, status = mod.batch_iterate(bid, n_iter)
        best, _, cnt = mod.batch_select_best(bid, n_groups=P, collision_free=True, by="smooth")
        mod.batch_destroy(bid)
        has = best >= 0
        return dict(has=has, smooth=np.where(has, costs[np.maximum(best, 0), 2], np.nan), aborted=float((status == -1).mean()),
                    eligible=float(cnt.sum() / n_runs), survivors=survivors, lines=lines)

    for sg in sigmas:
        straight = leg(sg, (100,), None)
        rows = {"straight": straight}
        for collision in ("require", "prefer"):
            rows["50+50 " + collision] = leg(sg, (50, 50), collision)
            rows["4x25 " + collision] = leg(sg, (25, 25, 25, 25), collision)
        for name, r in rows.items():
            both = r["has"] & straight["has"]
            out["sigma%g %s" % (sg, name)] = dict(
                share_with_winner=float(r["has"].mean()), median_smooth=med(r["smooth"][r["has"]]),
                gained=int((r["has"] & ~straight["has"]).sum()), lost=int((~r["has"] & straight["has"]).sum()),
                median_smooth_ratio_to_straight=med(r["smooth"][both] / straight["smooth"][both]),
                aborted_share=r["aborted"], eligible_share_of_runs=r["eligible"], survivors=r["survivors"], line_runs=r["lines"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default="", help="the parent build's library for the host route")
    ap.add_argument("--headline", default="")
    ap.add_argument("--cost-child", default="")
    ap.add_argument("--gain-from", default="", help="a record of this script whose gain table is taken over instead of measured again")
    ap.add_argument("--verdict-child", default="")
    ap.add_argument("--verdict-subset", action="store_true", help="the verdict-subset legs alone, to profiles/verdict_subset_<build>.json")
    args = ap.parse_args()
    if args.cost_child:
        return cost_child(args.cost_child)
    if args.verdict_child:
        return verdict_child(args.verdict_child)
    if args.verdict_subset:
        rec = dict(build=_capi.csrc_hash(), reps=args.reps, verdict_subset=verdict_rounds(args))
        if args.headline:
            with open(args.headline) as f:
                rec["headline"] = json.load(f)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "verdict_subset_%s.json" % rec["build"]), "w") as f:
            json.dump(rec, f, indent=1)
        v = rec["verdict_subset"]
        print(json.dumps(dict(build=rec["build"], verdict_subset={k: (round(x, 5) if isinstance(x, float) else x) for k, x in v.items()
                                                                  if not k.endswith("_rounds")})))
        return
    rec = dict(build=_capi.csrc_hash(), reps=args.reps, cost=cost_rounds(args))
    if args.gain_from:
        with open(args.gain_from) as f:
            rec["gain"] = json.load(f)["gain"]
    else:
        mod = or_cdchomp_amd.Module(0)
        model = common.setup_product_wam(mod)
        rec["gain"] = gain(mod, model)
        mod.close()
    if args.headline:
        with open(args.headline) as f:
            rec["headline"] = json.load(f)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "respawn_%s.json" % rec["build"]), "w") as f:
        json.dump(rec, f, indent=1)
    c = rec["cost"]
    print(json.dumps(dict(build=rec["build"],
                          cost=dict(device_s=round(c["device_s"], 5), host_s=round(c["host_s"], 4), ratio=round(c["host_over_device"], 2),
                                    verdict_alone_s=round(c["verdict_alone_s"], 4), no_verdict_device_s=round(c["ignore_device_s"], 5),
                                    no_verdict_host_s=round(c["ignore_host_s"], 4), no_verdict_ratio=round(c["ignore_host_over_device"], 1),
                                    device_bytes=c["device_bytes"], host_bytes=c["host_bytes"]),
                          gain={k: (round(v["share_with_winner"], 3), round(v["median_smooth"], 3), v["gained"], v["lost"])
                                for k, v in rec["gain"].items()})))


if __name__ == "__main__":
    main()
