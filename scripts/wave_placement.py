"""Where the wavefronts of config 2's workgroups sit: python scripts/wave_placement.py [n_runs [n_iter]]

Runs one batch of the headline workload (the WAM, 100 waypoints, fp64, the plan of overlapping launches: 256 threads, four
workgroups per CU) with ORC_PHASE_TIMERS=1 and reads the "waves" state: the hardware-ID register of every wavefront of every
run's workgroup at kernel start.  Three tables:
  1. which SIMD hardware wavefront k of a workgroup lands on;
  2. whether the four wavefronts of a workgroup sit on four distinct SIMDs;
  3. which workgroup indices share a CU, and what ORC_WAVE_ROTATE=1 (rotation from bits 8.. of the workgroup index) makes of it:
     on how many SIMDs of a CU the residents' logical wavefront 0 -- the one with the partial cost round, the update phase's
     single-wavefront work and the joint-limit rounds -- then sits.
What the numbers decided is in NOTES/wave-roles.md."""
import os
import sys
from collections import Counter, defaultdict

os.environ["ORC_PHASE_TIMERS"] = "1"
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
import numpy as np

import common
import or_cdchomp_amd
from or_cdchomp_amd import _capi

n_runs = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
n_iter = int(sys.argv[2]) if len(sys.argv) > 2 else 20
mod = or_cdchomp_amd.Module(0)
model = common.setup_product_wam(mod)
mod.set_num_streams(2)
bid = mod.batch_create(model.name, common.wam_goals(n_runs), **common.CONFIG2_KW)
plan = mod.batch_plan(bid)
mod.batch_iterate(bid, n_iter)
raw = np.zeros((n_runs, 8, 2))
mod._check(mod._lib.orc_batch_get_state(mod._h, bid, b"waves", raw.ctypes.data_as(_capi.c_double_p), raw.size))
mod.batch_destroy(bid)
waves = plan["threads"] // 64
hw = raw[:, :waves, 0].astype(np.int64)
xcc = raw[:, :waves, 1].astype(np.int64) & 15
assert (raw[:, waves:, 0] == 0xFFFFFFFF).all() and (hw != 0xFFFFFFFF).all(), "a wavefront without a record"
slot, simd, cu, sa, se = hw & 15, (hw >> 4) & 3, (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7
print("plan: %s" % plan)
print("%d workgroups of %d wavefronts, one launch of %d iterations" % (n_runs, waves, n_iter))

print("\n1. SIMD of hardware wavefront k (workgroups)")
print("   wave  " + "".join("  SIMD %d" % s for s in range(4)))
for k in range(waves):
    print("   %4d  " % k + "".join("%8d" % int((simd[:, k] == s).sum()) for s in range(4)))
start = Counter(int(s) for s in simd[:, 0])
stride = Counter(tuple(int(v) for v in (simd[r] - simd[r, 0]) % 4) for r in range(n_runs))
print("   SIMD of wavefront 0: %s" % dict(sorted(start.items())))
print("   SIMDs of wavefronts 0.. relative to wavefront 0's: %s" % dict(stride))

print("\n2. distinct SIMDs among a workgroup's wavefronts")
distinct = Counter(len(set(int(s) for s in simd[r])) for r in range(n_runs))
for d in sorted(distinct):
    print("   %d distinct: %5d workgroups" % (d, distinct[d]))
same_cu = sum(1 for r in range(n_runs) if len(set(zip(xcc[r], se[r], sa[r], cu[r]))) == 1)
print("   all wavefronts on one CU: %d of %d workgroups" % (same_cu, n_runs))

print("\n3. workgroups that share a CU (CU = XCC, shader engine, shader array, CU id of wavefront 0)")
by_cu = defaultdict(list)
for r in range(n_runs):
    by_cu[(int(xcc[r, 0]), int(se[r, 0]), int(sa[r, 0]), int(cu[r, 0]))].append(r)
print("   CUs in use: %d; workgroups per CU: %s" % (len(by_cu), dict(sorted(Counter(len(v) for v in by_cu.values()).items()))))
diffs = Counter()
for v in by_cu.values():
    for a in v:
        for b in v:
            if a < b:
                diffs[b - a] += 1
print("   index distance of co-resident pairs (most common): %s" % diffs.most_common(8))
bits = Counter(len(set((r >> 8) & 3 for r in v)) for v in by_cu.values())
print("   distinct values of (index >> 8) & 3 among a CU's residents: %s (CUs)" % dict(sorted(bits.items())))
for key in sorted(by_cu)[:6]:
    print("   xcc %d se %d sa %d cu %2d: workgroups %s, SIMD of their wavefront 0: %s" % (key + (by_cu[key], [int(simd[r, 0]) for r in by_cu[key]])))
for mode in (0, 1):
    spread = Counter()
    for v in by_cu.values():
        # logical wavefront 0 is hardware wavefront (0 - rot) mod waves
        where = [int(simd[r, (-(((r >> 8) & 7) % waves if mode else 0)) % waves]) for r in v]
        spread[len(set(where))] += 1
    print("   ORC_WAVE_ROTATE=%d: SIMDs of a CU that carry a resident's logical wavefront 0: %s (CUs)" % (mode, dict(sorted(spread.items()))))
