#!/usr/bin/env python3
"""What the phase calls of one iterate-kernel instantiation cost, from a device assembly listing (scripts/asm_fast.sh):
per function the static counts of vector instructions, of the lane moves among them (v_writelane_b32 / v_readlane_b32: scalar
registers saved in VGPR lanes around a call, this target has no scalar spill to memory), of scratch stores and loads, and the
calls a wavefront makes per iteration; then their sum per wavefront and iteration.

    scripts/asm_fast.sh /tmp/k.s && python scripts/call_overhead.py /tmp/k.s [--real double] [--tree] [--wide] [--block 256]
                                                                    [--kind 11] [--wgs 4] [--tiles 2] [--lean 1]

--tree / --wide: a tree instead of a chain / the many-sphere pass instead of the 16-lane one (GS16); --tiles: cost tiles per
iteration (an FK and a cost call each); --lean: the update mode the workload takes (0 general, 1 lean, 2 lean with TSR).

The counts are static: a function's instructions in the listing, whichever branch they are on.  They compare two builds of the
same source shape; they are not what a wavefront executes (NOTES/call-overhead.md sets them beside the measured counter).
The kernel function's share is what lies between its call of phase_setup and its call of phase_finish, in the order of the
listing: the loop that sequences the phase calls.  It is added to the sum once."""
import argparse
import re
import subprocess


def parse(path):
    """functions of the listing in order: name -> list of instruction lines (label lines and directives dropped)"""
    funcs, order, name = {}, [], None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            funcs[name] = []
            order.append(name)
            continue
        if name is None:
            continue
        s = line.strip()
        if not s or s.startswith((".", ";")) or s.endswith(":"):
            continue
        funcs[name].append(s)
    return funcs, order


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        return dict(zip(names, out))
    except OSError:
        return {n: n for n in names}


def count(lines):
    c = dict(valu=0, lane=0, st=0, ld=0)
    for s in lines:
        op = s.split()[0]
        if op.startswith("v_"):
            c["valu"] += 1
            if op.startswith(("v_readlane", "v_writelane")):
                c["lane"] += 1
        elif op.startswith("scratch_store"):
            c["st"] += 1
        elif op.startswith("scratch_load"):
            c["ld"] += 1
    return c


def loop_part(lines, dem):
    """the kernel function's lines between its call of phase_setup and its call of phase_finish (the address of a callee is
    formed from its label a few lines before the call)"""
    first = last = None
    for i, s in enumerate(lines):
        m = re.search(r"(_Z\w+)@rel32@lo", s)
        if not m:
            continue
        callee = dem.get(m.group(1), m.group(1))
        if "phase_setup<" in callee and first is None:
            first = i
        if "phase_finish<" in callee:
            last = i
    if first is None or last is None or last <= first:
        return lines
    return lines[first:last]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("--real", default="double")
    ap.add_argument("--tree", action="store_true")
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--kind", type=int, default=11)
    ap.add_argument("--wgs", type=int, default=4)
    ap.add_argument("--tiles", type=int, default=2)
    ap.add_argument("--lean", type=int, default=1)
    a = ap.parse_args()

    funcs, order = parse(a.listing)
    dem = demangle(order)
    tree, gs16 = ("true" if a.tree else "false"), ("false" if a.wide else "true")
    head = "%s, %s, %s, %d" % (a.real, tree, gs16, a.block)
    # (name in the listing, calls per wavefront and iteration; None: the kernel function)
    want = [
        ("phase_fk<%s, %d>" % (head, a.wgs), a.tiles),
        ("phase_cost<%s, %d, true, %d>" % (head, a.kind, a.wgs), a.tiles),
        ("phase_update_costs<%s, %d, %d>" % (head, a.wgs, a.lean), 1),
        ("phase_update<%s, %d, %d>" % (head, a.wgs, a.lean), 1),
        ("phase_costs<%s, %s, %d, %d>" % (a.real, gs16, a.block, a.wgs), 1),
        ("chomp_iterate_kernel<%s, %d, %d>" % (head, a.kind, a.wgs), None),
    ]
    by_name = {}
    for k in order:
        d = dem.get(k, k).replace("(anonymous namespace)::", "")
        d = re.sub(r"^\S+ (?=\w+<)", "", d)      # the return type of a function template
        by_name[d.split("(")[0]] = k
    # a build that makes update and costs in one call has the two-call functions beside it (other modes, the cost-only pass):
    # they are listed, but a wavefront of this workload does not call them in an iteration
    fused = want[2][0] in by_name
    print("%-66s %6s %10s %8s %8s %6s" % ("function", "VALU", "lane moves", "scr. st", "scr. ld", "calls"))
    total = dict(valu=0, lane=0, st=0, ld=0)
    for name, calls in want:
        if name not in by_name:
            continue
        lines = funcs[by_name[name]]
        c = count(lines)
        if calls is None:
            print("%-66s %6d %10d %8d %8d %6s" % (name, c["valu"], c["lane"], c["st"], c["ld"], "-"))
            c = count(loop_part(lines, dem))
            print("%-66s %6d %10d %8d %8d %6s" % ("   of it between phase_setup and phase_finish", c["valu"], c["lane"], c["st"], c["ld"], 1))
            calls = 1
        else:
            if fused and name.startswith(("phase_update<", "phase_costs<")):
                calls = 0
            print("%-66s %6d %10d %8d %8d %6d" % (name, c["valu"], c["lane"], c["st"], c["ld"], calls))
        for k in total:
            total[k] += calls * c[k]
    print("%-66s %6d %10d %8d %8d" % ("sum per wavefront and iteration (static)", total["valu"], total["lane"], total["st"], total["ld"]))


if __name__ == "__main__":
    main()
