"""The table of iterate-kernel instantiations (csrc/kernel_table.h) against the planner, on the host: no GPU, no HIP.

tests/kernel_table_driver.cpp is compiled with csrc/plan.cpp by a host compiler and walks a grid of planner inputs -- every variant
mask the fold can emit, both precisions, the shapes and budgets a caller can ask for, constrained and free-start runs, 1 .. 4000
moving waypoints, the planner's switches.  Every plan must name a row of the table, and the row's register budget must hold the
resident workgroups per CU the plan sized its share of the LDS for (IteratePlan::per_cu).

(Why per_cu and not IteratePlan::workgroups_per_cu(): the latter is what the plan's LDS bytes alone would admit, 160 KB / bytes.  A
short trajectory needs a few KB, so it "admits" twenty workgroups where the registers hold three; that is no planner fault and
holds for more than half of the grid's plans, the driver counts them as lds_above_registers.  A plan is wrong when it was SIZED for
more residents than its kernel's registers hold, and that is what is asserted.)

A missing host compiler fails the test: the check must not be skipped."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "or_cdchomp_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler (g++, c++, clang++ or $CXX) to build tests/kernel_table_driver.cpp with")


def _build(tmp_path, sources, name):
    exe = str(tmp_path / name)
    cmd = [_compiler(), "-std=c++17", "-O2", "-Wall", "-Wno-attributes", "-Wno-unknown-attributes", "-I", CSRC] + sources + ["-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    return exe


def test_the_table_is_host_code_with_93_distinct_rows(tmp_path):
    src = tmp_path / "rows.cpp"
    src.write_text('''#include "kernel_table.h"
using namespace orc;
constexpr bool distinct()
{
   for (int i=0; i<N_ITERATE_KERNELS; i++) for (int j=0; j<i; j++) if (ITERATE_KERNELS[i] == ITERATE_KERNELS[j]) return false;
   return true;
}
static_assert(N_ITERATE_KERNELS == 93, "rows of the table");
static_assert(distinct(), "a row twice");
int main() { return 0; }
''')
    _build(tmp_path, [str(src)], "rows")


def test_every_plan_names_a_kernel_whose_registers_hold_it(tmp_path):
    exe = _build(tmp_path, [os.path.join(ROOT, "tests", "kernel_table_driver.cpp"), os.path.join(CSRC, "plan.cpp")], "kernel_table_driver")
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(res.stdout)
    summary = dict(zip(*[iter(res.stdout.strip().splitlines()[-1].split())] * 2))
    assert res.returncode == 0, res.stdout[-4000:]
    assert int(summary["failures"]) == 0 and int(summary["empty"]) == 0
    assert int(summary["plans"]) > 100000 and int(summary["rows"]) == 93
