"""csrc/wave_roles.h on the host: no GPU, no HIP.

tests/wave_roles_driver.cpp is compiled by a host compiler and checks, for workgroups of 128, 192, 256 and 512 threads:
the logical thread index is a permutation of 0 .. BLOCK-1 for every rotation, maps wavefronts onto wavefronts and keeps the
lane (tid & 63); the rotation ORC_WAVE_ROTATE derives from the workgroup index and the iteration stays below the workgroup's
wavefronts; and the FK phase's hand-out of waypoint groups to the last wavefronts walks every waypoint of a tile exactly once
(once per segment for a split joint tree) for 1 .. 4 * 20 * BLOCK/64 waypoints.

A missing host compiler fails the test: the check must not be skipped."""
import os
import subprocess

from test_kernel_table import ROOT, _build


def test_logical_index_and_fk_roles(tmp_path):
    exe = _build(tmp_path, [os.path.join(ROOT, "tests", "wave_roles_driver.cpp")], "wave_roles_driver")
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-4000:]
    summary = dict(zip(*[iter(res.stdout.strip().splitlines()[-1].split())] * 2))
    assert int(summary["failures"]) == 0
    # 128 + 192 + 256 + 512 threads times their 2, 3, 4 and 8 rotations; 160 + 240 + 320 + 640 tile sizes, twice where pairs walk
    assert int(summary["mappings"]) == 128 * 2 + 192 * 3 + 256 * 4 + 512 * 8
    assert int(summary["walks"]) == 2 * 160 + 240 + 2 * 320 + 2 * 640

