"""The fold's canonical joint frames (csrc/fold.cpp canonical_rotation) on the host: no GPU, no HIP.

tests/fk_canonical_driver.cpp is compiled with csrc/fold.cpp, env.cpp and host_math.cpp by a host compiler.  For random robots --
chains and trees, revolute, prismatic and fixed links, frozen joints between the optimized ones, axes in general position and along
+- a coordinate axis, fixed and floating bases -- it folds the robot as `create` does and walks the folded records the way fk.h does
(a turn about z, a shift along z).  The link frames (walked frame o C^T), the active spheres' centres and the frame fold_tsrs hands
the constraint are held against RobotModel.link_frames at random configurations.

The bound, from the operation count.  u = 2^-53; rows and columns of a rotation have norm 1, so a dot product of three terms is wrong
by at most 3u in a rotation's entry.  A link costs either side two such products (R Rfix, then the joint's turn), the sin and cos
(1u), and on the folded side the rounding of Rfix' = C_p^T Rfix C (1u, summed in extended precision) and of the two C (1u each):
at most 8u per link, E_R(k) <= 8 k u after k links.  A translation t <- R tfix + t is four terms of size at most L, the largest
coordinate: 4 u L, plus E_R(k) |tfix_k|.  Over a path of d links with P the sum of its offsets and p the largest sphere offset,
    E_t <= d u (4 L + 8 (P + p)) + 4 u L,
and twice that between two computations that both carry it.  d, P, p and L are those of the item's OWN path from the base: its
links, their offsets, the sphere's own offset, the largest coordinate of the path's origins and of the item at that configuration.
A few ulp of the largest coordinate is not derivable as a worst case: the rotation alone carries 8u per link either side, 100u
after six links, before any translation.  The bound comes to a few tens to a few hundred u L with the path (1.6e-15 .. 6.5e-14 for the origins here);
what is measured is a few u L, and the largest error over its bound is printed.

A missing host compiler fails the test: the check must not be skipped."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from or_cdchomp_amd import robots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "or_cdchomp_amd", "csrc")
U = 2.0 ** -53
N_ROBOTS = 24
N_CONFIGS = 4


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no host C++ compiler (g++, c++, clang++ or $CXX) to build tests/fk_canonical_driver.cpp with")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fk_canonical") / "fk_canonical_driver")
    sources = [os.path.join(ROOT, "tests", "fk_canonical_driver.cpp")] + [os.path.join(CSRC, f) for f in ("fold.cpp", "env.cpp", "host_math.cpp")]
    cmd = [_compiler(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-attributes", "-Wno-unknown-attributes", "-Wno-unknown-pragmas",
           "-I", CSRC] + sources + ["-o", exe]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    return exe


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def random_robot(seed):
    """(model, floating, active dofs, frozen dof values, base pose, constrained link): 5 .. 8 links below the base link"""
    rng = np.random.default_rng([20251021, seed])
    model = robots.RobotModel("canonical%d" % seed)
    model.add_link("l0")
    n_links = int(rng.integers(6, 10))
    tree = seed % 3 == 0
    moving = 0
    for li in range(1, n_links):
        parent = "l%d" % (int(rng.integers(0, li)) if tree and rng.uniform() < 0.4 else li - 1)
        kind = rng.uniform()
        joint = robots.JOINT_REVOLUTE if kind < 0.6 else (robots.JOINT_PRISMATIC if kind < 0.75 else robots.JOINT_FIXED)
        if li <= 2:
            joint = robots.JOINT_REVOLUTE
        if rng.uniform() < 0.5:
            axis = np.zeros(3); axis[int(rng.integers(0, 3))] = 1.0 if rng.uniform() < 0.5 else -1.0
        else:
            axis = _unit(rng.normal(size=3))
        model.add_link("l%d" % li, parent, rng.uniform(-0.3, 0.3, size=3), _unit(rng.normal(size=4)), joint=joint, axis=axis, limits=(-2.0, 2.0))
        moving += joint != robots.JOINT_FIXED
    for li in range(n_links):
        for _ in range(int(rng.integers(1, 3))):
            model.add_sphere("l%d" % li, rng.uniform(-0.2, 0.2, size=3), 0.05)
    floating = seed % 4 == 1
    n_active = max(2, int(rng.integers(2, model.n_dof + 1)))
    adofs = sorted(int(d) for d in rng.choice(model.n_dof, size=n_active, replace=False))
    dofvals = rng.uniform(-1.5, 1.5, size=model.n_dof)
    base = list(rng.uniform(-1.0, 1.0, size=3)) + list(_unit(rng.normal(size=4)))
    return model, floating, adofs, dofvals, base, int(rng.integers(1, n_links))


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, dtype=np.float64).ravel())


def run_driver(driver, tmp_path, seed):
    model, floating, adofs, dofvals, base, ee_link = random_robot(seed)
    a = model.arrays()
    rng = np.random.default_rng([7, seed])
    configs = []
    for _ in range(N_CONFIGS):
        row = list(rng.uniform(-1.0, 1.0, size=3)) + list(_unit(rng.normal(size=4))) if floating else []
        configs.append(row + list(rng.uniform(-1.9, 1.9, size=len(adofs))))
    lines = ["%d %d %d %d %d %d %d" % (a["n_links"], a["n_dof"], a["n_spheres"], int(floating), len(adofs), N_CONFIGS, ee_link)]
    for li in range(a["n_links"]):
        lines.append("%d %d %d %s %s" % (a["parent"][li], a["joint_type"][li], a["dof_index"][li], _hex(a["pose_parent_joint"][li]), _hex(a["axis"][li])))
    lines.append(" ".join("%s %s" % (float(lo).hex(), float(hi).hex()) for lo, hi in zip(a["limit_lower"], a["limit_upper"])))
    lines += [_hex(base), _hex(dofvals), " ".join(str(d) for d in adofs)]
    for s in range(a["n_spheres"]):
        lines.append("%d %s %s" % (a["sphere_link"][s], _hex(a["sphere_pos"][s]), float(a["sphere_radius"][s]).hex()))
    lines += [_hex(row) for row in configs]
    path = tmp_path / ("robot%d.txt" % seed)
    path.write_text("\n".join(lines) + "\n")
    res = subprocess.run([driver, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = dict(C=[], J=[], S=[], E=[])
    for line in res.stdout.splitlines():
        tok = line.split()
        ints = dict(C=2, J=2, S=2, E=1)[tok[0]]
        out[tok[0]].append(([int(t) for t in tok[1:1 + ints]], np.array([float.fromhex(t) for t in tok[1 + ints:]])))
    return dict(model=model, floating=floating, adofs=adofs, dofvals=dofvals, base=base, ee_link=ee_link, configs=configs, out=out)


def bound(a, t, base_t, li, item=None, p=0.0):
    """(rotation entries, positions): the docstring's bound for link li's own path, both sides.  a: model.arrays(); t: the link
    origins at this configuration; base_t: the base's; item, p: a point riding on the link and its offset in the link's frame"""
    path = []
    while li >= 0:
        path.append(li); li = int(a["parent"][li])
    d = len(path)
    P = float(np.linalg.norm(a["pose_parent_joint"][path, :3], axis=1).sum())
    L = max(float(np.abs(t[path]).max()), float(np.abs(base_t).max()), 0.0 if item is None else float(np.abs(item).max()))
    return 2.0 * 8.0 * d * U, 2.0 * (d * U * (4.0 * L + 8.0 * (P + p)) + 4.0 * U * L)


@pytest.fixture(scope="module")
def results(driver, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fk_canonical_inputs")
    return [run_driver(driver, tmp, seed) for seed in range(N_ROBOTS)]


def test_canonical_rotations(results):
    """C e_z = axis; a signed permutation of determinant +1, entry for entry, for +- a coordinate axis; orthonormal to rounding otherwise"""
    n_coord = n_general = 0
    worst = 0.0
    for res in results:
        assert res["out"]["C"], "a robot without optimized joints"
        for (_, li), v in res["out"]["C"]:
            C, axis = v[:9].reshape(3, 3), v[9:]
            assert np.array_equal(axis, res["model"].arrays()["axis"][li])
            if np.abs(axis).max() == 1.0 and np.count_nonzero(axis) == 1:
                n_coord += 1
                assert np.isin(C, (0.0, 1.0, -1.0)).all() and (np.count_nonzero(C, axis=0) == 1).all() and (np.count_nonzero(C, axis=1) == 1).all(), C
                assert np.array_equal(C[:, 2], axis) and np.linalg.det(C) == 1.0, C
            else:
                n_general += 1
                worst = max(worst, float(np.abs(C.T @ C - np.eye(3)).max()), float(np.abs(C[:, 2] - axis).max()))
                assert np.linalg.det(C) > 0.0
    print("canonical rotations: %d signed permutations, %d general (C^T C - I and C e_z - axis at most %.2e)" % (n_coord, n_general, worst))
    assert n_coord >= 20 and n_general >= 20
    assert worst <= 4.0 * U * 2.0      # three rounded products of entries below 1, the entries themselves rounded once


def test_walked_frames_and_spheres_against_link_frames(results):
    """every optimized joint's link frame, every active sphere and the constrained link's frame at N_CONFIGS configurations"""
    worst = dict(R=0.0, t=0.0, S=0.0, E=0.0)
    n_frames = n_spheres = 0
    lo_tol, hi_tol = np.inf, 0.0
    kinds = set()
    for res in results:
        model, a = res["model"], res["model"].arrays()
        frames = []
        for cfg in res["configs"]:
            q = np.array(res["dofvals"])
            q[res["adofs"]] = cfg[7:] if res["floating"] else cfg
            frames.append(model.link_frames(cfg[:7] if res["floating"] else res["base"], q))
        centres = [[R[a["sphere_link"][s]] @ a["sphere_pos"][s] + t[a["sphere_link"][s]] for s in range(a["n_spheres"])] for R, t in frames]
        base_ts = [np.asarray(cfg[:3] if res["floating"] else res["base"][:3]) for cfg in res["configs"]]
        kinds.add((res["floating"], len(res["adofs"]) < a["n_dof"]))
        for (cfg, li), v in res["out"]["J"]:
            R, t = frames[cfg]
            tol_R, tol_t = bound(a, t, base_ts[cfg], li)
            lo_tol, hi_tol = min(lo_tol, tol_t), max(hi_tol, tol_t)
            eR, et = float(np.abs(v[:9].reshape(3, 3) - R[li]).max()), float(np.abs(v[9:] - t[li]).max())
            worst["R"] = max(worst["R"], eR / tol_R); worst["t"] = max(worst["t"], et / tol_t)
            assert eR <= tol_R and et <= tol_t, (model.name, cfg, li, eR, tol_R, et, tol_t)
            n_frames += 1
        for (cfg, s), v in res["out"]["S"]:
            _, tol_t = bound(a, frames[cfg][1], base_ts[cfg], int(a["sphere_link"][s]), centres[cfg][s], float(np.linalg.norm(a["sphere_pos"][s])))
            e = float(np.abs(v - centres[cfg][s]).max())
            worst["S"] = max(worst["S"], e / tol_t)
            assert e <= tol_t, (model.name, cfg, s, e, tol_t)
            n_spheres += 1
        for (cfg,), v in res["out"]["E"]:
            R, t = frames[cfg]
            tol_R, tol_t = bound(a, t, base_ts[cfg], res["ee_link"])
            e = max(float(np.abs(v[:9].reshape(3, 3) - R[res["ee_link"]]).max()) / tol_R, float(np.abs(v[9:] - t[res["ee_link"]]).max()) / tol_t)
            worst["E"] = max(worst["E"], e)
            assert e <= 1.0, (model.name, cfg, e)
    print("%d link frames, %d sphere centres; the largest error over its bound: rotations %.3f, origins %.3f, spheres %.3f, constrained link %.3f; "
          "the origins' bounds run from %.1e to %.1e" % (n_frames, n_spheres, worst["R"], worst["t"], worst["S"], worst["E"], lo_tol, hi_tol))
    assert n_frames >= 200 and n_spheres >= 400
    assert kinds >= {(False, False), (False, True), (True, True)}      # fixed and floating bases, robots with frozen joints


def test_gpu_cases_keep_clear_of_every_switch(oracle):
    """the inputs of tests/test_gpu_fk_canonical.py, on the oracle alone: no sphere of a seed within 1e-6 of a switch of the field
    lookup or of a branch of the cost (dist = 0, dist = epsilon), and every run has spheres the obstacle term acts on"""
    import fk_canonical as fc
    for case in fc.CASES:
        ref = fc.reference(case, oracle)
        total = {key: sum(c[key] for c in ref["counts"]) for key in ref["counts"][0]}
        print("%s: %s, joint-limit rounds %s" % (case.id, total, ref["rounds"]))
        assert total["face"] == 0 and total["zero"] == 0 and total["eps"] == 0, (case.id, total)
        assert min(c["in_reach"] for c in ref["counts"]) > 0 and min(np.abs(g).max() for g in ref["G"]) > fc.G_FLOOR, (case.id, total)
        assert not any(ref["rounds"]), (case.id, ref["rounds"])      # (a joint-limit round leaves its workspace in the oracle's G and AG)
        assert 4 <= case.n_runs <= 8 and 8 <= case.n_points <= 12
