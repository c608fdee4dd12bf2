"""TEST INFRASTRUCTURE: the configurations and the one-sample trajectories of tests/test_gpu_config_clearance.py, whose premises
tests/test_host_config_clearance.py checks without a GPU.

The exact yardstick of orc_batch_config_clearance is orc_batch_clearance itself: a trajectory whose C-space length lies
between 0 and 0.04 rad has exactly one sample, on segment 0 at u = 0, whose row is a0 + (a1 - a0) * 0 = a0 -- so the
clearance of such a run is the clearance of its first row, computed by the kernel that was there before."""
import numpy as np

import clearance as CL
import common
from or_cdchomp_amd import robots

STEP = 0.01            # rad: what the rows behind the first are moved by, on one column
STEP_DOF = 4           # the dof (behind col0) that moves
WAM_VMAX = [0.5, 1.0, 2.0, 1.0, 4.0, 1.0, 0.25]
AWAY = [-2.5, 1.5, 0.0, 0.5, 0.0, 0.0, 0.0]       # the arm stretched away from the table: every active sphere outside its field


def one_sample(q, n_points=4, col0=0):
    """rows q, q + e, q + e, ...: a trajectory of C-space length STEP, one sample, at q"""
    T = np.tile(np.asarray(q, dtype=np.float64), (n_points, 1))
    T[1:, col0 + STEP_DOF] += STEP
    return T


def one_sample_batch(configs, n_points=4, col0=0):
    return np.array([one_sample(q, n_points, col0) for q in configs])


def wam_fixed():
    """the five configurations of the WAM-and-table test, by name"""
    start = np.asarray(robots.WAM_START, dtype=np.float64)
    table = np.asarray(CL.IN_TABLE, dtype=np.float64)
    folded = start.copy(); folded[3] = 3.05
    return {"start": start, "in the table": table, "near": start + 0.15 * (table - start), "folded": folded,
            "away": np.asarray(AWAY, dtype=np.float64)}


def wam_pool():
    """8 distinct configurations of the WAM inside its joint limits"""
    return np.array(list(wam_fixed().values()) + list(common.wam_goals(3, seed=606)))


def tree_pool():
    """8 distinct configurations of the 30-dof tree inside its joint limits"""
    return np.asarray(common.config5_goals(8), dtype=np.float64)


def floating_configs(base):
    """6 rows [14] of the floating-base WAM: the pose moved a little, its quaternion NOT of unit length, then the joints"""
    joints = np.array([robots.WAM_START, wam_fixed()["near"]] + list(common.wam_goals(4, seed=607)))
    rows = np.zeros((len(joints), 14))
    for k in range(len(joints)):
        pose = np.asarray(base, dtype=np.float64).copy()
        pose[:3] += [0.01 * k, -0.005 * k, 0.004 * k]
        pose[3:] += [0.01 * k, 0.0, 0.006 * k, 0.0]
        pose[3:] *= (0.7, 0.9, 1.0, 1.1, 1.3, 2.0)[k] / np.linalg.norm(pose[3:])
        rows[k, :7] = pose; rows[k, 7:] = joints[k]
    return rows


def held_configs():
    """6 configurations of the WAM with the four-sphere body in its hand: the held spheres come near the table"""
    f = wam_fixed()
    return np.array([f["start"], f["near"], f["in the table"]] + list(common.wam_goals(3, seed=608)))


def folding_configs():
    """the hand on its way to the shoulder: 4 configurations, the last two in self collision"""
    rows = np.tile(np.asarray(robots.WAM_START, dtype=np.float64), (4, 1))
    rows[:, 3] = [2.3, 2.6, 2.9, 3.05]
    return rows


def draw(length, pool_size, n_runs, seed):
    """a query list of `length` drawn from the pool with repeats by a seeded permutation: (configuration, run) of every query"""
    rng = np.random.default_rng(seed)
    return rng.permutation(length) % pool_size, rng.permutation(length) % n_runs


def lengths(chunk):
    return (1, 19, 20, 21, 79, 80, 81, chunk, chunk + 1, 3 * chunk + 7)
