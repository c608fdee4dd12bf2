"""-m gpu: the collision verdict that plans its own samples (orc_batch_collision_verdict_device,
Module.batch_collision_verdict(on_device=True), orc_batch_select_best with require_collision_free) against the host-planned
orc_batch_collision_verdict, which stays the yardstick: the same first contact bit for bit, the sample count of the
specification (or_cdchomp_amd.module.verdict_samples), on every kind of batch the host-planned verdict covers."""
import numpy as np
import pytest

import clearance as CL
import common
import or_cdchomp_amd
from or_cdchomp_amd import _capi, robots, scenes
from or_cdchomp_amd.module import contiguous_groups, select_best, verdict_samples

pytestmark = pytest.mark.gpu

KW = dict(common.CONFIG2_KW)                     # n_points 100, lambda 100, obs_factor 500
IN_TABLE = [1.2, -0.2, 0.0, 0.3, 0.0, 0.0, 0.0]    # the forearm in the table top (tests/test_gpu_multistart.py)
WAM_VMAX = [0.5, 1.0, 2.0, 1.0, 4.0, 1.0, 0.25]
CHUNK = 64                                       # samples the kernel walks at a time, at most (fewer for a robot whose rows fill the LDS)


def same(a, b):
    """bit-identical arrays"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def first_contact_sample(traj, vmax, col0, time):
    """index of the sample whose time is `time` in the plan of `traj`"""
    times = verdict_samples(traj, vmax, col0)[2]
    k = int(np.searchsorted(times, time))
    assert k < len(times) and times[k] == time, "a contact's time is a sample's time"
    return k, len(times)


def late_contact(line, frac_contact, col0, n_points):
    """a trajectory over the configurations of the straight line `line` whose first contact lies beyond the first chunk of
    samples: back and forth over the part of the line in front of the contact until more than CHUNK samples (0.04 rad
    each) have passed, then the line itself"""
    a, b = line[0], line[-1]
    length = float(np.linalg.norm((b - a)[col0:]))
    f = 0.7 * frac_contact
    assert f * length > 0.05, "the line must have a free part to walk"
    k = int(np.ceil(CHUNK * 0.04 / (2 * f * length))) + 1
    knots = np.array([0.0] + [f, 0.0] * k + [1.0])
    assert len(knots) <= n_points
    arc = np.concatenate([[0.0], np.cumsum(np.abs(np.diff(knots)))])
    s = np.interp(np.linspace(0.0, arc[-1], n_points), arc, knots)
    assert s.max() <= 1.0 and s[0] == 0.0 and abs(s[-1] - 1.0) < 1e-12
    return a[None, :] + s[:, None] * (b - a)[None, :]


def compare(mod, bid, vmax, col0):
    """both verdicts of a batch; the device-planned one must be the host-planned one"""
    host = mod.batch_collision_verdict(bid)
    dev = mod.batch_collision_verdict(bid, on_device=True)
    traj = mod.batch_gettraj(bid)
    for key in ("collides", "sphere", "field"):
        assert np.array_equal(dev[key], host[key]), (key, np.flatnonzero(dev[key] != host[key]), dev[key], host[key])
        assert dev[key].dtype == np.int32
    assert same(dev["time"], host["time"]), np.flatnonzero(dev["time"] != host["time"])
    assert same(dev["depth"], host["depth"]), np.flatnonzero(dev["depth"] != host["depth"])
    want = np.array([len(verdict_samples(traj[k], vmax, col0)[0]) for k in range(len(traj))], dtype=np.int32)
    assert dev["n_samples"].dtype == np.int32
    assert np.array_equal(dev["n_samples"], want), (np.flatnonzero(dev["n_samples"] != want), dev["n_samples"], want)
    return host, dev, traj


def check_workload(mod, bid, vmax, col0, n_iter, pick=None):
    """The batch's seeds are straight lines: one that collides is turned into a trajectory whose contact comes late and put
    in that run's place after n_iter iterations; then both verdicts.  Asserts that the workload decides something."""
    n_points = mod.batch_dims(bid)[1]
    seeds = mod.batch_gettraj(bid)
    v0 = mod.batch_collision_verdict(bid)
    hits = [k for k in np.flatnonzero(v0["collides"]) if v0["time"][k] > 0.0] if pick is None else [pick]
    assert hits, "a seed must collide"
    fracs = []
    for k in hits:
        idx, cnt = first_contact_sample(seeds[k], vmax, col0, v0["time"][k])
        fracs.append(idx / cnt)
    r = hits[int(np.argmax(fracs))]
    if n_iter:
        mod.batch_iterate(bid, n_iter)
    traj = mod.batch_gettraj(bid)
    traj[r] = late_contact(seeds[r], max(fracs), col0, n_points)
    mod.batch_set_traj(bid, traj)
    host, dev, traj = compare(mod, bid, vmax, col0)
    assert host["collides"].any() and not host["collides"].all(), "both outcomes must occur"
    assert host["collides"][r] == 1, "the late trajectory ends in the obstacle"
    idx, cnt = first_contact_sample(traj[r], vmax, col0, dev["time"][r])
    print("late contact at sample %d of %d; %d of %d runs collide" % (idx, cnt, host["collides"].sum(), len(traj)))
    assert idx >= CHUNK, "a first contact must lie beyond the first chunk of samples"
    return host, dev, traj


def wam_goals_with_table(n_runs, seed, k_table=4):
    goals = common.wam_goals(n_runs, seed=seed)
    goals[-k_table:] = IN_TABLE
    return goals


def set_wam_vmax(mod, model):
    vmax = np.ones(model.n_dof); vmax[:7] = WAM_VMAX
    mod.set_velocity_limits(model.name, vmax)
    return vmax[:7]


# ---- 1. device equals host, exactly ----------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [64, 32])
def test_config2_after_100_iterations(precision):
    """config 2's goals and the goal in the table after 100 iterations; precision 32: the plan is made in double on the
    widened trajectory, as the host's"""
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    vmax = set_wam_vmax(mod, model)
    goals = wam_goals_with_table(72, seed=20250101)
    bid = mod.batch_create(model.name, goals, **dict(KW, precision=precision))
    host, dev, traj = check_workload(mod, bid, vmax, 0, 100, pick=len(goals) - 1)
    if precision == 32:
        assert same(traj, traj.astype(np.float32)), "a precision 32 batch holds floats"
    assert host["collides"][-4:].all(), "every run that ends in the table collides"
    assert (host["field"][host["collides"] == 1] >= 0).any()
    mod.batch_destroy(bid)
    mod.close()


def test_floating_base():
    """columns 0..6 are the base pose: the plan reads the columns from 7 on, the interpolated rows are renormalised.
    With a floating base every sphere is active, the one on the WAM's pedestal too, and where config 2 puts the robot that
    sphere stands 4 cm inside the table's field: every run would collide at its first sample.  The robot stands 20 cm
    further from the table here, where the start pose is 8 cm clear of the field (cell values of the field at the sphere
    centres) and the line to the goal in the table enters it after a third of the way."""
    mod = or_cdchomp_amd.Module(0)
    model, base, dofvals, adofs = common.wam_state()
    base = np.asarray(base, dtype=np.float64)
    base[0] -= 0.2
    mod.add_robot(model, transform=list(base), dof_values=dofvals, active_dofs=adofs)
    scenes.add_tabletop(mod)
    mod.SendCommand("computedistancefield kinbody table")
    vmax = set_wam_vmax(mod, model)
    n_runs = 24
    goals = wam_goals_with_table(n_runs, seed=77)
    # four runs that only turn the wrist and stay where the start pose is: free of everything
    start = np.asarray(dofvals[:7], dtype=np.float64)
    goals[1:5] = start + np.array([[0, 0, 0, 0, 1.0, 0, 1.0], [0, 0, 0, 0, -1.0, 0.3, -1.0], [0, 0, 0.2, 0, 0.5, -0.3, 0.8], [0, -0.1, 0, 0.1, 1.0, 0, 0]])
    basegoals = np.tile(base, (n_runs, 1))
    basegoals[:, :3] += [0.04, -0.03, 0.02]                 # the base moves and turns a little on the way
    basegoals[:, 3:] += [0.05, 0.0, 0.03, 0.0]
    basegoals[:, 3:] /= np.linalg.norm(basegoals[:, 3:], axis=1)[:, None]
    bid = mod.batch_create(model.name, goals, basegoals=basegoals, **dict(KW, n_points=40, floating_base=1))
    assert mod.batch_dims(bid)[2] == 14
    host, dev, traj = check_workload(mod, bid, vmax, 7, 10)
    assert np.abs(traj[:, -1, :7] - traj[:, 0, :7]).max() > 0.03, "the base must move"
    mod.batch_destroy(bid)
    mod.close()


def test_tree_robot():
    """the 30-dof tree among config 5's bodies: saved frames in the FK walk, more spheres than a DPP row.  Without box2,
    which the robot's start pose touches (every run would collide at its first sample): against the other three the
    straight lines to config 5's goals give free runs, contacts with a field on the way and a pair of the robot's own spheres."""
    mod = or_cdchomp_amd.Module(0)
    model = robots.tree30()
    mod.add_robot(model, transform=[0.0] * 6 + [1.0], dof_values=np.zeros(model.n_dof), active_dofs=list(range(model.n_dof)))
    for name, (boxes, pose) in common.config5_bodies().items():
        if name != "box2":
            mod.add_kinbody_boxes(name, boxes, transform=pose)
            mod.SendCommand("computedistancefield kinbody %s cube_extent %f aabb_padding %f" % (name, common.CONFIG5_CUBE, common.CONFIG5_PADDING))
    vmax = np.linspace(0.5, 2.0, model.n_dof)
    mod.set_velocity_limits(model.name, vmax)
    goals = common.config5_goals(48)
    bid = mod.batch_create(model.name, goals, **dict(common.CONFIG5_KW, n_points=60))
    assert mod.batch_plan(bid)["variant"] & 1, "the robot must be a tree"
    host, dev, traj = check_workload(mod, bid, vmax, 0, 5)
    print("first contacts by field:", sorted(set(host["field"][host["collides"] == 1].tolist())))
    mod.batch_destroy(bid)
    mod.close()


def test_scene_batch():
    """per-run scenes: every run against its own fields; an empty scene has no contact with anything but the robot"""
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    mod.SendCommand("computedistancefield kinbody mug")
    vmax = set_wam_vmax(mod, model)
    shift = np.array([0.03, -0.04, 0.02, 0.0, 0.0, 0.0, 1.0])
    scenes = [[("table", None), ("mug", None)], [("table", shift), ("mug", shift)], [("mug", None), ("table", None)], []]
    n_runs = 32
    goals = wam_goals_with_table(n_runs, seed=78, k_table=8)
    scene_of_run = (np.arange(n_runs) % len(scenes)).astype(np.int32)
    bid = mod.batch_create(model.name, goals, scenes=scenes, scene_of_run=scene_of_run, **dict(KW, n_points=40))
    host, dev, traj = check_workload(mod, bid, vmax, 0, 10, pick=n_runs - 4)      # (run n_runs - 4: scene 0)
    ends = np.arange(n_runs - 8, n_runs)
    assert host["collides"][ends[scene_of_run[ends] != 3]].all()
    assert not (host["field"][ends[scene_of_run[ends] == 3]] >= 0).any(), "the empty scene has no field to touch"
    print("fields of the runs that end in the table, by scene:", [(int(scene_of_run[k]), int(host["field"][k])) for k in ends])
    mod.batch_destroy(bid)
    mod.close()


def test_held_body():
    """the WAM with a four-sphere box in its hand: 19 active spheres"""
    mod = or_cdchomp_amd.Module(0)
    model, hand, pose = common.setup_product_wam_held4(mod)
    vmax = set_wam_vmax(mod, model)
    goals = wam_goals_with_table(32, seed=79)
    bid = mod.batch_create(model.name, goals, **dict(KW, n_points=40))
    host, dev, traj = check_workload(mod, bid, vmax, 0, 10, pick=len(goals) - 1)
    print("first contacts by sphere:", np.bincount(host["sphere"][host["collides"] == 1]).tolist())
    mod.batch_destroy(bid)
    mod.close()


def test_self_check_on_and_off():
    """the arm folds until the hand reaches the shoulder, far from any field (tests/test_gpu_commands.py): contacts of
    pairs of spheres with the robot's self check on, none with it off"""
    mod = or_cdchomp_amd.Module(0)
    model, base, dofvals, adofs = common.wam_state()
    mod.add_robot(model, transform=base, dof_values=dofvals, active_dofs=adofs)
    mod.add_kinbody_boxes("far", [([0, 0, 0, 0, 0, 0, 1], [0.05, 0.05, 0.05])], transform=[5, 5, 5, 0, 0, 0, 1])
    mod.SendCommand("computedistancefield kinbody far")
    vmax = set_wam_vmax(mod, model)
    n_runs = 24
    rng = np.random.default_rng(41)
    goals = np.tile(np.asarray(robots.WAM_START), (n_runs, 1))
    goals[:, 3] = np.linspace(2.3, 3.05, n_runs)
    goals[:, 2] += rng.uniform(-0.3, 0.3, n_runs); goals[:, 5] += rng.uniform(-0.5, 0.5, n_runs); goals[:, 4] += rng.uniform(-1, 1, n_runs)
    bid = mod.batch_create(model.name, goals, **dict(n_points=40, lambda_=100.0, obs_factor=0.0, obs_factor_self=0.0))
    host, dev, traj = check_workload(mod, bid, vmax, 0, 0)
    assert (host["field"][host["collides"] == 1] <= -2).all(), "nothing but the robot itself is near"
    n_self = int(host["collides"].sum())
    mod.set_self_check(model.name, False)
    off_host, off_dev, _ = compare(mod, bid, vmax, 0)
    assert off_dev["collides"].sum() == 0 and np.array_equal(off_dev["n_samples"], dev["n_samples"])
    mod.set_self_check(model.name, True)
    assert compare(mod, bid, vmax, 0)[1]["collides"].sum() == n_self
    mod.batch_destroy(bid)
    mod.close()


@pytest.fixture(scope="module")
def wam():
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    vmax = set_wam_vmax(mod, model)
    yield mod, model, vmax
    mod.close()


@pytest.fixture(scope="module")
def wam2():
    """the same scene on a module of two in-process shards on one card"""
    mod = or_cdchomp_amd.Module([0, 0])
    model = common.setup_product_wam(mod)
    vmax = set_wam_vmax(mod, model)
    yield mod, model, vmax
    mod.close()


def test_two_shards_plan_their_own_runs(wam, wam2):
    res = []
    goals = wam_goals_with_table(50, seed=80)
    for mod, model, vmax in (wam, wam2):
        bid = mod.batch_create(model.name, goals, **KW)
        res.append(check_workload(mod, bid, vmax, 0, 30, pick=len(goals) - 1))
        mod.batch_destroy(bid)
    assert same(res[0][2], res[1][2])
    for key in ("collides", "sphere", "field", "n_samples"):
        assert np.array_equal(res[0][1][key], res[1][1][key])
    assert same(res[0][1]["time"], res[1][1]["time"]) and same(res[0][1]["depth"], res[1][1]["depth"])


# ---- 2. degenerate trajectories --------------------------------------------------------------------------------------

def test_degenerate_trajectories(wam):
    """a trajectory that does not move has no sample (and no contact, wherever it stands); one with a NaN in a middle
    waypoint has one, at its start: the host path's results, and the runs next to them are not disturbed"""
    mod, model, vmax = wam
    n_runs = 8
    goals = wam_goals_with_table(n_runs, seed=81, k_table=2)
    bid = mod.batch_create(model.name, goals, **KW)
    traj = mod.batch_gettraj(bid)
    before = mod.batch_collision_verdict(bid, on_device=True)
    traj[1] = traj[1][0]                                     # constant, free
    traj[2] = np.asarray(IN_TABLE)                           # constant, inside the table: nothing is sampled
    traj[3, 50, 2] = np.nan
    traj[4, 50] = np.nan
    mod.batch_set_traj(bid, traj)
    host, dev, back = compare(mod, bid, vmax, 0)
    assert np.isnan(back[3, 50, 2]) and np.isnan(back[4, 50]).all(), "batch_set_traj must take the NaN"
    assert dev["n_samples"][[1, 2, 3, 4]].tolist() == [0, 0, 1, 1]
    assert dev["collides"][[1, 2, 3, 4]].tolist() == [0, 0, 0, 0]
    assert (dev["time"][[1, 2, 3, 4]] == -1.0).all()
    others = [0, 5, 6, 7]
    for key in dev:
        assert same(dev[key][others], before[key][others]), key
    assert dev["collides"][6:].all()
    mod.batch_destroy(bid)


def test_chunk_edges(wam):
    """the synthetic runs of tests/clearance.py, whose sample counts sit on the chunk's edges: a walk without a contact whose
    samples are exactly two chunks ends on an empty chunk, not on a partial one; one of no sample; one that ends on the
    second sample of a chunk"""
    mod, model, vmax = wam
    runs = CL.synthetic_runs(robots.WAM_START)
    bid = mod.batch_create(model.name, common.wam_goals(len(runs), seed=1), **dict(KW, n_points=CL.SYNTH_POINTS))
    mod.batch_set_traj(bid, runs)
    host, dev, back = compare(mod, bid, vmax, 0)
    m, z = CL.SYNTH_NAMES.index("chunk multiple"), CL.SYNTH_NAMES.index("zero length")
    assert dev["n_samples"][m] == 2 * CHUNK and host["collides"][m] == 0, "two full chunks, walked to the end"
    assert dev["n_samples"][z] == 0 and host["collides"][z] == 0
    assert host["collides"][CL.SYNTH_NAMES.index("penetrates")] == 1
    mod.batch_destroy(bid)


# ---- 3. the selection reads the verdict on the device ------------------------------------------------------------------

K = 8
N_PROBLEMS = 15
N_GROUPS = N_PROBLEMS + 1
N_RUNS = N_GROUPS * K


@pytest.mark.parametrize("shards", [1, 2])
def test_select_best_collision_free(wam, wam2, shards):
    mod, model, vmax = wam if shards == 1 else wam2
    rng = np.random.default_rng(5)
    base = common.wam_goals(N_PROBLEMS, seed=20250101)
    goals = np.concatenate([np.repeat(base, K, axis=0), np.tile(IN_TABLE, (K, 1))])
    bid = mod.batch_create(model.name, goals, **KW)
    mod.batch_perturb(bid, 0.3, np.arange(N_RUNS, dtype=np.uint32) + 9000)
    mod.batch_iterate(bid, 100)
    costs, status = mod.batch_sync(bid)
    col = mod.batch_collision_verdict(bid)["collides"]      # host-planned
    assert (col == 1).any() and (col == 0).any() and col[-K:].all()
    contiguous = contiguous_groups(N_RUNS, N_GROUPS)
    shuffled = rng.permutation(contiguous).astype(np.int32)  # groups that span the shards
    differs = False
    for grp in (contiguous, shuffled, None):
        got = mod.batch_select_best(bid, groups=grp, n_groups=N_GROUPS, collision_free=True)
        g = contiguous if grp is None else grp
        want = select_best(costs, status, col, g, N_GROUPS)
        assert np.array_equal(got[0], want[0]), (got[0], want[0])
        assert same(got[1], want[1]) and np.array_equal(got[2], want[2])
        free = select_best(costs, status, None, g, N_GROUPS)
        differs = differs or bool((free[0] != want[0]).any())
        off = mod.batch_select_best(bid, groups=grp, n_groups=N_GROUPS, collision_free=False)
        assert np.array_equal(off[0], free[0]) and same(off[1], free[1]) and np.array_equal(off[2], free[2])
    assert differs, "the verdict must matter"
    on = mod.batch_select_best(bid, n_groups=N_GROUPS, collision_free=True)
    assert on[0][-1] == -1 and on[2][-1] == 0, "no run that ends in the table is eligible"
    assert (on[0] >= 0).any(), "some problem must have a collision-free winner"
    if shards == 2:
        first = (shuffled[:N_RUNS // 2], shuffled[N_RUNS // 2:])
        assert len(np.intersect1d(*first)) > 0, "groups must span the shards"
    mod.batch_destroy(bid)


# ---- 4. independence of composition ------------------------------------------------------------------------------------

def test_a_run_does_not_depend_on_its_batch(wam, wam2):
    mod, model, vmax = wam
    mod2 = wam2[0]
    n_runs = 50
    goals = wam_goals_with_table(n_runs, seed=82)
    bid = mod.batch_create(model.name, goals, **KW)
    mod.batch_iterate(bid, 30)
    full = mod.batch_gettraj(bid)
    everything = mod.batch_collision_verdict(bid, on_device=True)
    mod.batch_destroy(bid)
    assert everything["collides"].any() and not everything["collides"].all()
    free, hit = np.flatnonzero(everything["collides"] == 0), np.flatnonzero(everything["collides"] == 1)
    sub = np.concatenate([hit[:2], free[:3], hit[-2:], free[-1:]])      # (out of order, both outcomes, a repeat when there are few)
    for m_ in (mod, mod2):
        bid = m_.batch_create(model.name, goals[sub], **KW)
        m_.batch_set_traj(bid, full[sub])
        part = m_.batch_collision_verdict(bid, on_device=True)
        m_.batch_destroy(bid)
        assert part["collides"].any() and not part["collides"].all()
        for key in everything:
            assert same(part[key], everything[key][sub]), key


# ---- 5. errors -----------------------------------------------------------------------------------------------------------

def test_rejected_calls(wam):
    mod, model, vmax = wam
    lib, h = mod._lib, mod._h
    bid = mod.batch_create(model.name, common.wam_goals(4, seed=83), **KW)
    col = np.zeros(4, dtype=np.int32)
    cp = col.ctypes.data_as(_capi.c_int_p)
    assert lib.orc_batch_collision_verdict_device(h, bid, None, None, None, None, None, None) == \
        lib.orc_batch_collision_verdict(h, bid, None, None, None, None, None) == 1
    assert lib.orc_batch_collision_verdict_device(h, bid + 1000, cp, None, None, None, None, None) == 1
    assert lib.orc_last_error(h).decode()
    assert lib.orc_batch_collision_verdict_device(h, bid, cp, None, None, None, None, None) == 0      # only collides_out is required
    assert np.array_equal(col, mod.batch_collision_verdict(bid)["collides"])
    mod.batch_destroy(bid)
