"""Host-side Python mirror of the orcdchomp module object.

``Module.SendCommand`` takes the same command strings as the reference's OpenRAVE
module (/root/reference src/orcdchomp_mod.h:58-66) and returns the same text;
errors surface as ``RuntimeError`` carrying the reference's exception message
(openravepy turns openrave_exception into a Python exception the same way).
Everything is executed by liborcdchomp_amd.so through its C ABI.
"""
import ctypes as C
import math

import numpy as np

from . import _capi, project, pushout


def _dp(a):
    return a.ctypes.data_as(_capi.c_double_p)


def _ip(a):
    return a.ctypes.data_as(_capi.c_int_p)


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def scenes_to_csr(scenes):
    """A list of scenes, each a list of (kinbody, pose7 or None), as the scene table of orc_batch_create_scenes:
    (scene_begin int32 [n_scenes + 1], kinbody names [n_fields], poses float64 [n_fields][7] with NaN rows where the
    pose is None -- or None when every pose is None).  Pure: no library call."""
    begin = [0]
    names, poses = [], []
    for sc in scenes:
        for kinbody, pose in sc:
            names.append(str(kinbody))
            if pose is None:
                poses.append(None)
            else:
                pv = np.asarray(pose, dtype=np.float64).reshape(-1)
                if pv.size != 7:
                    raise ValueError("a field placement's pose has 7 entries (x y z qx qy qz qw), not %d" % pv.size)
                poses.append(pv)
        begin.append(len(names))
    begin = np.asarray(begin, dtype=np.int32)
    if all(p is None for p in poses):
        return begin, names, None
    out = np.full((len(names), 7), np.nan)
    for k, pv in enumerate(poses):
        if pv is not None:
            out[k] = pv
    return begin, names, out


def convergence_stop(trace, rtol, patience, obs_max=float("inf")):
    """The convergence stop of orc_batch_set_convergence, applied to the cost trace of an iterate call made without it.

    trace: [n_iter][3] or [n_runs][n_iter][3] rows (total, obs, smooth) as orc_batch_get_trace returns them, NaN rows
    for iterations a run did not make.  With tot_k = obs_k + smooth_k, iteration k is settled when k > 0 (the call's first
    iteration has no predecessor), |tot_{k-1} - tot_k| <= rtol |tot_{k-1}| and obs_k <= obs_max.  The streak of settled
    iterations starts at 0 and drops to 0 on an unsettled one; the run stops after the first iteration k at which it
    reaches patience.  Returns (iters, stopped): iters = k+1 where the run stops, else the rows it made (those before its
    first NaN row); stopped True where it stops.  Arrays of n_runs entries for a 3-d trace, scalars for a 2-d one.
    Pure: no library call."""
    tr = np.asarray(trace, dtype=np.float64)
    if tr.ndim == 2:
        it, st = convergence_stop(tr[None], rtol, patience, obs_max)
        return int(it[0]), bool(st[0])
    if tr.ndim != 3 or tr.shape[2] != 3:
        raise ValueError("a trace has rows of 3 costs (total, obs, smooth)")
    if not rtol > 0 or not patience >= 1 or np.isnan(obs_max):
        raise ValueError("the criterion needs rtol > 0, patience >= 1 and obs_max not NaN")
    n_runs, n_iter = tr.shape[:2]
    iters = np.zeros(n_runs, dtype=np.int32)
    stopped = np.zeros(n_runs, dtype=bool)
    for r in range(n_runs):
        made = n_iter
        for k in range(n_iter):
            if np.isnan(tr[r, k]).all():
                made = k
                break
        iters[r] = made
        streak = 0
        for k in range(made):
            obs = float(tr[r, k, 1])
            tot = obs + float(tr[r, k, 2])     # (the kernel's pc.obs + pc.smooth: the same double as the trace's column 0)
            settled = False
            if k > 0:
                prev = float(tr[r, k - 1, 1]) + float(tr[r, k - 1, 2])
                settled = bool(abs(prev - tot) <= rtol * abs(prev)) and bool(obs <= obs_max)
            streak = streak + 1 if settled else 0
            if streak >= patience:
                iters[r] = k + 1
                stopped[r] = True
                break
    return iters, stopped


def seed_perturbation(m, n, derivative, dt, sigma, seed, lower, upper, base):
    """The seed perturbation of orc_batch_perturb for one run, from the library's host utilities (no GPU).

    base: the run's m moving rows [m][n]; lower, upper: the limits of the n columns.  xi is the first m n unit Gaussians of
    a fresh GSL stream seeded `seed` (orc_host_gsl_stream; 0 is GSL's 4357) in [waypoint][dof] order; delta = sigma c A^-1 xi
    column by column with A the smoothness metric of orc_host_metric(m, derivative, dt) and c = 1 / |row m // 2 of A^-1|_2,
    so that sigma is the standard deviation of the displacement of the middle waypoint.  Returns clip(base + delta, lower,
    upper) [m][n]; sigma == 0 returns base as it is."""
    m = int(m); n = int(n)
    base = np.array(base, dtype=np.float64).reshape(m, n)
    if not (sigma >= 0 and np.isfinite(sigma)):
        raise ValueError("sigma must be a finite number >= 0")
    if sigma == 0:
        return base
    lib = _capi.lib()
    xi = np.zeros(m * n)
    lib.orc_host_gsl_stream(int(seed), 1.0, m * n, _dp(xi), None)
    mid = np.zeros((m, 1))
    mid[m // 2, 0] = 1.0
    row = np.zeros((m, 1))
    sol = np.zeros((m, n))
    xi = np.ascontiguousarray(xi.reshape(m, n))
    if lib.orc_host_metric(m, int(derivative), float(dt), None, None, None, None, _dp(mid), 1, _dp(row)) != 0 or \
       lib.orc_host_metric(m, int(derivative), float(dt), None, None, None, None, _dp(xi), n, _dp(sol)) != 0:
        raise ValueError("no smoothness metric for m %d, derivative %d" % (m, derivative))
    c = 1.0 / float(np.sqrt(np.sum(row * row)))
    lo = np.broadcast_to(np.asarray(lower, dtype=np.float64), (n,))
    hi = np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,))
    return np.minimum(np.maximum(base + (float(sigma) * c) * sol, lo), hi)


def verdict_samples(traj, vmax, col0=0):
    """The sample plan of the collision verdict for one trajectory [n_points][n]: the library's retime_linear and
    plan_collision_samples restated line for line in scalar Python doubles (orc_host_verdict_samples is the host's own;
    the kernel of orc_batch_collision_verdict_device reproduces the same roundings).  vmax [n - col0]: the velocity limits
    of the columns col0 .. n-1.  Returns (seg int32 [], u float64 [], time float64 []): per sample the segment it lies on,
    its position on the segment, its time.  Every sum runs in index order and the clock advances by repeated addition,
    as the host's do: no numpy reduction, which adds pairwise.  Pure: no library call."""
    T = np.asarray(traj, dtype=np.float64)
    if T.ndim != 2 or T.shape[0] < 2:
        raise ValueError("a trajectory is [n_points][n] with at least two points")
    n_points, n = T.shape
    col0 = int(col0)
    vm = [float(x) for x in np.asarray(vmax, dtype=np.float64).reshape(-1)]
    if not 0 <= col0 < n or len(vm) != n - col0:
        raise ValueError("vmax has an entry for every column from col0 on")
    rows = [[float(x) for x in row] for row in T]
    # retime_linear: every segment at the largest constant velocity the limits allow
    dtm = [0.0] * n_points
    for i in range(1, n_points):
        for j in range(col0, n):
            v = vm[j - col0] if vm[j - col0] > 0.0 else 1.0
            c = abs(rows[i][j] - rows[i - 1][j]) / v
            dtm[i] = c if dtm[i] < c else dtm[i]          # std::max(dtm[i], c): a NaN candidate is ignored
    # plan_collision_samples
    total_dist = 0.0
    duration = 0.0
    for i in range(n_points - 1):
        d2 = 0.0
        for j in range(col0, n):
            d = rows[i][j] - rows[i + 1][j]
            d2 += d * d
        total_dist += math.sqrt(d2)
        duration += dtm[i + 1]
    step_time = duration * 0.04 / total_dist if total_dist > 0.0 else duration + 1.0
    seg_out, u_out, time_out = [], [], []
    seg = 0
    tseg0 = 0.0
    time = 0.0
    while time < duration:
        while seg < n_points - 2 and tseg0 + dtm[seg + 1] < time:
            tseg0 += dtm[seg + 1]
            seg += 1
        u = (time - tseg0) / dtm[seg + 1] if dtm[seg + 1] > 0.0 else 0.0
        seg_out.append(seg); u_out.append(u); time_out.append(time)
        time += step_time
    return np.asarray(seg_out, dtype=np.int32), np.asarray(u_out, dtype=np.float64), np.asarray(time_out, dtype=np.float64)


def candidates(costs, status):
    """The runs an iterate call left worth asking about: status 0 or 1 and a finite TOTAL cost -- the eligibility of
    select_best without the collision verdict, the candidates of respawn_plan before theirs, and the runs
    orc_batch_collision_verdict_subset examines with which 1 (orc_run_candidate of csrc/run_candidate.h).  costs [n_runs]
    total costs or [n_runs][3] rows as batch_iterate returns them, status [n_runs].  Returns a bool array [n_runs].  Pure
    numpy."""
    costs = np.asarray(costs, dtype=np.float64)
    total = costs[:, 0] if costs.ndim == 2 else costs.reshape(-1)
    status = np.asarray(status).reshape(-1)
    if status.shape[0] != total.shape[0]:
        raise ValueError("costs and status have one entry per run")
    return ((status == 0) | (status == 1)) & np.isfinite(total)


VERDICT_SKIPPED = -1       # collides and n_samples of a run the subset verdict did not examine
VERDICT_TOO_LONG = -2      # ... of an examined run of 2^30 samples or more


def verdict_subset(full, examine):
    """What orc_batch_collision_verdict_subset must return for the runs `examine` [n_runs] (nonzero: examined), given `full`,
    the dict batch_collision_verdict(on_device=True) returns for every run of the same batch: an examined run keeps every
    entry of `full` bit for bit; any other run reports collides -1 and n_samples -1, and time -1, sphere -1, field -1,
    depth +0 as a run without a contact does.  (A run of 2^30 samples or more has no entry in any `full` -- that call fails
    -- and reports collides -2, n_samples -2 and the rest alike.)  Returns a new dict with the keys of `full`.  Pure numpy."""
    ex = np.asarray(examine).reshape(-1) != 0
    skipped = dict(collides=VERDICT_SKIPPED, time=-1.0, sphere=-1, field=-1, depth=0.0, n_samples=VERDICT_SKIPPED)
    out = {}
    for key, val in full.items():
        val = np.asarray(val)
        if val.shape != ex.shape:
            raise ValueError("%s has %s entries for %d runs" % (key, val.shape, ex.size))
        if key not in skipped:
            raise ValueError("%s is no output of the collision verdict" % key)
        res = np.full(val.shape, skipped[key], dtype=val.dtype)
        res[ex] = val[ex]
        out[key] = res
    return out


def select_best(costs, status, collides, group_of_run, n_groups, column=0):
    """The rule of orc_batch_select_best and, with column 1 (obs) or 2 (smooth), of orc_batch_select_best_by.  costs [n_runs]
    total costs (or [n_runs][3] rows as batch_iterate returns them: needed for a column other than 0), status [n_runs],
    collides [n_runs] (None: the collision verdict is not asked for), group_of_run [n_runs] with entries in [0, n_groups).
    A run is eligible when its status is 0 or 1, its TOTAL cost is finite and it does not collide, whatever the column; per
    group the eligible run of lowest costs[run][column] wins, a tie goes to the lowest run index.  Returns (best_run int32
    [n_groups], -1 for a group without an eligible run; best_cost [n_groups], that column's value, +inf there; n_eligible
    int32 [n_groups]).  Pure numpy."""
    costs = np.asarray(costs, dtype=np.float64)
    if column not in (0, 1, 2):
        raise ValueError("column is 0 (total), 1 (obs) or 2 (smooth)")
    total = costs[:, 0] if costs.ndim == 2 else costs
    if costs.ndim == 2:
        costs = costs[:, column]
    elif column != 0:
        raise ValueError("a column other than 0 needs the [n_runs][3] cost rows")
    status = np.asarray(status).reshape(-1)
    group = np.asarray(group_of_run).reshape(-1)
    n_runs = costs.shape[0]
    if status.shape[0] != n_runs or group.shape[0] != n_runs:
        raise ValueError("costs, status and group_of_run have one entry per run")
    if n_groups < 1 or (n_runs and (group.min() < 0 or group.max() >= n_groups)):
        raise ValueError("group_of_run entries must lie in [0, n_groups)")
    ok = candidates(total, status)
    if collides is not None:
        ok &= np.asarray(collides).reshape(-1) == 0
    best_run = np.full(n_groups, -1, dtype=np.int32)
    best_cost = np.full(n_groups, np.inf)
    n_eligible = np.zeros(n_groups, dtype=np.int32)
    for r in range(n_runs):
        if not ok[r]:
            continue
        g = int(group[r])
        n_eligible[g] += 1
        if costs[r] < best_cost[g]:      # (strictly: an equal cost later in the batch does not take over)
            best_run[g] = r
            best_cost[g] = costs[r]
    return best_run, best_cost, n_eligible


def clearance_too_long(traj, vmax, col0, max_samples):
    """Whether orc_batch_clearance finds one trajectory [n_points][n] too long for `max_samples`: the rule its kernel decides
    before anything is walked, in the scalar Python doubles of verdict_samples (the same sums, in the same order):
    duration > 0 and (total_dist / 0.04 >= max_samples or step_time <= 0).  A trajectory it passes has at most max_samples + 2
    samples.  Pure: no library call."""
    T = np.asarray(traj, dtype=np.float64)
    if T.ndim != 2 or T.shape[0] < 2:
        raise ValueError("a trajectory is [n_points][n] with at least two points")
    n_points, n = T.shape
    col0 = int(col0)
    vm = [float(x) for x in np.asarray(vmax, dtype=np.float64).reshape(-1)]
    if not 0 <= col0 < n or len(vm) != n - col0:
        raise ValueError("vmax has an entry for every column from col0 on")
    rows = [[float(x) for x in row] for row in T]
    total_dist = 0.0
    duration = 0.0
    for i in range(1, n_points):
        dt = 0.0
        d2 = 0.0
        for j in range(col0, n):
            v = vm[j - col0] if vm[j - col0] > 0.0 else 1.0
            c = abs(rows[i][j] - rows[i - 1][j]) / v
            dt = c if dt < c else dt
            d = rows[i - 1][j] - rows[i][j]
            d2 += d * d
        total_dist += math.sqrt(d2)
        duration += dt
    step_time = duration * 0.04 / total_dist if total_dist > 0.0 else duration + 1.0
    return bool(duration > 0.0 and (total_dist / 0.04 >= float(max_samples) or step_time <= 0.0))


def select_clear(costs, status, clearance, n_samples, group_of_run, n_groups, margin, column):
    """The rule of orc_batch_select_clear.  costs [n_runs][3] rows as batch_iterate returns them, status [n_runs], clearance
    [n_runs][2] and n_samples [n_runs] as batch_clearance(runs="candidates") returns them, group_of_run [n_runs] with entries
    in [0, n_groups).  A run is eligible when it is a candidate (candidates), was walked (n_samples >= 0) and
    fmin(clearance[run]) >= margin.  column 0..2: the eligible run of lowest costs[run][column] wins; column 3: the one of
    largest clearance, its cost is -clearance; a tie goes to the lowest run index, and -0 ties with +0.  Returns (best_run
    int32 [n_groups], -1 for a group without an eligible run; best_cost [n_groups], +inf there; best_clearance [n_groups], NaN
    there; n_eligible int32 [n_groups]).  Pure numpy."""
    costs = np.asarray(costs, dtype=np.float64)
    if column not in (0, 1, 2, 3):
        raise ValueError("column is 0 (total), 1 (obs), 2 (smooth) or 3 (clearance)")
    if costs.ndim != 2 or costs.shape[1] != 3:
        raise ValueError("costs are the [n_runs][3] cost rows")
    margin = float(margin)
    if margin != margin:
        raise ValueError("margin is NaN")
    n_runs = costs.shape[0]
    status = np.asarray(status).reshape(-1)
    group = np.asarray(group_of_run).reshape(-1)
    clear = np.asarray(clearance, dtype=np.float64).reshape(-1, 2)
    ns = np.asarray(n_samples).reshape(-1)
    if status.shape[0] != n_runs or group.shape[0] != n_runs or clear.shape[0] != n_runs or ns.shape[0] != n_runs:
        raise ValueError("costs, status, clearance, n_samples and group_of_run have one entry per run")
    if n_groups < 1 or (n_runs and (group.min() < 0 or group.max() >= n_groups)):
        raise ValueError("group_of_run entries must lie in [0, n_groups)")
    cand = candidates(costs[:, 0], status)
    best_run = np.full(n_groups, -1, dtype=np.int32)
    best_cost = np.full(n_groups, np.inf)
    best_clear = np.full(n_groups, np.nan)
    n_eligible = np.zeros(n_groups, dtype=np.int32)
    for r in range(n_runs):
        c = float(np.fmin(clear[r, 0], clear[r, 1]))
        if not (cand[r] and ns[r] >= 0 and c >= margin):
            continue
        g = int(group[r])
        key = (costs[r, column] if column < 3 else -c) + 0.0
        n_eligible[g] += 1
        # the device's order: cost_key, in which a NaN cost is above every number and ties keep the earlier run
        if best_run[g] < 0 or cost_key(key) < cost_key(best_cost[g]):
            best_run[g] = r
            best_cost[g] = key
            best_clear[g] = c
    return best_run, best_cost, best_clear, n_eligible


def cost_key(c):
    """A cost as the unsigned key of the same order that the device compares (cost_key of csrc/cost_key.h): the
    bits of c + 0.0, so that -0 is +0, inverted for a negative number and with the sign bit set otherwise.  Python int."""
    b = int((np.float64(c) + np.float64(0.0)).view(np.uint64))
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | 0x8000000000000000


def respawn_plan(costs, status, collides, group_of_run, n_groups, keep, mode=2, column=0):
    """The rule of orc_batch_respawn: which runs of every group survive and what every other run becomes a copy of.  costs
    [n_runs][3] rows as batch_iterate returns them (or [n_runs] total costs with column 0), status [n_runs], collides
    [n_runs] (may be None with mode 0), group_of_run [n_runs] with entries in [0, n_groups).
    A run is a candidate when its status is 0 or 1 and its TOTAL cost is finite; mode 0 ignores the verdict, mode 1 drops a
    colliding run from the candidates (select_best's eligibility), mode 2 keeps it but ranks it behind every collision-free
    candidate.  A group's candidates are ordered by (collides -- mode 2 only --, cost_key(costs[run][column]), run index),
    ascending; the first min(keep, candidates) are its survivors.  A survivor's source is itself; the group's other runs,
    candidates or not, in ascending run index: the j-th gets the survivor of rank j mod n_survivors; in a group without a
    survivor every run's source is -1, the straight line.  Returns (source_of_run int32 [n_runs], n_survivors int32
    [n_groups]).  Pure numpy."""
    costs = np.asarray(costs, dtype=np.float64)
    if column not in (0, 1, 2):
        raise ValueError("column is 0 (total), 1 (obs) or 2 (smooth)")
    if mode not in (0, 1, 2):
        raise ValueError("mode is 0 (ignore), 1 (require) or 2 (prefer)")
    if keep < 1:
        raise ValueError("keep must be >= 1")
    total = costs[:, 0] if costs.ndim == 2 else costs
    if costs.ndim == 2:
        costs = costs[:, column]
    elif column != 0:
        raise ValueError("a column other than 0 needs the [n_runs][3] cost rows")
    status = np.asarray(status).reshape(-1)
    group = np.asarray(group_of_run).reshape(-1)
    n_runs = costs.shape[0]
    if status.shape[0] != n_runs or group.shape[0] != n_runs:
        raise ValueError("costs, status and group_of_run have one entry per run")
    if n_groups < 1 or (n_runs and (group.min() < 0 or group.max() >= n_groups)):
        raise ValueError("group_of_run entries must lie in [0, n_groups)")
    if mode == 0:
        hit = np.zeros(n_runs, dtype=bool)
    else:
        if collides is None:
            raise ValueError("modes 1 and 2 need the collision verdict")
        hit = np.asarray(collides).reshape(-1) != 0
        if hit.shape[0] != n_runs:
            raise ValueError("collides has one entry per run")
    candidate = candidates(total, status)
    if mode == 1:
        candidate &= ~hit
    source = np.full(n_runs, -1, dtype=np.int32)
    n_survivors = np.zeros(n_groups, dtype=np.int32)
    members = [[] for _ in range(n_groups)]
    for r in range(n_runs):
        members[int(group[r])].append(r)
    for g in range(n_groups):
        order = sorted((r for r in members[g] if candidate[r]),
                       key=lambda r: (int(hit[r]) if mode == 2 else 0, cost_key(costs[r]), r))
        survivors = order[:min(int(keep), len(order))]
        n_survivors[g] = len(survivors)
        if not survivors:
            continue
        kept = set(survivors)
        j = 0
        for r in members[g]:
            if r in kept:
                source[r] = r
            else:
                source[r] = survivors[j % len(survivors)]
                j += 1
    return source, n_survivors


RUN_PARAMS = ("lambda", "epsilon", "obs_factor", "obs_factor_self")      # the columns of the "run_params" read-back


def run_params_table(shared, n_runs, precision, lambda_=None, epsilon=None, obs_factor=None, obs_factor_self=None):
    """What orc_batch_get_state "run_params" returns after orc_batch_set_run_params with these arguments: [n_runs][4]
    doubles in the order of RUN_PARAMS.  shared: the batch's own four values (a dict with RUN_PARAMS' keys -- "lambda_" is
    accepted for "lambda" -- or a sequence in that order); each argument a scalar (every run), an array [n_runs], or None
    (the shared value); precision 32 rounds every entry to float, as the device holds it.  Raises ValueError where the call
    is rejected: a NaN or infinite entry, a lambda or epsilon <= 0 (the shared values are checked too when they are used:
    the call validates the table it would install), an array of another length.  Pure numpy."""
    if isinstance(shared, dict):
        shared = [shared["lambda_"] if (k == "lambda" and "lambda_" in shared) else shared[k] for k in RUN_PARAMS]
    shared = [float(x) for x in shared]
    if len(shared) != 4:
        raise ValueError("shared holds lambda, epsilon, obs_factor, obs_factor_self")
    if precision not in (32, 64):
        raise ValueError("precision is 32 or 64")
    n_runs = int(n_runs)
    out = np.zeros((n_runs, 4))
    for c, v in enumerate((lambda_, epsilon, obs_factor, obs_factor_self)):
        if v is None:
            col = np.full(n_runs, shared[c])
        else:
            col = np.asarray(v, dtype=np.float64)
            if col.ndim == 0:
                col = np.full(n_runs, float(col))
            col = col.reshape(-1)
            if col.size != n_runs:
                raise ValueError("%s has %d entries for %d runs" % (RUN_PARAMS[c], col.size, n_runs))
        if not np.isfinite(col).all():
            raise ValueError("%s has an entry that is not a finite number" % RUN_PARAMS[c])
        if c < 2 and not (col > 0.0).all():
            raise ValueError("%s entries must be > 0" % RUN_PARAMS[c])
        out[:, c] = col
    if precision == 32:
        out = out.astype(np.float32).astype(np.float64)
    return out


def contiguous_groups(n_runs, n_groups):
    """group_of_run of n_groups contiguous equal blocks: what orc_batch_select_best takes a NULL group_of_run for"""
    if n_groups < 1 or n_runs % n_groups:
        raise ValueError("%d runs do not divide into %d equal groups" % (n_runs, n_groups))
    return np.repeat(np.arange(n_groups, dtype=np.int32), n_runs // n_groups)


def pose_apply(pose, p):
    """cd_kin_pose_compos (reference src/libcd/kin.c:180-212) as the library's pose_apply evaluates it, in scalar Python
    doubles: the expanded quaternion products (not normalised), the factor 2 folded into the matrix, each row summed left
    to right, then the translation.  Returns a list of 3 floats.  Pure: no library call."""
    x, y, z, qx, qy, qz, qw = (float(v) for v in pose)
    qx2 = qx * qx; qy2 = qy * qy; qz2 = qz * qz; qw2 = qw * qw
    qxqy = qx * qy; qxqz = qx * qz; qxqw = qx * qw; qyqz = qy * qz; qyqw = qy * qw; qzqw = qz * qw
    R = ((qx2 - qy2 - qz2 + qw2, 2 * (qxqy - qzqw), 2 * (qxqz + qyqw)),
         (2 * (qxqy + qzqw), -qx2 + qy2 - qz2 + qw2, 2 * (qyqz - qxqw)),
         (2 * (qxqz - qyqw), 2 * (qyqz + qxqw), -qx2 - qy2 + qz2 + qw2))
    v = [float(c) for c in p]
    t = (x, y, z)
    return [(R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2]) + t[i] for i in range(3)]


def pose_invert(pose):
    """cd_kin_pose_invert (reference src/libcd/kin.c:288-326) as the library evaluates it: the conjugate quaternion, and
    minus the translation turned by it.  Returns a list of 7 floats.  Pure: no library call."""
    q = [0.0, 0.0, 0.0, -float(pose[3]), -float(pose[4]), -float(pose[5]), float(pose[6])]
    r = pose_apply(q, pose[:3])
    return [-r[0], -r[1], -r[2]] + q[3:]


def grid_interp(data, lengths, p):
    """cd_grid_double_interp (reference src/libcd/grid.c:386-454) in scalar Python doubles, operation for operation:
    returns (outside, value).  outside is True when a coordinate of p, divided by the grid's length, is not in [0, 1] (a NaN
    is outside); a cell that holds +inf, or whose neighbour on the side of p does, gives +inf (the reference's poisoning);
    the first and last cell of an axis take their neighbour inwards.  data [nx][ny][nz].  Pure: no library call."""
    data = np.asarray(data, dtype=np.float64)
    sizes = data.shape
    sub = [0, 0, 0]
    for d in range(3):
        x = float(p[d]) / float(lengths[d])
        if not (x >= 0.0 and x <= 1.0):
            return True, 0.0
        s = int(math.floor(x * sizes[d]))
        if s == sizes[d]:
            s -= 1
        sub[d] = s
    v = float(data[sub[0], sub[1], sub[2]])
    if v == math.inf:
        return False, math.inf
    for d in (2, 1, 0):
        center = (0.5 + sub[d]) / sizes[d] * float(lengths[d])
        if sub[d] == 0:
            prev = False
        elif sub[d] == sizes[d] - 1:
            prev = True
        else:
            prev = float(p[d]) < center
        lo = list(sub); hi = list(sub)
        if prev:
            lo[d] -= 1
        else:
            hi[d] += 1
        after = float(data[hi[0], hi[1], hi[2]]); before = float(data[lo[0], lo[1], lo[2]])
        if after == math.inf or before == math.inf:
            return False, math.inf
        v += (after - before) * sizes[d] / float(lengths[d]) * (float(p[d]) - center)
    return False, v


def merged_grid_dims(source_boxes, cell, bounds=None):
    """The grid orc_scene_merge_fields merges into (orc_host_merge_grid is the library's own).  source_boxes: per source
    (lengths[3], pose7): its grid's box and the grid's pose in the TARGET KINBODY's frame; cell: the edge of the merged
    grid's cubic cells; bounds: six numbers lo[3], hi[3] in the target kinbody's frame, or None: the axis-aligned box
    around the eight corners of every source's box (pose_apply of the corner).  sizes[d] = max(2, ceil((hi[d] - lo[d]) /
    cell)), lengths[d] = sizes[d] * cell, and the grid's pose in the target kinbody's frame is (lo, identity quaternion):
    the merged grid's axes are the target kinbody's.  Returns (sizes [3] ints, lengths [3] floats, pose [7] floats).
    Raises ValueError where the call is rejected.  Pure: no library call."""
    cell = float(cell)
    if not (math.isfinite(cell) and cell > 0.0):
        raise ValueError("cell must be a positive finite number")
    if bounds is not None:
        b = [float(v) for v in bounds]
        if len(b) != 6:
            raise ValueError("bounds holds lo[3] and hi[3]")
        lo, hi = b[:3], b[3:]
    else:
        if len(source_boxes) < 1:
            raise ValueError("without bounds there must be a source")
        lo = hi = None
        for lengths, pose in source_boxes:
            if not all(math.isfinite(float(v)) for v in list(lengths) + list(pose)):
                raise ValueError("poses and lengths must be finite numbers")
            for corner in range(8):
                c = [float(lengths[0]) if corner & 4 else 0.0, float(lengths[1]) if corner & 2 else 0.0,
                     float(lengths[2]) if corner & 1 else 0.0]
                w = pose_apply(pose, c)
                lo = list(w) if lo is None else [min(a, x) for a, x in zip(lo, w)]
                hi = list(w) if hi is None else [max(a, x) for a, x in zip(hi, w)]
    if not all(math.isfinite(v) for v in lo + hi):
        raise ValueError("poses and bounds must be finite numbers")
    if not all(a < b for a, b in zip(lo, hi)):
        raise ValueError("bounds must have lo < hi in every dimension")
    sizes = [max(2, int(math.ceil((hi[d] - lo[d]) / cell))) for d in range(3)]
    if sizes[0] * sizes[1] * sizes[2] * 8 >= 2 ** 31:
        raise ValueError("signed distance field too large for this build")
    lengths = [sizes[d] * cell for d in range(3)]
    return sizes, lengths, [lo[0], lo[1], lo[2], 0.0, 0.0, 0.0, 1.0]


def merged_field(sources, sizes, lengths, pose_world_gsdf, interp=grid_interp):
    """The field orc_scene_merge_fields computes (orc_host_merge_fields is the host twin, merge_fields_kernel the device's).
    sources: an ordered list of (data [nx][ny][nz], lengths [3], pose_world_gsrc [7]); sizes, lengths, pose_world_gsdf: the
    merged grid and its world pose.  For cell (i, j, k): c[d] = (0.5 + sub[d]) / sizes[d] * lengths[d] (the cell centre as
    the voxelizer forms it), p_w = pose_apply(pose_world_gsdf, c), and for every source in order p_s =
    pose_apply(pose_invert(pose_world_gsrc), p_w) and (outside, val) = interp(data, lengths, p_s); the cell is the smallest
    val, by strict <, of the sources that are not outside, starting from +inf: the best-of-N field loop of the cost function
    evaluated at the cell centre.  A poisoned (+inf) value never wins and a cell no source covers holds +inf.  interp:
    grid_interp, or another reading of cd_grid_double_interp with its signature.  Returns data [sizes].  (The library composes
    the two pose_apply calls into one affine per source, in double: the same point to a few roundings.)  Pure: no library
    call."""
    sizes = [int(s) for s in sizes]
    lengths = [float(v) for v in lengths]
    inv = [pose_invert(src[2]) for src in sources]
    out = np.full(sizes, np.inf)
    for i in range(sizes[0]):
        for j in range(sizes[1]):
            for k in range(sizes[2]):
                sub = (i, j, k)
                c = [(0.5 + sub[d]) / sizes[d] * lengths[d] for d in range(3)]
                p_w = pose_apply(pose_world_gsdf, c)
                best = math.inf
                for (data, slen, _), pinv in zip(sources, inv):
                    outside, val = interp(data, slen, pose_apply(pinv, p_w))
                    if not outside and val < best:
                        best = val
                out[i, j, k] = best
    return out


class Module:
    def __init__(self, device=0):
        """device: one HIP ordinal, or a list of them (batches are then sharded over the list inside
        this process, host-side gather, no collective)."""
        self._lib = _capi.lib()
        if isinstance(device, (list, tuple)):
            devs = np.ascontiguousarray(device, dtype=np.int32)
            self._h = self._lib.orc_module_new_multi(_ip(devs), len(devs))
        else:
            self._h = self._lib.orc_module_new(int(device))
        if not self._h:
            raise RuntimeError(self._lib.orc_last_error(None).decode())
        self._keep = []
        self._models = {}      # the robots add_robot was given, by name: what names a link or a manipulator, and the limits
        self._adofs = {}       # their active dofs as set through this object
        self._batch_robot = {} # batch id -> (robot name, its active dofs at batch_create)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.orc_module_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self._lib.orc_last_error(self._h).decode())

    # ---- the reference's surface ------------------------------------------------
    def SendCommand(self, cmd, releasegil=False):
        buf = C.create_string_buffer(4096)
        self._check(self._lib.orc_send_command(self._h, cmd.encode(), buf, len(buf)))
        size = self._lib.orc_last_reply_size(self._h)
        if size >= len(buf):
            big = C.create_string_buffer(size + 1)
            self._lib.orc_last_reply(self._h, big, len(big))
            return big.value.decode()
        return buf.value.decode()

    def set_stream(self, hip_stream):
        self._check(self._lib.orc_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_workgroup_threads(self, threads):
        """0 (default plan), 192 or 256 threads per workgroup for the batches created from now on"""
        self._check(self._lib.orc_set_workgroup_threads(self._h, int(threads)))

    def set_workgroups_per_cu(self, workgroups):
        """0 (default budget) or 4: four 256-thread workgroups per CU at 128 registers where a kernel is built for it"""
        self._check(self._lib.orc_set_workgroups_per_cu(self._h, int(workgroups)))

    def set_num_streams(self, n):
        self._check(self._lib.orc_set_num_streams(self._h, int(n)))

    # ---- environment stand-ins -----------------------------------------------------
    def add_robot(self, model, transform=None, dof_values=None, active_dofs=None):
        a = model.arrays()
        d = _capi.RobotDesc()
        d.n_links = a["n_links"]
        d.parent = _ip(a["parent"]); d.pose_parent_joint = _dp(a["pose_parent_joint"])
        d.joint_type = _ip(a["joint_type"]); d.axis = _dp(a["axis"]); d.dof_index = _ip(a["dof_index"])
        d.n_dof = a["n_dof"]
        d.limit_lower = _dp(a["limit_lower"]); d.limit_upper = _dp(a["limit_upper"])
        d.n_spheres = a["n_spheres"]
        d.sphere_link = _ip(a["sphere_link"]); d.sphere_pos = _dp(a["sphere_pos"])
        d.sphere_radius = _dp(a["sphere_radius"])
        self._check(self._lib.orc_env_add_robot(self._h, model.name.encode(), C.byref(d)))
        self._models[model.name] = model
        names =(C.c_char_p * len(model.link_names))(*[nm.encode() for nm in model.link_names])
        self._check(self._lib.orc_robot_set_link_names(self._h, model.name.encode(), names, len(model.link_names)))
        for mname, link, tool in getattr(model, "manipulators", []):
            self.add_manipulator(model.name, mname, model.link_names.index(link), tool)
        adj = getattr(model, "adjacent", [])
        if adj:
            pairs = np.ascontiguousarray([[model.link_names.index(a), model.link_names.index(b)] for a, b in adj], dtype=np.int32)
            self._check(self._lib.orc_robot_set_adjacent_links(self._h, model.name.encode(), _ip(pairs), len(adj)))
        if transform is not None:
            self.set_robot_transform(model.name, transform)
        if dof_values is not None:
            self.set_dof_values(model.name, dof_values)
        if active_dofs is not None:
            self.set_active_dofs(model.name, active_dofs)

    def add_manipulator(self, robot, name, ee_link, tool_pose=(0, 0, 0, 0, 0, 0, 1)):
        """a manipulator: end-effector link index + local tool transform (GetEndEffectorTransform = link o tool);
        the first one added is the active manipulator"""
        self._check(self._lib.orc_robot_add_manipulator(self._h, robot.encode(), name.encode(), int(ee_link), _dp(_f64(tool_pose))))

    def set_active_manipulator(self, robot, name):
        self._check(self._lib.orc_robot_set_active_manipulator(self._h, robot.encode(), name.encode()))

    def set_self_check(self, robot, enabled=True):
        """the sphere-pair stand-in for CheckSelfCollision in gettraj's re-check, per robot (default on)"""
        self._check(self._lib.orc_robot_set_self_check(self._h, robot.encode(), 1 if enabled else 0))

    def set_robot_transform(self, name, pose):
        self._check(self._lib.orc_robot_set_transform(self._h, name.encode(), _dp(_f64(pose))))

    def set_dof_values(self, name, values):
        v = _f64(values)
        self._check(self._lib.orc_robot_set_dof_values(self._h, name.encode(), _dp(v), len(v)))

    def set_active_dofs(self, name, indices):
        idx = np.ascontiguousarray(indices, dtype=np.int32)
        self._check(self._lib.orc_robot_set_active_dofs(self._h, name.encode(), _ip(idx), len(idx)))
        self._adofs[name] = [int(i) for i in idx]

    def set_velocity_limits(self, name, limits):
        v = _f64(limits)
        self._check(self._lib.orc_robot_set_velocity_limits(self._h, name.encode(), _dp(v), len(v)))

    def last_collision_details(self):
        return self._lib.orc_last_collision_details(self._h).decode()

    def batch_set_traj(self, bid, traj):
        t = _f64(traj)
        self._check(self._lib.orc_batch_set_traj(self._h, bid, _dp(t), t.size))

    def add_kinbody_boxes(self, name, boxes, transform=None):
        """boxes: list of (pose7, half_extents3) in the kinbody frame."""
        poses = _f64([b[0] for b in boxes]).reshape(-1, 7)
        halfs = _f64([b[1] for b in boxes]).reshape(-1, 3)
        self._check(self._lib.orc_env_add_kinbody_boxes(self._h, name.encode(), len(boxes), _dp(poses), _dp(halfs)))
        if transform is not None:
            self.set_kinbody_transform(name, transform)

    def add_kinbody_trimesh(self, name, triangles, transform=None):
        """triangles: [n][3][3] vertices in the kinbody frame (KinBody::InitFromTrimesh); added to a kinbody of that name if there is one"""
        tri = _f64(triangles).reshape(-1, 9)
        self._check(self._lib.orc_env_add_kinbody_trimesh(self._h, name.encode(), len(tri), _dp(tri)))
        if transform is not None:
            self.set_kinbody_transform(name, transform)

    def set_kinbody_transform(self, name, pose):
        self._check(self._lib.orc_kinbody_set_transform(self._h, name.encode(), _dp(_f64(pose))))

    def body_transform(self, name):
        """GetTransform of a robot or kinbody (a held kinbody: where its link carries it now)"""
        pose = np.zeros(7)
        self._check(self._lib.orc_body_get_transform(self._h, name.encode(), _dp(pose)))
        return pose

    def set_kinbody_spheres(self, name, pos, radius):
        """the <orcdchomp><spheres> data of a kinbody: what `create` reads from a body the robot holds"""
        pos = _f64(pos).reshape(-1, 3); radius = _f64(radius).reshape(-1)
        assert len(pos) == len(radius)
        self._check(self._lib.orc_kinbody_set_spheres(self._h, name.encode(), len(radius), _dp(pos), _dp(radius)))

    def grab(self, robot, kinbody, link):
        """RobotBase::Grab(body, link): link = robot link index"""
        self._check(self._lib.orc_robot_grab(self._h, robot.encode(), kinbody.encode(), int(link)))

    def release(self, robot, kinbody=None):
        """RobotBase::Release(body), or ReleaseAllGrabbed() without a body"""
        if kinbody is None:
            self._check(self._lib.orc_robot_release_all(self._h, robot.encode()))
        else:
            self._check(self._lib.orc_robot_release(self._h, robot.encode(), kinbody.encode()))

    def enable_kinbody(self, name, enabled=True):
        self._check(self._lib.orc_kinbody_enable(self._h, name.encode(), 1 if enabled else 0))

    # ---- fields ---------------------------------------------------------------------
    def add_sdf(self, kinbody, data, lengths, pose_kinbody_gsdf):
        data = _f64(data)
        sizes = np.asarray(data.shape, dtype=np.int32)
        self._check(self._lib.orc_scene_add_sdf(self._h, kinbody.encode(), _ip(sizes), _dp(_f64(lengths)),
                                                _dp(_f64(pose_kinbody_gsdf)), _dp(data)))

    def get_sdf(self, kinbody):
        sizes = np.zeros(3, dtype=np.int32); lengths = np.zeros(3); pose = np.zeros(7)
        self._check(self._lib.orc_scene_get_sdf(self._h, kinbody.encode(), _ip(sizes), _dp(lengths), _dp(pose), None, 0))
        data = np.zeros(tuple(int(s) for s in sizes))
        self._check(self._lib.orc_scene_get_sdf(self._h, kinbody.encode(), _ip(sizes), _dp(lengths), _dp(pose),
                                                _dp(data), data.size))
        return data, lengths, pose

    def merge_fields(self, target, fields, cell, bounds=None):
        """Bake a layout into one field (orc_scene_merge_fields; the rule is merged_grid_dims' and merged_field's): the
        fields of `fields`, a list of (kinbody, pose7 or None: where the kinbody stands now) -- the element type of
        batch_create's scenes --, resampled on the device into one grid with the axes of `target`, an existing kinbody
        without a field (add_kinbody_boxes(name, []) makes one), with cubic cells of edge `cell` over `bounds` (lo[3] + hi[3]
        in the target's frame; None: the box around all the sources).  The result is an ordinary field of `target`:
        get_sdf(target) reads it, batch_create(scenes=[[(target, None)]], ...) plans against it."""
        fields = list(fields)
        _, names, poses = scenes_to_csr([fields])
        if poses is not None:
            for k in range(len(names)):
                if fields[k][1] is None:
                    poses[k] = self.body_transform(names[k])
            poses = np.ascontiguousarray(poses)
        cnames = (C.c_char_p * max(len(names), 1))(*[nm.encode() for nm in names])
        bd = None if bounds is None else _f64(bounds).reshape(-1)
        if bd is not None and bd.size != 6:
            raise ValueError("bounds holds lo[3] and hi[3]")
        self._check(self._lib.orc_scene_merge_fields(self._h, target.encode(), len(names), cnames,
                                                     None if poses is None else _dp(poses), float(cell),
                                                     None if bd is None else _dp(bd)))

    # ---- kernel-level batch API -------------------------------------------------------
    def batch_params(self, **kw):
        p = _capi.BatchParams()
        self._lib.orc_batch_params_default(C.byref(p))
        for k, v in kw.items():
            if k in ("lambda", "lambda_"):
                p.lambda_ = v
            elif k == "D":
                p.derivative = v
            else:
                if not hasattr(p, k):
                    raise TypeError("unknown batch parameter %s" % k)
                setattr(p, k, v)
        return p

    def batch_create(self, robot, goals, starts=None, basegoals=None, seeds=None, scenes=None, scene_of_run=None, **params):
        """scenes: obstacles per run (orc_batch_create_scenes) -- a list of scenes, each a list of (kinbody, pose7 or None:
        where the kinbody stands now), and scene_of_run [n_runs] the scene of every run; without them every run sees the
        module's fields where their kinbodies stand."""
        p = self.batch_params(**params)
        goals = _f64(goals)
        goals = goals.reshape(1, -1) if goals.ndim == 1 else goals
        n_runs = goals.shape[0]
        st = None if starts is None else _f64(starts)
        bg = None if basegoals is None else _f64(basegoals)
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint32)
        bid = C.c_int(0)
        if scenes is not None or scene_of_run is not None:
            if scenes is None or scene_of_run is None:
                raise ValueError("scenes and scene_of_run go together")
            begin, names, poses = scenes_to_csr(scenes)
            if poses is not None:
                for k in range(len(names)):
                    if np.isnan(poses[k, 0]):
                        poses[k] = self.body_transform(names[k])
                poses = np.ascontiguousarray(poses)
            sor = np.ascontiguousarray(scene_of_run, dtype=np.int32).reshape(-1)
            if sor.size != n_runs:
                raise ValueError("scene_of_run has %d entries for %d runs" % (sor.size, n_runs))
            cnames = (C.c_char_p * max(len(names), 1))(*[nm.encode() for nm in names])
            self._check(self._lib.orc_batch_create_scenes(
                self._h, robot.encode(), C.byref(p), n_runs,
                None if st is None else _dp(st), _dp(goals), None if bg is None else _dp(bg),
                None if sd is None else sd.ctypes.data_as(_capi.c_uint_p),
                len(begin) - 1, _ip(begin), cnames, None if poses is None else _dp(poses), _ip(sor), C.byref(bid)))
            self._batch_robot[bid.value] = (robot, self._adofs.get(robot))
            return bid.value
        self._check(self._lib.orc_batch_create(
            self._h, robot.encode(), C.byref(p), n_runs,
            None if st is None else _dp(st), _dp(goals), None if bg is None else _dp(bg),
            None if sd is None else sd.ctypes.data_as(_capi.c_uint_p), C.byref(bid)))
        self._batch_robot[bid.value] = (robot, self._adofs.get(robot))
        return bid.value

    def batch_dims(self, bid):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.orc_batch_dims(self._h, bid, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def batch_iterate(self, bid, n_iter):
        n_runs = self.batch_dims(bid)[0]
        costs = np.zeros((n_runs, 3)); status = np.zeros(n_runs, dtype=np.int32)
        self._check(self._lib.orc_batch_iterate(self._h, bid, n_iter, _dp(costs), _ip(status)))
        return costs, status

    def batch_iterate_async(self, bid, n_iter):
        self._check(self._lib.orc_batch_iterate_async(self._h, bid, n_iter))

    def batch_sync(self, bid, fetch=True):
        if not fetch:
            self._check(self._lib.orc_batch_sync(self._h, bid, None, None))
            return None
        n_runs = self.batch_dims(bid)[0]
        costs = np.zeros((n_runs, 3)); status = np.zeros(n_runs, dtype=np.int32)
        self._check(self._lib.orc_batch_sync(self._h, bid, _dp(costs), _ip(status)))
        return costs, status

    def batch_iterations_done(self, bid):
        """iterations every run completed in the last iterate call (n_iter unless it left its joint limits or converged)"""
        n_runs = self.batch_dims(bid)[0]
        it = np.zeros(n_runs, dtype=np.int32)
        self._check(self._lib.orc_batch_iterations_done(self._h, bid, _ip(it)))
        return it

    def batch_trace(self, bid, n_iter):
        n_runs = self.batch_dims(bid)[0]
        tr = np.zeros((n_runs, n_iter, 3))
        self._check(self._lib.orc_batch_get_trace(self._h, bid, _dp(tr), tr.size))
        return tr

    def batch_set_convergence(self, bid, rtol, patience=1, obs_max=float("inf")):
        """Stop each run of the batch on the device once its cost has settled (orc_batch_set_convergence; the rule is
        convergence_stop's).  Sticky for the batch's later iterate calls; patience <= 0 switches it off.  A run that
        stops reports status 1."""
        self._check(self._lib.orc_batch_set_convergence(self._h, bid, float(rtol), int(patience), float(obs_max)))

    def batch_set_noise(self, bid, noise):
        noise = _f64(noise)
        self._check(self._lib.orc_batch_set_noise(self._h, bid, _dp(noise), noise.shape[1]))

    def batch_gettraj(self, bid):
        n_runs, n_points, n = self.batch_dims(bid)
        out = np.zeros((n_runs, n_points, n))
        self._check(self._lib.orc_batch_gettraj(self._h, bid, _dp(out), out.size))
        return out

    # ---- multi-start: perturbed seeds, the best run per problem, its trajectory ----------------------------------
    def batch_perturb(self, bid, sigma, seeds):
        """Add a smooth random displacement to the moving waypoints of every run, on the device (orc_batch_perturb; the
        rule is seed_perturbation's): sigma is the standard deviation at the middle waypoint in dof units, seeds [n_runs]
        the GSL seed of every run's displacement.  After batch_create / batch_set_traj, before batch_iterate."""
        n_runs = self.batch_dims(bid)[0]
        sd = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
        if sd.size != n_runs:
            raise ValueError("seeds has %d entries for %d runs" % (sd.size, n_runs))
        self._check(self._lib.orc_batch_perturb(self._h, bid, float(sigma), sd.ctypes.data_as(_capi.c_uint_p)))

    def batch_set_run_params(self, bid, lambda_=None, epsilon=None, obs_factor=None, obs_factor_self=None):
        """lambda, epsilon, obs_factor and obs_factor_self per run for the batch's later iterate calls
        (orc_batch_set_run_params; the table is run_params_table's).  Each argument: an array [n_runs], a scalar (every
        run), or None (the value the batch was created with).  The call replaces the whole table; all four None switches
        it off."""
        n_runs = self.batch_dims(bid)[0]
        arrs = []
        for name, v in zip(RUN_PARAMS, (lambda_, epsilon, obs_factor, obs_factor_self)):
            if v is None:
                arrs.append(None)
                continue
            a = np.asarray(v, dtype=np.float64)
            a = np.full(n_runs, float(a)) if a.ndim == 0 else np.ascontiguousarray(a.reshape(-1))
            if a.size != n_runs:
                raise ValueError("%s has %d entries for %d runs" % (name, a.size, n_runs))
            arrs.append(a)
        self._check(self._lib.orc_batch_set_run_params(self._h, bid, *[None if a is None else _dp(a) for a in arrs]))

    def batch_select_best(self, bid, groups=None, n_groups=None, collision_free=True, by="total"):
        """The best run of every group after an iterate call, reduced on the device (orc_batch_select_best; the rule is
        select_best's).  by: the cost that is minimised and returned, "total" (the default), "obs" or "smooth"
        (orc_batch_select_best_by: the one that compares across runs of different obs_factor is "smooth").  groups: group_of_run [n_runs] (n_groups defaults to its maximum + 1), or None for n_groups
        contiguous equal blocks (one group when n_groups is None too).  Returns (best_run int32 [n_groups], -1 for a
        group without an eligible run; best_cost [n_groups], +inf there; n_eligible int32 [n_groups])."""
        if by not in ("total", "obs", "smooth"):
            raise ValueError('by is "total", "obs" or "smooth"')
        n_runs = self.batch_dims(bid)[0]
        gp = None
        if groups is not None:
            gp = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
            if gp.size != n_runs:
                raise ValueError("groups has %d entries for %d runs" % (gp.size, n_runs))
            if n_groups is None:
                n_groups = int(gp.max()) + 1
        elif n_groups is None:
            n_groups = 1
        n_groups = int(n_groups)
        size = max(n_groups, 1)
        best = np.zeros(size, dtype=np.int32); cost = np.zeros(size); cnt = np.zeros(size, dtype=np.int32)
        if by == "total":
            self._check(self._lib.orc_batch_select_best(self._h, bid, n_groups, None if gp is None else _ip(gp),
                                                        1 if collision_free else 0, _ip(best), _dp(cost), _ip(cnt)))
        else:
            self._check(self._lib.orc_batch_select_best_by(self._h, bid, ("total", "obs", "smooth").index(by), n_groups,
                                                           None if gp is None else _ip(gp), 1 if collision_free else 0,
                                                           _ip(best), _dp(cost), _ip(cnt)))
        return best[:n_groups], cost[:n_groups], cnt[:n_groups]

    def batch_respawn(self, bid, keep, sigma, seeds, groups=None, n_groups=None, collision="prefer", by="total"):
        """Successive halving between two iterate calls, on the device (orc_batch_respawn; the rule is respawn_plan's):
        every group keeps its best `keep` runs untouched, and every other run of the group becomes a copy of one of them
        (moving waypoints, momentum), perturbed like batch_perturb(sigma, seeds) would perturb it; a group without a
        candidate restarts from the straight line.  The runs of a group are meant to share start and goal: a copy keeps
        its own end rows.  collision: "ignore", "require" (a colliding run is no candidate) or "prefer" (it ranks behind
        every collision-free one); by: "total", "obs" or "smooth", the cost that orders the candidates; groups and
        n_groups as in batch_select_best.  sigma 0 clones only, and seeds may then be None.  Afterwards the batch counts as
        not iterated: batch_select_best and another batch_respawn need an iterate call first (0 iterations are enough).
        Returns (source_of_run int32 [n_runs]: the run itself for a survivor, -1 for the straight line; n_survivors int32
        [n_groups])."""
        if by not in ("total", "obs", "smooth"):
            raise ValueError('by is "total", "obs" or "smooth"')
        if collision not in ("ignore", "require", "prefer"):
            raise ValueError('collision is "ignore", "require" or "prefer"')
        n_runs = self.batch_dims(bid)[0]
        gp = None
        if groups is not None:
            gp = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
            if gp.size != n_runs:
                raise ValueError("groups has %d entries for %d runs" % (gp.size, n_runs))
            if n_groups is None:
                n_groups = int(gp.max()) + 1
        elif n_groups is None:
            n_groups = 1
        n_groups = int(n_groups)
        sd = None
        if seeds is not None:
            sd = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
            if sd.size != n_runs:
                raise ValueError("seeds has %d entries for %d runs" % (sd.size, n_runs))
        source = np.zeros(n_runs, dtype=np.int32); kept = np.zeros(max(n_groups, 1), dtype=np.int32)
        self._check(self._lib.orc_batch_respawn(self._h, bid, ("total", "obs", "smooth").index(by), n_groups,
                                                None if gp is None else _ip(gp), ("ignore", "require", "prefer").index(collision),
                                                int(keep), float(sigma), None if sd is None else sd.ctypes.data_as(_capi.c_uint_p),
                                                _ip(source), _ip(kept)))
        return source, kept[:n_groups]

    def batch_gettraj_runs(self, bid, runs):
        """The rows `runs` of batch_gettraj, gathered on the device (orc_batch_gettraj_runs): [len(runs)][n_points][n];
        an entry -1 (select_best's "no eligible run") gives a row of NaN, duplicates are allowed."""
        _, n_points, n = self.batch_dims(bid)
        rs = np.ascontiguousarray(runs, dtype=np.int32).reshape(-1)
        out = np.zeros((rs.size, n_points, n))
        self._check(self._lib.orc_batch_gettraj_runs(self._h, bid, _ip(rs), rs.size, _dp(out), out.size))
        return out

    def batch_set_verdict_scope(self, bid, scope):
        """Which runs the verdict inside batch_select_best(collision_free=True) and batch_respawn("require" / "prefer")
        examines (orc_batch_set_verdict_scope): "all", the default, or "candidates" (candidates(costs, status): the only runs
        those calls can pick).  The results of those calls do not depend on it; what changes is what the verdict walks, and
        that a run which is no candidate can no longer fail them by being too long.  Kept until it is set again."""
        if scope not in ("all", "candidates"):
            raise ValueError('scope is "all" or "candidates"')
        self._check(self._lib.orc_batch_set_verdict_scope(self._h, bid, ("all", "candidates").index(scope)))

    def batch_collision_verdict(self, bid, on_device=False, runs=None, count=True):
        """gettraj's collision re-check for every run of the batch, on the device: returns a dict of
        arrays per run: collides (0/1), time of the first contact on the retimed trajectory, XML index
        of the sphere, index of the field, penetration depth [m].  on_device: the samples are planned on the device
        too (orc_batch_collision_verdict_device; the plan is verdict_samples'): the same results without a read-back of
        the trajectories, and n_samples, the samples of every run's retimed trajectory.  runs (with on_device): a boolean /
        0-1 array [n_runs] of the runs to examine, or "candidates" (candidates(costs, status) of the last iterate call,
        decided on the device): orc_batch_collision_verdict_subset, whose result is verdict_subset's -- a run that is not
        examined costs nothing and reports collides -1, an examined run of 2^30 samples or more reports -2 instead of
        failing the call.  count=False (with runs): n_samples_out == NULL, the samples behind a first contact are not
        counted and the dict has no n_samples; the other entries are the same"""
        n_runs = self.batch_dims(bid)[0]
        col = np.zeros(n_runs, dtype=np.int32); sph = np.zeros(n_runs, dtype=np.int32); fld = np.zeros(n_runs, dtype=np.int32)
        tim = np.zeros(n_runs); dep = np.zeros(n_runs)
        if runs is not None:
            if not on_device:
                raise ValueError("runs needs on_device=True: the host-planned verdict reads every trajectory back")
            cnt = np.zeros(n_runs, dtype=np.int32) if count else None
            if isinstance(runs, str):
                if runs != "candidates":
                    raise ValueError('runs is an array [n_runs] or "candidates"')
                which, ex = 1, None
            else:
                ex = np.ascontiguousarray(np.asarray(runs).reshape(-1) != 0, dtype=np.uint8)
                if ex.size != n_runs:
                    raise ValueError("runs has %d entries for %d runs" % (ex.size, n_runs))
                which = 0
            self._check(self._lib.orc_batch_collision_verdict_subset(
                self._h, bid, which, None if ex is None else ex.ctypes.data_as(_capi.c_ubyte_p), _ip(col), _dp(tim), _ip(sph),
                _ip(fld), _dp(dep), None if cnt is None else _ip(cnt)))
            out = dict(collides=col, time=tim, sphere=sph, field=fld, depth=dep)
            if cnt is not None:
                out["n_samples"] = cnt
            return out
        if not count:
            raise ValueError("count=False needs runs: the all-runs verdict always counts")
        if on_device:
            cnt = np.zeros(n_runs, dtype=np.int32)
            self._check(self._lib.orc_batch_collision_verdict_device(self._h, bid, _ip(col), _dp(tim), _ip(sph), _ip(fld), _dp(dep),
                                                                     _ip(cnt)))
            return dict(collides=col, time=tim, sphere=sph, field=fld, depth=dep, n_samples=cnt)
        self._check(self._lib.orc_batch_collision_verdict(self._h, bid, _ip(col), _dp(tim), _ip(sph), _ip(fld), _dp(dep)))
        return dict(collides=col, time=tim, sphere=sph, field=fld, depth=dep)

    def batch_clearance(self, bid, runs=None, max_samples=65536):
        """How far every run stays from the fields of its scene and from itself, on the device (orc_batch_clearance): the
        walk of batch_collision_verdict(on_device=True) without its stop at a contact.  runs: None (every run), "candidates"
        (candidates(costs, status) of the last iterate call) or a boolean / 0-1 array [n_runs].  Returns a dict of arrays:
        clearance [n_runs][2] (the smallest value - radius over spheres and fields; the smallest distance - radius sum over
        the self-collision pairs), time [n_runs][2], sphere [n_runs][2], other [n_runs][2] (the field; the other sphere),
        n_samples [n_runs].  A minimum over nothing is +inf with time -1 and sphere, other -1.  A run that is not examined
        reports NaN / -1 and n_samples -1; one that clearance_too_long(traj, vmax, col0, max_samples) marks the same with
        n_samples -2."""
        n_runs = self.batch_dims(bid)[0]
        if runs is None:
            which, ex = 2, None
        elif isinstance(runs, str):
            if runs != "candidates":
                raise ValueError('runs is None, an array [n_runs] or "candidates"')
            which, ex = 1, None
        else:
            ex = np.ascontiguousarray(np.asarray(runs).reshape(-1) != 0, dtype=np.uint8)
            if ex.size != n_runs:
                raise ValueError("runs has %d entries for %d runs" % (ex.size, n_runs))
            which = 0
        clr = np.zeros((n_runs, 2)); tim = np.zeros((n_runs, 2))
        sph = np.zeros((n_runs, 2), dtype=np.int32); oth = np.zeros((n_runs, 2), dtype=np.int32)
        cnt = np.zeros(n_runs, dtype=np.int32)
        self._check(self._lib.orc_batch_clearance(self._h, bid, which, None if ex is None else ex.ctypes.data_as(_capi.c_ubyte_p),
                                                  int(max_samples), _dp(clr), _dp(tim), _ip(sph), _ip(oth), _ip(cnt)))
        return dict(clearance=clr, time=tim, sphere=sph, other=oth, n_samples=cnt)

    def _config_queries(self, bid, configs, runs):
        """the arguments of the calls that take configurations: (configs [n_q][n] of doubles, runs int32 [n_q] or None)"""
        n_runs, _, n = self.batch_dims(bid)
        cf = np.ascontiguousarray(configs, dtype=np.float64)
        if cf.ndim == 1:
            cf = cf.reshape(1, -1)
        if cf.ndim != 2 or cf.shape[1] != n or cf.shape[0] < 1:
            raise ValueError("configs is [n_q][%d], n_q >= 1" % n)
        n_q = cf.shape[0]
        rq = None
        if runs is not None:
            rq = np.asarray(runs)
            rq = np.full(n_q, int(rq), dtype=np.int32) if rq.ndim == 0 else np.ascontiguousarray(rq, dtype=np.int32).reshape(-1)
            if rq.size != n_q:
                raise ValueError("runs has %d entries for %d configurations" % (rq.size, n_q))
            if ((rq < 0) | (rq >= n_runs)).any():
                raise ValueError("a run lies outside [0, %d)" % n_runs)
        return cf, rq

    def _waypoint_queries(self, bid, runs, points):
        """the arguments of the calls that take waypoints: (runs, points: int32 [n_q], or both None for the profile; the
        shape of the answer without its last axis)"""
        n_runs, n_points, _ = self.batch_dims(bid)
        if points is None and runs is not None:
            raise ValueError("runs needs points: both None is the whole profile")
        shape = (n_runs, n_points)
        rq = pq = None
        if points is not None:
            pq = np.asarray(points)
            if pq.dtype.kind not in "iu":
                raise ValueError("points is an int or a sequence of ints")
            pq = pq.astype(np.int64).reshape(-1)
            if ((pq < -n_points) | (pq >= n_points)).any():
                raise ValueError("a point lies outside [-%d, %d)" % (n_points, n_points))
            pq = np.where(pq < 0, pq + n_points, pq)
            if runs is None:
                if pq.size < 1:
                    raise ValueError("points is empty")
                shape = (n_runs, pq.size)
                rq = np.repeat(np.arange(n_runs), pq.size)
                pq = np.tile(pq, n_runs)
            else:
                rq = np.ascontiguousarray(runs, dtype=np.int32).reshape(-1)
                if rq.size != pq.size or rq.size < 1:
                    raise ValueError("runs has %d entries for %d points" % (rq.size, pq.size))
                if ((rq < 0) | (rq >= n_runs)).any():
                    raise ValueError("a run lies outside [0, %d)" % n_runs)
                shape = (rq.size,)
            rq = np.ascontiguousarray(rq, dtype=np.int32); pq = np.ascontiguousarray(pq, dtype=np.int32)
        return rq, pq, shape

    def batch_config_clearance(self, bid, configs, runs=None):
        """The clearance of given configurations, on the device (orc_batch_config_clearance): the per-sample body of
        batch_clearance's walk without a trajectory around it.  configs [n_q][n] (or one row [n]), rows as batch_gettraj
        returns them; runs: the run whose scene each is tested against, an int array [n_q], one int for all, or None for
        run 0.  Returns a dict: clearance [n_q][2] (fields; self), sphere [n_q][2], other [n_q][2] (the field; the other
        sphere).  A minimum over nothing is +inf with -1, -1; a row with a non-finite entry reports NaN with -1, -1."""
        cf, rq = self._config_queries(bid, configs, runs)
        n_q = cf.shape[0]
        clr = np.zeros((n_q, 2)); sph = np.zeros((n_q, 2), dtype=np.int32); oth = np.zeros((n_q, 2), dtype=np.int32)
        self._check(self._lib.orc_batch_config_clearance(self._h, bid, n_q, None if rq is None else _ip(rq), _dp(cf), _dp(clr),
                                                         _ip(sph), _ip(oth)))
        return dict(clearance=clr, sphere=sph, other=oth)

    def batch_config_chunk(self, bid):
        """how many consecutive queries a workgroup of the configuration-clearance kernel takes for this batch (64, or what
        the LDS of a CU holds of the robot); a query's answer does not depend on it"""
        out = np.zeros(1)
        self._check(self._lib.orc_batch_get_state(self._h, bid, b"config_chunk", _dp(out), out.size))
        return int(out[0])

    def batch_waypoint_clearance(self, bid, runs=None, points=None):
        """The clearance of waypoints of the batch's trajectories as they stand on the device
        (orc_batch_waypoint_clearance); nothing is uploaded but indices.  runs and points None: the whole profile, arrays
        [n_runs][n_points][2].  points an int or a sequence with runs None: those waypoints of every run,
        [n_runs][len(points)][2]; a negative index counts from the end, so points=(0, -1) is "starts and goals".  runs and
        points both arrays [n_q]: those waypoints, [n_q][2].  Returns a dict: clearance, sphere, other, as
        batch_config_clearance."""
        rq, pq, shape = self._waypoint_queries(bid, runs, points)
        n_q = int(np.prod(shape))
        clr = np.zeros(shape + (2,)); sph = np.zeros(shape + (2,), dtype=np.int32); oth = np.zeros(shape + (2,), dtype=np.int32)
        self._check(self._lib.orc_batch_waypoint_clearance(self._h, bid, n_q, None if rq is None else _ip(rq),
                                                           None if pq is None else _ip(pq), _dp(clr), _ip(sph), _ip(oth)))
        return dict(clearance=clr, sphere=sph, other=oth)

    def batch_path_clearance(self, bid, paths, runs=None, max_samples=65536):
        """The clearance of given paths, on the device (orc_batch_path_clearance): per path what batch_clearance reports for
        a run that holds it as its trajectory, bit for bit, whatever n_points the batch has.  paths [n_q][n_rows][n] (or one
        path [n_rows][n]), rows as batch_gettraj returns them, n_rows >= 2; [n_q][2][n] are segments.  runs: the run whose
        scene each is tested against, an int array [n_q], one int for all, or None for run 0.  Returns a dict with the keys
        of batch_clearance: clearance, time, sphere, other [n_q][2], n_samples [n_q].  The samples are verdict_samples': THE
        END ROW IS NOT ONE (ask batch_config_clearance about it).  A path of zero length has no sample (+inf, -1, -1 / -1,
        n_samples 0); one that clearance_too_long(path, vmax, col0, max_samples) marks reports NaN / -1 and n_samples -2."""
        n_runs, _, n = self.batch_dims(bid)
        pt = np.ascontiguousarray(paths, dtype=np.float64)
        if pt.ndim == 2:
            pt = pt.reshape((1,) + pt.shape)
        if pt.ndim != 3 or pt.shape[2] != n or pt.shape[0] < 1:
            raise ValueError("paths is [n_q][n_rows][%d], n_q >= 1" % n)
        n_q, n_rows = pt.shape[0], pt.shape[1]
        rq = None
        if runs is not None:
            rq = np.asarray(runs)
            rq = np.full(n_q, int(rq), dtype=np.int32) if rq.ndim == 0 else np.ascontiguousarray(rq, dtype=np.int32).reshape(-1)
            if rq.size != n_q:
                raise ValueError("runs has %d entries for %d paths" % (rq.size, n_q))
        clr = np.zeros((n_q, 2)); tim = np.zeros((n_q, 2))
        sph = np.zeros((n_q, 2), dtype=np.int32); oth = np.zeros((n_q, 2), dtype=np.int32)
        cnt = np.zeros(n_q, dtype=np.int32)
        self._check(self._lib.orc_batch_path_clearance(self._h, bid, n_q, None if rq is None else _ip(rq), n_rows, _dp(pt),
                                                       int(max_samples), _dp(clr), _dp(tim), _ip(sph), _ip(oth), _ip(cnt)))
        return dict(clearance=clr, time=tim, sphere=sph, other=oth, n_samples=cnt)

    def batch_waypoint_segment_clearance(self, bid, runs, points_from, points_to, max_samples=65536):
        """The clearance of the straight segments between waypoints of the batch's trajectories as they stand on the device
        (orc_batch_waypoint_segment_clearance); nothing is uploaded but indices.  runs, points_from, points_to: int arrays
        [n_q] (one int stands for all); query q is the segment from T[runs[q]][points_from[q]] to T[runs[q]][points_to[q]],
        from > to the reverse direction, from == to without a sample.  Returns what batch_path_clearance returns for those
        two rows, bit for bit."""
        arrs = [np.asarray(a) for a in (runs, points_from, points_to)]
        n_q = max([a.size for a in arrs if a.ndim] or [1])
        arrs = [np.full(n_q, int(a), dtype=np.int32) if a.ndim == 0 else np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in arrs]
        if n_q < 1 or any(a.size != n_q for a in arrs):
            raise ValueError("runs, points_from and points_to have one entry per segment")
        rq, fq, tq = arrs
        clr = np.zeros((n_q, 2)); tim = np.zeros((n_q, 2))
        sph = np.zeros((n_q, 2), dtype=np.int32); oth = np.zeros((n_q, 2), dtype=np.int32)
        cnt = np.zeros(n_q, dtype=np.int32)
        self._check(self._lib.orc_batch_waypoint_segment_clearance(self._h, bid, n_q, _ip(rq), _ip(fq), _ip(tq), int(max_samples),
                                                                   _dp(clr), _dp(tim), _ip(sph), _ip(oth), _ip(cnt)))
        return dict(clearance=clr, time=tim, sphere=sph, other=oth, n_samples=cnt)

    @staticmethod
    def _margins(margin):
        m = np.asarray(margin, dtype=np.float64).reshape(-1)
        if m.size == 1:
            m = np.repeat(m, 2)
        if m.size != 2 or not np.isfinite(m).all() or (m < 0).any():
            raise ValueError("margin is (fields, self): finite and not negative")
        return float(m[0]), float(m[1])

    def batch_config_penetration(self, bid, configs, runs=None, margin=(0.02, 0.0)):
        """Which way is out of contact, on the device (orc_batch_config_penetration): configs and runs as in
        batch_config_clearance; margin (fields, self) in metres.  Returns a dict: cost [n_q][2], the penetration cost
        1/2 sum max(0, margin - gap)^2 of the field leg and of the self-collision leg; grad [n_q][n], the derivative of their
        sum with respect to the row; clearance, sphere, other as batch_config_clearance returns them, bit for bit.  A row
        with a non-finite entry reports NaN everywhere and -1, -1."""
        cf, rq = self._config_queries(bid, configs, runs)
        mf, ms = self._margins(margin)
        n_q, n = cf.shape
        cst = np.zeros((n_q, 2)); grd = np.zeros((n_q, n)); clr = np.zeros((n_q, 2))
        sph = np.zeros((n_q, 2), dtype=np.int32); oth = np.zeros((n_q, 2), dtype=np.int32)
        self._check(self._lib.orc_batch_config_penetration(self._h, bid, n_q, None if rq is None else _ip(rq), _dp(cf), mf, ms, _dp(cst),
                                                           _dp(grd), _dp(clr), _ip(sph), _ip(oth)))
        return dict(cost=cst, grad=grd, clearance=clr, sphere=sph, other=oth)

    def batch_penetration_chunk(self, bid):
        """how many consecutive queries a workgroup of the penetration kernel takes for this batch; a query's answer does
        not depend on it"""
        out = np.zeros(1)
        self._check(self._lib.orc_batch_get_state(self._h, bid, b"penetration_chunk", _dp(out), out.size))
        return int(out[0])

    def batch_waypoint_penetration(self, bid, runs=None, points=None, margin=(0.02, 0.0)):
        """batch_config_penetration of waypoints of the batch's trajectories as they stand on the device
        (orc_batch_waypoint_penetration); runs and points as in batch_waypoint_clearance, and the arrays of the answer are
        shaped the same way, grad with n as its last axis."""
        rq, pq, shape = self._waypoint_queries(bid, runs, points)
        mf, ms = self._margins(margin)
        n = self.batch_dims(bid)[2]
        n_q = int(np.prod(shape))
        cst = np.zeros(shape + (2,)); grd = np.zeros(shape + (n,)); clr = np.zeros(shape + (2,))
        sph = np.zeros(shape + (2,), dtype=np.int32); oth = np.zeros(shape + (2,), dtype=np.int32)
        self._check(self._lib.orc_batch_waypoint_penetration(self._h, bid, n_q, None if rq is None else _ip(rq),
                                                             None if pq is None else _ip(pq), mf, ms, _dp(cst), _dp(grd), _dp(clr),
                                                             _ip(sph), _ip(oth)))
        return dict(cost=cst, grad=grd, clearance=clr, sphere=sph, other=oth)

    def batch_push_out(self, bid, configs, runs=None, margin=(0.02, 0.0), slack=2e-3, max_steps=20, step_cap=0.2, lower=None,
                       upper=None):
        """Move configurations in contact out to `margin` (pushout.push_out around batch_config_penetration): configs and
        runs as in batch_config_penetration, lower and upper [n] the limits a row is clipped to (None: none).  Returns (rows
        [n_q][n], steps int32 [n_q], status int32 [n_q]: 0 clear, 1 the gradient vanished while in contact, 2 out of steps)."""
        cf, rq = self._config_queries(bid, configs, runs)

        def evaluate(rows, m, index):      # (the rows still active: their runs go with them)
            return self.batch_config_penetration(bid, rows, runs=None if rq is None else rq[index], margin=m)

        return pushout.push_out(evaluate, cf, margin, slack, max_steps, step_cap, lower, upper, indexed=True)

    def _batch_model(self, bid):
        """(model, active dofs or None) of the batch's robot: what batch_create recorded, or the only robot there is"""
        name, adofs = self._batch_robot.get(bid, (None, None))
        if name is None and len(self._models) == 1:
            name = next(iter(self._models))
            adofs = self._adofs.get(name)
        if name not in self._models:
            raise ValueError("the robot of batch %d is not known to this object: address the end effector by a link index, and pass "
                             "lower and upper" % bid)
        return self._models[name], adofs

    def _tsr_records(self, bid, tsrs, link, manip):
        """robots.Tsr objects as an array of orc_tsr.  The end effector is addressed as the head of `con_tsr '...'` addresses it:
        neither link nor manip: the active manipulator; manip NAME: that manipulator's link and tool; link NAME (or a link
        index): that link's frame."""
        if isinstance(tsrs, tuple) and len(tsrs) == 2 and isinstance(tsrs[0], C.Array):
            return tsrs      # (records made before: batch_tsr_records)
        tsrs = list(tsrs) if isinstance(tsrs, (list, tuple)) else [tsrs]
        if not tsrs:
            raise ValueError("tsrs is empty")
        if link is not None and manip is not None:
            raise ValueError("link and manip exclude each other")
        ee, tool = -1, [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
        if manip is not None:
            model, _ = self._batch_model(bid)
            found = [m for m in model.manipulators if m[0] == manip]
            if not found:
                raise ValueError("con_tsr manip not found!")
            ee, tool = model.link_names.index(found[0][1]), [float(v) for v in found[0][2]]
        elif link is not None:
            if isinstance(link, str):
                model, _ = self._batch_model(bid)
                if link not in model.link_names:
                    raise ValueError("con_tsr link not found!")
                link = model.link_names.index(link)
            ee = int(link)
            if ee < 0:
                raise ValueError("con_tsr link not found!")
        rec = (_capi.Tsr * len(tsrs))()
        ks = np.zeros(len(tsrs), dtype=np.int32)
        for t, tsr in enumerate(tsrs):
            T0w, Twe = tsr.poses()
            rec[t].ee_link = ee
            for i in range(7):
                rec[t].tool[i] = tool[i]; rec[t].T0w[i] = float(T0w[i]); rec[t].Twe[i] = float(Twe[i])
            for r in range(6):
                rec[t].Bw[r][0] = float(tsr.Bw[r, 0]); rec[t].Bw[r][1] = float(tsr.Bw[r, 1])
            ks[t] = int(((tsr.Bw[:, 0] == 0.0) & (tsr.Bw[:, 1] == 0.0)).sum())
        return rec, ks

    def batch_tsr_records(self, bid, tsrs, link=None, manip=None):
        """the form batch_config_tsr and batch_project_tsr turn their tsrs into, made once for many calls: pass the result as
        `tsrs` (link and manip are then those given here)"""
        return self._tsr_records(bid, tsrs, link, manip)

    def _tsr_queries(self, bid, configs, tsr_of, n_tsr):
        n = self.batch_dims(bid)[2]
        cf = np.ascontiguousarray(configs, dtype=np.float64)
        if cf.ndim == 1:
            cf = cf.reshape(1, -1)
        if cf.ndim != 2 or cf.shape[1] != n or cf.shape[0] < 1:
            raise ValueError("configs is [n_q][%d], n_q >= 1" % n)
        tq = None
        if tsr_of is not None:
            tq = np.ascontiguousarray(tsr_of, dtype=np.int32).reshape(-1)
            if tq.size != cf.shape[0]:
                raise ValueError("tsr_of has %d entries for %d configurations" % (tq.size, cf.shape[0]))
            if ((tq < 0) | (tq >= n_tsr)).any():
                raise ValueError("a tsr_of entry lies outside [0, %d)" % n_tsr)
        return cf, tq

    def batch_config_tsr(self, bid, tsrs, configs, tsr_of=None, link=None, manip=None):
        """The value and the Jacobian of task space regions at given configurations, on the device (orc_batch_config_tsr).
        tsrs: robots.Tsr objects (or one); configs [n_q][n] (or one row), rows as batch_gettraj returns them; tsr_of [n_q]: the
        TSR of every row (None: the first); link / manip: the end effector, as the head of `con_tsr '...'` names it (neither:
        the active manipulator).  Returns a dict: h [n_q][6], the k enforced entries of the xyzrpy value in the order of the Bw
        rows; jac [n_q][6][n], their Jacobian rows; k int32 [n_q]; rows from k on are zero.  These are the h and J the
        constraint step of batch_iterate sees for a trajectory row."""
        rec, ks = self._tsr_records(bid, tsrs, link, manip)
        cf, tq = self._tsr_queries(bid, configs, tsr_of, len(rec))
        n_q, n = cf.shape
        h = np.zeros((n_q, 6)); jac = np.zeros((n_q, 6, n))
        self._check(self._lib.orc_batch_config_tsr(self._h, bid, len(rec), rec, n_q, None if tq is None else _ip(tq), _dp(cf), _dp(h),
                                                   _dp(jac)))
        return dict(h=h, jac=jac, k=ks[tq] if tq is not None else np.full(n_q, ks[0], dtype=np.int32))

    def _project_box(self, bid, lower, upper, n):
        """[lower, upper] of a projection as arrays [n] or None ("limits": the robot's joint limits of the batch's active dofs)"""
        box = []
        for name, side in (("limit_lower", lower), ("limit_upper", upper)):
            if isinstance(side, str):
                if side != "limits":
                    raise ValueError('lower and upper are arrays [n], None or "limits"')
                model, adofs = self._batch_model(bid)
                lim = np.asarray(getattr(model, name), dtype=np.float64)
                side = lim[adofs] if adofs is not None else lim
            if side is not None:
                side = np.ascontiguousarray(side, dtype=np.float64).reshape(-1)
                if side.size != n:
                    raise ValueError("lower and upper have %d entries, one per column" % n)
            box.append(side)
        return box

    def batch_project_tsr(self, bid, tsrs, configs, tsr_of=None, link=None, manip=None, lower="limits", upper="limits", tol=1e-6,
                          mu=1e-8, step_cap=0.5, max_steps=30, clearance=False, runs=None):
        """Project configurations onto task space regions, the whole iteration on the device (orc_batch_project_tsr; the rule is
        project.project): batched inverse kinematics with thousands of seeds at once.  tsrs, configs, tsr_of, link and manip as
        in batch_config_tsr; lower, upper [n]: the box every step is clipped to ("limits": the robot's joint limits of the
        batch's active dofs; None: no box).  Returns (rows [n_q][n], resid [n_q], steps int32 [n_q], status int32 [n_q]: 0
        within tol, 1 a singular system or a step that moves nothing, 2 out of steps, 3 a row with a non-finite entry).  A row
        that is not done is the visited iterate of smallest residual.  clearance=True appends batch_config_clearance's dict of
        the returned rows (runs: the run whose scene each is tested against, as there): what keeps the collision-free
        solutions."""
        rec, _ = self._tsr_records(bid, tsrs, link, manip)
        cf, tq = self._tsr_queries(bid, configs, tsr_of, len(rec))
        n_q, n = cf.shape
        box = self._project_box(bid, lower, upper, n)
        rows = np.zeros((n_q, n)); resid = np.zeros(n_q)
        steps = np.zeros(n_q, dtype=np.int32); status = np.zeros(n_q, dtype=np.int32)
        self._check(self._lib.orc_batch_project_tsr(self._h, bid, len(rec), rec, n_q, None if tq is None else _ip(tq), _dp(cf),
                                                    None if box[0] is None else _dp(box[0]), None if box[1] is None else _dp(box[1]),
                                                    int(max_steps), float(tol), float(mu), float(step_cap), _dp(rows), _dp(resid),
                                                    _ip(steps), _ip(status)))
        if clearance:
            return rows, resid, steps, status, self.batch_config_clearance(bid, rows, runs=runs)
        return rows, resid, steps, status

    def batch_project_tsr_clear(self, bid, tsrs, configs, tsr_of=None, runs=None, link=None, manip=None, lower="limits", upper="limits",
                                margin=(0.02, 0.0), slack=2e-3, tol=1e-6, mu=1e-8, step_cap=0.5, push_cap=0.2, max_steps=40):
        """Project configurations onto task space regions and out of contact at once, on the device
        (orc_batch_project_tsr_clear; the rule is project_clear.project_clear): a task step plus the push-out step in the null
        space of the TSR's Jacobian.  tsrs, configs, tsr_of, link, manip, lower, upper, tol, mu and step_cap as in
        batch_project_tsr; runs, margin and slack as in batch_push_out; push_cap: the longest push of a step.  Returns a dict:
        configs [n_q][n], the best iterate of every row (on its TSR and clear; else on its TSR, of smallest penetration cost;
        else of smallest residual); resid [n_q] and clearance [n_q][2] of that iterate; steps int32 [n_q]; status int32 [n_q]:
        0 on the TSR and clear, 1 a singular system or a step that moves nothing, 2 out of steps, 3 a row with a non-finite
        entry."""
        rec, _ = self._tsr_records(bid, tsrs, link, manip)
        cf, tq = self._tsr_queries(bid, configs, tsr_of, len(rec))
        _, rq = self._config_queries(bid, cf, runs)
        mf, ms = self._margins(margin)
        n_q, n = cf.shape
        box = self._project_box(bid, lower, upper, n)
        rows = np.zeros((n_q, n)); resid = np.zeros(n_q); clr = np.zeros((n_q, 2))
        steps = np.zeros(n_q, dtype=np.int32); status = np.zeros(n_q, dtype=np.int32)
        self._check(self._lib.orc_batch_project_tsr_clear(self._h, bid, len(rec), rec, n_q, None if tq is None else _ip(tq),
                                                          None if rq is None else _ip(rq), _dp(cf),
                                                          None if box[0] is None else _dp(box[0]), None if box[1] is None else _dp(box[1]),
                                                          int(max_steps), float(tol), float(mu), float(step_cap), float(push_cap), mf, ms,
                                                          float(slack), _dp(rows), _dp(resid), _dp(clr), _ip(steps), _ip(status)))
        return dict(configs=rows, resid=resid, clearance=clr, steps=steps, status=status)

    def batch_project_state(self, bid):
        """where a lane's state of the projection kernel lives for this batch: (TSRs of up to 3 enforced rows, of up to 6), each
        "lds" or "global"; a row's answer does not depend on it"""
        out = np.zeros(2)
        self._check(self._lib.orc_batch_get_state(self._h, bid, b"project_state", _dp(out), out.size))
        return tuple("lds" if v else "global" for v in out)

    def batch_select_clear(self, bid, groups=None, n_groups=None, margin=0.0, by="total", max_samples=65536):
        """The best run of every group among the candidates that keep `margin` metres of clearance, on the device
        (orc_batch_select_clear; the rule is select_clear's).  by: "total", "obs", "smooth" (the cost that is minimised) or
        "clearance" (the largest clearance wins; the cost returned is -clearance).  groups and n_groups as in
        batch_select_best.  Returns (best_run int32 [n_groups], -1 for a group without an eligible run; best_cost [n_groups],
        +inf there; best_clearance [n_groups], NaN there; n_eligible int32 [n_groups]; n_samples int32 [n_runs], as
        batch_clearance(runs="candidates") reports it)."""
        if by not in ("total", "obs", "smooth", "clearance"):
            raise ValueError('by is "total", "obs", "smooth" or "clearance"')
        n_runs = self.batch_dims(bid)[0]
        gp = None
        if groups is not None:
            gp = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
            if gp.size != n_runs:
                raise ValueError("groups has %d entries for %d runs" % (gp.size, n_runs))
            if n_groups is None:
                n_groups = int(gp.max()) + 1
        elif n_groups is None:
            n_groups = 1
        n_groups = int(n_groups)
        size = max(n_groups, 1)
        best = np.zeros(size, dtype=np.int32); cost = np.zeros(size); clr = np.zeros(size); cnt = np.zeros(size, dtype=np.int32)
        ns = np.zeros(n_runs, dtype=np.int32)
        self._check(self._lib.orc_batch_select_clear(self._h, bid, ("total", "obs", "smooth", "clearance").index(by), n_groups,
                                                     None if gp is None else _ip(gp), float(margin), int(max_samples),
                                                     _ip(best), _dp(cost), _dp(clr), _ip(cnt), _ip(ns)))
        return best[:n_groups], cost[:n_groups], clr[:n_groups], cnt[:n_groups], ns

    def batch_plan(self, bid):
        """what the planner chose for this batch (orc_batch_get_state "plan")"""
        out = np.zeros(9)
        self._check(self._lib.orc_batch_get_state(self._h, bid, b"plan", _dp(out), out.size))
        keys = ("variant", "threads", "lds_bytes", "tile_m", "solve_mode", "workgroups_per_cu", "tiles", "lanes_per_waypoint",
                "tile_first")
        return {k: int(v) for k, v in zip(keys, out)}

    def batch_tsr_plan(self, bid):
        """which form of the constraint step this batch runs (orc_batch_get_state "tsr_plan"; csrc/tsr_form.h): n_tsrs, cons_k,
        structured, n_max, then width (16 or 32 lanes per row of the register form, 0 the one-wavefront LDS form, -1 the dense
        step), regs, aug, meet (tsr_meet_regs<2>, <4>; 0 tsr_meet), subst (tsr_substitute's two template numbers) and m, the moving
        waypoints"""
        out = np.zeros(11)
        self._check(self._lib.orc_batch_get_state(self._h, bid, b"tsr_plan", _dp(out), out.size))
        v = [int(x) for x in out]
        return dict(n_tsrs=v[0], cons_k=v[1], structured=v[2], n_max=v[3], width=v[4], regs=v[5], aug=v[6], meet=v[7], subst=(v[8], v[9]), m=v[10])

    def batch_state(self, bid, which):
        """"G", "AG", "T": [n_runs][m][n] (m moving waypoints: n_points - 2, n_points - 1 with start_tsr); "run_params": [n_runs][4] lambda, epsilon, obs_factor, obs_factor_self as the
        device holds them (run_params_table)"""
        n_runs, n_points, n = self.batch_dims(bid)
        out = np.zeros((n_runs, 4)) if which == "run_params" else np.zeros((n_runs, self.batch_tsr_plan(bid)["m"], n))
        self._check(self._lib.orc_batch_get_state(self._h, bid, which.encode(), _dp(out), out.size))
        return out

    def batch_destroy(self, bid):
        self._check(self._lib.orc_batch_destroy(self._h, bid))
        self._batch_robot.pop(bid, None)

    def kernel_time(self, reset=False):
        ms = C.c_double(); n = C.c_int()
        self._check(self._lib.orc_kernel_time(self._h, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value
