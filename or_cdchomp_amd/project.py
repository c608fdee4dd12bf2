"""Projecting configurations onto a task space region: the step rule and the loop around a TSR evaluation.

The evaluation is stateless (Module.batch_config_tsr on the device, the oracle's eval_contsr, or any function of the same
shape): per row the k enforced entries h of the TSR's xyzrpy value and their Jacobian rows J.  The device runs the same rule in
one kernel (Module.batch_project_tsr, csrc/project_kernels.hip); this file is its specification.  Everything here is numpy on
the host and runs without a GPU."""
import numpy as np

DONE, STALLED, OUT_OF_STEPS, NOT_FINITE = 0, 1, 2, 3


def residual(h, k=None):
    """r = max_i |h_i| over a row's k enforced entries (all of them when k is None); a NaN entry makes it NaN"""
    h = np.abs(np.asarray(h))
    if h.ndim == 1:
        h = h[None, :]
    if k is not None:
        h = np.where(np.arange(h.shape[1])[None, :] < np.asarray(k).reshape(-1, 1), h, 0.0)
    return np.where(np.isnan(h).any(axis=1), np.nan, h.max(axis=1, initial=0.0))


def project_step(rows, h, J, lower=None, upper=None, mu=1e-8, step_cap=0.5, k=None, dtype=np.float64):
    """One step of every row: solve (J J^T + mu I_k) y = h by Cholesky in the order of the rows, dq = -J^T y, shorten dq to
    step_cap in the 2-norm, rows <- clip(rows + dq, lower, upper).

    rows [q][n], h [q][K], J [q][K][n]; k [q] (or an int, or None for K): the enforced entries of a row -- entries from k on
    are carried as the identity (A[i][i] = 1, h[i] = 0), which leaves their y at zero and the k x k system as it is.  The
    arithmetic is done in dtype.  Returns (new rows [q][n], ok [q], moved [q]): ok False where a pivot was not positive and
    finite (the row is returned as it was); moved False where no entry changed."""
    rows = np.array(rows, dtype=dtype, ndmin=2)
    q, n = rows.shape
    h = np.asarray(h, dtype=dtype).reshape(q, -1)
    K = h.shape[1]
    J = np.asarray(J, dtype=dtype).reshape(q, K, n)
    kk = np.full(q, K) if k is None else np.broadcast_to(np.asarray(k), (q,))
    on = np.arange(K)[None, :] < kk[:, None]                      # [q][K]
    J = np.where(on[:, :, None], J, dtype(0))
    h = np.where(on, h, dtype(0))
    mu, step_cap = dtype(mu), dtype(step_cap)
    A = np.zeros((q, K, K), dtype=dtype)
    with np.errstate(all="ignore"):
        for c in range(n):                                         # every sum in the order of the columns
            A += J[:, :, None, c] * J[:, None, :, c]
    for i in range(K):
        A[:, i, i] = np.where(on[:, i], A[:, i, i] + mu, dtype(1))
    L = np.zeros((q, K, K), dtype=dtype)
    ok = np.ones(q, dtype=bool)
    with np.errstate(all="ignore"):
        for i in range(K):
            for j in range(i + 1):
                s = A[:, i, j].copy()
                for p in range(j):
                    s -= L[:, i, p] * L[:, j, p]
                if j == i:
                    good = (s > 0) & (s < np.inf)
                    ok &= good
                    L[:, i, i] = np.sqrt(np.where(good, s, dtype(1)))
                else:
                    L[:, i, j] = s / L[:, j, j]
        y = np.zeros((q, K), dtype=dtype)
        for i in range(K):                                         # L z = h
            s = h[:, i].copy()
            for p in range(i):
                s -= L[:, i, p] * y[:, p]
            y[:, i] = s / L[:, i, i]
        for i in range(K - 1, -1, -1):                             # L^T y = z
            s = y[:, i].copy()
            for p in range(i + 1, K):
                s -= L[:, p, i] * y[:, p]
            y[:, i] = s / L[:, i, i]
        dq = np.zeros((q, n), dtype=dtype)
        for i in range(K):
            dq += J[:, i, :] * y[:, i, None]
        dq = -dq
        nn = np.zeros(q, dtype=dtype)
        for c in range(n):
            nn += dq[:, c] * dq[:, c]
        length = np.sqrt(nn)
        scale = np.where(length > step_cap, step_cap / np.where(length > step_cap, length, dtype(1)), dtype(1))
        new = rows + dq * scale[:, None]
        # (a limit that dtype rounds outwards is taken one step inwards: a clipped row lies inside the caller's box)
        if lower is not None:
            lo = np.asarray(lower, dtype=dtype)
            lo = np.where(lo.astype(np.float64) < np.asarray(lower, dtype=np.float64), np.nextafter(lo, dtype(np.inf)), lo)
            new = np.where(new < lo, lo, new)
        if upper is not None:
            hi = np.asarray(upper, dtype=dtype)
            hi = np.where(hi.astype(np.float64) > np.asarray(upper, dtype=np.float64), np.nextafter(hi, dtype(-np.inf)), hi)
            new = np.where(new > hi, hi, new)
        new = np.where(ok[:, None], new, rows)
        moved = (new != rows).any(axis=1)
    return new, ok, moved


def project(evaluate, rows, lower=None, upper=None, tol=1e-6, mu=1e-8, step_cap=0.5, max_steps=30, k=None, indexed=False,
            dtype=np.float64, history=None):
    """Project every row of rows [n_q][n] onto its TSR.

    evaluate(rows) -> (h [q][K], J [q][K][n]) of the q rows it is given -- only the rows still active; indexed:
    evaluate(rows, index) also gets their positions in the input, so that a row's own TSR can go with it.  k as in
    project_step.  At an iterate with r = max_i |h_i|: r <= tol ends the row with status 0; else one project_step.  Status 1:
    a pivot that is not positive and finite, or a step that moves no entry; 2: out of steps; 3: a row with a non-finite entry
    (its outputs are NaN, its steps 0).  Returns (rows [n_q][n], resid [n_q], steps [n_q], status [n_q]): a row that is not
    done comes back as the visited iterate of smallest r, never worse than the input; a row that starts within tol, and every
    row when max_steps is 0, comes back bit for bit, and so does every entry a projection did not move.  history: a list that receives (index, iterates, r) of every round."""
    given = np.array(rows, dtype=np.float64, ndmin=2)
    n_q = len(given)
    kq = None if k is None else np.broadcast_to(np.asarray(k), (n_q,))
    out = given.copy()
    resid = np.full(n_q, np.nan)
    steps = np.zeros(n_q, dtype=np.int32)
    status = np.full(n_q, OUT_OF_STEPS, dtype=np.int32)
    finite = np.isfinite(given).all(axis=1)
    status[~finite] = NOT_FINITE
    out[~finite] = np.nan
    cur = given.astype(dtype)
    best_r = np.full(n_q, np.nan)
    active = np.flatnonzero(finite)
    for it in range(int(max_steps) + 1):
        if not len(active):
            break
        h, J = evaluate(cur[active], active) if indexed else evaluate(cur[active])
        h = np.asarray(h, dtype=dtype).reshape(len(active), -1)
        ka = None if kq is None else kq[active]
        r = residual(h, ka).astype(dtype)
        if history is not None:
            history.append((active.copy(), cur[active].copy(), r.copy()))
        # the visited iterate of smallest r (a NaN is never better, and anything is better than a NaN)
        better = np.full(len(active), True) if it == 0 else (~np.isnan(r) & ~(best_r[active] <= r))
        if it > 0:
            out[active[better]] = cur[active[better]]
        best_r[active[better]] = r[better]
        done = r <= dtype(tol)
        status[active[done]] = DONE
        if it == max_steps:
            break
        go = ~done
        if not go.any():
            break
        new, ok, moved = project_step(cur[active[go]], h[go], np.asarray(J)[go], lower, upper, mu, step_cap,
                                      None if ka is None else ka[go], dtype)
        stepped = ok & moved
        status[active[go][~stepped]] = STALLED
        cur[active[go][stepped]] = new[stepped]
        steps[active[go][stepped]] += 1
        active = active[go][stepped]
    resid[finite] = best_r[finite]
    # an entry the projection left where it was (in dtype) is the caller's own double
    with np.errstate(invalid="ignore"):
        out = np.where(out.astype(dtype) == given.astype(dtype), given, out)
    return out, resid, steps, status
