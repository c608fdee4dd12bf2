"""Projecting configurations onto a task space region and out of contact at once: the step rule and the loop around a TSR
evaluation and a penetration evaluation.

The two evaluations are stateless: evaluate_tsr as project.project takes it (per row the k enforced entries h of the TSR's xyzrpy
value and their Jacobian rows J), evaluate_pen as pushout.push_out takes it (per row the penetration cost U = U_field + U_self at
a pair of margins, its gradient g and the two clearances).  A step is the task step of project.py plus the push-out step of
pushout.py projected into the null space of J, its length taken from the projected gradient.  The device runs the same rule, one
round per pair of launches (Module.batch_project_tsr_clear, csrc/project_clear_kernels.hip); this file is its specification.
Everything here is numpy on the host and runs without a GPU.

The order of every sum, which the kernel follows (c a column 0 .. n-1, i and p rows 0 .. K-1, rows from k on carried as the
identity: A[i][i] = 1, h[i] = 0, J[i] = 0):
  A[i][j]  = sum over c ascending of J[i][c] J[j][c], then + mu on the diagonal
  L        by rows i, within a row j = 0 .. i: s = A[i][j] - L[i][0] L[j][0] - ... - L[i][j-1] L[j][j-1]
  A^-1 b   L z = b by rows ascending (s = b[i] - L[i][0] z[0] - ...), then L^T y = z by rows descending (s = z[i] - L[i+1][i] y[i+1] - ...)
  dq[c]    = -(J[0][c] y[0] + ... + J[K-1][c] y[K-1]) with y = A^-1 h
  w[i]     = sum over c ascending of J[i][c] g[c];  z = A^-1 w
  g_N[c]   = g[c] - (J[0][c] z[0] + ... + J[K-1][c] z[K-1]);  s = sum over c ascending of g_N[c]^2
  p[c]     = -(((2 U) / s) g_N[c]);  |p|^2 = sum over c ascending of p[c]^2;  p <- p (push_cap / |p|) where |p| > push_cap
  dq      <- dq + p;  |dq|^2 = sum over c ascending;  new[c] = cur[c] + dq[c] scale, scale = step_cap / |dq| where |dq| > step_cap, else 1
  U        = cost[0] + cost[1]"""
import numpy as np

from .project import DONE, STALLED, OUT_OF_STEPS, NOT_FINITE, residual      # noqa: F401  (the statuses are project.py's)

ON_AND_CLEAR, ON, OFF = 0, 1, 2      # the classes of an iterate's key


def key_of(r, U, clr, tol, margin):
    """(class [q], value [q]) of iterates with residual r, cost U and clearance clr [q][2]: class 0 on the TSR (r <= tol) and
    clear (clr >= margin on both legs; a NaN is never clear), value 0; class 1 on the TSR, value U; class 2 everything else,
    value r"""
    r = np.asarray(r); U = np.asarray(U)
    clr = np.asarray(clr, dtype=np.float64).reshape(-1, 2)
    margin = np.asarray(margin, dtype=np.float64).reshape(2)
    with np.errstate(invalid="ignore"):
        on = r <= tol
        clear = (clr[:, 0] >= margin[0]) & (clr[:, 1] >= margin[1])
    cls = np.where(on & clear, ON_AND_CLEAR, np.where(on, ON, OFF)).astype(np.int32)
    val = np.where(cls == ON_AND_CLEAR, np.zeros_like(r), np.where(cls == ON, U.astype(r.dtype), r))
    return cls, val


def key_better(cls, val, best_cls, best_val):
    """bool [q]: the key (cls, val) is better than (best_cls, best_val).  The lower class wins; within a class the smaller value
    wins, a NaN is never better and anything beats a NaN; a tie is not better (the earlier iterate keeps it)"""
    cls = np.asarray(cls); best_cls = np.asarray(best_cls)
    val = np.asarray(val); best_val = np.asarray(best_val)
    with np.errstate(invalid="ignore"):
        return (cls < best_cls) | ((cls == best_cls) & ~np.isnan(val) & ~(best_val <= val))


def _box(side, outwards, dtype):
    """a limit in dtype; one that dtype rounds outwards is taken one step inwards (project.py: a clipped row lies inside the box)"""
    if side is None:
        return None
    x = np.asarray(side, dtype=dtype)
    given = np.asarray(side, dtype=np.float64)
    if outwards < 0:
        return np.where(x.astype(np.float64) < given, np.nextafter(x, dtype(np.inf)), x)
    return np.where(x.astype(np.float64) > given, np.nextafter(x, dtype(-np.inf)), x)


def _solve(L, b, K):
    """y = (L L^T)^-1 b, in the order of the docstring"""
    y = np.zeros_like(b)
    for i in range(K):                                         # L z = b
        s = b[:, i].copy()
        for p in range(i):
            s -= L[:, i, p] * y[:, p]
        y[:, i] = s / L[:, i, i]
    for i in range(K - 1, -1, -1):                             # L^T y = z
        s = y[:, i].copy()
        for p in range(i + 1, K):
            s -= L[:, p, i] * y[:, p]
        y[:, i] = s / L[:, i, i]
    return y


def clear_step(rows, h, J, cost, grad, lower=None, upper=None, mu=1e-8, step_cap=0.5, push_cap=0.2, k=None, dtype=np.float64,
               detail=None):
    """One step of every row: the task step dq = -J^T A^-1 h with A = J J^T + mu I_k (project.project_step's), plus, where
    U = cost[0] + cost[1] is finite and positive and g = grad is finite, the push p = -(2U / s) g_N with g_N = g - J^T A^-1 (J g)
    and s = g_N . g_N (where s is finite and positive), shortened to push_cap in the 2-norm; dq + p is shortened to step_cap, then
    rows <- clip(rows + dq, lower, upper).

    rows [q][n], h [q][K], J [q][K][n], cost [q][2] (or U [q]), grad [q][n]; k as in project_step.  The arithmetic is done in
    dtype, every sum in the order of the module's docstring.  Returns (new rows [q][n], ok [q], moved [q]) as project_step does.
    detail: a dict that receives dq_task, push [q][n] (zero where there was none), pushed [q], y and z [q][K]."""
    rows = np.array(rows, dtype=dtype, ndmin=2)
    q, n = rows.shape
    h = np.asarray(h, dtype=dtype).reshape(q, -1)
    K = h.shape[1]
    J = np.asarray(J, dtype=dtype).reshape(q, K, n)
    kk = np.full(q, K) if k is None else np.broadcast_to(np.asarray(k), (q,))
    on = np.arange(K)[None, :] < kk[:, None]                      # [q][K]
    J = np.where(on[:, :, None], J, dtype(0))
    h = np.where(on, h, dtype(0))
    cost = np.asarray(cost, dtype=dtype)
    with np.errstate(all="ignore"):
        U = cost[:, 0] + cost[:, 1] if cost.ndim == 2 else cost.reshape(q)
    g = np.asarray(grad, dtype=dtype).reshape(q, n)
    mu, step_cap, push_cap = dtype(mu), dtype(step_cap), dtype(push_cap)
    A = np.zeros((q, K, K), dtype=dtype)
    with np.errstate(all="ignore"):
        for c in range(n):
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
        y = _solve(L, h, K)
        dq = np.zeros((q, n), dtype=dtype)
        for i in range(K):
            dq += J[:, i, :] * y[:, i, None]
        dq = -dq
        # the push, in the null space of J (up to the damping: J g_N = mu A^-1 J g)
        pushed = np.isfinite(U) & (U > 0) & np.isfinite(g).all(axis=1)
        gs = np.where(pushed[:, None], g, dtype(0))
        w = np.zeros((q, K), dtype=dtype)
        for c in range(n):
            w += J[:, :, c] * gs[:, c, None]
        z = _solve(L, w, K)
        t = np.zeros((q, n), dtype=dtype)
        for i in range(K):
            t += J[:, i, :] * z[:, i, None]
        gN = gs - t
        s = np.zeros(q, dtype=dtype)
        for c in range(n):
            s += gN[:, c] * gN[:, c]
        pushed &= np.isfinite(s) & (s > 0)
        coef = (dtype(2) * np.where(pushed, U, dtype(0))) / np.where(pushed, s, dtype(1))
        p = -(coef[:, None] * gN)
        pp = np.zeros(q, dtype=dtype)
        for c in range(n):
            pp += p[:, c] * p[:, c]
        plen = np.sqrt(pp)
        long = pushed & (plen > push_cap)
        p = p * np.where(long, push_cap / np.where(long, plen, dtype(1)), dtype(1))[:, None]
        p = np.where(pushed[:, None], p, dtype(0))
        if detail is not None:
            detail.update(dq_task=dq.copy(), push=p.copy(), pushed=pushed.copy(), y=y.copy(), z=z.copy())
        dq = np.where(pushed[:, None], dq + p, dq)
        nn = np.zeros(q, dtype=dtype)
        for c in range(n):
            nn += dq[:, c] * dq[:, c]
        length = np.sqrt(nn)
        scale = np.where(length > step_cap, step_cap / np.where(length > step_cap, length, dtype(1)), dtype(1))
        new = rows + dq * scale[:, None]
        lo, hi = _box(lower, -1, dtype), _box(upper, +1, dtype)
        if lo is not None:
            new = np.where(new < lo, lo, new)
        if hi is not None:
            new = np.where(new > hi, hi, new)
        new = np.where(ok[:, None], new, rows)
        moved = (new != rows).any(axis=1)
    return new, ok, moved


def project_clear(evaluate_tsr, evaluate_pen, rows, lower=None, upper=None, margin=(0.02, 0.0), slack=2e-3, tol=1e-6, mu=1e-8,
                  step_cap=0.5, push_cap=0.2, max_steps=40, k=None, indexed=False, dtype=np.float64, history=None):
    """Move every row of rows [n_q][n] onto its TSR and out of contact: r = max_i |h_i| <= tol and clearance >= margin on both
    legs (fields, self).

    evaluate_tsr(rows) -> (h [q][K], J [q][K][n]) and evaluate_pen(rows, margin) -> dict with cost [q][2], grad [q][n],
    clearance [q][2], of the q rows they are given -- only the rows still active (indexed: both also get their positions in the
    input).  evaluate_pen is called with margin + slack, so that a step that lands on the cost's zero set is clear of `margin`
    proper.  k as in project_step.

    Per row and round it = 0 .. max_steps: the key of the iterate is (class, value) as key_of has it, and the best iterate by
    key_better is kept.  On the TSR and clear: status 0, stop.  it == max_steps: status 2, stop.  Else one clear_step.  Status 1:
    a pivot that is not positive and finite, or a step that moves no entry.  Status 3: a row with a non-finite entry (its
    outputs are NaN, its steps 0).

    Returns (rows [n_q][n], resid [n_q], clearance [n_q][2], steps [n_q], status [n_q]): the best iterate, its r and its
    clearance.  A row that starts on its TSR and clear, and every row when max_steps is 0, comes back bit for bit, and so does
    every entry the loop left where it was.  history: a list that receives (index, iterates, r, U, clearance) of every round."""
    given = np.array(rows, dtype=np.float64, ndmin=2)
    n_q = len(given)
    margin = np.asarray(margin, dtype=np.float64).reshape(2)
    at = tuple(margin + slack)
    kq = None if k is None else np.broadcast_to(np.asarray(k), (n_q,))
    out = given.copy()
    resid = np.full(n_q, np.nan)
    clearance = np.full((n_q, 2), np.nan)
    steps = np.zeros(n_q, dtype=np.int32)
    status = np.full(n_q, OUT_OF_STEPS, dtype=np.int32)
    finite = np.isfinite(given).all(axis=1)
    status[~finite] = NOT_FINITE
    out[~finite] = np.nan
    cur = given.astype(dtype)
    best_cls = np.full(n_q, OFF, dtype=np.int32)
    best_val = np.full(n_q, np.nan, dtype=dtype)
    best_r = np.full(n_q, np.nan)
    active = np.flatnonzero(finite)
    for it in range(int(max_steps) + 1):
        if not len(active):
            break
        m = len(active)
        pen = evaluate_pen(cur[active], at, active) if indexed else evaluate_pen(cur[active], at)
        cost = np.asarray(pen["cost"], dtype=dtype).reshape(m, 2)
        grad = np.asarray(pen["grad"], dtype=dtype).reshape(m, -1)
        clr = np.asarray(pen["clearance"], dtype=np.float64).reshape(m, 2)
        with np.errstate(all="ignore"):
            U = cost[:, 0] + cost[:, 1]
        h, J = evaluate_tsr(cur[active], active) if indexed else evaluate_tsr(cur[active])
        h = np.asarray(h, dtype=dtype).reshape(m, -1)
        ka = None if kq is None else kq[active]
        r = residual(h, ka).astype(dtype)
        if history is not None:
            history.append((active.copy(), cur[active].copy(), r.copy(), U.copy(), clr.copy()))
        cls, val = key_of(r, U, clr, dtype(tol), margin)
        better = np.full(m, True) if it == 0 else key_better(cls, val, best_cls[active], best_val[active])
        if it > 0:
            out[active[better]] = cur[active[better]]
        best_cls[active[better]] = cls[better]
        best_val[active[better]] = val[better]
        best_r[active[better]] = r[better]
        clearance[active[better]] = clr[better]
        done = cls == ON_AND_CLEAR
        status[active[done]] = DONE
        if it == max_steps:
            break
        go = ~done
        if not go.any():
            break
        new, ok, moved = clear_step(cur[active[go]], h[go], np.asarray(J)[go], cost[go], grad[go], lower, upper, mu, step_cap, push_cap,
                                    None if ka is None else ka[go], dtype)
        stepped = ok & moved
        status[active[go][~stepped]] = STALLED
        cur[active[go][stepped]] = new[stepped]
        steps[active[go][stepped]] += 1
        active = active[go][stepped]
    resid[finite] = best_r[finite]
    # an entry the loop left where it was (in dtype) is the caller's own double
    with np.errstate(invalid="ignore"):
        out = np.where(out.astype(dtype) == given.astype(dtype), given, out)
    return out, resid, clearance, steps, status
