"""Pushing configurations out of contact: the step rule and the loop around a penetration evaluation.

The evaluation is stateless (Module.batch_config_penetration on the device, or any function of the same shape): per row the
penetration cost U = U_field + U_self at a pair of margins, its gradient with respect to the row, and the two clearances.
Everything here is numpy on the host and runs without a GPU."""
import numpy as np

CLEAR, STALLED, OUT_OF_STEPS = 0, 1, 2


def push_step(rows, cost, grad, lower=None, upper=None, step_cap=0.2):
    """rows - 2 U g / (g.g) with U = cost.sum(-1): the Newton step on U = 1/2 d^2 when one item violates (it takes d to zero
    to first order).  The step is shortened to step_cap in the 2-norm, then the row is clipped to [lower, upper].  A row
    with g.g == 0 (or a cost or gradient that is not finite) does not move."""
    rows = np.asarray(rows, dtype=np.float64)
    g = np.asarray(grad, dtype=np.float64)
    U = np.asarray(cost, dtype=np.float64).sum(axis=-1)
    gg = (g * g).sum(axis=-1)
    ok = np.isfinite(gg) & (gg > 0.0) & np.isfinite(U)
    scale = np.where(ok, 2.0 * U / np.where(ok, gg, 1.0), 0.0)
    step = -scale[..., None] * np.where(ok[..., None], g, 0.0)
    length = np.sqrt((step * step).sum(axis=-1))
    shrink = np.where(length > step_cap, step_cap / np.where(length > 0.0, length, 1.0), 1.0)
    out = rows + step * shrink[..., None]
    if lower is not None:
        out = np.maximum(out, np.asarray(lower, dtype=np.float64))
    if upper is not None:
        out = np.minimum(out, np.asarray(upper, dtype=np.float64))
    return np.where(ok[..., None], out, rows)


def push_out(evaluate, rows, margin=(0.02, 0.0), slack=2e-3, max_steps=20, step_cap=0.2, lower=None, upper=None, indexed=False):
    """Move every row of rows [n_q][n] until its clearance is >= margin on both legs (fields, self).

    evaluate(rows, margin) -> dict with cost [k][2], grad [k][n], clearance [k][2] of the k rows it is given; it is called with
    margin + slack, so that a step that lands on the cost's zero set is clear of `margin` proper, and only with the rows still
    active (indexed: evaluate(rows, margin, index) also gets their positions in the input).  Returns (rows [n_q][n], steps
    [n_q], status [n_q]): 0 clear, 1 the gradient vanished while in contact, 2 out of steps.  A row that starts clear comes back bit for bit with 0 steps; a row that does not get clear comes back as the
    visited row of smallest U (never worse than the input)."""
    rows = np.array(rows, dtype=np.float64, ndmin=2)
    margin = np.asarray(margin, dtype=np.float64).reshape(2)
    n_q = len(rows)
    steps = np.zeros(n_q, dtype=np.int32)
    status = np.full(n_q, OUT_OF_STEPS, dtype=np.int32)
    best = rows.copy()
    best_u = np.full(n_q, np.inf)
    cur = rows.copy()
    active = np.arange(n_q)
    for it in range(int(max_steps) + 1):
        if not len(active):
            break
        res = evaluate(cur[active], tuple(margin + slack), active) if indexed else evaluate(cur[active], tuple(margin + slack))
        cost = np.asarray(res["cost"], dtype=np.float64).reshape(len(active), 2)
        grad = np.asarray(res["grad"], dtype=np.float64).reshape(len(active), -1)
        clr = np.asarray(res["clearance"], dtype=np.float64).reshape(len(active), 2)
        U = cost.sum(axis=-1)
        clear = (clr >= margin).all(axis=-1)
        better = clear | (U < best_u[active])          # (a NaN cost is never better)
        best[active[better]] = cur[active[better]]
        best_u[active[better]] = np.where(clear, -np.inf, U)[better]
        status[active[clear]] = CLEAR
        stalled = ~clear & ~(np.isfinite(U) & ((grad * grad).sum(axis=-1) > 0.0))
        status[active[stalled]] = STALLED
        go = ~clear & ~stalled
        if it == max_steps:
            break
        cur[active[go]] = push_step(cur[active[go]], cost[go], grad[go], lower, upper, step_cap)
        steps[active[go]] += 1
        active = active[go]
    return best, steps, status
