"""Shared inputs and the restatement of the clear-projection tests (tests/test_host_project_clear.py,
tests/test_gpu_project_clear.py).

The restatement is or_cdchomp_amd.project_clear.project_clear around the oracle's eval_contsr (project.OracleTsrs.evaluate) and
the restated penetration (penetration.restate).  The scene is common.tabletop_problem, the WAM has its default base, the link
is handbase with project.TOOL, and the TSR of a row sits at the row's own hand pose: a goal in contact is on its TSR and not
clear."""
import numpy as np

import clearance as CL
import common
import penetration as PN
import project as PJ
from or_cdchomp_amd import project_clear

PARAMS = dict(margin=(0.02, 0.0), slack=2e-3, tol=1e-6, mu=1e-8, step_cap=0.5, push_cap=0.2, max_steps=40)
CONTACT_48 = [0, 1, 2, 8, 9, 15, 17, 19, 24, 26, 31, 34, 35, 41, 43]      # the goals of common.wam_goals(48) in contact (a clearance below zero)
# the rows of the 15 that the committed rule finishes, with its steps, measured on the host (tests/test_host_project_clear.py
# asserts them): the compared rows of the device tests.  The other rows run out of steps and amplify rounding
FINISH = {"BW6": {0: 9, 14: 13}, "BW3": {0: 5, 2: 6, 3: 4, 8: 10, 10: 32, 11: 6, 12: 8, 14: 8}}
BWS = {"BW6": PJ.BW6, "BW3": PJ.BW3}
BENT = 0.05              # the bent rows: the goal plus this much of a fixed draw


def world(O):
    """the WAM on its default base over the tabletop: dict(model, base, dofvals, adofs, tab, table, shifted, lower, upper)"""
    prob = common.tabletop_problem(O)
    model, base, dofvals, adofs = common.wam_state()
    table = CL.Field(O, prob["sdf"], None, prob["pose"])
    shifted = CL.Field(O, prob["sdf"], None, PN.compose(O, PN.SHIFT, prob["pose"]))
    lo, hi = PJ.wam_limits()
    return dict(model=model, base=base, dofvals=dofvals, adofs=adofs, tab=CL.Tables(O, model, base, dofvals, adofs, [table]), table=table,
                shifted=shifted, lower=lo, upper=hi, prob=prob)


def in_contact(w, rows, margin=(0.0, 0.0), fields=None):
    """bool [len(rows)]: the restated clearance of a leg is below its margin (zero: in contact)"""
    fields = [w["table"]] if fields is None else fields
    clr = np.array([PN.restate(w["tab"], r, 0, fields, margin)["clearance"] for r in rows])
    return (clr[:, 0] < margin[0]) | (clr[:, 1] < margin[1])


def contact_rows(w):
    """the 15 goals of common.wam_goals(48) in contact"""
    return common.wam_goals(48)[CONTACT_48]


def bent_rows(w):
    """the 15 rows bent: goal + BENT * default_rng(21).standard_normal, clipped to the limits"""
    rows = contact_rows(w)
    return np.clip(rows + BENT * np.random.default_rng(21).standard_normal(rows.shape), w["lower"], w["upper"])


def tsrs_of(w, rows, Bw):
    """robots.Tsr objects at the hand poses of `rows`"""
    Rs, ds = PJ.target_frames(w["model"], w["base"], w["dofvals"], w["adofs"], "handbase", PJ.TOOL, rows)
    return PJ.tsrs_at(Rs, ds, Bw)


class Restated:
    """the restatement on one list of TSRs: tsr_of [n_q] the TSR of a row, fields_of [n_q] the list of fields a row is tested
    against (None: the table)"""

    def __init__(self, O, w, tsrs, tsr_of, fields_of=None):
        self.w = w
        self.tsr_of = np.asarray(tsr_of)
        self.ora = PJ.OracleTsrs(O, w["model"], w["base"], w["dofvals"], w["adofs"], "handbase", PJ.TOOL, tsrs, tsr_of=self.tsr_of)
        self.fields_of = [[w["table"]]] * len(self.tsr_of) if fields_of is None else fields_of
        self.k = self.ora.ks(np.arange(len(self.tsr_of)))

    def pen(self, rows, margin, index):
        res = [PN.restate(self.w["tab"], r, 0, self.fields_of[i], margin) for r, i in zip(np.atleast_2d(rows), index)]
        return {key: np.array([r[key] for r in res]) for key in ("cost", "grad", "clearance")}

    def run(self, rows, history=None, dtype=np.float64, **kw):
        """project_clear.project_clear of rows (row q with tsr_of[q] and fields_of[q]) inside the WAM's limits"""
        p = dict(PARAMS, lower=self.w["lower"], upper=self.w["upper"]); p.update(kw)
        return project_clear.project_clear(self.ora.evaluate, self.pen, rows, k=self.k, indexed=True, dtype=dtype, history=history, **p)

    def residual(self, rows):
        """the oracle's max |h| of rows, row q on tsr_of[q]"""
        h = self.ora.evaluate(rows, np.arange(len(self.tsr_of)))[0]
        return np.abs(h).max(axis=1)

    def clearance(self, rows):
        """the restated clearance [n_q][2] of rows, row q against fields_of[q]"""
        return self.pen(rows, PARAMS["margin"], np.arange(len(self.tsr_of)))["clearance"]

    def keys(self, rows, tol=PARAMS["tol"], margin=PARAMS["margin"], slack=PARAMS["slack"]):
        """(class, value) of rows as the rule keys them"""
        r = self.residual(rows)
        at = (margin[0] + slack, margin[1] + slack)
        pen = self.pen(rows, at, np.arange(len(self.tsr_of)))
        return project_clear.key_of(r, pen["cost"].sum(axis=1), pen["clearance"], tol, margin)

    def destroy(self):
        self.ora.destroy()


def decisions(history, tol=PARAMS["tol"], margin=PARAMS["margin"]):
    """per input row the closest decisions over all visited iterates: (|r - tol| / tol [n_q], |clearance - margin| [n_q], the
    smaller over the two legs; a leg without an item, clearance +inf, decides nothing)"""
    n_q = max(int(h[0].max()) for h in history) + 1
    dr = np.full(n_q, np.inf); dc = np.full(n_q, np.inf)
    for index, _, r, _, clr in history:
        dr[index] = np.minimum(dr[index], np.abs(r - tol) / tol)
        with np.errstate(invalid="ignore"):
            gap = np.abs(clr - np.asarray(margin)[None, :])
        dc[index] = np.minimum(dc[index], np.where(np.isfinite(gap), gap, np.inf).min(axis=1))
    return dr, dc


def not_worse(cls, val, cls0, val0, bound):
    """bool [n_q]: the key (cls, val) is not worse than (cls0, val0), values compared up to `bound`"""
    return (cls < cls0) | ((cls == cls0) & (val <= val0 + bound))
