"""-m gpu: one iteration of robots that exercise the canonical joint frames of the FK walk, against the oracle, near rounding.

The fold (csrc/fold.cpp canonical_rotation) turns every optimized joint's moved frame so that the joint's axis is its z, and fk.h
turns every joint about z.  What the walk writes in the world -- sphere centres, joint axes, anchors -- must be what the general
Rodrigues step wrote: the gradient G of one iteration and A^-1 G are held to the oracle at the bound tests/test_gpu_parity.py's
test_seed_and_first_gradient uses, 1e-10 relative L2 per run (costs: 1e-9 relative).  The cases (tests/fk_canonical.py): axes in general
position behind fixed rotations, a prismatic joint between them, the negative coordinate axes, a fork whose frame is saved and
loaded and a link with more than four spheres, a floating base, the WAM with a one-row `con_tsr` on wam7 (the constraint's value h
needs the link's TRUE frame) and the WAM holding a four-sphere box.

The seeds keep every sphere of the oracle's side 1e-6 clear of a switch of the field lookup and of the cost's branches
(tests/test_host_fk_canonical.py asserts it without a GPU; NOTES/fk-canonical.md has the counts)."""
import numpy as np
import pytest

import common
import fk_canonical as fc
import or_cdchomp_amd
from or_cdchomp_amd import robots

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.id)
def test_first_gradient_with_canonical_frames(oracle, monkeypatch, case):
    monkeypatch.setenv("ORC_DEBUG_STATE", "1")      # keep the gradient of the last iteration readable
    pr = fc.problem(case, oracle)
    ref = fc.reference(case, oracle)
    for counts in ref["counts"]:
        assert counts["face"] == 0 and counts["zero"] == 0 and counts["eps"] == 0, (case.id, counts)
    mod = or_cdchomp_amd.Module(0)
    try:
        name = fc.setup_product(case, mod, oracle)
        if case.tsr:
            li, R, t = fc.tsr_frame(pr, oracle)
            tsr = robots.Tsr(T0w_R=R, T0w_d=t, Bw=fc.TSR_BW)
            bid = int(mod.SendCommand("createbatch robot %s n_runs %d adofgoals 0x%x n_points %d lambda %.17g obs_factor %.17g con_tsr 'all link %s' '%s'"
                                      % (name, case.n_runs, pr["goals"].ctypes.data, case.n_points, pr["kw"]["lambda_"], pr["kw"]["obs_factor"],
                                         fc.TSR_LINK, tsr.serialize())))
        else:
            bid = mod.batch_create(name, pr["goals"], basegoals=pr["basegoals"], n_points=case.n_points, **pr["kw"])
        assert np.array_equal(mod.batch_gettraj(bid), ref["T0"]), "the seed trajectories must be bit-exact"
        if case.tsr:
            rows = ref["T0"].reshape(-1, ref["T0"].shape[2])
            h = mod.batch_config_tsr(bid, tsr, rows, link=fc.TSR_LINK)["h"][:, :1].reshape(case.n_runs, case.n_points, 1)
        costs, status = mod.batch_iterate(bid, 1)
        G, AG, trace = mod.batch_state(bid, "G"), mod.batch_state(bid, "AG"), mod.batch_trace(bid, 1)[:, 0]
        plan = mod.batch_plan(bid)
        mod.batch_destroy(bid)
    finally:
        mod.close()
    assert (status == 0).all()
    worst = dict(G=0.0, AG=0.0, cost=0.0, h=0.0)
    for k in range(case.n_runs):
        assert np.abs(ref["G"][k]).max() > fc.G_FLOOR
        worst["G"] = max(worst["G"], common.rel_l2(G[k], ref["G"][k])); worst["AG"] = max(worst["AG"], common.rel_l2(AG[k], ref["AG"][k]))
        worst["cost"] = max(worst["cost"], float(np.abs(trace[k] / ref["trace"][k] - 1.0)[ref["trace"][k] != 0.0].max()))
        if case.tsr:
            assert np.abs(ref["h"][k][1:-1]).max() > 1e-3      # (the straight line leaves the constraint: h is no rounding noise)
            worst["h"] = max(worst["h"], common.rel_l2(h[k], ref["h"][k]))
    print("%s (%d threads, variant %s): rel L2 of G %.2e, of AG %.2e; costs %.2e%s" % (
        case.id, plan["threads"], plan.get("variant"), worst["G"], worst["AG"], worst["cost"], "; h %.2e" % worst["h"] if case.tsr else ""))
    assert worst["G"] < TOL and worst["AG"] < TOL, (case.id, worst)
    assert worst["cost"] < 1e-9, (case.id, worst)
    if case.tsr:
        assert worst["h"] < TOL, (case.id, worst)
