"""The plan of the headline workload (BASELINE configs[1]: the WAM, 100 waypoints, fp64, launches that overlap) and its tiling.

98 moving waypoints at 16 lanes per waypoint and 256 threads: a cost round of the workgroup covers 16 waypoints. Tiles of
50 + 48 take 4 + 3 = 7 rounds per iteration; the 49 + 49 of the earlier carve-up took 4 + 4, the fourth round of each tile
being one wavefront with one waypoint. The tiling changes which lanes evaluate a waypoint, not its arithmetic: the
trajectories equal those of a run forced to tiles of 49 (ORC_TILE_M) bit for bit."""
import numpy as np
import pytest

import common
import or_cdchomp_amd

pytestmark = pytest.mark.gpu


def _run(mod, model, goals, n_iter):
    bid = mod.batch_create(model.name, goals, **common.CONFIG2_KW)
    costs, status = mod.batch_iterate(bid, n_iter)
    out = dict(costs=costs, status=status, traj=mod.batch_gettraj(bid), plan=mod.batch_plan(bid))
    mod.batch_destroy(bid)
    return out


def test_headline_plan_takes_whole_cost_rounds(monkeypatch):
    if common.plan_switches_active():
        pytest.skip("an experiment switch is set: the planner's own choice is what this test reads")
    mod = or_cdchomp_amd.Module(0)
    model = common.setup_product_wam(mod)
    mod.set_num_streams(2)          # (bench.py's overlapping leg: four workgroups per CU)
    goals = common.wam_goals(64)
    new = _run(mod, model, goals, 30)
    plan = new["plan"]
    assert plan["threads"] == 256 and plan["workgroups_per_cu"] == 4 and plan["lanes_per_waypoint"] == 16, plan
    assert plan["lds_bytes"] <= 40960, plan
    assert plan["tiles"] == 2 and plan["tile_m"] == 50, plan
    first = plan["tile_first"]
    sizes = [first, 98 - first]
    assert max(sizes) <= plan["tile_m"] and sum(-(-s // 16) for s in sizes) == 7, (plan, sizes)

    monkeypatch.setenv("ORC_TILE_M", "49")
    old = _run(mod, model, goals, 30)
    monkeypatch.delenv("ORC_TILE_M")
    assert old["plan"]["tile_m"] == 49 and old["plan"]["tiles"] == 2, old["plan"]

    assert (new["status"] == 0).all() and (old["status"] == 0).all()
    assert np.array_equal(new["traj"], old["traj"])
    # (the obstacle cost is summed over lanes: another tiling sums it in another order)
    assert np.allclose(new["costs"], old["costs"], rtol=1e-12, atol=0)
