"""-m gpu: the GSL streams that hmc_plan_kernel draws one wavefront per run (csrc/mt_wave.h) held to the stream itself.

With lambda_ = 1e300 (1e30 in fp32) AG after an iterate call is the last noise block that the call, or an earlier one, drew,
and the trajectory stays the seed (tests/hmc_stream.py, NOTES/hmc-stream.md; the premise is asserted on the oracle in
tests/test_host_hmc_stream.py).  After every call batch_state(bid, "AG") is compared per run with the long-double reference
made from the stream's words -- 8 ulp in fp64, float32(reference) exactly in fp32 -- and with the oracle's AG under the same
bound; the status is 0 and the trajectory bit-equal to the one before the call.  A resample drawn one iteration off has a sigma
1 % off, one that was not drawn leaves an older block, and a stream one word off gives other values altogether."""
import numpy as np
import pytest

import common
import hmc_stream as H

pytestmark = pytest.mark.gpu


def _module(devices=0):
    import or_cdchomp_amd
    mod = or_cdchomp_amd.Module(devices)
    model = common.setup_product_wam(mod)
    return mod, model


def _iterate_command(mod, bid, n_iter, n_runs):
    """iteratebatch ... max_time: one launch per iteration, iter_begin is not 0 from the second on"""
    costs = np.zeros((n_runs, 3)); status = np.zeros(n_runs, dtype=np.int32)
    mod.SendCommand("iteratebatch run %d n_iter %d max_time 1e9 costs 0x%x status 0x%x" % (bid, n_iter, costs.ctypes.data, status.ctypes.data))
    return costs, status


def run_case(oracle, c, devices=0, by_command=False):
    """the case on the product: every check of the module docstring after every call; returns AG after each call"""
    ref = H.reference_ag(oracle, c)
    ora = H.oracle_case(oracle, c)
    mod, model = _module(devices)
    goals, basegoals = H.case_goals(c)
    bid = mod.batch_create(model.name, goals, basegoals=basegoals, seeds=None if c["seeds"] is None else np.asarray(c["seeds"], dtype=np.uint32),
                           precision=c["precision"], **H.case_kw(c))
    assert mod.batch_dims(bid) == (c["n_runs"], c["n_points"], H.case_n(c))
    out = []
    worst_ref = worst_ora = 0.0
    for q, n_iter in enumerate(c["calls"]):
        before = mod.batch_gettraj(bid)
        if by_command:
            costs, status = _iterate_command(mod, bid, n_iter, c["n_runs"])
        else:
            costs, status = mod.batch_iterate(bid, n_iter)
        assert (status == 0).all(), status
        got = mod.batch_state(bid, "AG").reshape(c["n_runs"], -1)
        if not c["floating"]:
            assert np.array_equal(mod.batch_gettraj(bid), before), "the trajectory moved"
        for k in range(c["n_runs"]):
            if c["precision"] == 64:
                e_ref = H.ulp_error(got[k], ref[q][k]).max()
                e_ora = H.ulp_error(got[k], ora["ag"][q, k].astype(H.LD)).max()
                worst_ref, worst_ora = max(worst_ref, e_ref), max(worst_ora, e_ora)
                assert e_ref <= H.ULP_BOUND, (c["name"], "call", q, "run", k, e_ref)
                assert e_ora <= H.ULP_BOUND, (c["name"], "call", q, "run", k, e_ora)
            else:
                want = ref[q][k].astype(np.float32).astype(np.float64)
                bad = np.flatnonzero(got[k] != want)
                assert bad.size == 0, (c["name"], "call", q, "run", k, bad[:4], got[k][bad[:4]], want[bad[:4]])
                assert np.array_equal(got[k], ora["ag"][q, k].astype(np.float32).astype(np.float64))
        out.append(got)
    mod.batch_destroy(bid)
    mod.close()
    if c["precision"] == 64:
        print("%s: worst distance of the device's AG from the long-double reference %.2f ulp, from the oracle's AG %.2f ulp"
              % (c["name"], worst_ref, worst_ora))
    else:
        print("%s: every entry is float32(reference)" % c["name"])
    return out


@pytest.fixture
def device_streams(monkeypatch):
    monkeypatch.setenv("ORC_HMC_DEVICE", "1")


@pytest.mark.parametrize("name", ["first_block", "first_block_no_seeds"])
def test_first_block(oracle, device_streams, name):
    """210 values from a fresh stream, 9 runs (the last workgroup has one wavefront): seeds 0 and 4357 are one stream, two seeds
    hold a zero word inside the block (the chunk's one-at-a-time walk), and without seeds every run draws seed 0's"""
    got = run_case(oracle, H.CASE[name])[0]
    assert np.array_equal(got[0], got[1])
    if name == "first_block_no_seeds":
        assert all(np.array_equal(got[0], g) for g in got)
    else:
        assert not np.array_equal(got[0], got[2])


@pytest.fixture(scope="module")
def plan_stream_bits():
    """AG after each call of the every-iteration case on the plan stream, for the other planners to equal"""
    return {}


@pytest.mark.parametrize("name", ["every_iteration", "every_iteration_fp32"])
def test_every_iteration(oracle, device_streams, plan_stream_bits, name):
    """a resample in every iteration, calls of 12 and 20: the second resamples from iteration 12 on only"""
    plan_stream_bits[name] = run_case(oracle, H.CASE[name])


@pytest.mark.parametrize("name", ["sparse_0.3", "sparse_0.05"])
def test_sparse(oracle, device_streams, name):
    """calls of 1, 15 and 40 iterations at hmc_resample_lambda 0.3 and 0.05: the schedule from the uniforms"""
    run_case(oracle, H.CASE[name])


@pytest.mark.parametrize("name", ["length_7", "length_238", "length_245", "length_252", "length_686"])
def test_lengths(oracle, device_streams, name):
    """values per block around the ~245 Gaussians of one state and across three twists; six blocks, begun at both word parities"""
    run_case(oracle, H.CASE[name])


@pytest.mark.parametrize("planner", ["sync_retry", "command", "two_shards"])
def test_planners(oracle, device_streams, plan_stream_bits, monkeypatch, planner):
    """the every-iteration case through the synchronous plan whose retry restores the generators (a first room of 1), through
    iteratebatch ... max_time (one launch per iteration: iter_begin is not 0), and on a module of two shards: the reference's
    values and the plan stream's bits"""
    c = H.CASE["every_iteration"]
    if "every_iteration" not in plan_stream_bits:
        plan_stream_bits["every_iteration"] = run_case(oracle, c)
    if planner == "sync_retry":
        monkeypatch.setenv("ORC_HMC_PLAN_SYNC", "1")
        monkeypatch.setenv("ORC_HMC_ROOM", "1")
    got = run_case(oracle, c, devices=[0, 0] if planner == "two_shards" else 0, by_command=(planner == "command"))
    for a, b in zip(got, plan_stream_bits["every_iteration"]):
        assert np.array_equal(a, b)


def test_default_trigger(oracle):
    """260 runs and no switch of this file's: the device streams are what a batch of 256 runs and more gets"""
    run_case(oracle, H.CASE["default_trigger"])


def test_floating_base(oracle, device_streams):
    """the config-4 shape, n = 14: AG only (the quaternion is renormalised every iteration)"""
    run_case(oracle, H.CASE["floating_base"])
