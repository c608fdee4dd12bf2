"""CPU: the convergence stop's rule (or_cdchomp_amd.module.convergence_stop, the specification the -m gpu tests in
test_gpu_convergence.py hold the device to) on hand-made cost traces."""
import math
import os

import numpy as np
import pytest

from or_cdchomp_amd import _capi
from or_cdchomp_amd.module import convergence_stop

NAN = float("nan")


def trace(tots, obs=None):
    """rows (total, obs, smooth) with the given totals; obs 0 unless given (smooth = total - obs)"""
    tots = np.asarray(tots, dtype=np.float64)
    ob = np.zeros_like(tots) if obs is None else np.asarray(obs, dtype=np.float64)
    return np.stack([ob + (tots - ob), ob, tots - ob], axis=-1)


def test_first_row_never_counts():
    # a constant cost: every iteration after the first is settled; patience 1 stops after the second (k = 1)
    assert convergence_stop(trace([5.0] * 6), 1e-3, 1) == (2, True)
    assert convergence_stop(trace([5.0] * 6), 1e-3, 5) == (6, True)
    assert convergence_stop(trace([5.0] * 6), 1e-3, 6) == (6, False)
    assert convergence_stop(trace([5.0]), 1e-3, 1) == (1, False)


def test_streak_breaks_and_restarts():
    # settled: k=1, 2 | unsettled: k=3 | settled: k=4, 5, 6
    t = [10.0, 10.0, 10.0, 20.0, 20.0, 20.0, 20.0, 20.0]
    assert convergence_stop(trace(t), 1e-3, 3) == (7, True)
    assert convergence_stop(trace(t), 1e-3, 2) == (3, True)
    assert convergence_stop(trace(t), 1e-3, 4) == (8, True)
    assert convergence_stop(trace(t), 1e-3, 5) == (8, False)


def test_relative_threshold_is_against_the_previous_cost():
    # |prev - tot| <= rtol |prev|: 100 -> 99.9 is exactly 1e-3 of 100 (settled), 99.9 -> 99.7 is not
    assert convergence_stop(trace([100.0, 99.9, 99.7]), 1e-3, 1) == (2, True)
    assert convergence_stop(trace([100.0, 99.7, 99.4]), 1e-3, 1) == (3, False)
    # a cost that goes UP by a small relative amount settles as well: the rule is on the size of the change
    assert convergence_stop(trace([100.0, 100.05, 100.1]), 1e-3, 2) == (3, True)
    # a cost that goes up by a lot does not
    assert convergence_stop(trace([100.0, 150.0, 150.0, 150.0]), 1e-3, 2) == (4, True)
    assert convergence_stop(trace([100.0, 150.0, 150.0, 150.0]), 1e-3, 3) == (4, False)


def test_obs_max():
    tots = [10.0] * 6
    obs = [1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    assert convergence_stop(trace(tots, obs), 1e-3, 2) == (3, True)
    # the obstacle cost must be at most obs_max: iterations 1 and 2 are not settled, 3 (previous 2) and 4 are
    assert convergence_stop(trace(tots, obs), 1e-3, 2, obs_max=0.0) == (5, True)
    assert convergence_stop(trace(tots, obs), 1e-3, 3, obs_max=0.0) == (6, True)
    assert convergence_stop(trace(tots, obs), 1e-3, 4, obs_max=0.0) == (6, False)
    assert convergence_stop(trace(tots, obs), 1e-3, 2, obs_max=0.5) == (5, True)
    assert convergence_stop(trace(tots, obs), 1e-3, 2, obs_max=1.0) == (3, True)


def test_nan_tail_of_an_aborted_run():
    # a run that left its joint limits after 4 iterations: NaN rows from there on.  It made 4 iterations and did not stop
    t = trace([10.0, 9.0, 8.0, 7.0, 7.0, 7.0])
    t[4:] = NAN
    assert convergence_stop(t, 1e-3, 2) == (4, False)
    assert convergence_stop(t, 1e-3, 1) == (4, False)      # (the NaN rows are not settled: 7 -> NaN does not stop it)
    # a run whose rule stops it before it would have left its limits
    t2 = trace([10.0, 10.0, 10.0, 7.0, 7.0, 7.0])
    t2[3:] = NAN
    assert convergence_stop(t2, 1e-3, 2) == (3, True)
    assert convergence_stop(t2, 1e-3, 3) == (3, False)
    # a run that made no iteration at all
    assert convergence_stop(np.full((4, 3), NAN), 1e-3, 1) == (0, False)


def test_batch_form():
    runs = np.stack([trace([5.0] * 5), trace([5.0, 6.0, 7.0, 8.0, 9.0]), trace([1.0, 2.0, 2.0, 2.0, 2.0])])
    iters, stopped = convergence_stop(runs, 1e-3, 2)
    assert iters.tolist() == [3, 5, 4]
    assert stopped.tolist() == [True, False, True]
    assert iters.dtype == np.int32 and stopped.dtype == bool


def test_zero_and_infinite_costs():
    # a cost of exactly zero settles only when it stays exactly zero (rtol * 0 = 0)
    assert convergence_stop(trace([0.0, 0.0, 0.0]), 1e-3, 2) == (3, True)
    assert convergence_stop(trace([0.0, 1e-300, 0.0]), 1e-3, 1) == (3, False)
    # inf - inf is NaN: never settled
    assert convergence_stop(trace([math.inf] * 4), 1e-3, 1) == (4, False)


@pytest.mark.parametrize("rtol,patience,obs_max", [(0.0, 1, math.inf), (-1e-3, 1, math.inf), (NAN, 1, math.inf),
                                                   (1e-3, 0, math.inf), (1e-3, 1, NAN)])
def test_bad_criterion(rtol, patience, obs_max):
    with pytest.raises(ValueError):
        convergence_stop(trace([1.0, 1.0]), rtol, patience, obs_max)


def test_setter_is_in_the_c_abi():
    names = [s[0] for s in _capi.SYMBOLS]
    assert "orc_batch_set_convergence" in names
    root = os.path.dirname(os.path.dirname(os.path.abspath(_capi.__file__)))
    with open(os.path.join(root, "include", "orcdchomp_amd.h")) as f:
        assert "int orc_batch_set_convergence(orc_module * mod, int batch_id, double rtol, int patience, double obs_max);" in f.read()
