"""CPU: the specifications of the per-run parameter calls (or_cdchomp_amd.module.run_params_table and select_best's `column`,
what the -m gpu tests in test_gpu_run_params.py hold orc_batch_set_run_params and orc_batch_select_best_by to) and the two
symbols."""
import ctypes as C
import os

import numpy as np
import pytest

from or_cdchomp_amd import _capi
from or_cdchomp_amd.module import RUN_PARAMS, run_params_table, select_best

INF = float("inf")
NAN = float("nan")
SHARED = dict(lambda_=100.0, epsilon=0.1, obs_factor=500.0, obs_factor_self=10.0)


# ---- run_params_table ------------------------------------------------------------------------------------------------

def test_columns_and_broadcast():
    assert RUN_PARAMS == ("lambda", "epsilon", "obs_factor", "obs_factor_self")
    t = run_params_table(SHARED, 3, 64)
    assert t.shape == (3, 4) and t.dtype == np.float64
    assert t.tolist() == [[100.0, 0.1, 500.0, 10.0]] * 3
    # a sequence in the order of RUN_PARAMS, and the key "lambda", are the same shared values
    assert np.array_equal(run_params_table([100.0, 0.1, 500.0, 10.0], 3, 64), t)
    assert np.array_equal(run_params_table({"lambda": 100.0, "epsilon": 0.1, "obs_factor": 500.0, "obs_factor_self": 10.0}, 3, 64), t)
    # a scalar goes to every run, an array to its runs, None keeps the shared value: every argument lands in its own column
    t = run_params_table(SHARED, 3, 64, lambda_=[50.0, 200.0, 400.0], obs_factor=7.0)
    assert t[:, 0].tolist() == [50.0, 200.0, 400.0] and t[:, 1].tolist() == [0.1] * 3
    assert t[:, 2].tolist() == [7.0] * 3 and t[:, 3].tolist() == [10.0] * 3
    t = run_params_table(SHARED, 2, 64, epsilon=[0.06, 0.14], obs_factor_self=[5.0, 20.0])
    assert t.tolist() == [[100.0, 0.06, 500.0, 5.0], [100.0, 0.14, 500.0, 20.0]]
    # negative and zero weights are values like any other
    t = run_params_table(SHARED, 2, 64, obs_factor=[0.0, -3.0], obs_factor_self=0.0)
    assert t[:, 2].tolist() == [0.0, -3.0] and t[:, 3].tolist() == [0.0, 0.0]
    assert run_params_table(SHARED, 0, 64).shape == (0, 4)


def test_precision_32_rounds_to_float():
    t64 = run_params_table(SHARED, 2, 64, epsilon=[0.06, 0.14])
    t32 = run_params_table(SHARED, 2, 32, epsilon=[0.06, 0.14])
    assert t64[0, 1] == 0.06 and t64[1, 1] == 0.14
    assert t32[0, 1] == float(np.float32(0.06)) and t32[0, 1] != 0.06
    assert t32[1, 1] == float(np.float32(0.14))
    assert t32[0, 0] == 100.0 and t32[0, 2] == 500.0            # (exact in float)
    # the shared values are rounded alike: 0.1 is not a float
    assert run_params_table(SHARED, 1, 32)[0, 1] == float(np.float32(0.1))
    with pytest.raises(ValueError):
        run_params_table(SHARED, 1, 16)


@pytest.mark.parametrize("kw", [
    dict(lambda_=[100.0, NAN]), dict(epsilon=[NAN, 0.1]), dict(obs_factor=[NAN, 1.0]), dict(obs_factor_self=[1.0, NAN]),
    dict(lambda_=[INF, 1.0]), dict(epsilon=[0.1, INF]), dict(obs_factor=[-INF, 1.0]), dict(obs_factor_self=INF),
    dict(lambda_=[0.0, 1.0]), dict(lambda_=-1.0), dict(epsilon=[0.1, 0.0]), dict(epsilon=[-1.0, 0.1]),
    dict(lambda_=[1.0, 2.0, 3.0]), dict(obs_factor=[1.0]),
])
def test_rejections(kw):
    with pytest.raises(ValueError):
        run_params_table(SHARED, 2, 64, **kw)
    with pytest.raises(ValueError):
        run_params_table(SHARED, 2, 32, **kw)


# ---- select_best by column -------------------------------------------------------------------------------------------

COSTS = np.array([[9.0, 8.0, 1.0],       # group 0: the smoothest, the highest total
                  [5.0, 2.0, 3.0],       #          the lowest total and obs
                  [6.0, 4.0, 2.0],
                  [7.0, 1.0, 6.0],       # group 1
                  [7.5, 5.5, 2.0],       #          the smoothest (tie with the next: the lower index)
                  [8.0, 6.0, 2.0]])
GROUPS = [0, 0, 0, 1, 1, 1]


def test_the_column_is_the_key_and_the_reported_cost():
    run, cost, cnt = select_best(COSTS, [0] * 6, None, GROUPS, 2, column=0)
    assert run.tolist() == [1, 3] and cost.tolist() == [5.0, 7.0] and cnt.tolist() == [3, 3]
    for x, y in zip(select_best(COSTS, [0] * 6, None, GROUPS, 2), (run, cost, cnt)):      # (the default is the total)
        assert np.array_equal(x, y)
    run, cost, cnt = select_best(COSTS, [0] * 6, None, GROUPS, 2, column=1)
    assert run.tolist() == [1, 3] and cost.tolist() == [2.0, 1.0]
    # the column-0 and column-2 winners differ, and a tie in the column goes to the lower index
    run, cost, cnt = select_best(COSTS, [0] * 6, None, GROUPS, 2, column=2)
    assert run.tolist() == [0, 4] and cost.tolist() == [1.0, 2.0] and cnt.tolist() == [3, 3]
    assert run.dtype == np.int32 and cnt.dtype == np.int32


def test_eligibility_does_not_depend_on_the_column():
    costs = COSTS.copy()
    costs[0, 0] = NAN          # the smoothest run of group 0 has no finite TOTAL: out, whatever the column
    run, cost, cnt = select_best(costs, [0, 0, 0, 0, -1, 1], [0, 0, 0, 1, 0, 0], GROUPS, 2, column=2)
    assert run.tolist() == [2, 5] and cost.tolist() == [2.0, 2.0] and cnt.tolist() == [2, 1]
    run, cost, cnt = select_best(costs, [0, 0, 0, 0, -1, 1], None, GROUPS, 2, column=1)
    assert run.tolist() == [1, 3] and cost.tolist() == [2.0, 1.0] and cnt.tolist() == [2, 2]
    # an empty group
    run, cost, cnt = select_best(COSTS, [0] * 6, None, [0, 0, 0, 2, 2, 2], 3, column=2)
    assert run.tolist() == [0, -1, 4] and cost.tolist() == [1.0, INF, 2.0] and cnt.tolist() == [3, 0, 3]


def test_bad_columns():
    for column in (3, -1):
        with pytest.raises(ValueError):
            select_best(COSTS, [0] * 6, None, GROUPS, 2, column=column)
    with pytest.raises(ValueError):
        select_best(COSTS[:, 0], [0] * 6, None, GROUPS, 2, column=2)      # (totals only: there is no smoothness column)


# ---- the C ABI -------------------------------------------------------------------------------------------------------

PROTOTYPES = [
    "int orc_batch_set_run_params(orc_module * mod, int batch_id,\n"
    "   const double * lambda, const double * epsilon,\n"
    "   const double * obs_factor, const double * obs_factor_self);",
    "int orc_batch_select_best_by(orc_module * mod, int batch_id, int cost_column, int n_groups,\n"
    "   const int * group_of_run, int require_collision_free,\n"
    "   int * best_run_out, double * best_cost_out, int * n_eligible_out);",
]


def test_symbols_are_in_the_c_abi():
    names = [s[0] for s in _capi.SYMBOLS]
    raw = C.CDLL(_capi.LIB_PATH)
    for name in ("orc_batch_set_run_params", "orc_batch_select_best_by"):
        assert name in names
        assert getattr(raw, name) is not None                  # (AttributeError: the built library lacks the symbol)
    root = os.path.dirname(os.path.dirname(os.path.abspath(_capi.__file__)))
    with open(os.path.join(root, "include", "orcdchomp_amd.h")) as f:
        header = f.read()
    for proto in PROTOTYPES:
        assert proto in header
    assert '"run_params"' in header
    # without a module the calls report "no module" like every other entry point
    lib = _capi.lib()
    assert lib.orc_batch_set_run_params(None, 1, None, None, None, None) == 2
    assert lib.orc_batch_select_best_by(None, 1, 2, 1, None, 0, None, None, None) == 2
