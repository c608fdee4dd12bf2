"""-m "not gpu": the premises of tests/test_gpu_config_clearance.py, without a GPU.  Every trajectory those tests build to hold
orc_batch_config_clearance to orc_batch_clearance has exactly one sample, on segment 0 at u = 0; the fixed configurations of the
WAM test are not set aside by the face premise of tests/clearance.py and cover the outcomes the test names; and the two calls'
place in the C ABI."""
import os
import re

import numpy as np
import pytest

import clearance as CL
import common
import config_clearance as CC
from or_cdchomp_amd import _capi, robots
from or_cdchomp_amd.module import verdict_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_one_sample(T, vmax, col0, what):
    seg, u, time = verdict_samples(T, vmax, col0)
    assert seg.tolist() == [0] and u.tolist() == [0.0] and time.tolist() == [0.0], (what, seg, u)


def test_one_sample_premise_of_the_issue():
    """rows q, q+e, q+e, q+e with e on dof 4, under unit and under unequal vmax"""
    q = np.asarray(robots.WAM_START, dtype=np.float64)
    for e in (1e-9, 0.01, 0.03, 0.0399):
        T = np.tile(q, (4, 1)); T[1:, 4] += e
        for vmax in (np.ones(7), CC.WAM_VMAX):
            assert_one_sample(T, vmax, 0, e)


def test_every_gpu_trajectory_has_one_sample():
    _, base, _, _ = common.wam_state()
    base = np.asarray(base, dtype=np.float64); base[0] -= 0.2
    tree_vmax = np.linspace(0.5, 2.0, 30)
    sets = [("wam", np.array(list(CC.wam_fixed().values())), CC.WAM_VMAX, 0), ("pool", CC.wam_pool(), CC.WAM_VMAX, 0),
            ("tree", CC.tree_pool(), tree_vmax, 0), ("floating", CC.floating_configs(base), CC.WAM_VMAX, 7),
            ("held", CC.held_configs(), CC.WAM_VMAX, 0), ("folding", CC.folding_configs(), CC.WAM_VMAX, 0)]
    for name, configs, vmax, col0 in sets:
        assert len(np.unique(configs, axis=0)) == len(configs), name
        for k, T in enumerate(CC.one_sample_batch(configs, 4, col0)):
            assert np.array_equal(T[0], configs[k])
            assert_one_sample(T, vmax, col0, (name, k))
            # a precision-32 batch holds the narrowed rows, and its plan is made on them widened
            assert_one_sample(T.astype(np.float32).astype(np.float64), vmax, col0, (name, k, "fp32"))


def test_configurations_stay_inside_the_joint_limits():
    wam = robots.wam7()
    lo, hi = np.asarray(wam.limit_lower[:7]), np.asarray(wam.limit_upper[:7])
    _, base, _, _ = common.wam_state()
    for configs in (np.array(list(CC.wam_fixed().values())), CC.wam_pool(), CC.held_configs(), CC.folding_configs(), CC.floating_configs(base)[:, 7:]):
        for T in CC.one_sample_batch(configs):
            assert (T >= lo).all() and (T <= hi).all()
    tree = robots.tree30()
    lo, hi = np.asarray(tree.limit_lower[:30]), np.asarray(tree.limit_upper[:30])
    for T in CC.one_sample_batch(CC.tree_pool()):
        assert (T >= lo).all() and (T <= hi).all()


@pytest.fixture(scope="module")
def wam(oracle):
    prob = common.tabletop_problem(oracle)
    model, base, dofvals, adofs = common.wam_state()
    field = CL.Field(oracle, prob["sdf"], None, prob["pose"])
    return dict(field=field, tab=CL.Tables(oracle, model, base, dofvals, adofs, [field]))


def test_fixed_configurations_of_the_wam(wam):
    """none is set aside, and they cover what the GPU test names: a penetration, a self collision, a configuration outside the field"""
    res = {}
    for name, q in CC.wam_fixed().items():
        r = CL.restate(wam["tab"], CC.one_sample(q)[:2], CC.WAM_VMAX, 0, [wam["field"]])
        assert r["n_samples"] == 1 and not CL.set_aside(r, [wam["field"]]), name
        res[name] = r["clearance"]
        print("%-14s %+.6f %+.6f" % (name, r["clearance"][0], r["clearance"][1]))
    assert res["in the table"][0] < 0.0
    assert 0.0 < res["near"][0] < 0.05
    assert res["folded"][1] < 0.0
    assert np.isposinf(res["away"][0]) and np.isfinite(res["away"][1])
    assert res["start"][0] > 0.0 and res["start"][1] > 0.0


def test_symbols_and_null_module():
    header = open(os.path.join(ROOT, "include", "orcdchomp_amd.h")).read()
    for name, args in (("orc_batch_config_clearance", ["orc_module * mod", "int batch_id", "int n_q", "const int * run_of_q", "const double * configs",
                                                       "double * clearance_out", "int * sphere_out", "int * other_out"]),
                       ("orc_batch_waypoint_clearance", ["orc_module * mod", "int batch_id", "int n_q", "const int * run_of_q", "const int * point_of_q",
                                                         "double * clearance_out", "int * sphere_out", "int * other_out"])):
        m = re.search(r"int %s\((.*?)\);" % name, header, re.S)
        assert m, name
        assert [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")] == args
        assert name in [s[0] for s in _capi.SYMBOLS] and hasattr(_capi.lib(), name)
    lib = _capi.lib()
    clr = np.full((3, 2), 7.0); cfg = np.zeros((3, 7))
    want = lib.orc_batch_clearance(None, 1, 2, None, 64, clr.ctypes.data_as(_capi.c_double_p), None, None, None, None)
    assert lib.orc_batch_config_clearance(None, 1, 3, None, cfg.ctypes.data_as(_capi.c_double_p), clr.ctypes.data_as(_capi.c_double_p), None, None) == want
    assert lib.orc_batch_waypoint_clearance(None, 1, 3, None, None, clr.ctypes.data_as(_capi.c_double_p), None, None) == want
    assert (clr == 7.0).all(), "a NULL module writes nothing"
