"""-m "not gpu": the host side of per-run scenes: the C-ABI symbol and the Python list-of-scenes -> CSR table conversion."""
import ctypes as C
import os

import numpy as np
import pytest

from or_cdchomp_amd import _capi
from or_cdchomp_amd.module import scenes_to_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_batch_create_scenes():
    lib = C.CDLL(_capi.LIB_PATH)
    assert hasattr(lib, "orc_batch_create_scenes")
    assert any(name == "orc_batch_create_scenes" for name, _, _ in _capi.SYMBOLS)
    with open(os.path.join(ROOT, "include", "orcdchomp_amd.h")) as f:
        assert "int orc_batch_create_scenes(" in f.read()


def test_csr_offsets_names_and_poses():
    p1 = [0.1, 0.2, 0.3, 0.0, 0.0, 0.0, 1.0]
    p2 = np.array([[1.0, 2.0, 3.0, 0.0, 0.0, 1.0, 0.0]])       # any shape of 7 entries
    begin, names, poses = scenes_to_csr([[("table", p1), ("mug", None)], [], [("mug", p2)], [("table", None)] * 3])
    assert begin.dtype == np.int32 and begin.tolist() == [0, 2, 2, 3, 6]
    assert names == ["table", "mug", "mug", "table", "table", "table"]
    assert poses.shape == (6, 7) and poses.dtype == np.float64
    assert np.array_equal(poses[0], p1) and np.array_equal(poses[2], p2.reshape(7))
    nan_rows = [k for k in range(6) if np.isnan(poses[k]).all()]
    assert nan_rows == [1, 3, 4, 5]


def test_csr_all_poses_none_passes_no_pose_table():
    begin, names, poses = scenes_to_csr([[("a", None)], [("b", None), ("a", None)]])
    assert begin.tolist() == [0, 1, 3] and names == ["a", "b", "a"] and poses is None
    begin, names, poses = scenes_to_csr([[]])
    assert begin.tolist() == [0, 0] and names == [] and poses is None
    begin, names, poses = scenes_to_csr([])
    assert begin.tolist() == [0] and names == []


@pytest.mark.parametrize("bad", [[0.0] * 6, [0.0] * 8, np.zeros((2, 7))])
def test_csr_rejects_poses_that_are_not_length_7(bad):
    with pytest.raises(ValueError, match="7 entries"):
        scenes_to_csr([[("table", None)], [("mug", bad)]])
