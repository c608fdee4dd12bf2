#!/usr/bin/env python3
"""Writes tests/golden/ref_random_scenes.npz: what the reference's OWN grid code (oracle/_ref/libcd_ref.so, see
oracle/Makefile) makes of the randomised scenes of tests/test_oracle_ref.py (the SDF and, at 400 probe points per
scene, interp / grad / lookup_index).  Run where the reference tree is present; the outputs are data and are committed.

   python tests/golden/make_ref_random_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle_py as O  # noqa: E402
import test_oracle_ref as T        # noqa: E402

O.build(ref=True)
R = O.ref()
assert R is not None, "oracle/_ref/libcd_ref.so missing (needs the reference tree)"
T.prepare(R)
out = {}
for seed in T.SEEDS:
    for k, v in T.reference_outputs(R, seed).items():
        out["%s_%d" % (k, seed)] = v
path = os.path.join(HERE, "ref_random_scenes.npz")
np.savez_compressed(path, **out)
print("%s: %d scenes, %d bytes" % (path, len(T.SEEDS), os.path.getsize(path)))
