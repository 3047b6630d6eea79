#!/usr/bin/env python3
"""tests/golden/ref_outputs*.npz: what the reference build (oracle/_ref, the reference's own ggml.c / utils.cpp) computes for the seeded
inputs of every test that compares against it -- the functions registered with refgolden.computed_by next to those tests, each written
to the store file it names.  Runs where oracle/_ref is built (the reference sources present at build time); the tests re-check the stored
arrays wherever it is."""
import glob
import importlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
import refgolden  # noqa: E402
import reflib  # noqa: E402

for f in sorted(glob.glob(os.path.join(TESTS, "test_*.py"))):
    importlib.import_module(os.path.basename(f)[:-3])
ref = reflib.RefLib()
for store in sorted({s for _, _, s in refgolden.FUNCS.values()}):
    keys = sorted(k for k, f in refgolden.FUNCS.items() if f[2] == store)
    out = {}
    for k in keys:
        with tempfile.TemporaryDirectory() as td:
            out.update({f"{k}/{n}": v for n, v in refgolden.compute(ref, td, k).items()})
    np.savez_compressed(store, **out)
    print(f"wrote {store}: {len(keys)} cases, {len(out)} arrays, {os.path.getsize(store)} bytes")
