"""What the reference build computes for the seeded inputs of the tests that compare against it, stored with the tests.

oracle/_ref (the reference's own ggml.c / utils.cpp) can only be built where the reference sources are present.  A test that compares
against it registers the reference side as a function of (RefLib, scratch directory, *case) -> {key: array} with @computed_by and reads
the arrays with outputs(); tests/golden/make_ref_golden.py runs every registered function and writes the store each one names
(tests/golden/ref_outputs.npz unless computed_by is given another file, which keeps every store a small file of its own).
Where oracle/_ref is present, outputs() runs the function again and the stored arrays must be its result bit for bit."""
import hashlib
import os

import numpy as np

STORE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_outputs.npz")
FUNCS = {}                                    # key -> (function, case, store file)
_stored = {}                                  # store file -> {array name: array}


def key(name, case=()):
    return name + "".join(f":{c}" for c in case)


def computed_by(name, cases=((),), store=STORE):
    def register(fn):
        for case in cases:
            FUNCS[key(name, case)] = (fn, tuple(case), store)
        return fn
    return register


def digest(a) -> np.ndarray:
    """sha256 of an array's dtype, shape and bytes: stands for arrays too large to store (model tensors, KV caches)."""
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode())
    h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def compute(ref, tmp_dir, k) -> dict:
    fn, case, _ = FUNCS[k]
    return {n: np.asarray(v) for n, v in fn(ref, str(tmp_dir), *case).items()}


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def outputs(name, ref, tmp_dir, *case) -> dict:
    k = key(name, case)
    store = FUNCS[k][2] if k in FUNCS else STORE
    if store not in _stored:
        with np.load(store) as z:
            _stored[store] = {n: z[n] for n in z.files}
    want = {n[len(k) + 1:]: v for n, v in _stored[store].items() if n.startswith(k + "/")}
    assert want, f"{store} has no reference outputs for {k}: run tests/golden/make_ref_golden.py where oracle/_ref is built"
    if ref is not None:
        live = compute(ref, tmp_dir, k)
        bad = sorted(n for n in live.keys() | want.keys() if n not in live or n not in want or not _same(live[n], want[n]))
        assert not bad, f"{store} does not hold what oracle/_ref computes for {k} ({bad}): run tests/golden/make_ref_golden.py"
    return want
