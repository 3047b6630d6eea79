"""CPU: k_q40_dot's plan at the LLaMA shapes, llamahip_op_gemv_q4_0_dot's refusals before any device is touched, llamahip_opts.fast_decode
at load (host-only handles: no device)."""
import ctypes as C
import os

import numpy as np
import pytest

import synth
from llama_swift_amd import binding

HP = synth.HParams(n_vocab=64, n_embd=64, n_mult=32, n_head=2, n_layer=1)

@pytest.mark.parametrize("d,F", [(4096, 11008), (5120, 13824), (6656, 17920), (8192, 22016)])      # 7B, 13B, 30B, 65B
def test_the_plan_at_the_llama_shapes(L, d, F):
    for K in (d, F):                                        # wo, w2
        p = L.q40_dot_plan(d, K)
        assert (p["slices"], p["threads"], p["grid"]) == (8, 512, d // 16) and p["grid"] <= 512, "S and the grid follow (M, K) alone"
        assert p["lds_bytes"] == -(-K // 256) * 288 + 512 <= 48 * 1024
        assert p["applies"] == 0, "the 7B matrices measured slower than k_gemv (DESIGN.md 12.40): from 4096 rows on the decode step keeps k_gemv"
    assert L.q40_dot_plan(256, 704) == dict(slices=8, threads=512, grid=16, lds_bytes=1376, applies=1)
    assert L.q40_dot_plan(8208, 4096) == dict(slices=4, threads=256, grid=513, lds_bytes=5120, applies=0), "513 pairs do not fit the hand-off"
    assert all(L.q40_dot_plan(*a) is None for a in [(64, 48), (64, 0), (0, 64), (64, 256 * 200)])

def test_refusals_name_their_limit(L):
    w, x, y, parts = np.zeros((16, 2 * 20), np.uint8), np.zeros(64, np.float32), np.zeros(16, np.float32), np.zeros((1, 2))
    err = C.create_string_buffer(256)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = dict(w=ptr(w), M=16, K=64, x=ptr(x), y=ptr(y), yc=16, p=ptr(parts), pc=1)
    for change, says in [(dict(K=48), b"K 48 must be a positive multiple of 32"), (dict(K=0), b"K 0 must be"), (dict(M=0), b"M 0 must be >= 1"),
                         (dict(yc=15), b"y_cap 15 < M 16"), (dict(M=17, yc=17), b"parts_cap 1 < 2 pairs"), (dict(K=256 * 200), b"bytes of LDS"),
                         (dict(w=None), b"not NULL"), (dict(x=None), b"not NULL"), (dict(y=None), b"not NULL"), (dict(p=None), b"not NULL")]:
        a = {**ok, **change}
        rc = L.lib().llamahip_op_gemv_q4_0_dot(a["w"], a["M"], a["K"], a["x"], None, a["y"], a["yc"], a["p"], a["pc"], err, len(err))
        assert rc != 0 and says in err.value, (change, err.value)

def load(L, path, size, fast_decode, tail=b""):
    """llamahip_model_load of a HOST_ONLY handle on an options struct cut at `size` bytes, `tail` lying behind it"""
    o = binding._Opts(size, -1, 0, -1, 0, 4, 1, 0, (C.c_int32 * 8)(), fast_decode)
    buf = (C.c_char * (C.sizeof(o) + len(tail)))()
    C.memmove(buf, C.byref(o), size)
    C.memmove(C.byref(buf, size), tail, len(tail))
    h, err = C.c_void_p(), C.create_string_buffer(256)
    rc = L.lib().llamahip_model_load(path.encode(), 32, C.cast(buf, C.POINTER(binding._Opts)), C.byref(h), err, len(err))
    if h:
        L.lib().llamahip_model_free(h)
    return rc, err.value.decode()

def test_the_field_at_load(L, tmp_path):
    path = os.path.join(str(tmp_path), "q4_0.bin")
    synth.write_model(path, HP, synth.random_tensors(HP, seed=7))
    assert C.sizeof(binding._Opts) == 68 and binding._Opts.fast_decode.offset == 64
    assert load(L, path, 68, 0)[0] == 0 and load(L, path, 68, 1)[0] == 0
    for bad in (2, -1):
        rc, msg = load(L, path, 68, bad)
        assert rc != 0 and f"fast_decode {bad}" in msg
    # the struct of the callers before the field, garbage behind it: loads, the field is not read
    for size in (24, 28, 64):
        assert load(L, path, size, 0, tail=b"\x7f" * 8) == (0, "")
