"""CPU: k_q41_dot's plan at the LLaMA shapes, llamahip_op_mul_mat_q4_1_dot's refusals before any device is touched, the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest


@pytest.mark.parametrize("d,F", [(4096, 11008), (5120, 13824), (6656, 17920), (8192, 22016)])      # 7B, 13B, 30B, 65B
def test_the_plan_at_the_llama_shapes(L, d, F):
    for M, K in [(3 * d, d), (d, d), (2 * F, d), (d, F), (32000, d)]:
        for N in (1, 9, 16, 17, 63):
            p = L.q41_dot_plan(M, K, N)
            assert p["nr"] in (1, 2, 4, 8, 12, 16) and p["nr"] >= min(N, 16) and p["threads"] == 256
            assert (p["grid_x"], p["grid_y"], p["klanes"]) == (-(-M // 16), -(-N // 16), 16), "the grid and the K split must not follow N"
            assert p["slab"] % 16 == 0 and p["lds_bytes"] == 2 * p["nr"] * p["slab"] * 32 <= 64 * 1024


def test_refusals_name_their_limit(L):
    assert L.q41_dot_plan(64, 48, 1) is None and L.q41_dot_plan(64, 64, 0) is None and L.q41_dot_plan(0, 64, 1) is None
    assert L.q41_dot_plan(64, 64, 16 * 65535)["grid_y"] == 65535 and L.q41_dot_plan(64, 64, 16 * 65535 + 1) is None
    w, x, y = np.zeros((16, 2 * 24), np.uint8), np.zeros((4, 64), np.float32), np.zeros((4, 16), np.float32)
    err = C.create_string_buffer(256)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = dict(w=ptr(w), M=16, K=64, x=ptr(x), N=4, y=ptr(y), ys=16)
    for change, says in [(dict(K=48), b"K 48 must be a positive multiple of 32"), (dict(N=0), b"N 0 must be >= 1"), (dict(M=0), b"M 0 must be >= 1"),
                         (dict(ys=15), b"y_stride 15 < M 16"), (dict(w=None), b"not NULL"), (dict(x=None), b"not NULL"), (dict(y=None), b"not NULL"),
                         (dict(N=16 * 65535 + 1), b"more than 65535 row tiles of 16")]:
        a = {**ok, **change}
        assert L.lib().llamahip_op_mul_mat_q4_1_dot(a["w"], a["M"], a["K"], a["x"], a["N"], None, a["y"], a["ys"], err, len(err)) != 0 and says in err.value


def test_the_new_symbols_are_declared_and_exported(L):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "llamahip.h")).read()
    for name in ("llamahip_op_mul_mat_q4_1_dot", "llamahip_debug_q41_dot_plan", "llamahip_debug_q41_dot_launches"):
        assert re.search(r"\b%s\(" % name, header) and getattr(L.lib(), name), name
    assert "#define LLAMAHIP_FLAG_FAST_Q41_DECODE 256" in header and L.FAST_Q41_DECODE == 256 and L.FAST_Q41_DECODE & (L.FAST_Q41 | L.FAST_ATTN) == 0
