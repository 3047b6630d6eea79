"""CPU: k_q40_few's plan at the LLaMA shapes, llamahip_op_mul_mat_q4_0_few's refusals before any device is touched, the new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

@pytest.mark.parametrize("d,F", [(4096, 11008), (5120, 13824), (6656, 17920), (8192, 22016)])      # 7B, 13B, 30B, 65B
def test_the_plan_at_the_llama_shapes(L, d, F):
    for M, K in [(3 * d, d), (d, d), (2 * F, d), (d, F), (32000, d)]:
        plans = [L.q40_few_plan(M, K, N) for N in range(1, 64)]
        assert {(p["slices"], p["threads"], p["grid"]) for p in plans} == {(8 if M <= 8192 else 4, 512 if M <= 8192 else 256, -(-M // 16))}, \
            "the K split and the grid must not follow N"
        assert [p["nt"] for p in plans] == [-(-N // 16) for N in range(1, 64)]
        assert all(p["lds_bytes"] == 8 * (p["nt"] * 1024 + 512) for p in plans)
    assert L.q40_few_plan(4096, 4096, 16) == dict(nt=1, slices=8, threads=512, grid=256, lds_bytes=12288)      # 7B wo: one workgroup per CU

def test_refusals_name_their_limit(L):
    assert all(L.q40_few_plan(*a) is None for a in [(64, 48, 2), (64, 0, 2), (0, 64, 2), (64, 64, 0), (64, 64, 64)])
    w, x, y = np.zeros((16, 2 * 20), np.uint8), np.zeros((4, 64), np.float32), np.zeros((4, 16), np.float32)
    err = C.create_string_buffer(256)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = dict(w=ptr(w), M=16, K=64, x=ptr(x), N=4, y=ptr(y), ys=16)
    for change, says in [(dict(K=48), b"K 48 must be a positive multiple of 32"), (dict(N=0), b"N 0 outside 1 .. 63"), (dict(N=64), b"N 64 outside 1 .. 63"),
                         (dict(M=0), b"M 0 must be >= 1"), (dict(ys=15), b"y_stride 15 < M 16"), (dict(w=None), b"not NULL"), (dict(x=None), b"not NULL"),
                         (dict(y=None), b"not NULL")]:
        a = {**ok, **change}
        assert L.lib().llamahip_op_mul_mat_q4_0_few(a["w"], a["M"], a["K"], a["x"], a["N"], None, a["y"], a["ys"], err, len(err)) != 0 and says in err.value

def test_the_new_symbols_are_declared_and_exported(L):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "llamahip.h")).read()
    for name in ("llamahip_op_mul_mat_q4_0_few", "llamahip_debug_q40_few_plan", "llamahip_debug_q40_few_launches"):
        assert re.search(r"\b%s\(" % name, header) and getattr(L.lib(), name), name
    others = [int(v) for n, v in re.findall(r"#define LLAMAHIP_FLAG_(\w+)\s+(\d+)", header) if n != "FAST_Q40_FEW"]
    assert "#define LLAMAHIP_FLAG_FAST_Q40_FEW 512" in header and L.FAST_Q40_FEW == 512 and len(others) == 9 and not any(v & 512 for v in others)
