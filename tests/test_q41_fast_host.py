"""CPU: the launch plan of k_q41_fast (q41_fast_plan) at the LLaMA-7B matrix shapes and at its refusals, and what
llamahip_op_mul_mat_q4_1_fast refuses before any device is touched, each with the limit in its message."""
import ctypes as C

import numpy as np
import pytest

TILES = {(128, 128, 64), (64, 64, 128), (64, 16, 256)}      # the compiled instances: activation rows x weight rows, K tile
SHAPES_7B = [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008), (32000, 4096)]      # wq|wk|wv, wo, w1|w3, w2, lm head


@pytest.mark.parametrize("M,K", SHAPES_7B)
@pytest.mark.parametrize("N", [64, 128, 512])
def test_the_plan_at_the_7b_shapes(L, M, K, N):
    p = L.q41_fast_plan(M, K, N)
    tile = (p["tile_rows"], p["tile_cols"], p["k_tile"])
    assert tile in TILES
    wgs = lambda t: -(-N // t[0]) * -(-M // t[1])
    assert tile == ((128, 128, 64) if wgs((128, 128)) >= 256 else (64, 64, 128) if wgs((64, 64)) >= 256 else (64, 16, 256))
    assert p["grid_x"] == -(-N // tile[0]) and p["grid_y"] == -(-M // tile[1])
    assert p["grid_x"] * p["grid_y"] >= 256, "fewer workgroups than CUs"
    assert p["lds_bytes"] == 2 * (tile[0] + tile[1]) * (tile[2] + 8) * 2 <= 160 * 1024


def test_shapes_the_plan_refuses(L):
    assert L.q41_fast_plan(64, 48, 64) is None and L.q41_fast_plan(64, 0, 64) is None       # K % 32
    assert L.q41_fast_plan(64, 64, 0) is None                                               # N < 1
    assert L.q41_fast_plan(0, 64, 64) is None
    assert L.q41_fast_plan(128 * 65535, 32, 1)["grid_y"] == 65535 and L.q41_fast_plan(128 * 65535 + 1, 32, 1) is None      # (wide) grid y past 65535


def test_refusals_name_their_limit(L):
    w, x = np.zeros((16, 2 * 24), np.uint8), np.zeros((4, 64), np.float32)
    with pytest.raises(L.LlamaHipError, match=r"K 48 must be a positive multiple of 32"):
        L.op_mul_mat_q4_1_fast(w, x[:, :48], K=48)
    with pytest.raises(L.LlamaHipError, match=r"N 0 must be >= 1"):
        L.op_mul_mat_q4_1_fast(w, x[:0])
    with pytest.raises(L.LlamaHipError, match=r"y_stride 15 < M 16"):
        L.op_mul_mat_q4_1_fast(w, x, y_stride=15)
    err = C.create_string_buffer(256)
    y = np.zeros((4, 16), np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((None, ptr(x), ptr(y)), (ptr(w), None, ptr(y)), (ptr(w), ptr(x), None)):
        assert L.lib().llamahip_op_mul_mat_q4_1_fast(args[0], 16, 64, args[1], 4, None, args[2], 16, err, len(err)) != 0
        assert b"w_q4_1, x, y not NULL" in err.value
    assert L.lib().llamahip_op_mul_mat_q4_1_fast(ptr(w), 128 * 65535 + 1, 32, ptr(x), 1, None, ptr(y), 128 * 65535 + 1, err, len(err)) != 0
    assert b"more than 65535 rows of workgroups" in err.value
