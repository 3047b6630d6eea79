"""CPU: what llamahip_op_mul_mat_f16_fast refuses before any device is touched, each with the limit in its message, and the instance rule of
k_dense_f16_fast (dense_fast_plan) at its edges."""
import ctypes as C

import numpy as np
import pytest


def test_refusals_name_their_limit(L):
    w, x = np.zeros((16, 64), np.float16), np.zeros((64, 64), np.float32)
    with pytest.raises(L.LlamaHipError, match=r"N 63: the kernel takes N >= 64 rows"):
        L.op_mul_mat_f16_fast(w, x[:63])
    with pytest.raises(L.LlamaHipError, match=r"K 48 must be a positive multiple of 32"):
        L.op_mul_mat_f16_fast(w[:, :48], x[:, :48])
    with pytest.raises(L.LlamaHipError, match=r"y_stride 15 < M 16"):
        L.op_mul_mat_f16_fast(w, x, y_stride=15)
    err = C.create_string_buffer(256)
    y = np.zeros((64, 16), np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((None, ptr(x), ptr(y)), (ptr(w), None, ptr(y)), (ptr(w), ptr(x), None)):
        assert L.lib().llamahip_op_mul_mat_f16_fast(args[0], 16, 64, args[1], 64, None, args[2], 16, err, len(err)) != 0
        assert b"w, x, y not NULL" in err.value


@pytest.mark.parametrize("M,K,N,tile", [
    (4096, 4096, 64, (64, 16, 256)),        # wo against 64 rows: 32 wide / 64 mid workgroups -> narrow, 256 workgroups
    (4096, 4096, 128, (64, 64, 128)),       # 128 mid workgroups
    (4096, 4096, 512, (64, 64, 128)),       # 128 wide workgroups are too few
    (12288, 4096, 512, (128, 128, 64)),     # wq|wk|wv at 512 rows: 384 wide workgroups
    (8128, 64, 64, (64, 16, 256)), (8129, 64, 64, (64, 64, 128)),          # 127 | 128 mid workgroups
    (16256, 64, 129, (64, 64, 128)), (16257, 64, 129, (128, 128, 64)),     # 254 | 256 wide workgroups
])
def test_the_instance_rule(L, M, K, N, tile):
    p = L.dense_fast_plan(M, K, N)
    assert (p["tile_rows"], p["tile_cols"], p["k_tile"]) == tile
    assert p["grid_x"] == -(-N // tile[0]) and p["grid_y"] == -(-M // tile[1])
    assert p["lds_bytes"] == 2 * (tile[0] + tile[1]) * (tile[2] + 8) * 2 <= 160 * 1024


def test_shapes_the_kernel_does_not_take(L):
    assert L.dense_fast_plan(64, 64, 63) is None and L.dense_fast_plan(64, 48, 64) is None and L.dense_fast_plan(0, 64, 64) is None
