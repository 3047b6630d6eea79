"""CPU: the matrix-core f16 / f32 mat-mul (k_dense_mfma) from the host side -- its launch plan over every dense mat-mul shape of the four LLaMA
widths and the lm head (LDS budget, grid coverage, every plan names a compiled instance), the process-wide kernel switch, and
llamahip_op_mul_mat_dense refusing what the kernel does not take with a message naming the limit before any device is touched."""
import numpy as np
import pytest

LDS_BYTES = 163840           # one CU's LDS (gfx950)
# (n_embd, n_ff) of LLaMA 7B / 13B / 30B / 65B; n_vocab 32000
WIDTHS = [(4096, 11008), (5120, 13824), (6656, 17920), (8192, 22016)]
ROWS = (17, 32, 64, 512)


def _shapes():
    out = []
    for d, F in WIDTHS:
        out += [(3 * d, d), (d, d), (2 * F, d), (d, F), (32000, d)]
    return out


def test_new_symbols_are_declared(L):
    for sym in ("llamahip_debug_dense_mfma_plan", "llamahip_debug_dense_mfma_launches", "llamahip_debug_dense_force"):
        assert sym in L.declared_symbols()
        assert hasattr(L.lib(), sym)
    assert L.binding.DENSE_PATHS == ("auto", "mv", "mm", "set", "mfma")
    assert list(L.dense_paths()) == ["mv", "mm", "set"]          # (the launch counts keep their three entries)
    assert isinstance(L.dense_mfma_launches(), int)


@pytest.mark.parametrize("wtype", [0, 1])
def test_plan_over_model_shapes(L, wtype):
    for M, K in _shapes():
        assert K % 128 == 0
        for N in ROWS:
            p = L.dense_mfma_plan(M, K, wtype, N)         # (raises where the plan names an instance that was never compiled)
            assert p is not None, (M, K, N)
            assert p["lds_bytes"] <= LDS_BYTES, (M, K, N, p)
            assert p["threads"] == 256 and p["tile_rows"] == 64 and p["tile_cols"] in (16, 32)
            assert p["lds_bytes"] == (p["tile_rows"] + p["tile_cols"]) * 260 * 4
            gx, gy = -(-M // p["tile_cols"]), -(-N // p["tile_rows"])
            assert p["grid"] == gx * gy, (M, K, N, p)                           # the grid covers M x N, no idle workgroup
            assert p["auto"] in (0, 1)
    assert L.dense_mfma_plan(40, 320, 1, 17) is None      # (AUTO stays k_dense_mm there: tests/test_gpu_dense_set_op.py)


def test_plan_refuses_what_the_kernel_does_not_take(L):
    assert L.dense_mfma_plan(64, 256, 1, 16) is None         # 16 rows and fewer are k_dense_mv / k_dense_set's
    assert L.dense_mfma_plan(64, 320, 1, 17) is None         # K not a multiple of 128
    assert L.dense_mfma_plan(64, 1344, 0, 64) is None
    assert L.dense_mfma_plan(64, 96, 1, 17) is None
    assert L.dense_mfma_plan(64, 256, 3, 17) is None         # Q4_1 has its own kernel
    assert L.dense_mfma_plan(0, 256, 1, 17) is None
    assert L.dense_mfma_plan(64, 1 << 20, 1, 2048) is None   # n_rows * k must stay below 2^31
    assert L.dense_mfma_plan(64, 128, 0, 17) is not None and L.dense_mfma_plan(64, 384, 1, 17) is not None


def test_force_returns_the_previous_value_and_rejects_other_paths(L):
    try:
        assert L.dense_force(0) == "auto"
        assert L.dense_force("mfma") == "auto"
        assert L.dense_force("mm") == "mfma"
        for bad in ("mv", "set", 5, -1):
            with pytest.raises(ValueError):
                L.dense_force(bad)
        assert L.dense_force("auto") == "mm"                 # (a rejected path changed nothing)
        assert L.dense_force(0) == "auto"
    finally:
        L.dense_force(0)


def _refused(L, *a, **kw):
    with pytest.raises(L.LlamaHipError) as e:
        L.op_mul_mat_dense(*a, **kw)
    assert e.value.code == -1001
    return e.value.message


def test_the_op_refuses_before_any_device_is_touched(L):
    before = L.dense_mfma_launches()
    w = np.ones((8, 256), np.float16)
    msg = _refused(L, w, np.ones((16, 256), np.float32), path="mfma")       # (up to 16 rows the path does not exist: tests/test_dense_set_host.py)
    assert "unknown path 4 for N 16 rows" in msg and "path MFMA takes N > 16 rows" in msg
    assert "K a multiple of 128" in _refused(L, np.ones((8, 320), np.float16), np.ones((17, 320), np.float32), path="mfma")
    assert "wtype 3" in _refused(L, w, np.ones((17, 256), np.float32), path="mfma", wtype=3)
    assert "unknown path 5" in _refused(L, w, np.ones((17, 256), np.float32), path=5)
    assert L.dense_mfma_launches() == before
