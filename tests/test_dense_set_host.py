"""CPU: the few-row f16 / f32 mat-mul (k_dense_set) from the host side -- its launch plan over every dense mat-mul shape of the four LLaMA
widths and over the shapes of tests/test_gpu_dense_set_op.py (LDS budget, grid coverage, every plan names a compiled instance), and the
single-op entry point llamahip_op_mul_mat_dense refusing bad arguments with a message naming the limit before any device is touched."""
import numpy as np
import pytest

LDS_BYTES = 163840           # one CU's LDS (gfx950)
# (n_embd, n_ff) of LLaMA 7B / 13B / 30B / 65B; n_vocab 32000
WIDTHS = [(4096, 11008), (5120, 13824), (6656, 17920), (8192, 22016)]
OP_KS, OP_MS = (256, 320, 896, 1344, 4096, 11008), (40, 250, 1024)      # tests/test_gpu_dense_set_op.py


def _shapes():
    out = []
    for d, F in WIDTHS:
        out += [(3 * d, d), (d, d), (2 * F, d), (d, F), (32000, d)]
    out += [(M, K) for K in OP_KS for M in OP_MS]
    return out


def test_new_symbols_are_declared(L):
    for sym in ("llamahip_op_mul_mat_dense", "llamahip_debug_dense_set_plan", "llamahip_debug_dense_paths"):
        assert sym in L.declared_symbols()
        assert hasattr(L.lib(), sym)
    assert list(L.dense_paths()) == ["mv", "mm", "set"]


@pytest.mark.parametrize("wtype", [0, 1])
def test_plan_over_model_and_test_shapes(L, wtype):
    for M, K in _shapes():
        for N in range(2, 17):
            p = L.dense_set_plan(M, K, wtype, N)          # (raises where the plan names an instance that was never compiled)
            assert p is not None, (M, K, N)
            assert p["lds_bytes"] <= LDS_BYTES, (M, K, N, p)
            assert p["threads"] % 32 == 0 and p["threads"] <= 256
            rows_per_wg = p["threads"] // 32 * p["rows_per_half_wave"]
            assert p["grid"] * rows_per_wg >= M > (p["grid"] - 1) * rows_per_wg, (M, K, N, p)      # the grid covers M, no idle workgroup
            assert N <= p["rows"] <= 16
            assert p["lds_bytes"] == 2 * p["slab_groups"] * p["rows"] * 256 * 4


def test_plan_refuses_what_the_kernel_does_not_take(L):
    assert L.dense_set_plan(64, 48, 1, 4) is None            # K not a multiple of 32
    assert L.dense_set_plan(64, 256, 1, 17) is None          # more than 16 rows
    assert L.dense_set_plan(64, 256, 1, 0) is None
    assert L.dense_set_plan(64, 256, 3, 4) is None           # Q4_1 has its own kernel
    assert L.dense_set_plan(0, 256, 1, 4) is None


def _refused(L, *a, **kw):
    with pytest.raises(L.LlamaHipError) as e:
        L.op_mul_mat_dense(*a, **kw)
    assert e.value.code == -1001
    return e.value.message


def test_bad_arguments_are_refused_before_any_device_is_touched(L):
    w = np.ones((8, 256), np.float16)
    assert "N 0 must be >= 1" in _refused(L, w, np.ones((0, 256), np.float32))
    assert "path SET takes N 1 .. 16 rows (got 17)" in _refused(L, w, np.ones((17, 256), np.float32), path="set")
    assert "K 48 must be a positive multiple of 32" in _refused(L, np.ones((8, 48), np.float16), np.ones((2, 48), np.float32))
    assert "wtype 3" in _refused(L, w, np.ones((2, 256), np.float32), wtype=3)
    assert "y_stride 7 < M 8" in _refused(L, w, np.ones((2, 256), np.float32), y_stride=7)
    assert "unknown path 4" in _refused(L, w, np.ones((2, 256), np.float32), path=4)


def test_fails_loudly_without_a_gpu(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert "no CPU fallback" in _refused(L, np.ones((8, 256), np.float16), np.ones((17, 256), np.float32))
