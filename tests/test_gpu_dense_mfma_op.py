"""GPU (-m gpu): the matrix-core f16 / f32 mat-mul k_dense_mfma alone (llamahip_op_mul_mat_dense, path MFMA), bit for bit against the one-row
kernel k_dense_mv run on each row (path MV: the kernel tests/test_gpu_dense_mv_op.py pins op by op to the reference's ggml_vec_dot_f16 /
_f32).

K walks the structures of the kernel's loop:  128 the 4-step tail group alone | 256 one group | 384 a group + the tail | 1280 five groups |
4096 sixteen | 11008 43 groups.  The kernel takes multiples of 128 only: 320 and 1344 must be REFUSED with a message that names the limit.
M: 40 (three 16-row tiles, the last one partial), 250 (a column tail inside a tile), 1024 (the 32-row workgroup tile once N reaches 512 /
the 16-row one below).  N: 17 (one row over an MFMA tile), 31, 32, 33, 47, 64, 130 (three workgroup rows) at K 1280, M 250; 17 and 64
elsewhere.  Store and residual epilogues; y rows M + 8 apart with NaN guard columns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (128, 256, 384, 1280, 4096, 11008)
KS_REFUSED = (320, 1344)
MS = (40, 250, 1024)
GUARD = 8
ROWS = 130


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _operands(M, K, wtype, seed, rows=ROWS):
    """tests/test_gpu_dense_set_op.py's operands grown to `rows` rows: weights of the synthetic models' scale (sigma 0.02), activation rows of
    a normed row's scale, rows 1, 6, 11 with a DC offset; all finite"""
    rng = np.random.default_rng(seed)
    w = (0.02 * rng.standard_normal((M, K))).astype(np.float16 if wtype == 1 else np.float32)
    x = rng.standard_normal((rows, K)).astype(np.float32)
    x[1] += 3.0; x[6] -= 1.5; x[11] += 0.25
    resid = rng.standard_normal((rows, M)).astype(np.float32)
    assert np.isfinite(w.astype(np.float32)).all() and np.isfinite(x).all()
    return w, x, resid


def _run(L, w, x, resid, path):
    N, M = x.shape[0], w.shape[0]
    y, taken = L.op_mul_mat_dense(w, x, resid[:N] if resid is not None else None, path=path, y_stride=M + GUARD)
    assert taken == path
    assert np.isnan(y[:, M:]).all(), f"{path}: guard columns written (N {N}, M {M}, K {w.shape[1]})"
    assert not np.isnan(y[:, :M]).any(), f"{path}: an output left unwritten (N {N}, M {M}, K {w.shape[1]})"
    return y[:, :M]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("wtype", [1, 0], ids=["f16", "f32"])
def test_mfma_equals_the_one_row_kernel(L, wtype, K):
    before = L.dense_mfma_launches()
    n_launch = 0
    for M in (MS if K != 11008 else (40,)):
        ns = (17, 31, 32, 33, 47, 64, 130) if (K, M) == (1280, 250) else (17, 64)
        w, x, resid = _operands(M, K, wtype, seed=K * 7 + M + wtype, rows=max(ns))
        for r in (None, resid):
            want = _run(L, w, x, r, "mv")                                       # one launch of k_dense_mv per row
            for N in ns:
                got = _run(L, w, x[:N], r, "mfma")
                n_launch += 1
                assert same(got, want[:N]), f"mfma vs mv: wtype {wtype}, M {M}, K {K}, N {N}, resid {r is not None}: " \
                                            f"{int((got != want[:N]).sum())} of {got.size} outputs differ"
    assert L.dense_mfma_launches() - before == n_launch


def test_the_wide_workgroup_tile(L):
    """M 1024 x N 512: the plan's 32-row tile (two accumulator tiles per wave), eight workgroup rows"""
    assert L.dense_mfma_plan(1024, 256, 1, 512)["tile_cols"] == 32 and L.dense_mfma_plan(1024, 256, 1, 64)["tile_cols"] == 16
    for wtype in (1, 0):
        w, x, resid = _operands(1000, 384, wtype, seed=99 + wtype, rows=32)
        x = np.concatenate([x] * 16)                                            # 512 rows: every block of 32 must repeat the first
        resid = np.concatenate([resid] * 16)
        assert L.dense_mfma_plan(1000, 384, wtype, 512)["tile_cols"] == 32
        for r in (None, resid):
            want = _run(L, w, x[:32], r, "mv")
            got = _run(L, w, x, r, "mfma")
            assert same(got, np.concatenate([want] * 16)), f"wtype {wtype}, resid {r is not None}"


@pytest.mark.parametrize("wtype", [1, 0], ids=["f16", "f32"])
def test_zeros_signed_zeros_subnormals_and_exact_cancellation(L, wtype):
    """where a flushed denormal, a padded step or a re-ordered fold shows: K 384 (a group + the 4-step tail), M 40, N 17"""
    M, K, N = 40, 384, 17
    w, x, resid = _operands(M, K, wtype, seed=4242 + wtype, rows=N)
    w = w.astype(np.float32)
    step = (np.arange(K) // 32) % 2                                             # chain l = elements l, l + 32, ...: 12 steps each
    w[0] = 0.0; w[1] = -0.0                                                     # all-zero weight rows of either sign
    w[2] = 0.5; w[3] = np.where(step == 0, 0.25, -0.25)                         # constant / alternating by step
    w[4, ::3] = 0.0; w[4, 1::3] = -0.0
    x[0] = 0.0; x[2] = -0.0                                                     # all-zero activation rows
    x[3] = np.where(step == 0, 1.5, -1.5)                                       # x w[2]: every chain +p -p +p ... = +0 exactly
    x[4] = 1.5                                                                  # x w[3]: the same cancellation from the weight side
    x[5, ::2] = 0.0; x[5, 1::5] = -0.0
    if wtype == 0:
        w[5] = 1e-40; w[6] = np.where(step == 0, 3e-39, -2e-39)                 # subnormal weights
        w[7] = 1e-30                                                            # x 1e-30: products that underflow to subnormals / to zero
        w[8, ::2] = 1e-25
        x[7] = 1e-40; x[8] = 1e-30; x[9] = np.where(step == 0, 1e-12, -1e-15)
        x[10, ::7] = 1.4e-45
    else:
        w[5] = 6e-8; w[6] = np.where(step == 0, 3e-6, -2e-6)                    # fp16 subnormals
        w[7] = 6.1e-5                                                           # the smallest normal half
        x[7] = 6e-8; x[8] = 1e-9; x[9] = np.where(step == 0, 6.1e-5, -3e-6)     # activations that round to fp16 subnormals / zero
    w = w.astype(np.float16 if wtype == 1 else np.float32)
    resid[:, 0] = -0.0; resid[0] = 0.0
    for r in (None, resid):
        want = _run(L, w, x, r, "mv")
        if r is None:
            assert want[3, 2] == 0.0 and want[4, 3] == 0.0                      # (the cancellations are exact in the reference chain too)
        got = _run(L, w, x, r, "mfma")
        assert same(got, want), f"wtype {wtype}, resid {r is not None}: outputs {np.argwhere(got.view(np.uint32) != want.view(np.uint32)).tolist()[:8]} differ"


def test_refusals_happen_without_a_launch(L):
    before = L.dense_mfma_launches()
    w, x, _ = _operands(40, 384, 1, seed=3, rows=17)
    with pytest.raises(L.LlamaHipError, match=r"N > 16"):
        L.op_mul_mat_dense(w, x[:16], path="mfma")
    for K in KS_REFUSED:
        wk, xk, _ = _operands(40, K, 1, seed=K, rows=17)
        with pytest.raises(L.LlamaHipError, match=r"multiple of 128"):
            L.op_mul_mat_dense(wk, xk, path="mfma")
    with pytest.raises(L.LlamaHipError, match=r"wtype 3"):
        L.op_mul_mat_dense(w, x, path="mfma", wtype=3)                          # Q4_1 has its own kernel: every path is refused
    assert L.dense_mfma_launches() == before


def test_auto_keeps_mm_where_the_kernel_does_not_take_the_shape(L):
    w, x, _ = _operands(40, 320, 1, seed=5, rows=17)
    assert L.op_mul_mat_dense(w, x)[1] == "mm"
    # ... and whatever the measured rule picks where it does equals the one-row kernel
    w, x, _ = _operands(250, 1280, 1, seed=6, rows=64)
    y, taken = L.op_mul_mat_dense(w, x)
    assert taken in ("mm", "mfma") and taken == ("mfma" if L.dense_mfma_plan(250, 1280, 1, 64)["auto"] else "mm")
    assert same(y, L.op_mul_mat_dense(w, x, path="mv")[0])
