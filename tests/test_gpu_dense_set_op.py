"""GPU (-m gpu): the few-row f16 / f32 mat-mul k_dense_set alone (llamahip_op_mul_mat_dense, path SET), bit for bit against the one-row kernel
k_dense_mv run on each row (path MV: the kernel tests/test_gpu_dense_mv_op.py pins op by op to the reference's ggml_vec_dot_f16 / _f32);
k_dense_mm (path MM) must equal it too.

K walks the structures of the kernel's loop:  256 one group | 320 a group + a 2-step tail | 896 three groups + a 4-step tail | 1344 five groups
+ a tail (an odd number of slabs: the second half of the last double iteration is a clamped re-read) | 4096 whole double iterations | 11008 43
groups.  M: 40 a partial workgroup, 250 a row tail inside a half-wave, 1024 full.  Every row count 2 .. 16 at K 1344, M 250 (every compiled
instance, with and without a padded row); 2, 9, 16 elsewhere.  Store and residual epilogues; y rows M + 8 apart with NaN guard columns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (256, 320, 896, 1344, 4096, 11008)
MS = (40, 250, 1024)
GUARD = 8


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _operands(M, K, wtype, seed):
    """weights of the synthetic models' scale (sigma 0.02), 16 activation rows of a normed row's scale, rows 1, 6, 11 with a DC offset"""
    rng = np.random.default_rng(seed)
    w = (0.02 * rng.standard_normal((M, K))).astype(np.float16 if wtype == 1 else np.float32)
    x = rng.standard_normal((16, K)).astype(np.float32)
    x[1] += 3.0; x[6] -= 1.5; x[11] += 0.25
    resid = rng.standard_normal((16, M)).astype(np.float32)
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
def test_set_and_mm_equal_the_one_row_kernel(L, wtype, K):
    before = L.dense_paths()
    n_set = 0
    for M in (MS if K != 11008 else (40,)):
        w, x, resid = _operands(M, K, wtype, seed=K * 7 + M + wtype)
        for r in (None, resid):
            want = _run(L, w, x, r, "mv")                                       # 16 rows, one launch of k_dense_mv each
            for N in (range(2, 17) if (K, M) == (1344, 250) else (2, 9, 16)):
                for path in ("set", "mm"):
                    got = _run(L, w, x[:N], r, path)
                    assert same(got, want[:N]), f"{path} vs mv: wtype {wtype}, M {M}, K {K}, N {N}, resid {r is not None}: " \
                                                f"{int((got != want[:N]).sum())} of {got.size} outputs differ"
                n_set += 1
    after = L.dense_paths()
    assert after["set"] - before["set"] == n_set and after["mm"] - before["mm"] == n_set, (before, after)


def test_auto_sends_one_row_to_the_decode_kernel_and_many_to_mm(L):
    w, x, _ = _operands(40, 320, 1, seed=5)
    xx = np.concatenate([x, x])[:17]
    assert L.op_mul_mat_dense(w, x[:1])[1] == "mv"
    y17, taken = L.op_mul_mat_dense(w, xx)
    assert taken == "mm"
    assert L.op_mul_mat_dense(w, x[:9])[1] in ("set", "mm")                      # (the measured rule: DESIGN.md 12.16)
    y1, taken = L.op_mul_mat_dense(w, x[:1], path="set")                         # one row on the few-row kernel (a padded second row)
    assert taken == "set" and same(y1, y17[:1])
