"""GPU (-m gpu): k_q40_few (llamahip_op_mul_mat_q4_0_few) against float64 numpy over the un-rounded operands:
    |y - y64| <= gamma(K/32 + 4) * mass + one fp32 ulp,   mass = sum_blocks |d_w d_a| sum |q c| + |resid|
Two roundings per block term, at most K/32 adds on a term's way out (its slice's later blocks, then the other slices), one residual add.
NT = 1 .. 4 column tiles of 16; 8 K-slices of whole chunks (256 elements) up to 8192 weight rows, 4 above.  Measured: max err / bound
0.0008 .. 0.12 over the cases, 0.023 .. 0.18 over the regimes (the outlier)."""
import numpy as np
import pytest

import synth
from gemm_ref import gamma, split

pytestmark = pytest.mark.gpu

GUARD = 8
F32 = np.float32
CASES = [                   # N, M, K
    (1, 16, 32),            # one row, one workgroup of one tile, one block: seven slices without a chunk, seven blocks of padding
    (2, 17, 544),           # a tile group read twice; 17 blocks = 3 chunks, the last of one block: fewer chunks than slices
    (15, 33, 288),          # NT 1 holding 15 rows; a ragged third row tile of weights; 9 blocks
    (16, 16, 2304),         # NT 1 full; 9 chunks: slice 0 takes a second chunk
    (17, 33, 800),          # NT 2 with a last tile of one row; 25 blocks
    (33, 17, 544),          # NT 3 with a last tile of one row
    (63, 33, 1056),         # NT 4
    (3, 8200, 1312),        # above 8192 weight rows: 4 slices of 2, 2, 1, 1 chunks
    (5, 33, 4416),          # 18 chunks: slices 0 and 1 take a third (the ring's second turn); also compared with the exact path's bits
]

def quantize(x):
    """quantize_row_q4_0 as the activation kernels run it (ggml.c:456-523): (code int64 [N, nb, 32], d float64 [N, nb])"""
    xb = np.ascontiguousarray(x, F32).reshape(x.shape[0], -1, 32)
    amax = np.abs(xb).max(axis=2, keepdims=True)
    with np.errstate(divide="ignore"):
        idv = np.where(amax != 0, F32(7.0) / np.where(amax != 0, amax, F32(1.0)), F32(0.0)).astype(F32)
    return np.rint((xb * idv).astype(F32)).astype(np.int64), (amax / F32(7.0)).astype(F32)[..., 0].astype(np.float64)

def check(L, w, x, resid, label):
    M, (N, K) = w.shape[0], x.shape
    dw, q = split(w)
    c, da = quantize(x)
    q = q.astype(np.int64)
    s = dw[None] * da[:, None]                                              # [N, M, nb]
    want = (s * np.einsum("mbk,nbk->nmb", q, c)).sum(2)
    mass = (np.abs(s) * np.einsum("mbk,nbk->nmb", np.abs(q), np.abs(c))).sum(2)
    if resid is not None:
        want, mass = want + resid, mass + np.abs(resid)
    before = L.q40_few_launches()
    y = L.op_mul_mat_q4_0_few(w, x, resid, y_stride=M + GUARD)
    assert L.q40_few_launches() == before + 1
    assert np.isnan(y[:, M:]).all(), "columns past M must keep the caller's NaN"
    y = y[:, :M]
    assert np.isfinite(y).all(), "an output left unwritten"
    bound = gamma(K // 32 + 4) * mass + np.spacing(np.abs(want).astype(F32)).astype(np.float64)
    err = np.abs(y.astype(np.float64) - want)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"{label} N {N} M {M} K {K} resid {resid is not None}: max err / bound = {(err / bound).max():.4f}, max err = {err.max():.3e}")
    assert (err <= bound).all(), f"output {worst}: |y - y64| = {err[worst]:.3e} > bound {bound[worst]:.3e} ({int((err > bound).sum())} of {err.size} outputs)"
    return y

def inputs(N, M, K):
    rng = np.random.default_rng(N * 31 + M + K)
    w = synth.quantize_q4_0_offline((rng.standard_normal((M, K)) * 2.0 ** rng.integers(-4, 1, (M, 1))).astype(F32))
    return w, (rng.standard_normal((N, K)) * 2.0 ** rng.integers(-3, 3, (N, 1))).astype(F32), rng

@pytest.mark.parametrize("N,M,K", CASES)
@pytest.mark.parametrize("with_resid", [False, True], ids=["store", "resid"])
def test_few_mat_mul_within_the_derived_bound(L, N, M, K, with_resid):
    p = L.q40_few_plan(M, K, N)
    assert p["nt"] == -(-N // 16) and p["slices"] == (8 if M <= 8192 else 4)
    w, x, rng = inputs(N, M, K)
    r = (4.0 * rng.standard_normal((N, M))).astype(F32) if with_resid else None
    y = check(L, w, x, r, "case")
    if K == max(c[2] for c in CASES):
        exact = L.op_gemv_set_q4_0(w, "resid" if with_resid else "store", x, resid=r)["y"]
        assert not np.array_equal(y.view(np.uint32), exact.view(np.uint32)), "bit-equal to the exact path: the few-row kernel did not run"

@pytest.mark.parametrize("regime", ["d_zero", "zero_block", "outlier", "negative"])
def test_value_regimes(L, regime):
    w, x, _ = inputs(5, 33, 256)
    if regime == "d_zero":                  # weight blocks of scale 0 (codes kept)
        w[::3, 2, :4] = 0
        w[5, :, :4] = 0
    elif regime == "zero_block":            # an all-zero activation block: d_a = 0, id = 0
        x[1, 64:96] = 0.0
        x[2, :] = 0.0
    elif regime == "outlier":               # one value 1e4 times the rest: every other code of the block collapses
        x[0, 37] = F32(1.0e4)
        x[2, 200] = F32(-1.0e4)
    else:
        x = (-np.abs(x) - F32(0.5)).astype(F32)
    check(L, w, x, None, regime)

@pytest.mark.parametrize("N,n", [(2, 1), (16, 7), (17, 16), (33, 32), (63, 62)])
def test_a_row_does_not_depend_on_the_rows_around_it(L, N, n):
    w, x, _ = inputs(N, 33, 1056)
    many, one = L.op_mul_mat_q4_0_few(w, x), L.op_mul_mat_q4_0_few(w, x[n:n + 1])
    assert np.array_equal(many[n].view(np.uint32), one[0].view(np.uint32)), f"row {n} of {N} differs in bits from the one-row call"
