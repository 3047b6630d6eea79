"""GPU (-m gpu): k_q41_act_q + k_q41_dot (llamahip_op_mul_mat_q4_1_dot) against float64 numpy over the un-rounded operands:
    |y - y64| <= gamma(K/32 + 8) * mass + one fp32 ulp,   mass = sum_blocks (|d0 d1| S_qc + |d0 m1| S_q + |m0 d1| S_c + 32 |m0 m1|) + |resid|
Instances of 1, 2, 4, 8, 12, 16 rows; 16 K-lanes; record slabs of 64 blocks up to 4 rows, 32 at 8, 16 from 12."""
import numpy as np
import pytest

from gemm_ref import gamma
from q41_cases import REGIMES, make_weights, split_weights

pytestmark = pytest.mark.gpu

GUARD = 8
F32 = np.float32
CASES = [                   # N, M, K
    (1, 16, 32),            # one workgroup, one row, one block: fifteen K-lanes without a block
    (2, 17, 512),           # instance 2; one weight row over a workgroup; exactly one block per K-lane
    (3, 65, 544),           # instance 4 holding 3 rows; a row-block of 63 zero rows; one block per K-lane + 32
    (4, 33, 2080),          # instance 4 full; 65 blocks: a second slab of one block (slab 64)
    (8, 16, 1376),          # instance 8; 43 blocks: no multiple of the K-lane stride, a second slab of 11 (slab 32)
    (11, 17, 544),          # instance 12 holding 11 rows
    (16, 65, 1056),         # instance 16 full; 33 blocks: a third slab of one block (slab 16)
    (17, 16, 512),          # a second row tile of one row: a launch of instance 16 and one of instance 1
    (63, 33, 288),          # three full tiles on gridDim.y and a tile of 15 rows
    (5, 40, 2048),          # instance 8 holding 5 rows; the largest K: also compared with the exact path's bits
]


def quantize(x):
    """quantize_row_q4_1 (q41_cases.expand_x without its last line): (code int64 [N, nb, 32], d1 f32 [N, nb, 1], m1 f32 [N, nb, 1])"""
    x = np.ascontiguousarray(x, F32)
    N, K = x.shape
    xb = x.reshape(N, K // 32, 32)
    mn, mx = xb.min(axis=2, keepdims=True), xb.max(axis=2, keepdims=True)
    d = ((mx - mn) / F32(15.0)).astype(F32)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, F32(1.0) / np.where(d != 0, d, F32(1.0)), F32(0.0)).astype(F32)
    t = ((xb - mn).astype(F32) * idv).astype(F32)
    return np.floor(t.astype(np.float64) + 0.5).astype(np.int64) & 0xFF & 0xF, d, mn


def check(L, w, x, resid, label):
    M, (N, K) = w.shape[0], x.shape
    m0, d0, qb = split_weights(w, K)
    q = np.stack([qb & 0xF, qb >> 4], axis=2).reshape(M, K // 32, 32).astype(np.int64)      # byte j: elements 2 j (low nibble), 2 j + 1
    c, d1, m1 = quantize(x)
    m0, d0, d1, m1 = m0.astype(np.float64)[None], d0.astype(np.float64)[None], d1.astype(np.float64), m1.astype(np.float64)      # [1, M, nb], [N, 1 -> nb, 1]
    d1, m1 = d1.transpose(0, 2, 1), m1.transpose(0, 2, 1)                                   # [N, 1, nb]
    sqc = np.einsum("mbk,nbk->nmb", q, c).astype(np.float64)
    sq, sc = q.sum(2)[None].astype(np.float64), c.sum(2)[:, None].astype(np.float64)
    parts = (d0 * d1 * sqc, d0 * m1 * sq, m0 * d1 * sc, 32.0 * m0 * m1)
    want, mass = sum(parts).sum(2), sum(np.abs(p) for p in parts).sum(2)
    if resid is not None:
        want, mass = want + resid, mass + np.abs(resid)
    before = L.q41_dot_launches()
    y = L.op_mul_mat_q4_1_dot(w, x, resid, y_stride=M + GUARD)
    assert L.q41_dot_launches() == before + 1
    assert np.isnan(y[:, M:]).all(), "columns past M must keep the caller's NaN"
    y = y[:, :M]
    assert np.isfinite(y).all(), "an output left unwritten"
    bound = gamma(K // 32 + 8) * mass + np.spacing(np.abs(want).astype(F32)).astype(np.float64)
    err = np.abs(y.astype(np.float64) - want)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"{label} N {N} M {M} K {K} resid {resid is not None}: max err / bound = {(err / bound).max():.4f}, max err = {err.max():.3e}")
    assert (err <= bound).all(), f"output {worst}: |y - y64| = {err[worst]:.3e} > bound {bound[worst]:.3e} ({int((err > bound).sum())} of {err.size} outputs)"
    return y


def inputs(N, M, K):
    rng = np.random.default_rng(N * 31 + M + K)
    return make_weights(M, K, seed=N + M + K), (rng.standard_normal((N, K)) * 2.0 ** rng.integers(-3, 3, (N, 1))).astype(F32), rng


@pytest.mark.parametrize("N,M,K", CASES)
@pytest.mark.parametrize("with_resid", [False, True], ids=["store", "resid"])
def test_dot_mat_mul_within_the_derived_bound(L, N, M, K, with_resid):
    assert L.q41_dot_plan(M, K, N)["nr"] >= min(N % 16 or 16, 16)
    w, x, rng = inputs(N, M, K)
    r = (4.0 * rng.standard_normal((N, M))).astype(F32) if with_resid else None
    y = check(L, w, x, r, "case")
    if K == max(c[2] for c in CASES):
        exact = L.op_mul_mat_q4_1(w, x, r)[0]
        assert not np.array_equal(y.view(np.uint32), exact.view(np.uint32)), "bit-equal to the exact path: the dot kernel did not run"


@pytest.mark.parametrize("regime", REGIMES)
def test_value_regimes(L, regime):
    M, K, N = 33, 256, 5
    w = make_weights(M, K, seed=4301, d_zero_every=3 if regime == "d_zero" else 0, neg_min=regime == "neg_min")
    x = np.random.default_rng(4302).standard_normal((N, K)).astype(F32)
    if regime == "equal_block":             # an activation block of 32 equal values: d1 = 0, id = 0
        x[1, 64:96] = F32(0.375)
        x[2, 0:32] = F32(-1.25)
    elif regime == "outlier":               # one value 1e4 times the rest: the codes collapse to 0 / 15
        x[0, 37] = F32(1.0e4)
        x[2, 200] = F32(-1.0e4)
    elif regime == "neg_min":               # negative min on both sides
        x = (-np.abs(x) - F32(0.5)).astype(F32)
    check(L, w, x, None, regime)


@pytest.mark.parametrize("N,n", [(2, 1), (3, 0), (9, 4), (16, 7), (17, 16), (63, 62)])
def test_a_row_does_not_depend_on_the_rows_around_it(L, N, n):
    w, x, _ = inputs(N, 33, 1056)
    many, one = L.op_mul_mat_q4_1_dot(w, x), L.op_mul_mat_q4_1_dot(w, x[n:n + 1])
    assert np.array_equal(many[n].view(np.uint32), one[0].view(np.uint32)), f"row {n} of {N} differs in bits from the one-row call"
