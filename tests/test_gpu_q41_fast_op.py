"""GPU (-m gpu): the opt-in fp16 matrix-core Q4_1 mat-mul (k_q41_act_f16 + k_q41_fast, llamahip_op_mul_mat_q4_1_fast) against float64 numpy over
the STATED narrowed operands: f^ = float16(fl(fl(d0 q) + m0)), a^ = float16(expand_x(x)) (numpy's cast rounds to nearest even), reference
a^64 @ f^64.T (+ resid).  Every product is exact in fp32 and an output is one fp32 sum of K terms in an unknown order plus one residual add:
    |y - y64| <= gamma(K + 1) * (sum_k |f^ a^| + |resid|) + one fp32 ulp of the result + sum of |f^ a^| over products with an fp16-subnormal factor
(the last term: whether the narrowing or the matrix core flushes a subnormal input is not part of the contract; such a product may be counted
or dropped).  One wrong activation code moves an output by d1 |f| ~ 1e-2 .. 1e-1 against a bound of ~1e-4: an order of magnitude and more.
Cases walk the three instances (q41_fast_plan): per instance one tile (narrow) or the fewest tiles the rule gives it, one row over a tile in
N and in M (M no multiple of 64), a ragged N whose last workgroup has a wave partly and a wave wholly past N, K of one tile, two tiles + 32
and a multiple of 32 that is no multiple of the tile."""
import numpy as np
import pytest

from gemm_ref import gamma
from q41_cases import REGIMES, expand_x, make_weights, split_weights

pytestmark = pytest.mark.gpu

GUARD = 8
F32 = np.float32
CASES = [
    (64, 16, 256, "narrow"),        # one workgroup, one K tile
    (65, 17, 544, "narrow"),        # one row over both tiles; K = two tiles + 32
    (89, 40, 1376, "narrow"),       # rows 80 .. 88 in wave 1, waves 2 and 3 past N; K = 5 tiles + 96
    (64, 16321, 128, "mid"),        # the first M at which 64 rows take the mid tile; one K tile; M = 255 tiles + 1
    (89, 8129, 288, "mid"),         # second workgroup row: one wave pair partly, one wholly past N; K = two tiles + 32; M = 127 tiles + 1
    (65, 16300, 160, "mid"),        # one row over the tile in N; M = 254 tiles + 44; K no multiple of the tile
    (128, 32768, 64, "wide"),       # one row tile, one K tile
    (150, 16257, 160, "wide"),      # rows 128 .. 149 partly, 192 .. 255 wholly past N; M = 127 tiles + 1 (an odd count of 64-row blocks); K = two tiles + 32
    (129, 16300, 96, "wide"),       # one row over the tile in N; M no multiple of 64; K no multiple of the tile
    (130, 250, 2048, "narrow"),     # the largest K: also compared with the exact path's bits
]
TILE = {"narrow": (64, 16, 256), "mid": (64, 64, 128), "wide": (128, 128, 64)}


def narrowed(w, x):
    """the stated operands: (f^ [M, K], a^ [N, K]) as float16, after checking that saturation cannot enter"""
    K = x.shape[1]
    mn, d, q = split_weights(w, K)
    code = np.stack([q & 0xF, q >> 4], axis=2).reshape(q.shape[0], K).astype(F32)      # byte j: elements 2 j (low nibble), 2 j + 1
    f32 = ((np.repeat(d, 32, axis=1) * code).astype(F32) + np.repeat(mn, 32, axis=1)).astype(F32)
    a32 = expand_x(x)
    assert np.abs(f32).max() < 65504 and np.abs(a32).max() < 65504, "the inputs must stay clear of fp16 saturation"
    return f32.astype(np.float16), a32.astype(np.float16)


def check(L, w, x, resid, K, label):
    M, N = w.shape[0], x.shape[0]
    fh, ah = narrowed(w, x)
    before = L.q41_fast_launches()
    y = L.op_mul_mat_q4_1_fast(w, x, resid, y_stride=M + GUARD)
    assert L.q41_fast_launches() == before + 1
    assert np.isnan(y[:, M:]).all(), "columns past M must keep the caller's bits"
    y = y[:, :M]
    assert np.isfinite(y).all(), "an output left unwritten"
    f64, a64 = fh.astype(np.float64), ah.astype(np.float64)
    fa, aa = np.abs(f64), np.abs(a64)
    fsub, asub = (fa > 0) & (fa < 2.0 ** -14), (aa > 0) & (aa < 2.0 ** -14)
    want, mass = a64 @ f64.T, aa @ fa.T
    sub = (aa * asub) @ fa.T + (aa * ~asub) @ (fa * fsub).T
    if resid is not None:
        want, mass = want + resid, mass + np.abs(resid)
    bound = gamma(K + 1) * mass + np.spacing(np.abs(want).astype(F32)).astype(np.float64) + sub
    err = np.abs(y.astype(np.float64) - want)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"{label} N {N} M {M} K {K} resid {resid is not None}: max err / bound = {(err / bound).max():.4f}, max err = {err.max():.3e}, "
          f"subnormal term max = {sub.max():.3e}")
    assert (err <= bound).all(), f"output {worst}: |y - y64| = {err[worst]:.3e} > bound {bound[worst]:.3e} ({int((err > bound).sum())} of {err.size} outputs)"
    return y


@pytest.mark.parametrize("N,M,K,instance", CASES)
@pytest.mark.parametrize("with_resid", [False, True], ids=["store", "resid"])
def test_fast_mat_mul_within_the_summation_bound(L, N, M, K, instance, with_resid):
    plan = L.q41_fast_plan(M, K, N)
    assert (plan["tile_rows"], plan["tile_cols"], plan["k_tile"]) == TILE[instance]
    rng = np.random.default_rng(N * 31 + M + K)
    w = make_weights(M, K, seed=N + M + K)
    x = (rng.standard_normal((N, K)) * 2.0 ** rng.integers(-3, 3, (N, 1))).astype(F32)
    r = (4.0 * rng.standard_normal((N, M))).astype(F32) if with_resid else None
    y = check(L, w, x, r, K, instance)
    if K == max(c[2] for c in CASES):
        exact = L.op_mul_mat_q4_1(w, x, r)[0]
        assert not np.array_equal(y.view(np.uint32), exact.view(np.uint32)), "bit-equal to the exact path: the fast kernel did not run"


@pytest.mark.parametrize("regime", REGIMES)
def test_value_regimes(L, regime):
    M, K, N = 33, 256, 5
    w = make_weights(M, K, seed=4201, d_zero_every=3 if regime == "d_zero" else 0, neg_min=regime == "neg_min")
    x = np.random.default_rng(4202).standard_normal((N, K)).astype(F32)
    if regime == "equal_block":             # an activation block of 32 equal values: d1 = 0, id = 0
        x[1, 64:96] = F32(0.375)
        x[2, 0:32] = F32(-1.25)
    elif regime == "outlier":               # one value 1e4 times the rest: the codes collapse to 0 / 15
        x[0, 37] = F32(1.0e4)
        x[2, 200] = F32(-1.0e4)
    elif regime == "neg_min":               # negative min on both sides
        x = (-np.abs(x) - F32(0.5)).astype(F32)
    check(L, w, x, None, K, regime)
