"""GPU (-m gpu): the opt-in fp16 matrix-core mat-mul k_dense_f16_fast alone (llamahip_op_mul_mat_f16_fast) against float64 numpy on the same
fp16-rounded operands.  The kernel re-associates the sum, so it is held to a derived bound, not to bits: every product is exact, each
output is one fp32 sum of K terms in an unknown order plus one residual add --
    |y - y64| <= gamma(K + 1) * (sum_k |w x| + |resid|) + one fp32 ulp of the result.
Operands have random signs and magnitudes over seven binades: the bound is ~1e-5 of sum |w x| while one missing product is ~1 / K of it,
so a missing tile, a swapped operand half or a dropped K tail fails by orders of magnitude.
Cases (N, M, K) walk the three instances (dense_fast_plan): narrow 64 x 16 rows, K tile 256; mid 64 x 64, K tile 128; wide 128 x 128, K
tile 64.  Per instance: one tile / one row over a tile; a ragged N whose last workgroup has a wave partly and a wave wholly past N; M one
over a tile; K one tile, two tiles + 32, and a multiple of 32 that is no multiple of the tile."""
import numpy as np
import pytest

from gemm_ref import gamma

pytestmark = pytest.mark.gpu

GUARD = 8
CASES = [
    (64, 16, 256, "narrow"),        # one workgroup, one K tile
    (65, 17, 544, "narrow"),        # one row over both tiles; K = two tiles + 32
    (89, 40, 1376, "narrow"),       # rows 80 .. 88 in wave 1, waves 2 and 3 past N; K = 5 tiles + 96 (11008 scaled down)
    (64, 8129, 128, "mid"),         # the first M at which 64 rows take the mid tile; one K tile; M = 127 tiles + 1
    (89, 4033, 288, "mid"),         # second workgroup row: one wave pair partly, one wholly past N; K = two tiles + 32
    (150, 16257, 160, "wide"),      # rows 128 .. 149 partly, 192 .. 255 wholly past N; M = 127 tiles + 1; K = two tiles + 32
    (130, 250, 2048, "narrow"),     # the largest K: also compared with the exact path's bits
]
TILE = {"narrow": (64, 16, 256), "mid": (64, 64, 128), "wide": (128, 128, 64)}


def _operands(N, M, K, seed):
    rng = np.random.default_rng(seed)
    mag = lambda shape: rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 2.0, shape) * 2.0 ** rng.integers(-4, 3, shape)
    w = (0.25 * mag((M, K))).astype(np.float16)
    x = mag((N, K)).astype(np.float32)
    resid = (4.0 * mag((N, M))).astype(np.float32)
    return w, x, resid


@pytest.mark.parametrize("N,M,K,instance", CASES)
@pytest.mark.parametrize("with_resid", [False, True], ids=["store", "resid"])
def test_fast_mat_mul_within_the_summation_bound(L, N, M, K, instance, with_resid):
    plan = L.dense_fast_plan(M, K, N)
    assert (plan["tile_rows"], plan["tile_cols"], plan["k_tile"]) == TILE[instance]
    w, x, resid = _operands(N, M, K, seed=N * 31 + M + K)
    r = resid if with_resid else None
    before = L.dense_fast_launches()
    y = L.op_mul_mat_f16_fast(w, x, r, y_stride=M + GUARD)
    assert L.dense_fast_launches() == before + 1
    assert np.isnan(y[:, M:]).all(), "columns past M must keep the caller's bits"
    y = y[:, :M]
    assert np.isfinite(y).all(), "an output left unwritten"
    w64, x64 = w.astype(np.float64), x.astype(np.float16).astype(np.float64)      # act(x): RNE to fp16, as the reference's mat-mul
    want, mass = x64 @ w64.T, np.abs(x64) @ np.abs(w64).T
    if with_resid:
        want, mass = want + resid, mass + np.abs(resid)
    bound = gamma(K + 1) * mass + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(y.astype(np.float64) - want)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"N {N} M {M} K {K} {instance} resid {with_resid}: max err / bound = {(err / bound).max():.4f}, max err = {err.max():.3e}, "
          f"smallest |product| scale = {mass.min() / K:.3e}")
    assert (err <= bound).all(), f"output {worst}: |y - y64| = {err[worst]:.3e} > bound {bound[worst]:.3e} ({int((err > bound).sum())} of {err.size} outputs)"
    if K == max(c[2] for c in CASES):
        exact = L.op_mul_mat_dense(w, x, r)[0]
        assert not np.array_equal(y.view(np.uint32), exact.view(np.uint32)), "bit-equal to the exact path: the fast kernel did not run"
