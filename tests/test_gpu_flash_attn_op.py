"""GPU (-m gpu): the opt-in fused attention k_flash_attn alone (llamahip_op_flash_attention) against float64 numpy on the un-rounded fp32
rotated q, K and V, held to the derived bound of tests/flash_ref.py per output.  d 256, H 2 (head size 128), n_ctx 384; both instances
(64- and 128-query tiles) on every case.  Every case is poisoned: cache rows at or past T = n_past + N are NaN in K and V, merged starts
as NaN with rows d + 8 floats apart.  The rotated q is what the exact op appends to the K cache when q is passed in k's place (the same
rotation at the same positions, bit for bit); the appended cache rows are compared with the exact op_attention(path="row")'s.
Measured max error / bound over all cases (the same on both tiles): gaussian 0.053, peaked 0.047, flat 0.31, binades 0.054."""
import functools

import numpy as np
import pytest

from flash_ref import flash_reference

pytestmark = pytest.mark.gpu

D, H, N_CTX, PAD = 256, 2, 384, 8
# (N, n_past, key splits; 0 = the plan's choice)
CASES = [
    (64, 0, 1),
    (65, 0, 1), (127, 1, 1),        # a ragged last query tile
    (130, 63, 1),                   # keys across a tile edge, the diagonal inside a tile
    (64, 200, 0),                   # the long-conversation chunk: the plan splits the keys
    (130, 0, 4),                    # early rows with empty splits
    (64, 255, 3),                   # splits that do not divide the tiles
    (192, 64, 2),
]
REGIMES = ["gaussian", "peaked", "flat", "binades", "saturating"]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@functools.lru_cache(maxsize=None)
def _case(L, N, n_past, regime):
    """the operands, the exact op's caches and the float64 reference of one (case, regime): computed once, shared by both tiles, left unchanged"""
    rng = np.random.default_rng(N * 1000 + n_past * 7 + REGIMES.index(regime))
    T = n_past + N
    qkv = rng.standard_normal((N, 3 * D)).astype(np.float32)
    K0 = rng.standard_normal((N_CTX, D)).astype(np.float32)
    V0 = rng.standard_normal((N_CTX, D)).astype(np.float32)
    if regime == "peaked":          # kq q.k has standard deviation 20: scores span about +-60, one key takes all the weight
        qkv[:, :2 * D] *= np.float32(np.sqrt(20.0))
        K0 *= np.float32(np.sqrt(20.0))
    elif regime == "flat":          # q = 0: the output is the mean of the narrowed v, l is exercised alone
        qkv[:, :D] = 0.0
    elif regime == "binades":       # v over seven binades with random signs
        mag = lambda shape: (rng.choice([-1.0, 1.0], shape) * rng.uniform(1.0, 2.0, shape) * 2.0 ** rng.integers(-4, 3, shape)).astype(np.float32)
        qkv[:, 2 * D:], V0 = mag((N, D)), mag((N_CTX, D))
    elif regime == "saturating":    # entries of 1e6 in q, k and v: beyond the largest finite half
        for a in (qkv, K0, V0):
            a[rng.random(a.shape) < 0.01] = 1e6
            a[rng.random(a.shape) < 0.01] = -1e6
    K0[n_past:], V0[n_past:] = np.nan, np.nan          # rows n_past .. T - 1 are appended by the op, rows >= T must never be loaded
    Kx, Vx = K0.copy(), V0.copy()
    L.op_attention(qkv, H, n_past, Kx, Vx, n_threads=1, path="row", want_wo=False)
    Kq, Vq = K0.copy(), V0.copy()
    q_as_k = qkv.copy()
    q_as_k[:, D:2 * D] = qkv[:, :D]
    L.op_attention(q_as_k, H, n_past, Kq, Vq, n_threads=1, path="row", want_wo=False)
    ref = None if regime == "saturating" else flash_reference(Kq[n_past:T], Kx, Vx, H, n_past)
    for a in (qkv, K0, V0, Kx, Vx):
        a.setflags(write=False)
    return qkv, K0, V0, Kx, Vx, ref


def _run(L, qkv, K0, V0, n_past, tile, ks):
    Kc, Vc = K0.copy(), V0.copy()
    before = L.flash_attn_launches()
    merged, tt, st = L.op_flash_attention(qkv, H, n_past, Kc, Vc, tile=tile, key_splits=ks, merged_stride=D + PAD)
    assert L.flash_attn_launches() - before == (1 if st == 1 else 2)
    return merged, tt, st, Kc, Vc


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("N,n_past,ks", CASES)
def test_flash_attention_within_the_derived_bound(L, N, n_past, ks, tile, regime):
    qkv, K0, V0, Kx, Vx, ref = _case(L, N, n_past, regime)
    T = n_past + N
    merged, tt, st, Kc, Vc = _run(L, qkv, K0, V0, n_past, tile, ks)
    assert tt == tile and st == (ks if ks else L.flash_attn_plan(N, T, H)["key_splits"]) and (ks or st > 1)
    assert np.isnan(merged[:, D:]).all(), "the floats between d and merged_stride must keep the caller's bits"
    assert same(Kc[:n_past], K0[:n_past]) and same(Vc[:n_past], V0[:n_past]), "cache rows before n_past"
    assert same(Kc[n_past:T], Kx[n_past:T]) and same(Vc[n_past:T], Vx[n_past:T]), "appended rows: the exact path's bits"
    assert np.isnan(Kc[T:]).all() and np.isnan(Vc[T:]).all() and same(Kc[T:], K0[T:]) and same(Vc[T:], V0[T:]), "rows at or past T"
    o = merged[:, :D].astype(np.float64)
    assert np.isfinite(o).all(), "an output left unwritten, or a non-finite one"
    if regime == "saturating":
        assert np.abs(o).max() <= 65504.0
        return
    want, bound = ref
    err = np.abs(o - want)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"N {N} n_past {n_past} tile {tile} KS {st} {regime}: max err / bound = {(err / bound).max():.4f}, max err = {err.max():.3e}")
    assert (err <= bound).all(), f"output {worst}: |o - o64| = {err[worst]:.3e} > bound {bound[worst]:.3e} ({int((err > bound).sum())} of {err.size} outputs)"
    if st > 1:      # split and unsplit walks of the same case: not bit-equal by contract, within twice the bound
        one = _run(L, qkv, K0, V0, n_past, tile, 1)[0][:, :D].astype(np.float64)
        assert (np.abs(o - one) <= 2 * bound).all()
