"""GPU (-m gpu): k_q40_dot (llamahip_op_gemv_q4_0_dot) against a host restatement of its stated arithmetic, bit for bit, and against float64
numpy over the un-rounded operands:
    |y - y64| <= gamma(K/32 + 4) * mass + one fp32 ulp,   mass = sum_blocks |d_w d_a| sum |q c| + |resid|
Two roundings per block term, at most K/32 adds on a term's way out (its slice's later blocks, then the other slices), one residual add.
The extremes regime reaches |isum| = 1792, not 2048: quantize_row_q4_0 produces activation codes - 8 in -7 .. 7 (32 * 8 * 7)."""
import functools

import numpy as np
import pytest

from gemm_ref import gamma, split

pytestmark = pytest.mark.gpu

GUARD = 8
F32, F64 = np.float32, np.float64
KS = [32, 256, 288, 2304, 11008]    # one padded block | fewer chunks than slices | a ragged chunk | 9 chunks over 8 slices | 7B's w2
MS = [8, 9, 24, 4096]               # one row-group read twice | a ragged second group | a second workgroup of one group | 7B's width

def quantize(x):
    """quantize_row_q4_0 as the activation kernels run it (ggml.c:456-523): (code - 8 int32 [nb, 32], d float32 [nb])"""
    xb = np.ascontiguousarray(x, F32).reshape(-1, 32)
    amax = np.abs(xb).max(axis=1, keepdims=True)
    idv = np.where(amax != 0, F32(7.0) / np.where(amax != 0, amax, F32(1.0)), F32(0.0)).astype(F32)
    return np.rint((xb * idv).astype(F32)).astype(np.int32), (amax / F32(7.0)).astype(F32)[:, 0]

def fma32(a, b, c):
    """fmaf on float32 arrays, |a| an integer below 2^12: a b is exact in float64; the sum is rounded to odd there (TwoSum), so that the
    narrowing to float32 is the one rounding of the exact a b + c"""
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)

def stated(w, x, resid):
    """the header of csrc/q40_dot.hip in numpy: (y float32 [M], parts float64 [ceil(M / 16), 2]) and the float64 yardstick (y64, mass)"""
    M, nb = w.shape[0], w.shape[1]
    dw, q = split(w)
    c, da = quantize(x)
    isum = (q.astype(np.int32) * c[None]).sum(2)                            # [M, nb], exact
    term = dw * da.astype(F64)[None] * isum
    y64, mass = term.sum(1), np.abs(dw * da.astype(F64)[None] * (np.abs(q.astype(np.int32)) * np.abs(c)[None]).sum(2)).sum(1)
    nchunks = -(-nb // 8)
    S = 8 if -(-M // 16) <= 512 else 4
    fi = np.zeros((M, nchunks * 8), F32)                                    # (float) isum and fl(d_w * d_a), blocks of the padding: 0, 0
    sc = np.zeros((M, nchunks * 8), F32)
    fi[:, :nb], sc[:, :nb] = isum.astype(F32), dw.astype(F32) * da[None]
    y = None
    for s in range(S):
        acc = np.zeros(M, F32)
        for ch in range(s, nchunks, S):
            for b in range(ch * 8, ch * 8 + 8):
                acc = fma32(fi[:, b], sc[:, b], acc)
        y = acc if y is None else y + acc
    if resid is not None:
        y = y + resid
        y64, mass = y64 + resid, mass + np.abs(resid)
    G = -(-M // 16)
    yd = np.zeros(G * 16)
    yd[:M] = y
    tree = lambda v: functools.reduce(lambda a, _: a[:, 0::2] + a[:, 1::2], range(4), v.reshape(G, 16))[:, 0]
    return y, np.stack([tree(yd), tree(yd * yd)], axis=1), y64, mass

@functools.lru_cache(maxsize=2)
def inputs(M, K):
    """gaussian weights as Q4_0 file bytes (codes drawn directly: the offline quantizer takes seconds at 4096 x 11008), x, resid"""
    rng = np.random.default_rng(M * 31 + K)
    nb = K // 32
    v = (np.clip(np.rint(rng.standard_normal((M, nb, 32), F32) * F32(2.5)), -8, 7) + 8).astype(np.uint8)
    w = np.empty((M, nb, 20), np.uint8)
    w[:, :, :4] = (np.abs(rng.standard_normal((M, nb), F32)) * 2.0 ** rng.integers(-6, -1, (M, 1))).astype(F32).view(np.uint8).reshape(M, nb, 4)
    w[:, :, 4:] = v[:, :, 0::2] | (v[:, :, 1::2] << 4)
    return w, (rng.standard_normal(K) * 4.0).astype(F32), (4.0 * rng.standard_normal(M)).astype(F32)

def check(L, w, x, resid, label):
    M, K = w.shape[0], x.shape[0]
    G = -(-M // 16)
    want, want_parts, y64, mass = stated(w, x, resid)
    before = L.q40_dot_launches()
    y, parts = L.op_gemv_q4_0_dot(w, x, resid, y_cap=M + GUARD, parts_cap=G + 2)
    assert L.q40_dot_launches() == before + 1
    assert np.isnan(y[M:]).all() and np.isnan(parts[G:]).all(), "floats past M and pairs past the grid must keep the caller's NaN"
    y, parts = y[:M], parts[:G]
    assert np.isfinite(y).all() and np.isfinite(parts).all(), "an output left unwritten"
    bound = gamma(K // 32 + 4) * mass + np.spacing(np.abs(y64).astype(F32)).astype(F64)
    err = np.abs(y.astype(F64) - y64)
    print(f"{label} M {M} K {K} resid {resid is not None}: max err / bound = {(err / bound).max():.4f}, bits differ in {int((y.view(np.uint32) != want.view(np.uint32)).sum())} of {M}")
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), f"y is not the stated arithmetic's bits (first at row {int(np.argmax(y.view(np.uint32) != want.view(np.uint32)))})"
    assert (err <= bound).all(), f"|y - y64| above the bound in {int((err > bound).sum())} of {M} outputs"
    assert np.array_equal(parts.view(np.uint64), want_parts.view(np.uint64)), "parts are not {sum y, sum y^2} of the stored y in the stated order"

@pytest.mark.parametrize("with_resid", [False, True], ids=["store", "resid"])
@pytest.mark.parametrize("M,K", [(M, K) for M in MS for K in KS] + [(8200, 288)])          # 8200: above 8192 rows, 4 slices
def test_the_stated_arithmetic_and_the_bound(L, M, K, with_resid):
    assert L.q40_dot_plan(M, K)["slices"] == (8 if M <= 8192 else 4)
    w, x, r = inputs(M, K)
    check(L, w, x, r if with_resid else None, "case")

@pytest.mark.parametrize("regime", ["extremes", "zero_scales"])
def test_value_regimes(L, regime):
    w, x, r = (a.copy() for a in inputs(24, 2304))
    if regime == "extremes":                # every weight code 0 (value -8), every activation code +-7: |isum| = 1792 in every block
        w[:, :, 4:] = 0
        x = np.where(np.arange(x.size) // 32 % 2 == 0, F32(3.0), F32(-3.0)).astype(F32)
    else:                                   # weight blocks of scale 0 (codes kept), all-zero activation blocks (d_a = 0), a whole zero row of scales
        w[::3, 2, :4] = 0
        w[5, :, :4] = 0
        x[64:96] = 0.0
        x[512:1024] = 0.0
    check(L, w, x, r, regime)
