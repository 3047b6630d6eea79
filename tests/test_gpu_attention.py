"""GPU: every attention path of a layer, op by op (llamahip_op_attention), against the oracle bit for bit and against float64.

Each case appends the eval's rows to K / V caches whose later rows hold a NaN canary (tests/attn_cases.py), runs ONE path, and asserts
  1. merged rows equal orc_attention's bit for bit (the sign of zero and NaN payloads count), and merged columns >= d keep their canary;
  2. the caches equal the oracle's after its append, every bit of them: new rows n_past .. T-1 rotated as orc_rope does, the rest untouched;
  3. SHORT / DEC / DEC_STREAM: the wo operand they write equals orc_quantize_row_q4_0 of the oracle's merged rows byte for byte;
  4. merged stays within a bound of softmax(QK^T scale + mask) V evaluated in float64 on the same rotated operands.
Every path a shape admits runs on it, so paths that share a shape also agree with each other.

The float64 bound.  Per (head, query): s_t = scale * sum_i k_ti q_i; the kernels' fp32 score has |s^_t - s_t| <= ds_t = gamma_(dh/32+6) *
scale * sum_i |k_ti q_i| + 2^-23 |s_t| (32 FMA chains of dh/32 terms, a 5-level tree, the scale's rounding).  x_t = s_t - max is rounded
to fp16 (relative 2^-11) and looked up in the exp table (exp rounded to f32, then to fp16: 2^-11 + 2^-23): the kernel's
e^_t = e_t exp(+-dx_t)(1 +- (2^-11 + 2^-23)) +- 2^-25 with dx_t = 2^-11 (|x_t| + ds_t + ds_max) + ds_t + ds_max; the absolute term covers
entries that land among the fp16 subnormals or at 0.  The row maximum's entry is exactly 1, so sum e >= 1 and the double sum's error is
E = sum_t (e_t r_t + 2^-25) with r_t = expm1(dx_t) + 2^-11 + 2^-23.  Then |p^_t - p_t| <= p_t (r_t + E / (sum e - E) + 2^-22) + 2^-25 / sum e,
and the V*P chains and the ordered merge add gamma_(T + nth) sum_t p^_t |v_t|, plus 2^-150 per operation where a product or sum falls
among the fp32 subnormals.  The test allows 1.25 times sum_t |v_t| |p^_t - p_t| + gamma_(T + nth) sum_t p_t |v_t| + (T + nth) 2^-150.
On ordinary rows dropping the largest key moves some column of every (row, head) by more than 10 times that bound (more than 20 times
in 99 % of them): test_float64_bound_would_catch_one_dropped_key."""
import numpy as np
import pytest

import attn_cases
from attn_ref import f64_reference

pytestmark = pytest.mark.gpu


def describe(got, want, H):
    """first differing (row, head, column) of two merged arrays, by bit pattern"""
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(gb != wb)
    if not len(bad):
        return "equal"
    n, c = bad[0]
    dh = want.shape[1] // H
    return (f"{len(bad)} elements differ; first: row {n}, head {c // dh}, column {c % dh}: got {got[n, c]!r} ({gb[n, c]:#010x}), "
            f"want {want[n, c]!r} ({wb[n, c]:#010x})")


def run(L, oracle, paths, regime, N, H, dh, n_past, n_ctx, nth, chunk=0, ws_rows=0, extra=8, f64=True):
    d = H * dh
    qkv, Kc, Vc = attn_cases.make(regime, N, d, H, n_past, n_ctx, seed=11)
    want, Kw, Vw, qr = attn_cases.oracle_side(oracle, qkv, Kc, Vc, H, n_past, nth, chunk)
    wo_want = np.stack([oracle.quantize_row(r) for r in want]).reshape(N, d // 32, 20)
    canary = np.full((N, d + extra), attn_cases.CANARY, np.uint32).view(np.float32)
    taken = {}
    for path in paths:
        Kg, Vg = Kc.copy(), Vc.copy()
        merged, wo, name = L.op_attention(qkv, H, n_past, Kg, Vg, nth, chunk, path, ws_rows, d + extra, canary)
        taken[path] = name
        tag = f"{path}->{name} {regime} N={N} H={H} dh={dh} n_past={n_past} n_ctx={n_ctx} nth={nth} chunk={chunk} ws_rows={ws_rows}"
        assert np.array_equal(merged[:, :d].view(np.uint32), want.view(np.uint32)), f"{tag}: merged: {describe(merged[:, :d], want, H)}"
        assert np.all(merged[:, d:].view(np.uint32) == attn_cases.CANARY), f"{tag}: merged columns >= d written"
        for nm, got, exp in (("K", Kg, Kw), ("V", Vg, Vw)):
            bad = np.argwhere(got.view(np.uint32) != exp.view(np.uint32))
            assert not len(bad), f"{tag}: {nm} cache: {len(bad)} words differ, first at row {bad[0][0]} column {bad[0][1]} (T = {n_past + N})"
        if name in ("short", "dec", "dec_stream"):
            assert wo is not None and np.array_equal(wo, wo_want), f"{tag}: wo operand differs in {np.argwhere(wo != wo_want)[:1]}"
    if f64:
        ref64, bound, _ = f64_reference(qr, Kw, Vw, H, n_past, nth)
        err = np.abs(want.astype(np.float64) - ref64)
        assert np.all(err <= bound), f"{regime}: float64 bound exceeded at {np.argwhere(err > bound)[:3]}"
    return taken


# (regime, N, H, n_past, n_ctx, n_threads, chunk, ws_rows) at head size 128: MFMA, and AUTO's pick, and k_attn
MFMA_CASES = [
    ("plain", 2, 1, 0, 8, 1, 0, 0), ("plain", 15, 2, 1, 64, 3, 0, 0), ("ties", 16, 4, 31, 47, 8, 0, 0), ("plain", 17, 1, 200, 300, 8, 0, 0),
    ("wide", 63, 2, 0, 63, 3, 0, 0), ("negzero", 64, 1, 1, 80, 1, 0, 0), ("leak", 65, 2, 31, 96, 8, 0, 0), ("zeroq", 100, 4, 200, 300, 3, 0, 0),
    ("plain", 100, 32, 0, 100, 8, 0, 0), ("plain", 300, 1, 0, 300, 8, 0, 64), ("negzero", 513, 1, 0, 520, 3, 0, 512),
    ("leak", 513, 2, 7, 520, 8, 0, 64), ("plain", 100, 2, 5, 110, 8, 9, 0), ("negzero", 130, 1, 0, 130, 3, 63, 0),
    ("plain", 130, 1, 31, 161, 8, 65, 64), ("leak", 40, 2, 0, 40, 8, 1, 0), ("negzero", 70, 2, 200, 270, 8, 0, 0),
]


@pytest.mark.parametrize("regime,N,H,n_past,n_ctx,nth,chunk,ws_rows", MFMA_CASES)
def test_mfma_and_row(L, oracle, regime, N, H, n_past, n_ctx, nth, chunk, ws_rows):
    taken = run(L, oracle, ("mfma", "auto", "row"), regime, N, H, 128, n_past, n_ctx, nth, chunk, ws_rows)
    assert taken["mfma"] == "mfma" and taken["row"] == "row"
    assert taken["auto"] == L.debug_attn_path(N, 128, n_past, nth, n_ctx) == ("short" if N <= 60 else "mfma")


def test_mfma_refuses_nine_threads_and_auto_takes_k_attn(L, oracle):
    with pytest.raises(L.LlamaHipError, match="n_threads <= 8"):
        run(L, oracle, ("mfma",), "plain", 70, 2, 128, 0, 80, 9)
    assert run(L, oracle, ("auto",), "plain", 70, 2, 128, 3, 80, 9)["auto"] == "row"


# k_attn at head sizes 64 .. 256: (regime, N, H, dh, n_past, n_ctx, n_threads, chunk)
ROW_CASES = [("plain", 1, 4, 64, 0, 4, 1, 0), ("negzero", 9, 2, 96, 5, 16, 3, 0), ("leak", 70, 2, 64, 31, 110, 12, 9),
             ("wide", 33, 1, 256, 200, 233, 8, 0), ("ties", 17, 2, 256, 1, 20, 33, 0), ("negzero", 65, 3, 64, 0, 70, 64, 0),
             ("zeroq", 20, 2, 96, 63, 90, 9, 7)]


@pytest.mark.parametrize("regime,N,H,dh,n_past,n_ctx,nth,chunk", ROW_CASES)
def test_row(L, oracle, regime, N, H, dh, n_past, n_ctx, nth, chunk):
    assert run(L, oracle, ("row",), regime, N, H, dh, n_past, n_ctx, nth, chunk)["row"] == "row"


# the short path (the reference's 9-token flow): (regime, N, H, dh, n_past, n_ctx, n_threads, chunk); dh 128 also runs MFMA and k_attn
SHORT_CASES = [("plain", 2, 2, 128, 0, 2, 1, 0), ("negzero", 8, 2, 64, 3, 16, 8, 0), ("plain", 9, 32, 128, 0, 40, 8, 0),
               ("leak", 9, 2, 128, 31, 40, 12, 0), ("ties", 16, 1, 256, 7, 23, 33, 0), ("wide", 17, 2, 64, 100, 117, 8, 9),
               ("negzero", 60, 2, 128, 0, 60, 8, 9), ("zeroq", 60, 1, 96, 451, 511, 1, 0), ("negzero", 33, 2, 128, 40, 80, 3, 9)]


@pytest.mark.parametrize("regime,N,H,dh,n_past,n_ctx,nth,chunk", SHORT_CASES)
def test_short(L, oracle, regime, N, H, dh, n_past, n_ctx, nth, chunk):
    paths = ("short", "row") + (("mfma",) if dh == 128 and nth <= 8 else ())
    assert run(L, oracle, paths, regime, N, H, dh, n_past, n_ctx, nth, chunk)["short"] == "short"


# one row (the decode step's two-launch kernels) at n_ctx 2 048: (regime, H, dh, n_past, n_threads)
DEC_CASES = [("plain", 2, 128, 0, 1), ("negzero", 2, 64, 1, 8), ("plain", 1, 128, 511, 32), ("wide", 2, 64, 1023, 17),
             ("negzero", 2, 128, 2047, 3), ("zeroq", 4, 64, 1023, 1), ("ties", 2, 128, 511, 8), ("plain", 32, 128, 700, 8)]


@pytest.mark.parametrize("regime,H,dh,n_past,nth", DEC_CASES)
def test_dec(L, oracle, regime, H, dh, n_past, nth):
    taken = run(L, oracle, ("dec", "dec_stream", "row"), regime, 1, H, dh, n_past, 2048, nth)
    assert taken == {"dec": "dec", "dec_stream": "dec_stream", "row": "row"}


def test_float64_bound_would_catch_one_dropped_key(oracle):
    """On ordinary rows dropping the row's largest key moves some column of every (row, head) by more than 10 times the bound, and by more
    than 20 times in 99 % of them: a kernel that lost a key (or let a masked one in) would fail check 4.  (Per element the bound is a few
    tenths of a percent of the output -- the fp16 rounding of s - max alone is worth |s - max| 2^-11 in every weight -- so it cannot
    resolve one key of a long row in EVERY column.)"""
    for N, H, n_past in ((9, 2, 40), (100, 4, 200)):
        qkv, Kc, Vc = attn_cases.make("plain", N, H * 128, H, n_past, n_past + N, seed=11)
        _, Kw, Vw, qr = attn_cases.oracle_side(oracle, qkv, Kc, Vc, H, n_past, 8)
        _, bound, drop = f64_reference(qr, Kw, Vw, H, n_past, 8)
        ratio = (drop / bound).reshape(N, H, 128).max(axis=2)
        assert ratio.min() > 10 and np.mean(ratio > 20) >= 0.99, (ratio.min(), np.mean(ratio > 20))
