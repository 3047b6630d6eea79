"""GPU: the producers of every mat-mul's activation operand, op by op -- k_prep_fast and k_prep_qa in their three modes (llamahip_op_prep)
and the embedding gather k_embed / k_embed_part (llamahip_op_embed) -- against the oracle, bit for bit.  The gathers write
dense rows on the device; the op checks a guard behind them and copies them out at the caller's stride, so the canaries between the
returned rows test the op's placement only.

Every prep case (tests/prep_cases.py: shapes at which each branch of the launch rule and of the kernels exists, value regimes at the
quantizer's edges) runs on every kernel family that takes its shape -- AUTO, FAST, LDS -- and asserts
  1. the whole raw operand of the N rows equals a numpy packing of the oracle's Q4_0 blocks, bit for bit: codes, scales, the unused nibbles,
     and every padded block between K/32 and Kp/32 zero (the buffers go in filled with 0xFF);
  2. the Q4_0 blocks the library's own conversion makes of it equal the oracle's;
  3. the LDS kernel's fp32 rows y equal the oracle's, bit for bit;
  4. the rows past N keep the caller's 0xFF in every byte;
  5. FAST and LDS leave identical buffers;
  6. kernel_taken follows launch_prep's rule.
References: PLAIN oracle.quantize_row; NORM oracle.unary_rows("norm", x), one fp32 multiply by w, quantize_row; SILU_MUL
oracle.unary_rows("silu", gate), one fp32 multiply by up, quantize_row; the embedding oracle.dequantize_row.

The norm statistics are double sums whose ORDER differs from the reference's (sequential there, per thread then by tree here).  Every
NORM row of the cases is order-proof (prep_cases' docstring: no (float) (x_i - mean) and no (float) scale has a rounding boundary inside
the interval any summation order can reach -- asserted on the inputs, with no row excluded), so bit-equality is required of them.
test_norm_that_is_not_order_proof then takes a row built to cancel (pairs of +-1e8 among unit-scale values) and holds oracle and kernels
to a float64 bound instead (prep_cases.norm_f64_bound)."""
import math

import numpy as np
import pytest

import prep_cases as pc

pytestmark = pytest.mark.gpu
FILL = 0xFFFFFFFF


def first_diff(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]:#x}, want {want[tuple(bad[0])]:#x}" if len(bad) else "equal"


def run_kernels(L, mode, x, b, layout, want_A, want_d, want_blocks, want_y, tag):
    """every kernel family that takes the shape; returns {kernel asked for: (qa_A, qa_d)}"""
    N, K = x.shape
    buf, kw = pc.lay_out(mode, x, b, layout)
    out = {}
    for kernel, want_yes, expect in pc.kernels_for(mode, K):
        t = f"{tag} kernel={kernel} y={want_yes}"
        qa_A, qa_d, y, taken = L.op_prep(mode, buf, K, N, kernel=kernel, want_y=want_yes, qa_rows=N + 2, **kw)
        assert taken == expect, f"{t}: ran {taken}, launch_prep's rule says {expect}"
        dv = qa_d.view(np.uint32)
        if want_A is not None:
            assert np.array_equal(qa_A[:N], want_A), f"{t}: qa_A: {first_diff(qa_A[:N], want_A)}"
            assert np.array_equal(dv[:N], want_d.view(np.uint32)), f"{t}: qa_d: {first_diff(dv[:N], want_d.view(np.uint32))}"
            assert np.array_equal(L.qa_to_blocks(qa_A, qa_d, N, K), want_blocks), f"{t}: Q4_0 blocks differ"
        nb, nbp = K // 32, pc.kp(K) // 32
        pad = qa_A[:N].reshape(N, nbp // 8, 8, 8)[:, nb // 8:, :, nb % 8 if nb % 8 else 8:] if nb < nbp else np.zeros(0, np.uint32)
        assert not pad.any() and not dv[:N, nb:].any(), f"{t}: padded blocks {nb} .. {nbp - 1} are not zero"
        assert np.all(qa_A[N:] == FILL) and np.all(dv[N:] == FILL), f"{t}: rows past N written"
        if want_yes and want_y is not None:
            assert np.array_equal(y.view(np.uint32), want_y.view(np.uint32)), f"{t}: y: {first_diff(y.view(np.uint32), want_y.view(np.uint32))}"
        out[(kernel, want_yes)] = (qa_A, qa_d, y)
    if ("fast", False) in out:
        f, l = out[("fast", False)], out[("lds", False)]
        assert np.array_equal(f[0], l[0]) and np.array_equal(f[1].view(np.uint32), l[1].view(np.uint32)), f"{tag}: FAST and LDS buffers differ"
    return out


@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_prep(L, oracle, case):
    mode, K, N, regime, layout = case
    x, b = pc.build(oracle, mode, K, N, regime)
    if mode == "norm":          # a condition on the INPUTS: with it, no summation order can change a float (no row is excused)
        proof = [pc.norm_stats(r)["proof"] for r in x]
        assert all(proof), f"rows {np.flatnonzero(~np.array(proof))} are not order-proof"
    y, blocks = pc.reference(oracle, mode, x, b)
    if regime == "ties":
        p, a = pc.tie_products(y).reshape(-1, 32), np.abs(y).reshape(-1, 32)
        inner = a != a.max(axis=1, keepdims=True)
        assert inner.sum() == 30 * p.shape[0] and np.all(p[inner] - np.floor(p[inner]) == 0.5), "the oracle's products are not exact halves"
    if regime == "maxpos":
        codes = np.concatenate([blocks[..., 4:] & 0xF, blocks[..., 4:] >> 4], axis=-1)
        assert (codes == 15).any() and (codes == 1).any()
    if regime != "silu_edges":
        amax = np.abs(y).reshape(-1, 32).max(axis=1)
        assert np.all((amax == 0) | (amax >= 1e-30)) and np.all(np.isfinite(y))
    want_A, want_d = pc.pack_qa(blocks, K)
    run_kernels(L, mode, x, b, layout, want_A, want_d, blocks, y, pc.case_id(case))


def test_fast_is_refused_where_a_norm_row_exceeds_one_workgroup(L):
    with pytest.raises(L.LlamaHipError, match="FAST refused for NORM with K 16416"):
        L.op_prep("norm", np.zeros(2 * 16416, np.float32), 16416, 1, in1_offset=16416, kernel="fast")


def test_norm_that_is_not_order_proof(L, oracle):
    """Heavy cancellation (prep_cases.cancel_row, K = 4096): the mean's interval is ~1.8e-7 wide around 0.009, so floats DO depend on the
    order and bit-equality is not asked.  Instead, with B = prep_cases.norm_f64_bound (derived there from the same interval, propagated through
    w * ((float) (x - mean) * scale) with its four fp32 roundings):  |y - y64| <= B for the LDS kernel's y and for the oracle's;
    |d q - y64| <= d / 2 + B for every code of both kernels and of the oracle; and B < d / 4 in every block, or the check would prove nothing."""
    x, w, y_orc, blocks_orc, y64, B = pc.cancel_case(oracle)
    assert not pc.norm_stats(x[0])["v_ok"]
    K = x.shape[1]

    def check(name, y, blocks):
        if y is not None:
            err = np.abs(y.astype(np.float64) - y64)
            print(f"{name}: max |y - y64| / B = {(err / B).max():.3f}")
            assert np.all(err <= B), f"{name}: y outside the float64 bound at {np.flatnonzero(err > B)[:4]}"
        dq, d = pc.dequantize(blocks)
        assert np.all(B < d[0] / 4), f"{name}: the bound does not resolve a quantization step"
        err = np.abs(dq[0] - y64)
        print(f"{name}: max (|d q - y64| - B) / d = {((err - B) / d[0]).max():.6f}")
        assert np.all(err <= d[0] / 2 + B), f"{name}: codes outside d / 2 + B at {np.flatnonzero(err > d[0] / 2 + B)[:4]}"

    check("oracle", y_orc, blocks_orc)
    out = run_kernels(L, "norm", x, w, "dense", None, None, None, None, "cancel")
    for (kernel, want_yes), (qa_A, qa_d, y) in out.items():
        check(f"{kernel} y={want_yes}", y, L.qa_to_blocks(qa_A, qa_d, 1, K))


# ------------------------------------------------------------------------------------------------ embedding
CANARY = np.uint32(0x7FC0BEEF)
V_EMB = 11


@pytest.fixture(scope="module")
def emb_refs(oracle):
    """d -> (matrix [V, d/32, 20], its rows dequantized by the oracle [V, d]); computed once"""
    out = {}
    for d in (32, 64, 480, 4096, 5152):
        m = pc.embed_matrix(np.random.default_rng(d), V_EMB, d)
        codes = np.concatenate([m[..., 4:] & 0xF, m[..., 4:] >> 4], axis=-1)
        assert (codes == 0).any() and (codes == 15).any() and (np.ascontiguousarray(m[..., :4]).view(np.float32) == 0).any()
        out[d] = (m, np.stack([oracle.dequantize_row(r) for r in m]))
    return out


@pytest.mark.parametrize("N", [1, 2, 64, 65])          # (grid.y slices the row up to 64 rows, one workgroup per row from 65)
@pytest.mark.parametrize("d", [32, 64, 480, 4096, 5152])
def test_embed(L, emb_refs, d, N):
    m, rows = emb_refs[d]
    tokens = np.array([0, V_EMB - 1, 3, 3, 0, 7][:N] + list(np.random.default_rng(N).integers(0, V_EMB, max(N - 6, 0))), np.int32)
    assert N < 2 or (0 in tokens and V_EMB - 1 in tokens)
    stride = d + 8
    x = L.op_embed(tokens, m, stride, np.full((N, stride), CANARY, np.uint32).view(np.float32))
    got, want = x[:, :d].view(np.uint32), rows[tokens].view(np.uint32)
    assert np.array_equal(got, want), f"d={d} N={N}: {first_diff(got, want)}"
    # (k_embed writes dense [N][d] rows into a device buffer of the op's own, which the op then places `stride` apart with a 2-D copy: the
    # canaries check that placement, not the kernel -- against a kernel overrun the op keeps 64 guard floats after row N - 1 and fails if
    # one of them changed)
    assert np.all(x[:, d:].view(np.uint32) == CANARY), "the floats between the rows were written"


@pytest.mark.parametrize("d", [32, 64, 480, 4096, 5152])
def test_embed_part(L, emb_refs, d):
    """k_embed_part: the row k_embed gathers, plus {sum x, sum x^2} in double within gamma_d sum|v| (gamma_d sum v^2) of the exact sums: the
    terms are exact doubles (an fp32 value, the square of one), so only the additions round, d - 1 of them in any order"""
    m, rows = emb_refs[d]
    for tok in (0, V_EMB - 1, 4):
        x, stats = L.op_embed([tok], m, d + 8, np.full((1, d + 8), CANARY, np.uint32).view(np.float32), want_stats=True)
        plain = L.op_embed([tok], m)
        assert np.array_equal(x[:, :d].view(np.uint32), plain.view(np.uint32)) and np.array_equal(plain.view(np.uint32), rows[[tok]].view(np.uint32))
        assert np.all(x[:, d:].view(np.uint32) == CANARY)          # (the op's placement, as in test_embed)
        v = rows[tok].astype(np.float64)
        s1, s2, a1 = math.fsum(v), math.fsum(v * v), math.fsum(np.abs(v))
        assert abs(stats[0] - s1) <= pc.gamma(d) * a1, (tok, stats[0], s1)
        assert abs(stats[1] - s2) <= pc.gamma(d) * s2, (tok, stats[1], s2)
        assert s2 == 0 or stats[1] > 0
