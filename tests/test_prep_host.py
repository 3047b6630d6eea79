"""CPU: llamahip_op_prep / llamahip_op_embed are exported, refuse every bad argument before they look for a device, and the QA-to-blocks
helper llamahip_op_attention and the prep tests share inverts a numpy statement of the QA layout.  Also the CPU half of
tests/test_gpu_prep.py: its inputs meet their own conditions (exact ties, order-proof rows, a bound the oracle meets)."""
import numpy as np
import pytest

import prep_cases as pc


def test_new_symbols_are_exported(L):
    for s in ("llamahip_op_prep", "llamahip_op_embed", "llamahip_debug_qa_to_blocks"):
        assert s in L.declared_symbols() and hasattr(L.lib(), s), s


def prep(L, mode="plain", K=64, N=2, n=None, **kw):
    return L.op_prep(mode, np.zeros(4 * 64 * 8 if n is None else n, np.float32), K, N, **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(mode=0), "unknown mode 0"), (dict(mode=4), "unknown mode 4"), (dict(kernel=3), "unknown kernel 3"), (dict(kernel=-1), "unknown kernel -1"),
    (dict(K=0), "K 0 must be a multiple of 32"), (dict(K=48), "K 48 must be a multiple of 32"), (dict(K=32800), "K 32800 must be"),
    (dict(N=0), "N 0 >= 1"), (dict(qa_rows=1), "qa_rows 1 >= N"),
    (dict(in_stride=32), "row stride 32 / 0 < K 64"), (dict(mode="silu_mul", in1_offset=128, in1_stride=60), "row stride 64 / 60 < K 64"),
    (dict(in_stride=66), "multiples of 4 floats"), (dict(in0_offset=2), "multiples of 4 floats"), (dict(mode="norm", in1_offset=130), "multiples of 4 floats"),
    (dict(mode="silu_mul", in1_offset=128, in1_stride=70), "multiples of 4 floats"),
    (dict(n=100), "end at float 128 / 0 of a buffer of 100"), (dict(mode="norm", in1_offset=2000), "end at float 128 / 2064 of a buffer of 2048"),
    (dict(mode="silu_mul", in1_offset=1920, in1_stride=128), "end at float 128 / 2112 of a buffer of 2048"), (dict(in0_offset=-4), "end at float"),
    (dict(kernel="fast", want_y=True), "FAST .k_prep_fast. has no fp32 output"),
    (dict(mode="norm", kernel="fast", K=16416, n=40000, in1_offset=20000), "FAST refused for NORM with K 16416"),
])
def test_prep_refusals_need_no_device(L, kw, msg):
    with pytest.raises(L.LlamaHipError, match=msg):
        prep(L, **kw)


def test_good_arguments_pass_every_host_check(L):
    """the limits themselves are accepted: what stops these calls on a machine without a GPU is the device check, nothing earlier"""
    emb = pc.embed_matrix(np.random.default_rng(1), 4, 64)
    for call in (lambda: prep(L, mode="norm", K=16384, N=1, n=40000, in1_offset=20000, kernel="fast"),
                 lambda: prep(L, mode="silu_mul", in1_offset=64, in_stride=128, in1_stride=128, want_y=True),
                 lambda: L.op_embed([0, 3], emb, x_stride=64), lambda: L.op_embed([3], emb, want_stats=True)):
        try:
            call()
        except L.LlamaHipError as e:
            assert "no HIP device available" in str(e)


@pytest.mark.parametrize("kw,msg", [(dict(tokens=[0, 4]), "token 4 of row 1 outside .0, 4."), (dict(tokens=[-1]), "token -1 of row 0"),
                                    (dict(tokens=[1], x_stride=60), "x_stride 60 < d 64"), (dict(tokens=[1, 2], want_stats=True), "takes one token"),
                                    (dict(tokens=[]), "bad arguments")])
def test_embed_refusals_need_no_device(L, kw, msg):
    emb = pc.embed_matrix(np.random.default_rng(1), 4, 64)
    with pytest.raises(L.LlamaHipError, match=msg):
        L.op_embed(kw.pop("tokens"), emb, **kw)


@pytest.mark.parametrize("K,N", [(32, 1), (96, 3), (288, 2), (4128, 2)])
def test_qa_to_blocks_inverts_the_numpy_packer(L, K, N):
    rng = np.random.default_rng(K)
    blocks = rng.integers(0, 256, (N, K // 32, 20), dtype=np.uint8)
    qa_A, qa_d = pc.pack_qa(blocks, K)
    assert qa_A.shape == (N, pc.kp(K) // 4) and qa_d.shape == (N, pc.kp(K) // 32)
    assert np.array_equal(L.qa_to_blocks(qa_A, qa_d, N, K), blocks)
    # the packer against the layout's definition, element by element, on one block: element l of block b is nibble (l % 16 // 2 ... ) of chain k
    n, b = N - 1, K // 32 - 1
    qs = blocks[n, b, 4:].astype(int)
    q = np.array([(qs[l // 2] >> (4 * (l & 1))) & 0xF for l in range(32)])
    for k in range(8):
        dw = int(qa_A[n, ((b >> 3) * 8 + k) * 8 + (b & 7)]) >> (4 * (b & 1))
        assert [(dw >> s) & 0xF for s in (0, 8, 16, 24)] == [(q[l] - 8) & 0xF for l in (2 * k, 2 * k + 1, 16 + 2 * k, 17 + 2 * k)]
        assert dw & 0xF0F0F0F0 == 0
    assert not qa_A[:, (K // 32 // 8) * 64:].reshape(N, -1, 8, 8)[..., (K // 32) % 8:].any() or K % 256 == 0


def test_every_norm_row_of_the_gpu_cases_is_order_proof_and_the_ties_are_exact(oracle):
    for c in pc.CASES:
        mode, K, N, regime, _ = c
        x, b = pc.build(oracle, mode, K, N, regime)
        if mode == "norm":
            assert all(pc.norm_stats(r)["proof"] for r in x), pc.case_id(c)
        if regime == "ties":
            y, _ = pc.reference(oracle, mode, x, b)
            p, a = pc.tie_products(y).reshape(-1, 32), np.abs(y).reshape(-1, 32)
            inner = a != a.max(axis=1, keepdims=True)
            assert inner.sum() == 30 * p.shape[0] and np.all(p[inner] - np.floor(p[inner]) == 0.5), pc.case_id(c)
            assert set(np.floor(p[inner]).astype(int)) == set(range(-7, 7))


def test_order_proof_check_rejects_what_it_should():
    """the check is not vacuous: the cancelling row fails it, so do some ordinary rows of the widest width (which is why the rows come from a
    table of draws), and rows whose sums are exact in any order have a mean interval of width zero"""
    assert not pc.norm_stats(pc.cancel_row(np.random.default_rng(3)))["v_ok"]
    wide = [pc.norm_stats(np.random.default_rng([9, a]).standard_normal(22016).astype(np.float32))["proof"] for a in range(24)]
    assert 0 < sum(wide) < len(wide)
    assert pc.norm_stats(np.full(4096, 0.7, np.float32))["rad"] == 0.0 and pc.norm_stats(np.zeros(64, np.float32))["proof"]


def test_oracle_meets_the_float64_bound_on_the_cancelling_row(oracle):
    x, w, y, blocks, y64, B = pc.cancel_case(oracle)
    assert np.all(np.abs(y.astype(np.float64) - y64) <= B)
    dq, d = pc.dequantize(blocks)
    assert np.all(np.abs(dq[0] - y64) <= d[0] / 2 + B)
    assert np.all(B < d[0] / 4), "the bound must resolve a quantization step"
