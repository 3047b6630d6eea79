"""CPU: the standalone restatement against the reference's own ggml.c compiled in place
(oracle/_ref where the reference sources are present; its outputs for these inputs are stored in
tests/golden/ref_outputs.npz, tests/refgolden.py).  Randomised, larger shapes than the committed fixtures.  Bit-exact."""
import numpy as np
import pytest

import refgolden
import synth


def _quantizer_input():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((64, 4096)) * rng.uniform(0.01, 5, (64, 1))).astype(np.float32)
    x[3, 64:96] = 0
    return x


@refgolden.computed_by("oracle_vs_ref.quantizers")
def _ref_quantizers(ref, tmp):
    x = _quantizer_input()
    return {"rows": np.stack([ref.quantize_row(r) for r in x[:16]]), "offline": ref.quantize_offline(x)}


def test_quantizers(oracle, ref, tmp_path):
    x = _quantizer_input()
    want = refgolden.outputs("oracle_vs_ref.quantizers", ref, tmp_path)
    for r, w in zip(x[:16], want["rows"]):
        assert np.array_equal(oracle.quantize_row(r), w)
    assert np.array_equal(oracle.quantize_offline(x), want["offline"])
    assert np.array_equal(synth.quantize_q4_0_offline(x), want["offline"])      # the numpy writer too


MUL_MAT_CASES = [(64, 4096, 1), (32, 11008, 3), (40, 5120, 9), (16, 8192, 2), (128, 64, 4)]


def _mul_mat_inputs(M, K, N):
    rng = np.random.default_rng(M * 7 + K + N)
    w = synth.quantize_q4_0_offline((0.02 * rng.standard_normal((M, K))).astype(np.float32))
    x = rng.standard_normal((N, K)).astype(np.float32)
    return w, x


@refgolden.computed_by("oracle_vs_ref.mul_mat", MUL_MAT_CASES)
def _ref_mul_mat(ref, tmp, M, K, N):
    w, x = _mul_mat_inputs(M, K, N)
    return {"y": ref.mul_mat_q4_0(w, x, 8)}


@pytest.mark.parametrize("M,K,N", MUL_MAT_CASES)
def test_mul_mat(oracle, ref, tmp_path, M, K, N):
    w, x = _mul_mat_inputs(M, K, N)
    assert np.array_equal(oracle.mul_mat_q4_0(w, x, 4), refgolden.outputs("oracle_vs_ref.mul_mat", ref, tmp_path, M, K, N)["y"])


def _row_ops_inputs():
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((9, 5120)) * 2).astype(np.float32)
    s = (rng.standard_normal((40, 513)) * 4).astype(np.float32)
    s[::3, 200:] = -np.inf
    r = rng.standard_normal((12, 4, 128)).astype(np.float32)
    return x, s, r


@refgolden.computed_by("oracle_vs_ref.row_ops")
def _ref_row_ops(ref, tmp):
    x, s, r = _row_ops_inputs()
    return {"norm": ref.unary_rows("norm", x, 4), "silu": ref.unary_rows("silu", x, 4), "soft_max": ref.unary_rows("soft_max", s, 4),
            "rope_37_0": ref.rope(r, 37, 0), "rope_5_1": ref.rope(r, 5, 1)}


def test_row_ops(oracle, ref, tmp_path):
    x, s, r = _row_ops_inputs()
    want = refgolden.outputs("oracle_vs_ref.row_ops", ref, tmp_path)
    assert np.array_equal(oracle.unary_rows("norm", x), want["norm"])
    assert np.array_equal(oracle.unary_rows("silu", x), want["silu"])
    assert np.array_equal(oracle.unary_rows("soft_max", s), want["soft_max"])
    assert np.array_equal(oracle.rope(r, 37, 0), want["rope_37_0"])
    assert np.array_equal(oracle.rope(r, 5, 1), want["rope_5_1"])


MODEL_CASES = [(8, 1), (5, 2)]
MODEL_TENSORS = ("tok_embeddings.weight", "layers.1.attention.wo.weight", "layers.2.feed_forward.w2.weight",
                 "layers.0.feed_forward.w1.weight", "output.weight", "norm.weight")


def _model(tmp, parts):
    hp = synth.HParams(n_vocab=128, n_embd=256, n_mult=256, n_head=2, n_layer=3)
    path = str(tmp) + "/m.bin"
    synth.write_model(path, hp, synth.random_tensors(hp, seed=77), n_parts=parts)
    return path, synth.synth_prompt(11, hp.n_vocab, seed=5)


@refgolden.computed_by("oracle_vs_ref.model", MODEL_CASES)
def _ref_model(ref, tmp, nth, parts):
    path, toks = _model(tmp, parts)
    mr = ref.load(path, 48, parts)
    out = {f"tensor/{name}": refgolden.digest(mr.tensor_bytes(name)) for name in MODEL_TENSORS}
    out.update({f"eval9/{k}": v for k, v in mr.eval(toks[:9], 0, nth, all_logits=True, dump_layer=2).items()})
    out["eval2_logits_all"] = mr.eval(toks[9:], 9, nth, all_logits=True)["logits_all"]
    tok, n_past, steps = int(np.argmax(out["eval2_logits_all"][-1])), 11, []
    for _ in range(10):
        steps.append(mr.eval(np.array([tok], np.int32), n_past, nth)["logits"])
        tok = int(np.argmax(steps[-1])); n_past += 1
    out["decode_logits"] = np.stack(steps)
    mr.close()
    return out


@pytest.mark.parametrize("nth,parts", MODEL_CASES)
def test_model_eval_and_multipart_merge(oracle, ref, tmp_path, nth, parts):
    want = refgolden.outputs("oracle_vs_ref.model", ref, tmp_path, nth, parts)
    path, toks = _model(tmp_path, parts)
    mo = oracle.load(path, 48, parts)
    for name in MODEL_TENSORS:
        assert np.array_equal(refgolden.digest(mo.tensor_bytes(name)), want[f"tensor/{name}"]), name
    a = mo.eval(toks[:9], 0, nth, all_logits=True, dump_layer=2)
    b = {k[len("eval9/"):]: v for k, v in want.items() if k.startswith("eval9/")}
    assert b
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    a = mo.eval(toks[9:], 9, nth, all_logits=True)
    assert np.array_equal(a["logits_all"], want["eval2_logits_all"])
    tok, n_past = int(np.argmax(want["eval2_logits_all"][-1])), 11
    for lb in want["decode_logits"]:
        la = mo.eval(np.array([tok], np.int32), n_past, nth)["logits"]
        assert np.array_equal(la, lb)
        tok = int(np.argmax(lb)); n_past += 1


# one layer's attention (.mm:614-646): (regime, dh, H, N, n_past, n_threads) -- head sizes 32 .. 256, one / nine / seventy rows with and
# without earlier keys, n_threads 1, 3, 8, 12 and more than the keys (16 > 9), key counts the split does not divide
ATTN_CASES = [("plain", 32, 4, 1, 0, 1), ("plain", 64, 2, 9, 0, 3), ("plain", 128, 2, 70, 5, 8), ("plain", 256, 1, 9, 20, 12),
              ("plain", 64, 2, 9, 0, 16), ("plain", 128, 2, 1, 40, 8), ("wide", 128, 2, 70, 0, 3), ("ties", 64, 2, 9, 7, 8),
              ("leak", 128, 2, 70, 3, 12), ("negzero", 64, 2, 70, 0, 1), ("negzero", 128, 1, 9, 4, 3), ("negzero", 32, 2, 70, 6, 8),
              ("zeroq", 32, 4, 70, 11, 8)]
# a chunked pass (chunk > 0) against successive reference calls of `chunk` rows: (regime, dh, H, N, n_past, n_threads, chunk)
ATTN_CHUNK_CASES = [("plain", 64, 2, 70, 5, 8, 9), ("negzero", 64, 2, 30, 0, 3, 7), ("plain", 128, 1, 20, 3, 12, 1)]
ATTN_STORE = refgolden.os.path.join(refgolden.os.path.dirname(refgolden.STORE), "ref_attention.npz")


def _attn_ref(ref):
    """the reference build where it has the attention op, else None (its stored outputs)"""
    return ref if ref is not None and ref.has_attention else None


def _attn_inputs(oracle, regime, dh, H, N, n_past):
    import attn_cases
    qkv, Kc, Vc = attn_cases.make(regime, N, H * dh, H, n_past, n_past + N + 3, seed=5)
    _, Kr, Vr, qr = attn_cases.oracle_side(oracle, qkv, Kc, Vc, H, n_past, 1)
    return qr, Kr, Vr


@refgolden.computed_by("oracle_vs_ref.attention", ATTN_CASES, store=ATTN_STORE)
def _ref_attention(ref, tmp, regime, dh, H, N, n_past, nth):
    import reflib
    qr, Kr, Vr = _attn_inputs(reflib.OracleLib(), regime, dh, H, N, n_past)
    return {"merged": refgolden.digest(ref.attention(qr, Kr, Vr, H, n_past, nth))}


@pytest.mark.parametrize("regime,dh,H,N,n_past,nth", ATTN_CASES)
def test_attention(oracle, ref, tmp_path, regime, dh, H, N, n_past, nth):
    qr, Kr, Vr = _attn_inputs(oracle, regime, dh, H, N, n_past)
    got = oracle.attention(qr, Kr, Vr, H, n_past, nth)
    want = refgolden.outputs("oracle_vs_ref.attention", _attn_ref(ref), tmp_path, regime, dh, H, N, n_past, nth)
    assert np.array_equal(refgolden.digest(got), want["merged"])
    if regime == "negzero":              # the regime reaches -0 sums (else it would not test their sign)
        assert np.any(got.view(np.uint32) == 0x80000000)


@refgolden.computed_by("oracle_vs_ref.attention_chunks", ATTN_CHUNK_CASES, store=ATTN_STORE)
def _ref_attention_chunks(ref, tmp, regime, dh, H, N, n_past, nth, chunk):
    import reflib
    qr, Kr, Vr = _attn_inputs(reflib.OracleLib(), regime, dh, H, N, n_past)
    rows = [ref.attention(qr[c0:c0 + chunk], Kr, Vr, H, n_past + c0, nth) for c0 in range(0, N, chunk)]
    return {"merged": refgolden.digest(np.concatenate(rows))}


@pytest.mark.parametrize("regime,dh,H,N,n_past,nth,chunk", ATTN_CHUNK_CASES)
def test_attention_chunks_are_successive_calls(oracle, ref, tmp_path, regime, dh, H, N, n_past, nth, chunk):
    qr, Kr, Vr = _attn_inputs(oracle, regime, dh, H, N, n_past)
    want = refgolden.outputs("oracle_vs_ref.attention_chunks", _attn_ref(ref), tmp_path, regime, dh, H, N, n_past, nth, chunk)
    assert np.array_equal(refgolden.digest(oracle.attention(qr, Kr, Vr, H, n_past, nth, chunk)), want["merged"])
    # ... and the one-call pass differs (else the case would not test the split)
    assert not np.array_equal(refgolden.digest(oracle.attention(qr, Kr, Vr, H, n_past, nth)), want["merged"])
