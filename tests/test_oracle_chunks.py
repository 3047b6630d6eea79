"""CPU: the claim behind llamahip_eval_chunks, checked on the CPU side alone.  The reference's driver hands a prompt to llama_eval
n_batch + 1 = 9 tokens at a time (.mm:840-848, 880-888).  Every operator of the eval graph works row by row except the V*P key split over
n_threads, whose chunk length comes from the key count OF THAT llama_eval CALL (ggml.c:5459-5480).  So ONE pass over all prompt rows in
which row n splits n_past + min(N, (n // 9 + 1) * 9) keys must leave the same KV cache and logits, bit for bit, as the successive calls
-- here: the reference build's successive calls (oracle/_ref, the reference's own ggml.c; stored in tests/golden/ref_outputs.npz) against
the restatement's one pass with orc_set_split_chunk(9) -- and an ordinary one-call eval of the same rows must NOT (else the test would say
nothing)."""
import numpy as np
import pytest

import refgolden
import synth

CASES = [(8, 9, 40, 2), (3, 9, 100, 2), (5, 4, 30, 4), (1, 9, 25, 2)]
WARM = np.array([0, 1, 2, 3], np.int32)
N_PAST = 4
N_LAYER = 2


def _model(tmp, n_prompt, n_head):
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=64, n_head=n_head, n_layer=N_LAYER)
    path = str(tmp) + "/m.bin"
    synth.write_model(path, hp, synth.random_tensors(hp, seed=31))
    return path, synth.synth_prompt(n_prompt, hp.n_vocab, seed=8), n_prompt + 8


@refgolden.computed_by("oracle_chunks.successive_calls", CASES)
def _ref_successive_calls(ref, tmp, nth, chunk, n_prompt, n_head):
    path, prompt, n_ctx = _model(tmp, n_prompt, n_head)
    rm = ref.load(path, n_ctx)
    rm.eval(WARM, 0, nth)
    for c0 in range(0, n_prompt, chunk):
        want = rm.eval(prompt[c0:c0 + chunk], N_PAST + c0, nth)["logits"]
    out = {"logits": want}
    for il in range(N_LAYER):
        k, v = rm.kv(il, N_PAST + n_prompt)
        out[f"k{il}"], out[f"v{il}"] = refgolden.digest(k), refgolden.digest(v)
    rm.close()
    return out


@pytest.mark.parametrize("nth,chunk,n_prompt,n_head", CASES)
def test_one_pass_with_per_row_key_split_equals_successive_calls(oracle, ref, tmp_path, nth, chunk, n_prompt, n_head):
    ref_out = refgolden.outputs("oracle_chunks.successive_calls", ref, tmp_path, nth, chunk, n_prompt, n_head)
    want = ref_out["logits"]
    path, prompt, n_ctx = _model(tmp_path, n_prompt, n_head)
    om = oracle.load(path, n_ctx)
    om.eval(WARM, 0, nth)
    oracle.L.orc_set_split_chunk(chunk)
    try:
        got = om.eval(prompt, N_PAST, nth)["logits"]
    finally:
        oracle.L.orc_set_split_chunk(0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    T = N_PAST + n_prompt
    for il in range(N_LAYER):
        gk, gv = om.kv(il, T)
        assert np.array_equal(refgolden.digest(gk), ref_out[f"k{il}"]) and np.array_equal(refgolden.digest(gv), ref_out[f"v{il}"]), f"kv cache layer {il}"
    if nth > 1:
        o1 = oracle.load(path, n_ctx)
        o1.eval(WARM, 0, nth)
        one = o1.eval(prompt, N_PAST, nth)["logits"]
        assert not np.array_equal(one.view(np.uint32), want.view(np.uint32))
