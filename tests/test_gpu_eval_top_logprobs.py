"""GPU (-m gpu): llamahip_eval_top_logprobs -- llamahip_eval_logprobs' pass with k_row_topn behind it.

Row i of the result equals llamahip_op_top_logprobs on row i of llamahip_eval_debug's logits_all (a second handle evaluates the same chunks);
the KV cache and logits_last are bit for bit what llamahip_eval / llamahip_eval_chunks leave.  Plain and two-stage pipeline handles, a Q4_0,
an f16 and a Q4_1 file."""
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
HP = synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=4, n_layer=2)
N_CTX = 64
PAST = 5


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def write_file(L, tmp_path, kind):
    path = str(tmp_path / f"top_{kind}.bin")
    if kind == "q4_0":
        synth.write_model(path, HP, synth.random_tensors(HP, seed=3101))
        return path
    src = path + ".f16" if kind == "q4_1" else path
    synth.write_model_unquantized(src, HP, synth.random_tensors(HP, seed=3102), 1)
    if kind == "q4_1":
        L.quantize_file(src, path, 3)
        os.remove(src)
    return path


def check_handle(L, path, note, **kw):
    prefix = synth.synth_prompt(PAST, HP.n_vocab, seed=3110)
    with L.Model(path, n_ctx=N_CTX, **kw) as m, L.Model(path, n_ctx=N_CTX) as ref:
        for h in (m, ref):
            h.eval(prefix, 0, n_threads=8)
        for N in (1, 20):
            toks = synth.synth_prompt(N, HP.n_vocab, seed=3120 + N)
            for chunk in (0, 9):
                for n_top, nth in ((1, 8), (7, 3), (64, 8)):
                    got = m.eval_top_logprobs(toks, PAST, n_top, n_threads=nth, chunk_tokens=chunk)
                    kv = [m.kv(il, PAST + N) for il in range(HP.n_layer)]
                    # the reference handle: the same evals with every row of logits, then the plain entry point for the cache and the last row
                    step = chunk if chunk and N > chunk else N
                    rows = np.concatenate([ref.eval_debug(toks[c0:c0 + step], PAST + c0, n_threads=nth)["logits_all"] for c0 in range(0, N, step)])
                    last = ref.eval_chunks(toks, PAST, chunk_tokens=chunk, n_threads=nth) if chunk else ref.eval(toks, PAST, n_threads=nth)
                    rkv = [ref.kv(il, PAST + N) for il in range(HP.n_layer)]
                    ids, lp = L.op_top_logprobs(rows, n_top)
                    tag = (note, N, chunk, n_top, nth)
                    assert got["ids"].shape == (N, n_top) and same(got["ids"], ids), tag
                    assert same(got["logprob"], lp), tag
                    assert np.all(ids >= 0) and np.all(np.diff(lp, axis=1) <= 0), tag
                    assert same(got["logits"], last) and same(last, rows[-1]), tag
                    for il in range(HP.n_layer):
                        assert same(kv[il][0], rkv[il][0]) and same(kv[il][1], rkv[il][1]), (tag, il)


def test_plain_handle(L, tmp_path):
    check_handle(L, write_file(L, tmp_path, "q4_0"), "plain")


def test_two_stage_pipeline_handle(L, tmp_path):
    check_handle(L, write_file(L, tmp_path, "q4_0"), "pipe2", devices=[0, 0])


@pytest.mark.parametrize("kind", ["f16", "q4_1"])
def test_dense_files(L, tmp_path, kind):
    check_handle(L, write_file(L, tmp_path, kind), kind)


def test_refusals(L, tmp_path):
    path = write_file(L, tmp_path, "q4_0")
    toks = synth.synth_prompt(4, HP.n_vocab, seed=1)
    with L.Model(path, n_ctx=N_CTX) as m:
        for n_top, text in ((0, "llamahip_eval_top_logprobs: n_top 0 outside 1 .. 64"), (65, "llamahip_eval_top_logprobs: n_top 65 outside 1 .. 64")):
            with pytest.raises(L.LlamaHipError) as e:
                m.eval_top_logprobs(toks, 0, n_top)
            assert e.value.message == text
        with pytest.raises(L.LlamaHipError, match="llamahip_eval_top_logprobs: context overflow"):
            m.eval_top_logprobs(toks, N_CTX - 2, 3)
        with pytest.raises(L.LlamaHipError, match="llamahip_eval_top_logprobs: token id"):
            m.eval_top_logprobs([HP.n_vocab], 0, 3)
        with pytest.raises(L.LlamaHipError, match="llamahip_eval_top_logprobs: chunk_tokens must be >= 0"):
            m.eval_top_logprobs(toks, 0, 3, chunk_tokens=-1)
