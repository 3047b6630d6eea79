"""GPU (-m gpu): set steps on f16 / f32 model files -- llamahip_stage_bind / _step / _step_set on dense whole-model handles, the multi-sequence
loops on top of them and the 2 .. 16-row evals -- against the reference build's own arithmetic (its outputs stored in
tests/golden/ref_outputs_dense_set.npz, tests/refgolden.py).  Per sequence the reference does its own evals: the prompt as one eval, then
single-token greedy evals; a set step's row must be bit for bit that sequence's single-token eval.
  odd_widths    K = 1344 (five groups + a 2-step tail), 250 lm-head rows (row tails), H = 21
  tails         n_embd 320, n_ff 896: tail groups in both K
  f16_7b_width  K = 4096 / 11008, the 8-half-wave workgroups of the wide mat-muls
Five sequences with prompts of 3, 9, 17, 30 and 121 tokens (the first two evaluated on the few-row kernel themselves); the longest crosses
the 128-position score bucket of a set step inside the run."""
import os
import shutil

import numpy as np
import pytest

import refgolden
import synth
from test_gpu_sample_multi import _prefill, _single_stream

HERE = os.path.dirname(os.path.abspath(__file__))
STORE = os.path.join(HERE, "golden", "ref_outputs_dense_set.npz")

SHAPES = {
    "f16_7b_width": synth.HParams(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=1),
    "odd_widths": synth.HParams(n_vocab=250, n_embd=1344, n_mult=64, n_head=21, n_layer=2),
    "tails": synth.HParams(n_vocab=200, n_embd=320, n_mult=64, n_head=10, n_layer=2),
}
CASES = [("odd_widths", "f16", 8), ("odd_widths", "f16", 3), ("odd_widths", "f32", 8), ("tails", "f16", 8), ("f16_7b_width", "f16", 8)]
PROMPT_LENS, N_CTX, T = (3, 9, 17, 30, 121), 160, 12
MULTI_S, MULTI_T, MULTI_CTX = 18, 6, 64


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def write_model(tmp, shape, ftype):
    hp = SHAPES[shape]
    path = os.path.join(str(tmp), f"{shape}_{ftype}.bin")
    synth.write_model_unquantized(path, hp, synth.random_tensors(hp, seed=1601), 0 if ftype == "f32" else 1)
    return path


def prompts(hp):
    return [synth.synth_prompt(n, hp.n_vocab, seed=80 + i) for i, n in enumerate(PROMPT_LENS)]


def multi_prompts(hp):
    return [synth.synth_prompt(3 + (5 * i) % 23, hp.n_vocab, seed=120 + i) for i in range(MULTI_S)]


def _ref_stream(rm, prompt, n_steps, nth):
    """the reference's own evals of one sequence: the prompt as one eval, then n_steps single-token greedy evals"""
    first = lo = rm.eval(prompt, 0, nth)["logits"]
    toks = [int(np.argmax(lo))]
    for t in range(n_steps):
        lo = rm.eval(np.array([toks[-1]], np.int32), len(prompt) + t, nth)["logits"]
        toks.append(int(np.argmax(lo)))
    return first, np.array(toks, np.int32), lo


@refgolden.computed_by("gpu_dense_set.sequences", CASES, store=STORE)
def _ref_sequences(ref, tmp, shape, ftype, nth):
    hp = SHAPES[shape]
    rm = ref.load(write_model(tmp, shape, ftype), N_CTX)
    out = {}
    for s, p in enumerate(prompts(hp)):
        out[f"prompt{s}"], out[f"tokens{s}"], out[f"last{s}"] = _ref_stream(rm, p, T, nth)      # tokens: the prompt's pick, then the T steps' picks
        for il in range(hp.n_layer):
            k, v = rm.kv(il, len(p) + T)
            out[f"k{s}_{il}"], out[f"v{s}_{il}"] = refgolden.digest(k), refgolden.digest(v)
    rm.close()
    return out


@refgolden.computed_by("gpu_dense_set.multi", store=STORE)
def _ref_multi(ref, tmp):
    hp = SHAPES["odd_widths"]
    rm = ref.load(write_model(tmp, "odd_widths", "f16"), MULTI_CTX)
    out = {"tokens": np.array([_ref_stream(rm, p, MULTI_T, 8)[1] for p in multi_prompts(hp)], np.int32)}
    rm.close()
    return out


@pytest.fixture(scope="module")
def model_files(tmp_path_factory):
    """one file per (shape, file type) for the whole module (the 7B-width f16 file is 0.4 GB), removed when the module is done"""
    d = tmp_path_factory.mktemp("dense_set_models")
    made = {}

    def get(shape, ftype):
        if (shape, ftype) not in made:
            made[(shape, ftype)] = write_model(d, shape, ftype)
        return made[(shape, ftype)]
    yield get
    shutil.rmtree(str(d), ignore_errors=True)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,ftype,nth", CASES)
def test_stage_set_steps_vs_reference(L, ref, tmp_path, model_files, shape, ftype, nth):
    """stage_bind + 6 set steps of all five slots, 3 steps of a set of three (in another order) while the other two take single stage steps,
    3 set steps of all five again: traces, the logits of every row of the last step and the KV rows of every slot"""
    import torch
    want = refgolden.outputs("gpu_dense_set.sequences", ref, tmp_path, shape, ftype, nth)
    hp = SHAPES[shape]
    ps = prompts(hp)
    S = len(ps)
    sub, rest = [4, 2, 0], [1, 3]
    st = torch.cuda.current_stream().cuda_stream
    for flags in (0, 1):                                       # 1: LLAMAHIP_FLAG_NO_GRAPH, the same launches issued eagerly
        before = L.dense_paths()
        with L.Model(model_files(shape, ftype), n_ctx=N_CTX, n_seq=S, flags=flags) as m:
            assert m.stage_set_applies(S, nth) and m.stage_set_applies(16, nth) and not m.stage_set_applies(17, nth)
            assert not m.stage_set_applies(S, 33)              # (the V*P key split of a set step covers n_threads <= 32)
            firsts = []
            for s, p in enumerate(ps):
                m.set_seq(s)
                lo = m.eval(p, 0, nth)
                assert same(lo, want[f"prompt{s}"]), f"flags {flags}: {len(p)}-row prompt eval of sequence {s}"
                firsts.append(int(np.argmax(lo)))
            m.set_seq(0)
            bufs = [torch.tensor([firsts[s]], dtype=torch.int32, device="cuda") for s in range(S)]
            for s in range(S):
                m.stage_bind(s, len(ps[s]), token_in=bufs[s].data_ptr(), token_out=bufs[s].data_ptr())
            for _ in range(6):
                m.stage_step_set(list(range(S)), nth, st)
            for _ in range(3):
                m.stage_step_set(sub, nth, st)
                for s in rest:
                    m.stage_step(s, nth, st)
            for _ in range(3):
                m.stage_step_set(list(range(S)), nth, st)
            last = [m.stage_logits(s) for s in range(S)]
            for s in range(S):
                n, pos, got = m.stage_trace(s, T)
                assert n == T and pos == len(ps[s]) + T, f"flags {flags}: sequence {s}: {n} steps, position {pos}"
                assert [firsts[s]] + got.tolist() == want[f"tokens{s}"].tolist(), f"flags {flags}: sequence {s}: tokens"
                assert same(last[s], want[f"last{s}"]), f"flags {flags}: sequence {s}: logits of the last set step"
                m.set_seq(s)
                for il in range(hp.n_layer):
                    k, v = m.kv(il, len(ps[s]) + T)
                    assert same(refgolden.digest(k), want[f"k{s}_{il}"]) and same(refgolden.digest(v), want[f"v{s}_{il}"]), \
                        f"flags {flags}: sequence {s}: KV rows of layer {il}"
            m.set_seq(0)
            with pytest.raises(L.LlamaHipError, match="twice"):
                m.stage_step_set([0, 1, 0], nth, st)
        after = L.dense_paths()
        assert after["set"] > before["set"] and after["mv"] > before["mv"], (before, after)


@pytest.mark.gpu
def test_refusals_that_stay(L, tmp_path):
    """layer-range f16 handles, Q4_1 files and LLAMAHIP_FLAG_UNFUSED handles keep their refusal, with a message naming the limit"""
    hp = SHAPES["tails"]
    path = str(tmp_path / "m.bin")
    synth.write_model_unquantized(path, hp, synth.random_tensors(hp, seed=3), 1)
    with L.Model(path, n_ctx=32, n_seq=2, layer_begin=0, layer_end=1) as m:
        assert not m.stage_set_applies(2, 8)
        with pytest.raises(L.LlamaHipError, match=r"whole-model handle \(this one holds layers \[0, 1\)\): use llamahip_eval_stage"):
            m.stage_bind(0, 0, token_in=1, hidden_out=1)
    q41 = str(tmp_path / "q41.bin")
    L.quantize_file(path, q41, 3)
    with L.Model(q41, n_ctx=32, n_seq=2) as m:
        assert not m.stage_set_applies(2, 8)
        with pytest.raises(L.LlamaHipError, match="Q4_1 model.*llamahip_eval_stage"):
            m.stage_bind(0, 0, token_in=1)
    with L.Model(path, n_ctx=32, n_seq=2, flags=2) as m:
        assert not m.stage_set_applies(2, 8)
        with pytest.raises(L.LlamaHipError, match="LLAMAHIP_FLAG_UNFUSED.*llamahip_eval_stage"):
            m.stage_bind(0, 0, token_in=1)
    with L.Model(path, n_ctx=32, n_seq=2) as m:
        with pytest.raises(L.LlamaHipError, match="pipeline mailboxes need a Q4_0 stage handle"):
            m.stage_mailbox(0)
        with pytest.raises(L.LlamaHipError, match="token_in 0x1 is not device-accessible memory"):      # (refused at bind, not a fault at the first step)
            m.stage_bind(0, 0, token_in=1)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [4, 18])
def test_greedy_multi_takes_the_set_path(L, ref, tmp_path, model_files, S):
    """decode_greedy_multi on an f16 file: one group of 4, two groups of 9 -- per sequence the reference's own tokens"""
    want = refgolden.outputs("gpu_dense_set.multi", ref, tmp_path)["tokens"]
    hp = SHAPES["odd_widths"]
    ps = multi_prompts(hp)[:S]
    before = L.dense_paths()
    with L.Model(model_files("odd_widths", "f16"), n_ctx=MULTI_CTX, n_seq=S) as m:
        firsts = []
        for s, p in enumerate(ps):
            m.set_seq(s)
            firsts.append(int(np.argmax(m.eval(p, 0, 8))))
        m.set_seq(0)
        assert firsts == want[:S, 0].tolist()
        got = m.decode_greedy_multi(firsts, [len(p) for p in ps], MULTI_T, 8)
        assert got.tolist() == want[:S, 1:].tolist()
    assert L.dense_paths()["set"] > before["set"]


@pytest.mark.gpu
def test_sample_multi_takes_the_set_path(L, model_files):
    """decode_sample_multi on an f16 file, six sequences: tokens, exact flags, sampler windows and the rng's next draw equal the documented
    eval_topk -> draw -> accept loop on a second handle"""
    hp = SHAPES["odd_widths"]
    S, nth, K = 6, 8, 8
    ps = multi_prompts(hp)[:S]
    seeds = [7 * i + 3 for i in range(S)]
    path = model_files("odd_widths", "f16")
    before = L.dense_paths()
    with L.Model(path, n_ctx=MULTI_CTX, n_seq=S) as h, L.Model(path, n_ctx=MULTI_CTX, n_seq=S) as one:
        samplers, firsts = _prefill(L, h, ps, seeds, nth)
        mid = L.dense_paths()
        got, exact = h.decode_sample_multi(firsts, [len(p) for p in ps], K, samplers, n_threads=nth, want_exact=True)
        assert L.dense_paths()["set"] > mid["set"]
        ref_samplers, ref_firsts = _prefill(L, one, ps, seeds, nth)
        assert firsts == ref_firsts
        lg = np.linspace(-2.0, 2.0, hp.n_vocab).astype(np.float32)
        for i in range(S):
            toks, fl = _single_stream(L, one, i, firsts[i], len(ps[i]), ref_samplers[i], K, nth)
            assert got[i].tolist() == toks and exact[i].tolist() == fl, f"sequence {i}"
            assert samplers[i].window().tolist() == ref_samplers[i].window().tolist(), f"sequence {i}: sampler window"
            assert samplers[i].sample(h, lg) == ref_samplers[i].sample(one, lg), f"sequence {i}: the rng's next draw"
    assert L.dense_paths()["set"] > before["set"]


@pytest.mark.gpu
def test_nine_row_evals_vs_reference(L, ref, tmp_path, model_files):
    """the runner's 9-token prompt evals: a 9-row eval and eval_chunks(..., 9) through launch_dense_mm AUTO, the reference's logits"""
    want = refgolden.outputs("gpu_dense_set.sequences", ref, tmp_path, "odd_widths", "f16", 8)
    p = prompts(SHAPES["odd_widths"])[1]
    assert len(p) == 9
    before = L.dense_paths()
    with L.Model(model_files("odd_widths", "f16"), n_ctx=N_CTX) as m:
        assert same(m.eval(p, 0, 8), want["prompt1"])
        assert same(m.eval_chunks(p, 0, 9, 8), want["prompt1"])
    after = L.dense_paths()
    assert after["set"] > before["set"] and after["mm"] == before["mm"], (before, after)      # (AUTO sends 9 rows to k_dense_set: DESIGN.md 12.16)
