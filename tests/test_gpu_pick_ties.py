"""GPU (-m gpu): greedy and sampled picks on models whose logits TIE on every step.

Random weights never tie, so a tie-break in the wrong direction in k_argmax, k_argmax_set, k_verify_rows or the lm head's pick epilogue
(EPI_STORE_PICK) passes every other test.  Here `output.weight` has duplicated rows: two identical weight rows give bit-identical logits,
on the device and in the oracle, so every step's maximum is a tie and the right pick -- np.argmax of the oracle's logits, the first index --
is the lower twin.  Two layouts: "halves" (row i + V/2 := row i; the twins land in different workgroups of the lm head) and "neighbours"
(row 2i + 1 := row 2i; the same row-group).  Small models take k_argmax, the model at the 7B lm-head width (K = 4096) takes the pick
epilogue; which one is asserted.  Every greedy path must produce the oracle's tokens.  The sampled paths run on a model with one row in
eight duplicated, where ties reach the cut on some steps and not on others (tests/topk_ref.py decides which)."""
import os

import numpy as np
import pytest

import synth
import topk_ref as T
from conftest import synth_tool
from test_gpu_sample_lookup import _lookup_run, _truth
from test_gpu_sample_multi import _prefill, _single_stream
from variants import EPI_STORE_PICK, PREP_NORM

pytestmark = pytest.mark.gpu
SMALL = synth.HParams(n_vocab=2048, n_embd=256, n_mult=64, n_head=4, n_layer=2)
WIDE = dict(n_vocab=8192, n_embd=4096, n_mult=256, n_head=32, n_layer=2)          # the 7B lm head's row length; two layers: a pipeline can split it
N_CTX, N_STEPS, NTH = 64, 12, 8


def _twin_rows(w, layout):
    """duplicate rows of a [V, ...] array in place"""
    V = w.shape[0]
    if layout == "halves":
        w[V // 2:] = w[:V // 2]
    elif layout == "neighbours":
        w[1::2] = w[0::2]
    else:
        assert layout == "eighth"
        w[4::8] = w[0::8]
    return w


def _upper_twin(tok, V, layout):
    return tok + V // 2 if layout == "halves" else tok + 1


def _oracle_greedy(oracle, path, prompt, n_steps):
    """the oracle stepped token by token, the next token np.argmax of its logits (the first index): (first, tokens, every step's logits)"""
    om = oracle.load(path, N_CTX)
    rows = [om.eval(prompt, 0, NTH)["logits"]]
    toks = [int(np.argmax(rows[0]))]
    for s in range(n_steps):
        rows.append(om.eval(np.array([toks[-1]], np.int32), len(prompt) + s, NTH)["logits"])
        toks.append(int(np.argmax(rows[-1])))
    om.close()
    return toks[0], toks[1:], rows


def _assert_every_step_ties(rows, toks, V, layout):
    for lg, t in zip(rows, toks):
        top = np.sort(lg)[-2:]
        assert top[0].tobytes() == top[1].tobytes(), "the two largest logits must be bit-equal"
        assert lg[t] == top[1] and lg[_upper_twin(t, V, layout)].tobytes() == lg[t].tobytes()
        assert t < V // 2 if layout == "halves" else t % 2 == 0


@pytest.fixture(scope="module", params=["small_halves", "small_neighbours", "wide_halves", "wide_neighbours"])
def tied(request, L, oracle, tmp_path_factory):
    width, layout = request.param.split("_")
    d = tmp_path_factory.mktemp(request.param)
    path = str(d / "m.bin")
    if width == "small":
        V, K, n_layer = SMALL.n_vocab, SMALL.n_embd, SMALL.n_layer
        tensors = synth.random_tensors(SMALL, seed=31)
        _twin_rows(tensors["output.weight"], layout)
        synth.write_model(path, SMALL, tensors)
    else:
        V, K, n_layer = WIDE["n_vocab"], WIDE["n_embd"], WIDE["n_layer"]
        synth_tool(path, seed=33, **WIDE)
        off, nbytes, shape, ftype = synth.tensor_offsets(path)["output.weight"]
        assert shape == (V, K) and ftype == 2 and nbytes == V * (K // 32) * 20      # rows of K / 32 twenty-byte blocks
        mm = np.memmap(path, np.uint8, "r+", offset=off, shape=(V, (K // 32) * 20))
        _twin_rows(mm, layout)
        mm.flush()
        del mm
    # which picker the fused greedy step of this model gets: a silent fall-back must not count as coverage.  A plan is necessary, not
    # sufficient: the host folds the pick into the lm head only in llamahip_decode_greedy's captured step on a plain Q4_0 handle with
    # default flags (llamahip.cpp, `fold`: first and last stage in one, no LLAMAHIP_FLAG_NO_GRAPH / _UNFUSED).  So on the wide models it is
    # the graph_fused runs that reach the epilogue; eager_fused, eager_unfused and the pipeline handle pick with k_argmax there as well.
    plan = L.gemv_plan(V, K, PREP_NORM, EPI_STORE_PICK)
    assert (plan is not None) == (width == "wide"), (request.param, plan)
    prompts = [synth.synth_prompt(n, V, seed=40 + n) for n in (9, 3, 6, 14)]
    streams = [_oracle_greedy(oracle, path, p, N_STEPS) for p in prompts]
    for first, toks, rows in streams:
        _assert_every_step_ties(rows, [first] + toks, V, layout)
    yield dict(path=path, V=V, layout=layout, n_layer=n_layer, prompts=prompts, streams=streams, width=width)
    os.remove(path)


@pytest.mark.parametrize("flags", [0, 1, 3], ids=["graph_fused", "eager_fused", "eager_unfused"])
def test_decode_greedy_picks_the_lower_twin(L, tied, flags):
    prompt, (first, want, _) = tied["prompts"][0], tied["streams"][0]
    with L.Model(tied["path"], n_ctx=N_CTX, flags=flags) as m:
        assert int(np.argmax(m.eval(prompt, 0, NTH))) == first
        assert m.decode_greedy(first, len(prompt), N_STEPS, NTH).tolist() == want
        # in two calls: the second starts from the first's last pick
        m.eval(prompt, 0, NTH)
        a = m.decode_greedy(first, len(prompt), 5, NTH).tolist()
        assert a + m.decode_greedy(a[-1], len(prompt) + 5, N_STEPS - 5, NTH).tolist() == want


def test_decode_greedy_multi_picks_the_lower_twin(L, tied):
    """4 sequences at different positions (k_argmax_set)"""
    with L.Model(tied["path"], n_ctx=N_CTX, n_seq=4) as m:
        for i, p in enumerate(tied["prompts"]):
            m.set_seq(i)
            assert int(np.argmax(m.eval(p, 0, NTH))) == tied["streams"][i][0]
        m.set_seq(0)
        got = m.decode_greedy_multi([s[0] for s in tied["streams"]], [len(p) for p in tied["prompts"]], N_STEPS, NTH)
        for i in range(4):
            assert got[i].tolist() == tied["streams"][i][1], f"sequence {i}"


def test_verify_greedy_accepts_the_lower_twin_and_rejects_the_upper(L, tied):
    prompt, (first, want, _) = tied["prompts"][0], tied["streams"][0]
    P = len(prompt)
    with L.Model(tied["path"], n_ctx=N_CTX) as m:
        m.eval(prompt, 0, NTH)
        n_acc, picks = m.verify_greedy(first, want[:-1], P, NTH)          # the true continuation as the draft: all of it is accepted
        assert n_acc == N_STEPS - 1 and picks.tolist() == want
        for j in (0, 4, N_STEPS - 2):
            draft = list(want[:-1])
            draft[j] = _upper_twin(want[j], tied["V"], tied["layout"])      # the same logit, the higher index: not the pick
            m.eval(prompt, 0, NTH)
            n_acc, picks = m.verify_greedy(first, draft, P, NTH)
            assert n_acc == j and picks[:j + 1].tolist() == want[:j + 1], (j, n_acc, picks.tolist())


def test_decode_greedy_lookup_picks_the_lower_twin(L, tied):
    prompt, (first, want, _) = tied["prompts"][0], tied["streams"][0]
    V, layout = tied["V"], tied["layout"]
    with L.Model(tied["path"], n_ctx=N_CTX) as m:
        # drafts from a corpus that holds the true continuation, and from one that holds the upper twins in its place
        for corpus in (np.array([first] + want, np.int32), np.array([first] + [_upper_twin(t, V, layout) for t in want], np.int32), None):
            m.eval(prompt, 0, NTH)
            got, stats = m.decode_greedy_lookup(first, N_STEPS, len(prompt), prompt, corpus=corpus, n_threads=NTH)
            assert got.tolist() == want, stats


def test_pipeline_handle_picks_the_lower_twin(L, tied):
    assert tied["n_layer"] == 2
    prompt, (first, want, _) = tied["prompts"][0], tied["streams"][0]
    with L.Model(tied["path"], n_ctx=N_CTX, devices=[0, 0]) as m:
        assert int(np.argmax(m.eval(prompt, 0, NTH))) == first
        assert m.decode_greedy(first, len(prompt), N_STEPS, NTH).tolist() == want


@pytest.mark.parametrize("layout", ["halves", "neighbours"])
def test_f16_file_of_the_same_tensors(L, tmp_path, layout):
    """the small models' tensors written as f16; no oracle for f16: the expectation is the host-driven loop of eval + np.argmax on the same
    handle"""
    V = SMALL.n_vocab
    tensors = synth.random_tensors(SMALL, seed=31)
    _twin_rows(tensors["output.weight"], layout)
    f16 = str(tmp_path / "m_f16.bin")
    synth.write_model_unquantized(f16, SMALL, tensors, 1)
    prompt = synth.synth_prompt(9, V, seed=49)
    with L.Model(f16, n_ctx=N_CTX, n_seq=2) as m:
        rows = [m.eval(prompt, 0, NTH)]
        toks = [int(np.argmax(rows[0]))]
        for s in range(N_STEPS):
            rows.append(m.eval(np.array([toks[-1]], np.int32), len(prompt) + s, NTH))
            toks.append(int(np.argmax(rows[-1])))
        _assert_every_step_ties(rows, toks, V, layout)
        first, want = toks[0], toks[1:]
        m.eval(prompt, 0, NTH)
        assert m.decode_greedy(first, len(prompt), N_STEPS, NTH).tolist() == want
        m.eval(prompt, 0, NTH)
        n_acc, picks = m.verify_greedy(first, want[:-1], len(prompt), NTH)
        assert n_acc == N_STEPS - 1 and picks.tolist() == want
        draft = list(want[:-1])
        draft[3] = _upper_twin(want[3], V, layout)
        m.eval(prompt, 0, NTH)
        n_acc, picks = m.verify_greedy(first, draft, len(prompt), NTH)
        assert n_acc == 3 and picks[:4].tolist() == want[:4]
        m.eval(prompt, 0, NTH)
        assert m.decode_greedy_lookup(first, N_STEPS, len(prompt), prompt, n_threads=NTH)[0].tolist() == want
        m.set_seq(1)
        m.eval(prompt[:5], 0, NTH)
        m.set_seq(0)
        m.eval(prompt, 0, NTH)
        got = m.decode_greedy_multi([first, int(prompt[5])], [len(prompt), 5], 4, NTH)
        assert got[0].tolist() == want[:4]


# ------------------------------------------------------------------------------------------------ sampled picks
S_SEED, S_TOP_K, S_STEPS, S_RLN = 52, 3, 48, 64


@pytest.fixture(scope="module")
def eighth(tmp_path_factory):
    """one row in eight duplicated: row 8i + 4 := row 8i"""
    path = str(tmp_path_factory.mktemp("eighth") / "m.bin")
    tensors = synth.random_tensors(SMALL, seed=S_SEED)
    _twin_rows(tensors["output.weight"], "eighth")
    synth.write_model(path, SMALL, tensors)
    return path


def sampled_walk(L, oracle, path, top_k=S_TOP_K, n_steps=S_STEPS):
    """the oracle's greedy stream and, per step, (token fed, position, logits, the window of a sampler that has accepted the stream so far,
    the expected flag) -- all of it known on the CPU"""
    prompt = synth.synth_prompt(9, SMALL.n_vocab, seed=2)
    first, toks, rows = _oracle_greedy(oracle, path, prompt, n_steps)
    s = L.Sampler(seed=1, repeat_last_n=S_RLN)
    for t in prompt:
        s.accept(int(t))
    steps = []
    for i, tok in enumerate([first] + toks[:-1]):
        s.accept(tok)
        win = s.window().copy()
        steps.append((tok, len(prompt) + i, rows[i + 1], win, T.expected_flag(rows[i + 1], win, top_k, 1.3, T.F32_TEMP)))
    return prompt, steps


def test_eval_topk_on_a_stream_whose_ties_come_and_go(L, oracle, eighth):
    """exact and inexact selections alternate on one handle's persistent workspace; every step is safe and live by the float64 reference"""
    prompt, steps = sampled_walk(L, oracle, eighth)
    flags = [st[4] for st in steps]
    assert flags.count(T.MUST_BE_EXACT) >= 5 and flags.count(T.MUST_BE_INEXACT) >= 5, flags
    assert any(a != b for a, b in zip(flags, flags[1:]))
    s = L.Sampler(seed=1, repeat_last_n=S_RLN)
    for t in prompt:
        s.accept(int(t))
    with L.Model(eighth, n_ctx=N_CTX) as m:
        m.eval(prompt, 0, NTH)
        for i, (tok, n_past, lg, win, flag) in enumerate(steps):
            s.accept(tok)
            assert s.window().tolist() == win.tolist()
            exact, sc, ids, got_lg = m.eval_topk(np.array([tok], np.int32), n_past, s, top_k=S_TOP_K, n_threads=NTH)
            assert got_lg is None or got_lg.tobytes() == lg.tobytes(), f"step {i}: logits"
            T.check(f"step {i}", lg, win, S_TOP_K, 1.3, T.F32_TEMP, flag, exact, sc, ids)


def test_sampled_decodes_equal_the_single_sequence_loop(L, eighth):
    """decode_sample_multi and decode_sample_lookup on the tie-ridden model against eval_topk -> sample_from_candidates / sample -> accept"""
    S, K = 5, 14
    V = SMALL.n_vocab
    prompts, seeds = [synth.synth_prompt(3 + 2 * i, V, seed=80 + i) for i in range(S)], [11 * i + 2 for i in range(S)]
    with L.Model(eighth, n_ctx=N_CTX, n_seq=S) as h, L.Model(eighth, n_ctx=N_CTX, n_seq=S) as one:
        samplers, firsts = _prefill(L, h, prompts, seeds, NTH, top_k=S_TOP_K)
        got, exact = h.decode_sample_multi(firsts, [len(p) for p in prompts], K, samplers, top_k=S_TOP_K, n_threads=NTH, want_exact=True)
        ref_samplers, ref_firsts = _prefill(L, one, prompts, seeds, NTH, top_k=S_TOP_K)
        assert ref_firsts == firsts
        for i in range(S):
            toks, flags = _single_stream(L, one, i, firsts[i], len(prompts[i]), ref_samplers[i], K, NTH, top_k=S_TOP_K)
            assert got[i].tolist() == toks and exact[i].tolist() == flags, f"sequence {i}"
            assert samplers[i].window().tolist() == ref_samplers[i].window().tolist()
        assert 0 < exact.sum() < exact.size, exact
    with L.Model(eighth, n_ctx=N_CTX, n_seq=2) as h:
        truth = _truth(L, h, prompts[2], 40, NTH, seed=5, rln=S_RLN, top_k=S_TOP_K)
        assert 0 < sum(truth["flags"]) < 40, truth["flags"]
        h.set_seq(1)
        for corpus in (None, np.array([truth["first"]] + truth["G"], np.int32)):
            ex, st = _lookup_run(L, h, truth, corpus)
            assert ex.tolist() == truth["flags"], st
