"""GPU (-m gpu): greedy decode with drafted tokens verified in one multi-row eval (llamahip_verify_greedy, llamahip_decode_greedy_lookup,
kernels k_verify_rows / k_accept_drafts).

The feature's claim is that the token stream, the last logits and the KV cache are llamahip_decode_greedy's, bit for bit.  It rests on one
fact -- row j of an eval at n_past whose rows each take the V*P key split of their own single-token eval (eval_chunks with chunk_tokens = 1)
is the single-token eval at n_past + j -- which is tested first; then the two kernels against numpy, one verify step against a known
answer, and the loop against decode_greedy on plain, pipeline, dense, Q4_1 and un-captured handles, its step counts against the Python
restatement of drafter and accept rule (tests/lookup_ref.py)."""
import os

import numpy as np
import pytest

import lookup_ref
import synth
from conftest import synth_tool

pytestmark = pytest.mark.gpu
SMALL = dict(n_vocab=2000, n_embd=512, n_mult=256, n_head=4, n_layer=3)
W7B = dict(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=2)
W13B = dict(n_vocab=512, n_embd=5120, n_mult=256, n_head=40, n_layer=2)
SHAPES = {"small": SMALL, "7b_width": W7B, "13b_width": W13B}
NO_GRAPH = 1


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _kv_equal(h, n_layer, n, slots=(0, 1)):
    """KV rows [0, n) of every layer: slot slots[1] against slot slots[0]"""
    bad = []
    for il in range(n_layer):
        h.set_seq(slots[0])
        k0, v0 = h.kv(il, n)
        h.set_seq(slots[1])
        k1, v1 = h.kv(il, n)
        if not (same(k0, k1) and same(v0, v1)):
            rows = np.flatnonzero((k0 != k1).any(axis=1) | (v0 != v1).any(axis=1))
            bad.append((il, rows[:6].tolist()))
    h.set_seq(slots[0])
    return bad


# ------------------------------------------------------------------------------------------------ 1. the ground it stands on
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_rows_of_a_chunk_1_eval_are_single_token_evals(L, tmp_path, shape):
    """eval_chunks(tokens, n_past, chunk_tokens=1) of 2, 5, 9 and 16 rows leaves KV rows and last-row logits bit-identical to that many
    single-token evals, n_threads 1 / 3 / 8; the 16 rows at positions 116 .. 131 straddle a 128-key slice boundary"""
    kw = SHAPES[shape]
    path = synth_tool(tmp_path / "m.bin", seed=61, **kw)
    V = kw["n_vocab"]
    prompt = synth.synth_prompt(100, V, seed=5)
    rng = np.random.default_rng(17)
    with L.Model(path, n_ctx=160, n_seq=2) as h:
        for nth in (1, 3, 8):
            for s in (0, 1):
                h.set_seq(s)
                h.eval(prompt, 0, nth)
            n_past = 100
            for N in (2, 5, 9, 16):
                toks = rng.integers(3, V, N).astype(np.int32)
                h.set_seq(0)
                for j in range(N):
                    want = h.eval(toks[j:j + 1], n_past + j, nth)
                h.set_seq(1)
                got = h.eval_chunks(toks, n_past, 1, nth)
                assert same(got, want), (shape, nth, N, "last-row logits")
                n_past += N
                assert not _kv_equal(h, kw["n_layer"], n_past), (shape, nth, N, "KV rows")
            assert n_past == 132


# ------------------------------------------------------------------------------------------------ 2. the two kernels against numpy
def _np_pick(row):
    return 0 if np.isnan(row).all() else int(np.nanargmax(row))          # (first index of the largest non-NaN value)


def _verify_rows_case(L, lg, note):
    N, V = lg.shape
    want = np.array([_np_pick(r) for r in lg], np.int32)
    rng = np.random.default_rng(N * 7 + V)
    for agree in sorted({0, N // 2, N - 1}):
        # tokens[j + 1] = the pick of row j for j < agree, something else at `agree`, anything behind it
        toks = rng.integers(0, V, N).astype(np.int32)
        toks[1:agree + 1] = want[:agree]
        if agree + 1 < N:
            toks[agree + 1] = (want[agree] + 1) % V if V > 1 else want[agree]
        n_acc, picks = L.op_verify_rows(lg, toks)
        assert picks.tolist() == want.tolist(), (note, N, V, agree)
        assert n_acc == lookup_ref.n_accept(toks, want), (note, N, V, agree)
        if V > 1:
            assert n_acc == agree, (note, N, V, agree)


@pytest.mark.parametrize("V", [1200, 32000, 32768])
@pytest.mark.parametrize("N", [1, 2, 7, 16])
def test_op_verify_rows_against_numpy(L, N, V):
    rng = np.random.default_rng(N * 100003 + V)
    _verify_rows_case(L, (rng.standard_normal((N, V)) * 3).astype(np.float32), "random")
    ties = (rng.integers(-40, 41, (N, V)) * 0.25).astype(np.float32)          # quarter steps: the maximum occurs many times over
    assert all((r == r.max()).sum() > 1 for r in ties)
    _verify_rows_case(L, ties, "ties")
    # non-finite entries: NaNs scattered over a row, a NaN at the front of a tie, a +inf, a row of only -inf, a row of only NaN, -0 / +0
    odd = (rng.integers(-40, 41, (N, V)) * 0.25).astype(np.float32)
    for r in range(N):
        kind = r % 6
        if kind == 0:
            odd[r, rng.integers(0, V, V // 10)] = np.nan
            odd[r, 0] = np.nan
        elif kind == 1:
            odd[r, rng.integers(0, V)] = np.inf
            odd[r, rng.integers(0, V, 5)] = np.nan
        elif kind == 2:
            odd[r] = -np.inf
        elif kind == 3:
            odd[r] = np.nan
        elif kind == 4:
            odd[r] = -1.0
            odd[r, V // 2] = -0.0
            odd[r, V - 1] = 0.0
        else:
            odd[r] = -np.inf
            odd[r, V - 1] = np.nan
            odd[r, V // 3] = -3.0e38
    _verify_rows_case(L, odd, "non-finite")


def test_op_verify_rows_takes_any_vocabulary_size(L):
    rng = np.random.default_rng(2)
    for V in (1, 2, 63, 1025, 32769, 50001):
        _verify_rows_case(L, (rng.integers(-8, 9, (5, V)) * 0.5).astype(np.float32), "sizes")
    with pytest.raises(L.LlamaHipError, match=r"n_rows 17 of 1 \.\. 16"):
        L.op_verify_rows(np.zeros((17, 8), np.float32), np.zeros(17, np.int32))


# ------------------------------------------------------------------------------------------------ 3. one verify step, known answer
def _truth(h, prompt, T, nth):
    """slot 0: the prompt, then T single greedy steps -- the stream S (S[i] = the token at position P + i; S[i + 1] = the pick there) and
    every step's logits; checked against ONE decode_greedy call of T steps on slot 1, which leaves slot 1 holding the same rows"""
    P = len(prompt)
    for s in (0, 1):
        h.set_seq(s)
        first = int(np.argmax(h.eval(prompt, 0, nth)))
    h.set_seq(0)
    S, LG = [first], []
    for i in range(T):
        t, lg = h.decode_greedy(S[i], P + i, 1, nth, want_logits=True)
        S.append(int(t[0]))
        LG.append(lg)
    h.set_seq(1)
    G = h.decode_greedy(first, P, T, nth)
    assert G.tolist() == S[1:]
    h.set_seq(0)
    return S, LG


@pytest.mark.parametrize("shape,nth", [("small", 8), ("small", 3), ("7b_width", 8), ("13b_width", 8)])
def test_verify_greedy_with_a_known_answer(L, tmp_path, shape, nth):
    kw = SHAPES[shape]
    V, P, T = kw["n_vocab"], 9, 60
    path = synth_tool(tmp_path / "m.bin", seed=62, **kw)
    prompt = synth.synth_prompt(P, V, seed=8)
    with L.Model(path, n_ctx=96, n_seq=2) as h:
        S, LG = _truth(h, prompt, T, nth)
        # slot 1 holds the true rows [0, P + T): a verify at start i needs [0, P + i) and rewrites rows from P + i on -- so the starts go
        # in descending order, every one finds the rows below it untouched
        for i in (40, 7, 0):
            for K in (1, 4, 8, 15):
                for c in (0, K // 2, None):
                    d = np.array(S[i + 1:i + 1 + K], np.int32)
                    if c is not None:
                        d[c] = (d[c] + 1) % V
                    want_acc = K if c is None else c
                    h.set_seq(1)
                    n_acc, picks, lg = h.verify_greedy(S[i], d, P + i, nth, want_logits=True)
                    tag = (shape, nth, i, K, c)
                    assert n_acc == want_acc, tag
                    assert picks[:n_acc + 1].tolist() == S[i + 1:i + n_acc + 2], tag
                    assert same(lg, LG[i + n_acc]), tag
                    assert not _kv_equal(h, kw["n_layer"], P + i + n_acc + 1), tag
        # n_draft = 0 is one plain step; a draft that would pass n_ctx is refused
        h.set_seq(1)
        n_acc, picks, lg = h.verify_greedy(S[3], [], P + 3, nth, want_logits=True)
        assert (n_acc, picks.tolist()) == (0, [S[4]]) and same(lg, LG[3])
        with pytest.raises(L.LlamaHipError, match=r"n_past \(90\) \+ n_draft \(6\) \+ 1 > n_ctx \(96\)"):
            h.verify_greedy(5, [1] * 6, 90, nth)


def test_verify_greedy_without_the_pinned_block(tmp_path):
    """LLAMAHIP_NO_HOST_IO: tokens and results travel as small copies instead of through the mapped host block (a fresh process: the
    switch is read at load)"""
    import subprocess
    import sys
    path = synth_tool(tmp_path / "m.bin", seed=62, **SMALL)
    code = f"""
import sys
sys.path[:0] = [{os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r}, {os.path.dirname(os.path.abspath(__file__))!r}]
import numpy as np, llama_swift_amd as L, synth
prompt = synth.synth_prompt(9, 2000, seed=8)
with L.Model({path!r}, n_ctx=64, n_seq=2) as h:
    for s in (0, 1):
        h.set_seq(s)
        first = int(np.argmax(h.eval(prompt, 0, 8)))
    h.set_seq(0)
    G, lg = h.decode_greedy(first, 9, 24, 8, want_logits=True)
    S = [first] + G.tolist()
    h.set_seq(1)
    d = np.array(S[1:9], np.int32); d[5] += 1
    n_acc, picks = h.verify_greedy(S[0], d, 9, 8)
    assert n_acc == 5 and picks[:6].tolist() == S[1:7], (n_acc, picks)
    out, st, lg2 = h.decode_greedy_lookup(first, 24, 9, prompt, corpus=G, want_logits=True)
    assert out.tolist() == G.tolist() and np.array_equal(lg.view(np.uint32), lg2.view(np.uint32)) and st["n_accepted"] > 0, st
print("NO_HOST_IO_OK")
"""
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LLAMAHIP_NO_HOST_IO="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "NO_HOST_IO_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ 4. the loop equals decode_greedy
def _corrupt(G, V):
    c = np.array(G, np.int32)
    c[6::7] = (c[6::7] + 1) % V          # every 7th token is not the true one
    return c


def _lookup_case(h, n_layer, prompt, n_steps, nth, corpus_of, **kw):
    """slot 0: decode_greedy; slot 1: decode_greedy_lookup with corpus_of(G) -- tokens, last logits, KV rows [0, P + n_steps) bit for bit,
    step counts as the restatement predicts.  Returns (G, stats)."""
    P = len(prompt)
    for s in (0, 1):
        h.set_seq(s)
        first = int(np.argmax(h.eval(prompt, 0, nth)))
    h.set_seq(0)
    G, lg = h.decode_greedy(first, P, n_steps, nth, want_logits=True)
    corpus = corpus_of(G)
    h.set_seq(1)
    out, st, lg2 = h.decode_greedy_lookup(first, n_steps, P, prompt, corpus=corpus, n_threads=nth, want_logits=True, **kw)
    assert out.tolist() == G.tolist(), (st, np.flatnonzero(out != G)[:5])
    assert same(lg, lg2), "logits_last"
    assert not _kv_equal(h, n_layer, P + n_steps), "KV rows"
    want = lookup_ref.loop_stats(prompt, first, G, corpus, kw.get("draft_len", 0), kw.get("ngram_min", 0), kw.get("ngram_max", 0))
    assert st == want, (st, want)
    assert st["n_verify_steps"] + st["n_single_steps"] + st["n_accepted"] == n_steps
    h.set_seq(0)
    return G, st


_CORPORA = {"a_no_corpus": lambda V: (lambda G: None), "b_true_stream": lambda V: (lambda G: G), "c_every_7th_wrong": lambda V: (lambda G: _corrupt(G, V))}


def _check_stats(case, st, n_steps):
    if case.startswith("b"):
        assert st["n_accepted"] > 0 and st["n_verify_steps"] + st["n_single_steps"] < n_steps, st
    if case.startswith("c"):
        assert 0 < st["n_accepted"] < st["n_drafted"], st          # an acceptance AND a rejection were seen


@pytest.mark.parametrize("case", sorted(_CORPORA))
@pytest.mark.parametrize("shape,nth", [("small", 8), ("small", 1), ("7b_width", 8), ("13b_width", 3)])
def test_lookup_equals_decode_greedy(L, tmp_path, shape, nth, case):
    kw = SHAPES[shape]
    path = synth_tool(tmp_path / "m.bin", seed=63, **kw)
    prompt = synth.synth_prompt(12, kw["n_vocab"], seed=9)
    n_steps = 150           # (positions 12 .. 161: over the 128-key slice boundary)
    with L.Model(path, n_ctx=192, n_seq=2) as h:
        _, st = _lookup_case(h, kw["n_layer"], prompt, n_steps, nth, _CORPORA[case](kw["n_vocab"]))
        _check_stats(case, st, n_steps)


def test_lookup_run_that_ends_exactly_at_n_ctx(L, tmp_path):
    path = synth_tool(tmp_path / "m.bin", seed=63, **SMALL)
    prompt = synth.synth_prompt(12, SMALL["n_vocab"], seed=9)
    with L.Model(path, n_ctx=80, n_seq=2) as h:
        for case in ("b_true_stream", "c_every_7th_wrong"):
            _, st = _lookup_case(h, SMALL["n_layer"], prompt, 68, 8, _CORPORA[case](SMALL["n_vocab"]))
            _check_stats(case, st, 68)
        with pytest.raises(L.LlamaHipError, match=r"n_past \(12\) \+ n_steps \(69\) > n_ctx \(80\)"):
            h.decode_greedy_lookup(5, 69, 12, prompt)


@pytest.mark.parametrize("draft_len", [1, 15])
def test_lookup_draft_lengths_1_and_15(L, tmp_path, draft_len):
    path = synth_tool(tmp_path / "m.bin", seed=63, **SMALL)
    prompt = synth.synth_prompt(12, SMALL["n_vocab"], seed=9)
    with L.Model(path, n_ctx=128, n_seq=2) as h:
        for case in ("b_true_stream", "c_every_7th_wrong"):
            _, st = _lookup_case(h, SMALL["n_layer"], prompt, 100, 8, _CORPORA[case](SMALL["n_vocab"]), draft_len=draft_len)
            if draft_len == 15:
                _check_stats(case, st, 100)
            else:
                assert st["n_drafted"] == st["n_verify_steps"] > 0, st
        _lookup_case(h, SMALL["n_layer"], prompt, 100, 8, _CORPORA["b_true_stream"](0), draft_len=draft_len, ngram_min=2, ngram_max=5)


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["two_stages", "three_stages"])
def test_lookup_on_pipeline_handles(L, tmp_path, devices):
    kw = dict(SMALL, n_layer=5) if len(devices) == 3 else W7B
    path = synth_tool(tmp_path / "m.bin", seed=64, **kw)
    prompt = synth.synth_prompt(12, kw["n_vocab"], seed=9)
    n_steps = 60
    with L.Model(path, n_ctx=96, n_seq=2, devices=devices) as pm, L.Model(path, n_ctx=96) as one:
        one.eval(prompt, 0, 8)
        want = one.decode_greedy(int(np.argmax(one.eval(prompt, 0, 8))), 12, n_steps, 8)
        for case in sorted(_CORPORA):
            G, st = _lookup_case(pm, kw["n_layer"], prompt, n_steps, 8, _CORPORA[case](kw["n_vocab"]))
            assert G.tolist() == want.tolist()
            _check_stats(case, st, n_steps)
        # one verify step on the pipeline: the plain handle's answer
        S = [int(np.argmax(one.eval(prompt, 0, 8)))] + want.tolist()
        d = np.array(S[1:9], np.int32)
        d[4] = (d[4] + 1) % kw["n_vocab"]
        pm.set_seq(1)
        one.eval(prompt, 0, 8)
        a = pm.verify_greedy(S[0], d, 12, 8, want_logits=True)
        b = one.verify_greedy(S[0], d, 12, 8, want_logits=True)
        assert a[0] == b[0] == 4 and a[1].tolist() == b[1].tolist() and same(a[2], b[2])


@pytest.mark.parametrize("kind", ["f16", "q4_1"])
def test_lookup_on_files_without_a_per_row_key_split(L, tmp_path, kind):
    """f16 / Q4_1 files: the loop is decode_greedy and reports zero drafts; a verify step runs its rows one by one and stops at the mismatch"""
    hp = synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=4, n_layer=2)
    path = str(tmp_path / "m.bin")
    src = path + ".f16" if kind == "q4_1" else path
    synth.write_model_unquantized(src, hp, synth.random_tensors(hp, seed=9), 1)
    if kind == "q4_1":
        L.quantize_file(src, path, 3)
    prompt = synth.synth_prompt(12, hp.n_vocab, seed=9)
    for devices in (None, [0, 0]):
        with L.Model(path, n_ctx=64, n_seq=2, devices=devices) as h:
            G, st = _dense_case(h, hp, prompt)
            assert st == dict(n_verify_steps=0, n_single_steps=40, n_drafted=0, n_accepted=0)
            S = [int(np.argmax(h.eval(prompt, 0, 8)))] + G.tolist()
            d = np.array(S[1:7], np.int32)
            d[3] = (d[3] + 1) % hp.n_vocab
            h.set_seq(1)
            n_acc, picks, lg = h.verify_greedy(S[0], d, 12, 8, want_logits=True)
            assert n_acc == 3 and picks.tolist() == S[1:5] + [-1, -1, -1]
            h.set_seq(0)
            assert same(lg, h.decode_greedy(S[3], 15, 1, 8, want_logits=True)[1])
            assert not _kv_equal(h, hp.n_layer, 16)


def _dense_case(h, hp, prompt):
    P, n_steps = len(prompt), 40
    for s in (0, 1):
        h.set_seq(s)
        first = int(np.argmax(h.eval(prompt, 0, 8)))
    h.set_seq(0)
    G, lg = h.decode_greedy(first, P, n_steps, 8, want_logits=True)
    h.set_seq(1)
    out, st, lg2 = h.decode_greedy_lookup(first, n_steps, P, prompt, corpus=G, want_logits=True)
    assert out.tolist() == G.tolist() and same(lg, lg2)
    assert not _kv_equal(h, hp.n_layer, P + n_steps)
    return G, st


@pytest.mark.parametrize("flags", [NO_GRAPH, 2], ids=["no_graph", "unfused"])
def test_lookup_with_eager_and_unfused_steps(L, tmp_path, flags):
    path = synth_tool(tmp_path / "m.bin", seed=63, **SMALL)
    prompt = synth.synth_prompt(12, SMALL["n_vocab"], seed=9)
    with L.Model(path, n_ctx=96, n_seq=2, flags=flags) as h:
        for case in sorted(_CORPORA):
            _, st = _lookup_case(h, SMALL["n_layer"], prompt, 70, 8, _CORPORA[case](SMALL["n_vocab"]))
            _check_stats(case, st, 70)


def test_lookup_refuses_a_stage_handle(L, tmp_path):
    path = synth_tool(tmp_path / "m.bin", seed=63, **SMALL)
    with L.Model(path, n_ctx=64, layer_begin=0, layer_end=2) as st:
        with pytest.raises(L.LlamaHipError, match="pipeline-stage handle"):
            st.verify_greedy(5, [1, 2], 0)
        with pytest.raises(L.LlamaHipError, match="pipeline-stage handle"):
            st.decode_greedy_lookup(5, 4, 0, [])


# ------------------------------------------------------------------------------------------------ 5. the full-depth 7B
def test_lookup_on_the_full_depth_7b(L):
    path = os.path.join(os.environ.get("LLAMAHIP_MODEL_DIR", "/tmp/llamahip_models"), "7B-seed20230312", "ggml-model-q4_0.bin")
    if not os.path.exists(path + ".done"):
        pytest.skip("the full-depth synthetic 7B file is not on this machine (tests/test_gpu_fullsize.py writes it)")
    prompt = synth.synth_prompt(16, 32000, seed=4)
    with L.Model(path, n_ctx=512, n_seq=2) as h:
        _, st = _lookup_case(h, 32, prompt, 256, 8, lambda G: _corrupt(G, 32000))
        _check_stats("c", st, 256)
