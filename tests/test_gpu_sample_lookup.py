"""GPU (-m gpu): sampled decode with drafted tokens verified in one multi-row eval (llamahip_verify_sample, llamahip_decode_sample_lookup,
llamahip_op_topk_slide, kernel k_topk_keys_slide; the runner's lookup steps).

The claim is that the token stream, the exact flags, the sampler's window and rng state and the KV cache are those of the documented
single-sequence loop  eval_topk -> sample_from_candidates (exact) / sample (not exact) -> accept,  bit for bit.  It rests on the fact tested in
tests/test_gpu_lookup.py (row j of a chunk-1 eval is the single-token eval at n_past + j) and on the device half tested first here: row r of
op_topk_slide is op_topk on that row with the window ids[r : r + n_last].  (The single-op entry point owns its workspace, so its second call
only shows that two calls agree; that the selection clears its per-row workspace between calls is what every model-level test below shows --
a handle runs all its verify steps on one workspace.)"""
import json
import os
import subprocess
import sys

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
PAIRS = [("small", 8), ("small", 3), ("7b_width", 8), ("13b_width", 8)]
NO_GRAPH, UNFUSED = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = dict(n_verify_steps=0, n_single_steps=0, n_drafted=0, n_accepted=0)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _kv_rows(h, n_layer, n):
    return [h.kv(il, n) for il in range(n_layer)]


def _kv_same(a, b):
    return all(same(ka, kb) and same(va, vb) for (ka, va), (kb, vb) in zip(a, b))


def _rng_print(s):
    """the sampler's rng state, by what it draws next: 8 draws over 64 equally likely candidates (this consumes them: last use of s)"""
    return [s.sample_from_candidates(np.zeros(64), np.arange(64, dtype=np.int32), top_p=1.0) for _ in range(8)]


# ------------------------------------------------------------------------------------------------ 1. the device half
def _rows(rng, R, V):
    """the rows of tests/test_gpu_sample_multi.py: plain, tie-heavy (quarter steps, some with a little noise), a NaN row and a +inf row (R > 1)"""
    lg = np.empty((R, V), np.float32)
    for r in range(R):
        kind = r % 5
        if kind in (0, 3):
            lg[r] = rng.standard_normal(V) * 3
        else:
            lg[r] = rng.integers(-40, 41, V) * 0.25
            if kind == 2:
                lg[r] += (rng.standard_normal(V) * 1e-3).astype(np.float32) * (rng.random(V) < 0.5)
        if R > 1 and r == 3:
            lg[r, rng.integers(0, V)] = np.nan
        if R > 1 and r == min(8, R - 1):
            lg[r, rng.integers(0, V)] = np.inf
    return lg


@pytest.mark.parametrize("V", [1200, 32000, 32768])
@pytest.mark.parametrize("R", [1, 2, 16])
def test_op_topk_slide_is_op_topk_row_by_row(L, R, V):
    rng = np.random.default_rng(R * 100003 + V)
    lg = _rows(rng, R, V)
    flags = []
    for n_last in (0, 1, 64, 1024):
        ids = rng.integers(0, V, n_last + R - 1).astype(np.int32)
        if ids.size:                                    # ids outside [0, V): ignored, as the host sampler ignores them
            ids[rng.integers(0, ids.size, max(1, ids.size // 8))] = rng.choice([-1, -7, V, V + 3, 2**31 - 1, -2**31], max(1, ids.size // 8))
        for k in ((1, 40, 64) if n_last == 64 else (40,)):
            first = L.op_topk_slide(lg, ids, n_last, top_k=k)
            again = L.op_topk_slide(lg, ids, n_last, top_k=k)          # a second call straight after the first
            ref = [L.op_topk(lg[r], ids[r:r + n_last], top_k=k) for r in range(R)]
            for exact, sc, out_ids in (first, again):
                assert sc.shape == (R, k) and out_ids.shape == (R, k)
                for r, (e1, s1, i1) in enumerate(ref):
                    assert exact[r] == e1, (R, V, n_last, k, r)
                    assert same(sc[r], s1) and same(out_ids[r], i1), (R, V, n_last, k, r)
            flags += first[0].tolist()
    if R == 16:
        assert any(flags) and not all(flags), flags          # exact rows and inexact rows (ties, the NaN row) were both seen


# ------------------------------------------------------------------------------------------------ the single-sequence loop (the yardstick)
def _start(L, h, prompt_logits, prompt, seed, rln, top_k=40):
    """a fresh sampler that has accepted the prompt and drawn + accepted the first token from the prompt's logits"""
    s = L.Sampler(seed=seed, repeat_last_n=rln)
    for t in prompt:
        s.accept(int(t))
    first = s.sample(h, prompt_logits, top_k=top_k)
    s.accept(first)
    return s, first


def _loop(h, sampler, tok, n_past, n_steps, nth, top_k=40):
    """eval_topk -> sample_from_candidates (exact) / sample (not exact) -> accept, n_steps times on the current slot"""
    toks, flags = [], []
    for t in range(n_steps):
        exact, sc, ids, lg = h.eval_topk(np.array([tok], np.int32), n_past + t, sampler, top_k=top_k, n_threads=nth)
        tok = sampler.sample_from_candidates(sc, ids) if exact else sampler.sample(h, lg, top_k=top_k)
        sampler.accept(tok)
        toks.append(tok)
        flags.append(int(exact))
    return toks, flags


# ------------------------------------------------------------------------------------------------ 2. one verify step, known answer
@pytest.mark.parametrize("shape,nth", PAIRS)
def test_verify_sample_with_a_known_answer(L, tmp_path, shape, nth):
    """slot 0: the loop; slot 1: ONE verify_sample with a second sampler of the same seed and the same accepts.  A correct draft of 15 is
    accepted whole, a draft wrong at 5 up to there, no draft is one step; afterwards windows, rng states and KV rows [0, context) agree.
    P = 120: the 16 rows at positions 120 .. 135 straddle the 128-key slice boundary."""
    kw = SHAPES[shape]
    V, seed = kw["n_vocab"], 11
    path = synth_tool(tmp_path / "m.bin", seed=62, **kw)
    with L.Model(path, n_ctx=160, n_seq=2) as h:
        for P in (9, 120):
            prompt = synth.synth_prompt(P, V, seed=8)
            for s in (1, 0):
                h.set_seq(s)
                plg = h.eval(prompt, 0, nth)
            ahead, first = _start(L, h, plg, prompt, seed, 64)
            S = [first] + _loop(h, ahead, first, P, 16, nth)[0]          # S[i] = the token at position P + i
            for case, wrong in (("all_15", None), ("wrong_at_5", 5), ("no_draft", None)):
                d = np.array([] if case == "no_draft" else S[1:16], np.int32)
                if wrong is not None:
                    d[wrong] = (d[wrong] + 1) % V
                want_acc = 0 if case == "no_draft" else (15 if wrong is None else wrong)
                s1, f1 = _start(L, h, plg, prompt, seed, 64)
                s2, f2 = _start(L, h, plg, prompt, seed, 64)
                assert f1 == f2 == first
                h.set_seq(1)
                n_acc, picks, exact = h.verify_sample(first, d, P, s2, n_threads=nth)
                got_kv = _kv_rows(h, kw["n_layer"], P + n_acc + 1)
                h.set_seq(0)
                toks, flags = _loop(h, s1, first, P, want_acc + 1, nth)
                tag = (shape, nth, P, case)
                assert toks == S[1:want_acc + 2], tag
                assert n_acc == want_acc, tag + (n_acc, picks.tolist())
                assert picks[:n_acc + 1].tolist() == toks and picks[n_acc + 1:].tolist() == [-1] * (d.size - n_acc), tag + (picks.tolist(),)
                assert exact[:n_acc + 1].tolist() == flags and exact[n_acc + 1:].tolist() == [-1] * (d.size - n_acc), tag + (exact.tolist(), flags)
                assert s2.window().tolist() == s1.window().tolist(), tag
                assert _rng_print(s2) == _rng_print(s1), tag
                assert _kv_same(got_kv, _kv_rows(h, kw["n_layer"], P + n_acc + 1)), tag
        with pytest.raises(L.LlamaHipError, match=r"n_past \(154\) \+ n_draft \(6\) \+ 1 > n_ctx \(160\)"):
            h.verify_sample(5, [1] * 6, 154, L.Sampler(seed=1), n_threads=nth)


# ------------------------------------------------------------------------------------------------ 3. the loop equals the single-sequence loop
def _corrupt(G, V):
    c = np.array(G, np.int32)
    c[6::7] = (c[6::7] + 1) % V          # every 7th token is not the true one
    return c


_CORPORA = {"a_no_corpus": lambda G, V: None, "b_true_stream": lambda G, V: np.array(G, np.int32), "c_every_7th_wrong": _corrupt}


def _check_stats(case, st, n_steps):
    assert st["n_verify_steps"] + st["n_single_steps"] + st["n_accepted"] == n_steps, st
    if case.startswith("b"):
        assert st["n_accepted"] > 0 and st["n_verify_steps"] + st["n_single_steps"] < n_steps, st
    if case.startswith("c"):
        assert 0 < st["n_accepted"] < st["n_drafted"], st          # an acceptance AND a rejection were seen


def _truth(L, h, prompt, n_steps, nth, seed, rln, top_k=40, slots=(0, 1)):
    """the prompt on both slots, then the loop on slots[0]: everything the lookup runs are compared with, computed once"""
    for s in reversed(slots):
        h.set_seq(s)
        plg = h.eval(prompt, 0, nth)
    s1, first = _start(L, h, plg, prompt, seed, rln, top_k)
    G, flags = _loop(h, s1, first, len(prompt), n_steps, nth, top_k)
    return dict(plg=plg, first=first, G=G, flags=flags, window=s1.window().tolist(), rng=_rng_print(s1), prompt=prompt, seed=seed, rln=rln, top_k=top_k,
                n_steps=n_steps, nth=nth)


def _lookup_run(L, h, T, corpus, **kw):
    """decode_sample_lookup on the current slot with a fresh sampler of the truth's seed: tokens, flags, window, rng state against the truth"""
    P = len(T["prompt"])
    s2, first = _start(L, h, T["plg"], T["prompt"], T["seed"], T["rln"], T["top_k"])
    assert first == T["first"]
    out, exact, st = h.decode_sample_lookup(first, T["n_steps"], P, T["prompt"], s2, corpus=corpus, top_k=T["top_k"], n_threads=T["nth"], **kw)
    assert out.tolist() == T["G"], (st, np.flatnonzero(out != np.array(T["G"]))[:5])
    assert s2.window().tolist() == T["window"]
    assert _rng_print(s2) == T["rng"]
    return exact, st


@pytest.mark.parametrize("shape,nth", PAIRS)
def test_sample_lookup_equals_the_loop(L, tmp_path, shape, nth):
    kw = SHAPES[shape]
    V, n_steps = kw["n_vocab"], 150          # (positions 12 .. 161: over the 128-key slice boundary)
    path = synth_tool(tmp_path / "m.bin", seed=63, **kw)
    prompt = synth.synth_prompt(12, V, seed=9)
    with L.Model(path, n_ctx=192, n_seq=2) as h:
        T = _truth(L, h, prompt, n_steps, nth, seed=21, rln=64)
        want_kv = _kv_rows(h, kw["n_layer"], 12 + n_steps)
        h.set_seq(1)
        for case in sorted(_CORPORA):
            corpus = _CORPORA[case](T["G"], V)
            exact, st = _lookup_run(L, h, T, corpus)
            assert exact.tolist() == T["flags"], case
            assert _kv_same(_kv_rows(h, kw["n_layer"], 12 + n_steps), want_kv), case
            assert st == lookup_ref.loop_stats(prompt, T["first"], T["G"], corpus), (case, st)
            _check_stats(case, st, n_steps)


@pytest.mark.parametrize("rln", [64, 0, 200])
def test_sample_lookup_windows_and_a_run_that_ends_exactly_at_n_ctx(L, tmp_path, rln):
    """repeat_last_n 64 / 0 (no window: the id stream is the draft alone) / 200; 68 steps from 12 tokens at n_ctx 80 end exactly at n_ctx"""
    path = synth_tool(tmp_path / "m.bin", seed=63, **SMALL)
    V, n_steps = SMALL["n_vocab"], 68
    prompt = synth.synth_prompt(12, V, seed=9)
    with L.Model(path, n_ctx=80, n_seq=2) as h:
        T = _truth(L, h, prompt, n_steps, 8, seed=22, rln=rln)
        want_kv = _kv_rows(h, SMALL["n_layer"], 80)
        h.set_seq(1)
        for case in ("b_true_stream", "c_every_7th_wrong"):
            corpus = _CORPORA[case](T["G"], V)
            exact, st = _lookup_run(L, h, T, corpus)
            assert exact.tolist() == T["flags"] and _kv_same(_kv_rows(h, SMALL["n_layer"], 80), want_kv), (rln, case)
            assert st == lookup_ref.loop_stats(prompt, T["first"], T["G"], corpus), (rln, case, st)
            _check_stats(case, st, n_steps)
        with pytest.raises(L.LlamaHipError, match=r"n_past \(12\) \+ n_steps \(69\) > n_ctx \(80\)"):
            h.decode_sample_lookup(5, 69, 12, prompt, L.Sampler(seed=1))


def test_sample_lookup_where_the_device_cannot_make_candidates(L, tmp_path):
    """top_k = 65 and a window of 1100 ids: zero drafts, the loop's tokens; one verify_sample there draws every row it reaches from its logits"""
    path = synth_tool(tmp_path / "m.bin", seed=63, **SMALL)
    V, n_steps = SMALL["n_vocab"], 40
    prompt = synth.synth_prompt(12, V, seed=9)
    with L.Model(path, n_ctx=64, n_seq=2) as h:
        for top_k, rln in ((65, 64), (40, 1100)):
            T = _truth(L, h, prompt, n_steps, 8, seed=23, rln=rln, top_k=top_k)
            assert not any(T["flags"])
            h.set_seq(1)
            exact, st = _lookup_run(L, h, T, np.array(T["G"], np.int32))
            assert not exact.any() and st == dict(ZERO, n_single_steps=n_steps), (top_k, rln, st)
            s2, first = _start(L, h, T["plg"], prompt, 23, rln, top_k)
            d = np.array(T["G"][:8], np.int32)
            d[5] = (d[5] + 1) % V
            n_acc, picks, ex = h.verify_sample(first, d, 12, s2, top_k=top_k)
            assert n_acc == 5 and picks[:6].tolist() == T["G"][:6] and ex.tolist() == [0] * 6 + [-1] * 3, (top_k, rln, n_acc, picks, ex)


# ------------------------------------------------------------------------------------------------ 4. handles and files
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=["two_stages", "three_stages"])
def test_sample_lookup_on_pipeline_handles(L, tmp_path, devices):
    """against the PLAIN handle's loop: tokens, window, rng state, KV rows, step counts.  (eval_topk on a pipeline handle returns the logits
    row, so the flags of single steps are 0 there; verify rows carry the last stage's selection: the plain handle's flags.)"""
    kw = dict(SMALL, n_layer=5) if len(devices) == 3 else W7B
    V, n_steps = kw["n_vocab"], 60
    path = synth_tool(tmp_path / "m.bin", seed=64, **kw)
    prompt = synth.synth_prompt(12, V, seed=9)
    with L.Model(path, n_ctx=96, n_seq=2, devices=devices) as pm, L.Model(path, n_ctx=96) as one:
        T = _truth(L, one, prompt, n_steps, 8, seed=24, rln=64, slots=(0,))
        want_kv = _kv_rows(one, kw["n_layer"], 12 + n_steps)
        pm.set_seq(1)
        assert same(pm.eval(prompt, 0, 8), T["plg"])
        for case in sorted(_CORPORA):
            corpus = _CORPORA[case](T["G"], V)
            exact, st = _lookup_run(L, pm, T, corpus)
            assert _kv_same(_kv_rows(pm, kw["n_layer"], 12 + n_steps), want_kv), case
            assert st == lookup_ref.loop_stats(prompt, T["first"], T["G"], corpus), (case, st)
            _check_stats(case, st, n_steps)
        # one verify step: the plain handle's answer, flags included
        d = np.array(T["G"][:8], np.int32)
        d[4] = (d[4] + 1) % V
        res = []
        for h in (pm, one):
            s2, first = _start(L, h, T["plg"], prompt, 24, 64)
            res.append(h.verify_sample(first, d, 12, s2) + (s2.window().tolist(), _rng_print(s2)))
        assert res[0][0] == res[1][0] == 4 and res[0][1].tolist() == res[1][1].tolist() and res[0][2].tolist() == res[1][2].tolist()
        assert res[0][3:] == res[1][3:] and res[0][1][:5].tolist() == T["G"][:5]


@pytest.mark.parametrize("flags", [NO_GRAPH, UNFUSED], ids=["no_graph", "unfused"])
def test_sample_lookup_with_eager_and_unfused_steps(L, tmp_path, flags):
    path = synth_tool(tmp_path / "m.bin", seed=63, **SMALL)
    V, n_steps = SMALL["n_vocab"], 70
    prompt = synth.synth_prompt(12, V, seed=9)
    with L.Model(path, n_ctx=96, n_seq=2, flags=flags) as h:
        T = _truth(L, h, prompt, n_steps, 8, seed=25, rln=64)
        want_kv = _kv_rows(h, SMALL["n_layer"], 12 + n_steps)
        h.set_seq(1)
        for case in sorted(_CORPORA):
            corpus = _CORPORA[case](T["G"], V)
            exact, st = _lookup_run(L, h, T, corpus)
            assert exact.tolist() == T["flags"] and _kv_same(_kv_rows(h, SMALL["n_layer"], 12 + n_steps), want_kv), case
            if flags == UNFUSED:          # no one-pass verify step next to the un-fused single step: nothing is drafted
                assert st == dict(ZERO, n_single_steps=n_steps), st
            else:
                assert st == lookup_ref.loop_stats(prompt, T["first"], T["G"], corpus), (case, st)
                _check_stats(case, st, n_steps)


@pytest.mark.parametrize("kind", ["f16", "q4_1"])
def test_sample_lookup_on_files_without_a_per_row_key_split(L, tmp_path, kind):
    """f16 / Q4_1 files: the loop's tokens and zero drafts; a verify step runs its rows one eval_topk step at a time and stops at the mismatch"""
    hp = synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=4, n_layer=2)
    path = str(tmp_path / "m.bin")
    src = path + ".f16" if kind == "q4_1" else path
    synth.write_model_unquantized(src, hp, synth.random_tensors(hp, seed=9), 1)
    if kind == "q4_1":
        L.quantize_file(src, path, 3)
    prompt = synth.synth_prompt(12, hp.n_vocab, seed=9)
    n_steps = 40
    with L.Model(path, n_ctx=64, n_seq=2) as h:
        T = _truth(L, h, prompt, n_steps, 8, seed=26, rln=64)
        want_kv = _kv_rows(h, hp.n_layer, 12 + n_steps)
        h.set_seq(1)
        exact, st = _lookup_run(L, h, T, np.array(T["G"], np.int32))
        assert exact.tolist() == T["flags"] and st == dict(ZERO, n_single_steps=n_steps), st
        assert _kv_same(_kv_rows(h, hp.n_layer, 12 + n_steps), want_kv)
        s2, first = _start(L, h, T["plg"], prompt, 26, 64)
        d = np.array(T["G"][:6], np.int32)
        d[3] = (d[3] + 1) % hp.n_vocab
        n_acc, picks, ex = h.verify_sample(first, d, 12, s2)
        assert n_acc == 3 and picks.tolist() == T["G"][:4] + [-1, -1, -1] and ex.tolist() == T["flags"][:4] + [-1, -1, -1]


def test_sample_lookup_without_the_pinned_block(tmp_path):
    """LLAMAHIP_NO_HOST_IO: the id stream and the rows' candidates travel as plain copies instead of through the mapped host block (a fresh
    process: the switch is read at load)"""
    path = synth_tool(tmp_path / "m.bin", seed=62, **SMALL)
    code = f"""
import sys
sys.path[:0] = [{ROOT!r}, {os.path.dirname(os.path.abspath(__file__))!r}]
import numpy as np, llama_swift_amd as L, synth
import test_gpu_sample_lookup as t
prompt = synth.synth_prompt(9, 2000, seed=8)
with L.Model({path!r}, n_ctx=64, n_seq=2) as h:
    T = t._truth(L, h, prompt, 24, 8, seed=27, rln=64)
    h.set_seq(1)
    s2, first = t._start(L, h, T["plg"], prompt, 27, 64)
    d = np.array(T["G"][:8], np.int32); d[5] = (d[5] + 1) % 2000
    n_acc, picks, ex = h.verify_sample(first, d, 9, s2)
    assert n_acc == 5 and picks[:6].tolist() == T["G"][:6] and ex[:6].tolist() == T["flags"][:6], (n_acc, picks, ex)
    exact, st = t._lookup_run(L, h, T, np.array(T["G"], np.int32))
    assert exact.tolist() == T["flags"] and st["n_accepted"] > 0, st
print("NO_HOST_IO_OK")
"""
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LLAMAHIP_NO_HOST_IO="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "NO_HOST_IO_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_sample_lookup_refuses_a_stage_handle(L, tmp_path):
    path = synth_tool(tmp_path / "m.bin", seed=63, **SMALL)
    with L.Model(path, n_ctx=64, layer_begin=0, layer_end=2) as st:
        with pytest.raises(L.LlamaHipError, match="pipeline-stage handle"):
            st.verify_sample(5, [1, 2], 0, L.Sampler(seed=1))
        with pytest.raises(L.LlamaHipError, match="pipeline-stage handle"):
            st.decode_sample_lookup(5, 4, 0, [], L.Sampler(seed=1))


# ------------------------------------------------------------------------------------------------ 5. the oracle
def _oracle_stream(L, oracle, path, n_ctx, h, prompt, seed, rln, n_steps, nth, top_k=40):
    """the expectation of tests/test_gpu_sample_multi.py: the oracle stepped one token at a time, a fresh sampler of the same seed drawing on
    its logits; returns the first token, the n_steps tokens after it, the sampler's window and the oracle handle (for its KV rows)"""
    om = oracle.load(path, n_ctx)
    s = L.Sampler(seed=seed, repeat_last_n=rln)
    for t in prompt:
        s.accept(int(t))
    tok = s.sample(h, om.eval(prompt, 0, nth)["logits"], top_k=top_k)
    s.accept(tok)
    first, toks = tok, []
    for k in range(n_steps):
        tok = s.sample(h, om.eval(np.array([tok], np.int32), len(prompt) + k, nth)["logits"], top_k=top_k)
        s.accept(tok)
        toks.append(tok)
    return first, toks, s.window(), om


def test_sample_lookup_equals_the_oracle_stepped_token_by_token(L, oracle, tmp_path):
    """the `small` true-stream case of test 3 against the oracle: tokens, window, KV rows of the first and the last layer"""
    path = synth_tool(tmp_path / "m.bin", seed=63, **SMALL)
    V, n_steps, n_ctx = SMALL["n_vocab"], 150, 192
    prompt = synth.synth_prompt(12, V, seed=9)
    with L.Model(path, n_ctx=n_ctx) as h:
        first, want, win, om = _oracle_stream(L, oracle, path, n_ctx, h, prompt, 21, 64, n_steps, 8)
        s2, f2 = _start(L, h, h.eval(prompt, 0, 8), prompt, 21, 64)
        assert f2 == first
        out, exact, st = h.decode_sample_lookup(first, n_steps, 12, prompt, s2, corpus=np.array(want, np.int32))
        assert out.tolist() == want and s2.window().tolist() == win.tolist()
        _check_stats("b", st, n_steps)
        for il in (0, SMALL["n_layer"] - 1):
            gk, gv = h.kv(il, 12 + n_steps)
            ok, ov = om.kv(il, 12 + n_steps)
            assert same(gk, ok) and same(gv, ov), f"KV cache layer {il}"
        om.close()


# ------------------------------------------------------------------------------------------------ 6. the runner
_RUN = dict(numThreads=8, numTokens=130, n_ctx=192, seed=5)
_TEXT = "hello world abc tok00050 zz"


def _runner_model(tmp_path):
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=64, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=21))
    return path


def test_runner_event_stream_is_the_same_with_lookup_on(L, tmp_path):
    """a vocabulary of 96 and more than 130 tokens of history: the pending token has occurred before again and again, so drafts are made"""
    path = _runner_model(tmp_path)

    def run(lookup, **cfg):
        r, events = L.LlamaRunner(path), []
        if lookup is not None:
            r.set_lookup(lookup)
        toks = r.run(_TEXT, L.Config(**dict(_RUN, **cfg)), lambda t: events.append(("token", t)), lambda s, e: events.append(("state", s.name)))
        st = r.lookup_stats()
        r.close()
        return toks, events, st

    off, on, zero_len = run(None), run(15), run(0)
    assert len(off[0]) > 130 and off[2] == ZERO and zero_len[2] == ZERO
    assert on[0] == off[0] and on[1] == off[1] and zero_len[:2] == off[:2]
    assert on[2]["n_verify_steps"] > 0 and on[2]["n_drafted"] > 0, on[2]
    # the environment switch, for a bridge that never calls the setter (a fresh process: nothing else here may see it)
    code = ("import sys, json, llama_swift_amd as L\n"
            "toks, states = [], []\n"
            "r = L.LlamaRunner(sys.argv[1])\n"
            f"r.run({_TEXT!r}, L.Config(**{_RUN!r}), toks.append, lambda s, e: states.append(s.name))\n"
            "print('RESULT' + json.dumps(dict(toks=[t.hex() for t in toks], states=states, st=r.lookup_stats())))\n")
    env = dict(os.environ, LLAMAHIP_RUNNER_LOOKUP="15", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", code, path], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    got = json.loads(p.stdout.split("RESULT", 1)[1])
    assert got["toks"] == [t.hex() for t in off[0]]
    assert got["states"] == [v for k, v in off[1] if k == "state"]
    assert got["st"] == on[2]
    # a greedy run takes no lookup step
    g_off, g_on = run(None, greedy=True), run(15, greedy=True)
    assert g_on[:2] == g_off[:2] and g_on[2] == ZERO
