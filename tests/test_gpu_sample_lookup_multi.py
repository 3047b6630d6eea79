"""GPU (-m gpu): sampled decode with drafted tokens for several sequences at once (llamahip_verify_sample_multi,
llamahip_decode_sample_lookup_multi, llamahip_op_topk_slide_set, kernel k_topk_keys_slide_set).

The claim is that every sequence's token stream, exact flags, sampler window and rng state and KV cache are those of the documented
single-sequence loop  eval_topk -> sample_from_candidates (exact) / sample (not exact) -> accept  on that slot alone, bit for bit.  It rests
on two facts tested elsewhere -- the rows of a segment are single-token evals of their slot (tests/test_gpu_lookup_multi.py) and the window
at row j is known before the eval (tests/test_gpu_sample_lookup.py) -- and on the device half tested first here: row r of
op_topk_slide_set is op_topk on that row with the window its segment's id stream gives it.

Every handle has twice the slots under test: the second half holds the truth, written by the single-sequence loop (_start / _loop of
tests/test_gpu_sample_lookup.py, restated here).  Sequence i draws with sampler seed base + i and repeat_last_n 64."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lookup_multi_ref
import synth
from conftest import synth_tool

pytestmark = pytest.mark.gpu
SMALL = dict(n_vocab=2000, n_embd=512, n_mult=256, n_head=4, n_layer=3)
W7B = dict(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=2)
SHAPES = {"small": SMALL, "7b_width": W7B}
NO_GRAPH, UNFUSED = 1, 2
N_CTX = 160
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = dict(n_verify_steps=0, n_single_steps=0, n_drafted=0, n_accepted=0)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _kv_diff(h, n_layer, hi, truth, test, h_truth=None):
    """KV rows [0, hi) of every layer, slot `test` of h against slot `truth` of h_truth (default h): [] or (layer, first differing rows)"""
    ht = h_truth if h_truth is not None else h
    bad = []
    for il in range(n_layer):
        ht.set_seq(truth)
        k0, v0 = ht.kv(il, hi)
        h.set_seq(test)
        k1, v1 = h.kv(il, hi)
        if not (same(k0, k1) and same(v0, v1)):
            bad.append((il, np.flatnonzero((k0 != k1).any(axis=1) | (v0 != v1).any(axis=1))[:6].tolist()))
    ht.set_seq(0)
    h.set_seq(0)
    return bad


def _rng_print(s):
    """the sampler's rng state, by what it draws next: 8 draws over 64 equally likely candidates (this consumes them: last use of s)"""
    return [s.sample_from_candidates(np.zeros(64), np.arange(64, dtype=np.int32), top_p=1.0) for _ in range(8)]


def _prompts(n, V, lens, seed):
    return [synth.synth_prompt(lens[i], V, seed=seed + i) for i in range(n)]


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


def _seed_slots(h, prompts, slots, nth):
    """the prompts evaluated into the given slots; returns each one's logits"""
    out = []
    for p, s in zip(prompts, slots):
        h.set_seq(s)
        out.append(h.eval(p, 0, nth))
    h.set_seq(0)
    return out


def _truth(L, h, prompts, half, T, nth, base, rln=64, top_k=40):
    """slot half + i: prompt i, then T steps of the loop with sampler seed base + i.  One record per sequence: S[j] = the token at position
    len(prompt) + j, flags[j] = the exact flag of the step that drew S[j + 1], the sampler's final window and rng print."""
    rl = rln if isinstance(rln, (list, tuple)) else [rln] * len(prompts)
    plg = _seed_slots(h, prompts, [half + i for i in range(len(prompts))], nth)
    out = []
    for i, p in enumerate(prompts):
        h.set_seq(half + i)
        s, first = _start(L, h, plg[i], p, base + i, rl[i], top_k)
        G, flags = _loop(h, s, first, len(p), T, nth, top_k)
        out.append(dict(plg=plg[i], first=first, S=[first] + G, G=G, flags=flags, window=s.window().tolist(), rng=_rng_print(s), seed=base + i, rln=rl[i]))
    h.set_seq(0)
    return out


def _fresh(L, h, T, prompts, top_k=40):
    """one fresh sampler per sequence, as the truth's was when its loop began"""
    smp = []
    for t, p in zip(T, prompts):
        s, first = _start(L, h, t["plg"], p, t["seed"], t["rln"], top_k)
        assert first == t["first"]
        smp.append(s)
    return smp


# ------------------------------------------------------------------------------------------------ 1. the device half
def _rows(rng, R, V):
    """the rows of tests/test_gpu_sample_lookup.py: plain, tie-heavy (quarter steps, some with a little noise), a NaN row and a +inf row (R > 1)"""
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


def _segmentations(R, rng):
    out = [[0, R], list(range(R + 1))]
    if R >= 3:
        for _ in range(2):
            cuts = sorted(rng.choice(np.arange(1, R), int(rng.integers(1, R - 1)), replace=False).tolist())
            out.append([0] + cuts + [R])
    return out


def _pool(rng, V, seg, n_last):
    """one id pool for the segments: every segment's stream (n_last + rows - 1 ids, some outside [0, V)) at its own offset, the streams in a
    shuffled order with unrelated ids between and around them"""
    streams = []
    for (b, e), nl in zip(zip(seg, seg[1:]), n_last):
        ids = rng.integers(0, V, nl + e - b - 1).astype(np.int32)
        if ids.size:                                    # ids outside [0, V): ignored, as the host sampler ignores them
            ids[rng.integers(0, ids.size, max(1, ids.size // 8))] = rng.choice([-1, -7, V, V + 3, 2**31 - 1, -2**31], max(1, ids.size // 8))
        streams.append(ids)
    off, parts, at = [0] * len(streams), [], 0
    for s in rng.permutation(len(streams)):
        gap = rng.integers(0, V, int(rng.integers(0, 5))).astype(np.int32)
        parts += [gap, streams[s]]
        off[s] = at + gap.size
        at += gap.size + streams[s].size
    parts.append(rng.integers(0, V, 3).astype(np.int32))
    return np.concatenate(parts), off, streams


@pytest.mark.parametrize("V", [1200, 32000, 32768])
@pytest.mark.parametrize("R", [1, 2, 16])
def test_op_topk_slide_set_is_op_topk_row_by_row(L, R, V):
    rng = np.random.default_rng(R * 100019 + V)
    lg = _rows(rng, R, V)
    flags, cache = [], {}

    def ref(r, window, k):          # op_topk on row r alone, computed once per (row, window, top_k)
        key = (r, window.tobytes(), k)
        if key not in cache:
            cache[key] = L.op_topk(lg[r], window, top_k=k)
        return cache[key]

    lens = [0, 1, 64, 1024]
    for si, seg in enumerate(_segmentations(R, rng)):
        G = len(seg) - 1
        uniform = si == 0 and G == 1
        for trial, k in enumerate((40, 1, 64) if si < 2 else (40,)):
            # mixed window lengths, every length in turn (one segment: that segment takes each of them over the trials and a fourth run)
            mixes = [[lens[(trial + si + g) % 4] for g in range(G)]]
            if uniform and trial == 0:
                mixes += [[lens[1]], [lens[2]], [lens[3]]]
            for n_last in mixes:
                ids, off, streams = _pool(rng, V, seg, n_last)
                first = L.op_topk_slide_set(lg, ids, seg, off, n_last, top_k=k)
                again = L.op_topk_slide_set(lg, ids, seg, off, n_last, top_k=k)          # a second call straight after the first
                for exact, sc, out_ids in (first, again):
                    assert sc.shape == (R, k) and out_ids.shape == (R, k)
                    for g, (b, e) in enumerate(zip(seg, seg[1:])):
                        for r in range(b, e):
                            e1, s1, i1 = ref(r, streams[g][r - b:r - b + n_last[g]], k)
                            assert exact[r] == e1, (R, V, seg, n_last, k, r)
                            assert same(sc[r], s1) and same(out_ids[r], i1), (R, V, seg, n_last, k, r)
                flags += first[0].tolist()
                if G == 1:          # one segment is the single-stream op
                    e2, s2, i2 = L.op_topk_slide(lg, streams[0], n_last[0], top_k=k)
                    assert first[0].tolist() == e2.tolist() and same(first[1], s2) and same(first[2], i2), (R, V, n_last, k)
                if G == R:          # all singletons is the batched op with one window per row
                    e2, s2, i2 = L.op_topk_rows(lg, streams, top_k=k)
                    assert first[0].tolist() == e2.tolist() and same(first[1], s2) and same(first[2], i2), (R, V, n_last, k)
    # a single segment at 1025 ids: its rows are inexact, the other segment's rows are what they are without it
    seg = [0, R] if R == 1 else [0, R // 2, R]
    n_last = [1025] if R == 1 else [1025, 64]
    ids, off, streams = _pool(rng, V, seg, n_last)
    for exact, sc, out_ids in (L.op_topk_slide_set(lg, ids, seg, off, n_last), L.op_topk_slide_set(lg, ids, seg, off, n_last)):
        assert not exact[:seg[1]].any(), (R, V, exact)
        for r in range(seg[1], R):
            e1, s1, i1 = ref(r, streams[1][r - seg[1]:r - seg[1] + 64], 40)
            assert exact[r] == e1 and same(sc[r], s1) and same(out_ids[r], i1), (R, V, r)
    if R == 16:
        assert any(flags) and not all(flags), flags          # exact rows and inexact rows (ties, the NaN row) were both seen


# ------------------------------------------------------------------------------------------------ 2. one step, known answers
@pytest.mark.parametrize("shape,nth", [("small", 8), ("small", 3), ("7b_width", 8)])
def test_verify_sample_multi_with_known_answers(L, tmp_path, shape, nth):
    """the row layouts of test_verify_greedy_multi_with_known_answers; per sequence the draft is wrong at 0, wrong part way, correct
    throughout or absent.  Sequence 0 starts at 122 and crosses position 128."""
    kw = SHAPES[shape]
    V, T = kw["n_vocab"], 36
    path = synth_tool(tmp_path / "m.bin", seed=72, **kw)
    lens = [122, 9, 30, 17]
    prompts = _prompts(4, V, lens, seed=50)
    with L.Model(path, n_ctx=N_CTX, n_seq=8) as h:
        Tr = _truth(L, h, prompts, 4, T, nth, base=300)
        _seed_slots(h, prompts, range(4), nth)
        smp = _fresh(L, h, Tr, prompts)
        shadow = [L.Sampler(seed=1, repeat_last_n=64) for _ in range(4)]          # (the window is a function of the accepted tokens alone)
        for i in range(4):
            for t in list(prompts[i]) + [Tr[i]["first"]]:
                shadow[i].accept(int(t))
        pos = list(lens)          # every test slot's context
        for rows, acc in (((7, 1, 4, 4), (3, None, 0, None)), ((4, 4, 4, 4), (None, 0, 2, 1)), ((1, 12, 1, 2), (None, 5, None, 0)),
                          ((8, 2, 3, 3), (None, None, None, None))):
            drafts, want = [], []
            for i in range(4):
                o = pos[i] - lens[i]
                d = np.array(Tr[i]["S"][o + 1:o + rows[i]], np.int32)
                a = len(d) if acc[i] is None else acc[i]
                if a < len(d):
                    d[a] = (d[a] + 1) % V
                drafts.append(d)
                want.append(a)
            n_acc, picks, exact = h.verify_sample_multi(range(4), [Tr[i]["S"][pos[i] - lens[i]] for i in range(4)], drafts, pos, smp, n_threads=nth)
            tag = (shape, nth, rows, acc)
            assert n_acc.tolist() == want, tag
            for i in range(4):
                o, a, nd = pos[i] - lens[i], want[i], len(drafts[i])
                assert picks[i].tolist() == Tr[i]["S"][o + 1:o + a + 2] + [-1] * (nd - a), tag + (i, picks[i].tolist())
                assert exact[i].tolist() == Tr[i]["flags"][o:o + a + 1] + [-1] * (nd - a), tag + (i, exact[i].tolist())
                for t in Tr[i]["S"][o + 1:o + a + 2]:
                    shadow[i].accept(int(t))
                assert smp[i].window().tolist() == shadow[i].window().tolist(), tag + (i,)
                assert not _kv_diff(h, kw["n_layer"], pos[i] + a + 1, 4 + i, i), tag + (i,)
                pos[i] += a + 1          # the next step starts from the new context: the rejected rows behind it do no harm
        assert pos[0] > 128
        # every slot goes on with the plain loop to the truth's end: its tokens, flags, KV rows, final window and rng state
        for i in range(4):
            o = pos[i] - lens[i]
            h.set_seq(i)
            toks, flags = _loop(h, smp[i], Tr[i]["S"][o], pos[i], T - o, nth)
            assert toks == Tr[i]["S"][o + 1:] and flags == Tr[i]["flags"][o:], (shape, nth, i)
            assert smp[i].window().tolist() == Tr[i]["window"] and _rng_print(smp[i]) == Tr[i]["rng"], (shape, nth, i)
            assert not _kv_diff(h, kw["n_layer"], lens[i] + T, 4 + i, i), (shape, nth, i)
        s2 = [L.Sampler(seed=1), L.Sampler(seed=2)]
        with pytest.raises(L.LlamaHipError, match=r"n_past \(157\) \+ n_draft \(3\) \+ 1 > n_ctx \(160\)"):
            h.verify_sample_multi([0, 1], [5, 5], [[1], [1, 2, 3]], [3, 157], s2, n_threads=nth)


# ------------------------------------------------------------------------------------------------ 3. the loop against the loop per slot
LENS = [100, 7, 23, 12, 41]
N_STEPS = 40          # (sequence 0: positions 100 .. 139, over the 128-key boundary)


def _corrupt(c, V):
    c = np.array(c, np.int32)
    c[6::7] = (c[6::7] + 1) % V          # every 7th token is not the true one
    return c


def _run_loop(L, h, Tr, prompts, n, corpus, nth, n_layer, h_truth=None, half=5, **kw):
    """the loop on slots 0 .. n - 1 with fresh samplers, checked per sequence against the truth; returns the stats"""
    _seed_slots(h, prompts[:n], range(n), nth)
    smp = _fresh(L, h, Tr[:n], prompts[:n], kw.get("top_k", 40))
    out, exact, st = h.decode_sample_lookup_multi([t["first"] for t in Tr[:n]], LENS[:n], N_STEPS, prompts[:n], smp, corpus=corpus, n_threads=nth,
                                                  want_exact=True, **kw)
    for i in range(n):
        assert out[i].tolist() == Tr[i]["G"], (n, i, st[i], np.flatnonzero(out[i] != np.array(Tr[i]["G"]))[:5])
        assert exact[i].tolist() == Tr[i]["flags"], (n, i)
        assert smp[i].window().tolist() == Tr[i]["window"] and _rng_print(smp[i]) == Tr[i]["rng"], (n, i)
        assert not _kv_diff(h, n_layer, LENS[i] + N_STEPS, half + i, i, h_truth), (n, i)
        assert st[i]["n_verify_steps"] + st[i]["n_single_steps"] + st[i]["n_accepted"] == N_STEPS, st[i]
    return st


def _loop_case(L, h, n_layer, V, nth, h_truth=None, base=400):
    """the truth on h_truth (default: the second half of h's slots), then the loop for 2, 3 and 5 sequences over both corpora"""
    prompts = _prompts(5, V, LENS, seed=80)
    ht = h_truth if h_truth is not None else h
    Tr = _truth(L, ht, prompts, 0 if h_truth is not None else 5, N_STEPS, nth, base=base)
    true = np.concatenate([np.array(t["G"], np.int32) for t in Tr])          # the concatenated truth streams: the loop is sure to draft
    for n in (2, 3, 5):
        firsts, Gs = [t["first"] for t in Tr[:n]], [t["G"] for t in Tr[:n]]
        for case, corpus in (("true", true), ("every_7th_wrong", _corrupt(true, V))):
            # the restatement alone, before the feature is called: with these seeds the run exercises it
            want = lookup_multi_ref.loop_stats(prompts[:n], firsts, Gs, corpus)
            assert all(x["n_verify_steps"] + x["n_single_steps"] + x["n_accepted"] == N_STEPS for x in want), want
            if case == "true":
                assert any(x["n_accepted"] > 0 for x in want), want
            else:
                assert 0 < sum(x["n_accepted"] for x in want) < sum(x["n_drafted"] for x in want), want
            st = _run_loop(L, h, Tr, prompts, n, corpus, nth, n_layer, h_truth, half=0 if h_truth is not None else 5)
            assert st == want, (n, case, st, want)
    return prompts, Tr, true


@pytest.mark.parametrize("shape,nth,flags", [("small", 8, 0), ("small", 3, 0), ("7b_width", 8, 0), ("small", 8, NO_GRAPH)],
                         ids=["small", "small_3_threads", "7b_width", "no_graph"])
def test_sample_lookup_multi_equals_the_loop_per_slot(L, tmp_path, shape, nth, flags):
    kw = SHAPES[shape]
    path = synth_tool(tmp_path / "m.bin", seed=73, **kw)
    with L.Model(path, n_ctx=N_CTX, n_seq=10, flags=flags) as h:
        assert h.stage_set_applies(16, nth)          # (these shapes take the set path, not the fall-back)
        _loop_case(L, h, kw["n_layer"], kw["n_vocab"], nth)


@pytest.mark.parametrize("shape", ["small", "7b_width"])
def test_sample_lookup_multi_on_two_stages(L, tmp_path, shape):
    """against the PLAIN handle's loop, flags included: every row of the loop is selected on the last stage's device"""
    kw = SHAPES[shape]
    path = synth_tool(tmp_path / "m.bin", seed=73, **kw)
    with L.Model(path, n_ctx=N_CTX, n_seq=5, devices=[0, 0]) as pm, L.Model(path, n_ctx=N_CTX, n_seq=5) as one:
        _loop_case(L, pm, kw["n_layer"], kw["n_vocab"], 8, h_truth=one)


# ------------------------------------------------------------------------------------------------ 4. edges of the loop
def test_sample_lookup_multi_edges(L, tmp_path):
    V, nl, nth = SMALL["n_vocab"], SMALL["n_layer"], 8
    path = synth_tool(tmp_path / "m.bin", seed=73, **SMALL)
    prompts = _prompts(5, V, LENS, seed=80)
    with L.Model(path, n_ctx=N_CTX, n_seq=10) as h:
        Tr = _truth(L, h, prompts, 5, N_STEPS, nth, base=400)
        true = np.concatenate([np.array(t["G"], np.int32) for t in Tr])
        firsts = [t["first"] for t in Tr]
        # the handle's current slot is as the caller left it: an eval behind the call lands there and nowhere else
        _seed_slots(h, prompts[:2], [0, 1], nth)
        smp = _fresh(L, h, Tr[:2], prompts[:2])
        h.set_seq(1)
        out, st = h.decode_sample_lookup_multi(firsts[:2], LENS[:2], N_STEPS, prompts[:2], smp, corpus=true, n_threads=nth)
        assert out.tolist() == [t["G"] for t in Tr[:2]]
        h.eval(prompts[1], 0, nth)
        assert not _kv_diff(h, nl, LENS[0] + N_STEPS, 5, 0) and not _kv_diff(h, nl, LENS[1] + N_STEPS, 6, 1)
        # one sequence: decode_sample_lookup on slot 0 -- tokens, flags, stats, KV
        _seed_slots(h, [prompts[0]] * 2, [0, 1], nth)
        sa, sb = _fresh(L, h, Tr[:1], prompts[:1]) + _fresh(L, h, Tr[:1], prompts[:1])
        out, ex, st = h.decode_sample_lookup_multi(firsts[:1], LENS[:1], N_STEPS, prompts[:1], [sa], corpus=true, n_threads=nth, want_exact=True)
        h.set_seq(1)
        out1, ex1, st1 = h.decode_sample_lookup(firsts[0], N_STEPS, LENS[0], prompts[0], sb, corpus=true, n_threads=nth)
        assert out[0].tolist() == out1.tolist() == Tr[0]["G"] and ex[0].tolist() == ex1.tolist() and st == [st1]
        assert sa.window().tolist() == sb.window().tolist() and _rng_print(sa) == _rng_print(sb)
        assert not _kv_diff(h, nl, LENS[0] + N_STEPS, 1, 0)
        # nothing to draft from (no corpus, n-grams longer than any repeat): decode_sample_multi's tokens, every step a single step
        st = _run_loop(L, h, Tr, prompts, 3, None, nth, nl, draft_len=1, ngram_min=24, ngram_max=24)
        assert st == lookup_multi_ref.loop_stats(prompts[:3], firsts[:3], [t["G"] for t in Tr[:3]], None, 1, 24, 24)
        assert st == [dict(ZERO, n_single_steps=N_STEPS)] * 3
        _seed_slots(h, prompts[:3], range(3), nth)
        out, ex = h.decode_sample_multi(firsts[:3], LENS[:3], N_STEPS, _fresh(L, h, Tr[:3], prompts[:3]), n_threads=nth, want_exact=True)
        assert out.tolist() == [t["G"] for t in Tr[:3]] and ex.tolist() == [t["flags"] for t in Tr[:3]]
        # top_k = 65: the device makes no candidates -- zero drafts, the loop's tokens
        T65 = _truth(L, h, prompts[:2], 5, N_STEPS, nth, base=400, top_k=65)
        assert not any(any(t["flags"]) for t in T65)
        st = _run_loop(L, h, T65, prompts, 2, np.concatenate([np.array(t["G"], np.int32) for t in T65]), nth, nl, top_k=65)
        assert st == [dict(ZERO, n_single_steps=N_STEPS)] * 2
        # one sampler with a window of 1100 ids among samplers with 64: that sequence drafts nothing, the others do, every stream is the truth
        Tw = _truth(L, h, prompts[:3], 5, N_STEPS, nth, base=400, rln=[64, 1100, 64])
        assert not any(Tw[1]["flags"]) and any(Tw[0]["flags"])
        st = _run_loop(L, h, Tw, prompts, 3, np.concatenate([np.array(t["G"], np.int32) for t in Tw]), nth, nl)
        assert st[1]["n_drafted"] == 0 and st[1] == dict(ZERO, n_single_steps=N_STEPS), st
        assert st[0]["n_drafted"] > 0 and st[2]["n_drafted"] > 0 and st[0]["n_accepted"] + st[2]["n_accepted"] > 0, st
        # ... and one step there: the long-window sequence's rows are drawn from their logits, the other's from the device's candidates
        _seed_slots(h, prompts[:2], [0, 1], nth)
        smp = _fresh(L, h, Tw[:2], prompts[:2])
        d = [np.array(Tw[0]["S"][1:6], np.int32), np.array(Tw[1]["S"][1:6], np.int32)]
        d[1][3] = (d[1][3] + 1) % V
        n_acc, picks, exact = h.verify_sample_multi([0, 1], firsts[:2], d, LENS[:2], smp, n_threads=nth)
        assert n_acc.tolist() == [5, 3] and picks[0].tolist() == Tw[0]["S"][1:7] and picks[1].tolist() == Tw[1]["S"][1:5] + [-1, -1]
        assert exact[0].tolist() == Tw[0]["flags"][:6] and exact[1].tolist() == [0] * 4 + [-1, -1]


# ------------------------------------------------------------------------------------------------ 5. fall-backs
def _fallback_case(L, h, n_layer, V, per_slot_stats):
    """handles without a set step: the loop's tokens through llamahip_decode_sample_lookup per slot, one step through llamahip_verify_sample"""
    prompts = _prompts(5, V, LENS, seed=80)
    Tr = _truth(L, h, prompts, 5, N_STEPS, 8, base=500)
    true = np.concatenate([np.array(t["G"], np.int32) for t in Tr])
    st = _run_loop(L, h, Tr, prompts, 3, true, 8, n_layer)
    assert st == per_slot_stats(prompts, Tr, true), st
    _seed_slots(h, prompts[:2], [0, 1], 8)
    smp = _fresh(L, h, Tr[:2], prompts[:2])
    d = [np.array(Tr[0]["S"][1:6], np.int32), np.array(Tr[1]["S"][1:4], np.int32)]
    d[0][3] = (d[0][3] + 1) % V
    n_acc, picks, exact = h.verify_sample_multi([0, 1], [Tr[0]["first"], Tr[1]["first"]], d, LENS[:2], smp)
    assert n_acc.tolist() == [3, 3] and picks[0].tolist() == Tr[0]["S"][1:5] + [-1, -1] and picks[1].tolist() == Tr[1]["S"][1:5]
    assert exact[0].tolist() == Tr[0]["flags"][:4] + [-1, -1] and exact[1].tolist() == Tr[1]["flags"][:4]
    assert not _kv_diff(h, n_layer, LENS[0] + 4, 5, 0) and not _kv_diff(h, n_layer, LENS[1] + 4, 6, 1)


@pytest.mark.parametrize("kind", ["f16", "q4_1"])
def test_sample_lookup_multi_on_files_without_a_set_step(L, tmp_path, kind):
    hp = synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=4, n_layer=2)
    path = str(tmp_path / "m.bin")
    src = path + ".f16" if kind == "q4_1" else path
    synth.write_model_unquantized(src, hp, synth.random_tensors(hp, seed=9), 1)
    if kind == "q4_1":
        L.quantize_file(src, path, 3)
    with L.Model(path, n_ctx=N_CTX, n_seq=10) as h:
        _fallback_case(L, h, hp.n_layer, hp.n_vocab, lambda p, Tr, c: [dict(ZERO, n_single_steps=N_STEPS)] * 3)


def test_sample_lookup_multi_with_unfused_steps(L, tmp_path):
    path = synth_tool(tmp_path / "m.bin", seed=73, **SMALL)
    with L.Model(path, n_ctx=N_CTX, n_seq=10, flags=UNFUSED) as h:
        _fallback_case(L, h, SMALL["n_layer"], SMALL["n_vocab"], lambda p, Tr, c: [dict(ZERO, n_single_steps=N_STEPS)] * 3)


def test_sample_lookup_multi_without_the_pinned_block(tmp_path):
    """LLAMAHIP_NO_HOST_IO: the id pool, the row table, the candidates and the slots' words travel as plain copies instead of through the
    mapped host block (a fresh process: the switch is read at load)"""
    path = synth_tool(tmp_path / "m.bin", seed=73, **SMALL)
    code = f"""
import sys
sys.path[:0] = [{ROOT!r}, {os.path.dirname(os.path.abspath(__file__))!r}]
import numpy as np, llama_swift_amd as L, synth
import test_gpu_sample_lookup_multi as t
prompts = t._prompts(5, 2000, t.LENS, seed=80)
with L.Model({path!r}, n_ctx=160, n_seq=10) as h:
    Tr = t._truth(L, h, prompts, 5, t.N_STEPS, 8, base=400)
    true = np.concatenate([np.array(x["G"], np.int32) for x in Tr])
    st = t._run_loop(L, h, Tr, prompts, 3, true, 8, 3)
    assert sum(x["n_accepted"] for x in st) > 0, st
    st = t._run_loop(L, h, Tr, prompts, 3, t._corrupt(true, 2000), 8, 3)
    assert 0 < sum(x["n_accepted"] for x in st) < sum(x["n_drafted"] for x in st), st
print("NO_HOST_IO_OK")
"""
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LLAMAHIP_NO_HOST_IO="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "NO_HOST_IO_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_sample_lookup_multi_refuses_a_stage_handle(L, tmp_path):
    path = synth_tool(tmp_path / "m.bin", seed=73, **SMALL)
    s = [L.Sampler(seed=1), L.Sampler(seed=2)]
    with L.Model(path, n_ctx=64, n_seq=2, layer_begin=0, layer_end=2) as st:
        with pytest.raises(L.LlamaHipError, match="pipeline-stage handle"):
            st.verify_sample_multi([0, 1], [5, 5], [[1], []], [0, 0], s)
        with pytest.raises(L.LlamaHipError, match="pipeline-stage handle"):
            st.decode_sample_lookup_multi([5, 5], [0, 0], 4, [[], []], s)


# ------------------------------------------------------------------------------------------------ 6. the oracle
def _oracle_stream(L, oracle, path, n_ctx, h, prompt, seed, rln, n_steps, nth, top_k=40):
    """the expectation of tests/test_gpu_sample_lookup.py: the oracle stepped one token at a time, a fresh sampler of the same seed drawing on
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


def test_sample_lookup_multi_equals_the_oracle_stepped_token_by_token(L, oracle, tmp_path):
    """the `small` true-corpus case with 3 sequences against the oracle: tokens, windows, KV rows of the first and the last layer"""
    path = synth_tool(tmp_path / "m.bin", seed=73, **SMALL)
    V = SMALL["n_vocab"]
    prompts = _prompts(3, V, LENS, seed=80)
    with L.Model(path, n_ctx=N_CTX, n_seq=3) as h:
        O = [_oracle_stream(L, oracle, path, N_CTX, h, prompts[i], 400 + i, 64, N_STEPS, 8) for i in range(3)]
        plg = _seed_slots(h, prompts, range(3), 8)
        smp = []
        for i in range(3):
            s, f = _start(L, h, plg[i], prompts[i], 400 + i, 64)
            assert f == O[i][0]
            smp.append(s)
        corpus = np.concatenate([np.array(o[1], np.int32) for o in O])
        out, st = h.decode_sample_lookup_multi([o[0] for o in O], LENS[:3], N_STEPS, prompts, smp, corpus=corpus)
        assert sum(x["n_accepted"] for x in st) > 0, st
        for i in range(3):
            assert out[i].tolist() == O[i][1] and smp[i].window().tolist() == O[i][2].tolist(), i
            h.set_seq(i)
            for il in (0, SMALL["n_layer"] - 1):
                gk, gv = h.kv(il, LENS[i] + N_STEPS)
                ok, ov = O[i][3].kv(il, LENS[i] + N_STEPS)
                assert same(gk, ok) and same(gv, ov), f"sequence {i}, KV cache layer {il}"
            O[i][3].close()
