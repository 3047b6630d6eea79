"""GPU (-m gpu): greedy decode with drafted tokens for several sequences at once (llamahip_verify_greedy_multi,
llamahip_decode_greedy_lookup_multi, kernel k_accept_drafts_set).

The feature's claim is that every sequence's token stream and KV cache are llamahip_decode_greedy's on that slot alone, bit for bit.  It
rests on one fact read from the kernels of a set step -- rows r .. r + j that share one KV offset and hold positions p .. p + j make row
r + j the single-token eval of that slot at p + j -- which is tested first; then the device tail against numpy, one step against known
answers, and the loop against decode_greedy per slot on plain, un-captured, pipeline, f16 and Q4_1 handles, its step counts against the
Python restatement of drafter, dealing and accept rule (tests/lookup_multi_ref.py).

Every handle has twice the slots under test: the second half holds the truth, written by plain decode_greedy."""
import os

import numpy as np
import pytest

import lookup_multi_ref
import lookup_ref
import synth
from conftest import synth_tool

pytestmark = pytest.mark.gpu
SMALL = dict(n_vocab=2000, n_embd=512, n_mult=256, n_head=4, n_layer=3)
W7B = dict(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=2)
SHAPES = {"small": SMALL, "7b_width": W7B}
NO_GRAPH = 1
N_CTX = 160


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _kv_diff(h, n_layer, lo, hi, truth, test):
    """KV rows [lo, hi) of every layer, slot `test` against slot `truth`: [] or (layer, first differing rows)"""
    bad = []
    for il in range(n_layer):
        h.set_seq(truth)
        k0, v0 = h.kv(il, hi)
        h.set_seq(test)
        k1, v1 = h.kv(il, hi)
        if not (same(k0[lo:], k1[lo:]) and same(v0[lo:], v1[lo:])):
            rows = lo + np.flatnonzero((k0[lo:] != k1[lo:]).any(axis=1) | (v0[lo:] != v1[lo:]).any(axis=1))
            bad.append((il, rows[:6].tolist()))
    h.set_seq(0)
    return bad


def _prompts(n, V, lens, seed):
    return [synth.synth_prompt(lens[i], V, seed=seed + i) for i in range(n)]


def _seed_slots(h, prompts, slots, nth):
    """the prompts evaluated into the given slots; returns each one's first token"""
    firsts = []
    for p, s in zip(prompts, slots):
        h.set_seq(s)
        firsts.append(int(np.argmax(h.eval(p, 0, nth))))
    h.set_seq(0)
    return firsts


def _truth(h, prompts, half, T, nth):
    """slot half + i: prompt i, then T steps of plain decode_greedy.  Returns S with S[i][j] = the token at position len(prompt i) + j."""
    firsts = _seed_slots(h, prompts, [half + i for i in range(len(prompts))], nth)
    S = []
    for i, p in enumerate(prompts):
        h.set_seq(half + i)
        S.append([firsts[i]] + h.decode_greedy(firsts[i], len(p), T, nth).tolist())
    h.set_seq(0)
    return S


# ------------------------------------------------------------------------------------------------ 1. the ground it stands on
@pytest.mark.parametrize("shape,nth", [("small", 1), ("small", 3), ("small", 8), ("7b_width", 3), ("7b_width", 8)])
def test_rows_that_share_a_slot_are_single_token_evals(L, tmp_path, shape, nth):
    """verify_greedy_multi with drafts from the truth stream: every pick the truth, KV rows of every layer bit-identical to the truth slots,
    a following decode_greedy continues every slot.  Sequence 0 sits at position 124: its rows straddle position 128, the key-slice and
    key-bucket boundary."""
    kw = SHAPES[shape]
    V, T = kw["n_vocab"], 20
    path = synth_tool(tmp_path / "m.bin", seed=71, **kw)
    lens = [124] + [5 + 2 * i for i in range(1, 16)]
    prompts = _prompts(16, V, lens, seed=30)
    with L.Model(path, n_ctx=N_CTX, n_seq=32) as h:
        S = _truth(h, prompts, 16, T, nth)
        _seed_slots(h, prompts, range(16), nth)
        # (sequence -> rows of its segment); sequence 0's segment crosses 128 in the first, the second and the last layout
        layouts = [[(3, 3), (7, 1), (0, 5)], [(0, 8), (5, 8)], [(i, 1) for i in range(16)], [(0, 16)], [(9, 16)], [(4, 2), (2, 14)]]
        for lay in layouts:
            seqs = [s for s, _ in lay]
            nd = [r - 1 for _, r in lay]
            n_acc, picks = h.verify_greedy_multi(seqs, [S[s][0] for s in seqs], [S[s][1:1 + k] for s, k in zip(seqs, nd)], [lens[s] for s in seqs], nth)
            assert n_acc.tolist() == nd, (shape, nth, lay)
            for s, k, pk in zip(seqs, nd, picks):
                assert pk.tolist() == S[s][1:k + 2], (shape, nth, lay, s)
                assert not _kv_diff(h, kw["n_layer"], 0, lens[s] + k + 1, 16 + s, s), (shape, nth, lay, s)
        # every slot goes on from where its last step left it (sequence i: len + 1 rows, but 0, 9 and 2: 16, 16 and 14)
        for s in range(16):
            k = {0: 15, 9: 15, 2: 13, 4: 1}.get(s, 0)
            h.set_seq(s)
            assert h.decode_greedy(S[s][k + 1], lens[s] + k + 1, 3, nth).tolist() == S[s][k + 2:k + 5], (shape, nth, s)
            assert not _kv_diff(h, kw["n_layer"], 0, lens[s] + k + 4, 16 + s, s), (shape, nth, s)


# ------------------------------------------------------------------------------------------------ 2. the device tail against numpy
def _np_pick(row):
    return 0 if np.isnan(row).all() else int(np.nanargmax(row))          # (first index of the largest non-NaN value)


def _segmentations(R, rng):
    out = [[0, R], list(range(R + 1))]
    if R >= 3:
        for _ in range(2):
            cuts = sorted(rng.choice(np.arange(1, R), int(rng.integers(1, R - 1)), replace=False).tolist())
            out.append([0] + cuts + [R])
    return out


def _rows_of_kind(kind, R, V, rng):
    if kind == "random":
        return (rng.standard_normal((R, V)) * 3).astype(np.float32)
    lg = (rng.integers(-40, 41, (R, V)) * 0.25).astype(np.float32)          # quarter steps: the maximum occurs many times over
    if kind == "ties":
        return lg
    for r in range(R):          # non-finite entries, as in the single-sequence op test
        k = r % 6
        if k == 0:
            lg[r, rng.integers(0, V, V // 10)] = np.nan
            lg[r, 0] = np.nan
        elif k == 1:
            lg[r, rng.integers(0, V)] = np.inf
            lg[r, rng.integers(0, V, 5)] = np.nan
        elif k == 2:
            lg[r] = -np.inf
        elif k == 3:
            lg[r] = np.nan
        elif k == 4:
            lg[r] = -1.0
            lg[r, V // 2] = -0.0
            lg[r, V - 1] = 0.0
        else:
            lg[r] = -np.inf
            lg[r, V - 1] = np.nan
            lg[r, V // 3] = -3.0e38
    return lg


@pytest.mark.parametrize("V", [1200, 32000, 32768])
def test_op_verify_rows_set_against_numpy(L, V):
    rng = np.random.default_rng(V)
    for R in range(1, 17):
        for kind in ("random", "ties", "non-finite"):
            lg = _rows_of_kind(kind, R, V, rng)
            want = np.array([_np_pick(r) for r in lg], np.int32)
            for seg in _segmentations(R, rng):
                # per segment: the draft agrees with the picks for a chosen length, then differs
                toks = rng.integers(0, V, R).astype(np.int32)
                agree = []
                for b, e in zip(seg, seg[1:]):
                    a = int(rng.integers(0, e - b))
                    toks[b + 1:b + 1 + a] = want[b:b + a]
                    if b + 1 + a < e:
                        toks[b + 1 + a] = (want[b + a] + 1) % V
                    agree.append(a)
                n_acc, picks = L.op_verify_rows_set(lg, toks, seg)
                assert picks.tolist() == want.tolist(), (kind, R, V, seg)
                assert n_acc.tolist() == [lookup_ref.n_accept(toks[b:e], want[b:e]) for b, e in zip(seg, seg[1:])], (kind, R, V, seg)
                assert n_acc.tolist() == agree, (kind, R, V, seg)
    # one segment is the single-sequence op
    lg = _rows_of_kind("ties", 9, V, rng)
    toks = rng.integers(0, V, 9).astype(np.int32)
    a, p = L.op_verify_rows(lg, toks)
    a2, p2 = L.op_verify_rows_set(lg, toks, [0, 9])
    assert (a, p.tolist()) == (int(a2[0]), p2.tolist())


def test_op_verify_rows_set_refusals(L):
    z = np.zeros((17, 8), np.float32)
    with pytest.raises(L.LlamaHipError, match=r"n_rows must be 1 \.\. 16 \(got 17\)"):
        L.op_verify_rows_set(z, np.zeros(17, np.int32), [0, 17])
    z = z[:6]
    t = np.zeros(6, np.int32)
    for seg, what in (([0, 4, 2, 6], r"seg_begin must ascend strictly \(segment 1: 4 \.\. 2\)"), ([0, 3, 3, 6], r"ascend strictly"),
                      ([1, 6], r"seg_begin must run from 0 to n_rows \(6; got 1 \.\. 6\)"), ([0, 5], r"must run from 0 to n_rows"),
                      ([0, 1, 2, 3, 4, 5, 6, 7], r"n_segs must be 1 \.\. n_rows \(6; got 7\)")):
        with pytest.raises(L.LlamaHipError, match=what):
            L.op_verify_rows_set(z, t, seg)


# ------------------------------------------------------------------------------------------------ 3. one step, known answers
@pytest.mark.parametrize("shape,nth", [("small", 8), ("small", 3), ("7b_width", 8)])
def test_verify_greedy_multi_with_known_answers(L, tmp_path, shape, nth):
    kw = SHAPES[shape]
    V, T = kw["n_vocab"], 36
    path = synth_tool(tmp_path / "m.bin", seed=72, **kw)
    lens = [122, 9, 30, 17]
    prompts = _prompts(4, V, lens, seed=50)
    with L.Model(path, n_ctx=N_CTX, n_seq=8) as h:
        S = _truth(h, prompts, 4, T, nth)
        _seed_slots(h, prompts, range(4), nth)
        pos = list(lens)          # every test slot's context
        # (rows per sequence, accepted length per sequence; None = the whole draft): 0, a part and the whole draft, with and without drafts
        for rows, acc in (((7, 1, 4, 4), (3, None, 0, None)), ((4, 4, 4, 4), (None, 0, 2, 1)), ((1, 12, 1, 2), (None, 5, None, 0)),
                          ((8, 2, 3, 3), (None, None, None, None))):
            drafts, want = [], []
            for i in range(4):
                o = pos[i] - lens[i]
                d = np.array(S[i][o + 1:o + rows[i]], np.int32)
                a = len(d) if acc[i] is None else acc[i]
                if a < len(d):
                    d[a] = (d[a] + 1) % V
                drafts.append(d)
                want.append(a)
            n_acc, picks = h.verify_greedy_multi(range(4), [S[i][pos[i] - lens[i]] for i in range(4)], drafts, pos, nth)
            tag = (shape, nth, rows, acc)
            assert n_acc.tolist() == want, tag
            for i in range(4):
                o = pos[i] - lens[i]
                assert picks[i][:want[i] + 1].tolist() == S[i][o + 1:o + want[i] + 2], tag + (i,)
                assert not _kv_diff(h, kw["n_layer"], 0, pos[i] + want[i] + 1, 4 + i, i), tag + (i,)
                pos[i] += want[i] + 1          # the next step starts from the new context: the rejected rows behind it do no harm
        assert pos[0] > 128
        for i in range(4):
            h.set_seq(i)
            o = pos[i] - lens[i]
            assert h.decode_greedy(S[i][o], pos[i], 2, nth).tolist() == S[i][o + 1:o + 3]
        with pytest.raises(L.LlamaHipError, match=r"n_past \(157\) \+ n_draft \(3\) \+ 1 > n_ctx \(160\)"):
            h.verify_greedy_multi([0, 1], [5, 5], [[1], [1, 2, 3]], [3, 157], nth)


# ------------------------------------------------------------------------------------------------ 4. the loop against decode_greedy per slot
LENS = [100, 7, 23, 12, 41]
N_STEPS = 40          # (sequence 0: positions 100 .. 139, over the 128-key boundary)


def _loop_case(h, n_layer, V, nth, dense=False):
    prompts = _prompts(5, V, LENS, seed=80)
    S = _truth(h, prompts, 5, N_STEPS, nth)
    Gs = [s[1:] for s in S]
    corpus = np.concatenate([np.array(g, np.int32) for g in Gs])          # the concatenated truth streams: the loop is sure to draft
    for n in (2, 3, 5):
        firsts = _seed_slots(h, prompts[:n], range(n), nth)
        assert firsts == [s[0] for s in S[:n]]
        want = lookup_multi_ref.loop_stats(prompts[:n], firsts, Gs[:n], corpus)
        if not dense:          # the restatement alone: with these seeds the run exercises the feature
            assert all(x["n_verify_steps"] + x["n_single_steps"] + x["n_accepted"] == N_STEPS for x in want), want
            assert sum(x["n_verify_steps"] for x in want) > 0 and sum(x["n_accepted"] > 0 for x in want) >= 2, want
        out, st = h.decode_greedy_lookup_multi(firsts, LENS[:n], N_STEPS, prompts[:n], corpus=corpus, n_threads=nth)
        for i in range(n):
            assert out[i].tolist() == Gs[i], (n, i, st[i], np.flatnonzero(out[i] != np.array(Gs[i]))[:5])
            assert not _kv_diff(h, n_layer, 0, LENS[i] + N_STEPS, 5 + i, i), (n, i)
            assert st[i]["n_verify_steps"] + st[i]["n_single_steps"] + st[i]["n_accepted"] == N_STEPS, st[i]
        if dense:          # the fall-back: llamahip_decode_greedy_lookup per slot, which drafts nothing on these files
            assert all(x == dict(n_verify_steps=0, n_single_steps=N_STEPS, n_drafted=0, n_accepted=0) for x in st), st
        else:
            assert st == want, (n, st, want)
    return prompts, S, corpus


@pytest.mark.parametrize("shape,nth,flags,devices", [("small", 8, 0, None), ("small", 3, 0, None), ("7b_width", 8, 0, None), ("small", 8, NO_GRAPH, None),
                                                     ("small", 8, 0, [0, 0]), ("7b_width", 8, 0, [0, 0])],
                         ids=["small", "small_3_threads", "7b_width", "no_graph", "two_stages", "two_stages_7b_width"])
def test_lookup_multi_equals_decode_greedy_per_slot(L, tmp_path, shape, nth, flags, devices):
    kw = SHAPES[shape]
    V = kw["n_vocab"]
    path = synth_tool(tmp_path / "m.bin", seed=73, **kw)
    with L.Model(path, n_ctx=N_CTX, n_seq=10, flags=flags, devices=devices) as h:
        prompts, S, corpus = _loop_case(h, kw["n_layer"], V, nth)
        assert h.stage_set_applies(16, nth) if devices is None else True          # (these shapes take the set path, not the fall-back)
        # the handle's current slot is as the caller left it: an eval behind the call lands there and nowhere else
        firsts = _seed_slots(h, prompts[:2], [0, 1], nth)
        h.set_seq(1)
        h.decode_greedy_lookup_multi(firsts, LENS[:2], N_STEPS, prompts[:2], corpus=corpus, n_threads=nth)
        h.eval(prompts[1], 0, nth)
        assert not _kv_diff(h, kw["n_layer"], 0, LENS[0] + N_STEPS, 5, 0) and not _kv_diff(h, kw["n_layer"], 0, LENS[1] + N_STEPS, 6, 1)
        # one sequence: decode_greedy_lookup on slot 0 -- tokens, KV and stats
        _seed_slots(h, prompts[:1], [0], nth)
        out, st = h.decode_greedy_lookup_multi([S[0][0]], LENS[:1], N_STEPS, prompts[:1], corpus=corpus, n_threads=nth)
        _seed_slots(h, prompts[:1], [1], nth)
        h.set_seq(1)
        out1, st1 = h.decode_greedy_lookup(S[0][0], N_STEPS, LENS[0], prompts[0], corpus=corpus, n_threads=nth)
        assert out[0].tolist() == out1.tolist() == S[0][1:] and st == [st1]
        assert not _kv_diff(h, kw["n_layer"], 0, LENS[0] + N_STEPS, 1, 0)
        # nothing to draft from (no corpus, n-grams longer than any repeat): decode_greedy_multi's tokens
        firsts = _seed_slots(h, prompts[:3], range(3), nth)
        out, st = h.decode_greedy_lookup_multi(firsts, LENS[:3], N_STEPS, prompts[:3], draft_len=1, ngram_min=24, ngram_max=24, n_threads=nth)
        _seed_slots(h, prompts[:3], range(3), nth)
        assert out.tolist() == h.decode_greedy_multi(firsts, LENS[:3], N_STEPS, nth).tolist() == [s[1:] for s in S[:3]]
        assert st == lookup_multi_ref.loop_stats(prompts[:3], firsts, [s[1:] for s in S[:3]], None, 1, 24, 24)


@pytest.mark.parametrize("kind", ["f16", "q4_1"])
def test_lookup_multi_on_files_without_a_set_step(L, tmp_path, kind):
    """f16 / Q4_1 files: the loop is decode_greedy_lookup per slot, one step is verify_greedy per slot"""
    hp = synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=4, n_layer=2)
    path = str(tmp_path / "m.bin")
    src = path + ".f16" if kind == "q4_1" else path
    synth.write_model_unquantized(src, hp, synth.random_tensors(hp, seed=9), 1)
    if kind == "q4_1":
        L.quantize_file(src, path, 3)
    with L.Model(path, n_ctx=N_CTX, n_seq=10) as h:
        prompts, S, _ = _loop_case(h, hp.n_layer, hp.n_vocab, 8, dense=True)
        _seed_slots(h, prompts[:2], [0, 1], 8)
        d = [np.array(S[0][1:6], np.int32), np.array(S[1][1:4], np.int32)]
        d[0][3] = (d[0][3] + 1) % hp.n_vocab
        n_acc, picks = h.verify_greedy_multi([0, 1], [S[0][0], S[1][0]], d, LENS[:2], 8)
        assert n_acc.tolist() == [3, 3] and picks[0].tolist() == S[0][1:5] + [-1, -1] and picks[1].tolist() == S[1][1:5]
        assert not _kv_diff(h, hp.n_layer, 0, LENS[0] + 4, 5, 0) and not _kv_diff(h, hp.n_layer, 0, LENS[1] + 4, 6, 1)


def test_lookup_multi_with_unfused_steps(L, tmp_path):
    path = synth_tool(tmp_path / "m.bin", seed=73, **SMALL)
    with L.Model(path, n_ctx=N_CTX, n_seq=10, flags=2) as h:
        prompts = _prompts(5, SMALL["n_vocab"], LENS, seed=80)
        S = _truth(h, prompts, 5, N_STEPS, 8)
        corpus = np.concatenate([np.array(s[1:], np.int32) for s in S])
        firsts = _seed_slots(h, prompts[:3], range(3), 8)
        out, st = h.decode_greedy_lookup_multi(firsts, LENS[:3], N_STEPS, prompts[:3], corpus=corpus)
        assert out.tolist() == [s[1:] for s in S[:3]]
        # (the fall-back runs the single-sequence loop per slot: its counts)
        assert st == [lookup_ref.loop_stats(prompts[i], firsts[i], S[i][1:], corpus) for i in range(3)]
        for i in range(3):
            assert not _kv_diff(h, SMALL["n_layer"], 0, LENS[i] + N_STEPS, 5 + i, i)


def test_lookup_multi_without_the_pinned_block(tmp_path):
    """LLAMAHIP_NO_HOST_IO: the step descriptor and the result travel as small copies instead of through the mapped host block (a fresh
    process: the switch is read at load)"""
    import subprocess
    import sys
    path = synth_tool(tmp_path / "m.bin", seed=73, **SMALL)
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"""
import sys
sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]
import numpy as np, llama_swift_amd as L, synth
lens = [100, 7, 23]
prompts = [synth.synth_prompt(lens[i], 2000, seed=80 + i) for i in range(3)]
with L.Model({path!r}, n_ctx=160, n_seq=6) as h:
    firsts, G = [], []
    for i in range(3):
        for s in (i, 3 + i):
            h.set_seq(s)
            f = int(np.argmax(h.eval(prompts[i], 0, 8)))
        firsts.append(f)
        G.append(h.decode_greedy(f, lens[i], 40, 8))
    out, st = h.decode_greedy_lookup_multi(firsts, lens, 40, prompts, corpus=np.concatenate(G))
    assert out.tolist() == [g.tolist() for g in G], st
    assert sum(x["n_accepted"] for x in st) > 0, st
print("NO_HOST_IO_OK")
"""
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LLAMAHIP_NO_HOST_IO="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "NO_HOST_IO_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_lookup_multi_refuses_a_stage_handle(L, tmp_path):
    path = synth_tool(tmp_path / "m.bin", seed=73, **SMALL)
    with L.Model(path, n_ctx=64, n_seq=2, layer_begin=0, layer_end=2) as st:
        with pytest.raises(L.LlamaHipError, match="pipeline-stage handle"):
            st.verify_greedy_multi([0, 1], [5, 5], [[1], []], [0, 0])
        with pytest.raises(L.LlamaHipError, match="pipeline-stage handle"):
            st.decode_greedy_lookup_multi([5, 5], [0, 0], 4, [[], []])
