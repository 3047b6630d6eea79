"""GPU (-m gpu): llamahip_eval_logprobs_multi and llamahip_score_choices -- several texts scored in one weight pass -- against the per-slot
sequences they stand for.

Yardstick: a second handle on the same file doing set_seq + eval_logprobs per slot (tests/test_gpu_logprobs.py holds that call against the
oracle).  logprob / argmax / rank of the scored rows and the KV rows of every layer are compared by bytes; an unscored row reports
0.0 / -1 / -1 (it takes no lm head); KV rows outside the appended ranges, slots the call does not name and the handle's current slot keep what
they had.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import synth
from conftest import synth_tool

pytestmark = pytest.mark.gpu
N_CTX, N_SEQ = 192, 6
FAST_PREFILL = 16
HP = synth.HParams(n_vocab=2000, n_embd=256, n_mult=64, n_head=4, n_layer=2)
# the mixed segments: rows, n_past, slots (never ascending); slot 5 is named by no call
LENS, PAST, SLOTS = [1, 9, 10, 17, 3], [0, 5, 0, 20, 40], [3, 0, 4, 1, 2]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def tokens_of(hp, lens, seed):
    return [synth.synth_prompt(n, hp.n_vocab, seed=seed + 7 * i)[:n] for i, n in enumerate(lens)]


def prefix_of(hp, slot, n):
    return synth.synth_prompt(max(n, 1), hp.n_vocab, seed=900 + slot)[:n]


def targets_of(hp, lens, mode, seed):
    """None: the default (the next token inside the segment).  'all': every row.  'scattered': every third row unscored, the one-token
    segment scored.  'seg_off': one whole segment unscored.  'none': nothing scored at all."""
    if mode is None:
        return None
    rng = np.random.default_rng(seed)
    tg = [rng.integers(0, hp.n_vocab, n).astype(np.int32) for n in lens]
    if mode == "scattered":
        r = 0
        for t in tg:
            for j in range(t.size):
                if t.size > 1 and r % 3 == 1:
                    t[j] = -1
                r += 1
    elif mode == "seg_off":
        tg[len(lens) // 2][:] = -1
    elif mode == "none":
        for t in tg:
            t[:] = -1
    return tg


def default_targets(toks):
    return [np.concatenate([np.asarray(t[1:], np.int32), np.array([-1], np.int32)]) for t in toks]


def kv_all(h, n_layer, n_ctx, slots):
    out = {}
    for s in slots:
        h.set_seq(s)
        out[s] = [h.kv(il, n_ctx) for il in range(n_layer)]
    return out


def prefill(handles, hp, slots, n_past, nth=8):
    for h in handles:
        for s, p in zip(slots, n_past):
            if p > 0:
                h.set_seq(s)
                h.eval(prefix_of(hp, s, p), 0, nth)


def check_call(hm, hl, hp, lens, n_past, slots, chunk, nth, mode, seed, note, n_ctx=N_CTX, n_seq=N_SEQ, n_passes=1):
    """one eval_logprobs_multi on hm against set_seq + eval_logprobs per slot on hl; returns the call's stats"""
    toks = tokens_of(hp, lens, seed)
    tg = targets_of(hp, lens, mode, seed + 1)
    before = kv_all(hm, hp.n_layer, n_ctx, range(n_seq))
    cur = slots[-1]
    hm.set_seq(cur)
    got = hm.eval_logprobs_multi(slots, n_past, toks, targets=tg, chunk_tokens=chunk, n_threads=nth, want_stats=True)
    k_cur, v_cur = hm.kv(0, n_ctx)          # (read through the handle's current slot, which the call must leave alone)
    R = sum(lens)
    assert got["logprob"].shape == got["argmax"].shape == got["rank"].shape == (R,) and got["seg_begin"] == [int(x) for x in np.cumsum([0] + lens[:-1])]
    eff = tg if tg is not None else default_targets(toks)
    n_scored = 0
    for i, s in enumerate(slots):
        hl.set_seq(s)
        want = hl.eval_logprobs(toks[i], n_past[i], nth, targets=tg[i] if tg is not None else None, chunk_tokens=chunk)
        b = got["seg_begin"][i]
        scored = eff[i] >= 0
        n_scored += int(scored.sum())
        want_am = np.where(scored, want["argmax"], -1).astype(np.int32)          # the one deviation: an unscored row takes no lm head
        for key, w in (("logprob", want["logprob"]), ("argmax", want_am), ("rank", want["rank"])):
            assert same(got[key][b:b + lens[i]], w), (note, key, f"segment {i} (slot {s}, {lens[i]} rows at {n_past[i]})", got[key][b:b + lens[i]], w)
        assert not scored.any() or (want["rank"][scored] >= 0).all()
        assert (want["logprob"][~scored] == 0.0).all() and (want["rank"][~scored] == -1).all()
    after, want_kv = kv_all(hm, hp.n_layer, n_ctx, range(n_seq)), kv_all(hl, hp.n_layer, n_ctx, slots)
    assert same(k_cur, after[cur][0][0]) and same(v_cur, after[cur][0][1]), (note, "the handle's current slot moved")
    for s in range(n_seq):
        for il in range(hp.n_layer):
            for w in (0, 1):
                g, was = after[s][il][w], before[s][il][w]
                if s not in slots:
                    assert same(g, was), (note, f"slot {s} layer {il}: a slot the call does not name")
                    continue
                i = slots.index(s)
                end = n_past[i] + lens[i]
                assert same(g[:end], want_kv[s][il][w][:end]), (note, f"slot {s} layer {il} {'KV'[w]} rows [0, {end})")
                assert same(g[:n_past[i]], was[:n_past[i]]) and same(g[end:], was[end:]), (note, f"slot {s} layer {il}: rows outside [{n_past[i]}, {end})")
    st = got["stats"]
    assert st["n_rows"] == R and st["n_scored_rows"] == n_scored and st["n_passes"] == n_passes, (note, st)
    return st


@pytest.fixture(scope="module")
def pair(L, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("score") / "m.bin")
    synth.write_model(path, HP, synth.random_tensors(HP, seed=44))
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hl:
        prefill((hm, hl), HP, SLOTS, PAST)
        yield path, hm, hl


@pytest.mark.parametrize("chunk", [9, 0, 1])
@pytest.mark.parametrize("nth", [8, 3])
def test_mixed_segments_default_targets(L, pair, chunk, nth):
    """35 scored rows in one pass: more than the 16 rows the lm head's row list held before"""
    _, hm, hl = pair
    st = check_call(hm, hl, HP, LENS, PAST, SLOTS, chunk, nth, None, seed=100 + chunk, note=("default", chunk, nth))
    assert st["n_scored_rows"] == 35 and st["n_short_segs"] == 5 and st["n_long_segs"] == 0


@pytest.mark.parametrize("mode", ["all", "scattered", "seg_off", "none"])
def test_mixed_segments_explicit_targets(L, pair, mode):
    """explicit targets: every row, scattered -1 rows, one segment with no scored row, and a call with nothing scored at all (no lm head)"""
    _, hm, hl = pair
    for chunk, nth in ((9, 8), (0, 3), (1, 8)):
        st = check_call(hm, hl, HP, LENS, PAST, SLOTS, chunk, nth, mode, seed=200 + chunk, note=(mode, chunk, nth))
        if mode == "none":
            assert st["n_scored_rows"] == 0
        if mode == "all":
            assert st["n_scored_rows"] == sum(LENS)


def test_one_segment_is_the_scoring_eval_itself(L, pair):
    """n_seqs == 1 runs llamahip_eval_logprobs on that slot; the unscored last row reports argmax -1 on this path too"""
    _, hm, hl = pair
    st = check_call(hm, hl, HP, [23], [4], [5], 9, 8, None, seed=300, note="one segment")
    assert st["n_short_segs"] == 0 and st["n_long_segs"] == 0


def test_wide_model_long_segments_and_the_many_row_lm_head(L, tmp_path):
    """7B width, one layer: segments of 61 and 70 rows take attention launches of their own, and 137 scored rows take the lm head's many-row
    kernels (with `output`'s prompt copies, as a scoring eval of that many rows)"""
    kw = dict(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=1)
    hp = synth.HParams(**kw)
    path = synth_tool(tmp_path / "wide.bin", seed=17, **kw)
    lens, n_past, slots, C = [61, 9, 70], [0, 6, 10], [2, 0, 1], 96
    with L.Model(path, n_ctx=C, n_seq=3) as hm, L.Model(path, n_ctx=C, n_seq=3) as hl:
        prefill((hm, hl), hp, slots, n_past)
        for chunk, nth, mode in ((9, 8, None), (0, 3, "all")):
            st = check_call(hm, hl, hp, lens, n_past, slots, chunk, nth, mode, seed=400, note=("wide", chunk, nth, mode), n_ctx=C, n_seq=3)
            assert st["n_scored_rows"] == (137 if mode is None else 140) and st["n_long_segs"] == 2 and st["n_short_segs"] == 1


def test_pipeline_handle(L, pair):
    """the mixed case on a two-stage in-process pipeline: the rows cross the stages, the scoring runs on the last one"""
    path, _, hl = pair
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, devices=[0, 0]) as hm:
        prefill((hm,), HP, SLOTS, PAST)
        for chunk, nth, mode in ((9, 8, None), (0, 3, "scattered"), (1, 8, "none")):
            check_call(hm, hl, HP, LENS, PAST, SLOTS, chunk, nth, mode, seed=500 + chunk, note=("pipe2", chunk, nth, mode))


@pytest.mark.parametrize("kind", ["f16", "q41", "fast_prefill"])
def test_fall_backs_run_the_per_slot_loop(L, tmp_path, kind):
    """f16 / Q4_1 files and FAST_PREFILL handles: llamahip_eval_logprobs slot by slot, equal outputs, n_passes = the evals the loop made"""
    path = str(tmp_path / f"d_{kind}.bin")
    flags = 0
    if kind == "fast_prefill":
        synth.write_model(path, HP, synth.random_tensors(HP, seed=45))
        flags = FAST_PREFILL
    else:
        src = path + ".f16" if kind == "q41" else path
        synth.write_model_unquantized(src, HP, synth.random_tensors(HP, seed=1701), 1)
        if kind == "q41":
            L.quantize_file(src, path, 3)
            os.remove(src)
    dense = kind != "fast_prefill"
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, flags=flags) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, flags=flags) as hl:
        prefill((hm, hl), HP, SLOTS, PAST)
        for chunk, mode in ((9, None), (0, "scattered")):
            # (f16 / Q4_1 files below 36 rows: one eval per chunk of 9; else one eval per segment)
            n_evals = sum((n + 8) // 9 for n in LENS) if dense and chunk else len(LENS)
            e0 = hm.stats()["n_evals"]
            st = check_call(hm, hl, HP, LENS, PAST, SLOTS, chunk, 8, mode, seed=600 + chunk, note=(kind, chunk, mode), n_passes=n_evals)
            assert hm.stats()["n_evals"] - e0 == n_evals and st["n_short_segs"] == 0 and st["n_long_segs"] == 0


def choices_ref(h, hp, context, endings, chunk, nth):
    """the contract's sequence on slot i for every choice i: the context but its last token, then one scoring eval of the ending's rows"""
    P = len(context) - 1
    rows, sums, greedy = [], [], []
    for i, e in enumerate(endings):
        h.set_seq(i)
        if P > 0:
            h.eval_chunks(context[:P], 0, chunk, nth) if chunk > 0 else h.eval(context[:P], 0, nth)
        toks = np.concatenate([np.asarray(context[P:], np.int32), np.asarray(e[:-1], np.int32)])
        r = h.eval_logprobs(toks, P, nth, targets=np.asarray(e, np.int32), chunk_tokens=0)
        rows.append(r["logprob"])
        s = 0.0
        for x in r["logprob"]:
            s = s + float(x)
        sums.append(s)
        greedy.append(int((r["rank"] == 0).sum()))
    return rows, np.array(sums, np.float64), np.array(greedy, np.int32)


@pytest.fixture(scope="module")
def pair16(L, pair):
    path = pair[0]
    with L.Model(path, n_ctx=64, n_seq=16) as hm, L.Model(path, n_ctx=64, n_seq=16) as hl:
        yield hm, hl


@pytest.mark.parametrize("n_choices", [1, 4, 16])
def test_score_choices_is_the_per_choice_sequence(L, pair16, n_choices):
    hm, hl = pair16
    for n_context in (1, 10, 40):
        for chunk in (9, 0):
            seed = 700 + 10 * n_context + chunk
            context = synth.synth_prompt(max(n_context, 2), HP.n_vocab, seed=seed)[:n_context]
            lens = [1 + (3 * i + n_context) % 11 for i in range(n_choices)]          # 1 .. 11 rows, the one-token ending among them
            endings = tokens_of(HP, lens, seed + 1)
            hm.set_seq(n_choices - 1)
            got = hm.score_choices(context, endings, chunk_tokens=chunk, n_threads=8)
            rows, sums, greedy = choices_ref(hl, HP, context, endings, chunk, 8)
            note = (n_choices, n_context, chunk)
            assert same(got["logprob_sum"], sums) and same(got["n_greedy"], greedy), (note, got["logprob_sum"], sums, got["n_greedy"], greedy)
            assert len(got["rows"]) == n_choices and all(same(a, b) for a, b in zip(got["rows"], rows)), note
            for i in range(n_choices):
                end = n_context - 1 + lens[i]
                hm.set_seq(i)
                hl.set_seq(i)
                for il in range(HP.n_layer):
                    assert all(same(a, b) for a, b in zip(hm.kv(il, end), hl.kv(il, end))), (note, f"slot {i} layer {il} rows [0, {end})")


def test_score_choices_is_refused_under_a_live_scheduler(L, pair16):
    hm, _ = pair16
    context, endings = synth.synth_prompt(10, HP.n_vocab, seed=5)[:10], tokens_of(HP, [3, 4], 6)
    with L.Scheduler(hm, max_active=2):
        with pytest.raises(L.LlamaHipError) as e:
            hm.score_choices(context, endings)
        assert "llamahip_score_choices" in e.value.message and "scheduler" in e.value.message
    assert hm.score_choices(context, endings)["logprob_sum"].shape == (2,)
