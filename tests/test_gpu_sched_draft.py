"""GPU (-m gpu): drafted tokens inside the request scheduler (llamahip_sched_opts.draft_len > 0) against every request running ALONE on its
slot -- the yardstick of tests/test_gpu_sched.py, unchanged, and its helpers.

Per request: the tokens, the DONE reason and position and the KV rows [0, n_prompt + n - 1) of its slot in every layer, read at its DONE
event, bit for bit; for a request that carries a sampler also the sampler's window and rng state.  The drafts come from a corpus of the
requests' own plain outputs (every draft accepted), the same corpus with every fifth token altered (rejections at known rows), the requests'
own histories (prompts with a repeated n-gram), or from nowhere (no hit: the steps of a scheduler without drafts).  Same tiny models:
n_vocab 1500, d 256, 2 layers, head sizes 64 and 128, n_ctx 160, 5 KV slots of which the scheduler owns 3."""
import numpy as np
import pytest

from test_gpu_sched import (MAX_ACTIVE, N_CTX, N_SEQ, NO_GRAPH, REQS, _file, _sampled_alone, alone, check_against_alone, hparams, pair, prompt_of,
                            run_sched, same)

pytestmark = pytest.mark.gpu
KINDS = ("n_steps", "n_mixed_steps", "n_set_steps", "n_single_steps", "n_fallback_steps", "n_rows", "n_prompt_rows", "n_tokens")


def requests(hp):
    return [(prompt_of(hp, i, n), k) for i, (n, k) in enumerate(REQS)]


def own_outputs(hl, hp, reqs, chunk, nth, cache, ids=None):
    """the corpus of the accept-everything case: each request's last prompt token and its plain output (made alone on slot 0, once per key)"""
    out = []
    for j, (p, k) in enumerate(reqs):
        i = j if ids is None else ids[j]
        out += [int(p[-1])] + alone(hl, hp, 0, p, k, chunk, nth, cache, (chunk, nth, i, 0))[0]
    return np.asarray(out, np.int32)


def check_stats(st, note, fallback=False):
    assert st["n_tokens"] == st["n_emit_segs"] + st["n_accepted"] - st["n_dropped"], (note, st)          # the identity of llamahip.h
    assert 0 <= st["n_accepted"] <= st["n_drafted"] and st["n_dropped"] <= st["n_accepted"], (note, st)
    assert st["n_draft_steps"] <= st["n_mixed_steps"] and (st["n_drafted"] > 0) == (st["n_draft_steps"] > 0), (note, st)
    assert st["n_steps"] == st["n_mixed_steps"] + st["n_set_steps"] + st["n_single_steps"] + st["n_fallback_steps"], (note, st)
    assert (st["n_fallback_steps"] == st["n_steps"]) if fallback else st["n_fallback_steps"] == 0, (note, st)
    assert st["n_submitted"] == st["n_done"], (note, st)


# chunk_tokens 0 / 1 / 9, row_budget 1 / 16 / 64, n_threads 1 / 3 / 8, draft_len 1 / 4 / 15: every value in some row
GRID = [(0, 1, 1, 1), (1, 16, 3, 4), (9, 64, 8, 15), (9, 16, 8, 4), (0, 64, 3, 15), (1, 1, 8, 1), (9, 1, 1, 15)]


@pytest.mark.parametrize("chunk,budget,nth,draft_len", GRID)
def test_every_draft_accepted_and_every_request_still_the_request_alone(L, pair, chunk, budget, nth, draft_len):
    hp, _, hm, hl, cache = pair
    reqs = requests(hp)
    note = (chunk, budget, nth, draft_len)
    corpus = own_outputs(hl, hp, reqs, chunk, nth, cache)
    plain, st0, _ = run_sched(hm, hp, reqs, chunk, budget, nth)
    res, st, occupants = run_sched(hm, hp, reqs, chunk, budget, nth, draft_len=draft_len, corpus=corpus)
    check_against_alone(hl, hp, reqs, res, chunk, nth, cache, note)          # (n_predict reached exactly, by accepted runs: reason "length")
    for i in range(len(reqs)):
        assert res[i][0] == plain[i][0] and all(x == 1 for x in res[i][3]), (note, i)
    check_stats(st, note)
    assert st["n_accepted"] > 0 and st["n_draft_steps"] > 0, (note, st)          # the test cannot pass by drafting nothing
    assert st["n_steps"] < st0["n_steps"], (note, st["n_steps"], st0["n_steps"])
    assert st["n_tokens"] == st0["n_tokens"] == sum(k for _, k in REQS) and st["n_dropped"] == 0, (note, st)
    assert st["n_prompt_rows"] == sum(n for n, _ in REQS) and st["n_rows"] == st["n_prompt_rows"] + st["n_emit_segs"] - len(REQS) + st["n_drafted"], (note, st)
    assert st0["n_drafted"] == st0["n_draft_steps"] == st0["n_accepted"] == 0 and st0["n_emit_segs"] == st0["n_tokens"], st0
    assert sorted(occupants) == [0, 1, 2] and all(len(v) >= 2 for v in occupants.values()), (note, occupants)


@pytest.mark.parametrize("chunk,budget,nth,draft_len", [(9, 16, 8, 15), (0, 64, 3, 4), (1, 16, 1, 15)])
def test_rejections_at_known_rows(L, pair, chunk, budget, nth, draft_len):
    """the corpus with every fifth token altered: no accepted run passes an altered token"""
    hp, _, hm, hl, cache = pair
    reqs = requests(hp)
    corpus = own_outputs(hl, hp, reqs, chunk, nth, cache)
    corpus[4::5] = (corpus[4::5] + 1) % hp.n_vocab
    res, st, _ = run_sched(hm, hp, reqs, chunk, budget, nth, draft_len=draft_len, corpus=corpus)
    check_against_alone(hl, hp, reqs, res, chunk, nth, cache, ("altered", chunk, budget, nth, draft_len))
    check_stats(st, "altered")
    assert 0 < st["n_accepted"] < st["n_drafted"], st


def test_the_history_drafter_fires_on_prompts_with_a_repeated_ngram(L, pair):
    hp, _, hm, hl, cache = pair
    shapes = [(30, 9), (12, 14), (45, 6), (7, 8)]
    reqs = []
    for i, (n, k) in enumerate(shapes):
        gram = prompt_of(hp, 300 + i, 5)
        reqs.append((np.resize(gram, n).astype(np.int32), k))          # the 5-gram over and over: every suffix has an earlier occurrence
    for chunk, budget, nth, draft_len in ((9, 16, 8, 4), (0, 64, 3, 15)):
        res, st, _ = run_sched(hm, hp, reqs, chunk, budget, nth, draft_len=draft_len)
        check_against_alone(hl, hp, reqs, res, chunk, nth, None, ("history", chunk))
        check_stats(st, "history")
        assert st["n_drafted"] > 0 and st["n_draft_steps"] > 0, st


def test_no_hit_anywhere_is_the_scheduler_without_drafts(L, pair):
    hp, _, hm, hl, cache = pair
    reqs = requests(hp)
    for chunk, budget, nth in ((9, 16, 8), (0, 64, 3)):
        _, st0, _ = run_sched(hm, hp, reqs, chunk, budget, nth)
        # a 100-gram ending in what a request produced does not occur earlier in its random prompt, and no request's history is in this corpus
        res, st, _ = run_sched(hm, hp, reqs, chunk, budget, nth, draft_len=15, ngram_min=100, ngram_max=100, corpus=np.arange(140, dtype=np.int32))
        check_against_alone(hl, hp, reqs, res, chunk, nth, cache, ("no hit", chunk))
        check_stats(st, "no hit")
        assert st["n_drafted"] == st["n_draft_steps"] == st["n_accepted"] == 0, st
        assert [st[k] for k in KINDS] == [st0[k] for k in KINDS], (st, st0)


@pytest.mark.parametrize("mix", ["all_sampled", "greedy_and_sampled"])
def test_sampled_requests_draw_what_they_draw_alone(L, pair, mix):
    hp, _, hm, hl, cache = pair
    shapes = [(31, 9), (3, 14), (61, 4), (10, 8), (1, 12), (20, 6)]
    reqs = [(prompt_of(hp, 50 + i, n), k) for i, (n, k) in enumerate(shapes)]
    sampled = [True] * 6 if mix == "all_sampled" else [True, False, True, False, False, True]
    rln = (64, 8, 0, 64, 200, 16)
    for chunk, budget, nth, draft_len in ((9, 16, 8, 15), (0, 64, 3, 4)):
        # every request alone on slot 0 first: its stream is the corpus (a request's stream does not depend on its slot)
        ref = []
        for i, (p, k) in enumerate(reqs):
            if sampled[i]:
                ref.append(_sampled_alone(L, hl, hp, 0, p, k, 3000 + 7 * i, rln[i], chunk, nth))
            else:
                ref.append(alone(hl, hp, 0, p, k, chunk, nth) + (None,))
        corpus = np.asarray(sum(([int(p[-1])] + r[0] for (p, _), r in zip(reqs, ref)), []), np.int32)
        samplers = []
        for i, (p, _) in enumerate(reqs):
            s = L.Sampler(seed=3000 + 7 * i, repeat_last_n=rln[i]) if sampled[i] else None
            for t in (p if s is not None else ()):
                s.accept(int(t))
            samplers.append(s)
        res, st, _ = run_sched(hm, hp, reqs, chunk, budget, nth, samplers=samplers, draft_len=draft_len, corpus=corpus)
        check_stats(st, (mix, chunk))
        assert st["n_accepted"] > 0 and st["n_dropped"] == 0, st
        for i, (p, k) in enumerate(reqs):
            toks, ev, kv, exact = res[i]
            want, _, ws = ref[i]
            assert toks == want and ev["reason"] == "length" and ev["position"] == len(p) + k - 1, (mix, chunk, i, toks, want)
            # the KV rows on the slot the request got
            if sampled[i]:
                _, want_kv, _ = _sampled_alone(L, hl, hp, ev["slot"], p, k, 3000 + 7 * i, rln[i], chunk, nth) if ev["slot"] else ref[i]
                assert samplers[i].window().tolist() == ws.window().tolist(), (mix, chunk, i, "sampler window")
                lg = np.linspace(-1, 1, hp.n_vocab).astype(np.float32)          # the rng's next draw, on a fixed row
                assert samplers[i].sample(hm, lg) == ws.sample(hl, lg), (mix, chunk, i, "rng state")
            else:
                _, want_kv = alone(hl, hp, ev["slot"], p, k, chunk, nth)
                assert all(x == 1 for x in exact)
            for il in range(hp.n_layer):
                assert same(kv[il][0], want_kv[il][0]) and same(kv[il][1], want_kv[il][1]), (mix, chunk, i, il)


def test_a_stop_token_inside_an_accepted_run_cuts_the_stream(L, pair):
    hp, _, hm, hl, cache = pair
    idx = [0, 1, 3, 4, 5, 6]
    reqs = [(prompt_of(hp, i, REQS[i][0]), REQS[i][1]) for i in idx]
    streams = [alone(hl, hp, 0, p, k, 9, 8, cache, (9, 8, i, 0))[0] for i, (p, k) in zip(idx, reqs)]
    stops, cut = [], []
    for j, s in enumerate(streams):
        first_at = [k for k in range(2, len(s) - 1) if s[k] not in s[:k]]          # behind the first decode row, ahead of the last token
        if j == len(streams) - 1 or not first_at:          # a stop token its stream never contains
            stops.append(next(t for t in range(hp.n_vocab) if t not in s))
            cut.append(None)
            continue
        k = first_at[len(first_at) // 2]
        stops.append(s[k])
        cut.append(k)
    assert sum(c is not None for c in cut) >= 2, streams
    corpus = own_outputs(hl, hp, reqs, 9, 8, cache, ids=idx)
    for max_active in (MAX_ACTIVE, 2):
        res, st, occupants = run_sched(hm, hp, reqs, 9, 16, 8, max_active=max_active, stops=stops, draft_len=15, corpus=corpus)
        for j in range(len(streams)):
            toks, ev, kv, _ = res[j]
            s, want_kv = alone(hl, hp, ev["slot"], reqs[j][0], reqs[j][1], 9, 8, cache, (9, 8, idx[j], ev["slot"]))
            assert s == streams[j]
            if cut[j] is None:
                assert ev["reason"] == "length" and toks == s, (j, toks, s)
                continue
            # nothing is reported behind the stop token, whatever was accepted behind it
            assert ev["reason"] == "stop" and toks == s[:cut[j] + 1] and toks[-1] == stops[j], (j, toks, s, stops[j])
            n = len(reqs[j][0]) + len(toks) - 1
            assert ev["position"] == n
            for il in range(hp.n_layer):
                assert same(kv[il][0], want_kv[il][0][:n]) and same(kv[il][1], want_kv[il][1][:n]), (j, il)
        check_stats(st, ("stop", max_active))
        assert st["n_tokens"] == sum(len(res[j][0]) for j in range(len(reqs)))
        assert st["n_dropped"] > 0 and st["n_accepted"] > 0, st          # some stop token fell inside an accepted run
        assert any(len(v) >= 2 for v in occupants.values()), occupants          # a slot left at a stop token is reused


def test_submission_order_and_a_request_that_ends_exactly_at_n_ctx(L, pair):
    hp, _, hm, hl, cache = pair
    reqs = requests(hp)
    corpus = own_outputs(hl, hp, reqs, 9, 8, cache)
    base, _, _ = run_sched(hm, hp, reqs, 9, 16, 8)
    for order, budget in ((list(range(len(reqs)))[::-1], 16), ([4, 0, 8, 1, 7, 2, 6, 3, 5], 7)):
        res, st, _ = run_sched(hm, hp, reqs, 9, budget, 8, order=order, draft_len=15, corpus=corpus)
        check_stats(st, order)
        assert st["n_accepted"] > 0
        for i in range(len(reqs)):
            assert res[i][0] == base[i][0], (order, budget, i)
        check_against_alone(hl, hp, reqs, res, 9, 8, cache, ("order", budget))
    p = prompt_of(hp, 99, 150)          # 150 + 11 - 1 == n_ctx: the last accepted run ends at the context's end
    want, want_kv = alone(hl, hp, 0, p, 11, 9, 8)
    for draft_len in (15, 4):
        res, st, _ = run_sched(hm, hp, [(p, 11)], 9, 32, 8, max_active=2, draft_len=draft_len, corpus=np.asarray([int(p[-1])] + want, np.int32))
        assert res[0][0] == want and res[0][1]["reason"] == "length" and res[0][1]["position"] == N_CTX, res[0][:2]
        for il in range(hp.n_layer):
            assert same(res[0][2][il][0], want_kv[il][0]) and same(res[0][2][il][1], want_kv[il][1]), il
        assert st["n_accepted"] > 0 and st["n_steps"] < 17 + 10, st          # (17 prompt pieces, then ten single rows without drafts)


@pytest.mark.parametrize("kind", ["no_graph", "pipe2", "f16"])
def test_handles(L, tmp_path, kind):
    """NO_GRAPH and a two-stage pipeline handle draft like a plain one; an f16 file is a fall-back handle: zero drafts, the same events.  The
    library's device memory is back where it started once the scheduler and the handles are freed."""
    hp = hparams(4, n_layer=3 if kind == "pipe2" else 2)
    path = _file(L, tmp_path, "f16" if kind == "f16" else "q40", hp, 171)
    opts = dict(no_graph=dict(flags=NO_GRAPH), pipe2=dict(devices=[0, 0])).get(kind, {})
    shapes = [(61, 5), (20, 9), (9, 12), (10, 3), (1, 6), (3, 1)]
    reqs = [(prompt_of(hp, 80 + i, n), k) for i, (n, k) in enumerate(shapes)]
    before = L.live_allocs()
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, **opts) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hl:
        for chunk, budget in ((9, 16), (0, 8)):
            corpus = own_outputs(hl, hp, reqs, chunk, 8, None)
            plain, st0, _ = run_sched(hm, hp, reqs, chunk, budget, 8)
            res, st, _ = run_sched(hm, hp, reqs, chunk, budget, 8, draft_len=15, corpus=corpus)
            check_against_alone(hl, hp, reqs, res, chunk, 8, None, (kind, chunk))
            check_stats(st, (kind, chunk), fallback=kind == "f16")
            if kind == "f16":
                assert st["n_drafted"] == st["n_draft_steps"] == st["n_accepted"] == 0 and [st[k] for k in KINDS] == [st0[k] for k in KINDS], (st, st0)
                assert [res[i][0] for i in range(len(reqs))] == [plain[i][0] for i in range(len(reqs))]
            else:
                assert st["n_accepted"] > 0 and st["n_steps"] < st0["n_steps"] and st["n_mixed_steps"] > 0, (kind, st, st0)
        if kind == "pipe2":          # a sampled request beside a greedy one: the stages' words are pushed from the host
            want, _, ws = _sampled_alone(L, hl, hp, 0, reqs[1][0], reqs[1][1], 77, 16, 9, 8)
            s = L.Sampler(seed=77, repeat_last_n=16)
            for t in reqs[1][0]:
                s.accept(int(t))
            g_want = alone(hl, hp, 1, reqs[2][0], reqs[2][1], 9, 8)[0]
            res, st, _ = run_sched(hm, hp, reqs[1:3], 9, 16, 8, samplers=[s, None], draft_len=15, corpus=np.asarray(want + [int(reqs[2][0][-1])] + g_want, np.int32))
            assert res[0][0] == want and s.window().tolist() == ws.window().tolist() and res[1][0] == g_want, kind
            assert st["n_accepted"] > 0, st
    assert L.live_allocs() == before
