"""GPU (-m gpu): the request scheduler (llamahip_sched_*) -- prompts admitted into a running multi-sequence decode -- against every request
running ALONE on its slot.

Yardstick: a second handle on the same file doing, per request, set_seq(slot) + eval_chunks / eval of the prompt, the pick (argmax, lowest
index on ties) or the draw from that logits row, then single-token steps (decode_greedy, or eval_topk -> draw -> accept); for one case per
model the oracle making the same llama_eval calls.  Per request: the tokens, the DONE reason and the KV rows [0, n_prompt + n - 1) of its slot
in every layer, read at its DONE event (before the slot is reused), bit for bit.  n_ctx 160, 5 KV slots of which the scheduler owns 3,
d 256 with head sizes 64 and 128; nine requests through three slots, every slot reused, every later occupant shorter than the stale rows
above it."""
import os

import numpy as np
import pytest

import synth
from test_gpu_sample_multi import _single_stream

pytestmark = pytest.mark.gpu
N_CTX, N_SEQ, MAX_ACTIVE = 160, 5, 3
NO_GRAPH, UNFUSED, FAST_PREFILL = 1, 2, 16
# (prompt length, n_predict) in submission order: the contexts they end with descend, so whoever takes a slot later is shorter than the rows
# left in it.  61 and 64 exceed the short attention path's 60 rows (a long segment's own launches inside a mixed pass); 121 crosses the
# 128-position bucket of a set step while decoding; the one-token prompt decodes longest and ends the run alone (single steps)
REQS = [(121, 12), (64, 17), (61, 5), (31, 17), (1, 40), (20, 12), (10, 5), (9, 1), (3, 2)]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def hparams(n_head, n_layer=2):
    return synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=n_head, n_layer=n_layer)


def prompt_of(hp, i, n):
    return synth.synth_prompt(n, hp.n_vocab, seed=2000 + 13 * i)[:n]


@pytest.fixture(scope="module", params=[4, 2], ids=["head64", "head128"])
def pair(request, L, tmp_path_factory):
    """(hparams, path, the handle under test, the yardstick handle, the alone runs made so far) -- one per head size for the whole module"""
    hp = hparams(request.param)
    path = str(tmp_path_factory.mktemp("sched") / f"m{request.param}.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=140 + request.param))
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hl:
        yield hp, path, hm, hl, {}


def alone(hl, hp, slot, prompt, n_predict, chunk, nth, cache=None, key=None):
    """the request alone on `slot` of the yardstick handle: (tokens [n_predict], KV rows [0, n_prompt + n_predict - 1) of every layer).  Computed
    once per key -- (chunk, n_threads, request, slot): a request is compared with its run on the slot the scheduler gave it -- and left
    unchanged; a stream cut at a stop token is a prefix of it, its KV rows a prefix of these."""
    if cache is not None and key in cache:
        return cache[key]
    hl.set_seq(slot)
    lg = hl.eval_chunks(prompt, 0, chunk, nth) if chunk > 0 else hl.eval(prompt, 0, nth)
    toks = [int(np.argmax(lg))]
    if n_predict > 1:
        toks += hl.decode_greedy(toks[0], len(prompt), n_predict - 1, nth).tolist()
    n = len(prompt) + n_predict - 1
    kv = [hl.kv(il, n) for il in range(hp.n_layer)]
    hl.set_seq(0)
    if cache is not None:
        cache[key] = (toks, kv)
    return toks, kv


def run_sched(hm, hp, reqs, chunk, budget, nth, max_active=MAX_ACTIVE, order=None, stops=None, samplers=None, **kw):
    """submit reqs = [(prompt, n_predict)] (in `order`), run to the end; returns per request index (tokens, done event, KV rows read at DONE), the
    stats and the list of requests each slot held"""
    res, by_id, occupants = {}, {}, {}
    with hm.scheduler(max_active=max_active, chunk_tokens=chunk, row_budget=budget, n_threads=nth, **kw) as sc:
        for i in (order if order is not None else range(len(reqs))):
            rid = sc.submit(reqs[i][0], reqs[i][1], stop_token=-1 if stops is None else stops[i], sampler=None if samplers is None else samplers[i])
            by_id[rid] = i
            res[i] = [[], None, None, []]
        hm.set_seq(N_SEQ - 1)          # (the handle's current slot: not the scheduler's to move)
        steps = 0
        while sc.pending():
            for e in sc.step():
                r = res[by_id[e["id"]]]
                if e["kind"] == "token":
                    r[0].append(e["token"])
                    r[3].append(e["exact"])
                    continue
                r[1] = e
                if e["slot"] >= 0:
                    occupants.setdefault(e["slot"], []).append(by_id[e["id"]])
                    hm.set_seq(e["slot"])
                    r[2] = [hm.kv(il, e["position"]) for il in range(hp.n_layer)] if e["position"] > 0 else []
                    hm.set_seq(N_SEQ - 1)
            steps += 1
            assert steps < 3000
        st = sc.stats()
    hm.set_seq(0)
    return res, st, occupants


def check_against_alone(hl, hp, reqs, res, chunk, nth, cache, note):
    for i, (prompt, n_predict) in enumerate(reqs):
        toks, ev, kv, _ = res[i]
        assert ev is not None and ev["reason"] == "length", (note, i, ev)
        want, want_kv = alone(hl, hp, ev["slot"], prompt, n_predict, chunk, nth, cache, (chunk, nth, i, ev["slot"]))
        assert toks == want, (note, f"request {i} ({len(prompt)} + {n_predict}) in slot {ev['slot']}: {toks} vs {want}")
        n = len(prompt) + n_predict - 1
        assert ev["position"] == n
        for il in range(hp.n_layer):
            for w in (0, 1):
                assert same(kv[il][w], want_kv[il][w][:n]), (note, f"request {i}: layer {il} {'KV'[w]} rows [0, {n})")


@pytest.mark.parametrize("budget", [1, 16, 64])
@pytest.mark.parametrize("chunk", [0, 1, 9])
def test_every_request_is_the_request_alone(L, pair, chunk, budget):
    hp, _, hm, hl, cache = pair
    reqs = [(prompt_of(hp, i, n), k) for i, (n, k) in enumerate(REQS)]
    for nth in (1, 3, 8):
        note = (chunk, budget, nth)
        hm.set_seq(N_SEQ - 1)
        k_cur = hm.kv(0, N_CTX)
        res, st, occupants = run_sched(hm, hp, reqs, chunk, budget, nth)
        hm.set_seq(N_SEQ - 1)
        hm_kv_cur = hm.kv(0, N_CTX)
        assert same(k_cur[0], hm_kv_cur[0]) and same(k_cur[1], hm_kv_cur[1]), (note, "a slot the scheduler does not own changed")
        check_against_alone(hl, hp, reqs, res, chunk, nth, cache, note)
        # every kind of step ran, nothing fell back silently; the rows and tokens add up
        assert st["n_mixed_steps"] > 0 and st["n_set_steps"] > 0 and st["n_single_steps"] > 0 and st["n_fallback_steps"] == 0, (note, st)
        assert st["n_steps"] == st["n_mixed_steps"] + st["n_set_steps"] + st["n_single_steps"], (note, st)
        assert st["n_tokens"] == sum(k for _, k in REQS) and st["n_prompt_rows"] == sum(n for n, _ in REQS), (note, st)
        assert st["n_rows"] == st["n_prompt_rows"] + st["n_tokens"] - len(REQS), (note, st)
        assert st["n_submitted"] == st["n_done"] == len(REQS), (note, st)          # (the set-step graphs may be there already: test_handles counts captures)
        assert sorted(occupants) == [0, 1, 2] and all(len(v) >= 2 for v in occupants.values()), (note, occupants)
        for v in occupants.values():          # every later occupant is shorter than the rows its predecessor left
            ends = [REQS[i][0] + REQS[i][1] - 1 for i in v]
            assert ends == sorted(ends, reverse=True), (note, occupants)


def test_against_the_oracles_evals(L, oracle, pair):
    """chunks of 9, 8 threads, budget 16: the oracle makes each request's llama_eval calls (prompt in 9-token evals, then one token at a time)"""
    hp, path, hm, _, _ = pair
    reqs = [(prompt_of(hp, i, n), k) for i, (n, k) in enumerate(REQS)]
    res, _, _ = run_sched(hm, hp, reqs, 9, 16, 8)
    for i in (0, 2, 4, 6):
        prompt, n_predict = reqs[i]
        om = oracle.load(path, n_ctx=N_CTX)
        for c0 in range(0, len(prompt), 9):
            lg = om.eval(prompt[c0:c0 + 9], c0, 8)["logits"]
        want = [int(np.argmax(lg))]
        for t in range(n_predict - 1):
            want.append(int(np.argmax(om.eval(np.array([want[-1]], np.int32), len(prompt) + t, 8)["logits"])))
        assert res[i][0] == want, ("oracle", i)
        n = len(prompt) + n_predict - 1
        for il in range(hp.n_layer):
            wk, wv = om.kv(il, n)
            assert same(res[i][2][il][0], wk) and same(res[i][2][il][1], wv), ("oracle", i, il)
        om.close()


def test_submission_order_and_budget_do_not_change_a_request(L, pair):
    hp, _, hm, hl, cache = pair
    reqs = [(prompt_of(hp, i, n), k) for i, (n, k) in enumerate(REQS)]
    base, _, _ = run_sched(hm, hp, reqs, 9, 16, 8)
    for order, budget in ((list(range(len(reqs)))[::-1], 16), (None, 40), ([4, 0, 8, 1, 7, 2, 6, 3, 5], 7)):
        res, st, _ = run_sched(hm, hp, reqs, 9, budget, 8, order=order)
        assert st["n_fallback_steps"] == 0
        for i in range(len(reqs)):
            assert res[i][0] == base[i][0], (order, budget, i)
        check_against_alone(hl, hp, reqs, res, 9, 8, cache, ("invariance", budget))


def test_stop_token_cuts_the_stream(L, pair):
    hp, _, hm, hl, cache = pair
    idx = [0, 1, 3, 4, 5, 6]
    reqs = [(prompt_of(hp, i, REQS[i][0]), REQS[i][1]) for i in idx]
    # (the streams the stop tokens are chosen from are made on slot 0, before anybody knows the slots; the comparison below is with the run on
    #  the slot the request got)
    streams = [alone(hl, hp, 0, p, k, 9, 8, cache, (9, 8, i, 0))[0] for i, (p, k) in zip(idx, reqs)]
    stops, cut = [], []
    for j, s in enumerate(streams):
        first_at = [k for k in range(1, len(s)) if s[k] not in s[:k]]          # tokens whose first occurrence is at an index k > 0
        if j == len(streams) - 1 or not first_at:          # a stop token its stream never contains
            stops.append(next(t for t in range(hp.n_vocab) if t not in s))
            cut.append(None)
            continue
        k = first_at[len(first_at) // 2]
        stops.append(s[k])
        cut.append(k)
    assert sum(c is not None for c in cut) >= 2, streams
    res, st, _ = run_sched(hm, hp, reqs, 9, 16, 8, stops=stops)
    for j in range(len(streams)):
        toks, ev, kv, _ = res[j]
        s, want_kv = alone(hl, hp, ev["slot"], reqs[j][0], reqs[j][1], 9, 8, cache, (9, 8, idx[j], ev["slot"]))
        assert s == streams[j]
        if cut[j] is None:
            assert ev["reason"] == "length" and toks == s, (j, toks, s)
            continue
        assert ev["reason"] == "stop" and toks == s[:cut[j] + 1] and toks[-1] == stops[j], (j, toks, s, stops[j])
        n = len(reqs[j][0]) + len(toks) - 1
        assert ev["position"] == n
        for il in range(hp.n_layer):
            assert same(kv[il][0], want_kv[il][0][:n]) and same(kv[il][1], want_kv[il][1][:n]), (j, il)
    assert st["n_tokens"] == sum(len(res[j][0]) for j in range(len(reqs)))


def test_cancel_a_queued_and_an_active_request(L, pair):
    hp, _, hm, hl, cache = pair
    idx = [1, 3, 5, 6, 7]
    reqs = [(prompt_of(hp, i, REQS[i][0]), REQS[i][1]) for i in idx]
    got, done = {}, {}
    with hm.scheduler(max_active=2, chunk_tokens=9, row_budget=16, n_threads=8) as sc:
        ids = [sc.submit(p, k) for p, k in reqs]
        assert sc.pending() == 5
        assert sc.cancel(ids[3]) and not sc.cancel(ids[3]) and not sc.cancel(12345)          # queued: it never gets a slot
        steps = 0
        while sc.pending():
            for e in sc.step():
                j = ids.index(e["id"])
                if e["kind"] == "token":
                    got.setdefault(j, []).append(e["token"])
                else:
                    done[j] = e
            steps += 1
            if steps == 12:
                assert 0 in got and 0 not in done
                assert sc.cancel(ids[0])          # active and decoding
            assert steps < 1000
    assert done[3]["reason"] == "cancelled" and done[3]["slot"] == -1 and 3 not in got
    assert done[0]["reason"] == "cancelled" and done[0]["slot"] in (0, 1) and 0 < len(got[0]) < reqs[0][1]
    want0 = alone(hl, hp, done[0]["slot"], reqs[0][0], reqs[0][1], 9, 8, cache, (9, 8, idx[0], done[0]["slot"]))[0]
    assert got[0] == want0[:len(got[0])]
    for j in (1, 2, 4):
        assert done[j]["reason"] == "length"
        assert got[j] == alone(hl, hp, done[j]["slot"], reqs[j][0], reqs[j][1], 9, 8, cache, (9, 8, idx[j], done[j]["slot"]))[0], j


def _sampled_alone(L, hl, hp, slot, prompt, n_predict, seed, rln, chunk, nth):
    hl.set_seq(slot)
    lg = hl.eval_chunks(prompt, 0, chunk, nth) if chunk > 0 else hl.eval(prompt, 0, nth)
    s = L.Sampler(seed=seed, repeat_last_n=rln)
    for t in prompt:
        s.accept(int(t))
    first = s.sample(hl, lg)
    s.accept(first)
    rest, _ = _single_stream(L, hl, slot, first, len(prompt), s, n_predict - 1, nth) if n_predict > 1 else ([], [])
    hl.set_seq(slot)
    n = len(prompt) + n_predict - 1
    kv = [hl.kv(il, n) for il in range(hp.n_layer)]
    hl.set_seq(0)
    return [first] + rest, kv, s


@pytest.mark.parametrize("mix", ["all_sampled", "greedy_and_sampled"])
def test_sampled_requests_draw_what_they_draw_alone(L, pair, mix):
    hp, _, hm, hl, cache = pair
    shapes = [(31, 9), (3, 14), (61, 4), (10, 8), (1, 12), (20, 6)]
    reqs = [(prompt_of(hp, 50 + i, n), k) for i, (n, k) in enumerate(shapes)]
    sampled = [True] * 6 if mix == "all_sampled" else [True, False, True, False, False, True]
    rln = (64, 8, 0, 64, 200, 16)
    for chunk, budget, nth in ((9, 16, 8), (0, 64, 3)):
        samplers = []
        for i, (p, _) in enumerate(reqs):
            s = L.Sampler(seed=3000 + 7 * i, repeat_last_n=rln[i]) if sampled[i] else None
            for t in (p if s is not None else ()):
                s.accept(int(t))
            samplers.append(s)
        res, st, _ = run_sched(hm, hp, reqs, chunk, budget, nth, samplers=samplers)
        assert st["n_mixed_steps"] > 0 and st["n_set_steps"] > 0 and st["n_fallback_steps"] == 0, st
        for i, (p, k) in enumerate(reqs):
            toks, ev, kv, exact = res[i]
            if not sampled[i]:
                want, want_kv = alone(hl, hp, ev["slot"], p, k, chunk, nth)
                assert all(x == 1 for x in exact)
            else:
                want, want_kv, ws = _sampled_alone(L, hl, hp, ev["slot"], p, k, 3000 + 7 * i, rln[i], chunk, nth)
                assert samplers[i].window().tolist() == ws.window().tolist(), (mix, chunk, i, "sampler window")
                lg = np.linspace(-1, 1, hp.n_vocab).astype(np.float32)          # the rng's next draw, on a fixed row
                assert samplers[i].sample(hm, lg) == ws.sample(hl, lg), (mix, chunk, i, "rng state")
            assert toks == want and ev["reason"] == "length", (mix, chunk, i, toks, want)
            for il in range(hp.n_layer):
                assert same(kv[il][0], want_kv[il][0]) and same(kv[il][1], want_kv[il][1]), (mix, chunk, i, il)


def _file(L, tmp_path, ftype, hp, seed):
    path = str(tmp_path / f"m_{ftype}.bin")
    if ftype == "q40":
        synth.write_model(path, hp, synth.random_tensors(hp, seed=seed))
        return path
    src = path + ".f16" if ftype == "q41" else path
    synth.write_model_unquantized(src, hp, synth.random_tensors(hp, seed=seed), 1)
    if ftype == "q41":
        L.quantize_file(src, path, 3)
        os.remove(src)
    return path


@pytest.mark.parametrize("kind", ["no_graph", "pipe2", "f16", "q41", "unfused", "fast_prefill", "threads_40"])
def test_handles(L, tmp_path, kind):
    """NO_GRAPH and a two-stage pipeline take mixed passes and set steps; f16 and Q4_1 files, LLAMAHIP_FLAG_UNFUSED handles and a thread count
    without a set step run the contract's per-slot calls: the stats show only fall-back steps; the same events and bits everywhere.  So does a
    LLAMAHIP_FLAG_FAST_PREFILL handle (yardstick: a handle with the same flag; its prompts here stay below the rows at which that flag
    changes a mat-mul, the one place it makes no parity claim)"""
    hp = hparams(4, n_layer=3 if kind == "pipe2" else 2)
    ftype = kind if kind in ("f16", "q41") else "q40"
    path = _file(L, tmp_path, ftype, hp, 171)
    opts = dict(no_graph=dict(flags=NO_GRAPH), pipe2=dict(devices=[0, 0]), unfused=dict(flags=UNFUSED), fast_prefill=dict(flags=FAST_PREFILL)).get(kind, {})
    nth = 40 if kind == "threads_40" else 8
    shapes = [(61, 5), (20, 9), (9, 12), (10, 3), (1, 6), (3, 1)]
    reqs = [(prompt_of(hp, 80 + i, n), k) for i, (n, k) in enumerate(shapes)]
    fallback = kind in ("f16", "q41", "unfused", "fast_prefill", "threads_40")
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, **opts) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, **(opts if kind == "fast_prefill" else {})) as hl:
        for chunk, budget in ((9, 16), (0, 8)):
            res, st, _ = run_sched(hm, hp, reqs, chunk, budget, nth)
            check_against_alone(hl, hp, reqs, res, chunk, nth, None, (kind, chunk))
            if fallback:
                assert st["n_fallback_steps"] == st["n_steps"] > 0 and st["n_mixed_steps"] == st["n_set_steps"] == st["n_single_steps"] == 0, (kind, st)
                assert st["n_graph_captures"] == 0
            else:
                assert st["n_fallback_steps"] == 0 and st["n_mixed_steps"] > 0 and st["n_set_steps"] > 0, (kind, st)
                assert st["n_graph_captures"] > 0 or chunk != 9, (kind, st)          # a fresh handle has to capture the sets of its first run
        if kind in ("pipe2", "f16"):          # a sampled request beside a greedy one
            s = L.Sampler(seed=77, repeat_last_n=16)
            for t in reqs[1][0]:
                s.accept(int(t))
            res, st, _ = run_sched(hm, hp, reqs[1:3], 9, 16, nth, samplers=[s, None])
            want, _, ws = _sampled_alone(L, hl, hp, 0, reqs[1][0], reqs[1][1], 77, 16, 9, nth)
            assert res[0][0] == want and s.window().tolist() == ws.window().tolist(), kind
            assert res[1][0] == alone(hl, hp, 1, reqs[2][0], reqs[2][1], 9, nth)[0], kind


def test_a_request_that_ends_exactly_at_n_ctx_and_the_refusals_of_a_live_scheduler(L, pair):
    hp, _, hm, hl, _ = pair
    ERR = L.binding.ERR_PREDICT
    p = prompt_of(hp, 99, 150)
    with hm.scheduler(max_active=2, chunk_tokens=9, row_budget=32, n_threads=8) as sc:
        for bad, word in ((dict(prompt=p, n_predict=12), "n_ctx"), (dict(prompt=[hp.n_vocab], n_predict=1), "token id"),
                          (dict(prompt=[], n_predict=1), "n_prompt"), (dict(prompt=[1], n_predict=0), "n_predict"),
                          (dict(prompt=[1], n_predict=1, stop_token=hp.n_vocab), "stop_token")):
            with pytest.raises(L.LlamaHipError) as e:
                sc.submit(**bad)
            assert e.value.code == ERR and word in e.value.message, (bad.keys(), e.value.message)
        s = L.Sampler(seed=1)
        sc.submit([5, 6], 2, sampler=s)
        with pytest.raises(L.LlamaHipError) as e:
            sc.submit([7], 2, sampler=s)
        assert "sampler" in e.value.message
        rid = sc.submit(p, 11)          # 150 + 11 - 1 == n_ctx
        # a cap too small for a step's events: refused, nothing consumed
        with pytest.raises(L.LlamaHipError) as e:
            sc.step(cap=2 * 2)
        assert e.value.code == ERR and "cap" in e.value.message and sc.pending() == 2 and sc.stats()["n_steps"] == 0
        out = sc.run()
        assert len(out[rid]) == 11
    want, _ = alone(hl, hp, 1, p, 11, 9, 8)
    assert out[rid] == want
    with hm.scheduler(max_active=2, chunk_tokens=0, row_budget=8, n_threads=8) as sc:          # chunk_tokens 0: the prompt is one piece
        rid = sc.submit(p, 11)
        assert sc.run()[rid] == alone(hl, hp, 0, p, 11, 0, 8)[0]
    with pytest.raises(L.LlamaHipError) as e:
        hm.scheduler(max_active=N_SEQ + 1)
    assert "max_active" in e.value.message


def test_one_scheduler_per_handle_and_a_handle_freed_first(L, pair, tmp_path):
    hp, path, hm, _, _ = pair
    with hm.scheduler(max_active=2) as sc:
        with pytest.raises(L.LlamaHipError) as e:
            hm.scheduler(max_active=1)
        assert e.value.code == L.binding.ERR_PREDICT and "already has a scheduler" in e.value.message
        rid = sc.submit([3, 4, 5], 2)
        assert len(sc.run()[rid]) == 2
    hm.scheduler(max_active=1).close()          # free again
    # the handle closed under a live scheduler: its steps fail, freeing it touches nothing
    h2 = L.Model(path, n_ctx=N_CTX, n_seq=2)
    sc = h2.scheduler(max_active=2)
    rid = sc.submit([3, 4, 5], 3)
    assert len(sc.step()) == 1
    h2.close()
    with pytest.raises(L.LlamaHipError) as e:
        sc.step()
    assert "freed" in e.value.message and sc.pending() == 1
    sc.close()
