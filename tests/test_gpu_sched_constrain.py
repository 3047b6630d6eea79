"""GPU (-m gpu): constrained requests inside the request scheduler (llamahip_request.constraint, llamahip_sched_opts.forced_drafts) against every
request running ALONE on its slot of a second handle -- the contract of include/llamahip.h, restated in tests/sched_dfa_ref.py: the tokens, the
DONE reason and the KV rows [0, n_prompt + n - 1) of every layer, read at the DONE event, bit for bit.  Tiny synthetic files as in
tests/test_gpu_constrain.py (n_vocab 300, n_embd 256, 2 layers, n_ctx 64), 6 KV slots of which the scheduler owns 4, chunks of 9.  Ten requests
in one scheduler: unconstrained greedy, unconstrained sampled and constrained greedy ones (the short regular expression, the choice set, a
choice set with long forced tails, a start state one token into an answer), two submission orders, row budgets 16 and the default; forced
drafts off, on, and on beside lookup drafts from a corpus.  For every constrained request the second handle's UNCONSTRAINED greedy stream from
the same prompt does not satisfy the constraint: the constraint acts."""
import re

import numpy as np
import pytest

import sched_dfa_ref as R
import synth
from test_gpu_sched import _sampled_alone
from test_gpu_sched import alone as free_alone

pytestmark = pytest.mark.gpu
HP = synth.HParams(n_vocab=300, n_embd=256, n_mult=64, n_head=4, n_layer=2)
VOCAB = synth.make_vocab(HP.n_vocab)
N_CTX, N_SEQ, MAX_ACTIVE, CHUNK, STOP, NTH = 64, 6, 4, 9, 2, 8
NO_GRAPH = 1
SHORT = "(ab|ba){1,3} tok0003[0-9]"
LONG = "[a-e]{20}"
CHOICES = [b"cab", b"cabbage", b"tok00100", b"d tok00200 e"]
BAD = 1          # an empty-text token: banned in every state of every constraint
# (kind, prompt length, n_predict): "s" sampled, "g" greedy, else the constraint's name; "choices+" starts one token into "d tok00200 e"
REQS = [("g", 7, 6), ("short", 1, 16), ("choices", 12, 16), ("s", 5, 5), ("tails", 20, 16), ("choices+", 4, 16), ("tails", 3, 3), ("g", 10, 8),
        ("short", 9, 16), ("tails", 2, 16)]
ORDERS = (list(range(len(REQS))), [9, 3, 0, 8, 4, 1, 7, 2, 6, 5])


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def prompt_of(i, n):
    return synth.synth_prompt(n, HP.n_vocab, seed=700 + 13 * i)[:n]


def write_file(L, tmp_path, kind):
    path = str(tmp_path / f"schedcst_{kind}.bin")
    if kind == "q4_0":
        synth.write_model(path, HP, synth.random_tensors(HP, seed=41))
    else:
        synth.write_model_unquantized(path, HP, synth.random_tensors(HP, seed=41), 1)
    return path


class World:
    """a handle under test, its yardstick handle, the constraints on both and the requests"""

    def __init__(self, L, hm, hl):
        self.L, self.hm, self.hl = L, hm, hl
        specs = dict(short=SHORT, choices=CHOICES, tails=R.TAILS, long=LONG)
        self.cs = {k: (hm.constraint(choices=v) if isinstance(v, list) else hm.constraint(regex=v)) for k, v in specs.items()}
        self.tables = {k: c.table() for k, c in self.cs.items()}
        self.cache = {}

    def close(self):
        for c in self.cs.values():
            c.close()

    def request(self, i, kind, n, k):
        """-> dict(prompt, n_predict, kind, constraint name or None, start state)"""
        name = None if kind in ("g", "s") else kind.rstrip("+")
        state = -1
        if kind == "choices+":
            state = self.cs[name].advance(self.cs[name].start, VOCAB.index(b"d"))
            assert state >= 0
        return dict(i=i, prompt=prompt_of(i, n), n_predict=k, kind=kind, name=name, state=state)

    def want(self, rq, slot):
        """the request alone on `slot` of the yardstick handle: (tokens, reason, KV rows), once per (request, slot)"""
        key = (rq["i"], slot, rq["n_predict"], rq["kind"])
        if key in self.cache:
            return self.cache[key]
        if rq["kind"] == "g":
            toks, kv = free_alone(self.hl, HP, slot, rq["prompt"], rq["n_predict"], CHUNK, NTH)
            out = (toks, "length", kv)
        elif rq["kind"] == "s":
            toks, kv, _ = _sampled_alone(self.L, self.hl, HP, slot, rq["prompt"], rq["n_predict"], 900 + rq["i"], 16, CHUNK, NTH)
            out = (toks, "length", kv)
        else:
            t = self.tables[rq["name"]]
            st = self.cs[rq["name"]].start if rq["state"] < 0 else rq["state"]
            out = R.alone(self.hl, HP.n_layer, slot, rq["prompt"], rq["n_predict"], CHUNK, t, st, STOP, NTH)
        self.cache[key] = out
        return out

    def the_constraint_acts(self, rq):
        """the condition on the inputs: the yardstick handle's unconstrained greedy stream from the same prompt does not satisfy the constraint"""
        if rq["name"] is None:
            return
        free, _ = free_alone(self.hl, HP, 0, rq["prompt"], 16, CHUNK, NTH, self.cache, ("free", rq["i"]))
        t = self.tables[rq["name"]]
        st = self.cs[rq["name"]].start if rq["state"] < 0 else rq["state"]
        assert not R.satisfied_by(t, st, free), (rq["i"], free)

    def run(self, reqs, order=None, budget=0, cancel_at=None, max_active=MAX_ACTIVE, **kw):
        """-> per request [tokens, DONE event, KV rows at DONE], the stats"""
        L, hm = self.L, self.hm
        res, by_id = {}, {}
        with hm.scheduler(max_active=max_active, chunk_tokens=CHUNK, row_budget=budget, n_threads=NTH, **kw) as sc:
            for j in (order if order is not None else range(len(reqs))):
                rq = reqs[j]
                smp = None
                if rq["kind"] == "s":
                    smp = L.Sampler(seed=900 + rq["i"], repeat_last_n=16)
                    for t in rq["prompt"]:
                        smp.accept(int(t))
                rid = sc.submit(rq["prompt"], rq["n_predict"], stop_token=-1, sampler=smp, constraint=None if rq["name"] is None else self.cs[rq["name"]],
                                constraint_state=rq["state"])
                by_id[rid] = j
                res[j] = [[], None, None]
            hm.set_seq(N_SEQ - 1)          # (the handle's current slot: not the scheduler's to move)
            steps = 0
            while sc.pending():
                for e in sc.step():
                    r = res[by_id[e["id"]]]
                    if e["kind"] == "token":
                        r[0].append(e["token"])
                        continue
                    r[1] = e
                    if e["slot"] >= 0 and e["position"] > 0:
                        hm.set_seq(e["slot"])
                        r[2] = [hm.kv(il, e["position"]) for il in range(HP.n_layer)]
                        hm.set_seq(N_SEQ - 1)
                if cancel_at is not None and len(res[cancel_at[0]][0]) >= cancel_at[1] and res[cancel_at[0]][1] is None:
                    rid = next(k for k, v in by_id.items() if v == cancel_at[0])
                    sc.cancel(rid)
                steps += 1
                assert steps < 500
            st = sc.stats()
        hm.set_seq(0)
        return res, st

    def check(self, reqs, res, note, skip=()):
        for j, rq in enumerate(reqs):
            if j in skip:
                continue
            toks, ev, kv = res[j]
            assert ev is not None and ev["slot"] >= 0, (note, j, ev)
            want, reason, want_kv = self.want(rq, ev["slot"])
            assert toks == want and ev["reason"] == reason, (note, f"request {j} {rq['kind']} in slot {ev['slot']}: {toks} {ev['reason']} vs {want} {reason}")
            n = len(rq["prompt"]) + len(toks) - 1
            assert ev["position"] == n, (note, j, ev)
            for il in range(HP.n_layer if n > 0 else 0):
                for w in (0, 1):
                    assert same(kv[il][w], want_kv[il][w][:n]), (note, f"request {j}: layer {il} {'KV'[w]} rows [0, {n})")


def check_stats(st, note, fallback=False):
    assert st["n_tokens"] == st["n_emit_segs"] + st["n_accepted"] - st["n_dropped"], (note, st)
    assert st["n_forced_accepted"] == st["n_forced_drafted"] <= st["n_drafted"] and st["n_forced_accepted"] <= st["n_accepted"] <= st["n_drafted"], (note, st)
    assert st["n_steps"] == st["n_mixed_steps"] + st["n_set_steps"] + st["n_single_steps"] + st["n_fallback_steps"], (note, st)
    assert (st["n_fallback_steps"] == st["n_steps"]) if fallback else st["n_fallback_steps"] == 0, (note, st)
    assert st["n_dfa_rows"] > 0, (note, st)


@pytest.fixture(scope="module")
def world(L, tmp_path_factory):
    path = write_file(L, tmp_path_factory.mktemp("schedcst"), "q4_0")
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hl:
        w = World(L, hm, hl)
        w.reqs = [w.request(i, *r) for i, r in enumerate(REQS)]
        yield w
        w.close()


def test_every_request_is_the_request_alone_with_forced_drafts_off_and_on(world):
    w = world
    for rq in w.reqs:
        w.the_constraint_acts(rq)
    steps = {}
    for forced in (False, True):
        for order, budget in zip(ORDERS, (16, 0)):
            note = ("forced" if forced else "plain", budget)
            res, st = w.run(w.reqs, order=order, budget=budget, forced_drafts=forced)
            w.check(w.reqs, res, note)
            check_stats(st, note)
            steps[(forced, budget)] = st["n_steps"]
            assert st["n_done"] == len(w.reqs)
            if forced:
                assert st["n_forced_drafted"] > 0 and st["n_draft_steps"] > 0, st
            else:
                assert st["n_drafted"] == st["n_forced_drafted"] == 0 and st["n_emit_segs"] == st["n_tokens"], st
            # the answers are what the constraints say, the short n_predict ends with LENGTH, the others at the stop token
            for j, rq in enumerate(w.reqs):
                toks, ev, _ = res[j]
                if rq["name"] is None:
                    continue
                if rq["n_predict"] == 3:
                    assert ev["reason"] == "length" and len(toks) == 3 and STOP not in toks
                    continue
                assert ev["reason"] == "stop" and toks[-1] == STOP
                text = b"".join(VOCAB[t] for t in toks[:-1])
                if rq["name"] == "short":
                    assert re.fullmatch(SHORT.encode(), text) is not None, text
                else:
                    assert (b"d" + text if rq["kind"] == "choices+" else text) in (CHOICES if rq["name"] == "choices" else R.TAILS), text
    for budget in (16, 0):          # forced tokens ride in spare rows: strictly fewer weight passes on the same workload
        assert steps[(True, budget)] < steps[(False, budget)], steps


def test_forced_drafts_beside_lookup_drafts(world):
    """draft_len 15 and a corpus beside forced drafts.  The unconstrained greedy requests' drafts come from their own plain outputs.  For a
    constrained request whose states force nothing ([a-e]{20}: every step starts where five tokens are allowed, so it drafts by lookup) the
    corpus holds, behind the end of its history at every point of its answer, its own next token and then a token every automaton bans: its
    lookup draft is cut in front of that token, and what is left of it is accepted"""
    w, L = world, world.L
    rl = w.request(21, "long", 6, 24)
    w.the_constraint_acts(rl)
    tl, cl = w.tables["long"], w.cs["long"]
    sl, _, _ = w.want(rl, 0)
    hist, pieces = [int(t) for t in rl["prompt"]], []
    for k, tok in enumerate(sl):
        if 1 <= k < len(sl) - 1:
            pieces += hist[-8:] + [tok, BAD, BAD]
        hist.append(tok)
    corpus = list(pieces)
    for j in (0, 7):
        corpus += [int(w.reqs[j]["prompt"][-1])] + w.want(w.reqs[j], 0)[0]
    corpus = np.asarray(corpus, np.int32)
    ngram = dict(ngram_min=4, ngram_max=8)
    # the condition on the inputs: behind the answer's first token the lookup draft is [the stream's next tokens ..., a banned token, ...]
    h1 = np.asarray([int(t) for t in rl["prompt"]] + sl[:1], np.int32)
    d = L.lookup_draft(h1, corpus, draft_len=15, **ngram).tolist()
    s1 = cl.advance(cl.start, sl[0])
    assert not R.forced(tl, s1, 15) and BAD in d[1:], d
    j = d.index(BAD)
    assert d[:j] == sl[1:1 + j], (d, sl)
    for t in d[:j]:
        s1 = cl.advance(s1, t)
        assert s1 >= 0
    assert cl.advance(s1, BAD) == -1
    # that request alone in the scheduler: an uncut draft would fail the step (the banned token has no state to be picked under); the cut
    # one carries the stream's own token, which is accepted
    for forced in (True, False):
        res, st1 = w.run([rl], forced_drafts=forced, draft_len=15, corpus=corpus, **ngram)
        w.check([rl], res, ("lookup, one request", forced))
        check_stats(st1, ("lookup, one request", forced))
        lookup_drafted, lookup_accepted = st1["n_drafted"] - st1["n_forced_drafted"], st1["n_accepted"] - st1["n_forced_accepted"]
        assert 0 < lookup_accepted <= lookup_drafted, st1
        assert forced or st1["n_forced_drafted"] == 0
    # the whole workload: lookup drafts of the unconstrained requests are accepted beside the forced ones
    for order, budget in zip(ORDERS, (16, 0)):
        res, st = w.run(w.reqs, order=order, budget=budget, forced_drafts=True, draft_len=15, corpus=corpus)
        w.check(w.reqs, res, ("lookup", budget))
        check_stats(st, ("lookup", budget))
        assert st["n_forced_drafted"] > 0 and st["n_accepted"] > st["n_forced_accepted"], st
    # draft_len alone: a constrained request drafts by lookup only, cut by its automaton
    res, st = w.run(w.reqs, budget=16, draft_len=15, corpus=corpus)
    w.check(w.reqs, res, "lookup without forced drafts")
    check_stats(st, "lookup without forced drafts")
    assert st["n_forced_drafted"] == 0 and st["n_drafted"] > 0, st


def test_decode_only_steps_reach_the_re_pick(world):
    """one short unconstrained request beside a 21-token constrained answer, no drafts: set steps while both decode, then single steps with the
    constrained slot alone -- the captured step as it is, k_sched_pick_dfa's re-pick behind it"""
    w = world
    reqs = [w.request(20, "g", 5, 3), w.request(21, "long", 6, 24), w.request(22, "tails", 8, 6)]
    for rq in reqs:
        w.the_constraint_acts(rq)
    res, st = w.run(reqs)
    w.check(reqs, res, "decode-only")
    check_stats(st, "decode-only")
    assert st["n_set_steps"] > 0 and st["n_single_steps"] > 0 and st["n_drafted"] == 0, st
    assert res[1][1]["reason"] == "stop" and len(res[1][0]) == 21 and st["n_single_steps"] >= 10
    # the same with forced drafts: [a-e]{20} forces nothing until its end, the choice set does
    res, st2 = w.run(reqs, forced_drafts=True)
    w.check(reqs, res, "decode-only, forced")
    check_stats(st2, "decode-only, forced")
    assert st2["n_set_steps"] + st2["n_single_steps"] > 0 and st2["n_forced_drafted"] > 0


def test_cancel_in_mid_answer(world):
    w = world
    reqs = [w.reqs[4], w.reqs[1], w.reqs[9]]
    for forced in (False, True):
        # (with forced drafts the step behind the first token carries the rest of the answer: the cancel comes in front of it)
        res, st = w.run(reqs, forced_drafts=forced, cancel_at=(0, 1 if forced else 2))
        toks, ev, kv = res[0]
        want, _, want_kv = w.want(reqs[0], ev["slot"])
        assert ev["reason"] == "cancelled" and 1 <= len(toks) < len(want) and toks == want[:len(toks)], (forced, toks, want)
        n = len(reqs[0]["prompt"]) + len(toks) - 1
        assert ev["position"] == n
        hm = w.hm
        for il in range(HP.n_layer):          # (the cancelled request's rows are still in its slot: nobody else was admitted)
            hm.set_seq(ev["slot"])
            k, v = hm.kv(il, n)
            hm.set_seq(0)
            assert same(k, want_kv[il][0][:n]) and same(v, want_kv[il][1][:n]), il
        w.check(reqs, res, ("cancel", forced), skip=(0,))
        check_stats(st, ("cancel", forced))


def test_submit_refusals_and_the_event_capacity(world):
    w, L = world, world.L
    hm = w.hm
    p = prompt_of(50, 4)
    with L.Model(hm.path, n_ctx=N_CTX, n_seq=N_SEQ, flags=4) as other, other.constraint(choices=CHOICES) as co:
        with hm.scheduler(max_active=2, chunk_tokens=CHUNK, forced_drafts=True) as sc:
            c = w.cs["choices"]
            with pytest.raises(L.LlamaHipError, match="llamahip_sched_submit: the constraint was made on another handle"):
                sc.submit(p, 4, constraint=co)
            with pytest.raises(L.LlamaHipError, match=rf"llamahip_sched_submit: constraint_state {c.n_states} out of range \[0, {c.n_states}\)"):
                sc.submit(p, 4, constraint=c, constraint_state=c.n_states)
            with pytest.raises(L.LlamaHipError, match=r"llamahip_sched_submit: constraint_state -2 out of range"):
                sc.submit(p, 4, constraint=c, constraint_state=-2)
            with pytest.raises(L.LlamaHipError, match=r"llamahip_sched_submit: stop_token 5 is neither -1 nor the constraint's stop token \(2\)"):
                sc.submit(p, 4, stop_token=5, constraint=c)
            with pytest.raises(L.LlamaHipError, match="llamahip_sched_submit: a sampler together with a constraint"):
                sc.submit(p, 4, constraint=c, sampler=L.Sampler(seed=1))
            assert sc.pending() == 0
            # forced_drafts with draft_len 0 requires LLAMAHIP_SCHED_EVENT_CAP(max_active, 1) events
            rid = sc.submit(p, 4, stop_token=STOP, constraint=c)
            with pytest.raises(L.LlamaHipError, match=r"llamahip_sched_step: cap \(18\) must be at least max_active \+ 17 \(19\)"):
                sc.step(cap=18)
            assert sc.pending() == 1 and sc.cancel(rid)
            sc.run()
    with L.Model(hm.path, n_ctx=N_CTX, n_seq=N_SEQ, devices=[0, 0]) as pipe, pipe.constraint(choices=CHOICES) as cp:
        with pipe.scheduler(max_active=2, chunk_tokens=CHUNK) as sc:
            with pytest.raises(L.LlamaHipError, match="llamahip_sched_submit: a constrained request on an in-process pipeline handle is not built"):
                sc.submit(p, 4, constraint=cp)


@pytest.mark.parametrize("kind", ["no_graph", "f16"])
def test_other_handles_and_live_allocations(L, tmp_path, kind):
    """NO_GRAPH steps like a plain handle; an f16 file takes fall-back steps (the contract's own loop per slot, nothing drafted).  The library's
    device memory is back where it started after constraint_free, sched_free and model_free."""
    path = write_file(L, tmp_path, "f16" if kind == "f16" else "q4_0")
    before = L.live_allocs()
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, **(dict(flags=NO_GRAPH) if kind == "no_graph" else {})) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hl:
        w = World(L, hm, hl)
        reqs = [w.request(i, *REQS[i]) for i in (0, 1, 4, 5, 6, 3)]
        for rq in reqs:
            w.the_constraint_acts(rq)
        for forced, extra in ((False, {}), (True, {}), (True, dict(draft_len=15))):
            res, st = w.run(reqs, budget=16, forced_drafts=forced, **extra)
            w.check(reqs, res, (kind, forced, extra))
            check_stats(st, (kind, forced), fallback=kind == "f16")
            if kind == "f16":
                assert st["n_drafted"] == st["n_forced_drafted"] == 0, st
            elif forced:
                assert st["n_forced_drafted"] > 0, st
        w.close()
    assert L.live_allocs() == before
