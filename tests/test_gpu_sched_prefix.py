"""GPU (-m gpu): the request scheduler with shared prompt prefixes (llamahip_sched_opts.prefix_share; include/llamahip.h "Evaluated prompt
prefixes shared between KV slots") -- against every request running ALONE on its slot from position 0.

Yardstick: tests/test_gpu_sched.py's, imported: a second handle doing, per request, set_seq(slot) + eval_chunks of the WHOLE prompt from 0,
the pick or the draw, then single-token steps.  Per request: the tokens, the DONE reason and the KV rows [0, n_prompt + n - 1) of its slot in
every layer, read at its DONE event, bit for bit -- whatever rows were taken over in place or copied from whichever donor.  Beside the
scheduler runs a Python model of its admissions (the policy restated in tests/test_sched_prefix_host.py, the step rule through
llamahip_sched_plan, the tokens a request produced taken from the events): the slot every request gets, n_shared_rows and n_copied_rows
must be the model's.  n_ctx 160, 5 KV slots of which the scheduler owns 3, d 256 with head sizes 64 and 128."""
import numpy as np
import pytest

import synth
from test_gpu_sched import (FAST_PREFILL, MAX_ACTIVE, N_CTX, N_SEQ, UNFUSED, _file, _sampled_alone, alone, check_against_alone, hparams,
                            prompt_of, same)
from test_sched_prefix_host import plan_prefix_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[4, 2], ids=["head64", "head128"])
def pair(request, L, tmp_path_factory):
    hp = hparams(request.param)
    path = str(tmp_path_factory.mktemp("prefix") / f"m{request.param}.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=240 + request.param))
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hl:
        yield hp, path, hm, hl


def with_prefix(hp, sys_id, n_sys, tail_id, n_tail):
    """the first n_sys tokens of system prompt `sys_id`, then n_tail tokens of its own"""
    return np.concatenate([prompt_of(hp, sys_id, 64)[:n_sys], prompt_of(hp, tail_id, n_tail + 1)[1:]]).astype(np.int32)


def unrelated(hp, i, n):
    """a prompt that shares not even the BOS with the others"""
    return prompt_of(hp, i, n + 1)[1:]


class Run:
    """a scheduler and the model of its admissions side by side; res[i] = [tokens, done event, KV rows read at DONE, exact flags]"""

    def __init__(self, L, hm, hp, chunk, budget, nth, share=True, handle_shares=True, max_active=MAX_ACTIVE, **kw):
        self.L, self.hm, self.hp, self.chunk, self.budget, self.A = L, hm, hp, chunk, budget, max_active
        self.sc = hm.scheduler(max_active=max_active, chunk_tokens=chunk, row_budget=budget, n_threads=nth, prefix_share=share, **kw)
        self.sharing = share and handle_shares and chunk > 0
        self.reqs, self.res, self.ids, self.samplers = [], {}, {}, {}
        self.queue, self.order, self.slot = [], [], [None] * max_active          # the model: request indices
        self.held = [([], 0) for _ in range(max_active)]
        self.off, self.slot_of, self.log, self.events = {}, {}, [], []
        self.shared = self.copied = self.copies = self.steps = 0
        hm.set_seq(N_SEQ - 1)          # (the handle's current slot: not the scheduler's to move)

    def submit(self, prompt, n_predict, sampler=None):
        i = len(self.reqs)
        self.ids[self.sc.submit(prompt, n_predict, sampler=sampler)] = i
        self.reqs.append((np.asarray(prompt, np.int32), n_predict))
        self.res[i] = [[], None, None, []]
        self.queue.append(i)
        return i

    def done(self, i):
        return self.res[i][1] is not None

    def decoding(self, i):
        return len(self.res[i][0]) > 0 and not self.done(i)

    def step(self):
        admitted = []
        while self.queue and None in self.slot:          # the model's admissions, one at a time over the records as they stand
            i = self.queue.pop(0)
            prompt = self.reqs[i][0].tolist()
            free = [int(x is None) for x in self.slot]
            if self.sharing:
                P, sl, donor, inplace = plan_prefix_ref(free, [h[:n] for h, n in self.held], prompt, self.chunk)
            else:
                P, sl, donor, inplace = 0, free.index(1), -1, 0
            state = None
            if donor >= 0:
                j = self.slot[donor]
                state = "finished" if j is None else "prefilling" if self.off[j] < len(self.reqs[j][0]) else "decoding"
                self.copied += P - inplace
                self.copies += 1
            self.log.append(dict(req=i, P=P, inplace=inplace, donor=donor, state=state, from_this_step=donor in admitted, step=self.steps))
            self.shared += P
            self.slot[sl], self.off[i], self.slot_of[i] = i, P, sl
            if self.sharing:
                self.held[sl] = (prompt, P)
            self.order.append(i)
            admitted.append(sl)
        left = [len(self.reqs[i][0]) - self.off[i] for i in self.order]
        rows = self.L.sched_plan(left, self.chunk, self.budget)[1].tolist() if left else []
        evs = self.sc.step()
        self.events.append(evs)
        self.steps += 1
        for i, l, r in zip(self.order, left, rows):
            if l > 0:
                self.off[i] += r
                if self.sharing:
                    self.held[self.slot_of[i]] = (self.held[self.slot_of[i]][0], self.off[i])
        for e in evs:
            i = self.ids[e["id"]]
            r = self.res[i]
            assert e["slot"] == self.slot_of[i], ("the model's slot", i, e, self.log)
            if e["kind"] == "token":
                r[0].append(e["token"])
                r[3].append(e["exact"])
                continue
            r[1] = e
            self.hm.set_seq(e["slot"])
            r[2] = [self.hm.kv(il, e["position"]) for il in range(self.hp.n_layer)]
            self.hm.set_seq(N_SEQ - 1)
            self.slot[e["slot"]] = None
            self.order.remove(i)
        assert self.steps < 3000

    def until(self, cond):
        while not cond():
            assert self.sc.pending() > 0, "nothing pending and the condition never held"
            self.step()

    def finish(self):
        self.until(lambda: self.sc.pending() == 0)
        st = self.sc.stats()
        self.sc.close()
        self.hm.set_seq(0)
        return st

    def check_stats(self, st, note):
        n_prompt = sum(len(p) for p, _ in self.reqs)
        assert st["n_prompt_rows"] + st["n_shared_rows"] == n_prompt, (note, st)
        assert st["n_shared_rows"] == self.shared and st["n_copied_rows"] == self.copied, (note, st, self.shared, self.copied, self.log)
        assert st["n_copy_launches"] % max(self.copies, 1) == 0 and (st["n_copy_launches"] > 0) == (self.copies > 0), (note, st, self.copies)
        assert st["n_submitted"] == st["n_done"] == len(self.reqs), (note, st)


def workload(hp):
    """a 40-token system prompt in front of distinct tails, an exact resubmission, the system prompt alone, a prompt no longer than one
    chunk, prompts with nothing in common; the contexts mostly descend, so later occupants sit under stale rows"""
    return [(with_prefix(hp, 300, 40, 301, 21), 6), (with_prefix(hp, 300, 40, 302, 9), 12), (with_prefix(hp, 300, 40, 303, 3), 4),
            (with_prefix(hp, 300, 40, 301, 21), 3), (with_prefix(hp, 300, 9, 0, 0), 5), (unrelated(hp, 305, 31), 7),
            (with_prefix(hp, 300, 40, 306, 30), 5), (unrelated(hp, 307, 10), 2), (with_prefix(hp, 300, 40, 0, 0), 8)]


def run_workload(L, hm, hp, reqs, chunk, budget, nth, samplers=None, **kw):
    run = Run(L, hm, hp, chunk, budget, nth, **kw)
    for i, (p, k) in enumerate(reqs):
        run.submit(p, k, sampler=None if samplers is None else samplers[i])
    return run, run.finish()


@pytest.mark.parametrize("chunk,budget,nth", [(9, 16, 8), (9, 1, 1), (9, 64, 3), (1, 16, 3), (1, 64, 8), (1, 1, 1)])
def test_every_request_is_the_request_alone_whatever_was_shared(L, pair, chunk, budget, nth):
    hp, _, hm, hl = pair
    reqs = workload(hp)
    note = (chunk, budget, nth)
    hm.set_seq(N_SEQ - 1)
    outside = [hm.kv(il, N_CTX) for il in range(hp.n_layer)]
    run, st = run_workload(L, hm, hp, reqs, chunk, budget, nth)
    hm.set_seq(N_SEQ - 1)
    for il in range(hp.n_layer):
        now = hm.kv(il, N_CTX)
        assert same(outside[il][0], now[0]) and same(outside[il][1], now[1]), (note, "a slot the scheduler does not own changed")
    hm.set_seq(0)
    check_against_alone(hl, hp, reqs, run.res, chunk, nth, {}, note)
    run.check_stats(st, note)
    assert st["n_shared_rows"] > 0 and st["n_fallback_steps"] == 0 and st["n_mixed_steps"] > 0, (note, st)
    assert st["n_copy_launches"] == run.copies, (note, st)          # a plain handle: one launch per copy
    # the exact resubmission shares everything but whole chunks below its last token; the one-chunk prompt nothing at chunk 9
    by_req = {a["req"]: a for a in run.log}
    assert by_req[3]["P"] == (len(reqs[3][0]) - 1) // chunk * chunk, (note, by_req[3])
    assert by_req[4]["P"] == (0 if chunk == 9 else 8) and by_req[5]["P"] == 0 and by_req[7]["P"] == 0, (note, by_req)


def test_chunk_0_shares_nothing_and_the_option_off_is_the_scheduler_as_it_was(L, pair):
    hp, _, hm, hl = pair
    reqs = workload(hp)
    off, st_off = run_workload(L, hm, hp, reqs, 9, 16, 8, share=False)
    check_against_alone(hl, hp, reqs, off.res, 9, 8, {}, "off")
    assert st_off["n_shared_rows"] == st_off["n_copied_rows"] == st_off["n_copy_launches"] == 0 and st_off["n_prompt_rows"] == sum(len(p) for p, _ in reqs)
    assert [a["P"] for a in off.log] == [0] * len(reqs)          # (the model without the option: lowest free slot first; Run.step checks every event's slot)
    # ... event for event what a scheduler made without naming the option makes
    plain = []
    with hm.scheduler(max_active=MAX_ACTIVE, chunk_tokens=9, row_budget=16, n_threads=8) as sc:
        for p, k in reqs:
            sc.submit(p, k)
        while sc.pending():
            plain.append(sc.step())
        st_plain = sc.stats()
    st_plain["n_graph_captures"] = st_off["n_graph_captures"]          # (the second run finds the first one's set-step graphs)
    assert plain == off.events and st_plain == st_off
    zero, st0 = run_workload(L, hm, hp, reqs, 0, 64, 8)          # chunk_tokens 0: every row's key count is its own prompt's length
    check_against_alone(hl, hp, reqs, zero.res, 0, 8, {}, "chunk 0")
    zero.check_stats(st0, "chunk 0")
    assert st0["n_shared_rows"] == st0["n_copied_rows"] == st0["n_copy_launches"] == 0


def test_donors_prefilling_decoding_finished_and_admitted_in_the_same_step(L, pair):
    """a staged run, chunks of 9, budget 16: every kind of donor, asserted from the model's admission log"""
    hp, _, hm, hl = pair
    run = Run(L, hm, hp, 9, 16, 8)
    # two unrelated prompts and a long-running request R with system prompt 300
    u1, u2 = run.submit(unrelated(hp, 310, 10), 2), run.submit(unrelated(hp, 311, 12), 2)
    r = run.submit(with_prefix(hp, 300, 40, 312, 21), 40)
    run.until(lambda: run.done(u1) and run.done(u2) and run.decoding(r))
    # two at once: the first copies from R, which decodes; the second from the first, whose rows an earlier launch of the same step copied
    s1, s2 = run.submit(with_prefix(hp, 300, 40, 313, 7), 3), run.submit(with_prefix(hp, 300, 40, 314, 12), 3)
    run.step()
    a1, a2 = run.log[-2], run.log[-1]
    assert (a1["req"], a1["P"], a1["inplace"], a1["state"], a1["from_this_step"]) == (s1, 36, 0, "decoding", False), a1
    assert (a2["req"], a2["P"], a2["inplace"], a2["state"], a2["from_this_step"]) == (s2, 36, 0, "prefilling", True), a2
    assert a1["step"] == a2["step"] and a2["donor"] == run.slot_of[s1]
    run.until(lambda: run.done(s1) and run.done(s2))
    # a finished donor, in place: its own slot is reused
    t = run.submit(with_prefix(hp, 300, 40, 315, 5), 2)
    run.step()
    assert (run.log[-1]["P"], run.log[-1]["inplace"], run.log[-1]["donor"]) == (36, 36, -1), run.log[-1]
    run.until(lambda: run.done(t) and run.done(r))
    # an exact resubmission of a finished prompt: everything but the chunk of its last token, in place in R's slot
    w = run.submit(run.reqs[r][0], 3)
    run.step()
    assert (run.log[-1]["P"], run.log[-1]["inplace"], run.slot_of[w]) == (54, 54, run.slot_of[r]), run.log[-1]
    run.until(lambda: run.done(w))
    # a donor that is still prefilling: what it has evaluated so far, whole chunks
    x = run.submit(with_prefix(hp, 320, 40, 321, 30), 2)
    run.step()
    run.step()
    assert run.off[x] == 18
    y = run.submit(with_prefix(hp, 320, 40, 322, 4), 2)
    run.step()
    assert (run.log[-1]["P"], run.log[-1]["inplace"], run.log[-1]["state"]) == (18, 0, "prefilling"), run.log[-1]
    run.until(lambda: run.done(x) and run.done(y))
    # a finished donor's rows copied into another slot.  An unrelated request first takes y's slot (the smallest record), so that only x's
    # slot holds system prompt 320; of two admitted at once the first then takes x's slot in place and the second copies x's rows from there
    f = run.submit(unrelated(hp, 325, 10), 2)
    run.until(lambda: run.done(f))
    assert run.slot_of[f] == run.slot_of[y]
    z1, z2 = run.submit(with_prefix(hp, 320, 40, 323, 6), 2), run.submit(with_prefix(hp, 320, 40, 324, 8), 2)
    run.step()
    b1, b2 = run.log[-2], run.log[-1]
    assert (b1["P"], b1["inplace"], b1["donor"], run.slot_of[z1]) == (36, 36, -1, run.slot_of[x]), b1
    assert (b2["P"], b2["inplace"], b2["donor"], b2["from_this_step"]) == (36, 0, run.slot_of[z1], True), b2
    st = run.finish()
    check_against_alone(hl, hp, run.reqs, run.res, 9, 8, {}, "staged")
    run.check_stats(st, "staged")
    assert {a["state"] for a in run.log} >= {"decoding", "prefilling"} and any(a["from_this_step"] for a in run.log)
    assert any(a["inplace"] > 0 and a["donor"] < 0 for a in run.log) and st["n_copied_rows"] > 0


def test_drafted_tokens_leave_stale_rows_above_the_donors_contexts(L, pair):
    """draft_len 15 with a corpus every draft comes from: verify steps write rows above the contexts of requests that are donors"""
    hp, _, hm, hl = pair
    reqs = workload(hp)
    streams = [alone(hl, hp, 0, p, k, 9, 8)[0] for p, k in reqs]
    corpus = np.concatenate([np.concatenate([p[-3:], np.asarray(s, np.int32)]) for (p, _), s in zip(reqs, streams)])
    run, st = run_workload(L, hm, hp, reqs, 9, 16, 8, draft_len=15, corpus=corpus)
    check_against_alone(hl, hp, reqs, run.res, 9, 8, {}, "drafts")
    run.check_stats(st, "drafts")
    assert st["n_shared_rows"] > 0 and st["n_drafted"] > 0 and st["n_accepted"] > 0 and st["n_draft_steps"] > 0, st


def test_sampled_requests_draw_what_they_draw_alone(L, pair):
    hp, _, hm, hl = pair
    reqs = workload(hp)
    sampled = [True, False, True, True, False, True, False, True, True]
    rln = (64, 0, 8, 0, 0, 64, 0, 200, 16)
    samplers = []
    for i, (p, _) in enumerate(reqs):
        s = L.Sampler(seed=3300 + 7 * i, repeat_last_n=rln[i]) if sampled[i] else None
        for t in (p if s is not None else ()):
            s.accept(int(t))
        samplers.append(s)
    run, st = run_workload(L, hm, hp, reqs, 9, 16, 8, samplers=samplers)
    run.check_stats(st, "sampled")
    assert st["n_shared_rows"] > 0 and st["n_fallback_steps"] == 0
    for i, (p, k) in enumerate(reqs):
        toks, ev, kv, exact = run.res[i]
        if not sampled[i]:
            want, want_kv = alone(hl, hp, ev["slot"], p, k, 9, 8)
        else:
            want, want_kv, ws = _sampled_alone(L, hl, hp, ev["slot"], p, k, 3300 + 7 * i, rln[i], 9, 8)
            assert samplers[i].window().tolist() == ws.window().tolist(), (i, "sampler window")
            lg = np.linspace(-1, 1, hp.n_vocab).astype(np.float32)          # the rng's next draw, on a fixed row
            assert samplers[i].sample(hm, lg) == ws.sample(hl, lg), (i, "rng state")
        assert toks == want and ev["reason"] == "length", (i, toks, want)
        for il in range(hp.n_layer):
            assert same(kv[il][0], want_kv[il][0]) and same(kv[il][1], want_kv[il][1]), (i, il)


@pytest.mark.parametrize("kind", ["pipe2", "unfused", "f16", "fast_prefill"])
def test_handles(L, tmp_path, kind):
    """a two-stage pipeline copies on every stage; LLAMAHIP_FLAG_UNFUSED handles and f16 files share through their per-slot calls (fall-back
    steps); a LLAMAHIP_FLAG_FAST_PREFILL handle shares nothing and reports zeros (yardstick: a handle with the same flag)"""
    hp = hparams(4, n_layer=3 if kind == "pipe2" else 2)
    path = _file(L, tmp_path, "f16" if kind == "f16" else "q40", hp, 271)
    opts = dict(pipe2=dict(devices=[0, 0]), unfused=dict(flags=UNFUSED), fast_prefill=dict(flags=FAST_PREFILL)).get(kind, {})
    reqs = workload(hp)
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, **opts) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, **(opts if kind == "fast_prefill" else {})) as hl:
        run, st = run_workload(L, hm, hp, reqs, 9, 16, 8, handle_shares=kind != "fast_prefill")
        check_against_alone(hl, hp, reqs, run.res, 9, 8, {}, kind)
        run.check_stats(st, kind)
        if kind == "fast_prefill":
            assert st["n_shared_rows"] == st["n_copied_rows"] == st["n_copy_launches"] == 0, st
            return
        assert st["n_shared_rows"] > 0 and st["n_copied_rows"] > 0, (kind, st)
        assert st["n_copy_launches"] == run.copies * (2 if kind == "pipe2" else 1), (kind, st)          # one launch per stage and copy
        if kind == "pipe2":
            assert st["n_fallback_steps"] == 0 and st["n_mixed_steps"] > 0, st
        else:
            assert st["n_fallback_steps"] == st["n_steps"] > 0, st
