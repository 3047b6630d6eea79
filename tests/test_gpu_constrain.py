"""GPU (-m gpu): llamahip_decode_greedy_constrained against its contract -- the loop "one-token eval -> pick -> advance" on a SECOND handle, with
tests/dfa_ref.py's pick on the table dfa_ref lifted: tokens, n_out, finished, the state, logits_last and the KV rows [0, n_past + n_out) of
every layer, bit for bit.  Tiny synthetic files (n_vocab 300, n_embd 256, 2 layers, n_ctx 64): Q4_0, f16, Q4_1; NO_GRAPH, UNFUSED and two-stage
pipeline handles.  Constraints: regular expressions over the synthetic vocabulary (a short answer inside two legs, and one of five legs and a part) and a set of
choices.  Resuming from a returned state equals one call; the all-allowed constraint gives decode_greedy's tokens; a finished answer's bytes
re.fullmatch the pattern while the same model's unconstrained greedy stream does not satisfy the constraint; n_steps shorter than the answer
and no multiple of the leg; live allocations come back after constraint_free and model_free.  llamahip_decode_greedy_constrained_multi with 2, 5
and 16 sequences under mixed constraints, start states and positions: per sequence the single call on a second handle, KV rows included.
Model.decode_sample_constrained against eval -> mask_row -> the reference sampler -> accept on a second handle: tokens, the sampler's window
and its rng state, with more than top_k tokens allowed (candidates from the device) and fewer (every step ties at -inf: exact = 0)."""
import os
import re

import numpy as np
import pytest

import dfa_ref
import synth

pytestmark = pytest.mark.gpu
HP = synth.HParams(n_vocab=300, n_embd=256, n_mult=64, n_head=4, n_layer=2)
VOCAB = synth.make_vocab(HP.n_vocab)
N_CTX, STOP, LEG = 64, 2, 4
NO_GRAPH, UNFUSED = 1, 2
SHORT = "(ab|ba){1,3} tok0003[0-9]"           # 5 .. 9 tokens with the stop token
LONG = "[a-e]{20}"                            # 21 tokens: five legs, the stop token at the head of the sixth (the leg runs past it)
CHOICES = [b"cab", b"cabbage", b"tok00100", b"d tok00200 e"]
PROMPT = synth.synth_prompt(6, HP.n_vocab, seed=5)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def write_file(L, tmp_path, kind):
    path = str(tmp_path / f"cst_{kind}.bin")
    if kind == "q4_0":
        synth.write_model(path, HP, synth.random_tensors(HP, seed=41))
        return path
    src = path + ".f16" if kind == "q4_1" else path
    synth.write_model_unquantized(src, HP, synth.random_tensors(HP, seed=41), 1)
    if kind == "q4_1":
        L.quantize_file(src, path, 3)
        os.remove(src)
    return path


def byte_dfa(spec):
    from llama_swift_amd import regex_dfa
    return dfa_ref.trie(spec) if isinstance(spec, list) else regex_dfa.compile(spec)


def accepts(spec, data):
    return data in spec if isinstance(spec, list) else re.fullmatch(spec.encode(), data) is not None


def reference(ref, table, state, first_token, n_past, n_steps):
    """the contract on the second handle: (tokens, finished, state, the logits the last token was picked from)"""
    done, tok, out, row = table.shape[0] - 1, first_token, [], None
    while len(out) < n_steps and state != done:
        row = ref.eval([tok], n_past + len(out))
        tok = dfa_ref.pick(table[state], row)
        assert tok >= 0
        state = int(table[state][tok])
        out.append(tok)
    return np.array(out, np.int32), state == done, state, row


def check(m, ref, c, table, n_steps, state=None, first_token=None, n_past=None, want_kv=True):
    first_token = int(PROMPT[-1]) if first_token is None else first_token
    n_past = PROMPT.size - 1 if n_past is None else n_past
    if n_past == PROMPT.size - 1:
        m.eval(PROMPT[:-1], 0), ref.eval(PROMPT[:-1], 0)
    s0 = c.start if state is None else state
    want = reference(ref, table, s0, first_token, n_past, n_steps)
    got = m.decode_greedy_constrained(first_token, n_past, n_steps, c, state=state, want_logits=True)
    assert got["tokens"].tolist() == want[0].tolist() and got["finished"] == want[1] and got["state"] == want[2], (got, want)
    assert same(got["logits"], want[3])
    if want_kv:
        for il in range(HP.n_layer):
            k, v = m.kv(il, n_past + want[0].size)
            rk, rv = ref.kv(il, n_past + want[0].size)
            assert same(k, rk) and same(v, rv), il
    return got


def run_handle(L, m, ref):
    for spec in (SHORT, CHOICES, LONG):
        tr, ac, st = byte_dfa(spec)
        table = dfa_ref.lift(VOCAB, tr, ac, st, STOP)
        with (m.constraint(choices=spec) if isinstance(spec, list) else m.constraint(regex=spec)) as c:
            assert c.table().tobytes() == table.tobytes()
            n_steps = 37 if spec == LONG else 12                  # 37: no multiple of the leg
            full = check(m, ref, c, table, n_steps)
            assert full["finished"] and full["tokens"][-1] == STOP and full["state"] == c.done
            assert (spec != LONG) or (LEG < full["tokens"].size and full["tokens"].size % LEG != 0)
            text = dfa_ref.decode(table, full["tokens"][:-1], VOCAB)
            assert accepts(spec, text), text
            # the constraint acts: the same model's unconstrained greedy stream does not satisfy it -- at no length
            m.eval(PROMPT[:-1], 0)
            free = m.decode_greedy(int(PROMPT[-1]), PROMPT.size - 1, n_steps)
            assert not any(accepts(spec, dfa_ref.decode(table, free[:n], VOCAB)) for n in range(n_steps + 1))
            # n_steps shorter than the answer, then resumed from the returned state: one call's tokens
            cut = 1 if spec != LONG else LEG + 3
            head = check(m, ref, c, table, cut)
            assert not head["finished"] and head["tokens"].size == cut and head["tokens"].tolist() == full["tokens"][:cut].tolist()
            tail = check(m, ref, c, table, n_steps - cut, state=head["state"], first_token=int(head["tokens"][-1]), n_past=PROMPT.size - 1 + cut)
            assert tail["finished"] and np.concatenate([head["tokens"], tail["tokens"]]).tolist() == full["tokens"].tolist()
            # a state that comes in as DONE: the stop token once
            again = m.decode_greedy_constrained(STOP, PROMPT.size - 1 + full["tokens"].size, 3, c, state=c.done)
            assert again["tokens"].tolist() == [STOP] and again["finished"] and again["state"] == c.done


@pytest.fixture(scope="module")
def q4_path(L, tmp_path_factory):
    return write_file(L, tmp_path_factory.mktemp("cst"), "q4_0")


def test_plain_handle_and_live_allocations(L, q4_path):
    before = L.live_allocs()
    with L.Model(q4_path, n_ctx=N_CTX) as m, L.Model(q4_path, n_ctx=N_CTX) as ref:
        run_handle(L, m, ref)
        loaded = L.live_allocs()
        c = m.constraint(regex=SHORT)
        assert L.live_allocs() == loaded                          # the device copy is made by the first device call that uses it
        m.eval(PROMPT[:-1], 0)
        m.decode_greedy_constrained(int(PROMPT[-1]), PROMPT.size - 1, 12, c)
        assert L.live_allocs() == (loaded[0] + 1, loaded[1] + 2 * c.n_states * HP.n_vocab)
        c.close()
        assert L.live_allocs() == loaded
        left = m.constraint(choices=CHOICES)                      # one the model outlives by mistake: freed afterwards, nothing touched
        m.decode_greedy_constrained(int(PROMPT[-1]), PROMPT.size - 1, 12, left)
    assert L.live_allocs() == before
    left.close()
    assert L.live_allocs() == before


def test_the_all_allowed_constraint_is_decode_greedy(L, q4_path):
    trans, accept = np.zeros((1, 256), np.int32), np.ones(1, np.uint8)
    with L.Model(q4_path, n_ctx=N_CTX) as m, L.Model(q4_path, n_ctx=N_CTX) as ref, m.constraint(dfa=(trans, accept, 0)) as c:
        t = c.table()
        assert (t[0, 3:] == 0).all() and t[0, :3].tolist() == [dfa_ref.BANNED, dfa_ref.BANNED, 1]      # everything with a text, and the stop token
        ref.eval(PROMPT[:-1], 0)
        free = ref.decode_greedy(int(PROMPT[-1]), PROMPT.size - 1, 40)
        assert free.min() >= 3                                    # (no empty-text token in the free stream: nothing for the constraint to ban)
        m.eval(PROMPT[:-1], 0)
        got = m.decode_greedy_constrained(int(PROMPT[-1]), PROMPT.size - 1, 40, c)
        assert got["tokens"].tolist() == free.tolist() and not got["finished"] and got["state"] == 0
        # decode_greedy's own captured steps are not disturbed by the constrained ones on the same handle, and the other way round
        m.eval(PROMPT[:-1], 0)
        assert m.decode_greedy(int(PROMPT[-1]), PROMPT.size - 1, 40).tolist() == free.tolist()
        m.eval(PROMPT[:-1], 0)
        assert m.decode_greedy_constrained(int(PROMPT[-1]), PROMPT.size - 1, 40, c)["tokens"].tolist() == free.tolist()


@pytest.mark.parametrize("kind", ["no_graph", "unfused", "pipe2", "f16", "q4_1"])
def test_other_handles(L, tmp_path, q4_path, kind):
    path = q4_path if kind in ("no_graph", "pipe2", "unfused") else write_file(L, tmp_path, kind)
    kw = {"no_graph": dict(flags=NO_GRAPH), "unfused": dict(flags=UNFUSED), "pipe2": dict(devices=[0, 0])}.get(kind, {})
    with L.Model(path, n_ctx=N_CTX, **kw) as m, L.Model(path, n_ctx=N_CTX) as ref:
        run_handle(L, m, ref)


def test_two_constraints_alternate_on_one_handle(L, q4_path):
    """each constraint's captured step holds its own table: alternating them, and freeing one, leaves the other's answers as they were"""
    with L.Model(q4_path, n_ctx=N_CTX) as m, L.Model(q4_path, n_ctx=N_CTX) as ref:
        a, b = m.constraint(regex=SHORT), m.constraint(choices=CHOICES)
        ta, tb = a.table(), b.table()
        first = [check(m, ref, c, t, 12, want_kv=False)["tokens"].tolist() for c, t in ((a, ta), (b, tb), (a, ta), (b, tb))]
        assert first[0] == first[2] and first[1] == first[3] and first[0] != first[1]
        a.close()
        assert check(m, ref, b, tb, 12)["tokens"].tolist() == first[1]
        b.close()


SPECS = (SHORT, CHOICES, LONG, "[a-z ]{1,30}")


def setup_multi(m, n):
    """slot i: its own prompt length (3 .. 6 rows evaluated), constraint, and -- every third sequence -- a start state one token into the answer"""
    cs = [m.constraint(choices=sp) if isinstance(sp, list) else m.constraint(regex=sp) for sp in SPECS]
    seqs = []
    for i in range(n):
        prompt = synth.synth_prompt(4 + i % 4, HP.n_vocab, seed=20 + i)
        c = cs[i % len(SPECS)]
        first, state = int(prompt[-1]), c.start
        if i % 3 == 2:                                   # resumed: the answer's first token is taken as given
            first = int(np.flatnonzero((c.table()[c.start] != dfa_ref.BANNED))[i % 2])
            state = c.advance(c.start, first)
            assert state >= 0 and state != c.done
        m.set_seq(i)
        m.eval(prompt[:-1], 0)
        seqs.append((c, first, prompt.size - 1, state))
    m.set_seq(0)
    return cs, seqs


def check_multi(L, m, ref, n, n_steps=24):
    cs, seqs = setup_multi(m, n)
    rcs, rseqs = setup_multi(ref, n)
    got = m.decode_greedy_constrained_multi([q[1] for q in seqs], [q[2] for q in seqs], n_steps, [q[0] for q in seqs], states=[q[3] for q in seqs])
    assert m.cur_seq == 0 and len(got) == n
    n_fin = 0
    for i, (c, first, n_past, state) in enumerate(rseqs):
        ref.set_seq(i)
        want = ref.decode_greedy_constrained(first, n_past, n_steps, c, state=state)
        g = got[i]
        assert g["tokens"].tolist() == want["tokens"].tolist() and g["finished"] == want["finished"] and g["state"] == want["state"], (i, g, want)
        n_fin += g["finished"]
        m.set_seq(i)
        for il in range(HP.n_layer):
            k, v = m.kv(il, n_past + g["tokens"].size)
            rk, rv = ref.kv(il, n_past + g["tokens"].size)
            assert same(k, rk) and same(v, rv), (i, il)
    m.set_seq(0), ref.set_seq(0)
    if n_steps >= 24:      # mixed answers, and the bounded ones finished
        assert n_fin >= min(n, 3) - 1 and len({tuple(g["tokens"].tolist()) for g in got}) >= min(n, 3)
    for c in cs + rcs:
        c.close()


@pytest.mark.parametrize("n", [2, 5, 16])
def test_multi_on_a_plain_handle(L, q4_path, n):
    with L.Model(q4_path, n_ctx=N_CTX, n_seq=16) as m, L.Model(q4_path, n_ctx=N_CTX, n_seq=16) as ref:
        check_multi(L, m, ref, n)
        check_multi(L, m, ref, n, n_steps=3)             # shorter than every answer, and than a leg


@pytest.mark.parametrize("kind", ["no_graph", "unfused", "pipe2", "f16", "q4_1"])
def test_multi_on_other_handles(L, tmp_path, q4_path, kind):
    path = q4_path if kind in ("no_graph", "pipe2", "unfused") else write_file(L, tmp_path, kind)
    kw = {"no_graph": dict(flags=NO_GRAPH), "unfused": dict(flags=UNFUSED), "pipe2": dict(devices=[0, 0])}.get(kind, {})
    with L.Model(path, n_ctx=N_CTX, n_seq=4, **kw) as m, L.Model(path, n_ctx=N_CTX, n_seq=4) as ref:
        check_multi(L, m, ref, 3)


def sampled_reference(L, ref, c, sampler, first_token, n_past, n_steps, **kw):
    """eval -> llamahip_constraint_mask_row -> llamahip_sample_top_p_top_k -> accept, on the second handle"""
    tok, state, out = first_token, c.start, []
    while len(out) < n_steps and state != c.done:
        row = ref.eval([tok], n_past + len(out))
        tok = sampler.sample(ref, c.mask_row(state, row), **kw)
        sampler.accept(tok)
        state = c.advance(state, tok)
        assert state >= 0
        out.append(tok)
    return out, state


@pytest.mark.parametrize("kind", ["plain", "pipe2"])
def test_the_sampled_loop_is_the_host_masked_sampler(L, q4_path, kind):
    kw = dict(devices=[0, 0]) if kind == "pipe2" else {}
    with L.Model(q4_path, n_ctx=N_CTX, **kw) as m, L.Model(q4_path, n_ctx=N_CTX) as ref:
        # more than top_k tokens allowed (27 letters and the space, top_k 8), and fewer (at most 13 with top_k 40: every step ties at -inf)
        for spec, top_k, n_steps in (("[a-z ]{1,30}", 8, 24), (SHORT, 40, 12), ("[a-z ]{1,30}", 40, 10)):
            par = dict(repeat_penalty=1.3, top_k=top_k, top_p=float(np.float32(0.95)), temp=float(np.float32(0.8)))
            with m.constraint(regex=spec) as c, ref.constraint(regex=spec) as cr:
                s1, s2 = L.Sampler(seed=77, repeat_last_n=16), L.Sampler(seed=77, repeat_last_n=16)
                m.eval(PROMPT[:-1], 0), ref.eval(PROMPT[:-1], 0)
                want, wstate = sampled_reference(L, ref, cr, s2, int(PROMPT[-1]), PROMPT.size - 1, n_steps, **par)
                got = m.decode_sample_constrained(int(PROMPT[-1]), PROMPT.size - 1, n_steps, c, s1, **par)
                assert got["tokens"].tolist() == want and got["state"] == wstate and got["finished"] == (wstate == c.done), (spec, top_k, got, want)
                assert s1.window().tolist() == s2.window().tolist()
                sc, ids = -np.arange(8, dtype=np.float64), np.arange(10, 18, dtype=np.int32)      # the rng state: the same draws from here on
                assert [s1.sample_from_candidates(sc, ids) for _ in range(6)] == [s2.sample_from_candidates(sc, ids) for _ in range(6)]
                n = got["tokens"].size
                if kind == "pipe2" or top_k == 40:
                    assert got["n_exact"] == 0           # fewer than top_k + 1 allowed: -inf ties at the k-th place; a pipeline handle masks on the host
                else:
                    assert got["n_exact"] >= n // 2, got  # the candidates came from the device on most steps
                # one step's candidates against the masked row directly: exact == 1 means the k best of the masked, penalised row
                if kind == "plain" and top_k == 8:
                    s3 = L.Sampler(seed=1, repeat_last_n=16)
                    exact, csc, cid, _ = m.eval_topk_constrained([int(PROMPT[-1])], PROMPT.size - 1, s3, c, c.start, top_k=8)
                    row = cr.mask_row(cr.start, ref.eval([int(PROMPT[-1])], PROMPT.size - 1)).astype(np.float64) * (1.0 / float(np.float32(0.8)))
                    order = np.argsort(-row, kind="stable")[:8]
                    assert exact and cid.tolist() == order.tolist() and csc.tobytes() == row[order].tobytes()


def test_refusals_on_a_device_handle(L, q4_path):
    with L.Model(q4_path, n_ctx=N_CTX) as m, L.Model(q4_path, n_ctx=N_CTX, layer_begin=0, layer_end=1) as stage:
        with m.constraint(regex=SHORT) as c, stage.constraint(regex=SHORT) as cs:
            with pytest.raises(L.LlamaHipError, match=r"llamahip_decode_greedy_constrained: context overflow: n_past \(60\) \+ n_steps \(5\) > n_ctx \(64\)"):
                m.decode_greedy_constrained(3, 60, 5, c)
            with pytest.raises(L.LlamaHipError, match="llamahip_decode_greedy_constrained: the constraint was made on another handle"):
                m.decode_greedy_constrained(3, 0, 5, cs)
            with pytest.raises(L.LlamaHipError, match="llamahip_decode_greedy_constrained: needs a whole-model handle"):
                stage.decode_greedy_constrained(3, 0, 5, cs)
