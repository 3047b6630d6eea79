"""GPU (-m gpu): llamahip_beam_search against its contract in plain Python (tests/beam_ref.py).

The expected result comes from beam_ref.search on a SECOND handle: for every hypothesis that handle runs eval_chunks(prompt) plus single-token
evals of the hypothesis' tokens on a slot of its own, with llamahip_op_top_logprobs for the candidates of the row it ends with.  Tokens, length,
reason and the score's bytes must be identical; for every LENGTH hypothesis the KV rows of its slot, in every layer, are the second handle's.
Every case asserts the conditions that make it a test from the reference run: a copy was made, a parent ended a step without a child, a stop
case produced a STOP hypothesis, and neighbouring candidates of every walk (and neighbouring keys of the ranking) differ by more than 1e-6."""
import os
import struct

import numpy as np
import pytest

import beam_ref
import synth

pytestmark = pytest.mark.gpu
HP = synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=4, n_layer=2)
N_CTX, N_PREDICT, N_SEQ = 64, 12, 16
NO_GRAPH, UNFUSED = 1, 2


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def write_file(L, tmp_path, kind):
    path = str(tmp_path / f"beam_{kind}.bin")
    if kind == "q4_0":
        synth.write_model(path, HP, synth.random_tensors(HP, seed=beam_ref.MODEL_SEED))
        return path
    src = path + ".f16" if kind == "q4_1" else path
    synth.write_model_unquantized(src, HP, synth.random_tensors(HP, seed=beam_ref.MODEL_SEED), 1)
    if kind == "q4_1":
        L.quantize_file(src, path, 3)
        os.remove(src)
    return path


class Rows:
    """the second handle: the contract's rows, one hypothesis at a time on its slot 0"""

    def __init__(self, L, ref, prompt, chunk, n_cand):
        self.L, self.ref, self.prompt, self.chunk, self.n_cand, self.memo = L, ref, prompt, chunk, n_cand, {}

    def run(self, tokens):
        """eval_chunks(prompt) + single-token evals of `tokens`: the last row of logits"""
        p = self.prompt
        row = self.ref.eval_chunks(p, 0, chunk_tokens=self.chunk) if self.chunk else self.ref.eval(p, 0)
        for j, t in enumerate(tokens):
            row = self.ref.eval([t], p.size + j)
        return row

    def cands_of(self, tokens):
        if tokens not in self.memo:
            ids, lp = self.L.op_top_logprobs(self.run(tokens), self.n_cand)
            self.memo[tokens] = (ids[0], lp[0])
        return self.memo[tokens]


def check_case(L, m, ref, n_beams, n_prompt, chunk, stop=False, n_return=0, length_norm=False, seed=0, fallback=False, n_stages=1):
    prompt = synth.synth_prompt(n_prompt, HP.n_vocab, seed=beam_ref.PROMPT_SEED + seed)
    rows = Rows(L, ref, prompt, chunk, 2 * n_beams)
    stop_token = -1
    if stop:
        free, _ = beam_ref.search(rows.cands_of, n_prompt, n_beams, N_PREDICT)
        stop_token = int(free[1]["tokens"][beam_ref.STOP_AT])      # a token of the second-ranked hypothesis of the stop-less run
    want, info = beam_ref.search(rows.cands_of, n_prompt, n_beams, N_PREDICT, stop_token, n_return, length_norm)
    tag = (n_beams, n_prompt, chunk, stop_token, n_return, length_norm)
    # ---- the case's own conditions, from the reference run
    assert info["min_gap"] > 1e-6, (tag, info["min_gap"])
    if n_beams >= 2:
        assert info["n_copies"] >= 1, tag
    if n_beams >= 3:
        assert info["childless"], tag
    if stop:
        assert info["n_stop"] >= 1 and any(h["reason"] == "stop" for h in want), tag
    # ---- the search
    before = m.cur_seq
    got, st = m.beam_search(prompt, n_beams, N_PREDICT, stop_token=stop_token, n_return=n_return, length_norm=length_norm, chunk_tokens=chunk, with_stats=True)
    assert m.cur_seq == before
    assert len(got) == len(want), (tag, len(got), len(want))
    for g, w in zip(got, want):
        assert np.array_equal(g["tokens"], w["tokens"]) and g["length"] == w["length"] and g["reason"] == w["reason"], (tag, g, w)
        assert struct.pack("d", g["score"]) == struct.pack("d", w["score"]), (tag, g["score"], w["score"])
        assert g["slot"] == w["slot"], (tag, g, w)
    # ---- the stats identities
    assert st["n_steps"] == info["n_steps"] and st["n_rows"] == info["n_rows"] == sum(len(s) for s in info["live_sets"]), (tag, st)
    assert st["n_copied_rows"] == info["n_copied_rows"] and st["n_stop"] == info["n_stop"] and st["n_dead"] == 0, (tag, st)
    assert st["n_copy_launches"] % n_stages == 0 and (st["n_copy_launches"] > 0) == (info["n_copies"] > 0), (tag, st)
    if fallback:
        assert st["n_fallback_steps"] == info["n_rows"] and st["n_set_steps"] == 0, (tag, st)
    else:
        assert st["n_fallback_steps"] == 0 and st["n_set_steps"] == info["n_steps"], (tag, st)
    # ---- a LENGTH hypothesis' slot holds its rows: prompt + all its tokens but the last
    for g in got:
        if g["reason"] != "length":
            continue
        n = n_prompt + g["length"] - 1
        rows.run(tuple(int(t) for t in g["tokens"][:-1]))
        m.set_seq(g["slot"])
        for il in range(HP.n_layer):
            k, v = m.kv(il, n)
            rk, rv = ref.kv(il, n)
            assert same(k, rk) and same(v, rv), (tag, g["slot"], il)
        m.set_seq(before)
    return got, want, info


CASES = beam_ref.CASES


@pytest.fixture(scope="module")
def q4_path(L, tmp_path_factory):
    return write_file(L, tmp_path_factory.mktemp("beam"), "q4_0")


@pytest.fixture(scope="module")
def plain(L, q4_path):
    with L.Model(q4_path, n_ctx=N_CTX, n_seq=N_SEQ) as m, L.Model(q4_path, n_ctx=N_CTX) as ref:
        yield m, ref


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(int(x)) for x in c))
def test_plain_handle(L, plain, case):
    m, ref = plain
    n_beams, n_prompt, chunk, stop, n_return, length_norm = case
    check_case(L, m, ref, n_beams, n_prompt, chunk, bool(stop), n_return, bool(length_norm))


def test_one_beam_is_the_greedy_decode(L, plain):
    m, ref = plain
    prompt = synth.synth_prompt(9, HP.n_vocab, seed=beam_ref.PROMPT_SEED)
    got = m.beam_search(prompt, 1, N_PREDICT)
    assert len(got) == 1 and got[0]["reason"] == "length" and got[0]["length"] == N_PREDICT and got[0]["slot"] == 0
    first = int(np.argmax(ref.eval(prompt, 0)))
    rest = ref.decode_greedy(first, 9, N_PREDICT - 1)
    assert np.array_equal(got[0]["tokens"], np.concatenate([[first], rest]))


@pytest.mark.parametrize("kind", ["no_graph", "pipe2", "f16", "q4_1", "unfused"])
def test_other_handles(L, tmp_path, q4_path, kind):
    path = q4_path if kind in ("no_graph", "pipe2", "unfused") else write_file(L, tmp_path, kind)
    kw = {"no_graph": dict(flags=NO_GRAPH), "unfused": dict(flags=UNFUSED), "pipe2": dict(devices=[0, 0])}.get(kind, {})
    fallback = kind in ("q4_1", "unfused")
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, **kw) as m, L.Model(path, n_ctx=N_CTX) as ref:
        # (the Q4_1 file's rows are not the Q4_0 file's: its own prompt seed, with which the stop-less case meets its conditions; the stop case of the
        #  per-beam eval loop runs on the unfused handle)
        for n_beams, n_prompt, chunk, stop, n_return, length_norm in beam_ref.HANDLE_CASES[:1 if kind == "q4_1" else None]:
            check_case(L, m, ref, n_beams, n_prompt, chunk, bool(stop), n_return, bool(length_norm), seed=1 if kind == "q4_1" else 0, fallback=fallback,
                       n_stages=2 if kind == "pipe2" else 1)


def test_refusals_on_a_device_handle(L, plain):
    m, _ = plain
    prompt = synth.synth_prompt(9, HP.n_vocab, seed=1)
    with pytest.raises(L.LlamaHipError, match=r"llamahip_beam_search: context overflow: n_prompt \(9\) \+ n_predict \(56\) > n_ctx \(64\)"):
        m.beam_search(prompt, 2, 56)
    with m.scheduler(2, chunk_tokens=9):
        with pytest.raises(L.LlamaHipError, match="llamahip_beam_search: the handle has a live scheduler"):
            m.beam_search(prompt, 2, 4)
