"""GPU (-m gpu): sampled decoding of several sequences at once (llamahip_decode_sample_multi) and the batched device half of the sampler
(llamahip_op_topk_rows, kernels k_topk_keys_rows / k_topk_select_rows / k_topk_spill).

Every sequence must draw, bit for bit, what the single-sequence route draws for it: stepping the oracle one token at a time and drawing with
a fresh Sampler of the same seed on the oracle's logits (llama_sample_top_p_top_k), and the documented eval_topk + sample_from_candidates /
sample + accept loop on that slot alone -- on plain handles (one group, two groups, per-slot steps), pipeline handles, handles with no set
step, and with the device selection off (top_k > 64, a window longer than 1024 ids)."""
import numpy as np
import pytest

import synth
from conftest import synth_tool

pytestmark = pytest.mark.gpu
SMALL = dict(n_vocab=2000, n_embd=512, n_mult=256, n_head=4, n_layer=3)
W7B = dict(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=2)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ op_topk_rows against op_topk
def _rows(rng, R, V):
    """R rows of logits and windows: plain, tie-heavy (quarter steps, half of them with a little noise), a NaN row and a +inf row (R > 1);
    window lengths 0 / 64 / 1024 in turn"""
    lg = np.empty((R, V), np.float32)
    wins = []
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
        wins.append(rng.integers(0, V, (0, 64, 1024)[r % 3]).astype(np.int32))
    return lg, wins


@pytest.mark.parametrize("V", [1200, 32000, 32768])
@pytest.mark.parametrize("R", [1, 5, 16, 33])
def test_op_topk_rows_is_op_topk_row_by_row(L, R, V):
    rng = np.random.default_rng(R * 100003 + V)
    lg, wins = _rows(rng, R, V)
    for k in (1, 40, 64):
        exact, sc, ids, spill = L.op_topk_rows(lg, wins, top_k=k, want_spill=True)
        assert sc.shape == (R, k) and ids.shape == (R, k)
        for r in range(R):
            e1, s1, i1 = L.op_topk(lg[r], wins[r], top_k=k)
            assert exact[r] == e1, (R, V, k, r)
            assert same(sc[r], s1) and same(ids[r], i1), (R, V, k, r)
            # the spill rule: exactly the rows reported inexact are copied out, bit for bit
            if e1:
                assert np.isnan(spill[r]).all(), (R, V, k, r)
            else:
                assert same(spill[r], lg[r]), (R, V, k, r)
        if R >= 5:
            assert exact.any() and not exact.all(), (R, V, k, exact)


def test_op_topk_rows_window_longer_than_the_device_takes(L):
    """a row whose window holds more than 1024 ids is reported inexact and spilled; its neighbours are unaffected"""
    rng = np.random.default_rng(5)
    lg = (rng.standard_normal((3, 32000)) * 3).astype(np.float32)
    wins = [rng.integers(0, 32000, 64), rng.integers(0, 32000, 1025), rng.integers(0, 32000, 1024)]
    exact, sc, ids, spill = L.op_topk_rows(lg, wins, top_k=40, want_spill=True)
    assert exact.tolist() == [True, False, True]
    assert same(spill[1], lg[1]) and np.isnan(spill[0]).all() and np.isnan(spill[2]).all()
    for r in (0, 2):
        e1, s1, i1 = L.op_topk(lg[r], wins[r], top_k=40)
        assert e1 and same(sc[r], s1) and same(ids[r], i1)


# ------------------------------------------------------------------------------------------------ decode_sample_multi
def _prompts(S, V):
    return [synth.synth_prompt(3 + (5 * i) % 23, V, seed=70 + i) for i in range(S)]


def _rln(i):
    return (64, 8, 0, 64, 200)[i % 5]


def _prefill(L, h, prompts, seeds, nth, top_k=40):
    """evaluate every slot's prompt, give each slot a fresh sampler that has accepted its prompt, draw its first token from the prompt's logits"""
    samplers, firsts = [], []
    for i, p in enumerate(prompts):
        h.set_seq(i)
        lg = h.eval(p, 0, nth)
        s = L.Sampler(seed=seeds[i], repeat_last_n=_rln(i))
        for t in p:
            s.accept(int(t))
        firsts.append(s.sample(h, lg, top_k=top_k))
        s.accept(firsts[-1])
        samplers.append(s)
    h.set_seq(0)
    return samplers, firsts


def _oracle_stream(L, oracle, path, n_ctx, h, prompt, seed, rln, n_steps, nth, top_k=40):
    """the expectation: the oracle stepped one token at a time, a fresh sampler of the same seed drawing on its logits; returns the first token,
    the n_steps tokens after it, the sampler's window and the oracle handle (for its KV rows)"""
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


def _single_stream(L, h, seq, first, n_past, sampler, n_steps, nth, top_k=40):
    """the documented single-sequence loop: eval_topk -> sample_from_candidates (exact) / sample (not exact) -> accept"""
    h.set_seq(seq)
    tok, toks, flags = first, [], []
    for t in range(n_steps):
        exact, sc, ids, lg = h.eval_topk(np.array([tok], np.int32), n_past + t, sampler, top_k=top_k, n_threads=nth)
        tok = sampler.sample_from_candidates(sc, ids) if exact else sampler.sample(h, lg, top_k=top_k)
        sampler.accept(tok)
        toks.append(tok)
        flags.append(int(exact))
    h.set_seq(0)
    return toks, flags


def _two_calls(h, firsts, n_past, samplers, K1, K2, nth, top_k=40):
    a, ea = h.decode_sample_multi(firsts, n_past, K1, samplers, top_k=top_k, n_threads=nth, want_exact=True)
    b, eb = h.decode_sample_multi(a[:, -1], [n + K1 for n in n_past], K2, samplers, top_k=top_k, n_threads=nth, want_exact=True)
    return np.concatenate([a, b], axis=1), np.concatenate([ea, eb], axis=1)


def _check_against_oracle(L, oracle, path, n_ctx, h, prompts, seeds, firsts, samplers, got, nth, n_layer, check, top_k=40):
    for i in check:
        first, want, win, om = _oracle_stream(L, oracle, path, n_ctx, h, prompts[i], seeds[i], _rln(i), got.shape[1], nth, top_k)
        assert first == firsts[i], f"sequence {i}: first token"
        assert got[i].tolist() == want, f"sequence {i}: {got[i].tolist()} vs {want}"
        assert samplers[i].window().tolist() == win.tolist(), f"sequence {i}: sampler window"
        n = len(prompts[i]) + got.shape[1]
        h.set_seq(i)
        for il in (0, n_layer - 1):
            gk, gv = h.kv(il, n)
            ok, ov = om.kv(il, n)
            assert same(gk, ok) and same(gv, ov), f"sequence {i}: KV cache layer {il}"
        h.set_seq(0)
        om.close()


# (S, n_threads): one group; two groups of 10; n_threads > 32 -- llamahip_stage_set_applies says no (the loader takes head sizes 32 / 64 /
# 128 / 256 only, so the thread count is what sends a Q4_0 handle down the per-slot steps), every slot stepped and selected on its own
_PLAIN = {"1_seq": (1, 8), "3_seqs": (3, 5), "16_seqs": (16, 8), "20_seqs_two_groups": (20, 5), "5_seqs_per_slot_steps": (5, 40)}


@pytest.mark.parametrize("case", sorted(_PLAIN))
def test_sample_multi_equals_the_oracle_on_plain_handles(L, oracle, tmp_path, case):
    S, nth = _PLAIN[case]
    path = synth_tool(tmp_path / "m.bin", seed=47, **SMALL)
    n_ctx, K1, K2 = 64, 7, 5
    prompts, seeds = _prompts(S, SMALL["n_vocab"]), [1000 + 17 * i for i in range(S)]
    with L.Model(path, n_ctx=n_ctx, n_seq=S) as h:
        assert h.stage_set_applies(min(S, 16), nth) == (nth <= 32)
        samplers, firsts = _prefill(L, h, prompts, seeds, nth)
        got, exact = _two_calls(h, firsts, [len(p) for p in prompts], samplers, K1, K2, nth)
        assert exact.mean() > 0.8, exact
        check = range(S) if S <= 5 else sorted({0, 1, S // 2, 9, 10, S - 1} & set(range(S)))
        _check_against_oracle(L, oracle, path, n_ctx, h, prompts, seeds, firsts, samplers, got, nth, SMALL["n_layer"], check)


@pytest.mark.parametrize("nth", [8, 40])
def test_sample_multi_equals_the_single_sequence_loop(L, tmp_path, nth):
    """per slot: the same tokens AND the same exact flags as eval_topk + sample_from_candidates / sample + accept on a second handle"""
    S = 18
    path = synth_tool(tmp_path / "m.bin", seed=48, **SMALL)
    prompts, seeds = _prompts(S, SMALL["n_vocab"]), [7 * i + 3 for i in range(S)]
    with L.Model(path, n_ctx=64, n_seq=S) as h, L.Model(path, n_ctx=64, n_seq=S) as one:
        samplers, firsts = _prefill(L, h, prompts, seeds, nth)
        got, exact = _two_calls(h, firsts, [len(p) for p in prompts], samplers, 6, 6, nth)
        ref_samplers, ref_firsts = _prefill(L, one, prompts, seeds, nth)
        assert ref_firsts == firsts
        for i in range(S):
            toks, flags = _single_stream(L, one, i, firsts[i], len(prompts[i]), ref_samplers[i], 12, nth)
            assert got[i].tolist() == toks, f"sequence {i}"
            assert exact[i].tolist() == flags, f"sequence {i}: exact flags"
            assert samplers[i].window().tolist() == ref_samplers[i].window().tolist()


_PIPES = {"7b_width_2_stages_16_seqs": (W7B, [0, 0], 16, 8), "small_3_stages_40_seqs": (dict(SMALL, n_layer=5), [0, 0, 0], 40, 5)}


@pytest.mark.parametrize("case", sorted(_PIPES))
def test_sample_multi_on_pipeline_handles_equals_the_plain_handle(L, oracle, tmp_path, case):
    kw, devices, S, nth = _PIPES[case]
    path = synth_tool(tmp_path / "m.bin", seed=49, **kw)
    n_ctx = 64
    prompts, seeds = _prompts(S, kw["n_vocab"]), [31 * i + 5 for i in range(S)]
    res = {}
    with L.Model(path, n_ctx=n_ctx, n_seq=S) as one, L.Model(path, n_ctx=n_ctx, n_seq=S, devices=devices) as pm:
        for tag, h in (("plain", one), ("pipeline", pm)):
            samplers, firsts = _prefill(L, h, prompts, seeds, nth)
            res[tag] = _two_calls(h, firsts, [len(p) for p in prompts], samplers, 6, 4, nth) + (samplers, firsts)
        assert same(res["pipeline"][0], res["plain"][0]) and same(res["pipeline"][1], res["plain"][1])
        assert all(a.window().tolist() == b.window().tolist() for a, b in zip(res["pipeline"][2], res["plain"][2]))
        got, _, samplers, firsts = res["pipeline"]
        _check_against_oracle(L, oracle, path, n_ctx, pm, prompts, seeds, firsts, samplers, got, nth, kw["n_layer"], (0, S // 2, S - 1))


def test_sample_multi_host_path(L, oracle, tmp_path):
    """top_k = 100 (> 64): no device selection, every draw from the full row; a window of 1100 ids (> 1024): that slot's rows are spilled
    and drawn on the host while the other slots keep their device candidates"""
    S, nth = 6, 8
    path = synth_tool(tmp_path / "m.bin", seed=47, **SMALL)
    n_ctx = 64
    prompts, seeds = _prompts(S, SMALL["n_vocab"]), [1000 + 17 * i for i in range(S)]
    with L.Model(path, n_ctx=n_ctx, n_seq=S) as h:
        samplers, firsts = _prefill(L, h, prompts, seeds, nth, top_k=100)
        got, exact = _two_calls(h, firsts, [len(p) for p in prompts], samplers, 5, 4, nth, top_k=100)
        assert not exact.any()
        _check_against_oracle(L, oracle, path, n_ctx, h, prompts, seeds, firsts, samplers, got, nth, SMALL["n_layer"], range(S), top_k=100)
        # a long window on slot 2 only
        samplers = [L.Sampler(seed=s, repeat_last_n=1100 if i == 2 else 64) for i, s in enumerate(seeds)]
        ref = [L.Sampler(seed=s, repeat_last_n=1100 if i == 2 else 64) for i, s in enumerate(seeds)]
        n_past = [len(p) for p in prompts]
        firsts = [int(p[-1]) for p in prompts]
        for i in range(S):
            h.set_seq(i)
            h.eval(prompts[i], 0, nth)
        h.set_seq(0)
        got, exact = h.decode_sample_multi(firsts, n_past, 8, samplers, n_threads=nth, want_exact=True)
        assert not exact[2].any() and exact[[0, 1, 3, 4, 5]].mean() > 0.8, exact
        with L.Model(path, n_ctx=n_ctx, n_seq=S) as one:
            for i in range(S):
                one.set_seq(i)
                one.eval(prompts[i], 0, nth)
                toks, flags = _single_stream(L, one, i, firsts[i], n_past[i], ref[i], 8, nth)
                assert got[i].tolist() == toks and exact[i].tolist() == flags, f"sequence {i}"
                assert samplers[i].window().tolist() == ref[i].window().tolist()


@pytest.mark.parametrize("kind", ["f16", "q4_1", "q4_0_unfused"])
def test_sample_multi_on_handles_without_a_set_step(L, tmp_path, kind):
    hp = synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=4, n_layer=2)
    path, flags = str(tmp_path / "m.bin"), 0
    if kind == "q4_0_unfused":
        synth.write_model(path, hp, synth.random_tensors(hp, seed=9))
        flags = 2
    else:
        src = path + ".f16" if kind == "q4_1" else path
        synth.write_model_unquantized(src, hp, synth.random_tensors(hp, seed=9), 1)
        if kind == "q4_1":
            L.quantize_file(src, path, 3)
    S, nth = 4, 8
    prompts, seeds = _prompts(S, hp.n_vocab), [5 * i + 1 for i in range(S)]
    with L.Model(path, n_ctx=64, n_seq=S, flags=flags) as h, L.Model(path, n_ctx=64, n_seq=S, flags=flags) as one:
        samplers, firsts = _prefill(L, h, prompts, seeds, nth)
        got, exact = _two_calls(h, firsts, [len(p) for p in prompts], samplers, 5, 3, nth)
        ref_samplers, _ = _prefill(L, one, prompts, seeds, nth)
        for i in range(S):
            toks, fl = _single_stream(L, one, i, firsts[i], len(prompts[i]), ref_samplers[i], 8, nth)
            assert got[i].tolist() == toks and exact[i].tolist() == fl, f"{kind}: sequence {i}"
            assert samplers[i].window().tolist() == ref_samplers[i].window().tolist()


def test_sample_multi_errors(L, tmp_path):
    path = synth_tool(tmp_path / "m.bin", seed=47, **SMALL)
    with L.Model(path, n_ctx=64, n_seq=3) as h:
        ss = [L.Sampler(seed=i) for i in range(3)]
        with pytest.raises(L.LlamaHipError, match="context overflow"):
            h.decode_sample_multi([5, 6, 7], [62, 62, 62], 3, ss)
        with pytest.raises(L.LlamaHipError, match="4 sequences on a handle with 3 KV slots"):
            h.decode_sample_multi([1, 2, 3, 4], [0, 0, 0, 0], 2, ss + [L.Sampler(seed=9)])
        # nothing was drawn: the samplers are untouched
        assert all(s.window().tolist() == [0] * 64 for s in ss)
