"""CPU: the host half of llamahip_beam_search -- the symbols, every refusal on a HOST_ONLY handle (the arguments first, the limit named, the
handle last), llamahip_beam_select and llamahip_beam_slots against tests/beam_ref.py's restatements (exhaustively for n_beams <= 3 over small
candidate tables, randomly up to 16: score ties, a stop candidate at every rank, NaN candidates, dead beams, every parent multiplicity,
sources never destinations), the conditions of the GPU cases shown on the CPU oracle's rows with numpy's log-softmax, and the host code under
ASan + UBSan in the stand-alone program `make asan` builds."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import beam_ref
import synth

HOST_ONLY = 4
HP = synth.HParams(n_vocab=96, n_embd=128, n_mult=64, n_head=2, n_layer=2)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
NEW = ("llamahip_op_top_logprobs", "llamahip_eval_top_logprobs", "llamahip_beam_search", "llamahip_beam_select", "llamahip_beam_slots")


def test_new_symbols_are_declared_and_exported(L):
    names = L.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for fn in NEW:
        assert fn in names and fn in exported, fn
    for fn in ("op_top_logprobs", "beam_select", "beam_slots"):
        assert callable(getattr(L, fn))
    assert callable(L.Model.beam_search) and callable(L.Model.eval_top_logprobs)


def test_every_refusal_comes_back_from_a_host_only_handle(L, tmp_path):
    path = str(tmp_path / "m.bin")
    synth.write_model(path, HP, synth.random_tensors(HP, seed=11))
    prompt = np.arange(1, 10, dtype=np.int32)
    ok = dict(prompt=prompt, n_beams=4, n_predict=12)
    bad = [(dict(n_beams=0), "n_beams 0 outside 1 .. 16"), (dict(n_beams=17), "n_beams 17 outside 1 .. 16"),
           (dict(n_beams=5), "n_beams 5 on a handle with 4 KV slots (llamahip_opts.n_seq)"),
           (dict(prompt=prompt[:0]), "n_prompt must be >= 1 (got 0)"), (dict(n_predict=0), "n_predict must be >= 1 (got 0)"),
           (dict(n_predict=40), "context overflow: n_prompt (9) + n_predict (40) > n_ctx (48)"),
           (dict(prompt=np.array([1, 96], np.int32)), "token id 96 at 1 out of range [0, 96)"),
           (dict(prompt=np.array([-1], np.int32)), "token id -1 at 0 out of range [0, 96)"),
           (dict(stop_token=96), "stop_token 96 out of range [-1, 96)"),
           (dict(n_return=5), "n_return 5 outside 0 .. n_beams (4)"), (dict(n_return=-1), "n_return -1 outside 0 .. n_beams (4)"),
           (dict(chunk_tokens=-1), "chunk_tokens must be >= 0 (0 = one eval; got -1)"), (dict(length_norm=2), "length_norm must be 0 or 1 (got 2)")]
    with L.Model(path, n_ctx=48, flags=HOST_ONLY, n_seq=4) as m:
        for change, text in bad:
            with pytest.raises(L.LlamaHipError) as e:
                m.beam_search(**dict(ok, **change))
            assert e.value.message == "llamahip_beam_search: " + text, e.value.message
        with pytest.raises(L.LlamaHipError, match="llamahip_beam_search: .*HOST_ONLY"):
            m.beam_search(**ok)
        with pytest.raises(L.LlamaHipError, match="llamahip_beam_search: .*HOST_ONLY"):
            m.beam_search(prompt, 4, 39, stop_token=95, n_return=4, length_norm=True, chunk_tokens=9)      # every limit reached, none crossed
        for n_top, text in ((0, "n_top 0 outside 1 .. 64"), (65, "n_top 65 outside 1 .. 64")):
            with pytest.raises(L.LlamaHipError) as e:
                m.eval_top_logprobs(prompt, 0, n_top)
            assert e.value.message == "llamahip_eval_top_logprobs: " + text
        with pytest.raises(L.LlamaHipError, match="HOST_ONLY"):
            m.eval_top_logprobs(prompt, 0, 5)
    tiny = synth.HParams(n_vocab=6, n_embd=128, n_mult=64, n_head=2, n_layer=1)
    synth.write_model(path, tiny, synth.random_tensors(tiny, seed=12))
    with L.Model(path, n_ctx=48, flags=HOST_ONLY, n_seq=4) as m:
        with pytest.raises(L.LlamaHipError) as e:
            m.beam_search(np.array([1], np.int32), 4, 2)
        assert e.value.message == "llamahip_beam_search: 2 * n_beams (8) candidates per row > n_vocab (6)"
        with pytest.raises(L.LlamaHipError, match="HOST_ONLY"):
            m.beam_search(np.array([1], np.int32), 3, 2)
        with pytest.raises(L.LlamaHipError, match="llamahip_eval_top_logprobs: n_top 7 > n_vocab 6"):
            m.eval_top_logprobs(np.array([1], np.int32), 0, 7)


def check_select(L, sc, ids, lp, B, stop):
    got = L.beam_select(sc, ids, lp, B, stop)
    new, fin, dead, _ = beam_ref.select(sc, ids, lp, B, stop)
    assert [tuple(x) for x in zip(got["parent"].tolist(), got["token"].tolist())] == [(i, v) for i, v, _ in new], (sc, ids, lp, B, stop)
    assert got["score"].tobytes() == np.array([c for _, _, c in new], np.float64).tobytes()
    assert got["fin_parent"].tolist() == [i for i, _ in fin] and got["fin_score"].tobytes() == np.array([c for _, c in fin], np.float64).tobytes()
    assert got["n_dead"] == dead
    return got


def check_slots(L, prev, parents, B):
    ns, copies = L.beam_slots(prev, parents, B)
    want_ns, want_copies = beam_ref.slots(list(prev), list(parents), B)
    assert ns.tolist() == want_ns and copies == want_copies, (prev, parents, B)
    assert len(set(ns.tolist())) == len(ns) and not ({s for s, _ in copies} & {d for _, d in copies})      # sources are never destinations
    assert all(0 <= s < B for s in ns.tolist())


def test_select_exhaustively_for_up_to_three_beams(L):
    """every table of candidate log-probabilities from a small set (ties included, a NaN, a -inf) x a stop id at every place or nowhere"""
    vals = (-0.5, -1.0, float("nan"), float("-inf"))
    n = 0
    for B in (1, 2, 3):
        nc = 2 * B
        for Lv in range(1, B + 1):
            scores = [(-0.5 * i) for i in range(Lv)]
            ids = np.array([[10 * i + j for j in range(nc)] for i in range(Lv)], np.int32)
            cells = Lv * nc
            tables = itertools.product(vals, repeat=cells) if cells <= 4 else (tuple(vals[(k * 7 + s) % 4] for k in range(cells)) for s in range(64))
            for tab in tables:
                lp = np.array(tab, np.float64).reshape(Lv, nc)
                for stop in [-1] + [int(v) for v in ids.reshape(-1)[:: max(1, cells // 6)]]:
                    check_select(L, scores, ids, lp, B, stop)
                    n += 1
            # dead beams: a row of -1 ids offers nothing
            dead_ids = ids.copy()
            dead_ids[0] = -1
            got = check_select(L, scores, dead_ids, np.full((Lv, nc), -0.25), B, -1)
            assert got["n_dead"] == 1 and 0 not in got["parent"].tolist()
    assert n > 500


def test_select_and_slots_randomly_up_to_sixteen_beams(L):
    rng = np.random.default_rng(5)
    for _ in range(400):
        B = int(rng.integers(1, 17))
        Lv, nc = int(rng.integers(1, B + 1)), 2 * B
        sc = -np.round(rng.random(Lv) * 4, 1)      # (coarse values: ties across beams)
        ids = np.stack([np.sort(rng.choice(60, size=nc, replace=False)) for _ in range(Lv)]).astype(np.int32)
        lp = -np.sort(np.round(rng.random((Lv, nc)) * 3, 1), axis=1)
        lp[rng.random((Lv, nc)) < 0.05] = np.nan
        if rng.random() < 0.3:
            ids[int(rng.integers(0, Lv))] = -1
        stop = int(rng.integers(-1, 60))
        got = check_select(L, sc, ids, lp, B, stop)
        prev = rng.permutation(B)[:Lv].astype(np.int32)
        check_slots(L, prev, got["parent"], B)


def test_slots_at_every_parent_multiplicity(L):
    for B in (1, 2, 3, 4):
        for Lv in range(1, B + 1):
            for prev in itertools.permutations(range(B), Lv):
                for n_new in range(0, B + 1):
                    for parents in itertools.product(range(Lv), repeat=n_new):
                        check_slots(L, np.array(prev, np.int32), np.array(parents, np.int32), B)
    with pytest.raises(L.LlamaHipError):
        L.beam_slots([0, 0], [0], 2)
    with pytest.raises(L.LlamaHipError):
        L.beam_slots([0], [1], 2)


def test_the_gpu_cases_meet_their_conditions_on_the_cpu_oracle(L, oracle, tmp_path):
    """tests/test_gpu_beam_search.py's Q4_0 cases on the oracle's rows with numpy's log-softmax: a copy, a childless parent, a STOP hypothesis
    in the stop cases, and neighbouring candidates more than 1e-6 apart -- so rows that differ in the last bits cannot change a case"""
    hp = synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=4, n_layer=2)
    path = str(tmp_path / "beam.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=beam_ref.MODEL_SEED))
    om = oracle.load(path, 64)
    early = 0
    try:
        for n_beams, n_prompt, chunk, stop, n_return, length_norm in beam_ref.CASES + beam_ref.HANDLE_CASES:
            prompt = synth.synth_prompt(n_prompt, hp.n_vocab, seed=beam_ref.PROMPT_SEED)
            memo = {}

            def cands_of(tokens):
                if tokens not in memo:
                    step = chunk or n_prompt
                    for c0 in range(0, n_prompt, step):
                        row = om.eval(prompt[c0:c0 + step], c0, 8)["logits"]
                    for j, t in enumerate(tokens):
                        row = om.eval(np.array([t], np.int32), n_prompt + j, 8)["logits"]
                    memo[tokens] = beam_ref.np_cands(row, 2 * n_beams)
                return memo[tokens]

            stop_token = -1
            if stop:
                free, _ = beam_ref.search(cands_of, n_prompt, n_beams, 12)
                stop_token = int(free[1]["tokens"][beam_ref.STOP_AT])
            want, info = beam_ref.search(cands_of, n_prompt, n_beams, 12, stop_token, n_return, bool(length_norm))
            tag = (n_beams, n_prompt, chunk, stop_token)
            assert info["min_gap"] > 1e-6, (tag, info["min_gap"])
            assert n_beams < 2 or info["n_copies"] >= 1, tag
            assert n_beams < 3 or info["childless"], tag
            assert not stop or (info["n_stop"] >= 1 and any(h["reason"] == "stop" for h in want)), tag
            early += info["early_end"]
        assert early >= 1, "no case ends early"
    finally:
        om.close()


def test_beam_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: beam.cpp (the step rule, the slots, the argument check at short and missing message buffers, the ranking) compiled with
    -fsanitize=address,undefined into the stand-alone tools/host_sanitize and run there -- never loaded into python"""
    subprocess.run(["make", "-s", "-C", CSRC, "asan"], check=True)
    src = open(os.path.join(CSRC, "tools", "host_sanitize.cpp")).read()
    assert "llamahip_beam_select(" in src and "llamahip_beam_slots(" in src and "lh::beam_check(" in src and "lh::beam_rank(" in src
    assert "beam.cpp" in open(os.path.join(CSRC, "Makefile")).read().split("asan:")[1].split("tools:")[0]
    path = str(tmp_path / "m.bin")
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(CSRC, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout and "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if "beam search:" in ln]
    assert len(line) == 1 and " 0 " not in line[0], r.stdout
