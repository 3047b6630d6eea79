"""CPU: the host half of drafted greedy decoding for several sequences at once -- llamahip_lookup_deal_rows against its Python restatement
(tests/lookup_multi_ref.py), every refusal of llamahip_verify_greedy_multi / llamahip_decode_greedy_lookup_multi on a HOST_ONLY handle
(the arguments are checked before any device work), and the new symbols in the header and the library's dynamic table."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lookup_multi_ref
import synth

HOST_ONLY = 4


def test_deal_rows_equals_the_restatement(L):
    rng = np.random.default_rng(5)
    for n in range(1, 17):
        for budget in range(n, 17):
            for trial in range(12):
                hi = (1, 4, 16)[trial % 3]          # nobody / a few / most want more than there is
                want = rng.integers(0, hi, n).astype(np.int32)
                give = L.lookup_deal_rows(want, budget)
                assert give.tolist() == lookup_multi_ref.deal_rows(want.tolist(), budget), (n, budget, want)
                assert give.sum() <= budget - n and (give <= want).all() and (give >= 0).all()
                assert give.sum() == min(budget - n, int(want.sum()))          # spares are left only when nobody wants more
                # round-robin: no sequence receives two more tokens than another that still wanted one
                for i in range(n):
                    for j in range(n):
                        if give[j] < want[j]:
                            assert give[i] <= give[j] + 1, (n, budget, want, give)
                # ... and of two that still wanted more, the one with the lower index is never behind
                short = [i for i in range(n) if give[i] < want[i]]
                assert all(give[a] >= give[b] for a, b in zip(short, short[1:]))
    assert L.lookup_deal_rows([15], 16).tolist() == [15]
    assert L.lookup_deal_rows([15, 15, 15], 16).tolist() == [5, 4, 4]
    assert L.lookup_deal_rows([1, 0, 9, 2], 16).tolist() == [1, 0, 9, 2]
    assert L.lookup_deal_rows([1, 0, 9, 4], 12).tolist() == [1, 0, 4, 3]


def test_deal_rows_refuses_bad_arguments(L):
    for want, budget in (([], 16), ([1] * 17, 16), ([1, 2], 1), ([1, 2], 17), ([16], 16), ([-1, 2], 16)):
        with pytest.raises(ValueError, match="lookup_deal_rows: bad arguments"):
            L.lookup_deal_rows(want, budget)
    f = L.lib().llamahip_lookup_deal_rows
    one = np.ones(2, np.int32)
    assert f(None, 2, 16, one.ctypes.data) == -1 and f(one.ctypes.data, 2, 16, None) == -1


def test_the_restatement_of_the_loop_keeps_the_identity():
    rng = np.random.default_rng(12)
    for n in (1, 2, 3, 5, 8, 16):
        n_steps = int(rng.integers(1, 60))
        ctxs = [rng.integers(0, 6, int(rng.integers(0, 30))).tolist() for _ in range(n)]
        Gs = [rng.integers(0, 6, n_steps).tolist() for _ in range(n)]
        corpus = sum(Gs, [])
        for c in (None, corpus):
            st = lookup_multi_ref.loop_stats(ctxs, [2] * n, Gs, c, int(rng.integers(0, 16)))
            for x in st:
                assert x["n_verify_steps"] + x["n_single_steps"] + x["n_accepted"] == n_steps and 0 <= x["n_accepted"] <= x["n_drafted"]
    # one sequence: the single-sequence loop's counts
    import lookup_ref
    G = rng.integers(0, 5, 50).tolist()
    assert lookup_multi_ref.loop_stats([[1, 2, 3]], [2], [G], G) == [lookup_ref.loop_stats([1, 2, 3], 2, G, G)]


@pytest.fixture()
def host_model(L, tmp_path):
    hp = synth.HParams(n_vocab=64, n_embd=64, n_mult=32, n_head=2, n_layer=1)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    with L.Model(path, n_ctx=32, n_seq=20, flags=HOST_ONLY) as m:
        yield m


def test_verify_greedy_multi_refusals_name_their_limit(L, host_model):
    m = host_model
    v = m.verify_greedy_multi
    for call, what in ((lambda: v(range(17), [5] * 17, [[]] * 17, [0] * 17), r"n_seqs must be 1 \.\. 16 \(got 17\).*llamahip_decode_greedy_multi"),
                       (lambda: v([], [], [], []), r"n_seqs must be 1 \.\. 16 \(got 0\)"),
                       (lambda: v([0, 20], [5, 5], [[], []], [0, 0]), r"sequence slot 20 out of range \[0, 20\)"),
                       (lambda: v([0, -1], [5, 5], [[], []], [0, 0]), r"sequence slot -1 out of range \[0, 20\)"),
                       (lambda: v([0, 3, 0], [5, 5, 5], [[], [], []], [0, 0, 0]), r"sequence slot 0 appears twice"),
                       (lambda: v([0], [5], [np.arange(16)], [0]), r"n_draft must be 0 \.\. 15 \(got 16 for slot 0\)"),
                       (lambda: v([0, 1], [5, 5], [[1], [1, 2, 3]], [0, 29]), r"n_past \(29\) \+ n_draft \(3\) \+ 1 > n_ctx \(32\)"),
                       (lambda: v([0, 1], [5, 5], [[1], [1]], [0, -1]), r"context overflow"),
                       (lambda: v([0, 1], [5, 64], [[1], [1]], [0, 0]), r"token id 64 out of range \[0, 64\)"),
                       (lambda: v([0, 1], [5, 5], [[1], [1, -2]], [0, 0]), r"draft token id -2 at 2 out of range \[0, 64\)"),
                       (lambda: v([0, 1, 2], [5, 5, 5], [[1] * 7, [1] * 6, [1]], [0, 0, 0]), r"at most 16 rows \(3 sequences"),
                       (lambda: v([0, 1], [5, 5], [[1, 2], []], [3, 4]), r"HOST_ONLY")):
        with pytest.raises(L.LlamaHipError, match=what) as e:
            call()
        assert e.value.code == -1001
    # null pointers
    import ctypes as C
    f, err = L.lib().llamahip_verify_greedy_multi, C.create_string_buffer(512)
    a = np.zeros(4, np.int32)
    p = a.ctypes.data
    for args, what in (((None, p, p, p, p, p, p), "null slots"), ((p, None, p, p, p, p, p), "null slots"), ((p, p, None, p, p, p, p), "null slots"),
                       ((p, p, p, p, None, p, p), "null slots"), ((p, p, p, p, p, None, p), "null output"), ((p, p, p, p, p, p, None), "null output")):
        assert f(m._h, 8, 1, *args, err, len(err)) == -1001 and what in err.value.decode()
    one = np.ones(1, np.int32)
    assert f(m._h, 8, 1, p, p, p, None, one.ctypes.data, p, p, err, len(err)) == -1001 and "null drafts" in err.value.decode()
    assert f(None, 8, 1, p, p, p, p, p, p, p, err, len(err)) == -1001 and "null model" in err.value.decode()


def test_decode_greedy_lookup_multi_refusals_name_their_limit(L, host_model):
    m = host_model
    g = m.decode_greedy_lookup_multi
    ctx = [np.arange(8, dtype=np.int32), np.arange(3, dtype=np.int32)]
    for call, what in ((lambda: g([5] * 17, [0] * 17, 4, [[]] * 17), r"n_seqs must be 1 \.\. 16 \(got 17\).*llamahip_decode_greedy_multi"),
                       (lambda: g([], [], 4, []), r"n_seqs must be 1 \.\. 16 \(got 0\)"),
                       (lambda: g([5, 5], [8, 3], 30, ctx), r"n_past \(8\) \+ n_steps \(30\) > n_ctx \(32\)"),
                       (lambda: g([5, 5], [8, 3], 0, ctx), r"context overflow"),
                       (lambda: g([5, 5], [8, -3], 4, ctx), r"context overflow"),
                       (lambda: g([5, 99], [8, 3], 4, ctx), r"token id 99 out of range \[0, 64\)"),
                       (lambda: g([5, 5], [8, 3], 4, [ctx[0], ctx[1] + 62]), r"context token id 64 at 2 out of range"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, corpus=[1, 2, 64]), r"corpus token id 64 at 2 out of range"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, draft_len=16), r"draft_len must be 1 \.\. 15"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, ngram_min=4), r"ngram_min \(4\) / ngram_max \(0\)"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, stats_size=8), r"stats->struct_size \(8\)"),
                       (lambda: g([5, 5], [8, 3], 4, ctx), r"HOST_ONLY")):
        with pytest.raises(L.LlamaHipError, match=what) as e:
            call()
        assert e.value.code == -1001
    import ctypes as C
    f, err = L.lib().llamahip_decode_greedy_lookup_multi, C.create_string_buffer(512)
    a = np.zeros(4, np.int32)
    p = a.ctypes.data
    assert f(m._h, 8, 1, None, p, 4, None, None, 0, 0, 0, 0, p, None, err, len(err)) == -1001 and "null n_past" in err.value.decode()
    assert f(m._h, 8, 1, p, None, 4, None, None, 0, 0, 0, 0, p, None, err, len(err)) == -1001 and "null n_past" in err.value.decode()
    assert f(m._h, 8, 1, p, p, 4, None, None, 0, 0, 0, 0, None, None, err, len(err)) == -1001 and "null out_tokens" in err.value.decode()
    one = np.ones(1, np.int32)
    assert f(m._h, 8, 1, one.ctypes.data, p, 4, None, None, 0, 0, 0, 0, p, None, err, len(err)) == -1001 and "null context" in err.value.decode()
    assert f(m._h, 8, 1, p, p, 4, None, None, 3, 0, 0, 0, p, None, err, len(err)) == -1001 and "corpus of 3 tokens at a null pointer" in err.value.decode()
    assert f(None, 8, 1, p, p, 4, None, None, 0, 0, 0, 0, p, None, err, len(err)) == -1001 and "null model" in err.value.decode()


def test_more_sequences_than_kv_slots_are_refused(L, tmp_path):
    hp = synth.HParams(n_vocab=64, n_embd=64, n_mult=32, n_head=2, n_layer=1)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    with L.Model(path, n_ctx=32, n_seq=2, flags=HOST_ONLY) as m:
        with pytest.raises(L.LlamaHipError, match=r"3 sequences on a handle with 2 KV slots"):
            m.decode_greedy_lookup_multi([5, 5, 5], [0, 0, 0], 4, [[], [], []])
        with pytest.raises(L.LlamaHipError, match=r"3 sequences on a handle with 2 KV slots"):
            m.verify_greedy_multi([0, 1, 0], [5, 5, 5], [[], [], []], [0, 0, 0])


def test_the_new_entry_points_are_declared_and_exported(L):
    so = L.LIB_PATH
    if not (shutil.which("nm") and os.path.exists(so)):
        pytest.fail("needs binutils' nm and the built libllamahip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    want = {"llamahip_verify_greedy_multi", "llamahip_decode_greedy_lookup_multi", "llamahip_lookup_deal_rows", "llamahip_op_verify_rows_set"}
    assert want <= exported and want <= set(L.declared_symbols())
    # the version script exports by prefix: every new name falls under one of its global patterns
    text = open(os.path.join(os.path.dirname(so), "exports.map")).read()
    pats = re.search(r"global:(.*?)local:", text, re.S).group(1).replace(";", " ").split()
    import fnmatch
    assert all(any(fnmatch.fnmatchcase(s, p) for p in pats) for s in want)
