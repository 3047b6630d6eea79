"""CPU (-m "not gpu"): the host half of drafted greedy decoding -- the drafter (llamahip_lookup_draft) against its Python restatement,
the argument refusals of llamahip_verify_greedy / llamahip_decode_greedy_lookup on a handle without device state, the symbol table."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lookup_ref
import synth

HOST_ONLY = 4


def _stream(rng, n, alphabet):
    """a low-entropy stream: short phrases over a small alphabet repeated with noise, so that n-grams of every length recur"""
    phrases = [rng.integers(0, alphabet, rng.integers(2, 7)).tolist() for _ in range(4)]
    out = []
    while len(out) < n:
        out += phrases[rng.integers(0, 4)] if rng.random() < 0.7 else rng.integers(0, alphabet, 2).tolist()
    return out[:n]


def test_header_defaults_are_the_restatements(L):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "llamahip.h")).read()
    for name, want in (("DRAFT_LEN", lookup_ref.DRAFT_LEN), ("NGRAM_MIN", lookup_ref.NGRAM_MIN), ("NGRAM_MAX", lookup_ref.NGRAM_MAX)):
        assert f"#define LLAMAHIP_LOOKUP_{name} {want}\n" in text


def test_lookup_draft_equals_the_restatement_on_random_streams(L):
    rng = np.random.default_rng(11)
    seen = {"hist": 0, "corpus": 0, "none": 0, "short": 0, "clipped": 0}
    hit_n = {1: 0, 2: 0, 3: 0, 4: 0}
    for case in range(600):
        alphabet = int(rng.integers(4, 9))
        hist = _stream(rng, int(rng.integers(1, 60)), alphabet)
        corpus = _stream(rng, int(rng.integers(0, 80)), alphabet + (4 if case % 3 == 0 else 0)) if case % 2 else None
        k, lo, hi = int(rng.integers(0, 16)), int(rng.integers(0, 4)), int(rng.integers(0, 5))
        if (lo or lookup_ref.NGRAM_MIN) > (hi or lookup_ref.NGRAM_MAX):
            with pytest.raises(ValueError):
                L.lookup_draft(hist, corpus, k, lo, hi)
            continue
        want = lookup_ref.draft(hist, corpus, k, lo, hi)
        got = L.lookup_draft(hist, corpus, k, lo, hi).tolist()
        assert got == want, (case, hist, corpus, k, lo, hi)
        assert L.lookup_draft(hist, corpus, k, lo, hi).tolist() == got          # deterministic
        # which branch this case took (the restatement run per n and per stream)
        if not want:
            seen["none"] += 1
            continue
        for n in range(min(hi or 3, len(hist)), (lo or 1) - 1, -1):
            if lookup_ref.draft(hist, None, k, n, n):
                seen["hist"] += 1
                hit_n[n] += 1
                break
            if lookup_ref.draft(hist, corpus, k, n, n):
                seen["corpus"] += 1
                hit_n[n] += 1
                break
        seen["short"] += len(want) < (k or lookup_ref.DRAFT_LEN)
        seen["clipped"] += len(want) == (k or lookup_ref.DRAFT_LEN)
    assert all(v > 5 for v in seen.values()), seen
    assert all(v > 5 for v in hit_n.values()), hit_n


def test_lookup_draft_named_cases(L):
    d = L.lookup_draft
    assert d([1, 2, 3, 4, 1, 2], draft_len=8).tolist() == [3, 4, 1, 2]             # a hit whose continuation runs into the end of the stream
    assert d([1, 2, 3, 4, 1, 2], draft_len=2).tolist() == [3, 4]                   # draft_len cuts it
    assert d([7, 1, 2, 9, 5, 1, 2], draft_len=3).tolist() == [9, 5, 1]             # 2-gram hit ...
    assert d([7, 1, 2, 9, 2, 8, 6, 2], draft_len=3).tolist() == [8, 6, 2]          # ... the MOST RECENT earlier occurrence of a 1-gram
    assert d([1, 2, 3], draft_len=4).tolist() == []                                # nothing recurs
    assert d([1, 2, 3], [9, 2, 3, 7, 7], draft_len=4).tolist() == [7, 7]           # corpus only, short: the corpus ends
    assert d([1, 2, 3], [2, 3, 5, 9, 2, 3], draft_len=4).tolist() == [5, 9, 2, 3]  # the corpus' last occurrence has no successor: the one before
    assert d([4, 2, 3, 6, 2, 3], [2, 3, 5, 5], draft_len=4).tolist() == [6, 2, 3]  # the history is tried before the corpus
    assert d([9, 9, 1, 2, 3], [1, 2, 3, 4, 8, 2, 3, 5], draft_len=2).tolist() == [4, 8]      # the longer n-gram wins over a later, shorter match
    assert d([9, 9, 1, 2, 3], [1, 2, 3, 4, 8, 2, 3, 5], draft_len=2, ngram_max=2).tolist() == [5]
    assert d([5], draft_len=3).tolist() == [] and d([], [1, 2], draft_len=3).tolist() == []
    with pytest.raises(ValueError):
        d([1, 2], draft_len=-1)
    with pytest.raises(ValueError):
        d([1, 2], ngram_min=3, ngram_max=2)


def test_loop_restatement_counts_add_up():
    """n_steps = verify steps + single steps + accepted tokens, whatever the corpus"""
    rng = np.random.default_rng(3)
    for _ in range(50):
        G = _stream(rng, 90, 6)
        ctx = _stream(rng, 12, 6)
        corpus = list(G)
        for i in range(6, len(corpus), 7):
            corpus[i] = (corpus[i] + 1) % 6
        for c in (None, G, corpus):
            st = lookup_ref.loop_stats(ctx, 2, G, c, int(rng.integers(0, 16)))
            assert st["n_verify_steps"] + st["n_single_steps"] + st["n_accepted"] == len(G)
            assert 0 <= st["n_accepted"] <= st["n_drafted"]


@pytest.fixture()
def host_model(L, tmp_path):
    hp = synth.HParams(n_vocab=64, n_embd=64, n_mult=32, n_head=2, n_layer=1)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    with L.Model(path, n_ctx=32, flags=HOST_ONLY) as m:
        yield m


def test_verify_greedy_refusals_name_their_limit(L, host_model):
    m = host_model
    for call, what in ((lambda: m.verify_greedy(5, np.arange(16), 0), r"n_draft must be 0 \.\. 15 \(got 16\)"),
                       (lambda: m.verify_greedy(5, [1, 2, 3], 29), r"n_past \(29\) \+ n_draft \(3\) \+ 1 > n_ctx \(32\)"),
                       (lambda: m.verify_greedy(5, [1, 2, 3], -1), r"context overflow"),
                       (lambda: m.verify_greedy(64, [1], 0), r"token id 64 out of range \[0, 64\)"),
                       (lambda: m.verify_greedy(5, [1, -2], 0), r"draft token id -2 at 1 out of range \[0, 64\)"),
                       (lambda: m.verify_greedy(5, [1, 2], 3), r"HOST_ONLY")):
        with pytest.raises(L.LlamaHipError, match=what) as e:
            call()
        assert e.value.code == -1001


def test_decode_greedy_lookup_refusals_name_their_limit(L, host_model):
    m = host_model
    ctx = np.arange(8, dtype=np.int32)
    for call, what in ((lambda: m.decode_greedy_lookup(5, 30, 8, ctx), r"n_past \(8\) \+ n_steps \(30\) > n_ctx \(32\)"),
                       (lambda: m.decode_greedy_lookup(5, 0, 8, ctx), r"context overflow"),
                       (lambda: m.decode_greedy_lookup(5, 2**31 - 1, 8, ctx), r"context overflow"),
                       (lambda: m.decode_greedy_lookup(99, 4, 8, ctx), r"token id 99 out of range \[0, 64\)"),
                       (lambda: m.decode_greedy_lookup(5, 4, 9, ctx), r"n_context \(8\) must equal n_past \(9\)"),
                       (lambda: m.decode_greedy_lookup(5, 4, 8, ctx + 60), r"context token id 64 at 4 out of range"),
                       (lambda: m.decode_greedy_lookup(5, 4, 8, ctx, corpus=[1, 2, 64]), r"corpus token id 64 at 2 out of range"),
                       (lambda: m.decode_greedy_lookup(5, 4, 8, ctx, draft_len=16), r"draft_len must be 1 \.\. 15"),
                       (lambda: m.decode_greedy_lookup(5, 4, 8, ctx, draft_len=-1), r"draft_len must be 1 \.\. 15"),
                       (lambda: m.decode_greedy_lookup(5, 4, 8, ctx, ngram_min=4), r"ngram_min \(4\) / ngram_max \(0\)"),
                       (lambda: m.decode_greedy_lookup(5, 4, 8, ctx, ngram_max=-1), r"ngram_min \(0\) / ngram_max \(-1\)"),
                       (lambda: m.decode_greedy_lookup(5, 4, 8, ctx), r"HOST_ONLY")):
        with pytest.raises(L.LlamaHipError, match=what) as e:
            call()
        assert e.value.code == -1001


def test_the_new_entry_points_are_exported(L):
    so = L.LIB_PATH
    if not (shutil.which("nm") and os.path.exists(so)):
        pytest.fail("needs binutils' nm and the built libllamahip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    want = {"llamahip_verify_greedy", "llamahip_decode_greedy_lookup", "llamahip_lookup_draft", "llamahip_op_verify_rows"}
    assert want <= exported and want <= set(L.declared_symbols())
