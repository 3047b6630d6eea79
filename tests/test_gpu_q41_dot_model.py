"""GPU (-m gpu): LLAMAHIP_FLAG_FAST_Q41_DECODE on model handles, a 2-layer synthetic Q4_1 file."""
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

HP = synth.HParams(n_vocab=256, n_embd=256, n_mult=64, n_head=4, n_layer=2)
N_CTX = 128
MM = 4 * HP.n_layer + 1         # mat-muls of an eval: wq|wk|wv, wo, w1|w3, w2 per layer + the lm head
# rows -> (1 - min cosine, max |d logit|) against the EXACT handle, as measured (12.38); asserted at ten times.  At 63 rows 4-bit codes flip downstream.
MEASURED = {1: (4.688e-13, 9.965e-07), 9: (1.037e-12, 1.490e-06), 63: (7.100e-04, 3.008e-02)}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def logits(h, p, nth=8):
    return h.eval_debug(p, 0, nth, all_logits=True)["logits_all"]


def pair(L, files, flags=None, name="q4_1"):
    f = L.FAST_Q41_DECODE if flags is None else flags
    return L.Model(files[name], n_ctx=N_CTX, flags=f), L.Model(files[name], n_ctx=N_CTX, flags=f)


@pytest.fixture(scope="module")
def files(tmp_path_factory, L):
    d = str(tmp_path_factory.mktemp("q41_dot"))
    t = synth.random_tensors(HP, seed=3801)
    out = {name: os.path.join(d, name + ".bin") for name in ("q4_1", "f16", "q4_0")}
    synth.write_model_unquantized(out["f16"], HP, t, 1)
    synth.write_model(out["q4_0"], HP, t)
    L.quantize_file(out["f16"], out["q4_1"], 3)
    return out


def test_short_evals_take_the_dot_kernel_and_stay_close(L, files):
    p = synth.synth_prompt(63, HP.n_vocab, seed=94)
    with L.Model(files["q4_1"], n_ctx=N_CTX) as exact, L.Model(files["q4_1"], n_ctx=N_CTX, flags=L.FAST_Q41_DECODE) as dot:
        for n, (floor_cos, floor_d) in MEASURED.items():
            want = logits(exact, p[:n]).astype(np.float64)
            before = L.q41_dot_launches()
            got32 = logits(dot, p[:n])
            assert L.q41_dot_launches() - before == MM
            got = got32.astype(np.float64)
            assert np.isfinite(got).all()
            cos = (got * want).sum(1) / np.sqrt((got * got).sum(1) * (want * want).sum(1))
            print(f"{n} rows: 1 - min cosine = {1.0 - cos.min():.3e}, max |d logit| = {np.abs(got - want).max():.3e}")
            assert 1.0 - cos.min() <= 10 * floor_cos and np.abs(got - want).max() <= 10 * floor_d
            assert not same(got32, want.astype(np.float32)), f"{n} rows: bit-equal to the exact handle -- the flag had no effect"
        before = L.q41_dot_launches()
        la = exact.decode_greedy(int(p[5]), 63, 12, 8, want_logits=True)[1]
        lb = dot.decode_greedy(int(p[5]), 63, 12, 8, want_logits=True)[1]
        assert L.q41_dot_launches() > before and np.isfinite(lb).all() and not same(la, lb)


def test_a_9_row_eval_equals_nine_one_row_evals(L, files):
    """With n_threads = 1: with more threads the reference's soft_max . V (ggml.c:5620-5665) splits a row's keys by thread, so the exact
    attention itself follows the row count of an eval -- the last lines pin that on an EXACT handle."""
    p = synth.synth_prompt(9, HP.n_vocab, seed=95)
    a, b = pair(L, files)
    with a, b:
        many = logits(a, p, 1)
        for i in range(9):
            assert same(b.eval(p[i:i + 1], i, 1), many[i]), f"row {i} of the 9-row eval against its one-row eval"
        for il in range(HP.n_layer):
            assert all(same(x, y) for x, y in zip(a.kv(il, 9), b.kv(il, 9))), f"KV rows of layer {il}"
    a, b = pair(L, files, flags=0)
    with a, b:
        many = logits(a, p, 8)
        assert same(b.eval(p[:1], 0, 8), many[0]) and not same(b.eval(p[1:2], 1, 8), many[1]), "the exact handle with 8 threads"


def test_decode_greedy_equals_the_loop_of_one_row_evals(L, files):
    p = synth.synth_prompt(9, HP.n_vocab, seed=95)
    a, b = pair(L, files)
    with a, b:
        for h in (a, b):
            h.eval(p, 0, 8)
        toks, last = a.decode_greedy(int(p[3]), 9, 12, 8, want_logits=True)
        t = int(p[3])
        for i in range(12):
            lg = b.eval(np.array([t], np.int32), 9 + i, 8)
            t = int(np.argmax(lg))
            assert t == int(toks[i]), f"step {i} of the greedy loop"
        assert same(lg, last)
        for il in range(HP.n_layer):
            assert all(same(x, y) for x, y in zip(a.kv(il, 21), b.kv(il, 21))), f"KV rows of layer {il}"


@pytest.mark.parametrize("flags,other", [("FAST_Q41_DECODE", ""), ("FAST_Q41|FAST_Q41_DECODE", "FAST_Q41")])
def test_evals_of_64_rows_and_more_go_where_they_went(L, files, flags, other):
    bits = lambda s: sum(getattr(L, f) for f in s.split("|") if f)
    p = synth.synth_prompt(70, HP.n_vocab, seed=96)
    with L.Model(files["q4_1"], n_ctx=N_CTX, flags=bits(other)) as ref, L.Model(files["q4_1"], n_ctx=N_CTX, flags=bits(flags)) as flagged:
        before = L.q41_dot_launches()
        for n in (64, 70):
            assert same(logits(flagged, p[:n]), logits(ref, p[:n])), f"{n} rows"
        assert L.q41_dot_launches() == before


@pytest.mark.parametrize("name", ["f16", "q4_0"])
def test_other_file_types_ignore_the_flag(L, files, name):
    p = synth.synth_prompt(9, HP.n_vocab, seed=97)
    before = L.q41_dot_launches()
    with L.Model(files[name], n_ctx=N_CTX) as exact, L.Model(files[name], n_ctx=N_CTX, flags=L.FAST_Q41_DECODE) as flagged:
        assert same(logits(flagged, p), logits(exact, p))
        assert same(flagged.decode_greedy(int(p[2]), 9, 6, 8, want_logits=True)[1], exact.decode_greedy(int(p[2]), 9, 6, 8, want_logits=True)[1])
    assert L.q41_dot_launches() == before
