"""GPU (-m gpu): LLAMAHIP_FLAG_FAST_DENSE on model handles.  A small synthetic f16 file (d 256, F 704, 2 layers): evals of >= 64 rows take
k_dense_f16_fast and stay close to the exact handle; everything below 64 rows and the greedy loop keep the exact handle's bits; an f32 file
ignores the flag.  f16 / f32 handles have no per-layer dumps, so closeness is the cosine of the logits against the EXACT handle."""
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

HP = synth.HParams(n_vocab=256, n_embd=256, n_mult=64, n_head=4, n_layer=2)
N_CTX = 128
# Every mat-mul output differs from the exact one by fp32 rounding of its sum; downstream an activation that lands across an fp16
# rounding boundary moves by 2^-11 of itself, and a logit row perturbed by a relative eps has 1 - cosine ~ eps^2 / 2.  Measured on the first
# run against the exact handle: 1 - min cosine = 1.0e-7 at 64 rows and 1.0e-7 at 70 (max |d logit| 4.6e-4); the floor leaves a margin of
# 100 x over that, and a wrong tile (cosine ~ 0.9 or NaN) is five orders of magnitude beyond it.
MIN_COSINE = 1.0 - 1e-5


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense_fast")
    t = synth.random_tensors(HP, seed=3501)
    out = {}
    for name, ftype in (("f16", 1), ("f32", 0)):
        out[name] = os.path.join(str(d), f"{name}.bin")
        synth.write_model_unquantized(out[name], HP, t, ftype)
    return out


def test_long_evals_take_the_fast_kernel_and_stay_close(L, files):
    p = synth.synth_prompt(70, HP.n_vocab, seed=71)
    with L.Model(files["f16"], n_ctx=N_CTX) as exact, L.Model(files["f16"], n_ctx=N_CTX, flags=L.FAST_DENSE) as fast:
        for n in (64, 70):
            want = exact.eval_debug(p[:n], 0, 8, all_logits=True)["logits_all"].astype(np.float64)
            before = L.dense_fast_launches()
            got32 = fast.eval_debug(p[:n], 0, 8, all_logits=True)["logits_all"]
            assert L.dense_fast_launches() - before == 4 * HP.n_layer + 1      # wq|wk|wv, wo, w1|w3, w2 per layer + the all-rows lm head
            got = got32.astype(np.float64)
            assert np.isfinite(got).all()
            cos = (got * want).sum(1) / np.sqrt((got * got).sum(1) * (want * want).sum(1))
            print(f"{n} rows: 1 - min cosine = {1.0 - cos.min():.3e}, max |d logit| = {np.abs(got - want).max():.3e}")
            assert cos.min() >= MIN_COSINE
            assert not same(got32, want.astype(np.float32)), f"{n} rows: bit-equal to the exact handle -- the flag had no effect"


def test_the_flag_does_not_leak_below_64_rows(L, files):
    p = synth.synth_prompt(63, HP.n_vocab, seed=72)
    with L.Model(files["f16"], n_ctx=N_CTX) as exact, L.Model(files["f16"], n_ctx=N_CTX, flags=L.FAST_DENSE) as fast:
        before = L.dense_fast_launches()
        for n in (1, 9, 63):
            assert same(fast.eval_debug(p[:n], 0, 8, all_logits=True)["logits_all"], exact.eval_debug(p[:n], 0, 8, all_logits=True)["logits_all"]), f"{n} rows"
        tok = int(p[5])
        a, la = exact.decode_greedy(tok, 63, 12, 8, want_logits=True)
        b, lb = fast.decode_greedy(tok, 63, 12, 8, want_logits=True)
        assert a.tolist() == b.tolist() and same(la, lb)
        assert L.dense_fast_launches() == before


def test_an_f32_file_ignores_the_flag(L, files):
    p = synth.synth_prompt(64, HP.n_vocab, seed=73)
    before = L.dense_fast_launches()
    with L.Model(files["f32"], n_ctx=N_CTX) as exact, L.Model(files["f32"], n_ctx=N_CTX, flags=L.FAST_DENSE) as flagged:
        assert same(flagged.eval_debug(p, 0, 8, all_logits=True)["logits_all"], exact.eval_debug(p, 0, 8, all_logits=True)["logits_all"])
    assert L.dense_fast_launches() == before
