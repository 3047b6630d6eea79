"""GPU (-m gpu): LLAMAHIP_FLAG_FAST_ATTN on model handles.  Synthetic Q4_0 and f16 files (d 256, 2 heads of 128, 2 layers, n_ctx 256): evals
of >= 64 rows take k_flash_attn and stay close to the exact handle; everything below 64 rows, the greedy loop and a head size of 64 keep the
exact handle's bits; decode behind a flagged eval reads the same cache format; eval_multi falls back to the per-slot loop."""
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

HP = synth.HParams(n_vocab=256, n_embd=256, n_mult=64, n_head=2, n_layer=2)
N_CTX = 256
# The fused kernel narrows q, k and v to fp16 once (2^-11 relative) where the exact chain perturbs the weights by its fp16 exp table (the same
# size); a logit row perturbed by a relative eps has 1 - cosine ~ eps^2 / 2.  Measured on the first run against the EXACT handle, the largest
# 1 - min cosine over 64 and 130 rows: f16 file 3.3e-7 (max |d logit| 8.0e-4) with and without FAST_DENSE; Q4_0 file 2.8e-2 (max |d logit|
# 0.26).  The floor is 100 x the measured value: on the f16 file a wrong tile (cosine ~ 0.9 or NaN) is orders of magnitude beyond it.  On the
# Q4_0 file the measured value is not the kernel's: launch_prep re-quantises every merged row to 4-bit blocks for wo, an attention output
# moved by 2^-11 lands across a quantisation step of 1 / 7 of its block's maximum, and the logits move as they do under FAST_PREFILL (cosine
# 0.986, llamahip.h).  100 x 2.8e-2 is no floor at all -- there the assertions that bite are the finite logits, the launch count and the bits
# that differ; the kernel itself is held to its derived bound by test_gpu_flash_attn_op.py and to the f16 floor here (the same launches).
ONE_MINUS_COSINE = {"f16": 3.3e-7, "q4_0": 2.8e-2}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("flash_attn"))
    t = synth.random_tensors(HP, seed=3601)
    out = {"q4_0": os.path.join(d, "q4_0.bin"), "f16": os.path.join(d, "f16.bin"), "head64": os.path.join(d, "head64.bin")}
    synth.write_model(out["q4_0"], HP, t)
    synth.write_model_unquantized(out["f16"], HP, t, 1)
    hp64 = synth.HParams(n_vocab=256, n_embd=256, n_mult=64, n_head=4, n_layer=2)
    synth.write_model(out["head64"], hp64, synth.random_tensors(hp64, seed=3602))
    return out


def launches_of(L, n_rows, n_past=0):
    """what one eval adds to the counter: k_flash_attn per layer, plus k_flash_combine where the plan splits"""
    return HP.n_layer * (1 if L.flash_attn_plan(n_rows, n_past + n_rows, HP.n_head)["key_splits"] == 1 else 2)


@pytest.mark.parametrize("name,flags", [("q4_0", "FAST_ATTN"), ("f16", "FAST_ATTN"), ("f16", "FAST_DENSE|FAST_ATTN")])
def test_long_evals_take_the_fused_kernel_and_stay_close(L, files, name, flags):
    p = synth.synth_prompt(130, HP.n_vocab, seed=81)
    fl = sum(getattr(L, f) for f in flags.split("|"))
    with L.Model(files[name], n_ctx=N_CTX) as exact, L.Model(files[name], n_ctx=N_CTX, flags=fl) as fast:
        for n in (64, 130):
            want = exact.eval_debug(p[:n], 0, 8, all_logits=True)["logits_all"].astype(np.float64)
            before, dense_before = L.flash_attn_launches(), L.dense_fast_launches()
            got32 = fast.eval_debug(p[:n], 0, 8, all_logits=True)["logits_all"]
            assert L.flash_attn_launches() - before == launches_of(L, n)
            assert (L.dense_fast_launches() > dense_before) == ("FAST_DENSE" in flags)
            got = got32.astype(np.float64)
            assert np.isfinite(got).all()
            cos = (got * want).sum(1) / np.sqrt((got * got).sum(1) * (want * want).sum(1))
            print(f"{name} {flags} {n} rows: 1 - min cosine = {1.0 - cos.min():.3e}, max |d logit| = {np.abs(got - want).max():.3e}")
            assert 1.0 - cos.min() <= 100 * ONE_MINUS_COSINE[name]
            assert not same(got32, want.astype(np.float32)), f"{n} rows: bit-equal to the exact handle -- the flag had no effect"


@pytest.mark.parametrize("name", ["q4_0", "f16", "head64"])
def test_the_flag_does_not_leak(L, files, name):
    """below 64 rows, in the greedy loop, and at every row count on a head size of 64: the unflagged handle's bits, no launch counted"""
    p = synth.synth_prompt(130, HP.n_vocab, seed=82)
    with L.Model(files[name], n_ctx=N_CTX) as exact, L.Model(files[name], n_ctx=N_CTX, flags=L.FAST_ATTN) as fast:
        before = L.flash_attn_launches()
        for n in (1, 9, 63) + ((64, 130) if name == "head64" else ()):
            assert same(fast.eval_debug(p[:n], 0, 8, all_logits=True)["logits_all"], exact.eval_debug(p[:n], 0, 8, all_logits=True)["logits_all"]), f"{n} rows"
        for h in (exact, fast):
            h.eval(p[:63], 0, 8)
        a, la = exact.decode_greedy(int(p[5]), 63, 8, 8, want_logits=True)
        b, lb = fast.decode_greedy(int(p[5]), 63, 8, 8, want_logits=True)
        assert a.tolist() == b.tolist() and same(la, lb)
        assert L.flash_attn_launches() == before


def test_decode_behind_a_flagged_eval_is_deterministic(L, files):
    p = synth.synth_prompt(130, HP.n_vocab, seed=83)
    with L.Model(files["q4_0"], n_ctx=N_CTX, flags=L.FAST_ATTN) as fast:
        runs = []
        for _ in range(2):
            first = int(np.argmax(fast.eval(p, 0, 8)))
            runs.append(fast.decode_greedy(first, 130, 8, 8, want_logits=True))
        assert runs[0][0].tolist() == runs[1][0].tolist() and same(runs[0][1], runs[1][1])
        assert np.isfinite(runs[0][1]).all()


def test_eval_multi_falls_back_to_the_per_slot_loop(L, files):
    toks = [synth.synth_prompt(70, HP.n_vocab, seed=84), synth.synth_prompt(9, HP.n_vocab, seed=85)]
    with L.Model(files["q4_0"], n_ctx=N_CTX, n_seq=2, flags=L.FAST_ATTN) as hm, L.Model(files["q4_0"], n_ctx=N_CTX, n_seq=2, flags=L.FAST_ATTN) as hl:
        before = L.flash_attn_launches()
        lg = hm.eval_multi([1, 0], [0, 0], toks, chunk_tokens=9, n_threads=8)
        assert L.flash_attn_launches() - before == launches_of(L, 70)          # the 70-row segment took the fused kernel in a pass of its own
        for i, s in enumerate([1, 0]):
            hl.set_seq(s)
            assert same(lg[i], hl.eval_chunks(toks[i], 0, 9, 8)), f"segment {i}"
