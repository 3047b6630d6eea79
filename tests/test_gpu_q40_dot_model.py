"""GPU (-m gpu): llamahip_opts.fast_decode = 1 on model handles, a 2-layer synthetic Q4_0 file of head size 128 (d 256: wo 256 x 256, one
chunk under eight slices; w2 256 x 704, a ragged third chunk)."""
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

HP = synth.HParams(n_vocab=256, n_embd=256, n_mult=64, n_head=2, n_layer=2)
N_CTX = 128
STEPS = 6
NO_GRAPH, UNFUSED = 1, 2
# 1 - min cosine of the logits over 32 decoded positions, fast_decode against the exact handle, as measured on these inputs (12.40);
# asserted at 100 times (12.36's margin: flipped 4-bit codes downstream amplify rounding, no bound can be derived)
MEASURED_COS = 1.654e-14

def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))

@pytest.fixture(scope="module")
def files(L, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("q40_dot"))
    t = synth.random_tensors(HP, seed=4001)
    out = {name: os.path.join(d, name + ".bin") for name in ("q4_0", "f16", "q4_1")}
    synth.write_model(out["q4_0"], HP, t)
    synth.write_model_unquantized(out["f16"], HP, t, 1)
    L.quantize_file(out["f16"], out["q4_1"], 3)
    return out

PROMPT = synth.synth_prompt(9, HP.n_vocab, seed=97)

def greedy(m, steps=STEPS):
    m.eval(PROMPT[:-1], 0)
    return m.decode_greedy(int(PROMPT[-1]), len(PROMPT) - 1, steps, want_logits=True)

def test_the_handle_runs_the_dot_kernel_whatever_launches_the_step(L, files):
    """the captured step, one-token llamahip_eval calls, NO_GRAPH and UNFUSED: 2 n_layer launches a step and the same bits"""
    with L.Model(files["q4_0"], n_ctx=N_CTX) as exact, L.Model(files["q4_0"], n_ctx=N_CTX, fast_decode=1) as fast:
        toks, logits = greedy(fast)
        assert L.q40_dot_launches(fast) == 2 * HP.n_layer * STEPS
        want_toks, want_logits = greedy(exact)
        assert L.q40_dot_launches(exact) == 0
        assert not same(logits, want_logits), "bit-equal to the exact handle -- the field had no effect"
        # the loop of one-token evals on the same handle
        fast.eval(PROMPT[:-1], 0)
        tok, loop = int(PROMPT[-1]), []
        for i in range(STEPS):
            row = fast.eval([tok], len(PROMPT) - 1 + i)
            tok = int(np.argmax(row))
            loop.append(tok)
        assert loop == list(toks) and same(row, logits)
        assert L.q40_dot_launches(fast) == 4 * HP.n_layer * STEPS
    for flags in (NO_GRAPH, UNFUSED):
        with L.Model(files["q4_0"], n_ctx=N_CTX, flags=flags, fast_decode=1) as other:
            t2, l2 = greedy(other)
            assert L.q40_dot_launches(other) == 2 * HP.n_layer * STEPS, flags
            assert list(t2) == list(toks) and same(l2, logits), flags

def test_everything_but_the_single_token_step_is_the_exact_handles(L, files):
    import torch
    p = synth.synth_prompt(9, HP.n_vocab, seed=98)
    def set_step(m):
        bufs = []
        for s in range(4):
            m.set_seq(s)
            m.eval(p[:5 + s], 0)
            bufs.append(torch.tensor([(7 * s + 3) % HP.n_vocab], dtype=torch.int32, device="cuda"))
            m.stage_bind(s, 5 + s, token_in=bufs[-1].data_ptr(), token_out=bufs[-1].data_ptr())
        m.set_seq(0)
        m.stage_step_set(list(range(4)), 8, torch.cuda.current_stream().cuda_stream)
        return np.stack([m.stage_logits(i) for i in range(4)])
    with L.Model(files["q4_0"], n_ctx=N_CTX, n_seq=4) as exact, L.Model(files["q4_0"], n_ctx=N_CTX, n_seq=4, fast_decode=1) as fast:
        assert same(fast.eval_debug(p, 0, 8, all_logits=True)["logits_all"], exact.eval_debug(p, 0, 8, all_logits=True)["logits_all"])
        assert same(fast.eval(p, 0), exact.eval(p, 0))
        assert same(set_step(fast), set_step(exact))
        assert L.q40_dot_launches(fast) == 0

@pytest.mark.parametrize("kind", ["f16", "q4_1"])
def test_other_file_types_ignore_the_field(L, files, kind):
    with L.Model(files[kind], n_ctx=N_CTX) as ref, L.Model(files[kind], n_ctx=N_CTX, fast_decode=1) as fast:
        (t0, l0), (t1, l1) = greedy(ref), greedy(fast)
        assert list(t0) == list(t1) and same(l0, l1) and L.q40_dot_launches(fast) == 0

def test_the_logits_stay_close_to_the_exact_handles(L, files):
    with L.Model(files["q4_0"], n_ctx=N_CTX) as exact, L.Model(files["q4_0"], n_ctx=N_CTX, fast_decode=1) as fast:
        toks = greedy(exact, 32)[0]
        seq = [int(PROMPT[-1])] + [int(t) for t in toks[:-1]]
        rows = []
        for m in (exact, fast):
            m.eval(PROMPT[:-1], 0)
            rows.append(np.stack([m.eval([t], len(PROMPT) - 1 + i) for i, t in enumerate(seq)]).astype(np.float64))
        want, got = rows
        assert np.isfinite(got).all()
        cos = (got * want).sum(1) / np.sqrt((got * got).sum(1) * (want * want).sum(1))
        print(f"1 - min cosine over {len(seq)} positions = {1.0 - cos.min():.3e}, max |d logit| = {np.abs(got - want).max():.3e}")
        assert 1.0 - cos.min() <= 100 * MEASURED_COS
