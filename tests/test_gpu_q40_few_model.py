"""GPU (-m gpu): LLAMAHIP_FLAG_FAST_Q40_FEW on model handles, a 2-layer synthetic Q4_0 file of head size 128."""
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

HP = synth.HParams(n_vocab=256, n_embd=256, n_mult=64, n_head=2, n_layer=2)
N_CTX = 128
S = 16                          # KV slots = the widest set step
MM = 4 * HP.n_layer + 1         # mat-muls of an eval of all rows or a set step: wq|wk|wv, wo, w1|w3, w2 per layer + the lm head
# what -> (1 - min cosine, max |d logit|) against the EXACT handle, as measured on these inputs (12.39); asserted at ten times
MEASURED = {"eval17": (1.454e-14, 2.980e-07), "set16": (1.266e-14, 1.788e-07)}

def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))

def logits(h, p, nth=8):
    return h.eval_debug(p, 0, nth, all_logits=True)["logits_all"]

def prompt(s):
    return synth.synth_prompt(5 + s % 5, HP.n_vocab, seed=400 + s)

def set_step(m, seqs, nth):
    """every slot of seqs evaluates prompt(slot), then one set step on a fixed token per slot; the rows' logits in the order of seqs"""
    import torch
    bufs = []
    for s in seqs:
        m.set_seq(s)
        m.eval(prompt(s), 0, nth)
        bufs.append(torch.tensor([(7 * s + 3) % HP.n_vocab], dtype=torch.int32, device="cuda"))
        m.stage_bind(s, len(prompt(s)), token_in=bufs[-1].data_ptr(), token_out=bufs[-1].data_ptr())
    m.set_seq(0)
    m.stage_step_set(list(seqs), nth, torch.cuda.current_stream().cuda_stream)
    return np.stack([m.stage_logits(i) for i in range(len(seqs))])

def close(got32, want32, what):
    got, want = got32.astype(np.float64), want32.astype(np.float64)
    assert np.isfinite(got).all()
    cos = (got * want).sum(1) / np.sqrt((got * got).sum(1) * (want * want).sum(1))
    print(f"{what}: 1 - min cosine = {1.0 - cos.min():.3e}, max |d logit| = {np.abs(got - want).max():.3e}")
    floor_cos, floor_d = MEASURED[what]
    assert 1.0 - cos.min() <= 10 * floor_cos and np.abs(got - want).max() <= 10 * floor_d
    assert not same(got32, want32), f"{what}: bit-equal to the exact handle -- the flag had no effect"

@pytest.fixture(scope="module")
def path(tmp_path_factory):
    p = os.path.join(str(tmp_path_factory.mktemp("q40_few")), "q4_0.bin")
    synth.write_model(p, HP, synth.random_tensors(HP, seed=3901))
    return p

def test_a_flagged_handle_runs_the_few_kernel_and_stays_close(L, path):
    """The handle's gate is 16 .. 63 rows (2 .. 15 went back to the exact kernels): a 17-row eval and a set step of 16, with a
    9-row eval and the slots' prompts of 5 .. 9 rows staying exact."""
    p = synth.synth_prompt(17, HP.n_vocab, seed=94)
    with L.Model(path, n_ctx=N_CTX, n_seq=S) as exact, L.Model(path, n_ctx=N_CTX, n_seq=S, flags=L.FAST_Q40_FEW) as few:
        before = L.q40_few_launches()
        assert same(logits(few, p[:9]), logits(exact, p[:9]))
        want, want_set = logits(exact, p), set_step(exact, range(S), 8)
        assert L.q40_few_launches() == before, "flag 0, or fewer than 16 rows, took the few-row kernel"
        got = logits(few, p)
        assert L.q40_few_launches() - before == MM
        close(got, want, "eval17")
        got = set_step(few, range(S), 8)
        assert L.q40_few_launches() - before == 2 * MM
        close(got, want_set, "set16")

def test_a_row_does_not_depend_on_the_rows_of_its_eval(L, path):
    """Row independence through the whole pass, between two row counts the gate both sends to the kernel (a set of 2 no longer is one): rows
    0 .. 16 of a 33-row eval against the 17-row eval (NT 3 against NT 2; causal attention: a row sees the rows before it alone).  n_threads
    1: with more the reference's soft_max . V splits a row's keys by thread and by the rows of the eval"""
    p = synth.synth_prompt(33, HP.n_vocab, seed=95)
    with L.Model(path, n_ctx=N_CTX, flags=L.FAST_Q40_FEW) as a, L.Model(path, n_ctx=N_CTX, flags=L.FAST_Q40_FEW) as b:
        assert same(logits(a, p, 1)[:17], logits(b, p[:17], 1))

def test_evals_of_64_rows_and_the_single_token_step_go_where_they_went(L, path, others=0):
    p = synth.synth_prompt(70, HP.n_vocab, seed=96)
    with L.Model(path, n_ctx=N_CTX, flags=others) as ref, L.Model(path, n_ctx=N_CTX, flags=others | L.FAST_Q40_FEW) as flagged:
        before = L.q40_few_launches()
        for n in (70, 64):
            assert same(logits(flagged, p[:n]), logits(ref, p[:n])), f"{n} rows"
        assert same(flagged.decode_greedy(int(p[64]), 64, 6, 8, want_logits=True)[1], ref.decode_greedy(int(p[64]), 64, 6, 8, want_logits=True)[1])
        assert L.q40_few_launches() == before
