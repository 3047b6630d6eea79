"""GPU: the decode mat-vec k_gemv at the shapes where its ENTRY can go wrong -- the argument blocks (hot / cold) and the per-lane
predicates that replaced the prologue's trip counts -- one launch per case through llamahip_op_gemv_q4_0, against the oracle bit for
bit.  Cases, inputs and references are tests/gemv_cases.py's (Case, build, reference) and the checks are test_gpu_gemv_op.run_case's:
y, the canary behind y, out_A / out_d and the operand row behind them, part_out's pairs and the canary pairs behind them, the plan.
No case is excused.

  QA prologue, operand granules (16 B of the A array; 16 per chunk) against threads
      K = 256            16 granules under one wave: most threads idle
      K = 4096, M 4096   two waves, exactly two granules per thread
      K = 11008, M 4096  the 12-granule budget: 688 granules on 128 threads, a sixth pass that is partly filled
  fp32 prologues (NORM, NORMP, PLAIN), half-block granules (16 floats) against threads
      K = 64             four granules (the op takes K in multiples of 64 -- tests/test_gemv_op_host.py pins that refusal -- so K = 32,
                         two granules, cannot be launched through it; 64 is the smallest row it takes)
      K = 4096           exactly one per thread at four waves
      K = 5120           320 granules on 256 threads: a second pass that is partly filled
  waves and rows past the end
      M = 8200           1 025 row-groups: the last workgroup has one live wave (four-wave QA plan) / one live wave of two
      M = 8197           not a multiple of 8: the last row-group has five live rows
  epilogue arguments that now arrive at entry
      RESID with part_out (every RESID case above with a grid of at most 512 workgroups), SILU_QA at the smallest interleaved
      w1|w3 the plan takes (F = 32: one block)

The pairs that wait on other workgroups are not the op's to launch (it refuses them, pinned by tests/test_gemv_op_host.py): the pick
epilogue (the cold block) and the half-block w1|w3 run here inside the smallest model whose plan gives them a kernel --
test_pick_and_half_block_kernels_in_a_model."""
import numpy as np
import pytest

import gemv_cases as gc
import synth
from conftest import synth_tool
from test_gpu_gemv_op import run_case

pytestmark = pytest.mark.gpu


def _cases():
    out = []
    for M, K in ((24, 256), (4096, 4096), (4096, 11008)):
        out.append(gc.Case("entry", "qa.store", M, K, "plain", "normal:1", 0, False))
        out.append(gc.Case("entry", "qa.resid", M, K, "plain", "normal:1", 0, True))
    for K in (64, 4096, 5120):
        out.append(gc.Case("entry", "norm.store", 24, K, "plain", "normal:1", 0, False))
        out.append(gc.Case("entry", "normp.store", 24, K, "plain", "normal:1", 3, False))
        out.append(gc.Case("entry", "normp.store", 24, K, "plain", "normal:1", 65, False))
        out.append(gc.Case("entry", "plain.resid", 24, K, "plain", "normal:1", 0, True))
    for M in (8200, 8197):
        out.append(gc.Case("entry", "qa.store", M, 320, "plain", "normal:1", 0, False))
        out.append(gc.Case("entry", "qa.resid", M, 320, "plain", "normal:1", 0, True))          # 257 workgroups of four waves
        out.append(gc.Case("entry", "plain.resid", M, 320, "plain", "normal:1", 0, False))      # (513 workgroups of two waves: more than part_out takes)
        out.append(gc.Case("entry", "norm.store", M, 320, "plain", "normal:1", 0, False))
        out.append(gc.Case("entry", "normp.store", M, 320, "plain", "normal:1", 64, False))
    for pair, n in (("norm.silu_qa", 0), ("normp.silu_qa", 2), ("qa.silu_qa", 0)):
        out.append(gc.Case("entry", pair, 64, 64, "wide", "normal:1", n, False))
    return out


CASES = _cases()
# what the shapes are chosen for, pinned against the plan (host side): (waves, granules per thread, ring depth, ring)
PLANS = {("qa.resid", 24, 256): (1, 4, 16, 0), ("qa.resid", 4096, 4096): (2, 4, 16, 0), ("qa.resid", 4096, 11008): (2, 12, 10, 1),
         ("norm.store", 24, 64): (1, 1, 16, 0), ("norm.store", 24, 4096): (4, 1, 16, 0), ("norm.store", 24, 5120): (4, 2, 10, 1),
         ("qa.resid", 8200, 320): (4, 4, 16, 0), ("norm.store", 8200, 320): (2, 1, 16, 0), ("norm.silu_qa", 64, 64): (8, 1, 16, 0)}


@pytest.mark.parametrize("case", CASES, ids=gc.case_id)
def test_entry_shapes(L, oracle, case):
    _, _, r = run_case(L, oracle, case)
    want = PLANS.get((case.pair, case.M, case.K))
    assert want is None or r["plan"][:4] == want, (gc.case_id(case), r["plan"])


def test_pick_and_half_block_kernels_in_a_model(L, oracle, tmp_path):
    """The two default-schedule instances that take the cold block, at the smallest shapes their plans accept: the lm head's pick
    epilogue needs a four-wave ring (2 048 row-groups and a row of 16 chunks or more: M = 16 384, K = 4 096, the ring of 4; one
    chunk less and the whole row is in flight, which the pick has no instance for), the half-block w1|w3 a row of more than 4
    chunks on 2 048 row-groups or more where halves balance the CUs better than blocks (F = 12 288: 384 blocks on 256 CUs).  One
    layer of that width, greedy decode in the captured loop: every token is the pick epilogue's (its index against the oracle's
    logits in numpy: the largest, the lowest index), and every step after the first starts from the row the pick epilogue embedded,
    so tokens and last logits equal to the oracle's pin that row too."""
    kw = dict(n_vocab=16384, n_embd=4096, n_mult=12288, n_head=32, n_layer=1)
    assert L.gemv_plan(16384, 4096, 4, 6)[:4] == (4, 1, 4, 1) and L.gemv_plan(16384, 3840, 4, 6) is None
    assert L.gemv_plan(2 * 12288, 4096, 4, 7, True)[:4] == (4, 1, 4, 1)
    path = synth_tool(tmp_path / "pick.bin", seed=41, **kw)
    prompt = synth.synth_prompt(5, kw["n_vocab"], seed=4)
    om = oracle.load(path, 32)
    lo = om.eval(prompt, 0, 8)["logits"]
    with L.Model(path, n_ctx=32) as gm:
        a = gm.eval(prompt, 0, 8)
        assert np.array_equal(a.view(np.uint32), lo.view(np.uint32))
        t = first = int(np.argmax(lo))
        want = []
        for i in range(4):
            lo = om.eval(np.array([t], np.int32), 5 + i, 8)["logits"]
            t = int(np.flatnonzero(lo == lo.max())[0])
            want.append(t)
        got, last = gm.decode_greedy(first, 5, 4, 8, want_logits=True)
        assert got.tolist() == want, (got.tolist(), want)
        assert np.array_equal(last.view(np.uint32), lo.view(np.uint32))
    om.close()
