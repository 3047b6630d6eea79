"""GPU: the fused wq|wk|wv + attention launch k_qkv_attn with its arguments in the hot blocks (AttnHot, GemvHot: decode.hip), one
llamahip_op_qkv_attn launch per case against the oracle with the inputs of tests/dec_attn_cases.py and the checks of
test_gpu_dec_attn_op.run_qkv: merged row, the wo operand, the K / V caches, the fault words, the plan.

The head count is the smallest the fused launch takes at its smallest width (d = 4096: H = 16, heads of 256; H = 8 has no plan), on
a context of two score slices, with and without the producer's norm statistics (the NORM and the NORMP prologue: the two kernels a
model's step launches).  Positions: 0 (no old key; one score workgroup per head does all the work), 31 and 32 -- the two sides of a
32-key score-slice boundary: at 31 the slice that owns the new key is the first and full, at 32 it is the second and holds that key
alone, and the workgroups of the slices behind it return at once."""
import pytest

import dec_attn_cases as dc
from test_gpu_dec_attn_op import run_qkv

pytestmark = pytest.mark.gpu

D, H, N_CTX = 4096, 16, 64
CASES = [dc.QkvCase("plain", D, H, N_CTX, n_past, nth, nparts) for n_past in (0, 31, 32) for nth, nparts in ((8, 0), (3, 64))]


@pytest.mark.parametrize("c", CASES, ids=dc.qkv_case_id)
def test_qkv_attn_entry(L, oracle, c):
    assert L.qkv_attn_plan(D, 8, N_CTX, c.nth, 0) is None, "H = 8 has a plan now: it is the smallest head count"
    w, norm_w, x, part_in, Kc, Vc, qkv = dc.qkv_inputs(oracle, c)
    plans = run_qkv(L, oracle, c.d, c.H, c.n_ctx, c.nth, 0, [(x, part_in, c.n_past, 0, 1)], Kc, Vc, w, norm_w, [qkv], [c.regime], dc.qkv_case_id(c))
    assert plans[0][0] == (4 if c.nparts else 2) and plans[0][1:3] == (8, 1)
