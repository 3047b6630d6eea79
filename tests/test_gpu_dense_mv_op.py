"""GPU (-m gpu): the one-row f16 / f32 mat-vec k_dense_mv alone (llamahip_op_mul_mat_dense, path MV) against the yardstick of
tests/dense_cases.py -- 32 fmaf chains per output and the reference's fold (orc_vec_dot_f32), the activations rounded to fp16 once where
the weights are fp16 -- which tests/test_dense_op_host.py holds against the reference build's own mat-mul for every case run here.
k_dense_mv is the oracle of tests/test_gpu_dense_set_op.py and tests/test_gpu_dense_mfma_op.py: this module is what anchors them.

Comparison rule: finite outputs bit for bit (the arithmetic and its order are the reference's: no tolerance), non-finite ones by class.
Per case: y rows lie M + 8 apart and the guard columns keep a bit pattern no kernel writes; path_taken is MV; the STORE and the RESID
epilogue both run.  K walks the loop's structure and M the row edges (dense_cases.MV_KS / MV_MS: the tail group alone, leftover groups
without a pipelined pass, one double batch exactly with its clamped prefetch, ..., both sides of the switch from 4 to 8 half-waves per
workgroup); the value regimes run at M 40, K 1344 (dense_cases.MV_REGIMES: signed zeros, subnormals and exact cancellation, fp16 rounding
ties of both parities, 65519 / +-65520 against zero weights, the bottom of fp16, fp32 products that underflow)."""
import numpy as np
import pytest

import dense_cases as dc

pytestmark = pytest.mark.gpu
GUARD_BITS = np.uint32(0x7FC0CAFE)          # (a NaN payload no arithmetic produces)


def run_case(L, oracle, case):
    wtype, K, M, N, regime = case
    w, x, resid = dc.mv_build(case)
    for r in (None, resid):
        tag = f"{dc.mv_id(case)} {'RESID' if r is not None else 'STORE'}"
        want = dc.yardstick(oracle, w, x, r, wtype)
        y_init = np.full((N, M + dc.GUARD), GUARD_BITS, np.uint32).view(np.float32)
        y, taken = L.op_mul_mat_dense(w, x, r, path="mv", y_stride=M + dc.GUARD, y_init=y_init)
        assert taken == "mv", f"{tag}: ran {taken}"
        assert y.shape == (N, M + dc.GUARD)
        assert np.all(y[:, M:].view(np.uint32) == GUARD_BITS), f"{tag}: guard columns written"
        assert np.all(y[:, :M].view(np.uint32) != GUARD_BITS), f"{tag}: an output left unwritten"
        assert not len(dc.differ(y[:, :M], want)), f"{tag}: {dc.first_diff(y[:, :M], want)}"


@pytest.mark.parametrize("K", dc.MV_KS)
@pytest.mark.parametrize("wtype", [1, 0], ids=["f16", "f32"])
def test_mv_equals_the_yardstick(L, oracle, wtype, K):
    cases = [c for c in dc.MV_CASES if c[0] == wtype and c[1] == K and c[4] == "gauss"]
    assert {c[2] for c in cases} >= set(dc.mv_ms(K)) and (K != dc.BASE["K"] or dc.base_case(wtype) in cases)
    before = L.dense_paths()["mv"]
    for c in cases:
        run_case(L, oracle, c)
    assert L.dense_paths()["mv"] - before == sum(2 * c[3] for c in cases)          # one launch of k_dense_mv per row and epilogue


@pytest.mark.parametrize("wtype,regime", [(wt, r) for wt in (1, 0) for r in dc.regimes_for(wt) if r != "gauss"],
                         ids=lambda v: dc.WNAMES[v] if isinstance(v, int) else v)
def test_value_regimes(L, oracle, wtype, regime):
    run_case(L, oracle, next(c for c in dc.MV_CASES if c[0] == wtype and c[4] == regime))
