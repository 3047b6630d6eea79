"""GPU (-m gpu): the producers of an f16 / f32 mat-mul's activation operand, op by op (llamahip_op_dense_prep): the fused k_dense_prep in its
three modes and the split path -- launch_prep's fp32 rows, then k_dense_perm_act -- that NORM rows wider than 16384 take.

Every case of prep_cases.CASES (the K values at which the thread layouts change, the strided and model layouts with poison between the
rows) runs for both weight types on every producer that takes the shape -- AUTO, FUSED, SPLIT -- and asserts
  1. the operand equals act(prep_cases.reference(oracle, mode, x, b)[0], wtype) scattered by dense_cases.perm_index (a numpy statement of
     the chain-major order): finite values bit for bit, non-finite ones by class;
  2. every float of [N][K] was written and the 64 guard floats behind them were not;
  3. kernel_taken follows the model's rule (FUSED unless a NORM row has K / 16 > 1024), and FUSED is refused there;
  4. FUSED and SPLIT leave the same operand wherever both run.
NORM rows are prep_cases' order-proof rows (asserted for every row used), so the reduction tree excuses nothing.

f16_double_rounding (dense_cases.dr_build; f16 weights): rows with 64 and more elements whose fp32 product lies exactly half way between
two fp16 values although the exact product does not, with the tie going the other way.  The reference rounds twice (ggml_mul to fp32, the
mat-mul's INIT phase to fp16); a compiler that folds `(_Float16) (a * b)` into one rounding of the exact product gets exactly these
elements wrong.  k_dense_prep fences its fp32 products with an empty `asm volatile` against that: this case fails without the fence."""
import numpy as np
import pytest

import dense_cases as dc
import prep_cases as pc

pytestmark = pytest.mark.gpu
FILL = np.uint32(0xFFFFFFFF)


def run_producers(L, mode, wtype, x, b, layout, want, tag):
    """every producer that takes the shape against `want` [N, K] (logical order); returns {kernel asked for: operand bits}"""
    N, K = x.shape
    buf, kw = pc.lay_out(mode, x, b, layout)
    want_p = dc.permute_rows(want)
    out = {}
    for kernel, expect in dc.prep_kernels_for(mode, K):
        t = f"{tag} {dc.WNAMES[wtype]} kernel={kernel}"
        xp, taken = L.op_dense_prep(mode, wtype, buf, K, N, kernel=kernel, **kw)
        assert taken == expect, f"{t}: ran {taken}, the model's rule says {expect}"
        assert xp.size == N * K + 64
        bits = xp.view(np.uint32)
        assert np.all(bits[N * K:] == FILL), f"{t}: guard floats written at {np.flatnonzero(bits[N * K:] != FILL)[:4]}"
        assert np.all(bits[:N * K] != FILL), f"{t}: floats {np.flatnonzero(bits[:N * K] == FILL)[:4]} of the operand never written"
        got = xp[:N * K].reshape(N, K)
        assert not len(dc.differ(got, want_p)), f"{t}: operand (permuted order): {dc.first_diff(got, want_p)}"
        out[kernel] = bits[:N * K].copy()
    if "fused" in out:
        same = out["fused"] == out["split"]
        nan = np.isnan(out["fused"].view(np.float32)) & np.isnan(out["split"].view(np.float32))
        assert np.all(same | nan), f"{tag} {dc.WNAMES[wtype]}: FUSED and SPLIT differ at {np.flatnonzero(~(same | nan))[:4]}"
    return out


@pytest.mark.parametrize("wtype", [1, 0], ids=["f16", "f32"])
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_dense_prep(L, oracle, case, wtype):
    mode, K, N, regime, layout = case
    x, b = pc.build(oracle, mode, K, N, regime)
    if mode == "norm":          # a condition on the INPUTS: with it, no summation order can change a float (no row is excused)
        proof = [pc.norm_stats(r)["proof"] for r in x]
        assert all(proof), f"rows {np.flatnonzero(~np.array(proof))} are not order-proof"
    y, _ = pc.reference(oracle, mode, x, b)
    out = run_producers(L, mode, wtype, x, b, layout, dc.act(y, wtype), pc.case_id(case))
    if mode == "norm" and K // 16 > 1024:
        assert set(out) == {"auto", "split"}
        buf, kw = pc.lay_out(mode, x, b, layout)
        with pytest.raises(L.LlamaHipError, match=f"FUSED .k_dense_prep. refused for NORM with K {K}"):
            L.op_dense_prep(mode, wtype, buf, K, N, kernel="fused", **kw)
    else:
        assert set(out) == {"auto", "fused", "split"}


@pytest.mark.parametrize("case", dc.DR_CASES, ids=pc.case_id)
def test_f16_double_rounding(L, oracle, case):
    mode, K, N, _, layout = case
    x, b, mask = dc.dr_build(oracle, mode, K, N)
    first = oracle.unary_rows("silu" if mode == "silu_mul" else "norm", x)
    hit = dc.rounds_twice(first, b if mode == "silu_mul" else np.broadcast_to(b, x.shape)) & mask
    assert (hit.sum(axis=1) >= dc.DR_MIN_PER_ROW).all()
    if mode == "norm":
        assert all(pc.norm_stats(r)["proof"] for r in x)
    y, _ = pc.reference(oracle, mode, x, b)
    run_producers(L, mode, 1, x, b, layout, dc.act(y, 1), pc.case_id(case))
