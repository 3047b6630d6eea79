"""GPU: the few-row Q4_0 mat-mul k_gemv_set, one launch per case through llamahip_op_gemv_set_q4_0 (two with x_prev), against the oracle bit
for bit (uint32, so signed zeros count).  The cases, their inputs and what each group is for: tests/gemv_set_cases.py; the CPU half (the
refusals, the coverage tables, the conditions on the inputs, what the yardstick can see): tests/test_gemv_set_op_host.py.

Every reference is what the suite already trusts:
  STORE     oracle.mul_mat_q4_0(w, x)
  RESID     that plus ONE fp32 add of the residual (a zero-weight row-group under residuals of -0, +0, +-inf; no NaN residual)
  ROPE_KV   acc = oracle.mul_mat_q4_0; qr and the K rows = oracle.rope of acc's q and k parts at the rows' positions, the V rows copied; the
            caches start as CANARY NaNs and are compared WHOLE: only the N written rows may differ from the fill
  SILU_*    prep_cases.reference("silu_mul", gate, up) of acc's two halves, prep_cases.pack_qa; out_A / out_d compared word for word, the
            blocks that pad F still zero, the rows from N on still 0xFFFFFFFF; SILU_QAH's fault word 0.  Both epilogues run the same x
            against the same reference wherever both run, so they agree word for word.
and, for STORE / RESID, the exact-path float64 bound of tests/gemm_ref.py (gamma_{n+4} sum |w| |x|): the project's tolerance, not this
kernel's.  The plan the op reports is the one asked for (forced cases: set_launch_shape's arithmetic restated in gemv_set_cases) or the
one llamahip_debug_set_plan answers (auto cases)."""
import numpy as np
import pytest

import gemv_set_cases as sc
from gemm_ref import Ref

pytestmark = pytest.mark.gpu


def first_diff(name, got, want):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    d = np.argwhere(g != w)
    if d.size == 0:
        return None
    i = tuple(int(v) for v in d[0])
    return f"{name}: {len(d)} of {g.size} words differ; first at {i}: got 0x{int(g[i]):08x} want 0x{int(w[i]):08x}"


def check_plan(L, c, plan):
    nc, cw, ncg, rgw, lds, grid, threads = plan
    assert 0 < lds <= sc.LDS_CAP, plan
    if c.force:
        assert (nc, cw, ncg, rgw, grid, threads) == sc.expected_forced_plan(c), (plan, sc.expected_forced_plan(c))
    else:
        assert plan[:5] == L.set_plan(c.M, c.K, c.N, sc.EPI[c.epi], c.epi.startswith("silu")), plan
        assert threads == rgw * cw * 64 and ncg == -(-c.N // (nc * cw))


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_gemv_set_case(L, oracle, c):
    ops, want = sc.build(oracle, c)
    w, x = ops.pop("w"), ops.pop("x")
    r = L.op_gemv_set_q4_0(w, x=x, **ops)
    check_plan(L, c, r["plan"])
    tag = sc.case_id(c) + f" plan {r['plan']}"
    if c.epi in ("store", "resid"):
        y = r["y"]
        assert first_diff("y past M", y[:, c.M:], want["y_pad"]) is None, tag + ": a float outside the N x M block was written"
        bad = first_diff("y (row, column)", y[:, :c.M], want["y"])
        assert bad is None, f"{tag}: {bad}"
        ref = Ref(oracle, w, x, ops.get("resid"))
        fin = np.isfinite(want["y"])
        with np.errstate(invalid="ignore"):          # (inf - inf under the +-inf residuals: those outputs are pinned by their bits alone)
            err, bound = ref.err(y[:, :c.M]), ref.bound_exact()
        assert np.all(err[fin] <= bound[fin]), f"{tag}: outside the float64 bound by {np.max(err[fin] - bound[fin]):.3e}"
    elif c.epi == "rope_kv":
        for name in ("qr", "Kc", "Vc"):
            bad = first_diff(name, r[name], want[name])
            assert bad is None, f"{tag}: {bad} (positions {want['pos'].tolist()}, slots {want['slot'].tolist()})"
        fill = np.count_nonzero(r["Kc"].view(np.uint32) == sc.CANARY)
        assert fill == r["Kc"].size - c.N * c.rope[0], f"{tag}: {fill} words of the K cache still hold the fill"
    else:
        assert sc.qah_condition(want["act"]) or c.N > sc.SET_MAX, tag
        if c.epi == "silu_qah":
            assert r["fault"] == 0, f"{tag}: fault word 0x{r['fault']:08x}"
        for name in ("out_d", "out_A"):
            bad = first_diff(name + " (row, word)", r[name], want[name])
            assert bad is None, f"{tag}: {bad}"
