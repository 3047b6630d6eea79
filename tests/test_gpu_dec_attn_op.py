"""GPU: the one-row decode attention through the kernels that hand data between workgroups inside one launch -- k_dec_attn_x (per-head
counters), k_dec_pv_stream with its chains split over workgroups and k_dec_pv_dma (tagged partial sums) -- op by op
(llamahip_op_dec_attention), against the oracle bit for bit.

Each case appends the step's row to K / V caches whose later rows hold a NaN canary (tests/attn_cases.py) and asserts
  1. the plan that ran (kernel, split, chains per workgroup, rows per stage or ring slots, LDS, grid) is the one llamahip_debug_dec_attn_plan
     reports for the case -- a case meant for the DMA ring cannot pass quietly through the stream kernel;
  2. the merged row equals orc_attention's bit for bit (the sign of zero and NaN payloads count);
  3. both caches equal the oracle's after its append, every bit of them;
  4. the wo operand equals orc_quantize_row_q4_0 of the oracle's merged row byte for byte;
  5. the fault word is zero after every step;
  6. plain, wide and zeroq steps stay within the float64 bound of tests/attn_ref.py (test_gpu_attention.py derives it).
Sequences run several steps on ONE set of hand-off buffers that the op zeroes once: counters a launch must have cleared, granules that
hold an older tag, the epoch across its 24-bit wrap, the last layer index.  tests/dec_attn_cases.py says what each case is for;
tests/test_dec_attn_op_host.py checks on the CPU that every edge has its case and every regime input its property."""
import numpy as np
import pytest

import dec_attn_cases as dc
from attn_ref import f64_reference

pytestmark = pytest.mark.gpu


def describe(got, want, H):
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    bad = np.argwhere(gb != wb).ravel()
    if not len(bad):
        return "equal"
    c, dh = int(bad[0]), want.size // H
    return f"{len(bad)} elements differ; first: head {c // dh}, column {c % dh}: got {got[c]!r} ({gb[c]:#010x}), want {want[c]!r} ({wb[c]:#010x})"


def run(L, oracle, path, H, dh, n_ctx, nth, force, epoch0, regimes, steps, Kc, Vc, tag):
    d = H * dh
    ref, Kw, Vw = dc.reference(oracle, steps, Kc, Vc, H, nth)
    f = force or (0, 0, 0)
    want_plan = dc.case_plan(L, dc.Case(path, "plain", H, dh, n_ctx, 0, nth, force))
    assert want_plan is not None and want_plan.kernel == {"x": "attn_x", "stream": "pv_stream", "dma": "pv_dma"}[path], f"{tag}: plan {want_plan}"
    Kg, Vg = Kc.copy(), Vc.copy()
    merged, wo, fault, plan = L.op_dec_attention(path, steps, H, Kg, Vg, nth, force=dict(split=f[0], stage_rows=f[1], ns=f[2]), epoch0=epoch0)
    assert plan == want_plan, f"{tag}: ran {plan}, the plan is {want_plan}"
    assert f[0] in (0, plan.split) and f[1] in (0, plan.SR) and f[2] in (0, plan.NS), f"{tag}: forced {f}, ran {plan}"
    assert not fault.any(), f"{tag}: fault words {fault.tolist()}"
    for i, ((want, wo_want, qr, Ki, Vi), (_, n_past, layer, bump)) in enumerate(zip(ref, steps)):
        st = f"{tag} step {i} (n_past {n_past}, layer {layer}, bump {bump})"
        assert np.array_equal(merged[i].view(np.uint32), want.view(np.uint32)), f"{st}: merged: {describe(merged[i], want, H)}"
        assert np.array_equal(wo[i], wo_want), f"{st}: wo operand differs in block {np.argwhere(wo[i] != wo_want)[:1]}"
        if regimes[i] in ("plain", "wide", "zeroq"):
            ref64, bound, _ = f64_reference(qr, Ki, Vi, H, n_past, nth)
            err = np.abs(want.astype(np.float64) - ref64[0])
            assert np.all(err <= bound[0]), f"{st}: float64 bound exceeded at {np.argwhere(err > bound[0])[:3]}"
    for nm, got, exp in (("K", Kg, Kw), ("V", Vg, Vw)):
        bad = np.argwhere(got.view(np.uint32) != exp.view(np.uint32))
        assert not len(bad), f"{tag}: {nm} cache: {len(bad)} words differ, first at row {bad[0][0]} column {bad[0][1]}"
    return plan


def run_case(L, oracle, c):
    qkv, Kc, Vc = dc.first_inputs(c.regime, c.H, c.dh, c.n_ctx, c.n_past)
    return run(L, oracle, c.path, c.H, c.dh, c.n_ctx, c.nth, c.force, 0, [c.regime], [(qkv[0], c.n_past, 0, 1)], Kc, Vc, dc.case_id(c))


@pytest.mark.parametrize("c", dc.X_CASES, ids=dc.case_id)
def test_attn_x(L, oracle, c):
    run_case(L, oracle, c)


@pytest.mark.parametrize("c", dc.STREAM_CASES, ids=dc.case_id)
def test_pv_stream(L, oracle, c):
    run_case(L, oracle, c)


@pytest.mark.parametrize("c", dc.DMA_CASES, ids=dc.case_id)
def test_pv_dma(L, oracle, c):
    run_case(L, oracle, c)


@pytest.mark.parametrize("c", dc.REGIME_CASES, ids=dc.case_id)
def test_regimes(L, oracle, c):
    run_case(L, oracle, c)


@pytest.mark.parametrize("s", dc.SEQS, ids=dc.seq_id)
def test_steps_on_one_set_of_hand_off_buffers(L, oracle, s):
    steps, Kc, Vc = dc.seq_inputs(s)
    run(L, oracle, s.path, s.H, s.dh, s.n_ctx, s.nth, s.force, s.epoch0, [r for r, _, _, _ in s.steps], steps, Kc, Vc, dc.seq_id(s))


# ------------------------------------------------------------------------------------------------ the fused launch (k_qkv_attn)
def run_qkv(L, oracle, d, H, n_ctx, nth, epoch0, steps, Kc, Vc, w, norm_w, qkvs, regimes, tag):
    """steps: [(x, part_in, n_past, layer, bump)]; qkvs: the q|k|v row each step's mat-vec must produce (the oracle's)"""
    ref, Kw, Vw = dc.reference(oracle, [(q, s[2], s[3], s[4]) for q, s in zip(qkvs, steps)], Kc, Vc, H, nth)
    Kg, Vg = Kc.copy(), Vc.copy()
    merged, wo, fault, plans = L.op_qkv_attn(w, norm_w, steps, H, Kg, Vg, nth, epoch0=epoch0)
    for i, s in enumerate(steps):
        want_plan = L.qkv_attn_plan(d, H, n_ctx, nth, 0 if s[1] is None else len(s[1]))
        assert plans[i] == want_plan and want_plan[0] == (2 if s[1] is None else 4), f"{tag} step {i}: ran {plans[i]}, the plan is {want_plan}"
    assert not fault.any(), f"{tag}: fault words {fault.tolist()}"
    for i, ((want, wo_want, qr, Ki, Vi), s) in enumerate(zip(ref, steps)):
        st = f"{tag} step {i} (n_past {s[2]}, layer {s[3]}, bump {s[4]})"
        assert np.array_equal(merged[i].view(np.uint32), want.view(np.uint32)), f"{st}: merged: {describe(merged[i], want, H)}"
        assert np.array_equal(wo[i], wo_want), f"{st}: wo operand differs in block {np.argwhere(wo[i] != wo_want)[:1]}"
        if regimes[i] in ("plain", "wide", "zeroq"):
            ref64, bound, _ = f64_reference(qr, Ki, Vi, H, s[2], nth)
            err = np.abs(want.astype(np.float64) - ref64[0])
            assert np.all(err <= bound[0]), f"{st}: float64 bound exceeded at {np.argwhere(err > bound[0])[:3]}"
    for nm, got, exp in (("K", Kg, Kw), ("V", Vg, Vw)):
        bad = np.argwhere(got.view(np.uint32) != exp.view(np.uint32))
        assert not len(bad), f"{tag}: {nm} cache: {len(bad)} words differ, first at row {bad[0][0]} column {bad[0][1]}"
    return plans


@pytest.mark.parametrize("c", dc.QKV_CASES + dc.QKV_WIDE_CASES, ids=dc.qkv_case_id)
def test_qkv_attn(L, oracle, c):
    w, norm_w, x, part_in, Kc, Vc, qkv = dc.qkv_inputs(oracle, c)
    plans = run_qkv(L, oracle, c.d, c.H, c.n_ctx, c.nth, 0, [(x, part_in, c.n_past, 0, 1)], Kc, Vc, w, norm_w, [qkv], [c.regime], dc.qkv_case_id(c))
    assert plans[0][1:3] == {v[0]: k for k, v in dc.QKV_WIDTHS.items()}[c.d]


@pytest.mark.parametrize("s", dc.QKV_SEQS, ids=dc.qkv_seq_id)
def test_qkv_attn_steps_on_one_set_of_hand_off_buffers(L, oracle, s):
    w, norm_w = dc.qkv_weights(s.d), dc.gc.norm_weight(s.d)
    c0 = dc.QkvCase("plain", s.d, s.H, s.n_ctx, s.steps[0][0], s.nth, 0)
    _, _, _, _, Kc, Vc, _ = dc.qkv_inputs(oracle, c0)
    steps, qkvs = [], []
    for i, (n_past, layer, bump, nparts) in enumerate(s.steps):
        x = dc.qkv_x(s.d, i)
        steps.append((x, dc.gc.norm_parts(x, nparts) if nparts else None, n_past, layer, bump))
        qkvs.append(dc.qkv_row(oracle, w, x, norm_w))
    run_qkv(L, oracle, s.d, s.H, s.n_ctx, s.nth, s.epoch0, steps, Kc, Vc, w, norm_w, qkvs, ["plain"] * len(steps), dc.qkv_seq_id(s))
