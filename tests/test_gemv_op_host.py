"""CPU: llamahip_op_gemv_q4_0 is exported and refuses, before it looks for a device, every pair it must not launch and every bad shape,
count or operand, each naming its limit.  Also the CPU half of tests/test_gpu_gemv_op.py: the case table (tests/gemv_cases.py) reaches every
kernel instance the plan table names for the nine untagged pairs, every NORM row is order-proof under both forms of the second moment,
the weight matrices hold what they must, and the one-pass order-proof check rejects what it should."""
import numpy as np
import pytest

import gemv_cases as gc
import prep_cases as pc


def test_new_symbol_is_exported(L):
    assert "llamahip_op_gemv_q4_0" in L.declared_symbols() and hasattr(L.lib(), "llamahip_op_gemv_q4_0")


def gemv(L, M=64, K=64, pre="qa", epi="store", in0=True, in1=None, resid=None, **kw):
    w = np.zeros((M, max(K, 0) // 32, 20), np.uint8)
    vec = lambda v, n: None if v is None or v is False else np.zeros(n, np.float32)
    return L.op_gemv_q4_0(w, pre, epi, vec(in0, max(K, 0)), vec(in1, max(K, 0)), vec(resid, M), **kw)


PARTS = np.zeros((600, 2))


@pytest.mark.parametrize("kw,msg", [
    (dict(pre=6), "PREP_NORM_TAG waits on other launches"), (dict(epi=4), "EPI_STORE_TAG waits"), (dict(epi=5), "EPI_RESID_TAG waits"),
    (dict(pre="norm", in1=True, epi=6), "EPI_STORE_PICK waits"), (dict(pre="norm", in1=True, epi=7, interleaved=True), "EPI_SILU_QAH waits"),
    (dict(pre=4), "PREP_NORMP is pre NORM with part_in"), (dict(pre=5), "unknown prologue 5"), (dict(pre=-1), "unknown prologue -1"),
    (dict(epi=3), "unknown epilogue 3"), (dict(epi=8), "unknown epilogue 8"),
    (dict(K=0), "K 0 must be a positive multiple of 64"), (dict(K=96), "K 96 must be a positive multiple of 64"),
    (dict(M=96, interleaved=True, pre="norm", in1=True, epi="silu_qa"), "M = 2F = 96 is not a multiple of 64"),
    (dict(in0=None), "null operand .w, in0."), (dict(pre="norm"), "null operand .w, in0, in1."), (dict(pre="silu_mul", epi="resid", resid=True), "null operand .w, in0, in1."),
    (dict(epi="resid"), "EPI_RESID needs resid"), (dict(want_y=False), "y is NULL"), (dict(y_init=np.zeros(63)), "y_floats 63 < the 64 outputs"),
    (dict(pre="norm", in1=True, epi="silu_qa", interleaved=True, out_rows=0), "out_rows 0 >= 1"),
    (dict(part_in=PARTS[:4]), "part_in is the NORM prologue's"),
    (dict(pre="norm", in1=True, part_in=PARTS[:1], n_part_in=0), "n_part_in 0 outside 1 .. 512"),
    (dict(pre="norm", in1=True, part_in=PARTS[:513]), "n_part_in 513 outside 1 .. 512 .NORM_PART_MAX."),
    (dict(part_out=PARTS[:8]), "part_out is the RESID epilogue's"),
    (dict(epi="resid", resid=True, part_out=PARTS[:9], n_part_out=7), "part_out takes 8 pairs .* got 7 in a buffer of 9"),
    (dict(epi="resid", resid=True, part_out=PARTS[:9]), "part_out takes 8 pairs .* got 9 in a buffer of 9"),
    (dict(M=16397, epi="resid", resid=True, part_out=PARTS[:513]), "part_out takes 513 pairs .*at most 512 .NORM_PART_MAX."),
    # pairs and shapes gemv_plan_has_kernel refuses: no such pair; SILU_QA on a plain matrix; a row wider than the prologue's registers
    (dict(pre="plain"), "no instance for prologue 1, epilogue 0"), (dict(pre="silu_mul", in1=True), "no instance for prologue 3, epilogue 0"),
    (dict(pre="norm", in1=True, epi="resid", resid=True), "no instance for prologue 2, epilogue 1"),
    (dict(pre="norm", in1=True, epi="silu_qa"), "no instance for prologue 2, epilogue 2 on M 64, K 64 .plan: 0 waves"),
    (dict(pre="norm", in1=True, K=8256), "no instance for prologue 2, epilogue 0 on M 64, K 8256"),
    (dict(pre="plain", epi="resid", resid=True, K=8256), "no instance for prologue 1, epilogue 1 on M 64, K 8256"),
    (dict(pre="norm", in1=True, epi="silu_qa", interleaved=True, K=8256), "no instance for prologue 2, epilogue 2 on M 64, K 8256 interleaved"),
    (dict(K=49216), "no instance for prologue 0, epilogue 0 on M 64, K 49216"),
    (dict(pre="silu_mul", in1=True, epi="resid", resid=True, K=32768), "K 32768 needs .* bytes of LDS, the kernels' cap is 163840"),
])
def test_refusals_need_no_device(L, kw, msg):
    with pytest.raises(L.LlamaHipError, match=msg):
        gemv(L, **kw)


def test_good_arguments_pass_every_host_check_and_report_the_plan(L):
    """the limits themselves are accepted: what stops these calls on a machine without a GPU is the device check, nothing earlier"""
    for kw in (dict(), dict(epi="resid", resid=True, part_out=PARTS[:12], n_part_out=8), dict(pre="norm", in1=True, part_in=PARTS[:512]),
               dict(pre="norm", in1=True, epi="silu_qa", interleaved=True, want_y=False), dict(pre="silu_mul", in1=True, epi="resid", resid=True, K=24640),
               dict(K=49152), dict(pre="plain", epi="resid", resid=True, K=8192), dict(M=1)):
        try:
            gemv(L, **kw)
        except L.LlamaHipError as e:
            assert "no HIP device available" in str(e), kw


def test_the_case_table_reaches_every_instance_of_the_nine_pairs(L):
    """the set difference between the instances the plan table names and the instances the GPU cases launch is empty; INSTANCES is what
    the walk finds today; every case of the table has a kernel"""
    reached = set()
    for c in gc.CASES:
        pre, epi, inter, _, _ = gc.PAIRS[c.pair]
        p = L.gemv_plan(c.M, c.K, pre, epi, inter)
        assert p is not None, gc.case_id(c)
        assert not c.part_out or p[4] <= gc.NORM_PART_MAX, gc.case_id(c)
        reached.add((pre, epi) + p[:4])
    want = gc.golden_instances()
    assert len(want) >= 79 and {k[:2] for k in want} == set(gc.PAIR_OF)
    assert want - reached == set(), sorted(want - reached)
    assert gc.find_instances(L) == sorted(gc.INSTANCES)
    assert max(M * (K // 32) * 20 for *_, M, K in gc.INSTANCES) <= 43 << 20
    ids = [gc.case_id(c) for c in gc.CASES]
    assert len(set(ids)) == len(ids)


def test_the_row_edges_leave_partly_valid_workgroups(L):
    """what the row-edge cases are for: dead rows in the last row-group, dead waves in the last workgroup"""
    for M, nw, groups in ((4099, 2, 513), (8203, 4, 1026), (16397, 4, 2050)):
        p = L.gemv_plan(M, 320, 0, 1)
        assert M % 8 in (3, 5) and (M + 7) // 8 == groups and p[0] == nw and groups % nw != 0 and p[4] == (groups + nw - 1) // nw, (M, p)
    assert L.gemv_plan(4160, 4160, 0, 0)[3] == 1 and L.gemv_plan(13, 320, 0, 0)[3] == 0          # the ring K, a whole-row K


def test_every_norm_row_is_order_proof_under_both_forms():
    rows = sorted({(c.K, c.regime) for c in gc.CASES if c.pair.startswith("norm")})
    assert len(rows) >= 30 and gc.find_norm_attempts(gc.CASES) == gc.NORM_ROW_ATTEMPTS
    for K, regime in rows:
        x = gc.norm_row(K, regime)
        assert pc.norm_stats(x)["proof"] and pc.one_pass_stats(x)["proof"], (K, regime)
        if regime.startswith("dc:"):          # 0.56 and 0.60 sigma straddle the kernel's switch, in every summation order
            o = pc.one_pass_stats(x)
            assert (o["fast_certain"] and o["scale_ok"]) if float(regime[3:]) < 0.577 else not o["fast_possible"], (K, regime, o)
    assert not pc.one_pass_stats(gc.norm_row(4096, "offset"))["fast_possible"] and pc.one_pass_stats(gc.norm_row(4096, "zeros:1"))["scale_ok"]


def test_the_one_pass_check_rejects_what_it_should():
    """not vacuous: the cancelling row fails the pair of checks (its mean is what depends on the order: the one-pass interval alone, relative
    to a second moment of 1.6e17, is narrow); a row whose mean dominates by 1e4 sigma has a one-pass interval that does NOT resolve the
    scale -- and is proved all the same, because no order can take the one-pass form on it; the interval always holds the exact second
    moment and what plain double arithmetic gives in three orders"""
    assert not pc.norm_proof_both(pc.cancel_row(np.random.default_rng(3)))
    off = pc.one_pass_stats((1e4 + np.random.default_rng(1).standard_normal(4096)).astype(np.float32))
    assert not off["scale_ok"] and not off["fast_possible"] and off["proof"]
    for a in range(8):
        x = (0.5 + np.random.default_rng([4, a]).standard_normal(640)).astype(np.float32)
        o, q = pc.one_pass_stats(x), pc.norm_stats(x)["q"]
        assert o["lo"] <= q <= o["hi"] and o["hi"] - o["lo"] < 1e-9 * q
        # the one-pass form in plain double arithmetic, in two different orders, lands inside the interval
        xd = x.astype(np.float64)
        for order in (xd, xd[::-1], np.sort(xd)):
            S1, S2 = 0.0, 0.0
            for v in order:
                S1 += v
                S2 += v * v
            assert o["lo"] <= S2 - (S1 / x.size) * S1 <= o["hi"]


def test_the_weight_matrices_hold_a_zero_scale_and_the_extreme_codes():
    shapes = sorted({(c.M, c.K, c.wkind) for c in gc.CASES} | {(1024, 64, "plain"), (4096, 64, "plain"), (24, 1024, "plain"), (24, 4096, "plain")})
    for M, K, wkind in shapes:
        if M * K > (1 << 22) and (M, K) not in ((16384, 4160), (16397, 4160)):          # (the largest two stand for the large ones: same generator)
            continue
        assert all(gc.weight_properties(gc.weights(M, K, wkind))), (M, K, wkind)
    z = gc.weights(24, 320, "zero_group")
    assert not np.ascontiguousarray(z[8:16, :, :4]).view(np.float32).any() and np.ascontiguousarray(z[:8, :, :4]).view(np.float32).any()
    s = gc.weights(448, 320, "silu_zero")
    assert not np.ascontiguousarray(s[:32, :, :4]).view(np.float32).any() and not np.ascontiguousarray(s[224 + 32:224 + 64, :, :4]).view(np.float32).any()


def test_the_references_of_the_edge_cases_are_what_the_cases_claim(oracle):
    """the CPU half of the epilogue-edge and SiLU cases: zero-weight rows give +0 in the oracle, the gates span about +-12, the SiLU edge
    rows are finite, and the residual row the parts are fed back from is order-proof"""
    for c in gc.CASES:
        if c.wkind == "zero_group":
            ops = gc.build(oracle, c)
            assert np.all(gc.reference(oracle, c, dict(ops, resid=np.zeros(c.M, np.float32)))["y"][8:16].view(np.uint32) == 0), gc.case_id(c)
        if c.wkind == "silu_zero":
            want = gc.reference(oracle, c, gc.build(oracle, c))
            g = want["gate"][64:]
            assert g.min() < -8 and g.max() > 8 and np.abs(g).max() < 24, (gc.case_id(c), g.min(), g.max())
            assert not want["out_d"][:2].any() and np.all(want["out_d"][2:7] > 0) and want["out_d"][7] == 0
        if c.regime == "silu_edges":
            ops = gc.build(oracle, c)
            want = gc.reference(oracle, c, ops)
            assert np.all(np.isfinite(want["row"])) and np.all(np.isfinite(want["y"])) and (ops["in0"] == 65504.0).any(), gc.case_id(c)
    for M in (1024, 4096):
        c = gc.Case("feed", "qa.resid", M, 64, "plain", "normal:1", 0, True)
        assert pc.norm_proof_both(gc.reference(oracle, c, gc.build(oracle, c))["y"]), M
