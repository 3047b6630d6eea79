"""GPU: the single-row decode mat-vec k_gemv, one launch per case through llamahip_op_gemv_q4_0, against the oracle bit for bit (uint32).

The cases are tests/gemv_cases.py's: one per kernel instance the plan table names for the nine untagged (prologue, epilogue) pairs, row
counts that are no multiple of 8 or of the workgroup, the value regimes of the quantizer's edges through the FUSED prologues, and the
epilogue's edges.  References, all from what the suite already trusts:
  QA/STORE                    oracle.mul_mat_q4_0(w, x)
  QA/RESID, PLAIN/RESID       that plus ONE fp32 add of resid
  NORM/STORE, NORMP/STORE     prep_cases.reference("norm", x, w_norm)'s fp32 row through oracle.mul_mat_q4_0
  SILU_MUL/RESID              prep_cases.reference("silu_mul", gate, up)'s row through oracle.mul_mat_q4_0, plus resid
  (NORM, NORMP, QA)/SILU_QA   gate and up rows from the w1 and w3 halves as above, then prep_cases.reference("silu_mul", gate, up): y against
                              its fp32 row, out_A / out_d against prep_cases.pack_qa of its blocks
Every case also asserts: the plan the op reports is L.gemv_plan's; the floats of y past the outputs keep a canary; out_A / out_d of a
padded last chunk are zero and the operand row behind the one written keeps its fill; part_out's pairs are the sums of their
workgroup's nw * 8 outputs -- |s1 - fsum(y)| <= gamma(nw * 8) sum|y| and likewise for the squares: the y are fp32, so every term is exact
in double and only the additions round -- and the pairs past the grid are untouched.
Every NORM / NORMP row is order-proof under both forms of the second moment (prep_cases.norm_proof_both: asserted on the inputs, no row
excused), so the one-pass branch, the two-pass branch and the folded partial sums must all give the oracle's bits."""
import math

import numpy as np
import pytest

import gemv_cases as gc
import prep_cases as pc

pytestmark = pytest.mark.gpu
TAIL = 8          # canary floats behind y, canary pairs behind part_out


def first_diff(got, want):
    bad = np.flatnonzero(got != want)
    return f"{bad.size} of {got.size} differ, first at {bad[0]}: got {got[bad[0]]:#010x}, want {want[bad[0]]:#010x}" if bad.size else "equal"


def check_parts(parts, y, nw, grid, tag):
    """pairs [grid + TAIL, 2] against the fp32 outputs y [M] of the same launch"""
    assert np.all(parts[grid:].view(np.uint64) == 0x7FF8DEADBEEF0000), f"{tag}: pairs past the grid were written"
    rows = nw * 8
    for b in range(grid):
        v = y[b * rows:(b + 1) * rows].astype(np.float64)
        if not np.all(np.isfinite(v)):          # (a zero-weight row-group under +-inf residuals: inf - inf, NaN either way)
            assert not np.isfinite(parts[b, 1]), (tag, b, parts[b])
            continue
        s1, s2, a1 = math.fsum(v), math.fsum(v * v), math.fsum(np.abs(v))
        assert abs(parts[b, 0] - s1) <= pc.gamma(rows) * a1 and abs(parts[b, 1] - s2) <= pc.gamma(rows) * s2, (tag, b, parts[b], s1, s2)


def run_case(L, oracle, c):
    pre, epi, inter, op_pre, op_epi = gc.PAIRS[c.pair]
    tag = gc.case_id(c)
    ops = gc.build(oracle, c)
    assert all(gc.weight_properties(ops["w"])), f"{tag}: the matrix lacks a d == 0 block or a code 0 / 15"
    if op_pre == "norm":          # a condition on the INPUT: with it no summation order, in either form, can change a float
        assert pc.norm_proof_both(ops["in0"]), f"{tag}: the row is not order-proof"
    want = gc.reference(oracle, c, ops)
    n_out = want["y"].size
    plan = L.gemv_plan(c.M, c.K, pre, epi, inter)
    y_init = np.full(n_out + TAIL, gc.CANARY, np.uint32).view(np.float32)
    po = np.full((plan[4] + TAIL, 2), 0x7FF8DEADBEEF0000, np.uint64).view(np.float64) if c.part_out else None
    r = L.op_gemv_q4_0(ops["w"], op_pre, op_epi, ops["in0"], ops["in1"], ops["resid"], interleaved=inter, part_in=ops["part_in"],
                       y_init=y_init, part_out=po, n_part_out=plan[4] if c.part_out else None)
    assert r["plan"] == plan, f"{tag}: launched {r['plan']}, the plan is {plan}"
    got, exp = r["y"][:n_out].view(np.uint32), np.ascontiguousarray(want["y"]).view(np.uint32)
    assert np.array_equal(got, exp), f"{tag}: y: {first_diff(got, exp)}"
    assert np.all(r["y"][n_out:].view(np.uint32) == gc.CANARY), f"{tag}: floats past the {n_out} outputs were written"
    if op_epi == "silu_qa":
        F = c.M // 2
        A, d = r["out_A"], r["out_d"].view(np.uint32)
        assert np.array_equal(A[0], want["out_A"]), f"{tag}: out_A: {first_diff(A[0], want['out_A'])}"
        assert np.array_equal(d[0], want["out_d"].view(np.uint32)), f"{tag}: out_d: {first_diff(d[0], want['out_d'].view(np.uint32))}"
        nb, nbp = F // 32, pc.kp(F) // 32
        assert nb == nbp or (not d[0, nb:].any() and not A[0].reshape(nbp // 8, 8, 8)[-1][:, nb % 8:].any()), f"{tag}: padded blocks are not zero"
        assert np.all(A[1:] == 0xFFFFFFFF) and np.all(d[1:] == 0xFFFFFFFF), f"{tag}: the operand row behind the launch's was written"
    if c.part_out:
        check_parts(r["part_out"], r["y"][:n_out], plan[0], plan[4], tag)
    return ops, want, r


def select(group):
    return [c for c in gc.CASES if c.group == group]


@pytest.mark.parametrize("case", select("inst"), ids=gc.case_id)
def test_every_kernel_instance(L, oracle, case):
    run_case(L, oracle, case)
    pre, epi, nw, pg, depth, ring = next(i[:6] for i in gc.INSTANCES if gc.PAIR_OF[i[:2]] == case.pair and i[6:] == (case.M, case.K))
    assert L.gemv_plan(case.M, case.K, pre, epi, gc.PAIRS[case.pair][2])[:4] == (nw, pg, depth, ring)


@pytest.mark.parametrize("case", select("rows"), ids=gc.case_id)
def test_row_edges(L, oracle, case):
    run_case(L, oracle, case)


@pytest.mark.parametrize("case", select("regime"), ids=gc.case_id)
def test_value_regimes_through_the_fused_prologues(L, oracle, case):
    ops, want, _ = run_case(L, oracle, case)
    if case.regime == "ties" and case.pair == "plain.resid":          # the fused quantizer saw exact halves
        p, a = pc.tie_products(want["row"]).reshape(-1, 32), np.abs(want["row"]).reshape(-1, 32)
        inner = a != a.max(axis=1, keepdims=True)
        assert inner.sum() == 30 * p.shape[0] and np.all(p[inner] - np.floor(p[inner]) == 0.5)
    if case.regime.startswith("dc:"):          # the offsets sit on the side of the switch they are meant for, in every summation order
        o = pc.one_pass_stats(ops["in0"])
        assert o["fast_certain"] if float(case.regime[3:]) < 0.577 else not o["fast_possible"], (case.regime, o)


@pytest.mark.parametrize("case", select("epi"), ids=gc.case_id)
def test_epilogue_edges(L, oracle, case):
    ops, want, r = run_case(L, oracle, case)
    if case.wkind == "zero_group":
        res = ops["resid"][8:16]
        assert np.array_equal(r["y"][8:16].view(np.uint32), (np.float32(0.0) + res).view(np.uint32)), "a zero-weight row must give +0 + resid"
        assert set(res.view(np.uint32).tolist()) == {0x80000000, 0, 0x7F800000, 0xFF800000}
    if case.wkind == "silu_zero":
        F = case.M // 2
        assert not want["gate"][:32].any() and not want["up"][32:64].any() and want["up"][:32].any() and want["gate"][32:64].any()
        assert not want["out_d"][:2].any() and want["out_d"][2] > 0, "blocks 0 and 1: amax 0, d 0"
        assert np.all(L.qa_to_blocks(r["out_A"], r["out_d"], 1, F)[0, :2, 4:] == 0x88), "... and codes 0 (q = 8 in file layout)"
        g = want["gate"][64:]
        assert g.min() < -8 and g.max() > 8 and np.abs(g).max() < 24, f"the gates span {g.min()} .. {g.max()}"


@pytest.mark.parametrize("M,nw", [(1024, 1), (4096, 2)])
def test_resid_parts_feed_the_norm_prologue(L, oracle, M, nw):
    """the hand-over as a model's step does it: the pairs an EPI_RESID launch leaves, fed back as part_in of a NORM launch on that y, give
    what the NORM launch computes from the row itself -- the oracle's bits, the row being order-proof"""
    c = gc.Case("feed", "qa.resid", M, 64, "plain", "normal:1", 0, True)
    _, want, r = run_case(L, oracle, c)
    assert r["plan"][0] == nw and r["plan"][4] == M // 8 // nw
    y = r["y"][:M].copy()
    assert pc.norm_proof_both(y), "the residual row is not order-proof"
    w2, wn = gc.weights(24, M, "plain"), gc.norm_weight(M)
    row = pc.reference(oracle, "norm", y[None, :], wn)[0][0]
    exp = oracle.mul_mat_q4_0(w2, row[None, :])[0].view(np.uint32)
    plain = L.op_gemv_q4_0(w2, "norm", "store", y, wn)
    fed = L.op_gemv_q4_0(w2, "norm", "store", y, wn, part_in=r["part_out"][:r["plan"][4]])
    assert fed["plan"] == L.gemv_plan(24, M, 4, 0) and plain["plan"] == L.gemv_plan(24, M, 2, 0)
    assert np.array_equal(plain["y"].view(np.uint32), exp), first_diff(plain["y"].view(np.uint32), exp)
    assert np.array_equal(fed["y"].view(np.uint32), exp), first_diff(fed["y"].view(np.uint32), exp)
