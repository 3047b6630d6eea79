"""GPU (-m gpu): the attention of a batched decode step op by op (llamahip_op_set_attention: k_rows_set fills SeqSet::pos, k_rope_kv_set
rotates and appends, k_decn_scores + k_dec_pv_blk<true> take the set), against the oracle bit for bit -- uint32 views, so the sign of zero
and NaN payloads count.  Cases, reference and what they are there for: tests/set_attn_cases.py (the conditions on the inputs are checked on
the CPU, tests/test_set_ops_host.py).  Per case, with a merged buffer (dense handles) and with a null one (Q4_0 handles):
  1. merged rows equal the oracle's B successive one-row evals, and merged columns >= d keep their canary;
  2. the wo operand equals orc_quantize_row_q4_0 of the oracle's merged rows (the op itself fails if a QA pad block is not zero or a state
     word moved);
  3. both caches equal the oracle's in every word: appended rows, canary rows behind them, slots no row names, the NaN guard slot.
Cross-checks on the device: a drafted segment equals llamahip_op_attention's SHORT path with chunk = 1 on that segment alone, a lone row
path DEC.  The score scratch starts as NaN words or as +1e30, the latter so that a score read past a row's T moves the maximum."""
import numpy as np
import pytest

import attn_cases
import set_attn_cases as sa

pytestmark = pytest.mark.gpu
EXTRA = 8


def diff(got, want):
    bad = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
    if not len(bad):
        return "equal"
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} words differ, first at {i}: got {got[i]!r}, want {want[i]!r}"


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def refs(oracle):
    """name -> (operands, (merged, Kc, Vc, wo) expected), computed once per case and left unchanged"""
    cache = {}

    def get(c):
        if c["name"] not in cache:
            ops = sa.build(c)
            cache[c["name"]] = (ops, sa.expect(oracle, c, ops))
        return cache[c["name"]]
    return get


@pytest.mark.parametrize("c", sa.CASES, ids=sa.case_id)
def test_set_attention_is_each_rows_own_eval(L, refs, c):
    ops, (want, Kw, Vw, wo_want) = refs(c)
    d, H, B = c["d"], c["H"], len(ops["row_pos"])
    canary = np.full((B, d + EXTRA), attn_cases.CANARY, np.uint32).view(np.float32)
    for with_merged in (True, False):
        tag = f"{c['name']} merged={with_merged}"
        Kg, Vg = ops["Kc"].copy(), ops["Vc"].copy()
        merged, wo = L.op_set_attention(ops["qkv"], H, Kg, Vg, ops["row_slot"], ops["row_pos"], c["nth"], sa.set_keys_of(c), merged_stride=d + EXTRA,
                                        merged_init=canary, want_merged=with_merged, score_fill=c["fill"])
        if with_merged:
            assert same(merged[:, :d], want), f"{tag}: merged: {diff(merged[:, :d], want)}"
            assert np.all(merged[:, d:].view(np.uint32) == attn_cases.CANARY), f"{tag}: merged columns >= d written"
        else:
            assert merged is None
        assert np.array_equal(wo, wo_want), f"{tag}: wo operand differs at {np.argwhere(wo != wo_want)[:1]}"
        assert same(Kg, Kw), f"{tag}: K cache: {diff(Kg, Kw)}"
        assert same(Vg, Vw), f"{tag}: V cache: {diff(Vg, Vw)}"


@pytest.mark.parametrize("c", sa.CASES, ids=sa.case_id)
def test_segments_and_lone_rows_against_the_one_sequence_paths(L, refs, c):
    ops, _ = refs(c)
    d, H = c["d"], c["H"]
    Kg, Vg = ops["Kc"].copy(), ops["Vc"].copy()
    merged, wo = L.op_set_attention(ops["qkv"], H, Kg, Vg, ops["row_slot"], ops["row_pos"], c["nth"], sa.set_keys_of(c), score_fill=c["fill"])
    r0 = 0
    for i, (s, p, n, _) in enumerate(c["segs"]):
        rows = ops["qkv"][r0:r0 + n]
        Ks, Vs = ops["Kc"][s].copy(), ops["Vc"][s].copy()
        if n >= 2:
            m1, w1, path = L.op_attention(rows, H, p, Ks, Vs, n_threads=c["nth"], chunk=1, path="short")
        else:
            m1, w1, path = L.op_attention(rows, H, p, Ks, Vs, n_threads=c["nth"], path="dec")
        assert path == ("short" if n >= 2 else "dec")
        assert same(merged[r0:r0 + n], m1), (c["name"], i, "merged rows", diff(merged[r0:r0 + n], m1))
        assert same(wo[r0:r0 + n], w1), (c["name"], i, "wo operand")
        assert same(Kg[s], Ks) and same(Vg[s], Vs), (c["name"], i, "the slot's cache")
        r0 += n
