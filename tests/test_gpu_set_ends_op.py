"""GPU (-m gpu): the first and last launches of a batched decode step, op by op (llamahip_op_set_entry, llamahip_op_set_exit).

Entry -- k_embed_set, k_embed_dense_set<f16 | f32>, k_rows_set (gather): every row's token word, state pair and hid_in row sits at a
scattered address inside one pool of 0xFF words.  x rows: the Q4_0 rows tests/test_gpu_prep.py expects of llamahip_op_embed
(oracle.dequantize_row), the exact widening of f16 / f32 rows in numpy, the hid_in rows bit for bit; x columns >= d keep the caller's
canary; the descriptor's pos[] equals row_pos (entries >= B untouched); the epoch word is next_epoch(epoch_in) -- restated in
set_attn_cases, not asked of the library -- when it is passed and untouched when not; the state words and every other word are unchanged.

Exit -- k_argmax_set, k_rows_set (scatter) + k_advance_set, and k_argmax with a state pointer (the kernel k_argmax_set is a copy of): the
picks follow rule() of tests/test_gpu_sched_pick_op.py on its eight kinds of rows (ties at the first and last index, +0 / -0, NaN, all
-inf, +inf, all NaN) and equal llamahip_op_verify_rows' picks; only trace[b][row_step[b]] changes; a null tok_out is not written; both
state words advance by one; hid_out rows equal x with the guards between them intact (the op fails otherwise)."""
import numpy as np
import pytest

import prep_cases as pc
import set_attn_cases as sa
from test_gpu_sched_pick_op import rows_of, rule

pytestmark = pytest.mark.gpu
CANARY = np.uint32(0x7FC0BEEF)
UNSET = 0x7F7F7F7F


def f16_matrix(rng, V, d):
    m = rng.standard_normal((V, d)).astype(np.float16)
    special = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00], np.uint16).view(np.float16)
    m[0, :len(special)] = special
    m[V - 1, -len(special):] = special
    return m


def f32_matrix(rng, V, d):
    m = rng.standard_normal((V, d)).astype(np.float32)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC0BEEF, 0xFFC00001], np.uint32).view(np.float32)
    m[0, :len(special)] = special
    m[V - 1, -len(special):] = special
    return m


@pytest.fixture(scope="module")
def matrices(oracle):
    """(mode, d) -> (the matrix in file layout, its rows as fp32 [V, d]); computed once"""
    out = {}
    for d in (32, 320, 4096):
        rng = np.random.default_rng(d)
        m = pc.embed_matrix(rng, sa.V_EMB, d)
        out["embed_q4_0", d] = (m, np.stack([oracle.dequantize_row(r) for r in m]))
        h = f16_matrix(rng, sa.V_EMB, d)
        out["embed_f16", d] = (h, h.astype(np.float32))
        f = f32_matrix(rng, sa.V_EMB, d)
        out["embed_f32", d] = (f, f)
    return out


@pytest.mark.parametrize("mode,d,B,epoch_in,pass_epoch", sa.ENTRY_CASES)
def test_entry(L, matrices, mode, d, B, epoch_in, pass_epoch):
    tokens, row_pos = sa.entry_rows(B)
    stride = d + 8
    x0 = np.full((B, stride), CANARY, np.uint32).view(np.float32)
    if mode == "rows":
        hid = f32_matrix(np.random.default_rng(B + d), B, d)
        out = L.op_set_entry(mode, row_pos, hid_in=hid, epoch_in=epoch_in, pass_epoch=pass_epoch, x_stride=stride, x_init=x0)
        want = hid
    else:
        emb, rows = matrices[mode, d]
        out = L.op_set_entry(mode, row_pos, emb=emb, tokens=tokens, epoch_in=epoch_in, pass_epoch=pass_epoch, x_stride=stride, x_init=x0)
        want = rows[tokens]
    tag = (mode, d, B, hex(epoch_in), pass_epoch)
    got = out["x"]
    assert np.array_equal(got[:, :d].view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (tag, np.argwhere(got[:, :d].view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))[:3])
    assert np.all(got[:, d:].view(np.uint32) == CANARY), (tag, "x columns >= d")
    assert out["pos"][:B].tolist() == row_pos.tolist() and np.all(out["pos"][B:] == UNSET), (tag, out["pos"])
    assert out["epoch"] == (sa.next_epoch(epoch_in) if pass_epoch else epoch_in), (tag, hex(out["epoch"]))          # opened exactly once
    assert out["state"].tolist() == [[int(row_pos[r]), 7 + 3 * r] for r in range(B)], (tag, out["state"])
    assert not out["changed"], (tag, "a word outside the named ones changed")


@pytest.mark.parametrize("V", sa.EXIT_VOCABS)
@pytest.mark.parametrize("B", [2, 16])
def test_exit_argmax_set(L, B, V):
    rng = np.random.default_rng(1000 * B + V)
    pos, step, null = sa.exit_rows(B)
    for rep in range(8 // B if B < 8 else 1):
        lg = rows_of(rng, max(B, 8), V)
        if B < 8:          # few rows: walk the eight kinds over the repetitions
            lg = np.ascontiguousarray(lg[[(rep * B + r) % 8 for r in range(B)]])
        want = [rule(lg[r]) for r in range(B)]
        _, yard = L.op_verify_rows(lg, np.zeros(B, np.int32))
        assert yard.tolist() == want, (B, V, "the yardstick kernel against the rule")
        out = L.op_set_exit("argmax", pos, step, sa.EXIT_N_CTX, logits=lg, tok_out_null=null)
        trace_want = np.full((B, sa.EXIT_N_CTX), -1, np.int32)
        trace_want[np.arange(B), step] = want
        assert np.array_equal(out["trace"], trace_want), (B, V, rep, out["trace"][np.arange(B), step].tolist(), want)
        assert out["tok_out"].tolist() == [-1 if null[r] else want[r] for r in range(B)], (B, V, rep)
        assert out["state"].tolist() == [[int(pos[r]) + 1, int(step[r]) + 1] for r in range(B)], (B, V, rep)


@pytest.mark.parametrize("V", sa.EXIT_VOCABS)
def test_exit_argmax_one_is_the_same_rule(L, V):
    """k_argmax on each of the eight kinds as its one row, with and without a next-token word; k_argmax_set must give the same picks"""
    rng = np.random.default_rng(V)
    lg = rows_of(rng, 8, V)
    want = [rule(lg[r]) for r in range(8)]
    pos8, step8, _ = sa.exit_rows(8)
    both = L.op_set_exit("argmax", pos8, step8, sa.EXIT_N_CTX, logits=lg)
    assert both["tok_out"].tolist() == want, (V, "k_argmax_set")
    for r in range(8):
        for null in (0, 1):
            p, s = (sa.EXIT_N_CTX - 1, 0) if r % 2 else (0, sa.EXIT_N_CTX - 1)
            out = L.op_set_exit("argmax_one", [p], [s], sa.EXIT_N_CTX, logits=lg[r:r + 1], tok_out_null=[null])
            trace_want = np.full((1, sa.EXIT_N_CTX), -1, np.int32)
            trace_want[0, s] = want[r]
            assert np.array_equal(out["trace"], trace_want), (V, r, null, out["trace"][0, s], want[r])
            assert out["tok_out"].tolist() == [-1 if null else want[r]] and out["state"].tolist() == [[p + 1, s + 1]], (V, r, null)
    if V == 1500:          # what the kinds are there for
        assert want[1] == 0 and want[2] == 1499 and want[3] == 500 and want[5] == 0 and want[6] == 1000 and want[7] == 0 and want[4] not in (0, 750)


@pytest.mark.parametrize("d,B", [(32, 2), (320, 3), (4096, 16)])
def test_exit_rows_out(L, d, B):
    x = f32_matrix(np.random.default_rng(d), B, d)
    pos, step, null = sa.exit_rows(B)
    out = L.op_set_exit("rows_out", pos, step, sa.EXIT_N_CTX, x=x, tok_out_null=null)
    assert np.array_equal(out["hid_out"].view(np.uint32), x.view(np.uint32)), (d, B)
    assert np.all(out["trace"] == -1) and np.all(out["tok_out"] == -1), (d, B, "the scatter and the advance write no pick")
    assert out["state"].tolist() == [[int(pos[r]) + 1, int(step[r]) + 1] for r in range(B)], (d, B)
