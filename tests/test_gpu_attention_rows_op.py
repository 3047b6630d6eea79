"""GPU (-m gpu): the row-table attention of llamahip_eval_multi's pass (llamahip_op_attention_rows: k_rope_kv_rows, k_rows_scores, k_rows_pv) op
by op.  R rows of several KV slots go through ONE launch chain; each segment's merged rows, wo operand and cache rows must be bit for bit what
llamahip_op_attention leaves on that segment alone with its slot's cache -- path SHORT (2 .. 60 rows), ROW / DEC where SHORT refuses the
shape (one row) -- with the same chunk and thread count.  The op's score scratch holds 16 rows, so 29 and 64 rows also walk it in batches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, N_CTX, N_SLOTS = 256, 128, 5          # slot 4 is never named: a NaN-filled guard
# (rows @ n_past) per segment, on the slots named beside them (non-ascending order)
TABLES = {
    "crossing16": ([(1, 5), (2, 0), (9, 17), (17, 3)], [2, 0, 3, 1]),          # R = 29
    "rows64": ([(60, 0), (4, 100)], [2, 0]),                                  # R = 64, a segment at the short path's limit
    "to_n_ctx": ([(3, 0), (5, 40), (7, 121)], [2, 0, 3]),                     # the last segment ends exactly at n_ctx
}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("H", [4, 2])
@pytest.mark.parametrize("table", list(TABLES))
def test_rows_attention_is_each_segments_own_attention(L, H, table):
    segs, slots = TABLES[table]
    rng = np.random.default_rng(1000 * H + len(table))
    n_tok, n_past = [s[0] for s in segs], [s[1] for s in segs]
    R = sum(n_tok)
    qkv = rng.standard_normal((R, 3 * D)).astype(np.float32)
    K0 = rng.standard_normal((N_SLOTS, N_CTX, D)).astype(np.float32)
    V0 = rng.standard_normal((N_SLOTS, N_CTX, D)).astype(np.float32)
    K0[4], V0[4] = np.nan, np.nan
    ms = D + 32
    for chunk in (0, 1, 9):
        seg, pos, keys = L.eval_multi_rows(N_CTX, n_past, n_tok, chunk)
        row_slot = np.array(slots, np.int32)[seg]
        for nth in (1, 3, 8):
            note = (H, table, chunk, nth)
            Kc, Vc = K0.copy(), V0.copy()
            merged, wo = L.op_attention_rows(qkv, H, Kc, Vc, row_slot, pos, keys, n_threads=nth, merged_stride=ms)
            assert np.isnan(merged[:, D:]).all(), (note, "the floats between d and merged_stride")
            r0 = 0
            for i, (n, p) in enumerate(segs):
                s = slots[i]
                Ks, Vs = K0[s].copy(), V0[s].copy()
                rows = qkv[r0:r0 + n]
                if n >= 2:
                    m1, w1, path = L.op_attention(rows, H, p, Ks, Vs, n_threads=nth, chunk=chunk, path="short", merged_stride=ms)
                    assert path == "short"
                else:
                    m1, _, path = L.op_attention(rows, H, p, Ks, Vs, n_threads=nth, chunk=chunk, path="row", merged_stride=ms)
                    assert path == "row"
                    Kd, Vd = K0[s].copy(), V0[s].copy()
                    _, w1, _ = L.op_attention(rows, H, p, Kd, Vd, n_threads=nth, path="dec")          # (the one-row path that returns wo's operand)
                    assert same(Kd, Ks) and same(Vd, Vs)
                assert same(merged[r0:r0 + n, :D], m1[:, :D]), (note, i, "merged rows")
                assert same(wo[r0:r0 + n], w1), (note, i, "wo operand")
                assert same(Kc[s], Ks) and same(Vc[s], Vs), (note, i, "the slot's cache: appended rows and everything around them")
                untouched = np.ones(N_CTX, bool)
                untouched[p:p + n] = False
                assert same(Kc[s][untouched], K0[s][untouched]) and same(Vc[s][untouched], V0[s][untouched]), (note, i, "rows outside the appended range")
                assert not same(Kc[s][p:p + n], K0[s][p:p + n])
                r0 += n
            for s in range(N_SLOTS):
                if s not in slots:
                    assert same(Kc[s], K0[s]) and same(Vc[s], V0[s]), (note, s, "a slot no row names")
            assert np.isnan(Kc[4]).all() and np.isnan(Vc[4]).all()
