"""Cases and references of the batched decode step's attention (llamahip_op_set_attention: k_rows_set -> k_rope_kv_set -> k_decn_scores +
k_dec_pv_blk<true> with a SeqSet), for tests/test_set_ops_host.py (CPU) and tests/test_gpu_set_attention_op.py.  Nothing here needs a GPU.

A case is B rows (2, 3 or 16), each the next token of a KV slot: singles (one row of a slot) and drafted segments (n rows of one slot at
consecutive positions, in adjacent rows).  Every segment's q|k|v rows and its slot's cache come from attn_cases.make(regime, n, ...) -- a
single is a segment of one row --, so cache rows past the appended positions hold attn_cases.CANARY.  Slots no row names hold random
values; the last slot is a NaN-filled guard.

expect() is the reference, bit for bit: the rows in order, row r = attn_cases.oracle_side on its own (N = 1) at row_pos[r] with n_threads,
on its slot's cache as the earlier rows of that slot left it.  wrong_models() are four things a kernel could do instead; the host test
asserts that each of them changes at least one word of a case's expected merged rows (a condition on the INPUTS):
  a  split   the key split of row_pos + B keys (the multi-row meaning: the masked tail is walked with weight 0, over whatever the cache
             holds there -- the rows the neighbours appended, canaries, the next slot)
  b  pos     the position off by one (one below; one above at position 0)
  c  slot0   slot 0's cache in place of the row's own (rows of other slots)
  d  stale   a segment's later row that does not see the key its neighbour appended in the same step"""
import numpy as np

import attn_cases

FILL_NAN = 0xFFFFFFFF
FILL_1E30 = int(np.array([1e30], np.float32).view(np.uint32)[0])          # a read past a row's T moves the maximum instead of making a NaN
SHAPES = ((128, 2), (192, 2), (256, 1), (256, 2), (320, 10))              # head sizes 64, 96, 256, 128, 32; only d = 256 has no QA pad blocks
BUCKET = 128


def rule_keys(n_ctx, max_pos):
    """the key bucket written out: what llamahip_debug_set_keys must return"""
    return min(n_ctx, (max_pos // BUCKET + 1) * BUCKET)


def _case(name, shape, n_ctx, nth, table, segs, keys, fill):
    """segs: (slot, first position, rows, regime) in row order"""
    d, H = shape
    return dict(name=name, d=d, H=H, n_ctx=n_ctx, nth=nth, table=table, segs=segs, keys=keys, fill=fill)


def _singles(slots, positions, r0=0):
    return [(s, p, 1, attn_cases.REGIMES[(r0 + i) % len(attn_cases.REGIMES)]) for i, (s, p) in enumerate(zip(slots, positions))]


_POS16 = [0, 1, 2, 5, 31, 32, 33, 63, 64, 95, 96, 100, 126, 127, 17, 7]
_SLOT16 = [9, 3, 15, 1, 0, 12, 7, 16, 2, 5, 11, 4, 14, 6, 10, 8]          # (slot 13 is never named)
CASES = [
    _case("ends2", SHAPES[0], 160, 8, "distinct", _singles([2, 1], [0, 159]), "zero", FILL_NAN),                 # position 0 with n_ctx - 1
    _case("slice3", SHAPES[1], 160, 32, "distinct", _singles([3, 0, 1], [0, 31, 32], 1), "rule", FILL_1E30),    # the DEC_TS slice edge
    _case("bucket3", SHAPES[2], 288, 3, "distinct", _singles([2, 3, 1], [127, 128, 287], 2), "rule", FILL_NAN),  # the bucket edge, n_ctx - 1
    _case("exact16", SHAPES[4], 288, 8, "distinct", _singles(_SLOT16, _POS16), "exact", FILL_1E30),              # highest row at 127: 128 keys
    _case("ends2_one", SHAPES[3], 288, 1, "distinct", _singles([1, 0], [287, 0], 4), "zero", FILL_1E30),
    _case("zero3", SHAPES[4], 160, 8, "distinct", _singles([2, 1, 0], [0, 31, 159], 3), "zero", FILL_1E30),
    _case("drafts16", SHAPES[3], 160, 3, "segments",
          [(4, 30, 3, "negzero"), (9, 0, 1, "plain"), (1, 125, 4, "leak")] + _singles([7, 0, 3, 8, 2, 6, 5, 10], [0, 31, 32, 127, 128, 159, 64, 1], 1),
          "zero", FILL_NAN),
    _case("drafts16_wide", SHAPES[0], 288, 32, "segments",
          _singles([6, 2], [287, 0]) + [(5, 30, 3, "ties")] + _singles([0, 9, 3, 7, 1, 8], [127, 128, 31, 32, 200, 5], 2) + [(4, 125, 4, "zeroq"), (10, 64, 1, "wide")],
          "rule", FILL_1E30),
    _case("one16_slice", SHAPES[1], 160, 1, "one_slot", [(1, 20, 16, "negzero")], "rule", FILL_1E30),           # 20 .. 35 crosses the slice edge
    _case("one16_bucket", SHAPES[2], 288, 8, "one_slot", [(1, 120, 16, "plain")], "rule", FILL_NAN),            # 120 .. 135 crosses the bucket edge
    _case("one16_end", SHAPES[4], 288, 3, "one_slot", [(2, 272, 16, "wide")], "zero", FILL_1E30),               # ends at n_ctx - 1
    _case("one16_leak", SHAPES[3], 160, 32, "one_slot", [(1, 112, 16, "leak")], "exact", FILL_NAN),             # 112 .. 127: 128 keys exactly
]


def case_id(c):
    return c["name"]


def rows_of(c):
    """(row_slot, row_pos) int32 [B]"""
    slot = np.concatenate([np.full(n, s, np.int32) for s, _, n, _ in c["segs"]])
    pos = np.concatenate([np.arange(p, p + n, dtype=np.int32) for _, p, n, _ in c["segs"]])
    return slot, pos


def set_keys_of(c):
    _, pos = rows_of(c)
    if c["keys"] == "zero":
        return 0
    k = rule_keys(c["n_ctx"], int(pos.max()))
    if c["keys"] == "exact":
        assert int(pos.max()) == BUCKET - 1 and k == BUCKET, c["name"]
    return k


def build(c):
    """dict(qkv [B][3d], Kc, Vc [n_slots][n_ctx][d], row_slot, row_pos, n_slots): a pure function of the case"""
    d, H, n_ctx = c["d"], c["H"], c["n_ctx"]
    row_slot, row_pos = rows_of(c)
    n_slots = int(row_slot.max()) + 3          # one slot no row names beyond the highest, then the NaN guard
    rng = np.random.default_rng([len(c["name"]), d, n_ctx, len(row_slot)])
    Kc = rng.standard_normal((n_slots, n_ctx, d)).astype(np.float32)
    Vc = rng.standard_normal((n_slots, n_ctx, d)).astype(np.float32)
    Kc[-1], Vc[-1] = np.nan, np.nan
    qkv = []
    for i, (s, p, n, regime) in enumerate(c["segs"]):
        q, Ks, Vs = attn_cases.make(regime, n, d, H, p, n_ctx, seed=100 + i)
        qkv.append(q)
        Kc[s], Vc[s] = Ks, Vs
    return dict(qkv=np.ascontiguousarray(np.concatenate(qkv)), Kc=Kc, Vc=Vc, row_slot=row_slot, row_pos=row_pos, n_slots=n_slots)


def _row(oracle, c, qkv_row, K, V, pos):
    m, K2, V2, _ = attn_cases.oracle_side(oracle, qkv_row, K, V, c["H"], pos, c["nth"])
    return m[0], K2, V2


def expect(oracle, c, ops):
    """(merged [B][d], Kc, Vc, wo [B][d/32][20]) as B successive one-row evals leave them"""
    d = c["d"]
    Kc, Vc = ops["Kc"].copy(), ops["Vc"].copy()
    B = len(ops["row_pos"])
    merged = np.empty((B, d), np.float32)
    for r in range(B):
        s, p = int(ops["row_slot"][r]), int(ops["row_pos"][r])
        merged[r], Kc[s], Vc[s] = _row(oracle, c, ops["qkv"][r:r + 1], Kc[s], Vc[s], p)
    wo = np.stack([oracle.quantize_row(m) for m in merged]).reshape(B, d // 32, 20)
    return merged, Kc, Vc, wo


def wrong_models(oracle, c, ops):
    """(the expected merged [B][d], {name: merged [B][d] under that wrong model, the rows it does not apply to as expected -- None where it
    applies to no row})"""
    d, H, n_ctx, nth = c["d"], c["H"], c["n_ctx"], c["nth"]
    B = len(ops["row_pos"])
    right, Kf, Vf, _ = expect(oracle, c, ops)          # (Kf, Vf: every row appended, as k_rope_kv_set leaves the caches before the scores)
    out = {k: right.copy() for k in "abcd"}
    hit = dict.fromkeys("abcd", False)
    Kc, Vc = ops["Kc"].copy(), ops["Vc"].copy()
    first = {}
    for r in range(B):
        s, p = int(ops["row_slot"][r]), int(ops["row_pos"][r])
        row = ops["qkv"][r:r + 1]
        first.setdefault(s, r)
        # a: row 0 of an eval of B rows at n_past = p sees keys 0 .. p and splits p + B of them; the tail is what lies behind in memory
        T = p + B
        flatK, flatV = Kf[s:].reshape(-1, d), Vf[s:].reshape(-1, d)
        pad = max(T - len(flatK), 0)
        Kx, Vx = np.concatenate([flatK[:T], np.zeros((pad, d), np.float32)]), np.concatenate([flatV[:T], np.zeros((pad, d), np.float32)])
        qr = oracle.rope(np.repeat(row[:, :d], B, axis=0).reshape(B, H, d // H), p, 0).reshape(B, d)
        out["a"][r] = oracle.attention(qr, Kx, Vx, H, p, nth)[0]
        hit["a"] = True
        # b: one position off
        out["b"][r] = _row(oracle, c, row, Kc[s], Vc[s], p - 1 if p > 0 else 1)[0]
        hit["b"] = True
        # c: slot 0's cache
        if s != 0:
            out["c"][r] = _row(oracle, c, row, Kc[0], Vc[0], p)[0]
            hit["c"] = True
        # d: the neighbour's key is still what the cache held before the step
        if first[s] != r:
            Ks, Vs = Kc[s].copy(), Vc[s].copy()
            Ks[p - 1], Vs[p - 1] = ops["Kc"][s][p - 1], ops["Vc"][s][p - 1]
            out["d"][r] = _row(oracle, c, row, Ks, Vs, p)[0]
            hit["d"] = True
        _, Kc[s], Vc[s] = _row(oracle, c, row, Kc[s], Vc[s], p)
    return right, {k: (v if hit[k] else None) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ the step's first and last launches
V_EMB = 64
ENTRY_MODES = ("embed_q4_0", "embed_f16", "embed_f32", "rows")
EXIT_MODES = ("argmax", "rows_out", "argmax_one")
# (mode, d, B, epoch_in, pass the epoch word): the dense kernels take no epoch word; 0x00FFFFFF / 0xFFFFFFFF: next_epoch skips a zero low part
ENTRY_CASES = [(m, d, B, e, p) for m in ENTRY_MODES for d, B in ((32, 2), (320, 3), (4096, 16))
               for e, p in ((0, True), (0x00FFFFFF, True), (0xFFFFFFFF, True), (41, False)) if p is False or m in ("embed_q4_0", "rows")]
EXIT_VOCABS = (1, 65, 1500, 32000)
EXIT_N_CTX = 160


def next_epoch(e):
    """the epoch arithmetic restated: + 1, and once more where the low 24 bits would be zero (a tag of epoch 0 means `never written`)"""
    e = (e + 1) & 0xFFFFFFFF
    if e & 0xFFFFFF == 0:
        e = (e + 1) & 0xFFFFFFFF
    return e


def entry_rows(B):
    """(tokens, row_pos): tokens 0 and V - 1 and one token shared by two rows; positions 0, large, and one shared by two rows"""
    tokens = np.array(([0, V_EMB - 1, 0, 5] + list(range(7, 7 + 12)))[:B], np.int32)
    if B == 2:
        tokens = np.array([V_EMB - 1, V_EMB - 1], np.int32)
    pos = np.array(([0, 287, 31, 31] + list(range(100, 112)))[:B], np.int32)
    return tokens, pos


def exit_rows(B, n_ctx=EXIT_N_CTX):
    """(row_pos, row_step, tok_out_null): steps 0 and n_ctx - 1 among them, one null tok_out (the second row; none where B = 1)"""
    pos = np.array(([n_ctx - 1, 0] + list(range(3, 3 + 14)))[:B], np.int32)
    step = np.array(([0, n_ctx - 1] + list(range(40, 40 + 14)))[:B], np.int32)
    null = np.zeros(B, np.int32)
    if B > 1:
        null[1] = 1
    return pos, step, null
