"""Cases, inputs and references for tests/test_gpu_gemv_set_op.py (and the CPU checks of tests/test_gemv_set_op_host.py): the few-row Q4_0
mat-mul k_gemv_set through llamahip_op_gemv_set_q4_0, one launch per case (two with x_prev), against the oracle bit for bit.  Nothing here
needs a GPU.

A case is Case(group, epi, M, K, N, force, wkind, rope, x_prev, layer):
  epi     "store" | "resid" | "rope_kv" | "silu_qa" | "silu_qah"
  force   None (the library's rule picks) or (nc, cw): that instance of the kernel, rgw derived, launched as asked or refused
  wkind   gemv_cases.weights' kinds: "plain"; "zero_group" under every residual (rows 8 .. 15 have every scale zero and sit under residuals
          of -0, +0, +-inf; M >= 16); "wide" / "silu_zero" for the interleaved w1|w3 matrices
  rope    None or (d, dh, n_ctx, n_past, table): table False = row r at position n_past + r of slot 0; True = make_table's rows
  x_prev  SILU_QAH: the same launch runs first on 4 x, on the exchange buffer the real launch then finds uncleared
The groups (the smallest shapes at which each thing can go wrong):
  inst    every one of the 14 (nc, cw) pairs forced, under STORE / RESID (M = 24 and 75: 3 and 10 row-groups, which rgw = 2 / 4 does not
          divide -- dead waves, and with column groups a grid padded to 8 ncg workgroups, most of them invalid), under ROPE_KV (d = 128 with
          dh 64, d = 192 with dh 96) and, the four cw == 1 pairs, under SILU_QA / SILU_QAH (F = 224).  Rows per pair: nc cw (a full group),
          nc cw - 1 (clamped duplicate columns), 2 nc cw - 1 (two column groups, the second ragged), 2 nc cw + 1 (three groups).
  steps   the ring: K so that for each cw every steps % 4 occurs, steps 1, 2, 3 (fewer than the ring's prefill: the zero tile) and padded
          last chunks (STEP_KS; the host test asserts the coverage table).  M = 24, N = nc cw, the smallest pair of a cw under STORE, the
          largest under RESID.
  auto    no force: row-group counts on both sides of the 768 and 1536 class edges x the row counts on both sides of every branch of
          set_plan; the LDS fallback of wide rows (K of 54 / 86 chunks); one wq|wk|wv launch of the unshared class in column groups 5 + 4.
  rows    M that is no multiple of 8 (the m < M mask, the clamped residual fetch), 4099 = 513 row-groups.
  rope    head sizes 64 .. 256, rows 2 .. 60, n_past 0, 5 and n_ctx - N; with tables: distinct positions out of order, three slots of
          which slot 1 is never touched, rows 0 and 1 a drafted segment (one slot, consecutive positions).
  silu    F = 32 (one block), 224 (a padded chunk), 288 (two operand chunks), both epilogues wherever both run, and SILU_QAH after a launch
          on 4 x at layer 0 and at the last layer (a stale granule read would quadruple a block's amax).
References (test file docstring): all from oracle.mul_mat_q4_0, oracle.rope, prep_cases.reference / pack_qa, bit for bit.
Not a case: NaN residuals (the payload an fp32 add hands on is the hardware's choice), SILU_QAH on a shared ring (not instantiated for
launch by gemv_set_applies), the fault-injection path."""
import collections

import numpy as np

import attn_cases
import gemv_cases as gc
import prep_cases as pc

SEED = 23
Case = collections.namedtuple("Case", "group epi M K N force wkind rope x_prev layer")
EPI = {"store": 0, "resid": 1, "silu_qa": 2, "rope_kv": 3, "silu_qah": 7}      # llamahip_internal.h
PAIRS = [(1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 3), (3, 4), (4, 1), (4, 2), (4, 4), (5, 1)]
AUTO_PAIRS = {(1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (2, 4), (3, 1), (4, 1), (4, 2), (5, 1)}      # what set_plan's rule can produce
FORCED_ONLY = {(2, 3), (3, 3), (3, 4), (4, 4)}
SET_MAX, ROWS_MAX, LDS_CAP, TAG_MAX_LAYERS, SET_DR = 16, 60, 160 * 1024, 250, 4
CANARY = attn_cases.CANARY
FILL = np.uint32(0xFFFFFFFF)
# steps = ceil(chunks / cw) of these K, for cw = 1, 2, 3, 4:
#   256: 1 1 1 1 | 320 (padded): 2 1 1 1 | 512: 2 1 1 1 | 768: 3 2 1 1 | 1024: 4 2 2 1 | 1344 (padded): 6 3 2 2 | 2048: 8 4 3 2
#   2304: 9 5 3 3 | 2816: 11 6 4 3 | 3392 (padded): 14 7 5 4 | 4352: 17 9 6 5
STEP_KS = (256, 320, 512, 768, 1024, 1344, 2048, 2304, 2816, 3392, 4352)


def case_id(c):
    s = f"{c.group}-{c.epi}-{c.M}x{c.K}-N{c.N}" + (f"-f{c.force[0]}x{c.force[1]}" if c.force else "")
    if c.rope:
        d, dh, n_ctx, n_past, table = c.rope
        s += f"-dh{dh}-" + ("table" if table else f"p{n_past}")
    if c.epi.startswith("silu"):
        s += f"-{c.wkind}"
    return s + (f"-prev-l{c.layer}" if c.x_prev else "")


def derived_rgw(epi, cw):
    return 4 if epi == "silu_qah" else 8 if epi == "silu_qa" else 2 if cw >= 3 else 4


def expected_forced_plan(c):
    """(nc, cw, ncg, rgw, grid, threads) a forced case must report (set_launch_shape's arithmetic, restated)"""
    nc, cw = c.force
    ncg, rgw, ng = -(-c.N // (nc * cw)), derived_rgw(c.epi, cw), (c.M + 7) // 8
    nwg = (ng // 8 + 7) // 8 * 16 if c.epi == "silu_qah" else -(-ng // rgw)
    return nc, cw, ncg, rgw, (nwg if ncg == 1 else (nwg + 7) // 8 * 8 * ncg), rgw * cw * 64


# ------------------------------------------------------------------------------------------------ inputs
def activation(c, attempt=0):
    """x fp32 [N, K]: every row at its own scale; row 0 opens with an all-zero block; row 1 is an exact-ties row (prep_cases.ties_rows, scaled
    by 2^-17 -- still exact halves -- so that a SiLU gate stays inside fp16); the last row of three or more is all zero"""
    rng = np.random.default_rng([SEED, c.M, c.K, c.N, 2 if c.epi.startswith("silu") else EPI[c.epi], attempt])      # (both SiLU epilogues: one x)
    x = (rng.standard_normal((c.N, c.K)) * rng.uniform(0.1, 4.0, (c.N, 1))).astype(np.float32)
    x[0, :32] = 0.0
    x[1] = pc.ties_rows(rng, 1, c.K)[0] * np.float32(2.0 ** -17)
    if c.N >= 3:
        x[c.N - 1] = 0.0
    return x


def activation_properties(x):
    """(the ordinary rows have scales of their own, row 0 opens with its zero block, row 1's products x * id are exact halves in 30 of
    every 32 elements, the last row of three or more is zero)"""
    N, K = x.shape
    live = [float(np.abs(x[n, 32:]).mean()) for n in range(N) if n != 1 and not (N >= 3 and n == N - 1)]
    t = pc.tie_products(x[1])
    return (len(set(live)) == len(live) and min(live) > 0, not x[0, :32].any(), np.count_nonzero(np.abs(t - np.trunc(t)) == 0.5) == K // 32 * 30,
            N < 3 or not x[N - 1].any())


def residual(c):
    rng = np.random.default_rng([SEED, c.M, c.K, c.N, 7])
    r = (rng.standard_normal((c.N, c.M)) * 3.0).astype(np.float32)
    if c.wkind == "zero_group":
        pat = np.array([-0.0, 0.0, np.inf, -np.inf, 0.0, -0.0, -np.inf, np.inf], np.float32)
        for n in range(c.N):
            r[n, 8:16] = np.roll(pat, n)
    return r


def make_table(c):
    """(row_pos, row_slot) of a table case: three slots, slot 1 never touched; positions distinct over ALL rows and out of order; rows 0 and 1
    one slot at consecutive positions (N >= 3; two rows: two slots, descending positions)"""
    d, dh, n_ctx, _, _ = c.rope
    rng = np.random.default_rng([SEED, c.N, d, dh, 3])
    if c.N == 2:
        return np.array([5, 3], np.int32), np.array([2, 0], np.int32)
    while True:
        p0 = int(rng.integers(0, n_ctx - 1))
        rest = [p for p in rng.permutation(n_ctx) if p not in (p0, p0 + 1)][:c.N - 2]
        pos = np.array([p0, p0 + 1] + rest, np.int32)
        if np.any(np.diff(pos) < 0):
            break
    slot = np.array([2, 2] + [0 if i % 2 == 0 else 2 for i in range(c.N - 2)], np.int32)
    return pos, slot


def positions(c):
    """(pos [N], slot [N]) of a ROPE_KV case, table or not"""
    d, dh, n_ctx, n_past, table = c.rope
    if table:
        return make_table(c)
    return np.arange(n_past, n_past + c.N, dtype=np.int32), np.zeros(c.N, np.int32)


def n_slots(c):
    return 3 if c.rope[4] else 1


def silu_buffers(c, rows=None):
    """out_A / out_d before the launch: 0xFF bytes, the blocks that pad F to a chunk zero in rows 0 .. N-1 (a handle zeroes its operand
    rows once and the launch never writes those blocks); two rows more than N"""
    F = c.M // 2
    Fp = (F + 255) // 256 * 256
    rows = c.N + 2 if rows is None else rows
    out_A = np.full((rows, Fp // 4), FILL, np.uint32)
    out_d = np.full((rows, Fp // 32), FILL, np.uint32)
    for b in range(F // 32, Fp // 32):          # (dword (c * 8 + k) * 8 + j holds chain k of block c * 8 + j)
        out_d[:c.N, b] = 0
        out_A[:c.N].reshape(c.N, Fp // 256, 8, 8)[:, b >> 3, :, b & 7] = 0
    return out_A, out_d


def half_amax(act):
    """act [N, F] -> (amax of elements 0 .. 15, amax of elements 16 .. 31) of every block, [N, F/32] each"""
    a = np.abs(act).reshape(act.shape[0], -1, 2, 16).max(axis=3)
    return a[:, :, 0], a[:, :, 1]


def qah_condition(act):
    """each half holds, for some (column, block), the strict block maximum alone: a lost or one-sided exchange changes out_d"""
    lo, hi = half_amax(act)
    return bool((lo > hi).any() and (hi > lo).any())


# ------------------------------------------------------------------------------------------------ operands and references
def _acc(oracle, c, x):
    return oracle.mul_mat_q4_0(gc.weights(c.M, c.K, c.wkind), x, 8)


def rope_rows(oracle, rows, pos, dh):
    """rows [N, d] rotated at pos [N]: one oracle call where the positions are consecutive, else one call per row"""
    N, d = rows.shape
    if N > 1 and np.all(np.diff(pos) == 1):
        return oracle.rope(rows.reshape(N, d // dh, dh), int(pos[0]), 0).reshape(N, d)
    return np.stack([oracle.rope(rows[r].reshape(1, d // dh, dh), int(pos[r]), 0).reshape(d) for r in range(N)])


def build(oracle, c):
    """(ops, want): ops = the op's keyword arguments (binding.op_gemv_set_q4_0) next to w and x; want = what the launch must leave.  SILU_QAH:
    the first draw of x whose reference meets qah_condition (never an excuse: the test asserts the condition on what it runs)"""
    w = gc.weights(c.M, c.K, c.wkind)
    ops, want = dict(epi=c.epi, force=c.force, interleaved=c.epi.startswith("silu")), {}
    with np.errstate(all="ignore"):
        if c.epi in ("store", "resid"):
            x = activation(c)
            acc = _acc(oracle, c, x)
            canary = np.full((c.N, c.M + 5), np.float32(-7.5e33), np.float32)
            canary[:, :c.M] = (np.random.default_rng([SEED, 9]).standard_normal((c.N, c.M)) * 1e6).astype(np.float32)
            ops.update(y_init=canary, y_stride=c.M + 5)
            if c.epi == "resid":
                ops["resid"] = residual(c)
                acc = acc + ops["resid"]                                   # ONE fp32 add
            want.update(y=acc, y_pad=canary[:, c.M:])
        elif c.epi == "rope_kv":
            d, dh, n_ctx, n_past, table = c.rope
            x = activation(c)
            acc = _acc(oracle, c, x)
            pos, slot = positions(c)
            S = n_slots(c)
            Kc, Vc = (np.full((S, n_ctx, d), CANARY, np.uint32).view(np.float32) for _ in range(2))
            ops.update(d=d, dh=dh, n_ctx=n_ctx, n_slots=S, n_past=0 if table else n_past, Kc=Kc, Vc=Vc,
                       row_pos=pos if table else None, row_slot=slot if table else None,
                       qr_init=np.full((c.N, d), CANARY, np.uint32).view(np.float32))
            wK, wV = Kc.copy(), Vc.copy()
            wK[slot, pos] = rope_rows(oracle, acc[:, d:2 * d], pos, dh)
            wV[slot, pos] = acc[:, 2 * d:]
            want.update(qr=rope_rows(oracle, acc[:, :d], pos, dh), Kc=wK, Vc=wV, acc=acc, pos=pos, slot=slot)
        else:
            F = c.M // 2
            for attempt in range(32):
                x = activation(c, attempt)
                acc = _acc(oracle, c, x)
                act, blocks = pc.reference(oracle, "silu_mul", acc[:, :F], acc[:, F:])
                if c.N > SET_MAX or qah_condition(act):          # (both epilogues take the draw the half-block exchange needs)
                    break
            out_A, out_d = silu_buffers(c)
            ops.update(out_A=out_A, out_d=out_d, layer=c.layer, x_prev=x * np.float32(4.0) if c.x_prev else None)
            wA, wd = out_A.copy(), out_d.copy()
            pA, pd = pc.pack_qa(blocks, F)
            wA[:c.N], wd[:c.N] = pA, pd.view(np.uint32)
            want.update(out_A=wA, out_d=wd, act=act, gate=acc[:, :F], up=acc[:, F:])
    ops.update(w=w, x=x)
    return ops, want


# ------------------------------------------------------------------------------------------------ the case table
def _ns(nc, cw):
    g = nc * cw
    return sorted({n for n in (g, g - 1, 2 * g - 1, 2 * g + 1) if 2 <= n <= ROWS_MAX})


def _rope(d, dh, N, n_past=None, table=False, n_ctx=None):
    n_ctx = N + 7 if n_ctx is None else n_ctx
    return (d, dh, n_ctx, (n_ctx - N if n_past is None else n_past), table)


def _cases():
    out = []
    C = lambda group, epi, M, K, N, force=None, wkind=None, rope=None, x_prev=False, layer=0: out.append(Case(
        group, epi, M, K, N, force, wkind or ("zero_group" if epi == "resid" and M >= 16 else "plain"), rope, x_prev, layer))
    for nc, cw in PAIRS:
        for N in _ns(nc, cw):
            for M in (24, 75):
                C("inst", "store", M, 320, N, (nc, cw))
                C("inst", "resid", M, 320, N, (nc, cw))
            for d, dh in ((128, 64), (192, 96)):
                C("inst", "rope_kv", 3 * d, 320, N, (nc, cw), rope=_rope(d, dh, N, 3, table=N <= SET_MAX))
            if cw == 1:
                C("inst", "silu_qa", 448, 320, N, (nc, cw), "silu_zero")
                C("inst", "silu_qah", 448, 320, N, (nc, cw), "silu_zero")
    for cw in (1, 2, 3, 4):
        of_cw = [p for p in PAIRS if p[1] == cw]
        for K in STEP_KS:
            C("steps", "store", 24, K, of_cw[0][0] * cw, of_cw[0])
            C("steps", "resid", 24, K, of_cw[-1][0] * cw, of_cw[-1])
    for M in (6136, 6144, 12280, 12288):
        for N in (2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 60):
            C("auto", "resid", M, 256, N)
    for K in (13824, 22016):
        for N in (8, 16):
            C("auto", "resid", 24, K, N)
    C("auto", "rope_kv", 12288, 256, 9, rope=_rope(4096, 128, 9, n_ctx=16))
    C("auto", "rope_kv", 12288, 256, 9, rope=_rope(4096, 128, 9, table=True, n_ctx=16))
    for M in (1, 5, 13, 4099):
        for K in (64, 320):
            for N in (2, 9):
                C("rows", "store", M, K, N)
                C("rows", "resid", M, K, N)
    for d, dh in ((128, 64), (192, 96), (256, 128), (256, 256)):
        for N in (2, 9, 16, 17, 60):
            for n_past in (0, 5, None):
                C("rope", "rope_kv", 3 * d, 320, N, rope=_rope(d, dh, N, n_past))
            if N <= SET_MAX:
                C("rope", "rope_kv", 3 * d, 320, N, rope=_rope(d, dh, N, 0, table=True))
    for i, F in enumerate((32, 224, 288)):
        for j, K in enumerate((320, 1344)):
            wkind = "wide" if F == 32 or (i + j) % 2 == 0 else "silu_zero"
            for N in (2, 5, 6, 9, 16, 17, 60):
                C("silu", "silu_qa", 2 * F, K, N, wkind=wkind)
                if N <= SET_MAX:
                    C("silu", "silu_qah", 2 * F, K, N, wkind=wkind)
        for N in (5, 16):
            for layer in (0, TAG_MAX_LAYERS - 1):
                C("silu", "silu_qah", 2 * F, 320, N, wkind="wide" if F == 32 else "silu_zero", x_prev=True, layer=layer)
    return out


CASES = _cases()
GROUPS = ("inst", "steps", "auto", "rows", "rope", "silu")
# the host test's yardstick checks run on these (a padded last chunk; seven blocks of SiLU; a table of nine rows)
BASE = Case("base", "store", 24, 1344, 9, None, "plain", None, False, 0)
BASE_SILU = Case("base", "silu_qah", 448, 320, 9, None, "silu_zero", None, False, 0)
BASE_ROPE = Case("base", "rope_kv", 384, 320, 9, None, "plain", _rope(128, 64, 9, 0, table=True), False, 0)
