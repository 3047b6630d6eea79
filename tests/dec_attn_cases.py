"""Cases, edge arithmetic and references for tests/test_gpu_dec_attn_op.py (and the CPU checks of tests/test_dec_attn_op_host.py): the one-row
decode attention through the kernels that hand data between workgroups inside a launch (llamahip_op_dec_attention), against the oracle bit
for bit.  Nothing here needs a GPU.

A case is Case(path, regime, H, dh, n_ctx, n_past, nth, force): ONE step of path "x" (k_dec_attn_x), "stream" (k_dec_pv_stream) or "dma"
(k_dec_pv_dma) on inputs attn_cases.make(regime, 1, ...); force None (the library's rule) or (split, stage_rows, ns) with 0 = the rule.
A sequence is Seq(path, H, dh, n_ctx, nth, force, epoch0, steps) with steps ((regime, n_past, layer, bump_epoch), ...): several steps on ONE
set of hand-off buffers (counters, tagged partial sums, epoch word), which the op zeroes once and never clears.

The tables X_CASES / STREAM_CASES / DMA_CASES are the committed output of find_x() / find_stream() / find_dma(): a greedy cover, smallest
shape first, of the features each kernel can go wrong at (x_features / stream_features / dma_features name them from the launch plan and
CPU arithmetic that restates the kernels' index computations).  tests/test_dec_attn_op_host.py asserts that the tables equal what the
searches return and that every feature has its case.  Splits are kept to one round of workgroups (at most 256), as the library's rule
keeps them: a workgroup that collects partial sums waits for workgroups dispatched before it.

References: attn_cases.oracle_side step by step on the evolving caches; the wo operand is oracle.quantize_row of its merged row; the float64
bound of tests/attn_ref.py on every plain, wide and zeroq step."""
import collections

import numpy as np

import attn_cases

SEED = 29
Case = collections.namedtuple("Case", "path regime H dh n_ctx n_past nth force")
Seq = collections.namedtuple("Seq", "path H dh n_ctx nth force epoch0 steps")
TAG_MAX_LAYERS = 250
ONE_ROUND = 256                      # workgroups of one round: the library's rule never splits beyond


def case_id(c):
    f = "" if not c.force else "-f" + "x".join(str(v) for v in c.force)
    return f"{c.path}-{c.regime}-H{c.H}x{c.dh}-ctx{c.n_ctx}-p{c.n_past}-t{c.nth}{f}"


def seq_id(s):
    return f"{s.path}-H{s.H}x{s.dh}-ctx{s.n_ctx}-t{s.nth}-e{s.epoch0:x}-" + "_".join(f"{p}l{l}{'b' if b else ''}" for _, p, l, b in s.steps)


def split_valid(nth, split):
    cpw = -(-nth // split)
    return 1 <= split <= nth and (split - 1) * cpw < nth


# ------------------------------------------------------------------------------------------------ edge arithmetic (restated from the kernels)
def chains(n_past, nth):
    """[(first row, end row)] of the nth key chains of a step (empty where first >= end)"""
    T = n_past + 1
    dc = -(-T // nth)
    return [(dc * th, min(dc * th + dc, T)) for th in range(nth)]


def x_features(c):
    """k_dec_attn_x: the early V prefetch of chain `sub` is taken iff the chain is not empty and min(first + 31, end - 1) < n_past -- only the
    chain that ends in the new row can fail it, and fails it iff it is at most 32 rows long; score slices of 32 keys"""
    ch = [(a, b) for a, b in chains(c.n_past, c.nth) if a < b]
    a, b = ch[-1]
    f = {("shape", c.H, c.dh), ("n_ctx", c.n_ctx), ("nth", c.nth), ("n_past", "last" if c.n_past == c.n_ctx - 1 else c.n_past),
         ("early", c.nth, min(a + 31, b - 1) < c.n_past), ("nth at n_past", c.nth, "last" if c.n_past == c.n_ctx - 1 else c.n_past)}
    if c.n_past + 1 < c.nth:
        f.add(("empty_chains", c.nth))
    if c.n_past % 32 == 31:
        f.add(("slice", "last key of a slice"))
    if c.n_past % 32 == 0 and c.n_past:
        f.add(("slice", "first key of a slice"))
    if c.n_past % 32 == 1 and c.n_past > 32:
        f.add(("slice", "second key of a slice"))
    return f


def stream_geometry(c, plan):
    T = c.n_past + 1
    dc = -(-T // c.nth)
    last = c.nth - (plan.split - 1) * plan.cpw
    return dict(dc=dc, nstage=-(-dc // plan.SR), ragged=plan.split > 1 and last < plan.cpw)


def stream_features(c, plan):
    g = stream_geometry(c, plan)
    f = {("shape", c.H, c.dh), ("n_ctx", c.n_ctx), ("stage_rows", c.force[1] if c.force and c.force[1] else "rule"),
         ("n_past", "last" if c.n_past == c.n_ctx - 1 else "nth-2" if c.n_past == c.nth - 2 and c.n_past > 0 else c.n_past),
         ("stages", "one" if g["nstage"] == 1 else "two" if g["nstage"] == 2 else "odd" if g["nstage"] % 2 else "even")}
    if c.n_past == c.n_ctx - 1:                              # (a split counts where every chain has rows to walk: the cache's last position)
        f.add(("pair", c.nth, plan.split if c.force and c.force[0] else "rule"))
        if g["ragged"]:
            f.add(("ragged last workgroup",))
        if plan.split > 1 and c.n_ctx >= 2048 and not (c.force and c.force[1]):
            f.add(("split chains over a long context at the rule's stage rows", c.nth))
    if c.n_past + 1 < c.nth:
        f.add(("empty_chains",))
    return f


def dma_geometry(c, plan):
    """k_dec_pv_dma: stages of 8 rows per chain in a ring of NS slots; a loader lets F = 60 / (2 nloc) stages be outstanding; the tail clamp is
    taken at stage s iff (s + 2) 8 + dc nth > n_ctx"""
    T = c.n_past + 1
    dc = -(-T // c.nth)
    nstage = -(-dc // 8)
    last = c.nth - (plan.split - 1) * plan.cpw
    return dict(dc=dc, nstage=nstage, wrapped=nstage > plan.NS, tail=(nstage + 1) * 8 + dc * c.nth > c.n_ctx, ragged=plan.split > 1 and last < plan.cpw,
                F={n: 60 // (2 * n) for n in {plan.cpw, last}})


def dma_features(c, plan):
    g = dma_geometry(c, plan)
    f = {("shape", c.H, c.dh), ("n_ctx", c.n_ctx), ("ns", c.force[2] if c.force and c.force[2] else "rule"), ("ring", "wrapped" if g["wrapped"] else "not wrapped")}
    full = c.n_past >= c.n_ctx // 2                          # (a thread count, a split count where every chain has rows to walk)
    if full:
        f |= {("nth", c.nth), ("cpw", plan.cpw), ("ring", c.nth, "wrapped" if g["wrapped"] else "not wrapped")}
    for nloc, F in g["F"].items():
        f.add(("F", nloc, "more stages than F" if g["nstage"] > F else "at most F stages"))
    if g["tail"]:
        f.add(("tail clamp",))
    if g["tail"] and not (c.force and c.force[2]) and c.n_past == c.n_ctx - 1 and c.n_ctx >= 2048:
        f.add(("tail clamp at the rule's NS", c.n_ctx))
    if g["ragged"] and full:
        f.add(("ragged last workgroup", c.nth, plan.split))
    if c.n_past + 1 < c.nth:
        f.add(("empty_chains",))
    if c.n_past == 0:
        f.add(("n_past", 0))
    return f


# ------------------------------------------------------------------------------------------------ the searches
def greedy_cover(cands, feats):
    """the candidates (in their given order: smallest first) that cover every feature some candidate has: repeatedly the one with the most
    uncovered features, the earliest among equals"""
    want = set().union(*feats)
    chosen = []
    while want:
        best = max(range(len(cands)), key=lambda i: (len(feats[i] & want), -i))
        chosen.append(best)
        want -= feats[best]
    return [cands[i] for i in sorted(chosen)]


X_SHAPES = ((8, 32), (16, 64), (8, 128), (8, 256), (32, 128))
X_CTX = (64, 100, 1024)
X_NTH = (1, 2, 3, 5, 8)


def find_x():
    cands = []
    for n_ctx in X_CTX:
        for H, dh in X_SHAPES:
            for nth in X_NTH:
                for n_past in (0, 1, 30, 31, 32, 33, 63, 64, n_ctx - 1):
                    if n_past < n_ctx:
                        cands.append(Case("x", "plain", H, dh, n_ctx, n_past, nth, None))
    cands = list(dict.fromkeys(cands))
    feats = [x_features(c) | {("shape_ctx", c.H, c.dh, c.n_ctx)} for c in cands]
    return greedy_cover(cands, feats)


STREAM_SHAPES = ((8, 32), (4, 64), (2, 128), (8, 128))
STREAM_CTX = (100, 2048, 4096)
STREAM_NTH = (1, 2, 3, 5, 8, 17, 32)
STREAM_SPLITS = (1, 2, 3, 4, 8, 16, 32)
STREAM_SR = (1, 2, 3, 0)


def find_stream(plan_of):
    """plan_of(case) -> DecAttnPlan (the library's: llama_swift_amd.dec_attn_plan through case_plan)"""
    cands = []
    for n_ctx in STREAM_CTX:
        for H, dh in STREAM_SHAPES:
            for nth in STREAM_NTH:
                for split in (0,) + STREAM_SPLITS:
                    if split and (not split_valid(nth, split) or H * (dh // 32) * split > ONE_ROUND):
                        continue
                    for sr in STREAM_SR:
                        for n_past in (0, nth - 2, 1023, 1024, n_ctx - 1):
                            # (short stages walk a long context in hundreds of barriers: the forced stage rows stay at the small context)
                            if 0 <= n_past < n_ctx and not (sr and n_ctx > 100):
                                cands.append(Case("stream", "plain", H, dh, n_ctx, n_past, nth, (split, sr, 0) if split or sr else None))
    cands = list(dict.fromkeys(cands))
    feats = [stream_features(c, plan_of(c)) for c in cands]
    return greedy_cover(cands, feats)


DMA_SHAPES = ((8, 128), (16, 128))
DMA_CTX = (400, 1001, 2048, 4096)
DMA_NTH = (1, 2, 3, 5, 6, 7, 8, 9, 24, 32)
DMA_NS = (2, 3, 0)


def find_dma(plan_of):
    cands = []
    for n_ctx in DMA_CTX:
        for H, dh in DMA_SHAPES:
            for nth in DMA_NTH:
                for split in range(0, 33):
                    if split and (not split_valid(nth, split) or -(-nth // split) > 3 or H * split > ONE_ROUND):
                        continue
                    for ns in DMA_NS:
                        for n_past in (0, nth - 2, n_ctx // 2, n_ctx - 1):
                            if 0 <= n_past < n_ctx:
                                cands.append(Case("dma", "plain", H, dh, n_ctx, n_past, nth, (split, 0, ns) if split or ns else None))
    cands = [c for c in dict.fromkeys(cands) if plan_of(c) is not None]          # (the rule's split of a thread count may leave more than 3 chains: not this kernel's)
    feats = [dma_features(c, plan_of(c)) for c in cands]
    must = {("ragged last workgroup", 5, 2), ("ragged last workgroup", 7, 3)}
    assert must <= set().union(*feats)
    return greedy_cover(cands, feats)


def case_plan(L, c):
    """the plan the library reports for a case (None where it refuses): what the GPU test asserts ran"""
    f = c.force or (0, 0, 0)
    force = dict(split=f[0], stage_rows=f[1], ns=f[2], dma={"x": -1, "stream": 0, "dma": 1}[c.path])
    try:
        return L.dec_attn_plan(c.H * c.dh, c.H, c.n_ctx, c.nth, long_ctx=c.path != "x", have_sync=c.path == "x", have_xpart=c.path != "x", force=force)
    except L.LlamaHipError:
        return None


# ------------------------------------------------------------------------------------------------ the committed tables
def _cases(path, rows):
    return [Case(path, "plain", *r) for r in rows]


# find_x(): (H, dh, n_ctx, n_past, nth, force); force = (split, stage_rows, ns)
X_CASES = _cases("x", [
    (8, 32, 64, 0, 1, None), (8, 32, 64, 1, 1, None), (8, 32, 64, 31, 1, None), (8, 32, 64, 32, 1, None), (8, 32, 64, 33, 1, None),
    (8, 32, 64, 1, 2, None), (8, 32, 64, 30, 2, None), (8, 32, 64, 31, 2, None), (8, 32, 64, 32, 2, None), (8, 32, 64, 33, 2, None),
    (8, 32, 64, 0, 3, None), (8, 32, 64, 30, 3, None), (8, 32, 64, 31, 3, None), (8, 32, 64, 32, 3, None), (8, 32, 64, 33, 3, None),
    (8, 32, 64, 1, 5, None), (8, 32, 64, 30, 5, None), (8, 32, 64, 31, 5, None), (8, 32, 64, 33, 5, None), (8, 32, 64, 1, 8, None),
    (8, 32, 64, 30, 8, None), (8, 32, 64, 31, 8, None), (8, 32, 64, 32, 8, None), (16, 64, 64, 63, 1, None), (8, 128, 64, 30, 1, None),
    (8, 256, 64, 32, 5, None), (32, 128, 64, 33, 8, None), (8, 32, 100, 63, 1, None), (8, 32, 100, 63, 2, None), (8, 32, 100, 64, 2, None),
    (8, 32, 100, 63, 3, None), (8, 32, 100, 64, 3, None), (8, 32, 100, 63, 5, None), (8, 32, 100, 64, 5, None), (8, 32, 100, 63, 8, None),
    (8, 32, 100, 64, 8, None), (16, 64, 100, 0, 2, None), (8, 128, 100, 64, 1, None), (8, 256, 100, 99, 2, None),
    (32, 128, 100, 0, 5, None), (8, 32, 1024, 1023, 3, None), (16, 64, 1024, 1023, 5, None), (8, 128, 1024, 1, 3, None),
    (8, 256, 1024, 0, 8, None), (32, 128, 1024, 1023, 8, None),
])
# find_stream()
STREAM_CASES = _cases("stream", [
    (8, 32, 100, 99, 1, (0, 2, 0)), (8, 32, 100, 99, 1, (1, 1, 0)), (8, 32, 100, 99, 2, (1, 1, 0)), (8, 32, 100, 99, 2, (2, 1, 0)),
    (8, 32, 100, 1, 3, (0, 1, 0)), (8, 32, 100, 99, 3, (1, 1, 0)), (8, 32, 100, 99, 3, (2, 1, 0)), (8, 32, 100, 99, 3, (3, 1, 0)),
    (8, 32, 100, 99, 5, (1, 1, 0)), (8, 32, 100, 99, 5, (2, 1, 0)), (8, 32, 100, 99, 5, (3, 1, 0)), (8, 32, 100, 99, 8, (1, 1, 0)),
    (8, 32, 100, 99, 8, (2, 1, 0)), (8, 32, 100, 99, 8, (3, 1, 0)), (8, 32, 100, 99, 8, (4, 1, 0)), (8, 32, 100, 99, 8, (8, 1, 0)),
    (8, 32, 100, 99, 17, (1, 1, 0)), (8, 32, 100, 99, 17, (3, 1, 0)), (8, 32, 100, 99, 17, (4, 1, 0)), (8, 32, 100, 99, 32, (1, 1, 0)),
    (8, 32, 100, 99, 32, (2, 1, 0)), (8, 32, 100, 99, 32, (3, 1, 0)), (8, 32, 100, 99, 32, (4, 1, 0)), (8, 32, 100, 99, 32, (8, 1, 0)),
    (8, 32, 100, 99, 32, (16, 1, 0)), (8, 32, 100, 99, 32, (32, 1, 0)), (4, 64, 100, 0, 2, (0, 1, 0)), (8, 128, 100, 99, 17, (0, 3, 0)),
    (8, 32, 2048, 1023, 1, None), (8, 32, 2048, 1024, 1, None), (8, 32, 2048, 2047, 3, None), (8, 32, 2048, 2047, 5, None),
    (8, 32, 2048, 2047, 8, None), (8, 32, 2048, 2047, 17, (2, 0, 0)), (8, 32, 2048, 2047, 32, None), (2, 128, 4096, 4095, 2, None),
])
# find_dma()
DMA_CASES = _cases("dma", [
    (8, 128, 400, 200, 1, None), (8, 128, 400, 0, 2, (0, 0, 2)), (8, 128, 400, 200, 2, (0, 0, 2)), (8, 128, 400, 200, 2, None),
    (8, 128, 400, 200, 3, None), (8, 128, 400, 200, 5, (0, 0, 2)), (8, 128, 400, 200, 5, (3, 0, 0)), (8, 128, 400, 200, 6, (0, 0, 2)),
    (8, 128, 400, 200, 6, None), (8, 128, 400, 200, 7, None), (8, 128, 400, 200, 8, None), (8, 128, 400, 200, 8, (3, 0, 2)),
    (8, 128, 400, 200, 9, (3, 0, 3)), (8, 128, 400, 200, 9, (5, 0, 2)), (8, 128, 400, 200, 24, (0, 0, 2)),
    (8, 128, 400, 399, 24, (0, 0, 2)), (16, 128, 400, 200, 32, (11, 0, 2)), (8, 128, 1001, 1000, 7, (3, 0, 3)),
    (8, 128, 1001, 1000, 32, (0, 0, 2)), (8, 128, 2048, 2047, 3, None), (8, 128, 4096, 4095, 1, None),
])

# every regime at two shapes per kernel family (x), and the regimes whose V*P chains and merges go wrong first on the split kernels: one
# case whose ring wraps (ns 2) and one whose ring holds the whole chain, each
REGIME_CASES = (
    [Case("x", r, 8, 128, 100, 70, 5, None) for r in attn_cases.REGIMES] + [Case("x", r, 16, 64, 1024, 700, 8, None) for r in attn_cases.REGIMES]
    + [Case("stream", r, 8, 32, 2048, 1500, 8, (4, 0, 0)) for r in attn_cases.REGIMES]
    + [Case("dma", r, 8, 128, 1001, 900, 7, (3, 0, 2)) for r in ("negzero", "wide", "ties", "zeroq")]
    + [Case("dma", r, 8, 128, 1001, 300, 8, None) for r in ("negzero", "wide", "ties", "leak")])

# several steps on one set of hand-off buffers
SEQS = [
    # the counters of a head are cleared by its last soft_max . V workgroup: positions 29 .. 35 one after another (a slice edge in the middle)
    Seq("x", 8, 32, 64, 3, None, 0, tuple(("plain", p, 0, 0) for p in range(29, 36))),
    Seq("x", 16, 64, 1024, 8, None, 0, (("plain", 900, 0, 0), ("negzero", 3, 1, 0))),          # 29 arrivals per head, then 1
    # tagged partial sums: layers 0 and 1 under one epoch, then after a bump layer 0 again at a LOWER position (its granules hold the old tag)
    Seq("stream", 8, 32, 2048, 8, (8, 0, 0), 0, (("plain", 1500, 0, 1), ("plain", 1501, 1, 0), ("negzero", 40, 0, 1))),
    Seq("dma", 8, 128, 1001, 7, (3, 0, 2), 0, (("plain", 900, 0, 1), ("wide", 901, 1, 0), ("plain", 5, 0, 1))),
    Seq("dma", 8, 128, 2048, 8, None, 5, (("plain", 2047, 0, 0), ("plain", 2046, 1, 0), ("ties", 17, 0, 1))),
    # the epoch crosses its 24-bit wrap (k_bump_epoch skips the epoch whose low 24 bits are zero), at the last layer index the tags carry
    Seq("dma", 8, 128, 400, 5, (2, 0, 3), 0x00FFFFFE, (("plain", 399, TAG_MAX_LAYERS - 1, 1), ("plain", 200, TAG_MAX_LAYERS - 1, 1), ("plain", 100, TAG_MAX_LAYERS - 1, 1))),
    Seq("stream", 2, 128, 100, 5, (3, 2, 0), 0x00FFFFFE, (("plain", 99, 7, 1), ("plain", 50, 7, 1), ("plain", 3, 7, 1))),
]


def next_epoch(e):
    e = (e + 1) & 0xFFFFFFFF
    return (e + 1) & 0xFFFFFFFF if e & 0xFFFFFF == 0 else e


# ------------------------------------------------------------------------------------------------ inputs and references
def first_inputs(regime, H, dh, n_ctx, n_past):
    return attn_cases.make(regime, 1, H * dh, H, n_past, n_ctx, seed=SEED)


def seq_inputs(s):
    """(the steps as the op takes them, Kc, Vc): the caches are the first step's; later steps bring their q|k|v row only"""
    steps, Kc, Vc = [], None, None
    for regime, n_past, layer, bump in s.steps:
        qkv, K0, V0 = first_inputs(regime, s.H, s.dh, s.n_ctx, n_past)
        if Kc is None:
            Kc, Vc = K0, V0
        steps.append((qkv[0], n_past, layer, bump))
    return steps, Kc, Vc


def reference(oracle, steps, Kc, Vc, H, nth):
    """[(merged [d], wo operand [d/32, 20], rotated q [1, d], K, V after the step)] per step, caches evolving; and the final caches"""
    out = []
    for qkv, n_past, _, _ in steps:
        want, Kc, Vc, qr = attn_cases.oracle_side(oracle, qkv[None, :], Kc, Vc, H, n_past, nth)
        out.append((want[0], oracle.quantize_row(want[0]).reshape(-1, 20), qr, Kc, Vc))
    return out, Kc, Vc


def scores(qr, K, H, n_past):
    """float64 scores [H][T] of the step's rotated query against the rotated keys (exact where the regime makes them exact)"""
    d = qr.shape[1]
    T = n_past + 1
    return np.einsum("hi,thi->ht", qr.astype(np.float64).reshape(H, d // H), K[:T].astype(np.float64).reshape(T, H, d // H))


def regime_property(regime, qr, K, merged, H, n_past):
    """None where the input has the property its regime is named for, else what is missing"""
    dh = qr.shape[1] // H
    s = scores(qr, K, H, n_past) * np.float64(np.float32(1.0) / np.sqrt(np.float32(dh)))
    if regime == "ties":
        n = (s == s.max(axis=1, keepdims=True)).sum(axis=1)
        return None if n.min() >= 2 else f"heads with one key at the maximum: {np.argwhere(n < 2).ravel().tolist()}"
    if regime == "wide":
        x = (s.astype(np.float32) - s.astype(np.float32).max(axis=1, keepdims=True)).astype(np.float16)
        with np.errstate(under="ignore"):
            e = np.exp(x.astype(np.float32)).astype(np.float16)
        return None if np.any(e == 0) and np.any((e > 0) & (e < np.float16(2.0 ** -14))) else "no exp-table entry of 0 and a subnormal one"
    if regime == "negzero":
        return None if np.any(merged.view(np.uint32) == 0x80000000) else "no merged column is -0"
    if regime == "zeroq":
        return None if not qr.any() else "q is not zero"
    return None


# ================================================================================================ the fused launch (k_qkv_attn)
# A case is QkvCase(regime, d, H, n_ctx, n_past, nth, nparts): ONE step of llamahip_op_qkv_attn.  The activation row is
# prep_cases.reference(oracle, "norm", ...) of gemv_cases.norm_row (order-proof under both forms of the second moment, so NORM and NORMP
# with any number of parts give the same row), the q|k|v row oracle.mul_mat_q4_0 on gemv_cases.q4_random weights, then oracle_side.  The
# mat-vec makes the new token's q, k and v, so the value regimes live in the OLD cache rows (and in weight rows whose scales are zero):
#   ties     rows 0 and 2 of every head are the same multiple of the head's rotated query, scaled to score above every other key
#   wide     the old keys scaled to a score spread of ~40
#   negzero  attn_cases' V columns in the old rows, and EVERY old key the same multiple of the query, so far above the new key that its weight
#            is exactly 0 and every old key weighs 1 / n_past: every chain of a -2^-149 column ends in -0, and so does the merged column
#            wherever the new token's own v is negative (+0 times a positive v would turn the last chain to +0)
#   zeroq    the scales of every second head's q rows are zero (gemv_cases.set_d): uniform weights in those heads
#   leak     comes free: rows above n_past hold the NaN canary
import functools                                                               # noqa: E402

import gemv_cases as gc                                                        # noqa: E402
import prep_cases as pc                                                        # noqa: E402

QkvCase = collections.namedtuple("QkvCase", "regime d H n_ctx n_past nth nparts")
QkvSeq = collections.namedtuple("QkvSeq", "d H n_ctx nth epoch0 steps")          # steps ((n_past, layer, bump_epoch, nparts), ...)
QKV_REGIMES = ("plain", "ties", "wide", "negzero", "zeroq")


def qkv_case_id(c):
    return f"qkv-{c.regime}-d{c.d}-H{c.H}-ctx{c.n_ctx}-p{c.n_past}-t{c.nth}-parts{c.nparts}"


def qkv_seq_id(s):
    return f"qkv-d{s.d}-H{s.H}-ctx{s.n_ctx}-t{s.nth}-e{s.epoch0:x}-" + "_".join(f"{p}l{l}{'b' if b else ''}n{n}" for p, l, b, n in s.steps)


def find_qkv_widths(plan_of):
    """the smallest d (a multiple of 256 up to 8192) per instance (depth, pg) of k_qkv_attn, with the largest H <= 64 it takes there"""
    out = {}
    for d in range(256, 8192 + 1, 256):
        for H in (64, 56, 48, 40, 32, 24, 16, 8):
            p = plan_of(d, H) if d % H == 0 else None
            if p and p[1:3] not in out:
                out[p[1:3]] = (d, H)
    return out


# find_qkv_widths(): smaller than the 13B / 65B widths (5120, 8192) that run the same two instances -- a weight upload is 40 / 71 MB there
QKV_WIDTHS = {(8, 1): (4096, 64), (10, 2): (4608, 48), (4, 2): (6144, 64)}


def qkv_features(c):
    ch = [(a, b) for a, b in chains(c.n_past, c.nth) if a < b]
    a, b = ch[-1]
    return {("H", c.H), ("nth", c.nth), ("n_past", c.n_past), ("n_ctx", c.n_ctx), ("parts", c.nparts), ("regime", c.regime), ("H nth", c.H, c.nth),
            ("H regime", c.H, c.regime), ("early", c.nth, min(a + 31, b - 1) < c.n_past), ("parts n_past", c.nparts, c.n_past), ("H n_past", c.H, c.n_past)}


def find_qkv():
    cands = [QkvCase(r, 4096, H, n_ctx, n_past, nth, parts) for n_ctx in (1280, 2048) for H in (16, 32, 64, 128) for nth in (1, 3, 5, 8)
             for n_past in (0, 31, 32, 33, 500, 1279) for parts in (0, 1, 64, 512) for r in QKV_REGIMES
             if not (r in ("ties", "wide", "negzero") and n_past < 31)                 # (the old-row regimes need old rows ...
             and not (r == "negzero" and any(a >= b for a, b in chains(n_past, nth)))]     # ... and an empty chain's +0 would turn a -0 sum to +0)
    return greedy_cover(cands, [qkv_features(c) for c in cands])


def _qkv(rows):
    return [QkvCase(*r) for r in rows]


# find_qkv(): (regime, d, H, n_ctx, n_past, nth, nparts)
QKV_CASES = _qkv([
    ('plain', 4096, 16, 1280, 0, 1, 0), ('zeroq', 4096, 16, 1280, 32, 1, 512), ('plain', 4096, 16, 1280, 33, 1, 64),
    ('negzero', 4096, 16, 1280, 500, 3, 0), ('ties', 4096, 16, 1280, 1279, 5, 0), ('wide', 4096, 16, 1280, 31, 8, 0),
    ('plain', 4096, 32, 1280, 32, 1, 0), ('negzero', 4096, 32, 1280, 33, 1, 1), ('plain', 4096, 32, 1280, 1279, 1, 1),
    ('zeroq', 4096, 32, 1280, 0, 5, 1), ('wide', 4096, 32, 1280, 500, 8, 1), ('plain', 4096, 64, 1280, 0, 1, 64),
    ('negzero', 4096, 64, 1280, 500, 1, 64), ('plain', 4096, 64, 1280, 1279, 1, 64), ('ties', 4096, 64, 1280, 31, 3, 64),
    ('wide', 4096, 64, 1280, 32, 5, 64), ('zeroq', 4096, 64, 1280, 33, 8, 0), ('plain', 4096, 128, 1280, 0, 1, 512),
    ('negzero', 4096, 128, 1280, 500, 1, 512), ('plain', 4096, 128, 1280, 1279, 1, 512), ('ties', 4096, 128, 1280, 31, 3, 512),
    ('wide', 4096, 128, 1280, 32, 5, 1), ('zeroq', 4096, 128, 1280, 33, 8, 512), ('ties', 4096, 32, 2048, 31, 3, 1),
])
# the other two instances at QKV_WIDTHS' shapes (head size 96), three cases each
QKV_WIDE_CASES = _qkv([
    ("plain", 4608, 48, 1280, 700, 8, 1), ("ties", 4608, 48, 1280, 33, 5, 0), ("negzero", 4608, 48, 1280, 1279, 8, 64),
    ("plain", 6144, 64, 1280, 700, 8, 1), ("ties", 6144, 64, 1280, 33, 3, 0), ("negzero", 6144, 64, 1280, 1279, 8, 512),
])
QKV_SEQS = [
    # layers 0, 1 and the last one the tags carry, under one epoch
    QkvSeq(4096, 32, 1280, 8, 0, ((100, 0, 1, 1), (101, 1, 0, 0), (102, TAG_MAX_LAYERS - 1, 0, 64))),
    # the epoch across its 24-bit wrap, a bump per step
    QkvSeq(4096, 32, 1280, 8, 0x00FFFFFE, ((40, 0, 1, 1), (41, 0, 1, 1), (42, 0, 1, 0))),
    # position 600, then on the same layer after a bump position 2: sc2 holds 598 stale granules with the old tag
    QkvSeq(4096, 32, 1280, 8, 0, ((600, 3, 1, 1), (2, 3, 1, 1))),
]


@functools.lru_cache(maxsize=2)
def qkv_weights(d, zeroq_H=0):
    rng = np.random.default_rng([SEED, d, 3])
    m = gc.q4_random(rng, 3 * d, d, 1.0 / np.sqrt(21.0 * d))
    if zeroq_H:
        dh = d // zeroq_H
        for h in range(0, zeroq_H, 2):
            gc.set_d(m, slice(h * dh, h * dh + dh), 0.0)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=2)
def _base_caches(d, n_ctx):
    rng = np.random.default_rng([SEED, d, n_ctx, 4])
    K = rng.standard_normal((n_ctx, d), np.float32)
    V = rng.standard_normal((n_ctx, d), np.float32)
    K.setflags(write=False)
    V.setflags(write=False)
    return K, V


def qkv_x(d, step=0):
    """the residual-stream row of a step: order-proof under both forms of the second moment (the host test asserts it), each step its own scale"""
    return gc.norm_row(d, "normal:1") * np.float32(1.0 + 0.25 * step)


def qkv_row(oracle, w, x, norm_w):
    row = pc.reference(oracle, "norm", x[None, :], norm_w)[0][0]
    return oracle.mul_mat_q4_0(w, row[None, :])[0]


def _dominate(K, V, qkv, oracle, H, n_past, rows, margin):
    """the old key rows `rows` of every head become the same multiple of the head's rotated query, scoring `margin` above every other visible
    key (identical rows score identically whatever the order of the fp32 dot product: exact ties)"""
    d = qkv.size // 3
    dh = d // H
    _, Kn, _, qr = attn_cases.oracle_side(oracle, qkv[None, :], K, V, H, n_past, 1)
    s = scores(qr, Kn, H, n_past) / np.sqrt(dh)
    q = qr.reshape(H, dh).astype(np.float64)
    for h in range(H):
        alpha = (np.delete(s[h], rows).max() + margin) * np.sqrt(dh) / (q[h] @ q[h])
        K[rows, h * dh:(h + 1) * dh] = (alpha * q[h]).astype(np.float32)


def qkv_inputs(oracle, c):
    """(w, norm_w, x, part_in, Kc, Vc, the q|k|v row the mat-vec must produce) of a case"""
    w = qkv_weights(c.d, c.H if c.regime == "zeroq" else 0)
    norm_w, x = gc.norm_weight(c.d), qkv_x(c.d)
    qkv = qkv_row(oracle, w, x, norm_w)
    K0, V0 = _base_caches(c.d, c.n_ctx)
    Kc = np.full((c.n_ctx, c.d), attn_cases._f(attn_cases.CANARY), np.float32)
    Vc = Kc.copy()
    Kc[:c.n_past], Vc[:c.n_past] = K0[:c.n_past], V0[:c.n_past]
    if c.regime == "wide":
        _, Kn, _, qr = attn_cases.oracle_side(oracle, qkv[None, :], Kc, Vc, c.H, c.n_past, 1)
        Kc[:c.n_past] *= np.float32(8.0 / (scores(qr, Kn, c.H, c.n_past)[:, :c.n_past] / np.sqrt(c.d // c.H)).std())
    if c.regime == "negzero":
        Vc[:c.n_past] = attn_cases.make("negzero", 1, c.d, c.H, c.n_past, c.n_ctx, seed=SEED)[2][:c.n_past]
        _dominate(Kc, Vc, qkv, oracle, c.H, c.n_past, list(range(c.n_past)), 40.0)
    if c.regime == "ties":
        _dominate(Kc, Vc, qkv, oracle, c.H, c.n_past, [0, 2], 1.0)
    return w, norm_w, x, (gc.norm_parts(x, c.nparts) if c.nparts else None), Kc, Vc, qkv


def qkv_regime_property(c, qkv, qr, K, merged):
    if c.regime == "zeroq":
        dh = c.d // c.H
        q = qkv[:c.d].reshape(c.H, dh)
        return None if not q[::2].any() and q[1::2].any() else "the q rows of every second head are not exactly zero"
    return regime_property(c.regime, qr, K, merged, c.H, c.n_past)
