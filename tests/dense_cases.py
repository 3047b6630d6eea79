"""The yardstick and the case tables of the f16 / f32 op tests: tests/test_dense_op_host.py (CPU), tests/test_gpu_dense_mv_op.py,
tests/test_gpu_dense_prep_op.py and tests/test_gpu_dense_embed_op.py.  Nothing here needs a GPU.

The yardstick.  ggml_compute_forward_mul_mat_f16_f32 rounds every activation to fp16 once (RNE; overflow to inf, subnormals kept) and
then every output is ggml_vec_dot_f16 of the widened halves; the f32 mat-mul is ggml_vec_dot_f32 on the values as they are.  Both are 32
fp32 FMA chains (chain c = elements c, c + 32, ...) folded by GGML_F32x8_REDUCE, which the project's CPU oracle states with real fmaf
(orc_vec_dot_f32).  So  y[n][m] = vec_dot_f32(widen(w[m]), act(x[n])),  and with a residual one fp32 add follows.
tests/test_dense_op_host.py holds this against the reference build's own mat-mul for every case below, at 1 and 8 threads.

Comparison rule (`differ`).  The arithmetic and its order are the reference's, so finite values compare bit for bit and no tolerance
exists anywhere; a non-finite value compares by class -- NaN, +inf, -inf -- because which NaN an inf - inf or an inf * 0 leaves is the
producer's choice."""
import numpy as np

F32 = np.float32
GUARD = 8                                   # guard columns behind the M outputs of a row of y
WNAMES = {0: "f32", 1: "f16"}
FULL_MAX = 4096                             # reference outputs up to this many floats are stored whole, larger ones as a digest


# ------------------------------------------------------------------------------------------------ the yardstick
def wdtype(wtype):
    return np.float16 if wtype == 1 else np.float32


def act(x, wtype):
    """what the mat-mul makes of an activation: f32 weights nothing; f16 weights ONE rounding to fp16 (RNE, overflow to inf, subnormals kept)"""
    x = np.asarray(x, F32)
    if wtype == 0:
        return x
    with np.errstate(over="ignore"):
        return x.astype(np.float16).astype(F32)


def widen(w):
    return np.ascontiguousarray(w).astype(F32)


def yardstick(oracle, w, x, resid, wtype):
    """y f32 [N, M]: every output oracle.vec_dot_f32(widen(w[m]), act(x[n])) (orc_mul_mat_dense is that loop), then one fp32 add of resid"""
    with np.errstate(all="ignore"):
        y = oracle.mul_mat_dense(widen(w), np.ascontiguousarray(act(x, wtype)))
        return y if resid is None else (y + np.asarray(resid, F32)).astype(F32)


def differ(got, want):
    """indices where `got` is not `want` under the comparison rule: finite wanted values bit for bit, non-finite ones by class"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape, (got.shape, want.shape)
    with np.errstate(invalid="ignore"):
        ok = np.where(np.isfinite(want), got.view(np.uint32) == want.view(np.uint32),
                      (np.isnan(want) & np.isnan(got)) | (np.isinf(want) & (got == want)))
    return np.argwhere(~ok)


def first_diff(got, want):
    bad = differ(got, want)
    if not len(bad):
        return "equal"
    i = tuple(bad[0])
    g, w = np.asarray(got, F32)[i], np.asarray(want, F32)[i]
    return f"{len(bad)} of {np.asarray(want).size} differ, first at {i}: got {g!r} ({g.view(np.uint32):#010x}), want {w!r} ({w.view(np.uint32):#010x})"


def canon(a):
    """the array with every NaN replaced by one NaN: equal bytes <=> equal under the comparison rule (for digests of large outputs)"""
    a = np.array(a, F32)
    a[np.isnan(a)] = np.uint32(0x7FC00000).view(F32)
    return a


def perm_index(e, K):
    """Where element e of a row of K lies in the kernels' operand order (dense.hip's header comment): the row is cut into groups of 256
    elements = 8 steps of the 32 chains, a tail group of K % 256 elements has st = (K % 256) / 32 steps; element 32 s + l of a group --
    step s of chain l -- is stored at l * st + s of that group, so that a chain's steps are contiguous."""
    e = np.asarray(e, np.int64)
    group, within = e // 256, e % 256
    chain, step = within % 32, within // 32
    steps = np.minimum(256, K - group * 256) // 32
    return group * 256 + chain * steps + step


def permute_rows(rows):
    """rows [N, K] in logical order -> the operand order"""
    rows = np.asarray(rows)
    out = np.empty_like(rows)
    out[:, perm_index(np.arange(rows.shape[1]), rows.shape[1])] = rows
    return out


# ------------------------------------------------------------------------------------------------ mat-vec cases
# K walks k_dense_mv's loop (an f16 double batch is 4 groups of 256, an f32 one 2):
#   32 / 224 a 1- / 7-step tail alone | 256 one leftover group | 512 two (f32: one double batch) | 768 three (f32: a batch + 1) |
#   1024 one double batch exactly, its prefetch past the end the clamped re-read (f32: two) | 1056 + a 1-step tail |
#   1344 a batch + 1 leftover + a 2-step tail (f32: 2 + 1 + tail) | 4096 4 / 8 batches | 11008 10 batches + 3 leftover / 21 + 1
# M: 1 every row pointer clamped | 3, 4, 5 around a half-wave's 4 rows | 16, 17 a second workgroup holding one row | 250 |
#    16352, 16353 (K 256) the two sides of the switch from 4 to 8 half-waves per workgroup | K 4096, 11008: 5 and 40 only.
MV_KS = (32, 224, 256, 512, 768, 1024, 1056, 1344, 4096, 11008)
MV_MS = (1, 3, 4, 5, 16, 17, 250)
MV_MS_SWITCH = (16352, 16353)
BASE = dict(M=40, K=1344, N=3)
MV_REGIMES = ("gauss", "zeros", "midpoints", "overflow", "tiny", "underflow")      # all at the base shape's M and K


def mv_ms(K):
    return (5, 40) if K >= 4096 else MV_MS + (MV_MS_SWITCH if K == 256 else ())


def regimes_for(wtype):
    return ("gauss", "zeros") + (("midpoints", "overflow", "tiny") if wtype == 1 else ("underflow",))


# (wtype, K, M, N, regime)
MV_CASES = [(wt, K, M, 1 if M > 1000 else 2, "gauss") for wt in (1, 0) for K in MV_KS for M in mv_ms(K)] + \
           [(wt, BASE["K"], BASE["M"], {"gauss": BASE["N"], "zeros": 11, "overflow": 4}.get(r, 2), r) for wt in (1, 0) for r in regimes_for(wt)]


def mv_id(c):
    return f"{WNAMES[c[0]]}-K{c[1]}-M{c[2]}-N{c[3]}-{c[4]}"


MV_BY_ID = {mv_id(c): c for c in MV_CASES}


def base_case(wtype):
    return (wtype, BASE["K"], BASE["M"], BASE["N"], "gauss")


def fp16_midpoints(rng, n):
    """n fp32 values exactly half way between two neighbouring fp16 values, both parities of the lower one (then repeats), random signs;
    returns (x, the fp16 bits RNE must give: the neighbour whose last bit is 0)"""
    h = rng.integers(0x2000, 0x5000, n).astype(np.uint16)                      # normal halves, 2^-7 .. 2^5
    h[0::2] &= np.uint16(0xFFFE)
    h[1::2] |= np.uint16(1)
    lo, hi = h.view(np.float16).astype(F32), (h + np.uint16(1)).view(np.float16).astype(F32)
    sign = np.where(rng.random(n) < 0.5, F32(-1), F32(1))
    x = ((lo + hi) * F32(0.5) * sign).astype(F32)                             # exact: 12 significant bits
    even = np.where(h & 1, h + np.uint16(1), h).astype(np.uint16) | np.where(sign < 0, np.uint16(0x8000), np.uint16(0))
    return x, even.astype(np.uint16)


def mv_build(case, seed=11):
    """(w [M, K] in the weight dtype, x f32 [N, K], resid f32 [N, M])"""
    wtype, K, M, N, regime = case
    rng = np.random.default_rng([seed, wtype, K, M, MV_REGIMES.index(regime)])
    w = (0.02 * rng.standard_normal((M, K))).astype(F32)                        # the synthetic models' weight scale
    x = rng.standard_normal((N, K)).astype(F32)                                 # a normed row's scale
    resid = rng.standard_normal((N, M)).astype(F32)
    step = (np.arange(K) // 32) % 2                                             # chain l = elements l, l + 32, ...: K / 32 steps each
    if regime == "gauss":
        if N > 1:
            x[1] += F32(3.0)                                                    # a row with a DC offset
    elif regime == "zeros":
        # the rows of tests/test_gpu_dense_mfma_op.py: where a flushed denormal, a padded step or a re-ordered fold shows
        assert (K // 32) % 2 == 0
        w[0] = 0.0; w[1] = -0.0
        w[2] = 0.5; w[3] = np.where(step == 0, 0.25, -0.25)
        w[4, ::3] = 0.0; w[4, 1::3] = -0.0
        x[0] = 0.0; x[2] = -0.0
        x[3] = np.where(step == 0, 1.5, -1.5)                                   # x w[2]: every chain +p -p +p ... = +0 exactly
        x[4] = 1.5                                                              # x w[3]: the same cancellation from the weight side
        x[5, ::2] = 0.0; x[5, 1::5] = -0.0
        if wtype == 0:
            w[5] = 1e-40; w[6] = np.where(step == 0, 3e-39, -2e-39)             # subnormal weights
            w[7] = 1e-30                                                        # x 1e-30: products that underflow to subnormals / to zero
            w[8, ::2] = 1e-25
            x[7] = 1e-40; x[8] = 1e-30; x[9] = np.where(step == 0, 1e-12, -1e-15)
            x[10, ::7] = 1.4e-45
        else:
            w[5] = 6e-8; w[6] = np.where(step == 0, 3e-6, -2e-6)                # fp16 subnormals
            w[7] = 6.1e-5                                                       # the smallest normal half
            x[7] = 6e-8; x[8] = 1e-9; x[9] = np.where(step == 0, 6.1e-5, -3e-6) # activations that round to fp16 subnormals / zero
        resid[:, 0] = -0.0; resid[0] = 0.0
    elif regime == "midpoints":
        for n in range(N):
            x[n] = fp16_midpoints(rng, K)[0]
    elif regime == "overflow":
        # 65519 rounds to 65504, +-65520 to +-inf; column 7 / 9 of the weights: exact zeros (inf * 0 = NaN), positive, negative
        w[:, 7] = np.where(np.arange(M) % 3 == 0, 0.0, np.where(np.arange(M) % 3 == 1, 0.03125, -0.03125))
        w[:, 9] = np.where(np.arange(M) % 4 == 0, -0.0, np.where(np.arange(M) % 4 < 3, 0.0625, -0.0625))
        x[0, 5] = 65519.0; x[0, 70] = -65519.0                                  # finite: every output of row 0 is
        x[1, 7] = 65520.0
        x[2, 9] = -65520.0
        x[3, 7] = 65520.0; x[3, 9] = -65520.0; x[3, 5] = 65519.0                # inf - inf across chains 7 and 9
    elif regime == "tiny":
        # around the bottom of fp16: 2^-25 is the tie between 0 and the smallest subnormal 2^-24 (-> 0, even), a bit above it -> 2^-24,
        # 1.5 * 2^-24 the tie between 2^-24 and 2^-23 (-> 2^-23), 2.5 * 2^-24 -> 2^-23 (even) ...
        t = F32(2.0) ** -25
        pool = np.array([t, np.nextafter(t, F32(1)), np.nextafter(t, F32(0)), 2 * t, 3 * t, np.nextafter(3 * t, F32(0)), np.nextafter(3 * t, F32(1)),
                         5 * t, 4 * t, 0.99 * t, 7 * t, 1000 * t], F32)
        for n in range(N):
            x[n] = rng.choice(pool, K) * np.where(rng.random(K) < 0.5, F32(-1), F32(1))
        w *= F32(50.0)                                                          # (sums of ~1e-7: far from fp32's own bottom)
    elif regime == "underflow":
        # f32: products around 1e-40 (subnormal sums) and 1e-50 (every product underflows to zero or to the smallest subnormal)
        w = (rng.standard_normal((M, K)) * 1e-20).astype(F32)
        x[0] = (rng.standard_normal(K) * 1e-20).astype(F32)
        x[1] = (rng.standard_normal(K) * 1e-25).astype(F32)
        x[1, ::2] = (rng.standard_normal((K + 1) // 2) * 3e-26).astype(F32)
        resid = (resid * F32(1e-40)).astype(F32)                                # (subnormal residuals: the add must keep them)
    else:
        raise KeyError(regime)
    w = w.astype(wdtype(wtype))
    return w, x, resid


def stored(a):
    """what the store keeps of a reference output: the array, or the digest of canon(array) where it is large"""
    import refgolden
    a = np.asarray(a, F32)
    return a if a.size <= FULL_MAX else refgolden.digest(canon(a))


def agrees_with_stored(a, st):
    """-> '' or what differs: `a` (f32) against a stored reference output under the comparison rule"""
    import refgolden
    a = np.asarray(a, F32)
    if a.size <= FULL_MAX:
        return "" if not len(differ(a, st)) else first_diff(a, st)
    return "" if np.array_equal(refgolden.digest(canon(a)), st) else "digests differ"


# ------------------------------------------------------------------------------------------------ what the inputs must tell apart
def mutations(oracle, w, x, wtype):
    """{name: y [N, M]} of the base case under each neighbour of the reference's arithmetic"""
    ww, xa = widen(w), act(x, wtype)
    dot = lambda xs, **kw: np.array([[oracle.vec_dot_f32_variant(ww[m], xs[n], **kw) for m in range(ww.shape[0])] for n in range(xs.shape[0])], F32)
    out = {"self": dot(xa), "fold in lane order": dot(xa, lane_order=True), "multiply and add rounded separately": dot(xa, fused=False),
           "16 chains": dot(xa, chains=16), "64 chains": dot(xa, chains=64)}
    if wtype == 1:
        out["activations not rounded to fp16"] = dot(np.asarray(x, F32))
    return out


# ------------------------------------------------------------------------------------------------ activation preparation
DENSE_PREP_KERNELS = ("auto", "fused", "split")


def fused_applies(mode, K):
    return mode != "norm" or K // 16 <= 1024


def prep_kernels_for(mode, K):
    """(kernel asked for, kernel that must run) for every producer that takes the shape"""
    ok = fused_applies(mode, K)
    return [("auto", "fused" if ok else "split")] + ([("fused", "fused")] if ok else []) + [("split", "split")]


# the f16_double_rounding regime: (mode, K, N, regime, layout) in prep_cases' form; f16 weights only
DR = "f16_double_rounding"
DR_MIN_PER_ROW = 64
DR_CASES = [("silu_mul", 288, 2, DR, "dense"), ("norm", 288, 2, DR, "dense"), ("silu_mul", 4096, 2, DR, "dense"), ("norm", 4096, 2, DR, "dense")]
DR_NORM_ROWS = {288: ("norm", 288, 2, "normal:1e3"), 4096: ("norm", 4096, 2, "offset")}      # the order-proof rows of prep_cases used as x


def rounds_twice(a, b):
    """a, b f32 (their product exact in float64: 24 + 24 bits) -> where fp16(exact a * b) != fp16(fp32(a * b)): the fp32 product lands
    exactly half way between two fp16 values although the exact one does not, and the tie goes the other way"""
    with np.errstate(all="ignore"):
        exact = a.astype(np.float64) * b.astype(np.float64)
        once = exact.astype(np.float16)                                        # numpy narrows float64 -> float16 in ONE rounding
        twice = exact.astype(F32).astype(np.float16)
    return np.isfinite(exact) & (once.view(np.uint16) != twice.view(np.uint16)) & ~np.isnan(once)


def dr_search(first, draw, rng, want, reps=16):
    """for each of `want` given first factors first[i] a second factor s with rounds_twice(first[i], s), by search: draw(rng, shape)
    proposes ordinary values u; the candidates are the three fp32 neighbours of T / first[i], T the fp16 tie next to first[i] * u (a
    purely random candidate qualifies about once in 2^14, one of these about once in 10); rounds_twice decides"""
    first = np.asarray(first, F32)
    assert first.shape == (want,) and np.all(first != 0)
    out = np.zeros(want, F32)
    todo = np.arange(want)
    for _ in range(200):
        if not todo.size:
            return out
        f = first[todo, None].astype(np.float64)
        with np.errstate(all="ignore"):
            v = f * draw(rng, (todo.size, reps)).astype(np.float64)
            hb = np.abs(v).astype(np.float16).view(np.uint16)
            hb = np.clip(hb, 0x0400, 0x7BFE)                                   # (normal halves with a finite upper neighbour)
            tie = (hb.view(np.float16).astype(np.float64) + (hb + np.uint16(1)).view(np.float16).astype(np.float64)) * 0.5 * np.sign(v)
            c = (tie / f).astype(F32)
        cand = np.concatenate([c, np.nextafter(c, F32(np.inf)), np.nextafter(c, F32(-np.inf))], axis=1)
        hit = rounds_twice(np.broadcast_to(first[todo, None], cand.shape), cand)
        has = hit.any(axis=1)
        out[todo[has]] = cand[has, hit[has].argmax(axis=1)]
        todo = todo[~has]
    raise AssertionError(f"no double-rounding partner for {todo.size} elements")


_dr_built = {}


def dr_build(oracle, mode, K, N, seed=23):
    """(x, b, mask [N, K]): operands of prep_cases' form; mask marks the elements built so that the product's fp32 rounding is an fp16 tie.
    SILU_MUL: gates are ordinary, every third `up` (up to 128 per row) is searched against p = silu_table(gate).  NORM: x are order-proof
    rows of prep_cases, row n owns the weights at positions i % N == n of the first 3/4 of the row (up to 128 per row), searched against
    t_i = (float) (x_i - mean) * scale.  Everything else is ordinary."""
    import prep_cases as pc
    key = (mode, K, N, seed)
    if key not in _dr_built:
        _dr_built[key] = _dr_build(oracle, pc, mode, K, N, seed)
    return _dr_built[key]


def _dr_build(oracle, pc, mode, K, N, seed):
    rng = np.random.default_rng([seed, K, N, pc.MODES.index(mode)])
    mask = np.zeros((N, K), bool)
    if mode == "silu_mul":
        gate = (rng.standard_normal((N, K)) * 2.0).astype(F32)
        up = rng.standard_normal((N, K)).astype(F32)
        p = oracle.unary_rows("silu", gate)
        mask[:, :3 * 128:3] = p[:, :3 * 128:3] != 0
        up[mask] = dr_search(p[mask], lambda r, s: r.standard_normal(s).astype(F32), rng, int(mask.sum()))
        return gate, up, mask
    assert mode == "norm"
    x, _ = pc.build(oracle, *DR_NORM_ROWS[K])
    assert x.shape == (N, K)
    t = oracle.unary_rows("norm", x)
    w = (1.0 + 0.5 * rng.standard_normal(K)).astype(F32)
    pos = np.arange(min(K * 3 // 4, 128 * N))
    for n in range(N):
        mask[n, pos[pos % N == n]] = True
    mask &= t != 0
    own = mask.any(axis=0)
    assert (mask.sum(axis=0) <= 1).all()
    w[own] = dr_search(t.T[mask.T], lambda r, s: (1.0 + 0.5 * r.standard_normal(s)).astype(F32), rng, int(own.sum()))
    return x, w, mask


# ------------------------------------------------------------------------------------------------ embedding gather
EMBED_V = 37
EMBED_DS = (32, 96, 288, 4096, 4128)
EMBED_WTYPES = (0, 1, 3)
EMBED_NS = (1, 2, 13)
EMBED_SPECIAL_ROW = 5
EMBED_TOKENS = {1: [EMBED_V - 1], 2: [0, EMBED_V - 1], 13: [0, EMBED_V - 1, 5, 5, 0, 7, 36, 1, 5, 20, 11, 0, 36]}
EMBED_CASES = [(wt, d, N) for wt in EMBED_WTYPES for d in EMBED_DS for N in EMBED_NS]
ENAMES = {0: "f32", 1: "f16", 3: "q41"}


def embed_id(c):
    return f"{ENAMES[c[0]]}-d{c[1]}-N{c[2]}"


def embed_matrix_q41(rng, V, d):
    """Q4_1 rows in file layout uint8 [V, d/32 * 24] ([nb f32 min][nb f32 d][nb * 16 nibble bytes]) with every code, scales and mins of both
    signs and some d == 0 blocks; rows 0 and V-1 hold codes 15 / 0 and 0 / 15 in the first half of every block, with the largest and the
    smallest scales and mins"""
    nb = d // 32
    mn = (rng.standard_normal((V, nb)) * 0.3).astype(F32)
    dd = (rng.standard_normal((V, nb)) * 0.05).astype(F32)
    dd[rng.random((V, nb)) < 0.1] = 0.0
    dd[:, 0] = np.where(np.arange(V) % 3 == 0, 0.0, dd[:, 0])
    q = rng.integers(0, 256, (V, nb * 16), dtype=np.uint8)
    q.reshape(V, nb, 16)[0, :, :8] = 0x0F                                       # (the other half of each block keeps random codes: with one
    q.reshape(V, nb, 16)[V - 1, :, :8] = 0xF0                                   #  code per block a block tells a fused multiply-add or not at all)
    jit = lambda: (1.0 + 0.1 * rng.random(nb)).astype(F32)                      # (random significands: code * d is not exact)
    mn[0], dd[0] = F32(-3.0e37) * jit(), F32(2.0e37) * jit()                    # 15 d + m: near the top of fp32, finite
    mn[V - 1], dd[V - 1] = F32(1e-37) * jit(), F32(-1e-38) * jit()              # near the bottom of the normal range ...
    mn[V - 1, 1::2], dd[V - 1, 1::2] = F32(1e-40), F32(-1e-41)                  # ... and, in the odd blocks, a subnormal scale and min
    return np.concatenate([mn.view(np.uint8), dd.view(np.uint8), q], axis=1)


def dequant_q41(rows):
    """dequantize_row_q4_1 (ggml.c:686-717) as plain C compiles it without contraction: (float) code * d rounded, + m rounded.  (The
    reference build decides: tests/test_dense_op_host.py holds this against its stored get_rows outputs.)"""
    rows = np.ascontiguousarray(rows, np.uint8)
    V = rows.shape[0]
    nb = rows.shape[1] // 24
    mn, dd, q = rows[:, :4 * nb].copy().view(F32), rows[:, 4 * nb:8 * nb].copy().view(F32), rows[:, 8 * nb:].reshape(V, nb, 16)
    code = np.empty((V, nb, 32), F32)
    code[..., 0::2] = q & 0xF
    code[..., 1::2] = q >> 4
    with np.errstate(all="ignore"):
        return ((code * dd[..., None]).astype(F32) + mn[..., None]).astype(F32).reshape(V, nb * 32)


def dequant_q41_fused(rows):
    """the neighbour dequant_q41 must be told from: code * d + m in ONE rounding (float64 holds the product exactly; its own rounding of
    the sum before the narrowing matters once in ~2^29 elements -- this only counts elements)"""
    rows = np.ascontiguousarray(rows, np.uint8)
    V, nb = rows.shape[0], rows.shape[1] // 24
    mn, dd, q = rows[:, :4 * nb].copy().view(F32), rows[:, 4 * nb:8 * nb].copy().view(F32), rows[:, 8 * nb:].reshape(V, nb, 16)
    code = np.empty((V, nb, 32), np.float64)
    code[..., 0::2] = q & 0xF
    code[..., 1::2] = q >> 4
    with np.errstate(all="ignore"):
        return (code * dd[..., None].astype(np.float64) + mn[..., None].astype(np.float64)).astype(F32).reshape(V, nb * 32)


def embed_table(wtype, d):
    """the embedding matrix of a case: float32 / float16 [V, d] or Q4_1 rows uint8 [V, d/32 * 24]"""
    rng = np.random.default_rng([31, wtype, d])
    V = EMBED_V
    if wtype == 3:
        return embed_matrix_q41(rng, V, d)
    m = rng.standard_normal((V, d)).astype(F32)
    big, small = (F32(65504.0), F32(2.0) ** -14) if wtype == 1 else (np.finfo(F32).max, np.finfo(F32).tiny)
    m[0] = np.where(np.arange(d) % 2 == 0, big, -big)                            # rows 0 and V - 1 extreme
    m[V - 1] = np.where(np.arange(d) % 2 == 0, small, -small / 2)                # (the smallest normal, a subnormal)
    m = m.astype(wdtype(wtype))
    if wtype == 1 and d >= 4096:          # every fp16 subnormal of both signs, +-0, +-inf and a NaN in one row
        sub = np.arange(1, 0x400, dtype=np.uint16)
        sp = np.concatenate([sub, sub | np.uint16(0x8000), np.array([0x0000, 0x8000, 0x7C00, 0xFC00, 0x7E00], np.uint16)])
        m[EMBED_SPECIAL_ROW, rng.permutation(d)[:sp.size]] = sp.view(np.float16)
    if wtype == 0:
        sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.4e-45, -1.4e-45, 1e-40, -1e-40], F32)
        m[EMBED_SPECIAL_ROW, rng.permutation(d)[:sp.size]] = sp
    return m


def embed_rows(wtype, table):
    """every row of the table as the gather must leave it: f32 a copy, f16 the exact widening, Q4_1 dequant_q41"""
    return dequant_q41(table) if wtype == 3 else np.ascontiguousarray(table).astype(F32)
