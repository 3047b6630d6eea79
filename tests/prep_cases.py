"""Inputs, references and the order-proof argument for tests/test_gpu_prep.py (and the CPU checks of tests/test_prep_host.py).

Nothing here needs a GPU.  A case is (mode, K, N, regime, layout); `build` makes its logical operands, `lay_out` places them in the one
buffer llamahip_op_prep uploads (poison between the rows where the layout has a stride > K), `reference` evaluates the oracle.

Input range.  Inputs are finite and every non-zero block of y has amax >= 1e-30: below about 2e-38 the quantizer's 7 / amax overflows to
infinity, and what the conversion of x * inf (or of inf * 0) to an integer gives is not something the oracle pins against the
reference -- that range is not tested.

The norm's sum order.  ggml_norm sums the row in index order in double; the kernels sum per thread and then by a tree.  Every double sum
of K terms, in ANY order, lies within gamma_(K-1) sum|x| of the exact sum (gamma_n = n u / (1 - n u), u = 2^-53), so every mean any order
can produce lies within rad = gamma_K sum|x| / K of the exact one (the division's rounding included).  (float) (x_i - mean) is monotone
in mean, so if it is the same float at both ends of that interval it is the same float for every order.  The squares are summed likewise:
sum_i (x_i - m)^2 over m in the interval lies in [Q(m*), max Q(ends)] (Q is a parabola around the exact mean m*), each term carries
three roundings and the sum K - 1 more, all terms are non-negative, so the computed sum lies within a factor 1 +- gamma_(K+3) of that
range; 1 / sqrt(sum2 / K + eps) is monotone, so if (float) scale agrees at both ends (widened by 2^-50 for the division, the sqrt and the
reciprocal) the scale is the same float for every order.  A row that passes both checks is ORDER-PROOF: the kernels must then equal the
reference bit for bit, whatever their reduction tree.  Where every partial sum is exact (all elements multiples of one power of two,
sum|x| below 2^53 of them: constant and all-zero rows) no order can change the sum at all and rad is 0.
The rows come from a committed table of draws (NORM_ATTEMPTS, found on the CPU with find_attempts: the first draw of each row that is
order-proof); the tests assert the property for every NORM row they use."""
import math

import numpy as np

MODES = ("plain", "norm", "silu_mul")
U = 2.0 ** -53
LD = np.longdouble
POISON = np.uint32(0x7FC0DEAD)            # a NaN between the rows of a strided layout: a kernel that reads it poisons its block
EPS_NORM = np.float64(np.float32(1e-5))


def gamma(n):
    return n * U / (1 - n * U)


def kp(K):
    return (K + 255) // 256 * 256


def fast_applies(mode, K):
    return mode != "norm" or K // 16 <= 1024


def kernels_for(mode, K):
    """(kernel asked for, want_y, kernel that must run) for every kernel family that takes the shape"""
    rule = "fast" if fast_applies(mode, K) else "lds"
    return [("auto", False, rule)] + ([("fast", False, "fast")] if fast_applies(mode, K) else []) + [("lds", True, "lds"), ("lds", False, "lds"), ("auto", True, "lds")]


# ------------------------------------------------------------------------------------------------ QA layout
def pack_qa(blocks, K):
    """numpy statement of the QA layout: Q4_0 file blocks uint8 [N, K/32, 20] -> (qa_A uint32 [N, Kp/4], qa_d float32 [N, Kp/32]) with the
    padded blocks all zero.  Dword (c * 8 + k) * 8 + j of a row = chain k of block c * 8 + j: elements (2k, 2k+1, 16+2k, 17+2k) as signed
    nibbles (q - 8) & 0xF at bits 0, 8, 16, 24, the whole dword shifted left by 4 in odd blocks."""
    blocks = np.ascontiguousarray(blocks, np.uint8)
    N, nb, _ = blocks.shape
    nbp = kp(K) // 32
    qd = np.zeros((N, nbp), np.float32)
    qd[:, :nb] = np.ascontiguousarray(blocks[..., :4]).view(np.float32).reshape(N, nb)
    qs = blocks[..., 4:].astype(np.uint32)
    e = np.empty((N, nb, 32), np.uint32)
    e[..., 0::2] = (qs & 0xF) ^ 8
    e[..., 1::2] = (qs >> 4) ^ 8
    k = np.arange(8)
    dw = e[..., 2 * k] | (e[..., 2 * k + 1] << 8) | (e[..., 16 + 2 * k] << 16) | (e[..., 17 + 2 * k] << 24)      # [N, nb, k]
    dw = dw << (4 * (np.arange(nb) & 1)).astype(np.uint32)[None, :, None]
    full = np.zeros((N, nbp, 8), np.uint32)
    full[:, :nb] = dw
    qa = full.reshape(N, nbp // 8, 8, 8).transpose(0, 1, 3, 2)                                                   # [n][c][k][j]
    return np.ascontiguousarray(qa).reshape(N, kp(K) // 4), qd


# ------------------------------------------------------------------------------------------------ the order-proof check
def sums_are_exact(x):
    """every partial sum of x, in any order, is exact: all elements are multiples of one power of two q and sum|x| < 2^53 q"""
    nz = np.abs(x[x != 0].astype(np.float64))
    if nz.size == 0:
        return True
    m, e = np.frexp(nz)
    M = (m * 2.0 ** 24).astype(np.int64)                    # 24-bit significands
    tz = np.log2((M & -M).astype(np.float64)).astype(np.int64)
    q = int((e - 24 + tz).min())
    return math.fsum(nz) / 2.0 ** q < 2.0 ** 53


def norm_stats(x):
    """The exact statistics of one fp32 row and the interval any summation order can reach (module docstring):
    dict(mean, rad, m_lo, m_hi, q, rho_t, v_ok, scale_ok, proof)."""
    xd = x.astype(np.float64)
    K = x.size
    S, A = math.fsum(xd), math.fsum(np.abs(xd))
    mean = S / K
    exact = sums_are_exact(x)
    rad = 0.0 if exact else gamma(K) * A / K * (1 + 2.0 ** -40) + abs(mean) * 2.0 ** -52      # (the slack: fsum's and this division's own rounding)
    m_lo, m_hi = (mean, mean) if exact else (np.nextafter(mean - rad, -np.inf), np.nextafter(mean + rad, np.inf))
    v_at_hi, v_at_lo = (xd - m_hi).astype(np.float32), (xd - m_lo).astype(np.float32)
    v_ok = np.array_equal(v_at_hi.view(np.uint32), v_at_lo.view(np.uint32))
    xl = xd.astype(LD)
    Q = lambda m: ((xl - LD(m)) ** 2).sum()
    mstar = LD(S) / K
    q_star = Q(mstar)
    q_min = Q(min(max(mstar, LD(m_lo)), LD(m_hi)))
    q_max = max(Q(m_lo), Q(m_hi))
    g = gamma(K + 3) + 2.0 ** -50
    s2_lo, s2_hi = q_min * LD(1 - g), q_max * LD(1 + g)
    w = LD(2.0 ** -50)
    t_lo, t_hi = (s2_lo / K + LD(EPS_NORM)) * (1 - w), (s2_hi / K + LD(EPS_NORM)) * (1 + w)
    sc_hi, sc_lo = np.float32(1 / np.sqrt(t_lo) * (1 + w)), np.float32(1 / np.sqrt(t_hi) * (1 - w))
    t_star = q_star / K + LD(EPS_NORM)
    rho_t = float(max(t_hi - t_star, t_star - t_lo) / t_star)
    return dict(mean=float(mstar), rad=float(max(m_hi - mean, mean - m_lo)), m_lo=m_lo, m_hi=m_hi, q=float(q_star), rho_t=rho_t,
                v_ok=v_ok, scale_ok=bool(sc_lo == sc_hi), proof=bool(v_ok and sc_lo == sc_hi), scale=float(1 / np.sqrt(t_star)))


def one_pass_stats(x):
    """The ONE-PASS second moment of one fp32 row, sum2 = fma(-mean, S1, S2) with S1 = sum x, S2 = sum x^2 and mean = S1 / K in double (the
    fused norm prologue of the decode mat-vec; S1 / S2 reduced by the kernel in its own order or handed over as per-slice partial sums),
    and the interval every order can reach.  With u = 2^-53, A = sum|x|, exact S1, S2 and Q* = S2 - S1^2 / K = sum (x - m*)^2:
      S1^: K - 1 additions of exact terms in any tree (rounded partial sums of slices that are then added are such a tree):
           |S1^ - S1| <= e1 = gamma_K A   (0 where every partial sum is exact, sums_are_exact)
      S2^: x^2 is exact in double (48 bits), so again only the additions round:   |S2^ - S2| <= e2 = gamma_K S2
      mean^ = fl(S1^ / K):   |mean^ - m*| <= em = e1 / K + 2^-52 |m*|
      mean^ S1^ - m* S1 = mean^ (S1^ - S1) + S1 (mean^ - m*):   |.| <= (|m*| + em) e1 + |S1| em
      the fma rounds once:   |sum2^ - Q*| <= E + 2^-52 (|Q*| + E),   E = e2 + (|m*| + em) e1 + |S1| em
    (each bound carries a factor 1 + 2^-40 for the roundings of this evaluation itself).  1 / sqrt(sum2 / K + eps) is monotone, so if
    (float) scale agrees at both ends -- widened by 2^-50 as in norm_stats -- it is the same float for every order, and since Q* lies in
    this interval and in norm_stats' two-pass one, it is the two-pass float too.  The kernel takes this form only where mean^ S1^ <= 0.25
    S2^; `fast_possible` says whether ANY order can satisfy that (lower bound of the left side against the upper bound of the right),
    `fast_certain` whether every order does.  A row on which no order can take the one-pass form is proved by norm_stats alone; every
    other row needs scale_ok.  dict(fast_possible, fast_certain, lo, hi, scale_ok, proof)."""
    xd = x.astype(np.float64)
    K = x.size
    sl = 1 + 2.0 ** -40
    S1, A, S2 = math.fsum(xd), math.fsum(np.abs(xd)), math.fsum(xd * xd)
    m = abs(S1) / K
    e1 = 0.0 if sums_are_exact(x) else gamma(K) * A * sl
    e2 = gamma(K) * S2 * sl
    em = (e1 / K + 2.0 ** -52 * m) * sl
    E = (e2 + (m + em) * e1 + abs(S1) * em) * sl
    q = norm_stats(x)["q"]
    w = 2.0 ** -50
    lo, hi = q - E - w * (abs(q) + E), q + E + w * (abs(q) + E)
    lhs_lo, lhs_hi = max(m - em, 0.0) * max(abs(S1) - e1, 0.0) * (1 - w), (m + em) * (abs(S1) + e1) * (1 + w)
    rhs_lo, rhs_hi = 0.25 * (S2 - e2) * (1 - w), 0.25 * (S2 + e2) * (1 + w)
    fast_possible, fast_certain = bool(lhs_lo <= rhs_hi), bool(lhs_hi <= rhs_lo)
    t_lo, t_hi = (LD(lo) / K + LD(EPS_NORM)) * (1 - LD(w)), (LD(hi) / K + LD(EPS_NORM)) * (1 + LD(w))
    scale_ok = bool(t_lo > 0 and np.float32(1 / np.sqrt(t_lo) * (1 + LD(w))) == np.float32(1 / np.sqrt(t_hi) * (1 - LD(w))))
    return dict(fast_possible=fast_possible, fast_certain=fast_certain, lo=lo, hi=hi, scale_ok=scale_ok, proof=bool(scale_ok or not fast_possible))


def norm_proof_both(x):
    """order-proof under the two-pass form (norm_stats) AND under the one-pass form wherever an order can take it (one_pass_stats)"""
    return norm_stats(x)["proof"] and one_pass_stats(x)["proof"]


def find_attempts(make_row, N, seed, limit=2000, proof=lambda x: norm_stats(x)["proof"]):
    """per row n the first attempt a whose row make_row(default_rng([seed, n, a]), n) is order-proof -- how NORM_ATTEMPTS was made"""
    out = []
    for n in range(N):
        a = next((a for a in range(limit) if proof(make_row(np.random.default_rng([seed, n, a]), n))), None)
        assert a is not None, f"no order-proof row in {limit} draws (row {n}, seed {seed})"
        out.append(a)
    return tuple(out)


# The committed selection: per NORM case (K, N, regime) and row, which draw is used (found once on the CPU with find_attempts; 0 = the
# first draw).  The tests assert that every row so chosen IS order-proof, so a stale entry fails instead of weakening anything.
NORM_ATTEMPTS = {
    (32, 1, 'normal:1'): (0,),
    (64, 2, 'offset'): (0, 0),
    (96, 13, 'offset'): (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    (288, 9, 'zeros'): (0, 0, 0, 0, 0, 0, 0, 0, 0),
    (288, 2, 'normal:1e3'): (0, 0),
    (4096, 2, 'maxpos'): (0, 0),
    (4096, 9, 'normal:1'): (0, 0, 0, 0, 0, 0, 0, 0, 0),
    (4096, 2, 'offset'): (0, 0),
    (4128, 2, 'normal:1e-3'): (0, 0),
    (4128, 9, 'zeros'): (0, 0, 0, 0, 0, 0, 0, 0, 0),
    (8224, 2, 'normal:1'): (0, 0),
    (11008, 1, 'normal:1e3'): (0,),
    (16384, 2, 'normal:1'): (0, 0),
    (16416, 2, 'normal:1'): (0, 0),
    (22016, 1, 'normal:1e-3'): (1,),
}


def norm_rows(make_row, N, seed, key):
    """N rows: row n is make_row(default_rng([seed, n, a]), n) with a = NORM_ATTEMPTS[key][n]"""
    return np.stack([make_row(np.random.default_rng([seed, n, a]), n) for n, a in enumerate(NORM_ATTEMPTS[key])])


# ------------------------------------------------------------------------------------------------ value regimes
TIE_EXPONENTS = (-12, -3, 0, 5, 20)


def tie_block(rng, e):
    """32 values around amax = 7 * 2^e: +-amax once each, and amax * (k + 0.5) / 7 = (k + 0.5) 2^e for every k in -7 .. 6 (then repeats).  id = 7 /
    amax = 2^-e exactly, so every product x * id is the exact half k + 0.5: rint takes it to the even neighbour, round-half-away does not."""
    ties = (np.arange(-7, 7) + 0.5) * 2.0 ** e
    v = np.concatenate([[7 * 2.0 ** e, -7 * 2.0 ** e], ties, rng.choice(ties, 16)])
    return rng.permutation(v).astype(np.float32)


def ties_rows(rng, N, K):
    x = np.empty((N, K // 32, 32), np.float32)
    for n in range(N):
        for b in range(K // 32):
            x[n, b] = tie_block(rng, TIE_EXPONENTS[(n * (K // 32) + b) % len(TIE_EXPONENTS)])
    return x.reshape(N, K)


def tie_products(y):
    """the oracle's products x * id of every element, in fp32 as it computes them"""
    yb = y.reshape(-1, 32)
    amax = np.abs(yb).max(axis=1, keepdims=True)
    return (yb * (np.float32(7.0) / amax)).reshape(y.shape)


def maxpos_rows(rng, N, K):
    """block g (counted over all rows) has one +amax (g / 32 even) or -amax (odd) at position g % 32 and small values elsewhere: the maximum
    visits both half-blocks (the DPP exchange of k_prep_fast) and the codes 15 and 1 appear at every position"""
    nb = K // 32
    x = (rng.standard_normal((N * nb, 32)) * 0.01).astype(np.float32)
    g = np.arange(N * nb)
    x[g, g % 32] = np.where((g // 32) % 2 == 0, 1.0, -1.0).astype(np.float32) * np.float32(1.75)
    return x.reshape(N, K)


def zeros_rows(rng, N, K, scale=1.0):
    """row 0: ordinary with one all-zero block; row 1: all zero; row 2: constant; the rest ordinary"""
    x = (rng.standard_normal((N, K)) * scale).astype(np.float32)
    b = min(1, K // 32 - 1)
    x[0, 32 * b:32 * b + 32] = 0.0
    if N > 1:
        x[1] = 0.0
    if N > 2:
        x[2] = np.float32(0.7)
    return x


# gate values at the edges of the fp16 index of the SiLU table: +-0, fp16 subnormals (and what rounds to them or to 0), +-65504, the
# largest fp32 values that still round to 65504, negatives whose SiLU is -0 or underflows, ordinary negatives around the minimum
SILU_FINITE_EDGES = np.array([0.0, -0.0, 5.9604645e-8, -5.9604645e-8, 2.9802322e-8, -2.9802322e-8, 2.9802326e-8, 3.0e-5, -3.0e-5, 6.0975552e-5,
                              6.1035156e-5, 65504.0, -65504.0, 65519.99, -65519.99, -17.5, -20.0, -30.0, -100.0, -1000.0, -1.2784645, 1.2784645],
                             np.float32)
SILU_TO_PLUS_INF = np.array([65520.0, 70000.0, 1e30, 3.0e38], np.float32)          # round to fp16 +inf: SiLU = +inf
SILU_TO_MINUS_INF = np.array([-65520.0, -70000.0, -1e30], np.float32)              # round to fp16 -inf: the table holds -inf / inf = NaN


def silu_edge_rows(rng, N, K):
    """NOTE on blocks 1 and 2: their y is +-inf / NaN (finite inputs, so they are in range), their scale d = inf is defined, but their CODES
    are the integer conversion of NaN (x * (7 / inf) with x = +-inf or NaN), which C leaves undefined.  The oracle's x86 conversion gives
    INT_MIN (+ 8 -> code 8) and the device's gives 0 (-> code 8): the agreement is observed on this toolchain and hardware, not guaranteed
    by the reference -- if it ever breaks, compare only the scales of those two blocks.
    (gate, up): block 0 of every row ordinary + the finite edges; block 1 the gates that round to +inf; block 2 those that round to -inf
    (their y is +-inf / NaN: kept apart so that the other blocks quantize finite values); later blocks ordinary with edges sprinkled in.
    up has negatives and zeros -- but not under a non-finite SiLU (inf * 0 is a NaN whose sign is the producer's choice)."""
    assert K >= 128
    gate = rng.standard_normal((N, K)).astype(np.float32) * np.float32(2.0)
    up = rng.standard_normal((N, K)).astype(np.float32)
    up[:, ::7] = 0.0
    up[:, 3::11] = -0.0
    ne = SILU_FINITE_EDGES.size
    for n in range(N):
        gate[n, rng.permutation(32)[:ne]] = SILU_FINITE_EDGES
        gate[n, 32 + rng.permutation(32)[:SILU_TO_PLUS_INF.size]] = SILU_TO_PLUS_INF
        gate[n, 64 + rng.permutation(32)[:SILU_TO_MINUS_INF.size]] = SILU_TO_MINUS_INF
        for b in range(3, K // 32):          # (the small ones: a 65504 would flatten the block's other codes)
            gate[n, 32 * b + rng.permutation(32)[:4]] = rng.choice(SILU_FINITE_EDGES[np.abs(SILU_FINITE_EDGES) < 50], 4)
        blk = up[n, 32:96]
        blk[blk == 0] = np.float32(-1.5)
    return gate, up


def cancel_row(rng, K=4096, pairs=8):
    """NOT order-proof on purpose: pairs of +-1e8 among unit-scale values, shuffled -- the double sums cancel by eight orders of magnitude"""
    x = rng.standard_normal(K).astype(np.float32)
    x[:2 * pairs] = np.tile(np.array([1e8, -1e8], np.float32), pairs)
    return rng.permutation(x)


def power_of_two_silu(oracle):
    """a positive gate (fp32, exactly an fp16 value) whose table SiLU is a power of two p: silu_table(gate) * (v / p) == v exactly"""
    silu, _ = oracle.tables()
    h = np.arange(0x0400, 0x7C00, dtype=np.uint16)                 # positive normal fp16 inputs
    out = silu[h]
    hit = h[((out & 0x03FF) == 0) & (out >= 0x0400) & (out < 0x7C00)]
    assert hit.size, "no fp16 input whose table SiLU is a power of two"
    g = hit[hit.size // 2: hit.size // 2 + 1]
    return np.float32(g.view(np.float16)[0]), np.float32(silu[g].view(np.float16)[0])


# ------------------------------------------------------------------------------------------------ cases
# (mode, K, N, regime, layout).  layout: "dense" rows K apart; "strided" in0 (and SILU's in1) rows K + 8 (in1: K + 12) apart with poison
# between them; "model" (SILU_MUL) the FFN's [N][2K] buffer: in1 = in0 + K, both strides 2K.
# K: 32 / 64 / 96 the smallest rows; 288 seven padded blocks; 4096; 4128 = 258 half-blocks: a second slice holding two (PLAIN, SILU_MUL),
# a 320-thread workgroup with 62 dead lanes (NORM); 8224 ragged and wide; 11008 the w2 operand; 16384 NORM's widest one-workgroup row
# (1024 threads); 16416 NORM: AUTO must take the LDS kernel, FAST is refused; 22016 the widest row.
CASES = [
    ("plain", 32, 1, "normal:1", "dense"), ("plain", 64, 2, "normal:1e-3", "dense"), ("plain", 96, 9, "zeros", "dense"),
    ("plain", 288, 13, "normal:1e3", "strided"), ("plain", 288, 2, "ties", "dense"), ("plain", 4096, 2, "maxpos", "dense"),
    ("plain", 4096, 1, "ties", "dense"), ("plain", 4128, 9, "normal:1", "dense"), ("plain", 4128, 9, "zeros", "strided"),
    ("plain", 8224, 2, "normal:1e3", "dense"), ("plain", 11008, 9, "normal:1", "strided"), ("plain", 16384, 1, "normal:1e-3", "dense"),
    ("plain", 22016, 2, "normal:1", "dense"),
    ("norm", 32, 1, "normal:1", "dense"), ("norm", 64, 2, "offset", "dense"), ("norm", 96, 13, "offset", "strided"),
    ("norm", 288, 9, "zeros", "dense"), ("norm", 288, 2, "normal:1e3", "dense"), ("norm", 4096, 2, "maxpos", "dense"),
    ("norm", 4096, 9, "normal:1", "dense"), ("norm", 4096, 2, "offset", "dense"), ("norm", 4128, 2, "normal:1e-3", "dense"), ("norm", 4128, 9, "zeros", "strided"),
    ("norm", 8224, 2, "normal:1", "dense"), ("norm", 11008, 1, "normal:1e3", "dense"), ("norm", 16384, 2, "normal:1", "dense"),
    ("norm", 16416, 2, "normal:1", "strided"), ("norm", 22016, 1, "normal:1e-3", "dense"),
    ("silu_mul", 32, 1, "normal:1", "dense"), ("silu_mul", 64, 2, "normal:1e-3", "model"), ("silu_mul", 96, 9, "zeros", "dense"),
    ("silu_mul", 288, 2, "silu_edges", "dense"), ("silu_mul", 288, 13, "normal:1e3", "strided"), ("silu_mul", 4096, 2, "maxpos", "dense"),
    ("silu_mul", 4096, 1, "ties", "model"), ("silu_mul", 4128, 9, "normal:1", "model"), ("silu_mul", 8224, 2, "normal:1", "dense"),
    ("silu_mul", 11008, 9, "normal:1", "model"), ("silu_mul", 11008, 2, "silu_edges", "model"), ("silu_mul", 16384, 1, "normal:1e-3", "dense"),
    ("silu_mul", 22016, 2, "normal:1", "model"),
]


def case_id(c):
    return "-".join(str(v) for v in c)


def build(oracle, mode, K, N, regime, seed=5):
    """the logical operands of a case: (x [N, K], b): b = None (plain), the weights [K] (norm) or the up rows [N, K] (silu_mul)"""
    rng = np.random.default_rng([seed, K, N, MODES.index(mode)])
    name, _, arg = regime.partition(":")
    scale = float(arg) if arg else 1.0
    if mode == "norm":
        w = (1.0 + 0.5 * rng.standard_normal(K)).astype(np.float32)          # (some negative, a few near zero)
        if name == "normal":
            x = norm_rows(lambda r, n: (r.standard_normal(K) * scale).astype(np.float32), N, seed, (K, N, regime))
        elif name == "offset":          # mean 100 standard deviations from zero
            x = norm_rows(lambda r, n: (100.0 * scale + scale * r.standard_normal(K)).astype(np.float32), N, seed, (K, N, regime))
        elif name == "zeros":
            x = norm_rows(lambda r, n: zeros_rows(r, 3, K)[n] if n < 3 else r.standard_normal(K).astype(np.float32), N, seed, (K, N, regime))
        elif name == "maxpos":
            base = maxpos_rows(rng, N, K)
            x = norm_rows(lambda r, n: base[n] + (r.standard_normal(K) * 1e-3).astype(np.float32), N, seed, (K, N, regime))
        else:
            raise KeyError(regime)
        return x, w
    if name == "normal":
        x = (rng.standard_normal((N, K)) * scale).astype(np.float32)
    elif name == "zeros":
        x = zeros_rows(rng, N, K)
    elif name == "ties":
        x = ties_rows(rng, N, K)
    elif name == "maxpos":
        x = maxpos_rows(rng, N, K)
    elif name == "silu_edges":
        return silu_edge_rows(rng, N, K)
    else:
        raise KeyError(regime)
    if mode == "plain":
        return x, None
    if name in ("ties", "maxpos"):          # y = p * (x / p) = x exactly, through one table entry
        g, p = power_of_two_silu(oracle)
        return np.full((N, K), g, np.float32), (x / p).astype(np.float32)
    up = rng.standard_normal((N, K)).astype(np.float32)
    up[:, ::5] *= np.float32(-1.0)
    up[:, 2::9] = 0.0
    if name == "zeros" and N > 2:
        up[2] = np.float32(-1.25)
    return x, up


def lay_out(mode, x, b, layout):
    """-> (buf float32 [..], kwargs of op_prep): the one buffer, poison wherever no operand lies"""
    N, K = x.shape
    poison = lambda n: np.full(n, POISON, np.uint32).view(np.float32)
    if layout == "model":
        assert mode == "silu_mul"
        buf = np.concatenate([x, b], axis=1).ravel()
        return buf, dict(in_stride=2 * K, in0_offset=0, in1_offset=K, in1_stride=2 * K)
    s0 = K if layout == "dense" else K + 8
    off0 = 4 if layout == "strided" else 0
    a = poison(off0 + N * s0)
    for n in range(N):
        a[off0 + n * s0: off0 + n * s0 + K] = x[n]
    if mode == "plain":
        return a, dict(in_stride=s0, in0_offset=off0)
    if mode == "norm":
        tail = poison(K + 4)
        tail[4:] = b
        return np.concatenate([a, tail]), dict(in_stride=s0, in0_offset=off0, in1_offset=a.size + 4)
    s1 = K if layout == "dense" else K + 12
    t = poison(N * s1)
    for n in range(N):
        t[n * s1: n * s1 + K] = b[n]
    return np.concatenate([a, t]), dict(in_stride=s0, in0_offset=off0, in1_offset=a.size, in1_stride=s1)


def reference(oracle, mode, x, b):
    """(y float32 [N, K], Q4_0 blocks uint8 [N, K/32, 20]) from the oracle: the unary op, ONE fp32 multiply, quantize_row"""
    with np.errstate(all="ignore"):
        if mode == "plain":
            y = x
        elif mode == "norm":
            y = oracle.unary_rows("norm", x) * b[None, :]
        else:
            y = oracle.unary_rows("silu", x) * b
    y = np.ascontiguousarray(y, np.float32)
    blocks = np.stack([oracle.quantize_row(r) for r in y]).reshape(x.shape[0], x.shape[1] // 32, 20)
    return y, blocks


# ------------------------------------------------------------------------------------------------ embedding
def embed_matrix(rng, V, d):
    """Q4_0 rows [V, d/32, 20] with every code, scales of both signs and some d == 0 blocks; row 0 and row V-1 hold codes 0 and 15 everywhere"""
    nb = d // 32
    m = np.empty((V, nb, 20), np.uint8)
    m[..., 4:] = rng.integers(0, 256, (V, nb, 16), dtype=np.uint8)
    dd = (rng.standard_normal((V, nb)) * 0.05).astype(np.float32)
    dd[rng.random((V, nb)) < 0.1] = 0.0
    dd[:, 0] = np.where(np.arange(V) % 3 == 0, 0.0, dd[:, 0])
    m[..., :4] = dd.view(np.uint8).reshape(V, nb, 4)
    m[0, :, 4:] = 0x0F                      # elements alternate code 15, code 0
    m[V - 1, :, 4:] = 0xF0
    return m


# ------------------------------------------------------------------------------------------------ the row that is not order-proof
def norm_f64_bound(x, w):
    """(y64 [K], B [K]): the norm formula w (x - m*) s* in float64 from the exact statistics, and a bound on |y - y64| that holds for EVERY
    summation order of the two double sums and the kernels' fp32 roundings.  With rad the radius of the mean's interval, rho_t the
    relative width of sum2 / K + eps over it (norm_stats) and e = 2^-24:
      v^ = (float) (x - mean):       |v^ - v*| <= dv = rad (1 + 2e) + |v*| (e + 2^-52)               the double subtraction, rounding 1
      s^ = (float) (1 / sqrt(t)):    |s^ - s*| <= s* rho_s, rho_s = rho_t + 2^-50 + e                 (t^-1/2 halves rho_t: kept whole), rounding 2
      p^ = fl(v^ s^):                |p^ - v* s*| <= e1 + e a,  e1 = dv s* (1 + rho_s) + |v*| s* rho_s,  a = (|v*| + dv) s* (1 + rho_s) >= |v^ s^|    rounding 3
      y^ = fl(w p^):                 |y^ - w v* s*| <= |w| (e2 + e (a + e2)),  e2 = e1 + e a                                                    rounding 4
    plus 2^-149 for a result among the subnormals and 2^-50 |y64| for the float64 evaluation itself."""
    st = norm_stats(x)
    e = 2.0 ** -24
    xd, wd = x.astype(np.float64), np.abs(w.astype(np.float64))
    v, s = np.abs(xd - st["mean"]), st["scale"]
    dv = st["rad"] * (1 + 2 * e) + v * (e + 2.0 ** -52)
    rho_s = st["rho_t"] + 2.0 ** -50 + e
    a = (v + dv) * s * (1 + rho_s)
    e1 = dv * s * (1 + rho_s) + v * s * rho_s
    e2 = e1 + e * a
    y64 = w.astype(np.float64) * (xd - st["mean"]) * s
    return y64, wd * (e2 + e * (a + e2)) + 2.0 ** -149 + 2.0 ** -50 * np.abs(y64)


def dequantize(blocks):
    """(d * q float64 [N, K], d per element [N, K]) of Q4_0 file blocks"""
    blocks = np.ascontiguousarray(blocks, np.uint8)
    N, nb, _ = blocks.shape
    d = np.ascontiguousarray(blocks[..., :4]).view(np.float32).reshape(N, nb, 1).astype(np.float64)
    qs = blocks[..., 4:].astype(np.int64)
    q = np.empty((N, nb, 32), np.int64)
    q[..., 0::2] = (qs & 0xF) - 8
    q[..., 1::2] = (qs >> 4) - 8
    return (d * q).reshape(N, nb * 32), np.broadcast_to(d, (N, nb, 32)).reshape(N, nb * 32)


def cancel_case(oracle, seed=3):
    """(x [1, K], w, the oracle's y [K] and blocks [1, K/32, 20], y64, B)"""
    rng = np.random.default_rng(seed)
    x = cancel_row(rng)[None, :]
    w = (1.0 + 0.3 * rng.standard_normal(x.shape[1])).astype(np.float32)
    y, blocks = reference(oracle, "norm", x, w)
    y64, B = norm_f64_bound(x[0], w)
    return x, w, y[0], blocks, y64, B
