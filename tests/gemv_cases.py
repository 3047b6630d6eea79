"""Cases, inputs and references for tests/test_gpu_gemv_op.py (and the CPU checks of tests/test_gemv_op_host.py): the single-row decode
mat-vec k_gemv through llamahip_op_gemv_q4_0, one launch per case, against the oracle bit for bit.  Nothing here needs a GPU.

A case is Case(group, pair, M, K, wkind, regime, nparts, part_out):
  pair    one of PAIRS, the nine untagged (prologue, epilogue) pairs a launcher dispatches.  The tagged, pick and half-block pairs wait
          on other launches or workgroups; the op refuses them and the model tests / test_gpu_pick_ties.py cover them.
  wkind   how the weight matrix is drawn (weights): random Q4_0 blocks, not quantized floats, so a 40 MB matrix costs well under a second
  regime  how the activation row is drawn (activation)
  nparts  NORMP: the row's {sum x, sum x^2} arrive as this many per-slice partial sums
The groups:
  inst    one case per kernel instance (pre, epi, waves, granules, depth, ring) that tests/golden/gemv_plans.json names for the nine
          pairs, at the smallest M x K that reaches it.  INSTANCES is the committed result of find_instances, which walks the library's
          own plan (L.gemv_plan, host only) over M at the row-group class edges (1, 512, 1024, 2048 row-groups and one above each;
          interleaved matrices: 8, 512, 1024, 2048 and eight above each) and K in steps of 64.
  rows    M that is no multiple of 8 (the m < M mask, the clamped residual fetch, dead lanes in part_out) and row-group counts that
          leave the last workgroup partly valid: 4099 = 513 row-groups under two waves (three live rows), 8203 = 1026 under four, 16397.
  regime  prep_cases' value regimes through the FUSED prologues, which are implementations of their own, and DC offsets on either
          side of the norm prologue's one-pass / two-pass switch (mean * S1 <= 0.25 * S2, i.e. |mean| <= sigma / sqrt(3) = 0.577 sigma).
  epi     epilogue edges: a zero-weight row-group under residuals of -0, +0, +-inf; SILU_QA blocks whose gate or up rows are all zero.

What the reference cannot pin, and is therefore not a case:
  * a NaN residual: the payload an fp32 add hands on is the hardware's choice.
  * SILU_MUL's non-finite blocks (prep_cases.silu_edge_rows blocks 1 and 2: y = +-inf / NaN, scale inf): through a mat-vec 0 * inf makes
    EVERY output a NaN of unpinned sign and payload.  activation("silu_edges") replaces those two blocks with ordinary values; the
    non-finite blocks stay pinned where they can be observed, on the stand-alone producers (test_gpu_prep.py).
  * exact .5 ties behind a norm: the tie rows go IN to the norm ("ties"), but after the scale the quantizer's products are no longer
    exact halves; exact ties reach the fused quantizer through PLAIN.
Every NORM / NORMP row is order-proof under both forms of the second moment (prep_cases.norm_proof_both): NORM_ROW_ATTEMPTS is the
committed selection (find_norm_attempts), and the tests assert the property on every row they use."""
import collections
import functools
import json
import math
import os

import numpy as np

import prep_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 11
Case = collections.namedtuple("Case", "group pair M K wkind regime nparts part_out")
# name -> (the plan's prologue, epilogue (llamahip_internal.h), interleaved, the op's pre, the op's epi)
PAIRS = {
    "qa.store": (0, 0, False, "qa", "store"), "qa.resid": (0, 1, False, "qa", "resid"), "qa.silu_qa": (0, 2, True, "qa", "silu_qa"),
    "norm.store": (2, 0, False, "norm", "store"), "normp.store": (4, 0, False, "norm", "store"),
    "norm.silu_qa": (2, 2, True, "norm", "silu_qa"), "normp.silu_qa": (4, 2, True, "norm", "silu_qa"),
    "plain.resid": (1, 1, False, "plain", "resid"), "silu_mul.resid": (3, 1, False, "silu_mul", "resid"),
}
PAIR_OF = {v[:2]: k for k, v in PAIRS.items()}
NORM_PART_MAX = 512
NPARTS = (1, 2, 63, 64, 65, 512)
CANARY = np.uint32(0x7FC0BEEF)


def case_id(c):
    return f"{c.group}-{c.pair}-{c.M}x{c.K}-{c.wkind}-{c.regime}" + (f"-p{c.nparts}" if c.nparts else "") + ("-po" if c.part_out else "")


# ------------------------------------------------------------------------------------------------ kernel instances
# (pre, epi, waves, granules, depth, ring, M, K): find_instances(L)'s answer, committed
INSTANCES = [
    (0, 0, 1, 4, 16, 0, 8, 64), (0, 0, 1, 12, 10, 1, 8, 4160), (0, 0, 1, 12, 16, 1, 8, 7744), (0, 0, 1, 12, 18, 1, 8, 8256),
    (0, 0, 2, 4, 10, 1, 4096, 4160), (0, 0, 2, 4, 16, 0, 4096, 64), (0, 0, 2, 4, 16, 1, 4096, 7744), (0, 0, 2, 12, 10, 1, 8, 12352),
    (0, 0, 2, 12, 18, 1, 4096, 8256), (0, 0, 4, 4, 4, 1, 16384, 3904), (0, 0, 4, 4, 8, 1, 8192, 3904), (0, 0, 4, 4, 10, 1, 8192, 4160),
    (0, 0, 4, 4, 16, 0, 8192, 64), (0, 0, 4, 12, 10, 1, 8, 24640), (0, 1, 1, 4, 16, 0, 8, 64), (0, 1, 1, 12, 10, 1, 8, 4160),
    (0, 1, 1, 12, 16, 1, 8, 7744), (0, 1, 1, 12, 18, 1, 8, 8256), (0, 1, 2, 4, 10, 1, 4096, 4160), (0, 1, 2, 4, 16, 0, 4096, 64),
    (0, 1, 2, 4, 16, 1, 4096, 7744), (0, 1, 2, 12, 10, 1, 8, 12352), (0, 1, 2, 12, 18, 1, 4096, 8256), (0, 1, 4, 4, 4, 1, 16384, 3904),
    (0, 1, 4, 4, 8, 1, 8192, 3904), (0, 1, 4, 4, 10, 1, 8192, 4160), (0, 1, 4, 4, 16, 0, 8192, 64), (0, 1, 4, 12, 10, 1, 8, 24640),
    (0, 2, 8, 1, 4, 1, 16384, 3904), (0, 2, 8, 1, 8, 1, 64, 5696), (0, 2, 8, 1, 10, 1, 64, 4160), (0, 2, 8, 1, 16, 0, 64, 64),
    (0, 2, 8, 1, 16, 1, 64, 7744), (1, 1, 1, 1, 16, 0, 8, 64), (1, 1, 2, 1, 16, 0, 8, 1088), (1, 1, 4, 1, 4, 1, 16384, 3904),
    (1, 1, 4, 1, 8, 1, 8192, 3904), (1, 1, 4, 1, 16, 0, 8, 2112), (1, 1, 4, 2, 4, 1, 16384, 4160), (1, 1, 4, 2, 8, 1, 8, 5696),
    (1, 1, 4, 2, 10, 1, 8, 4160), (1, 1, 4, 2, 16, 1, 8, 7744), (2, 0, 1, 1, 16, 0, 8, 64), (2, 0, 2, 1, 16, 0, 8, 1088),
    (2, 0, 4, 1, 4, 1, 16384, 3904), (2, 0, 4, 1, 8, 1, 8192, 3904), (2, 0, 4, 1, 16, 0, 8, 2112), (2, 0, 4, 2, 4, 1, 16384, 4160),
    (2, 0, 4, 2, 8, 1, 8, 5696), (2, 0, 4, 2, 10, 1, 8, 4160), (2, 0, 4, 2, 16, 1, 8, 7744), (2, 2, 8, 1, 4, 1, 16384, 3904),
    (2, 2, 8, 1, 8, 1, 64, 5696), (2, 2, 8, 1, 10, 1, 64, 4160), (2, 2, 8, 1, 16, 0, 64, 64), (2, 2, 8, 1, 16, 1, 64, 7744),
    (3, 1, 1, 1, 10, 1, 8, 4160), (3, 1, 1, 1, 16, 0, 8, 64), (3, 1, 1, 1, 16, 1, 8, 7744), (3, 1, 1, 1, 18, 1, 8, 8256),
    (3, 1, 2, 1, 8, 1, 8192, 3904), (3, 1, 2, 1, 10, 1, 8192, 4160), (3, 1, 2, 1, 16, 0, 8192, 64), (3, 1, 4, 1, 4, 1, 16384, 3904),
    (3, 1, 4, 1, 16, 0, 16384, 64), (4, 0, 1, 1, 16, 0, 8, 64), (4, 0, 2, 1, 16, 0, 8, 1088), (4, 0, 4, 1, 4, 1, 16384, 3904),
    (4, 0, 4, 1, 8, 1, 8192, 3904), (4, 0, 4, 1, 16, 0, 8, 2112), (4, 0, 4, 2, 4, 1, 16384, 4160), (4, 0, 4, 2, 8, 1, 8, 5696),
    (4, 0, 4, 2, 10, 1, 8, 4160), (4, 0, 4, 2, 16, 1, 8, 7744), (4, 2, 8, 1, 4, 1, 16384, 3904), (4, 2, 8, 1, 8, 1, 64, 5696),
    (4, 2, 8, 1, 10, 1, 64, 4160), (4, 2, 8, 1, 16, 0, 64, 64), (4, 2, 8, 1, 16, 1, 64, 7744),
]
K_WALK_MAX = 49152          # PRE_QA's widest row: 12 granules x 256 threads = 192 chunks


def golden_instances():
    """the (pre, epi, waves, granules, depth, ring) the plan table names for the nine pairs"""
    with open(os.path.join(HERE, "golden", "gemv_plans.json")) as f:
        return {(pre, epi) + tuple(p[:4]) for _, _, _, pre, epi, p in json.load(f) if p and (pre, epi) in PAIR_OF}


def find_instances(L):
    """instance -> the (M, K) with the fewest weights that reaches it, by the walk of the module docstring; the wanted ones as INSTANCES rows"""
    found = {}
    for pre, epi, inter, _, _ in PAIRS.values():
        for ng in ((8, 16, 512, 520, 1024, 1032, 2048, 2056) if inter else (1, 2, 512, 513, 1024, 1025, 2048, 2049)):
            for K in range(64, K_WALK_MAX + 64, 64):
                p = L.gemv_plan(8 * ng, K, pre, epi, inter)
                if p is not None and ((pre, epi) + p[:4] not in found or 8 * ng * K < np.prod(found[(pre, epi) + p[:4]])):
                    found[(pre, epi) + p[:4]] = (8 * ng, K)
    return sorted(k + found[k] for k in golden_instances() if k in found)


# ------------------------------------------------------------------------------------------------ weights
def q4_random(rng, M, K, dscale):
    """Q4_0 rows uint8 [M, K/32, 20] drawn directly: every byte of codes random, scales of both signs, 2 % of them zero"""
    nb = K // 32
    m = np.empty((M, nb, 20), np.uint8)
    m[..., 4:] = rng.integers(0, 256, (M, nb, 16), dtype=np.uint8)
    dd = (rng.standard_normal((M, nb)) * dscale).astype(np.float32)
    dd[rng.random((M, nb)) < 0.02] = 0.0
    dd[M - 1, nb - 1] = 0.0
    m[..., :4] = dd.view(np.uint8).reshape(M, nb, 4)
    m[0, 0, 4:] = 0x0F                      # elements alternate code 15, code 0
    return m


def set_d(m, rows, value):
    m[rows, :, :4] = np.frombuffer(np.float32(value).tobytes(), np.uint8)


@functools.lru_cache(maxsize=3)
def weights(M, K, wkind):
    """the matrix of every case of this shape and kind (shared; read-only).  "plain": outputs of unit scale; "wide" (interleaved w1|w3):
    scaled so the gates span about +-12; "zero_group": rows 8 .. 15 have every scale zero; "silu_zero": F = M / 2, w1's rows 0 .. 31 and
    w3's rows 32 .. 63 have every scale zero (one block with all-zero gates, one with all-zero ups), the rest as "wide"."""
    rng = np.random.default_rng([SEED, M, K, ("plain", "wide", "zero_group", "silu_zero").index(wkind)])
    m = q4_random(rng, M, K, (4.0 if wkind in ("wide", "silu_zero") else 1.0) / math.sqrt(21.0 * K))
    if wkind == "zero_group":
        set_d(m, slice(8, 16), 0.0)
    if wkind == "silu_zero":
        set_d(m, slice(0, 32), 0.0)
        set_d(m, slice(M // 2 + 32, M // 2 + 64), 0.0)
    m.setflags(write=False)
    return m


def weight_properties(m):
    """what every matrix must hold: a block with d == 0, the codes 0 and 15"""
    d = np.ascontiguousarray(m[..., :4]).view(np.float32)
    lo, hi = m[..., 4:] & 0xF, m[..., 4:] >> 4
    return bool((d == 0).any()), bool((lo == 0).any() or (hi == 0).any()), bool((lo == 15).any() or (hi == 15).any())


# ------------------------------------------------------------------------------------------------ activation rows
NORM_REGIMES = ("normal:1", "normal:1e3", "normal:1e-3", "offset", "zeros:0", "zeros:1", "zeros:2", "ties", "maxpos",
                "dc:0.29", "dc:0.56", "dc:0.60", "dc:0.86")


def make_row(rng, K, regime):
    """one fp32 row [K] of a value regime (prep_cases' generators; "dc:f": unit-variance noise standardised to mean exactly f sigma)"""
    name, _, arg = regime.partition(":")
    if name == "normal":
        return (rng.standard_normal(K) * float(arg)).astype(np.float32)
    if name == "offset":          # mean 100 standard deviations from zero: the two-pass branch
        return (100.0 + rng.standard_normal(K)).astype(np.float32)
    if name == "zeros":           # 0: ordinary with one all-zero block; 1: all zero; 2: constant
        return pc.zeros_rows(rng, 3, K)[int(arg)]
    if name == "ties":
        return pc.ties_rows(rng, 1, K)[0]
    if name == "maxpos":
        return pc.maxpos_rows(rng, 1, K)[0] + (rng.standard_normal(K) * 1e-3).astype(np.float32)
    if name == "dc":
        z = rng.standard_normal(K)
        return (float(arg) + (z - z.mean()) / z.std()).astype(np.float32)
    raise KeyError(regime)


# (K, regime) -> the draw whose row is order-proof under both forms (find_norm_attempts' answer, committed; 0 = the first draw is not
# listed).  Empty: the first draw of every row of the table passes both checks -- K stays below 8192 here, where prep_cases' own table needs a
# second draw only at 22016.  tests/test_gemv_op_host.py recomputes it, so a changed case that needs another draw fails there.
NORM_ROW_ATTEMPTS = {
}


def row_seed(K, regime):
    return (SEED * 100000 + K) * 100 + NORM_REGIMES.index(regime)


def norm_row(K, regime):
    """the NORM / NORMP row of (K, regime): draw NORM_ROW_ATTEMPTS[(K, regime)] of prep_cases.find_attempts' sequence (row 0)"""
    a = NORM_ROW_ATTEMPTS.get((K, regime), 0)
    return make_row(np.random.default_rng([row_seed(K, regime), 0, a]), K, regime)


def find_norm_attempts(cases, limit=200):
    """the entries of NORM_ROW_ATTEMPTS that are not 0, for every NORM / NORMP row of `cases`: prep_cases.find_attempts under both checks"""
    out = {}
    for K, regime in sorted({(c.K, c.regime) for c in cases if c.pair.startswith("norm")}):
        a, = pc.find_attempts(lambda rng, n: make_row(rng, K, regime), 1, row_seed(K, regime), limit, proof=pc.norm_proof_both)
        if a:
            out[(K, regime)] = a
    return out


def norm_weight(K):
    return (1.0 + 0.5 * np.random.default_rng([SEED, K]).standard_normal(K)).astype(np.float32)          # (some negative, a few near zero)


def norm_parts(x, n):
    """n pairs {fsum(x), fsum(x^2)} of contiguous slices of the row (empty slices where n > K), float64 [n, 2]"""
    xd = x.astype(np.float64)
    return np.array([[math.fsum(s), math.fsum(s * s)] for s in np.array_split(xd, n)], np.float64).reshape(n, 2)


def silu_finite_edges(rng, K):
    """prep_cases.silu_edge_rows with its two non-finite blocks replaced by ordinary values (module docstring)"""
    gate, up = pc.silu_edge_rows(rng, 1, K)
    gate[0, 32:96] = rng.standard_normal(64).astype(np.float32) * np.float32(2.0)
    return gate[0], up[0]


def resid_row(rng, c):
    r = rng.standard_normal(c.M).astype(np.float32)
    if c.wkind == "zero_group":
        r[8:16] = np.array([-0.0, 0.0, np.inf, -np.inf, 0.0, -0.0, -np.inf, np.inf], np.float32)
    return r


def build(oracle, c):
    """the operands of a case: dict(w, in0, in1, resid, part_in) as llamahip_op_gemv_q4_0 takes them (None where the pair takes none)"""
    pre, epi, inter, op_pre, op_epi = PAIRS[c.pair]
    rng = np.random.default_rng([SEED, c.M, c.K, sorted(PAIRS).index(c.pair), 1])
    in1 = part_in = None
    if op_pre == "norm":
        in0, in1 = norm_row(c.K, c.regime), norm_weight(c.K)
        if c.nparts:
            part_in = norm_parts(in0, c.nparts)
    elif op_pre == "silu_mul":
        if c.regime == "silu_edges":
            in0, in1 = silu_finite_edges(rng, c.K)
        else:
            in0, in1 = (rng.standard_normal(c.K) * 2.0).astype(np.float32), rng.standard_normal(c.K).astype(np.float32)
    else:
        in0 = make_row(np.random.default_rng([SEED, c.K, 99]), c.K, c.regime)          # (QA and PLAIN share the row of a (K, regime))
    return dict(w=weights(c.M, c.K, c.wkind), in0=in0, in1=in1, resid=resid_row(rng, c) if op_epi == "resid" else None, part_in=part_in)


_acc = collections.OrderedDict()          # (M, K, wkind, the row's bytes) -> the oracle's mat-vec, shared among the pairs of a shape


def reference(oracle, c, ops):
    """dict(row, y, out_A, out_d): the activation row the prologue must make (fp32), the outputs the launch must leave (module docstring
    of the test file: every reference is what the suite already trusts)"""
    pre, epi, inter, op_pre, op_epi = PAIRS[c.pair]
    with np.errstate(all="ignore"):
        if op_pre == "norm":
            row = pc.reference(oracle, "norm", ops["in0"][None, :], ops["in1"])[0][0]
        elif op_pre == "silu_mul":
            row = pc.reference(oracle, "silu_mul", ops["in0"][None, :], ops["in1"][None, :])[0][0]
        else:
            row = ops["in0"]
        key = (c.M, c.K, c.wkind, row.tobytes())
        if key not in _acc:
            _acc[key] = oracle.mul_mat_q4_0(ops["w"], row[None, :])[0]
            while len(_acc) > 4:
                _acc.popitem(last=False)
        acc = _acc[key]
        if op_epi == "store":
            return dict(row=row, y=acc, out_A=None, out_d=None)
        if op_epi == "resid":
            return dict(row=row, y=acc + ops["resid"], out_A=None, out_d=None)          # ONE fp32 add
        F = c.M // 2
        y, blocks = pc.reference(oracle, "silu_mul", acc[None, :F], acc[None, F:])
        out_A, out_d = pc.pack_qa(blocks, F)
        return dict(row=row, y=y[0], out_A=out_A[0], out_d=out_d[0], gate=acc[:F], up=acc[F:])


# ------------------------------------------------------------------------------------------------ the case table
def _cases():
    out = []
    for pre, epi, nw, pg, depth, ring, M, K in INSTANCES:
        pair = PAIR_OF[(pre, epi)]
        grid = ((M + 7) // 8 + nw - 1) // nw
        out.append(Case("inst", pair, M, K, "wide" if PAIRS[pair][2] else "plain", "normal:1", 3 if pre == 4 else 0, epi == 1 and grid <= NORM_PART_MAX))
    for K in (64, 320, 4160):
        for M in (1, 5, 13, 4099, 8203, 16397):
            out.append(Case("rows", "qa.store", M, K, "plain", "normal:1", 0, False))
            out.append(Case("rows", "qa.resid", M, K, "plain", "normal:1", 0, M != 16397))          # (16397: 513 workgroups > NORM_PART_MAX)
            out.append(Case("rows", "plain.resid", M, K, "plain", "normal:1", 0, False))
    for K in (320, 4096):
        for i, regime in enumerate(NORM_REGIMES):
            out.append(Case("regime", "norm.store", 24, K, "plain", regime, 0, False))
            every = regime in ("normal:1", "dc:0.56", "dc:0.60")
            for n in (NPARTS if every else (NPARTS[(i + K // 4096) % len(NPARTS)],)):
                out.append(Case("regime", "normp.store", 24, K, "plain", regime, n, False))
        for regime in ("ties", "maxpos", "zeros:0", "zeros:1"):
            out.append(Case("regime", "plain.resid", 24, K, "plain", regime, 0, False))
        out.append(Case("regime", "silu_mul.resid", 24, K, "plain", "silu_edges", 0, False))
    for K in (320, 4160):
        out.append(Case("epi", "qa.resid", 24, K, "zero_group", "normal:1", 0, True))
        out.append(Case("epi", "plain.resid", 24, K, "zero_group", "normal:1", 0, False))
    for K in (320, 4096):
        for pair, n in (("norm.silu_qa", 0), ("normp.silu_qa", 65), ("qa.silu_qa", 0)):
            out.append(Case("epi", pair, 448, K, "silu_zero", "normal:1", n, False))          # (F = 224: seven blocks, a padded last chunk)
    return out


CASES = _cases()
SILU = [c for c in CASES if "silu" in c.pair]          # the cases that read the SiLU table: also run with the table gathered (tests/variants.py)
