"""The yardstick and the case list of the Q4_1 mat-mul tests (tests/test_q41_host.py, tests/test_gpu_q41_op.py).

The yardstick restates the reference's quantize_row_q4_1 (ggml.c:606-648) and ggml_vec_dot_q4_1 (ggml.c:1584-1626, scalar, built without
contraction) in numpy: every array float32, vectorised over (m, n), a Python loop over the K/2 byte pairs in order so that every `*` and
`+` is one fp32 rounding.  Weights are generated directly in FILE layout: per row [K/32 f32 min][K/32 f32 d][K/32 * 16 nibble bytes]."""
import numpy as np

BASE = dict(M=65, K=896, N=3)
F32 = np.float32


def make_weights(M, K, seed, d_zero_every=0, neg_min=False):
    """file-layout rows uint8 [M, K/32 * 24]: random fp32 min (both signs; neg_min: all negative), d in [0.01, 0.11) and nibble bytes;
    d_zero_every = e > 0: every e-th block of every row has d = 0"""
    rng = np.random.default_rng(seed)
    nb = K // 32
    mn = ((rng.random((M, nb), dtype=F32) - F32(0.5)) * F32(0.6)).astype(F32)
    if neg_min:
        mn = -np.abs(mn) - F32(0.01)
    d = (rng.random((M, nb), dtype=F32) * F32(0.1) + F32(0.01)).astype(F32)
    if d_zero_every:
        d[:, ::d_zero_every] = 0
    q = rng.integers(0, 256, (M, nb * 16), dtype=np.uint8)
    return np.concatenate([mn.view(np.uint8), d.view(np.uint8), q], axis=1)


def make_x(N, K, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, K)) * scale).astype(F32)


def make_resid(N, M, seed):
    return np.random.default_rng(seed).standard_normal((N, M)).astype(F32)


def split_weights(w, K):
    """file-layout rows -> (min [M, nb], d [M, nb], nibble bytes [M, nb * 16])"""
    nb = K // 32
    w = np.ascontiguousarray(w, np.uint8)
    return w[:, :4 * nb].copy().view(F32), w[:, 4 * nb:8 * nb].copy().view(F32), w[:, 8 * nb:]


def expand_x(x):
    """quantize_row_q4_1 followed by the expansion ggml_vec_dot_q4_1 does: a = d1 * code + m1, f32 [N, K]"""
    x = np.ascontiguousarray(x, F32)
    N, K = x.shape
    xb = x.reshape(N, K // 32, 32)
    mn, mx = xb.min(axis=2, keepdims=True), xb.max(axis=2, keepdims=True)
    d = ((mx - mn) / F32(15.0)).astype(F32)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, F32(1.0) / np.where(d != 0, d, F32(1.0)), F32(0.0)).astype(F32)
    t = ((xb - mn).astype(F32) * idv).astype(F32)                                # t >= 0
    code = (np.floor(t.astype(np.float64) + 0.5).astype(np.int64) & 0xFF & 0xF)    # C round() of the fp32 t, (uint8), 4 bits survive
    return ((d * code.astype(F32)).astype(F32) + mn).astype(F32).reshape(N, K)


def pair_terms(w, x, fused=False):
    """the K/2 pair terms of every output in pair order: f32 [K/2, N, M].  fused: each term formed as fma(f1, a1, f0 * a0) (emulated in
    float64: the product of two fp32 values is exact there, and the one rounding of the sum to fp32 follows) -- what the yardstick must
    be able to tell from the reference's four roundings"""
    N, K = x.shape
    mn, d, q = split_weights(w, K)
    a = expand_x(x)
    out = np.empty((K // 2, N, w.shape[0]), F32)
    for j in range(K // 2):
        i = j // 16
        b = q[:, j]
        f0 = ((d[:, i] * (b & 0xF).astype(F32)).astype(F32) + mn[:, i]).astype(F32)
        f1 = ((d[:, i] * (b >> 4).astype(F32)).astype(F32) + mn[:, i]).astype(F32)
        a0, a1 = a[:, 2 * j, None], a[:, 2 * j + 1, None]
        t = (f0[None, :] * a0).astype(F32)
        if fused:
            out[j] = (t.astype(np.float64) + f1[None, :].astype(np.float64) * a1.astype(np.float64)).astype(F32)
        else:
            out[j] = (t + (f1[None, :] * a1).astype(F32)).astype(F32)
    return out


def chain(terms, reverse=False):
    """sumf += term, one fp32 accumulator per output, in pair order (reverse: the same terms from the last pair to the first)"""
    s = np.zeros(terms.shape[1:], F32)
    for j in (range(terms.shape[0] - 1, -1, -1) if reverse else range(terms.shape[0])):
        s = (s + terms[j]).astype(F32)
    return s


def yardstick(w, x, resid=None):
    """y f32 [N, M]"""
    y = chain(pair_terms(w, x))
    return y if resid is None else (y + np.ascontiguousarray(resid, F32)).astype(F32)


def base_inputs():
    return make_weights(BASE["M"], BASE["K"], seed=4101), make_x(BASE["N"], BASE["K"], seed=4102)


# value regimes on the base shape: name -> (w, x).  Every operand and product stays in the normal fp32 range.
def regime_inputs(name):
    M, K, N = BASE["M"], BASE["K"], BASE["N"]
    w, x = base_inputs()
    if name == "equal_block":               # an activation block of 32 equal values: d1 = 0, id = 0
        x = x.copy()
        x[1, 64:96] = F32(0.375)
        x[2, 0:32] = F32(-1.25)
    elif name == "outlier":                 # one value 1e4 times the rest: the codes collapse to 0 / 15
        x = x.copy()
        x[0, 37] = F32(1.0e4)
        x[2, 500] = F32(-1.0e4)
    elif name == "d_zero":                  # weight blocks with d = 0
        w = make_weights(M, K, seed=4103, d_zero_every=3)
    elif name == "neg_min":                 # negative min on both sides
        w = make_weights(M, K, seed=4104, neg_min=True)
        x = (-np.abs(x) - F32(0.5)).astype(F32)
    else:
        raise KeyError(name)
    return w, x


REGIMES = ("equal_block", "outlier", "d_zero", "neg_min")
