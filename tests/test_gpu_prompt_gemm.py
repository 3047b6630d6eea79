"""GPU (-m gpu): the prompt GEMMs op by op (llamahip_op_prompt_gemm_q4_0), each kernel forced at the tails a model rarely reaches.

a. The exact kernels -- what launch_gemm picks for a model handle (AUTO), k_gemm_mfma4, the int8 matrix-core kernel, k_gemm_rows, k_gemv_set
   and k_gemm_lds -- equal oracle.mul_mat_q4_0 bit for bit (with a residual: that product + resid in fp32) at ragged M (an odd number of
   32-row tiles, row pairs that do not fill the 8-XCD stride), padded K (K % 256 != 0) and every N from 1 up past the 64-column tiles.
b. The fast kernel (LLAMAHIP_FLAG_FAST_PREFILL) is not the reference's arithmetic; it is held to a proven bound instead.  Per output it
   rounds t_b's scale product once and runs one fp32 FMA chain over the n = Kp/32 blocks, so with y* = sum_b t_b in float64
   (t_b = d_w,b * d_a,b * s_b, s_b the exact integer dot product of block b):  |y - y*| <= gamma_{n+1} * sum_b |t_b|,
   gamma_k = k u / (1 - k u), u = 2^-24 (+ u |y* + r| and the float64 slack with a residual).  The looser sum |w| |x| replaces sum |t_b|
   at the big shapes.  The bound is shown to be tight enough to catch a lost block: on ordinary outputs it stays below 1/20 of the
   median |t_b|.  The exact kernels' error is bounded the same way (eight chains and a depth-3 tree: gamma_{n+4} * sum |w| |x|).
c. The fast kernel's structure, bit for bit: a column depends on its activation row only, and two runs agree.
Every call gets a y buffer wider than M (y_stride > M) filled with canaries: nothing outside the N x M block may change."""
import numpy as np
import pytest

import synth
from gemm_ref import U, Ref, gamma, split  # noqa: F401  (the yardstick, shared with test_gpu_gemv_set_op.py)

pytestmark = pytest.mark.gpu
EXACT = ("auto", "mfma4", "mfma_i8", "rows", "set", "lds")
REPORT: dict = {}            # path -> list of (shape, largest |y - y*| / bound)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def describe(got, want):
    d = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if d.size == 0:
        return "bitwise-equal values, different NaN payloads or signs of zero"
    n, m = d[0]
    return f"{len(d)} of {got.size} outputs differ; first at (n {n}, m {m}): got {got[n, m]!r} want {want[n, m]!r}"


def special_rows(M):
    return sorted({0, 1 % M, M // 2, M - 1})


def make_weights(M, K, seed):
    """offline-quantized random rows, then: row 0 saturating (a block of code -8 everywhere, one of -8 / +7 alternating), row 1 a block
    with d = 0, rows M/2 and M-1 block scales from 1e-3 to 1e3 (chain order matters)"""
    rng = np.random.default_rng(seed)
    w = synth.quantize_q4_0_offline((0.02 * rng.standard_normal((M, K))).astype(np.float32))
    nb = K // 32
    w[0, 1, 4:] = 0x00                                  # 32 codes of -8
    w[0, 2, 4:] = 0xF0                                  # -8, +7, -8, +7, ...
    w[1 % M, 0, :4] = np.zeros(1, np.float32).view(np.uint8)
    for r in {M // 2, M - 1} - {0, 1 % M}:
        w[r, :, :4] = (10.0 ** rng.uniform(-3, 3, nb)).astype(np.float32).view(np.uint8).reshape(nb, 4)
    return w


def make_x(N, K, seed):
    """random rows at per-row scales; row 0 opens with an all-zero block, row 1 has a block at one magnitude (codes +-7), the last row of
    three or more is all zero"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((N, K)) * rng.uniform(0.1, 4, (N, 1))).astype(np.float32)
    x[0, :32] = 0
    x[1 % N, 32:64] = np.where(rng.random(32) < 0.5, -1.5, 1.5).astype(np.float32)
    if N >= 3:
        x[N - 1] = 0
    return x


def record(path, shape, ratio):
    REPORT.setdefault(path, []).append((shape, ratio))


def run(L, w, x, resid, path, canary):
    N, M = x.shape[0], w.shape[0]
    y, taken = L.op_prompt_gemm_q4_0(w, x, resid, path=path, y_stride=canary.shape[1], y_init=canary)
    assert same(y[:, M:], canary[:, M:]), f"{path}: a column past M was written (y_stride {canary.shape[1]}, M {M})"
    return y[:, :M], taken


def canaries(N, M, seed):
    c = np.random.default_rng(seed).standard_normal((N, M + 5)).astype(np.float32) * np.float32(1e6)
    c[:, M:] = np.float32(-7.5e33)
    return c


# (M, K, N, with resid): M in {8, 32, 33, 96, 250, 512, 544, 4096, 4097}, K in {256, 320, 1344, 4096, 11008}, N in {1, 2, 31, 63, 64, 65,
# 127, 128, 129, 200, 512} (and 33), paired so that every value meets several others; the 7B shapes last
SHAPES = [(8, 256, 1, False), (8, 320, 65, True), (32, 1344, 2, False), (33, 320, 31, True), (33, 1344, 129, False), (96, 256, 63, False),
          (96, 4096, 64, True), (96, 11008, 200, False), (250, 1344, 127, False), (250, 320, 200, True), (512, 256, 128, False),
          (512, 11008, 31, False), (544, 1344, 65, False), (544, 4096, 129, True), (544, 320, 512, False), (4096, 4096, 127, False),
          (4096, 320, 33, True), (4097, 256, 512, False), (4097, 1344, 63, True), (4097, 11008, 1, False), (4097, 4096, 128, False),
          (12288, 4096, 65, False), (12288, 4096, 512, False), (22016, 4096, 65, False), (4096, 11008, 129, True)]


@pytest.mark.parametrize("M,K,N,with_resid", SHAPES)
def test_prompt_gemm_paths(L, oracle, M, K, N, with_resid):
    seed = M * 7 + K * 3 + N
    w, x = make_weights(M, K, seed), make_x(N, K, seed + 1)
    resid = (np.random.default_rng(seed + 2).standard_normal((N, M)) * 3).astype(np.float32) if with_resid else None
    want = oracle.mul_mat_q4_0(w, x, 8)
    if resid is not None:
        want = want + resid                              # fp32 + fp32: the kernels' epilogue
    ref = Ref(oracle, w, x, resid)
    canary = canaries(N, M, seed + 3)
    shape = f"{M}x{K} N={N}" + (" +resid" if with_resid else "")
    b_exact = ref.bound_exact()
    for path in EXACT:
        try:
            got, taken = run(L, w, x, resid, path, canary)
        except L.LlamaHipError as e:
            assert path == "set" and "k_gemv_set" in e.message, e.message     # only the few-row kernel refuses a shape
            continue
        assert taken == path or path == "auto" or (path == "lds" and N == 1 and taken == "gemv"), (path, taken)
        assert same(got, want), f"{path} (took {taken}) at {shape}: " + describe(got, want)
        err = ref.err(got)
        assert np.all(err <= b_exact), f"{path}: exact path outside its bound"
        record(path if path != "auto" else f"auto -> {taken}", shape, float(np.max(np.where(b_exact > 0, err / np.maximum(b_exact, 1e-300), 0))))
    fast, taken = run(L, w, x, resid, "fast", canary)
    assert taken == "fast"
    assert np.all(np.isfinite(fast[np.isfinite(want)]))
    b_fast = ref.bound_fast()
    err = ref.err(fast)
    bad = np.argwhere(err > b_fast)
    assert bad.size == 0, (f"fast kernel at {shape}: {len(bad)} outputs outside the bound; first (n {bad[0][0]}, m {bad[0][1]}): "
                           f"|y - y*| {err[tuple(bad[0])]:.6e} > bound {b_fast[tuple(bad[0])]:.6e}")
    assert np.all(np.abs(fast.astype(np.float64) - want.astype(np.float64)) <= b_fast + b_exact)
    ratio = float(np.max(np.where(b_fast > 0, err / np.maximum(b_fast, 1e-300), 0)))
    ord_w = [m for m in range(M) if m not in special_rows(M)] or list(range(M))
    ord_x = [n for n in range(N) if np.any(x[n] != 0)]
    margin = ref.lost_block_margin(ord_w, ord_x, np.random.default_rng(seed + 4))
    record("fast", shape + f" (bound / median |t_b| <= {margin:.1e}" + (", sum |w||x| form" if ref.sabs_t is None else "") + ")", ratio)


def test_fast_kernel_columns_are_independent_and_runs_repeat(L):
    """k_gemm_mfma<*, true> bit for bit against itself: the rows of an N = 512 product equal the same rows run as N = 65 and one at a time
    (the smallest N the kernel takes), and the rows permuted; a second run gives the same bits; and it is not the int8 exact kernel."""
    M, K, N = 544, 1344, 512
    w, x = make_weights(M, K, 5), make_x(N, K, 6)
    canary = canaries(N, M, 7)
    full, _ = run(L, w, x, None, "fast", canary)
    again, _ = run(L, w, x, None, "fast", canary)
    assert same(full, again), "two runs of the fast kernel differ"
    part, _ = run(L, w, x[:65], None, "fast", canary[:65])
    assert same(part, full[:65]), "N = 65 differs from the first 65 rows of N = 512: " + describe(part, full[:65])
    for n in (0, 1, 64, 200, 511):
        one, _ = run(L, w, x[n:n + 1], None, "fast", canary[:1])
        assert same(one, full[n:n + 1]), f"row {n} alone differs"
    perm = np.random.default_rng(8).permutation(N)
    pm, _ = run(L, w, x[perm], None, "fast", canary)
    assert same(pm, full[perm]), "permuted rows differ: " + describe(pm, full[perm])
    exact, _ = run(L, w, x, None, "mfma_i8", canary)
    assert not same(full, exact), "the fast kernel gave the exact kernel's bits: it did not run"


def test_zz_report():
    """(last in the module) what the forced paths ran and how close each came to its bound"""
    for path in sorted(REPORT):
        rows = REPORT[path]
        print(f"\n{path}: {len(rows)} shapes, largest |y - y*| / bound {max(r for _, r in rows):.3e}")
        for shape, r in rows:
            print(f"    {shape:58s} {r:.3e}")
