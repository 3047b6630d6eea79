"""The float64 numpy restatement of k_kv_shift_rows (include/llamahip.h, llamahip_kv_shift_rows), the derived rounding bound, and the
op-level cases shared by tests/test_kv_shift_host.py (the restatement's own properties, CPU) and tests/test_gpu_kv_shift_op.py (the kernel).

The kernel's arithmetic is its definition: with (c, s) = table[n_discard][pair] from the LIBRARY's table (llamahip_debug_rope_table; other
libms differ in the last bit of some entries),
    y0 = f32(rn(rn(f64(x0) * c) + rn(f64(x1) * s)))      y1 = f32(rn(rn(f64(x1) * c) - rn(f64(x0) * s)))
numpy's float64 multiply / add / subtract are one rounded operation each, astype(float32) rounds to nearest even: the same bits.

The bound.  A key written at position p is k_p = f32(R_p k) (one narrowing, error <= 2^-24 |component| <= 2^-24 ||pair||).  The shift
gives f32(R_-n k_p): the first narrowing's error vector (each component <= 2^-24 ||pair||, so its length <= sqrt(2) 2^-24 ||pair||) is
rotated, which keeps its length, and may land on one component: sqrt(2) 2^-24 ||pair||; the second narrowing adds 2^-24 ||pair||; the
direct key f32(R_(p-n) k) it is compared with carries its own 2^-24 ||pair||.  Sum: (2 + sqrt(2)) 2^-24 ||pair|| < 3.5 * 2^-24 ||pair||
per component (the float64 operations' and the tables' own errors, ~2^-52, vanish in the margin)."""
import numpy as np

BOUND = 3.5 * 2.0 ** -24
U = 8          # LLAMAHIP_KV_SHIFT_ROWS_IN_FLIGHT (asserted against the library where the cases are used)
BAND = 4 * U    # rows of the "long" cases below: several batches per thread
MAGS = (1e-3, 1.0, 50.0)

# (row_begin, n_rows, n_discard) at n_ctx 40
N_CTX = 40
GEOMETRY = [(1, 1, 1), (39, 1, 39), (20, 20, 20), (20, 20, 19), (1, 39, 1), (3, 37, 3), (7, 33, 5), (30, 5, 10)]
# the kernel's batch edges: n_rows of U - 1, U, U + 1, 2U + 1 at n_discard 1 and U
BATCH_EDGES = [(nd, n, nd) for nd in (1, U) for n in (U - 1, U, U + 1, 2 * U + 1)]
# (d, dh): two heads of 64; three heads of 128 (a row that is not a power of two in bytes)
WIDTHS = [(128, 64), (384, 128)]
# long shifts whose ranges do not alias, at n_ctx 160 (n_rows <= n_discard, so n_ctx >= 2 n_rows) -- the plan's crossing at every real context
# size is of this kind, a thread walking many batches of rows: 4U + 1 rows, 8U, 8U + 5 (a tail that is no multiple of U), and n_rows < n_discard
N_CTX_BANDS = 160
BANDED = [(BAND + 1, BAND + 1, BAND + 1), (2 * BAND, 2 * BAND, 2 * BAND), (2 * BAND + 6, 2 * BAND + 5, 2 * BAND + 6), (80, 2 * BAND + 5, 75)]
# 16 shifts of different geometry, one per slot of a 16-slot cache: empty ones (which have no items in the kernel's numbering), aliasing
# ones and long non-aliasing ones side by side
SIXTEEN = [(s,) + g for s, g in enumerate(GEOMETRY + [(5, 0, 2), (40, 0, 40), (12, 28, 12), (70, 69, 70), (2, 17, 2), (64, 64, 64), (25, 15, 25), (80, 80, 80)])]


def rotate_down(rows, tab, n_discard, dh):
    """rows f32 [..., d] -> the kernel's re-rotation by -n_discard positions, f32"""
    x = np.asarray(rows, np.float32).astype(np.float64)
    d = x.shape[-1]
    cs = np.tile(tab[n_discard], (d // dh, 1))          # [d / 2, 2]: pair e / 2 reads entry (e % dh) / 2
    c, s = cs[:, 0], cs[:, 1]
    x0, x1 = x[..., 0::2], x[..., 1::2]
    y = np.empty_like(x)
    y[..., 0::2] = x0 * c + x1 * s
    y[..., 1::2] = x1 * c - x0 * s
    return y.astype(np.float32)


def shift_restated(K, V, tab, dh, shifts):
    """K, V f32 [n_slots, n_layers, n_ctx, d], changed in place: every shift (slot, row_begin, n_rows, n_discard) on every layer"""
    for slot, rb, n, nd in shifts:
        if n == 0:
            continue
        K[slot, :, rb - nd:rb - nd + n] = rotate_down(K[slot, :, rb:rb + n].copy(), tab, nd, dh)
        V[slot, :, rb - nd:rb - nd + n] = V[slot, :, rb:rb + n].copy()


def no_subnormals(a):
    """the contract's condition on the inputs: every expected output is zero or at least 2^-126 in magnitude"""
    m = np.abs(np.asarray(a, np.float32))
    return bool(np.all((m == 0) | (m >= np.float32(2.0 ** -126))))


def within_bound(got, direct, raw):
    """got, direct f32 [..., d]; raw: the un-rotated rows (f32): |got - direct| <= BOUND * ||pair||_2 per component; returns the worst ratio
    to 2^-24 ||pair|| (so the assertion is `< 3.5`), 0 where every pair is zero"""
    r = np.asarray(raw, np.float32).astype(np.float64)
    norm = np.repeat(np.sqrt(r[..., 0::2] ** 2 + r[..., 1::2] ** 2), 2, axis=-1)
    err = np.abs(np.asarray(got, np.float32).astype(np.float64) - np.asarray(direct, np.float32).astype(np.float64))
    assert np.all(err[norm == 0] == 0)
    nz = norm > 0
    return float(np.max(err[nz] / (norm[nz] * 2.0 ** -24))) if nz.any() else 0.0


def make_caches(oracle, seed, n_slots, n_layers, n_ctx, d, dh):
    """(raw, K, V): raw random rows in the three magnitude regimes (one per row) with some exact +0.0 / -0.0 pairs, K = oracle.rope of raw
    at the rows' positions, V random: no byte of either cache is a constant fill"""
    rng = np.random.default_rng(seed)
    shape = (n_slots, n_layers, n_ctx, d)
    mag = np.asarray(MAGS, np.float32)[rng.integers(0, 3, size=shape[:3])][..., None]
    raw = (rng.standard_normal(shape).astype(np.float32) * mag).astype(np.float32)
    pairs = raw.reshape(shape[:3] + (d // 2, 2))
    z = rng.random(pairs.shape[:-1]) < 0.02
    pairs[z] = np.where(rng.random((int(z.sum()), 2)) < 0.5, np.float32(0.0), np.float32(-0.0))
    K = np.empty(shape, np.float32)
    for s in range(n_slots):
        for il in range(n_layers):
            K[s, il] = oracle.rope(raw[s, il].reshape(n_ctx, d // dh, dh), 0, 0).reshape(n_ctx, d)          # row i at position i
    V = (rng.standard_normal(shape).astype(np.float32) * mag).astype(np.float32)
    return raw, K, V


def direct_keys(oracle, raw_rows, new_begin, dh):
    """oracle.rope of the un-rotated rows [n, d] at positions new_begin, new_begin + 1, ..."""
    n, d = raw_rows.shape
    return oracle.rope(raw_rows.reshape(n, d // dh, dh), new_begin, 0).reshape(n, d)


def op_cases():
    """(id, n_slots, n_layers, n_ctx, d, dh, shifts): every op-level case of the GPU file"""
    out = []
    for d, dh in WIDTHS:
        for rb, n, nd in GEOMETRY:
            out.append((f"d{d}-rb{rb}-n{n}-nd{nd}", 3, 3, N_CTX, d, dh, [(1, rb, n, nd)]))
        out.append((f"d{d}-empty_beside_real", 3, 3, N_CTX, d, dh, [(0, 10, 0, 3), (2, 7, 33, 5)]))
        for rb, n, nd in BATCH_EDGES:
            out.append((f"d{d}-edge-n{n}-nd{nd}", 3, 3, N_CTX, d, dh, [(2, rb, n, nd)]))
        for rb, n, nd in BANDED:
            out.append((f"d{d}-bands-rb{rb}-n{n}-nd{nd}", 3, 3, N_CTX_BANDS, d, dh, [(1, rb, n, nd)]))
        out.append((f"d{d}-bands_beside_an_aliasing_shift", 3, 3, N_CTX_BANDS, d, dh, [(2, 2 * BAND + 6, 2 * BAND + 5, 2 * BAND + 6), (0, 1, 159, 1), (1, BAND + 1, BAND + 1, BAND + 1)]))
    out.append(("d128-sixteen_shifts", 16, 3, N_CTX_BANDS, 128, 64, SIXTEEN))
    out.append(("d4096-two_slots", 2, 2, 64, 4096, 128, [(1, 32, 32, 32), (0, 9, 55, 9)]))
    return out
