"""The inputs of tests/test_gpu_pool_op.py (llamahip_op_pool_rows against tests/pool_ref.py, by bytes) and what tests/test_pool_host.py
asserts about them on the CPU: the coverage of the shapes and value regimes, and that every row is order-proof for the norm
(prep_cases.norm_stats), so that bit equality with the reference's sequential sums is a property of the kernel and not of a seed.

A case is (name, d, segment lengths, nan).  Every row's value regime is fixed by its place:
  the rows cycle through  unit (standard normal), offset (normal + a DC term of 3 .. 40), big (normal x 1e18), with -0.0 written into a few
  elements of every fifth row;
  the LAST row of every segment of exactly 7 rows is all zero (a zero row under LAST, with and without the normalisation);
  every segment of exactly 2 rows is all zero (a zero vector stays zero under `normalize`, under both pools);
  nan: one element of the middle row of the longest segment is NaN -- that segment's output is NaN, every other segment compares by bytes.
Each row is drawn from default_rng([seed, row, attempt]) with the first attempt that is order-proof (prep_cases.find_attempts)."""
import functools

import numpy as np

import prep_cases as pc

MIXED = (1, 2, 7, 61, 300)
SIXTEEN = tuple(1 + (5 * i) % 9 for i in range(16))          # 1 .. 9 rows, the one-row, two-row and seven-row segments among them
CASES = [("mixed", d, MIXED, False) for d in (32, 96, 256, 320, 4096)] + [
    ("mixed_nan", 96, MIXED, True),
    ("mixed_nan", 4096, (1, 2, 7, 61), True),
    ("long", 32, (2048,), False),
    ("one", 96, (5,), False),
    ("one", 4096, (1,), False),
    ("sixteen", 320, SIXTEEN, False),
    ("sixteen", 32, (1,) * 16, False),
]
VARIANTS = [(pool, normalize) for pool in ("last", "mean") for normalize in (False, True)]
SEED = 2028


def case_id(c):
    return f"{c[0]}-d{c[1]}-{len(c[2])}seg-{sum(c[2])}rows"


def seg_begin(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def row_regimes(lens):
    """the regime of every row, by its place"""
    out = []
    r = 0
    for n in lens:
        for j in range(n):
            if n == 2 or (n == 7 and j == n - 1):
                out.append("zero")
            else:
                out.append(("unit", "offset", "big")[r % 3])
            r += 1
    return out


def make_row(d, regimes):
    def f(rng, n):
        kind = regimes[n]
        if kind == "zero":
            return np.zeros(d, np.float32)
        x = rng.standard_normal(d).astype(np.float32)
        if kind == "offset":
            x = (x + np.float32(rng.uniform(3, 40))).astype(np.float32)
        elif kind == "big":
            x = (x * np.float32(1e18)).astype(np.float32)
        if n % 5 == 0:
            x[rng.permutation(d)[:3]] = np.float32(-0.0)
        return x
    return f


@functools.lru_cache(maxsize=None)
def build(c):
    """(x float32 [R, d], norm_w float32 [d], seg_begin int32 [n_segs + 1], the segment that holds the NaN or -1)"""
    name, d, lens, nan = c
    R = sum(lens)
    regimes = row_regimes(lens)
    mk = make_row(d, regimes)
    seed = SEED + d
    att = pc.find_attempts(mk, R, seed)
    x = np.stack([mk(np.random.default_rng([seed, n, a]), n) for n, a in enumerate(att)])
    w = (1.0 + 0.3 * np.random.default_rng([seed, 7]).standard_normal(d)).astype(np.float32)
    sb = seg_begin(lens)
    nan_seg = -1
    if nan:
        nan_seg = int(np.argmax(lens))
        x[(sb[nan_seg] + sb[nan_seg + 1]) // 2, d // 3] = np.float32(np.nan)
    x.setflags(write=False)
    w.setflags(write=False)
    return x, w, sb, nan_seg


def cancel_input(seed=3):
    """the row that is NOT order-proof (prep_cases.cancel_row): (x [1, 4096], w) -- held against prep_cases.norm_f64_bound, not by bytes"""
    rng = np.random.default_rng(seed)
    x = pc.cancel_row(rng)[None, :]
    w = (1.0 + 0.3 * rng.standard_normal(x.shape[1])).astype(np.float32)
    return x, w
