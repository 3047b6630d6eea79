"""GPU (-m gpu): llamahip_op_pool_rows -- k_norm_rows_f32, k_pool_rows and the L2 normalisation on caller-supplied rows -- against
tests/pool_ref.py, the float64 numpy restatement over the oracle's norm.  Compared by bytes, no tolerance: every input row is order-proof for
the norm (asserted on the CPU in tests/test_pool_host.py), the pooling and the normalisation have a stated order.  The cases, shapes and
value regimes are tests/pool_cases.py's.  The output buffer is pre-filled with a sentinel and has one spare segment's room behind it."""
import numpy as np
import pytest

import pool_cases as cases
import pool_ref
import prep_cases as pc

pytestmark = pytest.mark.gpu
SENTINEL = np.uint32(0x7FC0BEEF)


@pytest.fixture(scope="module")
def normed(oracle):
    """the reference's normed rows per case, computed once and left unchanged"""
    out = {}
    for c in cases.CASES:
        x, w, _, _ = cases.build(c)
        y = pool_ref.norm_rows(oracle, x, w)
        y.setflags(write=False)
        out[c] = y
    return out


@pytest.mark.parametrize("pool,normalize", cases.VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_pool_rows_against_the_restatement_by_bytes(L, normed, c, pool, normalize):
    x, w, sb, nan_seg = cases.build(c)
    n_segs, d = len(sb) - 1, x.shape[1]
    want = pool_ref.pool_normed(normed[c], sb, pool, normalize)
    buf = np.full((n_segs + 1) * d, SENTINEL, np.uint32).view(np.float32)
    got = L.op_pool_rows(x, w, sb, pool, normalize, out=buf)
    assert got.shape == (n_segs, d) and np.shares_memory(got, buf)
    assert (buf.view(np.uint32)[n_segs * d:] == SENTINEL).all(), "written behind the result"
    for s in range(n_segs):
        g, wv = got[s], want[s]
        if s == nan_seg and (pool == "mean" or np.isnan(wv).any()):
            # the NaN stays in its segment: where the restatement has a NaN the kernel has one, every other element by bytes
            assert np.isnan(wv).any() and np.array_equal(np.isnan(g), np.isnan(wv)), (cases.case_id(c), s)
            ok = ~np.isnan(wv)
            assert np.array_equal(g[ok].view(np.uint32), wv[ok].view(np.uint32)), (cases.case_id(c), s)
            continue
        bad = np.flatnonzero(g.view(np.uint32) != wv.view(np.uint32))
        assert bad.size == 0, (cases.case_id(c), pool, normalize, f"segment {s}: {bad.size} elements differ, first at {bad[:4]}", g[bad[:4]], wv[bad[:4]])
        assert np.isfinite(g).all()
    # the zero vectors stay zero under the normalisation (a whole all-zero segment under both pools, a zero last row under LAST)
    lens = np.diff(sb)
    for s in np.flatnonzero(lens == 2):
        assert not got[s].any()
    if pool == "last":
        for s in np.flatnonzero(lens == 7):
            assert not got[s].any()


def test_the_row_that_is_not_order_proof_meets_the_float64_bound(L):
    """prep_cases.cancel_row: the double sums cancel by eight orders of magnitude, so the kernel's order of them may show -- within the bound that
    holds for EVERY order (prep_cases.norm_f64_bound)"""
    x, w = cases.cancel_input()
    y64, B = pc.norm_f64_bound(x[0], w)
    got = L.op_pool_rows(x, w, [0, 1], "last", False)[0]
    err = np.abs(got.astype(np.float64) - y64)
    print("cancel row: max |y - y64| / B =", float((err / B).max()))
    assert np.all(err <= B)
    # ... and MEAN over the one row is the row itself: acc = 0.0 + y, divided by 1.0
    assert np.array_equal(L.op_pool_rows(x, w, [0, 1], "mean", False)[0].view(np.uint32), got.view(np.uint32))
