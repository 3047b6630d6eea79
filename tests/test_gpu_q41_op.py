"""GPU (-m gpu): the Q4_1 mat-mul kernels alone (llamahip_op_mul_mat_q4_1), bit for bit: k_q41_chain (path CHAIN, what model handles run) =
k_q41_mm (path LANE) = the numpy restatement of the reference's quantize_row_q4_1 + ggml_vec_dot_q4_1 (tests/q41_cases.py).  From the base
case (M 65, K 896, N 3) one axis moves at a time over the sizes at which the chain kernel can go wrong: a row tail against a workgroup
edge, every compiled row count and a second (partial) row tile, and K around the slab boundaries read from the kernel's own plan (a
short slab, the carried sum, the second buffer, the buffer's reuse)."""
import numpy as np
import pytest

import q41_cases as qc

pytestmark = pytest.mark.gpu
B = qc.BASE


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check(L, w, x, resid=None, paths=("chain", "lane")):
    """every path = the yardstick; returns it"""
    M = w.shape[0]
    want = qc.yardstick(w, x, resid)
    for path in paths:
        y, taken = L.op_mul_mat_q4_1(w, x, resid=resid, path=path)
        assert taken == path
        bad = np.argwhere(y.view(np.uint32) != want.view(np.uint32))
        assert not len(bad), f"path {path}, M {M}, K {x.shape[1]}, N {x.shape[0]}: {len(bad)} outputs differ, first (n, m) = {bad[0].tolist()}"
    return want


def test_base_case_with_and_without_resid_and_a_strided_y(L):
    w, x = qc.base_inputs()
    M, N = B["M"], B["N"]
    resid = qc.make_resid(N, M, seed=4110)
    for r in (None, resid):
        want = check(L, w, x, r)
        init = np.full((N, M + 3), np.float32(np.nan))
        init.view(np.uint32)[:, M:] = 0x7FC0BEEF                     # a bit pattern no kernel writes
        for path in ("chain", "lane"):
            y, _ = L.op_mul_mat_q4_1(w, x, resid=r, path=path, y_stride=M + 3, y_init=init)
            assert same(y[:, :M], want), path
            assert (y.view(np.uint32)[:, M:] == 0x7FC0BEEF).all(), f"path {path}: the spare columns of y were written"


def _ms(L):
    r = L.q41_plan(B["M"], B["K"], B["N"])["rows_per_workgroup"]
    return sorted({1, 15, 17, 64, 200, r - 1, r + 1})


def test_weight_rows_against_the_workgroup_edge(L):
    for M in _ms(L):
        check(L, qc.make_weights(M, B["K"], seed=4200 + M), qc.make_x(B["N"], B["K"], seed=4102))


@pytest.mark.parametrize("N", [1, 2, 8, 15, 16, 17, 33])
def test_activation_rows_at_every_tile_edge(L, N):
    w, _ = qc.base_inputs()
    check(L, w, qc.make_x(N, B["K"], seed=4300 + N), qc.make_resid(N, B["M"], seed=4400 + N) if N in (8, 17) else None)


def test_k_at_the_slab_boundaries(L):
    ks = {32, 64, 320, 1376}
    S =2 * L.q41_plan(B["M"], B["K"], B["N"])["slab_pairs"]          # the slab length in elements at the base shape
    ks |= {S - 32, S, S + 32, 2 * S + 32}
    for K in sorted(k for k in ks if k >= 32):
        check(L, qc.make_weights(B["M"], K, seed=4500 + K), qc.make_x(B["N"], K, seed=4600 + K))


@pytest.mark.parametrize("M,K,N,with_resid", [(17, 4096, 1, False), (17, 11008, 2, False), (200, 1376, 17, True)])
def test_corners(L, M, K, N, with_resid):
    check(L, qc.make_weights(M, K, seed=4700 + N), qc.make_x(N, K, seed=4800 + N), qc.make_resid(N, M, seed=4900 + N) if with_resid else None)


@pytest.mark.parametrize("regime", qc.REGIMES)
def test_value_regimes(L, regime):
    w, x = qc.regime_inputs(regime)
    want = check(L, w, x)
    assert np.isfinite(want).all()


def test_path_reporting_and_counters(L):
    w, x = qc.base_inputs()
    before = L.q41_paths()
    y_auto, taken = L.op_mul_mat_q4_1(w, x)
    assert taken == "chain"                                          # AUTO runs what a model handle runs
    mid = L.q41_paths()
    assert mid["chain"] == before["chain"] + 1 and mid["lane"] == before["lane"]
    y_lane, taken = L.op_mul_mat_q4_1(w, x, path="lane")
    assert taken == "lane"
    after = L.q41_paths()
    assert after["lane"] == mid["lane"] + 1 and after["chain"] == mid["chain"]
    assert same(y_auto, y_lane)
    assert list(L.dense_paths()) == ["mv", "mm", "set"]              # (the f16 / f32 counters keep their shape)
