"""GPU (-m gpu): k_row_topn through llamahip_op_top_logprobs, bit for bit against the two oracles the project already has.

Per row: ids == np.argsort(-row, kind="stable")[:n] (value descending, the lower index first on equal values, +0.0 == -0.0); logprob[j] has the
bytes of op_logprob(row, target = ids[j]) (k_row_logprob: the same maximum, the same double sum in the same order); and it lies within the
project's 1e-10 (TOL of tests/test_gpu_logprobs.py) of the float64 numpy log-softmax.  A row with a NaN or a +inf: every id -1, every logprob
NaN -- and only that row.  A row's result does not depend on the rows around it."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-10      # tests/test_gpu_logprobs.py
VOCABS = (1, 2, 3, 5, 64, 255, 256, 257, 1023, 1024, 1028, 32000, 32001)
PLACES = (1, 2, 5, 32, 64)
ROWS = (1, 2, 16, 17, 65)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def flagged(rows):
    return np.isnan(rows).any(axis=1) | (rows == np.inf).any(axis=1)


def check(L, rows, n, note=""):
    """every property of the op's result on rows [R, V]; returns (ids, logprob)"""
    rows = np.ascontiguousarray(rows, np.float32)
    R, V = rows.shape
    ids, lp = L.op_top_logprobs(rows, n)
    assert ids.shape == (R, n) and lp.shape == (R, n) and ids.dtype == np.int32 and lp.dtype == np.float64
    bad = flagged(rows)
    assert np.all(ids[bad] == -1) and np.all(np.isnan(lp[bad])), (note, "flagged rows")
    good = np.flatnonzero(~bad)
    if good.size == 0:
        return ids, lp
    g = rows[good]
    want = np.stack([np.argsort(-r, kind="stable")[:n] for r in g]).astype(np.int32)
    assert np.array_equal(ids[good], want), (note, "ids")
    # k_row_logprob on every (row, place): the row repeated n times, one target each
    got_lp, am, _ = L.op_logprob(np.repeat(g, n, axis=0), ids[good].reshape(-1))
    assert same(lp[good].reshape(-1), got_lp), (note, "logprob bytes against op_logprob")
    assert np.array_equal(am.reshape(-1, n)[:, 0], ids[good][:, 0]), (note, "ids[0] is the greedy pick")
    r64 = g.astype(np.float64)
    mx = g.max(axis=1).astype(np.float64)
    lse = np.log(np.exp(r64 - mx[:, None]).sum(axis=1))
    ref = (np.take_along_axis(r64, want.astype(np.int64), axis=1) - mx[:, None]) - lse[:, None]
    fin = np.isfinite(ref)
    assert np.array_equal(np.isneginf(ref), np.isneginf(lp[good])), (note, "-inf entries")
    assert not fin.any() or np.max(np.abs(lp[good][fin] - ref[fin])) <= TOL, (note, "logprob against numpy")
    return ids, lp


def shape_pairs(V):
    """(rows, n) for a vocabulary: the full product on the small ones; on the two wide ones every row count and every n once"""
    ns = sorted({min(n, V) for n in PLACES})
    if V < 32000:
        return [(R, n) for R in ROWS for n in ns]
    return [(1, 64), (2, 5), (16, 32), (17, 1), (65, 2)]


@pytest.mark.parametrize("V", VOCABS)
def test_normal_draws_at_every_shape(L, V):
    rng = np.random.default_rng(1000 + V)
    base = (rng.standard_normal((max(ROWS), V)) * 3.0).astype(np.float32)
    for R, n in shape_pairs(V):
        check(L, base[:R], n, note=(V, R, n))


def regime_rows(name, V, n, rng):
    """three rows of a value regime (the kernel runs one workgroup per row, so each row is a case of its own)"""
    R = 3
    x = (rng.standard_normal((R, V)) * 2.0).astype(np.float32)
    k = int(rng.integers(0, 256))
    if name == "all_equal":
        x[0], x[1], x[2] = np.float32(1.25), np.float32(-7.0), np.float32(0.0)
    elif name == "plateau":
        # n // 2 entries above a plateau of equal values that straddles the n-th place: the plateau's lowest indices win the cut
        for r in range(R):
            x[r] = np.float32(-3.0) + (x[r] * np.float32(0.01)).astype(np.float32) - np.float32(1.0)
            pl = rng.choice(V, size=min(V, n + 7), replace=False)
            x[r, pl] = np.float32(0.5)
            x[r, rng.choice(V, size=min(V, max(n // 2, 1)), replace=False)] = np.float32(2.0)
    elif name == "signed_zeros":
        x[:] = np.where(rng.integers(0, 2, size=(R, V)) == 1, np.float32(0.0), np.float32(-0.0))
        x[1, rng.choice(V, size=max(V // 3, 1), replace=False)] = np.float32(-1.0)
    elif name == "few_finite":
        for r in range(R):
            keep = rng.choice(V, size=min(V, max(1, (n // 2) * (r > 0) + 1)), replace=False)
            y = np.full(V, -np.inf, np.float32)
            y[keep] = x[r, keep]
            x[r] = y
    elif name == "nan_and_inf_rows":
        x = (rng.standard_normal((5, V)) * 2.0).astype(np.float32)
        x[1, int(rng.integers(0, V))] = np.nan
        x[3, V - 1] = np.inf
    elif name == "spread_2000":
        x = (x * np.float32(400.0)).astype(np.float32)
        x[0, 0], x[0, V - 1] = np.float32(1000.0), np.float32(-1000.0)
    elif name == "ascending":
        x = np.sort(x, axis=1)
    elif name == "descending":
        x = -np.sort(-x, axis=1)
    elif name == "one_thread_owns_the_winners":
        # the n largest at indices k, k + 256, k + 512, ... (V % 4 != 0: one thread's entries) and at the float4s k, k + 256, ... (V % 4 == 0)
        for r in range(R):
            x[r] = np.minimum(x[r], np.float32(1.0))
            if V % 4:
                idx = np.arange(k % min(V, 256), V, 256)[:n]
            else:
                q = np.arange(k % min(V // 4, 256), V // 4, 256)
                idx = (4 * q[:, None] + np.arange(4)[None, :]).reshape(-1)[:n]
            x[r, idx] = np.float32(5.0) + rng.standard_normal(idx.size).astype(np.float32)
    elif name == "winners_in_the_scalar_tail":
        # ... all behind the last full float4 (V % 4 of them at the most: the rest of the places follows from the body)
        for r in range(R):
            x[r] = np.minimum(x[r], np.float32(1.0))
            t0 = V - (V % 4 or 4)
            x[r, t0:] = np.float32(6.0) + np.arange(V - t0, dtype=np.float32) * np.float32(0.5 if r else 0.0)
    elif name == "winners_in_the_last_256":
        for r in range(R):
            x[r] = np.minimum(x[r], np.float32(1.0))
            idx = V - 1 - rng.choice(min(V, 256), size=min(V, 256, n), replace=False)
            x[r, idx] = np.float32(5.0) + rng.standard_normal(idx.size).astype(np.float32)
    else:
        raise AssertionError(name)
    return x


REGIMES = ("all_equal", "plateau", "signed_zeros", "few_finite", "nan_and_inf_rows", "spread_2000", "ascending", "descending",
           "one_thread_owns_the_winners", "winners_in_the_scalar_tail", "winners_in_the_last_256")


@pytest.mark.parametrize("name", REGIMES)
def test_value_regimes(L, name):
    for V in (5, 255, 1028, 2051, 32000, 32001):
        for n in (1, 5, 64):
            n = min(n, V)
            rng = np.random.default_rng([REGIMES.index(name), V, n])
            rows = regime_rows(name, V, n, rng)
            ids, lp = check(L, rows, n, note=(name, V, n))
            if name == "nan_and_inf_rows":
                assert np.array_equal(np.flatnonzero(ids[:, 0] < 0), [1, 3]), (V, n, "only the flagged rows are flagged")


def test_a_rows_result_does_not_depend_on_its_neighbours(L):
    for V, n in ((257, 32), (32000, 64)):
        rng = np.random.default_rng(V)
        rows = (rng.standard_normal((65, V)) * 3.0).astype(np.float32)
        rows[7, 3] = np.nan
        alone = L.op_top_logprobs(rows[40:41], n)
        among = L.op_top_logprobs(rows, n)
        assert same(alone[0][0], among[0][40]) and same(alone[1][0], among[1][40])
        again = rows.copy()
        again[:40] = np.float32(1.0)
        moved = L.op_top_logprobs(np.concatenate([again[40:], again[:40]]), n)
        assert same(moved[0][0], among[0][40]) and same(moved[1][0], among[1][40])


def test_refusals_name_the_limit(L):
    x = np.zeros((2, 8), np.float32)
    ids, lp = np.zeros((2, 64), np.int32), np.zeros((2, 64), np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def call(logits, R, V, n, i, l):
        err = C.create_string_buffer(512)
        rc = L.lib().llamahip_op_top_logprobs(logits, R, V, n, i, l, err, len(err))
        return rc, err.value.decode()

    for args, text in (((p(x), 0, 8, 1, p(ids), p(lp)), "llamahip_op_top_logprobs: n_rows must be >= 1 (got 0)"),
                       ((p(x), 2, 0, 1, p(ids), p(lp)), "llamahip_op_top_logprobs: n_vocab must be >= 1 (got 0)"),
                       ((p(x), 2, 8, 0, p(ids), p(lp)), "llamahip_op_top_logprobs: n_top 0 outside 1 .. 64"),
                       ((p(x), 2, 8, -3, p(ids), p(lp)), "llamahip_op_top_logprobs: n_top -3 outside 1 .. 64"),
                       ((p(x), 2, 8, 65, p(ids), p(lp)), "llamahip_op_top_logprobs: n_top 65 outside 1 .. 64"),
                       ((p(x), 2, 8, 9, p(ids), p(lp)), "llamahip_op_top_logprobs: n_top 9 > n_vocab 8"),
                       ((None, 2, 8, 1, p(ids), p(lp)), "llamahip_op_top_logprobs: logits is NULL"),
                       ((p(x), 2, 8, 1, None, p(lp)), "llamahip_op_top_logprobs: ids_out is NULL"),
                       ((p(x), 2, 8, 1, p(ids), None), "llamahip_op_top_logprobs: logprob_out is NULL")):
        rc, msg = call(*args)
        assert rc != 0 and msg == text, (args[1:4], msg)
    with pytest.raises(L.LlamaHipError, match="n_top 9 > n_vocab 8"):
        L.op_top_logprobs(x, 9)
