"""GPU (-m gpu): the sampler's device selection (k_topk_keys* / k_topk_select* / k_topk_spill) at the inputs where a selection goes wrong:
signed zeros, ties placed at the cut, ties made and unmade by the repeat penalty, infinities, NaN, the 768-survivor cap, vocabularies from 1
to 32768 and odd windows (tests/topk_ref.py; tests/test_topk_cases_host.py shows on the CPU that the inputs are what they claim).

Each of llamahip_op_topk, _rows, _slide and _slide_set is compared directly with the float64 reference, none with another entry point.  Per
row -- safety, always: exact = 1 implies the row is not ambiguous, the ids are the reference's and the scores are the reference's bit for
bit; liveness: a `must_be_exact` row is reported exact, a `must_be_inexact` row inexact, an `either` row (a tie just below the cut, which
the kernel may flag) only has to be safe."""
import numpy as np
import pytest

import topk_ref as T

pytestmark = pytest.mark.gpu
CASES = T.all_cases()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _check_row(tag, c, window, exact, sc, ids):
    flag = T.expected_flag(c.logits, window, c.k, c.penalty, c.temp)
    assert flag == c.expected_flag, f"{tag}: the row is no longer what it was built to be"
    T.check(tag, c.logits, window, c.k, c.penalty, c.temp, flag, bool(exact), sc, ids)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_every_entry_point_on_one_row(L, c):
    kw = dict(repeat_penalty=c.penalty, top_k=c.k, temp=c.temp)
    row, n = c.logits.reshape(1, -1), c.window.size
    exact, sc, ids = L.op_topk(c.logits, c.window, **kw)
    _check_row("op_topk", c, c.window, exact, sc, ids)
    exact, sc, ids, spill = L.op_topk_rows(row, [c.window], want_spill=True, **kw)
    _check_row("op_topk_rows", c, c.window, exact[0], sc[0], ids[0])
    assert np.isnan(spill[0]).all() if exact[0] else _same(spill[0], c.logits), "op_topk_rows: the spill"
    exact, sc, ids = L.op_topk_slide(row, c.window, n, **kw)
    _check_row("op_topk_slide", c, c.window, exact[0], sc[0], ids[0])
    exact, sc, ids = L.op_topk_slide_set(row, c.window, [0, 1], [0], [n], **kw)
    _check_row("op_topk_slide_set", c, c.window, exact[0], sc[0], ids[0])


# ------------------------------------------------------------------------------------------------ 16 rows of mixed kinds in one call
@pytest.fixture(scope="module")
def mixed():
    rows = T.mixed_rows()
    return rows, np.stack([r.logits for r in rows]), dict(repeat_penalty=rows[0].penalty, top_k=rows[0].k, temp=rows[0].temp)


def _flags_seen(exact, rows):
    """the call really held rows of both kinds"""
    want = [r.expected_flag for r in rows]
    assert [bool(e) for e, w in zip(exact, want) if w != T.EITHER_FLAG] == [w == T.MUST_BE_EXACT for w in want if w != T.EITHER_FLAG]


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_rows_of_mixed_kinds_do_not_disturb_each_other(L, mixed, order):
    """every row equals its own single-row reference, whichever rows lie next to it; exactly the rows reported inexact are spilled"""
    rows, lg, kw = mixed
    idx = list(range(16)) if order == "forward" else list(range(15, -1, -1))
    rows, lg = [rows[i] for i in idx], lg[idx]
    exact, sc, ids, spill = L.op_topk_rows(lg, [r.window for r in rows], want_spill=True, **kw)
    for r, c in enumerate(rows):
        _check_row(f"op_topk_rows row {r} ({c.name})", c, c.window, exact[r], sc[r], ids[r])
        assert np.isnan(spill[r]).all() if exact[r] else _same(spill[r], c.logits), f"row {r} ({c.name}): the spill"
    _flags_seen(exact, rows)
    # one id stream: row r's window is ids[r : r + n_last]
    rng = np.random.default_rng(21)
    for n_last in (0, 5, 1024):
        stream = T.quiet_ids(rng, n_last + 15)
        exact, sc, ids = L.op_topk_slide(lg, stream, n_last, **kw)
        for r, c in enumerate(rows):
            _check_row(f"op_topk_slide n_last {n_last} row {r} ({c.name})", c, stream[r:r + n_last], exact[r], sc[r], ids[r])
        _flags_seen(exact, rows)


def test_rows_window_of_1025_ids(L, mixed):
    """op_topk_rows: n_last of 1025 on one row -- that row is inexact and spilled, its neighbours are their own reference"""
    rows, lg, kw = mixed
    rng = np.random.default_rng(22)
    wins = [r.window for r in rows]
    wins[9] = T.quiet_ids(rng, 1025)
    exact, sc, ids, spill = L.op_topk_rows(lg, wins, want_spill=True, **kw)
    assert rows[9].expected_flag == T.MUST_BE_EXACT and not exact[9] and _same(spill[9], lg[9])
    for r, c in enumerate(rows):
        if r != 9:
            _check_row(f"row {r} ({c.name})", c, wins[r], exact[r], sc[r], ids[r])
            assert np.isnan(spill[r]).all() if exact[r] else _same(spill[r], c.logits), f"row {r}: the spill"


def test_slide_a_token_entering_and_leaving_the_window_changes_the_status(L):
    """temp 1, penalty 2, windows of 2 ids: while id A (logit 2.0) is in the window it ties with id B (1.0) -- rows 1, 2, 5 and 6; once it has
    left they differ again; C and D (both 0.5, below the cut for top_k = 1) never matter"""
    V, A, B = 2048, 1024 + 17, 600
    lg = T.low(V)
    lg[A], lg[B], lg[40], lg[41] = 2.0, 1.0, 0.5, 0.5
    X, Y = 900, 901
    stream = np.array([X, Y, A, X, Y, X, A, Y, X], np.int32)            # windows: XY YA AX XY YX XA AY YX
    want = [T.MUST_BE_EXACT, T.MUST_BE_INEXACT, T.MUST_BE_INEXACT, T.MUST_BE_EXACT, T.MUST_BE_EXACT, T.MUST_BE_INEXACT, T.MUST_BE_INEXACT, T.MUST_BE_EXACT]
    rows = np.tile(lg, (8, 1))
    for k, flags in ((1, want), (2, [T.EITHER_FLAG if f == T.MUST_BE_EXACT else f for f in want])):     # (top_k = 2: C == D sits just below the cut)
        assert [T.expected_flag(lg, stream[r:r + 2], k, 2.0, 1.0) for r in range(8)] == flags
        exact, sc, ids = L.op_topk_slide(rows, stream, 2, repeat_penalty=2.0, top_k=k, temp=1.0)
        for r in range(8):
            T.check(f"k {k} row {r}", lg, stream[r:r + 2], k, 2.0, 1.0, flags[r], bool(exact[r]), sc[r], ids[r])
    # and the other way round: equal logits at A and B tie until one of them enters the window
    lg[B] = 2.0
    want = [T.MUST_BE_EXACT if f == T.MUST_BE_INEXACT else T.MUST_BE_INEXACT for f in want]
    rows = np.tile(lg, (8, 1))
    assert [T.expected_flag(lg, stream[r:r + 2], 1, 2.0, 1.0) for r in range(8)] == want
    exact, sc, ids = L.op_topk_slide(rows, stream, 2, repeat_penalty=2.0, top_k=1, temp=1.0)
    for r in range(8):
        T.check(f"equal logits, row {r}", lg, stream[r:r + 2], 1, 2.0, 1.0, want[r], bool(exact[r]), sc[r], ids[r])


@pytest.mark.parametrize("n_last", [(0, 3, 64), (64, 1025, 3), (1024, 1, 1100)])
def test_slide_set_segments_of_1_2_and_13_rows(L, mixed, n_last):
    """segments with different window lengths whose id ranges overlap in the pool; a segment with more than 1024 ids is inexact and its
    neighbours are unaffected"""
    rows, lg, kw = mixed
    rng = np.random.default_rng(23)
    pool = T.quiet_ids(rng, 1200)
    seg_begin, off = [0, 1, 3, 16], [40, 0, 30]                         # [40, ..), [0, ..), [30, ..): they overlap
    exact, sc, ids = L.op_topk_slide_set(lg, pool, seg_begin, off, list(n_last), **kw)
    for s in range(3):
        for j, r in enumerate(range(seg_begin[s], seg_begin[s + 1])):
            c = rows[r]
            if n_last[s] > 1024:
                assert not exact[r], f"segment {s} row {r}: a window of {n_last[s]} ids"
            else:
                _check_row(f"segment {s} row {r} ({c.name})", c, pool[off[s] + j:off[s] + j + n_last[s]], exact[r], sc[r], ids[r])
    assert exact.any() and not exact.all()
