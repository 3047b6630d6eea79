"""GPU (-m gpu): llamahip_op_sched_accept -- k_verify_rows + k_sched_accept, the device half of a scheduler step that carries drafted
tokens -- alone, against numpy.

Hand-made logits rows (n_vocab 1500 and 33) whose picks are known by construction, and the rule restated in Python: per segment n_accept =
the largest a <= N - 1 with pick[b + j] == token[b + j + 1] for all j < a; with slot words position = base + rows consumed, cursor = base
cursor + tokens produced, next-token word = pick[n_accept], trace entries pick[0 .. n_accept] at the base cursor; everything else keeps a
sentinel.  Segments of 1, 2 and 16 rows; accept none / a proper prefix / all; a mismatch followed by later matches; non-emitting segments
between emitting ones; ties, +0 / -0, a row of NaN."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENT = -777
N_SLOTS, LOG_CAP = 9, 20


def pick_ref(row):
    """the largest value, the lowest index on ties (-0 == +0); a NaN is never taken; nothing taken: 0"""
    ok = ~np.isnan(row)
    if not ok.any():
        return 0
    m = row[ok].max()
    return int(np.flatnonzero(ok & (row == m))[0])


def accept_ref(lg, tab, toks, words=None):
    picks = [pick_ref(r) for r in lg]
    n_acc = []
    for emit, slot, pos, cur, b, rows in tab:
        N = rows if emit == 2 else 1 if emit == 1 else 0
        a = 0
        while N > 1 and a < N - 1 and picks[b + a] == toks[b + a + 1]:
            a += 1
        n_acc.append(a)
        if words is None:
            continue
        state, log, nxt = words
        made = a + 1 if N > 0 else 0
        for j in range(made):
            if cur + j < log.shape[1]:
                log[slot, cur + j] = picks[b + j]
        if N > 0:
            nxt[slot] = picks[b + a]
        state[slot] = [pos + (a + 1 if emit == 2 else rows), cur + made]
    return n_acc, picks


def rows_with_picks(V, want, seed):
    """finite random rows whose greedy pick is want[r]"""
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((len(want), V)).astype(np.float32)
    for r, w in enumerate(want):
        lg[r, w] = 9.0 + r
    return lg


def run_both_ways(L, lg, tab, toks, note):
    """without slot words, then with them on sentinel-filled arrays: the result and every word against the restated rule"""
    tab = np.asarray(tab, np.int32)
    toks = np.asarray(toks, np.int32)
    want_acc, want_picks = accept_ref(lg, tab.tolist(), toks.tolist())
    n_acc, picks = L.op_sched_accept(lg, tab, toks)
    assert n_acc.tolist() == want_acc and picks.tolist() == want_picks, (note, n_acc, want_acc, picks, want_picks)
    state = np.full((N_SLOTS, 2), SENT, np.int32)
    log = np.full((N_SLOTS, LOG_CAP), SENT, np.int32)
    nxt = np.full(N_SLOTS, SENT, np.int32)
    ws = (state.copy(), log.copy(), nxt.copy())
    accept_ref(lg, tab.tolist(), toks.tolist(), ws)
    n_acc, picks = L.op_sched_accept(lg, tab, toks, state, log, nxt)
    assert n_acc.tolist() == want_acc and picks.tolist() == want_picks, (note, "with words")
    assert np.array_equal(state, ws[0]), (note, "position / cursor", state.tolist(), ws[0].tolist())
    assert np.array_equal(nxt, ws[2]), (note, "next-token words", nxt.tolist(), ws[2].tolist())
    assert np.array_equal(log, ws[1]), (note, "trace", log.tolist(), ws[1].tolist())
    return want_acc, want_picks, ws


@pytest.mark.parametrize("V", [1500, 33])
def test_the_segments_of_a_mixed_step(L, V):
    """sixteen logits rows in seven segments: 2 rows all accepted | a piece that does not emit | a piece that ends its prompt | 3 rows, a
    proper prefix | a piece that does not emit | 9 rows, a mismatch at its row 2 and matches behind it that must not count | one decode row"""
    toks, want = [0] * 16, [0] * 16
    toks[0:2], want[0:2] = [5, 11], [11, 12]                    # draft [11]: row 0 picks 11, row 1 the bonus token
    toks[2], want[2] = 3, 30                                    # the last row of a 7-row piece
    toks[3:6], want[3:6] = [6, 7, 8], [7, 9, 10]                # draft [7, 8]: row 3 picks 7, row 4 picks 9, not 8
    toks[6:15] = [20, 1, 2, 3, 4, 5, 6, 7, 8]                   # draft [1 .. 8]: rows 6, 7 agree, row 8 does not, rows 9 .. 13 agree again
    want[6:15] = [1, 2, 31, 4, 5, 6, 7, 8, 32]
    toks[15], want[15] = 4, 0
    lg = rows_with_picks(V, want, seed=V)
    #       emit slot pos cursor row0 rows
    tab = [[2, 4, 50, 3, 0, 2], [0, 1, 18, 0, 0, 5], [1, 0, 9, 0, 2, 7], [2, 5, 100, 17, 3, 3], [0, 2, 0, 0, 0, 1], [2, 3, 31, 18, 6, 9], [1, 7, 77, 6, 15, 1]]
    n_acc, picks, (state, log, nxt) = run_both_ways(L, lg, tab, toks, V)
    assert n_acc == [1, 0, 0, 1, 0, 2, 0] and picks == want
    # spelled out once, independent of accept_ref
    assert state.tolist() == [[16, 1], [23, 0], [1, 0], [34, 21], [52, 5], [102, 19], [SENT, SENT], [78, 7], [SENT, SENT]]
    assert nxt.tolist() == [30, SENT, SENT, 31, 12, 9, SENT, 0, SENT]
    assert log[4].tolist() == [SENT] * 3 + [11, 12] + [SENT] * 15 and log[0].tolist() == [30] + [SENT] * 19
    assert log[5].tolist() == [SENT] * 17 + [7, 9, SENT]
    assert log[3].tolist() == [SENT] * 18 + [1, 2]          # the third entry would lie at log_cap: dropped
    assert log[7].tolist() == [SENT] * 6 + [0] + [SENT] * 13
    for s in (1, 2, 6, 8):
        assert (log[s] == SENT).all()


@pytest.mark.parametrize("V", [1500, 33])
def test_one_segment_of_sixteen_rows_at_ties_signed_zeros_and_nan(L, V):
    """all fifteen draft tokens accepted through a row of NaN (pick 0), a tie (lowest index), +0 against -0 (equal: lowest index), a row of
    -inf (pick 0) and a NaN above the largest value; then the same rows with ONE draft token changed: none, a proper prefix"""
    want = [3, 4, 5, 0, 6, 7, 8, 9, 0, 10, 0, 12, 13, 14, 15, 16]
    lg = rows_with_picks(V, want, seed=100 + V)
    lg[3, :] = np.nan
    lg[5, 7] = lg[5, 20] = lg[5, 32] = 50.0                    # a tie: the lowest index
    lg[8, :] = -0.0
    lg[8, 9] = 0.0                                             # +0 at 9 is not larger than -0 at 0
    lg[10, :] = -np.inf
    lg[11, 2] = np.nan                                         # never taken, below or above the pick's index
    lg[11, 30] = np.nan
    assert [pick_ref(r) for r in lg] == want
    toks = [1] + want[:15]                                     # the draft is exactly what the rows pick
    n_acc, picks, (state, log, nxt) = run_both_ways(L, lg, [[2, 6, 3, 2, 0, 16]], toks, (V, "all"))
    assert n_acc == [15] and picks == want
    assert state[6].tolist() == [19, 18] and nxt[6] == 16 and log[6].tolist() == [SENT, SENT] + want + [SENT, SENT]
    for k, acc in ((1, 0), (4, 3), (9, 8), (15, 14)):          # draft token k - 1 is not row k - 1's pick
        t = list(toks)
        t[k] = (t[k] + 1) % V
        n_acc, _, (state, _, nxt) = run_both_ways(L, lg, [[2, 6, 3, 2, 0, 16]], t, (V, k))
        assert n_acc == [acc] and state[6].tolist() == [3 + acc + 1, 2 + acc + 1] and nxt[6] == want[acc]


def test_segments_of_one_and_two_rows(L):
    V = 33
    lg = rows_with_picks(V, [7, 8, 9, 10], seed=5)
    for emit in (1, 2):
        n_acc, picks, _ = run_both_ways(L, lg[:1], [[emit, 2, 40, 0, 0, 1]], [3], ("one row", emit))
        assert n_acc == [0] and picks == [7]
    assert run_both_ways(L, lg[:2], [[2, 0, 5, 1, 0, 2]], [3, 7], "two rows, accepted")[0] == [1]
    assert run_both_ways(L, lg[:2], [[2, 0, 5, 1, 0, 2]], [3, 6], "two rows, rejected")[0] == [0]
    # sixteen one-row segments, emitting and not, in one step
    lg16 = rows_with_picks(V, list(range(16)), seed=6)
    tab, b = [], 0
    for s in range(16):
        emit = 0 if s % 5 == 2 else 1 + s % 2
        tab.append([emit, s % N_SLOTS if s < N_SLOTS else 0, s, s % 3, b if emit else 0, 1])
        b += emit > 0
    for s in range(N_SLOTS, 16):          # (one segment per slot: the later segments go without words)
        tab[s][1] = -1
    n_acc, picks = L.op_sched_accept(lg16[:b], np.asarray(tab, np.int32), np.zeros(b, np.int32))
    assert n_acc.tolist() == [0] * 16 and picks.tolist() == list(range(b))
    run_both_ways(L, lg16[:6], tab[:8], [0] * 6, "eight one-row segments")


def test_refusals_name_their_limit_and_launch_nothing(L):
    V = 33
    lg = np.zeros((17, V), np.float32)
    ok = [[2, 0, 0, 0, 0, 2]]

    def refused(word, lg_, tab, toks, **kw):
        with pytest.raises(L.LlamaHipError) as e:
            L.op_sched_accept(lg_, np.asarray(tab, np.int32), toks, **kw)
        assert e.value.code == L.binding.ERR_PREDICT and "llamahip_op_sched_accept" in e.value.message and word in e.value.message, e.value.message

    refused("n_rows must be 1 .. 16", lg, [[2, 0, 0, 0, 0, 17]], [0] * 17)
    refused("n_segs must be 1 .. 16", lg[:2], [[0, 0, 0, 0, 0, 1]] * 16 + ok, [0, 0])
    refused("emit 3 outside 0 .. 2", lg[:2], [[3, 0, 0, 0, 0, 2]], [0, 0])
    refused("row count 0", lg[:2], [[1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 1, 1]], [0, 0])
    refused("row count 17", lg[:2], [[2, 0, 0, 0, 0, 17]], [0, 0])
    refused("must tile [0, n_rows = 2)", lg[:2], [[1, 0, 0, 0, 1, 1], [1, 1, 0, 0, 0, 1]], [0, 0])
    refused("must tile [0, n_rows = 2)", lg[:2], [[2, 0, 0, 0, 0, 3]], [0, 0])
    refused("name 1 logits rows, n_rows is 2", lg[:2], [[1, 0, 0, 0, 0, 4]], [0, 0])
    refused("base position -1", lg[:2], [[2, 0, -1, 0, 0, 2]], [0, 0])
    st, lo, nx = np.zeros((2, 2), np.int32), np.zeros((2, 4), np.int32), np.zeros(2, np.int32)
    refused("slot 2 out of range [0, n_slots = 2)", lg[:2], [[2, 2, 0, 0, 0, 2]], [0, 0], state=st, log=lo, next_tok=nx)
    refused("slot 1 has two segments", lg[:2], [[1, 1, 0, 0, 0, 1], [1, 1, 0, 0, 1, 1]], [0, 0], state=st, log=lo, next_tok=nx)
    refused("all three or not at all", lg[:2], ok, [0, 0], state=st)
    assert (st == 0).all() and (lo == 0).all() and (nx == 0).all()
    err = L.binding.C.create_string_buffer(256)
    assert L.lib().llamahip_op_sched_accept(None, 1, 8, None, 1, None, 0, 0, None, None, None, None, None, err, len(err)) == L.binding.ERR_PREDICT
