"""GPU (-m gpu): k_pick_dfa and k_mask_rows_dfa through llamahip_op_pick_dfa / llamahip_op_mask_rows_dfa against tests/dfa_ref.py, exactly
(token ids, state words, bit patterns).  Rows 1 / 2 / 16; n_vocab 1, 299 (odd: table rows 2 bytes off a dword), 1023 / 1024 / 1025 (the
workgroup's width), 32 000, 32 768 / 32 769 (the 32 x 1024 stride of a thread's loads in flight); tables of 1, 2 and 300 states with the rows
in different states.  Regimes per row: the global argmax banned (what tells the kernel from k_argmax), one allowed entry at index 0 and at
n_vocab - 1, a tie of two allowed entries, a tie whose lower index is banned, +0.0 / -0.0, a NaN on the allowed maximum, every allowed entry
NaN, only -inf allowed, +inf banned.  Safety: a row with nothing allowed and state words out of range pick the fallback token, set dead, keep
the state and leave every other word as it was; result buffers pre-filled with NaN words are overwritten entry by entry."""
import numpy as np
import pytest

import dfa_ref

pytestmark = pytest.mark.gpu

BANNED = dfa_ref.BANNED
VOCABS = (1, 299, 1023, 1024, 1025, 32000, 32768, 32769)
NAN, INF = np.float32("nan"), np.float32("inf")
REGIMES = ("argmax_banned", "only_first", "only_last", "tie", "tie_lower_banned", "signed_zero", "nan_on_max", "all_nan", "only_ninf", "inf_banned")


APPLIED = {}          # (n_vocab, regime) -> rows that really carried the regime


def make_table(rng, S, V):
    t = rng.integers(0, S, size=(S, V)).astype(np.uint16)
    t[rng.random((S, V)) < 0.7] = BANNED
    for s in range(S):                       # (every row allows something: the empty row is a safety case of its own)
        if (t[s] == BANNED).all():
            t[s, int(rng.integers(0, V))] = rng.integers(0, S)
    return t


def make_row(rng, regime, trow, own_row):
    """-> logits for a row in a state whose table row is trow (modified in place where the regime is about the table and the row is this
    logits row's alone)"""
    V = trow.size
    x = rng.standard_normal(V).astype(np.float32)
    if regime in ("only_first", "only_last") and own_row:
        keep = 0 if regime == "only_first" else V - 1
        q = trow[keep] if trow[keep] != BANNED else 0
        trow[:] = BANNED
        trow[keep] = q
        x[rng.integers(0, V)] = 50.0
        return x, True
    allowed, banned = np.flatnonzero(trow != BANNED), np.flatnonzero(trow == BANNED)
    applied = True
    if regime == "argmax_banned" and banned.size:
        x[banned[rng.integers(0, banned.size)]] = 100.0
    elif regime == "tie" and allowed.size >= 2:
        x[rng.choice(allowed, 2, replace=False)] = 9.0
    elif regime == "tie_lower_banned" and banned.size and allowed.size and banned[0] < allowed[-1]:
        x[banned[0]] = 9.0
        x[allowed[-1]] = 9.0
    elif regime in ("argmax_banned", "tie", "tie_lower_banned", "only_first", "only_last"):
        applied = False                      # the row cannot carry the regime (no banned entry, one allowed entry, a shared table row): a plain row
    elif regime == "signed_zero":
        x[:] = -0.0
        x[allowed[-1]] = 0.0                 # +0.0 == -0.0: the lowest allowed index wins, not the +0.0
        x[banned] = 1.0
    elif regime == "nan_on_max":
        x[allowed[np.argmax(x[allowed])]] = NAN
    elif regime == "all_nan":
        x[allowed] = NAN
    elif regime == "only_ninf":
        x[allowed] = -INF
    elif regime == "inf_banned":
        x[banned] = INF
        applied = banned.size > 0
    return x, applied


def case(rng, R, S, V, regimes):
    table = make_table(rng, S, V)
    states = rng.permutation(S)[:R] if S >= R else rng.integers(0, S, R)
    uniq = {int(s): int((states == s).sum()) == 1 for s in states}
    rows = [make_row(rng, regimes[r % len(regimes)], table[states[r]], uniq[int(states[r])]) for r in range(R)]
    for r, (_, applied) in enumerate(rows):
        APPLIED[(V, regimes[r % len(regimes)])] = APPLIED.get((V, regimes[r % len(regimes)]), 0) + int(applied)
    return np.stack([x for x, _ in rows]), table, states.astype(np.int32)


def check(L, logits, table, states, fallback):
    R, V = logits.shape
    want = dfa_ref.pick_rows(table, states, logits, fallback)
    sent = np.where(want[2] == 1, 1, 5).astype(np.int32)       # a live row's dead word must come back as it went up
    got = L.op_pick_dfa(logits, table, states, fallback, picks=np.full(R, -1, np.int32), dead=np.where(want[2] == 1, 0, 5))
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2].tolist() == sent.tolist(), (R, table.shape[0], V)
    in_range = (states >= 0) & (states < table.shape[0])
    nanw = np.full((R, V), np.nan, np.float32)
    nanw.view(np.uint32)[:] = 0xFFFFFFFF
    masked = L.op_mask_rows_dfa(logits[in_range], table, states[in_range], out=nanw[in_range])
    assert masked.tobytes() == np.stack([dfa_ref.mask(table[s], x) for s, x in zip(states[in_range], logits[in_range])]).tobytes()
    return want


@pytest.mark.parametrize("V", VOCABS)
def test_pick_and_mask_against_the_reference(L, V):
    rng = np.random.default_rng(100 + V)
    n_banned_argmax = 0
    for R, S in ((1, 1), (2, 2), (16, 300), (16, 1), (2, 300), (16, 2)):
        # R rows take R regimes per call: enough calls for every regime to meet every row count
        for k in range(0, len(REGIMES), R):
            regimes = REGIMES[k:] + REGIMES[:k]
            logits, table, states = case(rng, R, S, V, regimes)
            want = check(L, logits, table, states, fallback=V - 1)
            assert (want[2] == 0).all()
            n_banned_argmax += sum(int(np.nanargmax(np.where(np.isnan(x), -INF, x)) != p) for x, p in zip(logits, want[0]))
    assert V == 1 or n_banned_argmax >= 5          # the constraint decided picks: k_argmax would have answered otherwise
    # every regime was really applied at this n_vocab, several times -- but for what one entry cannot carry (a banned entry, two allowed ones)
    vacuous = ("argmax_banned", "tie", "tie_lower_banned", "inf_banned") if V == 1 else ()
    for regime in REGIMES:
        assert APPLIED.get((V, regime), 0) >= (0 if regime in vacuous else 3), (V, regime, APPLIED.get((V, regime), 0))


@pytest.mark.parametrize("V", (1, 299, 1025, 32769))
def test_dead_rows_pick_the_fallback_and_write_nothing_else(L, V):
    rng = np.random.default_rng(7 + V)
    R, S = 16, 300
    logits, table, states = case(rng, R, S, V, ("argmax_banned",))
    table[states[3]] = BANNED                       # a row with nothing allowed (no table of llamahip_constraint_new has a reachable one)
    states[5], states[6], states[9], states[15] = -1, S, 0x7FFFFFFF, -0x80000000      # state words out of range: nothing is indexed
    for fallback in (0, V - 1):
        want = check(L, logits, table, states.copy(), fallback)
        assert np.flatnonzero(want[2]).tolist() == [3, 5, 6, 9, 15] and (want[0][[3, 5, 6, 9, 15]] == fallback).all()
        assert want[1][[5, 6, 9, 15]].tolist() == [-1, S, 0x7FFFFFFF, -0x80000000] and want[1][3] == states[3]
    # logits that are NaN words throughout: every live row picks its lowest allowed index
    nanw = np.empty((R, V), np.float32)
    nanw.view(np.uint32)[:] = 0xFFFFFFFF
    want = check(L, nanw, table, states.copy(), 0)
    live = np.flatnonzero(want[2] == 0)
    assert [int(want[0][r]) for r in live] == [int(np.flatnonzero(table[states[r]] != BANNED)[0]) for r in live]
