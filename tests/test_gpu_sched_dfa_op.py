"""GPU (-m gpu): k_verify_rows_dfa and k_sched_pick_dfa -- the scheduler's two pick kernels with a per-row allow-list -- on caller-supplied
rows (llamahip_op_verify_rows_allow / llamahip_op_sched_pick_allow), bit for bit against tests/dfa_ref.py's pick.  The cases are
tests/sched_dfa_ref.py's (tests/test_sched_constrain_host.py holds them to their conditions on the CPU): the maximum banned, ties among allowed
entries and across a banned one, +0.0 against -0.0, a NaN among the allowed entries, every allowed entry a NaN, one entry allowed at index 0
and at n_vocab - 1, nothing allowed (fallback + dead, the other rows untouched), unconstrained rows (state -1: op_verify_rows' and
op_sched_pick's picks on the same logits), mixed in one launch of 1, 5 and 16 rows.  n_vocab 1, 63 .. 65, 299 (an odd table-row stride),
2047 .. 2049 (the wave kernel's second trip through its 32-deep load loop), 32767 .. 32769 (the workgroup kernel's).  For k_sched_pick_dfa also
the slot words, emit 0 segments and a cursor at log_cap."""
import numpy as np
import pytest

import sched_dfa_ref as R

pytestmark = pytest.mark.gpu


def seeds(rows):
    return range(len(R.KINDS)) if rows == 1 else range(2) if rows == 5 else range(1)


@pytest.mark.parametrize("V", R.OP_VOCABS)
def test_both_kernels_pick_by_the_rule(L, V):
    kinds = set()
    for rows in R.OP_ROWS:
        for seed in seeds(rows):
            case = R.op_case(V, rows, seed)
            want_p, want_d = R.op_expected(case)
            kinds |= set(case["kinds"])
            note = (V, rows, seed, case["kinds"])
            picks, dead = L.op_verify_rows_dfa(case["logits"], case["table"], case["states"], case["fallback"])
            assert picks.tolist() == want_p.tolist() and dead.tolist() == want_d.tolist(), note
            emit = np.ones(rows, np.int32)
            picks, dead = L.op_sched_pick_dfa(case["logits"], emit, case["table"], case["states"], case["fallback"])
            assert picks.tolist() == want_p.tolist() and dead.tolist() == want_d.tolist(), note
            # the unconstrained rows: the two kernels these stand in for, on the same logits
            free = np.flatnonzero(case["states"] < 0)
            if free.size:
                _, plain = L.op_verify_rows(case["logits"], np.zeros(rows, np.int32))
                assert picks[free].tolist() == np.asarray(plain)[free].tolist() == L.op_sched_pick(case["logits"], emit)[free].tolist(), note
    assert V < 3 or kinds == set(R.KINDS)


def test_sched_pick_dfa_slot_words_emit_and_the_log_edge(L):
    V, rows, n_slots, log_cap = 299, 5, 7, 6
    case = R.op_case(V, rows, 3)          # kinds 3 .. 7: zeros, nan_among, all_nan, one_first, one_last
    case["states"][1] = -1                # ... and an unconstrained segment
    want_p, want_d = R.op_expected(case)
    emit = np.array([1, 1, 0, 1, 1], np.int32)
    # {slot, position, cursor}: a cursor at log_cap (the last entry), one past it (dropped), 0 (no entry), and two inside
    words = np.array([[4, 10, log_cap], [0, 3, log_cap + 1], [6, 20, 2], [2, 7, 0], [5, 1, 1]], np.int32)
    state = np.full((n_slots, 2), -5, np.int32)
    log = np.full((n_slots, log_cap), -6, np.int32)
    nxt = np.full(n_slots, -7, np.int32)
    want_state, want_log, want_nxt = state.copy(), log.copy(), nxt.copy()
    for r in range(rows):
        slot, pos, cur = words[r]
        want_state[slot] = (pos, cur)
        if emit[r]:
            want_nxt[slot] = want_p[r]
            if 1 <= cur <= log_cap:
                want_log[slot, cur - 1] = want_p[r]
    picks, dead = L.op_sched_pick_dfa(case["logits"], emit, case["table"], case["states"], case["fallback"], seg_words=words, state=state, log=log, next_tok=nxt)
    assert picks.tolist() == [int(p) if e else -1 for p, e in zip(want_p, emit)]
    assert dead.tolist() == [int(d) if e else 0 for d, e in zip(want_d, emit)]
    assert state.tolist() == want_state.tolist() and log.tolist() == want_log.tolist() and nxt.tolist() == want_nxt.tolist()
    # a segment that allows nothing: its fallback token in the slot's words, its dead word set, the other segments as before
    case["table"][3, :] = R.BANNED
    state2, log2, nxt2 = np.full((n_slots, 2), -5, np.int32), np.full((n_slots, log_cap), -6, np.int32), np.full(n_slots, -7, np.int32)
    words[3] = (2, 7, 3)
    p2, d2 = L.op_sched_pick_dfa(case["logits"], emit, case["table"], case["states"], case["fallback"], seg_words=words, state=state2, log=log2, next_tok=nxt2)
    fb = int(case["fallback"][3])
    assert p2.tolist() == picks.tolist()[:3] + [fb] + picks.tolist()[4:] and d2.tolist() == [0, 0, 0, 1, 0]
    assert nxt2[2] == fb and log2[2].tolist() == [-6, -6, fb, -6, -6, -6] and state2[2].tolist() == [7, 3]
