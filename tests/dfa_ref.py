"""The constrained-decoding contract of include/llamahip.h in plain Python / numpy: the lift of a byte automaton to a vocabulary, the
prune, the trie of a set of choices, the pick rule, the mask.  tests/test_constrain_host.py holds the C library to it, the GPU tests hold the
kernels to it."""
import numpy as np

BANNED = 0xFFFF


def lift(vocab, trans, accept, start, stop_token):
    """-> uint16 [n_states + 1, n_vocab], or None where the start state is not live.  Written token by token, state by state, as the header
    states it -- no sharing with the library's loops."""
    trans = np.asarray(trans, np.int64)
    S, V, DONE = trans.shape[0], len(vocab), trans.shape[0]
    nxt = [[BANNED] * V for _ in range(S + 1)]
    for s in range(S):
        for t, text in enumerate(vocab):
            if t == stop_token:
                if accept[s]:
                    nxt[s][t] = DONE
                continue
            if len(text) == 0:
                continue
            q = s
            for b in text:
                q = int(trans[q, b])
                if q < 0:
                    break
            if q >= 0:
                nxt[s][t] = q
    nxt[DONE][stop_token] = DONE
    # live: the least fixed point, by plain iteration
    live = [bool(accept[s]) for s in range(S)] + [True]
    changed = True
    while changed:
        changed = False
        for s in range(S):
            if not live[s] and any(q != BANNED and live[q] for q in nxt[s]):
                live[s] = changed = True
    if not live[start]:
        return None
    for s in range(S):
        for t in range(V):
            if nxt[s][t] != BANNED and not live[nxt[s][t]]:
                nxt[s][t] = BANNED
    return np.array(nxt, np.uint16)


def trie(strings):
    """the byte automaton of a set of byte strings: (trans, accept, start = 0), states numbered in order of first use"""
    rows, accept = [[-1] * 256], [0]
    for s in strings:
        q = 0
        for b in s:
            if rows[q][b] < 0:
                rows[q][b] = len(rows)
                rows.append([-1] * 256)
                accept.append(0)
            q = rows[q][b]
        accept[q] = 1
    return np.array(rows, np.int32), np.array(accept, np.uint8), 0


def pick(row, logits):
    """the pick rule on one table row: the largest allowed value, the lowest index on ties (+0.0 == -0.0), a NaN never wins; every allowed
    entry a NaN: the lowest allowed index; nothing allowed: -1"""
    allowed = np.flatnonzero(np.asarray(row) != BANNED)
    if allowed.size == 0:
        return -1
    v = np.asarray(logits, np.float32)[allowed]
    ok = ~np.isnan(v)
    if not ok.any():
        return int(allowed[0])
    best = v[ok].max()
    return int(allowed[ok][np.flatnonzero(v[ok] == best)[0]])


def mask(row, logits):
    out = np.array(logits, np.float32)
    out[np.asarray(row) == BANNED] = -np.inf
    return out


def pick_rows(table, states, logits2d, fallback):
    """k_pick_dfa's results for rows under one table: (picks, next states, dead)"""
    table = np.asarray(table)
    picks, nxt, dead = [], [], []
    for st, lg in zip(states, logits2d):
        p = pick(table[st], lg) if 0 <= st < table.shape[0] else -1
        if p < 0:
            picks.append(fallback), nxt.append(int(st)), dead.append(1)
        else:
            picks.append(p), nxt.append(int(table[st][p])), dead.append(0)
    return np.array(picks, np.int32), np.array(nxt, np.int32), np.array(dead, np.int32)


def decode(table, tokens, vocab):
    return b"".join(vocab[t] for t in tokens)
