"""Constrained requests in the request scheduler (include/llamahip.h) in plain Python / numpy, on top of tests/dfa_ref.py:
the forced run of a state, the contract loop of a constrained request ALONE on its slot, and the operands of the two allow-list pick
kernels' op tests (built here once, so that the CPU test can hold the cases to their own conditions before a GPU sees them)."""
import numpy as np

import dfa_ref

BANNED = dfa_ref.BANNED
TAILS = [b"yes please", b"no thanks", b"cab", b"cabbage"]          # long forced tails over the synthetic vocabulary


def forced(table, state, cap):
    """llamahip_forced_run: while the state is not DONE and allows exactly one token, that token; DONE yields nothing"""
    table = np.asarray(table)
    done, out = table.shape[0] - 1, []
    while len(out) < cap and state != done:
        allowed = np.flatnonzero(table[state] != BANNED)
        if allowed.size != 1:
            break
        out.append(int(allowed[0]))
        state = int(table[state][allowed[0]])
    return out


def satisfied_by(table, state, tokens):
    """the stream walks the automaton from `state` into DONE"""
    done = table.shape[0] - 1
    for t in tokens:
        q = int(table[state][t])
        if q == BANNED:
            return False
        state = q
        if state == done:
            return True
    return False


def alone(ref, n_layer, slot, prompt, n_predict, chunk, table, state, stop, nth=8):
    """the contract: set_seq(slot), eval_chunks(prompt), then pick -> advance -> one-token eval; cut behind the stop token (reason "stop") or at
    n_predict ("length").  -> (tokens, reason, the KV rows [0, n_prompt + n - 1) of every layer)"""
    ref.set_seq(slot)
    row = ref.eval_chunks(prompt, 0, chunk, nth) if chunk > 0 else ref.eval(prompt, 0, nth)
    out, reason = [], "length"
    while True:
        tok = dfa_ref.pick(table[state], row)
        assert tok >= 0
        state = int(table[state][tok])
        out.append(tok)
        if tok == stop:
            reason = "stop"
            break
        if len(out) >= n_predict:
            break
        row = ref.eval([tok], len(prompt) + len(out) - 1, nth)
    n = len(prompt) + len(out) - 1
    kv = [ref.kv(il, n) for il in range(n_layer)] if n > 0 else []
    ref.set_seq(0)
    return out, reason, kv


# ---- the operands of llamahip_op_verify_rows_allow / llamahip_op_sched_pick_allow -------------------------------------------------------------
KINDS = ("max_banned", "tie_allowed", "tie_across_banned", "zeros", "nan_among", "all_nan", "one_first", "one_last", "none", "free")
OP_VOCABS = (1, 63, 64, 65, 299, 2047, 2048, 2049, 32767, 32768, 32769)
OP_ROWS = (1, 5, 16)


def op_case(V, R, seed):
    """R rows over n_vocab V, row r of kind KINDS[(seed + r) % 10] where V has room for it (else one_first / none / free): the table has one state
    per row -- state r is row r's allow-list -- and one more.  -> dict(logits, table, states, fallback, kinds)"""
    rng = np.random.default_rng(1000 * V + 10 * R + seed)
    logits = rng.standard_normal((R, V)).astype(np.float32)
    table = np.full((R + 1, V), BANNED, np.uint16)
    states, kinds = np.arange(R, dtype=np.int32), []
    fallback = rng.integers(0, V, R).astype(np.int32)
    for r in range(R):
        kind = KINDS[(seed + r) % len(KINDS)]
        need = {"max_banned": 2, "tie_allowed": 2, "tie_across_banned": 3, "zeros": 2, "nan_among": 2}.get(kind, 1)
        if V < need:
            kind = ("one_first", "none", "free")[r % 3]
        allow = rng.random(V) < 0.5
        row = logits[r]
        if kind in ("max_banned", "tie_allowed", "tie_across_banned", "zeros", "nan_among", "all_nan"):
            idx = np.sort(rng.choice(V, size=min(V, 3), replace=False))          # three (or V) distinct places, ascending
            top = np.float32(9.0)
            if kind == "max_banned":
                allow[idx[0]], allow[idx[-1]] = False, True
                row[idx[0]] = top
            elif kind == "tie_allowed":
                allow[idx[0]] = allow[idx[-1]] = True
                row[idx[0]] = row[idx[-1]] = top
            elif kind == "tie_across_banned":          # the banned holder of the maximum has the lowest index
                allow[idx[0]], allow[idx[1]], allow[idx[2]] = False, True, True
                row[idx] = top
            elif kind == "zeros":          # -0.0 at the lower allowed index, +0.0 at the higher, everything else below zero
                row[:] = -np.abs(row) - np.float32(1.0)
                allow[idx[0]] = allow[idx[-1]] = True
                row[idx[0]], row[idx[-1]] = np.float32(-0.0), np.float32(0.0)
            elif kind == "nan_among":          # a NaN where the maximum would be; a finite allowed entry elsewhere
                allow[idx[0]] = allow[idx[-1]] = True
                row[idx[0]] = np.float32(np.nan)
            else:          # all_nan: every allowed entry a NaN, the banned ones finite
                allow[idx[-1]] = True
                row[allow] = np.float32(np.nan)
        elif kind == "one_first":
            allow[:] = False
            allow[0] = True
        elif kind == "one_last":
            allow[:] = False
            allow[V - 1] = True
        elif kind == "none":
            allow[:] = False
        else:          # free: the row is unconstrained (its table row is never read)
            states[r] = -1
        table[r, allow] = rng.integers(0, R + 1, int(allow.sum())).astype(np.uint16)
        kinds.append(kind)
    return dict(logits=logits, table=table, states=states, fallback=fallback, kinds=kinds)


def free_pick(row):
    """k_verify_rows' rule: the largest value, the lowest index on ties, a NaN never taken; nothing but NaN: 0"""
    row = np.asarray(row, np.float32)
    ok = ~np.isnan(row)
    return int(np.flatnonzero(ok & (row == row[ok].max()))[0]) if ok.any() else 0


def op_expected(case):
    """(picks, dead) by dfa_ref.pick on each row's allow-list; the fallback token and dead = 1 where nothing is allowed"""
    picks, dead = [], []
    for r, st in enumerate(case["states"]):
        p = free_pick(case["logits"][r]) if st < 0 else dfa_ref.pick(case["table"][st], case["logits"][r])
        picks.append(int(case["fallback"][r]) if p < 0 else p)
        dead.append(1 if p < 0 else 0)
    return np.array(picks, np.int32), np.array(dead, np.int32)
