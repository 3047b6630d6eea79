"""llamahip_beam_search's contract (include/llamahip.h) in plain Python, for the tests: the step rule, the slots, the search itself over a
callable `cands_of(tokens) -> (ids, logprob)` -- the 2 * n_beams top entries of the logits row that follows prompt + tokens -- and the numpy
stand-in for k_row_topn that the CPU-side seed checks use."""
import math

import numpy as np

DONE_LENGTH, DONE_STOP = "length", "stop"
# the GPU cases of tests/test_gpu_beam_search.py (model synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=4, n_layer=2), n_ctx 64, n_predict 12):
# (n_beams, n_prompt, chunk_tokens, stop, n_return, length_norm); a stop case stops at token STOP_AT of the stop-less run's second hypothesis
MODEL_SEED, PROMPT_SEED, STOP_AT = 4101, 4110, 2
CASES = [(1, 1, 0, 0, 0, 0), (2, 9, 0, 0, 0, 0), (3, 20, 9, 0, 0, 0), (4, 20, 0, 0, 0, 0), (8, 9, 9, 0, 0, 0), (16, 20, 9, 0, 0, 0), (16, 1, 0, 0, 0, 0),
         (4, 9, 0, 1, 2, 0), (8, 20, 9, 1, 0, 1), (16, 9, 0, 1, 4, 0), (3, 1, 0, 1, 0, 0)]
HANDLE_CASES = [(4, 9, 9, 0, 0, 0), (4, 20, 0, 1, 2, 0)]


def np_cands(row, n):
    """k_row_topn's contract on one row, in numpy: ids by value descending (the lower index first on equal values) and the float64
    log-softmax at those ids; a row with a NaN or a +inf gives ids -1 and NaN"""
    row = np.asarray(row, np.float32)
    if np.isnan(row).any() or (row == np.inf).any():
        return np.full(n, -1, np.int32), np.full(n, np.nan)
    ids = np.argsort(-row, kind="stable")[:n].astype(np.int32)
    r = row.astype(np.float64)
    mx = float(row.max())
    lse = math.log(float(np.exp(r - mx).sum()))
    return ids, (r[ids] - mx) - lse


def select(live_score, cand_ids, cand_logprob, n_beams, stop_token):
    """one step's walk: (new = [(parent, token, score)], fin = [(parent, score)], n_dead, walked) -- walked: the ordered candidates up to and
    including the first one the walk did not take (for the tests' gap condition)"""
    cands, dead = [], 0
    for i, S in enumerate(live_score):
        if int(cand_ids[i][0]) < 0:
            dead += 1
            continue
        for v, lp in zip(cand_ids[i], cand_logprob[i]):
            c = float(S) + float(lp)
            if int(v) < 0 or c != c:
                continue
            cands.append((c, i, int(v)))
    cands.sort(key=lambda t: (-t[0], t[1], t[2]))
    new, fin, k = [], [], 0
    while k < len(cands) and len(new) < n_beams:
        c, i, v = cands[k]
        if stop_token >= 0 and v == stop_token:
            fin.append((i, c))
        else:
            new.append((i, v, c))
        k += 1
    return new, fin, dead, cands[: k + 1]


def slots(prev_slot, parents, n_beams):
    """(new_slot, copies = [(src, dst)]): in rank order the first child keeps its parent's slot, every further child takes the lowest slot
    of [0, n_beams) that no beam kept and none took before it"""
    kept = {prev_slot[p] for p in parents}
    free = [s for s in range(n_beams) if s not in kept]
    seen, out, copies = set(), [], []
    for p in parents:
        if p not in seen:
            seen.add(p)
            out.append(prev_slot[p])
        else:
            s = free.pop(0)
            out.append(s)
            copies.append((prev_slot[p], s))
    return out, copies


def search(cands_of, n_prompt, n_beams, n_predict, stop_token=-1, n_return=0, length_norm=False):
    """the search: returns (hyps, info).  hyps: dicts tokens / length / reason / slot / score, best first.  info: the counters of
    llamahip_beam_stats that the contract fixes (n_steps, n_rows, n_copies, n_copied_rows, n_stop, n_dead), the facts the tests' conditions
    are about (childless: a live beam ended a step without a child; min_gap: the smallest difference between neighbouring candidates of a
    walk and between neighbouring keys of the final ranking), and live_sets: per evaluated step the [(tokens, slot)] of its beams"""
    n_return = n_return or n_beams
    live = [{"tokens": (), "S": 0.0, "slot": 0}]
    fin = []
    info = {"n_steps": 0, "n_rows": 0, "n_copies": 0, "n_copied_rows": 0, "n_stop": 0, "n_dead": 0, "childless": False, "min_gap": math.inf,
            "live_sets": [], "early_end": False}
    t = 1
    while True:
        cs = [cands_of(b["tokens"]) for b in live]
        new, done, dead, walked = select([b["S"] for b in live], [c[0] for c in cs], [c[1] for c in cs], n_beams, stop_token)
        for a, b in zip(walked, walked[1:]):
            info["min_gap"] = min(info["min_gap"], abs(a[0] - b[0]))
        info["n_dead"] += dead
        info["n_stop"] += len(done)
        for i, c in done:
            fin.append({"tokens": live[i]["tokens"] + (stop_token,), "S": c, "reason": DONE_STOP, "slot": -1})
        nxt = [{"tokens": live[i]["tokens"] + (v,), "S": c, "parent": i} for i, v, c in new]
        if t == n_predict:
            fin += [{"tokens": b["tokens"], "S": b["S"], "reason": DONE_LENGTH, "slot": live[b["parent"]]["slot"]} for b in nxt]
            break
        if not nxt:
            break
        if not length_norm and stop_token >= 0 and len(fin) >= n_return:
            if sorted((f["S"] for f in fin), reverse=True)[n_return - 1] >= nxt[0]["S"]:
                info["early_end"] = True
                break
        if {b["parent"] for b in nxt} != set(range(len(live))):
            info["childless"] = True
        rows = n_prompt + t - 1
        sl, copies = slots([b["slot"] for b in live], [b["parent"] for b in nxt], n_beams)
        for b, s in zip(nxt, sl):
            b["slot"] = s
        info["n_copies"] += len(copies)
        info["n_copied_rows"] += len(copies) * rows
        info["n_steps"] += 1
        info["n_rows"] += len(nxt)
        info["live_sets"].append([(b["tokens"], b["slot"]) for b in nxt])
        live = nxt
        t += 1
    key = (lambda f: f["S"] / float(len(f["tokens"]))) if length_norm else (lambda f: f["S"])
    order = sorted(range(len(fin)), key=lambda k: -key(fin[k]))      # (stable: ties to the earlier entry)
    ranked = [fin[k] for k in order]
    for a, b in zip(ranked[:n_return], ranked[1:n_return + 1]):
        info["min_gap"] = min(info["min_gap"], abs(key(a) - key(b)))
    hyps = [{"tokens": np.asarray(f["tokens"], np.int32), "length": len(f["tokens"]), "reason": f["reason"], "slot": f["slot"], "score": f["S"]}
            for f in ranked[:n_return]]
    return hyps, info
