"""The sampler's front half in float64 numpy (the reference's scores and its top-k candidates, utils.cpp:345-395) and the inputs at which a
device selection can go wrong: signed zeros, ties placed at the cut, ties made and unmade by the repeat penalty, infinities, NaN, the
768-survivor cap, tiny vocabularies and odd windows.  A plain module: tests/test_topk_cases_host.py checks the inputs on the CPU,
tests/test_gpu_topk_edges.py and tests/test_gpu_pick_ties.py hold the kernels to them.

What a case expects comes from `classify` (which knows nothing about the device) plus the three documented limits of the device selection
(include/llamahip.h, llamahip_eval_topk): a NaN score, more than 768 values at or above the threshold, top_k above the number of non-empty
groups.  The builders only use the documented structure (element i belongs to group (i % 1024) / 16, the threshold is the top_k-th largest of
the 64 group maxima) to PLACE values; nothing here ranks the way the kernel does."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

UNIQUE, EITHER, AMBIGUOUS = "unique", "either", "ambiguous"
MUST_BE_EXACT, MUST_BE_INEXACT, EITHER_FLAG = "must_be_exact", "must_be_inexact", "either"
LCAP = 768                                   # the device ranks at most this many survivors
F32_TEMP = float(np.float32(0.8))
FLT_MAX = float(np.finfo(np.float32).max)
DENORM_MIN = float(np.float32(2.0 ** -149))
NEG_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]


class Case(NamedTuple):
    logits: np.ndarray                       # float32 [V]
    window: np.ndarray                       # int32 ids (any length, any value)
    k: int
    penalty: float
    temp: float
    expected_flag: str
    name: str = ""
    pre: dict = {}                           # what the builder promises about the input (checked on the CPU)


# ------------------------------------------------------------------------------------------------ the reference
def scores(logits, window, repeat_penalty, temp) -> np.ndarray:
    """float64 scores: logit * (1 / temp), and for ids in the window * penalty where the logit is < 0, else / penalty (-0.0 is not < 0);
    window ids outside [0, V) are ignored"""
    lg = np.ascontiguousarray(logits, np.float32).ravel()
    V = lg.size
    w = np.asarray(window, np.int64).ravel()
    seen = np.zeros(V, bool)
    seen[w[(w >= 0) & (w < V)]] = True
    with np.errstate(all="ignore"):
        sc = lg.astype(np.float64) * (1.0 / float(temp))
        neg = lg < 0
        sc[seen & neg] = sc[seen & neg] * float(repeat_penalty)
        sc[seen & ~neg] = sc[seen & ~neg] / float(repeat_penalty)
    return sc


def order_of(sc) -> np.ndarray:
    """all ids in (score descending, id ascending) order; == on scores, so +0 and -0 are one value; NaN last"""
    return np.argsort(-np.asarray(sc, np.float64), kind="stable")


def classify(sc, k: int):
    """-> (status, ids[k], top_scores[k]).  AMBIGUOUS: a NaN anywhere, or two of the first k + 1 positions hold equal scores; EITHER: not
    that, but the (k + 1)-th equals the (k + 2)-th; UNIQUE: everything else."""
    sc = np.asarray(sc, np.float64)
    order = order_of(sc)
    ids = order[:k].astype(np.int32)
    top = sc[order[:k + 2]]
    n = min(k, top.size - 1)                     # (a vocabulary of k entries has no (k + 1)-th)
    if np.isnan(sc).any() or bool((top[:n] == top[1:n + 1]).any()):
        status = AMBIGUOUS
    elif top.size == k + 2 and top[k] == top[k + 1]:
        status = EITHER
    else:
        status = UNIQUE
    return status, ids, sc[ids]


# ------------------------------------------------------------------------------------------------ the documented device limits
def group_of(i):
    return (np.asarray(i) % 1024) // 16


def n_nonempty_groups(V: int) -> int:
    return min(64, (V + 15) // 16)


def threshold(sc, k: int) -> float:
    """the k-th largest of the group maxima (k <= the number of non-empty groups; no NaN)"""
    sc = np.asarray(sc, np.float64)
    g = group_of(np.arange(sc.size))
    gmax = np.array([sc[g == j].max() for j in range(n_nonempty_groups(sc.size))])
    return float(np.sort(gmax)[::-1][k - 1])


def n_survivors(sc, k: int) -> int:
    return int(np.count_nonzero(np.asarray(sc, np.float64) >= threshold(sc, k)))


def expected_flag(logits, window, k, penalty, temp) -> str:
    """classify + the three limits -> must_be_exact / must_be_inexact / either"""
    sc = scores(logits, window, penalty, temp)
    status = classify(sc, k)[0]
    if status == AMBIGUOUS or k > n_nonempty_groups(sc.size) or n_survivors(sc, k) > LCAP:
        return MUST_BE_INEXACT
    return EITHER_FLAG if status == EITHER else MUST_BE_EXACT


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check(tag, logits, window, k, penalty, temp, flag, exact, got_scores, got_ids) -> None:
    """one row of any entry point against the reference: safety always, liveness by `flag`"""
    sc = scores(logits, window, penalty, temp)
    status, ids, top = classify(sc, k)
    if exact:
        assert status != AMBIGUOUS, f"{tag}: exact = 1 on an ambiguous row; device ids {np.asarray(got_ids).tolist()} scores {np.asarray(got_scores).tolist()}"
        assert np.asarray(got_ids).tolist() == ids.tolist(), f"{tag}: ids {np.asarray(got_ids).tolist()} want {ids.tolist()}"
        assert bits(got_scores).tolist() == bits(top).tolist(), f"{tag}: scores {np.asarray(got_scores).tolist()} want {top.tolist()}"
    if flag == MUST_BE_EXACT:
        assert exact, f"{tag}: must be exact ({status})"
    elif flag == MUST_BE_INEXACT:
        assert not exact, f"{tag}: must be inexact ({status})"
    else:
        assert flag == EITHER_FLAG, flag


# ------------------------------------------------------------------------------------------------ builders
def low(V: int, start: float = -2.0) -> np.ndarray:
    """V distinct negative float32 values, descending with the id, exact in float32"""
    return (start - np.arange(V) * 2.0 ** -6).astype(np.float32)


def _i32(w) -> np.ndarray:
    return np.asarray(w, np.int64).astype(np.int32).ravel()


def _above(lg, n: int, avoid) -> None:
    """n distinct positive values (5, 6, ...) at ids of n different groups, none of them in `avoid`"""
    V, put, j = lg.size, 0, 0
    while put < n:
        i = (7 + 48 * j) % V
        j += 1
        if i in avoid or lg[i] > 0:
            continue
        lg[i] = 5.0 + put
        put += 1


def zero_pair(V, k, p, a, b, neg_first, flag, name) -> Case:
    """a (+0, -0) pair at the positions (p, p + 1) of the order, ids a < b, the -0 at a (neg_first) or at b; everything else distinct"""
    lg = low(V)
    _above(lg, p - 1, (a, b))
    lg[a], lg[b] = (np.float32(-0.0), np.float32(0.0)) if neg_first else (np.float32(0.0), np.float32(-0.0))
    return Case(lg, _i32([]), k, 1.3, F32_TEMP, flag, name, {"tie_at": (p, p + 1), "tie_ids": (a, b)})


def lone_neg_zero(V, k, p, z, window, name, penalty=1.3, temp=F32_TEMP) -> Case:
    """one -0.0 logit at position p <= k, nothing equal to it"""
    lg = low(V)
    _above(lg, p - 1, (z,))
    lg[z] = np.float32(-0.0)
    return Case(lg, _i32(window), k, penalty, temp, MUST_BE_EXACT, name, {"neg_zero_at": (p, z)})


def signed_zero_cases() -> list[Case]:
    out = []
    for where, k, p, flag in (("inside_k", 3, 2, MUST_BE_INEXACT), ("at_cut", 2, 2, MUST_BE_INEXACT), ("at_cut_k1", 1, 1, MUST_BE_INEXACT),
                              ("k1_k2", 1, 2, EITHER_FLAG), ("k2_k3", 1, 3, MUST_BE_EXACT)):
        for V, a, b, arr in ((64, 20, 41, "one_block"), (2048, 16, 1024 + 40, "two_blocks")):
            for neg_first in (True, False):
                out.append(zero_pair(V, k, p, a, b, neg_first, flag, f"zero_pair_{where}_{arr}_{'neg' if neg_first else 'pos'}_first"))
    for V, z in ((64, 33), (2048, 1500)):
        out.append(lone_neg_zero(V, 2, 2, z, [], f"lone_neg_zero_V{V}"))
        out.append(lone_neg_zero(V, 2, 2, z, [z, 7], f"lone_neg_zero_in_window_V{V}"))
        out.append(lone_neg_zero(V, 1, 1, z, [z], f"neg_zero_on_top_V{V}", penalty=0.5, temp=1.0))
    return out


def zero_in_window_inf_penalty_cases() -> list[Case]:
    """a zero logit in the window is DIVIDED by the penalty (0 / inf = 0), never multiplied (0 * inf = NaN)"""
    out = []
    for V, z in ((64, 33), (2048, 1500)):
        c = lone_neg_zero(V, 2, 2, z, [z], f"neg_zero_in_window_inf_penalty_V{V}", penalty=float("inf"))
        out.append(c)
        lg = c.logits.copy()
        lg[z] = 0.0
        out.append(Case(lg, c.window, 2, c.penalty, c.temp, MUST_BE_EXACT, f"pos_zero_in_window_inf_penalty_V{V}", {}))
    return out


def four_way_tie(mirrored: bool) -> Case:
    """V = 2048, top_k = 8: seven larger values, then FOUR equal ones at the positions 8 .. 11 (the 8th ties with its three runners-up), then
    one smaller value; everything else far below.  The twelve sit in two waves of the selection's workgroup, eight in one (among them the two
    tied entries with the higher ids) and four in the other (the two with the lower ids), so that a rank pass which mixes up its id order
    inside a group of equals cannot hide behind a pair: with two equal entries any order flags the row, with four it need not."""
    V, k = 2048, 8
    lg = low(V, -50.0)
    if not mirrored:                                               # ids 64 .. 127 hold eight, ids 0 .. 63 four
        big, hi_pair, one_big, lo_pair, mid = [64, 65, 80, 81, 96, 112], (100, 116), 0, (17, 33), 49
    else:                                                          # ids 1024 .. 1087 hold eight, ids 960 .. 1023 four
        big, hi_pair, one_big, lo_pair, mid = [1040, 1041, 1056, 1057, 1072, 1073], (1024, 1025), 960, (977, 993), 1009
    lg[big + [one_big]] = 20.0 + np.arange(7)
    lg[list(hi_pair + lo_pair)] = 10.0
    lg[mid] = 5.0
    return Case(lg, _i32([]), k, 1.3, F32_TEMP, MUST_BE_INEXACT, f"four_way_tie_at_cut{'_mirrored' if mirrored else ''}",
                {"tie_run": (8, 11), "n_survivors": 12})


ARRANGEMENTS = {"same_group": (1024 + 35, 1024 + 44), "other_wave": (37, 37 + 64 * 9), "other_block": (2048 + 5, 3 * 1024 + 700)}


def tie(V, k, p, a, b, flag, name, seed=0) -> Case:
    """two equal logits (ids a, b) at exactly the positions (p, p + 1) of the order; every other value is distinct"""
    rng = np.random.default_rng(seed)
    vals = (40.0 - np.arange(V) * 2.0 ** -5).astype(np.float32)       # descending, distinct
    vals[p] = vals[p - 1]                                               # 0-based p - 1 and p hold the positions p and p + 1
    rest = np.delete(np.arange(V), [a, b])
    rng.shuffle(rest)
    rest = np.concatenate([rest[rest < 16384], rest[rest >= 16384]])   # (the positive values stay out of `quiet_ids`)
    lg = np.empty(V, np.float32)
    lg[a], lg[b] = vals[p - 1], vals[p]
    lg[rest] = np.delete(vals, [p - 1, p])
    return Case(lg, _i32(rest[-64:]), k, 1.3, F32_TEMP, flag, name, {"tie_at": (p, p + 1), "tie_ids": (a, b)})


def tie_cases() -> list[Case]:
    out = []
    for k in (5, 64):
        for what, p, flag in (("km1_k", k - 1, MUST_BE_INEXACT), ("k_k1", k, MUST_BE_INEXACT), ("k1_k2", k + 1, EITHER_FLAG), ("k2_k3", k + 2, MUST_BE_EXACT)):
            for arr, (a, b) in ARRANGEMENTS.items():
                if k == 5 or arr == "other_block":
                    out.append(tie(4096, k, p, a, b, flag, f"tie_{what}_k{k}_{arr}", seed=1000 * k + p))
    return out


def penalty_cases() -> list[Case]:
    """temp = 1, penalty = 2: 2.0 in the window ties with 1.0 outside it; equal logits with one of them in the window do not tie"""
    out = []
    for V, a, b in ((64, 3, 40), (2048, 3, 1024 + 300)):
        for k in (1, 2):
            lg = low(V)
            lg[a], lg[b] = 2.0, 1.0
            out.append(Case(lg, _i32([a]), k, 2.0, 1.0, MUST_BE_INEXACT, f"penalty_makes_tie_V{V}_k{k}", {"tie_at": (1, 2), "tie_ids": (a, b)}))
            out.append(Case(lg, _i32([b, b]), k, 2.0, 1.0, MUST_BE_EXACT, f"penalty_no_tie_V{V}_k{k}", {}))
            lg = low(V)
            lg[a], lg[b] = 2.0, 2.0
            out.append(Case(lg, _i32([b]), k, 2.0, 1.0, MUST_BE_EXACT, f"penalty_unmakes_tie_V{V}_k{k}", {}))
            out.append(Case(lg, _i32([V, -1]), k, 2.0, 1.0, MUST_BE_INEXACT, f"equal_logits_no_window_V{V}_k{k}", {"tie_at": (1, 2), "tie_ids": (a, b)}))
            lg = low(V)
            lg[a], lg[b] = -0.25, -0.5                             # -0.25 * 2 == -0.5
            out.append(Case(lg, _i32([a]), k, 2.0, 1.0, MUST_BE_INEXACT, f"penalty_makes_negative_tie_V{V}_k{k}", {"tie_at": (1, 2), "tie_ids": (a, b)}))
    return out


def pos_inf(V, k, ids, window, flag, name) -> Case:
    lg = low(V)
    lg[list(ids)] = np.inf
    pre = {"tie_at": (1, 2), "tie_ids": tuple(ids)} if len(ids) == 2 else {}
    return Case(lg, _i32(window), k, 1.3, F32_TEMP, flag, name, pre)


def inf_cases() -> list[Case]:
    out = [pos_inf(64, 3, [11], [11], MUST_BE_EXACT, "one_pos_inf"), pos_inf(64, 3, [11, 50], [11], MUST_BE_INEXACT, "two_pos_inf")]
    lg = low(64)
    lg[63] = lg[5] = -np.inf
    out.append(Case(lg, _i32([63, 0]), 3, 1.3, F32_TEMP, MUST_BE_EXACT, "neg_inf_in_window", {}))
    k = 4                                                          # a masked vocabulary: all but n entries are -inf
    for V in (640, 2048):
        for n, flag in ((k + 2, MUST_BE_EXACT), (k + 9, MUST_BE_EXACT), (k - 1, MUST_BE_INEXACT), (1, MUST_BE_INEXACT)):
            lg = np.full(V, -np.inf, np.float32)
            ids = (np.arange(n) * 48 + 5) % V                      # one group each
            lg[ids] = 3.0 - np.arange(n) * 0.5
            out.append(Case(lg, _i32(ids[:2]), k, 1.3, F32_TEMP, flag, f"masked_V{V}_n{n}", {"n_finite": n}))
    lg = low(2048)
    lg[3], lg[200], lg[1999], lg[700], lg[2000] = FLT_MAX, DENORM_MIN, -DENORM_MIN, -1.0, -FLT_MAX
    for temp in (1.0, 0.01):
        out.append(Case(lg, _i32([3, 1999]), 4, 1.3, temp, MUST_BE_EXACT, f"flt_max_and_denormals_temp{temp}", {}))
    out.append(Case(np.array([-FLT_MAX], np.float32), _i32([0]), 1, 1.3, 0.01, MUST_BE_EXACT, "neg_flt_max_alone", {}))
    return out


def nan_row(V, k, at, val, window, name, penalty=1.3) -> Case:
    rng = np.random.default_rng(V + at)
    lg = rng.permutation(low(V, 30.0))
    lg[at] = val
    return Case(lg, _i32(window), k, penalty, F32_TEMP, MUST_BE_INEXACT, name, {"nan_scores": 1})


def nan_cases() -> list[Case]:
    out = []
    for V in (1500, 4096):
        out += [nan_row(V, 8, 900, NEG_NAN, [], f"neg_nan_below_cut_V{V}"), nan_row(V, 8, 900, np.float32(np.nan), [], f"pos_nan_V{V}"),
                nan_row(V, 8, V - 1, NEG_NAN, [], f"nan_at_last_id_V{V}"), nan_row(V, 8, 70, NEG_NAN, [70], f"nan_logit_in_window_V{V}"),
                nan_row(V, 8, 70, np.float32(np.inf), [70], f"inf_over_inf_penalty_V{V}", penalty=float("inf"))]
    return out


def cap(V, k, extra, flag, name) -> Case:
    """all values distinct; group g's first element is 100 - g, so the threshold is group (k - 1)'s maximum; `extra` other values lie above
    it (inside groups whose own maximum is larger still) -> k + extra survivors"""
    assert 3 <= k <= 64 and V >= 8192
    lg = low(V)
    lg[np.arange(64) * 16] = 100.0 - np.arange(64)
    others = np.array([i for i in range(1024, V) if group_of(i) <= min(5, k - 3)])
    lg[others[:extra]] = (100.0 - (k - 1)) + (1 + np.arange(extra)) / 1024.0
    return Case(lg, _i32(np.arange(V - 1000, V - 936)), k, 1.3, F32_TEMP, flag, name, {"n_survivors": k + extra})


def cap_cases() -> list[Case]:
    return [cap(32000, 64, 704, MUST_BE_EXACT, "cap_768_survivors"), cap(32000, 64, 705, MUST_BE_INEXACT, "cap_769_survivors")]


VOCABS = (1, 16, 17, 640, 1008, 1009, 1023, 1024, 1025, 2047, 4096, 32000, 32768)


def vocab_cases() -> list[Case]:
    out = []
    for V in VOCABS:
        rng = np.random.default_rng(V)
        lg = (rng.permutation(V).astype(np.float32) - V // 2) * np.float32(2.0 ** -7)        # distinct, both signs
        full = (V + 15) // 16
        ks = {1, min(full, 64), 64 if V >= 64 else 1}
        if full + 1 <= min(64, V):
            ks.add(full + 1)
        win = rng.integers(0, V, 64)
        for k in sorted(ks):
            flag = MUST_BE_INEXACT if k > n_nonempty_groups(V) else MUST_BE_EXACT
            out.append(Case(lg, _i32(win), k, 1.3, F32_TEMP, flag, f"vocab_V{V}_k{k}", {"k_over_groups": k > n_nonempty_groups(V)}))
    return out


def plain(V, k, seed, n_window=64) -> Case:
    rng = np.random.default_rng(seed)
    lg = (rng.permutation(V).astype(np.float32) - V // 3) * np.float32(2.0 ** -6)
    return Case(lg, _i32(rng.integers(0, V, n_window)), k, 1.3, F32_TEMP, MUST_BE_EXACT, f"plain_V{V}_k{k}_{seed}", {})


def window_cases() -> list[Case]:
    out = []
    V, k = 1500, 8
    rng = np.random.default_rng(9)
    lg = (rng.standard_normal(V) * 3).astype(np.float32)
    best = np.argsort(-lg)[:12]
    wins = {"len0": [], "len1": [best[0]], "len1024": np.concatenate([best[:6], rng.integers(0, V, 1018)]), "duplicates": [best[1]] * 5 + [best[3]] * 2,
            "out_of_range": [-1, V, 2 ** 31 - 1, best[0], -2 ** 31, V + 1024], "only_out_of_range": [-1, V, 2 ** 31 - 1]}
    for name, w in wins.items():
        out.append(Case(lg, _i32(w), k, 1.3, F32_TEMP, MUST_BE_EXACT, f"window_{name}", {"window_len": len(w)}))
    for pen in (1.0, 0.5, 1.3):
        for temp in (1.0, F32_TEMP, 0.01):
            w = np.concatenate([best[::2], rng.integers(0, V, 58)])
            out.append(Case(lg, _i32(w), 40, pen, temp, MUST_BE_EXACT, f"params_pen{pen}_temp{temp:.2f}", {}))
    return out


_ALL = None


def all_cases() -> list[Case]:
    global _ALL
    if _ALL is None:
        _ALL = signed_zero_cases() + zero_in_window_inf_penalty_cases() + tie_cases() + [four_way_tie(False), four_way_tie(True)] + penalty_cases() + inf_cases() + nan_cases() + cap_cases() + vocab_cases() + window_cases()
        assert len({c.name for c in _ALL}) == len(_ALL)
    return _ALL


MIXED_V, MIXED_K = 32000, 8
MIXED_KINDS = (MUST_BE_EXACT, MUST_BE_INEXACT, MUST_BE_EXACT, MUST_BE_INEXACT, MUST_BE_INEXACT, MUST_BE_EXACT, MUST_BE_INEXACT, MUST_BE_EXACT,
               MUST_BE_INEXACT, MUST_BE_EXACT, MUST_BE_EXACT, MUST_BE_EXACT, EITHER_FLAG, MUST_BE_EXACT, MUST_BE_INEXACT, MUST_BE_EXACT)


def mixed_rows() -> list[Case]:
    """16 rows of one vocabulary, one top_k, one penalty and one temp for the multi-row entry points: a NaN row, a 769-survivor row, +-0 rows
    and tie rows between exact rows (MIXED_KINDS, whatever window of `quiet_ids` a row gets)"""
    V, k = MIXED_V, MIXED_K
    a, b = ARRANGEMENTS["other_block"]
    rows = [plain(V, k, 160, 0), nan_row(V, k, 9000, NEG_NAN, [], "nan"), plain(V, k, 162, 64), cap(V, k, LCAP + 1 - k, MUST_BE_INEXACT, "cap_769"),
            zero_pair(V, k, k, 16, 1024 + 40, True, MUST_BE_INEXACT, "zero_pair_at_cut"), plain(V, k, 165, 1024),
            tie(V, k, k, a, b, MUST_BE_INEXACT, "tie_k_k1", seed=6), cap(V, k, LCAP - k, MUST_BE_EXACT, "cap_768"),
            zero_pair(V, k, k - 1, 20, 41, False, MUST_BE_INEXACT, "zero_pair_inside_k"), plain(V, k, 169, 64),
            lone_neg_zero(V, k, k, 1500, [1500], "lone_neg_zero"), tie(V, k, k + 2, a, b, MUST_BE_EXACT, "tie_k2_k3", seed=11),
            tie(V, k, k + 1, a, b, EITHER_FLAG, "tie_k1_k2", seed=12), plain(V, k, 173, 1), pos_inf(V, k, [11, 5000], [11], MUST_BE_INEXACT, "two_pos_inf"),
            plain(V, k, 175, 64)]
    assert [r.expected_flag for r in rows] == list(MIXED_KINDS)
    return rows


def quiet_ids(rng, n: int) -> np.ndarray:
    """n ids of MIXED_V that no row of `mixed_rows` gives a special value: whichever of them a window holds, the crafted rows keep their kind"""
    return _i32(16384 + 1024 * rng.integers(0, 14, n) + rng.integers(512, 1024, n))
