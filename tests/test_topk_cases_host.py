"""CPU: the inputs of tests/test_gpu_topk_edges.py are what they claim to be.  For every case of tests/topk_ref.py the float64 reference
(`classify`) together with the three documented limits of the device selection yields the case's expected flag, and what the builders
promise -- exactly 768 / 769 survivors, a tie at exactly the stated positions, the stated number of finite values -- is counted here in
numpy.  Nothing in this file ranks the way the kernel does."""
import numpy as np
import pytest

import topk_ref as T

CASES = T.all_cases()


def _sc(c):
    return T.scores(c.logits, c.window, c.penalty, c.temp)


def test_scores_follow_the_host_formula():
    lg = np.array([2.0, -2.0, -0.0, 0.0, -np.inf, np.inf, 1.0, -1.0], np.float32)
    sc = T.scores(lg, [0, 1, 2, 3, 4, 5, -1, 8, 2 ** 31 - 1], 2.0, 0.5)
    assert T.bits(sc).tolist() == T.bits([2.0, -8.0, -0.0, 0.0, -np.inf, np.inf, 2.0, -2.0]).tolist()
    assert np.signbit(sc[2]) and not np.signbit(sc[3])                  # -0.0 is not < 0: it is divided, and stays -0.0
    t = float(np.float32(0.8))
    sc = T.scores(np.array([3.0, -3.0], np.float32), [0, 1, 1], 1.3, t)
    assert sc.tolist() == [3.0 * (1.0 / t) / 1.3, -3.0 * (1.0 / t) * 1.3]


def test_classify_on_hand_made_rows():
    c = lambda v, k: T.classify(np.array(v, np.float64), k)
    assert c([5, 4, 3, 2, 1], 2)[0] == T.UNIQUE and c([5, 4, 3, 2, 1], 2)[1].tolist() == [0, 1]
    assert c([1, 5, 4, 4, 3], 2)[0] == T.AMBIGUOUS                      # k-th == (k+1)-th
    assert c([4, 4, 3, 2, 1], 2)[0] == T.AMBIGUOUS                      # inside the k best
    assert c([5, 4, 3, 3, 1], 2)[0] == T.EITHER                         # (k+1)-th == (k+2)-th
    assert c([5, 4, 3, 2, 2], 2)[0] == T.UNIQUE                         # (k+2)-th == (k+3)-th
    assert c([5, 0.0, -0.0, -1], 2)[0] == T.AMBIGUOUS and c([5, -0.0, 0.0, -1], 2)[0] == T.AMBIGUOUS
    assert c([5, -0.0, -1], 2)[0] == T.UNIQUE and np.signbit(c([5, -0.0, -1], 2)[2][1])
    assert c([5, 4, 3, np.nan], 1)[0] == T.AMBIGUOUS
    assert c([np.inf, np.inf, 0], 1)[0] == T.AMBIGUOUS and c([np.inf, 1, 0], 1)[0] == T.UNIQUE
    assert c([3, 7, 7, 1], 2)[1].tolist() == [1, 2]                     # ties: the lower id first
    assert c([2.0], 1) [0] == T.UNIQUE and c([2.0, 1.0], 2)[0] == T.UNIQUE


def test_every_kind_of_case_is_there():
    names = " ".join(c.name for c in CASES)
    for word in ("zero_pair_inside_k", "zero_pair_at_cut", "lone_neg_zero", "lone_neg_zero_in_window", "tie_km1_k", "tie_k_k1", "tie_k1_k2", "tie_k2_k3",
                 "same_group", "other_wave", "other_block", "penalty_makes_tie", "penalty_unmakes_tie", "four_way_tie", "zero_in_window_inf_penalty", "one_pos_inf", "two_pos_inf", "masked_", "neg_inf_in_window",
                 "flt_max_and_denormals", "neg_nan_below_cut", "nan_at_last_id", "nan_logit_in_window", "cap_768", "cap_769", "window_len0", "window_len1024",
                 "window_duplicates", "window_out_of_range") + tuple(f"vocab_V{V}_k1" for V in T.VOCABS):
        assert word in names, word
    flags = [c.expected_flag for c in CASES]
    assert min(flags.count(f) for f in (T.MUST_BE_EXACT, T.MUST_BE_INEXACT, T.EITHER_FLAG)) >= 8
    for c in CASES:
        assert c.logits.dtype == np.float32 and c.window.dtype == np.int32 and 1 <= c.k <= min(64, c.logits.size) and c.logits.size <= 32768 and c.window.size <= 1024


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_case_is_what_it_claims(c):
    sc = _sc(c)
    status, ids, top = T.classify(sc, c.k)
    assert T.expected_flag(c.logits, c.window, c.k, c.penalty, c.temp) == c.expected_flag, status
    order = T.order_of(sc)
    pre = c.pre
    if "tie_at" in pre:
        p, q = pre["tie_at"]
        assert q == p + 1 and sc[order[p - 1]] == sc[order[q - 1]]
        assert sorted(order[p - 1:q].tolist()) == sorted(pre["tie_ids"])
        s = sc[order[:c.k + 4]]
        eq = np.flatnonzero(s[:-1] == s[1:]) + 1                        # 1-based first positions of equal neighbours
        assert eq.tolist() == ([p] if p <= s.size - 1 else []), eq      # no other equality near the cut
    if "tie_run" in pre:
        p, q = pre["tie_run"]
        s = sc[order[:q + 1]]
        assert p <= c.k < q and np.all(s[p - 1:q] == s[p - 1]) and s[p - 2] > s[p - 1] > s[q] and T.n_survivors(sc, c.k) == pre["n_survivors"]
        ids = np.sort(order[p - 1:q])                                   # the lower two in one wave (64 ids), the higher two in another
        assert ids[0] // 64 == ids[1] // 64 != ids[2] // 64 == ids[3] // 64
    elif "n_survivors" in pre:
        assert T.n_survivors(sc, c.k) == pre["n_survivors"] and np.unique(sc).size == sc.size and status == T.UNIQUE
        assert T.threshold(sc, c.k) == sc[(c.k - 1) * 16]               # group (k - 1)'s first element
    if "n_finite" in pre:
        assert np.count_nonzero(np.isfinite(sc)) == pre["n_finite"] and np.count_nonzero(np.isneginf(sc)) == sc.size - pre["n_finite"]
    if "neg_zero_at" in pre:
        p, z = pre["neg_zero_at"]
        assert p <= c.k and order[p - 1] == z and np.signbit(sc[z]) and sc[z] == 0 and np.count_nonzero(sc == 0) == 1 and status == T.UNIQUE
    if "nan_scores" in pre:
        assert np.count_nonzero(np.isnan(sc)) == pre["nan_scores"]
    if "k_over_groups" in pre:
        assert status == T.UNIQUE and pre["k_over_groups"] == (c.k > T.n_nonempty_groups(sc.size))
        assert pre["k_over_groups"] or T.n_survivors(sc, c.k) <= T.LCAP
    if c.expected_flag == T.MUST_BE_EXACT:
        assert status == T.UNIQUE and not np.isnan(top).any()


def test_mixed_rows_keep_their_kind_under_any_quiet_window():
    rows = T.mixed_rows()
    rng = np.random.default_rng(3)
    assert len(rows) == 16 and len({(r.logits.size, r.k, r.penalty, r.temp) for r in rows}) == 1
    kinds = [r.expected_flag for r in rows]
    assert kinds[0] == kinds[-1] == T.MUST_BE_EXACT and kinds == list(T.MIXED_KINDS)
    for n in (0, 3, 64, 1024):
        for r in rows:
            assert T.expected_flag(r.logits, T.quiet_ids(rng, n), r.k, r.penalty, r.temp) == r.expected_flag, (r.name, n)
    assert T.n_survivors(_sc(rows[3]), T.MIXED_K) == 769 and T.n_survivors(_sc(rows[7]), T.MIXED_K) == 768
