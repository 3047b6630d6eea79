"""Python restatement of the row dealing and of the loop of drafted greedy decoding for several sequences at once (include/llamahip.h:
llamahip_lookup_deal_rows, llamahip_decode_greedy_lookup_multi) -- what tests/test_lookup_multi_host.py and tests/test_gpu_lookup_multi.py
check the library against.  The drafter and the accept rule are lookup_ref's."""
import lookup_ref

ROWS = 16          # rows of a step (SET_MAX)


def deal_rows(want, budget=ROWS):
    """every sequence has its base row; the budget - len(want) spare rows go one draft token at a time, round-robin in ascending order,
    to the sequences that still want more, until the spares are used up or nobody wants more"""
    give = [0] * len(want)
    spare = budget - len(want)
    while spare > 0 and any(g < w for g, w in zip(give, want)):
        for i, w in enumerate(want):
            if spare > 0 and give[i] < w:
                give[i] += 1
                spare -= 1
    return give


def loop_stats(contexts, firsts, Gs, corpus=None, draft_len=0, ngram_min=0, ngram_max=0):
    """the steps llamahip_decode_greedy_lookup_multi takes to produce the true greedy streams Gs[i] after contexts[i] + [firsts[i]]: one
    stats dict per sequence (a step in which a sequence carries no draft is one of its single steps)"""
    n = len(Gs)
    n_steps = len(Gs[0])
    k = draft_len or lookup_ref.DRAFT_LEN
    hist = [[int(t) for t in contexts[i]] + [int(firsts[i])] for i in range(n)]
    Gs = [[int(t) for t in G] for G in Gs]
    st = [dict(n_verify_steps=0, n_single_steps=0, n_drafted=0, n_accepted=0) for _ in range(n)]
    done = [0] * n
    while True:
        act = [i for i in range(n) if done[i] < n_steps]
        if not act:
            return st
        drafts = []
        for i in act:
            room = min(k, n_steps - done[i] - 1)
            drafts.append(lookup_ref.draft(hist[i], corpus, room, ngram_min, ngram_max) if room > 0 else [])
        give = deal_rows([len(d) for d in drafts])
        for i, d, g in zip(act, drafts, give):
            d = d[:g]
            a = 0
            if d:
                while a < len(d) and d[a] == Gs[i][done[i] + a]:
                    a += 1
                st[i]["n_verify_steps"] += 1
                st[i]["n_drafted"] += len(d)
                st[i]["n_accepted"] += a
            else:
                st[i]["n_single_steps"] += 1
            hist[i] += Gs[i][done[i]:done[i] + a + 1]
            done[i] += a + 1
