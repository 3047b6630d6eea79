"""Python restatement of the drafter and of the accept rule of drafted greedy decoding (include/llamahip.h: llamahip_lookup_draft,
llamahip_decode_greedy_lookup) -- what tests/test_lookup_host.py and tests/test_gpu_lookup.py check the library against."""
DRAFT_LEN, NGRAM_MIN, NGRAM_MAX = 15, 1, 3        # the header's defaults (LLAMAHIP_LOOKUP_*)


def draft(history, corpus=None, draft_len=0, ngram_min=0, ngram_max=0):
    """the tokens that followed the most recent earlier occurrence of history's last n tokens, in history, else in corpus (an occurrence
    counts if a token follows it); the longest n of ngram_max .. ngram_min that occurs anywhere wins"""
    h, c = [int(t) for t in history], [int(t) for t in (corpus if corpus is not None else [])]
    k, lo, hi = draft_len or DRAFT_LEN, ngram_min or NGRAM_MIN, ngram_max or NGRAM_MAX
    for n in range(min(hi, len(h)), lo - 1, -1):
        key = h[len(h) - n:]
        for src in (h, c):
            last = len(h) - n - 1 if src is h else len(c) - n - 1
            for s in range(last, -1, -1):
                if src[s:s + n] == key:
                    return src[s + n:s + n + k]
    return []


def n_accept(tokens, picks):
    """tokens = [last token, draft ...], picks[j] = the greedy pick of row j: the number of leading draft tokens the picks reproduce"""
    a = 0
    while a < len(tokens) - 1 and int(picks[a]) == int(tokens[a + 1]):
        a += 1
    return a


def loop_stats(context, first, G, corpus=None, draft_len=0, ngram_min=0, ngram_max=0):
    """the steps llamahip_decode_greedy_lookup takes to produce the true greedy stream G after context + [first]"""
    hist = [int(t) for t in context] + [int(first)]
    G = [int(t) for t in G]
    k = draft_len or DRAFT_LEN
    st = dict(n_verify_steps=0, n_single_steps=0, n_drafted=0, n_accepted=0)
    done = 0
    while done < len(G):
        room = min(k, len(G) - done - 1)
        d = draft(hist, corpus, room, ngram_min, ngram_max) if room > 0 else []
        a = 0
        if d:
            while a < len(d) and d[a] == G[done + a]:
                a += 1
            st["n_verify_steps"] += 1
            st["n_drafted"] += len(d)
            st["n_accepted"] += a
        else:
            st["n_single_steps"] += 1
        hist += G[done:done + a + 1]
        done += a + 1
    return st
