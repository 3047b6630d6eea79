// lookup.cpp -- the drafter of llamahip_decode_greedy_lookup (include/llamahip.h): prompt-lookup drafting, pure host code, no handle;
// and the dealing of a multi-sequence verify step's spare rows (llamahip_lookup_deal_rows).
// The guess for "what comes next" is "what came next the last time the text ended like this": the last n tokens are looked up in the
// tokens seen so far, then in a caller-supplied corpus, longest n first.  Deterministic; a wrong guess costs speed, never a token.
#include <stdint.h>

#include "../../include/llamahip.h"

namespace {

// the largest s <= s_max with stream[s .. s + n) == key[0 .. n), or -1
int find_last(const int32_t *stream, int s_max, const int32_t *key, int n) {
    for (int s = s_max; s >= 0; s--) {
        int j = n - 1;                              // (the key's last token first: it differs most often)
        while (j >= 0 && stream[s + j] == key[j]) j--;
        if (j < 0) return s;
    }
    return -1;
}

}  // namespace

extern "C" int32_t llamahip_lookup_draft(const int32_t *history, int32_t n_history, const int32_t *corpus, int32_t n_corpus,
                                         int32_t draft_len, int32_t ngram_min, int32_t ngram_max, int32_t *draft_out) {
    if (draft_len == 0) draft_len = LLAMAHIP_LOOKUP_DRAFT_LEN;
    if (ngram_min == 0) ngram_min = LLAMAHIP_LOOKUP_NGRAM_MIN;
    if (ngram_max == 0) ngram_max = LLAMAHIP_LOOKUP_NGRAM_MAX;
    if (n_history < 0 || n_corpus < 0 || (n_history > 0 && !history) || (n_corpus > 0 && !corpus) || !draft_out || draft_len < 0 || ngram_min < 1 ||
        ngram_max < ngram_min)
        return -1;
    for (int n = ngram_max < n_history ? ngram_max : n_history; n >= ngram_min; n--) {
        const int32_t *key = history + (n_history - n);
        // an earlier occurrence in the history starts before the key itself does, so at least one token follows it
        const int32_t *src = history;
        int n_src = n_history, s = find_last(history, n_history - n - 1, key, n);
        if (s < 0) { src = corpus; n_src = n_corpus; s = find_last(corpus, n_corpus - n - 1, key, n); }
        if (s < 0) continue;
        int k = 0;
        for (int i = s + n; i < n_src && k < draft_len; i++) draft_out[k++] = src[i];
        return k;
    }
    return 0;
}

// Every sequence has its base row; the budget - n_seqs spare rows go one draft token at a time, round-robin in ascending sequence order, to
// the sequences that still want more, until the spares are used up or nobody wants more.
extern "C" int32_t llamahip_lookup_deal_rows(const int32_t *want, int32_t n_seqs, int32_t budget, int32_t *give) {
    if (!want || !give || n_seqs < 1 || n_seqs > 16 || budget < n_seqs || budget > 16) return -1;
    for (int i = 0; i < n_seqs; i++) if (want[i] < 0 || want[i] > 15) return -1;
    for (int i = 0; i < n_seqs; i++) give[i] = 0;
    int spare = budget - n_seqs, dealt = 0;
    for (bool any = true; spare > 0 && any;) {
        any = false;
        for (int i = 0; i < n_seqs && spare > 0; i++)
            if (give[i] < want[i]) { give[i]++; spare--; dealt++; any = true; }
    }
    return dealt;
}
