// eval_multi.cpp -- the host half of llamahip_eval_multi (include/llamahip.h): the row table of a pass over several KV slots
// (llamahip_eval_multi_rows), what the entry point refuses of its arguments (eval_multi_check) and what llamahip_op_attention_rows refuses of a
// caller's table (rows_table_check); and of llamahip_eval_logprobs_multi / llamahip_score_choices: their argument checks (score_multi_check,
// score_choices_check), the scored rows of a pass (score_multi_rows) and the way their results go back to row order (score_scatter); and what
// llamahip_text_embedding[_multi] and llamahip_op_pool_rows refuse of theirs (embed_check, pool_rows_check).
// Pure host code, no device, no handle: tools/host_sanitize runs it under ASan + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/llamahip.h"

namespace lh {

// prompt_attn.hip split_keys, restated for the host: the key count row j of an eval of N rows at n_past splits over the threads in V*P --
// n_past + N of the eval the row belongs to (ggml.c:5459-5480), which in a chunked pass is the eval of its chunk
static inline int32_t split_keys_host(int32_t n_past, int32_t N, int32_t j, int32_t chunk) {
    return chunk > 0 ? n_past + std::min(N, (j / chunk + 1) * chunk) : n_past + N;
}

// what llamahip_eval_multi refuses of its ARGUMENTS (the handle is the caller's business): 0, or LLAMAHIP_ERR_PREDICT with the limit in err
// (fn: the entry point the messages name)
static int segments_check(const char *fn, int32_t n_ctx, int32_t n_vocab, int32_t n_slots, int32_t n_seqs, const int32_t *slots, const int32_t *n_past,
                          const int32_t *tokens, const int32_t *n_tokens, int32_t chunk_tokens, char *err, size_t err_cap) {
    if (!err) err_cap = 0;
    if (n_seqs < 1 || n_seqs > n_slots) { snprintf(err, err_cap, "%s: n_seqs (%d) outside 1 .. %d, the handle's KV slots (llamahip_opts.n_seq)", fn, n_seqs, n_slots); return LLAMAHIP_ERR_PREDICT; }
    if (!slots || !n_past || !tokens || !n_tokens) { snprintf(err, err_cap, "%s: null slots, n_past, tokens or n_tokens", fn); return LLAMAHIP_ERR_PREDICT; }
    if (chunk_tokens < 0) { snprintf(err, err_cap, "%s: chunk_tokens (%d) must be >= 0 (0 = one eval per segment)", fn, chunk_tokens); return LLAMAHIP_ERR_PREDICT; }
    std::vector<char> seen((size_t) n_slots, 0);
    int64_t R = 0;
    for (int32_t i = 0; i < n_seqs; i++) {
        if (slots[i] < 0 || slots[i] >= n_slots) { snprintf(err, err_cap, "%s: slots[%d] = %d out of range [0, %d)", fn, i, slots[i], n_slots); return LLAMAHIP_ERR_PREDICT; }
        if (seen[slots[i]]) { snprintf(err, err_cap, "%s: slot %d is named twice (slots[%d]): one segment per KV slot", fn, slots[i], i); return LLAMAHIP_ERR_PREDICT; }
        seen[slots[i]] = 1;
        if (n_tokens[i] < 1) { snprintf(err, err_cap, "%s: n_tokens[%d] must be >= 1 (got %d)", fn, i, n_tokens[i]); return LLAMAHIP_ERR_PREDICT; }
        if (n_past[i] < 0 || (int64_t) n_past[i] + n_tokens[i] > n_ctx) {
            snprintf(err, err_cap, "%s: context overflow in segment %d: n_past (%d) + n_tokens (%d) > n_ctx (%d)", fn, i, n_past[i], n_tokens[i], n_ctx);
            return LLAMAHIP_ERR_PREDICT;
        }
        R += n_tokens[i];
    }
    for (int64_t r = 0; r < R; r++)
        if (tokens[r] < 0 || tokens[r] >= n_vocab) { snprintf(err, err_cap, "%s: token id %d at %lld out of range [0, %d)", fn, tokens[r], (long long) r, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (R > LLAMAHIP_EVAL_MULTI_MAX_ROWS) { snprintf(err, err_cap, "%s: %lld rows in all, more than LLAMAHIP_EVAL_MULTI_MAX_ROWS (%d)", fn, (long long) R, LLAMAHIP_EVAL_MULTI_MAX_ROWS); return LLAMAHIP_ERR_PREDICT; }
    return 0;
}
int eval_multi_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, int32_t n_seqs, const int32_t *slots, const int32_t *n_past,
                     const int32_t *tokens, const int32_t *n_tokens, int32_t chunk_tokens, char *err, size_t err_cap) {
    return segments_check("llamahip_eval_multi", n_ctx, n_vocab, n_slots, n_seqs, slots, n_past, tokens, n_tokens, chunk_tokens, err, err_cap);
}

// what llamahip_eval_logprobs_multi refuses of its arguments: eval_multi_check's rules, and a target (targets may be null) outside [-1, n_vocab)
int score_multi_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, int32_t n_seqs, const int32_t *slots, const int32_t *n_past,
                      const int32_t *tokens, const int32_t *n_tokens, int32_t chunk_tokens, const int32_t *targets, char *err, size_t err_cap) {
    static const char *fn = "llamahip_eval_logprobs_multi";
    const int rc = segments_check(fn, n_ctx, n_vocab, n_slots, n_seqs, slots, n_past, tokens, n_tokens, chunk_tokens, err, err_cap);
    if (rc || !targets) return rc;
    if (!err) err_cap = 0;
    int64_t r = 0;
    for (int32_t i = 0; i < n_seqs; i++)
        for (int32_t j = 0; j < n_tokens[i]; j++, r++)
            if (targets[r] < -1 || targets[r] >= n_vocab) {
                snprintf(err, err_cap, "%s: target %d of row %lld (row %d of segment %d) out of range [-1, %d)", fn, targets[r], (long long) r, j, i, n_vocab);
                return LLAMAHIP_ERR_PREDICT;
            }
    return 0;
}

// the targets of the R rows of checked segments resolved (targets null: the next token inside the row's segment, the segment's last row -1)
// into tgt [R], and the scored rows in ascending row order into scored (at most R entries): returns their count
int32_t score_multi_rows(int32_t n_seqs, const int32_t *tokens, const int32_t *n_tokens, const int32_t *targets, int32_t *tgt, int32_t *scored) {
    int32_t r = 0, nl = 0;
    for (int32_t i = 0; i < n_seqs; i++)
        for (int32_t j = 0; j < n_tokens[i]; j++, r++) {
            tgt[r] = targets ? targets[r] : j + 1 < n_tokens[i] ? tokens[r + 1] : -1;
            if (tgt[r] >= 0) scored[nl++] = r;
        }
    return nl;
}

// k_row_logprob's results of the nl scored rows -- packed: [nl] logprob (double) | [nl] argmax | [nl] rank, 16 nl bytes -- back to row order;
// an unscored row reports 0.0 / -1 / -1.  Any output may be null.
void score_scatter(int32_t R, int32_t nl, const int32_t *scored, const void *packed, double *lp, int32_t *am, int32_t *rk) {
    for (int32_t r = 0; r < R; r++) { if (lp) lp[r] = 0.0; if (am) am[r] = -1; if (rk) rk[r] = -1; }
    const char *p = (const char *) packed;
    for (int32_t k = 0; k < nl; k++) {
        const int32_t r = scored[k];
        if (lp) memcpy(&lp[r], p + (size_t) k * 8, 8);
        if (am) memcpy(&am[r], p + (size_t) nl * 8 + (size_t) k * 4, 4);
        if (rk) memcpy(&rk[r], p + (size_t) nl * 12 + (size_t) k * 4, 4);
    }
}

// what llamahip_score_choices refuses of its arguments
int score_choices_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, const int32_t *context, int32_t n_context, int32_t n_choices,
                        const int32_t *endings, const int32_t *n_ending, int32_t chunk_tokens, char *err, size_t err_cap) {
    static const char *fn = "llamahip_score_choices";
    if (!err) err_cap = 0;
    const int32_t max_choices = std::min(LLAMAHIP_SCORE_CHOICES_MAX, n_slots);
    if (n_context < 1) { snprintf(err, err_cap, "%s: n_context (%d) must be >= 1: the last context token predicts an ending's first", fn, n_context); return LLAMAHIP_ERR_PREDICT; }
    if (n_choices < 1 || n_choices > max_choices) {
        snprintf(err, err_cap, "%s: n_choices (%d) outside 1 .. %d (LLAMAHIP_SCORE_CHOICES_MAX %d, the handle's KV slots %d: llamahip_opts.n_seq)", fn, n_choices, max_choices, LLAMAHIP_SCORE_CHOICES_MAX, n_slots);
        return LLAMAHIP_ERR_PREDICT;
    }
    if (!context || !endings || !n_ending) { snprintf(err, err_cap, "%s: null context, endings or n_ending", fn); return LLAMAHIP_ERR_PREDICT; }
    if (chunk_tokens < 0) { snprintf(err, err_cap, "%s: chunk_tokens (%d) must be >= 0 (0 = one eval of the context)", fn, chunk_tokens); return LLAMAHIP_ERR_PREDICT; }
    int64_t E = 0;
    for (int32_t i = 0; i < n_choices; i++) {
        if (n_ending[i] < 1) { snprintf(err, err_cap, "%s: n_ending[%d] must be >= 1 (got %d)", fn, i, n_ending[i]); return LLAMAHIP_ERR_PREDICT; }
        if ((int64_t) n_context - 1 + n_ending[i] > n_ctx) {
            snprintf(err, err_cap, "%s: context overflow in choice %d: n_context - 1 (%d) + n_ending (%d) > n_ctx (%d)", fn, i, n_context - 1, n_ending[i], n_ctx);
            return LLAMAHIP_ERR_PREDICT;
        }
        E += n_ending[i];
    }
    for (int32_t i = 0; i < n_context; i++)
        if (context[i] < 0 || context[i] >= n_vocab) { snprintf(err, err_cap, "%s: context token id %d at %d out of range [0, %d)", fn, context[i], i, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    for (int64_t r = 0; r < E; r++)
        if (endings[r] < 0 || endings[r] >= n_vocab) { snprintf(err, err_cap, "%s: ending token id %d at %lld out of range [0, %d)", fn, endings[r], (long long) r, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (E > LLAMAHIP_EVAL_MULTI_MAX_ROWS) { snprintf(err, err_cap, "%s: %lld ending rows in all, more than LLAMAHIP_EVAL_MULTI_MAX_ROWS (%d)", fn, (long long) E, LLAMAHIP_EVAL_MULTI_MAX_ROWS); return LLAMAHIP_ERR_PREDICT; }
    return 0;
}

// what llamahip_text_embedding_multi (fn names it; llamahip_text_embedding: its one segment on the current slot) refuses of its arguments:
// eval_multi_check's rules, pool / normalize outside {0, 1}, a null out, and a named slot that a live scheduler owns (sched_max_active: the
// slots [0, max_active) of the handle's scheduler, 0 = none)
int embed_check(const char *fn, int32_t n_ctx, int32_t n_vocab, int32_t n_slots, int32_t sched_max_active, int32_t n_seqs, const int32_t *slots,
                const int32_t *n_past, const int32_t *tokens, const int32_t *n_tokens, int32_t chunk_tokens, int32_t pool, int32_t normalize,
                const float *out, char *err, size_t err_cap) {
    const int rc = segments_check(fn, n_ctx, n_vocab, n_slots, n_seqs, slots, n_past, tokens, n_tokens, chunk_tokens, err, err_cap);
    if (rc) return rc;
    if (!err) err_cap = 0;
    if (pool != LLAMAHIP_POOL_LAST && pool != LLAMAHIP_POOL_MEAN) { snprintf(err, err_cap, "%s: pool (%d) must be LLAMAHIP_POOL_LAST (0) or LLAMAHIP_POOL_MEAN (1)", fn, pool); return LLAMAHIP_ERR_PREDICT; }
    if (normalize != 0 && normalize != 1) { snprintf(err, err_cap, "%s: normalize (%d) must be 0 or 1", fn, normalize); return LLAMAHIP_ERR_PREDICT; }
    if (!out) { snprintf(err, err_cap, "%s: null out", fn); return LLAMAHIP_ERR_PREDICT; }
    for (int32_t i = 0; i < n_seqs; i++)
        if (slots[i] < sched_max_active) {
            snprintf(err, err_cap, "%s: slot %d (slots[%d]) belongs to the handle's live scheduler, which owns KV slots 0 .. %d: name a slot from %d, or free it first", fn, slots[i], i, sched_max_active - 1, sched_max_active);
            return LLAMAHIP_ERR_PREDICT;
        }
    return 0;
}

// what llamahip_op_pool_rows refuses of its arguments
int pool_rows_check(const float *x, int32_t R, int32_t d, const float *norm_w, const int32_t *seg_begin, int32_t n_segs, int32_t pool, int32_t normalize,
                    const float *out, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_pool_rows";
    if (!err) err_cap = 0;
    if (!x || !norm_w || !seg_begin || !out) { snprintf(err, err_cap, "%s: null x, norm_w, seg_begin or out", fn); return LLAMAHIP_ERR_PREDICT; }
    if (R < 1 || R > LLAMAHIP_EVAL_MULTI_MAX_ROWS) { snprintf(err, err_cap, "%s: R (%d) outside 1 .. LLAMAHIP_EVAL_MULTI_MAX_ROWS (%d)", fn, R, LLAMAHIP_EVAL_MULTI_MAX_ROWS); return LLAMAHIP_ERR_PREDICT; }
    if (d < 32 || d % 32 != 0) { snprintf(err, err_cap, "%s: d (%d) must be a multiple of 32, at least 32", fn, d); return LLAMAHIP_ERR_PREDICT; }
    if (n_segs < 1 || n_segs > LLAMAHIP_POOL_MAX_SEGS) { snprintf(err, err_cap, "%s: n_segs (%d) outside 1 .. LLAMAHIP_POOL_MAX_SEGS (%d)", fn, n_segs, LLAMAHIP_POOL_MAX_SEGS); return LLAMAHIP_ERR_PREDICT; }
    if (pool != LLAMAHIP_POOL_LAST && pool != LLAMAHIP_POOL_MEAN) { snprintf(err, err_cap, "%s: pool (%d) must be LLAMAHIP_POOL_LAST (0) or LLAMAHIP_POOL_MEAN (1)", fn, pool); return LLAMAHIP_ERR_PREDICT; }
    if (normalize != 0 && normalize != 1) { snprintf(err, err_cap, "%s: normalize (%d) must be 0 or 1", fn, normalize); return LLAMAHIP_ERR_PREDICT; }
    if (seg_begin[0] != 0 || seg_begin[n_segs] != R) { snprintf(err, err_cap, "%s: seg_begin must run from 0 to R (%d): seg_begin[0] = %d, seg_begin[%d] = %d", fn, R, seg_begin[0], n_segs, seg_begin[n_segs]); return LLAMAHIP_ERR_PREDICT; }
    for (int32_t s = 0; s < n_segs; s++)
        if (seg_begin[s + 1] <= seg_begin[s]) { snprintf(err, err_cap, "%s: seg_begin must rise strictly: seg_begin[%d] = %d, seg_begin[%d] = %d", fn, s, seg_begin[s], s + 1, seg_begin[s + 1]); return LLAMAHIP_ERR_PREDICT; }
    return 0;
}

// what llamahip_op_attention_rows refuses of a caller's table: every entry inside its cache, and the rows of one slot one run of consecutive
// positions in ascending row order whose key counts stay inside what the run appends (the masked tail of V*P reads those rows)
int rows_table_check(int32_t R, int32_t n_ctx, int32_t n_slots, const int32_t *row_slot, const int32_t *row_pos, const int32_t *row_keys,
                     char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_attention_rows";
    if (!err) err_cap = 0;
    if (R < 1 || R > LLAMAHIP_EVAL_MULTI_MAX_ROWS) { snprintf(err, err_cap, "%s: R (%d) outside 1 .. LLAMAHIP_EVAL_MULTI_MAX_ROWS (%d)", fn, R, LLAMAHIP_EVAL_MULTI_MAX_ROWS); return LLAMAHIP_ERR_PREDICT; }
    if (n_ctx < 1 || n_slots < 1) { snprintf(err, err_cap, "%s: n_ctx (%d) and n_slots (%d) must be >= 1", fn, n_ctx, n_slots); return LLAMAHIP_ERR_PREDICT; }
    if (!row_slot || !row_pos || !row_keys) { snprintf(err, err_cap, "%s: null row_slot, row_pos or row_keys", fn); return LLAMAHIP_ERR_PREDICT; }
    std::vector<char> closed((size_t) n_slots, 0);
    for (int32_t r = 0; r < R;) {
        const int32_t s = row_slot[r];
        if (s < 0 || s >= n_slots) { snprintf(err, err_cap, "%s: row_slot[%d] = %d out of range [0, %d)", fn, r, s, n_slots); return LLAMAHIP_ERR_PREDICT; }
        if (closed[s]) { snprintf(err, err_cap, "%s: the rows of slot %d are not consecutive (row %d)", fn, s, r); return LLAMAHIP_ERR_PREDICT; }
        closed[s] = 1;
        int32_t e = r;
        while (e < R && row_slot[e] == s) {
            if (row_pos[e] < 0 || row_pos[e] >= n_ctx) { snprintf(err, err_cap, "%s: row_pos[%d] = %d out of range [0, n_ctx = %d)", fn, e, row_pos[e], n_ctx); return LLAMAHIP_ERR_PREDICT; }
            if (e > r && row_pos[e] != row_pos[e - 1] + 1) {
                snprintf(err, err_cap, "%s: the rows of slot %d must be consecutive positions in ascending row order (row %d at %d follows %d)", fn, s, e, row_pos[e], row_pos[e - 1]);
                return LLAMAHIP_ERR_PREDICT;
            }
            e++;
        }
        const int32_t end = row_pos[e - 1] + 1;          // the run appends positions [row_pos[r], end)
        for (int32_t q = r; q < e; q++)
            if (row_keys[q] <= row_pos[q] || row_keys[q] > end || row_keys[q] > n_ctx) {
                snprintf(err, err_cap, "%s: row_keys[%d] = %d outside (row_pos = %d, %d], the end of slot %d's rows (n_ctx %d)", fn, q, row_keys[q], row_pos[q], end, s, n_ctx);
                return LLAMAHIP_ERR_PREDICT;
            }
        r = e;
    }
    return 0;
}

}  // namespace lh

extern "C" int32_t llamahip_eval_multi_rows(int32_t n_ctx, int32_t n_seqs, const int32_t *n_past, const int32_t *n_tokens, int32_t chunk_tokens,
                                            int32_t *row_seg, int32_t *row_pos, int32_t *row_keys) {
    if (n_ctx < 1 || n_seqs < 1 || !n_past || !n_tokens || chunk_tokens < 0) return -1;
    int64_t R = 0;
    for (int32_t i = 0; i < n_seqs; i++) {
        if (n_tokens[i] < 1 || n_past[i] < 0 || (int64_t) n_past[i] + n_tokens[i] > n_ctx) return -1;
        R += n_tokens[i];
    }
    if (R > LLAMAHIP_EVAL_MULTI_MAX_ROWS) return -1;
    int32_t r = 0;
    for (int32_t i = 0; i < n_seqs; i++)
        for (int32_t j = 0; j < n_tokens[i]; j++, r++) {
            if (row_seg) row_seg[r] = i;
            if (row_pos) row_pos[r] = n_past[i] + j;
            if (row_keys) row_keys[r] = lh::split_keys_host(n_past[i], n_tokens[i], j, chunk_tokens);
        }
    return r;
}
