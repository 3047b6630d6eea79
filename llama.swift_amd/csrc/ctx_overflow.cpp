// ctx_overflow.cpp -- generating past the context window (include/llamahip.h): the one rule for what to drop when the KV cache is full
// (llamahip_ctx_overflow_plan) and the device-resident greedy loop run in legs around it (llamahip_decode_greedy_window).  Pure host
// code above the C ABI: the legs are llamahip_decode_greedy calls, the wall is crossed by llamahip_eval / llamahip_eval_chunks of the
// surviving tail (LLAMAHIP_CTX_REEVAL) or by llamahip_kv_shift_rows of the surviving rows (LLAMAHIP_CTX_SHIFT, not the reference's arithmetic).
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/llamahip.h"

namespace lh {
// llamahip.cpp: what llamahip_decode_greedy refuses of a HANDLE (null, HOST_ONLY, a pipeline-stage handle), without touching a device
int decode_handle_check(const llamahip_model *m, const char *fn, char *err, size_t err_cap);
}

extern "C" int32_t llamahip_ctx_overflow_plan(int32_t n_ctx, int32_t n_past, int32_t n_keep, int32_t *n_discard) {
    if (n_discard) *n_discard = 0;
    if (n_ctx < 1 || n_past < 0 || n_past > n_ctx || n_keep < 0 || n_keep > n_past) return -1;
    const int32_t nd = (n_past - n_keep) / 2;
    if (nd < 1) return -1;
    if (n_discard) *n_discard = nd;
    return n_past - nd;
}

extern "C" int llamahip_decode_greedy_window(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token, int32_t n_steps,
                                             const int32_t *context, int32_t n_context, int32_t n_keep, int32_t mode, int32_t chunk_tokens,
                                             int32_t *out_tokens, float *logits_last, int32_t *n_past_out, char *err, size_t err_cap) {
    static const char *fn = "llamahip_decode_greedy_window";
    if (!err) err_cap = 0;
    if (!m) { snprintf(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    const int32_t C = llamahip_n_ctx(m), V = llamahip_n_vocab(m);
    if (mode != LLAMAHIP_CTX_REEVAL && mode != LLAMAHIP_CTX_SHIFT) { snprintf(err, err_cap, "%s: mode %d is not LLAMAHIP_CTX_REEVAL (1) or LLAMAHIP_CTX_SHIFT (4)", fn, mode); return LLAMAHIP_ERR_PREDICT; }
    if (n_steps < 1 || !out_tokens) { snprintf(err, err_cap, "%s: n_steps (%d) must be >= 1 and out_tokens non-null", fn, n_steps); return LLAMAHIP_ERR_PREDICT; }
    if (n_past < 0 || n_past > C) { snprintf(err, err_cap, "%s: n_past (%d) outside [0, n_ctx = %d]", fn, n_past, C); return LLAMAHIP_ERR_PREDICT; }
    if (n_context != n_past || (n_context > 0 && !context)) { snprintf(err, err_cap, "%s: n_context (%d) must equal n_past (%d): context holds the tokens at positions [0, n_past)", fn, n_context, n_past); return LLAMAHIP_ERR_PREDICT; }
    if (first_token < 0 || first_token >= V) { snprintf(err, err_cap, "%s: token id %d out of range [0, %d)", fn, first_token, V); return LLAMAHIP_ERR_PREDICT; }
    for (int32_t i = 0; i < n_context; i++)
        if (context[i] < 0 || context[i] >= V) { snprintf(err, err_cap, "%s: context token id %d at %d out of range [0, %d)", fn, context[i], i, V); return LLAMAHIP_ERR_PREDICT; }
    if (chunk_tokens < 0) { snprintf(err, err_cap, "%s: chunk_tokens (%d) must be >= 0 (0 = one eval)", fn, chunk_tokens); return LLAMAHIP_ERR_PREDICT; }
    int32_t nd = 0;
    if (n_keep < 0 || llamahip_ctx_overflow_plan(C, C, n_keep, &nd) < 0) { snprintf(err, err_cap, "%s: n_keep (%d) leaves nothing to discard at n_ctx %d (0 <= n_keep <= n_ctx - 2)", fn, n_keep, C); return LLAMAHIP_ERR_PREDICT; }
    int rc = lh::decode_handle_check(m, fn, err, err_cap);
    if (rc) return rc;

    // toks: the tokens at positions [0, pos); `pending` is the token at pos, not evaluated yet
    std::vector<int32_t> toks(context, context + n_context);
    int32_t pos = n_past, pending = first_token, done = 0;
    while (done < n_steps) {
        if (pos == C) {
            // the pending token has no room: keep [0, n_keep), drop the older half of the rest (the plan), go on
            const int32_t np = llamahip_ctx_overflow_plan(C, pos, n_keep, &nd);
            if (np < 0) { snprintf(err, err_cap, "%s: nothing to discard at position %d with n_keep %d", fn, pos, n_keep); return LLAMAHIP_ERR_PREDICT; }
            const int32_t *tail = toks.data() + n_keep + nd, M = pos - n_keep - nd;
            if (mode == LLAMAHIP_CTX_SHIFT) {
                // in place: the surviving rows move down by nd positions, the keys re-rotated; nothing is evaluated
                const int32_t slot = llamahip_cur_seq(m), row_begin = n_keep + nd;
                rc = llamahip_kv_shift_rows(m, 1, &slot, &row_begin, &M, &nd, err, err_cap);
            } else
                rc = chunk_tokens > 0 ? llamahip_eval_chunks(m, n_threads, n_keep, tail, M, chunk_tokens, nullptr, err, err_cap)
                                      : llamahip_eval(m, n_threads, n_keep, tail, M, nullptr, err, err_cap);
            if (rc) return rc;
            toks.erase(toks.begin() + n_keep, toks.begin() + n_keep + nd);
            pos = np;
        }
        const int32_t leg = std::min(n_steps - done, C - pos);
        rc = llamahip_decode_greedy(m, n_threads, pos, pending, leg, out_tokens + done, done + leg == n_steps ? logits_last : nullptr, err, err_cap);
        if (rc) return rc;
        toks.push_back(pending);                                              // positions [pos, pos + leg): the pending token, then all picks but the last
        toks.insert(toks.end(), out_tokens + done, out_tokens + done + leg - 1);
        pending = out_tokens[done + leg - 1];
        pos += leg;
        done += leg;
    }
    if (n_past_out) *n_past_out = pos;
    return LLAMAHIP_OK;
}
