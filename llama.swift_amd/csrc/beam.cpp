// beam.cpp -- the host half of llamahip_beam_search (include/llamahip.h): the step rule (llamahip_beam_select), the slots of a step's beams and
// the KV copies they need (llamahip_beam_slots), what the entry point refuses of its arguments (beam_check) and the ranking of the finished
// hypotheses (beam_rank).  The device loop that calls them is llamahip.cpp's.
// Pure host code, no device, no handle: tools/host_sanitize runs it under ASan + UBSan.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/llamahip.h"

extern "C" {

// One step's walk: see llamahip.h.  The step rule lives here and nowhere else.
int32_t llamahip_beam_select(int32_t n_live, const double *live_score, int32_t n_cand, const int32_t *cand_ids, const double *cand_logprob,
                             int32_t n_beams, int32_t stop_token, int32_t *new_parent, int32_t *new_token, double *new_score, int32_t *n_new,
                             int32_t *fin_parent, double *fin_score, int32_t *n_fin, int32_t *n_dead) {
    if (n_live < 0 || n_live > LLAMAHIP_BEAM_MAX || n_cand < 1 || n_cand > 2 * LLAMAHIP_BEAM_MAX || n_beams < 1 || n_beams > LLAMAHIP_BEAM_MAX) return LLAMAHIP_ERR_PREDICT;
    if (!new_parent || !new_token || !new_score || !n_new || !fin_parent || !fin_score || !n_fin) return LLAMAHIP_ERR_PREDICT;
    if (n_live > 0 && (!live_score || !cand_ids || !cand_logprob)) return LLAMAHIP_ERR_PREDICT;
    struct Cand { int32_t i, v; double c; };
    std::vector<Cand> cs;
    cs.reserve((size_t) n_live * n_cand);
    int32_t dead = 0;
    for (int32_t i = 0; i < n_live; i++) {
        const int32_t *ids = cand_ids + (size_t) i * n_cand;
        const double *lp = cand_logprob + (size_t) i * n_cand;
        if (ids[0] < 0) { dead++; continue; }          // a non-finite row (k_row_topn: every id -1) offers nothing
        for (int32_t j = 0; j < n_cand; j++) {
            const double c = live_score[i] + lp[j];
            if (ids[j] < 0 || c != c) continue;
            cs.push_back({ i, ids[j], c });
        }
    }
    std::stable_sort(cs.begin(), cs.end(), [](const Cand &a, const Cand &b) {
        if (a.c != b.c) return a.c > b.c;
        if (a.i != b.i) return a.i < b.i;
        return a.v < b.v;
    });
    int32_t nn = 0, nf = 0;
    for (size_t k = 0; k < cs.size() && nn < n_beams; k++) {
        const Cand &c = cs[k];
        if (stop_token >= 0 && c.v == stop_token) { fin_parent[nf] = c.i; fin_score[nf] = c.c; nf++; }      // (at most one per live beam)
        else { new_parent[nn] = c.i; new_token[nn] = c.v; new_score[nn] = c.c; nn++; }
    }
    *n_new = nn; *n_fin = nf;
    if (n_dead) *n_dead = dead;
    return LLAMAHIP_OK;
}

// The slots of a step's new beams and the copies: see llamahip.h.  Returns the number of copies, -1 for arguments it refuses.
int32_t llamahip_beam_slots(int32_t n_prev, const int32_t *prev_slot, int32_t n_new, const int32_t *parent, int32_t n_beams,
                            int32_t *new_slot, int32_t *copy_src, int32_t *copy_dst) {
    if (n_beams < 1 || n_beams > LLAMAHIP_BEAM_MAX || n_prev < 0 || n_prev > n_beams || n_new < 0 || n_new > n_beams) return -1;
    if ((n_prev > 0 && !prev_slot) || (n_new > 0 && (!parent || !new_slot || !copy_src || !copy_dst))) return -1;
    bool used[LLAMAHIP_BEAM_MAX] = { false }, kept[LLAMAHIP_BEAM_MAX] = { false }, has_child[LLAMAHIP_BEAM_MAX] = { false };
    for (int32_t i = 0; i < n_prev; i++) {
        if (prev_slot[i] < 0 || prev_slot[i] >= n_beams || used[prev_slot[i]]) return -1;
        used[prev_slot[i]] = true;
    }
    for (int32_t k = 0; k < n_new; k++) {
        if (parent[k] < 0 || parent[k] >= n_prev) return -1;
        kept[prev_slot[parent[k]]] = true;
    }
    int32_t nc = 0, next_free = 0;
    for (int32_t k = 0; k < n_new; k++) {
        const int32_t p = parent[k], ps = prev_slot[p];
        if (!has_child[p]) { has_child[p] = true; new_slot[k] = ps; continue; }
        while (next_free < n_beams && kept[next_free]) next_free++;
        if (next_free >= n_beams) return -1;          // (cannot happen: n_new <= n_beams)
        new_slot[k] = next_free;
        copy_src[nc] = ps; copy_dst[nc] = next_free; nc++;
        next_free++;
    }
    return nc;
}

}  // extern "C"

namespace lh {

// what llamahip_beam_search refuses of its ARGUMENTS (the handle is the caller's business): 0, or LLAMAHIP_ERR_PREDICT with the limit in err
int beam_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, const llamahip_beam_opts *o, const int32_t *prompt, int32_t n_prompt,
               const void *hyps_out, const void *tokens_out, const void *n_hyps_out, char *err, size_t err_cap) {
    static const char *fn = "llamahip_beam_search";
    if (!err) err_cap = 0;
    if (!o || o->struct_size < (int32_t) sizeof(llamahip_beam_opts)) { snprintf(err, err_cap, "%s: opts is NULL or its struct_size is below %d", fn, (int) sizeof(llamahip_beam_opts)); return LLAMAHIP_ERR_PREDICT; }
    if (!prompt || !hyps_out || !tokens_out || !n_hyps_out) {
        snprintf(err, err_cap, "%s: %s is NULL", fn, !prompt ? "prompt" : !hyps_out ? "hyps_out" : !tokens_out ? "tokens_out" : "n_hyps_out"); return LLAMAHIP_ERR_PREDICT; }
    if (o->n_beams < 1 || o->n_beams > LLAMAHIP_BEAM_MAX) { snprintf(err, err_cap, "%s: n_beams %d outside 1 .. %d", fn, o->n_beams, LLAMAHIP_BEAM_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (o->n_beams > n_slots) { snprintf(err, err_cap, "%s: n_beams %d on a handle with %d KV slots (llamahip_opts.n_seq)", fn, o->n_beams, n_slots); return LLAMAHIP_ERR_PREDICT; }
    if (2 * o->n_beams > n_vocab) { snprintf(err, err_cap, "%s: 2 * n_beams (%d) candidates per row > n_vocab (%d)", fn, 2 * o->n_beams, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (n_prompt < 1) { snprintf(err, err_cap, "%s: n_prompt must be >= 1 (got %d)", fn, n_prompt); return LLAMAHIP_ERR_PREDICT; }
    if (o->n_predict < 1) { snprintf(err, err_cap, "%s: n_predict must be >= 1 (got %d)", fn, o->n_predict); return LLAMAHIP_ERR_PREDICT; }
    if ((int64_t) n_prompt + o->n_predict > n_ctx) { snprintf(err, err_cap, "%s: context overflow: n_prompt (%d) + n_predict (%d) > n_ctx (%d)", fn, n_prompt, o->n_predict, n_ctx); return LLAMAHIP_ERR_PREDICT; }
    for (int32_t i = 0; i < n_prompt; i++)
        if (prompt[i] < 0 || prompt[i] >= n_vocab) { snprintf(err, err_cap, "%s: token id %d at %d out of range [0, %d)", fn, prompt[i], i, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (o->stop_token < -1 || o->stop_token >= n_vocab) { snprintf(err, err_cap, "%s: stop_token %d out of range [-1, %d)", fn, o->stop_token, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (o->n_return < 0 || o->n_return > o->n_beams) { snprintf(err, err_cap, "%s: n_return %d outside 0 .. n_beams (%d)", fn, o->n_return, o->n_beams); return LLAMAHIP_ERR_PREDICT; }
    if (o->chunk_tokens < 0) { snprintf(err, err_cap, "%s: chunk_tokens must be >= 0 (0 = one eval; got %d)", fn, o->chunk_tokens); return LLAMAHIP_ERR_PREDICT; }
    if (o->length_norm != 0 && o->length_norm != 1) { snprintf(err, err_cap, "%s: length_norm must be 0 or 1 (got %d)", fn, o->length_norm); return LLAMAHIP_ERR_PREDICT; }
    return 0;
}

// the finished list's ranking: order[k] = the entry of rank k.  By S (length_norm 0) or S / length as one IEEE double division (1), descending;
// ties go to the earlier entry
void beam_rank(int32_t n, const double *score, const int32_t *length, int32_t length_norm, int32_t *order) {
    std::vector<double> key((size_t) n);
    for (int32_t k = 0; k < n; k++) { key[k] = length_norm ? score[k] / (double) length[k] : score[k]; order[k] = k; }
    std::stable_sort(order, order + n, [&](int32_t a, int32_t b) { return key[a] > key[b]; });
}

}  // namespace lh
