// constrain.cpp -- the host half of constrained decoding (include/llamahip.h): the lift of a byte automaton to the model's
// tokens, the prune that leaves every reachable state a token to go on with, the choices builder (a trie is a byte automaton), and the host
// statements of what the device kernels compute (constrain.hip): advance, pick, mask_row.
// Pure host code: the handle is read through llamahip_n_vocab / llamahip_token_text alone.  tools/host_sanitize runs it under ASan + UBSan.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "constrain.h"

using lh::DFA_BANNED;

namespace lh {

int32_t dfa_pick_row(const uint16_t *row, int32_t n_vocab, const float *logits) {
    float best = -INFINITY;
    int32_t idx = -1, lowest = -1;
    for (int32_t i = 0; i < n_vocab; i++) {
        if (row[i] == DFA_BANNED) continue;
        if (lowest < 0) lowest = i;
        const float v = logits[i];
        if (v > best || (v == best && idx < 0)) { best = v; idx = i; }      // ascending i: a tie keeps the lower index; a NaN is never taken
    }
    return idx >= 0 ? idx : lowest;                                        // every allowed entry a NaN: the lowest allowed index
}

}  // namespace lh

#define REFUSE(...) do { snprintf(err, err_cap, __VA_ARGS__); return LLAMAHIP_ERR_PREDICT; } while (0)

extern "C" {

int llamahip_constraint_new(const llamahip_model *m, int32_t n_states, const int32_t *trans, const uint8_t *accept, int32_t start, int32_t stop_token,
                            llamahip_constraint **out, char *err, size_t err_cap) {
    static const char *fn = "llamahip_constraint_new";
    if (!err) err_cap = 0;
    if (out) *out = nullptr;
    if (!m || !trans || !accept || !out) REFUSE("%s: %s is NULL", fn, !m ? "model" : !trans ? "trans" : !accept ? "accept" : "out");
    if (n_states < 1 || n_states > lh::DFA_STATES_MAX) REFUSE("%s: n_states %d outside 1 .. %d", fn, n_states, lh::DFA_STATES_MAX);
    const int32_t V = llamahip_n_vocab(m), S = n_states, DONE = n_states;
    if (V < 1) REFUSE("%s: the handle has no vocabulary", fn);
    const size_t bytes = (size_t) (S + 1) * (size_t) V * 2;
    if (bytes > lh::DFA_TABLE_BYTES_MAX)
        REFUSE("%s: table of (%d + 1) states x %d tokens x 2 bytes = %zu bytes over the limit of %zu (256 MiB)", fn, S, V, bytes, lh::DFA_TABLE_BYTES_MAX);
    for (size_t i = 0; i < (size_t) S * 256; i++)
        if (trans[i] < -1 || trans[i] >= S) REFUSE("%s: trans[%zu][%zu] = %d outside [-1, %d)", fn, i / 256, i % 256, trans[i], S);
    if (start < 0 || start >= S) REFUSE("%s: start %d out of range [0, %d)", fn, start, S);
    if (stop_token < 0 || stop_token >= V) REFUSE("%s: stop_token %d out of range [0, %d)", fn, stop_token, V);
    bool any = false;
    for (int32_t s = 0; s < S; s++) any = any || accept[s] != 0;
    if (!any) REFUSE("%s: no accepting state among the %d", fn, S);

    llamahip_constraint *c = new (std::nothrow) llamahip_constraint();
    if (!c) REFUSE("%s: out of memory", fn);
    c->m = m; c->n_states = S + 1; c->n_vocab = V; c->start = start; c->stop_token = stop_token;
    try { c->next.assign((size_t) (S + 1) * V, DFA_BANNED); } catch (const std::bad_alloc &) { delete c; REFUSE("%s: out of memory (%zu bytes)", fn, bytes); }
    uint16_t *next = c->next.data();
    // the lift: token t from state s = the walk of its bytes; an empty text adds no bytes and is banned everywhere; the stop token is
    // allowed exactly in accepting states and leads to DONE, whatever its text
    for (int32_t t = 0; t < V; t++) {
        if (t == stop_token) continue;
        uint32_t len = 0;
        const uint8_t *text = (const uint8_t *) llamahip_token_text(m, t, &len);
        if (!text || len == 0) continue;
        for (int32_t s = 0; s < S; s++) {
            int32_t q = s;
            for (uint32_t k = 0; k < len && q >= 0; k++) q = trans[(size_t) q * 256 + text[k]];
            if (q >= 0) next[(size_t) s * V + t] = (uint16_t) q;
        }
    }
    for (int32_t s = 0; s < S; s++) if (accept[s]) next[(size_t) s * V + stop_token] = (uint16_t) DONE;
    next[(size_t) DONE * V + stop_token] = (uint16_t) DONE;
    // the prune: live = accepting, or a token away from a live state -- the least fixed point, walked backwards from the accepting states
    std::vector<std::vector<int32_t>> preds((size_t) S);
    {
        std::vector<int32_t> mark((size_t) S, -1);
        for (int32_t s = 0; s < S; s++)
            for (int32_t t = 0; t < V; t++) {
                const uint16_t q = next[(size_t) s * V + t];
                if (q == DFA_BANNED || q >= S || mark[q] == s) continue;
                mark[q] = s;
                preds[q].push_back(s);
            }
    }
    std::vector<uint8_t> live((size_t) S + 1, 0);
    std::vector<int32_t> work;
    for (int32_t s = 0; s < S; s++) if (accept[s]) { live[s] = 1; work.push_back(s); }
    live[DONE] = 1;
    while (!work.empty()) {
        const int32_t q = work.back();
        work.pop_back();
        for (int32_t s : preds[q]) if (!live[s]) { live[s] = 1; work.push_back(s); }
    }
    if (!live[start]) { delete c; REFUSE("%s: start state %d is not live: no sequence of tokens leads from it to an accepting state", fn, start); }
    // ... and, in the same walk, every state's single allowed token (-1: none allowed, -2: more than one) for llamahip_forced_run
    try { c->single.assign((size_t) S + 1, -1); } catch (const std::bad_alloc &) { delete c; REFUSE("%s: out of memory", fn); }
    for (int32_t s = 0; s < S; s++)
        for (int32_t t = 0; t < V; t++) {
            uint16_t &q = next[(size_t) s * V + t];
            if (q != DFA_BANNED && !live[q]) q = DFA_BANNED;
            if (q != DFA_BANNED) c->single[(size_t) s] = c->single[(size_t) s] == -1 ? t : -2;
        }
    *out = c;
    return LLAMAHIP_OK;
}

int llamahip_constraint_new_choices(const llamahip_model *m, const uint8_t *const *strings, const int32_t *lens, int32_t n, int32_t stop_token,
                                    llamahip_constraint **out, char *err, size_t err_cap) {
    static const char *fn = "llamahip_constraint_new_choices";
    if (!err) err_cap = 0;
    if (out) *out = nullptr;
    if (!m || !strings || !lens || !out) REFUSE("%s: %s is NULL", fn, !m ? "model" : !strings ? "strings" : !lens ? "lens" : "out");
    if (n < 1) REFUSE("%s: n must be >= 1 (got %d)", fn, n);
    size_t total = 1;
    for (int32_t i = 0; i < n; i++) {
        if (!strings[i]) REFUSE("%s: strings[%d] is NULL", fn, i);
        if (lens[i] < 1) REFUSE("%s: strings[%d] is empty (length %d): a choice has at least one byte", fn, i, lens[i]);
        total += (size_t) lens[i];
        if (total > (size_t) lh::DFA_STATES_MAX) REFUSE("%s: the trie of the choices has more than %d states (n_states outside 1 .. %d)", fn, lh::DFA_STATES_MAX, lh::DFA_STATES_MAX);
    }
    // the trie, root = state 0; a string's end is accepting (a string that is a prefix of another: both ends are)
    std::vector<int32_t> trans(256, -1);
    std::vector<uint8_t> accept(1, 0);
    for (int32_t i = 0; i < n; i++) {
        int32_t q = 0;
        for (int32_t k = 0; k < lens[i]; k++) {
            const size_t at = (size_t) q * 256 + strings[i][k];
            if (trans[at] < 0) {
                const int32_t fresh = (int32_t) accept.size();
                trans[at] = fresh;                       // (before the resize: `at` stays valid, the reference would not)
                trans.resize(trans.size() + 256, -1);
                accept.push_back(0);
            }
            q = trans[at];
        }
        accept[(size_t) q] = 1;
    }
    std::vector<char> e(err_cap ? err_cap : 1, 0);
    const int rc = llamahip_constraint_new(m, (int32_t) accept.size(), trans.data(), accept.data(), 0, stop_token, out, e.data(), err_cap ? e.size() : 0);
    if (rc && err_cap) {          // the same refusals under this function's name
        const char *msg = e.data();
        const char *colon = strstr(msg, ": ");
        snprintf(err, err_cap, "%s: %s", fn, colon ? colon + 2 : msg);
    }
    return rc;
}

void llamahip_constraint_free(llamahip_constraint *c) {
    if (!c) return;
    if (c->dev_release) c->dev_release(c);
    delete c;
}

int32_t llamahip_constraint_n_states(const llamahip_constraint *c) { return c ? c->n_states : 0; }
int32_t llamahip_constraint_start(const llamahip_constraint *c) { return c ? c->start : -1; }
int32_t llamahip_constraint_done(const llamahip_constraint *c) { return c ? c->n_states - 1 : -1; }

int64_t llamahip_constraint_table(const llamahip_constraint *c, uint16_t *out, int64_t cap) {
    if (!c) return -1;
    const int64_t n = (int64_t) c->next.size();
    if (out && cap >= n) memcpy(out, c->next.data(), (size_t) n * 2);
    return n;
}

int32_t llamahip_constraint_advance(const llamahip_constraint *c, int32_t state, int32_t token) {
    if (!c || state < 0 || state >= c->n_states || token < 0 || token >= c->n_vocab) return -1;
    const uint16_t q = c->next[(size_t) state * c->n_vocab + token];
    return q == DFA_BANNED ? -1 : (int32_t) q;
}

int32_t llamahip_forced_run(const llamahip_constraint *c, int32_t state, int32_t *out, int32_t cap) {
    if (!c || state < 0 || state >= c->n_states || cap < 0 || (cap > 0 && !out)) return -1;
    const int32_t done = c->n_states - 1;
    int32_t n = 0;
    while (n < cap && state != done && c->single[(size_t) state] >= 0) {
        const int32_t t = c->single[(size_t) state];
        out[n++] = t;
        state = (int32_t) c->next[(size_t) state * c->n_vocab + t];
    }
    return n;
}

int32_t llamahip_constraint_pick(const llamahip_constraint *c, int32_t state, const float *logits) {
    if (!c || !logits || state < 0 || state >= c->n_states) return -1;
    return lh::dfa_pick_row(c->next.data() + (size_t) state * c->n_vocab, c->n_vocab, logits);
}

int llamahip_constraint_mask_row(const llamahip_constraint *c, int32_t state, const float *logits_in, float *logits_out) {
    if (!c || !logits_in || !logits_out || state < 0 || state >= c->n_states) return LLAMAHIP_ERR_PREDICT;
    const uint16_t *row = c->next.data() + (size_t) state * c->n_vocab;
    const uint32_t ninf = 0xFF800000u;
    for (int32_t i = 0; i < c->n_vocab; i++) memcpy(&logits_out[i], row[i] == DFA_BANNED ? (const void *) &ninf : (const void *) &logits_in[i], 4);
    return LLAMAHIP_OK;
}

}  // extern "C"
