// sched.cpp -- the host half of the request scheduler (include/llamahip.h "request scheduler"): the step rule
// (llamahip_sched_plan), the draft policy (llamahip_sched_plan_drafts: what rides in the rows a step leaves spare), the prefix policy
// (llamahip_sched_plan_prefix: which slot a request takes and whose evaluated prompt rows it takes over), the queue, the slots, what
// llamahip_sched_new / _submit / _step refuse, and the events of a step.  What a planned
// step runs on the handle is the device half's business (sched.h, llamahip.cpp).  Pure host code, no device, no HIP header:
// tools/host_sanitize compiles this file as it is and runs it under ASan + UBSan against a stubbed device half.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <vector>

#include "constrain.h"
#include "sched.h"

namespace {

struct Req {
    int64_t id = 0;
    std::vector<int32_t> prompt;
    std::vector<int32_t> hist;    // a drafting scheduler only: the prompt, then everything produced (the drafter's history)
    int32_t n_predict = 0, stop_token = -1;
    llamahip_sampler *sampler = nullptr;
    llamahip_constraint *cst = nullptr;      // the caller's; lives until the request's DONE
    int32_t cst_state = 0;        // the automaton's state behind everything produced: the state of the next pick
    int32_t off = 0;              // prompt tokens evaluated
    int32_t last = 0;             // the token the next decode row evaluates
    int32_t n_out = 0;            // tokens produced
    bool cancelled = false;
    int32_t left() const { return (int32_t) prompt.size() - off; }
};

// a slot's held record (prefix_share): its latest occupant's prompt and how many of its KV rows [0, n) are evaluated prompt rows; it outlives
// the occupant until the next one replaces it
struct Held {
    std::vector<int32_t> prompt;
    int32_t n = 0;
};

}  // namespace

struct llamahip_sched {
    llamahip_model *m = nullptr;
    lh::SchedDev *dev = nullptr;
    llamahip_sched_opts o = {};
    std::vector<int32_t> corpus;          // the caller's, copied (o.corpus points here)
    lh::SchedHandleInfo hi = {};
    int64_t next_id = 1;
    std::deque<Req> queue;
    std::vector<Req> slot;                // [max_active]; id 0 = free
    std::vector<int32_t> order;           // the active slots in admission order, oldest first
    bool sharing = false;                 // prefix_share on a handle and at a chunking that can share (not FAST_PREFILL, chunk_tokens > 0)
    std::vector<Held> held;               // [max_active], kept only while sharing
    std::vector<llamahip_sched_event> pend;      // DONE events of cancelled requests, delivered by the next step
    llamahip_sched_stats st = {};
};

static int refuse(char *err, size_t err_cap, const char *fmt, long a = 0, long b = 0, long c = 0) {
    if (err && err_cap) snprintf(err, err_cap, fmt, a, b, c);
    return LLAMAHIP_ERR_PREDICT;
}

extern "C" int32_t llamahip_sched_plan(int32_t n_active, const int32_t *prompt_left, int32_t chunk_tokens, int32_t row_budget, int32_t *rows_out) {
    if (n_active < 0 || n_active > 16 || chunk_tokens < 0 || row_budget < 1 || (n_active > 0 && (!prompt_left || !rows_out))) return -1;
    int64_t rest = row_budget, total = 0;
    for (int32_t i = 0; i < n_active; i++) {
        if (prompt_left[i] < 0) return -1;
        if (prompt_left[i] == 0) rest--;
    }
    bool given = false, stopped = false;
    for (int32_t i = 0; i < n_active; i++) {
        const int32_t left = prompt_left[i];
        int64_t r = 0;
        if (left == 0) r = 1;
        else if (!stopped) {
            r = chunk_tokens > 0 ? std::min<int64_t>(left, std::max<int64_t>(rest, 0) / chunk_tokens * chunk_tokens) : (left <= rest ? left : 0);
            if (r < 1) {
                if (!given) r = chunk_tokens > 0 ? std::min(left, chunk_tokens) : left;      // the progress guarantee
                else { stopped = true; r = 0; }
            }
            if (r > 0) { given = true; rest -= r; }
        }
        rows_out[i] = (int32_t) r;
        total += r;
    }
    return (int32_t) std::min<int64_t>(total, INT32_MAX);
}

extern "C" int32_t llamahip_sched_plan_drafts(int32_t n_active, const int32_t *prompt_left, const int32_t *rows, const int32_t *want, int32_t *give) {
    if (n_active < 0 || n_active > 16 || (n_active > 0 && (!prompt_left || !rows || !want || !give))) return -1;
    int32_t dec_want[16], dec_give[16], dec_at[16], n_dec = 0, emitting = 0;
    int64_t total = 0;
    for (int32_t i = 0; i < n_active; i++) {
        if (prompt_left[i] < 0 || rows[i] < 0 || want[i] < 0 || want[i] > 15 || (prompt_left[i] > 0 && (want[i] != 0 || rows[i] > prompt_left[i])) ||
            (prompt_left[i] == 0 && rows[i] != 1))
            return -1;
        give[i] = 0;
        total += rows[i];
        if (prompt_left[i] == 0) { dec_want[n_dec] = want[i]; dec_at[n_dec++] = i; emitting++; }
        else if (rows[i] == prompt_left[i]) emitting++;
    }
    const int64_t spare = std::min<int64_t>(16 - emitting, LLAMAHIP_EVAL_MULTI_MAX_ROWS - total);
    if (n_dec == 0 || spare < 1) return 0;
    // (the dealing rule, not restated: every decoding sequence has its base row, the spare rows go round-robin in admission order)
    const int32_t dealt = llamahip_lookup_deal_rows(dec_want, n_dec, n_dec + (int32_t) spare, dec_give);
    if (dealt < 0) return -1;
    for (int32_t k = 0; k < n_dec; k++) give[dec_at[k]] = dec_give[k];
    return dealt;
}

extern "C" int32_t llamahip_sched_plan_prefix(int32_t n_slots, const int32_t *slot_free, const int32_t *held, const int32_t *n_held, const int32_t *prompt,
                                              int32_t n_prompt, int32_t chunk_tokens, int32_t *slot_out, int32_t *donor_out, int32_t *n_inplace_out) {
    if (n_slots < 1 || n_slots > 16 || !slot_free || !n_held || !prompt || n_prompt < 1 || chunk_tokens < 0 || !slot_out || !donor_out || !n_inplace_out) return -1;
    int64_t n_all = 0;
    bool any_free = false;
    for (int32_t s = 0; s < n_slots; s++) {
        if (slot_free[s] < 0 || n_held[s] < 0) return -1;
        any_free = any_free || slot_free[s] != 0;
        n_all += n_held[s];
    }
    if (!any_free || (n_all > 0 && !held)) return -1;
    for (int32_t j = 0; j < n_prompt; j++) if (prompt[j] < 0) return -1;
    for (int64_t j = 0; j < n_all; j++) if (held[j] < 0) return -1;
    // share(s): the whole chunks of the common prefix that the record holds as prompt rows, the prompt's last token never among them
    int32_t share[16];
    const int32_t *h = held;
    for (int32_t s = 0; s < n_slots; h += n_held[s], s++) {
        const int32_t lim = std::min(n_held[s], n_prompt - 1);
        int32_t l = 0;
        while (l < lim && h[l] == prompt[l]) l++;
        share[s] = chunk_tokens > 0 ? l / chunk_tokens * chunk_tokens : 0;
    }
    int32_t slot = -1, donor = -1;
    for (int32_t s = 0; s < n_slots; s++)
        if (slot_free[s] && (slot < 0 || share[s] > share[slot] || (share[s] == share[slot] && n_held[s] < n_held[slot]))) slot = s;
    for (int32_t t = 0; t < n_slots; t++)
        if (t != slot && (donor < 0 || share[t] > share[donor])) donor = t;
    *slot_out = slot;
    *n_inplace_out = share[slot];
    if (donor >= 0 && share[donor] > share[slot]) { *donor_out = donor; return share[donor]; }
    *donor_out = -1;
    return share[slot];
}

extern "C" int llamahip_sched_new(llamahip_model *m, const llamahip_sched_opts *o, llamahip_sched **out, char *err, size_t err_cap) {
    static const char *fn = "llamahip_sched_new";
    if (out) *out = nullptr;
    if (!o || !out) { if (err && err_cap) snprintf(err, err_cap, "%s: null options or output", fn); return LLAMAHIP_ERR_PREDICT; }
    llamahip_sched_opts op = {};
    memcpy(&op, o, std::min((size_t) std::max(o->struct_size, 0), sizeof(op)));
    if (o->struct_size < (int32_t) offsetof(llamahip_sched_opts, repeat_penalty)) return refuse(err, err_cap, "llamahip_sched_new: struct_size (%ld) is smaller than the options up to row_budget", o->struct_size);
    if (op.max_active < 1 || op.max_active > 16) return refuse(err, err_cap, "llamahip_sched_new: max_active (%ld) outside 1 .. 16", op.max_active);
    if (op.chunk_tokens < 0) return refuse(err, err_cap, "llamahip_sched_new: chunk_tokens (%ld) must be >= 0 (0 = a prompt is one eval)", op.chunk_tokens);
    if (op.row_budget < 0 || op.row_budget > LLAMAHIP_EVAL_MULTI_MAX_ROWS - 16)
        return refuse(err, err_cap, "llamahip_sched_new: row_budget (%ld) outside 0 .. LLAMAHIP_EVAL_MULTI_MAX_ROWS - 16 (%ld)", op.row_budget, LLAMAHIP_EVAL_MULTI_MAX_ROWS - 16);
    if (op.row_budget == 0) op.row_budget = LLAMAHIP_SCHED_ROW_BUDGET;
    if (op.draft_len < 0 || op.draft_len > 15) return refuse(err, err_cap, "llamahip_sched_new: draft_len (%ld) outside 0 .. 15 (0 = no drafting)", op.draft_len);
    {
        const int32_t mn = op.ngram_min ? op.ngram_min : LLAMAHIP_LOOKUP_NGRAM_MIN, mx = op.ngram_max ? op.ngram_max : LLAMAHIP_LOOKUP_NGRAM_MAX;
        if (op.ngram_min < 0 || op.ngram_max < 0 || mx < mn)          // (what llamahip_lookup_draft refuses)
            return refuse(err, err_cap, "llamahip_sched_new: ngram_min (%ld) / ngram_max (%ld) must be >= 0 (0 = LLAMAHIP_LOOKUP_NGRAM_MIN / _MAX) with ngram_max >= ngram_min", op.ngram_min, op.ngram_max);
    }
    if (o->struct_size < (int32_t) (offsetof(llamahip_sched_opts, prefix_share) + sizeof(op.prefix_share))) op.prefix_share = 0;          // (a shorter struct: off)
    if (op.prefix_share != 0 && op.prefix_share != 1) return refuse(err, err_cap, "llamahip_sched_new: prefix_share (%ld) must be 0 (off) or 1", op.prefix_share);
    if (o->struct_size < (int32_t) (offsetof(llamahip_sched_opts, forced_drafts) + sizeof(op.forced_drafts))) op.forced_drafts = 0;          // (a shorter struct: off)
    if (op.forced_drafts != 0 && op.forced_drafts != 1) return refuse(err, err_cap, "llamahip_sched_new: forced_drafts (%ld) must be 0 (off) or 1", op.forced_drafts);
    if (op.n_corpus < 0 || (op.n_corpus > 0 && !op.corpus)) return refuse(err, err_cap, "llamahip_sched_new: n_corpus (%ld) must be >= 0, with a corpus where it is > 0", op.n_corpus);
    if (const int32_t V = llamahip_n_vocab(m))          // (a null handle is refused below)
        for (int32_t i = 0; i < op.n_corpus; i++)
            if (op.corpus[i] < 0 || op.corpus[i] >= V) return refuse(err, err_cap, "llamahip_sched_new: corpus token id %ld at %ld out of range [0, %ld)", op.corpus[i], i, V);
    if (op.top_k == 0 && op.repeat_penalty == 0.0 && op.top_p == 0.0 && op.temp == 0.0) { op.repeat_penalty = 1.3; op.top_p = (double) 0.95f; op.temp = (double) 0.8f; op.top_k = 40; }      // (the reference's float defaults)
    int rc = lh::sched_sampler_check(op.repeat_penalty, op.top_k, op.top_p, op.temp, err, err_cap);
    if (rc) return rc;
    lh::SchedHandleInfo hi = {};
    if ((rc = lh::sched_handle_info(m, &hi, err, err_cap)) != 0) return rc;
    if (op.max_active > hi.n_seq) return refuse(err, err_cap, "llamahip_sched_new: max_active (%ld) on a handle with %ld KV slots (llamahip_opts.n_seq)", op.max_active, hi.n_seq);
    lh::SchedDev *dev = nullptr;
    if ((rc = lh::sched_dev_new(m, &op, &dev, err, err_cap)) != 0) return rc;          // (the handle already has a scheduler)
    llamahip_sched *s = new llamahip_sched();
    s->m = m; s->o = op; s->hi = hi; s->dev = dev;
    if (op.n_corpus > 0) s->corpus.assign(op.corpus, op.corpus + op.n_corpus);
    s->o.corpus = s->corpus.data();
    s->slot.resize((size_t) op.max_active);
    // a FAST_PREFILL handle makes no parity claim for its prompt rows and at chunk_tokens 0 a row's key count is its own prompt's length:
    // nothing is shareable there, no record is kept and the slots are chosen as without the option
    s->sharing = op.prefix_share == 1 && op.chunk_tokens > 0 && !hi.fast_prefill;
    if (s->sharing) s->held.resize((size_t) op.max_active);
    s->st.struct_size = (int32_t) sizeof(s->st);
    *out = s;
    return LLAMAHIP_OK;
}

extern "C" void llamahip_sched_free(llamahip_sched *s) {
    if (!s) return;
    lh::sched_dev_free(s->dev);
    delete s;
}

extern "C" int llamahip_sched_submit(llamahip_sched *s, const llamahip_request *r, int64_t *id, char *err, size_t err_cap) {
    static const char *fn = "llamahip_sched_submit";
    if (!s || !r) { if (err && err_cap) snprintf(err, err_cap, "%s: null scheduler or request", fn); return LLAMAHIP_ERR_PREDICT; }
    // the request up to `sampler` (the struct before constraints) or the whole of it; the new fields are read only where struct_size covers them
    if (r->struct_size < (int32_t) offsetof(llamahip_request, constraint))
        return refuse(err, err_cap, "llamahip_sched_submit: struct_size (%ld) is smaller than the request up to sampler (%ld; sizeof(llamahip_request) is %ld)", r->struct_size, offsetof(llamahip_request, constraint), sizeof(llamahip_request));
    llamahip_constraint *cst = r->struct_size >= (int32_t) (offsetof(llamahip_request, constraint) + sizeof(r->constraint)) ? r->constraint : nullptr;
    int32_t cst_state = r->struct_size >= (int32_t) (offsetof(llamahip_request, constraint_state) + sizeof(r->constraint_state)) ? r->constraint_state : -1;
    if (!r->prompt || r->n_prompt < 1) return refuse(err, err_cap, "llamahip_sched_submit: n_prompt must be >= 1 (got %ld)", r->n_prompt);
    if (r->n_predict < 1) return refuse(err, err_cap, "llamahip_sched_submit: n_predict must be >= 1 (got %ld)", r->n_predict);
    if ((int64_t) r->n_prompt + r->n_predict - 1 > s->hi.n_ctx)
        return refuse(err, err_cap, "llamahip_sched_submit: context overflow: n_prompt (%ld) + n_predict (%ld) - 1 > n_ctx (%ld)", r->n_prompt, r->n_predict, s->hi.n_ctx);
    for (int32_t i = 0; i < r->n_prompt; i++)
        if (r->prompt[i] < 0 || r->prompt[i] >= s->hi.n_vocab) return refuse(err, err_cap, "llamahip_sched_submit: token id %ld at %ld out of range [0, %ld)", r->prompt[i], i, s->hi.n_vocab);
    if (r->stop_token < -1 || r->stop_token >= s->hi.n_vocab) return refuse(err, err_cap, "llamahip_sched_submit: stop_token %ld out of range [0, %ld) (-1 = none)", r->stop_token, s->hi.n_vocab);
    const int32_t piece = s->o.chunk_tokens > 0 ? std::min(r->n_prompt, s->o.chunk_tokens) : r->n_prompt;
    if (piece > LLAMAHIP_EVAL_MULTI_MAX_ROWS - s->o.max_active)
        return refuse(err, err_cap, s->o.chunk_tokens > 0 ? "llamahip_sched_submit: a prompt piece of %ld tokens (chunk_tokens) is more than LLAMAHIP_EVAL_MULTI_MAX_ROWS - max_active (%ld) rows"
                                                          : "llamahip_sched_submit: with chunk_tokens 0 a prompt of %ld tokens is one piece, more than LLAMAHIP_EVAL_MULTI_MAX_ROWS - max_active (%ld) rows",
                      piece, LLAMAHIP_EVAL_MULTI_MAX_ROWS - s->o.max_active);
    if (r->sampler) {
        bool held = false;
        for (const Req &q : s->queue) held = held || (q.sampler == r->sampler && !q.cancelled);
        for (const Req &q : s->slot) held = held || (q.id && q.sampler == r->sampler && !q.cancelled);
        if (held) return refuse(err, err_cap, "llamahip_sched_submit: the sampler is held by another live request: every request draws with its own");
    }
    if (cst) {
        if (cst->m != s->m) return refuse(err, err_cap, "llamahip_sched_submit: the constraint was made on another handle");
        if (cst_state < -1 || cst_state >= cst->n_states) return refuse(err, err_cap, "llamahip_sched_submit: constraint_state %ld out of range [0, %ld) (-1 = the constraint's start)", cst_state, cst->n_states);
        if (r->stop_token != -1 && r->stop_token != cst->stop_token)
            return refuse(err, err_cap, "llamahip_sched_submit: stop_token %ld is neither -1 nor the constraint's stop token (%ld), which ends a constrained request", r->stop_token, cst->stop_token);
        if (r->sampler) return refuse(err, err_cap, "llamahip_sched_submit: a sampler together with a constraint: sampled constrained requests are not built (greedy only)");
        if (s->hi.pipeline) return refuse(err, err_cap, "llamahip_sched_submit: a constrained request on an in-process pipeline handle is not built (the table's device copy belongs to one device)");
        if (cst_state < 0) cst_state = cst->start;
    }
    Req q;
    q.id = s->next_id++;
    q.prompt.assign(r->prompt, r->prompt + r->n_prompt);
    if (s->o.draft_len > 0) q.hist = q.prompt;
    q.n_predict = r->n_predict; q.stop_token = cst ? cst->stop_token : r->stop_token; q.sampler = r->sampler;
    q.cst = cst; q.cst_state = cst ? cst_state : 0;
    s->queue.push_back(std::move(q));
    s->st.n_submitted++;
    if (id) *id = s->queue.back().id;
    return LLAMAHIP_OK;
}

extern "C" int llamahip_sched_cancel(llamahip_sched *s, int64_t id) {
    if (!s) return -1;
    for (auto it = s->queue.begin(); it != s->queue.end(); ++it)
        if (it->id == id) {
            s->pend.push_back({ id, LLAMAHIP_EV_DONE, -1, 0, -1, 0, LLAMAHIP_DONE_CANCELLED });
            s->queue.erase(it);
            return 0;
        }
    for (Req &q : s->slot)
        if (q.id == id && !q.cancelled) { q.cancelled = true; return 0; }
    return -1;
}

extern "C" int32_t llamahip_sched_pending(const llamahip_sched *s) {
    return s ? (int32_t) (s->queue.size() + s->order.size() + s->pend.size()) : 0;
}

extern "C" int llamahip_sched_get_stats(const llamahip_sched *s, llamahip_sched_stats *out) {
    if (!s || !out || out->struct_size < 4) return LLAMAHIP_ERR_UNKNOWN;
    llamahip_sched_stats v = s->st;
    const int32_t n = (int32_t) std::min((size_t) out->struct_size, sizeof(v));
    v.struct_size = n;
    memcpy(out, &v, (size_t) n);
    return LLAMAHIP_OK;
}

extern "C" int llamahip_sched_step(llamahip_sched *s, llamahip_sched_event *ev, int32_t cap, int32_t *n_ev, char *err, size_t err_cap) {
    static const char *fn = "llamahip_sched_step";
    if (n_ev) *n_ev = 0;
    if (!s || !ev || !n_ev) { if (err && err_cap) snprintf(err, err_cap, "%s: null scheduler, events or n_ev", fn); return LLAMAHIP_ERR_PREDICT; }
    const int32_t A = s->o.max_active;
    // (forced drafts put several tokens of a request into one step whatever draft_len is: the capacity of a drafting scheduler)
    const int32_t cap_len = std::max(s->o.draft_len, s->o.forced_drafts);
    if (cap_len == 0 && cap < 2 * A + 1) return refuse(err, err_cap, "llamahip_sched_step: cap (%ld) must be at least 2 * max_active + 1 (%ld) events", cap, 2 * A + 1);
    if (cap < LLAMAHIP_SCHED_EVENT_CAP(A, cap_len))
        return refuse(err, err_cap, "llamahip_sched_step: cap (%ld) must be at least max_active + 17 (%ld) events with draft_len > 0 or forced_drafts (LLAMAHIP_SCHED_EVENT_CAP(max_active, 1))", cap, A + 17);
    const int32_t own_events = LLAMAHIP_SCHED_EVENT_CAP(A, cap_len) - 1;          // what the step's own TOKEN and DONE events may take
    // 1. cancelled active requests leave their slots; then as many waiting DONE events as the step's own events leave room for
    for (size_t k = 0; k < s->order.size();) {
        Req &q = s->slot[(size_t) s->order[k]];
        if (!q.cancelled) { k++; continue; }
        s->pend.push_back({ q.id, LLAMAHIP_EV_DONE, -1, 0, s->order[k], q.off + std::max(q.n_out - 1, 0), LLAMAHIP_DONE_CANCELLED });
        q = Req();
        s->order.erase(s->order.begin() + (long) k);
    }
    // (the waiting DONE events are handed over only by a step that succeeds: a step that fails delivers nothing and loses nothing)
    int32_t n = 0;
    auto deliver_pending = [&]() {
        const size_t room = (size_t) (cap - own_events), take = std::min(room, s->pend.size());
        for (size_t k = 0; k < take; k++) { ev[n++] = s->pend[k]; s->st.n_done++; }
        s->pend.erase(s->pend.begin(), s->pend.begin() + (long) take);
    };
    // 2. queued requests take the free slots, lowest slot first, in submission order
    for (int32_t i = 0; !s->sharing && i < A && !s->queue.empty(); i++)
        if (s->slot[(size_t) i].id == 0) {
            s->slot[(size_t) i] = std::move(s->queue.front());
            s->queue.pop_front();
            s->order.push_back(i);
        }
    // ... with shared prefixes: one at a time, the prefix policy over the held records as they stand; the copy is enqueued before the
    // admission is committed (a copy that cannot be enqueued leaves the request queued; what was admitted before it stays admitted)
    while (s->sharing && !s->queue.empty() && (int32_t) s->order.size() < A) {
        int32_t is_free[16], n_held[16], sl = -1, donor = -1, inplace = 0, launches = 0;
        std::vector<int32_t> held;
        for (int32_t i = 0; i < A; i++) {
            const Held &h = s->held[(size_t) i];
            is_free[i] = s->slot[(size_t) i].id == 0;
            n_held[i] = h.n;
            held.insert(held.end(), h.prompt.begin(), h.prompt.begin() + h.n);
        }
        held.push_back(0);          // (never read: a non-null array where nothing is held)
        const Req &front = s->queue.front();
        const int32_t P = llamahip_sched_plan_prefix(A, is_free, held.data(), n_held, front.prompt.data(), (int32_t) front.prompt.size(), s->o.chunk_tokens, &sl, &donor, &inplace);
        if (P < 0 || P >= (int32_t) front.prompt.size() || sl < 0 || sl >= A || s->slot[(size_t) sl].id != 0 || inplace < 0 || inplace > P || (donor >= 0 && (donor >= A || donor == sl)))
            return refuse(err, err_cap, "llamahip_sched_step: the prefix policy gave %ld shared rows in slot %ld for a prompt of %ld tokens", P, sl, (long) front.prompt.size());
        if (donor >= 0) {
            const int rc = lh::sched_dev_copy_prefix(s->dev, donor, sl, inplace, P - inplace, &launches, err, err_cap);
            if (rc) return rc;
            s->st.n_copied_rows += P - inplace; s->st.n_copy_launches += launches;
        }
        s->st.n_shared_rows += P;
        Req &q = s->slot[(size_t) sl];
        q = std::move(s->queue.front());
        s->queue.pop_front();
        q.off = P;
        s->held[(size_t) sl].prompt = q.prompt;
        s->held[(size_t) sl].n = P;
        s->order.push_back(sl);
    }
    const int32_t na = (int32_t) s->order.size();
    if (na == 0) { deliver_pending(); *n_ev = n; return LLAMAHIP_OK; }
    // 3. the rows of this step
    int32_t left[16], rows[16];
    bool mixed = false;
    for (int32_t k = 0; k < na; k++) left[k] = s->slot[(size_t) s->order[(size_t) k]].left();
    const int32_t total = llamahip_sched_plan(na, left, s->o.chunk_tokens, s->o.row_budget, rows);
    if (total < 1) return refuse(err, err_cap, "llamahip_sched_step: the step rule gave %ld rows for %ld active requests", total, na);
    // 3b. drafted tokens in the rows the step leaves spare: what every decoding request could use, then the one policy
    int32_t want[16] = { 0 }, give[16] = { 0 }, draft_rows = 0;
    int32_t drafts[16][15];
    bool forced[16] = { false };
    if ((s->o.draft_len > 0 || s->o.forced_drafts) && lh::sched_dev_drafts(s->dev)) {
        bool any = false;
        for (int32_t k = 0; k < na; k++) {
            Req &q = s->slot[(size_t) s->order[(size_t) k]];
            if (left[k] > 0 || q.n_out < 1) continue;
            // a constrained request's forced run, from the state behind the token it is about to evaluate: a draft accepted by construction
            if (q.cst && s->o.forced_drafts) {
                const int32_t n = llamahip_forced_run(q.cst, q.cst_state, drafts[k], std::max(std::min(15, q.n_predict - q.n_out - 1), 0));
                if (n > 0) { want[k] = n; forced[k] = true; any = true; continue; }
            }
            int32_t room = std::min(s->o.draft_len, q.n_predict - q.n_out - 1);          // a verify step never passes n_predict (and so never n_ctx)
            if (room < 1) continue;
            if (q.sampler && (s->o.top_k > 64 || s->hi.n_vocab > 32768 || llamahip_sampler_window(q.sampler, nullptr, 0) > 1024)) continue;      // (no candidates on the device)
            int32_t n = llamahip_lookup_draft(q.hist.data(), (int32_t) q.hist.size(), s->corpus.data(), (int32_t) s->corpus.size(), room, s->o.ngram_min, s->o.ngram_max, drafts[k]);
            // a sampled request draws nothing behind its stop token (the draws are accepted into its sampler as they are made): its draft
            // ends before one.  A greedy request's accepted tokens behind a stop token are dropped below
            for (int32_t j = 0; q.sampler && j < n; j++) if (q.stop_token >= 0 && drafts[k][j] == q.stop_token) n = j;
            // a constrained request's lookup draft ends at the first token banned in the running state, and behind a drafted stop token
            for (int32_t j = 0, st = q.cst_state; q.cst && j < n; j++) {
                st = llamahip_constraint_advance(q.cst, st, drafts[k][j]);
                if (st < 0) n = j;
                else if (drafts[k][j] == q.stop_token) n = j + 1;
            }
            want[k] = std::max(n, 0);
            any = any || want[k] > 0;
        }
        if (any && (draft_rows = llamahip_sched_plan_drafts(na, left, rows, want, give)) < 0)
            return refuse(err, err_cap, "llamahip_sched_step: the draft policy refused the step of %ld active requests", na);
    }
    lh::SchedSeg segs[16];
    int32_t seg_k[16], n_segs = 0, prompt_rows = 0;
    for (int32_t k = 0; k < na; k++) {
        if (rows[k] < 1) continue;
        const int32_t sl = s->order[(size_t) k];
        Req &q = s->slot[(size_t) sl];
        lh::SchedSeg &g = segs[n_segs];
        g = lh::SchedSeg();
        g.slot = sl; g.n_rows = rows[k]; g.n_out = q.n_out; g.sampler = q.sampler; g.token = -1;
        g.cst = q.cst; g.cst_state = q.cst_state;
        if (left[k] > 0) {
            g.pos = q.off; g.tokens = q.prompt.data() + q.off; g.emit = rows[k] == left[k] ? 1 : 0;
            if (!g.emit) g.cst = nullptr;
            mixed = true; prompt_rows += rows[k];
        } else {
            g.pos = (int32_t) q.prompt.size() + q.n_out - 1; g.tokens = &q.last; g.emit = 1;
            if (give[k] > 0) { g.draft = drafts[k]; g.n_draft = give[k]; mixed = true; }
        }
        seg_k[n_segs++] = k;
    }
    int32_t kind = -1, captures = 0;
    const int rc = lh::sched_dev_step(s->dev, segs, n_segs, mixed, &kind, &captures, err, err_cap);
    if (rc) return rc;          // (requests admitted by this step keep their slots: the next step plans the same rows again)
    for (int32_t j = 0; j < n_segs; j++) {
        lh::SchedSeg &g = segs[j];
        if (!g.emit) continue;
        if (g.n_draft == 0) { g.n_accept = 0; g.toks[0] = g.token; g.exacts[0] = g.exact; }
        if (g.n_accept < 0 || g.n_accept > g.n_draft) return refuse(err, err_cap, "llamahip_sched_step: the device half reported %ld accepted of %ld drafted tokens for slot %ld", g.n_accept, g.n_draft, g.slot);
        for (int32_t a = 0; a <= g.n_accept; a++)
            if (g.toks[a] < 0 || g.toks[a] >= s->hi.n_vocab || (a < g.n_accept && g.toks[a] != g.draft[a]))
                return refuse(err, err_cap, "llamahip_sched_step: the device half reported token %ld for slot %ld", g.toks[a], g.slot);
        // a constrained segment: every token it produced is allowed in the state it was picked in
        for (int32_t a = 0, st = g.cst_state; g.cst && a <= g.n_accept; a++)
            if ((st = llamahip_constraint_advance(g.cst, st, g.toks[a])) < 0)
                return refuse(err, err_cap, "llamahip_sched_step: the device half reported token %ld for slot %ld, which the request's constraint bans", g.toks[a], g.slot);
    }
    deliver_pending();
    s->st.n_steps++;
    (kind == lh::SCHED_STEP_MIXED ? s->st.n_mixed_steps : kind == lh::SCHED_STEP_SET ? s->st.n_set_steps : kind == lh::SCHED_STEP_SINGLE ? s->st.n_single_steps : s->st.n_fallback_steps)++;
    s->st.n_rows += total + draft_rows; s->st.n_prompt_rows += prompt_rows; s->st.n_graph_captures += captures;
    if (draft_rows > 0) { s->st.n_draft_steps++; s->st.n_drafted += draft_rows; }
    for (int32_t k = 0; k < na; k++) if (forced[k]) s->st.n_forced_drafted += give[k];
    // 4. the step's events; a request that produced its last token frees its slot (reused from the next step)
    bool freed[16] = { false };
    for (int32_t j = 0; j < n_segs; j++) {
        const lh::SchedSeg &g = segs[j];
        Req &q = s->slot[(size_t) g.slot];
        if (left[seg_k[j]] > 0) {
            q.off += g.n_rows;
            if (s->sharing) s->held[(size_t) g.slot].n = q.off;          // (evaluated prompt rows only: decode and draft rows lie above the prompt's end)
        }
        if (!g.emit) continue;
        s->st.n_emit_segs++;
        s->st.n_accepted += g.n_accept;
        if (forced[seg_k[j]]) s->st.n_forced_accepted += g.n_accept;
        if (g.cst) s->st.n_dfa_rows += 1 + g.n_draft;
        // the segment's n_accept + 1 tokens in order, cut at the stop token (what was accepted behind it is dropped) or at n_predict
        for (int32_t a = 0; a <= g.n_accept; a++) {
            q.last = g.toks[a]; q.n_out++;
            if (q.cst) q.cst_state = llamahip_constraint_advance(q.cst, q.cst_state, q.last);          // (checked above: never banned)
            if (s->o.draft_len > 0) q.hist.push_back(q.last);
            s->st.n_tokens++;
            const int32_t ctx = (int32_t) q.prompt.size() + q.n_out - 1;          // the KV rows the slot holds; the position the token would be evaluated at
            ev[n++] = { q.id, LLAMAHIP_EV_TOKEN, q.last, g.exacts[a], g.slot, ctx, 0 };
            const bool stop = q.stop_token >= 0 && q.last == q.stop_token;
            if (stop || q.n_out >= q.n_predict) {
                ev[n++] = { q.id, LLAMAHIP_EV_DONE, -1, 0, g.slot, ctx, stop ? LLAMAHIP_DONE_STOP : LLAMAHIP_DONE_LENGTH };
                s->st.n_done++;
                s->st.n_dropped += g.n_accept - a;
                freed[seg_k[j]] = true;
                break;
            }
        }
    }
    for (int32_t k = na - 1; k >= 0; k--)
        if (freed[k]) { s->slot[(size_t) s->order[(size_t) k]] = Req(); s->order.erase(s->order.begin() + k); }
    *n_ev = n;
    return LLAMAHIP_OK;
}
