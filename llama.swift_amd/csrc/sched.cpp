// sched.cpp -- the host half of the request scheduler (include/llamahip.h "request scheduler"): the step rule
// (llamahip_sched_plan), the queue, the slots, what llamahip_sched_new / _submit / _step refuse, and the events of a step.  What a planned
// step runs on the handle is the device half's business (sched.h, llamahip.cpp).  Pure host code, no device, no HIP header:
// tools/host_sanitize compiles this file as it is and runs it under ASan + UBSan against a stubbed device half.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <vector>

#include "sched.h"

namespace {

struct Req {
    int64_t id = 0;
    std::vector<int32_t> prompt;
    int32_t n_predict = 0, stop_token = -1;
    llamahip_sampler *sampler = nullptr;
    int32_t off = 0;              // prompt tokens evaluated
    int32_t last = 0;             // the token the next decode row evaluates
    int32_t n_out = 0;            // tokens produced
    bool cancelled = false;
    int32_t left() const { return (int32_t) prompt.size() - off; }
};

}  // namespace

struct llamahip_sched {
    llamahip_model *m = nullptr;
    lh::SchedDev *dev = nullptr;
    llamahip_sched_opts o = {};
    lh::SchedHandleInfo hi = {};
    int64_t next_id = 1;
    std::deque<Req> queue;
    std::vector<Req> slot;                // [max_active]; id 0 = free
    std::vector<int32_t> order;           // the active slots in admission order, oldest first
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
    s->slot.resize((size_t) op.max_active);
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
    if (r->struct_size < (int32_t) sizeof(llamahip_request)) return refuse(err, err_cap, "llamahip_sched_submit: struct_size (%ld) is not sizeof(llamahip_request) (%ld)", r->struct_size, sizeof(llamahip_request));
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
    Req q;
    q.id = s->next_id++;
    q.prompt.assign(r->prompt, r->prompt + r->n_prompt);
    q.n_predict = r->n_predict; q.stop_token = r->stop_token; q.sampler = r->sampler;
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
    if (cap < 2 * A + 1) return refuse(err, err_cap, "llamahip_sched_step: cap (%ld) must be at least 2 * max_active + 1 (%ld) events", cap, 2 * A + 1);
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
        const size_t room = (size_t) (cap - 2 * A), take = std::min(room, s->pend.size());
        for (size_t k = 0; k < take; k++) { ev[n++] = s->pend[k]; s->st.n_done++; }
        s->pend.erase(s->pend.begin(), s->pend.begin() + (long) take);
    };
    // 2. queued requests take the free slots, lowest slot first, in submission order
    for (int32_t i = 0; i < A && !s->queue.empty(); i++)
        if (s->slot[(size_t) i].id == 0) {
            s->slot[(size_t) i] = std::move(s->queue.front());
            s->queue.pop_front();
            s->order.push_back(i);
        }
    const int32_t na = (int32_t) s->order.size();
    if (na == 0) { deliver_pending(); *n_ev = n; return LLAMAHIP_OK; }
    // 3. the rows of this step
    int32_t left[16], rows[16];
    bool mixed = false;
    for (int32_t k = 0; k < na; k++) left[k] = s->slot[(size_t) s->order[(size_t) k]].left();
    const int32_t total = llamahip_sched_plan(na, left, s->o.chunk_tokens, s->o.row_budget, rows);
    if (total < 1) return refuse(err, err_cap, "llamahip_sched_step: the step rule gave %ld rows for %ld active requests", total, na);
    lh::SchedSeg segs[16];
    int32_t seg_k[16], n_segs = 0, prompt_rows = 0;
    for (int32_t k = 0; k < na; k++) {
        if (rows[k] < 1) continue;
        const int32_t sl = s->order[(size_t) k];
        Req &q = s->slot[(size_t) sl];
        lh::SchedSeg &g = segs[n_segs];
        g = lh::SchedSeg();
        g.slot = sl; g.n_rows = rows[k]; g.n_out = q.n_out; g.sampler = q.sampler; g.token = -1;
        if (left[k] > 0) {
            g.pos = q.off; g.tokens = q.prompt.data() + q.off; g.emit = rows[k] == left[k] ? 1 : 0;
            mixed = true; prompt_rows += rows[k];
        } else { g.pos = (int32_t) q.prompt.size() + q.n_out - 1; g.tokens = &q.last; g.emit = 1; }
        seg_k[n_segs++] = k;
    }
    int32_t kind = -1, captures = 0;
    const int rc = lh::sched_dev_step(s->dev, segs, n_segs, mixed, &kind, &captures, err, err_cap);
    if (rc) return rc;          // (requests admitted by this step keep their slots: the next step plans the same rows again)
    for (int32_t j = 0; j < n_segs; j++)
        if (segs[j].emit && (segs[j].token < 0 || segs[j].token >= s->hi.n_vocab))
            return refuse(err, err_cap, "llamahip_sched_step: the device half reported token %ld for slot %ld", segs[j].token, segs[j].slot);
    deliver_pending();
    s->st.n_steps++;
    (kind == lh::SCHED_STEP_MIXED ? s->st.n_mixed_steps : kind == lh::SCHED_STEP_SET ? s->st.n_set_steps : kind == lh::SCHED_STEP_SINGLE ? s->st.n_single_steps : s->st.n_fallback_steps)++;
    s->st.n_rows += total; s->st.n_prompt_rows += prompt_rows; s->st.n_graph_captures += captures;
    // 4. the step's events; a request that produced its last token frees its slot (reused from the next step)
    bool freed[16] = { false };
    for (int32_t j = 0; j < n_segs; j++) {
        const lh::SchedSeg &g = segs[j];
        Req &q = s->slot[(size_t) g.slot];
        if (left[seg_k[j]] > 0) q.off += g.n_rows;
        if (!g.emit) continue;
        q.last = g.token; q.n_out++;
        s->st.n_tokens++;
        const int32_t ctx = (int32_t) q.prompt.size() + q.n_out - 1;          // the KV rows the slot holds; the position g.token would be evaluated at
        ev[n++] = { q.id, LLAMAHIP_EV_TOKEN, g.token, g.exact, g.slot, ctx, 0 };
        const bool stop = q.stop_token >= 0 && g.token == q.stop_token;
        if (stop || q.n_out >= q.n_predict) {
            ev[n++] = { q.id, LLAMAHIP_EV_DONE, -1, 0, g.slot, ctx, stop ? LLAMAHIP_DONE_STOP : LLAMAHIP_DONE_LENGTH };
            s->st.n_done++;
            freed[seg_k[j]] = true;
        }
    }
    for (int32_t k = na - 1; k >= 0; k--)
        if (freed[k]) { s->slot[(size_t) s->order[(size_t) k]] = Req(); s->order.erase(s->order.begin() + k); }
    *n_ev = n;
    return LLAMAHIP_OK;
}
