// sched.h -- the seam between the request scheduler's host half (sched.cpp: queue, slots, the step rule, events) and its device half
// (llamahip.cpp: what a planned step runs on the handle).  Plain C++ types only, no HIP header: sched.cpp is compiled as it is into
// tools/host_sanitize, where the functions below are stubs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/llamahip.h"

namespace lh {

struct SchedDev;          // the device half's state for one scheduler (llamahip.cpp)

// what the host half needs to know of the handle; refuses (message in err, the handle named last) null, HOST_ONLY and stage handles
// fast_prefill: a LLAMAHIP_FLAG_FAST_PREFILL handle (no parity claim for its prompt rows: nothing of them is shared between slots)
// pipeline: an in-process pipeline handle (a constraint's device table belongs to one device: constrained requests are refused there)
struct SchedHandleInfo { int32_t n_ctx, n_vocab, n_seq, fast_prefill, pipeline; };
int sched_handle_info(const llamahip_model *m, SchedHandleInfo *out, char *err, size_t err_cap);
// the sampler parameters of llamahip_sched_opts, by llamahip_verify_sample's rule
int sched_sampler_check(double repeat_penalty, int32_t top_k, double top_p, double temp, char *err, size_t err_cap);

// One segment of a planned step: n_rows tokens of KV slot `slot` at position pos.  A prefilling sequence's piece, or a decoding sequence's
// one row [its last token].  emit: the segment's last row produces a token (a decode row, a piece that ends its prompt) -- the device half
// fills token / exact: the greedy pick (sampler == null) or the sampler's draw, already accepted into it.
// n_out: the tokens the request has produced before this step (the slot's trace cursor).
// draft / n_draft (a decoding sequence's segment only: n_rows == 1, emit): the drafted tokens that ride behind its one row -- the pass
// evaluates [tokens[0], draft ...] at pos, 1 + n_draft rows.  The device half fills n_accept (how many leading draft tokens the model
// reproduced, 0 .. n_draft) and toks / exacts [0 .. n_accept]: the tokens the segment produced -- picks, or draws already accepted into the
// sampler; token / exact = the first of them.  A segment without a draft gets token / exact only, as before.
// cst / cst_state (a greedy segment that emits; null = unconstrained): the request's constraint and the automaton state BEFORE the segment's
// first pick.  Every pick of the segment is then k_pick_dfa's rule under the state reached by advancing over the draft tokens in front of its
// logits row (the device half resolves the states: it has the table); a draft token banned in its state, or a row that allows nothing (the
// device's dead word), fails the step.  The host half advances the request's state over the tokens it reports.
constexpr int SCHED_SEG_TOKS = 16;
struct SchedSeg {
    int32_t slot, pos, n_rows, emit, n_out;
    const int32_t *tokens;
    llamahip_sampler *sampler;
    int32_t token, exact;
    const int32_t *draft;
    int32_t n_draft, n_accept;
    int32_t toks[SCHED_SEG_TOKS], exacts[SCHED_SEG_TOKS];
    llamahip_constraint *cst;
    int32_t cst_state;
};
enum { SCHED_STEP_MIXED = 0, SCHED_STEP_SET = 1, SCHED_STEP_SINGLE = 2, SCHED_STEP_FALLBACK = 3 };

// no device work (everything is set up by the first step); refuses a handle that already has a scheduler.  A handle freed under its
// scheduler orphans it: every later step fails, sched_dev_free never touches the handle
int sched_dev_new(llamahip_model *m, const llamahip_sched_opts *o, SchedDev **out, char *err, size_t err_cap);
void sched_dev_free(SchedDev *d);
// the handle takes drafted tokens in a step (it has the one pass and set steps: not a fall-back handle); 0 for a freed handle.  No device work
int sched_dev_drafts(SchedDev *d);
// one weight pass over the segments (mixed: some segment is a prompt piece or carries a draft; else every segment is one decode row).  *kind: SCHED_STEP_*;
// *captures: set-step graphs captured by this step.  Nothing of the host half's state is read: the segments say everything.
int sched_dev_step(SchedDev *d, SchedSeg *segs, int32_t n_segs, bool mixed, int32_t *kind, int32_t *captures, char *err, size_t err_cap);
// a shared prompt prefix: the KV rows [row_begin, row_begin + n_rows) of every layer, K and V, from slot src to the same rows of slot dst (both the
// scheduler's) -- one k_kv_copy_rows launch enqueued on every stage's stream and NOT waited for: the step's pass runs behind it, and so does a
// later copy of the same step that reads what this one wrote.  *launches: the launches made.  On an error the streams are drained.
int sched_dev_copy_prefix(SchedDev *d, int32_t src, int32_t dst, int32_t row_begin, int32_t n_rows, int32_t *launches, char *err, size_t err_cap);

}  // namespace lh
