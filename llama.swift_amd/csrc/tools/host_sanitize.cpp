// host_sanitize.cpp -- the host half of the drop-in (model-file reader, tokenizer, sampler, generation driver) under
// AddressSanitizer + UndefinedBehaviorSanitizer ("race / memory-error detection").  Built by
// `make asan` with g++ -fsanitize=address,undefined from model_file.cpp + runner.cpp as they are; the device-side
// entry points the driver calls are replaced by stubs that parse the file and then fail like a box without a GPU, so
// the run exercises: header / vocabulary / tensor-directory parsing (valid, truncated and corrupted files), multi-part
// shard merging through read_tensor, llamahip_tokenize, llamahip_sample_top_p_top_k / _from_candidates, and the
// bridge's failure path, and -- with evals that succeed on made-up logits -- the driver's whole control flow (prompt taken at once,
// chunk-exact pass + last chunk, one eval per generated token, event counts).  usage: host_sanitize <model file> [n_parts]   (exit code 0 = clean)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/llama_runner.h"
#include "../../../include/llamahip.h"
#include "../dev_owner.h"
#include "../model_file.h"
#include "../q41_plan.h"
#include "../set_plan.h"
#include "../dec_attn_plan.h"
#include "../sched.h"

struct llamahip_model { lh::ModelFile file; lh::SchedDev *sched = nullptr; };

extern "C" {
int llamahip_model_load(const char *path, int32_t n_ctx, const llamahip_opts *opts, llamahip_model **out, char *err, size_t err_cap) {
    llamahip_model *m = new llamahip_model();
    std::string e;
    if (!m->file.open(path, n_ctx, opts ? opts->n_parts : 0, e)) { snprintf(err, err_cap, "%s", e.c_str()); delete m; *out = nullptr; return LLAMAHIP_ERR_LOAD; }
    *out = m;
    return 0;
}
void llamahip_model_free(llamahip_model *m) { delete m; }
int32_t llamahip_n_vocab(const llamahip_model *m) { return m ? m->file.hp.n_vocab : 0; }
const char *llamahip_token_text(const llamahip_model *m, int32_t id, uint32_t *len) {
    if (!m || id < 0 || id >= m->file.hp.n_vocab) return nullptr;
    if (len) *len = (uint32_t) m->file.id_to_token[id].size();
    return m->file.id_to_token[id].data();
}
// Two modes.  Default: every eval fails like a box without a GPU.  g_drive: evals SUCCEED with deterministic made-up logits and are
// logged, so that the generation driver's control flow (warm-up, the prompt taken at once and evaluated chunk-exactly, the last
// chunk's sampled logits, one eval per generated token, the event sequence) runs end to end on the host, under the sanitizers.
struct EvalCall { int kind /* 0 eval, 1 eval_chunks, 2 eval_topk, 3 decode_greedy (n steps), 4 verify_sample (n rows) */, n_past, n, chunk; };
static bool g_drive = false;
static std::vector<EvalCall> g_calls;
static int fake_eval(llamahip_model *m, int kind, int32_t np, const int32_t *t, int32_t n, int32_t chunk, float *lg, char *err, size_t err_cap) {
    if (!g_drive) { snprintf(err, err_cap, "no HIP device available: libllamahip has no CPU fallback"); return LLAMAHIP_ERR_PREDICT; }
    if (!m || !t || n < 1 || np < 0 || np + n > m->file.hp.n_ctx) { snprintf(err, err_cap, "context overflow: n_past (%d) + n_tokens (%d) > n_ctx (%d)", np, n, m ? m->file.hp.n_ctx : 0); return LLAMAHIP_ERR_PREDICT; }
    g_calls.push_back({ kind, np, n, chunk });
    const int V = m->file.hp.n_vocab;
    for (int i = 0; lg && i < V; i++) lg[i] = (float) (((uint32_t) i * 2654435761u + (uint32_t) (np + n) * 97u + (uint32_t) t[n - 1] * 13u) >> 20 & 0xffu) * 0.03125f;
    return 0;
}
int llamahip_eval(llamahip_model *m, int32_t, int32_t np, const int32_t *t, int32_t n, float *lg, char *err, size_t err_cap) { return fake_eval(m, 0, np, t, n, 0, lg, err, err_cap); }
int llamahip_eval_chunks(llamahip_model *m, int32_t, int32_t np, const int32_t *t, int32_t n, int32_t chunk, float *lg, char *err, size_t err_cap) { return fake_eval(m, 1, np, t, n, chunk, lg, err, err_cap); }
int llamahip_eval_topk(llamahip_model *m, int32_t, int32_t np, const int32_t *t, int32_t n, const int32_t *, int32_t, double, int32_t, double,
                       double *, int32_t *, int32_t *exact, float *lg, char *err, size_t err_cap) { *exact = 0; return fake_eval(m, 2, np, t, n, 0, lg, err, err_cap); }
// the driver's lookup steps: off in the runs above (no setter call, no LLAMAHIP_RUNNER_LOOKUP); in the overflow runs with lookup on the
// step succeeds on made-up draws -- every draft token accepted at odd positions, none at even ones -- refuses rows past the cache and is logged
int llamahip_verify_sample(llamahip_model *m, int32_t, int32_t np, int32_t token, const int32_t *draft, int32_t nd, llamahip_sampler *s, double, int32_t, double, double,
                           int32_t *n_accept, int32_t *picks, int32_t *, char *err, size_t err_cap) {
    if (!g_drive) { snprintf(err, err_cap, "no HIP device available: libllamahip has no CPU fallback"); return LLAMAHIP_ERR_PREDICT; }
    if (!m || !draft || nd < 1 || nd > 15 || np < 0 || np + nd + 1 > m->file.hp.n_ctx) { snprintf(err, err_cap, "context overflow: n_past (%d) + n_draft (%d) + 1 > n_ctx (%d)", np, nd, m ? m->file.hp.n_ctx : 0); return LLAMAHIP_ERR_PREDICT; }
    g_calls.push_back({ 4, np, nd + 1, 0 });
    const int V = m->file.hp.n_vocab, acc = np % 2 ? nd : 0;
    for (int j = 0; j < acc; j++) picks[j] = draft[j];
    picks[acc] = (int32_t) (((uint32_t) token * 31u + (uint32_t) np * 7u + 5u) % (uint32_t) V);
    for (int j = acc + 1; j <= nd; j++) picks[j] = -1;
    for (int j = 0; j <= acc; j++) llamahip_sampler_accept(s, picks[j]);
    *n_accept = acc;
    return 0;
}
// past the context window (ctx_overflow.cpp, the driver's overflow modes): the greedy leg makes up its picks
int32_t llamahip_n_ctx(const llamahip_model *m) { return m ? m->file.hp.n_ctx : 0; }
int llamahip_decode_greedy(llamahip_model *m, int32_t, int32_t np, int32_t first, int32_t n, int32_t *out, float *lg, char *err, size_t err_cap) {
    if (!g_drive) { snprintf(err, err_cap, "no HIP device available: libllamahip has no CPU fallback"); return LLAMAHIP_ERR_PREDICT; }
    if (!m || n < 1 || np < 0 || np + n > m->file.hp.n_ctx) { snprintf(err, err_cap, "context overflow: n_past (%d) + n_steps (%d) > n_ctx (%d)", np, n, m ? m->file.hp.n_ctx : 0); return LLAMAHIP_ERR_PREDICT; }
    g_calls.push_back({ 3, np, n, 0 });
    const int V = m->file.hp.n_vocab;
    for (int i = 0; i < n; i++) out[i] = (int32_t) (((uint32_t) (i ? out[i - 1] : first) * 31u + (uint32_t) (np + i) * 7u + 3u) % (uint32_t) V);
    for (int i = 0; lg && i < V; i++) lg[i] = (float) i;
    return 0;
}
// the in-place shift (LLAMAHIP_CTX_SHIFT): one shift of slot 0 per call, inside the cache on both sides; logged as kind 5 {first row, rows, n_discard}
int32_t llamahip_cur_seq(const llamahip_model *m) { return m ? 0 : -1; }
int llamahip_kv_shift_rows(llamahip_model *m, int32_t n, const int32_t *slot, const int32_t *row_begin, const int32_t *n_rows, const int32_t *n_discard, char *err, size_t err_cap) {
    if (!g_drive) { snprintf(err, err_cap, "no HIP device available: libllamahip has no CPU fallback"); return LLAMAHIP_ERR_PREDICT; }
    if (!m || n != 1 || !slot || !row_begin || !n_rows || !n_discard || slot[0] != 0 || n_discard[0] < 1 || n_rows[0] < 0 || row_begin[0] < n_discard[0] ||
        row_begin[0] + n_rows[0] > m->file.hp.n_ctx) { snprintf(err, err_cap, "llamahip_kv_shift_rows: shift outside [0, n_ctx (%d)]", m ? m->file.hp.n_ctx : 0); return LLAMAHIP_ERR_PREDICT; }
    g_calls.push_back({ 5, row_begin[0], n_rows[0], n_discard[0] });
    return 0;
}
}
namespace lh {
// eval_multi.cpp (compiled in as it is): what llamahip_eval_multi refuses of its arguments / llamahip_op_attention_rows of a caller's table
int eval_multi_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, int32_t n_seqs, const int32_t *slots, const int32_t *n_past,
                     const int32_t *tokens, const int32_t *n_tokens, int32_t chunk_tokens, char *err, size_t err_cap);
int rows_table_check(int32_t R, int32_t n_ctx, int32_t n_slots, const int32_t *row_slot, const int32_t *row_pos, const int32_t *row_keys, char *err, size_t err_cap);
// ... the host half of llamahip_eval_logprobs_multi / llamahip_score_choices: argument checks, the scored rows, the results back in row order
int score_multi_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, int32_t n_seqs, const int32_t *slots, const int32_t *n_past,
                      const int32_t *tokens, const int32_t *n_tokens, int32_t chunk_tokens, const int32_t *targets, char *err, size_t err_cap);
int32_t score_multi_rows(int32_t n_seqs, const int32_t *tokens, const int32_t *n_tokens, const int32_t *targets, int32_t *tgt, int32_t *scored);
void score_scatter(int32_t R, int32_t nl, const int32_t *scored, const void *packed, double *lp, int32_t *am, int32_t *rk);
int score_choices_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, const int32_t *context, int32_t n_context, int32_t n_choices,
                        const int32_t *endings, const int32_t *n_ending, int32_t chunk_tokens, char *err, size_t err_cap);
// ... and of llamahip_text_embedding[_multi] / llamahip_op_pool_rows
int embed_check(const char *fn, int32_t n_ctx, int32_t n_vocab, int32_t n_slots, int32_t sched_max_active, int32_t n_seqs, const int32_t *slots,
                const int32_t *n_past, const int32_t *tokens, const int32_t *n_tokens, int32_t chunk_tokens, int32_t pool, int32_t normalize,
                const float *out, char *err, size_t err_cap);
int pool_rows_check(const float *x, int32_t R, int32_t d, const float *norm_w, const int32_t *seg_begin, int32_t n_segs, int32_t pool, int32_t normalize,
                    const float *out, char *err, size_t err_cap);
int decode_handle_check(const llamahip_model *m, const char *fn, char *err, size_t err_cap) {
    if (!m) { snprintf(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    return 0;
}
// beam.cpp (compiled in as it is): what llamahip_beam_search refuses of its arguments, the ranking of its finished hypotheses
int beam_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, const llamahip_beam_opts *o, const int32_t *prompt, int32_t n_prompt,
               const void *hyps_out, const void *tokens_out, const void *n_hyps_out, char *err, size_t err_cap);
void beam_rank(int32_t n, const double *score, const int32_t *length, int32_t length_norm, int32_t *order);
}

// the request scheduler's device half (sched.h), stubbed: every planned step is logged segment by segment, exactly sized copies of what the host
// half handed over (so that a read past a request's tokens is the sanitizer's to see), and answered with made-up tokens
struct SchedCall { bool mixed; std::vector<lh::SchedSeg> segs; std::vector<std::vector<int32_t>> toks, drafts; };
static std::vector<SchedCall> g_sched_calls;
static bool g_sched_fail = false;          // the next steps fail like a device error: nothing of the host half's state may be lost
static bool g_sched_drafts = true;         // the stubbed handle takes drafted tokens (false: a fall-back handle)
static int g_sched_accept = -1;            // the script: draft tokens a segment accepts (cut to its draft); -1: (position + slot) % (n_draft + 1)
// shared prefixes: the copies the host half asked for, and a shadow cache [slot][row] (kept while non-empty) in which every row a step evaluates
// becomes a hash chained on the row below it in its slot -- a row shared or copied wrongly, or not at all, shows in every row above it
struct CopyCall { int32_t src, dst, row_begin, n_rows; size_t n_steps_before; };
static std::vector<CopyCall> g_sched_copies;
static bool g_sched_copy_fail = false;
static std::vector<std::vector<uint64_t>> g_vkv;
static uint64_t vkv_mix(uint64_t below, int32_t tok) { return (below ^ (uint64_t) (uint32_t) tok) * 0x9e3779b97f4a7c15ull + 0x7f4a7c15ull; }
static const uint64_t VKV_SEED = 0x1234567ull;
namespace lh {
struct SchedDev { int V; llamahip_model *m; };
int sched_handle_info(const llamahip_model *m, SchedHandleInfo *out, char *err, size_t err_cap) {
    if (!m) { snprintf(err, err_cap, "llamahip_sched_new: null model"); return LLAMAHIP_ERR_PREDICT; }
    *out = { m->file.hp.n_ctx, m->file.hp.n_vocab, 4 };
    return 0;
}
int sched_sampler_check(double repeat_penalty, int32_t top_k, double, double temp, char *err, size_t err_cap) {
    if (top_k < 1 || !(temp > 0.0) || !(repeat_penalty > 0.0)) { snprintf(err, err_cap, "llamahip_sched_new: sampler parameters"); return LLAMAHIP_ERR_PREDICT; }
    return 0;
}
int sched_dev_new(llamahip_model *m, const llamahip_sched_opts *, SchedDev **out, char *err, size_t err_cap) {
    *out = nullptr;
    if (m->sched) { snprintf(err, err_cap, "llamahip_sched_new: the handle already has a scheduler"); return LLAMAHIP_ERR_PREDICT; }
    *out = m->sched = new SchedDev{ m->file.hp.n_vocab, m };
    return 0;
}
void sched_dev_free(SchedDev *d) { if (d) d->m->sched = nullptr; delete d; }
int sched_dev_drafts(SchedDev *d) { return d && g_sched_drafts ? 1 : 0; }
static int32_t sched_made_up(const SchedDev *d, int32_t tok, int32_t pos) { return (int32_t) (((uint32_t) tok * 31u + (uint32_t) pos * 7u + 3u) % (uint32_t) d->V); }
int sched_dev_step(SchedDev *d, SchedSeg *segs, int32_t n_segs, bool mixed, int32_t *kind, int32_t *captures, char *err, size_t err_cap) {
    if (g_sched_fail) { snprintf(err, err_cap, "llamahip_sched_step: made-up device error"); return LLAMAHIP_ERR_PREDICT; }
    SchedCall c;
    c.mixed = mixed;
    for (int j = 0; j < n_segs; j++) {
        for (int r = 0; !g_vkv.empty() && r < segs[j].n_rows + segs[j].n_draft; r++) {
            std::vector<uint64_t> &rows = g_vkv[(size_t) segs[j].slot];
            const size_t row = (size_t) (segs[j].pos + r);
            rows.at(row) = vkv_mix(row ? rows[row - 1] : VKV_SEED, r < segs[j].n_rows ? segs[j].tokens[r] : segs[j].draft[r - segs[j].n_rows]);
        }
        c.toks.emplace_back(segs[j].tokens, segs[j].tokens + segs[j].n_rows);
        c.drafts.emplace_back(segs[j].draft, segs[j].draft + segs[j].n_draft);          // (exactly sized, as the rows' tokens)
        if (segs[j].cst && segs[j].emit) {
            // a constrained segment: the rule's pick (llamahip_constraint_pick) on a synthetic logits row per logits row of the segment -- made up
            // from the row's token and position, with ties, a NaN and a -0.0 in it -- under the state behind the draft tokens in front of it
            SchedSeg &g = segs[j];
            if (g.sampler || g.n_draft > 15 || (g.n_draft > 0 && (!mixed || g.n_rows != 1))) { snprintf(err, err_cap, "llamahip_sched_step: a constraint where none belongs"); return LLAMAHIP_ERR_PREDICT; }
            std::vector<float> row((size_t) d->V);
            int32_t st = g.cst_state, tok = c.toks.back().back();
            g.n_accept = 0;
            for (int i = 0; i <= g.n_draft; i++) {
                for (int v = 0; v < d->V; v++) row[(size_t) v] = (float) (sched_made_up(d, tok + v, g.pos + g.n_rows + i) % 17) - 8.0f;
                row[(size_t) (tok % d->V)] = NAN; row[(size_t) ((tok + 1) % d->V)] = -0.0f;
                const int32_t p = llamahip_constraint_pick(g.cst, st, row.data());
                if (p < 0) { snprintf(err, err_cap, "llamahip_sched_step: a pick found no allowed token"); return LLAMAHIP_ERR_PREDICT; }
                g.toks[i] = p; g.exacts[i] = 1; g.n_accept = i;
                if (i == g.n_draft || p != g.draft[i]) break;
                st = llamahip_constraint_advance(g.cst, st, p);
                tok = p;
            }
            g.token = g.toks[0]; g.exact = 1;
        } else if (segs[j].n_draft > 0) {
            // the scripted number of draft tokens accepted, then a made-up token that is not the draft's next one
            SchedSeg &g = segs[j];
            if (!mixed || !g.emit || g.n_rows != 1 || g.n_draft > 15) { snprintf(err, err_cap, "llamahip_sched_step: a draft where none belongs"); return LLAMAHIP_ERR_PREDICT; }
            g.n_accept = std::min(g.n_draft, g_sched_accept >= 0 ? g_sched_accept : (g.pos + g.slot) % (g.n_draft + 1));
            for (int a = 0; a < g.n_accept; a++) g.toks[a] = c.drafts.back()[(size_t) a];
            int32_t t = sched_made_up(d, g.n_accept ? g.toks[g.n_accept - 1] : c.toks.back()[0], g.pos + g.n_accept + 1);
            if (g.n_accept < g.n_draft && t == c.drafts.back()[(size_t) g.n_accept]) t = (t + 1) % d->V;
            g.toks[g.n_accept] = t;
            for (int a = 0; a <= g.n_accept; a++) { g.exacts[a] = 1; if (g.sampler) llamahip_sampler_accept(g.sampler, g.toks[a]); }
            g.token = g.toks[0]; g.exact = 1;
        } else if (segs[j].emit) {
            segs[j].token = sched_made_up(d, c.toks.back().back(), segs[j].pos + segs[j].n_rows);
            segs[j].exact = 1;
            if (segs[j].sampler) llamahip_sampler_accept(segs[j].sampler, segs[j].token);
        }
        c.segs.push_back(segs[j]);
    }
    g_sched_calls.push_back(std::move(c));
    *kind = mixed ? SCHED_STEP_MIXED : n_segs >= 2 ? SCHED_STEP_SET : SCHED_STEP_SINGLE;
    *captures = 0;
    return 0;
}
int sched_dev_copy_prefix(SchedDev *, int32_t src, int32_t dst, int32_t row_begin, int32_t n_rows, int32_t *launches, char *err, size_t err_cap) {
    *launches = 0;
    if (g_sched_copy_fail) { snprintf(err, err_cap, "llamahip_sched_step: made-up device error in a prefix copy"); return LLAMAHIP_ERR_PREDICT; }
    g_sched_copies.push_back({ src, dst, row_begin, n_rows, g_sched_calls.size() });
    for (int r = 0; !g_vkv.empty() && r < n_rows; r++) g_vkv.at((size_t) dst).at((size_t) (row_begin + r)) = g_vkv.at((size_t) src).at((size_t) (row_begin + r));
    *launches = 1;
    return 0;
}
}

// DevOwner's allocator over malloc / free: counts the calls by kind and fails the k-th allocation like a device that ran out of memory
static int g_own_calls = 0, g_own_fail_at = 0, g_own_allocs[3], g_own_releases[3];
static int own_stub_alloc(void **p, size_t bytes, int kind, bool zero) {
    *p = nullptr;
    if (++g_own_calls == g_own_fail_at) return 2;
    *p = zero ? calloc(1, bytes ? bytes : 1) : malloc(bytes ? bytes : 1);
    g_own_allocs[kind]++;
    return *p ? 0 : 2;
}
static void own_stub_release(void *p, int kind) { g_own_releases[kind]++; free(p); }

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "host_sanitize: FAILED %s (line %d)\n", #c, __LINE__); failures++; } } while (0)

// scoring over several KV slots (llamahip_eval_logprobs_multi / llamahip_score_choices): the argument checks on exactly sized arrays and
// exactly sized message buffers (every refusal, at buffers too short for its message and with none), the scored rows against the rule
// restated, and the compacted results scattered back to row order from a buffer of exactly 16 bytes per scored row
__attribute__((noinline)) static void scoring_host_half(int V) {          // (its own frame: main is as large as the compiler's variable tracking takes)
    char err[512] = { 0 };
    long n_checks = 0, n_scatter = 0;
    auto refused = [&](auto call) {          // call(err, cap): refused with a message that fits a buffer of 1, 24 and 400 bytes, and with no buffer
        for (size_t cap : { (size_t) 1, (size_t) 24, (size_t) 400 }) {
            std::vector<char> e(cap, 'x');
            EXPECT(call(e.data(), cap) == LLAMAHIP_ERR_PREDICT);
            EXPECT(memchr(e.data(), 0, cap) != nullptr);
            if (cap == 400) EXPECT(strstr(e.data(), "llamahip_eval_logprobs_multi") || strstr(e.data(), "llamahip_score_choices"));
            n_checks++;
        }
        EXPECT(call(nullptr, 0) == LLAMAHIP_ERR_PREDICT);
    };
    for (int C : { 64, 128 })
        for (int n = 1; n <= 5; n++)
            for (int mode = 0; mode < 5; mode++) {          // targets: null | every row | scattered -1 rows | one segment unscored | none at all
                static const int lens[6] = { 1, 2, 9, 10, 18, 61 }, pasts[3] = { 0, 3, 37 };
                std::vector<int32_t> np((size_t) n), nt((size_t) n), slots((size_t) n);
                int R = 0;
                bool fits = true;
                for (int i = 0; i < n; i++) { np[i] = pasts[(mode + i) % 3]; nt[i] = lens[(mode * 5 + i) % 6]; slots[i] = n - 1 - i; R += nt[i]; fits = fits && np[i] + nt[i] <= C; }
                std::vector<int32_t> toks((size_t) R), tg((size_t) R);
                for (int r = 0; r < R; r++) toks[r] = (r * 7 + 3) % V;
                for (int r = 0, i = 0, j = 0; r < R; r++) {
                    tg[r] = mode == 1 ? (r * 5 + 1) % V : mode == 2 ? (r % 3 == 1 ? -1 : (r * 5 + 1) % V) : mode == 3 ? (i == n / 2 ? -1 : V - 1) : -1;
                    if (++j == nt[i]) { j = 0; i++; }
                }
                const int32_t *targets = mode == 0 ? nullptr : tg.data();
                EXPECT((lh::score_multi_check(C, V, n, n, slots.data(), np.data(), toks.data(), nt.data(), 0, targets, err, sizeof(err)) == 0) == fits);
                if (!fits) { refused([&](char *e, size_t cap) { return lh::score_multi_check(C, V, n, n, slots.data(), np.data(), toks.data(), nt.data(), 0, targets, e, cap); }); continue; }
                std::vector<int32_t> tgt((size_t) R), scored((size_t) R);
                const int32_t nl = lh::score_multi_rows(n, toks.data(), nt.data(), targets, tgt.data(), scored.data());
                int want_nl = 0;
                for (int r = 0, i = 0, j = 0; r < R; r++) {
                    const int32_t want = targets ? targets[r] : (j + 1 < nt[i] ? toks[r + 1] : -1);
                    EXPECT(tgt[r] == want);
                    if (want >= 0) { EXPECT(want_nl < nl && scored[want_nl] == r); want_nl++; }
                    if (++j == nt[i]) { j = 0; i++; }
                }
                EXPECT(nl == want_nl && (mode != 4 || nl == 0) && (mode != 1 || nl == R));
                // made-up results of the nl scored rows, exactly 16 nl bytes, back to row order
                std::vector<char> packed((size_t) nl * 16);
                for (int k = 0; k < nl; k++) {
                    const double l = -0.5 * (k + 1); const int32_t a = 1000 + k, q = k % 4;
                    memcpy(packed.data() + (size_t) k * 8, &l, 8);
                    memcpy(packed.data() + (size_t) nl * 8 + (size_t) k * 4, &a, 4);
                    memcpy(packed.data() + (size_t) nl * 12 + (size_t) k * 4, &q, 4);
                }
                std::vector<double> lp((size_t) R, 7.0);
                std::vector<int32_t> am((size_t) R, 7), rk((size_t) R, 7);
                lh::score_scatter(R, nl, scored.data(), packed.data(), lp.data(), am.data(), rk.data());
                for (int r = 0, k = 0; r < R; r++) {
                    if (tgt[r] >= 0) { EXPECT(lp[r] == -0.5 * (k + 1) && am[r] == 1000 + k && rk[r] == k % 4); k++; }
                    else EXPECT(lp[r] == 0.0 && am[r] == -1 && rk[r] == -1);
                }
                lh::score_scatter(R, nl, scored.data(), packed.data(), nullptr, nullptr, nullptr);
                lh::score_scatter(R, nl, scored.data(), packed.data(), lp.data(), nullptr, rk.data());
                n_scatter++;
                // the refusals: a target of n_vocab and of -2, then eval_multi_check's rules under this function's name
                if (mode == 0) continue;
                const int32_t keep = tg[R - 1];
                for (int32_t bad : { V, -2 }) {
                    tg[R - 1] = bad;
                    refused([&](char *e, size_t cap) { return lh::score_multi_check(C, V, n, n, slots.data(), np.data(), toks.data(), nt.data(), 0, tg.data(), e, cap); });
                }
                tg[R - 1] = keep;
                refused([&](char *e, size_t cap) { return lh::score_multi_check(C, V, n, n, slots.data(), np.data(), toks.data(), nt.data(), -1, tg.data(), e, cap); });
                refused([&](char *e, size_t cap) { return lh::score_multi_check(C, V, n - 1, n, slots.data(), np.data(), toks.data(), nt.data(), 0, tg.data(), e, cap); });
                refused([&](char *e, size_t cap) { return lh::score_multi_check(C, V, n, 0, slots.data(), np.data(), toks.data(), nt.data(), 0, tg.data(), e, cap); });
                if (n > 1) { slots[n - 1] = slots[0]; refused([&](char *e, size_t cap) { return lh::score_multi_check(C, V, n, n, slots.data(), np.data(), toks.data(), nt.data(), 0, tg.data(), e, cap); }); slots[n - 1] = 0; }
                nt[0] = 0;
                refused([&](char *e, size_t cap) { return lh::score_multi_check(C, V, n, n, slots.data(), np.data(), toks.data(), nt.data(), 0, tg.data(), e, cap); });
            }
    {   // one row more than a pass takes
        const int32_t slot0[1] = { 0 }, np0[1] = { 0 }, big[1] = { LLAMAHIP_EVAL_MULTI_MAX_ROWS + 1 };
        std::vector<int32_t> toks((size_t) big[0], 1);
        refused([&](char *e, size_t cap) { return lh::score_multi_check(4096, V, 1, 1, slot0, np0, toks.data(), big, 0, nullptr, e, cap); });
    }
    // llamahip_score_choices: contexts of 1, 10 and 40 tokens, 1 .. 16 endings, accepted; then every refusal
    for (int nc : { 1, 10, 40 })
        for (int n : { 1, 4, 16 }) {
            std::vector<int32_t> ctx((size_t) nc, 2), ne((size_t) n);
            int E = 0;
            for (int i = 0; i < n; i++) { ne[i] = 1 + (i * 3) % 7; E += ne[i]; }
            std::vector<int32_t> ends((size_t) E, 3);
            EXPECT(lh::score_choices_check(64, V, 16, ctx.data(), nc, n, ends.data(), ne.data(), 9, err, sizeof(err)) == 0);
            EXPECT(lh::score_choices_check(64, V, 16, ctx.data(), nc, n, ends.data(), ne.data(), 0, nullptr, 0) == 0);
            refused([&](char *e, size_t cap) { return lh::score_choices_check(64, V, 16, ctx.data(), 0, n, ends.data(), ne.data(), 0, e, cap); });
            refused([&](char *e, size_t cap) { return lh::score_choices_check(64, V, 16, ctx.data(), nc, 0, ends.data(), ne.data(), 0, e, cap); });
            refused([&](char *e, size_t cap) { return lh::score_choices_check(64, V, 32, ctx.data(), nc, 17, ends.data(), ne.data(), 0, e, cap); });
            refused([&](char *e, size_t cap) { return lh::score_choices_check(64, V, n - 1, ctx.data(), nc, n, ends.data(), ne.data(), 0, e, cap); });
            refused([&](char *e, size_t cap) { return lh::score_choices_check(64, V, 16, ctx.data(), nc, n, ends.data(), ne.data(), -1, e, cap); });
            refused([&](char *e, size_t cap) { return lh::score_choices_check(nc - 1 + ne[n - 1] - 1, V, 16, ctx.data(), nc, n, ends.data(), ne.data(), 0, e, cap); });
            refused([&](char *e, size_t cap) { return lh::score_choices_check(64, V, 16, nullptr, nc, n, ends.data(), ne.data(), 0, e, cap); });
            ctx[(size_t) nc - 1] = V;
            refused([&](char *e, size_t cap) { return lh::score_choices_check(64, V, 16, ctx.data(), nc, n, ends.data(), ne.data(), 0, e, cap); });
            ctx[(size_t) nc - 1] = 2; ends[(size_t) E - 1] = -1;
            refused([&](char *e, size_t cap) { return lh::score_choices_check(64, V, 16, ctx.data(), nc, n, ends.data(), ne.data(), 0, e, cap); });
            ends[(size_t) E - 1] = 3; ne[n - 1] = 0;          // an empty ending (the last one: no array is read past its end)
            refused([&](char *e, size_t cap) { return lh::score_choices_check(64, V, 16, ctx.data(), nc, n, ends.data(), ne.data(), 0, e, cap); });
        }
    printf("host_sanitize: scoring over KV slots: %ld refusals at short and missing message buffers, %ld scatters of compacted results against the rule restated\n", n_checks, n_scatter);
}

// text embeddings (llamahip_text_embedding[_multi] / llamahip_op_pool_rows): the argument checks on exactly sized arrays, every refusal at
// message buffers too short for its message and with none
__attribute__((noinline)) static void embedding_host_half(int V) {
    long n_checks = 0;
    auto refused = [&](const char *fn, auto call) {
        for (size_t cap : { (size_t) 1, (size_t) 24, (size_t) 400 }) {
            std::vector<char> e(cap, 'x');
            EXPECT(call(e.data(), cap) == LLAMAHIP_ERR_PREDICT);
            EXPECT(memchr(e.data(), 0, cap) != nullptr);
            if (cap == 400) EXPECT(strstr(e.data(), fn) != nullptr);
            n_checks++;
        }
        EXPECT(call(nullptr, 0) == LLAMAHIP_ERR_PREDICT);
        n_checks++;
    };
    static const char *fm = "llamahip_text_embedding_multi", *f1 = "llamahip_text_embedding", *fo = "llamahip_op_pool_rows";
    const int C = 64;
    float out1[1] = { 0.f };
    for (int n : { 1, 3, 16 }) {
        std::vector<int32_t> slots((size_t) n), np((size_t) n), nt((size_t) n);
        int R = 0;
        for (int i = 0; i < n; i++) { slots[i] = n - 1 - i; np[i] = i % 5; nt[i] = 1 + (i * 7) % 11; R += nt[i]; }
        std::vector<int32_t> toks((size_t) R, V - 1);
        char err[256];
        for (int pool : { 0, 1 })
            for (int nrm : { 0, 1 }) {
                EXPECT(lh::embed_check(fm, C, V, n, 0, n, slots.data(), np.data(), toks.data(), nt.data(), 9, pool, nrm, out1, err, sizeof(err)) == 0);
                EXPECT(lh::embed_check(fm, C, V, n, 0, n, slots.data(), np.data(), toks.data(), nt.data(), 0, pool, nrm, out1, nullptr, 0) == 0);
            }
        auto chk = [&](int n_slots, int sched, int n_seqs, int chunk, int pool, int nrm, const float *out) {
            return [=, &slots, &np, &toks, &nt](char *e, size_t cap) { return lh::embed_check(fm, C, V, n_slots, sched, n_seqs, slots.data(), np.data(), toks.data(), nt.data(), chunk, pool, nrm, out, e, cap); };
        };
        refused(fm, chk(n, 0, n, 0, 2, 0, out1));
        refused(fm, chk(n, 0, n, 0, -1, 0, out1));
        refused(fm, chk(n, 0, n, 0, 0, 2, out1));
        refused(fm, chk(n, 0, n, 0, 1, -1, out1));
        refused(fm, chk(n, 0, n, 0, 1, 1, nullptr));
        refused(fm, chk(n, 1, n, 0, 1, 1, out1));          // (slot 0 is named and is the scheduler's)
        refused(fm, chk(n, 0, n, -1, 0, 0, out1));
        refused(fm, chk(n - 1, 0, n, 0, 0, 0, out1));
        refused(fm, chk(n, 0, 0, 0, 0, 0, out1));
        toks[(size_t) R - 1] = V;
        refused(fm, chk(n, 0, n, 0, 0, 0, out1));
        toks[(size_t) R - 1] = 0; np[n - 1] = C;
        refused(fm, chk(n, 0, n, 0, 0, 0, out1));
        np[n - 1] = 0;
        if (n > 1) { slots[n - 1] = slots[0]; refused(fm, chk(n, 0, n, 0, 0, 0, out1)); slots[n - 1] = 0; }
        nt[n - 1] = 0;          // (the last segment: no array is read past its end)
        refused(fm, chk(n, 0, n, 0, 0, 0, out1));
    }
    {   // the single text: one segment on the current slot
        const int32_t slot = 2, past = 3, N = 5, toks[5] = { 1, 2, 3, 4, 5 };
        char err[256];
        EXPECT(lh::embed_check(f1, C, V, 4, 2, 1, &slot, &past, toks, &N, 0, 1, 1, out1, err, sizeof(err)) == 0);
        refused(f1, [&](char *e, size_t cap) { return lh::embed_check(f1, C, V, 4, 3, 1, &slot, &past, toks, &N, 0, 1, 1, out1, e, cap); });
        refused(f1, [&](char *e, size_t cap) { return lh::embed_check(f1, C, V, 4, 0, 1, &slot, &past, toks, &N, 0, 3, 0, out1, e, cap); });
        refused(f1, [&](char *e, size_t cap) { return lh::embed_check(f1, C, V, 4, 0, 1, &slot, &past, nullptr, &N, 0, 0, 0, out1, e, cap); });
        const int32_t far = C - 4;
        refused(f1, [&](char *e, size_t cap) { return lh::embed_check(f1, C, V, 4, 0, 1, &slot, &far, toks, &N, 0, 0, 0, out1, e, cap); });
    }
    {   // llamahip_op_pool_rows: x, norm_w and out are not read by the check
        const float x[1] = { 0.f }, w[1] = { 0.f };
        char err[256];
        for (int n : { 1, 5, 16 }) {
            std::vector<int32_t> seg((size_t) n + 1);
            for (int i = 0; i <= n; i++) seg[i] = i * 3;
            const int R = 3 * n;
            EXPECT(lh::pool_rows_check(x, R, 96, w, seg.data(), n, 1, 1, out1, err, sizeof(err)) == 0);
            EXPECT(lh::pool_rows_check(x, R, 32, w, seg.data(), n, 0, 0, out1, nullptr, 0) == 0);
            auto chk = [&](const float *xx, int RR, int d, const float *ww, int ns, int pool, int nrm, const float *out) {
                return [=, &seg](char *e, size_t cap) { return lh::pool_rows_check(xx, RR, d, ww, seg.data(), ns, pool, nrm, out, e, cap); };
            };
            refused(fo, chk(nullptr, R, 32, w, n, 0, 0, out1));
            refused(fo, chk(x, R, 32, nullptr, n, 0, 0, out1));
            refused(fo, chk(x, R, 32, w, n, 0, 0, nullptr));
            refused(fo, [&](char *e, size_t cap) { return lh::pool_rows_check(x, R, 32, w, nullptr, n, 0, 0, out1, e, cap); });
            refused(fo, chk(x, 0, 32, w, n, 0, 0, out1));
            refused(fo, chk(x, LLAMAHIP_EVAL_MULTI_MAX_ROWS + 1, 32, w, n, 0, 0, out1));
            refused(fo, chk(x, R, 0, w, n, 0, 0, out1));
            refused(fo, chk(x, R, 16, w, n, 0, 0, out1));
            refused(fo, chk(x, R, 48, w, n, 0, 0, out1));
            refused(fo, chk(x, R, 32, w, 0, 0, 0, out1));
            refused(fo, chk(x, R, 32, w, n, 2, 0, out1));
            refused(fo, chk(x, R, 32, w, n, 0, 2, out1));
            refused(fo, chk(x, R + 1, 32, w, n, 0, 0, out1));          // (seg_begin ends below R)
            seg[0] = 1;
            refused(fo, chk(x, R, 32, w, n, 0, 0, out1));
            seg[0] = 0;
            if (n > 1) { const int32_t keep = seg[1]; seg[1] = seg[2]; refused(fo, chk(x, R, 32, w, n, 0, 0, out1)); seg[1] = 0; refused(fo, chk(x, R, 32, w, n, 0, 0, out1)); seg[1] = keep; }
        }
        std::vector<int32_t> seg17(18);
        for (int i = 0; i <= 17; i++) seg17[i] = i;
        refused(fo, [&](char *e, size_t cap) { return lh::pool_rows_check(x, 17, 32, w, seg17.data(), 17, 0, 0, out1, e, cap); });
    }
    printf("host_sanitize: text embeddings: %ld refusals at short and missing message buffers\n", n_checks);
}

// beam search (llamahip_beam_search): the step rule and the slots on exactly sized arrays over a grid of beam counts, candidate tables with
// ties, stop candidates, NaN candidates and dead beams, against the rules restated; the argument check at short and missing message buffers;
// the ranking with ties
__attribute__((noinline)) static void beam_host_half(int V) {
    long n_sel = 0, n_slots = 0, n_checks = 0;
    uint32_t rng = 12345u;
    auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 8; };
    for (int B = 1; B <= LLAMAHIP_BEAM_MAX; B++)
        for (int L = 0; L <= B; L++)
            for (int rep = 0; rep < 6; rep++) {
                const int nc = 2 * B, stop = rep % 3 == 0 ? -1 : (int) (next() % 7);
                std::vector<double> sc((size_t) L), lp((size_t) L * nc);
                std::vector<int32_t> ids((size_t) L * nc);
                int want_dead = 0;
                for (int i = 0; i < L; i++) {
                    sc[i] = -0.25 * (double) (next() % 5);
                    const bool dead = rep == 4 && next() % 3 == 0;
                    want_dead += dead;
                    for (int j = 0; j < nc; j++) {
                        ids[(size_t) i * nc + j] = dead ? -1 : (int32_t) ((j * 3 + next() % 3) % 97);      // (ascending-ish, a stop id among them)
                        lp[(size_t) i * nc + j] = dead || (rep == 5 && next() % 4 == 0) ? NAN : -0.25 * (double) (j / 2) - (rep == 2 && j >= nc - 2 ? INFINITY : 0.0);
                    }
                    if (!dead) for (int j = 1; j < nc; j++) if (ids[(size_t) i * nc + j] <= ids[(size_t) i * nc + j - 1]) ids[(size_t) i * nc + j] = ids[(size_t) i * nc + j - 1] + 1;
                }
                std::vector<int32_t> par((size_t) B, -7), tok((size_t) B, -7), fpar((size_t) std::max(L, 1), -7);
                std::vector<double> nsc((size_t) B, 7.0), fsc((size_t) std::max(L, 1), 7.0);
                int32_t nn = -1, nf = -1, nd = -1;
                EXPECT(llamahip_beam_select(L, sc.data(), nc, ids.data(), lp.data(), B, stop, par.data(), tok.data(), nsc.data(), &nn, fpar.data(), fsc.data(), &nf, &nd) == 0);
                EXPECT(nd == want_dead && nn >= 0 && nn <= B && nf >= 0 && nf <= L);
                // the rule restated: every taken entry is a candidate, the walk's order is (c desc, i asc, v asc), nothing better was left out
                double prev_c = INFINITY;
                for (int k = 0; k < nn; k++) {
                    EXPECT(par[k] >= 0 && par[k] < L && tok[k] != stop && nsc[k] == nsc[k] && nsc[k] <= prev_c);
                    prev_c = nsc[k];
                    bool found = false;
                    for (int j = 0; j < nc && par[k] >= 0 && par[k] < L; j++)
                        found = found || (ids[(size_t) par[k] * nc + j] == tok[k] && sc[par[k]] + lp[(size_t) par[k] * nc + j] == nsc[k]);
                    EXPECT(found);
                }
                int n_valid = 0;
                for (int i = 0; i < L; i++)
                    for (int j = 0; j < nc; j++) {
                        const double c = sc[i] + lp[(size_t) i * nc + j];
                        const int32_t v = ids[(size_t) i * nc + j];
                        if (ids[(size_t) i * nc] < 0 || v < 0 || c != c) continue;
                        if (stop >= 0 && v == stop) { if (nn < B || c > nsc[nn - 1]) { bool in = false; for (int k = 0; k < nf; k++) in = in || (fpar[k] == i && fsc[k] == c); EXPECT(in); } continue; }
                        n_valid++;
                        if (nn == B) EXPECT(c <= nsc[nn - 1] || [&]() { for (int k = 0; k < nn; k++) if (par[k] == i && tok[k] == v) return true; return false; }());
                    }
                EXPECT(nn == std::min(B, n_valid));
                n_sel++;
                // the slots of those beams: the previous beams on a made-up permutation of distinct slots
                std::vector<int32_t> prev((size_t) L), ns((size_t) std::max(nn, 1), -7), cs((size_t) std::max(nn, 1), -7), cd((size_t) std::max(nn, 1), -7);
                for (int i = 0; i < L; i++) prev[i] = (i * 5 + rep) % B;
                bool distinct = true;
                for (int i = 0; i < L; i++) for (int j = 0; j < i; j++) distinct = distinct && prev[i] != prev[j];
                const int32_t ncp = llamahip_beam_slots(L, prev.data(), nn, par.data(), B, ns.data(), cs.data(), cd.data());
                if (!distinct) { EXPECT(ncp == -1); continue; }
                EXPECT(ncp >= 0 && ncp <= nn);
                for (int k = 0; k < nn; k++) for (int j = 0; j < k; j++) EXPECT(ns[k] != ns[j]);
                for (int c = 0; c < ncp; c++) {
                    for (int e = 0; e < ncp; e++) EXPECT(cs[c] != cd[e]);      // sources are never destinations
                    for (int e = 0; e < c; e++) EXPECT(cd[c] != cd[e]);
                }
                int firsts = 0;
                for (int k = 0; k < nn; k++) { bool first = true; for (int j = 0; j < k; j++) first = first && par[j] != par[k]; if (first) { EXPECT(ns[k] == prev[par[k]]); firsts++; } }
                EXPECT(ncp == nn - firsts);
                n_slots++;
            }
    {   // what the two refuse: counts out of range, null arrays
        double d1[2] = { 0, 0 }; int32_t i1[2] = { 1, 2 }, n = 0;
        EXPECT(llamahip_beam_select(17, d1, 2, i1, d1, 1, -1, i1, i1, d1, &n, i1, d1, &n, nullptr) != 0);
        EXPECT(llamahip_beam_select(1, d1, 33, i1, d1, 1, -1, i1, i1, d1, &n, i1, d1, &n, nullptr) != 0);
        EXPECT(llamahip_beam_select(1, d1, 2, i1, d1, 0, -1, i1, i1, d1, &n, i1, d1, &n, nullptr) != 0);
        EXPECT(llamahip_beam_select(1, nullptr, 2, i1, d1, 1, -1, i1, i1, d1, &n, i1, d1, &n, nullptr) != 0);
        EXPECT(llamahip_beam_slots(1, i1, 1, i1, 17, i1, i1, i1) == -1 && llamahip_beam_slots(2, i1, 1, i1, 1, i1, i1, i1) == -1);
        int32_t bad_par[1] = { 3 }, prev1[1] = { 0 }, o1[1], o2[1], o3[1];
        EXPECT(llamahip_beam_slots(1, prev1, 1, bad_par, 4, o1, o2, o3) == -1);
    }
    // the argument check: every refusal with a message that fits a buffer of 1, 24 and 400 bytes, and with no buffer
    llamahip_beam_opts ok = { (int32_t) sizeof(llamahip_beam_opts), 8, 4, 12, -1, 0, 0, 9 };
    std::vector<int32_t> prompt(20);
    for (int i = 0; i < 20; i++) prompt[i] = (i * 7 + 3) % V;
    int32_t out_i[4]; char out_h[4];
    EXPECT(lh::beam_check(64, V, 4, &ok, prompt.data(), 20, out_h, out_i, out_i, nullptr, 0) == 0);
    auto refused = [&](llamahip_beam_opts o, int n_prompt, int n_slots_, const int32_t *p) {
        for (size_t cap : { (size_t) 1, (size_t) 24, (size_t) 400 }) {
            std::vector<char> e(cap, 'x');
            EXPECT(lh::beam_check(64, V, n_slots_, &o, p, n_prompt, out_h, out_i, out_i, e.data(), cap) == LLAMAHIP_ERR_PREDICT);
            EXPECT(memchr(e.data(), 0, cap) != nullptr);
            if (cap == 400) EXPECT(strstr(e.data(), "llamahip_beam_search") != nullptr);
            n_checks++;
        }
        EXPECT(lh::beam_check(64, V, n_slots_, &o, p, n_prompt, out_h, out_i, out_i, nullptr, 0) == LLAMAHIP_ERR_PREDICT);
    };
    { auto o = ok; o.n_beams = 0; refused(o, 20, 4, prompt.data()); o.n_beams = 17; refused(o, 20, 32, prompt.data()); o.n_beams = 5; refused(o, 20, 4, prompt.data()); }
    { auto o = ok; o.struct_size = 8; refused(o, 20, 4, prompt.data()); }
    { auto o = ok; o.n_predict = 0; refused(o, 20, 4, prompt.data()); o.n_predict = 45; refused(o, 20, 4, prompt.data()); }
    { auto o = ok; o.n_return = 5; refused(o, 20, 4, prompt.data()); o.n_return = -1; refused(o, 20, 4, prompt.data()); }
    { auto o = ok; o.chunk_tokens = -1; refused(o, 20, 4, prompt.data()); o = ok; o.length_norm = 2; refused(o, 20, 4, prompt.data()); o = ok; o.stop_token = V; refused(o, 20, 4, prompt.data()); }
    refused(ok, 0, 4, prompt.data());
    refused(ok, 20, 4, nullptr);
    { std::vector<int32_t> p2(prompt); p2[19] = V; refused(ok, 20, 4, p2.data()); }
    EXPECT(lh::beam_check(64, 7, 4, &ok, prompt.data(), 20, out_h, out_i, out_i, nullptr, 0) == LLAMAHIP_ERR_PREDICT);      // 2 * 4 candidates > 7
    {   // the ranking: ties to the earlier entry, one division for the normalised key
        const double S[5] = { -2.0, -1.0, -2.0, -1.0, -3.0 }; const int32_t len[5] = { 4, 2, 2, 1, 3 }; int32_t order[5];
        lh::beam_rank(5, S, len, 0, order);
        EXPECT(order[0] == 1 && order[1] == 3 && order[2] == 0 && order[3] == 2 && order[4] == 4);
        lh::beam_rank(5, S, len, 1, order);      // keys -0.5 -0.5 -1 -1 -1
        EXPECT(order[0] == 0 && order[1] == 1 && order[2] == 2 && order[3] == 3 && order[4] == 4);
        lh::beam_rank(0, S, len, 1, order);
    }
    printf("host_sanitize: beam search: %ld walks and %ld slot assignments against the rules restated, %ld refusals at short and missing message buffers\n", n_sel, n_slots, n_checks);
}

// constrained decoding (constrain.cpp, compiled in as it is): the lift on the model file's vocabulary against the rule restated entry by entry,
// on exactly sized arrays; a prune case (a state no token leads out of: its row and every way into it banned, as a start refused); every
// refusal at message buffers too short for its text and with none; the choices builder against the walk of its strings; pick / mask_row /
// advance at their edges (ties, signed zeros, NaN, all allowed entries NaN, states and tokens out of range)
__attribute__((noinline)) static void constrain_host_half(const llamahip_model *m, int V) {
    long n_entries = 0, n_checks = 0, n_picks = 0;
    const int32_t stop = 2;
    // bytes of the vocabulary's words: a .. z, the space, "tok" and digits.  0: start; 1: behind letters (accepting); 2: behind a space; 3: trap
    const int S = 4;
    std::vector<int32_t> trans((size_t) S * 256, -1);
    std::vector<uint8_t> accept = { 0, 1, 0, 0 };
    for (int b = 'a'; b <= 'z'; b++) { trans[0 * 256 + b] = 1; trans[1 * 256 + b] = 1; trans[2 * 256 + b] = 1; }
    trans[1 * 256 + ' '] = 2;
    for (int b = '0'; b <= '9'; b++) trans[1 * 256 + b] = 1;
    trans[0 * 256 + ' '] = 3; trans[3 * 256 + ' '] = 3;      // the trap: enterable, never left towards an accepting state
    llamahip_constraint *c = nullptr;
    char err[256];
    EXPECT(llamahip_constraint_new(m, S, trans.data(), accept.data(), 0, stop, &c, err, sizeof(err)) == 0 && c);
    if (c) {
        EXPECT(llamahip_constraint_n_states(c) == S + 1 && llamahip_constraint_start(c) == 0 && llamahip_constraint_done(c) == S);
        const int64_t n = llamahip_constraint_table(c, nullptr, 0);
        EXPECT(n == (int64_t) (S + 1) * V);
        std::vector<uint16_t> tab((size_t) n), small((size_t) n - 1, 7);
        EXPECT(llamahip_constraint_table(c, small.data(), n - 1) == n && small[0] == 7);      // too small: the count, nothing copied
        EXPECT(llamahip_constraint_table(c, tab.data(), n) == n);
        for (int s = 0; s <= S; s++)
            for (int t = 0; t < V; t++) {
                uint32_t len = 0;
                const uint8_t *text = (const uint8_t *) llamahip_token_text(m, t, &len);
                int want = -1;
                if (s == S) want = t == stop ? S : -1;
                else if (t == stop) want = accept[(size_t) s] ? S : -1;
                else if (len > 0) {
                    int q = s;
                    for (uint32_t k = 0; k < len && q >= 0; k++) q = trans[(size_t) q * 256 + text[k]];
                    want = q == 3 ? -1 : q;      // the prune: the trap is not live
                }
                if (s == 3) want = -1;           // ... and nothing leaves it
                EXPECT(tab[(size_t) s * V + t] == (want < 0 ? LLAMAHIP_CONSTRAINT_BANNED : want));
                EXPECT(llamahip_constraint_advance(c, s, t) == want);
                n_entries++;
            }
        EXPECT(llamahip_constraint_advance(c, -1, 3) == -1 && llamahip_constraint_advance(c, S + 1, 3) == -1 && llamahip_constraint_advance(c, 0, V) == -1 && llamahip_constraint_advance(c, 0, -1) == -1);
        // pick and mask_row on exactly sized rows
        std::vector<float> row((size_t) V), out((size_t) V);
        std::mt19937 rng(9);
        for (int it = 0; it < 64; it++) {
            const int s = it % (S + 1), mode = it / (S + 1) % 5;
            for (int t = 0; t < V; t++) row[(size_t) t] = (float) ((int) (rng() % 17) - 8) * (mode == 1 ? 0.0f : 0.5f);      // coarse values: ties; mode 1: +0.0 / -0.0
            if (mode == 2) for (int t = 0; t < V; t += 3) row[(size_t) t] = NAN;
            if (mode == 3) for (int t = 0; t < V; t++) if (tab[(size_t) s * V + t] != LLAMAHIP_CONSTRAINT_BANNED) row[(size_t) t] = NAN;
            if (mode == 4) for (int t = 0; t < V; t++) row[(size_t) t] = tab[(size_t) s * V + t] != LLAMAHIP_CONSTRAINT_BANNED ? -INFINITY : INFINITY;
            int want = -1, lowest = -1;
            for (int t = 0; t < V; t++) {
                if (tab[(size_t) s * V + t] == LLAMAHIP_CONSTRAINT_BANNED) continue;
                if (lowest < 0) lowest = t;
                if (row[(size_t) t] == row[(size_t) t] && (want < 0 || row[(size_t) t] > row[(size_t) want])) want = t;
            }
            EXPECT(llamahip_constraint_pick(c, s, row.data()) == (want >= 0 ? want : lowest));
            EXPECT(llamahip_constraint_mask_row(c, s, row.data(), out.data()) == 0);
            for (int t = 0; t < V; t++) {
                const float w = tab[(size_t) s * V + t] == LLAMAHIP_CONSTRAINT_BANNED ? -INFINITY : row[(size_t) t];
                EXPECT(memcmp(&w, &out[(size_t) t], 4) == 0);
            }
            n_picks++;
        }
        EXPECT(llamahip_constraint_pick(c, S + 1, row.data()) == -1 && llamahip_constraint_pick(c, -1, row.data()) == -1 && llamahip_constraint_pick(c, 0, nullptr) == -1);
        EXPECT(llamahip_constraint_mask_row(c, S + 1, row.data(), out.data()) != 0 && llamahip_constraint_mask_row(c, 0, nullptr, out.data()) != 0);
        llamahip_constraint_free(c);
    }
    llamahip_constraint_free(nullptr);
    EXPECT(llamahip_constraint_n_states(nullptr) == 0 && llamahip_constraint_start(nullptr) == -1 && llamahip_constraint_done(nullptr) == -1 && llamahip_constraint_table(nullptr, nullptr, 0) == -1);
    // the refusals
    auto refused = [&](auto call, const char *fn) {
        for (size_t cap : { (size_t) 1, (size_t) 24, (size_t) 400 }) {
            std::vector<char> e(cap, 'x');
            llamahip_constraint *o = (llamahip_constraint *) 1;
            EXPECT(call(&o, e.data(), cap) == LLAMAHIP_ERR_PREDICT && o == nullptr);
            EXPECT(memchr(e.data(), 0, cap) != nullptr);
            if (cap == 400) EXPECT(strstr(e.data(), fn) == e.data());
            n_checks++;
        }
        llamahip_constraint *o = (llamahip_constraint *) 1;
        EXPECT(call(&o, nullptr, 0) == LLAMAHIP_ERR_PREDICT && o == nullptr);
    };
    const char *fn1 = "llamahip_constraint_new", *fn2 = "llamahip_constraint_new_choices";
    const int32_t *T = trans.data();
    const uint8_t *A = accept.data();
    refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(nullptr, S, T, A, 0, stop, o, e, cap); }, fn1);
    refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(m, S, nullptr, A, 0, stop, o, e, cap); }, fn1);
    refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(m, S, T, nullptr, 0, stop, o, e, cap); }, fn1);
    refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(m, 0, T, A, 0, stop, o, e, cap); }, fn1);
    refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(m, 4097, T, A, 0, stop, o, e, cap); }, fn1);
    refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(m, S, T, A, S, stop, o, e, cap); }, fn1);
    refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(m, S, T, A, -1, stop, o, e, cap); }, fn1);
    refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(m, S, T, A, 0, V, o, e, cap); }, fn1);
    refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(m, S, T, A, 0, -1, o, e, cap); }, fn1);
    refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(m, S, T, A, 3, stop, o, e, cap); }, fn1);      // the trap as the start: not live
    { const std::vector<uint8_t> none((size_t) S, 0);
      refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(m, S, T, none.data(), 0, stop, o, e, cap); }, fn1); }
    { std::vector<int32_t> bad = trans; bad.back() = S;
      refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(m, S, bad.data(), A, 0, stop, o, e, cap); }, fn1);
      bad.back() = -2;
      refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new(m, S, bad.data(), A, 0, stop, o, e, cap); }, fn1); }
    EXPECT(llamahip_constraint_new(m, S, T, A, 0, stop, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);
    // the choices builder: exactly sized strings; the table against the walk of the strings
    {
        const std::vector<std::vector<uint8_t>> strs = { { 'a', 'b' }, { 'a', 'b', 'c' }, { 'b' }, { 'a', 'b' }, { 't', 'o', 'k', '0', '0', '0', '4', '0' } };
        std::vector<const uint8_t *> ptr;
        std::vector<int32_t> len;
        for (const auto &s : strs) { ptr.push_back(s.data()); len.push_back((int32_t) s.size()); }
        llamahip_constraint *cc = nullptr;
        EXPECT(llamahip_constraint_new_choices(m, ptr.data(), len.data(), (int32_t) strs.size(), stop, &cc, err, sizeof(err)) == 0 && cc);
        if (cc) {
            EXPECT(llamahip_constraint_n_states(cc) == 1 + 2 + 1 + 1 + 8 + 1);      // root, a ab, abc, b, tok00040's eight, DONE
            const int done = llamahip_constraint_done(cc);
            // every token that is a prefix-walk of a choice advances; the stop token is allowed exactly at a string's end
            int q = 0;
            for (uint8_t b : strs[1]) { int t = -1; for (int v = 3; v < V && t < 0; v++) { uint32_t l = 0; const char *x = llamahip_token_text(m, v, &l); if (l == 1 && (uint8_t) x[0] == b) t = v; }
                                        EXPECT(llamahip_constraint_advance(cc, q, stop) == ((q == 0 || q == 1) ? -1 : done)); q = t < 0 ? -1 : llamahip_constraint_advance(cc, q, t); EXPECT(q > 0); if (q < 0) break; }
            if (q > 0) EXPECT(llamahip_constraint_advance(cc, q, stop) == done);
            EXPECT(llamahip_constraint_advance(cc, done, stop) == done);
            llamahip_constraint_free(cc);
        }
        refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new_choices(m, ptr.data(), len.data(), 0, stop, o, e, cap); }, fn2);
        refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new_choices(m, nullptr, len.data(), 2, stop, o, e, cap); }, fn2);
        refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new_choices(m, ptr.data(), nullptr, 2, stop, o, e, cap); }, fn2);
        refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new_choices(m, ptr.data(), len.data(), 2, V, o, e, cap); }, fn2);
        { std::vector<int32_t> l0 = len; l0[1] = 0;
          refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new_choices(m, ptr.data(), l0.data(), 3, stop, o, e, cap); }, fn2); }
        { std::vector<const uint8_t *> p0 = ptr; p0[2] = nullptr;
          refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new_choices(m, p0.data(), len.data(), 3, stop, o, e, cap); }, fn2); }
        { const std::vector<uint8_t> longs(5000, 'a'); const uint8_t *lp[1] = { longs.data() }; const int32_t ll[1] = { 5000 };
          refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new_choices(m, lp, ll, 1, stop, o, e, cap); }, fn2); }
        { const uint8_t hi[2] = { 0xff, 0xfe }; const uint8_t *lp[1] = { hi }; const int32_t ll[1] = { 2 };      // bytes no token supplies: the start is not live
          refused([&](llamahip_constraint **o, char *e, size_t cap) { return llamahip_constraint_new_choices(m, lp, ll, 1, stop, o, e, cap); }, fn2); }
    }
    printf("host_sanitize: constraints: %ld table entries against the lift restated, %ld picks and masked rows, %ld refusals at short and missing message buffers\n", n_entries, n_picks, n_checks);
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_sanitize <model file> [n_parts]\n"); return 2; }
    const std::string path = argv[1];
    const int parts = argc > 2 ? atoi(argv[2]) : 0;
    char err[512] = { 0 };
    llamahip_opts o; memset(&o, 0, sizeof(o)); o.struct_size = sizeof(o); o.device = -1; o.layer_end = -1; o.n_parts = parts;
    llamahip_model *m = nullptr;
    EXPECT(llamahip_model_load(path.c_str(), 64, &o, &m, err, sizeof(err)) == 0);
    if (!m) { fprintf(stderr, "%s\n", err); return 1; }
    // every tensor through the shard merge
    size_t total = 0;
    for (const auto &kv : m->file.tensors) {
        std::vector<uint8_t> buf((size_t) kv.second.nbytes());
        std::string e;
        EXPECT(m->file.read_tensor(kv.first, buf.data(), e));
        total += buf.size();
    }
    // tokenizer on vocabulary pieces, odd bytes and the empty string
    std::mt19937 rng(5);
    const int V = llamahip_n_vocab(m);
    for (int it = 0; it < 200; it++) {
        std::string text;
        const int n = (int) (rng() % 12);
        for (int i = 0; i < n; i++) {
            uint32_t len = 0;
            const char *t = llamahip_token_text(m, (int32_t) (rng() % V), &len);
            if (t && len && !memchr(t, 0, len)) text.append(t, len);
            if (rng() % 7 == 0) text.push_back((char) (rng() % 255 + 1));
        }
        std::vector<int32_t> out(text.size() + 2);
        const int32_t nt = llamahip_tokenize(m, text.c_str(), it & 1, out.data(), (int32_t) out.size());
        EXPECT(nt >= 0 && nt <= (int32_t) out.size());
        EXPECT(llamahip_tokenize(m, text.c_str(), 1, out.data(), 1) >= 0);          // cap smaller than the result
    }
    // sampler: both halves, tiny and oversized top_k, ties, a seen-everything window
    llamahip_sampler *s = llamahip_sampler_new(-1, 64);
    std::vector<float> lg(V);
    for (int it = 0; it < 300; it++) {
        for (int i = 0; i < V; i++) lg[i] = (float) ((int) (rng() % 41) - 20) * (it % 2 ? 0.25f : 0.37f);
        const int32_t id = llamahip_sample_top_p_top_k(m, s, lg.data(), 1.3, (int32_t) (it % 5 == 0 ? V + 7 : 1 + rng() % 40), it % 3 ? 0.95 : 1.0, 0.8);
        EXPECT(id >= 0 && id < V);
        llamahip_sampler_accept(s, id);
        double sc[4] = { 3.0, 2.0, 1.0, 0.5 }; int32_t ids[4] = { 1, 2, 3, 4 };
        EXPECT(llamahip_sample_from_candidates(s, sc, ids, 1 + it % 4, 0.95) >= 1);
    }
    int32_t win[64];
    EXPECT(llamahip_sampler_window(s, win, 64) == 64);
    EXPECT(llamahip_sampler_random_prompt(s) != nullptr);
    llamahip_sampler_free(s);
    constrain_host_half(m, V);      // (the lift reads the handle's vocabulary)
    llamahip_model_free(m);
    // corrupted copies of the file: every header field and a sweep of truncations must be load errors, never crashes
    std::vector<uint8_t> raw;
    { FILE *f = fopen(path.c_str(), "rb"); fseek(f, 0, SEEK_END); raw.resize((size_t) ftell(f)); fseek(f, 0, SEEK_SET); EXPECT(fread(raw.data(), 1, raw.size(), f) == raw.size()); fclose(f); }
    const std::string tmp = path + ".sanitize.tmp";
    auto try_load = [&](const std::vector<uint8_t> &bytes) {
        FILE *f = fopen(tmp.c_str(), "wb"); if (!bytes.empty()) fwrite(bytes.data(), 1, bytes.size(), f); fclose(f);
        llamahip_model *mm = nullptr;
        const int rc = llamahip_model_load(tmp.c_str(), 64, &o, &mm, err, sizeof(err));
        if (mm) llamahip_model_free(mm);
        return rc;
    };
    if (parts <= 1) {
        for (int field = 0; field < 8; field++)
            for (uint32_t v : { 0u, 0x7fffffffu, 0xffffffffu, 1u << 24 }) {
                std::vector<uint8_t> b = raw;
                memcpy(b.data() + 4 * field, &v, 4);
                (void) try_load(b);
            }
        for (size_t cut : { (size_t) 0, (size_t) 3, (size_t) 31, (size_t) 40, raw.size() / 3, raw.size() / 2, raw.size() - 1 }) {
            std::vector<uint8_t> b(raw.begin(), raw.begin() + (long) std::min(cut, raw.size()));
            EXPECT(try_load(b) != 0 || cut >= raw.size() - 1);
        }
    }
    remove(tmp.c_str());
    // the bridge without a GPU: load succeeds (stub), the first eval fails -> exactly one `failed` event, no leak
    struct Ev { int failed = 0, completed = 0; } ev;
    llama_runner_bridge *b = llama_runner_bridge_new(path.c_str());
    llama_runner_config c; llama_runner_config_default(&c); c.numberOfTokens = 4; c.n_ctx = 64;
    const int32_t rc = llama_runner_bridge_run(b, "", &c, [](void *u, llama_event_type t, const char *, uint32_t, int32_t) {
        Ev *e = (Ev *) u; if (t == LLAMA_EVENT_FAILED) e->failed++; if (t == LLAMA_EVENT_COMPLETED) e->completed++; }, &ev);
    EXPECT((rc == LLAMAHIP_ERR_PREDICT || rc == LLAMAHIP_ERR_LOAD) && ev.failed == 1 && ev.completed == 0);   // (a multi-part file of a non-LLaMA width fails in the loader: the bridge cannot force the part count)
    llama_runner_bridge_free(b);
    // the bridge's control flow with evals that succeed (made-up logits): prompts of 1 ... 40 tokens (one-part files: the bridge derives the
    // part count from n_embd, .mm:33-38, and cannot be told that a test file of another width has two)
    if (parts <= 1) {
        g_drive = true;
        llamahip_model *mv = nullptr;
        EXPECT(llamahip_model_load(path.c_str(), 64, &o, &mv, err, sizeof(err)) == 0);
        for (int want_tokens : { 1, 5, 9, 10, 18, 19, 27, 40 }) {
            if (!mv) break;
            // a prompt text made of vocabulary pieces; P = what the tokenizer (with BOS) makes of it
            std::string text;
            std::vector<int32_t> toks(512);
            int32_t P = 1;
            for (int tries = 0; tries < 400 && P < want_tokens; tries++) {
                uint32_t len = 0;
                const char *t = llamahip_token_text(mv, (int32_t) (3 + rng() % (uint32_t) (V - 3)), &len);
                if (!t || !len || memchr(t, 0, len)) continue;
                const std::string cand = text + std::string(t, len);
                const int32_t n = llamahip_tokenize(mv, cand.c_str(), 1, toks.data(), (int32_t) toks.size());
                if (n <= want_tokens) { text = cand; P = n; }
            }
            g_calls.clear();
            struct Ev2 { int tokens = 0, failed = 0, completed = 0; } e2;
            llama_runner_bridge *b2 = llama_runner_bridge_new(path.c_str());
            llama_runner_config c2; llama_runner_config_default(&c2); c2.numberOfTokens = 6; c2.n_ctx = 64;
            const int32_t rc2 = llama_runner_bridge_run(b2, text.c_str(), &c2, [](void *u, llama_event_type t, const char *, uint32_t, int32_t) {
                Ev2 *e = (Ev2 *) u; if (t == LLAMA_EVENT_OUTPUT_TOKEN) e->tokens++; if (t == LLAMA_EVENT_FAILED) e->failed++; if (t == LLAMA_EVENT_COMPLETED) e->completed++; }, &e2);
            llama_runner_bridge_free(b2);
            const int n_predict = std::min(6, 64 - P), chunk = 9;
            const int n_full = P > chunk ? ((P - 1) / chunk) * chunk : 0;
            EXPECT(rc2 == 0 && e2.failed == 0 && e2.completed == 1);
            EXPECT(e2.tokens == P + n_predict);                                        // the prompt echoed, then the generated tokens (.mm:892-895)
            size_t k = 0;
            EXPECT(g_calls.size() == (size_t) (1 + (n_full ? 1 : 0) + 1 + (n_predict - 1)));
            if (g_calls.size() == (size_t) (1 + (n_full ? 1 : 0) + 1 + (n_predict - 1))) {
                EXPECT(g_calls[k].kind == 0 && g_calls[k].n_past == 0 && g_calls[k].n == 4); k++;                      // warm-up (.mm:820-822)
                if (n_full) { EXPECT(g_calls[k].kind == 1 && g_calls[k].n_past == 0 && g_calls[k].n == n_full && g_calls[k].chunk == chunk); k++; }
                EXPECT(g_calls[k].kind == 2 && g_calls[k].n_past == n_full && g_calls[k].n == P - n_full); k++;          // the last chunk: its logits are sampled
                for (int g = 0; g + 1 < n_predict; g++, k++) EXPECT(g_calls[k].n_past == P + g && g_calls[k].n == 1);
            }
            printf("host_sanitize: driver with a %d-token prompt: %zu evals (%d tokens in one chunk-exact pass, %d in the last chunk), %d token events\n",
                   P, g_calls.size(), n_full, P - n_full, e2.tokens);
        }
        if (mv) llamahip_model_free(mv);
        g_drive = false;
    }
    // past the context window: the plan over a grid; the greedy loop in legs (exactly sized arrays, every n_keep that leaves
    // something to discard, a start at the wall) and its refusals; the driver with and without the overflow mode, with and without lookup steps
    for (int C = 1; C <= 12; C++)
        for (int np = -1; np <= C + 1; np++)
            for (int keep = -1; keep <= C + 1; keep++) {
                int32_t nd = -7;
                const int32_t got = llamahip_ctx_overflow_plan(C, np, keep, &nd);
                const bool bad = np < 0 || np > C || keep < 0 || keep > np || (np - keep) / 2 < 1;
                EXPECT(bad ? (got == -1 && nd == 0) : (nd == (np - keep) / 2 && got == np - nd));
                EXPECT(llamahip_ctx_overflow_plan(C, np, keep, nullptr) == got);
            }
    if (parts <= 1) {
        g_drive = true;
        llamahip_model *mw = nullptr;
        EXPECT(llamahip_model_load(path.c_str(), 16, &o, &mw, err, sizeof(err)) == 0);
        if (mw)
            for (int keep = 0; keep <= 14; keep++)
                for (int np0 : { 0, 5, 16 })
                    for (int chunk : { 0, 3 }) {
                        const int n_steps = 70;
                        std::vector<int32_t> ctx((size_t) np0), out((size_t) n_steps, -1);
                        for (int i = 0; i < np0; i++) ctx[i] = (int32_t) (rng() % (uint32_t) V);
                        int32_t np_out = -1;
                        g_calls.clear();
                        const int rcw = llamahip_decode_greedy_window(mw, 1, np0, 1, n_steps, ctx.data(), np0, keep, LLAMAHIP_CTX_REEVAL, chunk, out.data(), nullptr, &np_out, err, sizeof(err));
                        EXPECT(rcw == 0);
                        // replay: the calls against the plan, the steps they add up to, the final context
                        int pos = np0, steps = 0;
                        for (const EvalCall &c : g_calls) {
                            if (c.kind == 3) { EXPECT(c.n_past == pos && pos + c.n <= 16); pos += c.n; steps += c.n; continue; }
                            int32_t nd = 0;
                            const int32_t nn = llamahip_ctx_overflow_plan(16, pos, keep, &nd);
                            EXPECT(pos == 16 && nn > 0);
                            EXPECT(c.kind == (chunk ? 1 : 0) && c.chunk == chunk && c.n_past == keep && c.n == pos - keep - nd);
                            pos = nn;
                        }
                        EXPECT(steps == n_steps && np_out == pos);
                        for (int32_t t : out) EXPECT(t >= 0 && t < V);
                    }
        if (mw) {
            int32_t out1[4], one = 1, npo = 0;
            EXPECT(llamahip_decode_greedy_window(mw, 1, 1, 1, 4, &one, 1, 0, 0, 0, out1, nullptr, &npo, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);      // mode
            EXPECT(llamahip_decode_greedy_window(mw, 1, 1, 1, 4, &one, 1, 15, 1, 0, out1, nullptr, &npo, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);     // n_keep
            EXPECT(llamahip_decode_greedy_window(mw, 1, 1, 1, 4, &one, 1, -1, 1, 0, out1, nullptr, &npo, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);
            EXPECT(llamahip_decode_greedy_window(mw, 1, 1, 1, 4, &one, 0, 0, 1, 0, out1, nullptr, &npo, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);      // n_context
            EXPECT(llamahip_decode_greedy_window(mw, 1, 17, 1, 4, &one, 17, 0, 1, 0, out1, nullptr, &npo, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);    // n_past
            EXPECT(llamahip_decode_greedy_window(mw, 1, 1, 1, 0, &one, 1, 0, 1, 0, out1, nullptr, &npo, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);      // n_steps
            EXPECT(llamahip_decode_greedy_window(mw, 1, 1, 1, 4, &one, 1, 0, 1, -1, out1, nullptr, &npo, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);     // chunk_tokens
            EXPECT(llamahip_decode_greedy_window(mw, 1, 1, V, 4, &one, 1, 0, 1, 0, out1, nullptr, &npo, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);      // token id
            EXPECT(llamahip_decode_greedy_window(nullptr, 1, 1, 1, 4, &one, 1, 0, 1, 0, out1, nullptr, &npo, nullptr, 0) == LLAMAHIP_ERR_PREDICT);
            llamahip_model_free(mw);
        }
        // the driver: 60 tokens at n_ctx 24, without and with the overflow mode, greedy and sampled (made-up logits: eval_topk reports inexact, the host sampler draws)
        for (int mode = 0; mode <= 1; mode++)
            for (int greedy = 0; greedy <= 2; greedy++)          // (2: sampled with lookup steps of up to 4 draft tokens)
                for (int keep : { -1, 0, 3, 100 }) {
                    struct Ev3 { int tokens = 0, failed = 0, completed = 0; } e3;
                    g_calls.clear();
                    llama_runner_bridge *b3 = llama_runner_bridge_new(path.c_str());
                    llama_runner_bridge_set_overflow(b3, mode, keep);
                    if (greedy == 2) llama_runner_bridge_set_lookup(b3, 4);
                    llama_runner_config c3; llama_runner_config_default(&c3); c3.numberOfTokens = 60; c3.n_ctx = 24; c3.greedy = greedy == 1; c3.seed = 7;
                    const int32_t rc3 = llama_runner_bridge_run(b3, "", &c3, [](void *u, llama_event_type t, const char *, uint32_t, int32_t) {
                        Ev3 *e = (Ev3 *) u; if (t == LLAMA_EVENT_OUTPUT_TOKEN) e->tokens++; if (t == LLAMA_EVENT_FAILED) e->failed++; if (t == LLAMA_EVENT_COMPLETED) e->completed++; }, &e3);
                    llama_runner_bridge_free(b3);
                    EXPECT(rc3 == 0 && e3.failed == 0 && e3.completed == 1);
                    int reevals = 0, over = 0, verifies = 0;
                    for (size_t k = 1; k < g_calls.size(); k++) {          // (k = 0: the warm-up)
                        const EvalCall &c = g_calls[k];
                        if (c.kind == 4) verifies++;
                        else if (k > 1 && c.n > 1) reevals++;
                        if (c.n_past + c.n > 24) over++;
                    }
                    EXPECT(over == 0);
                    EXPECT(greedy == 2 ? verifies > 0 : verifies == 0);          // (a verify step whose rows pass the cache fails the run: counted in `failed`)
                    if (mode == 0) EXPECT(reevals == 0 && e3.tokens <= 24);
                    if (mode == 1) EXPECT(reevals >= 2 && e3.tokens > 60);
                }
        g_drive = false;
    }
    // the same in shift mode (LLAMAHIP_CTX_SHIFT): the greedy loop in legs on exactly sized arrays, every wall crossed by ONE shift of the plan's
    // rows and no eval; the driver in mode 4, greedy, sampled and with lookup steps -- the stub's call sequence replayed against the plan
    if (parts <= 1) {
        g_drive = true;
        llamahip_model *ms = nullptr;
        EXPECT(llamahip_model_load(path.c_str(), 16, &o, &ms, err, sizeof(err)) == 0);
        int shifts_window = 0, shifts_driver = 0;
        if (ms)
            for (int keep = 0; keep <= 14; keep++)
                for (int np0 : { 0, 5, 16 })
                    for (int chunk : { 0, 3 }) {          // (ignored by the mode)
                        const int n_steps = 70;
                        std::vector<int32_t> ctx((size_t) np0), out((size_t) n_steps, -1);
                        for (int i = 0; i < np0; i++) ctx[i] = (int32_t) (rng() % (uint32_t) V);
                        int32_t np_out = -1;
                        g_calls.clear();
                        EXPECT(llamahip_decode_greedy_window(ms, 1, np0, 1, n_steps, ctx.data(), np0, keep, LLAMAHIP_CTX_SHIFT, chunk, out.data(), nullptr, &np_out, err, sizeof(err)) == 0);
                        int pos = np0, steps = 0;
                        for (const EvalCall &c : g_calls) {
                            if (c.kind == 3) { EXPECT(c.n_past == pos && pos + c.n <= 16); pos += c.n; steps += c.n; continue; }
                            int32_t nd = 0;
                            const int32_t nn = llamahip_ctx_overflow_plan(16, pos, keep, &nd);
                            EXPECT(pos == 16 && nn > 0);
                            EXPECT(c.kind == 5 && c.n_past == keep + nd && c.n == pos - keep - nd && c.chunk == nd);
                            pos = nn;
                            shifts_window++;
                        }
                        EXPECT(steps == n_steps && np_out == pos);
                        for (int32_t t : out) EXPECT(t >= 0 && t < V);
                    }
        if (ms) {
            int32_t out1[4], one = 1, npo = 0;
            EXPECT(llamahip_decode_greedy_window(ms, 1, 1, 1, 4, &one, 1, 15, LLAMAHIP_CTX_SHIFT, 0, out1, nullptr, &npo, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);      // n_keep
            EXPECT(llamahip_decode_greedy_window(ms, 1, 1, 1, 4, &one, 1, 0, LLAMAHIP_CTX_SHIFT, -1, out1, nullptr, &npo, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);      // chunk_tokens
            EXPECT(llamahip_decode_greedy_window(ms, 1, 1, 1, 4, &one, 1, 0, 5, 0, out1, nullptr, &npo, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);                        // mode
            llamahip_model_free(ms);
        }
        for (int greedy = 0; greedy <= 2; greedy++)          // (2: sampled with lookup steps of up to 4 draft tokens)
            for (int keep : { -1, 0, 3, 100 }) {
                struct Ev4 { int tokens = 0, failed = 0, completed = 0; } e4;
                g_calls.clear();
                llama_runner_bridge *b4 = llama_runner_bridge_new(path.c_str());
                llama_runner_bridge_set_overflow(b4, LLAMAHIP_CTX_SHIFT, keep);
                if (greedy == 2) llama_runner_bridge_set_lookup(b4, 4);
                llama_runner_config c4; llama_runner_config_default(&c4); c4.numberOfTokens = 60; c4.n_ctx = 24; c4.greedy = greedy == 1; c4.seed = 7;
                const int32_t rc4 = llama_runner_bridge_run(b4, "", &c4, [](void *u, llama_event_type t, const char *, uint32_t, int32_t) {
                    Ev4 *e = (Ev4 *) u; if (t == LLAMA_EVENT_OUTPUT_TOKEN) e->tokens++; if (t == LLAMA_EVENT_FAILED) e->failed++; if (t == LLAMA_EVENT_COMPLETED) e->completed++; }, &e4);
                llama_runner_bridge_free(b4);
                EXPECT(rc4 == 0 && e4.failed == 0 && e4.completed == 1 && e4.tokens > 60);
                // replay: the evaluated rows add up to the position; a shift comes at the wall only and is the plan's; no eval of the tail follows it
                int pos = 0, shifts = 0, verifies = 0, n_keep = -1;
                for (size_t k = 1; k < g_calls.size(); k++) {          // (k = 0: the warm-up)
                    const EvalCall &c = g_calls[k];
                    if (c.kind == 5) {
                        // (n_keep as the driver clamps it: c.n_past - c.chunk; the same at every crossing of a run)
                        const int kp = c.n_past - c.chunk;
                        int32_t nd = 0;
                        const int32_t nn = llamahip_ctx_overflow_plan(24, pos, kp, &nd);
                        EXPECT(pos == 24 && nn > 0 && c.chunk == nd && c.n == pos - kp - nd && kp >= 0 && kp <= 12 && (n_keep < 0 || n_keep == kp));
                        if (keep >= 0) EXPECT(kp == std::min(keep, 12));
                        n_keep = kp;
                        pos = nn;
                        shifts++;
                        continue;
                    }
                    EXPECT(c.n_past == pos && pos + c.n <= 24);
                    if (c.kind == 4) { verifies++; pos = k + 1 < g_calls.size() && g_calls[k + 1].kind != 5 ? g_calls[k + 1].n_past : pos + c.n; continue; }      // (a verify step keeps n_accept + 1 of its rows)
                    EXPECT(shifts == 0 || c.n == 1);          // after the first crossing nothing but single steps
                    pos += c.n;
                }
                EXPECT(shifts >= 2);
                EXPECT(greedy == 2 ? verifies > 0 : verifies == 0);
                shifts_driver += shifts;
            }
        g_drive = false;
        printf("host_sanitize: shift mode: %d shifts in the greedy loop's legs and %d in the driver's runs, each the plan's, no tail evaluated again\n", shifts_window, shifts_driver);
    }
    // the dealing of a multi-sequence verify step's rows: exactly sized arrays, every n_seqs and budget, and the refusals
    for (int n = 1; n <= 16; n++)
        for (int budget = n; budget <= 16; budget++)
            for (int it = 0; it < 8; it++) {
                std::vector<int32_t> want((size_t) n), give((size_t) n, -7);
                int sum_want = 0;
                for (int i = 0; i < n; i++) { want[i] = (int32_t) (rng() % (it % 2 ? 16 : 3)); sum_want += want[i]; }
                const int32_t dealt = llamahip_lookup_deal_rows(want.data(), n, budget, give.data());
                int sum = 0;
                for (int i = 0; i < n; i++) { EXPECT(give[i] >= 0 && give[i] <= want[i]); sum += give[i]; }
                EXPECT(dealt == sum && sum == std::min(budget - n, sum_want));
            }
    {
        int32_t w[2] = { 1, 16 }, g[2] = { 0, 0 };
        EXPECT(llamahip_lookup_deal_rows(w, 2, 16, g) == -1 && llamahip_lookup_deal_rows(w, 1, 0, g) == -1 && llamahip_lookup_deal_rows(w, 17, 16, g) == -1);
        EXPECT(llamahip_lookup_deal_rows(nullptr, 1, 16, g) == -1 && llamahip_lookup_deal_rows(w, 1, 16, nullptr) == -1 && llamahip_lookup_deal_rows(w, 1, 17, g) == -1);
    }
    // the row table of llamahip_eval_multi: exactly sized arrays over a grid of segment shapes, each entry against the rule restated; the
    // argument checks and the op's table check on exactly sized arrays, accepted and refused
    for (int C : { 64, 128 })
        for (int n = 1; n <= 5; n++)
            for (int chunk : { 0, 1, 9 })
                for (int it = 0; it < 6; it++) {
                    static const int lens[6] = { 1, 2, 9, 10, 18, 61 }, pasts[3] = { 0, 3, 37 };
                    std::vector<int32_t> np((size_t) n), nt((size_t) n), slots((size_t) n);
                    int R = 0;
                    bool fits = true;
                    for (int i = 0; i < n; i++) { np[i] = pasts[(it + i) % 3]; nt[i] = lens[(it * 5 + i) % 6]; slots[i] = n - 1 - i; R += nt[i]; fits = fits && np[i] + nt[i] <= C; }
                    std::vector<int32_t> seg((size_t) R), pos((size_t) R), keys((size_t) R), toks((size_t) R, 1);
                    const int32_t got = llamahip_eval_multi_rows(C, n, np.data(), nt.data(), chunk, seg.data(), pos.data(), keys.data());
                    EXPECT(got == (fits ? R : -1));
                    EXPECT(llamahip_eval_multi_rows(C, n, np.data(), nt.data(), chunk, nullptr, nullptr, nullptr) == got);
                    EXPECT((lh::eval_multi_check(C, V, n, n, slots.data(), np.data(), toks.data(), nt.data(), chunk, err, sizeof(err)) == 0) == fits);
                    if (!fits) continue;
                    int r = 0;
                    for (int i = 0; i < n; i++)
                        for (int j = 0; j < nt[i]; j++, r++) {
                            const int want = chunk > 0 ? np[i] + std::min(nt[i], (j / chunk + 1) * chunk) : np[i] + nt[i];
                            EXPECT(seg[r] == i && pos[r] == np[i] + j && keys[r] == want);
                        }
                    std::vector<int32_t> rslot((size_t) R);
                    for (int q = 0; q < R; q++) rslot[q] = slots[seg[q]];
                    EXPECT(lh::rows_table_check(R, C, n, rslot.data(), pos.data(), keys.data(), err, sizeof(err)) == 0);
                    EXPECT(lh::rows_table_check(R, C, n, rslot.data(), pos.data(), keys.data(), nullptr, 0) == 0);
                    keys[R - 1] += 1;                                                                                    // past the end of the slot's rows
                    EXPECT(lh::rows_table_check(R, C, n, rslot.data(), pos.data(), keys.data(), err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);
                    keys[R - 1] = pos[R - 1];                                                                            // no key of its own
                    EXPECT(lh::rows_table_check(R, C, n, rslot.data(), pos.data(), keys.data(), err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);
                    keys[R - 1] = pos[R - 1] + 1;
                    rslot[R - 1] = n;                                                                                    // slot out of range
                    EXPECT(lh::rows_table_check(R, C, n, rslot.data(), pos.data(), keys.data(), err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);
                    rslot[R - 1] = slots[seg[R - 1]];
                    if (n > 1) { slots[n - 1] = slots[0]; EXPECT(lh::eval_multi_check(C, V, n, n, slots.data(), np.data(), toks.data(), nt.data(), chunk, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT); slots[n - 1] = 0; }
                    toks[R - 1] = V;
                    EXPECT(lh::eval_multi_check(C, V, n, n, slots.data(), np.data(), toks.data(), nt.data(), chunk, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);
                    toks[R - 1] = 1;
                    EXPECT(lh::eval_multi_check(C, V, n, n, slots.data(), np.data(), toks.data(), nt.data(), -1, nullptr, 0) == LLAMAHIP_ERR_PREDICT);
                    EXPECT(lh::eval_multi_check(C, V, n - 1, n, slots.data(), np.data(), toks.data(), nt.data(), chunk, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);
                }
    {
        const int32_t np1[1] = { 0 }, big[1] = { LLAMAHIP_EVAL_MULTI_MAX_ROWS + 1 }, zero[1] = { 0 }, neg[1] = { -1 };
        EXPECT(llamahip_eval_multi_rows(4096, 1, np1, big, 0, nullptr, nullptr, nullptr) == -1 && llamahip_eval_multi_rows(64, 1, np1, zero, 0, nullptr, nullptr, nullptr) == -1);
        EXPECT(llamahip_eval_multi_rows(64, 1, neg, np1, 0, nullptr, nullptr, nullptr) == -1 && llamahip_eval_multi_rows(64, 0, np1, np1, 0, nullptr, nullptr, nullptr) == -1);
        EXPECT(llamahip_eval_multi_rows(64, 1, nullptr, big, 0, nullptr, nullptr, nullptr) == -1 && llamahip_eval_multi_rows(64, 1, np1, big, -1, nullptr, nullptr, nullptr) == -1);
    }
    scoring_host_half(V);
    beam_host_half(V);
    embedding_host_half(V);
    // the request scheduler's host half against the stubbed device half: the step rule over a grid on exactly sized arrays against its
    // restatement; then whole runs -- every step's segments replayed against the rule and the requests' own state (positions, offsets, tokens,
    // emit flags), the events against the made-up tokens; the refusals of new / submit / step; cancelling queued and active requests
    auto plan_ref = [](const std::vector<int32_t> &left, int c, int budget, std::vector<int32_t> &rows) {
        long rest = budget, total = 0;
        for (int32_t l : left) if (l == 0) rest--;
        bool given = false, stop = false;
        rows.assign(left.size(), 0);
        for (size_t i = 0; i < left.size(); i++) {
            long r = 0;
            if (left[i] == 0) r = 1;
            else if (!stop) {
                const long room = rest > 0 ? rest : 0;
                r = c > 0 ? std::min<long>(left[i], room / c * c) : (left[i] <= rest ? left[i] : 0);
                if (r < 1 && !given) r = c > 0 ? std::min<long>(left[i], c) : left[i];
                else if (r < 1) stop = true;
                if (r > 0) { given = true; rest -= r; }
            }
            rows[i] = (int32_t) r; total += r;
        }
        return (int32_t) total;
    };
    for (int c : { 0, 1, 4, 9 })
        for (int budget : { 1, 8, 16, 17, 64 })
            for (int n = 0; n <= 16; n++)
                for (int it = 0; it < 6; it++) {
                    static const int lens[8] = { 0, 1, 3, 9, 10, 27, 61, 100 };
                    std::vector<int32_t> left((size_t) n), rows((size_t) n, -7), want;
                    for (int i = 0; i < n; i++) left[(size_t) i] = lens[rng() % 8];
                    const int32_t total = llamahip_sched_plan(n, n ? left.data() : nullptr, c, budget, n ? rows.data() : nullptr);
                    EXPECT(total == plan_ref(left, c, budget, want) && rows == want);
                }
    {
        int32_t l1[1] = { 3 }, r1[1] = { 0 }, neg[1] = { -1 };
        EXPECT(llamahip_sched_plan(1, l1, 0, 0, r1) == -1 && llamahip_sched_plan(1, l1, -1, 8, r1) == -1 && llamahip_sched_plan(17, l1, 0, 8, r1) == -1);
        EXPECT(llamahip_sched_plan(1, nullptr, 0, 8, r1) == -1 && llamahip_sched_plan(1, l1, 0, 8, nullptr) == -1 && llamahip_sched_plan(1, neg, 0, 8, r1) == -1);
        EXPECT(llamahip_sched_plan(-1, l1, 0, 8, r1) == -1 && llamahip_sched_plan(0, nullptr, 0, 8, nullptr) == 0);
    }
    if (parts <= 1) {
        llamahip_model *ms = nullptr;
        EXPECT(llamahip_model_load(path.c_str(), 48, &o, &ms, err, sizeof(err)) == 0);
        for (int c : { 0, 1, 4, 9 })
            for (int budget : { 1, 8, 17 })
                for (int max_active : { 1, 3, 4 }) {
                    if (!ms) break;
                    llamahip_sched_opts so; memset(&so, 0, sizeof(so));
                    so.struct_size = sizeof(so); so.n_threads = 2; so.max_active = max_active; so.chunk_tokens = c; so.row_budget = budget;
                    llamahip_sched *sc = nullptr;
                    EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == 0 && sc);
                    if (!sc) continue;
                    struct Want { std::vector<int32_t> prompt; int n_predict, stop; llamahip_sampler *smp; std::vector<int32_t> got; int done = 0, reason = 0, slot = -1, off = 0; };
                    std::vector<Want> reqs;
                    static const int plens[7] = { 1, 3, 9, 10, 20, 31, 40 }, npred[7] = { 1, 2, 5, 8, 3, 1, 4 };
                    for (int i = 0; i < 7; i++) {
                        Want w;
                        w.prompt.resize((size_t) plens[i]);          // exactly sized: submit copies n_prompt ids and no more
                        for (int32_t &t : w.prompt) t = (int32_t) (rng() % (uint32_t) V);
                        w.n_predict = npred[i]; w.stop = -1; w.smp = i % 3 == 1 ? llamahip_sampler_new(i, 8) : nullptr;
                        reqs.push_back(w);
                    }
                    std::vector<int64_t> ids(reqs.size());
                    for (size_t i = 0; i < reqs.size(); i++) {
                        llamahip_request rq; memset(&rq, 0, sizeof(rq));
                        rq.struct_size = sizeof(rq); rq.prompt = reqs[i].prompt.data(); rq.n_prompt = (int32_t) reqs[i].prompt.size();
                        rq.n_predict = reqs[i].n_predict; rq.stop_token = reqs[i].stop; rq.sampler = reqs[i].smp;
                        EXPECT(llamahip_sched_submit(sc, &rq, &ids[i], err, sizeof(err)) == 0 && ids[i] == (int64_t) i + 1);
                        if (reqs[i].smp) EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);      // the sampler is held
                    }
                    EXPECT(llamahip_sched_cancel(sc, ids[6]) == 0 && llamahip_sched_cancel(sc, ids[6]) == -1 && llamahip_sched_cancel(sc, 99) == -1);      // a queued request
                    // refusals of submit (exactly sized prompts) and of step: nothing is consumed
                    {
                        std::vector<int32_t> p1(1, V), p2(2, 1);
                        llamahip_request rq; memset(&rq, 0, sizeof(rq));
                        rq.struct_size = sizeof(rq); rq.prompt = p1.data(); rq.n_prompt = 1; rq.n_predict = 1; rq.stop_token = -1;
                        EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);          // token id
                        rq.prompt = p2.data(); rq.n_prompt = 2; rq.n_predict = 48;
                        EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);          // n_prompt + n_predict - 1 > n_ctx
                        rq.n_predict = 0;
                        EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);
                        rq.n_predict = 1; rq.n_prompt = 0;
                        EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);
                        rq.n_prompt = 2; rq.stop_token = V;
                        EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);
                        rq.stop_token = -1; rq.struct_size = 4;
                        EXPECT(llamahip_sched_submit(sc, &rq, nullptr, nullptr, 0) == LLAMAHIP_ERR_PREDICT);
                        std::vector<llamahip_sched_event> small((size_t) 2 * max_active);
                        int32_t ne = -1;
                        const int32_t before = llamahip_sched_pending(sc);
                        EXPECT(llamahip_sched_step(sc, small.data(), (int32_t) small.size(), &ne, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && ne == 0);
                        EXPECT(llamahip_sched_pending(sc) == before && before == 7);
                    }
                    g_sched_calls.clear();
                    std::vector<llamahip_sched_event> evs((size_t) 2 * max_active + 1);          // exactly the smallest cap
                    std::vector<int> slot_req((size_t) max_active, -1), admit;          // admit: the active requests in admission order
                    size_t next_q = 0, call = 0;
                    int steps = 0, cancelled_seen = 0;
                    bool cancel_active_done = false;
                    while (llamahip_sched_pending(sc) > 0 && steps < 400) {
                        int32_t ne = 0;
                        EXPECT(llamahip_sched_step(sc, evs.data(), (int32_t) evs.size(), &ne, err, sizeof(err)) == 0);
                        steps++;
                        // the model of the step: cancelled actives leave, admissions (lowest slot, submission order; request 6 was cancelled while queued), the rule
                        for (size_t k = 0; k < admit.size();) { if (reqs[(size_t) admit[k]].reason == -3) { slot_req[(size_t) reqs[(size_t) admit[k]].slot] = -1; admit.erase(admit.begin() + (long) k); } else k++; }
                        for (int sl = 0; sl < max_active && next_q < 6; sl++)
                            if (slot_req[(size_t) sl] < 0) { slot_req[(size_t) sl] = (int) next_q; reqs[next_q].slot = sl; admit.push_back((int) next_q); next_q++; }
                        std::vector<int32_t> left, rows;
                        for (int r : admit) left.push_back((int32_t) reqs[(size_t) r].prompt.size() - reqs[(size_t) r].off);
                        plan_ref(left, c, budget, rows);
                        if (!admit.empty()) {
                            EXPECT(call < g_sched_calls.size());
                            if (call >= g_sched_calls.size()) break;
                            const SchedCall &sc_call = g_sched_calls[call++];
                            size_t j = 0;
                            bool any_prompt = false;
                            for (size_t k = 0; k < admit.size(); k++) {
                                if (rows[k] < 1) continue;
                                Want &w = reqs[(size_t) admit[k]];
                                EXPECT(j < sc_call.segs.size());
                                if (j >= sc_call.segs.size()) break;
                                const lh::SchedSeg &g = sc_call.segs[j];
                                EXPECT(g.slot == w.slot && g.n_rows == rows[k] && g.sampler == w.smp && g.n_out == (int32_t) w.got.size());
                                if (left[k] > 0) {
                                    any_prompt = true;
                                    EXPECT(g.pos == w.off && g.emit == (rows[k] == left[k]) && (c == 0 || w.off % c == 0));
                                    EXPECT(std::equal(sc_call.toks[j].begin(), sc_call.toks[j].end(), w.prompt.begin() + w.off));
                                    w.off += rows[k];
                                } else {
                                    EXPECT(g.emit == 1 && g.pos == (int32_t) (w.prompt.size() + w.got.size()) - 1 && sc_call.toks[j][0] == w.got.back());
                                }
                                if (g.emit) w.got.push_back(g.token);
                                j++;
                            }
                            EXPECT(j == sc_call.segs.size() && sc_call.mixed == any_prompt);
                        }
                        // the events: a TOKEN per emitted token, DONE behind a request's last one; the model frees those slots
                        for (int32_t e = 0; e < ne; e++) {
                            const llamahip_sched_event &x = evs[(size_t) e];
                            EXPECT(x.id >= 1 && x.id <= 7);
                            Want &w = reqs[(size_t) (x.id - 1)];
                            if (x.kind == LLAMAHIP_EV_TOKEN) { EXPECT(!w.got.empty() && x.token == w.got.back() && x.slot == w.slot && x.position == (int32_t) (w.prompt.size() + w.got.size()) - 1); }
                            else {
                                EXPECT(x.kind == LLAMAHIP_EV_DONE && !w.done);
                                w.done = 1;
                                if (x.reason == LLAMAHIP_DONE_CANCELLED) { cancelled_seen++; continue; }
                                EXPECT(x.reason == LLAMAHIP_DONE_LENGTH && (int) w.got.size() == w.n_predict);
                                w.reason = x.reason;
                                slot_req[(size_t) w.slot] = -1;
                                admit.erase(std::find(admit.begin(), admit.end(), (int) (x.id - 1)));
                            }
                        }
                        // cancel an active request once it has produced a token (request 3: 10 prompt tokens, 8 to produce)
                        if (!cancel_active_done && reqs[3].got.size() >= 1 && !reqs[3].done) {
                            EXPECT(llamahip_sched_cancel(sc, ids[3]) == 0);
                            reqs[3].reason = -3;
                            cancel_active_done = true;
                        }
                    }
                    EXPECT(llamahip_sched_pending(sc) == 0 && cancelled_seen == 2 && cancel_active_done);
                    for (size_t i = 0; i < reqs.size(); i++) EXPECT(reqs[i].done == 1);
                    llamahip_sched_stats ss; memset(&ss, 0, sizeof(ss)); ss.struct_size = sizeof(ss);
                    EXPECT(llamahip_sched_get_stats(sc, &ss) == 0 && ss.n_submitted == 7 && ss.n_done == 7 && ss.n_steps == (int64_t) g_sched_calls.size());
                    EXPECT(ss.n_mixed_steps + ss.n_set_steps + ss.n_single_steps == ss.n_steps && ss.n_fallback_steps == 0);
                    llamahip_sched_free(sc);
                    for (Want &w : reqs) if (w.smp) llamahip_sampler_free(w.smp);
                }
        // drafted tokens (draft_len > 0) against the stub's scripted accepts: every step's segments against the policy (llamahip_sched_plan_drafts
        // on the requests' own state), the drafts against llamahip_lookup_draft on the model's history, the events against what the stub
        // reported -- in order, at consecutive positions, cut at the stop token and at n_predict -- on an event array of exactly the smallest cap
        int64_t dropped_in_all = 0;
        for (int script : { -1, 0, 15 })
            for (int draft_len : { 1, 4, 15 })
                for (int max_active : { 1, 3, 4 }) {
                    if (!ms) break;
                    g_sched_accept = script;
                    std::vector<int32_t> corpus(40);          // exactly sized: copied at llamahip_sched_new
                    for (size_t i = 0; i < corpus.size(); i++) corpus[i] = (int32_t) ((i * 5 + 1) % (size_t) V);
                    llamahip_sched_opts so; memset(&so, 0, sizeof(so));
                    so.struct_size = sizeof(so); so.n_threads = 2; so.max_active = max_active; so.chunk_tokens = 4; so.row_budget = 8;
                    so.draft_len = draft_len; so.corpus = corpus.data(); so.n_corpus = (int32_t) corpus.size();
                    llamahip_sched *sc = nullptr;
                    EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == 0 && sc);
                    if (!sc) continue;
                    std::fill(corpus.begin(), corpus.end(), -5);          // (the scheduler has its own copy)
                    struct DReq { std::vector<int32_t> hist; size_t n_prompt; int n_predict, stop; llamahip_sampler *smp; int n_out = 0, done = 0; };
                    std::vector<DReq> reqs;
                    static const int plens[6] = { 2, 5, 9, 12, 3, 7 }, npred[6] = { 30, 12, 1, 20, 36, 2 };
                    for (int i = 0; i < 6; i++) {
                        DReq w;
                        w.hist.resize((size_t) plens[i]);
                        for (size_t k = 0; k < w.hist.size(); k++) w.hist[k] = (int32_t) ((k % 3 * 5 + 1 + (size_t) i) % (size_t) V);      // a repeated 3-gram: the history drafter fires
                        w.n_prompt = w.hist.size(); w.n_predict = npred[i]; w.stop = i == 4 ? 6 : i == 0 ? 7 : i == 3 ? 11 : -1; w.smp = i % 3 == 1 ? llamahip_sampler_new(i, 8) : nullptr;
                        reqs.push_back(w);
                        llamahip_request rq; memset(&rq, 0, sizeof(rq));
                        rq.struct_size = sizeof(rq); rq.prompt = reqs.back().hist.data(); rq.n_prompt = plens[i]; rq.n_predict = npred[i]; rq.stop_token = w.stop; rq.sampler = w.smp;
                        int64_t id = 0;
                        EXPECT(llamahip_sched_submit(sc, &rq, &id, err, sizeof(err)) == 0 && id == (int64_t) i + 1);
                    }
                    {
                        std::vector<llamahip_sched_event> small((size_t) max_active + 16);
                        int32_t ne = -1;
                        EXPECT(llamahip_sched_step(sc, small.data(), (int32_t) small.size(), &ne, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && ne == 0 && strstr(err, "max_active + 17"));
                        EXPECT(llamahip_sched_pending(sc) == 6);
                    }
                    std::vector<llamahip_sched_event> evs((size_t) LLAMAHIP_SCHED_EVENT_CAP(max_active, draft_len));          // exactly the smallest cap
                    EXPECT(evs.size() == (size_t) max_active + 17);
                    g_sched_calls.clear();
                    int steps = 0;
                    int64_t emit_segs = 0, accepted = 0, drafted = 0, dropped = 0, tokens = 0, draft_steps = 0;
                    while (llamahip_sched_pending(sc) > 0 && steps < 600) {
                        int32_t ne = 0;
                        const size_t call0 = g_sched_calls.size();
                        EXPECT(llamahip_sched_step(sc, evs.data(), (int32_t) evs.size(), &ne, err, sizeof(err)) == 0 && ne <= (int32_t) evs.size());
                        steps++;
                        EXPECT(g_sched_calls.size() == call0 + 1);
                        if (g_sched_calls.size() != call0 + 1) break;
                        const SchedCall &cl = g_sched_calls.back();
                        int logit_rows = 0, step_drafted = 0;
                        int32_t e = 0;
                        for (size_t j = 0; j < cl.segs.size(); j++) {
                            const lh::SchedSeg &g = cl.segs[j];
                            EXPECT(g.n_draft >= 0 && g.n_draft <= draft_len && (g.n_draft == 0 || (g.emit && g.n_rows == 1)));
                            logit_rows += g.emit ? 1 + g.n_draft : 0;
                            step_drafted += g.n_draft;
                            if (!g.emit) continue;
                            // whose segment: the request in that slot is the one the segment's events name
                            EXPECT(e < ne && evs[(size_t) e].kind == LLAMAHIP_EV_TOKEN && evs[(size_t) e].slot == g.slot);
                            if (e >= ne) break;
                            DReq &w = reqs[(size_t) (evs[(size_t) e].id - 1)];
                            if (g.n_draft > 0) {
                                // the draft is the drafter's hit on the request's own history (then the corpus), cut to what is left to predict
                                int32_t want[15];
                                const int32_t room = std::min(draft_len, w.n_predict - w.n_out - 1);
                                EXPECT(room >= g.n_draft);
                                std::vector<int32_t> cp(40);
                                for (size_t i = 0; i < cp.size(); i++) cp[i] = (int32_t) ((i * 5 + 1) % (size_t) V);
                                const int32_t nw = llamahip_lookup_draft(w.hist.data(), (int32_t) w.hist.size(), cp.data(), 40, std::max(room, 1), 0, 0, want);
                                EXPECT(nw >= g.n_draft && std::equal(cl.drafts[j].begin(), cl.drafts[j].end(), want));
                                EXPECT(g.pos == (int32_t) w.hist.size() - 1 && cl.toks[j][0] == w.hist.back());
                                if (w.smp && w.stop >= 0) EXPECT(std::find(cl.drafts[j].begin(), cl.drafts[j].end(), w.stop) == cl.drafts[j].end());
                            }
                            emit_segs++; accepted += g.n_accept;
                            const int n_tok = g.n_draft > 0 ? g.n_accept + 1 : 1;
                            bool ended = false;
                            for (int a = 0; a < n_tok && !ended; a++) {
                                const int32_t tok = g.n_draft > 0 ? g.toks[a] : g.token;
                                EXPECT(e < ne);
                                if (e >= ne) break;
                                const llamahip_sched_event &x = evs[(size_t) e++];
                                w.hist.push_back(tok); w.n_out++; tokens++;
                                EXPECT(x.kind == LLAMAHIP_EV_TOKEN && x.token == tok && x.slot == g.slot && x.position == (int32_t) w.hist.size() - 1);
                                if (tok == w.stop || w.n_out == w.n_predict) {
                                    EXPECT(e < ne && evs[(size_t) e].kind == LLAMAHIP_EV_DONE && evs[(size_t) e].id == x.id && evs[(size_t) e].position == x.position);
                                    EXPECT(evs[(size_t) e].reason == (tok == w.stop ? LLAMAHIP_DONE_STOP : LLAMAHIP_DONE_LENGTH) && !w.done);
                                    e++; w.done = 1; ended = true;
                                    dropped += n_tok - 1 - a;
                                }
                            }
                        }
                        EXPECT(e == ne && logit_rows <= 16);
                        drafted += step_drafted;
                        draft_steps += step_drafted > 0;
                        EXPECT(step_drafted == 0 || cl.mixed);
                    }
                    EXPECT(llamahip_sched_pending(sc) == 0);
                    for (const DReq &w : reqs) EXPECT(w.done == 1 && w.n_out <= w.n_predict && (w.stop >= 0 || w.n_out == w.n_predict));
                    llamahip_sched_stats ss; memset(&ss, 0, sizeof(ss)); ss.struct_size = sizeof(ss);
                    EXPECT(llamahip_sched_get_stats(sc, &ss) == 0 && ss.n_tokens == tokens && ss.n_emit_segs == emit_segs && ss.n_accepted == accepted && ss.n_drafted == drafted);
                    EXPECT(ss.n_dropped == dropped && ss.n_draft_steps == draft_steps && ss.n_tokens == ss.n_emit_segs + ss.n_accepted - ss.n_dropped && ss.n_accepted <= ss.n_drafted);
                    EXPECT(drafted > 0 && (script == 0 ? accepted == 0 : accepted > 0));
                    if (script == 15) EXPECT(accepted == drafted);
                    dropped_in_all += dropped;
                    llamahip_sched_free(sc);
                    for (DReq &w : reqs) if (w.smp) llamahip_sampler_free(w.smp);
                }
        g_sched_accept = -1;
        EXPECT(!ms || dropped_in_all > 0);          // (some greedy request met its stop token inside an accepted run)
        printf("host_sanitize: scheduler with drafted tokens: scripted accepts at draft_len 1 / 4 / 15, %lld tokens dropped behind stop tokens\n", (long long) dropped_in_all);
        if (ms) {
            // a handle that takes no drafts (the fall-back handles): the drafting scheduler plans none; what llamahip_sched_new refuses of the draft options
            g_sched_drafts = false;
            llamahip_sched_opts so; memset(&so, 0, sizeof(so));
            so.struct_size = sizeof(so); so.max_active = 2; so.draft_len = 4;
            llamahip_sched *sc = nullptr;
            EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == 0 && sc);
            if (sc) {
                std::vector<int32_t> p(6, 1);
                llamahip_request rq; memset(&rq, 0, sizeof(rq));
                rq.struct_size = sizeof(rq); rq.prompt = p.data(); rq.n_prompt = 6; rq.n_predict = 9; rq.stop_token = -1;
                EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == 0);
                std::vector<llamahip_sched_event> evs(19);
                g_sched_calls.clear();
                int32_t ne = 0;
                while (llamahip_sched_pending(sc) > 0 && g_sched_calls.size() < 50) EXPECT(llamahip_sched_step(sc, evs.data(), 19, &ne, err, sizeof(err)) == 0);
                for (const SchedCall &cl : g_sched_calls) for (const lh::SchedSeg &g : cl.segs) EXPECT(g.n_draft == 0);
                llamahip_sched_stats ss; memset(&ss, 0, sizeof(ss)); ss.struct_size = sizeof(ss);
                EXPECT(llamahip_sched_get_stats(sc, &ss) == 0 && ss.n_drafted == 0 && ss.n_draft_steps == 0 && ss.n_tokens == 9 && g_sched_calls.size() == 9);
                llamahip_sched_free(sc);
            }
            g_sched_drafts = true;
            std::vector<int32_t> bad(3, 1);
            bad[2] = V;
            so.draft_len = 16; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc && strstr(err, "draft_len"));
            so.draft_len = -1; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc && strstr(err, "draft_len"));
            so.draft_len = 4; so.ngram_min = 3; so.ngram_max = 2; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc && strstr(err, "ngram"));
            so.ngram_min = -1; so.ngram_max = 0; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc && strstr(err, "ngram"));
            so.ngram_min = 0; so.corpus = bad.data(); so.n_corpus = 3; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc && strstr(err, "corpus token id"));
            so.n_corpus = 2; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == 0 && sc);          // (the id out of range lies behind n_corpus)
            llamahip_sched_free(sc); sc = nullptr;
            so.corpus = nullptr; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc && strstr(err, "n_corpus"));
            so.n_corpus = -1; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc && strstr(err, "n_corpus"));
            // a struct that ends before draft_len: no drafting, whatever lies behind it
            so.n_corpus = 0; so.draft_len = 99; so.struct_size = (int32_t) offsetof(llamahip_sched_opts, draft_len);
            EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == 0 && sc);
            llamahip_sched_free(sc);
        }
        if (ms) {
            // one scheduler per handle at a time; a step that fails delivers nothing and loses nothing (the waiting CANCELLED events, the
            // admitted requests and the stats are all there for the step that succeeds)
            llamahip_sched_opts so; memset(&so, 0, sizeof(so));
            so.struct_size = sizeof(so); so.max_active = 2; so.chunk_tokens = 9; so.row_budget = 16;
            llamahip_sched *sa = nullptr, *sb = nullptr;
            EXPECT(llamahip_sched_new(ms, &so, &sa, err, sizeof(err)) == 0 && sa);
            EXPECT(llamahip_sched_new(ms, &so, &sb, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sb && strstr(err, "already"));
            if (sa) {
                std::vector<int32_t> p3(3, 1);
                llamahip_request rq; memset(&rq, 0, sizeof(rq));
                rq.struct_size = sizeof(rq); rq.prompt = p3.data(); rq.n_prompt = 3; rq.n_predict = 2; rq.stop_token = -1;
                int64_t id[3] = { 0, 0, 0 };
                for (int i = 0; i < 3; i++) EXPECT(llamahip_sched_submit(sa, &rq, &id[i], err, sizeof(err)) == 0);
                EXPECT(llamahip_sched_cancel(sa, id[2]) == 0);          // queued: its DONE waits for a step
                std::vector<llamahip_sched_event> evs(5);
                int32_t ne = -1;
                g_sched_fail = true;
                EXPECT(llamahip_sched_step(sa, evs.data(), 5, &ne, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && ne == 0 && llamahip_sched_pending(sa) == 3);
                EXPECT(llamahip_sched_step(sa, evs.data(), 5, &ne, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && ne == 0 && llamahip_sched_pending(sa) == 3);
                llamahip_sched_stats ss; memset(&ss, 0, sizeof(ss)); ss.struct_size = sizeof(ss);
                EXPECT(llamahip_sched_get_stats(sa, &ss) == 0 && ss.n_done == 0 && ss.n_steps == 0 && ss.n_tokens == 0);
                g_sched_fail = false;
                g_sched_calls.clear();
                EXPECT(llamahip_sched_step(sa, evs.data(), 5, &ne, err, sizeof(err)) == 0 && ne == 3);          // the CANCELLED DONE first, then a token per request
                EXPECT(evs[0].id == id[2] && evs[0].kind == LLAMAHIP_EV_DONE && evs[0].reason == LLAMAHIP_DONE_CANCELLED && evs[1].kind == LLAMAHIP_EV_TOKEN && evs[2].kind == LLAMAHIP_EV_TOKEN);
                EXPECT(g_sched_calls.size() == 1 && g_sched_calls[0].segs.size() == 2 && g_sched_calls[0].segs[0].pos == 0 && g_sched_calls[0].segs[0].n_rows == 3);
                EXPECT(llamahip_sched_get_stats(sa, &ss) == 0 && ss.n_done == 1 && ss.n_steps == 1 && ss.n_tokens == 2);
                llamahip_sched_free(sa);
                EXPECT(llamahip_sched_new(ms, &so, &sb, err, sizeof(err)) == 0 && sb);          // free again after the first one is gone
                llamahip_sched_free(sb);
            }
        }
        // shared prompt prefixes (prefix_share): the policy over a grid on exactly sized arrays against its restatement, and its refusals; then
        // whole runs against the stub's shadow cache -- at every request's first token its slot's prompt rows must be the chain over ITS prompt,
        // whatever was shared in place or copied from whichever donor; the stats against the copies the stub saw; a copy and a step that fail
        {
            auto share_ref = [](const std::vector<int32_t> &h, const std::vector<int32_t> &p, int c) {
                size_t l = 0;
                while (l < h.size() && l + 1 < p.size() && h[l] == p[l]) l++;
                return c > 0 ? (int32_t) (l / (size_t) c * (size_t) c) : 0;
            };
            long n_plans = 0, n_donors = 0;
            for (int c : { 0, 1, 4, 9 })
                for (int n_slots : { 1, 3, 16 })
                    for (int it = 0; it < 80; it++) {
                        std::vector<int32_t> prompt((size_t) (1 + rng() % 40));          // exactly sized, a small alphabet: long common prefixes
                        for (int32_t &t : prompt) t = (int32_t) (rng() % 2);
                        std::vector<std::vector<int32_t>> recs((size_t) n_slots);
                        std::vector<int32_t> is_free((size_t) n_slots), n_held((size_t) n_slots), cat;
                        for (int sl = 0; sl < n_slots; sl++) {
                            std::vector<int32_t> &h = recs[(size_t) sl];
                            const int kind = (int) (rng() % 4);
                            if (kind == 1) h.assign(prompt.begin(), prompt.begin() + (long) (rng() % (prompt.size() + 1)));          // a prefix of the prompt
                            if (kind == 2) { h = prompt; for (int k = (int) (rng() % 9); k > 0; k--) h.push_back((int32_t) (rng() % 2)); }      // the prompt and more
                            if (kind == 3) { h.resize((size_t) (rng() % 45)); for (int32_t &t : h) t = (int32_t) (rng() % 2); }
                            is_free[(size_t) sl] = it % 3 == 0 ? 1 : (int32_t) (rng() % 2);
                            n_held[(size_t) sl] = (int32_t) h.size();
                            cat.insert(cat.end(), h.begin(), h.end());
                        }
                        is_free[rng() % (size_t) n_slots] = 1;
                        int32_t sl = -7, donor = -7, inplace = -7, want_slot = -1, want_donor = -1;
                        const int32_t P = llamahip_sched_plan_prefix(n_slots, is_free.data(), cat.data(), n_held.data(), prompt.data(), (int32_t) prompt.size(), c, &sl, &donor, &inplace);
                        for (int k = 0; k < n_slots; k++) {
                            if (!is_free[(size_t) k]) continue;
                            const int32_t a = share_ref(recs[(size_t) k], prompt, c), b = want_slot < 0 ? -1 : share_ref(recs[(size_t) want_slot], prompt, c);
                            if (want_slot < 0 || a > b || (a == b && n_held[(size_t) k] < n_held[(size_t) want_slot])) want_slot = k;
                        }
                        for (int k = 0; k < n_slots; k++)
                            if (k != want_slot && (want_donor < 0 || share_ref(recs[(size_t) k], prompt, c) > share_ref(recs[(size_t) want_donor], prompt, c))) want_donor = k;
                        const int32_t in_place = share_ref(recs[(size_t) want_slot], prompt, c), given = want_donor < 0 ? -1 : share_ref(recs[(size_t) want_donor], prompt, c);
                        EXPECT(sl == want_slot && inplace == in_place);
                        if (given > in_place) { EXPECT(donor == want_donor && P == given); n_donors++; }
                        else EXPECT(donor == -1 && P == in_place);
                        EXPECT(P >= 0 && P <= (int32_t) prompt.size() - 1 && (c == 0 ? P == 0 : P % c == 0));
                        n_plans++;
                    }
            EXPECT(n_plans == 4 * 3 * 80 && n_donors > 0);
            {
                int32_t f1[1] = { 1 }, f0[1] = { 0 }, h0[1] = { 0 }, h2[1] = { 2 }, neg[1] = { -1 }, p[2] = { 1, 2 }, hp2[2] = { 1, 2 }, a = 0, b = 0, cc = 0;
                EXPECT(llamahip_sched_plan_prefix(1, f1, hp2, h2, p, 2, 1, &a, &b, &cc) == 1 && a == 0 && b == -1 && cc == 1);
                EXPECT(llamahip_sched_plan_prefix(1, f1, nullptr, h0, p, 2, 1, &a, &b, &cc) == 0);          // nothing held: no array needed
                EXPECT(llamahip_sched_plan_prefix(0, f1, hp2, h2, p, 2, 1, &a, &b, &cc) == -1 && llamahip_sched_plan_prefix(17, f1, hp2, h2, p, 2, 1, &a, &b, &cc) == -1);
                EXPECT(llamahip_sched_plan_prefix(1, f0, hp2, h2, p, 2, 1, &a, &b, &cc) == -1);             // no free slot
                EXPECT(llamahip_sched_plan_prefix(1, nullptr, hp2, h2, p, 2, 1, &a, &b, &cc) == -1 && llamahip_sched_plan_prefix(1, f1, nullptr, h2, p, 2, 1, &a, &b, &cc) == -1);
                EXPECT(llamahip_sched_plan_prefix(1, f1, hp2, nullptr, p, 2, 1, &a, &b, &cc) == -1 && llamahip_sched_plan_prefix(1, f1, hp2, h2, nullptr, 2, 1, &a, &b, &cc) == -1);
                EXPECT(llamahip_sched_plan_prefix(1, f1, hp2, h2, p, 2, 1, nullptr, &b, &cc) == -1 && llamahip_sched_plan_prefix(1, f1, hp2, h2, p, 2, 1, &a, nullptr, &cc) == -1);
                EXPECT(llamahip_sched_plan_prefix(1, f1, hp2, h2, p, 2, 1, &a, &b, nullptr) == -1);
                EXPECT(llamahip_sched_plan_prefix(1, f1, hp2, neg, p, 2, 1, &a, &b, &cc) == -1 && llamahip_sched_plan_prefix(1, neg, hp2, h2, p, 2, 1, &a, &b, &cc) == -1);
                EXPECT(llamahip_sched_plan_prefix(1, f1, hp2, h2, p, 0, 1, &a, &b, &cc) == -1 && llamahip_sched_plan_prefix(1, f1, hp2, h2, p, 2, -1, &a, &b, &cc) == -1);
                EXPECT(llamahip_sched_plan_prefix(1, f1, hp2, h2, neg, 1, 1, &a, &b, &cc) == -1);
            }
            int64_t shared_in_all = 0, copied_in_all = 0;
            for (int share : { 1, 0 })
                for (int c : { 0, 1, 4, 9 })
                    for (int max_active : { 1, 3, 4 })
                        for (int draft_len : { 0, 4 }) {
                            if (!ms) break;
                            std::vector<int32_t> corpus(40);
                            for (size_t i = 0; i < corpus.size(); i++) corpus[i] = (int32_t) ((i * 5 + 1) % (size_t) V);
                            llamahip_sched_opts so; memset(&so, 0, sizeof(so));
                            so.struct_size = sizeof(so); so.n_threads = 2; so.max_active = max_active; so.chunk_tokens = c; so.row_budget = 8;
                            so.draft_len = draft_len; so.corpus = corpus.data(); so.n_corpus = (int32_t) corpus.size(); so.prefix_share = share;
                            llamahip_sched *sc = nullptr;
                            EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == 0 && sc);
                            if (!sc) continue;
                            // a 20-token system prompt in front of distinct tails; an exact resubmission; a prompt that IS the system prompt; a short
                            // one; one with nothing in common
                            std::vector<int32_t> sys(20);
                            for (size_t i = 0; i < sys.size(); i++) sys[i] = (int32_t) ((i * 7 + 3) % (size_t) V);
                            static const int tails[8] = { 5, 11, 0, 5, -17, -1, 2, 9 }, npred[8] = { 3, 5, 2, 1, 4, 2, 6, 3 };          // (negative: -n tokens of something else)
                            std::vector<std::vector<int32_t>> prompts;
                            for (int i = 0; i < 8; i++) {
                                std::vector<int32_t> pr;
                                if (tails[i] >= 0) { pr = sys; for (int k = 0; k < tails[i]; k++) pr.push_back((int32_t) ((k * 3 + (i == 3 ? 0 : i) * 11 + 40) % V)); }
                                else for (int k = 0; k < -tails[i]; k++) pr.push_back((int32_t) ((k * 5 + 50 + i) % V));
                                prompts.push_back(pr);          // exactly sized
                            }
                            EXPECT(prompts[0] == prompts[3]);
                            for (int i = 0; i < 8; i++) {
                                llamahip_request rq; memset(&rq, 0, sizeof(rq));
                                rq.struct_size = sizeof(rq); rq.prompt = prompts[(size_t) i].data(); rq.n_prompt = (int32_t) prompts[(size_t) i].size(); rq.n_predict = npred[i]; rq.stop_token = -1;
                                int64_t id = 0;
                                EXPECT(llamahip_sched_submit(sc, &rq, &id, err, sizeof(err)) == 0 && id == (int64_t) i + 1);
                            }
                            g_sched_calls.clear(); g_sched_copies.clear();
                            g_vkv.assign(4, std::vector<uint64_t>(48));
                            for (size_t a = 0; a < 4; a++) for (size_t r = 0; r < 48; r++) g_vkv[a][r] = 0xdead0000ull + a * 100 + r;
                            std::vector<llamahip_sched_event> evs((size_t) LLAMAHIP_SCHED_EVENT_CAP(max_active, draft_len));
                            int steps = 0, firsts = 0;
                            std::vector<int> n_out(8, 0), slot_of(8, -1);
                            while (llamahip_sched_pending(sc) > 0 && steps < 400) {
                                int32_t ne = 0;
                                EXPECT(llamahip_sched_step(sc, evs.data(), (int32_t) evs.size(), &ne, err, sizeof(err)) == 0);
                                steps++;
                                for (int32_t e = 0; e < ne; e++) {
                                    const llamahip_sched_event &x = evs[(size_t) e];
                                    if (x.kind != LLAMAHIP_EV_TOKEN) continue;
                                    const size_t i = (size_t) (x.id - 1);
                                    if (n_out[i]++ > 0) { EXPECT(x.slot == slot_of[i]); continue; }
                                    // the request's first token: the prompt rows of its slot are the chain over its own prompt
                                    slot_of[i] = x.slot;
                                    EXPECT(x.position == (int32_t) prompts[i].size());
                                    uint64_t h = VKV_SEED;
                                    for (size_t r = 0; r < prompts[i].size(); r++) { h = vkv_mix(h, prompts[i][r]); EXPECT(g_vkv[(size_t) x.slot][r] == h); }
                                    firsts++;
                                }
                            }
                            EXPECT(llamahip_sched_pending(sc) == 0 && firsts == 8);
                            // no piece starts off a chunk boundary; every copy lies below its recipient's first piece
                            for (const SchedCall &cl : g_sched_calls) for (const lh::SchedSeg &g : cl.segs) if (g.n_out == 0 && c > 0) EXPECT(g.pos % c == 0);
                            llamahip_sched_stats ss; memset(&ss, 0, sizeof(ss)); ss.struct_size = sizeof(ss);
                            int64_t sum_prompt = 0, copied = 0;
                            for (const auto &pr : prompts) sum_prompt += (int64_t) pr.size();
                            for (const CopyCall &cp : g_sched_copies) { copied += cp.n_rows; EXPECT(cp.src != cp.dst && cp.src < max_active && cp.dst < max_active && cp.n_rows > 0 && cp.row_begin % std::max(c, 1) == 0 && cp.n_rows % std::max(c, 1) == 0); }
                            EXPECT(llamahip_sched_get_stats(sc, &ss) == 0 && ss.n_done == 8 && ss.n_prompt_rows + ss.n_shared_rows == sum_prompt);
                            EXPECT(ss.n_copied_rows == copied && ss.n_copy_launches == (int64_t) g_sched_copies.size() && ss.n_copied_rows <= ss.n_shared_rows);
                            if (share && c > 0) EXPECT(ss.n_shared_rows > 0 && (max_active > 1 || copied == 0));          // (one slot: in place only; whether several slots copy depends on who has evaluated what at each admission)
                            else EXPECT(ss.n_shared_rows == 0 && g_sched_copies.empty());
                            shared_in_all += ss.n_shared_rows; copied_in_all += copied;
                            llamahip_sched_free(sc);
                        }
            g_vkv.clear();
            if (ms) {
                // a copy that cannot be enqueued leaves the request queued; a step that fails behind a committed admission keeps it, its slot and its rows
                llamahip_sched_opts so; memset(&so, 0, sizeof(so));
                so.struct_size = sizeof(so); so.max_active = 2; so.chunk_tokens = 4; so.row_budget = 16; so.prefix_share = 1;
                llamahip_sched *sc = nullptr;
                EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == 0 && sc);
                if (sc) {
                    std::vector<int32_t> pa(13), pb(15);
                    for (size_t i = 0; i < pa.size(); i++) pa[i] = (int32_t) (i + 1);
                    for (size_t i = 0; i < pb.size(); i++) pb[i] = (int32_t) (i < 12 ? i + 1 : 60 + i);
                    llamahip_request rq; memset(&rq, 0, sizeof(rq));
                    rq.struct_size = sizeof(rq); rq.prompt = pa.data(); rq.n_prompt = 13; rq.n_predict = 9; rq.stop_token = -1;
                    EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == 0);
                    std::vector<llamahip_sched_event> evs(5);
                    int32_t ne = 0;
                    g_sched_calls.clear(); g_sched_copies.clear();
                    EXPECT(llamahip_sched_step(sc, evs.data(), 5, &ne, err, sizeof(err)) == 0 && ne == 1);
                    rq.prompt = pb.data(); rq.n_prompt = 15; rq.n_predict = 2;
                    EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == 0);
                    llamahip_sched_stats ss; memset(&ss, 0, sizeof(ss)); ss.struct_size = sizeof(ss);
                    g_sched_copy_fail = true;
                    EXPECT(llamahip_sched_step(sc, evs.data(), 5, &ne, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && ne == 0 && strstr(err, "prefix copy") && llamahip_sched_pending(sc) == 2);
                    EXPECT(llamahip_sched_get_stats(sc, &ss) == 0 && ss.n_shared_rows == 0 && ss.n_copy_launches == 0 && ss.n_steps == 1 && g_sched_copies.empty());
                    g_sched_copy_fail = false; g_sched_fail = true;
                    EXPECT(llamahip_sched_step(sc, evs.data(), 5, &ne, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && ne == 0 && llamahip_sched_pending(sc) == 2);
                    EXPECT(llamahip_sched_get_stats(sc, &ss) == 0 && ss.n_shared_rows == 12 && ss.n_copied_rows == 12 && ss.n_copy_launches == 1 && ss.n_steps == 1);
                    EXPECT(g_sched_copies.size() == 1 && g_sched_copies[0].src == 0 && g_sched_copies[0].dst == 1 && g_sched_copies[0].row_begin == 0 && g_sched_copies[0].n_rows == 12);
                    g_sched_fail = false;
                    const size_t call0 = g_sched_calls.size();
                    EXPECT(llamahip_sched_step(sc, evs.data(), 5, &ne, err, sizeof(err)) == 0 && g_sched_calls.size() == call0 + 1 && g_sched_copies.size() == 1);
                    if (g_sched_calls.size() == call0 + 1) {
                        const SchedCall &cl = g_sched_calls.back();
                        EXPECT(cl.segs.size() == 2 && cl.segs[1].slot == 1 && cl.segs[1].pos == 12 && cl.segs[1].n_rows == 3 && cl.segs[1].emit == 1 && cl.toks[1][0] == pb[12]);
                    }
                    while (llamahip_sched_pending(sc) > 0 && g_sched_calls.size() < 60) EXPECT(llamahip_sched_step(sc, evs.data(), 5, &ne, err, sizeof(err)) == 0);
                    EXPECT(llamahip_sched_get_stats(sc, &ss) == 0 && ss.n_done == 2 && ss.n_prompt_rows + ss.n_shared_rows == 28);
                    llamahip_sched_free(sc);
                }
                // prefix_share other than 0 or 1; a struct that ends before it: off, whatever lies behind it
                so.prefix_share = 2; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc && strstr(err, "prefix_share"));
                so.prefix_share = -1; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc && strstr(err, "prefix_share"));
                so.prefix_share = 2; so.struct_size = (int32_t) offsetof(llamahip_sched_opts, prefix_share);
                EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == 0 && sc);
                llamahip_sched_free(sc);
            }
            EXPECT(!ms || (shared_in_all > 0 && copied_in_all > 0));
            printf("host_sanitize: scheduler with shared prefixes: %ld plans against the restatement, %lld rows shared and %lld of them copied over all runs\n", n_plans, (long long) shared_in_all, (long long) copied_in_all);
        }
        // constrained requests (sched.cpp + constrain.cpp as they are): choices with long forced tails over the file's vocabulary, forced drafts off
        // and on (with and without lookup drafts), a cancel in mid-answer, a stop token inside an accepted draft; every stream against the
        // contract's loop restated on the stub's rows (forced drafts change the steps, never the tokens), the three stats identities
        if (ms) {
            const int32_t stop = 2;
            // the vocabulary's words (constrain_host_half): letters, a space, tokNNNNN.  Every string below is spelt letter by letter
            static const char *strs[] = { "yes please", "no thanks", "cab", "cabbage" };
            const uint8_t *sp[4]; int32_t sl[4];
            for (int i = 0; i < 4; i++) { sp[i] = (const uint8_t *) strs[i]; sl[i] = (int32_t) strlen(strs[i]); }
            llamahip_constraint *cc = nullptr;
            EXPECT(llamahip_constraint_new_choices(ms, sp, sl, 4, stop, &cc, err, sizeof(err)) == 0 && cc);
            long n_forced_all = 0, n_streams = 0;
            std::vector<std::vector<int32_t>> base;          // the streams with forced drafts off: every other configuration repeats them
            for (int cfg = 0; cc && cfg < 4; cfg++) {          // 0: off; 1: forced; 2: forced + lookup drafts; 3: lookup drafts alone
                llamahip_sched_opts so; memset(&so, 0, sizeof(so));
                so.struct_size = sizeof(so); so.n_threads = 2; so.max_active = 3; so.chunk_tokens = 4; so.row_budget = 8;
                so.forced_drafts = cfg == 1 || cfg == 2; so.draft_len = cfg >= 2 ? 6 : 0;
                llamahip_sched *sc = nullptr;
                EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == 0 && sc);
                if (!sc) continue;
                g_sched_calls.clear(); g_sched_accept = -1;
                const int NR = 6;
                std::vector<std::vector<int32_t>> prompts((size_t) NR), got((size_t) NR);
                std::vector<int64_t> ids((size_t) NR);
                std::vector<int> reason((size_t) NR, 0);
                static const int plens[NR] = { 1, 5, 9, 3, 12, 2 }, npred[NR] = { 16, 16, 4, 16, 16, 16 };
                for (int i = 0; i < NR; i++) {
                    prompts[(size_t) i].resize((size_t) plens[i]);
                    for (size_t k = 0; k < prompts[(size_t) i].size(); k++) prompts[(size_t) i][k] = (int32_t) ((i * 37 + k * 11 + 5) % (size_t) V);
                    llamahip_request rq; memset(&rq, 0, sizeof(rq));
                    rq.struct_size = sizeof(rq); rq.prompt = prompts[(size_t) i].data(); rq.n_prompt = plens[i]; rq.n_predict = npred[i];
                    rq.stop_token = i % 2 ? stop : -1; rq.constraint = i == 3 ? nullptr : cc; rq.constraint_state = -1;
                    EXPECT(llamahip_sched_submit(sc, &rq, &ids[(size_t) i], err, sizeof(err)) == 0);
                }
                const int32_t cap = LLAMAHIP_SCHED_EVENT_CAP(3, so.draft_len > 0 || so.forced_drafts ? 1 : 0);
                std::vector<llamahip_sched_event> evs((size_t) cap);          // exactly sized
                int32_t ne = 0;
                if (cfg != 0) { EXPECT(llamahip_sched_step(sc, evs.data(), cap - 1, &ne, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && strstr(err, "cap")); }
                int steps = 0;
                bool cancelled = false;
                while (llamahip_sched_pending(sc) > 0 && steps++ < 200) {
                    EXPECT(llamahip_sched_step(sc, evs.data(), cap, &ne, err, sizeof(err)) == 0);
                    for (int32_t e = 0; e < ne; e++) {
                        size_t i = 0;
                        while (i < ids.size() && ids[i] != evs[(size_t) e].id) i++;
                        EXPECT(i < ids.size());
                        if (i >= ids.size()) continue;
                        if (evs[(size_t) e].kind == LLAMAHIP_EV_TOKEN) got[i].push_back(evs[(size_t) e].token);
                        else reason[i] = evs[(size_t) e].reason;
                    }
                    // a cancel in mid-answer: request 4, once it has produced its first token (with forced drafts the next step would end it)
                    if (!cancelled && got[4].size() >= 1 && reason[4] == 0) { EXPECT(llamahip_sched_cancel(sc, ids[4]) == 0); cancelled = true; }
                }
                EXPECT(llamahip_sched_pending(sc) == 0 && cancelled);
                for (int i = 0; i < NR; i++) {
                    const std::vector<int32_t> &t = got[(size_t) i];
                    if (i == 4) { EXPECT(reason[4] == LLAMAHIP_DONE_CANCELLED); continue; }
                    if (i == 3) { EXPECT(reason[3] == (t.size() == 16 ? LLAMAHIP_DONE_LENGTH : LLAMAHIP_DONE_STOP)); continue; }
                    // a constrained stream: a walk of the automaton from its start that ends in DONE at the stop token, or at n_predict
                    int32_t st = llamahip_constraint_start(cc);
                    for (int32_t tok : t) { st = llamahip_constraint_advance(cc, st, tok); EXPECT(st >= 0); if (st < 0) break; }
                    const bool stopped = !t.empty() && t.back() == stop;
                    EXPECT(stopped ? (st == llamahip_constraint_done(cc) && reason[(size_t) i] == LLAMAHIP_DONE_STOP) : ((int) t.size() == npred[i] && reason[(size_t) i] == LLAMAHIP_DONE_LENGTH));
                    for (size_t k = 0; k + 1 < t.size(); k++) EXPECT(t[k] != stop);
                    n_streams++;
                }
                EXPECT(reason[2] == LLAMAHIP_DONE_LENGTH && got[2].size() == 4);          // n_predict shorter than every answer
                // (the stub's constrained rows depend on a row's token and position alone, so every configuration produces the same constrained
                // streams; the unconstrained request's made-up tokens follow the scripted accepts)
                if (cfg == 0) base = got;
                else for (int i = 0; i < NR; i++) if (i != 4 && i != 3) EXPECT(got[(size_t) i] == base[(size_t) i]);
                llamahip_sched_stats ss; memset(&ss, 0, sizeof(ss)); ss.struct_size = sizeof(ss);
                EXPECT(llamahip_sched_get_stats(sc, &ss) == 0);
                EXPECT(ss.n_forced_accepted == ss.n_forced_drafted && ss.n_tokens == ss.n_emit_segs + ss.n_accepted - ss.n_dropped && ss.n_dfa_rows > 0);
                EXPECT((so.forced_drafts != 0) == (ss.n_forced_drafted > 0) && ss.n_forced_drafted <= ss.n_drafted && ss.n_forced_accepted <= ss.n_accepted);
                if (cfg == 1) EXPECT(ss.n_dropped > 0);          // a stop token inside an accepted draft: the row behind it is dropped
                n_forced_all += (long) ss.n_forced_drafted;
                // every draft handed to the device half for a constrained segment is allowed token by token from the segment's state
                for (const SchedCall &call : g_sched_calls)
                    for (size_t j = 0; j < call.segs.size(); j++) {
                        const lh::SchedSeg &g = call.segs[j];
                        int32_t st = g.cst_state;
                        for (int32_t tok : call.drafts[j]) { if (!g.cst) break; st = llamahip_constraint_advance(g.cst, st, tok); EXPECT(st >= 0); if (st < 0) break; }
                    }
                llamahip_sched_free(sc);
            }
            // what llamahip_sched_submit refuses of a constrained request, and the two struct sizes it takes
            if (cc) {
                llamahip_sched_opts so; memset(&so, 0, sizeof(so));
                so.struct_size = sizeof(so); so.max_active = 2;
                llamahip_sched *sc = nullptr;
                so.forced_drafts = 2; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc && strstr(err, "forced_drafts"));
                so.struct_size = (int32_t) offsetof(llamahip_sched_opts, forced_drafts);          // a struct that ends before it: off, whatever lies behind
                EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == 0 && sc);
                if (sc) {
                    const int32_t p1[1] = { 5 };
                    llamahip_request rq; memset(&rq, 0, sizeof(rq));
                    rq.struct_size = sizeof(rq); rq.prompt = p1; rq.n_prompt = 1; rq.n_predict = 2; rq.stop_token = -1; rq.constraint = cc; rq.constraint_state = -1;
                    llamahip_sampler *smp = llamahip_sampler_new(1, 8);
                    rq.constraint_state = llamahip_constraint_n_states(cc); EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && strstr(err, "constraint_state"));
                    rq.constraint_state = -2; EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && strstr(err, "constraint_state"));
                    rq.constraint_state = -1; rq.stop_token = 3; EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && strstr(err, "stop token"));
                    rq.stop_token = -1; rq.sampler = smp; EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && strstr(err, "sampler"));
                    rq.sampler = nullptr;
                    llamahip_model *mo = nullptr;          // the same file on another handle
                    llamahip_constraint *other = nullptr;
                    EXPECT(llamahip_model_load(path.c_str(), 48, &o, &mo, err, sizeof(err)) == 0 && mo);
                    EXPECT(mo && llamahip_constraint_new_choices(mo, sp, sl, 4, stop, &other, err, sizeof(err)) == 0 && other);
                    rq.constraint = other; EXPECT(!other ||llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && strstr(err, "another handle"));
                    rq.constraint = cc;
                    llamahip_constraint_free(other);
                    if (mo) llamahip_model_free(mo);
                    rq.struct_size = (int32_t) offsetof(llamahip_request, constraint);          // the request before constraints: taken, the fields behind it not read
                    rq.constraint_state = 99999; EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == 0);
                    rq.struct_size -= 1; EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && strstr(err, "struct_size"));
                    EXPECT(llamahip_sched_pending(sc) == 1);
                    llamahip_sampler_free(smp);
                    llamahip_sched_free(sc);
                }
                int32_t run[16];
                EXPECT(llamahip_forced_run(nullptr, 0, run, 4) == -1 && llamahip_forced_run(cc, -1, run, 4) == -1 && llamahip_forced_run(cc, 0, run, -1) == -1);
                EXPECT(llamahip_forced_run(cc, llamahip_constraint_n_states(cc), run, 4) == -1 && llamahip_forced_run(cc, llamahip_constraint_done(cc), run, 4) == 0);
                EXPECT(llamahip_forced_run(cc, 0, nullptr, 0) == 0);
                llamahip_constraint_free(cc);
            }
            EXPECT(n_forced_all > 0 && n_streams > 0);
            printf("host_sanitize: scheduler with constrained requests: %ld streams walk their automaton in 4 configurations, %ld forced tokens drafted and accepted\n", n_streams, n_forced_all);
        }
        // llamahip_sched_submit's row limit, on a handle whose context is long enough to reach it: with chunk_tokens 0 a prompt is one piece of
        // at most LLAMAHIP_EVAL_MULTI_MAX_ROWS - max_active rows; in chunks the piece is the chunk -- and a chunk that long is refused the same way
        {
            llamahip_model *ml = nullptr;
            EXPECT(llamahip_model_load(path.c_str(), 4096, &o, &ml, err, sizeof(err)) == 0);
            for (int max_active : { 1, 3, 4 }) {
                if (!ml) break;
                const int lim = LLAMAHIP_EVAL_MULTI_MAX_ROWS - max_active;
                std::vector<int32_t> fits((size_t) lim, 1), over((size_t) lim + 1, 1);          // exactly sized
                for (int c : { 0, 9, 4000 }) {
                    llamahip_sched_opts so; memset(&so, 0, sizeof(so));
                    so.struct_size = sizeof(so); so.max_active = max_active; so.chunk_tokens = c;
                    llamahip_sched *sc = nullptr;
                    EXPECT(llamahip_sched_new(ml, &so, &sc, err, sizeof(err)) == 0 && sc);
                    if (!sc) continue;
                    llamahip_request rq; memset(&rq, 0, sizeof(rq));
                    rq.struct_size = sizeof(rq); rq.n_predict = 1; rq.stop_token = -1;
                    rq.prompt = fits.data(); rq.n_prompt = lim;
                    EXPECT(llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err)) == 0);
                    rq.prompt = over.data(); rq.n_prompt = lim + 1;
                    err[0] = 0;
                    const int rc = llamahip_sched_submit(sc, &rq, nullptr, err, sizeof(err));
                    char want[32];
                    snprintf(want, sizeof(want), "(%d)", lim);
                    if (c == 9) EXPECT(rc == 0);          // pieces of 9 rows: accepted
                    else EXPECT(rc == LLAMAHIP_ERR_PREDICT && strstr(err, "LLAMAHIP_EVAL_MULTI_MAX_ROWS - max_active") && strstr(err, want) && strstr(err, c ? "chunk_tokens" : "chunk_tokens 0"));
                    EXPECT(llamahip_sched_pending(sc) == (c == 9 ? 2 : 1));
                    llamahip_sched_free(sc);
                }
            }
            if (ml) llamahip_model_free(ml);
        }
        if (ms) {
            llamahip_sched_opts so; memset(&so, 0, sizeof(so));
            so.struct_size = sizeof(so); so.max_active = 2;
            llamahip_sched *sc = nullptr;
            so.max_active = 0;  EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc);
            so.max_active = 17; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc);
            so.max_active = 5;  EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc);      // the stub handle has 4 slots
            so.max_active = 2; so.chunk_tokens = -1; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc);
            so.chunk_tokens = 0; so.row_budget = -1; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc);
            so.row_budget = LLAMAHIP_EVAL_MULTI_MAX_ROWS - 15; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc);
            so.row_budget = 0; so.temp = -1.0; EXPECT(llamahip_sched_new(ms, &so, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT && !sc);
            so.temp = 0.0; EXPECT(llamahip_sched_new(nullptr, &so, &sc, nullptr, 0) == LLAMAHIP_ERR_PREDICT && !sc);
            EXPECT(llamahip_sched_new(ms, nullptr, &sc, err, sizeof(err)) == LLAMAHIP_ERR_PREDICT);
            llamahip_model_free(ms);
        }
        printf("host_sanitize: scheduler host half: %zu steps logged in the last run\n", g_sched_calls.size());
    }
    {   // the Q4_1 mat-mul's host half (q41_plan.cpp): the plan over the model and test shapes, and every refusal of llamahip_op_mul_mat_q4_1 on
        // exactly sized message buffers (a one-byte one included)
        using namespace lh;
        const int widths[4][2] = { { 4096, 11008 }, { 5120, 13824 }, { 6656, 17920 }, { 8192, 22016 } };
        std::vector<std::pair<int, int>> shapes;
        for (auto &w : widths) for (auto mk : { std::pair<int, int>{ 3 * w[0], w[0] }, { w[0], w[0] }, { 2 * w[1], w[0] }, { w[0], w[1] }, { 32000, w[0] } }) shapes.push_back(mk);
        for (int K : { 32, 64, 224, 256, 288, 320, 544, 896, 1376, 4096, 11008 }) for (int M : { 1, 15, 16, 17, 64, 65, 200 }) shapes.push_back({ M, K });
        int plans = 0;
        for (auto &mk : shapes)
            for (int N : { 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 100, 1048560 }) {
                const Q41Plan p = q41_plan(mk.first, mk.second, N);
                EXPECT(p.nr >= std::min(N, 16) && p.nr <= 16 && q41_plan_has_kernel(p));
                EXPECT(p.lds <= 160 * 1024 && (int64_t) p.grid_x * p.rows >= mk.first && (int64_t) (p.grid_x - 1) * p.rows < mk.first && p.grid_y == (N + 15) / 16);
                plans++;
            }
        EXPECT(!q41_plan(0, 64, 1).nr && !q41_plan(8, 48, 1).nr && !q41_plan(8, 0, 1).nr && !q41_plan(8, 64, 0).nr && !q41_plan(8, 64, 1048561).nr);
        EXPECT(!q41_plan_has_kernel(Q41Plan{ 3, 16, 320, 1, 1, 64, 2 * 64 * 48 * 4, 48 }));            // (3 rows is no compiled instance)
        const float xy = 0.0f;
        const uint8_t wq = 0;
        struct { int32_t M, K, N, ys, path; const void *w; const char *says; } bad[] = {
            { 8, 48, 2, 8, 0, &wq, "K 48 must be a positive multiple of 32" }, { 8, 0, 2, 8, 0, &wq, "K 0 must be" }, { 8, 64, 0, 8, 0, &wq, "N 0 must be >= 1" },
            { 0, 64, 2, 8, 0, &wq, "M 0 must be >= 1" }, { 8, 64, 2, 7, 0, &wq, "y_stride 7 < M 8" }, { 8, 64, 2, 8, 3, &wq, "unknown path 3" },
            { 8, 64, 2, 8, -1, &wq, "unknown path -1" }, { 8, 64, 2, 8, 1, nullptr, "not NULL" }, { 8, 64, 1048561, 8, 1, &wq, "row tiles" },
        };
        for (auto &b : bad) {
            std::vector<char> e(256, 0), e1(1, 'x');
            EXPECT(q41_op_check(b.w, b.M, b.K, &xy, b.N, &xy, b.ys, b.path, e.data(), e.size()) == -1 && strstr(e.data(), b.says));
            EXPECT(q41_op_check(b.w, b.M, b.K, &xy, b.N, &xy, b.ys, b.path, e1.data(), e1.size()) == -1 && e1[0] == 0);
            EXPECT(q41_op_check(b.w, b.M, b.K, &xy, b.N, &xy, b.ys, b.path, nullptr, 0) == -1);
        }
        EXPECT(q41_op_check(&wq, 8, 64, &xy, 17, &xy, 8, 2, err, sizeof(err)) == 0);
        printf("host_sanitize: Q4_1 mat-mul host half: %d plans, %zu refusals\n", plans, sizeof(bad) / sizeof(bad[0]));
    }
    {   // the few-row Q4_0 mat-mul's host half (set_plan.cpp): the plan of every LLaMA matrix at every row count 2 .. 60 and its launch shape,
        // every (nc, cw) pair forced -- admitted or refused with a reason, on exactly sized message buffers -- and what the rule refuses
        using namespace lh;
        auto shape = [](int M, int K, bool inter) {
            SetShape s;
            s.M = M; s.K = K; s.ngroups = (M + 7) / 8; s.nchunks = (K + 255) / 256; s.gmapF8 = inter ? s.ngroups / 2 : 0; s.tiles = true;
            return s;
        };
        const int widths[4][2] = { { 4096, 11008 }, { 5120, 13824 }, { 6656, 17920 }, { 8192, 22016 } };
        struct Mat { int M, K; bool inter; int epi; };
        std::vector<Mat> mats;
        for (auto &w : widths) {
            mats.push_back({ 3 * w[0], w[0], false, SET_EPI_ROPE_KV }); mats.push_back({ w[0], w[0], false, SET_EPI_RESID });
            mats.push_back({ 2 * w[1], w[0], true, SET_EPI_SILU_QA });   mats.push_back({ 2 * w[1], w[0], true, SET_EPI_SILU_QAH });
            mats.push_back({ w[0], w[1], false, SET_EPI_RESID });        mats.push_back({ 32000, w[0], false, SET_EPI_STORE });
        }
        for (int M : { 1, 24, 75, 6136, 6144, 12280, 12288 }) for (int K : { 64, 320, 4352 }) mats.push_back({ M, K, false, SET_EPI_STORE });
        int plans = 0, admitted = 0, refused = 0;
        for (auto &m : mats) {
            const SetShape s = shape(m.M, m.K, m.inter);
            for (int N = 2; N <= SET_ROWS_MAX; N++) {
                const bool takes = set_applies(s, N, m.epi);
                long q[7] = { 0 }, q5[5] = { 0 };
                EXPECT(set_launch_query(s, N, m.epi, nullptr, q) == takes);
                EXPECT(gemv_set_plan_query(m.M, m.K, m.inter, N, m.epi, q5) == takes);
                if (takes) {
                    EXPECT(set_plan_instantiated((int) q[0], (int) q[1]) && q[0] * q[1] * q[2] >= N && q[0] * q[1] * (q[2] - 1) < N);
                    EXPECT(q[4] > 0 && (size_t) q[4] <= SET_LDS_CAP && q[6] == q[3] * q[1] * 64 && q[6] <= 512 && q[5] >= 1);
                    EXPECT(q[2] == 1 || q[5] % (8 * q[2]) == 0);
                    for (int i = 0; i < 5; i++) EXPECT(q[i] == q5[i]);
                    plans++;
                }
                for (int nc = 0; nc <= 6; nc++)
                    for (int cw = 0; cw <= 5; cw++)
                        for (int rgw : { 0, 2, 4, 8, 9 }) {
                            SetForce f;
                            f.nc = nc; f.cw = cw; f.rgw = rgw; f.strict = true;
                            std::vector<char> why(200, 0), why1(1, 'x');
                            const bool ok = set_force_check(s, N, m.epi, f, why.data(), why.size());
                            EXPECT(set_force_check(s, N, m.epi, f, why1.data(), why1.size()) == ok && (ok || why1[0] == 0));
                            if (!ok) { EXPECT(why[0] != 0); refused++; continue; }
                            EXPECT(set_plan_instantiated(nc, cw) && set_launch_query(s, N, m.epi, &f, q));
                            EXPECT(q[0] == nc && q[1] == cw && q[2] == (N + nc * cw - 1) / (nc * cw) && (rgw == 0 || q[3] == rgw) && (size_t) q[4] <= SET_LDS_CAP && q[6] <= 512);
                            admitted++;
                        }
            }
            EXPECT(!set_applies(s, 1, m.epi) && !set_applies(s, SET_ROWS_MAX + 1, m.epi));
        }
        SetShape bare = shape(4096, 4096, false);
        bare.tiles = false;
        EXPECT(!set_applies(bare, 4, SET_EPI_RESID));                                                 // no tile copy
        EXPECT(!set_applies(shape(4096, 4096, false), 4, SET_EPI_SILU_QA) && !set_applies(shape(4096, 4096, false), 4, SET_EPI_SILU_QAH));      // not the interleaved layout
        EXPECT(!set_applies(shape(22016, 4096, true), 4, SET_EPI_ROPE_KV) && !set_applies(shape(4096, 4096, false), 4, 4) && !set_applies(shape(64, 147456, false), 4, SET_EPI_STORE));
        EXPECT(plans > 0 && admitted > 0 && refused > 0);
        printf("host_sanitize: few-row mat-mul host half: %d plans, %d forced plans admitted, %d refused\n", plans, admitted, refused);
    }
    {   // the decode attention's host half (dec_attn_plan.cpp): the plan of every LLaMA head layout and of small ones at every thread count,
        // context and set of buffers; every forced {split, stage_rows, ns, dma} admitted as asked or refused with a reason; the fused launch's geometry
        using namespace lh;
        const int shapes[][2] = { { 4096, 32 }, { 5120, 40 }, { 6656, 52 }, { 8192, 64 }, { 256, 8 }, { 1024, 8 }, { 2048, 8 }, { 256, 2 }, { 96, 3 } };
        int plans = 0, admitted = 0, refused = 0;
        for (auto &sh : shapes) {
            const int d = sh[0], H = sh[1], dh = d / H;
            for (int n_ctx : { 1, 64, 100, 1001, 1024, 1025, 2048, 4096, 4097 })
                for (int nth = 1; nth <= 64; nth++)
                    for (int mode = 0; mode < 8; mode++) {
                        const bool long_ctx = mode & 1, sync = mode & 2, xpart = mode & 4;
                        const DecAttnPlan p = dec_attn_plan(d, H, n_ctx, nth, long_ctx, sync, xpart);
                        EXPECT(p.kernel >= DEC_ATTN_PV_BLK && p.kernel <= DEC_ATTN_PV_DMA && p.why[0] == 0 && p.gx >= 1 && p.gy >= 1 && p.lds > 0);
                        EXPECT(p.threads >= 64 && p.threads <= 1024 && p.threads % 64 == 0 && p.split >= 1 && p.cpw >= 1 && (p.split - 1) * p.cpw < nth && p.split * p.cpw >= nth);
                        if (p.kernel == DEC_ATTN_PV_STREAM) EXPECT(p.SR >= 1 && p.cpw * p.SR * 8 <= PV_STREAM_QUADS && p.lds <= DEC_ATTN_LDS_CAP && p.gx == H * (dh / 32) * p.split);
                        if (p.kernel == DEC_ATTN_PV_DMA) EXPECT(xpart && dh == 128 && p.cpw <= PV_DMA_CPW_MAX && p.NS >= 2 && p.lds <= DEC_ATTN_LDS_CAP && p.gx == H * p.split);
                        if (p.kernel == DEC_ATTN_X) EXPECT(sync && n_ctx <= DEC_ATTN_X_CTX_MAX && nth <= 8 && p.lds <= DEC_ATTN_LDS_CAP);
                        EXPECT((p.kernel >= DEC_ATTN_PV_STREAM) == (long_ctx && pv_stream_applies(dh, n_ctx, nth)));
                        plans++;
                        if ((nth > 9 && nth != 24 && nth != 32 && nth != 33) || n_ctx == 1 || n_ctx == 64 || n_ctx == 1001) continue;
                        for (int split : { -1, 0, 1, 2, 3, 4, 8, 16, 32, 33 })
                            for (int sr : { -1, 0, 1, 3, 171, 512, 513 })
                                for (int ns : { -1, 0, 1, 2, 3, 37, 256, 257 })
                                    for (int dma = -2; dma <= 2; dma++) {
                                        DecAttnForce f;
                                        f.split = split; f.stage_rows = sr; f.ns = ns; f.dma = dma; f.strict = true;
                                        const DecAttnPlan q = dec_attn_plan(d, H, n_ctx, nth, long_ctx, sync, xpart, &f);
                                        if (q.kernel < 0) { EXPECT(q.why[0] != 0 && strlen(q.why) < sizeof(q.why)); refused++; continue; }
                                        EXPECT(q.why[0] == 0 && q.lds <= DEC_ATTN_LDS_CAP && (split == 0 || q.split == split) && (sr == 0 || q.SR == sr) && (ns == 0 || q.NS == ns));
                                        EXPECT((dma != 1 || q.kernel == DEC_ATTN_PV_DMA) && (dma != 0 || q.kernel != DEC_ATTN_PV_DMA) && pv_split_valid(nth, q.split));
                                        EXPECT(q.kernel != DEC_ATTN_PV_DMA || q.cpw <= PV_DMA_CPW_MAX);
                                        admitted++;
                                    }
                    }
            char why[120] = "", why1[1] = { 'x' };
            for (int nth : { 1, 8, 9 }) {
                const bool ok = qkv_attn_shape_ok(d, H, nth, 3 * d, d, 3 * d / 8, 0, why, sizeof(why));
                EXPECT(ok == (H % 8 == 0 && dh % 32 == 0 && dh <= 256 && nth <= 8) && (ok || why[0] != 0));
                EXPECT(qkv_attn_shape_ok(d, H, nth, 3 * d, d, 3 * d / 8, 0, why1, sizeof(why1)) == ok && qkv_attn_shape_ok(d, H, nth, 3 * d, d, 3 * d / 8, 0) == ok);
                EXPECT(!qkv_attn_shape_ok(d, H, nth, 3 * d, d, 3 * d / 8, d / 8) && !qkv_attn_shape_ok(d, H, nth, d, d, d / 8, 0));
            }
            const QkvAttnGeom g = qkv_attn_geom(3 * d / 32, 1000, d, H, 2048, 8);
            EXPECT(g.grid == 3 * d / 32 + H * (64 + dh / 32) && g.lds == 32 * 8 + (2048 + 8 * 32 + 16) * 4);
        }
        EXPECT(qkv_attn_instance(4, true, 8, 1) && qkv_attn_instance(4, true, 10, 2) && qkv_attn_instance(4, true, 4, 2) && !qkv_attn_instance(4, false, 8, 1) &&
               !qkv_attn_instance(2, true, 8, 1) && !qkv_attn_instance(4, true, 8, 2) && !qkv_attn_instance(4, true, 16, 1));
        EXPECT(dec_attn_plan(0, 1, 64, 1, false, false, false).kernel < 0 && dec_attn_plan(64, 0, 64, 1, false, false, false).kernel < 0 &&
               dec_attn_plan(64, 1, 0, 1, false, false, false).kernel < 0 && dec_attn_plan(64, 1, 64, 0, false, false, false).kernel < 0);
        EXPECT(plans > 0 && admitted > 0 && refused > 0);
        printf("host_sanitize: decode attention host half: %d plans, %d forced plans admitted, %d refused\n", plans, admitted, refused);
    }
    {   // the owner of device memory (dev_owner.h) on the stub allocator: groups are all-or-nothing at every failing call, release, destruction by kind
        using lh::DevOwner;
        const int64_t n_before = DevOwner::live_n.load(), b_before = DevOwner::live_bytes.load();
        for (int n : { 1, 2, 12 }) {
            for (int k = 1; k <= n + 1; k++) {          // k = n + 1: no call fails
                DevOwner own(own_stub_alloc, own_stub_release);
                char *keep = nullptr;
                g_own_fail_at = 0;
                EXPECT(own.alloc(&keep, 24) == 0 && keep);
                const int64_t n0 = DevOwner::live_n.load(), b0 = DevOwner::live_bytes.load();
                EXPECT(n0 == n_before + 1 && b0 == b_before + 24);
                char *slot[12];
                for (char *&q : slot) q = (char *) 1;          // (stale values: a failed group nulls them)
                auto group = [&]() -> int {
                    if (n == 1) return own.alloc_all({ { &slot[0], 16, true } });
                    if (n == 2) return own.alloc_all({ { &slot[0], 16, true }, { &slot[1], 40, false, lh::MEM_PINNED } });
                    return own.alloc_all({ { &slot[0], 16, true }, { &slot[1], 40 }, { &slot[2], 8, true }, { &slot[3], 1 }, { &slot[4], 100, true }, { &slot[5], 64 },
                                           { &slot[6], 3, false, lh::MEM_MAILBOX }, { &slot[7], 5 }, { &slot[8], 7, true }, { &slot[9], 9 }, { &slot[10], 11 }, { &slot[11], 4096, true } });
                };
                g_own_calls = 0; g_own_fail_at = k;
                int rc = group();
                if (k <= n) {
                    EXPECT(rc == 2);
                    for (int i = 0; i < n; i++) EXPECT(slot[i] == nullptr);
                    EXPECT(DevOwner::live_n.load() == n0 && DevOwner::live_bytes.load() == b0 && own.entries.size() == 1);
                    g_own_fail_at = 0;                  // the allocator recovers: the same group now succeeds
                    rc = group();
                }
                EXPECT(rc == 0 && DevOwner::live_n.load() == n0 + n && own.entries.size() == (size_t) n + 1);
                for (int i = 0; i < n; i++) {
                    EXPECT(slot[i] != nullptr && slot[i] != keep);
                    for (int j = 0; j < i; j++) EXPECT(slot[i] != slot[j]);
                }
                EXPECT(slot[0][0] == 0 && slot[0][15] == 0);          // the zero fill
                slot[n - 1][0] = 1;                                   // (writable to its last block)
                const int64_t b1 = DevOwner::live_bytes.load();
                own.release(&slot[0]);
                EXPECT(slot[0] == nullptr && DevOwner::live_n.load() == n0 + n - 1 && DevOwner::live_bytes.load() == b1 - 16);
                own.release(&slot[0]);                                // a null slot: nothing happens
                EXPECT(DevOwner::live_n.load() == n0 + n - 1 && own.entries.size() == (size_t) n);
            }
            EXPECT(DevOwner::live_n.load() == n_before && DevOwner::live_bytes.load() == b_before);      // every owner gave everything back
        }
        {   // destruction releases every entry once, through the release function, with the entry's kind
            memset(g_own_allocs, 0, sizeof(g_own_allocs)); memset(g_own_releases, 0, sizeof(g_own_releases));
            g_own_calls = 0; g_own_fail_at = 0;
            {
                DevOwner own(own_stub_alloc, own_stub_release);
                int32_t *a = nullptr; uint64_t *b = nullptr; char *c = nullptr; float *d = nullptr;
                EXPECT(own.alloc(&a, 4) == 0 && own.alloc(&b, 2, true, lh::MEM_MAILBOX) == 0 && own.alloc(&c, 100, true, lh::MEM_PINNED) == 0 && own.alloc(&d, 3) == 0);
                EXPECT(DevOwner::live_n.load() == n_before + 4 && DevOwner::live_bytes.load() == b_before + 16 + 16 + 100 + 12);
                own.release(&d);
                EXPECT(g_own_releases[lh::MEM_DEVICE] == 1);
            }
            EXPECT(g_own_allocs[lh::MEM_DEVICE] == 2 && g_own_allocs[lh::MEM_MAILBOX] == 1 && g_own_allocs[lh::MEM_PINNED] == 1);
            for (int kind = 0; kind < 3; kind++) EXPECT(g_own_releases[kind] == g_own_allocs[kind]);
            EXPECT(DevOwner::live_n.load() == n_before && DevOwner::live_bytes.load() == b_before);
        }
        printf("host_sanitize: device-memory owner: groups of 1, 2 and 12 at every failing allocation, release, destruction by kind\n");
    }
    printf("host_sanitize: %zu tensor bytes merged, tokenizer + sampler + bridge failure path exercised: %s\n", total, failures ? "FAILED" : "clean");
    return failures ? 1 : 0;
}
