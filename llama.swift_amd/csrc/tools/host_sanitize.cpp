// host_sanitize.cpp -- the host half of the drop-in (model-file reader, tokenizer, sampler, generation driver) under
// AddressSanitizer + UndefinedBehaviorSanitizer ("race / memory-error detection").  Built by
// `make asan` with g++ -fsanitize=address,undefined from model_file.cpp + runner.cpp as they are; the device-side
// entry points the driver calls are replaced by stubs that parse the file and then fail like a box without a GPU, so
// the run exercises: header / vocabulary / tensor-directory parsing (valid, truncated and corrupted files), multi-part
// shard merging through read_tensor, llamahip_tokenize, llamahip_sample_top_p_top_k / _from_candidates, and the
// bridge's failure path, and -- with evals that succeed on made-up logits -- the driver's whole control flow (prompt taken at once,
// chunk-exact pass + last chunk, one eval per generated token, event counts).  usage: host_sanitize <model file> [n_parts]   (exit code 0 = clean)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../../include/llama_runner.h"
#include "../../../include/llamahip.h"
#include "../model_file.h"

struct llamahip_model { lh::ModelFile file; };

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
}
namespace lh {
// eval_multi.cpp (compiled in as it is): what llamahip_eval_multi refuses of its arguments / llamahip_op_attention_rows of a caller's table
int eval_multi_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, int32_t n_seqs, const int32_t *slots, const int32_t *n_past,
                     const int32_t *tokens, const int32_t *n_tokens, int32_t chunk_tokens, char *err, size_t err_cap);
int rows_table_check(int32_t R, int32_t n_ctx, int32_t n_slots, const int32_t *row_slot, const int32_t *row_pos, const int32_t *row_keys, char *err, size_t err_cap);
int decode_handle_check(const llamahip_model *m, const char *fn, char *err, size_t err_cap) {
    if (!m) { snprintf(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    return 0;
}
}

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "host_sanitize: FAILED %s (line %d)\n", #c, __LINE__); failures++; } } while (0)

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
    printf("host_sanitize: %zu tensor bytes merged, tokenizer + sampler + bridge failure path exercised: %s\n", total, failures ? "FAILED" : "clean");
    return failures ? 1 : 0;
}
