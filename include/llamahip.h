/* llamahip.h -- C ABI of libllamahip.so: the MI355X (gfx950) drop-in for the quantized-LLaMA hot
 * path of alexrozanski/llama.swift.
 *
 * The two entry points the reference's Objective-C++ bridge binds are
 *     llama_model_load()  Sources/llamaObjCxx/bridge/LlamaPredictOperation.mm:98
 *     llama_eval()        Sources/llamaObjCxx/bridge/LlamaPredictOperation.mm:510-518
 * (called from -[LlamaPredictOperation main], .mm:790, :822, :840; model released at :900).
 * Everything else here is either an accessor the caller needs because the model is now an opaque
 * handle (vocab, hparams), the host-side text utilities the same caller uses
 * (Sources/cpp/utils.cpp:275-311 tokenizer, :345-428 sampler), or measurement / debug hooks.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types cross this boundary;
 *   - return 0 on success, LLAMAHIP_ERR_LOAD (-1000) / LLAMAHIP_ERR_PREDICT (-1001) on failure --
 *     the values of LlamaErrorCodeFailedToLoadModel / LlamaErrorCodePredictionFailed
 *     (Sources/llamaObjCxx/headers/LlamaError.h:14-19); a UTF-8 message is written to `err`;
 *   - calls are synchronous; a handle is used by one thread at a time; distinct handles are
 *     independent (no process-wide scratch, unlike the reference's static buffer, .mm:532-533);
 *   - the library never falls back to a CPU path: without a HIP device every compute entry point
 *     fails with an error.
 *
 * Numerics: results are computed with the arithmetic order of the reference's x86 AVX2+FMA+F16C
 * build, so logits are expected to be bit-identical to that build for the same
 * `n_threads` (the reference's attention V*P product depends on its thread count,
 * Sources/cpp/ggml.c:5619-5665 / 5553-5577; `n_threads` selects the same split here).
 * One operator is exact BY TEST, NOT BY CONSTRUCTION: the norm (ggml.c:5327-5385).  Its two double-precision sums are formed in a
 * different association order than the reference's sequential loops, and the single-token decode kernels by default take the second
 * moment from the producer's partial sums in one pass (sum x^2 - mean * sum x, guarded against cancellation) instead of the reference's
 * two-pass form: both carry a few 2^-53 of rounding before the result is narrowed to fp32, where a difference survives with
 * probability ~2^-29 per row.  No parity test (504-token full-depth traces, rows with a DC offset on both sides of the guard) has ever
 * observed one; LLAMAHIP_NORM_MODE=0 selects the reference's two-pass formula in every decode prologue (prompt evals always use it).
 */
#ifndef LLAMAHIP_H
#define LLAMAHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the declarations of this header are its whole dynamic symbol table. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define LLAMAHIP_OK            0
#define LLAMAHIP_ERR_UNKNOWN   (-1)      /* LlamaErrorCodeUnknown            (LlamaError.h:15) */
#define LLAMAHIP_ERR_LOAD      (-1000)   /* LlamaErrorCodeFailedToLoadModel  (LlamaError.h:17) */
#define LLAMAHIP_ERR_PREDICT   (-1001)   /* LlamaErrorCodePredictionFailed   (LlamaError.h:18) */

typedef struct llamahip_model llamahip_model;

/* Optional load-time options (pass NULL for defaults).  Not part of the reference surface: these
 * are the knobs SURVEY.md section 5 "Config / flags" routes through an extended struct so the
 * Swift API stays unchanged. */
typedef struct llamahip_opts {
    int32_t struct_size;   /* sizeof(llamahip_opts) */
    int32_t device;        /* HIP device ordinal; -1 = current device */
    int32_t layer_begin;   /* pipeline stage: first layer held by this handle (0) */
    int32_t layer_end;     /* one past the last layer; -1 = n_layer */
    int32_t n_parts;       /* 0 = by n_embd as the reference (.mm:33-38; unknown widths -> 1) */
    int32_t flags;         /* LLAMAHIP_FLAG_* */
    int32_t n_seq;         /* independent KV caches held by this handle (pipeline micro-batching); 0 = 1 */
    int32_t n_devices;     /* > 1: an in-process layer pipeline, stage s = an even share of the layers on devices[s] (below); 0 / 1 = `device` */
    int32_t devices[8];    /* HIP device ordinals of the stages, in layer order (an ordinal may repeat: several stages on one GPU) */
} llamahip_opts;
#define LLAMAHIP_MAX_DEVICES 8
/* In-process layer pipeline (SURVEY.md section 8e behind the reference's own surface): the bridge makes ONE llama_model_load call from ONE
 * process (.mm:790; LlamaRunnerBridge.mm:18-26).  A handle loaded with n_devices > 1 -- or, for a caller that passes no options such as the
 * replacement bridge, with the environment variable LLAMAHIP_DEVICES="0,1,...,7" (or a count: "8" = devices 0 .. 7) -- holds one stage per
 * device; llamahip_eval / llamahip_eval_chunks / llamahip_eval_topk / llamahip_eval_logprobs / llamahip_perplexity / llamahip_decode_greedy /
 * llamahip_verify_greedy / llamahip_decode_greedy_lookup / llamahip_verify_sample / llamahip_decode_sample_lookup /
 * llamahip_verify_sample_multi / llamahip_decode_sample_lookup_multi / llamahip_decode_greedy_window / llamahip_kv_read / llamahip_get_stats and the llama_runner_* driver work on it unchanged, the residual stream (.mm:563-564, 687-690)
 * crosses devices as stream-ordered peer copies.
 * Waiting for a stage is bounded: LLAMAHIP_PIPE_WATCHDOG_S seconds (default 600) without the stage's stream completing is LLAMAHIP_ERR_PREDICT, not a hang.
 * Results are bit for bit the single-device handle's, for every file type and flag the plain handle takes (f16 / f32 / Q4_1 files and
 * LLAMAHIP_FLAG_UNFUSED decode one pipeline eval per token, the pick by the same argmax kernel).  The stage-level entry points (llamahip_eval_stage, llamahip_stage_*) and
 * llamahip_eval_debug's dumps refuse such a handle.  LLAMAHIP_DEVICES never applies to a handle loaded with an explicit device, layer range
 * or LLAMAHIP_FLAG_HOST_ONLY. */

#define LLAMAHIP_FLAG_NO_GRAPH   1   /* launch decode kernels eagerly instead of via hipGraph */
#define LLAMAHIP_FLAG_UNFUSED    2   /* use the separate prepare+GEMV kernels for decode */
#define LLAMAHIP_FLAG_HOST_ONLY  4   /* parse + validate the file and vocab only (no device work): the
                                        handle serves tokenize / token_text / tensor_bytes / sampler;
                                        every compute call on it fails with LLAMAHIP_ERR_PREDICT */
#define LLAMAHIP_FLAG_NO_PREFILL_COPY 8 /* never build the two extra copies of the layer matrices (row-lane
                                        tiles, MFMA tiles) that the multi-token prompt GEMMs read (they are
                                        built lazily, by the first eval of 61+ rows): a third of the weight
                                        memory, long prompt evals fall back to the slower LDS-staged GEMM.
                                        Results are bit-identical either way. */

#define LLAMAHIP_FLAG_FAST_PREFILL 16 /* OPT-IN, NOT the reference's arithmetic: multi-token evals that take the matrix-core
                                        GEMM (>= 64 rows at the 7B shapes) add each Q4_0 block's 32 integer products in one
                                        MFMA and run ONE fp32 accumulation chain per output instead of the reference's eight
                                        (ggml.c:1415-1466).  Same weights, same activation codes; sums re-associated, so a mat-mul
                                        agrees to rounding only -- and every flipped 4-bit activation code downstream amplifies
                                        that: after 32 layers of the thin-margin synthetic 7B the logits differ by 0.9 on
                                        average (cosine 0.986).  2.2x the exact path.  Decode and short evals are unaffected.
                                        Never the default, never used for a parity claim. */

/* ---- the drop-in boundary ------------------------------------------------------------------ */

/* Replaces llama_model_load(fname, model, vocab, n_ctx, &error)  (.mm:98).
 * Parses ggml-model-q4_0.bin[.1 ...] (magic 0x67676d6c, 7 int32 hparams, vocab, tensors; multi-part
 * shards merged as .mm:312-495), uploads and repacks the weights, allocates the fp32 KV cache
 * (.mm:290-304) on the device. */
int llamahip_model_load(const char *path, int32_t n_ctx, const llamahip_opts *opts,
                        llamahip_model **out, char *err, size_t err_cap);

/* Replaces llama_eval(model, n_threads, n_past, embd_inp, embd_w, mem_per_token, &error) (.mm:510).
 * Runs `n_tokens` tokens at context offset `n_past`; writes the n_vocab fp32 logits of the LAST
 * token to `logits_out` (.mm:724-725).  Fails (PREDICT) if n_past + n_tokens > n_ctx. */
int llamahip_eval(llamahip_model *m, int32_t n_threads, int32_t n_past,
                  const int32_t *tokens, int32_t n_tokens, float *logits_out,
                  char *err, size_t err_cap);

/* The caller's prompt loop in one call: the reference feeds a prompt to llama_eval n_batch + 1 = 9 tokens at a time
 * (-[LlamaPredictOperation main], .mm:840-848 + 880-888).  Afterwards the KV cache and `logits_out` (may be NULL) are bit for bit
 * what ceil(n_tokens / chunk_tokens) successive llamahip_eval calls of chunk_tokens tokens (the last one shorter) leave behind:
 * every operator of llama_eval's graph works row by row except the V*P key split, which depends on the eval a row belongs to
 * (ggml.c:5459-5480) and is applied per row.  One pass over all rows runs the matrix-core GEMMs instead of 9-row ones
 * (about 4x the tokens/s of the chunk-by-chunk loop on a 500-token prompt).  n_tokens <= chunk_tokens: llamahip_eval.
 * f16 / f32 files take the one pass from 36 tokens (an 8-layer f16 file of 7B width, chunks of 9: 36 tokens 6.5 -> 4.9 ms, 504 tokens
 * 97 -> 24 ms; 18 tokens are 3.3 ms in the loop and 3.6 in one pass: DESIGN.md 12.18), on plain and in-process pipeline handles;
 * shorter calls on such files, and Q4_1 files, run the evals themselves one after the other.  The bits are the same either way. */
int llamahip_eval_chunks(llamahip_model *m, int32_t n_threads, int32_t n_past,
                         const int32_t *tokens, int32_t n_tokens, int32_t chunk_tokens, float *logits_out,
                         char *err, size_t err_cap);

/* ---- scoring a text (perplexity) ------------------------------------------------------------- */
/* llamahip_eval / llamahip_eval_chunks (chunk_tokens 0 = one eval) + each row's next-token score, reduced on the device:
 * only n_tokens * 16 bytes come back.  KV cache and logits_last (may be NULL) are bit for bit what
 * llamahip_eval / llamahip_eval_chunks of the same arguments leave.  targets: n_tokens ids, -1 = not scored;
 * NULL = tokens[i + 1] for i < n_tokens - 1, last row not scored.  Any of the three outputs may be NULL.
 * Per row i: logprob_out[i] = log softmax(logits_i)[targets[i]] in double (0.0 for an unscored row), argmax_out[i] = the
 * largest logit's index (the lowest on ties: the greedy pick), rank_out[i] = the number of logits strictly greater than the
 * target's (0: the target was the greedy pick; -1 for an unscored row).  A row holding a NaN or a +inf gives NaN / -1 / -1.
 * The log-probability is deterministic: a pure function of the row's logits (DESIGN.md "Scoring"). */
int llamahip_eval_logprobs(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t n_tokens,
                           int32_t chunk_tokens, const int32_t *targets, double *logprob_out, int32_t *argmax_out,
                           int32_t *rank_out, float *logits_last, char *err, size_t err_cap);

/* Perplexity of a token stream: windows of `window` tokens (0 = n_ctx), floor(n_tokens / window) of them, the rest unused.
 * Window k's first window - 1 tokens are evaluated at n_past 0 (chunk_tokens as above).  Row j predicts token k*window + j + 1
 * and is scored if j >= score_from (-1 = window / 2, the usual tool's choice; 0 = every row).
 * nll_sum = -sum(logprob) in double, in window order then row order; ppl = exp(nll_sum / n_scored).
 * running_ppl (may be NULL): n_windows doubles, the ppl after each window.  Overwrites the current sequence slot's KV cache. */
int llamahip_perplexity(llamahip_model *m, int32_t n_threads, const int32_t *tokens, int32_t n_tokens, int32_t window,
                        int32_t score_from, int32_t chunk_tokens, double *nll_sum, int64_t *n_scored, double *running_ppl,
                        char *err, size_t err_cap);

/* Replaces ggml_free(model.ctx)  (.mm:900). */
void llamahip_model_free(llamahip_model *m);

/* ---- accessors (the reference reads these fields off llama_model / gpt_vocab directly) ------ */
int32_t llamahip_n_vocab(const llamahip_model *m);
int32_t llamahip_n_ctx(const llamahip_model *m);
int32_t llamahip_n_embd(const llamahip_model *m);
int32_t llamahip_n_head(const llamahip_model *m);
int32_t llamahip_n_layer(const llamahip_model *m);
int32_t llamahip_n_ff(const llamahip_model *m);
int32_t llamahip_n_parts(const llamahip_model *m);
/* vocab.id_to_token[id] (utils.h:49-55); returns NULL for an id out of range */
const char *llamahip_token_text(const llamahip_model *m, int32_t id, uint32_t *len);

/* ---- host-side text utilities used by the same caller --------------------------------------- */
/* llama_tokenize(vocab, text, bos)  (utils.cpp:275-311).  Returns the token count (may exceed cap). */
int32_t llamahip_tokenize(const llamahip_model *m, const char *text, int32_t bos,
                          int32_t *out, int32_t cap);

/* Sampler state = std::mt19937 rng(seed) + the last_n_tokens window (.mm:773, :827-829). */
typedef struct llamahip_sampler llamahip_sampler;
llamahip_sampler *llamahip_sampler_new(int32_t seed, int32_t repeat_last_n);
void              llamahip_sampler_free(llamahip_sampler *s);
void              llamahip_sampler_accept(llamahip_sampler *s, int32_t id);   /* .mm:867-868, 882-883 */
/* gpt_random_prompt(rng)  (utils.cpp:102-119): the prompt the caller substitutes for an empty one (.mm:774-776);
 * consumes one draw of the sampler's rng, exactly as the reference's shared std::mt19937 does. */
const char       *llamahip_sampler_random_prompt(llamahip_sampler *s);
/* llama_sample_top_p_top_k  (utils.cpp:345-428) */
int32_t llamahip_sample_top_p_top_k(const llamahip_model *m, llamahip_sampler *s, const float *logits,
                                    double repeat_penalty, int32_t top_k, double top_p, double temp);

/* The same sampler with its first half on the device ("avoids the 128 KB logits copy per token"):
 * llamahip_eval_topk = llamahip_eval + candidate scores (temperature, repetition penalty over `last_n_tokens`) + the
 * top_k selection of utils.cpp:345-395.  With *exact == 1, cand_scores / cand_ids [0, min(top_k, n_vocab)) are the
 * reference's candidates after its partial_sort, and llamahip_sample_from_candidates finishes the draw (soft-max,
 * top-p cut, std::discrete_distribution on the sampler's mt19937: utils.cpp:397-428) -- same ids, same rng draws.
 * With *exact == 0 (two equal scores whose order only libstdc++'s partial_sort defines, +0.0 and -0.0 being equal
 * scores, a NaN, n_vocab > 32768 or top_k > 64) logits_out holds the n_vocab logits and the caller uses
 * llamahip_sample_top_p_top_k as before.
 * cand_scores / cand_ids: room for 64 entries; logits_out: n_vocab floats. */
int llamahip_eval_topk(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t n_tokens,
                       const int32_t *last_n_tokens, int32_t n_last, double repeat_penalty, int32_t top_k, double temp,
                       double *cand_scores, int32_t *cand_ids, int32_t *exact, float *logits_out, char *err, size_t err_cap);
int32_t llamahip_sample_from_candidates(llamahip_sampler *s, const double *scores, const int32_t *ids, int32_t n, double top_p);
/* the sampler's last_n_tokens window (oldest first); returns its length */
int32_t llamahip_sampler_window(const llamahip_sampler *s, int32_t *out, int32_t cap);

/* ---- extensions -------------------------------------------------------------------------------- */

/* Greedy decode loop kept on the device: step i evaluates one token at n_past + i, takes
 * argmax(logits) (lowest index on ties -- the harness' definition of "temperature 0", SURVEY.md
 * fact 8) and feeds it to step i+1 without a host round trip.  out_tokens[i] = token produced by
 * step i.  If logits_last is non-NULL it receives the final step's logits. */
int llamahip_decode_greedy(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token,
                           int32_t n_steps, int32_t *out_tokens, float *logits_last,
                           char *err, size_t err_cap);

/* Greedy decode of n_seqs INDEPENDENT sequences at once (beyond the reference's surface, whose bridge holds one conversation; SURVEY.md section 8e:
 * "throughput scales only with independent sequences in flight").  Sequence i lives in KV slot i of the handle (llamahip_opts.n_seq >= n_seqs; its
 * context was evaluated with llamahip_set_seq(i) + llamahip_eval / llamahip_eval_chunks), continues at position n_past[i] with first_tokens[i], and
 * gets out_tokens[i * n_steps + t], t < n_steps: bit for bit the tokens of llamahip_decode_greedy on that sequence alone.  The slots are stepped in
 * groups of up to 16 as sets (llamahip_stage_step_set: the weights are streamed once per step for a whole group); on a pipeline handle
 * (n_devices > 1) the groups -- at least one per stage -- are additionally pipelined over the stages: in steady state every stage (GPU) works on a
 * different group, rows and picks move between stages as stream-ordered copies.  The native form of the schedule bench.py --gpus N runs over RCCL.
 * f16 / f32 files take the same set steps on plain handles (the few-row dense mat-mul k_dense_set streams the weights once per step: DESIGN.md
 * 12.16); Q4_1 files, LLAMAHIP_FLAG_UNFUSED handles and pipeline handles over f16 / f32 stages have no set step: their sequences run one after
 * the other, llamahip_decode_greedy each. */
int llamahip_decode_greedy_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens,
                                 int32_t n_steps, int32_t *out_tokens, char *err, size_t err_cap);

/* Sampled decode of n_seqs independent sequences at once: llamahip_decode_greedy_multi's schedule (KV slot i continues at n_past[i] with
 * first_tokens[i]; groups of up to 16 slots stepped as sets, pipelined over the stages of a pipeline handle) with the reference's sampler
 * (llama_sample_top_p_top_k, .mm:851-870) in place of the argmax.  Sequence i draws with samplers[i] -- its own mt19937 and last_n_tokens
 * window, each sequence a different sampler -- and every pick is accepted into it (.mm:865-868).  Bit for bit, per sequence, the loop
 *   llamahip_eval_topk(token, n_past[i] + t) -> llamahip_sample_from_candidates (exact) / llamahip_sample_top_p_top_k (not exact) -> accept
 * on that slot alone: out_tokens[i * n_steps + t]; the samplers' windows and rng states end where that loop leaves them.  The candidate
 * selection runs on the device behind each group's step; the draw stays on the host, one group at a time while the groups behind it run.
 * out_exact (may be NULL), the same shape: 1 = drawn from the device's candidates, 0 = from the full logits row on the host (a tie only
 * libstdc++'s partial_sort orders, a NaN, a window longer than 1024 ids, top_k > 64 or n_vocab > 32768).  f16 / f32 files on plain handles
 * take the set steps too; Q4_1 files, LLAMAHIP_FLAG_UNFUSED handles and pipeline handles over f16 / f32 stages run the single-sequence loop
 * above on each slot in turn. */
int llamahip_decode_sample_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens,
                                 int32_t n_steps, llamahip_sampler *const *samplers, double repeat_penalty, int32_t top_k, double top_p,
                                 double temp, int32_t *out_tokens, int32_t *out_exact, char *err, size_t err_cap);

/* ---- greedy decode with drafted tokens (prompt-lookup / speculative decoding, exact) --------------------------------------------
 * A decode step streams every weight once to produce ONE token; an eval of 2 .. 16 rows streams them once for all its rows.  So: guess the
 * next tokens cheaply (a DRAFT), evaluate [last token, draft ...] as one eval, take every row's greedy pick and keep the longest prefix of
 * the draft the model itself would have produced, plus the one token behind it that comes for free.  The token stream is
 * llamahip_decode_greedy's; only the number of weight passes changes.
 * Why it is exact: with every row on the V*P key split of its OWN single-token eval (llamahip_eval_chunks with chunk_tokens = 1) row j of an
 * eval at n_past holds, bit for bit, the logits of a single-token eval at n_past + j -- every other operator of llama_eval's graph works row
 * by row -- and the pick is k_argmax's rule (the largest value, the lowest index on ties, a NaN never).
 * (Norm statistics, as for llamahip_stage_step_set: the fused single step takes the norm's second moment in one pass, a multi-row eval in
 * two; both narrow to the same fp32 bits except with probability ~2^-29 per value.  The equality of a verify step and single steps is
 * therefore BY TEST (tests/test_gpu_lookup.py), not structural.)
 *
 * llamahip_verify_greedy -- one verify step: rows = [token, draft[0 .. n_draft)] at n_past, n_draft 0 .. 15 (0: one plain step).
 *   picks[j], j <= *n_accept: the token llamahip_decode_greedy produces at position n_past + j; *n_accept = the number of leading draft
 *   tokens that are those picks (draft[j] == picks[j] for j < *n_accept).  picks[j] beyond that: the pick of a row that was fed a token the
 *   model would not have produced (of no use), or -1 where the row was not evaluated.  The caller's new context is n_past + *n_accept + 1
 *   and its next token picks[*n_accept]; logits_next (may be NULL): the n_vocab logits that token was picked from.
 *   KV cache: rows [n_past, n_past + *n_accept + 1) are bit for bit what single steps leave; rows AT AND ABOVE the returned context are
 *   unspecified (rejected draft positions were written) -- they are never read before they are overwritten, because every eval writes
 *   its own positions first.  n_past + n_draft + 1 > n_ctx is refused.
 * llamahip_decode_greedy_lookup -- the loop: llamahip_decode_greedy's arguments and results (out_tokens[0 .. n_steps), logits_last, KV
 *   rows [0, n_past + n_steps): bit for bit), drafts by llamahip_lookup_draft from the tokens seen so far -- context (the n_context = n_past
 *   tokens at positions [0, n_past)), first_token, everything produced -- and then from `corpus` (optional: any token stream worth
 *   looking continuations up in; NULL / 0).  A draft that would pass position n_past + n_steps - 1 is cut; where the drafter finds
 *   nothing the step is the fused single-token step.  draft_len 1 .. 15, 0 = LLAMAHIP_LOOKUP_DRAFT_LEN; ngram_min / ngram_max > 0,
 *   0 = LLAMAHIP_LOOKUP_NGRAM_MIN / _MAX.  stats (may be NULL; struct_size set by the caller): steps of either kind, tokens drafted and
 *   accepted -- n_steps = n_verify_steps + n_single_steps + n_accepted.
 * Handles: plain and in-process pipeline handles.  f16 / f32 / Q4_1 files have no per-row key split in one pass: llamahip_verify_greedy
 *   evaluates its rows one single-token step at a time and stops behind the first mismatch, llamahip_decode_greedy_lookup is
 *   llamahip_decode_greedy and reports zero drafts.  Stage handles (layer_begin / layer_end) and HOST_ONLY handles are refused; the
 *   arguments are checked first, without a device.
 * llamahip_lookup_draft -- host only, no handle, deterministic: for n = ngram_max down to ngram_min take the last n tokens of `history`,
 *   find their most recent EARLIER occurrence in history, else their last occurrence in corpus (an occurrence counts if at least one token
 *   follows it), and on the first hit copy the tokens that followed it to draft_out, up to draft_len, stopping at the end of that stream.
 *   Returns the draft's length, 0 = no hit, -1 = bad arguments (0 = the defaults here too).  A linear scan from the end of each stream.
 * llamahip_op_verify_rows -- the device half on caller-supplied rows (parity tests): logits[n_rows][n_vocab], n_rows 1 .. 16, tokens[n_rows]
 *   = [last token, draft ...]; picks[n_rows], *n_accept.
 * Defaults.  n-grams of 3 down to 1 tokens: the longest match first, a single token as the last resort (a wrong draft costs a verify step
 * that still yields one token).  LLAMAHIP_LOOKUP_DRAFT_LEN: the draft length whose break-even acceptance rate is lowest in
 * profiles/lookup_probe_7b.json (tools/lookup_probe.py; DESIGN.md "Drafted greedy decoding"). */
#define LLAMAHIP_LOOKUP_DRAFT_LEN 15
#define LLAMAHIP_LOOKUP_NGRAM_MIN 1
#define LLAMAHIP_LOOKUP_NGRAM_MAX 3
typedef struct llamahip_lookup_stats {
    int32_t struct_size;               /* sizeof(llamahip_lookup_stats) */
    int32_t n_verify_steps, n_single_steps;
    int64_t n_drafted, n_accepted;     /* draft tokens evaluated / of those, reproduced by the model */
} llamahip_lookup_stats;
int llamahip_verify_greedy(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t token, const int32_t *draft, int32_t n_draft,
                           int32_t *n_accept, int32_t *picks /* n_draft + 1 */, float *logits_next, char *err, size_t err_cap);
int llamahip_decode_greedy_lookup(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token, int32_t n_steps,
                                  const int32_t *context, int32_t n_context, const int32_t *corpus, int32_t n_corpus,
                                  int32_t draft_len, int32_t ngram_min, int32_t ngram_max,
                                  int32_t *out_tokens, float *logits_last, llamahip_lookup_stats *stats, char *err, size_t err_cap);
int32_t llamahip_lookup_draft(const int32_t *history, int32_t n_history, const int32_t *corpus, int32_t n_corpus,
                              int32_t draft_len, int32_t ngram_min, int32_t ngram_max, int32_t *draft_out);
int llamahip_op_verify_rows(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *tokens,
                            int32_t *n_accept, int32_t *picks, char *err, size_t err_cap);

/* ---- greedy decode with drafted tokens for several sequences at once (exact) ------------------------------------------------------
 * llamahip_decode_greedy_multi steps up to 16 sequences as one set, one row each; llamahip_decode_greedy_lookup steps one sequence with up
 * to 15 drafted rows.  The price of a step is set by the weight stream, not by its row count, so a server that holds 2 .. 8 conversations
 * leaves 8 .. 14 rows of every set step unused: here they carry the sequences' drafts.  The rows of a step are cut into SEGMENTS, one per
 * sequence -- [the slot's last token, its draft ...] at the slot's position and the ones behind it.  The kernels of a set step read a
 * position, a KV-cache offset and a token per row and nothing in them requires the rows' slots to be distinct, so the step is the set
 * step's launches on a descriptor built on the host, then k_verify_rows over all rows and k_accept_drafts_set (one wave per segment,
 * llamahip_verify_greedy's rule): 4 (rows + segments) bytes come back, no logits row does.  Eager, as every verify step.
 * (Norm statistics, as for set steps and verify steps: one pass in the fused single step, two in a multi-row step.  The equality of a
 * segment's rows and single steps is therefore BY TEST (tests/test_gpu_lookup_multi.py), not by construction.)
 *
 * llamahip_verify_greedy_multi -- one step: for each i < n_seqs the rows [tokens[i], drafts of sequence i ...] of KV slot slots[i] at
 *   n_past[i]; the drafts concatenated in sequence order, n_draft[i] of them (0 allowed); sum(n_draft[i] + 1) <= 16, slots distinct.
 *   n_accept[i] and picks (concatenated, n_draft[i] + 1 each): llamahip_verify_greedy's, per sequence, and its KV contract per slot.
 * llamahip_decode_greedy_lookup_multi -- the loop: llamahip_decode_greedy_multi's arguments and results (sequence i in KV slot i;
 *   out_tokens[i * n_steps ..) and KV rows [0, n_past[i] + n_steps) of slot i: bit for bit llamahip_decode_greedy's on that slot alone; rows
 *   at and above a slot's final context unspecified) with llamahip_decode_greedy_lookup's drafter: each sequence drafts from its own
 *   history (contexts: concatenated, n_past[i] tokens each; its first token; everything it has produced), then from the shared corpus.  A
 *   draft that would pass position n_past[i] + n_steps - 1 is cut; a sequence that has produced n_steps tokens leaves the step and its rows
 *   become spare.  The spare rows of a step are dealt by llamahip_lookup_deal_rows.  A step in which nothing is drafted is the captured set
 *   step (llamahip_stage_step_set; one active sequence: llamahip_stage_step) plus one host wait for the picks.  stats (may be NULL):
 *   [n_seqs], struct_size set by the caller in each; per sequence n_steps = n_verify_steps + n_single_steps + n_accepted, a step in which
 *   the sequence carried no draft counting as one of its single steps.  The handle's current slot (llamahip_set_seq) is left alone.
 *   n_seqs = 1 is llamahip_decode_greedy_lookup on slot 0.
 * Handles: plain and in-process pipeline handles; n_seqs 1 .. 16 and <= llamahip_opts.n_seq (more than 16: llamahip_decode_greedy_multi
 *   -- a 16-row step has nothing to spare).  f16 / f32 / Q4_1 files, LLAMAHIP_FLAG_UNFUSED handles and handles without a set step
 *   (llamahip_stage_set_applies) run llamahip_decode_greedy_lookup / llamahip_verify_greedy on each slot in turn.  Stage handles and
 *   HOST_ONLY handles are refused; the arguments are checked first, without a device.
 * llamahip_lookup_deal_rows -- host only, no handle, a pure function: want[i] = the draft tokens sequence i could use (0 .. 15), budget =
 *   the rows of the step (n_seqs .. 16).  Every sequence has its base row; the budget - n_seqs spare rows go one draft token at a time,
 *   round-robin in ascending sequence order, to the sequences that still want more, until the spares are used up or nobody wants more.
 *   give[i] <= want[i]; returns sum(give), -1 = bad arguments.  The token stream does not depend on the dealing, only the step counts do.
 * llamahip_op_verify_rows_set -- the device half on caller-supplied rows (parity tests): logits[n_rows][n_vocab], n_rows 1 .. 16,
 *   tokens[n_rows], seg_begin[n_segs + 1] ascending from 0 to n_rows, n_segs 1 .. n_rows; n_accept[n_segs], picks[n_rows].
 * Measured on the 7B, 2 / 4 / 8 sequences (profiles/lookup_multi_probe_7b.json, tools/lookup_probe.py --multi): a set step
 *   takes 1.93 / 2.30 / 3.07 ms, a verify step over the set filled to 16 rows 4.1 .. 4.8 ms; the loop runs at 3652 / 3645 / 3573 tokens/s
 *   aggregate when every draft is accepted, against 1037 / 1741 / 2603 for llamahip_decode_greedy_multi in the same run, and at
 *   1025 / 1724 / 2583 when nothing is ever drafted -- about 1 % slower than llamahip_decode_greedy_multi: one host wait per step. */
int llamahip_verify_greedy_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *slots, const int32_t *n_past,
                                 const int32_t *tokens, const int32_t *drafts, const int32_t *n_draft, int32_t *n_accept /* [n_seqs] */,
                                 int32_t *picks /* concatenated, n_draft[i] + 1 each */, char *err, size_t err_cap);
int llamahip_decode_greedy_lookup_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens,
                                        int32_t n_steps, const int32_t *contexts /* concatenated, n_past[i] tokens each */,
                                        const int32_t *corpus, int32_t n_corpus, int32_t draft_len, int32_t ngram_min, int32_t ngram_max,
                                        int32_t *out_tokens /* [n_seqs][n_steps] */, llamahip_lookup_stats *stats /* [n_seqs], may be NULL */,
                                        char *err, size_t err_cap);
int32_t llamahip_lookup_deal_rows(const int32_t *want, int32_t n_seqs, int32_t budget, int32_t *give);
int llamahip_op_verify_rows_set(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *tokens, const int32_t *seg_begin,
                                int32_t n_segs, int32_t *n_accept, int32_t *picks, char *err, size_t err_cap);

/* ---- sampled decode with drafted tokens (exact) -----------------------------------------------------------------------------------
 * The same trade for the reference's sampler (llama_sample_top_p_top_k, .mm:851-870), which is what the bridge runs.  The sampler is a
 * deterministic function of the row's logits, the last_n_tokens window and the std::mt19937 state.  Row j of a verify step holds the logits
 * of the single-token eval at n_past + j (above); if draft tokens 0 .. j - 1 were accepted, the window at row j is the current window
 * shifted by j with those tokens pushed -- known before the eval.  The device selects every row's candidates under that window
 * (k_topk_keys_slide + k_topk_select_rows behind the eval, in place of the greedy pick), the host draws row 0 with the real sampler and
 * accepts the draw, draws row 1 only if that draw was draft[0], and so on: it stops at the first draw the draft does not continue with.
 * The walk consumes exactly the rng draws of the token-by-token loop
 *   llamahip_eval_topk -> llamahip_sample_from_candidates (exact) / llamahip_sample_top_p_top_k (not exact) -> llamahip_sampler_accept
 * and leaves the window where that loop leaves it: the token stream is that loop's, bit for bit.
 * (Norm statistics as above: the equality of a verify row and a single step is BY TEST -- tests/test_gpu_sample_lookup.py -- not structural.)
 *
 * llamahip_verify_sample -- one step.  `sampler` has already accepted `token` (the loop above: eval_topk -> draw -> accept); rows =
 *   [token, draft[0 .. n_draft)] at n_past, n_draft 0 .. 15.  For every row j the walk reaches: picks[j] = the sampler's draw at position
 *   n_past + j, accepted into the sampler; exact[j] (may be NULL) = 1 drawn from the device's candidates, 0 drawn from the row's logits (a
 *   tie only libstdc++'s partial_sort orders, a NaN: that row alone is copied to the host).  Rows not reached: picks[j] = exact[j] = -1.
 *   *n_accept = the row the walk stopped at = the number of leading draft tokens that are the draws.  New context n_past + *n_accept + 1,
 *   next token picks[*n_accept].  KV rows: llamahip_verify_greedy's contract.  Arguments (llamahip_verify_greedy's, a null sampler, top_k
 *   < 1, temp / repeat_penalty <= 0) are checked before any device work.
 *   Where the device cannot make candidates (top_k > 64, n_vocab > 32768, a window longer than 1024 ids) the walk takes every row it
 *   reaches from its logits.  f16 / f32 / Q4_1 files and LLAMAHIP_FLAG_UNFUSED handles evaluate their rows one llamahip_eval_topk step at a
 *   time and stop behind the first mismatch; so does n_draft = 0.
 * llamahip_decode_sample_lookup -- the loop: llamahip_decode_greedy_lookup's arguments, refusals, drafter, draft cut and stats identity
 *   (n_steps = n_verify_steps + n_single_steps + n_accepted); where nothing is drafted the step is one llamahip_eval_topk step.
 *   out_tokens [n_steps], out_exact [n_steps] (may be NULL), the sampler's window and rng state and KV rows [0, n_past + n_steps) are bit
 *   for bit what the single-sequence loop above leaves on that slot.  In all the cases of the previous paragraph nothing is drafted: the
 *   single-token loop runs and zero drafts are reported.  (On a pipeline handle llamahip_eval_topk returns the logits row, so single steps
 *   report exact = 0 there while verify rows report the last stage's selection; the tokens are the same either way.)
 * llamahip_op_topk_slide -- the device half on caller-supplied rows (parity tests): logits[n_rows][n_vocab], n_rows 1 .. 16; ids: ONE stream
 *   of n_last + n_rows - 1 ids, row r's window = ids[r .. r + n_last), n_last <= 1024 (ids outside [0, n_vocab) are ignored, as by the
 *   sampler); out_scores / out_ids [n_rows][64], out_exact [n_rows] -- row r bit for bit llamahip_op_topk on that row with that window. */
int llamahip_verify_sample(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t token, const int32_t *draft, int32_t n_draft,
                           llamahip_sampler *sampler, double repeat_penalty, int32_t top_k, double top_p, double temp,
                           int32_t *n_accept, int32_t *picks /* n_draft + 1 */, int32_t *exact /* n_draft + 1, may be NULL */,
                           char *err, size_t err_cap);
int llamahip_decode_sample_lookup(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token, int32_t n_steps,
                                  const int32_t *context, int32_t n_context, const int32_t *corpus, int32_t n_corpus,
                                  int32_t draft_len, int32_t ngram_min, int32_t ngram_max, llamahip_sampler *sampler,
                                  double repeat_penalty, int32_t top_k, double top_p, double temp,
                                  int32_t *out_tokens, int32_t *out_exact /* may be NULL */, llamahip_lookup_stats *stats,
                                  char *err, size_t err_cap);
int llamahip_op_topk_slide(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *ids, int32_t n_last,
                           double repeat_penalty, int32_t top_k, double temp,
                           double *out_scores, int32_t *out_ids, int32_t *out_exact, char *err, size_t err_cap);

/* ---- sampled decode with drafted tokens for several sequences at once ---------------------------------------------------------------
 * The eighth cell of {greedy, sampled} x {one sequence, several} x {plain, drafted}, and the one a server uses: the bridge never decodes
 * greedily (.mm:851-870).  Two halves that exist above meet here.  ROWS: a verify step over a set evaluates rows cut into per-slot segments,
 * every row the single-token eval of its slot at its own position (llamahip_verify_greedy_multi).  SAMPLER: the sampler is a deterministic
 * function of (row logits, last_n_tokens window, mt19937 state) and the window at row j of a segment is known before the eval
 * (llamahip_verify_sample).  So behind the set step's launches the device selects every row's candidates -- k_topk_keys_slide_set +
 * k_topk_select_rows on the last stage's stream, in place of k_verify_rows + k_accept_drafts_set: every segment slides inside its own id
 * stream (that sequence's window, then its draft) of one id pool, addressed through a per-row table of at most 16 entries that the host
 * builds -- and the host walks every segment with that sequence's own sampler exactly as llamahip_verify_sample walks its rows.  The accept
 * step is the host's: what a segment accepts depends on draws of a host-side mt19937, so no device kernel can count it, and the loop keeps
 * the slots' device words in step from the host.  Eager, as every verify step.
 * (Norm statistics, as for set steps and verify steps: one pass in the fused single step, two in a multi-row step.  The equality of a
 * segment's rows and single steps is therefore BY TEST (tests/test_gpu_sample_lookup_multi.py), not by construction.)
 *
 * llamahip_verify_sample_multi -- one step: llamahip_verify_greedy_multi's arguments (slots distinct, sum(n_draft[i] + 1) <= 16, context
 *   overflow per slot) plus one sampler per sequence (distinct, none NULL; llamahip_verify_sample's parameter checks), all checked first,
 *   without a device.  samplers[i] has already accepted tokens[i].  Per sequence llamahip_verify_sample's contract holds: n_accept[i]; picks
 *   and exact (concatenated, n_draft[i] + 1 each; exact may be NULL; -1 in both behind the walk); the sampler's window and rng state; KV
 *   rows [n_past[i], n_past[i] + n_accept[i] + 1) of slot slots[i] -- bit for bit.  A reached row flagged inexact is fetched alone from the
 *   device and drawn by llamahip_sample_top_p_top_k; where the device cannot make candidates for a sequence (a window longer than 1024
 *   ids) or for any (top_k > 64, n_vocab > 32768) those rows are drawn from their logits.
 * llamahip_decode_sample_lookup_multi -- the loop: llamahip_decode_greedy_lookup_multi's arguments, refusals, drafter, draft cut, dealing
 *   (llamahip_lookup_deal_rows) and stats identity (per sequence n_steps = n_verify_steps + n_single_steps + n_accepted), with one sampler
 *   per sequence as above.  A sequence whose sampler window exceeds 1024 ids wants no draft; with top_k > 64 or n_vocab > 32768 nobody
 *   drafts.  A step in which nothing is dealt is llamahip_decode_sample_multi's step: the captured set step (one active sequence: the
 *   single step), the candidate selection over the active rows and the host draw.  After a verify step the host writes the slots'
 *   {position, cursor} words on every stage before the next captured step continues them.  Per sequence, bit for bit the loop
 *   llamahip_eval_topk -> draw -> accept on that slot alone: out_tokens[i * n_steps ..), the sampler's window and rng state, KV rows
 *   [0, n_past[i] + n_steps) of slot i.  out_exact [n_seqs][n_steps] (may be NULL): that loop's flags on a PLAIN handle -- every row here,
 *   of plain and of verify steps, is selected on the last stage's device, on pipeline handles too (unlike llamahip_decode_sample_lookup,
 *   whose single steps report 0 there).  The handle's current slot (llamahip_set_seq) is left alone.  n_seqs = 1 is
 *   llamahip_decode_sample_lookup on slot 0.
 * Handles: plain and in-process pipeline handles; n_seqs 1 .. 16 and <= llamahip_opts.n_seq (more than 16: llamahip_decode_sample_multi).
 *   f16 / f32 / Q4_1 files, LLAMAHIP_FLAG_UNFUSED handles, handles without a set step (llamahip_stage_set_applies) and a one-row step run
 *   llamahip_decode_sample_lookup / llamahip_verify_sample on each slot in turn.  Stage handles and HOST_ONLY handles are refused.
 * llamahip_op_topk_slide_set -- the device half on caller-supplied rows (parity tests): logits[n_rows][n_vocab], n_rows 1 .. 16, top_k
 *   1 .. 64; seg_begin[n_segs + 1] ascending from 0 to n_rows; segment s slides inside ids[seg_ids_off[s] ..): its row j's window is
 *   ids[seg_ids_off[s] + j .. + seg_n_last[s]), and seg_ids_off[s] + seg_n_last[s] + rows_s - 1 <= n_ids.  seg_n_last[s] > 1024 reports that
 *   segment's rows inexact and leaves the others alone.  out_scores / out_ids [n_rows][64], out_exact [n_rows] -- row r bit for bit
 *   llamahip_op_topk on that row with that window.  Refusals name their limit, before any launch.
 * Measured on the 7B, 2 / 4 / 8 sequences (profiles/sample_lookup_multi_probe_7b.json, tools/lookup_probe.py --multi --sampled; DESIGN.md
 *   12.14): a sampled verify step over the set filled to 16 rows takes 4.1 .. 4.8 ms, 0.01 .. 0.08 ms more than the greedy one of the same
 *   rows in the same run; the loop runs at 3699 / 3701 / 3606 tokens/s aggregate when every draft is accepted, against 1015 / 1750 / 2580
 *   for llamahip_decode_sample_multi in the same run, and at 1016 / 1751 / 2588 when nothing is ever drafted -- level with it. */
int llamahip_verify_sample_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *slots, const int32_t *n_past,
                                 const int32_t *tokens, const int32_t *drafts, const int32_t *n_draft, llamahip_sampler *const *samplers,
                                 double repeat_penalty, int32_t top_k, double top_p, double temp, int32_t *n_accept /* [n_seqs] */,
                                 int32_t *picks /* concatenated, n_draft[i] + 1 each */, int32_t *exact /* same shape, may be NULL */,
                                 char *err, size_t err_cap);
int llamahip_decode_sample_lookup_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens,
                                        int32_t n_steps, const int32_t *contexts /* concatenated, n_past[i] tokens each */,
                                        const int32_t *corpus, int32_t n_corpus, int32_t draft_len, int32_t ngram_min, int32_t ngram_max,
                                        llamahip_sampler *const *samplers, double repeat_penalty, int32_t top_k, double top_p, double temp,
                                        int32_t *out_tokens /* [n_seqs][n_steps] */, int32_t *out_exact /* same, may be NULL */,
                                        llamahip_lookup_stats *stats /* [n_seqs], may be NULL */, char *err, size_t err_cap);
int llamahip_op_topk_slide_set(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *ids, int32_t n_ids,
                               const int32_t *seg_begin, int32_t n_segs, const int32_t *seg_ids_off, const int32_t *seg_n_last,
                               double repeat_penalty, int32_t top_k, double temp,
                               double *out_scores, int32_t *out_ids, int32_t *out_exact, char *err, size_t err_cap);

/* ---- generating past the context window ----------------------------------------------------------------------------------------------
 * The reference stops when the KV cache is full (n_predict = min(n_predict, n_ctx - n_inp), .mm:812) and every entry point above refuses
 * to pass n_ctx.  What every LLaMA runtime offers instead: keep the first n_keep tokens, drop the older half of the rest, go on.
 * Two modes carry the plan out; the exact one is the default everywhere:
 *   LLAMAHIP_CTX_REEVAL  rows [0, n_keep) stay; the surviving tail is evaluated again at its new positions (llamahip_eval /
 *                        llamahip_eval_chunks at n_past = n_keep).  Defined purely by llama_eval calls, so it is EXACT: the reference making
 *                        the same calls leaves the same bits.  Costs one eval of the tail.
 *
 * llamahip_ctx_overflow_plan -- host only, pure, the one rule every loop shares: *n_discard = (n_past - n_keep) / 2; returns the new
 *   context n_past - *n_discard, or -1 (and *n_discard = 0) where that leaves n_discard < 1 or the arguments are out of range
 *   (0 <= n_keep <= n_past <= n_ctx).
 * llamahip_decode_greedy_window -- llamahip_decode_greedy in legs.  context: the n_context = n_past tokens at positions [0, n_past), as
 *   llamahip_decode_greedy_lookup takes them.  Whenever the pending token has no room (position == n_ctx) the plan is applied -- the
 *   tail's tokens go through llamahip_eval_chunks(n_past = n_keep, chunk_tokens), chunk_tokens 0 = one
 *   llamahip_eval -- the loop's own token list drops the discarded tokens, and the pending token is evaluated as an ordinary single step.
 *   n_steps may exceed n_ctx many times over; n_past == n_ctx on entry is allowed.  out_tokens [n_steps]; logits_last (may be NULL): the
 *   last step's logits; *n_past_out (may be NULL): the context the cache holds afterwards.  Refused before any device work: what
 *   llamahip_decode_greedy refuses (HOST_ONLY and stage handles, token ids out of range), a mode other than LLAMAHIP_CTX_REEVAL or LLAMAHIP_CTX_SHIFT, n_context != n_past,
 *   n_past > n_ctx, chunk_tokens < 0, and n_keep outside [0, n_ctx - 2] (nothing could be discarded at the wall).
 *
 *   LLAMAHIP_CTX_SHIFT   NOT the reference's arithmetic -- opt-in, never a default, never used for a parity claim (as LLAMAHIP_FLAG_FAST_PREFILL).
 *                        The same plan carried out IN PLACE: the surviving K / V rows of every layer move down by n_discard positions on the
 *                        device and every key is re-rotated by -n_discard positions (llamahip_kv_shift_rows, one launch per stage); nothing is
 *                        evaluated again.  Two differences from re-evaluation: every moved key is narrowed to fp32 a second time, and the moved
 *                        rows of every layer but the first keep the influence of the dropped tokens (they were computed attending to them).
 *                        What IS claimed, and tested bit for bit: the kernel's arithmetic below, that no other row is written, and that the loop
 *                        equals llamahip_decode_greedy legs with llamahip_kv_shift_rows calls between them.  Its value is 4: modes 0, 2 and 3 stay
 *                        refused, as they always were.  Measured on the 7B (profiles/overflow_shift_probe_7b.json), per
 *                        crossing, median (min .. max) of five fresh processes, n_keep 0 and 1 (disjoint ranges / one row of overlap):
 *                        the shift 0.102 ms (0.096 .. 0.108) at n_ctx 512 and 0.37 ms (0.367 .. 0.380) at 2048 against 19.8 ms (19.8 .. 20.0)
 *                        and 70.8 ms (70.7 .. 71.0) for one eval of the same tail --
 *                        the shift's max lies below the re-eval's min at both sizes, the rule that justifies the mode.
 *   llamahip_decode_greedy_window with mode LLAMAHIP_CTX_SHIFT calls, at the wall, llamahip_kv_shift_rows on the current slot with row_begin =
 *   n_keep + n_discard, n_rows = position - n_keep - n_discard and the plan's n_discard in place of the eval; chunk_tokens is ignored (still
 *   checked); every other argument check is the same.
 *
 * llamahip_kv_shift_rows -- n_shifts (1 .. LLAMAHIP_KV_SHIFT_MAX) shifts {slot[i], row_begin[i], n_rows[i], n_discard[i]} in one
 *   k_kv_shift_rows launch per stage, each on its own device and stream, waited for; every file type.  Afterwards rows [row_begin - n_discard,
 *   row_begin - n_discard + n_rows) of every layer of the slot hold the rows [row_begin, row_begin + n_rows): V bytewise; a K pair (x0, x1) at
 *   elements (e, e + 1), e even, with pr = (e % head size) / 2 and (c, s) = (cos, sin) of entry [n_discard][pr] of the handle's own double
 *   table (llamahip_debug_rope_table gives the same values), as
 *       y0 = (float) (rn(rn((double) x0 * c) + rn((double) x1 * s)))        y1 = (float) (rn(rn((double) x1 * c) - rn((double) x0 * s)))
 *   every operation rounded on its own in double, nothing contracted.  The two ranges may overlap in any way (n_discard >= 1).  NO other row
 *   of any slot or layer is written; the current slot is left alone; n_rows[i] == 0 is a no-op entry.  Results that are subnormal in fp32
 *   are outside the contract.  Refused before any device work, the message naming the limit: a null handle, n_shifts outside 1 .. 16, null
 *   arrays, a slot outside [0, n_seq), a slot twice, n_discard < 1, rows outside [0, n_ctx] before or after the move, HOST_ONLY and stage
 *   handles, a slot below a live scheduler's max_active.
 * llamahip_cur_seq -- the handle's current slot (llamahip_set_seq), -1 for a null handle. */
#define LLAMAHIP_CTX_REEVAL 1
#define LLAMAHIP_CTX_SHIFT 4             /* (4: existing callers and tests know 0, 2 and 3 as refused) */
#define LLAMAHIP_KV_SHIFT_MAX 16         /* shifts in one llamahip_kv_shift_rows call */
#define LLAMAHIP_KV_SHIFT_ROWS_IN_FLIGHT 8   /* rows a thread of k_kv_shift_rows loads before it stores them (its batch edge, for tests) */
int32_t llamahip_ctx_overflow_plan(int32_t n_ctx, int32_t n_past, int32_t n_keep, int32_t *n_discard);
int llamahip_decode_greedy_window(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token, int32_t n_steps,
                                  const int32_t *context, int32_t n_context, int32_t n_keep, int32_t mode, int32_t chunk_tokens,
                                  int32_t *out_tokens, float *logits_last, int32_t *n_past_out, char *err, size_t err_cap);
int llamahip_kv_shift_rows(llamahip_model *m, int32_t n_shifts, const int32_t *slot, const int32_t *row_begin, const int32_t *n_rows,
                           const int32_t *n_discard, char *err, size_t err_cap);
int32_t llamahip_cur_seq(const llamahip_model *m);

/* ---- the prompts of several sequences in one weight pass ------------------------------------------------------------------------------
 * The *_multi decode loops above step up to 16 conversations per weight stream, but every slot's context still had to be evaluated with
 * llamahip_set_seq(i) + llamahip_eval / llamahip_eval_chunks: n_seqs evals, each streaming every weight matrix (a 9-token eval of the 7B is
 * almost all weight stream).  llamahip_eval_multi evaluates R = sum n_tokens[i] rows cut into SEGMENTS, one per KV slot -- segment i the
 * n_tokens[i] tokens of slot slots[i] at n_past[i] -- in ONE pass: every operator of llama_eval's graph works row by row except the RoPE /
 * KV append and the attention, and those two only need each row's position, cache and V*P key split, which they read from a device-resident
 * ROW TABLE {pos, keys, kv_off} (rows_attn.hip: one RoPE launch and one score / soft_max . V launch pair per layer for all the rows of all
 * the short segments; a segment of more than 60 rows takes the long eval's attention launches on its own rows and cache).  The mat-muls run
 * over all R rows with the kernel a single eval of R rows takes; the final norm and the lm head run over the n_seqs last rows only.
 *
 * Contract: for every i the call leaves the bits of llamahip_set_seq(slots[i]) + llamahip_eval_chunks(n_past[i], tokens_i, n_tokens[i],
 * chunk_tokens) on that slot alone (chunk_tokens 0: llamahip_eval) -- KV rows [n_past[i], n_past[i] + n_tokens[i]) of slot slots[i] in
 * every layer, and row i of logits_out.  No other KV row is touched, the handle's current slot is left alone, the logits row map of
 * llamahip_stage_logits is reset.  (A one-token segment is a single-token eval, whose norm statistics are one-pass in the fused step and
 * two-pass here: equality there is BY TEST -- tests/test_gpu_eval_multi.py -- not structural, as for set steps and verify steps.)
 * Refused before any device work, the message naming the limit, the handle last: n_seqs < 1 or > llamahip_opts.n_seq, a slot out of range
 * or named twice, n_tokens[i] < 1, n_past[i] < 0 or n_past[i] + n_tokens[i] > n_ctx, a token id out of range, chunk_tokens < 0,
 * R > LLAMAHIP_EVAL_MULTI_MAX_ROWS, HOST_ONLY and stage handles.
 * Handles: Q4_0 plain handles and in-process pipeline handles take the one pass (the R residual rows cross the stages as an eval's do, every
 * stage builds the table on its own device); LLAMAHIP_FLAG_UNFUSED / _NO_GRAPH / _NO_PREFILL_COPY do not change a multi-row eval.  f16 / f32
 * / Q4_1 files, LLAMAHIP_FLAG_FAST_PREFILL handles (their GEMM choice depends on the row count: no parity claim), n_seqs == 1 and the shapes of
 * the measured rule below run the per-slot loop of the contract itself and report its eval count in stats->n_passes.
 * Numbers (7B, one MI355X, chunks of 9, ms per call, one pass against the per-slot loop; tools/eval_multi_probe.py, profiles/eval_multi_probe_7b.json):
 *   segments x rows    2 x 9   4 x 9   8 x 9   16 x 9   8 x 32   16 x 32   2 x 128   16 x 128   2 x 512   4 x 512
 *   one pass            4.77    7.59   13.36    19.66    23.62     42.31     21.40     160.34     70.59    146.76
 *   loop                6.12   12.21   24.45    49.10    53.83    107.85     29.34     234.98     72.20    144.45
 *   The rule that follows from it: more than 1024 rows in segments of 512 rows or more each (the one shape family where the pass measured
 *   slower than the loop by more than the loop's spread) run the per-slot loop; the bits are the same.  Long segments keep their own
 *   attention launches because joining the table launch measured slower (16 x 128 rows: 155.9 against 175.7 ms).  DESIGN.md 12.17.
 * llamahip_eval_multi_rows -- host only, no handle, pure: the row table of such a pass.  Row r, the j-th of segment i's N_i rows:
 *   row_seg[r] = i, row_pos[r] = n_past[i] + j, row_keys[r] = the key count the reference splits over its threads for that row
 *   (n_past[i] + N_i; chunk_tokens > 0: n_past[i] + min(N_i, (j / chunk_tokens + 1) * chunk_tokens)).  Any output may be NULL.
 *   Returns R, or -1 for bad arguments (a segment outside [0, n_ctx], R > LLAMAHIP_EVAL_MULTI_MAX_ROWS). */
#define LLAMAHIP_EVAL_MULTI_MAX_ROWS 2048
typedef struct llamahip_eval_multi_stats {
    int32_t struct_size;
    int32_t n_rows;            /* sum of n_tokens */
    int32_t n_passes;          /* weight passes taken: 1 = one pass over all rows; the per-slot loop reports its eval count */
    int32_t n_short_segs, n_long_segs;   /* segments whose attention ran in the table launch / in launches of their own */
    int32_t attn_groups;       /* attention launch groups per layer: 1 for all short segments together + 1 per long segment */
} llamahip_eval_multi_stats;
int llamahip_eval_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *slots,
                        const int32_t *n_past, const int32_t *tokens /* concatenated, n_tokens[i] each */,
                        const int32_t *n_tokens, int32_t chunk_tokens /* 0 = one eval per segment */,
                        float *logits_out /* [n_seqs][n_vocab], may be NULL */,
                        llamahip_eval_multi_stats *stats /* may be NULL */, char *err, size_t err_cap);
int32_t llamahip_eval_multi_rows(int32_t n_ctx, int32_t n_seqs, const int32_t *n_past, const int32_t *n_tokens,
                                 int32_t chunk_tokens, int32_t *row_seg, int32_t *row_pos, int32_t *row_keys);

/* ---- scoring several texts in one weight pass ------------------------------------------------------------------------------------------
 * llamahip_eval_logprobs streams every weight matrix once per text; a multiple-choice item -- one context, a few short endings -- pays that
 * per ending for about ten useful rows.  llamahip_eval_logprobs_multi scores the segments of several KV slots in llamahip_eval_multi's ONE
 * pass: the final norm and the lm head run over the SCORED rows only (gathered side by side in ascending row order, the lm head with the
 * kernel a scoring eval of that many rows takes), k_row_logprob reduces those rows on the last stage's stream and 16 bytes per scored row
 * come back, scattered to row order on the host.  No scored row: no lm head at all.
 *
 * Contract: for every i the call leaves, bit for bit, what llamahip_set_seq(slots[i]) + llamahip_eval_logprobs(n_past[i], tokens_i,
 * n_tokens[i], chunk_tokens, targets_i, ...) leave on that slot alone -- logprob / argmax / rank of the scored rows, and KV rows
 * [n_past[i], n_past[i] + n_tokens[i]) of every layer.  No other KV row is touched, the handle's current slot is left alone, the logits row
 * map of llamahip_stage_logits is reset.  targets: R = sum n_tokens[i] ids in row order, -1 = not scored; NULL = the next token inside the
 * row's segment, each segment's last row unscored.
 * ONE DEVIATION: an unscored row takes no lm head, so it reports logprob 0.0, rank -1 and ARGMAX -1 (llamahip_eval_logprobs still computes
 * that row's argmax).  Skipping the row is the point: the context rows of a whole-text scoring job never reach the lm head.  The per-slot
 * loop below reports -1 there too, so the outputs do not depend on the path taken.
 * (A one-token segment is a single-token eval on the yardstick side -- the fused decode step with one-pass norm statistics, two-pass here:
 * equality there is BY TEST -- tests/test_gpu_score_multi.py -- not structural, as for llamahip_eval_multi.)
 * Refused before any device work, the message naming the limit and this function, the handle last: what llamahip_eval_multi refuses of the
 * same arguments, and a target outside [-1, n_vocab).
 * Handles and fall-backs: llamahip_eval_multi's -- f16 / f32 / Q4_1 files, LLAMAHIP_FLAG_FAST_PREFILL handles, n_seqs == 1, and more than
 * 1024 rows in segments of 512 rows or more each run llamahip_eval_logprobs slot by slot and report its eval count in stats->n_passes.
 * Numbers (7B, one MI355X, n_past 64, every row scored, ms per call, median of five fresh processes; tools/score_probe.py,
 * profiles/score_multi_probe_7b.json):
 *   segments x rows    4 x 10   8 x 10   16 x 10   16 x 32   4 x 128
 *   one pass             7.99    14.17     20.68     43.67     38.03
 *   per-slot loop       12.70    25.39     50.42    111.36     59.04
 *   No measured shape is slower than the loop, so the loop rule stays llamahip_eval_multi's.  llamahip_score_choices with four endings of 10
 *   tokens behind a context of 64 / 256 tokens: 19.87 / 28.83 ms, against 59.89 / 93.24 for the per-choice sequence of its contract and
 *   53.98 / 104.36 for four llamahip_eval_logprobs calls of the whole text.  DESIGN.md 12.25.
 *
 * llamahip_score_choices -- the multiple-choice call on KV slots 0 .. n_choices - 1, which it overwrites: the context is evaluated once on
 * slot 0, rows [0, n_context - 1) are copied to the other slots in one stream-ordered launch (llamahip_kv_copy_rows' kernel, no host wait),
 * and one pass of llamahip_eval_logprobs_multi scores segment i = [context[n_context - 1], ending_i[0 .. n_i - 1)] at n_context - 1 against
 * the targets ending_i, every row scored.
 * Contract: for every choice i, bit for bit, (1) if n_context > 1 llamahip_eval_chunks(0, context[0 .. n_context - 1), chunk_tokens)
 * (chunk_tokens 0: llamahip_eval), then (2) llamahip_eval_logprobs at n_context - 1 of that segment in one eval, on slot i alone: the
 * per-row logprobs, n_greedy[i] = the rows whose target had rank 0, KV rows [0, n_context - 1 + n_i) of slot i.  logprob_sum[i] =
 * 0.0 + lp[0] + lp[1] + ..., summed in double in ascending row order on the host.  n_choices == 1 is that sequence itself.
 * Refused before any device work: n_context < 1, n_choices outside 1 .. min(16, n_seq), n_ending[i] < 1, n_context - 1 + max(n_ending) >
 * n_ctx, a token id out of range, chunk_tokens < 0, a handle with a live scheduler (its low slots are the scheduler's), HOST_ONLY and stage
 * handles.  Picking the best choice is the caller's: n_choices doubles, and byte-length normalisation needs text the library does not have. */
typedef struct llamahip_score_multi_stats {
    int32_t struct_size;
    int32_t n_rows;            /* sum of n_tokens */
    int32_t n_scored_rows;     /* rows with a target: the rows the lm head ran over */
    int32_t n_passes;          /* 1 = one pass over all rows; the per-slot loop reports its eval count */
    int32_t n_short_segs, n_long_segs;   /* as llamahip_eval_multi_stats (0 on the per-slot loop) */
} llamahip_score_multi_stats;
int llamahip_eval_logprobs_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *slots,
                                 const int32_t *n_past, const int32_t *tokens /* concatenated, n_tokens[i] each */,
                                 const int32_t *n_tokens, int32_t chunk_tokens /* 0 = one eval per segment */,
                                 const int32_t *targets /* [R], -1 = not scored; NULL = the next token inside the segment */,
                                 double *logprob_out /* [R] */, int32_t *argmax_out /* [R] */, int32_t *rank_out /* [R]; any may be NULL */,
                                 llamahip_score_multi_stats *stats /* may be NULL */, char *err, size_t err_cap);
#define LLAMAHIP_SCORE_CHOICES_MAX 16
int llamahip_score_choices(llamahip_model *m, int32_t n_threads, const int32_t *context, int32_t n_context /* >= 1 */,
                           int32_t n_choices /* 1 .. 16, <= n_seq */, const int32_t *endings /* concatenated, n_ending[i] each */,
                           const int32_t *n_ending /* each >= 1 */, int32_t chunk_tokens /* of the context eval; 0 = one eval */,
                           double *logprob_sum /* [n_choices] */, int32_t *n_greedy /* [n_choices], may be NULL */,
                           double *logprob_rows /* concatenated, n_ending[i] each; may be NULL */, char *err, size_t err_cap);

/* ---- text embeddings: pooled final-norm rows, several texts per weight pass --------------------------------------------------------------
 * A text's embedding is the final-norm hidden state the lm head would have read (.mm:695-700: inpL after ggml_norm x model.norm), of the text's
 * last row (LLAMAHIP_POOL_LAST: what llama.cpp's --embedding of the reference's era returns) or the mean over the text's rows
 * (LLAMAHIP_POOL_MEAN).  An embedding pass is the eval of the same arguments with the lm head replaced by three small launches on the last
 * stage's stream (csrc/pool.hip): the final norm stored as plain fp32 rows (k_norm_rows_f32: the norm's arithmetic of every path here, mean and
 * second moment in double in the two-pass form, no fp16 rounding, no permutation), the pooling (k_pool_rows: LAST copies the segment's last
 * row -- only the last rows are gathered and normed; MEAN adds (double) y[j][c] over the segment's rows j in ascending order from 0.0 and
 * stores (float) (acc / (double) n_rows)), and with normalize = 1 the L2 normalisation (k_l2_rows: lane l of 64 sums (double) o[c] * (double) o[c]
 * over c = l, l + 64, ... ascending, the 64 partials are folded by the xor butterfly 32, 16, 8, 4, 2, 1, out[c] = (float) ((double) o[c] /
 * sqrt(ss)); ss == 0.0 leaves the zero vector).  No lm head runs (262 MB of the 7B's 4.1 GB), n_embd floats per text come back instead of
 * n_vocab, and no logits are written: the logits buffer and the row map of llamahip_stage_logits stay as the last eval left them.
 *
 * llamahip_text_embedding -- one text on the current KV slot.  Contract: the call leaves the KV rows [n_past, n_past + n_tokens) of every layer
 * that llamahip_eval_chunks(n_past, tokens, n_tokens, chunk_tokens) (chunk_tokens 0: llamahip_eval) leaves, bit for bit, and touches no other
 * KV row; out = the n_embd floats.  MEAN pools the rows of this call only: rows below n_past are context, not text.  A one-token text is legal
 * (it is evaluated as a one-row multi-row eval, not as a decode step: the decode step's final norm lives inside the lm head's launch).  The
 * norm's sums are folded in the kernel's own order; equality with the reference's sequential sums is BY TEST (tests/test_gpu_pool_op.py,
 * tests/test_gpu_text_embedding.py), on rows whose result no order can change.
 * llamahip_text_embedding_multi -- text i at n_past[i] on KV slot slots[i], all texts in llamahip_eval_multi's ONE pass; out [n_seqs][n_embd].
 * Contract: per text what llamahip_set_seq(slots[i]) + llamahip_text_embedding of its arguments returns, the KV rows llamahip_eval_multi of
 * the same arguments leaves, bit for bit; no other KV row is touched and the current slot is left alone.
 * Handles and fall-backs: llamahip_eval_multi's -- plain and in-process pipeline handles take the one pass under its loop rule; f16 / f32 /
 * Q4_1 files, LLAMAHIP_FLAG_FAST_PREFILL handles, n_seqs == 1 and head sizes the table kernels refuse run llamahip_text_embedding slot by
 * slot, restore the current slot and report the eval count in stats->n_passes (the one pass: 1).
 * Refused before any device work, the message naming the limit and the function, the handle last: what llamahip_eval_multi refuses of the same
 * arguments, pool outside {0, 1}, normalize outside {0, 1}, a null out, HOST_ONLY and stage handles, and a handle with a live scheduler when
 * a named slot (llamahip_text_embedding: the current slot) is below its max_active.
 * llamahip_op_pool_rows -- the three launches on caller-supplied rows x[R][d] (parity tests): also refuses R outside 1 ..
 * LLAMAHIP_EVAL_MULTI_MAX_ROWS, d < 32 or d % 32 != 0, n_segs outside 1 .. 16 and a seg_begin that does not rise strictly from 0 to R.
 * (llamahip_op_embed is the token-embedding GATHER at the bottom of the graph; these are the TEXT's embedding at its top.)
 * Numbers (7B, one MI355X, n_past 64, normalize on, ms per call, median of five fresh processes; tools/embed_probe.py,
 * profiles/embed_probe_7b.json):
 *   segments x rows (MEAN)        4 x 10   16 x 10   16 x 32   4 x 128
 *   one pass                        7.90     20.53     42.92     37.28
 *   llamahip_eval_multi + logits    7.88     20.52     42.96     37.43
 *   per-slot loop                  12.41     49.83    111.80     58.81
 *   LAST measured the same to within the spread.  Against llamahip_eval_multi with logits the difference is inside the spread: its lm head
 *   already runs over the segments' last rows only.  No measured shape is slower than the loop, so the loop rule stays llamahip_eval_multi's.
 *   DESIGN.md 12.28. */
#define LLAMAHIP_POOL_LAST 0
#define LLAMAHIP_POOL_MEAN 1
#define LLAMAHIP_POOL_MAX_SEGS 16
int llamahip_text_embedding(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t n_tokens,
                            int32_t chunk_tokens /* 0 = one eval */, int32_t pool, int32_t normalize, float *out /* n_embd */, char *err, size_t err_cap);
int llamahip_text_embedding_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *slots, const int32_t *n_past,
                                  const int32_t *tokens /* concatenated, n_tokens[i] each */, const int32_t *n_tokens, int32_t chunk_tokens,
                                  int32_t pool, int32_t normalize, float *out /* [n_seqs][n_embd] */,
                                  llamahip_eval_multi_stats *stats /* may be NULL */, char *err, size_t err_cap);
int llamahip_op_pool_rows(const float *x /* [R][d] */, int32_t R, int32_t d, const float *norm_w /* [d] */, const int32_t *seg_begin /* n_segs + 1 */,
                          int32_t n_segs, int32_t pool, int32_t normalize, float *out /* [n_segs][d] */, char *err, size_t err_cap);

/* ---- request scheduler: prompts admitted into a running multi-sequence decode --------------------------------------------------------
 * The *_multi loops above take their slots' contexts as given and run every sequence for the same n_steps; llamahip_eval_multi evaluates
 * several prompts in one pass.  The scheduler is the loop that joins them: requests wait in a queue, take a free KV slot, have their prompt
 * evaluated in the weight pass the other conversations' decode rows pay for anyway, decode, and leave at their stop token or their length.
 * One llamahip_sched_step makes ONE weight pass (one per stage group on a pipeline handle) and returns that step's events: a TOKEN event for
 * every token produced, a DONE event behind a request's last token (or for a cancelled request).
 *
 * Slots.  KV slots [0, max_active) belong to the scheduler while it lives; slots at and above max_active stay the caller's; the handle's
 *   current slot (llamahip_set_seq) is left alone.  At the start of a step queued requests take the free slots, lowest slot first, in
 *   submission order.  A slot freed by a DONE in step t is reused from step t + 1; its previous occupant's KV rows are stale and never read,
 *   because every eval writes its positions before it reads them.
 * The step rule (llamahip_sched_plan; host only, pure, deterministic -- the one place the policy lives).  prompt_left[i]: the prompt tokens
 *   sequence i still has to evaluate, sequences in admission order (oldest first), 0 = decoding.  Every decoding sequence gets one row.
 *   rest = row_budget - (decode rows); the prefilling sequences are walked oldest first: with chunk_tokens = c > 0 a sequence gets
 *   min(prompt_left, floor(max(rest, 0) / c) * c) rows, with c == 0 its whole prompt_left if that fits in rest; where that is less than one
 *   row and no prefilling sequence has been given rows yet in this step it gets min(prompt_left, c) rows (c == 0: the whole prompt) -- the
 *   progress guarantee, the only way a step exceeds the budget -- otherwise the walk stops.  rows_out[i]; returns the total, -1 for bad
 *   arguments (n_active outside 0 .. 16, a negative entry, chunk_tokens < 0, row_budget < 1).  A piece therefore starts at a multiple of c
 *   and ends at a multiple of c or at the prompt's end: its rows' key counts (llamahip_eval_multi_rows with n_past = the piece's offset) are
 *   those of the whole prompt's llamahip_eval_chunks.
 * What a step runs.  Some sequence prefilling: a MIXED PASS -- llamahip_eval_multi's pass over segments, a prefilling sequence's piece at its
 *   offset, a decoding sequence's one row [its last token] at its position; the lm head over the segments' last rows; k_sched_pick (one wave
 *   per segment, behind the lm head on the last stage's stream) takes the greedy pick of every segment that EMITS (a decode row, a piece
 *   that ends its prompt) by k_argmax's rule, stores it in the result block -- 4 bytes per segment come back, no logits row -- publishes it
 *   into the slot's next-token word and trace, and sets the slot's {position, step} words behind the segment's rows, so that the next
 *   captured step continues on the device (the other stages of a pipeline handle are kept in step from the host, as
 *   llamahip_decode_sample_lookup_multi does).  Sampled requests take the candidate selection over their emitting rows instead; the host
 *   draws, accepts and writes the token word, as llamahip_decode_sample_multi does.  Nobody prefilling: a DECODE-ONLY step, exactly the step
 *   llamahip_decode_greedy_multi / llamahip_decode_sample_multi take -- the captured llamahip_stage_step_set over the active slots,
 *   llamahip_stage_step for a single active slot -- with one host wait for the picks per step (stop tokens and streaming need it).
 *   Handles without the one pass or without a set step (f16 / f32 / Q4_1 files, LLAMAHIP_FLAG_UNFUSED and _FAST_PREFILL handles, head sizes
 *   the table kernels do not take, n_threads for which llamahip_stage_set_applies is 0) run the contract's own per-slot calls for every
 *   step (FALL-BACK steps): the same events, the same bits.  (A LLAMAHIP_FLAG_FAST_PREFILL handle makes no parity claim for evals long enough
 *   to take its mat-mul: there a prompt evaluated in the scheduler's pieces need not equal the prompt evaluated whole.)
 * Contract, for every request, whatever else is in flight, in whatever order the requests were submitted, for every row_budget: the tokens,
 *   the KV rows [0, n_prompt + n - 1) of its slot in every layer (n = the tokens produced; read after its DONE and before the slot is
 *   reused) and the sampler's window and rng state are bit for bit those of the request running ALONE on that slot:
 *   llamahip_set_seq(slot) + llamahip_eval_chunks(prompt, 0, chunk_tokens) (llamahip_eval when chunk_tokens == 0), the greedy pick or the
 *   draw from that logits row, then single-token steps (llamahip_decode_greedy, or llamahip_eval_topk -> draw -> accept), the stream cut
 *   behind stop_token or at n_predict.  (Norm statistics: one pass in the fused single step, two in a multi-row pass.  The equality is
 *   therefore BY TEST -- tests/test_gpu_sched.py -- not structural, as for set steps, verify steps and llamahip_eval_multi.)  `exact` of a
 *   TOKEN event is reported as the sampled loops report it (1 for a greedy pick) and is not part of the equality.
 * Refused before any device work, the message naming the limit.  llamahip_sched_new: max_active outside 1 .. 16 or > llamahip_opts.n_seq,
 *   chunk_tokens < 0, row_budget < 0 or > LLAMAHIP_EVAL_MULTI_MAX_ROWS - 16, sampler parameters llamahip_verify_sample refuses, HOST_ONLY and
 *   stage handles, a handle that already has a scheduler.  llamahip_sched_submit: n_prompt < 1, n_predict < 1, a token id (or a stop token other than -1) out of range, n_prompt +
 *   n_predict - 1 > n_ctx, with chunk_tokens == 0 a prompt longer than LLAMAHIP_EVAL_MULTI_MAX_ROWS - max_active, a sampler held by another
 *   live request.  llamahip_sched_step: cap < LLAMAHIP_SCHED_EVENT_CAP (2 * max_active + 1 without drafts; the call consumes nothing).
 * llamahip_sched_cancel: a queued or active request ends with a DONE event of reason CANCELLED in the next step's events (an active one
 *   takes no row in that step; its slot is free from that step on); -1 for an id that is not live.  llamahip_sched_pending: queued + active
 *   + cancelled requests whose DONE has not been delivered.  A step that fails (LLAMAHIP_ERR_PREDICT) delivers no event and loses none: the
 *   waiting DONE events and the requests it admitted are there for the next step.  One scheduler per handle at a time: llamahip_sched_new
 *   refuses a handle that has one until it is freed; a handle freed first leaves a scheduler whose steps fail and whose llamahip_sched_free
 *   is still safe.  Between steps the caller may use the slots at and above max_active with any other entry point.
 * llamahip_op_sched_pick -- the pick half of k_sched_pick on caller-supplied rows (parity tests): logits[n_rows][n_vocab], n_rows 1 .. 16;
 *   picks[r] = the greedy pick of row r where emit[r] != 0, -1 where emit[r] == 0.
 * Measured on the 7B (profiles/sched_probe_7b.json, tools/sched_probe.py): 64 requests, prompts of 9 .. 288 tokens, 8 .. 224
 *   tokens each, 16 slots, chunks of 9: 2321 tokens/s aggregate at row_budget 256 (1523 / 1807 / 1941 / 2116 at 16 / 32 / 64 / 128) against
 *   1124 for static waves of llamahip_eval_multi + llamahip_decode_greedy_multi, which keep stepping finished sequences; the longest step --
 *   the stall a decoding conversation sees while prompts are admitted -- is 24.3 ms at 256 and 7.5 ms at 32.  A set-step capture costs 1.2 ..
 *   1.35 ms and a run makes 8 .. 13 of them.
 * Drafted tokens in the rows a step leaves spare (llamahip_sched_opts.draft_len > 0; off by default).  A step has 16 logits
 *   rows (VERIFY_ROWS_MAX); whenever fewer than 16 segments emit, the rest carry prompt-lookup drafts of the decoding requests.  What a request
 *   WANTS: llamahip_lookup_draft over its prompt + everything it has produced, then the scheduler's corpus, cut to draft_len and to n_predict -
 *   n_out - 1 (a verify step never passes n_predict, hence never n_ctx); 0 for a sampled request whose window exceeds 1024 ids, and for every
 *   sampled request when top_k > 64 or n_vocab > 32768.  What it GETS: llamahip_sched_plan_drafts (host only, pure -- the one place the draft
 *   policy lives).  Sequences in admission order, rows = llamahip_sched_plan's; want[i] must be 0 unless prompt_left[i] == 0.  A segment
 *   emits if it is a decode row or a prompt piece with rows[i] == prompt_left[i]; spare = 16 - (emitting segments), further capped so that
 *   sum(rows) + sum(give) <= LLAMAHIP_EVAL_MULTI_MAX_ROWS; the spare rows go to the decoding sequences by llamahip_lookup_deal_rows' rule (one
 *   draft token at a time, round-robin in admission order).  Returns sum(give), -1 for bad arguments (n_active outside 0 .. 16, a null array,
 *   a negative entry, want outside 0 .. 15 or non-zero on a prefilling sequence, rows[i] != 1 on a decoding one).  Draft rows do not count
 *   against row_budget (it bounds the prompt rows and so the stall; at most 15 draft rows ride on any step).
 *   A step that carries at least one draft row is a MIXED PASS whether or not anybody prefills: a decoding segment is [last token, draft ...]
 *   at the slot's position, every row keyed as its own single-token eval (keys = position + 1, whatever chunk_tokens); the lm head runs over
 *   every row of a draft segment and the last row of every other emitting segment.  Greedy segments: k_verify_rows picks every logits row,
 *   k_sched_accept (one wave per segment) counts n_accept = the largest a <= n_draft with pick[j] == draft[j] for all j < a, publishes the
 *   slot's words and returns 4 (rows + segments) bytes.  Sampled segments (ordered first): the sliding-window candidate selection over their
 *   rows and the host walk of llamahip_verify_sample_multi (draw, accept, continue only while the draw is the draft's next token); after such
 *   a step the host pushes the slots' words.  The request then produces n_accept + 1 TOKEN events in that step, in order, at consecutive
 *   positions, ending at its stop token (accepted tokens behind a stop token are dropped and never reported; the slot's KV rows behind the
 *   reported context are stale and never read) or at n_predict; its DONE follows its last TOKEN.  A step in which nothing is dealt is exactly
 *   the step of a scheduler without drafts and is counted as such.  Fall-back handles draft nothing and report zero drafts.
 *   The contract above holds unchanged: tokens, KV rows [0, n_prompt + n - 1), sampler window and rng state of the request ALONE
 *   (BY TEST: tests/test_gpu_sched_draft.py).
 *   Event capacity: LLAMAHIP_SCHED_EVENT_CAP(max_active, draft_len) -- with draft_len > 0 max_active + 17 (at most 16 logits rows = TOKEN
 *   events per step, one DONE per request, one waiting DONE); 2 * max_active + 1 otherwise, as before.
 *   Stats identity: n_tokens == n_emit_segs + n_accepted - n_dropped (n_emit_segs: emitting segments over all steps; n_accepted: draft tokens
 *   the model reproduced; n_dropped: accepted tokens behind a stop token); n_accepted <= n_drafted.
 *   Refused by llamahip_sched_new before any device work: draft_len outside 0 .. 15, ngram bounds llamahip_lookup_draft refuses (negative,
 *   ngram_max < ngram_min after the defaults), n_corpus < 0 or without a corpus, a corpus token id out of range.
 *   llamahip_op_sched_accept -- k_verify_rows + k_sched_accept on caller-supplied rows (parity tests): logits[n_rows][n_vocab], n_rows 1 .. 16;
 *   seg_tab[n_segs][6] = {emit, slot, base position, base cursor, first logits row, row count}, n_segs 1 .. 16.  emit 0: no logits row (a
 *   prompt piece that does not end its prompt); 1: one logits row, the segment's last of `row count` rows (a piece that ends its prompt, a
 *   plain decode row); 2: every one of its `row count` rows has a logits row ([last token, draft ...]; tokens[r] = the token of logits row r).
 *   The logits rows of the emitting segments tile [0, n_rows) in segment order.  n_accept[s] as above (0 unless emit == 2), picks[r] = the
 *   greedy pick of logits row r.  With slot words (state[n_slots][2], log[n_slots][log_cap], next_tok[n_slots]: all three or none; copied
 *   both ways, what the launch does not write keeps the caller's bits): position = base + rows consumed (n_accept + 1 for emit 2, the row
 *   count otherwise), cursor = base cursor + tokens produced (n_accept + 1, 1, or 0 without a logits row), next-token word = pick[n_accept],
 *   log[slot][base cursor + j] = pick[j] for j <= n_accept (entries at or past log_cap are dropped).
 *   Measured on the 7B (profiles/sched_draft_probe_7b.json, tools/sched_probe.py --draft), the workload above at row_budget 256,
 *   draft_len 15: 2321 tokens/s without drafts; 2508 with a corpus from which every draft is accepted (311 steps for 437: the 16 slots are
 *   busy for most of the run, spare rows exist in its tail only); 2358 with 0.49 of the drafted tokens accepted; 2021 with none of 1578 accepted -- a
 *   decode-only step that carries a draft is a mixed pass, not the captured set step.  Drafting pays from an acceptance rate of 0.44 on this
 *   workload (interpolated); below it, leave draft_len at 0, the default.  draft_len == 0 against the parent commit's library, fresh processes,
 *   interleaved, five each: 2321 against 2324 tokens/s, inside the parent's own spread of 19.
 * Evaluated prompt prefixes shared between KV slots (llamahip_sched_opts.prefix_share = 1; off by default).  Every operator of
 *   an eval works row by row except the V.P key split, which depends on the eval a row belongs to: in a prompt evaluated by
 *   llamahip_eval_chunks with chunk_tokens = c > 0, row j has min(N, (j / c + 1) * c) keys (llamahip_eval_multi_rows).  For two prompts and a
 *   multiple P of c that is no larger than their common prefix and smaller than both lengths, every row j < P has the same tokens [0 .. j],
 *   the same position and the same key count (j / c + 1) * c <= P in both: the K and V rows [0, P) of every layer are the same bits, and a
 *   request that takes them over and evaluates the rest in pieces from offset P (what the step rule does for every later piece anyway) ends
 *   with exactly the rows its own llamahip_eval_chunks from 0 would have written.  A K row carries its position's rotation: a copy keeps the
 *   row index, only the slot changes.  NOT shareable, and never shared: rows written by decode or verify steps (keyed as single-token evals),
 *   anything at chunk_tokens == 0 (every row's key count is its prompt's length), rows of a LLAMAHIP_FLAG_FAST_PREFILL handle (no parity
 *   claim), the new prompt's last token (one row must be evaluated for the first logits).
 *   Held records.  With the option on the scheduler remembers per slot the occupant's prompt and how many of its rows are evaluated prompt
 *   rows (the request's offset; the whole prompt once it decodes).  The record outlives the request's DONE or cancel until the slot's next
 *   occupant replaces it; decode and draft rows lie at and above the prompt's end and never enter it.
 *   The policy (llamahip_sched_plan_prefix; host only, pure -- the one place it lives).  held / n_held[s]: the records, concatenated.
 *   share(s) = floor(min(lcp(prompt, held_s), n_held[s], n_prompt - 1) / c) * c, 0 for c == 0.  The slot: among the free ones the largest
 *   share(s) -- those rows are in place, nothing moves -- ties to the smallest n_held[s] (an empty slot loses nothing), then to the lowest
 *   index (with nothing held anywhere: lowest slot first, as without the option).  The donor: over all OTHER slots, free or active, the largest
 *   share(t), ties to the lowest index; if it exceeds the in-place share, *donor_out = t, rows [*n_inplace_out, share(t)) are to be copied
 *   and share(t) is returned; else *donor_out = -1 and the in-place share is returned.  -1 for bad arguments (n_slots outside 1 .. 16, no
 *   free slot, a null array, a negative entry, n_prompt < 1, chunk_tokens < 0).
 *   Admission, one request at a time in submission order: the plan over the records as they stand; where rows are to be copied, ONE
 *   k_kv_copy_rows launch per stage on the stage's stream; only then the request takes the slot, starts at offset P, and the record is
 *   replaced.  Launches are stream-ordered: a later admission of the same step may share what an earlier one copied, and the step's pass
 *   runs behind them.  A step that fails after admissions keeps them, their slots and their shared rows.  Fall-back handles share too
 *   (their per-slot llamahip_eval_chunks at n_past = offset is what later pieces run anyway); LLAMAHIP_FLAG_FAST_PREFILL handles and
 *   chunk_tokens == 0 share nothing, keep no records, choose slots lowest first and report zeros.  The contract above holds unchanged,
 *   whatever was shared from whatever donor (BY TEST: tests/test_gpu_sched_prefix.py).  Stats: n_shared_rows (prompt rows taken over, in
 *   place or copied), n_copied_rows (of those, moved), n_copy_launches; where every request reaches DONE uncancelled,
 *   n_prompt_rows + n_shared_rows == the sum of the prompts' lengths.  llamahip_sched_new refuses prefix_share other than 0 or 1.
 * llamahip_kv_copy_rows -- the copy for callers who manage slots themselves (evaluate a system prompt once, broadcast it, llamahip_eval_multi
 *   with n_past = P): for each i < n_copies the rows [row_begin[i], row_begin[i] + n_rows[i]) of EVERY layer, K and V, from slot src_slot[i]
 *   to the same rows of slot dst_slot[i]; one source may feed many destinations; n_rows[i] == 0 is a no-op entry.  One k_kv_copy_rows launch
 *   per stage (every stage of a pipeline handle on its own device and stream), waited for; every file type (the cache is the same fp32
 *   array for all).  No row outside the named ranges is touched, nor the handle's current slot.  Refused before any device work, the message
 *   naming the limit, the handle last: a null handle, n_copies outside 1 .. 16, a null array, a slot outside [0, n_seq), src == dst, a
 *   negative count or a range outside [0, n_ctx], a slot that is the destination of one copy and the source or destination of another,
 *   HOST_ONLY and stage handles, and while a scheduler lives on the handle a destination below its max_active.
 *   Measured on the 7B (tools/sched_probe.py --shared-prefix 256; the figures are in profiles/sched_prefix_probe_7b.json and DESIGN.md 12.23): 64 requests
 *   behind one 256-token system prompt run about a third faster with the option on; k_kv_copy_rows is faster than a loop of hipMemcpyAsync calls over
 *   the same ranges for 9 rows, for 256 rows and for a 15-way broadcast; prefix_share 0 is unchanged against the parent commit's library.
 * Constrained requests (llamahip_request.constraint; forced tokens as drafts: llamahip_sched_opts.forced_drafts, off by default; DESIGN.md
 *   12.34).  A greedy request may carry a constraint (llamahip_constraint_*, below) and the automaton state before its first pick
 *   (constraint_state; -1 = the constraint's start): every one of its picks is then k_pick_dfa's rule over the entries its state allows, the
 *   host half advances the state over every token it reports, and the constraint's stop token ends the request (stop_token is -1 or that
 *   token).  The caller keeps the constraint alive until the request's DONE.  The scheduler waits for every step's picks, so the host knows
 *   each request's state before it builds the next step: the kernels take, per logits row and BY VALUE in their arguments, a pointer to the
 *   table row next[state] (null = the row is unconstrained) and a range-checked fallback token -- no device-resident state word.
 *   CONTRACT, the sentence above extended: the tokens of a constrained request, its DONE reason and the KV rows [0, n_prompt + n - 1) of its
 *   slot in every layer are bit for bit those of the request ALONE on that slot -- llamahip_set_seq(slot), llamahip_eval_chunks(prompt, 0,
 *   chunk_tokens), then the loop llamahip_constraint_pick(c, state, logits) -> llamahip_constraint_advance -> one-token llamahip_eval, cut
 *   behind the stop token (reason STOP) or at n_predict (LENGTH) -- whatever else is in flight, for every submission order, row_budget,
 *   draft_len and forced_drafts.  BY TEST (tests/test_gpu_sched_constrain.py), as for every multi-row step.
 *   What a step launches.  No emitting greedy segment constrained: exactly what it launched before.  A mixed pass without drafts:
 *   k_sched_pick_dfa in k_sched_pick's place (same geometry, same stores, dead flags behind the picks in the result block).  A step with
 *   drafts: k_verify_rows_dfa in k_verify_rows' place -- each logits row picked under the state reached by advancing over the draft tokens
 *   in front of it -- and k_sched_accept unchanged behind it.  A decode-only step: the captured set step (the single step for one active
 *   slot) exactly as it is, then ONE k_sched_pick_dfa launch over the step's logits rows with the advanced {position, cursor} in its table; it
 *   overwrites the trace entry and the next-token word the step's own tail wrote, as llamahip_decode_greedy_constrained_multi does with
 *   k_pick_dfa.  (The stage step's tail only stores its pick; nothing reads the token word before the next step's embedding gather, which
 *   runs behind the re-pick on the same stream.  A single active constrained slot therefore keeps the single step.)  A row that allows
 *   nothing -- impossible with a state the constraint handed out -- picks the constraint's stop token and sets its dead word: the step fails
 *   with LLAMAHIP_ERR_PREDICT.  Fall-back handles run the contract's own loop per slot (one-token evals, the host pick) and draft nothing.
 *   Drafts of a constrained request.  With forced_drafts = 1 it wants its FORCED RUN (llamahip_forced_run) from the state behind the
 *   token it is about to evaluate, cut to 15 tokens and to n_predict - n_out - 1: a draft that is accepted by construction, because a forced
 *   token is the only allowed entry of its row and the rule picks it whatever the logits hold -- an answer of ten forced tokens costs one
 *   weight pass instead of ten, and the stream stays the single-token loop's.  Where the forced run is empty and draft_len > 0 it wants its
 *   lookup draft, cut at the first token banned in the running state and behind a drafted stop token.  The spare rows are dealt by
 *   llamahip_sched_plan_drafts, unchanged.  forced_drafts works with draft_len == 0; the event capacity a step then requires is
 *   LLAMAHIP_SCHED_EVENT_CAP(max_active, 1) = max_active + 17, and a smaller cap is refused.
 *   Stats: n_dfa_rows (logits rows picked under a constraint), n_forced_drafted / n_forced_accepted (counted in n_drafted / n_accepted too).
 *   n_forced_accepted == n_forced_drafted always, and n_tokens == n_emit_segs + n_accepted - n_dropped still holds.
 *   Struct sizes: llamahip_sched_submit takes a llamahip_request of the size before these fields (offsetof constraint) or larger and reads
 *   the new fields only where struct_size covers them; llamahip_sched_new reads forced_drafts only where struct_size covers it.
 *   Refused before any device work, the message naming the limit.  llamahip_sched_new: forced_drafts other than 0 or 1.
 *   llamahip_sched_submit: a constraint made on another handle; constraint_state outside [-1, n_states); a stop_token that is neither -1 nor
 *   the constraint's stop token; a sampler together with a constraint; a constrained request on an in-process pipeline handle (the table's
 *   device copy belongs to one device).
 *   llamahip_op_verify_rows_allow / llamahip_op_sched_pick_allow -- the two kernels on caller-supplied rows (parity tests): logits[n_rows][n_vocab],
 *   n_rows 1 .. 16, ONE table[n_table_states][n_vocab], states[n_rows] (-1 = unconstrained), fallback[n_rows]; picks / dead [n_rows] out.
 *   sched_pick_dfa also takes emit[n_rows] as llamahip_op_sched_pick does (picks -1 and dead 0 where emit == 0) and, optionally, slot words:
 *   seg_words[n_rows][3] = {slot, position, cursor} with state[n_slots][2], log[n_slots][log_cap], next_tok[n_slots] -- all four or none,
 *   copied both ways.  Refused before any launch: a NULL array, n_rows outside 1 .. 16, n_vocab < 1, n_table_states outside 1 .. 65535, a
 *   table entry that is neither a state nor BANNED, a state outside [-1, n_table_states), a fallback token out of range.
 *   Measured: not measured yet (tools/sched_probe.py --constrained).
 * Not built: sampled constrained requests; constrained requests on pipeline handles; forced rows without an lm head (a forced token's row
 *   still runs the lm head and the pick: the verify step is what keeps the stream the single-token loop's); the scheduler behind
 *   llama_runner; more than 16 active sequences; a set-step-descriptor form for
 *   decode-only drafted steps; drafts counted against row_budget; sharing decode rows or rows at chunk_tokens == 0; a prefix store beyond
 *   the slots' own records;
 *   generating past n_ctx (llamahip_decode_greedy_window's overflow plan); the mixed pass on the fused few-row launches. */
#define LLAMAHIP_SCHED_ROW_BUDGET 256     /* the candidate of 16 .. 256 with the highest median tokens/s on the probe workload: profiles/sched_probe_7b.json, DESIGN.md 12.19 */
#define LLAMAHIP_EV_TOKEN 1
#define LLAMAHIP_EV_DONE  2
#define LLAMAHIP_DONE_LENGTH    1
#define LLAMAHIP_DONE_STOP      2
#define LLAMAHIP_DONE_CANCELLED 3
typedef struct llamahip_sched llamahip_sched;
typedef struct llamahip_sched_opts {
    int32_t struct_size;
    int32_t n_threads;
    int32_t max_active;      /* KV slots [0, max_active) belong to the scheduler; 1 .. 16 and <= llamahip_opts.n_seq */
    int32_t chunk_tokens;    /* the contract's prompt chunking, as llamahip_eval_chunks; 0 = a prompt is one eval and is never split */
    int32_t row_budget;      /* rows a step aims at; 0 = LLAMAHIP_SCHED_ROW_BUDGET */
    double  repeat_penalty, top_p, temp;      /* for requests that carry a sampler; all three 0 with top_k 0: 1.3, 0.95f, 0.8f and top_k 40 */
    int32_t top_k;
    /* drafted tokens (read only where struct_size covers them; a shorter struct means no drafting) */
    int32_t draft_len;       /* 0 = off; 1 .. 15 draft tokens per request and step at the most */
    int32_t ngram_min, ngram_max;              /* llamahip_lookup_draft's; 0 = LLAMAHIP_LOOKUP_NGRAM_MIN / _MAX */
    const int32_t *corpus; int32_t n_corpus;   /* optional, searched behind a request's own history; copied at llamahip_sched_new */
    /* shared prompt prefixes (read only where struct_size covers it; a shorter struct means off) */
    int32_t prefix_share;    /* 0 = off; 1 = a request takes over the evaluated prompt rows it has in common with a slot's record */
    /* forced tokens as drafts (read only where struct_size covers it; a shorter struct means off) */
    int32_t forced_drafts;   /* 0 = off; 1 = a constrained greedy request's forced run rides as its draft (works with draft_len == 0) */
} llamahip_sched_opts;
#define LLAMAHIP_SCHED_EVENT_CAP(max_active, draft_len) ((draft_len) > 0 ? (max_active) + 17 : 2 * (max_active) + 1)   /* the smallest cap llamahip_sched_step takes */
typedef struct llamahip_request {
    int32_t struct_size;
    const int32_t *prompt; int32_t n_prompt;   /* >= 1; copied at submit */
    int32_t n_predict;                         /* >= 1 tokens to produce */
    int32_t stop_token;                        /* -1 = none; the request ends after producing it */
    llamahip_sampler *sampler;                 /* NULL = greedy; else drawn from and accepted into, as llamahip_decode_sample_multi */
    /* constrained requests (read only where struct_size covers them; the struct up to `sampler` is still taken) */
    struct llamahip_constraint *constraint;    /* NULL = none; the caller's, alive until the request's DONE; greedy requests only */
    int32_t constraint_state;                  /* the automaton's state before the first pick; -1 = the constraint's start */
} llamahip_request;
typedef struct llamahip_sched_event {
    int64_t id; int32_t kind;                  /* LLAMAHIP_EV_TOKEN / LLAMAHIP_EV_DONE */
    int32_t token, exact, slot, position, reason;   /* TOKEN: the token, its exact flag, the position it will be evaluated at; DONE: reason
                                                       LLAMAHIP_DONE_*, position = the context the slot holds (KV rows [0, position)); slot -1: never admitted */
} llamahip_sched_event;
typedef struct llamahip_sched_stats {
    int32_t struct_size;
    int32_t n_graph_captures;                  /* set-step graphs captured while the scheduler stepped */
    int64_t n_steps, n_mixed_steps, n_set_steps, n_single_steps, n_fallback_steps;   /* steps that made a pass, by kind */
    int64_t n_rows, n_prompt_rows, n_tokens;   /* rows evaluated, of those prompt rows, tokens produced */
    int64_t n_submitted, n_done;
    int64_t n_draft_steps;                     /* steps that carried at least one draft row */
    int64_t n_drafted, n_accepted;             /* draft tokens evaluated; of those, reproduced by the model */
    int64_t n_emit_segs, n_dropped;            /* emitting segments over all steps; accepted tokens dropped behind a stop token */
    int64_t n_shared_rows, n_copied_rows;      /* prompt rows taken over instead of evaluated (in place or copied); of those, moved */
    int64_t n_copy_launches;                   /* k_kv_copy_rows launches (one per stage and copy) */
    int64_t n_dfa_rows;                        /* logits rows picked under a constraint */
    int64_t n_forced_drafted, n_forced_accepted;   /* of n_drafted / n_accepted, the forced tokens of constrained requests: always equal */
} llamahip_sched_stats;
int     llamahip_sched_new   (llamahip_model *m, const llamahip_sched_opts *o, llamahip_sched **out, char *err, size_t err_cap);
int     llamahip_sched_submit(llamahip_sched *s, const llamahip_request *r, int64_t *id, char *err, size_t err_cap);
int     llamahip_sched_step  (llamahip_sched *s, llamahip_sched_event *ev, int32_t cap, int32_t *n_ev, char *err, size_t err_cap);
int     llamahip_sched_cancel(llamahip_sched *s, int64_t id);
int32_t llamahip_sched_pending(const llamahip_sched *s);
int     llamahip_sched_get_stats(const llamahip_sched *s, llamahip_sched_stats *out);
void    llamahip_sched_free  (llamahip_sched *s);
int32_t llamahip_sched_plan(int32_t n_active, const int32_t *prompt_left /* admission order, 0 = decoding */,
                            int32_t chunk_tokens, int32_t row_budget, int32_t *rows_out);
int llamahip_op_sched_pick(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *emit, int32_t *picks, char *err, size_t err_cap);
int32_t llamahip_sched_plan_drafts(int32_t n_active, const int32_t *prompt_left, const int32_t *rows /* llamahip_sched_plan's */,
                                   const int32_t *want, int32_t *give);
int llamahip_op_verify_rows_allow(const float *logits, int32_t n_rows, int32_t n_vocab, const uint16_t *table, int32_t n_table_states,
                                const int32_t *states /* -1 = unconstrained */, const int32_t *fallback, int32_t *picks, int32_t *dead,
                                char *err, size_t err_cap);
int llamahip_op_sched_pick_allow(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *emit, const uint16_t *table,
                               int32_t n_table_states, const int32_t *states /* -1 = unconstrained */, const int32_t *fallback,
                               const int32_t *seg_words /* [n_rows][3] = {slot, position, cursor}; with the slot words or NULL */,
                               int32_t n_slots, int32_t log_cap, int32_t *state, int32_t *log, int32_t *next_tok,
                               int32_t *picks, int32_t *dead, char *err, size_t err_cap);
int llamahip_op_sched_accept(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *seg_tab, int32_t n_segs, const int32_t *tokens,
                             int32_t n_slots, int32_t log_cap, int32_t *state, int32_t *log, int32_t *next_tok,
                             int32_t *n_accept, int32_t *picks, char *err, size_t err_cap);
int32_t llamahip_sched_plan_prefix(int32_t n_slots, const int32_t *slot_free, const int32_t *held /* concatenated */,
                                   const int32_t *n_held, const int32_t *prompt, int32_t n_prompt, int32_t chunk_tokens,
                                   int32_t *slot_out, int32_t *donor_out, int32_t *n_inplace_out);
#define LLAMAHIP_KV_COPY_MAX 16           /* copies in one llamahip_kv_copy_rows call */
int llamahip_kv_copy_rows(llamahip_model *m, int32_t n_copies, const int32_t *src_slot, const int32_t *dst_slot,
                          const int32_t *row_begin, const int32_t *n_rows, char *err, size_t err_cap);

/* ---- the n most probable next tokens of a row; beam search over KV slots ------ */
/* llamahip_eval_top_logprobs: llamahip_eval_logprobs' pass (its all-rows lm head, its handles and file types, its refusals) with k_row_topn
 * (topn.hip) behind it: per row i, ids_out[i][0 .. n_top) = the row's entries by value descending, the LOWER index first on equal values
 * (+0.0 == -0.0; ids_out[i][0] is the greedy pick), and logprob_out[i][j] = log softmax(logits_i)[ids_out[i][j]] in double -- bit for bit what
 * llamahip_eval_logprobs reports for that target.  A row holding a NaN or a +inf: every id -1, every logprob NaN; -inf entries are ordinary
 * and come last, in index order.  n_tokens * n_top * 12 bytes come back.  1 <= n_top <= 64 (LLAMAHIP_TOPN_MAX) and <= n_vocab.  KV cache and
 * logits_last (may be NULL) are bit for bit llamahip_eval / llamahip_eval_chunks' (chunk_tokens 0 = one eval). */
#define LLAMAHIP_TOPN_MAX 64
int llamahip_eval_top_logprobs(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t n_tokens, int32_t chunk_tokens,
                               int32_t n_top, int32_t *ids_out, double *logprob_out, float *logits_last, char *err, size_t err_cap);
/* ... its device half on caller-supplied rows logits[n_rows][n_vocab] (parity tests): ids_out / logprob_out [n_rows][n_top].  A row's result
 * depends on its bits, n_vocab and n_top only.  Refused before any launch: a NULL array, n_rows < 1, n_vocab < 1, n_top outside 1 .. 64, n_top > n_vocab. */
int llamahip_op_top_logprobs(const float *logits, int32_t n_rows, int32_t n_vocab, int32_t n_top, int32_t *ids_out, double *logprob_out,
                             char *err, size_t err_cap);

/* llamahip_beam_search: the n_beams best continuations of one prompt, searched over KV slots [0, n_beams).
 * SETUP.  The prompt is evaluated at position 0 on slot 0 by llamahip_eval (chunk_tokens 0) / llamahip_eval_chunks(chunk_tokens).  A live
 *   beam is (tokens, S, slot, row): the tokens produced so far, their summed score, the KV slot that holds their rows, and the logits row its
 *   next token is chosen from.  S is a double, S_L = S_{L-1} + lp_L, added in generation order.  The initial live list is one empty beam with
 *   S = 0 on the prompt's last row.
 * ONE STEP (llamahip_beam_select).  Beam i of the live list, in list order, offers the 2 * n_beams entries (id v, logprob) of k_row_topn on
 *   its row (llamahip_op_top_logprobs with n_top = 2 * n_beams): candidates (i, v, c = S_i + logprob).  A beam whose row is non-finite (ids -1)
 *   offers nothing -- it dies.  A candidate with a NaN c is dropped.  The candidates are ordered by c descending, then i ascending, then v
 *   ascending, and walked in that order until n_beams live successors are collected or the candidates run out: a candidate with
 *   v == stop_token (stop_token >= 0) goes to the finished list -- tokens = beam i's + v, score c, reason LLAMAHIP_DONE_STOP, in walk order --
 *   every other candidate becomes the next live beam of that rank: tokens = beam i's + v, S = c.
 * ENDING.  The step that gives the beams their n_predict-th token ends the search: its live beams join the finished list in rank order
 *   (reason LLAMAHIP_DONE_LENGTH) and their last token is not evaluated.  Otherwise: the search ends when no live beam is left; and, only
 *   with length_norm == 0 and stop_token >= 0, when behind a step's walk the finished list holds at least n_return entries and the
 *   n_return-th best finished score is >= the best live S (scores only fall: logprob <= 0 by construction) -- the live beams are dropped.
 *   Else every new live beam's last token is evaluated as a single-token step of its slot at position n_prompt + length - 1.
 * SLOTS (llamahip_beam_slots).  In rank order the first child of a parent keeps the parent's slot; every further child takes the lowest slot
 *   of [0, n_beams) that no beam kept and not yet taken, and receives the rows [0, rows the parent holds) of the parent's slot (k_kv_copy_rows:
 *   one launch per stage and step, stream-ordered in front of the step, not waited for; sources are never destinations).
 * RESULT.  The finished hypotheses ranked by S (length_norm 0) or S / length as one IEEE double division (length_norm 1), descending, ties
 *   to the earlier entry of the finished list; the first n_return (0 = n_beams) are returned, fewer if fewer finished: *n_hyps_out of them,
 *   hyps_out[k] = {length (a stop token counts), reason, slot, score = S}, tokens_out[k][0 .. length) of rows n_predict apart, -1 behind.
 *   slot: for a LENGTH hypothesis the slot whose KV rows [0, n_prompt + length - 1) are that hypothesis' rows (no copy is made for the last
 *   step, so several hypotheses may name one slot); -1 for a STOP hypothesis.  The other rows of slots [0, n_beams) are unspecified, and so
 *   is every slot's content after an early end; slots from n_beams on and the handle's current slot are untouched.
 * BITS.  Every live beam's logits row is bit for bit the row of llamahip_eval_chunks(prompt) followed by single-token llamahip_evals of the
 *   beam's tokens on a slot of its own -- BY TEST (tests/test_gpu_beam_search.py), as for every set step: the norm's one-pass against
 *   two-pass statistics.  So the result is what tests/beam_ref.py, this contract in plain Python, computes from such rows.
 * DEVICE LOOP.  llamahip_decode_sample_multi's: the slots bound with host-written token words, one set step over the live slots
 *   (llamahip_stage_step_set: the weights streamed once for all beams) with k_row_topn over the step's rows behind it, writing 2 * n_beams x
 *   12 bytes per beam into pinned memory; one wait per step; select, slots, the copies, the token words.  Positions advance on the device (a
 *   slot that sat out a step is re-bound at its position).  Plain and in-process pipeline handles; Q4_0 and f16 / f32 whole-model handles.
 *   Handles without set steps (Q4_1 files, LLAMAHIP_FLAG_UNFUSED, f16 / f32 pipeline stages) run one llamahip_eval per live beam on its slot
 *   with the same kernel over its device row -- the same bits -- counted in stats->n_fallback_steps.
 * Refused before any device work, the message naming the limit, the handle last: NULL arguments, n_beams outside 1 .. 16, above
 *   llamahip_opts.n_seq or with 2 * n_beams > n_vocab, n_prompt < 1, n_predict < 1, n_prompt + n_predict > n_ctx, a token id or a stop token
 *   out of range, n_return outside 0 .. n_beams, chunk_tokens < 0, length_norm other than 0 or 1; HOST_ONLY and stage handles, a live
 *   scheduler on the handle.
 * llamahip_beam_select -- live_score[n_live], cand_ids / cand_logprob [n_live][n_cand] (n_cand <= 32; the search passes 2 * n_beams);
 *   out: new_parent / new_token / new_score [n_beams] and *n_new, fin_parent / fin_score [n_live] and *n_fin (the finished entries of the
 *   walk: beam fin_parent's tokens + stop_token), *n_dead (may be NULL) = live beams on a non-finite row.  0, or LLAMAHIP_ERR_PREDICT for
 *   counts out of range or NULL arrays.
 * llamahip_beam_slots -- prev_slot[n_prev] (distinct, in [0, n_beams)), parent[n_new] (indices into prev); out: new_slot[n_new], copy_src /
 *   copy_dst [n_new].  Returns the number of copies, -1 for arguments it refuses.
 * Not built: more than 16 beams; diverse or sampled beams; beams inside the scheduler; sharing the prompt rows between beams instead of
 *   copying them. */
#define LLAMAHIP_BEAM_MAX 16
typedef struct llamahip_beam_opts {
    int32_t struct_size;
    int32_t n_threads;
    int32_t n_beams;         /* 1 .. 16, <= llamahip_opts.n_seq, 2 * n_beams <= n_vocab */
    int32_t n_predict;       /* >= 1 tokens per hypothesis at the most */
    int32_t stop_token;      /* -1 = none */
    int32_t n_return;        /* 1 .. n_beams; 0 = n_beams */
    int32_t length_norm;     /* 0 / 1 */
    int32_t chunk_tokens;    /* the prompt's chunking, as llamahip_eval_chunks; 0 = one eval */
} llamahip_beam_opts;
typedef struct llamahip_beam_hyp { int32_t length, reason /* LLAMAHIP_DONE_STOP / _LENGTH */, slot, reserved; double score; } llamahip_beam_hyp;
typedef struct llamahip_beam_stats {
    int32_t struct_size, reserved;
    int64_t n_steps;             /* steps that evaluated the live beams' tokens */
    int64_t n_rows;              /* rows those steps evaluated: the sum of their live beams */
    int64_t n_set_steps;         /* of the steps, those on the slots' stage steps (one set step, or one stage step for a single beam) */
    int64_t n_fallback_steps;    /* single llamahip_evals on handles without set steps */
    int64_t n_copy_launches;     /* k_kv_copy_rows launches (one per stage and step that forked a beam) */
    int64_t n_copied_rows;       /* KV rows (per layer, K and V counted once) those copies moved */
    int64_t n_stop;              /* hypotheses finished by the stop token */
    int64_t n_dead;              /* beams that died on a non-finite row */
} llamahip_beam_stats;
int llamahip_beam_search(llamahip_model *m, const llamahip_beam_opts *opts, const int32_t *prompt, int32_t n_prompt, llamahip_beam_hyp *hyps_out,
                         int32_t *tokens_out, int32_t *n_hyps_out, llamahip_beam_stats *stats /* may be NULL */, char *err, size_t err_cap);
int32_t llamahip_beam_select(int32_t n_live, const double *live_score, int32_t n_cand, const int32_t *cand_ids, const double *cand_logprob,
                             int32_t n_beams, int32_t stop_token, int32_t *new_parent, int32_t *new_token, double *new_score, int32_t *n_new,
                             int32_t *fin_parent, double *fin_score, int32_t *n_fin, int32_t *n_dead);
int32_t llamahip_beam_slots(int32_t n_prev, const int32_t *prev_slot, int32_t n_new, const int32_t *parent, int32_t n_beams,
                            int32_t *new_slot, int32_t *copy_src, int32_t *copy_dst);

/* ---- constrained decoding: token-level DFA masks applied on the device ------ */
/* A constraint is a deterministic automaton over BYTES, lifted once on the host to an automaton over the model's tokens: the table
 * uint16 next[n_states + 1][n_vocab], LLAMAHIP_CONSTRAINT_BANNED = the token is not allowed in that state.  A static allow-list is the
 * one-state case.
 * llamahip_constraint_new -- trans[n_states][256] (the next byte-state, -1 = dead), accept[n_states] (0 / 1), start, stop_token (required).
 *   THE LIFT.  Token t with text bytes b0 .. bk leads from state s to the state the walk of trans over those bytes reaches, and is BANNED
 *   where the walk dies.  A token with an empty text is BANNED in every state (it adds no bytes: a pick could loop in place).  stop_token is
 *   allowed exactly in accepting states, whatever its text, and leads to the extra sink state DONE (index n_states), in which only
 *   stop_token is allowed, looping on itself.
 *   THE PRUNE.  A state is live if it is accepting or some token leads from it to a live state (the least fixed point over the token graph);
 *   a transition into a state that is not live becomes BANNED; a start state that is not live is refused.  CONSEQUENCE: every state
 *   reachable from start has at least one allowed token -- an accepting state has stop_token, every other live state a token towards a
 *   live state -- so a row with nothing allowed cannot occur with a state this constraint handed out.  A byte-state that only bytes no
 *   token supplies would reach is never entered.  Any segmentation of an accepted string into tokens is admitted.
 *   Works on any handle, LLAMAHIP_FLAG_HOST_ONLY included: only the vocabulary is read.  The device copy of the table is made by the first
 *   device call that uses the constraint on its handle and belongs to the handle's owner (llamahip_debug_live_allocs counts it);
 *   llamahip_constraint_free releases it.  Free a constraint before its handle; one that outlives its handle may only be freed.
 *   Refused before any work, the message naming the limit: NULL arguments, n_states outside 1 .. 4096, a table over 256 MiB, a trans entry
 *   outside [-1, n_states), start or stop_token out of range, no accepting state; then a start state that is not live.
 * llamahip_constraint_new_choices -- "answer with one of these strings": the trie of n >= 1 non-empty byte strings as the byte automaton,
 *   accepting at each string's end, start = the root, through the same path (duplicates are fine; so is a string that is a prefix of another).
 * llamahip_constraint_n_states (DONE included), _start, _done (the sink's index); _table(c, out, cap): the whole table, n_states * n_vocab
 *   entries -- returns that count, copies where cap holds it; _advance(c, state, token): the next state, -1 if banned or out of range.
 * llamahip_constraint_pick(c, state, logits) -- THE PICK RULE, the host statement of k_pick_dfa (constrain.hip): k_argmax's rule over the
 *   allowed entries of next[state] -- the largest value, the lowest index on ties (+0.0 == -0.0), a NaN never wins; where every allowed entry
 *   is a NaN, the lowest allowed index.  -1 for a row with nothing allowed or a state out of range.
 * llamahip_constraint_mask_row(c, state, in, out) -- the host statement of k_mask_rows_dfa: banned entries become -INFINITY, all others are
 *   copied bit for bit (in == out is fine).
 * EXACT BY CONSTRUCTION: the lift and the prune (integers), the mask, the pick rule against its host statement (a total order on the
 *   non-NaN entries: every reduction tree gives the same pick) -- tests/test_constrain_host.py, tests/test_gpu_constrain_op.py.
 * EXACT BY TEST: the equality of the device loop below with one-token evals (tests/test_gpu_constrain.py) -- the norm's one-pass against
 *   two-pass statistics, as for every captured step.
 *
 * llamahip_decode_greedy_constrained -- llamahip_decode_greedy's un-folded step (forward + a pick kernel behind the lm head) with k_pick_dfa
 *   in k_argmax's place: the automaton's state is one more device-resident word, read and advanced by the pick like the position, so the
 *   step stays captured (a graph-key bit and cache of its own: llamahip_decode_greedy's graphs are neither shared nor disturbed); eager on
 *   LLAMAHIP_FLAG_NO_GRAPH / unfused handles.  *state_io comes in as the state before the first pick (llamahip_constraint_start for a fresh
 *   answer) and goes out as the state behind the last reported token, so a caller resumes with it.  The loop runs in legs of
 *   LLAMAHIP_CONSTRAIN_LEG steps; after each leg it reads {state, dead} (8 bytes) and stops once the state is DONE.  *n_out counts the
 *   tokens up to and including the stop token, *finished is 1 if the stop token was produced.
 *   CONTRACT, bit for bit -- out_tokens[0 .. *n_out), logits_last (the logits the last reported token was picked from; may be NULL), KV rows
 *   [0, n_past + *n_out) of the current slot: the loop "one-token llamahip_eval -> llamahip_constraint_pick -> llamahip_constraint_advance"
 *   on that slot.  Rows at and above n_past + *n_out are unspecified (a leg may run past the stop token).  BY TEST, see above.  With a
 *   constraint that allows everything the tokens are llamahip_decode_greedy's.
 *   SAFETY.  A pick becomes an embedding read on the next step: where the state word is out of range or its row allows nothing, the kernel
 *   indexes nothing, picks stop_token, leaves the state and sets a `dead` word; the loop then fails with LLAMAHIP_ERR_PREDICT.
 *   Handles: plain handles, every file type and flag.  In-process pipeline handles run the reference loop itself (llamahip_eval, the host
 *   pick).  Stage and HOST_ONLY handles are refused.  The arguments are checked first, without a device: NULL arguments, a constraint of
 *   another handle, a state out of range, first_token out of range, n_steps < 1, n_past + n_steps > n_ctx.
 * llamahip_op_pick_dfa / llamahip_op_mask_rows_dfa -- the two kernels on caller-supplied operands (parity tests): logits[n_rows][n_vocab],
 *   n_rows 1 .. 16, ONE table[n_table_states][n_vocab] with per-row states.  pick: states_io / picks / dead [n_rows] go up as they are and come
 *   back -- a row whose state is out of range or allows nothing gets fallback_token, dead = 1 and keeps its state; every other row its pick,
 *   its next state and its dead word untouched.  mask: out[n_rows][n_vocab]; states out of range are refused.  Refused before any launch: NULL
 *   arrays, n_rows outside 1 .. 16, n_vocab < 1, n_table_states outside 1 .. 65535, a table entry that is neither a state nor BANNED, a
 *   fallback_token out of range.
 * llamahip_decode_greedy_constrained_multi -- sequence i lives in KV slot i, as in llamahip_decode_greedy_multi; 1 .. 16 sequences, one weight
 *   pass per step for all of them, each under its own constraint (constraints[n_seqs]), start state (states_io[n_seqs], in / out) and position.
 *   The captured set step stays exactly as it is; ONE k_pick_dfa launch over the set's rows stands behind it and re-picks from the step's logits:
 *   it overwrites what the step's own tail wrote for that step -- the trace entry and the slot's next-token word -- and leaves the position as
 *   advanced.  llamahip_decode_greedy_multi and llamahip_stage_step_set are untouched.  A finished sequence stays in the set in DONE; the loop
 *   ends when all are finished or after n_steps, checked once per leg.  out_tokens[n_seqs][n_steps], n_out / finished [n_seqs] as above.
 *   CONTRACT: per sequence, bit for bit the single-sequence call on that slot alone, KV rows [0, n_past[i] + n_out[i]) included -- BY TEST.
 *   Pipeline handles and handles without a set step to batch (Q4_1 files, LLAMAHIP_FLAG_UNFUSED) run the single-sequence call per slot.
 *   Refused before any device work: NULL arguments, n_seqs outside 1 .. 16 or above llamahip_opts.n_seq, and per sequence what the
 *   single-sequence call refuses.
 * llamahip_eval_topk_constrained -- llamahip_eval_topk's arguments and results plus (c, state): the eval, then k_mask_rows_dfa from the logits
 *   row into a scratch row, then the existing candidate selection on that row.  Everything llamahip_eval_topk promises holds for the MASKED
 *   row: exact == 1 candidates are the reference sampler's on the masked row (llamahip_constraint_mask_row, then
 *   llamahip_sample_top_p_top_k); with exact == 0 logits_out holds the masked row and the caller samples on the host.  Ties among -inf at the
 *   k-th place report exact = 0: that is EVERY step on which fewer than top_k + 1 tokens are allowed.  Pipeline handles (and what else
 *   llamahip_eval_topk hands to the host) mask on the host.  There is no C loop: Model.decode_sample_constrained (binding.py) runs
 *   "eval_topk_constrained -> draw -> accept -> advance".
 * LLAMAHIP_CONSTRAIN_LEG in the ENVIRONMENT (1 .. 64, read once per process, like LLAMAHIP_NO_PICK_FOLD) overrides the macro below: a
 *   measurement switch for tools/constrain_probe.py's leg sweep, not an interface; results do not depend on it.
 * HAZARD: a constraint keeps a pointer to its handle.  After llamahip_model_free the constraint may only be passed to llamahip_constraint_free;
 *   the "made on another handle" check compares that pointer and cannot tell a freed handle from a new one at the same address.
 * llamahip_forced_run(c, state, out, cap) -- THE FORCED RUN of a state: while fewer than cap tokens are out, the state is not DONE and
 *   allows exactly ONE token, that token, and on to next[state][token].  An accepting state whose only allowed token is the stop token yields
 *   the stop token, enters DONE, and the run ends there; DONE itself yields nothing.  Returns the count; -1 for a null constraint, a state out
 *   of range or cap < 0 (out may be NULL when cap == 0).  The per-state "single allowed token or none" is computed once at the lift, in the
 *   prune's walk over the table: a call costs O(run).  What such a state's pick will be is known before the model runs -- the request
 *   scheduler drafts these tokens (llamahip_sched_opts.forced_drafts, "constrained requests" in the scheduler's section above).
 * Not built: constraints in the runner, beam search and the drafted loops (llamahip_decode_greedy_lookup*); sampled constrained requests in the
 *   scheduler; context-free grammars; canonical tokenisation. */
#define LLAMAHIP_CONSTRAINT_BANNED 0xFFFF
#define LLAMAHIP_CONSTRAIN_LEG 4          /* steps between two looks at the state word (measured: DESIGN.md 12.33, profiles/constrain_probe_7b.json) */
typedef struct llamahip_constraint llamahip_constraint;
int llamahip_constraint_new(const llamahip_model *m, int32_t n_states, const int32_t *trans, const uint8_t *accept, int32_t start, int32_t stop_token,
                            llamahip_constraint **out, char *err, size_t err_cap);
int llamahip_constraint_new_choices(const llamahip_model *m, const uint8_t *const *strings, const int32_t *lens, int32_t n, int32_t stop_token,
                                    llamahip_constraint **out, char *err, size_t err_cap);
void llamahip_constraint_free(llamahip_constraint *c);
int32_t llamahip_constraint_n_states(const llamahip_constraint *c);
int32_t llamahip_constraint_start(const llamahip_constraint *c);
int32_t llamahip_constraint_done(const llamahip_constraint *c);
int64_t llamahip_constraint_table(const llamahip_constraint *c, uint16_t *out, int64_t cap);
int32_t llamahip_constraint_advance(const llamahip_constraint *c, int32_t state, int32_t token);
int32_t llamahip_constraint_pick(const llamahip_constraint *c, int32_t state, const float *logits);
int32_t llamahip_forced_run(const llamahip_constraint *c, int32_t state, int32_t *out, int32_t cap);
int llamahip_constraint_mask_row(const llamahip_constraint *c, int32_t state, const float *logits_in, float *logits_out);
int llamahip_decode_greedy_constrained(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token, int32_t n_steps, llamahip_constraint *c,
                                       int32_t *state_io, int32_t *out_tokens, int32_t *n_out, int32_t *finished, float *logits_last,
                                       char *err, size_t err_cap);
int llamahip_decode_greedy_constrained_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens,
                                             int32_t n_steps, llamahip_constraint *const *constraints, int32_t *states_io, int32_t *out_tokens,
                                             int32_t *n_out, int32_t *finished, char *err, size_t err_cap);
int llamahip_eval_topk_constrained(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t n_tokens,
                                   const int32_t *last_n_tokens, int32_t n_last, double repeat_penalty, int32_t top_k, double temp,
                                   llamahip_constraint *c, int32_t state, double *cand_scores, int32_t *cand_ids, int32_t *exact, float *logits_out,
                                   char *err, size_t err_cap);
int llamahip_op_pick_dfa(const float *logits, int32_t n_rows, int32_t n_vocab, const uint16_t *table, int32_t n_table_states, int32_t *states_io,
                         int32_t fallback_token, int32_t *picks, int32_t *dead, char *err, size_t err_cap);
int llamahip_op_mask_rows_dfa(const float *logits, int32_t n_rows, int32_t n_vocab, const uint16_t *table, int32_t n_table_states, const int32_t *states,
                              float *out, char *err, size_t err_cap);

/* llamahip_eval + every token's logits (n_tokens * n_vocab) and, for dump_layer >= 0, that layer's
 * 17 intermediates in the order documented in DESIGN.md ("debug dump order").  Parity tooling. */
int llamahip_eval_debug(llamahip_model *m, int32_t n_threads, int32_t n_past,
                        const int32_t *tokens, int32_t n_tokens, float *logits_last, float *logits_all,
                        int32_t dump_layer, float *dump, int64_t dump_cap, int64_t *dump_sizes,
                        char *err, size_t err_cap);

/* Pipeline-stage evaluation for layer-sharded models (handle loaded with layer_begin/layer_end).
 * hidden_in / hidden_out are DEVICE pointers to n_tokens * n_embd fp32 (the residual stream that
 * crosses layers, .mm:563-564, 687-690).  The first stage ignores hidden_in and embeds `tokens`;
 * the last stage also writes logits (host pointer, may be NULL) . */
int llamahip_eval_stage(llamahip_model *m, int32_t n_threads, int32_t n_past,
                        const int32_t *tokens, int32_t n_tokens,
                        const void *hidden_in, void *hidden_out, float *logits_out,
                        char *err, size_t err_cap);

/* Asynchronous, stream-ordered single-token stage steps: the decode loop of the layer pipeline
 *  with no host round trip per token.
 *
 * llamahip_stage_bind fixes, for sequence slot `seq`, the context position of the next token and the
 * caller-owned DEVICE buffers the step reads and writes:
 *   token_in   int32[1]        the token to evaluate            (first stage; NULL elsewhere)
 *   hidden_in  fp32[n_embd]    residual stream from the previous stage (NULL on the first stage)
 *   hidden_out fp32[n_embd]    residual stream for the next stage      (NULL on the last stage)
 *   token_out  int32[1]        greedy pick (argmax, lowest index on ties) of the last stage; may be
 *                              NULL, and may alias token_in on a whole-model handle
 * token_in is checked at bind: an address that is not device-accessible memory is refused there (the step's first kernel reads it; with
 * tokens on the host use llamahip_eval_stage).  Handles: every Q4_0 handle shape; f16 / f32 whole-model handles (the un-fused dense step,
 * captured the same way); not Q4_1 files, LLAMAHIP_FLAG_UNFUSED handles or layer-range f16 / f32 handles.
 * llamahip_stage_step enqueues one token step for that slot on `stream` (a hipStream_t; NULL = the
 * null stream) and returns without waiting: the caller orders its receives before and its
 * sends after the step on the same stream.  The position advances on the device after every step
 * (the KV cache must already hold positions [0, n_past): llamahip_eval_stage with the same slot
 * selected fills it).  Stepping past n_ctx is refused.
 * llamahip_stage_trace waits for the device, returns the number of steps taken since the bind,
 * stores the current position in *n_past and (last stage) the picked tokens in tokens[0..min(cap,n)). */
int llamahip_stage_bind(llamahip_model *m, int32_t seq, int32_t n_past,
                        void *token_in, const void *hidden_in, void *hidden_out, void *token_out,
                        char *err, size_t err_cap);
int llamahip_stage_step(llamahip_model *m, int32_t seq, int32_t n_threads, void *stream,
                        char *err, size_t err_cap);
int llamahip_stage_trace(llamahip_model *m, int32_t seq, int32_t *n_past, int32_t *tokens, int32_t cap,
                         char *err, size_t err_cap);

/* One decode step for a SET of bound slots at once: the result is bit for bit that of n_seqs llamahip_stage_step calls, one per slot
 * (every operator of llama_eval's graph works row by row, .mm:563-705; each row keeps its own position, KV cache and V*P key split of
 * its own single-token eval, ggml.c:5459-5480) -- but every weight matrix is streamed ONCE per step for all the sequences, which is
 * what a decode step costs ("throughput scales only with independent sequences in flight").  2 .. 16 distinct
 * slots, each bound with plain buffers (no mailbox); one graph is captured per (set of slots, n_threads), at most 32 are kept (least
 * recently used first out).  n_seqs = 1 is llamahip_stage_step.
 * (Norm statistics: a set step runs the reference's two-pass form (ggml.c:5327-5385), a single step takes them one-pass from its
 * producer's partial sums -- both narrow to the same fp32 bits except with probability ~2^-29 per value; the equality
 * of set steps and single steps is therefore tested (tests/test_pipeline.py), not structural.)
 * The score launch of a set covers the key slices up to the set's highest position rounded up to 128 (the host tracks every slot's position;
 * a captured step is keyed by that bucket too and re-captured when a row crosses into the next one). */
int llamahip_stage_step_set(llamahip_model *m, const int32_t *seqs, int32_t n_seqs, int32_t n_threads, void *stream,
                            char *err, size_t err_cap);
/* 1 if llamahip_stage_step_set can step n_seqs slots of this handle with this n_threads as ONE set (Q4_0 handle with layers or f16 / f32
 * whole-model handle, head size a multiple of 32, n_threads <= 32); 0: step the slots one by one with llamahip_stage_step (up to 64 threads;
 * every Q4_0 handle shape, f16 / f32 whole-model handles). */
int32_t llamahip_stage_set_applies(const llamahip_model *m, int32_t n_seqs, int32_t n_threads);

/* Device-side mailboxes between pipeline stages: instead of the caller moving hidden_out -> hidden_in (and token_out -> token_in)
 * between stages with a collective per token, the LAST kernel of a stage step stores the residual-stream row (.mm:563-564, 687-690)
 * straight into the NEXT stage's inbox -- memory of the next stage's process / GPU, peer-mapped through HIP IPC (xGMI stores between
 * GPUs) -- as 8-byte {fp32 bits, tag} granules, and the FIRST kernel of the next stage's step polls them; the last stage's pick
 * kernel stores the token into the first stage's token inbox the same way.  The tag is the sequence position, which every stage
 * knows: no host call, no RCCL launch and no stream ordering between stages per token; every poll is bounded (a lost neighbour
 * surfaces as LLAMAHIP_ERR_PREDICT from the next llamahip_stage_trace).
 *   llamahip_stage_mailbox         creates (once) slot `seq`'s inboxes -- n_embd granules on every stage but the first, one token
 *                                  granule on the first stage of a multi-stage pipeline -- and returns their device pointers
 *                                  (same-process neighbours) and / or 64-byte hipIpcMemHandle_t's (other processes); outputs may be NULL.
 *   llamahip_stage_mailbox_connect gives the slot the NEXT stage's hidden inbox (every stage but the last) and / or the first stage's
 *                                  token inbox (last stage), each as an IPC handle or as a raw device pointer.
 * A slot with an inbox / a connected peer takes NULL for llamahip_stage_bind's hidden_in / hidden_out; on the first stage token_in
 * still carries the FIRST token (bind publishes it to the inbox), later tokens arrive through the mailbox. */
int llamahip_stage_mailbox(llamahip_model *m, int32_t seq, void **hidden_inbox, void **token_inbox,
                           void *hidden_handle64, void *token_handle64, char *err, size_t err_cap);
int llamahip_stage_mailbox_connect(llamahip_model *m, int32_t seq, const void *next_hidden_handle64, void *next_hidden_ptr,
                                   const void *token_handle64, void *token_ptr, char *err, size_t err_cap);

/* Row `row` of the logits the most recent step / eval left on the device (last stage; waits for the device): row 0 after
 * llamahip_stage_step, row i = the i-th slot of the set (in the caller's order) after llamahip_stage_step_set, row i = the i-th row of the
 * eval after llamahip_eval / llamahip_eval_stage.  Every entry point that rewrites the logits resets the row map; a caller that steps
 * a set's slots one by one instead (llamahip_stage_set_applies() == 0) finds the LAST stepped slot's logits in row 0.  Parity tooling. */
int llamahip_stage_logits(llamahip_model *m, int32_t row, float *logits_out, char *err, size_t err_cap);

/* Select which of the handle's n_seq KV caches subsequent evals read and write (default 0). */
int llamahip_set_seq(llamahip_model *m, int32_t seq, char *err, size_t err_cap);

/* Raw fp32 KV rows of layer il, positions [0, n_pos) copied to host (n_pos * n_embd floats each). */
int llamahip_kv_read(llamahip_model *m, int32_t il, int32_t n_pos, float *out_k, float *out_v,
                     char *err, size_t err_cap);

/* Copy a weight tensor's merged file-format bytes (Q4_0 blocks or fp32) back to the host:
 * loader / multi-part merge parity.  Returns the byte count, or -1 for an unknown name. */
int64_t llamahip_tensor_bytes(llamahip_model *m, const char *name, void *out, int64_t cap);

/* ---- the step before the path: f32 / f16 model file -> Q4_0 model file ------------------------
 * Replaces llama_model_quantize (Sources/cpp/quantize.cpp:32-286): same
 * container handling (every 2-D tensor named "*weight" is quantized, everything else is copied, the
 * header's f16 field becomes `itype`), the reference's offline quantizer (utils.cpp:431-485) run on the
 * device.  itype 2 = Q4_0, 3 = Q4_1.  Byte-identical output. */
int llamahip_quantize_file(const char *fname_inp, const char *fname_out, int32_t itype,
                           char *err, size_t err_cap);

/* ---- single-op entry points (parity tests and kernel benchmarks; host buffers in/out) ---------- */
/* y[n][m] = W . quantize_q4_0(x[n])  with W = M rows of K/32 Q4_0 blocks in file layout
 * (replaces ggml_compute_forward_mul_mat_q4_0_f32, ggml.c:5987-6285). */
int llamahip_op_mul_mat_q4_0(const void *w_q4_0, int32_t M, int32_t K, const float *x, int32_t N,
                             float *y, char *err, size_t err_cap);
/* The multi-row (prompt) mat-mul with its kernel chosen by the caller: y[n][m] = W . quantize_q4_0(x[n]) (+ resid[n][m]) through the
 * model's activation quantizer and ONE of its prompt GEMM kernels.  W: M rows of K/32 Q4_0 blocks in file layout, K a positive multiple
 * of 64; x [N][K]; resid [N][M] or NULL (no residual epilogue); y [N][y_stride], y_stride >= M: the WHOLE buffer is copied to the device
 * before the launch and back after it, so columns M .. y_stride - 1 keep what the caller put there unless a kernel writes out of place.
 * path: LLAMAHIP_GEMM_AUTO -- what a model handle with its prompt copies picks (exact kernels only); _MFMA4 k_gemm_mfma4 (exact); _MFMA_I8
 * the int8 matrix-core kernel (exact); _FAST the int8 kernel of LLAMAHIP_FLAG_FAST_PREFILL (NOT exact: one fp32 chain per output);
 * _ROWS k_gemm_rows; _SET k_gemv_set (2 .. 60 rows); _LDS k_gemm_lds (one row: the decode mat-vec).  A kernel that cannot take the shape
 * is refused with a message naming the limit, before anything is launched.  *path_taken (may be NULL): the path that ran --
 * LLAMAHIP_GEMM_GEMV for one row on the decode mat-vec. */
#define LLAMAHIP_GEMM_AUTO    0
#define LLAMAHIP_GEMM_MFMA4   1
#define LLAMAHIP_GEMM_MFMA_I8 2
#define LLAMAHIP_GEMM_FAST    3
#define LLAMAHIP_GEMM_ROWS    4
#define LLAMAHIP_GEMM_SET     5
#define LLAMAHIP_GEMM_LDS     6
#define LLAMAHIP_GEMM_GEMV    7   /* reported only */
int llamahip_op_prompt_gemm_q4_0(const void *w_q4_0, int32_t M, int32_t K, const float *x, int32_t N, const float *resid,
                                 float *y, int32_t y_stride, int32_t path, int32_t *path_taken, char *err, size_t err_cap);
/* The f16 / f32 mat-mul with its kernel chosen by the caller: y[n][m] = dot(W[m], act(x[n])) (+ resid[n][m]), bit for bit ggml_vec_dot_f16
 * (wtype 1: act rounds x to fp16, as the reference's mat-mul does once per row) or ggml_vec_dot_f32 (wtype 0).  w: M rows of K fp16 / fp32
 * values in file layout, K a positive multiple of 32; x [N][K]; resid [N][M] or NULL; y [N][y_stride], y_stride >= M: the WHOLE buffer is
 * copied to the device before the launch and back after it, so columns M .. y_stride - 1 keep what the caller put there unless a kernel
 * writes out of place.  path: LLAMAHIP_DENSE_AUTO -- what a model handle picks (one row _MV, 2 .. 16 rows _SET or _MM by the measured rule of
 * DESIGN.md 12.16, more _MFMA or _MM by the measured rule of DESIGN.md 12.18); _MV k_dense_mv, the decode mat-vec, one launch per row; _MM
 * k_dense_mm (any N: the weights are streamed once per 8 rows); _SET k_dense_set (N 1 .. 16: the weights streamed once); _MFMA k_dense_mfma (N
 * > 16, K a multiple of 128: the 32 chains of every output on the fp32 matrix cores, the weights streamed once per 64 rows, the same bits).
 * LLaMA-7B matrices of an 8-layer f16 file, us per launch, k_dense_mm -> k_dense_mfma (wq|wk|wv, wo, w1|w3, w2, lm head;
 * profiles/dense_mfma_probe.json): 17 rows 88 / 41 / 152 / 95 / 206 -> 108 / 36 / 161 / 89 / 215; 32 rows 103 / 46 / 185 / 103 / 266 -> 108 / 36 /
 * 161 / 90 / 214; 64 rows 192 / 86 / 343 / 207 / 514 -> 117 / 39 / 174 / 100 / 231; 512 rows 1416 / 489 / 2499 / 1254 / 3899 -> 690 / 234 /
 * 1256 / 604 / 1820 (74 TF of the instruction's 155): AUTO takes _MFMA from 64 rows, where it wins on all five.
 * Refusals name their limit and happen before any device is touched (_MFMA with N <= 16 is refused as an unknown path: it is a path of
 * longer evals only).  *path_taken (may be NULL): the path that ran. */
#define LLAMAHIP_DENSE_AUTO 0
#define LLAMAHIP_DENSE_MV   1
#define LLAMAHIP_DENSE_MM   2
#define LLAMAHIP_DENSE_SET  3
#define LLAMAHIP_DENSE_MFMA 4
int llamahip_op_mul_mat_dense(const void *w, int32_t wtype, int32_t M, int32_t K, const float *x, int32_t N, const float *resid,
                              float *y, int32_t y_stride, int32_t path, int32_t *path_taken, char *err, size_t err_cap);
/* The Q4_1 mat-mul with its kernel chosen by the caller: y[n][m] = ggml_vec_dot_q4_1(W[m], quantize_row_q4_1(x[n])) (+ resid[n][m]), bit for
 * bit: one fp32 accumulator per output over all K/2 byte pairs in order, every product and sum rounded on its own.  w_q4_1: M rows in FILE
 * layout, [K/32 floats min][K/32 floats d][K/32 * 16 nibble bytes] per row, K a positive multiple of 32; x [N][K]; resid [N][M] or NULL;
 * y [N][y_stride], y_stride >= M: the WHOLE buffer is copied to the device before the launch and back after it, so columns M .. y_stride - 1
 * keep what the caller put there unless a kernel writes out of place.  path: LLAMAHIP_Q41_AUTO -- what a model handle runs (_CHAIN);
 * _CHAIN k_q41_chain: row tiles of at most 16, the weights streamed and dequantised once per tile, the pair terms formed by product waves
 * and added in pair order by one chain lane per output; _LANE k_q41_mm: a lane per weight row does all of it, once per activation row.
 * Both read the same load-time copy of the weights.  LLaMA-7B matrices of an 8-layer Q4_1 file, us per launch, _LANE -> _CHAIN (wq|wk|wv,
 * wo, w1|w3, w2; profiles/q41_probe.json): 1 row 90 / 89 / 94 / 242 -> 29 / 24 / 54 / 61; 16 rows 130 / 90 / 225 / 249 -> 104 / 48 / 185 / 133
 * (whole evals of 1 .. 512 rows: DESIGN.md 12.24).  Refusals name their limit and happen before any device is
 * touched.  *path_taken (may be NULL): the path that ran. */
#define LLAMAHIP_Q41_AUTO  0
#define LLAMAHIP_Q41_CHAIN 1
#define LLAMAHIP_Q41_LANE  2
int llamahip_op_mul_mat_q4_1(const void *w_q4_1, int32_t M, int32_t K, const float *x, int32_t N, const float *resid,
                             float *y, int32_t y_stride, int32_t path, int32_t *path_taken, char *err, size_t err_cap);
/* One layer's attention (.mm:586-646) on caller-supplied operands with its kernels chosen by the caller.  qkv [N][3d]: the un-rotated q | k | v
 * rows of the eval (the wq | wk | wv product); Kc, Vc [n_ctx][d]: the caches, rows < n_past rotated keys / values, COPIED WHOLE to the device
 * and back, so rows >= n_past + N keep what the caller put there unless a kernel writes out of place.  The op appends rows n_past .. T - 1
 * (T = n_past + N <= n_ctx) with the model's RoPE table, then runs the path.  n_threads (1 .. 64) selects the reference's V*P key split,
 * chunk > 0 splits row n's keys as the eval of `chunk` rows it belongs to (llamahip_eval_chunks).  ws_rows: query rows per batch of the
 * matrix-core chain's workspace (a positive multiple of 64; 0: the model's 512), which the op allocates itself with every byte NaN.
 * merged [N][merged_stride] (merged_stride >= d) or NULL: copied whole both ways, rows merged_stride apart; wo_operand (SHORT, DEC,
 * DEC_STREAM; NULL: not returned): the Q4_0 operand of wo those paths write, as [N][d/32] blocks in file layout.
 * path: LLAMAHIP_ATTN_AUTO -- what a model's multi-row eval picks for the shape once its workspace exists (N >= 2); _MFMA k_rope_kv, then
 * k_attnq_scores_lds -> k_attnq_softmax -> k_attnq_pv_mfma -> k_attnq_merge (N >= 2, head size 128, n_threads <= 8); _ROW k_rope_kv, k_attn;
 * _SHORT k_rope_kv, k_decn_scores + k_dec_pv_blk<true> (2 .. 60 rows); _DEC k_dec_scores (RoPE and append inside, position from a device
 * state word) + k_dec_pv_blk<false> (N = 1); _DEC_STREAM k_dec_scores + k_dec_pv_stream with one workgroup per column block (N = 1).
 * A path that cannot take the shape is refused with a message naming the limit, before anything is launched.  *path_taken (may be NULL):
 * the path that ran.  Not covered here: the kernels with cross-workgroup hand-offs (k_dec_attn_x, k_dec_pv_dma, k_dec_pv_stream split
 * over workgroups: llamahip_op_dec_attention; k_qkv_attn: llamahip_op_qkv_attn).  The batched decode step's form of the short path (a
 * SeqSet: positions on the device, one cache per row) is llamahip_op_set_attention's. */
#define LLAMAHIP_ATTN_AUTO       0
#define LLAMAHIP_ATTN_MFMA       1
#define LLAMAHIP_ATTN_ROW        2
#define LLAMAHIP_ATTN_SHORT      3
#define LLAMAHIP_ATTN_DEC        4
#define LLAMAHIP_ATTN_DEC_STREAM 5
int llamahip_op_attention(const float *qkv, int32_t N, int32_t d, int32_t H, int32_t n_past, int32_t n_ctx, float *Kc, float *Vc,
                          int32_t n_threads, int32_t chunk, int32_t path, int32_t ws_rows, float *merged, int32_t merged_stride,
                          void *wo_operand, int32_t *path_taken, char *err, size_t err_cap);
/* The attention of llamahip_eval_multi's pass on caller-supplied operands: R rows of several KV slots through the row-table kernels
 * (rows_attn.hip: k_rope_kv_rows, then k_rows_scores + k_rows_pv over all R rows).  qkv [R][3d] un-rotated; Kc, Vc [n_slots][n_ctx][d],
 * copied whole both ways; row r belongs to slot row_slot[r], sits at position row_pos[r] and splits row_keys[r] keys over n_threads
 * (llamahip_eval_multi_rows builds such a table).  merged [R][merged_stride] or NULL, wo_operand [R][d/32] Q4_0 blocks or NULL: as
 * llamahip_op_attention's.  The table is checked on the host first, the message naming the limit: the rows of one slot must be one run of
 * consecutive positions in ascending row order with row_pos < row_keys <= the run's end <= n_ctx.  Each run's results are bit for bit
 * llamahip_op_attention's (_SHORT / _ROW) on that run alone with its slot's cache. */
int llamahip_op_attention_rows(const float *qkv, int32_t R, int32_t d, int32_t H, int32_t n_ctx, int32_t n_slots, float *Kc, float *Vc,
                               const int32_t *row_slot, const int32_t *row_pos, const int32_t *row_keys, int32_t n_threads,
                               float *merged, int32_t merged_stride, void *wo_operand, char *err, size_t err_cap);
/* The one-row decode attention through ONE of the kernels that hand data between workgroups inside a launch, for n_steps (1 .. 64) steps on
 * hand-off buffers that live across the steps: _X k_dec_attn_x (per-head counters; H % 8 == 0, n_threads <= 8, n_ctx <= 1024), _STREAM
 * k_dec_scores + k_dec_pv_stream and _DMA k_dec_scores + k_dec_pv_dma (tagged partial sums when the key chains are split over workgroups;
 * n_threads <= 32, n_ctx <= 4096; _DMA: head size 128, H % 8 == 0).  Step i: qkv row i of [n_steps][3d] (un-rotated, as the wq|wk|wv
 * product) at position n_past[i], tagged with layer[i] (0 .. 249); bump_epoch[i] != 0 advances the epoch word (first epoch0) before the
 * launch, as the first launch of a forward pass does.  Kc, Vc [n_ctx][d] go to the device once, every step appends its row, and the whole
 * caches come back.  The op allocates the counters [H][32], the partial sums [32 d], the epoch word and the fault word, zeroes them ONCE and
 * never clears them between steps (what a model handle's later steps see); its score and operand buffers start as 0xFF bytes.  First it
 * asks the placement self-test as a model load does (H x (d / H / 32 + ceil(n_ctx / 32)) workgroups; H % 8 != 0: the 1-D rule over as
 * many); a device that places workgroups otherwise is an error, not a fallback.  The fault-injection bit is never set.
 * force: NULL = the library's rule, else {split, stage_rows, ns, dma} with 0 (dma: -1) = the rule: taken exactly as asked or refused with
 * the reason (a split n_threads cannot take, a stage beyond 512 rows, more than 3 chains per workgroup of k_dec_pv_dma, ns < 2, LDS above
 * 160 KB, dma contradicting the path); the LLAMAHIP_PV_* switches are not read.  plan[8] (may be NULL), set before the device is looked
 * for: what llamahip_debug_dec_attn_plan reports.  Per step: merged [n_steps][d] (0xFF where the launch wrote nothing), wo_operand
 * [n_steps][d / 32] Q4_0 blocks (may be NULL), fault [n_steps] the fault word after the step.  A fault word that is not zero ends the
 * call with an error (later steps are not launched).  A layer used twice under one epoch with split chains is refused: a forward pass
 * spends each tag once.  Everything is refused before any device is touched. */
#define LLAMAHIP_DEC_ATTN_X      0
#define LLAMAHIP_DEC_ATTN_STREAM 1
#define LLAMAHIP_DEC_ATTN_DMA    2
int llamahip_op_dec_attention(const float *qkv, int32_t n_steps, const int32_t *n_past, const int32_t *layer, const int32_t *bump_epoch, uint32_t epoch0,
                              int32_t d, int32_t H, int32_t n_ctx, float *Kc, float *Vc, int32_t n_threads, int32_t path, const int32_t *force,
                              float *merged, void *wo_operand, uint32_t *fault, int64_t *plan, char *err, size_t err_cap);
/* The fused wq|wk|wv mat-vec + decode attention launch (k_qkv_attn: tagged q|k|v granules, tagged scores) for n_steps (1 .. 64) steps on
 * hand-off buffers that live across the steps.  w_q4_0 [3d][d] Q4_0 blocks in file layout (repacked as llamahip_op_gemv_q4_0 does), norm_w
 * [d], Kc / Vc [n_ctx][d] (n_ctx <= 4096; uploaded once, every step appends its row, the whole caches come back).  Step i: the residual-stream
 * row x[i] of [n_steps][d]; n_part[i] pairs {sum, sum of squares} at part_in + 2 i part_stride (0: none -- the pairs are what makes the
 * PREP_NORMP prologue apply); position n_past[i]; layer[i] (0 .. 249) enters the tags; bump_epoch[i] != 0 advances the epoch word (first
 * epoch0) before the launch.  The op allocates the granules of the q|k|v row [3d] and of the scores [H][n_ctx], the epoch word and the
 * fault word, zeroes them ONCE and never clears them between steps; it asks the placement self-test first, as a model load does.  Refused
 * on the host with the reason: everything the model's own predicate refuses (H % 8, head sizes, n_threads > 8, a d whose mat-vec role is
 * none of the three instances), tagged_in != 0 (the mailbox prologue PREP_NORM_TAG waits on another stage), a layer used twice under one
 * epoch, positions outside the cache.  plans [n_steps][5] (may be NULL): per step what llamahip_debug_qkv_attn_plan reports.  Per step:
 * merged [n_steps][d] (the op passes a buffer; the model passes none), wo_operand [n_steps][d / 32] Q4_0 blocks (may be NULL), fault
 * [n_steps].  A fault word that is not zero ends the call with an error.  The fault-injection bit is never set. */
int llamahip_op_qkv_attn(const void *w_q4_0, const float *norm_w, int32_t d, int32_t H, int32_t n_ctx, float *Kc, float *Vc, int32_t n_threads,
                         int32_t n_steps, const float *x, const double *part_in, const int32_t *n_part, int32_t part_stride,
                         const int32_t *n_past, const int32_t *layer, const int32_t *bump_epoch, uint32_t epoch0, int32_t tagged_in,
                         float *merged, void *wo_operand, uint32_t *fault, int64_t *plans, char *err, size_t err_cap);
/* Host-only (no device needed): the launch plan of the one-row decode attention (csrc/dec_attn_plan.cpp) for head layout (d, H), n_ctx and
 * n_threads.  long_ctx: the long-context schedule; have_sync / have_xpart: the handle owns the counters of k_dec_attn_x / the partial-sum
 * buffer of the split soft_max . V (both exist where the load-time placement self-test passed).  force NULL: the rule under the
 * LLAMAHIP_PV_* switches, what a model handle launches; else {split, stage_rows, ns, dma} as llamahip_op_dec_attention takes it (strict).
 * out = { kernel (LLAMAHIP_DEC_KERNEL_*), split, chains per workgroup, rows per stage (PV_STREAM), ring slots (PV_DMA), LDS bytes,
 * workgroups, threads } of the soft_max . V launch (_X: of the one launch).  Returns 1, or 0 with the reason in why (may be NULL). */
#define LLAMAHIP_DEC_KERNEL_PV_BLK    0
#define LLAMAHIP_DEC_KERNEL_X         1
#define LLAMAHIP_DEC_KERNEL_PV_STREAM 2
#define LLAMAHIP_DEC_KERNEL_PV_DMA    3
int32_t llamahip_debug_dec_attn_plan(int32_t d, int32_t H, int32_t n_ctx, int32_t n_threads, int32_t long_ctx, int32_t have_sync, int32_t have_xpart,
                                     const int32_t *force, int64_t out[8], char *why, size_t why_cap);
/* Host-only: the fused wq|wk|wv + attention launch (k_qkv_attn) a model handle of head layout (d, H) runs at n_ctx and n_threads, with
 * n_part_in norm statistics offered by the row's producer (0: none) -- out = { prologue (2 NORM, 4 NORMP), ring depth, granules per thread,
 * workgroups, LDS bytes }.  Returns 1, or 0 where the launch does not take the shape, the reason in why (may be NULL). */
int32_t llamahip_debug_qkv_attn_plan(int32_t d, int32_t H, int32_t n_ctx, int32_t n_threads, int32_t n_part_in, int64_t out[5], char *why, size_t why_cap);
/* the device half of llamahip_eval_topk on caller-supplied logits (n_vocab <= 32768, top_k <= 64) */
int llamahip_op_topk(const float *logits, int32_t n_vocab, const int32_t *last_n_tokens, int32_t n_last, double repeat_penalty,
                     int32_t top_k, double temp, double *cand_scores, int32_t *cand_ids, int32_t *exact, char *err, size_t err_cap);
/* the batched device half of llamahip_decode_sample_multi on caller-supplied rows: logits[n_rows][n_vocab], windows[n_rows][1024] with n_last[r]
 * ids in row r (n_last[r] > 1024: the row is reported inexact); out_scores / out_ids [n_rows][64], out_exact [n_rows] -- row r bit for bit
 * llamahip_op_topk on that row alone.  out_spill (may be NULL) [n_rows][n_vocab]: the rows reported inexact are copied there, the others keep
 * the caller's contents. */
int llamahip_op_topk_rows(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *windows, const int32_t *n_last, double repeat_penalty,
                          int32_t top_k, double temp, double *out_scores, int32_t *out_ids, int32_t *out_exact, float *out_spill, char *err, size_t err_cap);
/* the device half of llamahip_eval_logprobs on caller-supplied rows: logits[n_rows][n_vocab], targets n_rows ids (-1 = not scored,
 * NULL = none scored); any of the three outputs may be NULL */
int llamahip_op_logprob(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *targets,
                        double *logprob_out, int32_t *argmax_out, int32_t *rank_out, char *err, size_t err_cap);
/* One activation-preparation launch (the producers of every mat-mul's Q4_0 operand) on caller-supplied rows, kernel family chosen by the
 * caller.  buf [buf_floats]: ONE buffer uploaded as the caller laid it out; row n of in0 starts at float in0_offset + n * in_stride; in1
 * is the K norm weights at in1_offset (NORM), rows at in1_offset + n * in1_stride (SILU_MUL: the model's layout is in1_offset = in0_offset
 * + F with both strides 2F), unused for PLAIN.  K: a multiple of 32 up to 32768; offsets and strides multiples of 4 floats, strides >= K.
 * mode: _PLAIN y = in0; _NORM y = w * ((float) (x - mean) * scale) (ggml_norm + ggml_mul); _SILU_MUL y = silu_table(in0) * in1.
 * kernel: _AUTO the rule of the model's launches (k_prep_fast unless y is wanted or a NORM row has K / 16 > 1024), _FAST k_prep_fast
 * (register resident; no y; NORM rows up to K / 16 = 1024), _LDS k_prep_qa.  Refusals happen before any device is touched.
 * qa_A [qa_rows][Kp / 4] dwords and qa_d [qa_rows][Kp / 32] scales, Kp = K rounded up to 256, qa_rows >= N: the raw operand, copied to the
 * device before the launch and back after it, so whatever the launch does not write keeps the caller's bits.  y [N][K] (may be NULL):
 * the fp32 rows before quantization, likewise copied both ways.  *kernel_taken (may be NULL): _FAST or _LDS. */
#define LLAMAHIP_PREP_PLAIN    1
#define LLAMAHIP_PREP_NORM     2
#define LLAMAHIP_PREP_SILU_MUL 3
#define LLAMAHIP_PREP_KERNEL_AUTO 0
#define LLAMAHIP_PREP_KERNEL_FAST 1
#define LLAMAHIP_PREP_KERNEL_LDS  2
int llamahip_op_prep(int32_t mode, int32_t kernel, const float *buf, int64_t buf_floats, int64_t in0_offset, int64_t in_stride,
                     int64_t in1_offset, int64_t in1_stride, int32_t K, int32_t N, uint32_t *qa_A, float *qa_d, int32_t qa_rows,
                     float *y, int32_t *kernel_taken, char *err, size_t err_cap);
/* ONE launch of the single-row decode mat-vec (k_gemv) on caller-supplied operands: y = W * prologue(in0, in1), through the epilogue.
 * w_q4_0 [M][K / 32] blocks in file layout, K a positive multiple of 64; interleaved: w is w1's F rows then w3's (M = 2F, F % 32 == 0),
 * repacked into the w1|w3 tile order as a model load does it.  pre: _QA the op quantizes in0 [K] first (the activation launch of
 * llamahip_op_mul_mat_q4_0) and the kernel copies the operand; _PLAIN in0 [K] is quantized in the kernel; _NORM in0 [K] is normalised with
 * the weights in1 [K] (with part_in: n_part_in {sum x, sum x^2} pairs of doubles replace the row's reduction -- the PREP_NORMP instance,
 * selected as in a model's step, LLAMAHIP_NORM_MODE included); _SILU_MUL silu_table(in0 = gate [K]) * (in1 = up [K]).
 * epi: _STORE y [M]; _RESID y = acc + resid [M], and with part_out one {sum y, sum y^2} pair per workgroup (n_part_out must be the
 * launch's grid, plan[4], at most 512; the buffer holds part_out_cap >= n_part_out pairs); _SILU_QA (interleaved only) y [F] (may be
 * NULL) = silu_table(gate) * up and its Q4_0 operand in row 0 of out_A [out_rows][Fp / 4] / out_d [out_rows][Fp / 32], Fp = F rounded up
 * to 256.  y [y_floats], out_A, out_d and part_out are copied to the device before the launch and back after it: whatever the launch
 * does not write keeps the caller's bits.  plan[6] (may be NULL): the plan launched {waves, granules, depth, ring, grid, LDS bytes}, set
 * before the device is looked for.  Refused before any device is touched: the pairs whose kernels wait on other launches or workgroups
 * (tagged operands, the lm head's pick, half-block w1|w3), pairs and shapes without a kernel instance, bad counts, null operands. */
#define LLAMAHIP_GEMV_PRE_QA       0
#define LLAMAHIP_GEMV_PRE_PLAIN    1
#define LLAMAHIP_GEMV_PRE_NORM     2
#define LLAMAHIP_GEMV_PRE_SILU_MUL 3
#define LLAMAHIP_GEMV_EPI_STORE    0
#define LLAMAHIP_GEMV_EPI_RESID    1
#define LLAMAHIP_GEMV_EPI_SILU_QA  2
int llamahip_op_gemv_q4_0(const void *w_q4_0, int32_t M, int32_t K, int32_t interleaved, int32_t pre, int32_t epi, const float *in0, const float *in1,
                          const double *part_in, int32_t n_part_in, const float *resid, float *y, int64_t y_floats, uint32_t *out_A, float *out_d,
                          int32_t out_rows, double *part_out, int32_t n_part_out, int32_t part_out_cap, int64_t *plan, char *err, size_t err_cap);
/* ONE launch of the few-row mat-mul (k_gemv_set, 2 .. 60 rows) on caller-supplied operands: the kernel behind every batched decode step,
 * drafted / verify step, scheduler step and short eval.  w_q4_0 and interleaved as llamahip_op_gemv_q4_0; x [N][K] fp32, K a positive
 * multiple of 64, quantized by the plain activation launch as a model does it.  epi:
 *   _STORE / _RESID   y [N][y_stride] (y_stride >= M) = acc (+ resid [N][M]); copied to the device and back whole: the floats outside the
 *                     N x M block keep the caller's bits.
 *   _ROPE_KV          M == 3 d, d a multiple of 8 and of the head size dh (K need not be d): q rotated into qr [N][d], k rotated and v
 *                     copied into Kc / Vc [n_slots][n_ctx][d], modified in place.  Row r sits at position n_past + r of slot 0, or -- with
 *                     row_pos [N] / row_slot [N] (both or neither; N <= 16) -- at row_pos[r] of slot row_slot[r]: the op builds the SeqSet
 *                     of a batched decode step with pos[] and kv_off[] filled and every other member null.  Positions inside n_ctx and no
 *                     two rows on one (slot, position) are checked on the host.
 *   _SILU_QA / _SILU_QAH (interleaved only)  the Q4_0 operand of silu_table(gate) * up in rows 0 .. N-1 of out_A [out_rows][Fp / 4] /
 *                     out_d [out_rows][Fp / 32] (out_rows >= N, Fp = F rounded up to 256), uploaded and downloaded whole: the launch never
 *                     writes the blocks that pad F.  _SILU_QAH (half-block workgroups, N <= 16): the op owns a zeroed exchange buffer,
 *                     epoch word and fault word; layer in 0 .. 249 enters the tags; the epoch is bumped before each launch; *fault
 *                     receives the fault word.  x_prev [N][K] (may be NULL): the same launch runs first on x_prev into scratch operand
 *                     rows under its own epoch, then the epoch is bumped again and the launch on x runs on the SAME, uncleared exchange
 *                     buffer -- what a model's second step sees.  The fault-injection path is never taken.
 * force: NULL launches what the library's rule picks; else {nc, cw, rgw} (rgw 0: derived) is launched exactly or refused with the reason:
 * the pair must be instantiated, rgw x cw <= 8, the SiLU epilogues take cw == 1 and their own rgw, and the LDS must fit.  plan[7] (may be
 * NULL): the launch {nc, cw, ncg, rgw, LDS bytes, grid, threads}, set before the device is looked for.  Everything is refused before any
 * device is touched: N outside 2 .. 60, shapes the kernel does not take, SILU_QAH with N > 16, null operands, y_stride < M. */
#define LLAMAHIP_GEMV_EPI_ROPE_KV  3
#define LLAMAHIP_GEMV_EPI_SILU_QAH 7
int llamahip_op_gemv_set_q4_0(const void *w_q4_0, int32_t M, int32_t K, int32_t interleaved, int32_t epi, const float *x, int32_t N, const int32_t *force,
                              const float *resid, float *y, int32_t y_stride,
                              int32_t d, int32_t dh, int32_t n_ctx, int32_t n_slots, int32_t n_past, const int32_t *row_pos, const int32_t *row_slot,
                              float *qr, float *Kc, float *Vc,
                              uint32_t *out_A, float *out_d, int32_t out_rows, int32_t layer, const float *x_prev, uint32_t *fault,
                              int64_t *plan, char *err, size_t err_cap);
/* Host-only: N rows of the raw operand above -> [N][K / 32] Q4_0 blocks in file layout (what llamahip_op_attention's wo_operand holds). */
int llamahip_debug_qa_to_blocks(const uint32_t *qa_A, const float *qa_d, int32_t N, int32_t K, void *blocks);
/* The embedding gather (ggml_get_rows on a Q4_0 matrix): tokens [N] in [0, V) (checked on the host), emb [V][d / 32] blocks in file layout,
 * x [N][x_stride] (x_stride >= d) copied whole both ways: the kernels write dense [N][d] rows on the device (followed by a guard the op checks), which
 * the op places x_stride apart.  stats == NULL: k_embed as a multi-row eval launches it.  stats != NULL (N = 1):
 * the decode step's k_embed_part, which also leaves {sum x, sum x^2} of the row in stats[0 .. 1]. */
int llamahip_op_embed(const int32_t *tokens, int32_t N, const void *emb_q4_0, int32_t V, int32_t d, float *x, int32_t x_stride,
                      double *stats, char *err, size_t err_cap);
/* The producers of an f16 / f32 mat-mul's activation operand on caller-supplied rows.  mode, buf, buf_floats, the offsets and the strides
 * are llamahip_op_prep's; wtype 1 (fp16 weights: every value is rounded to fp16 once, RNE, and widened again) or 0 (fp32: unchanged).
 * kernel: _AUTO what a model's mat-mul launches (_FUSED unless a NORM row has K / 16 > 1024), _FUSED k_dense_prep (one launch; refused for
 * such NORM rows), _SPLIT launch_prep's fp32 rows (PLAIN: in0 as it lies) + k_dense_perm_act.  xp [N][K] floats + 64 guard floats, copied
 * to the device before the launch and back after it: the operand as the kernels wrote it, in the chain-major order of the mat-mul kernels
 * (element g * 256 + 32 s + l of a row at g * 256 + l * st + s, st = the steps of its group of 256: 8, fewer in a tail group); whatever
 * the launch does not write keeps the caller's bits.  *kernel_taken (may be NULL): _FUSED or _SPLIT.  Refusals happen before any device
 * is touched. */
#define LLAMAHIP_DENSE_PREP_AUTO  0
#define LLAMAHIP_DENSE_PREP_FUSED 1
#define LLAMAHIP_DENSE_PREP_SPLIT 2
int llamahip_op_dense_prep(int32_t mode, int32_t wtype, int32_t kernel, const float *buf, int64_t buf_floats, int64_t in0_offset, int64_t in_stride,
                           int64_t in1_offset, int64_t in1_stride, int32_t K, int32_t N, float *xp, int32_t *kernel_taken, char *err, size_t err_cap);
/* The embedding gather of an f16 / f32 / Q4_1 model file (ggml_get_rows): tokens [N] in [0, V) (checked on the host); emb [V] rows in file
 * layout, wtype 0 fp32 [d], 1 fp16 [d], 3 Q4_1 ([d / 32 floats min][d / 32 floats d][d / 32 * 16 nibble bytes]); x [N][x_stride] (x_stride >= d)
 * copied whole both ways: the kernels write dense [N][d] rows on the device (followed by a guard the op checks), which the op places
 * x_stride apart. */
int llamahip_op_embed_dense(const int32_t *tokens, int32_t N, const void *emb, int32_t wtype, int32_t V, int32_t d, float *x, int32_t x_stride,
                            char *err, size_t err_cap);
/* The attention of a BATCHED decode step (forward_set / forward_dense_set: llamahip_stage_step_set, the multi-sequence decoders, the verify
 * steps over a set, the request scheduler) on caller-supplied operands: B rows (2 .. 16), each the next token of its own sequence.
 * qkv [B][3d] un-rotated; Kc, Vc [n_slots][n_ctx][d], copied whole both ways; row r appends at position row_pos[r] of slot row_slot[r] and
 * sees keys 0 .. row_pos[r] of that slot, split over n_threads (1 .. 32) as its own one-row eval splits them.  The op builds a device
 * SeqSet: state[r] points at the row's {position, step} pair inside a pool (the pairs are NOT in row order), kv_off[r] = row_slot[r] n_ctx d,
 * pos[r] starts wrong; then, as a step: k_rows_set (gather, on dummy rows) fills pos[], k_rope_kv_set rotates and appends, and
 * launch_attn_short runs k_decn_scores + k_dec_pv_blk<true> with the set and set_keys (0: n_ctx; else the score grid is cut there and
 * every row_pos must lie below it).  The score scratch [16][H][n_ctx] starts filled with the word score_fill, the operand buffers as 0xFF.
 * merged [B][merged_stride] (copied whole both ways) or NULL -- the launch then gets a null merged, as on Q4_0 handles --; wo_operand
 * [B][d/32] Q4_0 blocks or NULL.  After the launch the op fails, naming the row, if the operand blocks that pad d up to a multiple of
 * 256 are not all zero or a state word changed.  Refused on the host with the limit named, before any device is looked for: head sizes
 * that are no multiple of 32 or above 256, n_threads outside 1 .. 32, B outside 2 .. 16, set_keys outside 0 .. n_ctx, slots and positions
 * outside their range, a row at or beyond set_keys, two rows on one (slot, position), rows of one slot that are not ONE run of
 * consecutive ascending positions in adjacent rows (a drafted segment: each row sees the key its neighbour appended in the same step). */
int llamahip_op_set_attention(const float *qkv, int32_t B, int32_t d, int32_t H, int32_t n_ctx, int32_t n_slots, float *Kc, float *Vc,
                              const int32_t *row_slot, const int32_t *row_pos, int32_t n_threads, int32_t set_keys,
                              float *merged, int32_t merged_stride, void *wo_operand, uint32_t score_fill, char *err, size_t err_cap);
/* The FIRST launch of a batched decode step on caller-supplied rows.  mode: _EMBED_Q4_0 k_embed_set, _EMBED_F16 / _EMBED_F32
 * k_embed_dense_set (emb [V][d] in file layout: Q4_0 blocks, fp16 or fp32), _ROWS k_rows_set gathering hid_in [B][d].  tokens [B] in
 * [0, V) (embed modes), row_pos [B] >= 0.  Every row's token word, {position, step} pair (step 7 + 3 r) and hid_in row lives at its own
 * scattered address inside ONE device pool whose other words are 0xFF; the descriptor's pos[] starts wrong.  epoch_in: the epoch word
 * before the launch; pass_epoch != 0 hands the word to the launch (_EMBED_Q4_0 and _ROWS only: the dense kernels take none).
 * x [B][x_stride] copied whole both ways (columns >= d keep the caller's bits; the kernels write dense [B][d] rows followed by a guard the
 * op checks).  Out: pos_out [16] the descriptor's pos[] after the launch (entries >= B must keep their 0x7F7F7F7F), *epoch_out the epoch
 * word, state_out [B][2] the rows' state words, *pool_changed whether any other word of the pool, of the descriptor or around the epoch
 * word changed.  B 2 .. 16, d a multiple of 32; refused on the host before any device is looked for. */
#define LLAMAHIP_SET_ENTRY_EMBED_Q4_0 0
#define LLAMAHIP_SET_ENTRY_EMBED_F16  1
#define LLAMAHIP_SET_ENTRY_EMBED_F32  2
#define LLAMAHIP_SET_ENTRY_ROWS       3
int llamahip_op_set_entry(int32_t mode, const void *emb, int32_t V, int32_t d, const int32_t *tokens, const float *hid_in, int32_t B,
                          const int32_t *row_pos, uint32_t epoch_in, int32_t pass_epoch, float *x, int32_t x_stride,
                          int32_t *pos_out, uint32_t *epoch_out, int32_t *state_out, int32_t *pool_changed, char *err, size_t err_cap);
/* The LAST launches of a batched decode step on caller-supplied rows.  mode: _ARGMAX k_argmax_set on logits [B][V]; _ROWS_OUT k_rows_set
 * scattering x [B][d] to the rows' hid_out, then k_advance_set; _ARGMAX_ONE k_argmax with a state pointer and no mailbox (B = 1: the
 * kernel k_argmax_set is a copy of).  Row r's state pair starts as {row_pos[r], row_step[r]} (row_step in [0, n_ctx)); its tok_out
 * pointer is null where tok_out_null[r] != 0.  State pairs, pick words, trace rows and hid_out rows are scattered inside one device pool
 * whose other words (the guards between the hid_out rows among them) are 0xFF: the op fails if any of those changed.
 * trace [B][n_ctx] copied whole both ways (the picks go to trace[r][row_step[r]]); tok_out [B] the pick words (-1 where nothing was
 * written), hid_out [B][d], state_out [B][2] after the launch.  Refused on the host before any device is looked for. */
#define LLAMAHIP_SET_EXIT_ARGMAX     0
#define LLAMAHIP_SET_EXIT_ROWS_OUT   1
#define LLAMAHIP_SET_EXIT_ARGMAX_ONE 2
int llamahip_op_set_exit(int32_t mode, const float *logits, int32_t V, const float *x, int32_t d, int32_t B, int32_t n_ctx,
                         const int32_t *row_pos, const int32_t *row_step, const int32_t *tok_out_null,
                         int32_t *trace, int32_t *tok_out, float *hid_out, int32_t *state_out, char *err, size_t err_cap);
/* Host only: the key bucket of a batched decode step whose highest row position is max_pos -- the set_keys its score launch is cut at:
 * min(n_ctx, (max_pos / 128 + 1) * 128), so max_pos < set_keys <= n_ctx.  -1 for n_ctx < 1 or max_pos outside [0, n_ctx). */
int32_t llamahip_debug_set_keys(int32_t n_ctx, int32_t max_pos);
/* runtime activation quantizer (ggml.c:456-523): x[k] -> k/32 blocks of 20 bytes */
int llamahip_op_quantize_row_q4_0(const float *x, int32_t k, void *y, char *err, size_t err_cap);

typedef struct llamahip_gemv_bench {
    int32_t M, K;            /* shape */
    int32_t iters;           /* timed launches */
    float   ms_total;        /* HIP-event time over the timed launches, on the launch stream */
    double  algo_bytes;      /* M*(K/32)*20 + (K/32)*20 + 4*M  per launch */
} llamahip_gemv_bench;
/* Times the decode GEMV kernel on the model's resident matrices:
 * which = 0 fused wq|wk|wv, 1 wo, 2 fused w1|w3, 3 w2, 4 output; layer = layer index, or -1 to cycle
 * over every layer so each launch streams different weights from HBM (`iters` = cycles; out->iters =
 * timed launches).  For `output` the matrix is evicted from the Infinity Cache between launches. */
int llamahip_bench_gemv(llamahip_model *m, int32_t which, int32_t layer, int32_t warmup, int32_t iters,
                        llamahip_gemv_bench *out, char *err, size_t err_cap);

/* Times llamahip_kv_copy_rows' launch against the obvious alternative on a plain handle: `iters` times over, the copies enqueued on the
 * handle's stream and the stream waited for -- how = 0: one k_kv_copy_rows launch; how = 1: a loop of hipMemcpyAsync device-to-device calls, one
 * per copy, layer and array (the same ranges, the same stream).  *ms_per_call: host wall time per enqueue + wait, the mean over `iters` after
 * one untimed call.  The arguments are llamahip_kv_copy_rows' and are refused the same way.  Measurement tooling only. */
int llamahip_bench_kv_copy(llamahip_model *m, int32_t n_copies, const int32_t *src_slot, const int32_t *dst_slot, const int32_t *row_begin,
                           const int32_t *n_rows, int32_t how, int32_t iters, double *ms_per_call, char *err, size_t err_cap);

/* Times llamahip_kv_shift_rows' launch on a plain handle: one untimed launch, then `iters` launches between two events on the handle's stream;
 * *ms_per_launch: the events' time / iters.  The arguments are llamahip_kv_shift_rows' and are refused the same way; the rows it moves are
 * moved iters + 1 times, so the slot's contents are spent afterwards.  Measurement tooling only. */
int llamahip_bench_kv_shift(llamahip_model *m, int32_t n_shifts, const int32_t *slot, const int32_t *row_begin, const int32_t *n_rows,
                            const int32_t *n_discard, int32_t iters, double *ms_per_launch, char *err, size_t err_cap);

/* One k_kv_shift_rows launch (llamahip_kv_shift_rows' kernel and arithmetic; NOT the reference's) on caller-supplied host caches Kc, Vc
 * [n_slots][n_layers][n_ctx][d] fp32, copied up and back, with the library's angle table for (n_ctx, dh).  Refused with the limit named, before
 * any device work: null caches, counts < 1, d not a multiple of 4, dh odd or not dividing d, and what llamahip_kv_shift_rows refuses of its table. */
int llamahip_op_kv_shift(float *Kc, float *Vc, int32_t n_slots, int32_t n_layers, int32_t n_ctx, int32_t d, int32_t dh, int32_t n_shifts,
                         const int32_t *slot, const int32_t *row_begin, const int32_t *n_rows, const int32_t *n_discard, char *err, size_t err_cap);
/* Host only: the library's RoPE angle table, out[n_ctx][dh / 2][2] = {cos, sin} of position * 10000^(-2 pair / dh) from the host libm's
 * sincos -- what a model load and the ops upload.  Other libms differ in the last bit of some entries, so a restatement of a kernel that
 * reads the table reads this.  Returns 0, or -1 for n_ctx < 1, dh odd or < 2, or a null out. */
int32_t llamahip_debug_rope_table(int32_t n_ctx, int32_t dh, double *out);

/* In-kernel phase probe of the decode GEMVs: runs n_steps greedy decode steps with the probe armed;
 * one record of 8 uint64 per GEMV launch {s_memtime at entry, loads issued, prologue done, weights
 * consumed, exit; ngroups; nchunks; PRE*16+EPI}.  Returns the record count.  Measurement tooling only. */
int64_t llamahip_debug_decode_phases(llamahip_model *m, int32_t n_past, int32_t first_token, int32_t n_steps,
                                     uint64_t *records, int64_t cap, char *err, size_t err_cap);

/* Launch counts of the multi-row mat-mul kernel families since process start, in the order
 * {matrix-core (k_gemm_mfma4 and k_gemm_mfma, every launch), row-per-lane (k_gemm_rows), LDS-staged (k_gemm_lds), mat-vec (k_gemv),
 *  few rows (k_gemv_set), the fast kernel of LLAMAHIP_FLAG_FAST_PREFILL (k_gemm_mfma<*, true>: also counted as matrix-core)}:
 * lets a test assert that a shape took the path it is meant to.  Returns the number of families. */
int32_t llamahip_debug_gemm_paths(int64_t *out, int32_t cap);
/* Launch counts of the f16 / f32 mat-mul kernels since process start: out[0 .. 2] = { k_dense_mv, k_dense_mm, k_dense_set } (at most `cap`
 * entries are written); returns 3.  Tests and measurement tooling. */
int32_t llamahip_debug_dense_paths(int64_t *out, int32_t cap);
/* Host only: the launch plan of k_dense_set for an M x K matrix of wtype (0 fp32, 1 fp16) and n_rows activation rows --
 * out = { grid, threads per workgroup, weight rows per half-wave, activation rows of the compiled instance, groups of 256 elements per
 * row and LDS slab, static LDS bytes }.  Returns 1, 0 where the kernel does not take the shape (K not a multiple of 32, n_rows outside
 * 1 .. 16, another wtype), -1 where the plan names an instance that was never compiled. */
int32_t llamahip_debug_dense_set_plan(int32_t m, int32_t k, int32_t wtype, int32_t n_rows, int64_t out[6]);
/* Host only: the launch plan of k_dense_mfma for an M x K matrix of wtype (0 fp32, 1 fp16) and n_rows activation rows --
 * out = { workgroups, threads per workgroup, activation rows per workgroup tile, weight rows per workgroup tile, dynamic LDS bytes,
 * 1 where LLAMAHIP_DENSE_AUTO picks the kernel for this shape else 0 }.  Returns 1, 0 where the kernel does not take the shape (n_rows <= 16,
 * K not a multiple of 128, another wtype, n_rows * k >= 2^31), -1 where the plan names an instance that was never compiled. */
int32_t llamahip_debug_dense_mfma_plan(int32_t m, int32_t k, int32_t wtype, int32_t n_rows, int64_t out[6]);
/* Q4_1 mat-muls per kernel since process start: out[0 .. 1] = { k_q41_chain, k_q41_mm } (at most `cap` entries are written); returns 2.
 * One count per mat-mul, however many row tiles it launched.  Tests and measurement tooling. */
int32_t llamahip_debug_q41_paths(int64_t *out, int32_t cap);
/* Host only: the launch plan of k_q41_chain for an M x K Q4_1 matrix and n_rows activation rows -- out = { activation rows of the compiled
 * instance, weight rows per workgroup, threads per workgroup, grid x, grid y (row tiles of at most 16), slab length in byte pairs
 * (2 elements each), dynamic LDS bytes, chain lanes per workgroup }.  For n_rows > 16 this is the plan of the full tiles; a last tile of
 * n_rows % 16 rows is a launch of its own on the plan of that row count.  Returns 1, 0 where the kernel does not take the shape (K not a
 * positive multiple of 32, m or n_rows < 1), -1 where the plan names an instance that was never compiled. */
int32_t llamahip_debug_q41_plan(int32_t m, int32_t k, int32_t n_rows, int64_t out[8]);
/* Launches of k_dense_mfma since process start (llamahip_debug_dense_paths keeps its three entries).  Tests and measurement tooling. */
int64_t llamahip_debug_dense_mfma_launches(void);
/* Process-wide, for tests and measurement: 0 -- the measured rule; LLAMAHIP_DENSE_MM / LLAMAHIP_DENSE_MFMA -- every f16 / f32 mat-mul of more
 * than 16 rows that a model handle (or LLAMAHIP_DENSE_AUTO) launches goes to that kernel where the kernel takes the shape, and to the rule's
 * choice where it does not.  LLAMAHIP_DENSE_MM=mm / mfma in the environment does the same.  Returns the previous value, -1 for another path
 * (nothing changes).  Not synchronised with evals in flight on other threads. */
int32_t llamahip_debug_dense_force(int32_t path);
/* Host-only (no device needed): the attention path (LLAMAHIP_ATTN_SHORT / _MFMA / _ROW) a model's multi-row eval of N rows after n_past
 * takes once its workspace exists (allocated with the first multi-row eval), or -1 for N < 2 -- the rule llamahip_op_attention's AUTO runs. */
int32_t llamahip_debug_attn_path(int32_t N, int32_t head_size, int32_t n_past, int32_t n_threads, int32_t n_ctx);
/* Host-only (no device needed): how the few-row mat-mul would take n_rows activation rows against an m x k Q4_0 matrix (interleaved:
 * the w1|w3 layout; epi: 0 store, 1 +residual, 2 / 7 SiLU*up -> Q4_0 in whole- / half-block workgroups, 3 RoPE + KV append) --
 * out = {columns per wave, column-waves per row-group, column groups, row-groups per workgroup, LDS bytes}; 0 = the kernel does not
 * take that shape (the caller's generic path runs).  Lets a CPU test walk every LLaMA shape and row count. */
int32_t llamahip_debug_set_plan(int32_t m, int32_t k, int32_t interleaved, int32_t n_rows, int32_t epi, int64_t out[5]);
/* Host-only (no device needed): the launch plan of the single-row decode mat-vec for an m x k Q4_0 matrix (interleaved: the w1|w3 layout)
 * under prologue `pre` (0 staged Q4_0 operand, 1 plain, 2 norm, 3 SiLU*up, 4 norm with the producer's statistics, 6 norm of a tagged row)
 * and epilogue `epi` (0 store, 1 +residual, 2 / 7 SiLU*up -> Q4_0 in whole- / half-block workgroups, 5 +residual with tagged rows, 6 store
 * + greedy pick) -- out = {waves per workgroup, operand granules per thread, ring depth, 1 ring / 0 whole row in flight, grid, LDS bytes}.
 * Returns 1; 0 = the kernel does not take that (matrix, pre, epi); -1 = the plan names an instance that was never compiled (a defect). */
int32_t llamahip_debug_gemv_plan(int32_t m, int32_t k, int32_t interleaved, int32_t pre, int32_t epi, int64_t out[6]);
/* in-kernel phase records of the few-row mat-mul (measurement builds only; 0 records in the product build) */
int64_t llamahip_debug_set_probe(uint64_t *records, int64_t cap, int32_t reset);

/* Bit 0 / bit 1: the decode kernels evaluate the reference's SiLU / exp fp16 tables with device arithmetic instead of
 * gathering them -- enabled only after a load-time check that all 65 536 entries are reproduced.  0 before any load. */
int32_t llamahip_debug_lut_math(void);

/* Host-only (no device needed): the device and pinned-host allocations this library holds at this moment, process-wide -- every model
 * handle's (weights, KV cache, workspaces, slots, set descriptors) and the scratch of a single-op call while it runs -- and their bytes.
 * Either pointer may be null.  The library's own exact count: a handle that is freed brings both back to what they were before its load,
 * which free device memory as the runtime reports it cannot show on a card that other processes use.  Tests. */
void llamahip_debug_live_allocs(int64_t *n, int64_t *bytes);

typedef struct llamahip_stats {
    int32_t struct_size;
    int64_t weight_bytes_device;   /* repacked Q4_0 bytes resident in HBM */
    int64_t kv_bytes_device;
    int64_t n_evals;
    double  t_load_ms;             /* the reference measures t_load_us/t_predict_us and drops them (.mm:778,845) */
    double  t_eval_ms_total;
    int32_t n_stages;              /* in-process layer pipeline: stages of this handle (1: a plain handle) */
    int32_t hand_off;              /* ... 1 once llamahip_decode_greedy has run on it: the row and the token move between its stages as stream-ordered copies */
} llamahip_stats;
int llamahip_get_stats(const llamahip_model *m, llamahip_stats *out);

const char *llamahip_version(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* LLAMAHIP_H */
