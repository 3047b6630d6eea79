/* llama_runner.h -- C mirror of the reference's bridge object and event stream, so the behaviour
 * of `LlamaRunner.run(with:config:...)` can be exercised (and tested) without a Swift / Objective-C
 * toolchain.  Names follow the reference:
 *
 *   _LlamaRunnerBridge        Sources/llamaObjCxx/headers/LlamaRunnerBridge.h:16-27
 *   _LlamaRunnerBridgeConfig  Sources/llamaObjCxx/headers/LlamaRunnerBridgeConfig.h:13-18
 *   _LlamaEvent (6 cases)     Sources/llamaObjCxx/headers/LlamaEvent.h:13-25
 *   LlamaErrorDomain / codes  Sources/llamaObjCxx/headers/LlamaError.h:12-19, LlamaError.m:10
 *   -[LlamaPredictOperation main]  Sources/llamaObjCxx/bridge/LlamaPredictOperation.mm:768-901
 *
 * Differences, all forced by the missing Apple runtime: events are delivered by a synchronous C
 * callback on the calling thread instead of dispatch_async onto a queue (.mm:903-910), and `run`
 * returns when the generation has completed instead of enqueueing an NSOperation
 * (LlamaRunnerBridge.mm:28-47).
 */
#ifndef LLAMA_RUNNER_H
#define LLAMA_RUNNER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the declarations of this header are its whole dynamic symbol table. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define LLAMA_ERROR_DOMAIN "com.alexrozanski.llama.error"   /* LlamaError.m:10 */

typedef enum llama_event_type {
    LLAMA_EVENT_STARTED_LOADING_MODEL = 0,
    LLAMA_EVENT_FINISHED_LOADING_MODEL = 1,
    LLAMA_EVENT_STARTED_GENERATING_OUTPUT = 2,
    LLAMA_EVENT_OUTPUT_TOKEN = 3,
    LLAMA_EVENT_COMPLETED = 4,
    LLAMA_EVENT_FAILED = 5,
} llama_event_type;

/* _LlamaRunnerBridgeConfig + the harness-only extensions SURVEY.md section 5 routes around the
 * Swift surface (n_ctx is hard-coded to 512 in the reference, .mm:790; greedy = argmax, fact 8). */
typedef struct llama_runner_config {
    uint32_t numberOfThreads;     /* LlamaRunner.Config.numThreads, default 8  (LlamaRunner.swift:17) */
    uint32_t numberOfTokens;      /* LlamaRunner.Config.numTokens,  default 512 */
    const char *reversePrompt;    /* tokenized and then unused by the reference (.mm:815) */
    int32_t n_ctx;                /* extension: 0 = 512 */
    int32_t greedy;               /* extension: 1 = argmax instead of top-k/top-p sampling */
    int32_t seed;                 /* gpt_params.seed, default -1 (utils.h:16) */
    int32_t keepModel;            /* extension: 1 = the bridge keeps the loaded model between
                                     runs instead of the reference's load + free per run (.mm:790, :900); the
                                     loading events are still posted.  The model is freed with the bridge. */
} llama_runner_config;

/* text = token bytes for OUTPUT_TOKEN, the NSLocalizedDescription message for FAILED, else NULL;
 * code = LlamaErrorCode for FAILED (-1000 load, -1001 predict), else 0 */
typedef void (*llama_event_handler)(void *user, llama_event_type type, const char *text, uint32_t text_len, int32_t code);

typedef struct llama_runner_bridge llama_runner_bridge;

llama_runner_bridge *llama_runner_bridge_new(const char *model_path);          /* -initWithModelPath: */
void llama_runner_bridge_free(llama_runner_bridge *b);
const char *llama_runner_bridge_model_path(const llama_runner_bridge *b);      /* @property modelPath */
int64_t llama_runner_bridge_loads(const llama_runner_bridge *b);              /* model loads performed so far (keepModel tests) */

/* -runWithPrompt:config:eventHandler:eventHandlerQueue:  -- one load + one generation per call,
 * exactly like one LlamaPredictOperation (unless config->keepModel).  Runs on one bridge are
 * serialised (the reference's operation queue runs one operation at a time, LlamaRunnerBridge.mm:18-26).
 * Returns 0 if `completed` was emitted, else the error code. */
int32_t llama_runner_bridge_run(llama_runner_bridge *b, const char *prompt, const llama_runner_config *config,
                                llama_event_handler handler, void *user);

void llama_runner_config_default(llama_runner_config *c);                       /* Config.default */

/* Extension: drafted sampled decoding in the generation loop (llamahip_verify_sample; llamahip.h "sampled decode with drafted tokens").
 * draft_len 0 = off (the default), 1 .. 15 = on with drafts of up to that many tokens (values outside are clamped).  A bridge that never
 * calls the setter -- the unchanged replacement bridge -- takes LLAMAHIP_RUNNER_LOOKUP=<1..15> from the environment at each run.
 * llama_runner_config keeps its layout (it has no size field and callers pass it by pointer).
 * When on, and the run is not `greedy`, LLAMAHIP_HOST_SAMPLER is not set, the prompt is used up and one token is pending: the loop drafts
 * from the prompt tokens plus everything generated so far (llamahip_lookup_draft, its default n-grams), cut to remaining - 1, runs one
 * llamahip_verify_sample and posts picks[0 .. n_accept] as token events in order; where nothing is drafted the step is the usual one.
 * The event stream is byte for byte the one the same seed produces with lookup off; runs with lookup off, `greedy` runs and the prompt
 * phase run the code they ran before.
 * llama_runner_bridge_lookup_stats: the counts of the bridge's last run (all zero before the first run and for runs without lookup steps);
 * out->struct_size is set by the caller; returns 0, or -1 for a null argument or a wrong struct_size. */
struct llamahip_lookup_stats;
void llama_runner_bridge_set_lookup(llama_runner_bridge *b, int32_t draft_len);
int32_t llama_runner_bridge_lookup_stats(const llama_runner_bridge *b, struct llamahip_lookup_stats *out);

/* Extension: generating past the context window (llamahip.h "generating past the context window").
 * mode 0 = stop at the wall (the default and the reference's behaviour: n_predict = min(numberOfTokens, n_ctx - n_inp), .mm:812),
 * 1 = re-evaluate (LLAMAHIP_CTX_REEVAL: exact), 4 = shift the cache in place (LLAMAHIP_CTX_SHIFT: NOT the reference's arithmetic, opt-in:
 * at the wall llamahip_kv_shift_rows moves the surviving rows down instead of the evals below; token bookkeeping, events and the lookup
 * room are the same); other values are 0.
 * n_keep: the tokens at the start of the context that are never dropped; -1 = the prompt's length; either way at most n_ctx / 2.
 * A bridge that never calls the setter -- a caller that cannot be changed -- takes LLAMAHIP_RUNNER_OVERFLOW=reeval (or =shift) from the
 * environment at each run (n_keep -1).  llama_runner_config keeps its layout.
 * With a mode set and a prompt that fits (n_inp <= n_ctx), n_predict is numberOfTokens, uncapped.  When the prompt is used up and the
 * pending token has no room (n_past == n_ctx) the loop applies llamahip_ctx_overflow_plan and feeds
 * the surviving tail's tokens again at n_past = n_keep the way the prompt is fed (llamahip_eval_chunks in chunks of n_batch + 1 = 9
 * tokens); then the loop goes on as before.  Lookup steps cut their draft to the room left in the cache.  With mode 0 the loop runs the
 * code it ran before and the event stream is unchanged; a prompt that does not fit is handled as before in every mode, and so
 * is a context so small that the plan could never discard a token (n_ctx - n_keep < 2): the run stops at the wall as with mode 0. */
void llama_runner_bridge_set_overflow(llama_runner_bridge *b, int32_t mode, int32_t n_keep);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
