// llamahip.cpp -- C ABI of libllamahip.so (include/llamahip.h): loader, device residency, forward
// pass schedule.  Replaces llama_model_load / llama_eval of the reference bridge
// (Sources/llamaObjCxx/bridge/LlamaPredictOperation.mm:98-498, 510-735).  There is no CPU
// fallback: every compute entry point needs a HIP device and fails loudly without one.
#include "../../include/llamahip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "host_util.h"
#include "llamahip_internal.h"
#include "model_file.h"
#include "sched.h"
#include "constrain.h"

using namespace lh;

// ------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------
void lh::set_err(char *err, size_t cap, const char *fmt, ...) {
    if (!err || !cap) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, cap, fmt, ap);
    va_end(ap);
}

namespace {

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// the n_threads of a call as the kernels take it (the key split of the attention follows it)
inline int clamp_threads(int n_threads) { return std::max(1, std::min(n_threads, 64)); }

struct Layer {
    float *attention_norm = nullptr, *ffn_norm = nullptr;   // fp32 [d]
    QMat qkv;    // rows [wq; wk; wv]  (3d x d)
    QMat wo;     // d x d
    QMat w13;    // rows [w1; w3]      (2F x d)
    QMat w2;     // d x F
    // f16 / f32 model files (hp.f16 = 1 / 0): the same matrices, row-major as in the file
    DMat dqkv, dwo, dw13, dw2;
};

// fp16 lookup tables, built on the host with the host libm exactly as ggml_init does
// (ggml.c:2376-2389): silu(x) = x/(1+exp(-x)) in double -> float -> fp16 ; exp(x) likewise.
uint16_t f32_to_f16_rne(float f) {
    // portable round-to-nearest-even conversion (same result as F16C _cvtss_sh(x, 0))
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    const uint32_t ax = x & 0x7FFFFFFFu;
    if (ax >= 0x7F800000u) return (uint16_t) (sign | (ax > 0x7F800000u ? 0x7E00u | ((ax >> 13) & 0x3FFu) : 0x7C00u));   // nan / inf
    if (ax >= 0x477FF000u) return (uint16_t) (sign | 0x7C00u);            // rounds to inf (>= 65520)
    if (ax < 0x33000001u) return (uint16_t) sign;                        // rounds to zero (<= 2^-25)
    int32_t exp = (int32_t) (ax >> 23) - 127;
    uint32_t mant = (ax & 0x7FFFFFu) | 0x800000u;
    uint32_t half;
    if (exp < -14) {                                                      // subnormal half
        const int shift = -14 - exp + 13;                                 // 14..24
        const uint32_t rem_mask = (1u << shift) - 1;
        const uint32_t rem = mant & rem_mask, halfway = 1u << (shift - 1);
        half = mant >> shift;
        if (rem > halfway || (rem == halfway && (half & 1))) half++;
    } else {
        const uint32_t rem = mant & 0x1FFFu;
        half = ((uint32_t) (exp + 15) << 10) | ((mant >> 13) & 0x3FFu);
        if (rem > 0x1000u || (rem == 0x1000u && (half & 1))) half++;      // carry may bump the exponent: still correct
    }
    return (uint16_t) (sign | half);
}

float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t) (h & 0x8000u) << 16;
    const uint32_t exp = (h >> 10) & 0x1F, mant = h & 0x3FFu;
    uint32_t out;
    if (exp == 0) {
        if (mant == 0) out = sign;
        else {
            int e = -1;
            uint32_t m = mant;
            do { e++; m <<= 1; } while (!(m & 0x400u));
            out = sign | ((uint32_t) (127 - 15 - e) << 23) | ((m & 0x3FFu) << 13);
        }
    } else if (exp == 31) {
        out = sign | 0x7F800000u | (mant << 13);
    } else {
        out = sign | ((exp + 112) << 23) | (mant << 13);
    }
    float f;
    memcpy(&f, &out, 4);
    return f;
}

}  // namespace

// the silu and exp tables of ggml_init (ggml.c:2376-2389) and the RoPE angle table [n_ctx][dh/2][cos, sin] (ggml.c:7113-7116), host libm
void lh::lut_tables(std::vector<uint16_t> &ts, std::vector<uint16_t> &te) {
    for (int i = 0; i < (1 << 16); i++) {
        const float f = f16_to_f32((uint16_t) i);
        ts[i] = f32_to_f16_rne((float) ((double) f / (1.0 + exp((double) -f))));
        te[i] = f32_to_f16_rne((float) exp((double) f));
    }
}
std::vector<double> lh::rope_table(int n_ctx, int dh) {
    std::vector<double> sc((size_t) n_ctx * dh);
    for (int p = 0; p < n_ctx; p++) {
        for (int i0 = 0; i0 < dh; i0 += 2) {
            const double theta = pow(10000.0, ((double) -i0) / dh);
            double sn, cs;
            sincos(p * theta, &sn, &cs);                  // the reference's -O3 build calls sincos()
            sc[(size_t) p * dh + i0] = cs;
            sc[(size_t) p * dh + i0 + 1] = sn;
        }
    }
    return sc;
}

// The step descriptor of a verify step over a set (llamahip_verify_greedy_multi): a SeqSet whose rows take their position and token from the
// per-row words behind it instead of a bound slot's -- set.state[r] points at state[r], set.tok_in[r] at tok[r] -- so the launches of a set step
// (forward_set) run it unchanged; the segments, the rows' picks and the result follow.  Built on the host up to `pick`, lives in device memory.
struct VsetBlock {
    SeqSet set;
    int32_t state[SET_MAX][2];          // row r: {position, unused}
    int32_t tok[SET_MAX];               // row r's token: a segment's first row the slot's last token, the rest its draft
    int32_t seg_begin[SET_MAX + 1];     // segment s = rows [seg_begin[s], seg_begin[s + 1])
    int32_t seg_slot[SET_MAX];
    int32_t pick[SET_MAX];              // (device) k_verify_rows
    int32_t res[2 * SET_MAX];           // (device) k_accept_drafts_set: {n_accept[n_segs], pick[n_rows]}
};

// ------------------------------------------------------------------------------------------------
// the model handle
// ------------------------------------------------------------------------------------------------
namespace lh {
void sched_dev_orphan(SchedDev *d);
int sched_dev_max_active(const SchedDev *d);          // the slots [0, max_active) a live scheduler owns (llamahip_kv_copy_rows writes none of them)
int kv_copy_enqueue(const std::vector<llamahip_model *> &stages, const KvCopyTab &tab, const char *fn, char *err, size_t err_cap);
}
struct llamahip_model {
    ModelFile file;
    HParams hp;
    int device = 0;
    int l0 = 0, l1 = 0;                  // layers [l0, l1) live on this handle
    bool first_stage = true, last_stage = true;
    int flags = 0;
    bool host_only = false;
    hipStream_t stream = nullptr;
    // Every device / pinned allocation of this handle, of its slots and of its set descriptors is registered here; the members below are
    // views.  Declared before the graph caches and the events: members go in reverse order, so the memory is released after them -- and
    // after the destructor's device-wide wait.
    DevOwner own;

    // weights
    uint8_t *tok_emb = nullptr;          // file-layout rows (gathered, never streamed)
    float *norm_w = nullptr;
    QMat output;
    bool dense = false;                  // f16 / f32 model file: DMat weights, un-fused schedule (dense.hip)
    DMat doutput;
    std::vector<Layer> layers;           // index il - l0

    // KV cache: fp32 [layer][n_ctx][d] each (.mm:290-304)
    float *Kc = nullptr, *Vc = nullptr;

    // tables
    uint16_t *T_silu = nullptr, *T_exp = nullptr;
    double *sincos = nullptr;            // [n_ctx][dh/2][2]

    // workspace (sized for ws_cap tokens)
    int ws_cap = 0;
    int32_t *d_tokens = nullptr;
    // single-token evals through the C ABI: token, sampler window and candidate results live in ONE pinned, device-mapped host
    // block that the kernels read / write directly (three ~4 us blit copies per sampled token otherwise)
    struct HostIo { int32_t tok[16]; int32_t window[1024]; double sc[64]; int32_t id[64]; int32_t fl[2];
                    int32_t slide[1024 + VERIFY_ROWS_MAX]; TopkOut rows[VERIFY_ROWS_MAX];      // (a sampled verify step: its id stream in, its rows' candidates out)
                    VsetBlock vset;                // (a verify step over a set: its descriptor out, vset.res back)
                    int32_t pool[SLIDE_SET_IDS]; int32_t row_tab[2 * VERIFY_ROWS_MAX];          // (a sampled verify step over a set: its id pool and {row_off, row_n_last} in; `rows` back)
                    int32_t slot_words[2 * SET_MAX]; };                                         // (the drafted sampled loop: the slots' {position, cursor} on their way to d_slot_state)
    HostIo *h_io = nullptr, *d_io = nullptr;       // host pointer / its device alias
    float *x = nullptr, *x1 = nullptr, *qkv = nullptr, *qr = nullptr, *merged = nullptr, *gu = nullptr;
    float *tmp = nullptr;                // debug: un-fused residual operand
    float *logits = nullptr;             // [ws_cap][V] (all rows only in debug evals)
    uint32_t *qa_A = nullptr;
    float *qa_d = nullptr;
    uint8_t *qb_ws = nullptr;            // [ws_cap][KpMax] int8 operand of the matrix-core prompt GEMM
    uint32_t *qaF_A = nullptr;           // short evals: QA operand of w2 written by the fused w1|w3 epilogue, [64][Kp(n_ff)]
    float *qaF_d = nullptr;              //   (zeroed once: the blocks that pad n_ff to a multiple of 256 are never written)
    float *dbg_y = nullptr, *dbg_p = nullptr, *dbg_kqv = nullptr;
    int32_t *d_out_tokens = nullptr;     // greedy decode results
    void *d_topk = nullptr;              // sampler front end on the device: [1024 window ids][64 scores][64 ids][2 flags]
    int out_tokens_cap = 0;

    // decode-path state (device resident so a captured graph can be replayed unchanged)
    int32_t *d_state = nullptr;          // [0] n_past, [1] decode step index
    float *sc = nullptr;                 // attention scores [H][n_ctx]
    float *part = nullptr;               // V*P partial sums [H][64][dh]
    uint32_t *qa1_A = nullptr, *qa2_A = nullptr;   // QA operands: attention output (K = d), FFN activation (K = F)
    float *qa1_d = nullptr, *qa2_d = nullptr;
    bool w13_interleaved = false;
    bool prompt_copies = false;          // the row-lane / matrix-core copies of the layer matrices exist (ensure_prompt_copies)
    bool output_copies_tried = false;    // ... and of `output`, for the scoring entry points' all-rows lm head (ensure_output_copies)
    void *d_score = nullptr;             // scoring of N rows: [N] logprob (double) | [N] argmax | [N] rank | [N] targets (score_io)
    int score_cap = 0;
    char *beam_blk = nullptr;            // llamahip_beam_search (last stage): pinned, mapped -- [16][32] logprob (double) | [16][32] ids; beam_dev: its device alias
    char *beam_dev = nullptr;
    char *d_topn = nullptr;              // the top-n places of N rows (last stage; topn_enqueue): [N][n] logprob (double) | [N][n] ids
    size_t topn_cap = 0;                 // ... its bytes
    // a text's embedding (last stage; embed_ensure): out [embed_segs_cap][d] | seg_begin [embed_segs_cap + 1] | the fp32 norm rows y [embed_rows_cap][d],
    // and the host copy seg_begin is uploaded from
    char *d_embed = nullptr;
    int embed_segs_cap = 0, embed_rows_cap = 0;
    std::vector<int32_t> h_embed_seg;
    char *d_slide = nullptr;             // sampled verify step (last stage): 16 x TOPK_WS_BYTES of selection workspace | the id stream (SLIDE_IDS_BYTES) | 16 TopkOut (slide_ensure)
    VsetBlock *d_vset = nullptr;         // a verify step over a set: the step's descriptor (vset_step)
    int32_t *d_slide_set = nullptr;      // sampled verify step over a set (last stage, no pinned block): the id pool (SLIDE_SET_IDS) | row_off[16] | row_n_last[16]
    int32_t *d_verify = nullptr;         // drafted greedy decoding (last stage): {position, cursor} | 16 row tokens | 16 picks | {n_accept, 16 picks} | from [64]: the token log, n_ctx entries (verify_io)
    uint32_t *d_attn_sync = nullptr;     // per-head hand-off counters of k_dec_attn_x ([H][32] dwords); null: two-launch attention
    uint64_t *d_qkv2 = nullptr, *d_sc2 = nullptr;   // tagged hand-off buffers of k_qkv_attn: [3 d] and [H][n_ctx] {fp32 bits, tag} granules
    uint32_t *d_epoch = nullptr;         // ... and the epoch word their tags are made from (bumped once per decode forward pass)
    uint64_t *d_set_amax = nullptr;      // the same for the rows of a short eval / a batched decode step (k_gemv_set): [SET_MAX][F / 16 + 16] granules
    uint64_t *d_w13_amax = nullptr;      // partial amaxes exchanged by the half-block workgroups of the w1|w3 decode mat-vec (EPI_SILU_QAH): [F / 16] granules
    unsigned long long *d_pick = nullptr; // greedy loop: {64-bit atomic-max key, arrival counter} of the lm head's pick epilogue (EPI_STORE_PICK)
    uint64_t *d_pvx = nullptr;           // tagged partial sums of k_dec_pv_stream's split workgroups: [H dh/32][32 threads of the split][32]
    uint32_t *h_fault = nullptr;         // sticky fault word in pinned, device-mapped host memory: a bounded in-launch spin that
    uint32_t *d_fault = nullptr;         //   ran out raises it; the host reads it (a plain load) after every synchronisation
    double *npart_a = nullptr, *npart_b = nullptr;   // norm statistics handed between decode launches: [NORM_PART_MAX]{sum, sum2}
                                                     // a: of the row in x (attention / final norm), b: of the row in x1 (ffn norm)
    int n_seq = 1, cur_seq = 0;          // KV caches: [seq][layer][n_ctx][d]
    AttnWs attn_ws;                      // many-row prompt attention workspace (allocated with the first eval of >= 2 tokens: ensure_attn_ws)
    GraphCache<int> decode_graphs;                 // keyed by nth * 4096 + seq + (attention schedule << 24)
    // constrained greedy decoding: the sequence's {automaton state, dead} words, the constraints whose tables this handle's owner holds, and the
    // captured steps -- decode_graphs' key with bit 28, per constraint (the step holds the table's address)
    int32_t *d_cst = nullptr;
    float *d_cst_row = nullptr;          // llamahip_eval_topk_constrained: the masked logits row, [n_vocab]
    std::vector<llamahip_constraint *> constraints;
    GraphCache<std::pair<int, const void *>> cst_graphs;
    // asynchronous pipeline-stage steps (llamahip_stage_bind / llamahip_stage_step)
    struct StageSlot {
        int32_t *token_in = nullptr, *token_out = nullptr;     // caller-owned device buffers
        const float *hidden_in = nullptr; float *hidden_out = nullptr;
        // device-side mailboxes (llamahip_stage_mailbox / _connect): this slot's inboxes (owned) and the neighbours' (peer-mapped)
        uint64_t *inbox_hidden = nullptr, *inbox_token = nullptr;     // [n_embd] granules (stages after the first) / 1 granule (first stage)
        uint64_t *peer_hidden = nullptr, *peer_token = nullptr;       // the next stage's hidden inbox / the first stage's token inbox
        bool peer_hidden_ipc = false, peer_token_ipc = false;         // opened with hipIpcOpenMemHandle (closed with the handle)
        bool bound = false;
        int next_pos = 0;                                       // host mirror of the device position (bounds check)
        GraphCache<int> graphs;                                 // keyed by nth + (attention schedule << 16)
    };
    std::vector<StageSlot> slots;        // one per sequence slot
    // batched decode steps over a SET of slots (llamahip_stage_step_set): one captured graph + device-resident row descriptor per set
    struct SetGraph { SeqSet *d_set = nullptr; uint64_t last_use = 0; };      // (d_set: through `own`, released on eviction and on clear)
    GraphCache<std::vector<int>, SetGraph> set_graphs;    // key: {n_threads, slot ids in ascending order}: at most SET_GRAPHS_MAX, least recently used evicted
    uint64_t set_graph_clock = 0;
    int64_t n_set_captures = 0;          // set steps captured (or, with LLAMAHIP_FLAG_NO_GRAPH, set descriptors built) since the load: llamahip_sched_stats
    std::vector<int> last_rows;          // llamahip_stage_logits: row of the caller's i-th slot in the most recent set step (empty: identity)
    float *set_sc = nullptr;             // attention scores of a set step: [SET_MAX][H][n_ctx]
    int32_t *d_slot_state = nullptr;     // [n_seq][2]: {position, step index}, advanced on the device
    int32_t *d_slot_trace = nullptr;     // [n_seq][n_ctx]: tokens picked by the last stage

    // stats
    int64_t weight_bytes = 0, kv_bytes = 0, n_evals = 0;
    double t_load_ms = 0, t_eval_ms = 0;

    // in-process layer pipeline (llamahip_opts.n_devices > 1 or LLAMAHIP_DEVICES; SURVEY.md 8e behind the reference's ONE llama_model_load /
    // llama_eval call, .mm:790, 840): a handle with `stages` is the FRONT -- file, vocab and hparams, no device state of its own -- and every
    // compute entry point walks its stage handles (layers [l0, l1) of stage s on devices[s]), handing the residual stream from one device to
    // the next with hipMemcpyPeerAsync + an event on the producer's stream.  The pipe_* members below live on the STAGE handles.
    std::vector<llamahip_model *> stages;
    float *pipe_in = nullptr;            // rows of the residual stream arriving from the previous stage: [pipe_in_cap][n_embd]
    int pipe_in_cap = 0;
    float *pipe_hout = nullptr;          // decode steps: the row this stage hands on, [n_embd]
    int32_t *pipe_tok = nullptr;         // decode steps: first stage token_in / last stage token_out
    hipEvent_t pipe_ev = nullptr;        // recorded on this stage's stream behind its hand-off (owned by `events`)
    Events events;
    // llamahip_decode_greedy_multi (any handle; on the stages of a pipeline handle): per-slot rows in / out and token words, one event per group of slots
    float *mq_in = nullptr, *mq_out = nullptr;     // [n_seq][n_embd]
    int32_t *mq_tok = nullptr;                     // [n_seq]
    Events mq_ev;
    // llamahip_decode_sample_multi: one pinned, device-mapped block per stage -- the first stage's token words, the last stage's sampler windows,
    // candidates and spilled rows -- and (last stage) the selection workspace of SET_MAX rows
    struct SampleIo { int32_t *tok = nullptr, *n_last = nullptr, *win = nullptr; TopkOut *out = nullptr; float *spill = nullptr; };
    char *smp_blk = nullptr;
    SampleIo smp_h, smp_d;                         // host view / device view: tok [n_seq], n_last [n_seq], win [n_seq][1024], out [n_seq], spill [n_seq][V]
    void *smp_ws = nullptr;                        // SET_MAX * TOPK_WS_BYTES, zeroed once (the selection leaves it zeroed)
    int pipe_hand_off = 0;               // (front) llamahip_stats.hand_off
    // llamahip_eval_multi (on the stages of a pipeline handle): the pass's row table, device resident -- RowTab [rows_cap] | the rows of the short
    // segments [rows_cap] | the segments' last rows [n_seq] -- and the host copy it is uploaded from
    char *d_rows = nullptr;
    int rows_cap = 0;
    std::vector<char> h_rows;
    // llamahip_sched_*: the one scheduler that owns KV slots of this handle (the front of a pipeline handle), and on the last stage its
    // k_sched_pick table {emit, slot, position, cursor} [SET_MAX] | res [SET_MAX]
    lh::SchedDev *sched = nullptr;
    int32_t *d_sched_tab = nullptr;

    ~llamahip_model();
};

// A pipeline mailbox is polled by this GPU's kernels while ANOTHER GPU's kernel stores into it over xGMI.  Ordinary hipMalloc
// memory is coarse-grained: the local L2 may keep serving a line it cached on an earlier look, and coherence with other agents is
// only promised at kernel boundaries.  Uncached (else fine-grained) device memory is what in-kernel flags between GPUs need;
// both can be exported with hipIpcGetMemHandle like any device allocation.
static hipError_t malloc_mailbox(void **p, size_t bytes) {
    if (hipExtMallocWithFlags(p, bytes, hipDeviceMallocUncached) == hipSuccess) return hipSuccess;
    (void) hipGetLastError();
    if (hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained) == hipSuccess) return hipSuccess;
    (void) hipGetLastError();
    // no coarse-grained fall-back: such an inbox could pass a one-token handshake and serve a stale line later in the run -- the caller
    // gets an error, reports "mailboxes unavailable" and the pipeline keeps its RCCL hand-off
    return hipErrorNotSupported;
}
// DevOwner's allocator in the library, by kind; the zero fill is the synchronous one
int lh::dev_alloc_default(void **p, size_t bytes, int kind, bool zero) {
    *p = nullptr;
    hipError_t e = kind == MEM_PINNED ? hipHostMalloc(p, bytes, hipHostMallocMapped) : kind == MEM_MAILBOX ? malloc_mailbox(p, bytes) : hipMalloc(p, bytes);
    if (e == hipSuccess && zero) {
        if (kind == MEM_PINNED) memset(*p, 0, bytes);
        else if ((e = hipMemset(*p, 0, bytes)) != hipSuccess) { dev_release_default(*p, kind); *p = nullptr; }
    }
    return (int) e;
}
void lh::dev_release_default(void *p, int kind) {
    if (kind == MEM_PINNED) (void) hipHostFree(p);
    else (void) hipFree(p);
}

llamahip_model::~llamahip_model() {
    if (sched) lh::sched_dev_orphan(sched);          // (a scheduler that outlives its handle: every later call on it fails, none touches the handle)
    for (llamahip_constraint *c : constraints) { c->dev = nullptr; c->dev_release = nullptr; }      // (the tables go with `own`)
    for (llamahip_model *st : stages) delete st;
    if (host_only) return;
    (void) hipSetDevice(device);
    (void) hipDeviceSynchronize();      // captured steps may still run on a caller's stream: nothing is freed or destroyed under them
    for (auto &sl : slots) {
        if (sl.peer_hidden && sl.peer_hidden_ipc) (void) hipIpcCloseMemHandle(sl.peer_hidden);
        if (sl.peer_token && sl.peer_token_ipc) (void) hipIpcCloseMemHandle(sl.peer_token);
    }
    if (stream) (void) hipStreamDestroy(stream);
}

namespace {

// upload one Q4_0 tensor (file layout) and repack it into rows [row0, row0 + M) of `dst`
int upload_q4(llamahip_model *m, const std::string &name, QMat &dst, int row0, uint8_t *d_stage, std::vector<uint8_t> &h_stage,
              char *err, size_t err_cap, int gmap = 0, int goff = 0) {
    const TensorInfo &t = m->file.tensors.at(name);
    h_stage.resize((size_t) t.nbytes());
    std::string e;
    if (!m->file.read_tensor(name, h_stage.data(), e)) { set_err(err, err_cap, "%s", e.c_str()); return LLAMAHIP_ERR_LOAD; }
    HIP_TRY(hipMemcpyAsync(d_stage, h_stage.data(), h_stage.size(), hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_LOAD);
    uint8_t *out = dst.tiles + (size_t) (row0 / 8) * (dst.nchunks + 1) * TILE_BYTES;
    HIP_TRY(launch_repack(d_stage, out, (int) t.ne1, (int) t.ne0, gmap, goff, m->stream), LLAMAHIP_ERR_LOAD);
    HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_LOAD);      // h_stage / d_stage are reused
    return 0;
}

// f16 / f32 model files: one tensor, merged, copied as it is into rows [row0, row0 + ne1) of `dst`
int upload_dense(llamahip_model *m, const std::string &name, DMat &dst, int row0, std::vector<uint8_t> &h_stage, char *err, size_t err_cap) {
    const TensorInfo &t = m->file.tensors.at(name);
    h_stage.resize((size_t) t.nbytes());
    std::string e;
    if (!m->file.read_tensor(name, h_stage.data(), e)) { set_err(err, err_cap, "%s", e.c_str()); return LLAMAHIP_ERR_LOAD; }
    // the raw rows on the device for the length of this call (released on every return path)
    DevOwner staging;
    uint8_t *d_raw = nullptr;
    HIP_TRY(staging.alloc(&d_raw, h_stage.size()), LLAMAHIP_ERR_LOAD);
    HIP_TRY(hipMemcpy(d_raw, h_stage.data(), h_stage.size(), hipMemcpyHostToDevice), LLAMAHIP_ERR_LOAD);
    hipError_t e1;
    if (dst.wtype == 3) {
        // Q4_1: regroup the rows into [row-block of 64][block][lane] (dense.hip); row0 is a multiple of 64
        DMat view = dst;
        const size_t at = (size_t) (row0 / 64) * (dst.K / 32) * 64;
        view.w = (uint8_t *) dst.w + at * 8; view.w2 = (uint8_t *) dst.w2 + at * 16; view.M = (int) t.ne1;
        e1 = launch_q41_repack(d_raw, view, m->stream);
    } else {
        // f16 / f32: rows into the chain-major order the dense mat-mul reads (dense.hip perm_index)
        e1 = launch_dense_perm_rows(d_raw, dst, row0, (int) t.ne1, m->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(m->stream);      // (also after a failed launch: d_raw goes with this call)
    HIP_TRY(e1, LLAMAHIP_ERR_LOAD);
    HIP_TRY(e2, LLAMAHIP_ERR_LOAD);
    return 0;
}

int alloc_dmat(DMat &q, int M, int K, llamahip_model *m, char *err, size_t err_cap) {
    q.M = M; q.K = K; q.wtype = m->hp.f16;
    HIP_TRY(m->own.alloc(&q.w, q.bytes()), LLAMAHIP_ERR_LOAD);
    if (q.bytes2()) HIP_TRY(m->own.alloc(&q.w2, q.bytes2()), LLAMAHIP_ERR_LOAD);
    m->weight_bytes += (int64_t) (q.bytes() + q.bytes2());
    return 0;
}

int alloc_qmat(QMat &q, int M, int K, llamahip_model *m, char *err, size_t err_cap) {
    q.set_shape(M, K);
    HIP_TRY(m->own.alloc(&q.tiles, q.bytes()), LLAMAHIP_ERR_LOAD);
    m->weight_bytes += (int64_t) q.bytes();
    return 0;
}

// The two extra resident copies of a layer matrix that the many-row prompt GEMMs read: row-lane tiles
// (k_gemm_rows) and matrix-core tiles (k_gemm_mfma), both derived on the device from the decode tiles.  They are
// built LAZILY, by the first eval of more than 60 rows (shorter evals -- the reference's 9-token prompt chunks -- and
// decode run on the decode tiles alone): a handle that only ever decodes keeps one copy of its weights (7B: 4.4 GB
// instead of 13 GB).  LLAMAHIP_FLAG_NO_PREFILL_COPY never builds them (the LDS-staged GEMM then serves long
// prompts); LLAMAHIP_EAGER_PREFILL_COPY=1 builds them at load time (measurement: keeps the first long eval's
// time free of the 10-20 ms build).
// The extra weight layouts of the prompt path, built lazily.  Returns 0 when the copies of `q` exist afterwards, 1 when device memory
// ran out or a conversion launch failed: whatever was allocated for `q` is released again and its pointers stay null (launch_gemm
// then takes the bit-identical LDS-staged kernel for this matrix) -- a pointer is only published after its conversion launch succeeded.
int make_rows(QMat &q, llamahip_model *m) {
    if (m->flags & LLAMAHIP_FLAG_NO_PREFILL_COPY) return 0;
    auto build = [&](uint8_t **slot, size_t bytes, auto convert) -> bool {
        if (*slot) return true;
        if (m->own.alloc(slot, bytes) != 0) { (void) hipGetLastError(); return false; }      // (the conversion launchers read the destination from the QMat)
        if (convert() != hipSuccess) { (void) hipGetLastError(); m->own.release(slot); return false; }
        m->weight_bytes += (int64_t) bytes;
        return true;
    };
    if (!build(&q.rows, q.rows_bytes(), [&]() { return launch_tiles_to_rows(q, m->stream); })) return 1;
    // matrix-core tiles: one byte per weight in four-chain operand order for the exact path (k_gemm_mfma4); the int8 order only for a
    // handle opened with LLAMAHIP_FLAG_FAST_PREFILL (or LLAMAHIP_MFMA_I8=1: the round-1 exact kernel, for A/B) -- one of the two
    static const bool want_i8 = getenv("LLAMAHIP_MFMA_I8") != nullptr;
    if ((m->flags & LLAMAHIP_FLAG_FAST_PREFILL) || want_i8) {
        if (!build(&q.mt, q.mt_bytes(), [&]() { return launch_tiles_to_mtiles(q, m->stream); })) return 1;
    } else if (!build(&q.mt4, q.mt4_bytes(), [&]() { return launch_tiles_to_mt4(q, m->stream); })) return 1;
    return 0;
}
constexpr int PROMPT_COPY_MIN_ROWS = 61;       // evals up to 60 rows take k_gemv_set on the decode tiles
int ensure_prompt_copies(llamahip_model *m, int N, char *err, size_t err_cap) {
    if (N < PROMPT_COPY_MIN_ROWS || m->dense || m->prompt_copies || (m->flags & LLAMAHIP_FLAG_NO_PREFILL_COPY)) return 0;
    (void) err; (void) err_cap;
    for (Layer &L : m->layers)
        for (QMat *q : { &L.qkv, &L.wo, &L.w13, &L.w2 })
            if (make_rows(*q, m)) {
                // out of device memory (the copies triple the resident weights): remember it as if the handle had been opened with
                // LLAMAHIP_FLAG_NO_PREFILL_COPY -- matrices that already have their copies keep using them, the rest run the
                // LDS-staged kernel on the decode tiles, every later long eval goes straight there instead of failing again
                m->flags |= LLAMAHIP_FLAG_NO_PREFILL_COPY;
                return 0;
            }
    m->prompt_copies = true;
    return 0;
}
// The lm head over EVERY row (llamahip_eval_logprobs / llamahip_perplexity) is a long-prompt GEMM of its own (7B: 32 000 x 4 096): from
// 64 rows it gets `output`'s copies too, built once, by the same code, so that it can take k_gemm_mfma4.  Out of device memory: it keeps
// the decode-tile kernels (bit-identical).  llamahip_eval / _chunks / _debug never build or read them (Pass::score_rows).
constexpr int OUTPUT_COPY_MIN_ROWS = 64;
void ensure_output_copies(llamahip_model *m, int N) {
    if (N < OUTPUT_COPY_MIN_ROWS || m->dense || m->output_copies_tried || (m->flags & LLAMAHIP_FLAG_NO_PREFILL_COPY)) return;
    m->output_copies_tried = true;
    (void) make_rows(m->output, m);
}

int upload_f32(llamahip_model *m, const std::string &name, float **dst, char *err, size_t err_cap) {
    const TensorInfo &t = m->file.tensors.at(name);
    std::vector<uint8_t> h((size_t) t.nbytes());
    std::string e;
    if (!m->file.read_tensor(name, h.data(), e)) { set_err(err, err_cap, "%s", e.c_str()); return LLAMAHIP_ERR_LOAD; }
    HIP_TRY(m->own.alloc((void **) dst, h.size()), LLAMAHIP_ERR_LOAD);
    HIP_TRY(hipMemcpy(*dst, h.data(), h.size(), hipMemcpyHostToDevice), LLAMAHIP_ERR_LOAD);
    return 0;
}

void drop_set_graphs(llamahip_model *m) {
    for (auto &kv : m->set_graphs.map) m->own.release(&kv.second.d_set);
    m->set_graphs.clear();
}
// the slot tables: {position, step} and the picks of every KV slot, with the host's slot records behind them
int ensure_slots(llamahip_model *m, char *err, size_t err_cap) {
    if (m->d_slot_state) return 0;
    HIP_TRY(m->own.alloc_all({ { &m->d_slot_state, (size_t) m->n_seq * 2 * sizeof(int32_t) },
                               { &m->d_slot_trace, (size_t) m->n_seq * m->hp.n_ctx * sizeof(int32_t) } }), LLAMAHIP_ERR_PREDICT);
    m->slots.resize(m->n_seq);
    return 0;
}
// the attention scores of a set step: [SET_MAX][H][n_ctx]
int ensure_set_sc(llamahip_model *m, char *err, size_t err_cap) {
    if (!m->set_sc) HIP_TRY(m->own.alloc(&m->set_sc, (size_t) SET_MAX * m->hp.n_head * m->hp.n_ctx), LLAMAHIP_ERR_PREDICT);
    return 0;
}
// The one capture path: the launches of a step (`body` issues them on m->stream and returns the project's code) recorded into an executable
// graph.  The capture is always ended and the hipGraph_t destroyed on every path.  Returns the body's code if that is non-zero, else
// LLAMAHIP_ERR_PREDICT with the HIP text on a runtime error; *exec is set on success only.
template <class Body> int capture_step(llamahip_model *m, Body body, hipGraphExec_t *exec, char *err, size_t err_cap) {
    *exec = nullptr;
    HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal), LLAMAHIP_ERR_PREDICT);
    const int rc = body();
    hipGraph_t graph = nullptr;
    hipGraphExec_t made = nullptr;
    hipError_t e = hipStreamEndCapture(m->stream, &graph);
    if (!rc && e == hipSuccess) e = hipGraphInstantiate(&made, graph, nullptr, nullptr, 0);
    if (graph) (void) hipGraphDestroy(graph);
    if (rc) return rc;
    HIP_TRY(e, LLAMAHIP_ERR_PREDICT);
    *exec = made;
    return 0;
}
int ensure_workspace(llamahip_model *m, int N, char *err, size_t err_cap) {
    if (N <= m->ws_cap) return 0;
    // captured graphs hold the old workspace pointers -- and they are launched on the CALLER's stream (llamahip_stage_step /
    // _step_set), so the handle's own stream says nothing about them: wait for the device before an exec or a buffer goes
    HIP_TRY(hipDeviceSynchronize(), LLAMAHIP_ERR_PREDICT);
    drop_set_graphs(m);
    m->decode_graphs.clear();
    m->cst_graphs.clear();
    for (auto &sl : m->slots) sl.graphs.clear();
    const HParams &hp = m->hp;
    const size_t d = hp.n_embd, F = hp.n_ff, V = hp.n_vocab, C = hp.n_ctx, H = hp.n_head;
    const size_t KpMax = ((std::max(d, F) + 255) / 256) * 256;
    float **bufs[] = { &m->x, &m->x1, &m->qkv, &m->qr, &m->merged, &m->gu, &m->tmp, &m->logits, &m->qa_d, &m->dbg_y, &m->dbg_p, &m->dbg_kqv };
    for (auto b : bufs) m->own.release(b);
    m->own.release(&m->qa_A);
    m->own.release(&m->qb_ws);
    m->own.release(&m->d_tokens);
    m->ws_cap = 0;
    const size_t n = (size_t) N;
    HIP_TRY(m->own.alloc_all({ { &m->d_tokens, n * 4 }, { &m->x, n * d * 4 }, { &m->x1, n * d * 4 }, { &m->qkv, n * 3 * d * 4 }, { &m->qr, n * d * 4 },
                               { &m->merged, n * d * 4 }, { &m->gu, n * 2 * F * 4 }, { &m->tmp, n * std::max(d, F) * 4 }, { &m->logits, n * V * 4 },
                               { &m->qa_A, n * KpMax }, { &m->qa_d, n * (KpMax / 32) * 4 },
                               { &m->qb_ws, n * KpMax * 2 },      // fp16 (or int8) operand of the matrix-core GEMM
                               { &m->dbg_y, n * std::max(d, F) * 4 }, { &m->dbg_p, H * n * C * 4 }, { &m->dbg_kqv, n * d * 4 } }), LLAMAHIP_ERR_PREDICT);
    if (!m->qaF_A) {
        const size_t KpF = ((F + 255) / 256) * 256;
        HIP_TRY(m->own.alloc_all({ { &m->qaF_A, 64 * KpF, true }, { &m->qaF_d, 64 * (KpF / 32) * 4, true } }), LLAMAHIP_ERR_PREDICT);
    }
    m->ws_cap = N;
    return 0;
}

// the score workspace of the multi-row prompt attention: [n_head][n_ctx][NB] fp32, NB = 512 query rows
// (a 2 048-token 7B eval with NB = 256 / 512 / 1 024 / 2 048: 225.9 / 201.8 / 200.3 / 212.4 ms on one box in round 3, 183.3 / 161.6 / 162.6 / 175.9 in
// round 4 (profiles/r04_v_attn_shapes_ab.txt) -- 512 keeps the workspace at a quarter and inside the Infinity Cache)
// per batch (7B, n_ctx 2560: 168 MB), allocated with the first multi-token eval
int ensure_attn_ws(llamahip_model *m, int N, char *err, size_t err_cap) {
    if (N < 2 || m->attn_ws.S) return 0;
    AttnWs &w = m->attn_ws;
    attn_ws_shape(w, m->hp.n_ctx);
    const AttnWsBytes b = attn_ws_bytes(w, m->hp.n_head);
    HIP_TRY(m->own.alloc_all({ { &w.S, b.S }, { &w.pmax, b.pmax }, { &w.inv, b.inv }, { &w.part, b.part } }), LLAMAHIP_ERR_PREDICT);
    return 0;
}

// a pinned, device-mapped host block and its device alias: both or neither
template <class T> hipError_t alloc_pinned(llamahip_model *m, T **host, T **dev, size_t bytes) {
    *dev = nullptr;
    hipError_t e = (hipError_t) m->own.alloc_all({ { host, bytes, true, MEM_PINNED } });
    if (e == hipSuccess && (e = hipHostGetDevicePointer((void **) dev, *host, 0)) != hipSuccess) { m->own.release(host); *dev = nullptr; }
    return e;
}

struct DumpSink {
    float *dump = nullptr;
    int64_t cap = 0, used = 0;
    int64_t *sizes = nullptr;
    hipStream_t st = nullptr;
    bool put(int idx, const float *dev, int64_t count) {
        if (!dump || !sizes) return true;
        if (used + count > cap) return true;        // silently truncated, size stays 0
        if (hipMemcpyAsync(dump + used, dev, (size_t) count * 4, hipMemcpyDeviceToHost, st) != hipSuccess) return false;
        if (hipStreamSynchronize(st) != hipSuccess) return false;
        sizes[idx] = count;
        used += count;
        return true;
    }
};

// What a forward pass for N tokens at n_past on this handle's layers (.mm:510-735) is told.  The caller fills the fields by name; the ones it
// leaves alone mean this handle's own token buffer, position words, current KV slot and stream.  Nothing of a pass is kept on the handle.
struct Pass {
    explicit Pass(const llamahip_model *m) : tokens(m->d_tokens), seq(m->cur_seq), stream(m->stream), state(m->d_state) {}
    int n_threads = 1, n_past = 0, N = 1;
    const float *hidden_in = nullptr;   // device fp32 [N][d] residual stream from the previous stage (nullptr on the first stage)
    bool want_all = false;              // logits for every token (debug, scoring) instead of only the last (.mm:724-725)
    bool score_rows = false;            // ... by the scoring entry points: the all-rows lm head takes `output`'s prompt copies
    int chunk = 0;                      // > 0: the rows are the evals of `chunk` tokens of llamahip_eval_chunks in one pass
    // an embedding pass (llamahip_text_embedding): no lm head, no logits; in its place the final norm of rows embed_first .. N - 1 as fp32 rows
    // into embed_y (null: nothing at all -- a chunk of a LAST-pooled text that is not its last)
    bool embed = false;
    float *embed_y = nullptr;
    int embed_first = 0;
    int dump_layer = -1; DumpSink *sink = nullptr;      // per-layer dumps (llamahip_eval_debug): both or neither
    const int32_t *tokens;              // device: where the embedding kernel finds the N tokens
    int seq;                            // KV slot
    hipStream_t stream;
    // ---- single-token steps only
    bool state_on_device = false;       // the position words are current (a captured / device-driven step); else n_past is published first
    int attn_sched = 0;                 // decode attention schedule (attn_sched_at): 0 fused, 1 two launches, 2 long-context
    // device-side endpoints of a stage step: the position words, and the residual-stream buffers read by the first / written by the
    // last layer of this stage in place of m->x (no staging copies)
    int32_t *state;
    const float *x_first = nullptr; float *x_last = nullptr;
    // device-side mailboxes instead of x_first / x_last / tokens (tagged granules, see MailboxIO)
    const uint64_t *mb_in = nullptr, *mb_token = nullptr;
    uint64_t *mb_out = nullptr;
    // the device-resident greedy loop: the lm head's launch also picks the token, advances the position and embeds the pick for the
    // next step (EPI_STORE_PICK); the step then starts from the row the previous step (or the caller) left in x / npart_a
    bool fold_pick = false;
    int32_t *pick_out = nullptr, *pick_next = nullptr;
};

// dense model files: activation preparation + mat-mul of `rows` rows.  f16 / f32 weights: launch_dense_act writes the rounded, permuted rows
// straight into the mat-mul's operand buffer (one fused launch, or launch_prep's fp32 rows + k_dense_perm_act where a NORM row is too wide for
// it); Q4_1: fp32 rows, expanded by the mat-mul itself.
static hipError_t dense_prep_mm(llamahip_model *m, const DMat &w, int epi, int mode, const float *in0, const float *in1, long in_stride, long in1_stride,
                                int K, int rows, float *out, long out_stride, const float *resid, long resid_stride, hipStream_t st) {
    if (w.wtype != 3) {                                    // fused where it applies, else split: launch_dense_act's rule (dense.hip)
        hipError_t e = launch_dense_act(DENSE_PREP_AUTO, mode, w.wtype, in0, in1, in_stride, in1_stride, K, rows, m->tmp, m->dbg_y, m->qa_A, m->qa_d, m->T_silu, st);
        if (e != hipSuccess) return e;
        return launch_dense_mm(w, epi, nullptr, K, rows, out, out_stride, resid, resid_stride, st, m->tmp);
    }
    const float *src = in0;
    long src_stride = in_stride;
    if (mode != PREP_PLAIN) {
        hipError_t e = launch_prep(mode, in0, in1, in_stride, in1_stride, K, rows, m->qa_A, m->qa_d, m->dbg_y, nullptr, m->T_silu, st);      // fp32 activations of the mat-mul: [rows][max(d, F)]
        if (e != hipSuccess) return e;
        src = m->dbg_y; src_stride = K;
    }
    return launch_dense_mm(w, epi, src, src_stride, rows, out, out_stride, resid, resid_stride, st, m->tmp);
}

// f16 / f32 model files: the same graph with dense mat-muls (dense.hip).  Un-fused:
// norm -> fp32 activations -> dense mat-mul; RoPE, KV cache and attention are the Q4_0 path's kernels.
// (single-row steps: the token word and the {position, step} words of a stage step -- llamahip_stage_step on a whole-model handle)
// chunk > 0: norm, RoPE and the mat-muls work row by row, the attention splits every row's keys as its own eval would (launch_attn)
int forward_dense(llamahip_model *m, const Pass &p, char *err, size_t err_cap) {
    const HParams &hp = m->hp;
    const int d = hp.n_embd, F = hp.n_ff, H = hp.n_head, dh = d / H, C = hp.n_ctx, V = hp.n_vocab;
    const int nth = clamp_threads(p.n_threads), n_past = p.n_past, N = p.N;
    hipStream_t st = p.stream;
    // the decode attention kernels read the position from device memory; only state[0] is written here (state[1], the step counter of the
    // greedy loop, belongs to k_argmax)
    if (N == 1 && !p.state_on_device) HIP_TRY(hipMemcpyAsync(m->d_state, &p.n_past, sizeof(int32_t), hipMemcpyHostToDevice, st), LLAMAHIP_ERR_PREDICT);
    if (m->first_stage) HIP_TRY(launch_embed_dense(p.tokens, m->tok_emb, hp.f16, m->x, d, N, st), LLAMAHIP_ERR_PREDICT);     // .mm:558-561
    else HIP_TRY(hipMemcpyAsync(m->x, p.hidden_in, (size_t) N * d * 4, hipMemcpyDeviceToDevice, st), LLAMAHIP_ERR_PREDICT);
    auto prep_mm = [&](const DMat &w, int epi, int mode, const float *in0, const float *in1, long in_stride, long in1_stride,
                       int K, int rows, float *out, long out_stride, const float *resid, long resid_stride) -> hipError_t {
        return dense_prep_mm(m, w, epi, mode, in0, in1, in_stride, in1_stride, K, rows, out, out_stride, resid, resid_stride, st);
    };
    for (int il = m->l0; il < m->l1; il++) {
        const Layer &L = m->layers[il - m->l0];
        const size_t kv_at = ((size_t) p.seq * (m->l1 - m->l0) + (il - m->l0)) * C * d;
        float *Kl = m->Kc + kv_at, *Vl = m->Vc + kv_at;
        HIP_TRY(prep_mm(L.dqkv, EPI_STORE, PREP_NORM, m->x, L.attention_norm, d, 0, d, N, m->qkv, 3L * d, nullptr, 0), LLAMAHIP_ERR_PREDICT);             // .mm:570-582
        if (N == 1) {
            // one row: the decode attention kernels of the Q4_0 path (position from device memory, fp32 output)
            HIP_TRY(launch_dec_attn(m->qkv, d, H, C, nth, m->sincos, Kl, Vl, m->sc, m->part, m->merged, m->qa1_A, m->qa1_d, m->T_exp, p.state, st, m->d_attn_sync, m->d_fault), LLAMAHIP_ERR_PREDICT);
        } else {
            HIP_TRY(launch_rope_kv(m->qkv, 3L * d, d, dh, m->sincos, m->qr, Kl, Vl, n_past, N, st), LLAMAHIP_ERR_PREDICT);                             // .mm:586-611
            HIP_TRY(launch_attn(m->qr, Kl, Vl, m->merged, nullptr, nullptr, n_past, N, d, H, nth, m->T_exp, &m->attn_ws, st, p.chunk), LLAMAHIP_ERR_PREDICT); // .mm:614-646
        }
        HIP_TRY(prep_mm(L.dwo, EPI_RESID, PREP_PLAIN, m->merged, nullptr, d, 0, d, N, m->x1, d, m->x, d), LLAMAHIP_ERR_PREDICT);                          // .mm:649-654
        HIP_TRY(prep_mm(L.dw13, EPI_STORE, PREP_NORM, m->x1, L.ffn_norm, d, 0, d, N, m->gu, 2L * F, nullptr, 0), LLAMAHIP_ERR_PREDICT);                  // .mm:660-675
        HIP_TRY(prep_mm(L.dw2, EPI_RESID, PREP_SILU_MUL, m->gu, m->gu + F, 2L * F, 2L * F, F, N, m->x, d, m->x1, d), LLAMAHIP_ERR_PREDICT);               // .mm:678-687
    }
    if (m->last_stage && p.embed) {
        if (p.embed_y) HIP_TRY(launch_norm_rows_f32(m->x + (size_t) p.embed_first * d, m->norm_w, d, N - p.embed_first, p.embed_y, st), LLAMAHIP_ERR_PREDICT);
    } else if (m->last_stage) {
        const size_t r0 = p.want_all ? 0 : N - 1;      // every row, or only the last
        HIP_TRY(prep_mm(m->doutput, EPI_STORE, PREP_NORM, m->x + r0 * d, m->norm_w, d, 0, d, N - (int) r0, m->logits + r0 * V, V, nullptr, 0), LLAMAHIP_ERR_PREDICT);
    }
    return 0;
}

// The decode attention schedule by position (a host-side fact at every entry point: n_past, or the slot's next position; graphs are
// captured per schedule):
//   0  wq|wk|wv + attention in one launch (k_qkv_attn)                                        short contexts
//   1  mat-vec, k_dec_scores, k_dec_pv_blk (three launches)                                   from LLAMAHIP_ATTN_TWO_FROM
//   2  mat-vec, k_dec_scores, k_dec_pv_stream (V through LDS, every thread of the chip loading) from LLAMAHIP_ATTN_LONG_FROM
// Defaults are the measured crossovers (profiles/r03_attn_by_context.txt): the fused launch's attention workgroups wait inside the
// launch, which costs more the longer the context; how soon depends on how many of them there are (H dh/32).  -1 = never.
static int attn_sched_at(const llamahip_model *m, int pos) {
    static const int env_two = getenv("LLAMAHIP_ATTN_TWO_FROM") ? atoi(getenv("LLAMAHIP_ATTN_TWO_FROM")) : -2;
    static const int env_long = getenv("LLAMAHIP_ATTN_LONG_FROM") ? atoi(getenv("LLAMAHIP_ATTN_LONG_FROM")) : -2;
    const int W = m->hp.n_embd / 32;                        // soft_max . V workgroups per launch: 128 (7B), 160 (13B), 256 (65B)
    const int two_from = env_two != -2 ? env_two : (W <= 128 ? -1 : W < 256 ? 544 : 448);
    const int long_from = env_long != -2 ? env_long : (W <= 128 ? 1280 : W < 256 ? 1600 : 2048);
    if (long_from >= 0 && pos >= long_from) return 2;
    if (two_from >= 0 && pos >= two_from) return 1;
    return 0;
}
// The fused single-token step of a Q4_0 handle: activation preparation lives in GEMV prologues / producer epilogues (four launches per
// layer), the context position is read from p.state by the attention kernels.
int forward_decode(llamahip_model *m, const Pass &p, char *err, size_t err_cap) {
    const HParams &hp = m->hp;
    const int d = hp.n_embd, F = hp.n_ff, H = hp.n_head, C = hp.n_ctx, V = hp.n_vocab;
    const int nth = clamp_threads(p.n_threads);
    hipStream_t st = p.stream;
    int32_t *state = p.state;
    const bool has_layers = m->l1 > m->l0, tagged = has_layers && m->l1 - m->l0 <= TAG_MAX_LAYERS;      // (tags are (epoch, layer))
    const int32_t hs[2] = { p.n_past, 0 };      // host-driven single-token eval: publish the position to the device-resident state
    if (!p.state_on_device) HIP_TRY(hipMemcpyAsync(m->d_state, hs, sizeof(hs), hipMemcpyHostToDevice, st), LLAMAHIP_ERR_PREDICT);
    const float *x_first = has_layers ? p.x_first : nullptr;
    float *x_last = has_layers ? p.x_last : nullptr;
    // the producer of every residual-stream row (embedding, wo and w2 mat-vecs) hands {sum, sum of squares} of the row to the norm-fused mat-vec
    // that consumes it, which then needs no reduction of its own (k_gemv PREP_NORMP).  LLAMAHIP_NORM_MODE=0 / 1: self-contained prologues (measurement only).
    const bool use_part = m->w13_interleaved && norm_mode_resolve();
    int n_part_x = 0;                                       // pairs in npart_a valid for the row currently in x (0: none)
    // wq|wk|wv + attention as one launch with tagged hand-offs (k_qkv_attn); one forward pass = one epoch
    // (long contexts: soft_max . V is a bandwidth problem of its own there -- separate mat-vec, k_dec_scores, k_dec_pv_stream)
    const bool long_attn = p.attn_sched == 2 && pv_stream_applies((int) (d / H), (int) C, nth);
    const bool two_attn = p.attn_sched == 1 || (p.attn_sched == 2 && !long_attn);
    const bool use_qkvx = !long_attn && !two_attn && m->d_attn_sync && tagged && qkv_attn_applies(m->layers[0].qkv, d, H, nth);
    const bool pv_split = long_attn && m->d_pvx && m->l1 - m->l0 <= TAG_MAX_LAYERS;
    // w1|w3 in half-block workgroups (balanced over the CUs; the halves of a block exchange their amax inside one XCD): needs the XCD
    // placement the load-time self-test confirmed (d_attn_sync) and the epoch for its tags
    const bool use_w13h = m->w13_interleaved && m->d_attn_sync && m->d_w13_amax && tagged && gemv_silu_half_applies(m->layers[0].w13);
    const bool use_epoch = use_qkvx || pv_split || use_w13h;
    if (use_epoch && !(m->first_stage && use_part)) HIP_TRY(launch_bump_epoch(m->d_epoch, st), LLAMAHIP_ERR_PREDICT);
    if (p.mb_token && m->first_stage && !use_part) { set_err(err, err_cap, "pipeline mailboxes need the default norm-statistics mode (LLAMAHIP_NORM_MODE unset)"); return LLAMAHIP_ERR_PREDICT; }
    const bool fold = p.fold_pick && use_part && m->first_stage && m->last_stage;
    if (m->first_stage && fold) {
        n_part_x = 1;               // x, npart_a and the epoch were left by the previous step's lm head (or by decode_greedy's first embedding launch)
    } else if (m->first_stage) {
        if (use_part) {
            HIP_TRY(launch_embed_part(p.tokens, m->tok_emb, m->x, d, m->npart_a, st, use_epoch ? m->d_epoch : nullptr, nullptr, p.mb_token, state, m->d_fault, V), LLAMAHIP_ERR_PREDICT);
            n_part_x = 1;
        } else
        HIP_TRY(launch_embed(p.tokens, m->tok_emb, m->x, d, 1, st), LLAMAHIP_ERR_PREDICT);      // .mm:558-561
    } else if (!x_first && !p.mb_in) {
        HIP_TRY(hipMemcpyAsync(m->x, p.hidden_in, (size_t) d * 4, hipMemcpyDeviceToDevice, st), LLAMAHIP_ERR_PREDICT);
    }
    // pipeline mailboxes: the first layer's row arrives / the last layer's row leaves as tagged granules
    static const int mb_test = getenv("LLAMAHIP_HANDOFF_FAULT_TEST") ? atoi(getenv("LLAMAHIP_HANDOFF_FAULT_TEST")) : 0;      // 3: the last layer publishes a tag nobody waits for (test only)
    MailboxIO mb_first, mb_last;
    const bool has_mb_in = p.mb_in && has_layers, has_mb_out = p.mb_out && has_layers;
    if (has_mb_in) { mb_first.in_t = p.mb_in; mb_first.resid_t = p.mb_in; mb_first.pos_w = state; mb_first.epoch = m->d_epoch; mb_first.fault = m->d_fault; mb_first.test_bits = mb_test ? 0x1000 : 0; }
    if (has_mb_out) { mb_last.out_t = p.mb_out; mb_last.pos_w = state; mb_last.epoch = m->d_epoch; mb_last.fault = m->d_fault; mb_last.test_bits = mb_test == 3 ? 0x2000 : 0; }

    for (int il = m->l0; il < m->l1; il++) {
        const Layer &L = m->layers[il - m->l0];
        const size_t kv_at = ((size_t) p.seq * (m->l1 - m->l0) + (il - m->l0)) * C * d;
        float *Kl = m->Kc + kv_at, *Vl = m->Vc + kv_at;
        const float *xa = (il == m->l0 && x_first) ? x_first : m->x;      // residual stream into this layer
        float *xo = (il == m->l1 - 1 && x_last) ? x_last : m->x;           // ... and out of it
        NormPart np_qkv, np_wo, np_w13, np_w2;
        if (use_part) {
            const int pw = gemv_resid_parts(L.wo), p2 = gemv_resid_parts(L.w2);
            if (n_part_x > 0) { np_qkv.in = m->npart_a; np_qkv.n_in = n_part_x; }
            if (pw > 0 && pw <= NORM_PART_MAX) { np_wo.out = m->npart_b; np_w13.in = m->npart_b; np_w13.n_in = pw; }
            n_part_x = 0;
            if (p2 > 0 && p2 <= NORM_PART_MAX) { np_w2.out = m->npart_a; n_part_x = p2; }
        }
        // (mailboxes: the first layer reads its row -- norm input and residual operand -- from the tagged inbox, the last layer's w2
        //  stores its row into the next stage's inbox; everything in between is the usual schedule)
        const MailboxIO *mbi = (has_mb_in && il == m->l0) ? &mb_first : nullptr, *mbo = (has_mb_out && il == m->l1 - 1) ? &mb_last : nullptr;
        if (use_qkvx) {
            HIP_TRY(launch_qkv_attn(L.qkv, xa, L.attention_norm, np_qkv, m->d_qkv2, m->d_sc2, m->d_epoch, il - m->l0, d, H, C, nth, m->sincos, Kl, Vl, nullptr,
                                    m->qa1_A, m->qa1_d, m->T_silu, m->T_exp, state, m->d_fault, st, mbi), LLAMAHIP_ERR_PREDICT);
        } else {
            HIP_TRY(launch_gemv(L.qkv, PREP_NORM, EPI_STORE, nullptr, nullptr, xa, L.attention_norm, m->qkv, nullptr, m->T_silu, nullptr, nullptr, st, &np_qkv, mbi), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(launch_dec_attn(m->qkv, d, H, C, nth, m->sincos, Kl, Vl, m->sc, m->part, nullptr, m->qa1_A, m->qa1_d, m->T_exp, state, st, two_attn ? nullptr : m->d_attn_sync, m->d_fault, long_attn,
                                    pv_split ? m->d_pvx : nullptr, m->d_epoch, il - m->l0), LLAMAHIP_ERR_PREDICT);
        }
        HIP_TRY(launch_gemv(L.wo, PRE_QA, EPI_RESID, m->qa1_A, m->qa1_d, nullptr, nullptr, m->x1, xa, m->T_silu, nullptr, nullptr, st, &np_wo, mbi), LLAMAHIP_ERR_PREDICT);
        if (m->w13_interleaved) {
            if (use_w13h) HIP_TRY(launch_gemv_silu_half(L.w13, m->x1, L.ffn_norm, m->T_silu, m->qa2_A, m->qa2_d, st, &np_w13, m->d_w13_amax, m->d_epoch, il - m->l0, m->d_fault), LLAMAHIP_ERR_PREDICT);
            else
            HIP_TRY(launch_gemv(L.w13, PREP_NORM, EPI_SILU_QA, nullptr, nullptr, m->x1, L.ffn_norm, nullptr, nullptr, m->T_silu, m->qa2_A, m->qa2_d, st, &np_w13), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(launch_gemv(L.w2, PRE_QA, EPI_RESID, m->qa2_A, m->qa2_d, nullptr, nullptr, mbo ? nullptr : xo, m->x1, m->T_silu, nullptr, nullptr, st, &np_w2, mbo), LLAMAHIP_ERR_PREDICT);
        } else {
            if (mbo) { set_err(err, err_cap, "pipeline mailboxes need the interleaved w1|w3 layout"); return LLAMAHIP_ERR_PREDICT; }
            HIP_TRY(launch_gemv(L.w13, PREP_NORM, EPI_STORE, nullptr, nullptr, m->x1, L.ffn_norm, m->gu, nullptr, m->T_silu, nullptr, nullptr, st), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(launch_gemv(L.w2, PREP_SILU_MUL, EPI_RESID, nullptr, nullptr, m->gu, m->gu + F, xo, m->x1, m->T_silu, nullptr, nullptr, st), LLAMAHIP_ERR_PREDICT);
        }
    }

    if (m->last_stage) {
        // final norm + lm head (.mm:695-705)
        NormPart np_out;
        if (n_part_x > 0 && has_layers) { np_out.in = m->npart_a; np_out.n_in = n_part_x; }      // (x_last is null on the last stage: the row is in m->x)
        if (fold) {
            const PickIO pk = { m->d_pick + 128, (uint32_t *) m->d_pick, p.pick_out, p.pick_next, state, m->tok_emb, m->x, m->npart_a,
                                (m->d_attn_sync || m->d_pvx || m->d_w13_amax) ? m->d_epoch : nullptr, V };      // (the NEXT step's epoch: its schedule may use the tags even if this one does not)
            HIP_TRY(launch_gemv_pick(m->output, m->x, m->norm_w, m->logits, m->T_silu, st, &np_out, pk), LLAMAHIP_ERR_PREDICT);
        } else
        HIP_TRY(launch_gemv(m->output, PREP_NORM, EPI_STORE, nullptr, nullptr, m->x, m->norm_w, m->logits, nullptr, m->T_silu, nullptr, nullptr, st, &np_out), LLAMAHIP_ERR_PREDICT);
    }
    return 0;
}

// The un-fused pass of a Q4_0 handle for N rows (prompt evals; one row on LLAMAHIP_FLAG_UNFUSED handles and in debug evals): prepare -> GEMM
// per mat-mul, the position comes from the host.
int forward_eval(llamahip_model *m, const Pass &p, char *err, size_t err_cap) {
    const HParams &hp = m->hp;
    const int d = hp.n_embd, F = hp.n_ff, H = hp.n_head, dh = d / H, C = hp.n_ctx, V = hp.n_vocab;
    const int nth = clamp_threads(p.n_threads), n_past = p.n_past, N = p.N, chunk = p.chunk;
    hipStream_t st = p.stream;
    DumpSink *sink = p.sink;
    const bool debug = p.dump_layer >= 0 && sink;
    const bool fast_prefill = (m->flags & LLAMAHIP_FLAG_FAST_PREFILL) != 0 && !debug;      // opt-in re-associated prompt GEMM (llamahip.h)
    // short prompt chunks (the reference evaluates prompts 8 tokens at a time, .mm / LlamaRunner n_batch) take the decode-shaped attention
    const bool short_chunk = attn_path_pick(&m->attn_ws, N, dh, n_past + N, nth) == ATTN_PATH_SHORT;
    // short evals (2 .. 16 rows): the w1|w3 launch of k_gemv_set runs half-block workgroups whose halves exchange their amax as tagged
    // granules -- needs the XCD placement the load-time self-test confirmed and one epoch per pass
    SiluHalfIO set_hx;
    if (short_chunk && !debug && N <= SET_MAX && m->d_attn_sync && m->d_set_amax && m->l1 > m->l0 && m->l1 - m->l0 <= TAG_MAX_LAYERS) {
        set_hx.amax_t = m->d_set_amax; set_hx.epoch = m->d_epoch; set_hx.fault = m->d_fault;
        HIP_TRY(launch_bump_epoch(m->d_epoch, st), LLAMAHIP_ERR_PREDICT);
    }
    if (m->first_stage) HIP_TRY(launch_embed(p.tokens, m->tok_emb, m->x, d, N, st), LLAMAHIP_ERR_PREDICT);      // .mm:558-561
    else HIP_TRY(hipMemcpyAsync(m->x, p.hidden_in, (size_t) N * d * 4, hipMemcpyDeviceToDevice, st), LLAMAHIP_ERR_PREDICT);

    for (int il = m->l0; il < m->l1; il++) {
        const Layer &L = m->layers[il - m->l0];
        const size_t kv_at = ((size_t) p.seq * (m->l1 - m->l0) + (il - m->l0)) * C * d;
        float *Kl = m->Kc + kv_at, *Vl = m->Vc + kv_at;
        const bool dmp = debug && il == p.dump_layer;
        const bool short_layer = short_chunk && !dmp;        // (a dumped layer runs every operator on its own)
        if (dmp && !sink->put(0, m->x, (int64_t) N * d)) goto dump_fail;
        HIP_TRY(launch_prep(PREP_NORM, m->x, L.attention_norm, d, 0, d, N, m->qa_A, m->qa_d, dmp ? m->dbg_y : nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);   // .mm:570-575
        if (dmp && !sink->put(1, m->dbg_y, (int64_t) N * d)) goto dump_fail;
        const bool rope_fused = short_layer && gemm_rope_kv_applies(L.qkv, N, d);
        if (rope_fused) {
            // short evals: q / k / v mat-mul, RoPE and the KV append in one launch (.mm:580-611)
            const RopeKvArgs ra = { m->sincos, m->qr, Kl, Vl, n_past, d, dh };
            HIP_TRY(launch_gemm_rope_kv(L.qkv, m->qa_A, m->qa_d, N, ra, st), LLAMAHIP_ERR_PREDICT);
        } else
        HIP_TRY(launch_gemm(L.qkv, EPI_STORE, m->qa_A, m->qa_d, N, m->qkv, 3L * d, nullptr, 0, st, m->qb_ws, fast_prefill), LLAMAHIP_ERR_PREDICT);   // .mm:580-582
        if (dmp) {
            for (int which = 0; which < 3; which++) {           // q, k, v are column slices of qkv[N][3d]
                HIP_TRY(hipMemcpy2DAsync(m->tmp, (size_t) d * 4, m->qkv + (size_t) which * d, (size_t) 3 * d * 4, (size_t) d * 4, N, hipMemcpyDeviceToDevice, st), LLAMAHIP_ERR_PREDICT);
                if (!sink->put(2 + which, m->tmp, (int64_t) N * d)) goto dump_fail;
            }
        }
        if (!rope_fused) HIP_TRY(launch_rope_kv(m->qkv, 3L * d, d, dh, m->sincos, m->qr, Kl, Vl, n_past, N, st), LLAMAHIP_ERR_PREDICT);        // .mm:586-611
        if (dmp && !sink->put(5, m->qr, (int64_t) N * d)) goto dump_fail;
        if (short_layer) {
            // the reference's n_batch = 8 prompt flow: per-row decode-style attention that also quantizes
            // the merged rows for wo (scores scratch: the many-row path's score matrix)
            HIP_TRY(launch_attn_short(m->qr, Kl, Vl, m->attn_ws.S, nullptr, m->qa_A, m->qa_d, n_past, N, d, H, C, nth, m->T_exp, st, chunk), LLAMAHIP_ERR_PREDICT);   // .mm:614-646
        } else {
        HIP_TRY(launch_attn(m->qr, Kl, Vl, m->merged, dmp ? m->dbg_p : nullptr, dmp ? m->dbg_kqv : nullptr, n_past, N, d, H, nth, m->T_exp, &m->attn_ws, st, chunk), LLAMAHIP_ERR_PREDICT);   // .mm:614-646
        if (dmp) {
            if (!sink->put(6, m->dbg_p, (int64_t) H * N * (n_past + N))) goto dump_fail;
            if (!sink->put(7, m->dbg_kqv, (int64_t) N * d)) goto dump_fail;
            if (!sink->put(8, m->merged, (int64_t) N * d)) goto dump_fail;
        }
        HIP_TRY(launch_prep(PREP_PLAIN, m->merged, nullptr, d, 0, d, N, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);
        }
        if (dmp) {
            HIP_TRY(launch_gemm(L.wo, EPI_STORE, m->qa_A, m->qa_d, N, m->tmp, d, nullptr, 0, st, m->qb_ws, fast_prefill), LLAMAHIP_ERR_PREDICT);      // .mm:649-651
            if (!sink->put(9, m->tmp, (int64_t) N * d)) goto dump_fail;
            HIP_TRY(launch_add(m->tmp, m->x, m->x1, (long) N * d, st), LLAMAHIP_ERR_PREDICT);                                   // .mm:654
            if (!sink->put(10, m->x1, (int64_t) N * d)) goto dump_fail;
        } else {
            HIP_TRY(launch_gemm(L.wo, EPI_RESID, m->qa_A, m->qa_d, N, m->x1, d, m->x, d, st, m->qb_ws, fast_prefill), LLAMAHIP_ERR_PREDICT);
        }
        HIP_TRY(launch_prep(PREP_NORM, m->x1, L.ffn_norm, d, 0, d, N, m->qa_A, m->qa_d, dmp ? m->dbg_y : nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);        // .mm:660-665
        if (dmp && !sink->put(11, m->dbg_y, (int64_t) N * d)) goto dump_fail;
        if (short_layer && m->w13_interleaved && N <= 64 && gemm_silu_qa_applies(L.w13, N)) {
            // short evals: w1 | w3, SiLU * up and the quantization for w2 in one launch (.mm:668-680)
            const long KpF = ((long) F + 255) / 256 * 256;
            set_hx.layer = il - m->l0;
            HIP_TRY(launch_gemm_silu_qa(L.w13, m->qa_A, m->qa_d, N, m->T_silu, m->qaF_A, m->qaF_d, KpF / 4, KpF / 32, st, &set_hx), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(launch_gemm(L.w2, EPI_RESID, m->qaF_A, m->qaF_d, N, m->x, d, m->x1, d, st, m->qb_ws, fast_prefill), LLAMAHIP_ERR_PREDICT);      // .mm:682-687
            continue;
        }
        HIP_TRY(launch_gemm(L.w13, EPI_STORE, m->qa_A, m->qa_d, N, m->gu, 2L * F, nullptr, 0, st, m->qb_ws, fast_prefill), LLAMAHIP_ERR_PREDICT);     // .mm:668-675
        if (dmp) {
            HIP_TRY(hipMemcpy2DAsync(m->tmp, (size_t) F * 4, m->gu + F, (size_t) 2 * F * 4, (size_t) F * 4, N, hipMemcpyDeviceToDevice, st), LLAMAHIP_ERR_PREDICT);
            if (!sink->put(12, m->tmp, (int64_t) N * F)) goto dump_fail;       // w3 output ("tmp" in the reference)
            HIP_TRY(hipMemcpy2DAsync(m->tmp, (size_t) F * 4, m->gu, (size_t) 2 * F * 4, (size_t) F * 4, N, hipMemcpyDeviceToDevice, st), LLAMAHIP_ERR_PREDICT);
            if (!sink->put(13, m->tmp, (int64_t) N * F)) goto dump_fail;       // w1 output
        }
        HIP_TRY(launch_prep(PREP_SILU_MUL, m->gu, m->gu + F, 2L * F, 2L * F, F, N, m->qa_A, m->qa_d, dmp ? m->dbg_y : nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);   // .mm:678-680
        if (dmp && !sink->put(14, m->dbg_y, (int64_t) N * F)) goto dump_fail;
        if (dmp) {
            HIP_TRY(launch_gemm(L.w2, EPI_STORE, m->qa_A, m->qa_d, N, m->tmp, d, nullptr, 0, st, m->qb_ws, fast_prefill), LLAMAHIP_ERR_PREDICT);      // .mm:682-684
            if (!sink->put(15, m->tmp, (int64_t) N * d)) goto dump_fail;
            HIP_TRY(launch_add(m->tmp, m->x1, m->x, (long) N * d, st), LLAMAHIP_ERR_PREDICT);                                   // .mm:687
            if (!sink->put(16, m->x, (int64_t) N * d)) goto dump_fail;
        } else {
            HIP_TRY(launch_gemm(L.w2, EPI_RESID, m->qa_A, m->qa_d, N, m->x, d, m->x1, d, st, m->qb_ws, fast_prefill), LLAMAHIP_ERR_PREDICT);
        }
    }

    if (m->last_stage && p.embed) {
        // an embedding pass: the final norm as fp32 rows in place of the lm head (m->x is fp32 on every path)
        if (p.embed_y) HIP_TRY(launch_norm_rows_f32(m->x + (size_t) p.embed_first * d, m->norm_w, d, N - p.embed_first, p.embed_y, st), LLAMAHIP_ERR_PREDICT);
    } else if (m->last_stage) {
        // final norm + lm head (.mm:695-705).  The reference multiplies all N rows and keeps the
        // last (.mm:724-725); only the last row is computed here unless every row is requested.
        if (p.want_all) {
            HIP_TRY(launch_prep(PREP_NORM, m->x, m->norm_w, d, 0, d, N, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);
            // (the scoring entry points: with `output`'s prompt copies and the operand workspace; llamahip_eval_debug: the decode tiles only)
            QMat out = m->output;
            if (!p.score_rows) { out.rows = nullptr; out.mt = nullptr; out.mt4 = nullptr; }
            HIP_TRY(launch_gemm(out, EPI_STORE, m->qa_A, m->qa_d, N, m->logits, V, nullptr, 0, st, p.score_rows ? m->qb_ws : nullptr), LLAMAHIP_ERR_PREDICT);
        } else {
            HIP_TRY(launch_prep(PREP_NORM, m->x + (size_t) (N - 1) * d, m->norm_w, d, 0, d, 1, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(launch_gemm(m->output, EPI_STORE, m->qa_A, m->qa_d, 1, m->logits + (size_t) (N - 1) * V, V, nullptr, 0, st), LLAMAHIP_ERR_PREDICT);
        }
    }
    return 0;

dump_fail:
    set_err(err, err_cap, "HIP error while copying debug dump");
    return LLAMAHIP_ERR_PREDICT;
}

// which of the three schedules a pass takes: fixed by the handle and the pass before anything is launched
int forward(llamahip_model *m, const Pass &p, char *err, size_t err_cap) {
    const bool debug = p.dump_layer >= 0 && p.sink;
    if (m->dense && debug) { set_err(err, err_cap, "per-layer dumps are available for Q4_0 models only"); return LLAMAHIP_ERR_PREDICT; }
    if (m->dense) return forward_dense(m, p, err, err_cap);
    if (p.N == 1 && !debug && !p.embed && !(m->flags & LLAMAHIP_FLAG_UNFUSED)) return forward_decode(m, p, err, err_cap);      // (the decode step's final norm lives inside its lm head)
    return forward_eval(m, p, err, err_cap);
}

// Every tagged hand-off is a bounded poll; one that runs out raises the sticky fault word (results are invalid then).
// Read after the stream has been synchronised.
int check_sync_timeout(llamahip_model *m, char *err, size_t err_cap) {
    if (m->h_fault && *(volatile uint32_t *) m->h_fault) {
        *(volatile uint32_t *) m->h_fault = 0;
        set_err(err, err_cap, "a tagged hand-off inside a launch (decode attention, the half-block w1|w3 workgroups of a decode step or of a short eval) timed out; LLAMAHIP_NO_ATTN_X=1 selects the launches without them");
        return LLAMAHIP_ERR_PREDICT;
    }
    return 0;
}

int check_eval_args(llamahip_model *m, int n_past, const int32_t *tokens, int N, bool need_tokens, char *err, size_t err_cap) {
    if (!m) { set_err(err, err_cap, "null model"); return LLAMAHIP_ERR_PREDICT; }
    if (m->host_only) { set_err(err, err_cap, "model was loaded with LLAMAHIP_FLAG_HOST_ONLY: no device state, cannot evaluate"); return LLAMAHIP_ERR_PREDICT; }
    if (N < 1) { set_err(err, err_cap, "llamahip_eval: n_tokens must be >= 1 (got %d)", N); return LLAMAHIP_ERR_PREDICT; }
    if (n_past < 0 || n_past + N > m->hp.n_ctx) {
        // the reference has no bounds check and writes past its cache (.mm:586-590); refuse instead
        set_err(err, err_cap, "context overflow: n_past (%d) + n_tokens (%d) > n_ctx (%d)", n_past, N, m->hp.n_ctx);
        return LLAMAHIP_ERR_PREDICT;
    }
    if (need_tokens) {
        if (!tokens) { set_err(err, err_cap, "null tokens"); return LLAMAHIP_ERR_PREDICT; }
        for (int i = 0; i < N; i++) {
            if (tokens[i] < 0 || tokens[i] >= m->hp.n_vocab) {
                set_err(err, err_cap, "token id %d out of range [0, %d)", tokens[i], m->hp.n_vocab);
                return LLAMAHIP_ERR_PREDICT;
            }
        }
    }
    return 0;
}

}  // namespace

// what llamahip_decode_greedy refuses of a HANDLE, for the loops above the C ABI (ctx_overflow.cpp): no device is touched
namespace lh {
// eval_multi.cpp: what llamahip_eval_multi refuses of its arguments
int eval_multi_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, int32_t n_seqs, const int32_t *slots, const int32_t *n_past,
                     const int32_t *tokens, const int32_t *n_tokens, int32_t chunk_tokens, char *err, size_t err_cap);
// ... what llamahip_eval_logprobs_multi / llamahip_score_choices refuse of theirs, the scored rows of a pass and their results back in row order
int score_multi_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, int32_t n_seqs, const int32_t *slots, const int32_t *n_past,
                      const int32_t *tokens, const int32_t *n_tokens, int32_t chunk_tokens, const int32_t *targets, char *err, size_t err_cap);
int32_t score_multi_rows(int32_t n_seqs, const int32_t *tokens, const int32_t *n_tokens, const int32_t *targets, int32_t *tgt, int32_t *scored);
void score_scatter(int32_t R, int32_t nl, const int32_t *scored, const void *packed, double *lp, int32_t *am, int32_t *rk);
int score_choices_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, const int32_t *context, int32_t n_context, int32_t n_choices,
                        const int32_t *endings, const int32_t *n_ending, int32_t chunk_tokens, char *err, size_t err_cap);
// beam.cpp: what llamahip_beam_search refuses of its arguments, and the ranking of its finished hypotheses
int beam_check(int32_t n_ctx, int32_t n_vocab, int32_t n_slots, const llamahip_beam_opts *o, const int32_t *prompt, int32_t n_prompt,
               const void *hyps_out, const void *tokens_out, const void *n_hyps_out, char *err, size_t err_cap);
void beam_rank(int32_t n, const double *score, const int32_t *length, int32_t length_norm, int32_t *order);
// ... and llamahip_text_embedding[_multi] of theirs
int embed_check(const char *fn, int32_t n_ctx, int32_t n_vocab, int32_t n_slots, int32_t sched_max_active, int32_t n_seqs, const int32_t *slots,
                const int32_t *n_past, const int32_t *tokens, const int32_t *n_tokens, int32_t chunk_tokens, int32_t pool, int32_t normalize,
                const float *out, char *err, size_t err_cap);
int decode_handle_check(const llamahip_model *m, const char *fn, char *err, size_t err_cap) {
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    if (!m->stages.empty()) return 0;
    if (m->host_only) { set_err(err, err_cap, "%s: model was loaded with LLAMAHIP_FLAG_HOST_ONLY: no device state, cannot evaluate", fn); return LLAMAHIP_ERR_PREDICT; }
    if (!m->first_stage || !m->last_stage) { set_err(err, err_cap, "%s on a pipeline-stage handle: load the whole model (or a device list)", fn); return LLAMAHIP_ERR_PREDICT; }
    return 0;
}
}  // namespace lh

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char *llamahip_version(void) { return "llamahip 0.1 (gfx950)"; }

static int model_load_impl(const char *path, int32_t n_ctx, const llamahip_opts *opts,
                           llamahip_model **out, char *err, size_t err_cap) {
    const double t0 = now_ms();
    if (!out || !path) { set_err(err, err_cap, "null argument"); return LLAMAHIP_ERR_LOAD; }
    *out = nullptr;
    if (n_ctx < 1) { set_err(err, err_cap, "n_ctx must be >= 1"); return LLAMAHIP_ERR_LOAD; }
    std::unique_ptr<llamahip_model> m(new llamahip_model());
    int force_parts = 0, layer_begin = 0, layer_end = -1, device = -1;
    if (opts && opts->struct_size >= 24) {             // fields up to `flags`
        force_parts = opts->n_parts; layer_begin = opts->layer_begin; layer_end = opts->layer_end;
        device = opts->device; m->flags = opts->flags;
        if (opts->struct_size >= 28 && opts->n_seq > 0) m->n_seq = opts->n_seq;      // (28: the struct up to n_seq, as older callers pass it)
    }
    std::string e;
    if (!m->file.open(path, n_ctx, force_parts, e)) { set_err(err, err_cap, "%s", e.c_str()); return LLAMAHIP_ERR_LOAD; }
    m->hp = m->file.hp;
    const HParams &hp = m->hp;
    const int d = hp.n_embd, F = hp.n_ff, V = hp.n_vocab, H = hp.n_head;
    if (d % H != 0 || (d / H) % 32 != 0 || 256 % (d / H) != 0) {
        set_err(err, err_cap, "unsupported head size %d (n_embd %d / n_head %d): must be 32, 64, 128 or 256", H ? d / H : 0, d, H);
        return LLAMAHIP_ERR_LOAD;
    }
    if (F % 8 != 0) { set_err(err, err_cap, "unsupported n_ff %d (must be a multiple of 8)", F); return LLAMAHIP_ERR_LOAD; }
    // hp.n_rot is read and ignored, like the reference: llama_eval derives the rotated span from
    // n_embd / n_head (.mm:528) and never looks at the header field (.mm:48,130), so a file whose n_rot
    // differs evaluates identically there and here
    if (layer_end < 0) layer_end = hp.n_layer;
    if (layer_begin < 0 || layer_begin >= layer_end || layer_end > hp.n_layer) {
        set_err(err, err_cap, "bad layer range [%d, %d) for n_layer %d", layer_begin, layer_end, hp.n_layer);
        return LLAMAHIP_ERR_LOAD;
    }
    m->l0 = layer_begin; m->l1 = layer_end;
    m->first_stage = (m->l0 == 0);
    m->last_stage = (m->l1 == hp.n_layer);
    if (m->flags & LLAMAHIP_FLAG_HOST_ONLY) {
        m->host_only = true;
        m->t_load_ms = now_ms() - t0;
        *out = m.release();
        return LLAMAHIP_OK;
    }

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        set_err(err, err_cap, "no HIP device available: libllamahip has no CPU fallback");
        return LLAMAHIP_ERR_LOAD;
    }
    if (device >= 0) HIP_TRY(hipSetDevice(device), LLAMAHIP_ERR_LOAD);
    HIP_TRY(hipGetDevice(&m->device), LLAMAHIP_ERR_LOAD);
    HIP_TRY(hipStreamCreate(&m->stream), LLAMAHIP_ERR_LOAD);
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_LOAD);

    // ---- lookup tables (ggml.c:2376-2389) and the RoPE angle table (ggml.c:7113-7116), host libm
    {
        std::vector<uint16_t> ts(1 << 16), te(1 << 16);
        lut_tables(ts, te);
        HIP_TRY(m->own.alloc(&m->T_silu, ts.size()), LLAMAHIP_ERR_LOAD);
        HIP_TRY(m->own.alloc(&m->T_exp, te.size()), LLAMAHIP_ERR_LOAD);
        HIP_TRY(hipMemcpy(m->T_silu, ts.data(), ts.size() * 2, hipMemcpyHostToDevice), LLAMAHIP_ERR_LOAD);
        HIP_TRY(hipMemcpy(m->T_exp, te.data(), te.size() * 2, hipMemcpyHostToDevice), LLAMAHIP_ERR_LOAD);
        HIP_TRY(launch_check_lut_math(m->T_silu, m->T_exp, m->stream), LLAMAHIP_ERR_LOAD);
        const std::vector<double> sc = rope_table(n_ctx, d / H);
        HIP_TRY(m->own.alloc(&m->sincos, sc.size()), LLAMAHIP_ERR_LOAD);
        HIP_TRY(hipMemcpy(m->sincos, sc.data(), sc.size() * 8, hipMemcpyHostToDevice), LLAMAHIP_ERR_LOAD);
    }

    // ---- weights
    size_t max_bytes = 0;
    for (const auto &kv : m->file.tensors) if (kv.second.q4) max_bytes = std::max(max_bytes, (size_t) kv.second.nbytes());
    DevOwner staging;                    // the file-layout tensor on its way into the tiles: released on every return path
    uint8_t *d_stage = nullptr;
    HIP_TRY(staging.alloc(&d_stage, std::max<size_t>(max_bytes, 256)), LLAMAHIP_ERR_LOAD);
    std::vector<uint8_t> h_stage;
    int rc = 0;
#define LOAD_TRY(x) do { rc = (x); if (rc != 0) return rc; } while (0)

    if (m->first_stage) {
        const TensorInfo &t = m->file.tensors.at("tok_embeddings.weight");
        h_stage.resize((size_t) t.nbytes());
        if (!m->file.read_tensor(t.name, h_stage.data(), e)) { set_err(err, err_cap, "%s", e.c_str()); return LLAMAHIP_ERR_LOAD; }
        HIP_TRY(m->own.alloc(&m->tok_emb, h_stage.size()), LLAMAHIP_ERR_LOAD);
        HIP_TRY(hipMemcpy(m->tok_emb, h_stage.data(), h_stage.size(), hipMemcpyHostToDevice), LLAMAHIP_ERR_LOAD);
        m->weight_bytes += (int64_t) h_stage.size();
    }
    m->dense = (hp.f16 != 2);
    if (m->dense && (d % 64 != 0 || F % 64 != 0)) { set_err(err, err_cap, "f16 / f32 / Q4_1 model: n_embd and n_ff must be multiples of 64"); return LLAMAHIP_ERR_LOAD; }
    m->layers.resize(m->l1 - m->l0);
    if (m->dense) {
        if (m->last_stage) {
            LOAD_TRY(upload_f32(m.get(), "norm.weight", &m->norm_w, err, err_cap));
            LOAD_TRY(alloc_dmat(m->doutput, V, d, m.get(), err, err_cap));
            LOAD_TRY(upload_dense(m.get(), "output.weight", m->doutput, 0, h_stage, err, err_cap));
        }
        for (int il = m->l0; il < m->l1; il++) {
            Layer &L = m->layers[il - m->l0];
            const std::string p = "layers." + std::to_string(il) + ".";
            LOAD_TRY(upload_f32(m.get(), p + "attention_norm.weight", &L.attention_norm, err, err_cap));
            LOAD_TRY(upload_f32(m.get(), p + "ffn_norm.weight", &L.ffn_norm, err, err_cap));
            LOAD_TRY(alloc_dmat(L.dqkv, 3 * d, d, m.get(), err, err_cap));
            LOAD_TRY(upload_dense(m.get(), p + "attention.wq.weight", L.dqkv, 0, h_stage, err, err_cap));
            LOAD_TRY(upload_dense(m.get(), p + "attention.wk.weight", L.dqkv, d, h_stage, err, err_cap));
            LOAD_TRY(upload_dense(m.get(), p + "attention.wv.weight", L.dqkv, 2 * d, h_stage, err, err_cap));
            LOAD_TRY(alloc_dmat(L.dwo, d, d, m.get(), err, err_cap));
            LOAD_TRY(upload_dense(m.get(), p + "attention.wo.weight", L.dwo, 0, h_stage, err, err_cap));
            LOAD_TRY(alloc_dmat(L.dw13, 2 * F, d, m.get(), err, err_cap));
            LOAD_TRY(upload_dense(m.get(), p + "feed_forward.w1.weight", L.dw13, 0, h_stage, err, err_cap));
            LOAD_TRY(upload_dense(m.get(), p + "feed_forward.w3.weight", L.dw13, F, h_stage, err, err_cap));
            LOAD_TRY(alloc_dmat(L.dw2, d, F, m.get(), err, err_cap));
            LOAD_TRY(upload_dense(m.get(), p + "feed_forward.w2.weight", L.dw2, 0, h_stage, err, err_cap));
        }
    } else {
    if (m->last_stage) {
        LOAD_TRY(upload_f32(m.get(), "norm.weight", &m->norm_w, err, err_cap));
        LOAD_TRY(alloc_qmat(m->output, V, d, m.get(), err, err_cap));
        LOAD_TRY(upload_q4(m.get(), "output.weight", m->output, 0, d_stage, h_stage, err, err_cap));
    }
    m->w13_interleaved = (F % 32 == 0);
    for (int il = m->l0; il < m->l1; il++) {
        Layer &L = m->layers[il - m->l0];
        const std::string p = "layers." + std::to_string(il) + ".";
        LOAD_TRY(upload_f32(m.get(), p + "attention_norm.weight", &L.attention_norm, err, err_cap));
        LOAD_TRY(upload_f32(m.get(), p + "ffn_norm.weight", &L.ffn_norm, err, err_cap));
        LOAD_TRY(alloc_qmat(L.qkv, 3 * d, d, m.get(), err, err_cap));
        LOAD_TRY(upload_q4(m.get(), p + "attention.wq.weight", L.qkv, 0, d_stage, h_stage, err, err_cap));
        LOAD_TRY(upload_q4(m.get(), p + "attention.wk.weight", L.qkv, d, d_stage, h_stage, err, err_cap));
        LOAD_TRY(upload_q4(m.get(), p + "attention.wv.weight", L.qkv, 2 * d, d_stage, h_stage, err, err_cap));
        LOAD_TRY(alloc_qmat(L.wo, d, d, m.get(), err, err_cap));
        LOAD_TRY(upload_q4(m.get(), p + "attention.wo.weight", L.wo, 0, d_stage, h_stage, err, err_cap));
        LOAD_TRY(alloc_qmat(L.w13, 2 * F, d, m.get(), err, err_cap));
        if (m->w13_interleaved) {
            // every 8 tile groups = 32 rows of w1 followed by the same 32 rows of w3 (k_repack_q4)
            L.w13.gmapF8 = F / 8;
            LOAD_TRY(upload_q4(m.get(), p + "feed_forward.w1.weight", L.w13, 0, d_stage, h_stage, err, err_cap, 1, 0));
            LOAD_TRY(upload_q4(m.get(), p + "feed_forward.w3.weight", L.w13, 0, d_stage, h_stage, err, err_cap, 1, 4));
        } else {
            LOAD_TRY(upload_q4(m.get(), p + "feed_forward.w1.weight", L.w13, 0, d_stage, h_stage, err, err_cap));
            LOAD_TRY(upload_q4(m.get(), p + "feed_forward.w3.weight", L.w13, F, d_stage, h_stage, err, err_cap));
        }
        LOAD_TRY(alloc_qmat(L.w2, d, F, m.get(), err, err_cap));
        LOAD_TRY(upload_q4(m.get(), p + "feed_forward.w2.weight", L.w2, 0, d_stage, h_stage, err, err_cap));
    }
    }
#undef LOAD_TRY
    staging.release(&d_stage);

    // ---- KV cache (.mm:290-304); zero-initialised (the reference leaves malloc garbage)
    const size_t kv_elems = (size_t) m->n_seq * (m->l1 - m->l0) * n_ctx * d;
    HIP_TRY(m->own.alloc_all({ { &m->Kc, kv_elems * 4, true }, { &m->Vc, kv_elems * 4, true } }), LLAMAHIP_ERR_LOAD);
    m->kv_bytes = (int64_t) kv_elems * 8;
    {
        const size_t Kp_d = ((size_t) d + 255) / 256 * 256, Kp_F = ((size_t) F + 255) / 256 * 256, dh = d / H;
        HIP_TRY(m->own.alloc(&m->d_state, 2, true), LLAMAHIP_ERR_LOAD);
        HIP_TRY(m->own.alloc(&m->sc, (size_t) H * n_ctx), LLAMAHIP_ERR_LOAD);
        HIP_TRY(m->own.alloc(&m->part, (size_t) H * 64 * dh), LLAMAHIP_ERR_LOAD);
        HIP_TRY(alloc_pinned(m.get(), &m->h_fault, &m->d_fault, 64), LLAMAHIP_ERR_LOAD);
        if (!getenv("LLAMAHIP_NO_HOST_IO")) HIP_TRY(alloc_pinned(m.get(), &m->h_io, &m->d_io, sizeof(llamahip_model::HostIo)), LLAMAHIP_ERR_LOAD);
        // decode attention as one launch needs every workgroup of a head behind one L2: check the placement on this
        // device before relying on it (LLAMAHIP_NO_ATTN_X: keep the two launches)
        if (!getenv("LLAMAHIP_NO_ATTN_X") && H % 8 == 0 && xcd_selftest(H, (int) (d / H / 32) + (n_ctx + 31) / 32, m->stream))
            HIP_TRY(m->own.alloc_all({ { &m->d_attn_sync, (size_t) H * 32 * 4, true }, { &m->d_qkv2, (size_t) 3 * d * 8, true },
                                       { &m->d_sc2, (size_t) H * n_ctx * 8, true }, { &m->d_pvx, (size_t) d * 32 * 8, true } }), LLAMAHIP_ERR_LOAD);
        HIP_TRY(m->own.alloc(&m->d_epoch, 16, true), LLAMAHIP_ERR_LOAD);
        HIP_TRY(m->own.alloc(&m->d_w13_amax, (size_t) F / 16 + 16, true), LLAMAHIP_ERR_LOAD);
        HIP_TRY(m->own.alloc(&m->d_set_amax, (size_t) SET_MAX * set_amax_granules(F), true), LLAMAHIP_ERR_LOAD);
        // lm-head pick epilogue: [0, 1024) bytes tickets, then one 8-byte key per workgroup of the lm head's launch (<= n_vocab / 8 + 8)
        HIP_TRY(m->own.alloc(&m->d_pick, 128 + (size_t) V / 8 + 8, true), LLAMAHIP_ERR_LOAD);
        HIP_TRY(m->own.alloc(&m->npart_a, NORM_PART_MAX * 2, true), LLAMAHIP_ERR_LOAD);
        HIP_TRY(m->own.alloc(&m->npart_b, NORM_PART_MAX * 2, true), LLAMAHIP_ERR_LOAD);
        // blocks past K/32 (padding up to a multiple of 256 columns) are never written again: keep them zero
        HIP_TRY(m->own.alloc_all({ { &m->qa1_A, Kp_d, true }, { &m->qa1_d, Kp_d / 32 * 4, true }, { &m->qa2_A, Kp_F, true }, { &m->qa2_d, Kp_F / 32 * 4, true } }), LLAMAHIP_ERR_LOAD);
    }

    rc = ensure_workspace(m.get(), 16, err, err_cap);
    if (rc != 0) return LLAMAHIP_ERR_LOAD;
    if (getenv("LLAMAHIP_EAGER_PREFILL_COPY") && ensure_prompt_copies(m.get(), PROMPT_COPY_MIN_ROWS, err, err_cap) != 0) return LLAMAHIP_ERR_LOAD;
    HIP_TRY(hipDeviceSynchronize(), LLAMAHIP_ERR_LOAD);
    m->t_load_ms = now_ms() - t0;
    *out = m.release();
    return LLAMAHIP_OK;
}

// ---- in-process layer pipeline: defined behind the stage entry points below
static int pipe_devices(const llamahip_opts *opts, std::vector<int> &devices, char *err, size_t err_cap);
static int pipe_load(const char *path, int32_t n_ctx, const llamahip_opts *opts, const std::vector<int> &devices, llamahip_model **out, char *err, size_t err_cap);
static int pipe_eval(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t N, int32_t chunk, float *logits_out, char *err, size_t err_cap);
static int pipe_decode_greedy(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token, int32_t n_steps, int32_t *out_tokens, float *logits_last,
                              char *err, size_t err_cap);
static int decode_greedy_multi_impl(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens, int32_t n_steps,
                                    int32_t *out_tokens, char *err, size_t err_cap);
#define PIPE_REFUSE(m, what) do { if ((m) && !(m)->stages.empty()) { set_err(err, err_cap, what " is not available on a multi-device pipeline handle (llamahip_opts.n_devices / LLAMAHIP_DEVICES): load a stage handle with layer_begin / layer_end"); return LLAMAHIP_ERR_PREDICT; } } while (0)

// No C++ exception may cross the C ABI (std::bad_alloc on a corrupt header would abort the host process).
int llamahip_model_load(const char *path, int32_t n_ctx, const llamahip_opts *opts,
                        llamahip_model **out, char *err, size_t err_cap) {
    try {
        std::vector<int> devices;
        const int rc = pipe_devices(opts, devices, err, err_cap);
        if (rc) { if (out) *out = nullptr; return rc; }
        if (devices.size() > 1) return pipe_load(path, n_ctx, opts, devices, out, err, err_cap);
        if (devices.size() == 1 && opts && opts->struct_size >= 24) {      // (a one-entry list is the plain handle on that device)
            llamahip_opts o = {}; memcpy(&o, opts, std::min((size_t) opts->struct_size, sizeof(o)));
            o.struct_size = (int32_t) std::min((size_t) opts->struct_size, sizeof(o)); o.device = devices[0];
            return model_load_impl(path, n_ctx, &o, out, err, err_cap);
        }
        if (devices.size() == 1) { llamahip_opts o = {}; o.struct_size = 28; o.device = devices[0]; o.layer_end = -1; return model_load_impl(path, n_ctx, &o, out, err, err_cap); }
        return model_load_impl(path, n_ctx, opts, out, err, err_cap);
    } catch (const std::exception &ex) {
        if (out) *out = nullptr;
        set_err(err, err_cap, "failed to load model '%s': %s", path ? path : "(null)", ex.what());
    } catch (...) {
        if (out) *out = nullptr;
        set_err(err, err_cap, "failed to load model '%s': unknown exception", path ? path : "(null)");
    }
    return LLAMAHIP_ERR_LOAD;
}

void llamahip_model_free(llamahip_model *m) { delete m; }

int32_t llamahip_n_vocab(const llamahip_model *m) { return m ? m->hp.n_vocab : 0; }
int32_t llamahip_n_ctx(const llamahip_model *m) { return m ? m->hp.n_ctx : 0; }
int32_t llamahip_n_embd(const llamahip_model *m) { return m ? m->hp.n_embd : 0; }
int32_t llamahip_n_head(const llamahip_model *m) { return m ? m->hp.n_head : 0; }
int32_t llamahip_n_layer(const llamahip_model *m) { return m ? m->hp.n_layer : 0; }
int32_t llamahip_n_ff(const llamahip_model *m) { return m ? m->hp.n_ff : 0; }
int32_t llamahip_n_parts(const llamahip_model *m) { return m ? m->hp.n_parts : 0; }

const char *llamahip_token_text(const llamahip_model *m, int32_t id, uint32_t *len) {
    if (!m || id < 0 || id >= (int32_t) m->file.id_to_token.size()) { if (len) *len = 0; return nullptr; }
    const std::string &s = m->file.id_to_token[id];
    if (len) *len = (uint32_t) s.size();
    return s.c_str();
}

static int eval_impl(llamahip_model *m, int32_t n_threads, int32_t n_past,
                     const int32_t *tokens, int32_t N, float *logits_last, float *logits_all,
                     int32_t dump_layer, float *dump, int64_t dump_cap, int64_t *dump_sizes,
                     bool sync, char *err, size_t err_cap, int chunk = 0) {
    if (m && !m->stages.empty()) {
        if (logits_all || (dump_layer >= 0 && dump)) PIPE_REFUSE(m, "llamahip_eval_debug (all rows of logits / per-layer dumps)");
        return pipe_eval(m, n_threads, n_past, tokens, N, chunk, logits_last, err, err_cap);      // (synchronous: `sync` = false is eval_topk's, which never gets here)
    }
    int rc = check_eval_args(m, n_past, tokens, N, true, err, err_cap);
    if (rc) return rc;
    if (!m->first_stage || !m->last_stage) { set_err(err, err_cap, "llamahip_eval on a pipeline-stage handle: use llamahip_eval_stage"); return LLAMAHIP_ERR_PREDICT; }
    const double t0 = now_ms();
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    rc = ensure_workspace(m, N, err, err_cap);
    if (rc) return rc;
    rc = ensure_attn_ws(m, N, err, err_cap);
    if (rc) return rc;
    rc = ensure_prompt_copies(m, N, err, err_cap);
    if (rc) return rc;
    const bool tok_mapped = N == 1 && m->h_io != nullptr;          // (the stream is idle here: every entry point synchronises before it returns)
    if (tok_mapped) m->h_io->tok[0] = tokens[0];
    else HIP_TRY(hipMemcpyAsync(m->d_tokens, tokens, (size_t) N * 4, hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
    Pass pass(m);
    pass.n_threads = n_threads; pass.n_past = n_past; pass.N = N; pass.chunk = chunk;
    pass.want_all = logits_all != nullptr;
    DumpSink sink;
    if (dump_layer >= 0 && dump && dump_sizes) {
        sink.dump = dump; sink.cap = dump_cap; sink.sizes = dump_sizes; sink.st = m->stream;
        for (int i = 0; i < 17; i++) dump_sizes[i] = 0;
        pass.dump_layer = dump_layer; pass.sink = &sink;
    }
    if (tok_mapped) pass.tokens = m->d_io->tok;
    if (N == 1) pass.attn_sched = attn_sched_at(m, n_past);
    rc = forward(m, pass, err, err_cap);
    m->last_rows.clear();
    if (rc) return rc;
    const size_t V = m->hp.n_vocab;
    if (logits_last) HIP_TRY(hipMemcpyAsync(logits_last, m->logits + (size_t) (N - 1) * V, V * 4, hipMemcpyDeviceToHost, m->stream), LLAMAHIP_ERR_PREDICT);
    if (logits_all) HIP_TRY(hipMemcpyAsync(logits_all, m->logits, (size_t) N * V * 4, hipMemcpyDeviceToHost, m->stream), LLAMAHIP_ERR_PREDICT);
    m->n_evals++;
    if (!sync) return LLAMAHIP_OK;          // (llamahip_eval_topk: more work follows on the stream before the one synchronisation)
    HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
    if ((rc = check_sync_timeout(m, err, err_cap)) != 0) return rc;        // (single-token steps and short evals take in-launch tagged hand-offs)
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}

int llamahip_eval_debug(llamahip_model *m, int32_t n_threads, int32_t n_past,
                        const int32_t *tokens, int32_t N, float *logits_last, float *logits_all,
                        int32_t dump_layer, float *dump, int64_t dump_cap, int64_t *dump_sizes,
                        char *err, size_t err_cap) {
    return eval_impl(m, n_threads, n_past, tokens, N, logits_last, logits_all, dump_layer, dump, dump_cap, dump_sizes, true, err, err_cap);
}

int llamahip_eval(llamahip_model *m, int32_t n_threads, int32_t n_past,
                  const int32_t *tokens, int32_t n_tokens, float *logits_out, char *err, size_t err_cap) {
    return llamahip_eval_debug(m, n_threads, n_past, tokens, n_tokens, logits_out, nullptr, -1, nullptr, 0, nullptr, err, err_cap);
}

// The reference feeds a prompt to llama_eval n_batch + 1 = 9 tokens at a time (.mm:880-888).  One pass over all the rows gives the
// same bits -- every operator of the graph works row by row except the V*P key split, which depends on the eval a row belongs to
// (prompt_attn.hip split_keys) and is applied per row here -- at the speed of a long eval (matrix-core GEMMs) instead of 9-row ones.
// f16 / f32 files take the one pass from DENSE_ONE_PASS_MIN_ROWS rows (below it the chunk loop on k_dense_set measured no slower: DESIGN.md
// 12.18); Q4_1 files (no one-pass chunked eval: DESIGN.md 12.24) keep the loop.  A pipeline handle's front is loaded HOST_ONLY and never learns the file
// type: its stages know it.
static bool chunks_in_one_pass(const llamahip_model *m, int n_tokens) {
    if (m->host_only && m->stages.empty()) return false;
    const llamahip_model *s0 = m->stages.empty() ? m : m->stages[0];
    if (!s0->dense) return true;
    return s0->hp.f16 != 3 && n_tokens >= DENSE_ONE_PASS_MIN_ROWS;
}
// (one_pass = false: llamahip_eval_multi's per-slot loop on f16 / f32 files, which reports the evals it made)
static int eval_chunks_impl(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t n_tokens,
                            int32_t chunk_tokens, float *logits_out, bool one_pass, char *err, size_t err_cap) {
    if (chunk_tokens < 1) { set_err(err, err_cap, "llamahip_eval_chunks: chunk_tokens must be >= 1"); return LLAMAHIP_ERR_PREDICT; }
    if (!m || n_tokens <= chunk_tokens) return llamahip_eval(m, n_threads, n_past, tokens, n_tokens, logits_out, err, err_cap);
    if (!one_pass || !chunks_in_one_pass(m, n_tokens)) {
        for (int32_t c0 = 0; c0 < n_tokens; c0 += chunk_tokens) {
            const int32_t n = std::min(chunk_tokens, n_tokens - c0);
            const int rc = llamahip_eval(m, n_threads, n_past + c0, tokens + c0, n, c0 + n == n_tokens ? logits_out : nullptr, err, err_cap);
            if (rc) return rc;
        }
        return LLAMAHIP_OK;
    }
    return eval_impl(m, n_threads, n_past, tokens, n_tokens, logits_out, nullptr, -1, nullptr, 0, nullptr, true, err, err_cap, chunk_tokens);
}
int llamahip_eval_chunks(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t n_tokens,
                         int32_t chunk_tokens, float *logits_out, char *err, size_t err_cap) {
    return eval_chunks_impl(m, n_threads, n_past, tokens, n_tokens, chunk_tokens, logits_out, true, err, err_cap);
}

// llamahip_eval + the candidate selection of llama_sample_top_p_top_k on the device (utils.cpp:345-395): 816 bytes come
// back instead of n_vocab logits.  *exact = 0 (a tie that only libstdc++'s partial_sort can order, a NaN, or an
// unsupported size): logits_out then holds the full row and the caller samples on the host as before.
int llamahip_eval_topk(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t n_tokens,
                       const int32_t *last_n_tokens, int32_t n_last, double repeat_penalty, int32_t top_k, double temp,
                       double *cand_scores, int32_t *cand_ids, int32_t *exact, float *logits_out, char *err, size_t err_cap) {
    if (!cand_scores || !cand_ids || !exact || !logits_out) { set_err(err, err_cap, "llamahip_eval_topk: null output"); return LLAMAHIP_ERR_PREDICT; }
    *exact = 0;
    const int V = m ? m->hp.n_vocab : 0;
    const int k = std::min(std::max(top_k, 1), V);
    // (a multi-device pipeline handle returns the logits row: *exact = 0, the caller samples on the host -- the documented fall-back)
    const bool device_ok = m && m->stages.empty() && !m->host_only && V <= 32768 && k <= 64 && n_last >= 0 && n_last <= 1024 && (n_last == 0 || last_n_tokens);
    if (!device_ok) return llamahip_eval(m, n_threads, n_past, tokens, n_tokens, logits_out, err, err_cap);
    const double t0 = now_ms();
    int rc = eval_impl(m, n_threads, n_past, tokens, n_tokens, nullptr, nullptr, -1, nullptr, 0, nullptr, false, err, err_cap);   // logits stay on the device, no wait
    if (rc) return rc;
    if (!m->d_topk) HIP_TRY(m->own.alloc(&m->d_topk, 8192 + TOPK_WS_BYTES, true), LLAMAHIP_ERR_PREDICT);
    int32_t *d_win = (int32_t *) m->d_topk;
    double *d_sc = (double *) ((char *) m->d_topk + 4096);
    int32_t *d_id = (int32_t *) ((char *) m->d_topk + 4096 + 512), *d_fl = d_id + 64;
    const bool mapped = m->h_io != nullptr;        // window in, candidates out through the pinned host block: no blit copies
    if (mapped) {
        if (n_last > 0) memcpy(m->h_io->window, last_n_tokens, (size_t) n_last * 4);
        d_win = m->d_io->window; d_sc = m->d_io->sc; d_id = m->d_io->id; d_fl = m->d_io->fl;
    } else if (n_last > 0) HIP_TRY(hipMemcpyAsync(d_win, last_n_tokens, (size_t) n_last * 4, hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
    const float *row = m->logits + (size_t) (n_tokens - 1) * V;
    HIP_TRY(launch_topk_candidates(row, V, d_win, n_last, 1.0 / temp, repeat_penalty, k, d_sc, d_id, d_fl, m->stream, (char *) m->d_topk + 8192), LLAMAHIP_ERR_PREDICT);
    struct { double sc[64]; int32_t id[64]; int32_t fl[2]; } h;
    if (!mapped) HIP_TRY(hipMemcpyAsync(&h, d_sc, sizeof(h), hipMemcpyDeviceToHost, m->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
    if (mapped) { memcpy(h.sc, m->h_io->sc, sizeof(h.sc)); memcpy(h.id, m->h_io->id, sizeof(h.id)); memcpy(h.fl, m->h_io->fl, sizeof(h.fl)); }
    if ((rc = check_sync_timeout(m, err, err_cap)) != 0) return rc;
    m->t_eval_ms += now_ms() - t0;
    if (h.fl[0] == 1) {
        for (int i = 0; i < k; i++) { cand_scores[i] = h.sc[i]; cand_ids[i] = h.id[i]; }
        *exact = 1;
        return LLAMAHIP_OK;
    }
    HIP_TRY(hipMemcpy(logits_out, row, (size_t) V * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    return LLAMAHIP_OK;
}

// the launches of a stage eval, enqueued on m->stream without waiting (llamahip_eval_stage; the in-process pipeline walks its stages with it)
// (want_all: the last stage computes the logits of every row, for k_row_logprob -- the scoring entry points)
// (embed: an embedding pass -- Pass::embed with {embed_y, embed_first} = *embed on the last stage; the logits and their row map stay as they are)
struct EmbedReq { float *y; int first; };
static int eval_stage_enqueue(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t N, const void *hidden_in,
                              int chunk, bool want_all, char *err, size_t err_cap, const EmbedReq *embed = nullptr) {
    int rc = check_eval_args(m, n_past, tokens, N, m && m->first_stage, err, err_cap);
    if (rc) return rc;
    if (!m->first_stage && !hidden_in) { set_err(err, err_cap, "stage [%d,%d) needs hidden_in", m->l0, m->l1); return LLAMAHIP_ERR_PREDICT; }
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    rc = ensure_workspace(m, N, err, err_cap);
    if (rc) return rc;
    rc = ensure_attn_ws(m, N, err, err_cap);
    if (rc) return rc;
    rc = ensure_prompt_copies(m, N, err, err_cap);
    if (rc) return rc;
    const bool all = want_all && m->last_stage;
    if (all) ensure_output_copies(m, N);
    if (m->first_stage) HIP_TRY(hipMemcpyAsync(m->d_tokens, tokens, (size_t) N * 4, hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
    Pass pass(m);
    pass.n_threads = n_threads; pass.n_past = n_past; pass.N = N; pass.chunk = chunk; pass.hidden_in = (const float *) hidden_in;
    pass.want_all = pass.score_rows = all;
    if (embed) { pass.embed = true; pass.embed_y = embed->y; pass.embed_first = embed->first; }
    if (N == 1) pass.attn_sched = attn_sched_at(m, n_past);
    rc = forward(m, pass, err, err_cap);
    if (!(embed && m->last_stage)) m->last_rows.clear();                 // (m->logits rewritten: llamahip_stage_logits rows are this eval's rows again)
    return rc;
}

int llamahip_eval_stage(llamahip_model *m, int32_t n_threads, int32_t n_past,
                        const int32_t *tokens, int32_t N, const void *hidden_in, void *hidden_out,
                        float *logits_out, char *err, size_t err_cap) {
    PIPE_REFUSE(m, "llamahip_eval_stage");
    const double t0 = now_ms();
    int rc = eval_stage_enqueue(m, n_threads, n_past, tokens, N, hidden_in, 0, false, err, err_cap);
    if (rc) return rc;
    const size_t d = m->hp.n_embd, V = m->hp.n_vocab;
    if (hidden_out) HIP_TRY(hipMemcpyAsync(hidden_out, m->x, (size_t) N * d * 4, hipMemcpyDeviceToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
    if (m->last_stage && logits_out) HIP_TRY(hipMemcpyAsync(logits_out, m->logits + (size_t) (N - 1) * V, V * 4, hipMemcpyDeviceToHost, m->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
    if ((rc = check_sync_timeout(m, err, err_cap)) != 0) return rc;       // (single-token and short stage evals take the in-launch hand-offs too)
    m->n_evals++;
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}

int llamahip_decode_greedy(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token,
                           int32_t n_steps, int32_t *out_tokens, float *logits_last, char *err, size_t err_cap) {
    if (m && !m->stages.empty()) return pipe_decode_greedy(m, n_threads, n_past, first_token, n_steps, out_tokens, logits_last, err, err_cap);
    int rc = check_eval_args(m, n_past, &first_token, 1, true, err, err_cap);
    if (rc) return rc;
    if (n_steps < 1 || n_past + n_steps > m->hp.n_ctx) {
        set_err(err, err_cap, "context overflow: n_past (%d) + n_steps (%d) > n_ctx (%d)", n_past, n_steps, m->hp.n_ctx);
        return LLAMAHIP_ERR_PREDICT;
    }
    if (!m->first_stage || !m->last_stage) { set_err(err, err_cap, "greedy decode needs a whole-model handle"); return LLAMAHIP_ERR_PREDICT; }
    m->last_rows.clear();
    const double t0 = now_ms();
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    rc = ensure_workspace(m, 1, err, err_cap);
    if (rc) return rc;
    if (!m->d_out_tokens) {      // sized once for the whole context: captured graphs hold this pointer
        HIP_TRY(m->own.alloc(&m->d_out_tokens, (size_t) m->hp.n_ctx), LLAMAHIP_ERR_PREDICT);
        m->out_tokens_cap = m->hp.n_ctx;
    }
    HIP_TRY(hipMemcpyAsync(m->d_tokens, &first_token, 4, hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
    {
        const int32_t hs[2] = { n_past, 0 };
        HIP_TRY(hipMemcpyAsync(m->d_state, hs, sizeof(hs), hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
    }
    const int nth = clamp_threads(n_threads);
    // (f16 / f32 / Q4_1 models: the un-fused single-row schedule is position-free as well, so it is captured too)
    const bool fusable = !(m->flags & LLAMAHIP_FLAG_UNFUSED) || m->dense;
    Pass pass(m);
    pass.n_threads = n_threads;
    pass.state_on_device = fusable;       // (published above, advanced by the pick; the un-fused Q4_0 pass takes n_past from the host)
    if (fusable && !(m->flags & LLAMAHIP_FLAG_NO_GRAPH)) {
        // One decode step (embed -> layers -> lm head -> argmax) captured once per n_threads value.
        // Nothing in it depends on the step: position and token slots live in device memory and
        // k_argmax advances them, so the same executable graph is replayed n_steps times.
        // Where the lm head's pick epilogue applies (EPI_STORE_PICK) the step is layers -> lm head alone: that launch picks the token,
        // advances the position and embeds the pick for the next step; only the FIRST token of the call is embedded by a launch of its own.
        static const bool no_fold = getenv("LLAMAHIP_NO_PICK_FOLD") != nullptr;
        const bool norm_default = norm_mode_resolve();
        const bool fold = !no_fold && norm_default && !m->dense && !(m->flags & LLAMAHIP_FLAG_UNFUSED) && m->w13_interleaved && m->l1 > m->l0 && gemv_pick_applies(m->output);
        pass.fold_pick = fold; pass.pick_out = m->d_out_tokens; pass.pick_next = m->d_tokens;
        if (fold) {
            // the first token's row, statistics and epoch (what k_embed_part does at the head of an un-folded step)
            const bool ep = m->d_attn_sync || m->d_pvx || m->d_w13_amax;
            HIP_TRY(launch_embed_part(m->d_tokens, m->tok_emb, m->x, m->hp.n_embd, m->npart_a, m->stream, ep ? m->d_epoch : nullptr), LLAMAHIP_ERR_PREDICT);
        }
        for (int i = 0; i < n_steps; i++) {
            pass.attn_sched = attn_sched_at(m, n_past + i);
            const int gkey = nth * 4096 + m->cur_seq + (pass.attn_sched << 24) + (fold ? 1 << 27 : 0);
            auto *g = m->decode_graphs.find(gkey);
            if (!g) {
                hipGraphExec_t exec = nullptr;
                rc = capture_step(m, [&]() -> int {
                    const int r = forward(m, pass, err, err_cap);
                    if (r || fold) return r;
                    HIP_TRY(launch_argmax(m->logits, m->hp.n_vocab, m->d_out_tokens, 0, m->d_tokens, m->d_state, m->stream), LLAMAHIP_ERR_PREDICT);
                    return 0;
                }, &exec, err, err_cap);
                if (rc) return rc;
                g = m->decode_graphs.put(gkey, exec);
            }
            HIP_TRY(hipGraphLaunch(g->exec, m->stream), LLAMAHIP_ERR_PREDICT);
        }
    } else {
        for (int i = 0; i < n_steps; i++) {
            pass.n_past = n_past + i;
            pass.attn_sched = attn_sched_at(m, n_past + i);
            rc = forward(m, pass, err, err_cap);
            if (rc) return rc;
            // argmax feeds the next step's token slot (and advances the position) on the device
            HIP_TRY(launch_argmax(m->logits, m->hp.n_vocab, m->d_out_tokens, i, m->d_tokens, m->d_state, m->stream), LLAMAHIP_ERR_PREDICT);
        }
    }
    if (out_tokens) HIP_TRY(hipMemcpyAsync(out_tokens, m->d_out_tokens, (size_t) n_steps * 4, hipMemcpyDeviceToHost, m->stream), LLAMAHIP_ERR_PREDICT);
    if (logits_last) HIP_TRY(hipMemcpyAsync(logits_last, m->logits, (size_t) m->hp.n_vocab * 4, hipMemcpyDeviceToHost, m->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
    if ((rc = check_sync_timeout(m, err, err_cap)) != 0) return rc;
    m->n_evals += n_steps;
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}

// ---- constrained greedy decoding (llamahip.h) ---------------------------------
// the device copy of a constraint's table: made by the first device call that uses it on its handle, registered with the handle's owner
static void cst_dev_release(llamahip_constraint *c) {
    llamahip_model *m = const_cast<llamahip_model *>(c->m);
    (void) hipSetDevice(m->device);
    (void) hipDeviceSynchronize();      // a captured step that reads the table may still run
    for (auto it = m->cst_graphs.map.begin(); it != m->cst_graphs.map.end();) {
        if (it->first.second != (const void *) c) { ++it; continue; }
        if (it->second.exec) (void) hipGraphExecDestroy(it->second.exec);
        it = m->cst_graphs.map.erase(it);
    }
    m->own.release(&c->dev);
    m->constraints.erase(std::remove(m->constraints.begin(), m->constraints.end(), c), m->constraints.end());
    c->dev_release = nullptr;
}
static int cst_ensure_dev(llamahip_model *m, llamahip_constraint *c, char *err, size_t err_cap) {
    if (!m->d_cst) HIP_TRY(m->own.alloc(&m->d_cst, (size_t) 2 * SET_MAX), LLAMAHIP_ERR_PREDICT);      // {state, dead} per sequence of a multi call
    if (c->dev) return 0;
    HIP_TRY(m->own.alloc(&c->dev, c->next.size()), LLAMAHIP_ERR_PREDICT);
    c->dev_release = cst_dev_release;
    m->constraints.push_back(c);
    HIP_TRY(hipMemcpy(c->dev, c->next.data(), c->next.size() * 2, hipMemcpyHostToDevice), LLAMAHIP_ERR_PREDICT);
    return 0;
}
// the contract itself: one-token llamahip_eval -> llamahip_constraint_pick -> llamahip_constraint_advance (pipeline handles run this)
static int cst_reference_loop(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token, int32_t n_steps, const llamahip_constraint *c,
                              int32_t *state_io, int32_t *out_tokens, int32_t *n_out, int32_t *finished, float *logits_last, char *err, size_t err_cap) {
    std::vector<float> row((size_t) m->hp.n_vocab);
    const int32_t done = c->n_states - 1;
    int32_t tok = first_token, state = *state_io, n = 0, fin = 0;
    while (n < n_steps && !fin) {
        const int rc = llamahip_eval(m, n_threads, n_past + n, &tok, 1, row.data(), err, err_cap);
        if (rc) return rc;
        tok = llamahip_constraint_pick(c, state, row.data());
        const int32_t q = tok < 0 ? -1 : llamahip_constraint_advance(c, state, tok);
        if (q < 0) { set_err(err, err_cap, "llamahip_decode_greedy_constrained: state %d allows no token (the state does not come from this constraint)", state); return LLAMAHIP_ERR_PREDICT; }
        out_tokens[n++] = tok;
        state = q;
        fin = state == done;
    }
    if (logits_last) memcpy(logits_last, row.data(), row.size() * 4);
    *state_io = state; *n_out = n; *finished = fin;
    return LLAMAHIP_OK;
}

int llamahip_decode_greedy_constrained(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token, int32_t n_steps, llamahip_constraint *c,
                                       int32_t *state_io, int32_t *out_tokens, int32_t *n_out, int32_t *finished, float *logits_last,
                                       char *err, size_t err_cap) {
    static const char *fn = "llamahip_decode_greedy_constrained";
    // the arguments first, without a device; the handle last
    if (!m || !c || !state_io || !out_tokens || !n_out || !finished) {
        set_err(err, err_cap, "%s: %s is NULL", fn, !m ? "model" : !c ? "constraint" : !state_io ? "state_io" : !out_tokens ? "out_tokens" : !n_out ? "n_out" : "finished");
        return LLAMAHIP_ERR_PREDICT;
    }
    if (c->m != m) { set_err(err, err_cap, "%s: the constraint was made on another handle", fn); return LLAMAHIP_ERR_PREDICT; }
    if (*state_io < 0 || *state_io >= c->n_states) { set_err(err, err_cap, "%s: state %d out of range [0, %d)", fn, *state_io, c->n_states); return LLAMAHIP_ERR_PREDICT; }
    if (first_token < 0 || first_token >= m->hp.n_vocab) { set_err(err, err_cap, "%s: token id %d out of range [0, %d)", fn, first_token, m->hp.n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (n_steps < 1) { set_err(err, err_cap, "%s: n_steps must be >= 1 (got %d)", fn, n_steps); return LLAMAHIP_ERR_PREDICT; }
    if (n_past < 0 || (int64_t) n_past + n_steps > m->hp.n_ctx) {
        set_err(err, err_cap, "%s: context overflow: n_past (%d) + n_steps (%d) > n_ctx (%d)", fn, n_past, n_steps, m->hp.n_ctx);
        return LLAMAHIP_ERR_PREDICT;
    }
    // (the front of a pipeline handle holds no device state of its own: its stages do)
    if (!m->stages.empty()) return cst_reference_loop(m, n_threads, n_past, first_token, n_steps, c, state_io, out_tokens, n_out, finished, logits_last, err, err_cap);
    if (m->host_only) { set_err(err, err_cap, "%s: model was loaded with LLAMAHIP_FLAG_HOST_ONLY: no device state, cannot evaluate", fn); return LLAMAHIP_ERR_PREDICT; }
    if (!m->first_stage || !m->last_stage) { set_err(err, err_cap, "%s: needs a whole-model handle (this one holds layers [%d, %d))", fn, m->l0, m->l1); return LLAMAHIP_ERR_PREDICT; }
    m->last_rows.clear();
    const double t0 = now_ms();
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    int rc = ensure_workspace(m, 1, err, err_cap);
    if (rc) return rc;
    if ((rc = cst_ensure_dev(m, c, err, err_cap)) != 0) return rc;
    if (!m->d_out_tokens) {      // sized once for the whole context: captured graphs hold this pointer
        HIP_TRY(m->own.alloc(&m->d_out_tokens, (size_t) m->hp.n_ctx), LLAMAHIP_ERR_PREDICT);
        m->out_tokens_cap = m->hp.n_ctx;
    }
    const int V = m->hp.n_vocab, nth = clamp_threads(n_threads), done = c->n_states - 1;
    const bool fusable = !(m->flags & LLAMAHIP_FLAG_UNFUSED) || m->dense;
    const bool graphs = fusable && !(m->flags & LLAMAHIP_FLAG_NO_GRAPH);
    Pass pass(m);
    pass.n_threads = n_threads;
    pass.state_on_device = fusable;
    DfaRows rows = {};
    rows.r[0] = { m->logits, c->dev, m->d_cst, m->d_out_tokens, m->d_tokens, m->d_state, c->n_states, c->stop_token, 0, 0 };
    // one step at position pos: llamahip_decode_greedy's un-folded step with k_pick_dfa in k_argmax's place
    auto step = [&](int pos) -> int {
        pass.attn_sched = attn_sched_at(m, pos);
        if (!graphs) {
            pass.n_past = pos;
            const int r = forward(m, pass, err, err_cap);
            if (r) return r;
            HIP_TRY(launch_pick_dfa(rows, 1, V, m->stream), LLAMAHIP_ERR_PREDICT);
            return 0;
        }
        const std::pair<int, const void *> gkey(nth * 4096 + m->cur_seq + (pass.attn_sched << 24) + (1 << 28), (const void *) c);
        auto *g = m->cst_graphs.find(gkey);
        if (!g) {
            hipGraphExec_t exec = nullptr;
            const int r = capture_step(m, [&]() -> int {
                const int rf = forward(m, pass, err, err_cap);
                if (rf) return rf;
                HIP_TRY(launch_pick_dfa(rows, 1, V, m->stream), LLAMAHIP_ERR_PREDICT);
                return 0;
            }, &exec, err, err_cap);
            if (r) return r;
            g = m->cst_graphs.put(gkey, exec);
        }
        HIP_TRY(hipGraphLaunch(g->exec, m->stream), LLAMAHIP_ERR_PREDICT);
        return 0;
    };
    // the device-resident words of step k: the token, {position, step index}, {state, dead}
    auto publish = [&](int32_t token, int32_t k, int32_t state) -> int {
        const int32_t hs[2] = { n_past + k, k }, hc[2] = { state, 0 };
        HIP_TRY(hipMemcpyAsync(m->d_tokens, &token, 4, hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipMemcpyAsync(m->d_state, hs, sizeof(hs), hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipMemcpyAsync(m->d_cst, hc, sizeof(hc), hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);      // (the words above are the caller's and this frame's)
        return 0;
    };
    // (measurement switch, read once per process: tools/constrain_probe.py sweeps the leg with it)
    static const int leg_env = getenv("LLAMAHIP_CONSTRAIN_LEG") ? atoi(getenv("LLAMAHIP_CONSTRAIN_LEG")) : 0;
    const int32_t leg_steps = leg_env >= 1 && leg_env <= 64 ? leg_env : LLAMAHIP_CONSTRAIN_LEG;
    if ((rc = publish(first_token, 0, *state_io)) != 0) return rc;
    int32_t ran = 0, hc[2] = { *state_io, 0 };
    do {      // (a state that comes in as DONE still takes a step: the stop token, as the reference loop)
        const int32_t leg = std::min<int32_t>(leg_steps, n_steps - ran);
        for (int32_t i = 0; i < leg; i++) if ((rc = step(n_past + ran + i)) != 0) return rc;
        ran += leg;
        HIP_TRY(hipMemcpyAsync(hc, m->d_cst, sizeof(hc), hipMemcpyDeviceToHost, m->stream), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
        if ((rc = check_sync_timeout(m, err, err_cap)) != 0) return rc;
        if (hc[1] != 0 || hc[0] < 0 || hc[0] >= c->n_states) {
            set_err(err, err_cap, "%s: a pick found no allowed token (state word %d, dead %d): the state does not come from this constraint", fn, hc[0], hc[1]);
            return LLAMAHIP_ERR_PREDICT;
        }
    } while (ran < n_steps && hc[0] != done);
    HIP_TRY(hipMemcpy(out_tokens, m->d_out_tokens, (size_t) ran * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    const int32_t fin = hc[0] == done;
    int32_t n = ran;
    if (fin) for (n = 0; n < ran && out_tokens[n] != c->stop_token; n++) {}
    if (fin) n = std::min(n + 1, ran);      // the stop token counts; what a leg produced behind it (stop tokens in DONE) is not reported
    if (logits_last && n < ran) {
        // the leg ran past the stop token: m->logits holds a later step's row.  The step that picked the stop token once more, from the words it
        // had then -- the same launches on the same operands, so the same bits, and KV row n_past + n - 1 is rewritten with what it holds
        int32_t state = *state_io;
        for (int32_t k = 0; k + 1 < n; k++) state = llamahip_constraint_advance(c, state, out_tokens[k]);
        if ((rc = publish(n >= 2 ? out_tokens[n - 2] : first_token, n - 1, state)) != 0) return rc;
        if ((rc = step(n_past + n - 1)) != 0) return rc;
    }
    if (logits_last) HIP_TRY(hipMemcpyAsync(logits_last, m->logits, (size_t) V * 4, hipMemcpyDeviceToHost, m->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
    if ((rc = check_sync_timeout(m, err, err_cap)) != 0) return rc;
    *state_io = hc[0]; *n_out = n; *finished = fin;
    m->n_evals += ran;
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}

// ---- asynchronous pipeline-stage steps ---------------------------------------------------------
// f16 / f32 files have stage steps (and set steps) on whole-model handles only; Q4_1 files have none
static bool dense_stage_steps(const llamahip_model *m) { return m->dense && m->hp.f16 != 3 && m->first_stage && m->last_stage; }
int llamahip_stage_bind(llamahip_model *m, int32_t seq, int32_t n_past,
                        void *token_in, const void *hidden_in, void *hidden_out, void *token_out,
                        char *err, size_t err_cap) {
    PIPE_REFUSE(m, "llamahip_stage_bind");
    if (!m) { set_err(err, err_cap, "null model"); return LLAMAHIP_ERR_PREDICT; }
    if (m->host_only) { set_err(err, err_cap, "model was loaded with LLAMAHIP_FLAG_HOST_ONLY: no device state, cannot evaluate"); return LLAMAHIP_ERR_PREDICT; }
    if (seq < 0 || seq >= m->n_seq) { set_err(err, err_cap, "sequence slot %d out of range [0, %d)", seq, m->n_seq); return LLAMAHIP_ERR_PREDICT; }
    if (n_past < 0 || n_past >= m->hp.n_ctx) { set_err(err, err_cap, "context overflow: n_past (%d) + n_tokens (1) > n_ctx (%d)", n_past, m->hp.n_ctx); return LLAMAHIP_ERR_PREDICT; }
    if ((m->flags & LLAMAHIP_FLAG_UNFUSED) || m->hp.f16 == 3) { set_err(err, err_cap, "llamahip_stage_step needs a captured decode step (LLAMAHIP_FLAG_UNFUSED handle or Q4_1 model): use llamahip_eval_stage"); return LLAMAHIP_ERR_PREDICT; }
    if (m->dense && !(m->first_stage && m->last_stage)) { set_err(err, err_cap, "llamahip_stage_step on an f16 / f32 model needs a whole-model handle (this one holds layers [%d, %d)): use llamahip_eval_stage", m->l0, m->l1); return LLAMAHIP_ERR_PREDICT; }
    if (m->first_stage && !token_in) { set_err(err, err_cap, "stage [%d,%d) is the first stage: token_in is required", m->l0, m->l1); return LLAMAHIP_ERR_PREDICT; }
    {   // (a slot with device-side mailboxes needs no hidden_in / hidden_out buffers: llamahip_stage_mailbox / _connect)
        const bool has_slot = seq < (int32_t) m->slots.size();
        const bool mb_in = has_slot && m->slots[seq].inbox_hidden, mb_out = has_slot && m->slots[seq].peer_hidden;
        if (!m->first_stage && !hidden_in && !mb_in) { set_err(err, err_cap, "stage [%d,%d) needs hidden_in", m->l0, m->l1); return LLAMAHIP_ERR_PREDICT; }
        if (!m->last_stage && !hidden_out && !mb_out) { set_err(err, err_cap, "stage [%d,%d) needs hidden_out", m->l0, m->l1); return LLAMAHIP_ERR_PREDICT; }
    }
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    if (token_in) {
        // the step's first kernel reads the token word on the device: an address the runtime does not know (a host variable, a stray integer)
        // would fault the GPU at the first step instead of failing here
        hipPointerAttribute_t pa;
        if (hipPointerGetAttributes(&pa, token_in) != hipSuccess || pa.type == hipMemoryTypeUnregistered || !pa.devicePointer) {
            (void) hipGetLastError();
            set_err(err, err_cap, "llamahip_stage_bind: token_in %p is not device-accessible memory (stage steps read the token on the device; with tokens on the host use llamahip_eval_stage)", token_in);
            return LLAMAHIP_ERR_PREDICT;
        }
    }
    int rc = ensure_workspace(m, 1, err, err_cap);
    if (rc) return rc;
    if ((rc = ensure_slots(m, err, err_cap)) != 0) return rc;
    auto &sl = m->slots[seq];
    const bool same = sl.bound && sl.token_in == token_in && sl.token_out == token_out && sl.hidden_in == hidden_in && sl.hidden_out == hidden_out;
    if (!same) {                 // captured graphs hold the old pointers (and may still run on a caller stream: device-wide wait)
        HIP_TRY(hipDeviceSynchronize(), LLAMAHIP_ERR_PREDICT);
        sl.graphs.clear();
        drop_set_graphs(m);
    }
    sl.token_in = (int32_t *) token_in; sl.token_out = (int32_t *) token_out;
    sl.hidden_in = (const float *) hidden_in; sl.hidden_out = (float *) hidden_out;
    sl.bound = true;
    sl.next_pos = n_past;
    const int32_t hs[2] = { n_past, 0 };
    HIP_TRY(hipMemcpy(m->d_slot_state + 2 * seq, hs, sizeof(hs), hipMemcpyHostToDevice), LLAMAHIP_ERR_PREDICT);
    // mailboxes: stale rows of an earlier binding must not match; the first stage's first token is the caller's (token_in), published
    // to its own token inbox with the tag of the position it is for
    if (sl.inbox_hidden) HIP_TRY(hipMemset(sl.inbox_hidden, 0, (size_t) m->hp.n_embd * 8), LLAMAHIP_ERR_PREDICT);
    if (sl.inbox_token) {
        int32_t tok = 0;
        HIP_TRY(hipMemcpy(&tok, token_in, 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
        const uint64_t g = (uint64_t) (uint32_t) tok | ((uint64_t) ((((uint32_t) n_past + 1u) << 8) | 0u) << 32);      // make_tag(n_past + 1, 0)
        HIP_TRY(hipMemcpy(sl.inbox_token, &g, 8, hipMemcpyHostToDevice), LLAMAHIP_ERR_PREDICT);
    }
    return LLAMAHIP_OK;
}

namespace {
static int drop_slot_graphs(llamahip_model *m, int seq, char *err, size_t err_cap) {
    HIP_TRY(hipDeviceSynchronize(), LLAMAHIP_ERR_PREDICT);
    m->slots[seq].graphs.clear();
    return 0;
}
}  // namespace

// ---- device-side mailboxes between pipeline stages (include/llamahip.h) -------------------------
int llamahip_stage_mailbox(llamahip_model *m, int32_t seq, void **hidden_inbox, void **token_inbox,
                           void *hidden_handle64, void *token_handle64, char *err, size_t err_cap) {
    PIPE_REFUSE(m, "llamahip_stage_mailbox");
    if (!m) { set_err(err, err_cap, "null model"); return LLAMAHIP_ERR_PREDICT; }
    if (m->host_only || m->dense || (m->flags & LLAMAHIP_FLAG_UNFUSED) || !m->w13_interleaved || m->l1 <= m->l0) {
        set_err(err, err_cap, "pipeline mailboxes need a Q4_0 stage handle with layers and the fused decode schedule"); return LLAMAHIP_ERR_PREDICT; }
    if (seq < 0 || seq >= m->n_seq) { set_err(err, err_cap, "sequence slot %d out of range [0, %d)", seq, m->n_seq); return LLAMAHIP_ERR_PREDICT; }
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    int rc = ensure_slots(m, err, err_cap);
    if (rc) return rc;
    auto &sl = m->slots[seq];
    if (!m->first_stage && !sl.inbox_hidden) {
        if ((rc = drop_slot_graphs(m, seq, err, err_cap)) != 0) return rc;
        HIP_TRY(m->own.alloc(&sl.inbox_hidden, (size_t) m->hp.n_embd, true, MEM_MAILBOX), LLAMAHIP_ERR_PREDICT);
    }
    if (m->first_stage && !m->last_stage && !sl.inbox_token) {
        if ((rc = drop_slot_graphs(m, seq, err, err_cap)) != 0) return rc;
        HIP_TRY(m->own.alloc(&sl.inbox_token, 8, true, MEM_MAILBOX), LLAMAHIP_ERR_PREDICT);
    }
    if (hidden_inbox) *hidden_inbox = sl.inbox_hidden;
    if (token_inbox) *token_inbox = sl.inbox_token;
    if (hidden_handle64 && sl.inbox_hidden) {
        hipIpcMemHandle_t h;
        HIP_TRY(hipIpcGetMemHandle(&h, sl.inbox_hidden), LLAMAHIP_ERR_PREDICT);
        static_assert(sizeof(h) == 64, "hipIpcMemHandle_t is 64 bytes");
        memcpy(hidden_handle64, &h, 64);
    }
    if (token_handle64 && sl.inbox_token) {
        hipIpcMemHandle_t h;
        HIP_TRY(hipIpcGetMemHandle(&h, sl.inbox_token), LLAMAHIP_ERR_PREDICT);
        memcpy(token_handle64, &h, 64);
    }
    return LLAMAHIP_OK;
}

int llamahip_stage_mailbox_connect(llamahip_model *m, int32_t seq, const void *next_hidden_handle64, void *next_hidden_ptr,
                                   const void *token_handle64, void *token_ptr, char *err, size_t err_cap) {
    PIPE_REFUSE(m, "llamahip_stage_mailbox_connect");
    if (!m) { set_err(err, err_cap, "null model"); return LLAMAHIP_ERR_PREDICT; }
    if (m->host_only || m->dense || (m->flags & LLAMAHIP_FLAG_UNFUSED) || !m->w13_interleaved || m->l1 <= m->l0) {
        set_err(err, err_cap, "pipeline mailboxes need a Q4_0 stage handle with layers and the fused decode schedule"); return LLAMAHIP_ERR_PREDICT; }
    if (seq < 0 || seq >= m->n_seq) { set_err(err, err_cap, "sequence slot %d out of range [0, %d)", seq, m->n_seq); return LLAMAHIP_ERR_PREDICT; }
    if ((next_hidden_handle64 || next_hidden_ptr) && m->last_stage) { set_err(err, err_cap, "the last stage has no next stage to hand its row to"); return LLAMAHIP_ERR_PREDICT; }
    if ((token_handle64 || token_ptr) && (!m->last_stage || m->first_stage)) { set_err(err, err_cap, "only the last stage of a multi-stage pipeline feeds the token back"); return LLAMAHIP_ERR_PREDICT; }
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    int rc = ensure_slots(m, err, err_cap);
    if (rc) return rc;
    if ((rc = drop_slot_graphs(m, seq, err, err_cap)) != 0) return rc;
    auto &sl = m->slots[seq];
    auto open = [&](const void *h64, void *raw, uint64_t **dst, bool *ipc) -> int {
        if (!h64 && !raw) return 0;
        if (*dst && *ipc) (void) hipIpcCloseMemHandle(*dst);
        *dst = nullptr; *ipc = false;
        if (raw) { *dst = (uint64_t *) raw; return 0; }
        hipIpcMemHandle_t h;
        memcpy(&h, h64, 64);
        void *p = nullptr;
        HIP_TRY(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess), LLAMAHIP_ERR_PREDICT);
        *dst = (uint64_t *) p; *ipc = true;
        return 0;
    };
    if ((rc = open(next_hidden_handle64, next_hidden_ptr, &sl.peer_hidden, &sl.peer_hidden_ipc)) != 0) return rc;
    if ((rc = open(token_handle64, token_ptr, &sl.peer_token, &sl.peer_token_ipc)) != 0) return rc;
    return LLAMAHIP_OK;
}

namespace {
// the launches of one stage step, issued on `st` (the caller's stream, or the handle's under capture)
static int stage_step_launches(llamahip_model *m, int seq, int nth, int attn_sched, hipStream_t st, char *err, size_t err_cap) {
    auto &sl = m->slots[seq];
    int32_t *state = m->d_slot_state + 2 * seq;
    Pass pass(m);
    pass.n_threads = nth; pass.hidden_in = sl.hidden_in; pass.seq = seq; pass.stream = st;
    pass.state_on_device = true; pass.state = state; pass.attn_sched = attn_sched;
    if (sl.token_in) pass.tokens = sl.token_in;
    pass.x_first = m->first_stage ? nullptr : sl.hidden_in;
    pass.x_last = m->last_stage ? nullptr : sl.hidden_out;
    // a slot bound WITHOUT hidden buffers runs on its mailboxes; one bound with them keeps the caller-ordered buffers (RCCL schedule)
    // even if mailboxes exist -- the way back when the mailbox handshake of a multi-GPU run fails
    const bool mb_mode = (m->first_stage || !sl.hidden_in) && (m->last_stage || !sl.hidden_out) && !(m->first_stage && m->last_stage);
    pass.mb_in = (mb_mode && !m->first_stage) ? sl.inbox_hidden : nullptr;
    pass.mb_out = (mb_mode && !m->last_stage) ? sl.peer_hidden : nullptr;
    pass.mb_token = (mb_mode && m->first_stage) ? sl.inbox_token : nullptr;
    uint64_t *mb_token_out = (mb_mode && m->last_stage) ? sl.peer_token : nullptr;
    int rc = forward(m, pass, err, err_cap);
    if (rc) return rc;
    const size_t d = m->hp.n_embd;
    if (!m->last_stage && m->l1 == m->l0)           // a stage without layers only forwards the stream
        HIP_TRY(hipMemcpyAsync(sl.hidden_out, m->x, d * 4, hipMemcpyDeviceToDevice, st), LLAMAHIP_ERR_PREDICT);
    if (m->last_stage) {
        // greedy pick on the device: trace[step] = token; token_out (if any) = token; position advances
        HIP_TRY(launch_argmax(m->logits, m->hp.n_vocab, m->d_slot_trace + (size_t) seq * m->hp.n_ctx, 0, sl.token_out, state, st, mb_token_out), LLAMAHIP_ERR_PREDICT);
    } else {
        HIP_TRY(launch_advance(state, st), LLAMAHIP_ERR_PREDICT);
    }
    return 0;
}
}  // namespace

int llamahip_stage_step(llamahip_model *m, int32_t seq, int32_t n_threads, void *stream, char *err, size_t err_cap) {
    PIPE_REFUSE(m, "llamahip_stage_step");
    if (!m) { set_err(err, err_cap, "null model"); return LLAMAHIP_ERR_PREDICT; }
    if (seq < 0 || seq >= (int32_t) m->slots.size() || !m->slots[seq].bound) { set_err(err, err_cap, "sequence slot %d is not bound (llamahip_stage_bind)", seq); return LLAMAHIP_ERR_PREDICT; }
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    const int nth = clamp_threads(n_threads);
    hipStream_t run_on = (hipStream_t) stream;          // NULL = the null stream, as everywhere in HIP
    auto &sl = m->slots[seq];
    if (sl.next_pos >= m->hp.n_ctx) { set_err(err, err_cap, "context overflow: n_past (%d) + n_tokens (1) > n_ctx (%d)", sl.next_pos, m->hp.n_ctx); return LLAMAHIP_ERR_PREDICT; }
    const int attn_sched = attn_sched_at(m, sl.next_pos);
    if (m->flags & LLAMAHIP_FLAG_NO_GRAPH) {
        const int rc = stage_step_launches(m, seq, nth, attn_sched, run_on, err, err_cap);
        if (rc) return rc;
    } else {
        const int gkey = nth + (attn_sched << 16);
        auto *g = sl.graphs.find(gkey);
        if (!g) {
            // One step of this stage (embed | stream in -> layers -> stream out | lm head + argmax)
            // captured once per (slot, n_threads); the position lives in device memory and the last
            // node advances it, so the same executable graph is replayed for every token.
            hipGraphExec_t exec = nullptr;
            const int rc = capture_step(m, [&]() { return stage_step_launches(m, seq, nth, attn_sched, m->stream, err, err_cap); }, &exec, err, err_cap);
            if (rc) return rc;
            g = sl.graphs.put(gkey, exec);
        }
        HIP_TRY(hipGraphLaunch(g->exec, run_on), LLAMAHIP_ERR_PREDICT);
    }
    sl.next_pos++;
    m->n_evals++;
    m->last_rows.clear();
    return LLAMAHIP_OK;
}

namespace {
// One decode step for B rows = B sequences (device-resident descriptor `d_set`): the 2..60-row schedule of forward_eval -- every operator of
// llama_eval's graph works row by row (.mm:563-705), so row b is bit for bit a single-token llama_eval of its sequence: its own
// position in RoPE / the KV append / the causal range, its own cache, and the V*P key split of ITS eval, n_past_b + 1 keys over
// n_threads (ggml.c:5459-5480).  The weights are streamed once per step for all rows.
// (tail = false, a verify step over a set: the rows stay where they are -- logits on the last stage, m->x on the others -- and no slot advances)
// f16 / f32 files: the same step on the dense schedule of forward_dense -- per mat-mul k_dense_prep + the few-row dense mat-mul (one pass over
// the weights for all rows: launch_dense_mm), RoPE and the KV append per row of the set (k_rope_kv_set), launch_attn_short with fp32 merged rows
static int forward_dense_set(llamahip_model *m, int nth, SeqSet *d_set, int B, hipStream_t st, char *err, size_t err_cap, int set_keys, bool tail) {
    const HParams &hp = m->hp;
    const int d = hp.n_embd, F = hp.n_ff, H = hp.n_head, dh = d / H, C = hp.n_ctx, V = hp.n_vocab;
    if (m->first_stage) HIP_TRY(launch_embed_dense_set(d_set, B, m->tok_emb, hp.f16, m->x, d, st), LLAMAHIP_ERR_PREDICT);                          // .mm:558-561
    else HIP_TRY(launch_rows_set(d_set, B, m->x, d, true, st), LLAMAHIP_ERR_PREDICT);
    for (int il = m->l0; il < m->l1; il++) {
        const Layer &L = m->layers[il - m->l0];
        float *Kl = m->Kc + (size_t) (il - m->l0) * C * d, *Vl = m->Vc + (size_t) (il - m->l0) * C * d;      // slot 0's cache of this layer; rows add their slot's offset
        HIP_TRY(dense_prep_mm(m, L.dqkv, EPI_STORE, PREP_NORM, m->x, L.attention_norm, d, 0, d, B, m->qkv, 3L * d, nullptr, 0, st), LLAMAHIP_ERR_PREDICT);        // .mm:570-582
        HIP_TRY(launch_rope_kv_set(m->qkv, 3L * d, d, dh, m->sincos, m->qr, Kl, Vl, d_set, B, st), LLAMAHIP_ERR_PREDICT);                           // .mm:586-611
        HIP_TRY(launch_attn_short(m->qr, Kl, Vl, m->set_sc, m->merged, m->qa_A, m->qa_d, 0, B, d, H, C, nth, m->T_exp, st, 0, d_set, set_keys), LLAMAHIP_ERR_PREDICT);   // .mm:614-646
        HIP_TRY(dense_prep_mm(m, L.dwo, EPI_RESID, PREP_PLAIN, m->merged, nullptr, d, 0, d, B, m->x1, d, m->x, d, st), LLAMAHIP_ERR_PREDICT);                     // .mm:649-654
        HIP_TRY(dense_prep_mm(m, L.dw13, EPI_STORE, PREP_NORM, m->x1, L.ffn_norm, d, 0, d, B, m->gu, 2L * F, nullptr, 0, st), LLAMAHIP_ERR_PREDICT);              // .mm:660-675
        HIP_TRY(dense_prep_mm(m, L.dw2, EPI_RESID, PREP_SILU_MUL, m->gu, m->gu + F, 2L * F, 2L * F, F, B, m->x, d, m->x1, d, st), LLAMAHIP_ERR_PREDICT);          // .mm:678-687
    }
    if (m->last_stage) {
        HIP_TRY(dense_prep_mm(m, m->doutput, EPI_STORE, PREP_NORM, m->x, m->norm_w, d, 0, d, B, m->logits, V, nullptr, 0, st), LLAMAHIP_ERR_PREDICT);             // .mm:695-705
        if (tail) HIP_TRY(launch_argmax_set(m->logits, V, d_set, B, st), LLAMAHIP_ERR_PREDICT);
    } else if (tail) {
        HIP_TRY(launch_rows_set(d_set, B, m->x, d, false, st), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(launch_advance_set(d_set, B, st), LLAMAHIP_ERR_PREDICT);
    }
    return 0;
}
static int forward_set(llamahip_model *m, int nth, SeqSet *d_set, int B, hipStream_t st, char *err, size_t err_cap, int set_keys = 0, bool tail = true) {
    if (m->dense) return forward_dense_set(m, nth, d_set, B, st, err, err_cap, set_keys, tail);
    const HParams &hp = m->hp;
    const int d = hp.n_embd, F = hp.n_ff, H = hp.n_head, dh = d / H, C = hp.n_ctx, V = hp.n_vocab;
    const long KpF = ((long) F + 255) / 256 * 256;
    SiluHalfIO set_hx;          // (see forward_eval: the half-block w1|w3 launch of k_gemv_set; the step's first launch opens the epoch)
    if (m->d_attn_sync && m->d_set_amax && m->l1 - m->l0 <= TAG_MAX_LAYERS) { set_hx.amax_t = m->d_set_amax; set_hx.epoch = m->d_epoch; set_hx.fault = m->d_fault; }
    if (m->first_stage) HIP_TRY(launch_embed_set(d_set, B, m->tok_emb, m->x, d, st, set_hx.amax_t ? m->d_epoch : nullptr), LLAMAHIP_ERR_PREDICT);                // .mm:558-561
    else HIP_TRY(launch_rows_set(d_set, B, m->x, d, true, st, set_hx.amax_t ? m->d_epoch : nullptr), LLAMAHIP_ERR_PREDICT);
    for (int il = m->l0; il < m->l1; il++) {
        const Layer &L = m->layers[il - m->l0];
        set_hx.layer = il - m->l0;
        float *Kl = m->Kc + (size_t) (il - m->l0) * C * d, *Vl = m->Vc + (size_t) (il - m->l0) * C * d;      // slot 0's cache of this layer; rows add their slot's offset
        HIP_TRY(launch_prep(PREP_NORM, m->x, L.attention_norm, d, 0, d, B, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);   // .mm:570-575
        RopeKvArgs ra = { m->sincos, m->qr, Kl, Vl, 0, d, dh };
        ra.set = d_set;
        HIP_TRY(launch_gemm_rope_kv(L.qkv, m->qa_A, m->qa_d, B, ra, st), LLAMAHIP_ERR_PREDICT);                                // .mm:580-611
        HIP_TRY(launch_attn_short(m->qr, Kl, Vl, m->set_sc, nullptr, m->qa_A, m->qa_d, 0, B, d, H, C, nth, m->T_exp, st, 0, d_set, set_keys), LLAMAHIP_ERR_PREDICT);   // .mm:614-646
        HIP_TRY(launch_gemm(L.wo, EPI_RESID, m->qa_A, m->qa_d, B, m->x1, d, m->x, d, st, m->qb_ws, false), LLAMAHIP_ERR_PREDICT);  // .mm:649-654
        HIP_TRY(launch_prep(PREP_NORM, m->x1, L.ffn_norm, d, 0, d, B, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);        // .mm:660-665
        if (m->w13_interleaved && gemm_silu_qa_applies(L.w13, B)) {
            HIP_TRY(launch_gemm_silu_qa(L.w13, m->qa_A, m->qa_d, B, m->T_silu, m->qaF_A, m->qaF_d, KpF / 4, KpF / 32, st, &set_hx), LLAMAHIP_ERR_PREDICT);       // .mm:668-680
            HIP_TRY(launch_gemm(L.w2, EPI_RESID, m->qaF_A, m->qaF_d, B, m->x, d, m->x1, d, st, m->qb_ws, false), LLAMAHIP_ERR_PREDICT);                 // .mm:682-687
        } else {
            HIP_TRY(launch_gemm(L.w13, EPI_STORE, m->qa_A, m->qa_d, B, m->gu, 2L * F, nullptr, 0, st, m->qb_ws, false), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(launch_prep(PREP_SILU_MUL, m->gu, m->gu + F, 2L * F, 2L * F, F, B, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(launch_gemm(L.w2, EPI_RESID, m->qa_A, m->qa_d, B, m->x, d, m->x1, d, st, m->qb_ws, false), LLAMAHIP_ERR_PREDICT);
        }
    }
    if (m->last_stage) {
        HIP_TRY(launch_prep(PREP_NORM, m->x, m->norm_w, d, 0, d, B, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);          // .mm:695-705
        HIP_TRY(launch_gemm(m->output, EPI_STORE, m->qa_A, m->qa_d, B, m->logits, V, nullptr, 0, st), LLAMAHIP_ERR_PREDICT);
        if (tail) HIP_TRY(launch_argmax_set(m->logits, V, d_set, B, st), LLAMAHIP_ERR_PREDICT);
    } else if (tail) {
        HIP_TRY(launch_rows_set(d_set, B, m->x, d, false, st), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(launch_advance_set(d_set, B, st), LLAMAHIP_ERR_PREDICT);
    }
    return 0;
}
}  // namespace

// 1 if llamahip_stage_step_set can step `n_seqs` slots of this handle with this n_threads as one set, 0 if the caller has to step them one
// by one (llamahip_stage_step takes up to 64 threads and every handle shape)
int32_t llamahip_stage_set_applies(const llamahip_model *m, int32_t n_seqs, int32_t n_threads) {
    if (!m || m->host_only || n_seqs < 1 || n_seqs > SET_MAX) return 0;
    if (n_seqs == 1) return 1;
    const int d = m->hp.n_embd, H = m->hp.n_head, dh = H > 0 ? d / H : 0;
    const int nth = clamp_threads(n_threads);
    if ((m->flags & LLAMAHIP_FLAG_UNFUSED) || m->l1 <= m->l0 || dh <= 0 || dh % 32 != 0 || dh > 256 || nth > 32) return 0;
    if (m->dense) return dense_stage_steps(m) ? 1 : 0;      // (f16 / f32 whole-model handles: the few-row dense mat-mul takes every width the loader takes)
    return gemm_rope_kv_applies(m->layers[0].qkv, n_seqs, d) ? 1 : 0;
}

int llamahip_stage_step_set(llamahip_model *m, const int32_t *seqs, int32_t n_seqs, int32_t n_threads, void *stream, char *err, size_t err_cap) {
    PIPE_REFUSE(m, "llamahip_stage_step_set");
    if (!m) { set_err(err, err_cap, "null model"); return LLAMAHIP_ERR_PREDICT; }
    if (!seqs || n_seqs < 1 || n_seqs > SET_MAX) { set_err(err, err_cap, "llamahip_stage_step_set: 1 .. %d slots per step (got %d)", SET_MAX, n_seqs); return LLAMAHIP_ERR_PREDICT; }
    if (n_seqs == 1) return llamahip_stage_step(m, seqs[0], n_threads, stream, err, err_cap);
    const HParams &hp = m->hp;
    const int d = hp.n_embd, H = hp.n_head, dh = d / H, C = hp.n_ctx;
    const int nth = clamp_threads(n_threads);
    for (int i = 0; i < n_seqs; i++) {
        const int sq = seqs[i];
        if (sq < 0 || sq >= (int32_t) m->slots.size() || !m->slots[sq].bound) { set_err(err, err_cap, "sequence slot %d is not bound (llamahip_stage_bind)", sq); return LLAMAHIP_ERR_PREDICT; }
        for (int j = 0; j < i; j++) if (seqs[j] == sq) { set_err(err, err_cap, "sequence slot %d appears twice in the set", sq); return LLAMAHIP_ERR_PREDICT; }
        const auto &sl = m->slots[sq];
        if (sl.next_pos >= C) { set_err(err, err_cap, "context overflow: n_past (%d) + n_tokens (1) > n_ctx (%d)", sl.next_pos, C); return LLAMAHIP_ERR_PREDICT; }
        if ((!m->first_stage && !sl.hidden_in) || (!m->last_stage && !sl.hidden_out)) { set_err(err, err_cap, "slot %d runs on its mailboxes: set steps need slots bound with hidden_in / hidden_out buffers", sq); return LLAMAHIP_ERR_PREDICT; }
    }
    if ((m->dense && !dense_stage_steps(m)) || (m->flags & LLAMAHIP_FLAG_UNFUSED) || m->l1 <= m->l0 || dh % 32 != 0 || dh > 256 || nth > 32 ||
        (!m->dense && !gemm_rope_kv_applies(m->layers[0].qkv, n_seqs, d))) {
        set_err(err, err_cap, "llamahip_stage_step_set needs a Q4_0 handle with layers or an f16 / f32 whole-model handle, a head size that is a multiple of 32 (<= 256) and n_threads <= 32: step the slots one by one");
        return LLAMAHIP_ERR_PREDICT;
    }
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    int rc = ensure_workspace(m, SET_MAX, err, err_cap);
    if (rc) return rc;
    if ((rc = ensure_set_sc(m, err, err_cap)) != 0) return rc;
    hipStream_t run_on = (hipStream_t) stream;
    // The rows of a step are independent (every sequence's results are those of stepping it alone), so a set is its slots in ascending
    // order: [0, 1] and [1, 0] share one captured graph and one device descriptor.  A server whose active set keeps changing would
    // otherwise accumulate graphs of hundreds of kernel nodes: the map is bounded, the least recently used set goes.
    constexpr size_t SET_GRAPHS_MAX = 32;
    std::vector<int> order(seqs, seqs + n_seqs);
    std::sort(order.begin(), order.end());
    // The score launch of a step covers the key slices up to the set's highest position, in buckets of SET_KEY_BUCKET positions: the host
    // tracks every slot's position (next_pos), a captured step is keyed by its bucket and replayed until a row crosses into the next one
    // (n_ctx / 128 captures per set at most; the launch used to cover every slice of n_ctx whatever the positions -- ADVICE r04).
    int max_pos = 0;
    for (int i = 0; i < n_seqs; i++) max_pos = std::max(max_pos, m->slots[seqs[i]].next_pos);
    const int set_keys = set_key_bucket(C, max_pos);
    std::vector<int> key;
    key.push_back(nth);
    key.push_back(set_keys);
    for (int i = 0; i < n_seqs; i++) key.push_back(order[i]);
    auto *g = m->set_graphs.find(key);
    if (!g) {
        if (m->set_graphs.size() >= SET_GRAPHS_MAX) {
            auto victim = m->set_graphs.map.begin();
            for (auto jt = m->set_graphs.map.begin(); jt != m->set_graphs.map.end(); ++jt) if (jt->second.last_use < victim->second.last_use) victim = jt;
            HIP_TRY(hipDeviceSynchronize(), LLAMAHIP_ERR_PREDICT);          // its graph may still run on a caller's stream
            m->own.release(&victim->second.d_set);
            m->set_graphs.erase(victim->first);
        }
        SeqSet hs;
        memset(&hs, 0, sizeof(hs));
        hs.n = n_seqs;
        for (int i = 0; i < n_seqs; i++) {
            const int sq = order[i];
            const auto &sl = m->slots[sq];
            hs.state[i] = m->d_slot_state + 2 * sq;
            hs.tok_in[i] = sl.token_in; hs.tok_out[i] = sl.token_out;
            hs.trace[i] = m->d_slot_trace + (size_t) sq * C;
            hs.hid_in[i] = sl.hidden_in; hs.hid_out[i] = sl.hidden_out;
            hs.kv_off[i] = (long) ((size_t) sq * (m->l1 - m->l0) * C * d);
        }
        llamahip_model::SetGraph sg;
        hipGraphExec_t exec = nullptr;
        HIP_TRY(m->own.alloc(&sg.d_set, 1), LLAMAHIP_ERR_PREDICT);
        if (hipMemcpy(sg.d_set, &hs, sizeof(SeqSet), hipMemcpyHostToDevice) != hipSuccess) { m->own.release(&sg.d_set); set_err(err, err_cap, "HIP error copying the set descriptor"); return LLAMAHIP_ERR_PREDICT; }
        if (!(m->flags & LLAMAHIP_FLAG_NO_GRAPH) &&
            (rc = capture_step(m, [&]() { return forward_set(m, nth, sg.d_set, n_seqs, m->stream, err, err_cap, set_keys); }, &exec, err, err_cap)) != 0) {
            m->own.release(&sg.d_set);
            return rc;
        }
        g = m->set_graphs.put(key, exec, sg);
        m->n_set_captures++;
    }
    g->last_use = ++m->set_graph_clock;
    m->last_rows.assign(n_seqs, 0);
    for (int i = 0; i < n_seqs; i++) m->last_rows[i] = (int) (std::lower_bound(order.begin(), order.end(), seqs[i]) - order.begin());
    if (g->exec) HIP_TRY(hipGraphLaunch(g->exec, run_on), LLAMAHIP_ERR_PREDICT);
    else if ((rc = forward_set(m, nth, g->d_set, n_seqs, run_on, err, err_cap, set_keys)) != 0) return rc;
    for (int i = 0; i < n_seqs; i++) m->slots[seqs[i]].next_pos++;
    m->n_evals += n_seqs;
    return LLAMAHIP_OK;
}

int llamahip_stage_trace(llamahip_model *m, int32_t seq, int32_t *n_past, int32_t *tokens, int32_t cap, char *err, size_t err_cap) {
    PIPE_REFUSE(m, "llamahip_stage_trace");
    if (!m) { set_err(err, err_cap, "null model"); return LLAMAHIP_ERR_PREDICT; }
    if (seq < 0 || seq >= (int32_t) m->slots.size() || !m->slots[seq].bound) { set_err(err, err_cap, "sequence slot %d is not bound (llamahip_stage_bind)", seq); return LLAMAHIP_ERR_PREDICT; }
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    int32_t hs[2] = { 0, 0 };
    HIP_TRY(hipDeviceSynchronize(), LLAMAHIP_ERR_PREDICT);       // steps may be in flight on any caller stream
    { const int rc = check_sync_timeout(m, err, err_cap); if (rc) return rc; }     // a hand-off of one of those steps that timed out: their results are invalid
    HIP_TRY(hipMemcpy(hs, m->d_slot_state + 2 * seq, sizeof(hs), hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    if (n_past) *n_past = hs[0];
    const int n = std::min(std::min(hs[1], cap), m->hp.n_ctx);
    if (tokens && m->last_stage && n > 0)
        HIP_TRY(hipMemcpy(tokens, m->d_slot_trace + (size_t) seq * m->hp.n_ctx, (size_t) n * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    return hs[1];
}

int llamahip_stage_logits(llamahip_model *m, int32_t row, float *logits_out, char *err, size_t err_cap) {
    PIPE_REFUSE(m, "llamahip_stage_logits");
    if (!m || m->host_only || !logits_out) { set_err(err, err_cap, "bad arguments"); return LLAMAHIP_ERR_PREDICT; }
    if (!m->last_stage || !m->logits || row < 0 || row >= m->ws_cap) { set_err(err, err_cap, "no logits row %d on this handle", row); return LLAMAHIP_ERR_PREDICT; }
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipDeviceSynchronize(), LLAMAHIP_ERR_PREDICT);
    const int r = row < (int) m->last_rows.size() ? m->last_rows[row] : row;      // (a set step orders its rows by slot id)
    HIP_TRY(hipMemcpy(logits_out, m->logits + (size_t) r * m->hp.n_vocab, (size_t) m->hp.n_vocab * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    return check_sync_timeout(m, err, err_cap);
}

// ------------------------------------------------------------------------------------------------
// In-process layer pipeline behind the reference's own surface (north_star: "the 65B model is layer-sharded across the
// 8 GPUs of one node ... called through a thin C-ABI shim from the existing Objective-C++ bridge").  The bridge makes ONE
// llama_model_load call from ONE process (.mm:790, LlamaRunnerBridge.mm:18-26) and one llama_eval per step (.mm:840, 865): a handle
// loaded with a device list holds one stage handle per device (layers split as evenly as possible, earlier stages take the remainder --
// pipeline.py layer_range) and llamahip_eval / llamahip_eval_chunks / llamahip_decode_greedy / llamahip_eval_topk walk them.  The only
// tensor that crosses a stage boundary is the residual stream inpL f32[n_embd][N] (.mm:563-564, 687-690): hipMemcpyPeerAsync on the
// producer's stream (an xGMI peer copy between two GPUs, a device copy when both stages sit on one), an event behind it, and the
// consumer's stream waits for that event -- no host round trip between stages, no collective.  Every stage runs the launches it would run
// as a stage of the multi-process RCCL pipeline (bench.py --gpus N), so results are bit for bit the whole-model handle's.
// ------------------------------------------------------------------------------------------------
static int pipe_devices(const llamahip_opts *opts, std::vector<int> &devices, char *err, size_t err_cap) {
    devices.clear();
    if (opts && opts->struct_size >= (int32_t) (offsetof(llamahip_opts, devices) + sizeof(opts->devices)) && opts->n_devices > 0) {
        if (opts->n_devices > LLAMAHIP_MAX_DEVICES) { set_err(err, err_cap, "llamahip_opts.n_devices %d: at most %d pipeline stages", opts->n_devices, LLAMAHIP_MAX_DEVICES); return LLAMAHIP_ERR_LOAD; }
        devices.assign(opts->devices, opts->devices + opts->n_devices);
    } else if (const char *env = getenv("LLAMAHIP_DEVICES")) {
        // the replacement bridge passes no options (integration/LlamaPredictOperation_llamahip.mm): "0,1,2,3,4,5,6,7", or a count "8" = devices 0 .. 7.
        // An explicit stage handle (layer range / device in opts) or a host-only handle is never turned into a pipeline.
        if (opts && opts->struct_size >= 24 && (opts->layer_begin != 0 || opts->layer_end >= 0 || opts->device >= 0 || (opts->flags & LLAMAHIP_FLAG_HOST_ONLY))) return 0;
        std::vector<int> v;
        const char *q = env;
        while (*q) {
            char *end = nullptr;
            const long x = strtol(q, &end, 10);
            if (end == q || x < 0 || x > 1023) { set_err(err, err_cap, "LLAMAHIP_DEVICES='%s': expected a device count or a comma-separated list of device ordinals", env); return LLAMAHIP_ERR_LOAD; }
            v.push_back((int) x);
            q = end;
            if (*q == ',') q++;
            else if (*q) { set_err(err, err_cap, "LLAMAHIP_DEVICES='%s': expected a device count or a comma-separated list of device ordinals", env); return LLAMAHIP_ERR_LOAD; }
        }
        if (v.size() == 1 && !strchr(env, ',') && v[0] >= 1) { const int n = v[0]; v.clear(); for (int i = 0; i < n; i++) v.push_back(i); }
        if ((int) v.size() > LLAMAHIP_MAX_DEVICES) { set_err(err, err_cap, "LLAMAHIP_DEVICES='%s': at most %d pipeline stages", env, LLAMAHIP_MAX_DEVICES); return LLAMAHIP_ERR_LOAD; }
        devices = v;
    }
    for (int dv : devices) if (dv < 0) { set_err(err, err_cap, "pipeline device ordinal %d is negative", dv); return LLAMAHIP_ERR_LOAD; }
    return 0;
}

static int pipe_load(const char *path, int32_t n_ctx, const llamahip_opts *opts, const std::vector<int> &devices, llamahip_model **out, char *err, size_t err_cap) {
    const double t0 = now_ms();
    if (!out || !path) { set_err(err, err_cap, "null argument"); return LLAMAHIP_ERR_LOAD; }
    *out = nullptr;
    llamahip_opts base = {};
    if (opts) memcpy(&base, opts, std::min((size_t) std::max(opts->struct_size, 0), sizeof(base)));
    if (!opts || opts->struct_size < 24) { base.n_parts = 0; base.flags = 0; }
    if (!opts || opts->struct_size < 28) base.n_seq = 0;
    if (opts && opts->struct_size >= 24 && (opts->layer_begin != 0 || opts->layer_end >= 0)) { set_err(err, err_cap, "a device list and a layer range exclude each other: the pipeline splits the layers itself"); return LLAMAHIP_ERR_LOAD; }
    if (base.flags & LLAMAHIP_FLAG_HOST_ONLY) { set_err(err, err_cap, "a device list and LLAMAHIP_FLAG_HOST_ONLY exclude each other"); return LLAMAHIP_ERR_LOAD; }
    // the front: file, vocab, hparams (the reader's validation and error messages, .mm:98-498), no device state
    llamahip_opts fo = base;
    fo.struct_size = 28; fo.device = -1; fo.layer_begin = 0; fo.layer_end = -1; fo.flags = base.flags | LLAMAHIP_FLAG_HOST_ONLY;
    llamahip_model *front = nullptr;
    int rc = model_load_impl(path, n_ctx, &fo, &front, err, err_cap);
    if (rc) return rc;
    std::unique_ptr<llamahip_model> guard(front);
    front->flags = base.flags;
    const int S = (int) devices.size(), L = front->hp.n_layer;
    if (S > L) { set_err(err, err_cap, "%d pipeline stages for a model of %d layers", S, L); return LLAMAHIP_ERR_LOAD; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { set_err(err, err_cap, "no HIP device available: libllamahip has no CPU fallback"); return LLAMAHIP_ERR_LOAD; }
    for (int dv : devices) if (dv >= ndev) { set_err(err, err_cap, "pipeline device %d: this process sees %d HIP device(s)", dv, ndev); return LLAMAHIP_ERR_LOAD; }
    // the stages load side by side (one thread each: the file reads and repack launches of different devices overlap)
    std::vector<llamahip_model *> stages(S, nullptr);
    std::vector<int> rcs(S, 0);
    std::vector<std::string> errs(S);
    std::vector<std::thread> th;
    for (int s = 0; s < S; s++) {
        th.emplace_back([&, s]() {
            char e[512] = "";
            llamahip_opts so = base;
            so.struct_size = 28; so.device = devices[s];
            const int bq = L / S, rem = L % S;
            so.layer_begin = s * bq + std::min(s, rem);
            so.layer_end = so.layer_begin + bq + (s < rem ? 1 : 0);
            try { rcs[s] = model_load_impl(path, n_ctx, &so, &stages[s], e, sizeof(e)); }
            catch (const std::exception &ex) { rcs[s] = LLAMAHIP_ERR_LOAD; snprintf(e, sizeof(e), "%s", ex.what()); }
            errs[s] = e;
        });
    }
    for (auto &t : th) t.join();
    front->stages = stages;                                  // (owned from here on: the front's destructor frees whatever loaded)
    front->stages.erase(std::remove(front->stages.begin(), front->stages.end(), nullptr), front->stages.end());
    for (int s = 0; s < S; s++) if (rcs[s]) { set_err(err, err_cap, "pipeline stage %d of %d (device %d): %s", s, S, devices[s], errs[s].c_str()); return LLAMAHIP_ERR_LOAD; }
    for (int s = 0; s < S; s++) {
        llamahip_model *st = stages[s];
        HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_LOAD);
        HIP_TRY(st->events.create(&st->pipe_ev, hipEventDisableTiming), LLAMAHIP_ERR_LOAD);
        HIP_TRY(st->own.alloc(&st->pipe_tok, 16, true), LLAMAHIP_ERR_LOAD);
        HIP_TRY(st->own.alloc(&st->pipe_hout, (size_t) front->hp.n_embd), LLAMAHIP_ERR_LOAD);
        // direct peer copies to the next stage's device and (last stage) back to the first; without peer access the copy is staged by the runtime
        // peer access lets the runtime copy device to device over xGMI (without it hipMemcpyPeerAsync stages through host memory)
        const int peers[2] = { stages[(s + 1) % S]->device, stages[0]->device };
        for (int pd : peers) {
            if (pd == st->device) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, st->device, pd) == hipSuccess && can) {
                const hipError_t e = hipDeviceEnablePeerAccess(pd, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_TRY(e, LLAMAHIP_ERR_LOAD);
                (void) hipGetLastError();
            }
        }
    }
    front->t_load_ms = now_ms() - t0;
    *out = guard.release();
    return LLAMAHIP_OK;
}

// consumer side of a hand-off: room for N rows on stage `st` (grown outside any enqueued work: the stage is idle between entry points)
static int pipe_ensure_in(llamahip_model *st, int N, char *err, size_t err_cap) {
    if (N <= st->pipe_in_cap) return 0;
    HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipStreamSynchronize(st->stream), LLAMAHIP_ERR_PREDICT);
    st->own.release(&st->pipe_in); st->pipe_in_cap = 0;
    const int cap = std::max(N, 16);
    HIP_TRY(st->own.alloc(&st->pipe_in, (size_t) cap * st->hp.n_embd), LLAMAHIP_ERR_PREDICT);
    st->pipe_in_cap = cap;
    return 0;
}
// producer side: `bytes` from `src` on stage a's device to `dst` on stage b's, ordered behind a's stream; b's stream waits for the copy.  (A copy,
// not a store by a's kernels into b's memory: hipMemcpyPeerAsync + an event is the hand-off whose visibility on the consumer's device the HIP
// runtime guarantees, and it is the path the one-GPU tests exercise; a round-6 build that let the stage kernels store into peer-mapped memory
// measured 679 against 675 tokens/s at two stages on one GPU and could not be validated across two.)
static int pipe_hand_off(llamahip_model *a, llamahip_model *b, void *dst, const void *src, size_t bytes, char *err, size_t err_cap) {
    HIP_TRY(hipSetDevice(a->device), LLAMAHIP_ERR_PREDICT);
    if (a->device == b->device) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, a->stream), LLAMAHIP_ERR_PREDICT);
    else HIP_TRY(hipMemcpyPeerAsync(dst, b->device, src, a->device, bytes, a->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipEventRecord(a->pipe_ev, a->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipSetDevice(b->device), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipStreamWaitEvent(b->stream, a->pipe_ev, 0), LLAMAHIP_ERR_PREDICT);
    return 0;
}
// Waiting for a stage is bounded (the watchdog the Python pipeline keeps around its collectives, here behind the C ABI): a stage whose GPU stops
// making progress -- a hung device, a lost xGMI link under a peer copy -- turns into LLAMAHIP_ERR_PREDICT after LLAMAHIP_PIPE_WATCHDOG_S seconds
// (default 600; the longest legitimate wait is a 2 048-token eval of a 65B stage, well under a second) instead of blocking the caller's thread for
// ever.  Spins on hipStreamQuery for the first milliseconds (token steps), then yields 100 us per look.
// (ev: wait for that event of the stage's stream instead of the whole stream -- llamahip_decode_sample_multi waits for one group at a time)
static int pipe_wait_stage(llamahip_model *st, int s, char *err, size_t err_cap, hipEvent_t ev = nullptr) {
    static const double limit_ms = (getenv("LLAMAHIP_PIPE_WATCHDOG_S") ? atof(getenv("LLAMAHIP_PIPE_WATCHDOG_S")) : 600.0) * 1e3;
    HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_PREDICT);
    const double t0 = now_ms();
    for (;;) {
        const hipError_t e = ev ? hipEventQuery(ev) : hipStreamQuery(st->stream);
        if (e == hipSuccess) return 0;
        (void) hipGetLastError();
        if (e != hipErrorNotReady) { set_err(err, err_cap, "HIP error: %s while waiting for pipeline stage %d (device %d)", hipGetErrorString(e), s, st->device); return LLAMAHIP_ERR_PREDICT; }
        const double waited = now_ms() - t0;
        if (waited > limit_ms) {
            set_err(err, err_cap, "pipeline stage %d (device %d, layers [%d, %d)) did not finish within %.3g s (LLAMAHIP_PIPE_WATCHDOG_S): results are invalid", s, st->device, st->l0, st->l1, limit_ms / 1e3);
            return LLAMAHIP_ERR_PREDICT;
        }
        if (waited > 5.0) std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}
// wait for every stage and collect their fault words (a hand-off that timed out inside a launch of ANY stage invalidates the result)
static int pipe_sync_stages(const std::vector<llamahip_model *> &stages, char *err, size_t err_cap) {
    int rc = 0;
    for (int s = (int) stages.size() - 1; s >= 0; s--) {
        llamahip_model *st = stages[s];
        int r = pipe_wait_stage(st, s, rc ? nullptr : err, rc ? 0 : err_cap);
        if (!r) r = check_sync_timeout(st, rc ? nullptr : err, rc ? 0 : err_cap);
        if (r && !rc) rc = r;
    }
    return rc;
}
static int pipe_sync(llamahip_model *m, char *err, size_t err_cap) { return pipe_sync_stages(m->stages, err, err_cap); }

static int pipe_eval(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t N, int32_t chunk, float *logits_out, char *err, size_t err_cap) {
    const int S = (int) m->stages.size();
    int rc = check_eval_args(m->stages[0], n_past, tokens, N, true, err, err_cap);
    if (rc) return rc;
    const double t0 = now_ms();
    const size_t d = m->hp.n_embd, V = m->hp.n_vocab;
    for (int s = 1; s < S; s++) if ((rc = pipe_ensure_in(m->stages[s], N, err, err_cap)) != 0) return rc;
    for (int s = 0; s < S; s++) {
        llamahip_model *st = m->stages[s];
        st->cur_seq = m->cur_seq;
        if ((rc = eval_stage_enqueue(st, n_threads, n_past, tokens, N, s ? st->pipe_in : nullptr, chunk, false, err, err_cap)) != 0) { (void) pipe_sync(m, nullptr, 0); return rc; }
        if (s + 1 < S && (rc = pipe_hand_off(st, m->stages[s + 1], m->stages[s + 1]->pipe_in, st->x, (size_t) N * d * 4, err, err_cap)) != 0) { (void) pipe_sync(m, nullptr, 0); return rc; }
    }
    // (the bounded wait first, the copy of the logits row behind it: a device-to-host copy into the caller's pageable buffer blocks inside the
    //  runtime until the stream has drained, without a bound)
    if ((rc = pipe_sync(m, err, err_cap)) != 0) return rc;
    llamahip_model *last = m->stages[S - 1];
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    if (logits_out) HIP_TRY(hipMemcpy(logits_out, last->logits + (size_t) (N - 1) * V, V * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    m->n_evals++;
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Scoring a text: llamahip_eval_logprobs / llamahip_perplexity.  The eval is llamahip_eval's (llamahip_eval_chunks' with chunk_tokens)
// except that the last stage's lm head runs over every row; k_row_logprob (logprob.hip) then reduces each row on that stage's stream, and
// only the N x 16 bytes of results cross to the host.
// ------------------------------------------------------------------------------------------------
struct ScoreIo { double *lp; int32_t *am, *rk, *tgt; };
static ScoreIo score_io(llamahip_model *m, int N) {
    char *b = (char *) m->d_score;
    return { (double *) b, (int32_t *) (b + 8L * N), (int32_t *) (b + 12L * N), (int32_t *) (b + 16L * N) };
}
// targets up, k_row_logprob over the N rows of m->logits, ordered behind the eval on m->stream
static int score_enqueue(llamahip_model *m, int N, const int32_t *targets, char *err, size_t err_cap) {
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    if (N > m->score_cap) {
        m->own.release(&m->d_score); m->score_cap = 0;
        HIP_TRY(m->own.alloc(&m->d_score, (size_t) N * 20), LLAMAHIP_ERR_PREDICT);
        m->score_cap = N;
    }
    const ScoreIo io = score_io(m, N);
    HIP_TRY(hipMemcpyAsync(io.tgt, targets, (size_t) N * 4, hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(launch_row_logprob(m->logits, N, m->hp.n_vocab, io.tgt, io.lp, io.am, io.rk, m->stream), LLAMAHIP_ERR_PREDICT);
    return 0;
}
// after the wait: the results of the N rows to the host in one copy
static int score_fetch(llamahip_model *m, int N, double *lp, int32_t *am, int32_t *rk, char *err, size_t err_cap) {
    std::vector<char> h((size_t) N * 16);
    HIP_TRY(hipMemcpy(h.data(), m->d_score, h.size(), hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    if (lp) memcpy(lp, h.data(), (size_t) N * 8);
    if (am) memcpy(am, h.data() + (size_t) N * 8, (size_t) N * 4);
    if (rk) memcpy(rk, h.data() + (size_t) N * 12, (size_t) N * 4);
    return 0;
}

// llamahip_eval_top_logprobs: k_row_topn over the N rows of m->logits in k_row_logprob's place, ordered behind the eval on m->stream
static int topn_enqueue(llamahip_model *m, int N, int n_top, char *err, size_t err_cap) {
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    const size_t cells = (size_t) N * n_top, bytes = cells * 12;
    if (bytes > m->topn_cap) {
        m->own.release(&m->d_topn); m->topn_cap = 0;
        HIP_TRY(m->own.alloc(&m->d_topn, bytes), LLAMAHIP_ERR_PREDICT);
        m->topn_cap = bytes;
    }
    HIP_TRY(launch_row_topn(m->logits, N, m->hp.n_vocab, n_top, (int32_t *) (m->d_topn + cells * 8), (double *) m->d_topn, m->stream), LLAMAHIP_ERR_PREDICT);
    return 0;
}
static int topn_fetch(llamahip_model *m, int N, int n_top, double *lp, int32_t *ids, char *err, size_t err_cap) {
    const size_t cells = (size_t) N * n_top;
    HIP_TRY(hipMemcpy(lp, m->d_topn, cells * 8, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipMemcpy(ids, m->d_topn + cells * 8, cells * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    return 0;
}

// one eval of N rows at n_past (chunk: the key split of llamahip_eval_chunks, 0 = none) + the scores of its rows, on a plain or a pipeline handle
// (n_top > 0: the rows' top-n places instead -- lp [N][n_top], am = the ids [N][n_top], targets and rk unused)
static int eval_score(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t N, int chunk, const int32_t *targets,
                      double *lp, int32_t *am, int32_t *rk, float *logits_last, char *err, size_t err_cap, int n_top = 0) {
    const double t0 = now_ms();
    llamahip_model *last = m;
    int rc;
    if (m->stages.empty()) {
        if ((rc = eval_stage_enqueue(m, n_threads, n_past, tokens, N, nullptr, chunk, true, err, err_cap)) != 0) return rc;
        if ((rc = n_top ? topn_enqueue(m, N, n_top, err, err_cap) : score_enqueue(m, N, targets, err, err_cap)) != 0) return rc;
        HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
        if ((rc = check_sync_timeout(m, err, err_cap)) != 0) return rc;
    } else {
        // pipe_eval's walk, the last stage with every row of logits and k_row_logprob behind it; the bounded wait before any copy to the host
        const int S = (int) m->stages.size();
        const size_t d = m->hp.n_embd;
        for (int s = 1; s < S; s++) if ((rc = pipe_ensure_in(m->stages[s], N, err, err_cap)) != 0) return rc;
        for (int s = 0; s < S; s++) {
            llamahip_model *st = m->stages[s];
            st->cur_seq = m->cur_seq;
            if ((rc = eval_stage_enqueue(st, n_threads, n_past, tokens, N, s ? st->pipe_in : nullptr, chunk, s == S - 1, err, err_cap)) != 0) { (void) pipe_sync(m, nullptr, 0); return rc; }
            if (s + 1 < S && (rc = pipe_hand_off(st, m->stages[s + 1], m->stages[s + 1]->pipe_in, st->x, (size_t) N * d * 4, err, err_cap)) != 0) { (void) pipe_sync(m, nullptr, 0); return rc; }
        }
        last = m->stages[S - 1];
        if ((rc = n_top ? topn_enqueue(last, N, n_top, err, err_cap) : score_enqueue(last, N, targets, err, err_cap)) != 0) { (void) pipe_sync(m, nullptr, 0); return rc; }
        if ((rc = pipe_sync(m, err, err_cap)) != 0) return rc;
        HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    }
    if ((rc = n_top ? topn_fetch(last, N, n_top, lp, am, err, err_cap) : score_fetch(last, N, lp, am, rk, err, err_cap)) != 0) return rc;
    const size_t V = m->hp.n_vocab;
    if (logits_last) HIP_TRY(hipMemcpy(logits_last, last->logits + (size_t) (N - 1) * V, V * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    m->n_evals++;
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}

// llamahip_eval_chunks' split: Q4_0 files in one pass, f16 / f32 files too from DENSE_ONE_PASS_MIN_ROWS rows, else (and Q4_1 files) chunk by
// chunk, each chunk's rows scored
static int logprobs_impl(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t N, int32_t chunk_tokens,
                         const int32_t *targets, double *lp, int32_t *am, int32_t *rk, float *logits_last, char *err, size_t err_cap, int n_top = 0) {
    const bool chunked = chunk_tokens > 0 && N > chunk_tokens;
    if (!chunked || chunks_in_one_pass(m, N)) return eval_score(m, n_threads, n_past, tokens, N, chunked ? chunk_tokens : 0, targets, lp, am, rk, logits_last, err, err_cap, n_top);
    const size_t w = n_top ? n_top : 1;      // (cells per row of lp / am)
    for (int32_t c0 = 0; c0 < N; c0 += chunk_tokens) {
        const int32_t n = std::min(chunk_tokens, N - c0);
        const int rc = eval_score(m, n_threads, n_past + c0, tokens + c0, n, 0, targets ? targets + c0 : nullptr, lp ? lp + c0 * w : nullptr, am ? am + c0 * w : nullptr,
                                  rk ? rk + c0 : nullptr, c0 + n == N ? logits_last : nullptr, err, err_cap, n_top);
        if (rc) return rc;
    }
    return LLAMAHIP_OK;
}

// the arguments first (a HOST_ONLY handle knows n_vocab / n_ctx: the checks are the same without a device), then the handle
static int check_score_args(llamahip_model *m, int32_t n_past, const int32_t *tokens, int32_t N, int32_t chunk_tokens, const int32_t *targets,
                            const char *fn, char *err, size_t err_cap) {
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    const int V = m->hp.n_vocab, C = m->hp.n_ctx;
    if (N < 1) { set_err(err, err_cap, "%s: n_tokens must be >= 1 (got %d)", fn, N); return LLAMAHIP_ERR_PREDICT; }
    if (n_past < 0 || n_past + N > C) { set_err(err, err_cap, "%s: context overflow: n_past (%d) + n_tokens (%d) > n_ctx (%d)", fn, n_past, N, C); return LLAMAHIP_ERR_PREDICT; }
    if (chunk_tokens < 0) { set_err(err, err_cap, "%s: chunk_tokens must be >= 0 (0 = one eval; got %d)", fn, chunk_tokens); return LLAMAHIP_ERR_PREDICT; }
    if (!tokens) { set_err(err, err_cap, "%s: null tokens", fn); return LLAMAHIP_ERR_PREDICT; }
    for (int i = 0; i < N; i++)
        if (tokens[i] < 0 || tokens[i] >= V) { set_err(err, err_cap, "%s: token id %d at %d out of range [0, %d)", fn, tokens[i], i, V); return LLAMAHIP_ERR_PREDICT; }
    if (targets)
        for (int i = 0; i < N; i++)
            if (targets[i] < -1 || targets[i] >= V) { set_err(err, err_cap, "%s: target %d of row %d out of range [-1, %d)", fn, targets[i], i, V); return LLAMAHIP_ERR_PREDICT; }
    if (m->stages.empty() && (!m->first_stage || !m->last_stage)) { set_err(err, err_cap, "%s on a pipeline-stage handle: load the whole model (or a device list)", fn); return LLAMAHIP_ERR_PREDICT; }
    return check_eval_args(m->stages.empty() ? m : m->stages[0], n_past, tokens, N, true, err, err_cap);      // (HOST_ONLY: refused here)
}

int llamahip_eval_logprobs(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t n_tokens,
                           int32_t chunk_tokens, const int32_t *targets, double *logprob_out, int32_t *argmax_out,
                           int32_t *rank_out, float *logits_last, char *err, size_t err_cap) {
    int rc = check_score_args(m, n_past, tokens, n_tokens, chunk_tokens, targets, "llamahip_eval_logprobs", err, err_cap);
    if (rc) return rc;
    std::vector<int32_t> tgt(n_tokens, -1);
    if (targets) std::copy(targets, targets + n_tokens, tgt.begin());
    else for (int i = 0; i + 1 < n_tokens; i++) tgt[i] = tokens[i + 1];
    return logprobs_impl(m, n_threads, n_past, tokens, n_tokens, chunk_tokens, tgt.data(), logprob_out, argmax_out, rank_out, logits_last, err, err_cap);
}

int llamahip_eval_top_logprobs(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t n_tokens, int32_t chunk_tokens,
                               int32_t n_top, int32_t *ids_out, double *logprob_out, float *logits_last, char *err, size_t err_cap) {
    static const char *fn = "llamahip_eval_top_logprobs";
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    if (n_top < 1 || n_top > TOPN_MAX) { set_err(err, err_cap, "%s: n_top %d outside 1 .. %d", fn, n_top, TOPN_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (n_top > m->hp.n_vocab) { set_err(err, err_cap, "%s: n_top %d > n_vocab %d", fn, n_top, m->hp.n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (!ids_out || !logprob_out) { set_err(err, err_cap, "%s: %s is NULL", fn, !ids_out ? "ids_out" : "logprob_out"); return LLAMAHIP_ERR_PREDICT; }
    const int rc = check_score_args(m, n_past, tokens, n_tokens, chunk_tokens, nullptr, fn, err, err_cap);
    if (rc) return rc;
    return logprobs_impl(m, n_threads, n_past, tokens, n_tokens, chunk_tokens, nullptr, logprob_out, ids_out, nullptr, logits_last, err, err_cap, n_top);
}

int llamahip_perplexity(llamahip_model *m, int32_t n_threads, const int32_t *tokens, int32_t n_tokens, int32_t window,
                        int32_t score_from, int32_t chunk_tokens, double *nll_sum, int64_t *n_scored, double *running_ppl,
                        char *err, size_t err_cap) {
    if (!m) { set_err(err, err_cap, "llamahip_perplexity: null model"); return LLAMAHIP_ERR_PREDICT; }
    const int C = m->hp.n_ctx;
    const int W = window == 0 ? C : window;
    if (window < 0 || W < 2) { set_err(err, err_cap, "llamahip_perplexity: window must be >= 2 tokens (0 = n_ctx; got %d)", window); return LLAMAHIP_ERR_PREDICT; }
    if (W - 1 > C) { set_err(err, err_cap, "llamahip_perplexity: window %d: its %d evaluated tokens exceed n_ctx (%d)", W, W - 1, C); return LLAMAHIP_ERR_PREDICT; }
    if (!tokens || n_tokens < W) { set_err(err, err_cap, "llamahip_perplexity: a stream of %d tokens is shorter than one window of %d", n_tokens, W); return LLAMAHIP_ERR_PREDICT; }
    const int sf = score_from == -1 ? W / 2 : score_from;
    if (score_from < -1 || sf > W - 2) { set_err(err, err_cap, "llamahip_perplexity: score_from %d: rows 0 .. %d of a window of %d predict a token (-1 = window / 2)", score_from, W - 2, W); return LLAMAHIP_ERR_PREDICT; }
    const int n_win = n_tokens / W;
    for (int i = 0; i < n_win * W; i++)
        if (tokens[i] < 0 || tokens[i] >= m->hp.n_vocab) { set_err(err, err_cap, "llamahip_perplexity: token id %d at %d out of range [0, %d)", tokens[i], i, m->hp.n_vocab); return LLAMAHIP_ERR_PREDICT; }
    int rc = check_score_args(m, 0, tokens, W - 1, chunk_tokens, nullptr, "llamahip_perplexity", err, err_cap);
    if (rc) return rc;
    std::vector<int32_t> tgt(W - 1);
    std::vector<double> lp(W - 1);
    double nll = 0.0;
    int64_t cnt = 0;
    for (int k = 0; k < n_win; k++) {
        const int32_t *win = tokens + (size_t) k * W;
        for (int j = 0; j < W - 1; j++) tgt[j] = j >= sf ? win[j + 1] : -1;
        if ((rc = logprobs_impl(m, n_threads, 0, win, W - 1, chunk_tokens, tgt.data(), lp.data(), nullptr, nullptr, nullptr, err, err_cap)) != 0) return rc;
        for (int j = sf; j < W - 1; j++) { nll -= lp[j]; cnt++; }
        if (running_ppl) running_ppl[k] = exp(nll / (double) cnt);
    }
    if (nll_sum) *nll_sum = nll;
    if (n_scored) *n_scored = cnt;
    return LLAMAHIP_OK;
}

// The greedy loop on the pipeline: every stage's single-token step is its captured graph (llamahip_stage_step), the row travels stage to
// stage and the picked token travels from the last stage back to the first as stream-ordered copies (pipe_hand_off); the host enqueues all
// n_steps without waiting and reads the trace at the end.
// (Round 6 also wired the device-side mailboxes of include/llamahip.h between the stages of such a handle -- no event, the consumer's first
//  kernel polls.  With every stage on ONE GPU it passed the two- and three-stage oracle tests on narrow models and then timed out
//  intermittently on the full 7B (a polling stage holds CU slots and queue positions its producer needs; profiles/r06_g_inprocess_mailbox_diag.txt);
//  it cannot be validated without a second GPU, so it was removed again.  The multi-process pipeline keeps its mailbox schedule behind a
//  one-token handshake with a common fall-back to RCCL: bench.py --gpus N.)
static int pipe_decode_greedy(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token, int32_t n_steps, int32_t *out_tokens, float *logits_last,
                              char *err, size_t err_cap) {
    const int S = (int) m->stages.size();
    llamahip_model *first = m->stages[0], *last = m->stages[S - 1];
    int rc = check_eval_args(first, n_past, &first_token, 1, true, err, err_cap);
    if (rc) return rc;
    if (n_steps < 1 || n_past + n_steps > m->hp.n_ctx) { set_err(err, err_cap, "context overflow: n_past (%d) + n_steps (%d) > n_ctx (%d)", n_past, n_steps, m->hp.n_ctx); return LLAMAHIP_ERR_PREDICT; }
    if (!out_tokens) { set_err(err, err_cap, "null out_tokens"); return LLAMAHIP_ERR_PREDICT; }
    if (first->dense || (first->flags & LLAMAHIP_FLAG_UNFUSED)) {
        // un-fused stages (f16 / f32 / Q4_1 files, LLAMAHIP_FLAG_UNFUSED) have no captured stage step: one pipeline eval per token, the pick by
        // k_argmax itself on the last stage's logits row -- the plain handle's rule (lowest index on ties, NaN never picked) -- read back for the
        // next step's token
        int32_t tok = first_token;
        for (int i = 0; i < n_steps; i++) {
            if ((rc = pipe_eval(m, n_threads, n_past + i, &tok, 1, 0, i + 1 == n_steps ? logits_last : nullptr, err, err_cap)) != 0) return rc;
            HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(launch_argmax(last->logits, m->hp.n_vocab, last->pipe_tok, 0, nullptr, nullptr, last->stream), LLAMAHIP_ERR_PREDICT);
            if ((rc = pipe_wait_stage(last, S - 1, err, err_cap)) != 0) return rc;
            HIP_TRY(hipMemcpy(&tok, last->pipe_tok, 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
            out_tokens[i] = tok;
        }
        return LLAMAHIP_OK;                                                // (pipe_eval counted the evals and their time)
    }
    const double t0 = now_ms();
    const size_t d = m->hp.n_embd;
    const int seq = m->cur_seq;
    for (int s = 1; s < S; s++) if ((rc = pipe_ensure_in(m->stages[s], 1, err, err_cap)) != 0) return rc;
    HIP_TRY(hipSetDevice(first->device), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipMemcpy(first->pipe_tok, &first_token, 4, hipMemcpyHostToDevice), LLAMAHIP_ERR_PREDICT);
    m->pipe_hand_off = 1;
    for (int s = 0; s < S; s++) {
        llamahip_model *st = m->stages[s];
        if ((rc = llamahip_stage_bind(st, seq, n_past, s == 0 ? first->pipe_tok : nullptr, s ? st->pipe_in : nullptr, s + 1 < S ? st->pipe_hout : nullptr,
                                      s + 1 == S ? last->pipe_tok : nullptr, err, err_cap)) != 0) return rc;
    }
    for (int i = 0; i < n_steps && rc == 0; i++) {
        for (int s = 0; s < S && rc == 0; s++) {
            llamahip_model *st = m->stages[s];
            if ((rc = llamahip_stage_step(st, seq, n_threads, st->stream, err, err_cap)) != 0) break;
            if (s + 1 < S) rc = pipe_hand_off(st, m->stages[s + 1], m->stages[s + 1]->pipe_in, st->pipe_hout, d * 4, err, err_cap);
            else if (i + 1 < n_steps) rc = pipe_hand_off(last, first, first->pipe_tok, last->pipe_tok, 4, err, err_cap);
        }
    }
    if (rc) { (void) pipe_sync(m, nullptr, 0); return rc; }
    if ((rc = pipe_sync(m, err, err_cap)) != 0) return rc;
    int32_t pos = 0;
    const int n = llamahip_stage_trace(last, seq, &pos, out_tokens, n_steps, err, err_cap);
    if (n < 0) return n;
    if (n != n_steps || pos != n_past + n_steps) { set_err(err, err_cap, "pipeline decode: %d of %d steps recorded, position %d", n, n_steps, pos); return LLAMAHIP_ERR_PREDICT; }
    if (logits_last && (rc = llamahip_stage_logits(last, 0, logits_last, err, err_cap)) != 0) return rc;
    m->n_evals += n_steps;
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// The drafted and the multi-sequence decoders, from here to llamahip_set_seq, are one family built on a few shared pieces, each described
// once where it is defined:
//   stages_of / first_of / last_of    a handle as its list of stages (a plain handle: the one stage)
//   each_slot, drain_stages           the per-slot fall-back (a single-sequence function on each slot in turn); the wait that ends every
//                                     stretch of enqueued stage work, on the error paths too
//   SampleParams, sample_draw,        the sampler's parameters, one draw (candidates or logits, accept, exact flag) and the walk over
//   sample_walk                       the rows of a verify step
//   LookupRun                         a lookup run over n sequences: histories, drafting, segments, accounting
//   group_cut, multi_begin,           the groups of a multi-sequence step, the slots' binding, and one group stepped through every
//   step_group                        stage with its hand-offs
// ------------------------------------------------------------------------------------------------
static std::vector<llamahip_model *> stages_of(llamahip_model *m) { return m->stages.empty() ? std::vector<llamahip_model *>{ m } : m->stages; }
static llamahip_model *first_of(llamahip_model *m) { return m->stages.empty() ? m : m->stages[0]; }
static llamahip_model *last_of(llamahip_model *m) { return m->stages.empty() ? m : m->stages.back(); }

// the end of everything enqueued on the stages: every stage waited for (bounded: pipe_wait_stage), their fault words collected.  rc: what the
// enqueuing returned -- an error reported there stays the call's error, and the stages are drained all the same
static int drain_stages(const std::vector<llamahip_model *> &stages, int rc, char *err, size_t err_cap) {
    const int rc_sync = pipe_sync_stages(stages, rc ? nullptr : err, rc ? 0 : err_cap);
    return rc ? rc : rc_sync;
}

// fn(i) with slot slots[i] current (slots == nullptr: slot i), for i = 0 .. n - 1 until one fails; the handle's current slot is restored
static int each_slot(llamahip_model *m, int32_t n, const int32_t *slots, char *err, size_t err_cap, const std::function<int(int)> &fn) {
    const int save_seq = m->cur_seq;
    int rc = 0;
    for (int i = 0; i < n && rc == 0; i++)
        if ((rc = llamahip_set_seq(m, slots ? slots[i] : i, err, err_cap)) == 0) rc = fn(i);
    (void) llamahip_set_seq(m, save_seq, nullptr, 0);
    return rc;
}

// ------------------------------------------------------------------------------------------------
// The prompts of several sequences in one weight pass: llamahip_eval_multi (llamahip.h).  R rows cut into segments, one per KV
// slot, each a multi-row eval of its own.  The mat-muls and the activation preparations run over all R rows as a single eval of R rows runs them
// (launch_prep / launch_gemm, the kernel chosen by R: every exact kernel gives the same bits); the RoPE / KV append and the attention read each
// row's {position, key split, cache offset} from a device-resident table (rows_attn.hip), built and validated here, uploaded once per pass and
// stage on the stage's stream ahead of the first launch that reads it.  A segment of more than ATTN_SHORT_MAX rows keeps launch_attn on its own
// rows and its slot's cache -- the launches its own eval takes -- and writes fp32 merged rows; the table launch then writes merged rows too and
// one PREP_PLAIN over all R rows makes wo's operand.
// ------------------------------------------------------------------------------------------------
constexpr int EVAL_MULTI_LOOP_SEG_ROWS = 512, EVAL_MULTI_LOOP_ROWS = 1024;      // the measured rule of llamahip_eval_multi: see there
struct RowsPass {
    int n_seqs = 0, R = 0, chunk = 0, short_max = ATTN_SHORT_MAX;      // short_max: segments up to this many rows run in the table launch
    const int32_t *slots = nullptr, *n_past = nullptr, *n_tokens = nullptr;
    std::vector<int32_t> pos, keys, seg;          // llamahip_eval_multi_rows
    int n_short_segs = 0, n_long_segs = 0, n_short_rows = 0, max_keys = 1;      // max_keys: the largest position + 1 among the short segments' rows
    // a scheduler step with drafted tokens (empty otherwise: llamahip_eval_multi's pass as it is).  seg_single[i]: every row of segment i is keyed
    // as its own single-token eval, keys = position + 1, whatever `chunk` -- the per-segment override of the key rule.  logit_rows: the rows the
    // lm head runs over, in logits-row order (empty: every segment's last row), at most ROWS_LOGITS_MAX
    std::vector<char> seg_single;
    std::vector<int32_t> logit_rows;
    // scoring (llamahip_eval_logprobs_multi): logit_rows = the scored rows, up to logits_cap = R of them and possibly none (then no lm head at all);
    // the lm head over them is a scoring eval's (Pass::score_rows), k_row_logprob follows it on the last stage
    bool score = false;
    int logits_cap = VERIFY_ROWS_MAX;             // (= ROWS_LOGITS_MAX: a scheduler's step)
    int n_logits() const { return logit_rows.empty() && !score ? n_seqs : (int) logit_rows.size(); }
    // an embedding pass (llamahip_text_embedding_multi): in place of the lm head the fp32 final norm, the pooling per segment and the optional L2
    // normalisation into the last stage's d_embed (embed_tail_rows); the logits and their row map stay as they are
    bool embed = false;
    int embed_pool = 0, embed_normalize = 0;
};
constexpr int ROWS_LOGITS_MAX = VERIFY_ROWS_MAX;
// the lm head's row list: a row per KV slot or ROWS_LOGITS_MAX rows, and as many as the table has rows (a scoring pass may score every row)
static size_t rows_idx_entries(const llamahip_model *m, int cap) { return (size_t) std::max(std::max(m->n_seq, ROWS_LOGITS_MAX), cap); }
struct RowsDev { RowTab *tab; int32_t *short_idx, *last_idx; };
static RowsDev rows_dev(llamahip_model *m) {
    char *b = m->d_rows;
    return { (RowTab *) b, (int32_t *) (b + (size_t) m->rows_cap * sizeof(RowTab)), (int32_t *) (b + (size_t) m->rows_cap * (sizeof(RowTab) + 4)) };
}
// the stage's table for this pass: built from the pass's rows with the stage's own cache stride, every entry checked against n_ctx and n_seq
static int rows_upload(llamahip_model *m, const RowsPass &rp, char *err, size_t err_cap) {
    const size_t C = m->hp.n_ctx, d = m->hp.n_embd;
    if (rp.R > m->rows_cap) {
        HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
        m->own.release(&m->d_rows); m->rows_cap = 0;
        const int cap = std::max(rp.R, 64);
        HIP_TRY(m->own.alloc(&m->d_rows, (size_t) cap * (sizeof(RowTab) + 4) + rows_idx_entries(m, cap) * 4), LLAMAHIP_ERR_PREDICT);
        m->rows_cap = cap;
    }
    const size_t cap = (size_t) m->rows_cap, n_idx = rows_idx_entries(m, m->rows_cap), bytes = cap * (sizeof(RowTab) + 4) + n_idx * 4;
    const int logits_max = std::max(m->n_seq, rp.logits_cap);
    if (rp.logit_rows.size() > (size_t) rp.logits_cap || (size_t) rp.n_logits() > n_idx || (rp.logit_rows.empty() && !rp.score && rp.n_seqs > logits_max)) {
        set_err(err, err_cap, "llamahip_eval_multi: %d logits rows in one pass (at most %d)", rp.n_logits(), logits_max);
        return LLAMAHIP_ERR_PREDICT;
    }
    m->h_rows.assign(bytes, 0);
    RowTab *tab = (RowTab *) m->h_rows.data();
    int32_t *short_idx = (int32_t *) (m->h_rows.data() + cap * sizeof(RowTab)), *last_idx = short_idx + cap;
    const long slot_stride = (long) (m->l1 - m->l0) * (long) C * (long) d;      // [seq][layer][n_ctx][d]
    int ns = 0;
    for (int r = 0; r < rp.R; r++) {
        const int i = rp.seg[r], slot = rp.slots[i];
        if (slot < 0 || slot >= m->n_seq || rp.pos[r] < 0 || rp.keys[r] <= rp.pos[r] || rp.keys[r] > (int) C || rp.keys[r] > rp.n_past[i] + rp.n_tokens[i]) {
            set_err(err, err_cap, "llamahip_eval_multi: row %d of the table (slot %d, position %d, %d keys) is outside the cache (n_seq %d, n_ctx %d)", r, slot, rp.pos[r], rp.keys[r], m->n_seq, (int) C);
            return LLAMAHIP_ERR_PREDICT;
        }
        tab[r] = { rp.pos[r], rp.keys[r], (long) slot * slot_stride };
        if (rp.n_tokens[i] <= rp.short_max) short_idx[ns++] = r;
        if (rp.logit_rows.empty() && !rp.score && (r + 1 == rp.R || rp.seg[r + 1] != i)) last_idx[i] = r;
    }
    for (size_t k = 0; k < rp.logit_rows.size(); k++) {
        if (rp.logit_rows[k] < 0 || rp.logit_rows[k] >= rp.R) { set_err(err, err_cap, "llamahip_eval_multi: logits row %d names row %d of %d", (int) k, rp.logit_rows[k], rp.R); return LLAMAHIP_ERR_PREDICT; }
        last_idx[k] = rp.logit_rows[k];
    }
    HIP_TRY(hipMemcpyAsync(m->d_rows, m->h_rows.data(), bytes, hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
    return 0;
}

// ---- a text's embedding: the device buffer of the last stage and the tail of a pass (pool.hip; llamahip_text_embedding[_multi] below)
struct EmbedDev { float *out; int32_t *seg; float *y; };
static EmbedDev embed_dev(llamahip_model *m) {
    const size_t d = m->hp.n_embd, out_b = (size_t) m->embed_segs_cap * d * 4, seg_b = ((size_t) m->embed_segs_cap + 1 + 3) / 4 * 16;
    return { (float *) m->d_embed, (int32_t *) (m->d_embed + out_b), (float *) (m->d_embed + out_b + seg_b) };
}
// room for n_segs pooled rows and n_rows norm rows (grown outside any enqueued work: the stage is idle between entry points)
static int embed_ensure(llamahip_model *m, int n_segs, int n_rows, char *err, size_t err_cap) {
    if (m->d_embed && n_segs <= m->embed_segs_cap && n_rows <= m->embed_rows_cap) return 0;
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
    m->own.release(&m->d_embed);
    const int segs = std::max(std::max(n_segs, m->embed_segs_cap), LLAMAHIP_POOL_MAX_SEGS), rows = std::max(std::max(n_rows, m->embed_rows_cap), 64);
    m->embed_segs_cap = m->embed_rows_cap = 0;
    const size_t d = m->hp.n_embd;
    HIP_TRY(m->own.alloc(&m->d_embed, (size_t) segs * d * 4 + ((size_t) segs + 1 + 3) / 4 * 16 + (size_t) rows * d * 4), LLAMAHIP_ERR_PREDICT);
    m->embed_segs_cap = segs; m->embed_rows_cap = rows;
    return 0;
}
// seg_begin (n_segs + 1 entries over the rows of y) up, the pooling and the optional L2 normalisation behind whatever wrote y on m->stream
static int embed_pool_enqueue(llamahip_model *m, const std::vector<int32_t> &seg_begin, int pool, int normalize, char *err, size_t err_cap) {
    const EmbedDev ed = embed_dev(m);
    const int n_segs = (int) seg_begin.size() - 1;
    m->h_embed_seg = seg_begin;          // (alive until the stream has drained)
    HIP_TRY(hipMemcpyAsync(ed.seg, m->h_embed_seg.data(), m->h_embed_seg.size() * 4, hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(launch_pool_rows(ed.y, ed.seg, n_segs, m->hp.n_embd, pool, normalize, ed.out, m->stream), LLAMAHIP_ERR_PREDICT);
    return 0;
}
struct RowsPass;
static int embed_tail_rows(llamahip_model *m, const RowsPass &rp, const int32_t *last_idx, char *err, size_t err_cap);

// the pass on one handle's layers, enqueued on its stream (the multi-row branch of forward, with the table kernels where the rows' segments matter)
static int forward_rows(llamahip_model *m, int n_threads, const RowsPass &rp, const float *hidden_in, char *err, size_t err_cap) {
    const HParams &hp = m->hp;
    const int d = hp.n_embd, F = hp.n_ff, H = hp.n_head, dh = d / H, C = hp.n_ctx, V = hp.n_vocab, R = rp.R;
    const int nth = clamp_threads(n_threads);
    hipStream_t st = m->stream;
    int rc = rows_upload(m, rp, err, err_cap);
    if (rc) return rc;
    const RowsDev rd = rows_dev(m);
    if (m->first_stage) HIP_TRY(launch_embed(m->d_tokens, m->tok_emb, m->x, d, R, st), LLAMAHIP_ERR_PREDICT);
    else HIP_TRY(hipMemcpyAsync(m->x, hidden_in, (size_t) R * d * 4, hipMemcpyDeviceToDevice, st), LLAMAHIP_ERR_PREDICT);
    for (int il = m->l0; il < m->l1; il++) {
        const Layer &L = m->layers[il - m->l0];
        float *K0 = m->Kc + (size_t) (il - m->l0) * C * d, *V0 = m->Vc + (size_t) (il - m->l0) * C * d;      // slot 0's cache of this layer: the table's offsets start here
        HIP_TRY(launch_prep(PREP_NORM, m->x, L.attention_norm, d, 0, d, R, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(launch_gemm(L.qkv, EPI_STORE, m->qa_A, m->qa_d, R, m->qkv, 3L * d, nullptr, 0, st, m->qb_ws, false), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(launch_rope_kv_rows(m->qkv, 3L * d, d, dh, m->sincos, m->qr, K0, V0, rd.tab, R, st), LLAMAHIP_ERR_PREDICT);
        if (rp.n_long_segs == 0) {
            // every segment short: one launch pair for all rows, quantizing the merged rows straight into wo's operand
            HIP_TRY(launch_attn_rows(m->qr, K0, V0, m->attn_ws.S, m->attn_ws.NB, nullptr, 0, m->qa_A, m->qa_d, rd.tab, nullptr, R, rp.max_keys, d, H, C, nth, m->T_exp, st), LLAMAHIP_ERR_PREDICT);
        } else {
            if (rp.n_short_rows > 0)
                HIP_TRY(launch_attn_rows(m->qr, K0, V0, m->attn_ws.S, m->attn_ws.NB, m->merged, d, m->qa_A, m->qa_d, rd.tab, rd.short_idx, rp.n_short_rows, rp.max_keys, d, H, C, nth, m->T_exp, st), LLAMAHIP_ERR_PREDICT);
            for (int i = 0, r0 = 0; i < rp.n_seqs; r0 += rp.n_tokens[i], i++) {
                if (rp.n_tokens[i] <= rp.short_max) continue;
                const size_t off = (size_t) rp.slots[i] * (m->l1 - m->l0) * C * d;
                HIP_TRY(launch_attn(m->qr + (size_t) r0 * d, K0 + off, V0 + off, m->merged + (size_t) r0 * d, nullptr, nullptr, rp.n_past[i], rp.n_tokens[i], d, H, nth, m->T_exp, &m->attn_ws, st, rp.chunk), LLAMAHIP_ERR_PREDICT);
            }
            HIP_TRY(launch_prep(PREP_PLAIN, m->merged, nullptr, d, 0, d, R, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);
        }
        HIP_TRY(launch_gemm(L.wo, EPI_RESID, m->qa_A, m->qa_d, R, m->x1, d, m->x, d, st, m->qb_ws, false), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(launch_prep(PREP_NORM, m->x1, L.ffn_norm, d, 0, d, R, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(launch_gemm(L.w13, EPI_STORE, m->qa_A, m->qa_d, R, m->gu, 2L * F, nullptr, 0, st, m->qb_ws, false), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(launch_prep(PREP_SILU_MUL, m->gu, m->gu + F, 2L * F, 2L * F, F, R, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(launch_gemm(L.w2, EPI_RESID, m->qa_A, m->qa_d, R, m->x, d, m->x1, d, st, m->qb_ws, false), LLAMAHIP_ERR_PREDICT);
    }
    if (m->last_stage && rp.embed) return embed_tail_rows(m, rp, rd.last_idx, err, err_cap);
    if (m->last_stage) {
        // the segments' last rows (a drafted scheduler step: its list of rows) side by side (x1 is free here), the final norm and the lm head over
        // those nl rows: logits rows 0 .. nl - 1
        // (a scoring pass: the scored rows, none at all: no lm head; and the lm head a scoring eval of nl rows takes -- `output`'s prompt copies
        //  and the operand workspace at row counts that use them, as forward_eval's under Pass::score_rows)
        const int nl = rp.n_logits();
        if (nl > 0) {
            HIP_TRY(launch_gather_rows(m->x, rd.last_idx, nl, d, m->x1, st), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(launch_prep(PREP_NORM, m->x1, m->norm_w, d, 0, d, nl, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, st), LLAMAHIP_ERR_PREDICT);
            QMat out = m->output;
            if (!rp.score) { out.rows = nullptr; out.mt = nullptr; out.mt4 = nullptr; }          // (the decode tiles, as llamahip_eval's lm head)
            HIP_TRY(launch_gemm(out, EPI_STORE, m->qa_A, m->qa_d, nl, m->logits, V, nullptr, 0, st, rp.score ? m->qb_ws : nullptr), LLAMAHIP_ERR_PREDICT);
        }
    }
    m->last_rows.clear();          // (m->logits rewritten)
    return 0;
}

// the tail of an embedding pass over the R rows of m->x.  LAST: the segments' last rows side by side (x1 is free here, as for the lm head), the
// norm over those n_seqs rows alone, each a segment of one row; MEAN: the norm over all R rows, the segments as the pass has them
static int embed_tail_rows(llamahip_model *m, const RowsPass &rp, const int32_t *last_idx, char *err, size_t err_cap) {
    const int d = m->hp.n_embd, n = rp.n_seqs;
    const EmbedDev ed = embed_dev(m);
    std::vector<int32_t> seg((size_t) n + 1, 0);
    if (rp.embed_pool == LLAMAHIP_POOL_LAST) {
        HIP_TRY(launch_gather_rows(m->x, last_idx, n, d, m->x1, m->stream), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(launch_norm_rows_f32(m->x1, m->norm_w, d, n, ed.y, m->stream), LLAMAHIP_ERR_PREDICT);
        for (int i = 0; i <= n; i++) seg[(size_t) i] = i;
    } else {
        HIP_TRY(launch_norm_rows_f32(m->x, m->norm_w, d, rp.R, ed.y, m->stream), LLAMAHIP_ERR_PREDICT);
        for (int i = 0; i < n; i++) seg[(size_t) i + 1] = seg[(size_t) i] + rp.n_tokens[i];
    }
    return embed_pool_enqueue(m, seg, rp.embed_pool, rp.embed_normalize, err, err_cap);
}

// one stage of the pass: its workspaces, the tokens (first stage), the launches -- enqueued, not waited for
static int rows_stage_enqueue(llamahip_model *st, int n_threads, const RowsPass &rp, const int32_t *tokens, const float *hidden_in, char *err, size_t err_cap) {
    HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_PREDICT);
    int rc;
    if ((rc = ensure_workspace(st, rp.R, err, err_cap)) != 0) return rc;
    if ((rc = ensure_attn_ws(st, 2, err, err_cap)) != 0) return rc;
    if ((rc = ensure_prompt_copies(st, rp.R, err, err_cap)) != 0) return rc;
    if (rp.score && st->last_stage) ensure_output_copies(st, rp.n_logits());
    if (rp.embed && st->last_stage && (rc = embed_ensure(st, rp.n_seqs, rp.embed_pool == LLAMAHIP_POOL_LAST ? rp.n_seqs : rp.R, err, err_cap)) != 0) return rc;
    if (st->first_stage) HIP_TRY(hipMemcpyAsync(st->d_tokens, tokens, (size_t) rp.R * 4, hipMemcpyHostToDevice, st->stream), LLAMAHIP_ERR_PREDICT);
    return forward_rows(st, n_threads, rp, hidden_in, err, err_cap);
}

// the handle takes the one pass at all: not f16 / f32 / Q4_1 files, not fast-prefill handles (their GEMM choice depends on the row count), a
// head size the table kernels take (llamahip_eval_multi and the scheduler's mixed pass share the rule)
static bool rows_pass_applies(llamahip_model *m) {
    const int dh = m->hp.n_embd / std::max(m->hp.n_head, 1);
    return !first_of(m)->dense && !(m->flags & LLAMAHIP_FLAG_FAST_PREFILL) && dh % 32 == 0 && dh <= 256;
}
// the pass's row table and its short / long segment counts, from rp's segments (slots, n_past, n_tokens, chunk, R set by the caller)
static int rows_pass_build(RowsPass &rp, int n_ctx) {
    rp.pos.resize((size_t) rp.R); rp.keys.resize((size_t) rp.R); rp.seg.resize((size_t) rp.R);
    if (llamahip_eval_multi_rows(n_ctx, rp.n_seqs, rp.n_past, rp.n_tokens, rp.chunk, rp.seg.data(), rp.pos.data(), rp.keys.data()) != rp.R) return -1;
    if (!rp.seg_single.empty())
        for (int r = 0; r < rp.R; r++) if (rp.seg_single[(size_t) rp.seg[r]]) rp.keys[r] = rp.pos[r] + 1;
    for (int i = 0; i < rp.n_seqs; i++) {
        if (rp.n_tokens[i] > rp.short_max) { rp.n_long_segs++; continue; }
        rp.n_short_segs++; rp.n_short_rows += rp.n_tokens[i];
        rp.max_keys = std::max(rp.max_keys, rp.n_past[i] + rp.n_tokens[i]);
    }
    return 0;
}
// the pass enqueued on every stage, the residual rows handed from stage to stage; not waited for
static int rows_pass_enqueue(const std::vector<llamahip_model *> &stages, int n_threads, const RowsPass &rp, const int32_t *tokens, char *err, size_t err_cap) {
    const int S = (int) stages.size();
    const size_t d = stages[0]->hp.n_embd;
    int rc = 0;
    for (int s = 1; s < S; s++) if ((rc = pipe_ensure_in(stages[s], rp.R, err, err_cap)) != 0) return rc;
    for (int s = 0; s < S && rc == 0; s++) {
        llamahip_model *st = stages[s];
        rc = rows_stage_enqueue(st, n_threads, rp, tokens, s ? st->pipe_in : nullptr, err, err_cap);
        if (rc == 0 && s + 1 < S) rc = pipe_hand_off(st, stages[s + 1], stages[s + 1]->pipe_in, st->x, (size_t) rp.R * d * 4, err, err_cap);
    }
    return rc;
}

int llamahip_eval_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *slots, const int32_t *n_past, const int32_t *tokens,
                        const int32_t *n_tokens, int32_t chunk_tokens, float *logits_out, llamahip_eval_multi_stats *stats, char *err, size_t err_cap) {
    static const char *fn = "llamahip_eval_multi";
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    int rc = eval_multi_check(m->hp.n_ctx, m->hp.n_vocab, m->n_seq, n_seqs, slots, n_past, tokens, n_tokens, chunk_tokens, err, err_cap);
    if (rc) return rc;
    if ((rc = decode_handle_check(m, fn, err, err_cap)) != 0) return rc;
    const std::vector<llamahip_model *> stages = stages_of(m);
    const int S = (int) stages.size();
    llamahip_model *last = stages[S - 1];
    const size_t V = m->hp.n_vocab;
    RowsPass rp;
    rp.n_seqs = n_seqs; rp.chunk = chunk_tokens; rp.slots = slots; rp.n_past = n_past; rp.n_tokens = n_tokens;
    for (int i = 0; i < n_seqs; i++) rp.R += n_tokens[i];
    llamahip_eval_multi_stats out = {};
    out.struct_size = (int32_t) sizeof(out);
    out.n_rows = rp.R;
    auto report = [&]() { if (stats) { const int32_t n = std::min((size_t) std::max(stats->struct_size, 0), sizeof(out)); if (n >= 4) { out.struct_size = n; memcpy(stats, &out, (size_t) n); } } };
    const bool dense = stages[0]->dense;
    // The per-slot loop of the contract itself: f16 / f32 / Q4_1 files, fast-prefill handles (their GEMM choice depends on the row count), one
    // segment (llamahip_eval_chunks is that pass), head sizes the table kernels do not take.
    // ... and the one shape family where the pass measured slower than the loop by more than the loop's spread (profiles/eval_multi_probe_7b.json:
    // 4 x 512 rows 0.98 x, 2 x 512 rows 1.02 x): more than 1024 rows in segments of 512 rows or more each -- evals that long no longer wait for weights.
    bool all_huge = rp.R > EVAL_MULTI_LOOP_ROWS;
    for (int i = 0; i < n_seqs; i++) all_huge = all_huge && n_tokens[i] >= EVAL_MULTI_LOOP_SEG_ROWS;
    if (!rows_pass_applies(m) || n_seqs == 1 || all_huge) {
        for (int i = 0; i < n_seqs; i++)
            out.n_passes += (dense && chunk_tokens > 0 && n_tokens[i] > chunk_tokens) ? (n_tokens[i] + chunk_tokens - 1) / chunk_tokens : 1;      // (llamahip_eval_chunks on such a file: one eval per chunk)
        std::vector<size_t> at((size_t) n_seqs, 0);
        for (int i = 1; i < n_seqs; i++) at[i] = at[i - 1] + (size_t) n_tokens[i - 1];
        rc = each_slot(m, n_seqs, slots, err, err_cap, [&](int i) {
            float *lo = logits_out ? logits_out + (size_t) i * V : nullptr;
            return chunk_tokens > 0 ? eval_chunks_impl(m, n_threads, n_past[i], tokens + at[i], n_tokens[i], chunk_tokens, lo, !dense, err, err_cap)
                                    : llamahip_eval(m, n_threads, n_past[i], tokens + at[i], n_tokens[i], lo, err, err_cap); });
        if (rc == 0) report();
        return rc;
    }
    // (measurement only, tools/eval_multi_probe.py --short-max: segments of up to that many rows join the table launch instead of taking launch_attn)
    static const int env_short_max = getenv("LLAMAHIP_EVAL_MULTI_SHORT_MAX") ? atoi(getenv("LLAMAHIP_EVAL_MULTI_SHORT_MAX")) : 0;
    if (env_short_max > 0) rp.short_max = env_short_max;
    const double t0 = now_ms();
    if (rows_pass_build(rp, m->hp.n_ctx) != 0) { set_err(err, err_cap, "%s: the row table could not be built", fn); return LLAMAHIP_ERR_PREDICT; }
    out.n_passes = 1; out.n_short_segs = rp.n_short_segs; out.n_long_segs = rp.n_long_segs;
    out.attn_groups = (rp.n_short_segs > 0 ? 1 : 0) + rp.n_long_segs;
    rc = rows_pass_enqueue(stages, n_threads, rp, tokens, err, err_cap);
    // (the bounded wait first, the copy of the logits rows behind it: pipe_eval)
    if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    if (logits_out) HIP_TRY(hipMemcpy(logits_out, last->logits, (size_t) n_seqs * V * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    m->last_rows.clear();
    m->n_evals++;
    m->t_eval_ms += now_ms() - t0;
    report();
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Scoring over several KV slots: llamahip_eval_logprobs_multi / llamahip_score_choices (llamahip.h).  llamahip_eval_multi's
// pass with RowsPass::logit_rows = the scored rows in ascending row order: the lm head runs over those nl rows alone, score_enqueue reduces
// them behind it on the last stage's stream with the targets compacted in the same order, nl x 16 bytes come back and score_scatter
// (eval_multi.cpp) puts them back into row order.
// ------------------------------------------------------------------------------------------------
static int logprobs_multi_impl(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *slots, const int32_t *n_past, const int32_t *tokens,
                               const int32_t *n_tokens, int32_t chunk_tokens, const int32_t *targets, double *lp, int32_t *am, int32_t *rk,
                               llamahip_score_multi_stats *stats, char *err, size_t err_cap) {
    static const char *fn = "llamahip_eval_logprobs_multi";
    const std::vector<llamahip_model *> stages = stages_of(m);
    llamahip_model *last = stages.back();
    RowsPass rp;
    rp.n_seqs = n_seqs; rp.chunk = chunk_tokens; rp.slots = slots; rp.n_past = n_past; rp.n_tokens = n_tokens;
    for (int i = 0; i < n_seqs; i++) rp.R += n_tokens[i];
    const int R = rp.R;
    std::vector<int32_t> tgt((size_t) R), scored((size_t) R);
    const int nl = score_multi_rows(n_seqs, tokens, n_tokens, targets, tgt.data(), scored.data());
    llamahip_score_multi_stats out = {};
    out.struct_size = (int32_t) sizeof(out);
    out.n_rows = R; out.n_scored_rows = nl;
    auto report = [&]() { if (stats) { const int32_t n = std::min((size_t) std::max(stats->struct_size, 0), sizeof(out)); if (n >= 4) { out.struct_size = n; memcpy(stats, &out, (size_t) n); } } };
    // llamahip_eval_multi's rule for the per-slot loop of the contract itself (see there); the argmax of an unscored row is dropped, so that
    // the outputs do not depend on the path
    bool all_huge = R > EVAL_MULTI_LOOP_ROWS;
    for (int i = 0; i < n_seqs; i++) all_huge = all_huge && n_tokens[i] >= EVAL_MULTI_LOOP_SEG_ROWS;
    if (!rows_pass_applies(m) || n_seqs == 1 || all_huge) {
        std::vector<size_t> at((size_t) n_seqs, 0);
        for (int i = 1; i < n_seqs; i++) at[i] = at[i - 1] + (size_t) n_tokens[i - 1];
        const int64_t evals0 = m->n_evals;
        const int rc = each_slot(m, n_seqs, slots, err, err_cap, [&](int i) {
            return logprobs_impl(m, n_threads, n_past[i], tokens + at[i], n_tokens[i], chunk_tokens, tgt.data() + at[i], lp ? lp + at[i] : nullptr,
                                 am ? am + at[i] : nullptr, rk ? rk + at[i] : nullptr, nullptr, err, err_cap); });
        if (rc) return rc;
        for (int r = 0; am && r < R; r++) if (tgt[r] < 0) am[r] = -1;
        out.n_passes = (int32_t) (m->n_evals - evals0);
        report();
        return LLAMAHIP_OK;
    }
    const double t0 = now_ms();
    rp.score = true; rp.logits_cap = R;
    rp.logit_rows.assign(scored.begin(), scored.begin() + nl);
    if (rows_pass_build(rp, m->hp.n_ctx) != 0) { set_err(err, err_cap, "%s: the row table could not be built", fn); return LLAMAHIP_ERR_PREDICT; }
    out.n_passes = 1; out.n_short_segs = rp.n_short_segs; out.n_long_segs = rp.n_long_segs;
    int rc = rows_pass_enqueue(stages, n_threads, rp, tokens, err, err_cap);
    std::vector<int32_t> ctgt((size_t) nl);          // (alive until the stages have drained)
    for (int k = 0; k < nl; k++) ctgt[k] = tgt[(size_t) scored[k]];
    if (rc == 0 && nl > 0) rc = score_enqueue(last, nl, ctgt.data(), err, err_cap);
    // (the bounded wait first, the copy of the results behind it: pipe_eval)
    if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
    std::vector<char> packed((size_t) nl * 16);
    if (nl > 0) {
        HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipMemcpy(packed.data(), last->d_score, packed.size(), hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    }
    score_scatter(R, nl, scored.data(), packed.data(), lp, am, rk);
    m->last_rows.clear();
    m->n_evals++;
    m->t_eval_ms += now_ms() - t0;
    report();
    return LLAMAHIP_OK;
}

int llamahip_eval_logprobs_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *slots, const int32_t *n_past, const int32_t *tokens,
                                 const int32_t *n_tokens, int32_t chunk_tokens, const int32_t *targets, double *logprob_out, int32_t *argmax_out,
                                 int32_t *rank_out, llamahip_score_multi_stats *stats, char *err, size_t err_cap) {
    static const char *fn = "llamahip_eval_logprobs_multi";
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    int rc = score_multi_check(m->hp.n_ctx, m->hp.n_vocab, m->n_seq, n_seqs, slots, n_past, tokens, n_tokens, chunk_tokens, targets, err, err_cap);
    if (rc) return rc;
    if ((rc = decode_handle_check(m, fn, err, err_cap)) != 0) return rc;
    return logprobs_multi_impl(m, n_threads, n_seqs, slots, n_past, tokens, n_tokens, chunk_tokens, targets, logprob_out, argmax_out, rank_out, stats, err, err_cap);
}

int llamahip_score_choices(llamahip_model *m, int32_t n_threads, const int32_t *context, int32_t n_context, int32_t n_choices, const int32_t *endings,
                           const int32_t *n_ending, int32_t chunk_tokens, double *logprob_sum, int32_t *n_greedy, double *logprob_rows,
                           char *err, size_t err_cap) {
    static const char *fn = "llamahip_score_choices";
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    int rc = score_choices_check(m->hp.n_ctx, m->hp.n_vocab, m->n_seq, context, n_context, n_choices, endings, n_ending, chunk_tokens, err, err_cap);
    if (rc) return rc;
    if (!logprob_sum) { set_err(err, err_cap, "%s: null logprob_sum", fn); return LLAMAHIP_ERR_PREDICT; }
    if (m->sched) { set_err(err, err_cap, "%s: the handle has a live scheduler, which owns KV slots 0 .. %d: free it first", fn, sched_dev_max_active(m->sched) - 1); return LLAMAHIP_ERR_PREDICT; }
    if ((rc = decode_handle_check(m, fn, err, err_cap)) != 0) return rc;
    const int n = n_choices, P = n_context - 1;
    // the segments: choice i = [the context's last token, ending_i without its last token] at P on slot i, every row scored against ending_i
    std::vector<int32_t> slots((size_t) n), past((size_t) n, P), toks, tgt;
    for (int i = 0, e = 0; i < n; e += n_ending[i], i++) {
        slots[i] = i;
        toks.push_back(context[P]);
        toks.insert(toks.end(), endings + e, endings + e + n_ending[i] - 1);
        tgt.insert(tgt.end(), endings + e, endings + e + n_ending[i]);
    }
    const int R = (int) toks.size();
    if (P > 0) {
        // the context once, on slot 0 (enqueued and waited for as the entry point it is), then its rows to the other slots: one launch per stage,
        // stream-ordered ahead of the pass, no host wait
        const int32_t zero = 0;
        rc = each_slot(m, 1, &zero, err, err_cap, [&](int) {
            return chunk_tokens > 0 ? eval_chunks_impl(m, n_threads, 0, context, P, chunk_tokens, nullptr, true, err, err_cap)
                                    : llamahip_eval(m, n_threads, 0, context, P, nullptr, err, err_cap); });
        if (rc) return rc;
        if (n > 1) {
            KvCopyTab tab = {};
            tab.n = n - 1;
            for (int i = 1; i < n; i++) { tab.src[i - 1] = 0; tab.dst[i - 1] = i; tab.row_begin[i - 1] = 0; tab.n_rows[i - 1] = P; }
            const std::vector<llamahip_model *> stages = stages_of(m);
            if ((rc = kv_copy_enqueue(stages, tab, fn, err, err_cap)) != 0) return drain_stages(stages, rc, err, err_cap);
        }
    }
    std::vector<double> lp((size_t) R);
    std::vector<int32_t> rk((size_t) R);
    rc = logprobs_multi_impl(m, n_threads, n, slots.data(), past.data(), toks.data(), n_ending, 0, tgt.data(), lp.data(), nullptr, rk.data(), nullptr, err, err_cap);
    if (rc) return rc;
    for (int i = 0, r = 0; i < n; i++) {
        double sum = 0.0;
        int32_t greedy = 0;
        for (int j = 0; j < n_ending[i]; j++, r++) { sum += lp[(size_t) r]; greedy += rk[(size_t) r] == 0; }
        logprob_sum[i] = sum;
        if (n_greedy) n_greedy[i] = greedy;
    }
    if (logprob_rows) std::copy(lp.begin(), lp.end(), logprob_rows);
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// A text's embedding: llamahip_text_embedding / llamahip_text_embedding_multi (llamahip.h).  The eval of the same arguments --
// llamahip_eval_chunks' split for one text, llamahip_eval_multi's pass for several -- with the lm head replaced by pool.hip's launches on the last
// stage's stream; n_embd floats per text come back from the last stage's d_embed.
// ------------------------------------------------------------------------------------------------
// one text on the current slot (checked by the caller), on a plain or a pipeline handle, every file type
static int embed_text_impl(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t N, int32_t chunk_tokens, int32_t pool,
                           int32_t normalize, float *out, char *err, size_t err_cap) {
    const std::vector<llamahip_model *> stages = stages_of(m);
    const int S = (int) stages.size();
    llamahip_model *last = stages[S - 1];
    const size_t d = m->hp.n_embd;
    const bool mean = pool == LLAMAHIP_POOL_MEAN;
    int rc;
    if ((rc = embed_ensure(last, 1, mean ? N : 1, err, err_cap)) != 0) return rc;
    const EmbedDev ed = embed_dev(last);
    // llamahip_eval_chunks' split: one pass with the chunks' key splits where the file type has one, else eval by eval
    const bool chunked = chunk_tokens > 0 && N > chunk_tokens, one_pass = !chunked || chunks_in_one_pass(m, N);
    const int step = one_pass ? N : chunk_tokens;
    for (int32_t c0 = 0; c0 < N; c0 += step) {
        const double t0 = now_ms();
        const int32_t n = std::min(step, N - c0);
        const bool final = c0 + n == N;
        const EmbedReq rq = mean ? EmbedReq{ ed.y + (size_t) c0 * d, 0 } : final ? EmbedReq{ ed.y, n - 1 } : EmbedReq{ nullptr, 0 };
        rc = 0;
        for (int s = 1; s < S && rc == 0; s++) rc = pipe_ensure_in(stages[s], n, err, err_cap);
        if (rc) return rc;
        for (int s = 0; s < S && rc == 0; s++) {
            llamahip_model *st = stages[s];
            st->cur_seq = m->cur_seq;
            rc = eval_stage_enqueue(st, n_threads, n_past + c0, tokens + c0, n, s ? st->pipe_in : nullptr, one_pass && chunked ? chunk_tokens : 0, false, err, err_cap, &rq);
            if (rc == 0 && s + 1 < S) rc = pipe_hand_off(st, stages[s + 1], stages[s + 1]->pipe_in, st->x, (size_t) n * d * 4, err, err_cap);
        }
        if (rc == 0 && final) {
            HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
            rc = embed_pool_enqueue(last, { 0, mean ? N : 1 }, pool, normalize, err, err_cap);
        }
        // (the bounded wait first, the copy of the result behind it: pipe_eval)
        if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
        m->n_evals++;
        m->t_eval_ms += now_ms() - t0;
    }
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipMemcpy(out, ed.out, d * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    return LLAMAHIP_OK;
}

int llamahip_text_embedding(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t n_tokens, int32_t chunk_tokens,
                            int32_t pool, int32_t normalize, float *out, char *err, size_t err_cap) {
    static const char *fn = "llamahip_text_embedding";
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    const int32_t slot = m->cur_seq;
    int rc = embed_check(fn, m->hp.n_ctx, m->hp.n_vocab, m->n_seq, m->sched ? sched_dev_max_active(m->sched) : 0, 1, &slot, &n_past, tokens, &n_tokens,
                         chunk_tokens, pool, normalize, out, err, err_cap);
    if (rc) return rc;
    if ((rc = decode_handle_check(m, fn, err, err_cap)) != 0) return rc;
    return embed_text_impl(m, n_threads, n_past, tokens, n_tokens, chunk_tokens, pool, normalize, out, err, err_cap);
}

int llamahip_text_embedding_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *slots, const int32_t *n_past, const int32_t *tokens,
                                  const int32_t *n_tokens, int32_t chunk_tokens, int32_t pool, int32_t normalize, float *out,
                                  llamahip_eval_multi_stats *stats, char *err, size_t err_cap) {
    static const char *fn = "llamahip_text_embedding_multi";
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    int rc = embed_check(fn, m->hp.n_ctx, m->hp.n_vocab, m->n_seq, m->sched ? sched_dev_max_active(m->sched) : 0, n_seqs, slots, n_past, tokens, n_tokens,
                         chunk_tokens, pool, normalize, out, err, err_cap);
    if (rc) return rc;
    if ((rc = decode_handle_check(m, fn, err, err_cap)) != 0) return rc;
    const std::vector<llamahip_model *> stages = stages_of(m);
    llamahip_model *last = stages.back();
    const size_t d = m->hp.n_embd;
    RowsPass rp;
    rp.n_seqs = n_seqs; rp.chunk = chunk_tokens; rp.slots = slots; rp.n_past = n_past; rp.n_tokens = n_tokens;
    for (int i = 0; i < n_seqs; i++) rp.R += n_tokens[i];
    llamahip_eval_multi_stats st_out = {};
    st_out.struct_size = (int32_t) sizeof(st_out);
    st_out.n_rows = rp.R;
    auto report = [&]() { if (stats) { const int32_t n = std::min((size_t) std::max(stats->struct_size, 0), sizeof(st_out)); if (n >= 4) { st_out.struct_size = n; memcpy(stats, &st_out, (size_t) n); } } };
    // llamahip_eval_multi's rule for the per-slot loop (see there)
    bool all_huge = rp.R > EVAL_MULTI_LOOP_ROWS;
    for (int i = 0; i < n_seqs; i++) all_huge = all_huge && n_tokens[i] >= EVAL_MULTI_LOOP_SEG_ROWS;
    if (!rows_pass_applies(m) || n_seqs == 1 || all_huge) {
        std::vector<size_t> at((size_t) n_seqs, 0);
        for (int i = 1; i < n_seqs; i++) at[i] = at[i - 1] + (size_t) n_tokens[i - 1];
        const int64_t evals0 = m->n_evals;
        rc = each_slot(m, n_seqs, slots, err, err_cap, [&](int i) {
            return embed_text_impl(m, n_threads, n_past[i], tokens + at[i], n_tokens[i], chunk_tokens, pool, normalize, out + (size_t) i * d, err, err_cap); });
        if (rc) return rc;
        st_out.n_passes = (int32_t) (m->n_evals - evals0);
        report();
        return LLAMAHIP_OK;
    }
    const double t0 = now_ms();
    rp.embed = true; rp.embed_pool = pool; rp.embed_normalize = normalize;
    if (rows_pass_build(rp, m->hp.n_ctx) != 0) { set_err(err, err_cap, "%s: the row table could not be built", fn); return LLAMAHIP_ERR_PREDICT; }
    st_out.n_passes = 1; st_out.n_short_segs = rp.n_short_segs; st_out.n_long_segs = rp.n_long_segs;
    st_out.attn_groups = (rp.n_short_segs > 0 ? 1 : 0) + rp.n_long_segs;
    rc = rows_pass_enqueue(stages, n_threads, rp, tokens, err, err_cap);
    // (the bounded wait first, the copy of the vectors behind it: pipe_eval)
    if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipMemcpy(out, embed_dev(last).out, (size_t) n_seqs * d * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    m->n_evals++;
    m->t_eval_ms += now_ms() - t0;
    report();
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Drafted greedy decoding: llamahip_verify_greedy / llamahip_decode_greedy_lookup.  A verify step is ONE eval of the rows
// [last accepted token, draft ...] at n_past in which every row takes the V*P key split of its own single-token eval (chunk = 1, as
// llamahip_eval_chunks) and the last stage's lm head runs over every row (as the scoring entry points); row j then holds the logits of
// a single-token eval at n_past + j.  k_verify_rows picks each row's token and k_accept_drafts counts how much of the draft the picks
// reproduce (verify.hip), on the last stage's stream: {n_accept, picks} come back through the pinned block, 4 (N + 1) bytes.
// ------------------------------------------------------------------------------------------------
struct VerifyIo { int32_t *state, *tok, *pick, *res, *log; };
static VerifyIo verify_io(llamahip_model *m) { return { m->d_verify, m->d_verify + 2, m->d_verify + 18, m->d_verify + 34, m->d_verify + 64 }; }
static int verify_ensure(llamahip_model *last, char *err, size_t err_cap) {
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    if (last->d_verify) return 0;
    HIP_TRY(last->own.alloc(&last->d_verify, 64 + (size_t) last->hp.n_ctx, true), LLAMAHIP_ERR_PREDICT);
    return 0;
}
// the two kernels over the N rows of last->logits, ordered behind the eval on last->stream (restart_pos >= 0: the log starts over there)
static int verify_enqueue(llamahip_model *last, const int32_t *rows, int N, int restart_pos, char *err, size_t err_cap) {
    int rc = verify_ensure(last, err, err_cap);
    if (rc) return rc;
    const VerifyIo io = verify_io(last);
    const int32_t *tok = io.tok;
    int32_t *res = io.res;
    if (last->h_io) {                       // (the stream is idle: every entry point synchronises before it returns)
        memcpy(last->h_io->tok, rows, (size_t) N * 4);
        tok = last->d_io->tok; res = last->d_io->id;
    } else HIP_TRY(hipMemcpyAsync(io.tok, rows, (size_t) N * 4, hipMemcpyHostToDevice, last->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(launch_verify_rows(last->logits, N, last->hp.n_vocab, io.pick, last->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(launch_accept_drafts(tok, io.pick, 0, N, restart_pos, io.log, last->hp.n_ctx, io.state, res, last->stream), LLAMAHIP_ERR_PREDICT);
    return 0;
}
// a single-token step of the lookup loop took `pick` by the fused decode step: the same log and position word, one more entry (not waited for)
static int verify_append(llamahip_model *last, int32_t pick, int restart_pos, char *err, size_t err_cap) {
    int rc = verify_ensure(last, err, err_cap);
    if (rc) return rc;
    const VerifyIo io = verify_io(last);
    HIP_TRY(launch_accept_drafts(nullptr, nullptr, pick, 1, restart_pos, io.log, last->hp.n_ctx, io.state, io.res, last->stream), LLAMAHIP_ERR_PREDICT);
    return 0;
}

// The sampled verify step's device half (llamahip_verify_sample): behind the eval, in place of the two kernels above, the sampler's candidate
// selection over the N rows with row r's window = ids[r .. r + n_last) (launch_topk_slide).  ids: the sampler's window followed by the draft,
// n_last + N - 1 ids; k == 0: the device cannot make candidates (top_k > 64, n_vocab > 32768, a window longer than 1024 ids) -- nothing is
// launched and the walk takes every row it reaches from its logits.  out: N rows, valid after the step.
struct SlideReq { const int32_t *ids; int n_last; double scale, repeat_penalty; int k; TopkOut *out; };
constexpr size_t SLIDE_WS_BYTES = (size_t) VERIFY_ROWS_MAX * TOPK_WS_BYTES, SLIDE_IDS_BYTES = (1024 + VERIFY_ROWS_MAX) * 4;
static int slide_ensure(llamahip_model *last, char *err, size_t err_cap) {
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    if (last->d_slide) return 0;
    const size_t bytes = SLIDE_WS_BYTES + SLIDE_IDS_BYTES + VERIFY_ROWS_MAX * sizeof(TopkOut);
    HIP_TRY(last->own.alloc(&last->d_slide, bytes, true), LLAMAHIP_ERR_PREDICT);
    return 0;
}
static int slide_enqueue(llamahip_model *last, const SlideReq &sl, int N, char *err, size_t err_cap) {
    if (sl.k == 0) return 0;
    int rc = slide_ensure(last, err, err_cap);
    if (rc) return rc;
    const size_t n_ids = (size_t) sl.n_last + N - 1;
    int32_t *ids = (int32_t *) (last->d_slide + SLIDE_WS_BYTES);
    TopkOut *out = (TopkOut *) (last->d_slide + SLIDE_WS_BYTES + SLIDE_IDS_BYTES);
    if (last->h_io) {                       // (the stream is idle: every entry point synchronises before it returns)
        memcpy(last->h_io->slide, sl.ids, n_ids * 4);
        ids = last->d_io->slide; out = last->d_io->rows;
    } else HIP_TRY(hipMemcpyAsync(ids, sl.ids, n_ids * 4, hipMemcpyHostToDevice, last->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(launch_topk_slide(last->logits, N, last->hp.n_vocab, ids, sl.n_last, sl.scale, sl.repeat_penalty, sl.k, out, last->stream, last->d_slide), LLAMAHIP_ERR_PREDICT);
    return 0;
}
// the N rows of candidates a sampled step (slide_enqueue, slide_set_enqueue) left, after the step was waited for; the last stage's device is current
static int slide_fetch(llamahip_model *last, TopkOut *out, int N, char *err, size_t err_cap) {
    if (last->h_io) memcpy(out, last->h_io->rows, (size_t) N * sizeof(TopkOut));
    else HIP_TRY(hipMemcpy(out, last->d_slide + SLIDE_WS_BYTES + SLIDE_IDS_BYTES, (size_t) N * sizeof(TopkOut), hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    return 0;
}

// one verify step of N = 2 .. 16 rows on a Q4_0 handle, plain or pipeline (eval_score's walk); res: {n_accept, picks[N]}
// (sl != nullptr: the sampled step -- res and logits_next unused, sl->out receives the rows' candidates)
static int verify_step(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *rows, int N, int restart_pos, int32_t *res,
                       float *logits_next, char *err, size_t err_cap, const SlideReq *sl = nullptr) {
    const double t0 = now_ms();
    llamahip_model *last = last_of(m);
    int rc;
    if (m->stages.empty()) {
        if ((rc = eval_stage_enqueue(m, n_threads, n_past, rows, N, nullptr, 1, true, err, err_cap)) != 0) return rc;
        if ((rc = sl ? slide_enqueue(m, *sl, N, err, err_cap) : verify_enqueue(m, rows, N, restart_pos, err, err_cap)) != 0) return rc;
        HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
        if ((rc = check_sync_timeout(m, err, err_cap)) != 0) return rc;
    } else {
        const int S = (int) m->stages.size();
        const size_t d = m->hp.n_embd;
        for (int s = 1; s < S; s++) if ((rc = pipe_ensure_in(m->stages[s], N, err, err_cap)) != 0) return rc;
        for (int s = 0; s < S; s++) {
            llamahip_model *st = m->stages[s];
            st->cur_seq = m->cur_seq;
            if ((rc = eval_stage_enqueue(st, n_threads, n_past, rows, N, s ? st->pipe_in : nullptr, 1, s == S - 1, err, err_cap)) != 0) { (void) pipe_sync(m, nullptr, 0); return rc; }
            if (s + 1 < S && (rc = pipe_hand_off(st, m->stages[s + 1], m->stages[s + 1]->pipe_in, st->x, (size_t) N * d * 4, err, err_cap)) != 0) { (void) pipe_sync(m, nullptr, 0); return rc; }
        }
        if ((rc = sl ? slide_enqueue(last, *sl, N, err, err_cap) : verify_enqueue(last, rows, N, restart_pos, err, err_cap)) != 0) { (void) pipe_sync(m, nullptr, 0); return rc; }
        if ((rc = pipe_sync(m, err, err_cap)) != 0) return rc;
        HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    }
    if (sl) {
        if (sl->k > 0 && (rc = slide_fetch(last, sl->out, N, err, err_cap)) != 0) return rc;
        m->n_evals++;
        m->t_eval_ms += now_ms() - t0;
        return LLAMAHIP_OK;
    }
    if (last->h_io) memcpy(res, last->h_io->id, (size_t) (N + 1) * 4);
    else HIP_TRY(hipMemcpy(res, verify_io(last).res, (size_t) (N + 1) * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    if (res[0] < 0 || res[0] > N - 1) { set_err(err, err_cap, "verify step: the device reported %d accepted of %d drafted tokens", res[0], N - 1); return LLAMAHIP_ERR_PREDICT; }
    const size_t V = m->hp.n_vocab;
    if (logits_next) HIP_TRY(hipMemcpy(logits_next, last->logits + (size_t) res[0] * V, V * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    m->n_evals++;
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}

static bool lookup_dense(llamahip_model *m) { return first_of(m)->dense; }

// the arguments first (a HOST_ONLY handle knows n_vocab / n_ctx: the checks are the same without a device), then the handle
static int check_verify_args(llamahip_model *m, int32_t n_past, int32_t token, const int32_t *draft, int32_t n_draft, const char *fn, char *err, size_t err_cap) {
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    const int V = m->hp.n_vocab, C = m->hp.n_ctx;
    if (n_draft < 0 || n_draft > VERIFY_ROWS_MAX - 1) { set_err(err, err_cap, "%s: n_draft must be 0 .. %d (got %d): a verify step has at most %d rows", fn, VERIFY_ROWS_MAX - 1, n_draft, VERIFY_ROWS_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (n_past < 0 || n_past > C - n_draft - 1) { set_err(err, err_cap, "%s: context overflow: n_past (%d) + n_draft (%d) + 1 > n_ctx (%d)", fn, n_past, n_draft, C); return LLAMAHIP_ERR_PREDICT; }
    if (token < 0 || token >= V) { set_err(err, err_cap, "%s: token id %d out of range [0, %d)", fn, token, V); return LLAMAHIP_ERR_PREDICT; }
    if (n_draft > 0 && !draft) { set_err(err, err_cap, "%s: null draft", fn); return LLAMAHIP_ERR_PREDICT; }
    for (int i = 0; i < n_draft; i++)
        if (draft[i] < 0 || draft[i] >= V) { set_err(err, err_cap, "%s: draft token id %d at %d out of range [0, %d)", fn, draft[i], i, V); return LLAMAHIP_ERR_PREDICT; }
    if (m->stages.empty() && (!m->first_stage || !m->last_stage)) { set_err(err, err_cap, "%s on a pipeline-stage handle: load the whole model (or a device list)", fn); return LLAMAHIP_ERR_PREDICT; }
    return check_eval_args(first_of(m), n_past, &token, 1, true, err, err_cap);      // (HOST_ONLY: refused here)
}

static int verify_greedy_impl(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t token, const int32_t *draft, int32_t n_draft, int restart_pos,
                              int32_t *n_accept, int32_t *picks, float *logits_next, char *err, size_t err_cap) {
    const int N = n_draft + 1;
    if (N == 1 || lookup_dense(m)) {
        // one plain step -- and f16 / f32 / Q4_1 files, which have no per-row key split in one pass: the rows one single-token step at a
        // time, stopping behind the first pick the draft does not continue with
        int a = 0;
        int32_t tok = token;
        for (;; a++) {
            int rc = llamahip_decode_greedy(m, n_threads, n_past + a, tok, 1, &picks[a], nullptr, err, err_cap);
            if (rc) return rc;
            if (a == n_draft || picks[a] != draft[a]) break;
            tok = draft[a];
        }
        for (int j = a + 1; j < N; j++) picks[j] = -1;
        *n_accept = a;
        llamahip_model *last = last_of(m);
        if (logits_next) {
            HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(hipMemcpy(logits_next, last->logits, (size_t) m->hp.n_vocab * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
        }
        return LLAMAHIP_OK;
    }
    int32_t rows[VERIFY_ROWS_MAX], res[VERIFY_ROWS_MAX + 1];
    rows[0] = token;
    for (int i = 0; i < n_draft; i++) rows[1 + i] = draft[i];
    int rc = verify_step(m, n_threads, n_past, rows, N, restart_pos, res, logits_next, err, err_cap);
    if (rc) return rc;
    *n_accept = res[0];
    memcpy(picks, res + 1, (size_t) N * 4);
    return LLAMAHIP_OK;
}

int llamahip_verify_greedy(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t token, const int32_t *draft, int32_t n_draft,
                           int32_t *n_accept, int32_t *picks, float *logits_next, char *err, size_t err_cap) {
    int rc = check_verify_args(m, n_past, token, draft, n_draft, "llamahip_verify_greedy", err, err_cap);
    if (rc) return rc;
    if (!n_accept || !picks) { set_err(err, err_cap, "llamahip_verify_greedy: null output"); return LLAMAHIP_ERR_PREDICT; }
    return verify_greedy_impl(m, n_threads, n_past, token, draft, n_draft, n_past, n_accept, picks, logits_next, err, err_cap);
}

// the arguments of the two lookup loops (greedy and sampled), checked without a device; the handle last
static int check_lookup_args(llamahip_model *m, const char *fn, int32_t n_past, int32_t first_token, int32_t n_steps, const int32_t *context, int32_t n_context,
                             const int32_t *corpus, int32_t n_corpus, int32_t draft_len, int32_t ngram_min, int32_t ngram_max, const int32_t *out_tokens,
                             const llamahip_lookup_stats *stats, char *err, size_t err_cap, bool handle = true) {      // handle = false: the arguments alone
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    const int V = m->hp.n_vocab, C = m->hp.n_ctx;
    if (n_steps < 1 || n_past < 0 || n_past > C - n_steps) { set_err(err, err_cap, "%s: context overflow: n_past (%d) + n_steps (%d) > n_ctx (%d)", fn, n_past, n_steps, C); return LLAMAHIP_ERR_PREDICT; }
    if (first_token < 0 || first_token >= V) { set_err(err, err_cap, "%s: token id %d out of range [0, %d)", fn, first_token, V); return LLAMAHIP_ERR_PREDICT; }
    if (n_context != n_past) { set_err(err, err_cap, "%s: n_context (%d) must equal n_past (%d): the drafter's history is the tokens at positions [0, n_past)", fn, n_context, n_past); return LLAMAHIP_ERR_PREDICT; }
    if (n_context > 0 && !context) { set_err(err, err_cap, "%s: null context", fn); return LLAMAHIP_ERR_PREDICT; }
    for (int i = 0; i < n_context; i++)
        if (context[i] < 0 || context[i] >= V) { set_err(err, err_cap, "%s: context token id %d at %d out of range [0, %d)", fn, context[i], i, V); return LLAMAHIP_ERR_PREDICT; }
    if (n_corpus < 0 || (n_corpus > 0 && !corpus)) { set_err(err, err_cap, "%s: a corpus of %d tokens at a null pointer", fn, n_corpus); return LLAMAHIP_ERR_PREDICT; }
    for (int i = 0; i < n_corpus; i++)
        if (corpus[i] < 0 || corpus[i] >= V) { set_err(err, err_cap, "%s: corpus token id %d at %d out of range [0, %d)", fn, corpus[i], i, V); return LLAMAHIP_ERR_PREDICT; }
    if (draft_len < 0 || draft_len > VERIFY_ROWS_MAX - 1) { set_err(err, err_cap, "%s: draft_len must be 1 .. %d (0 = the default, %d; got %d)", fn, VERIFY_ROWS_MAX - 1, LLAMAHIP_LOOKUP_DRAFT_LEN, draft_len); return LLAMAHIP_ERR_PREDICT; }
    if (ngram_min < 0 || ngram_max < 0 || ((ngram_min ? ngram_min : LLAMAHIP_LOOKUP_NGRAM_MIN) > (ngram_max ? ngram_max : LLAMAHIP_LOOKUP_NGRAM_MAX))) {
        set_err(err, err_cap, "%s: ngram_min (%d) / ngram_max (%d) must be positive with ngram_min <= ngram_max (0 = the defaults, %d and %d)", fn, ngram_min, ngram_max,
                LLAMAHIP_LOOKUP_NGRAM_MIN, LLAMAHIP_LOOKUP_NGRAM_MAX);
        return LLAMAHIP_ERR_PREDICT;
    }
    if (!out_tokens) { set_err(err, err_cap, "%s: null out_tokens", fn); return LLAMAHIP_ERR_PREDICT; }
    if (stats && stats->struct_size != (int32_t) sizeof(llamahip_lookup_stats)) { set_err(err, err_cap, "%s: stats->struct_size (%d) is not sizeof(llamahip_lookup_stats) (%d)", fn, stats->struct_size, (int) sizeof(llamahip_lookup_stats)); return LLAMAHIP_ERR_PREDICT; }
    if (!handle) return 0;
    if (m->stages.empty() && (!m->first_stage || !m->last_stage)) { set_err(err, err_cap, "%s on a pipeline-stage handle: load the whole model (or a device list)", fn); return LLAMAHIP_ERR_PREDICT; }
    return check_eval_args(first_of(m), n_past, &first_token, 1, true, err, err_cap);      // (HOST_ONLY: refused here)
}

// the rows of a verify step over a set (vset_step, below), cut into segments: one per sequence, [its last token, its draft ...]
struct VsetReq {
    int n_segs = 0, n_rows = 0;
    int32_t slot[SET_MAX], pos[SET_MAX];        // per segment: KV slot, position of its first row
    int32_t seg_begin[SET_MAX + 1];
    int32_t rows[SET_MAX];                      // the rows' tokens
    bool bound = false;                         // the slots are bound (the loop): logs, {position, cursor} and next-token words are kept on the device
};

// A lookup run over n sequences (n = 1: the single-sequence loops): what the host knows of each sequence and what it does between two steps.
// A round is: active() -> draft_round() -> one step of the caller's (a plain step, or a verify step over segments()) -> accept() per sequence.
struct LookupRun {
    const char *fn = nullptr;
    int n = 0, n_steps = 0, K = 0, n_corpus = 0, ngram_min = 0, ngram_max = 0;
    const int32_t *n_past = nullptr, *corpus = nullptr;
    int32_t *out_tokens = nullptr, *out_exact = nullptr;    // the sampled loops: accept() writes sequence i's picks (and exact flags) at [i * n_steps + done[i], ..)
    std::vector<size_t> coff;                               // sequence i's context: n_past[i] tokens at contexts + coff[i]
    std::vector<std::vector<int32_t>> hist;                 // hist[i][0 .. pos]: the tokens at positions [0, pos], the last one not evaluated yet
    std::vector<int> done;
    std::vector<llamahip_lookup_stats> ls;
    int32_t want[SET_MAX], give[SET_MAX], draft[SET_MAX][VERIFY_ROWS_MAX];      // the round's drafts, by index into its active list

    int pos(int i) const { return n_past[i] + done[i]; }
    int32_t token(int i) const { return hist[i][(size_t) pos(i)]; }
    // the context offsets (a negative n_past is refused here, in check_lookup_args' words, before that function is given a context pointer)
    int open(const char *fn_, int n_ctx, int n_, const int32_t *n_past_, int n_steps_, char *err, size_t err_cap) {
        fn = fn_; n = n_; n_past = n_past_; n_steps = n_steps_;
        coff.assign((size_t) n + 1, 0);
        for (int i = 0; i < n; i++) {
            if (n_past[i] < 0) { set_err(err, err_cap, "%s: context overflow: n_past (%d) + n_steps (%d) > n_ctx (%d)", fn, n_past[i], n_steps, n_ctx); return LLAMAHIP_ERR_PREDICT; }
            coff[i + 1] = coff[i] + (size_t) n_past[i];
        }
        return 0;
    }
    void start(const int32_t *first_tokens, const int32_t *contexts, const int32_t *corpus_, int n_corpus_, int draft_len, int ngram_min_, int ngram_max_) {
        corpus = corpus_; n_corpus = n_corpus_; ngram_min = ngram_min_; ngram_max = ngram_max_;
        K = draft_len ? draft_len : LLAMAHIP_LOOKUP_DRAFT_LEN;
        hist.resize(n);
        done.assign(n, 0);
        ls.assign(n, llamahip_lookup_stats{ (int32_t) sizeof(llamahip_lookup_stats), 0, 0, 0, 0 });
        for (int i = 0; i < n; i++) {
            hist[i].resize((size_t) n_past[i] + n_steps + 1);
            if (n_past[i] > 0) memcpy(hist[i].data(), contexts + coff[i], (size_t) n_past[i] * 4);
            hist[i][n_past[i]] = first_tokens[i];
        }
    }
    bool active(std::vector<int32_t> &act) const {
        act.clear();
        for (int i = 0; i < n; i++) if (done[i] < n_steps) act.push_back(i);
        return !act.empty();
    }
    // what every active sequence that may draft wants (want, draft), then the spare rows of a 16-row step dealt among them (give); *dealt: their sum
    int draft_round(const std::vector<int32_t> &act, const std::function<bool(int)> &may_draft, int *dealt, char *err, size_t err_cap) {
        const int A = (int) act.size();
        for (int a = 0; a < A; a++) {
            const int i = act[a];
            // (the last row evaluated is position n_past + n_steps - 1: a draft that would pass it is cut)
            const int room = may_draft(i) ? std::min(K, n_steps - done[i] - 1) : 0;
            want[a] = room > 0 ? llamahip_lookup_draft(hist[i].data(), pos(i) + 1, corpus, n_corpus, room, ngram_min, ngram_max, draft[a]) : 0;
            if (want[a] < 0 || want[a] > room) { set_err(err, err_cap, "%s: the drafter returned %d tokens for a draft of %d", fn, want[a], room); return LLAMAHIP_ERR_PREDICT; }
        }
        *dealt = llamahip_lookup_deal_rows(want, A, SET_MAX, give);
        if (*dealt < 0) { set_err(err, err_cap, "%s: dealing the rows of a step failed", fn); return LLAMAHIP_ERR_PREDICT; }
        return 0;
    }
    // the verify step of the round: segment a = sequence act[a] in slot act[a], its last token and the give[a] draft tokens it was dealt
    void segments(const std::vector<int32_t> &act, VsetReq &rq) const {
        const int A = (int) act.size();
        int R = 0;
        for (int a = 0; a < A; a++) {
            const int i = act[a];
            rq.slot[a] = i; rq.pos[a] = pos(i); rq.seg_begin[a] = R;
            rq.rows[R++] = token(i);
            for (int j = 0; j < give[a]; j++) rq.rows[R++] = draft[a][j];
        }
        rq.seg_begin[A] = R; rq.n_segs = A; rq.n_rows = R;
    }
    // sequence i took n_picks tokens in a step that carried n_give draft tokens for it (0: a single step); mirror: the stages whose host-side
    // slot position follows (a verify step over a set moves the slots' device words without the stage API)
    void accept(int i, int n_give, const int32_t *picks, const int32_t *exact, int n_picks, const std::vector<llamahip_model *> *mirror = nullptr) {
        memcpy(hist[i].data() + pos(i) + 1, picks, (size_t) n_picks * 4);
        if (out_tokens) memcpy(out_tokens + (size_t) i * n_steps + done[i], picks, (size_t) n_picks * 4);
        if (out_exact) memcpy(out_exact + (size_t) i * n_steps + done[i], exact, (size_t) n_picks * 4);
        done[i] += n_picks;
        if (n_give > 0) { ls[i].n_verify_steps++; ls[i].n_drafted += n_give; ls[i].n_accepted += n_picks - 1; }
        else ls[i].n_single_steps++;
        if (mirror) for (llamahip_model *st : *mirror) st->slots[i].next_pos += n_picks;
    }
};

int llamahip_decode_greedy_lookup(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token, int32_t n_steps,
                                  const int32_t *context, int32_t n_context, const int32_t *corpus, int32_t n_corpus,
                                  int32_t draft_len, int32_t ngram_min, int32_t ngram_max,
                                  int32_t *out_tokens, float *logits_last, llamahip_lookup_stats *stats, char *err, size_t err_cap) {
    static const char *fn = "llamahip_decode_greedy_lookup";
    int rc = check_lookup_args(m, fn, n_past, first_token, n_steps, context, n_context, corpus, n_corpus, draft_len, ngram_min, ngram_max, out_tokens, stats, err, err_cap);
    if (rc) return rc;
    const int V = m->hp.n_vocab;
    if (lookup_dense(m)) {
        // f16 / f32 / Q4_1 files: no multi-row eval with every row's own key split -- nothing is drafted
        if ((rc = llamahip_decode_greedy(m, n_threads, n_past, first_token, n_steps, out_tokens, logits_last, err, err_cap)) != 0) return rc;
        if (stats) *stats = llamahip_lookup_stats{ (int32_t) sizeof(llamahip_lookup_stats), 0, n_steps, 0, 0 };
        return LLAMAHIP_OK;
    }
    llamahip_model *last = last_of(m);
    LookupRun run;
    if ((rc = run.open(fn, m->hp.n_ctx, 1, &n_past, n_steps, err, err_cap)) != 0) return rc;
    run.start(&first_token, context, corpus, n_corpus, draft_len, ngram_min, ngram_max);
    const std::vector<int32_t> act{ 0 };
    while (run.done[0] < n_steps) {
        const int done = run.done[0], pos = n_past + done, restart = done == 0 ? n_past : -1;
        int nd = 0;
        if ((rc = run.draft_round(act, [](int) { return true; }, &nd, err, err_cap)) != 0) return rc;
        int32_t res[VERIFY_ROWS_MAX + 1] = { 0 };       // {n_accept, picks}
        if (nd == 0) {
            // nothing to verify: the fused single-token step, its pick appended to the device log behind it
            if ((rc = llamahip_decode_greedy(m, n_threads, pos, run.token(0), 1, res + 1, done + 1 == n_steps ? logits_last : nullptr, err, err_cap)) != 0) return rc;
            if ((rc = verify_append(last, res[1], restart, err, err_cap)) != 0) return rc;
        } else {
            VsetReq rq;                                  // (one segment: its rows are the step's)
            run.segments(act, rq);
            if ((rc = verify_step(m, n_threads, pos, rq.rows, nd + 1, restart, res, nullptr, err, err_cap)) != 0) return rc;
            if (done + nd + 1 == n_steps && res[0] == nd && logits_last) {      // (all accepted: row nd is the call's last position)
                HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
                HIP_TRY(hipMemcpy(logits_last, last->logits + (size_t) nd * V, (size_t) V * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
            }
        }
        run.accept(0, nd, res + 1, nullptr, res[0] + 1);
    }
    // the result is the device's log, checked against what the host saw step by step
    const std::vector<int32_t> &hist = run.hist[0];
    const int done = run.done[0];
    std::vector<int32_t> h(64 + (size_t) n_steps);
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipStreamSynchronize(last->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipMemcpy(h.data(), last->d_verify, h.size() * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    if (done != n_steps || h[0] != n_past + n_steps || h[1] != n_steps || memcmp(h.data() + 64, hist.data() + n_past + 1, (size_t) n_steps * 4) != 0) {
        set_err(err, err_cap, "%s: the device log holds %d tokens up to position %d, the host counted %d of %d up to %d", fn, h[1], h[0], done, n_steps, n_past + n_steps);
        return LLAMAHIP_ERR_PREDICT;
    }
    memcpy(out_tokens, h.data() + 64, (size_t) n_steps * 4);
    if (stats) *stats = run.ls[0];
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Drafted SAMPLED decoding: llamahip_verify_sample / llamahip_decode_sample_lookup.  The reference's sampler is a deterministic function of
// the row's logits, the last_n_tokens window and the mt19937 state; row j of a verify step holds the logits of the single-token eval at
// n_past + j, and IF draft tokens 0 .. j - 1 were accepted the window at row j is the current one shifted by j with those tokens pushed --
// known before the eval.  So the device selects every row's candidates under that window (launch_topk_slide on the last stage's stream,
// in place of k_verify_rows / k_accept_drafts) and the host walks the rows with the real sampler: row 0, then row j + 1 only if row j's
// draw was draft[j].  Exactly the rng draws and accepts of the token-by-token loop; only the number of weight passes changes.
// ------------------------------------------------------------------------------------------------
// the sampling parameters' own rule (llamahip_sched_new checks them before any request brings a sampler)
static int check_sampling_rule(const char *fn, double repeat_penalty, int32_t top_k, double top_p, double temp, char *err, size_t err_cap) {
    if (top_k < 1) { set_err(err, err_cap, "%s: top_k must be >= 1 (got %d)", fn, top_k); return LLAMAHIP_ERR_PREDICT; }
    if (!(temp > 0.0)) { set_err(err, err_cap, "%s: temp must be > 0 (got %g)", fn, temp); return LLAMAHIP_ERR_PREDICT; }
    if (!(repeat_penalty > 0.0)) { set_err(err, err_cap, "%s: repeat_penalty must be > 0 (got %g)", fn, repeat_penalty); return LLAMAHIP_ERR_PREDICT; }
    if (top_p != top_p) { set_err(err, err_cap, "%s: top_p is NaN", fn); return LLAMAHIP_ERR_PREDICT; }
    return 0;
}
static int check_sampler_params(const char *fn, const llamahip_sampler *sampler, double repeat_penalty, int32_t top_k, double top_p, double temp, char *err, size_t err_cap) {
    if (!sampler) { set_err(err, err_cap, "%s: null sampler", fn); return LLAMAHIP_ERR_PREDICT; }
    return check_sampling_rule(fn, repeat_penalty, top_k, top_p, temp, err, err_cap);
}
// the sampling parameters of a call and what every sampled entry point derives from them.  dev_sel: the device can make a row's candidates
// (not with top_k > 64 or n_vocab > 32768; a window of more than 1024 ids rules it out for that sampler's rows only, checked where the window is known)
struct SampleParams { double repeat_penalty; int32_t top_k; double top_p, temp; int k; double scale; bool dev_sel; };
static SampleParams sample_params(const llamahip_model *m, double repeat_penalty, int32_t top_k, double top_p, double temp) {
    const int V = m->hp.n_vocab, k = std::min(std::max(top_k, 1), V);
    return { repeat_penalty, top_k, top_p, temp, k, 1.0 / temp, V <= 32768 && k <= 64 };
}
// one draw: from the row's candidates where the device made them exactly (ex), else by the whole sampler on the row's logits; accepted at once
static int32_t sample_draw(llamahip_model *m, llamahip_sampler *sampler, const SampleParams &sp, bool ex, const double *sc, const int32_t *ids, const float *logits, int32_t *exact) {
    const int32_t tok = ex ? llamahip_sample_from_candidates(sampler, sc, ids, sp.k, sp.top_p)
                           : llamahip_sample_top_p_top_k(m, sampler, logits, sp.repeat_penalty, sp.top_k, sp.top_p, sp.temp);
    llamahip_sampler_accept(sampler, tok);
    if (exact) *exact = ex ? 1 : 0;
    return tok;
}
// handles whose verify step is a loop of single steps: f16 / f32 / Q4_1 files (no per-row key split in one pass) and LLAMAHIP_FLAG_UNFUSED
static bool sample_lookup_by_rows(llamahip_model *m) { return first_of(m)->dense || (first_of(m)->flags & LLAMAHIP_FLAG_UNFUSED) != 0; }
// the documented single step: llamahip_eval_topk -> draw -> accept; *exact as llamahip_eval_topk reports it
static int sample_single_step(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t token, llamahip_sampler *sampler, const SampleParams &sp,
                              std::vector<int32_t> &win, std::vector<float> &logits, int32_t *pick, int32_t *exact, char *err, size_t err_cap) {
    win.resize((size_t) std::max(llamahip_sampler_window(sampler, nullptr, 0), 1));
    const int32_t nw = std::min(llamahip_sampler_window(sampler, win.data(), (int32_t) win.size()), (int32_t) win.size());
    logits.resize((size_t) m->hp.n_vocab);
    double sc[64];
    int32_t ids[64], ex = 0;
    int rc = llamahip_eval_topk(m, n_threads, n_past, &token, 1, win.data(), nw, sp.repeat_penalty, sp.top_k, sp.temp, sc, ids, &ex, logits.data(), err, err_cap);
    if (rc) return rc;
    *pick = sample_draw(m, sampler, sp, ex == 1, sc, ids, logits.data(), exact);
    return 0;
}
// the walk behind a sampled verify step: the draft's rows are rows r0 .. r0 + n_draft of the step (out, last->logits); row 0, then row j + 1 only if
// row j's draw was draft[j].  sel: the device made candidates for these rows.  picks / exact: the rows reached (the caller set the rest to -1)
static int sample_walk(llamahip_model *m, llamahip_model *last, int r0, const int32_t *draft, int n_draft, llamahip_sampler *sampler, bool sel, const TopkOut *out,
                       const SampleParams &sp, int32_t *n_accept, int32_t *picks, int32_t *exact, std::vector<float> &logits, char *err, size_t err_cap) {
    const size_t V = m->hp.n_vocab;
    int a = 0;
    for (;; a++) {
        const TopkOut &c = out[r0 + a];
        const bool ex = sel && c.fl[0] == 1;
        if (!ex) {
            // (the rows stay on the device until the next eval: a row the walk reaches and finds inexact is fetched now, that row only)
            logits.resize(V);
            HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(hipMemcpy(logits.data(), last->logits + (size_t) (r0 + a) * V, V * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
        }
        picks[a] = sample_draw(m, sampler, sp, ex, c.sc, c.id, logits.data(), exact ? &exact[a] : nullptr);
        if (a == n_draft || picks[a] != draft[a]) break;
    }
    *n_accept = a;
    return 0;
}

static int verify_sample_impl(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t token, const int32_t *draft, int32_t n_draft, llamahip_sampler *sampler,
                              const SampleParams &sp, int32_t *n_accept, int32_t *picks, int32_t *exact, std::vector<int32_t> &win, std::vector<float> &logits,
                              char *err, size_t err_cap) {
    const int N = n_draft + 1;
    for (int j = 0; j < N; j++) { picks[j] = -1; if (exact) exact[j] = -1; }
    int rc;
    if (N == 1 || sample_lookup_by_rows(m)) {
        // one plain step -- and the handles without a one-pass verify eval: the rows one llamahip_eval_topk step at a time, stopping behind
        // the first draw the draft does not continue with
        int a = 0;
        int32_t tok = token, ex = 0;
        for (;; a++) {
            if ((rc = sample_single_step(m, n_threads, n_past + a, tok, sampler, sp, win, logits, &picks[a], &ex, err, err_cap)) != 0) return rc;
            if (exact) exact[a] = ex;
            if (a == n_draft || picks[a] != draft[a]) break;
            tok = draft[a];
        }
        *n_accept = a;
        return LLAMAHIP_OK;
    }
    // the id stream: the sampler's window, then the draft (the last draft token is in no row's window)
    const int32_t nw = llamahip_sampler_window(sampler, nullptr, 0);
    const bool dev_sel = sp.dev_sel && nw <= 1024;
    int32_t ids[1024 + VERIFY_ROWS_MAX], rows[VERIFY_ROWS_MAX];
    TopkOut out[VERIFY_ROWS_MAX];
    if (dev_sel) {
        (void) llamahip_sampler_window(sampler, ids, nw);
        for (int i = 0; i + 1 < N; i++) ids[nw + i] = draft[i];
    }
    rows[0] = token;
    for (int i = 0; i < n_draft; i++) rows[1 + i] = draft[i];
    const SlideReq sl = { ids, nw, sp.scale, sp.repeat_penalty, dev_sel ? sp.k : 0, out };
    if ((rc = verify_step(m, n_threads, n_past, rows, N, -1, nullptr, nullptr, err, err_cap, &sl)) != 0) return rc;
    return sample_walk(m, last_of(m), 0, draft, n_draft, sampler, dev_sel, out, sp, n_accept, picks, exact, logits, err, err_cap);
}

int llamahip_verify_sample(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t token, const int32_t *draft, int32_t n_draft,
                           llamahip_sampler *sampler, double repeat_penalty, int32_t top_k, double top_p, double temp,
                           int32_t *n_accept, int32_t *picks, int32_t *exact, char *err, size_t err_cap) {
    static const char *fn = "llamahip_verify_sample";
    int rc = check_sampler_params(fn, sampler, repeat_penalty, top_k, top_p, temp, err, err_cap);
    if (rc) return rc;
    if (!n_accept || !picks) { set_err(err, err_cap, "%s: null output", fn); return LLAMAHIP_ERR_PREDICT; }
    if ((rc = check_verify_args(m, n_past, token, draft, n_draft, fn, err, err_cap)) != 0) return rc;
    std::vector<int32_t> win;
    std::vector<float> logits;
    return verify_sample_impl(m, n_threads, n_past, token, draft, n_draft, sampler, sample_params(m, repeat_penalty, top_k, top_p, temp), n_accept, picks, exact, win, logits, err, err_cap);
}

int llamahip_decode_sample_lookup(llamahip_model *m, int32_t n_threads, int32_t n_past, int32_t first_token, int32_t n_steps,
                                  const int32_t *context, int32_t n_context, const int32_t *corpus, int32_t n_corpus,
                                  int32_t draft_len, int32_t ngram_min, int32_t ngram_max, llamahip_sampler *sampler,
                                  double repeat_penalty, int32_t top_k, double top_p, double temp,
                                  int32_t *out_tokens, int32_t *out_exact, llamahip_lookup_stats *stats, char *err, size_t err_cap) {
    static const char *fn = "llamahip_decode_sample_lookup";
    int rc = check_sampler_params(fn, sampler, repeat_penalty, top_k, top_p, temp, err, err_cap);
    if (rc) return rc;
    if ((rc = check_lookup_args(m, fn, n_past, first_token, n_steps, context, n_context, corpus, n_corpus, draft_len, ngram_min, ngram_max, out_tokens, stats, err, err_cap)) != 0) return rc;
    const SampleParams sp = sample_params(m, repeat_penalty, top_k, top_p, temp);
    // nothing is drafted where a verify step would stream the weights once per row anyway, or where every row would come back whole
    const bool drafts = !sample_lookup_by_rows(m) && sp.dev_sel && llamahip_sampler_window(sampler, nullptr, 0) <= 1024;
    LookupRun run;
    if ((rc = run.open(fn, m->hp.n_ctx, 1, &n_past, n_steps, err, err_cap)) != 0) return rc;
    run.start(&first_token, context, corpus, n_corpus, draft_len, ngram_min, ngram_max);
    run.out_tokens = out_tokens; run.out_exact = out_exact;
    const std::vector<int32_t> act{ 0 };
    std::vector<int32_t> win;
    std::vector<float> logits;
    while (run.done[0] < n_steps) {
        int32_t nd = 0, n_acc = 0, picks[VERIFY_ROWS_MAX], exact[VERIFY_ROWS_MAX];
        if ((rc = run.draft_round(act, [&](int) { return drafts; }, &nd, err, err_cap)) != 0) return rc;
        if (nd == 0) rc = sample_single_step(m, n_threads, run.pos(0), run.token(0), sampler, sp, win, logits, &picks[0], &exact[0], err, err_cap);
        else rc = verify_sample_impl(m, n_threads, run.pos(0), run.token(0), run.draft[0], nd, sampler, sp, &n_acc, picks, exact, win, logits, err, err_cap);
        if (rc) return rc;
        run.accept(0, nd, picks, exact, n_acc + 1);
    }
    if (stats) *stats = run.ls[0];
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// llamahip_decode_greedy_multi: n_seqs independent greedy streams at once -- the micro-batched schedule of the layer pipeline (SURVEY.md 8e:
// "throughput scales only with independent sequences in flight"), native, behind the C ABI.  The slots are cut into G >= n_stages groups of
// consecutive slots (group_cut); a stage steps a group as ONE set (llamahip_stage_step_set: its weights streamed once for the group) and hands
// the group's residual rows to the next stage with one stream-ordered copy + event while it goes on with the next group (step_group) -- so in
// steady state every stage (every GPU of a pipeline handle) works on a different group; the last stage's picks go back to the first stage's
// token words the same way.  Host order (step, group, stage): every wait refers to an event recorded by work enqueued before it, so nothing
// here blocks but the first capture of a set's graph.  A plain handle is the one-stage case: its groups are stepped one after the other, no copies.
// ------------------------------------------------------------------------------------------------
// g0[0 .. G]: groups of consecutive slots, at least one per stage (so that every stage has a group to work on), at most SET_MAX slots each
static std::vector<int> group_cut(int n_seqs, int n_stages) {
    const int G = std::min(n_seqs, std::max(n_stages, (n_seqs + SET_MAX - 1) / SET_MAX));
    std::vector<int> g0(G + 1, 0);
    for (int g = 0; g < G; g++) g0[g + 1] = g0[g] + n_seqs / G + (g < n_seqs % G ? 1 : 0);
    return g0;
}

// the multi-sequence loops have a stage step to batch: not Q4_1 files, f16 / f32 pipeline stages or LLAMAHIP_FLAG_UNFUSED handles
static bool multi_stage_steps(const llamahip_model *first) { return !(first->dense && !dense_stage_steps(first)) && !(first->flags & LLAMAHIP_FLAG_UNFUSED); }

static int multi_prepare(llamahip_model *st, int n_groups, char *err, size_t err_cap) {
    HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_PREDICT);
    const size_t d = st->hp.n_embd;
    if (!st->mq_tok)
        HIP_TRY(st->own.alloc_all({ { &st->mq_tok, (size_t) st->n_seq * 4 + 64, true }, { &st->mq_in, (size_t) st->n_seq * d * 4 },
                                    { &st->mq_out, (size_t) st->n_seq * d * 4 } }), LLAMAHIP_ERR_PREDICT);
    while ((int) st->mq_ev.size() < n_groups) {
        hipEvent_t e = nullptr;
        HIP_TRY(st->mq_ev.create(&e, hipEventDisableTiming), LLAMAHIP_ERR_PREDICT);
    }
    return 0;
}

// the pinned block of the sampled decoders: token words, windows, candidates and spill rows, mapped into the device
static int sample_prepare(llamahip_model *st, bool last, char *err, size_t err_cap) {
    if (st->smp_blk) return 0;
    HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_PREDICT);
    const size_t n = st->n_seq, V = last ? st->hp.n_vocab : 0;
    const size_t o_last = (n * 4 + 63) / 64 * 64, o_win = o_last + (n * 4 + 63) / 64 * 64, o_out = o_win + n * 1024 * 4;
    const size_t o_spill = o_out + (last ? n * sizeof(TopkOut) : 0), bytes = o_spill + n * V * 4;
    // the block, (last stage) the selection workspace and the block's device alias: all or none
    const size_t ws_bytes = (size_t) SET_MAX * TOPK_WS_BYTES;
    hipError_t e = (hipError_t) (last ? st->own.alloc_all({ { &st->smp_blk, bytes, true, MEM_PINNED }, { &st->smp_ws, ws_bytes, true } })
                                      : st->own.alloc_all({ { &st->smp_blk, bytes, true, MEM_PINNED } }));
    char *d = nullptr;
    if (e == hipSuccess && (e = hipHostGetDevicePointer((void **) &d, st->smp_blk, 0)) != hipSuccess) { st->own.release(&st->smp_blk); st->own.release(&st->smp_ws); }
    HIP_TRY(e, LLAMAHIP_ERR_PREDICT);
    for (int v = 0; v < 2; v++) {
        char *b = v ? d : st->smp_blk;
        llamahip_model::SampleIo &io = v ? st->smp_d : st->smp_h;
        io.tok = (int32_t *) b; io.n_last = (int32_t *) (b + o_last); io.win = (int32_t *) (b + o_win);
        io.out = last ? (TopkOut *) (b + o_out) : nullptr; io.spill = last ? (float *) (b + o_spill) : nullptr;
    }
    return 0;
}

// The start of every multi-sequence loop: the stages' queues, and sequence i bound to slot i of every stage at n_past[i].
// first_tokens != nullptr, the greedy loops: the token words are the first stage's mq_tok, fed by the last stage's pick (one stage: the pick goes
// straight back into the slot's token word, as the whole-model stage step allows).  nullptr, the sampled loops: the token words lie in the first
// stage's pinned block and the host writes its draws there (token_out NULL: the argmax of the stage step still advances the slot's position).
static int multi_begin(const std::vector<llamahip_model *> &stages, int n_groups, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens, char *err, size_t err_cap) {
    const int S = (int) stages.size();
    llamahip_model *first = stages[0], *last = stages[S - 1];
    const size_t d = first->hp.n_embd;
    int rc;
    for (llamahip_model *st : stages) if ((rc = multi_prepare(st, n_groups, err, err_cap)) != 0) return rc;
    if (first_tokens) {
        HIP_TRY(hipSetDevice(first->device), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipMemcpy(first->mq_tok, first_tokens, (size_t) n_seqs * 4, hipMemcpyHostToDevice), LLAMAHIP_ERR_PREDICT);
    } else {
        if ((rc = sample_prepare(last, true, err, err_cap)) != 0) return rc;
        if (first != last && (rc = sample_prepare(first, false, err, err_cap)) != 0) return rc;
    }
    int32_t *tok_in = first_tokens ? first->mq_tok : first->smp_d.tok, *tok_out = first_tokens ? last->mq_tok : nullptr;
    for (int s = 0; s < S; s++) {
        llamahip_model *st = stages[s];
        for (int i = 0; i < n_seqs; i++)
            if ((rc = llamahip_stage_bind(st, i, n_past[i], s == 0 ? tok_in + i : nullptr, s ? st->mq_in + (size_t) i * d : nullptr,
                                          s + 1 < S ? st->mq_out + (size_t) i * d : nullptr, s + 1 == S && tok_out ? tok_out + i : nullptr, err, err_cap)) != 0) return rc;
    }
    return 0;
}

// One group of bound slots stepped through every stage.  Stage s waits for stage s - 1's event `ev`, steps the n slots -- as ONE set where it
// takes sets of n, else slot by slot -- and hands the residual rows of slots [c0, c0 + cn) to stage s + 1 with one stream-ordered copy.  On the
// last stage `hook` (if any) runs on the stream behind each step -- hook(j, R): rows [0, R) of the logits are the group's slots j .. j + R - 1 (a
// set orders its rows by slot id; a single step leaves row 0, taken before the next slot's step rewrites it) -- and with copy_picks, on a
// pipeline, the token words of slots [c0, c0 + cn) go back to the first stage, which with wait_picks waits for that copy of the step before.
// A stage records its event `ev` behind whatever it enqueued after its step.  The host waits for nothing here, and an error comes back as the
// return code with work enqueued: every caller drains the stages (drain_stages) before it returns.
struct SlotGroup { const int32_t *slots; int n, c0, cn, ev; };
static int step_group(const std::vector<llamahip_model *> &stages, const SlotGroup &g, int32_t n_threads, bool wait_picks, bool copy_picks,
                      const std::function<int(int, int)> &hook, char *err, size_t err_cap) {
    const int S = (int) stages.size();
    llamahip_model *first = stages[0], *last = stages[S - 1];
    const size_t d = first->hp.n_embd;
    for (int s = 0; s < S; s++) {
        llamahip_model *st = stages[s], *to = s + 1 < S ? stages[s + 1] : first;
        const bool tail = s + 1 == S;
        int rc;
        HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_PREDICT);
        if (s > 0) HIP_TRY(hipStreamWaitEvent(st->stream, stages[s - 1]->mq_ev[g.ev], 0), LLAMAHIP_ERR_PREDICT);
        else if (wait_picks) HIP_TRY(hipStreamWaitEvent(st->stream, last->mq_ev[g.ev], 0), LLAMAHIP_ERR_PREDICT);
        if (g.n >= 2 && llamahip_stage_set_applies(st, g.n, n_threads)) {
            if ((rc = llamahip_stage_step_set(st, g.slots, g.n, n_threads, st->stream, err, err_cap)) != 0) return rc;
            if (tail && hook && (rc = hook(0, g.n)) != 0) return rc;
        } else for (int j = 0; j < g.n; j++) {
            if ((rc = llamahip_stage_step(st, g.slots[j], n_threads, st->stream, err, err_cap)) != 0) return rc;
            if (tail && hook && (rc = hook(j, 1)) != 0) return rc;
        }
        const bool picks = tail && copy_picks && S > 1;
        if (!tail || picks) {
            void *dst = tail ? (void *) (first->mq_tok + g.c0) : (void *) (to->mq_in + (size_t) g.c0 * d);
            const void *src = tail ? (const void *) (last->mq_tok + g.c0) : (const void *) (st->mq_out + (size_t) g.c0 * d);
            const size_t bytes = tail ? (size_t) g.cn * 4 : (size_t) g.cn * d * 4;
            if (st->device == to->device) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st->stream), LLAMAHIP_ERR_PREDICT);
            else HIP_TRY(hipMemcpyPeerAsync(dst, to->device, src, st->device, bytes, st->stream), LLAMAHIP_ERR_PREDICT);
        }
        if (!tail || picks || hook) HIP_TRY(hipEventRecord(st->mq_ev[g.ev], st->stream), LLAMAHIP_ERR_PREDICT);
    }
    return 0;
}

int llamahip_decode_greedy_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens, int32_t n_steps,
                                 int32_t *out_tokens, char *err, size_t err_cap) {
    if (!m) { set_err(err, err_cap, "null model"); return LLAMAHIP_ERR_PREDICT; }
    const std::vector<llamahip_model *> stages = stages_of(m);
    const int S = (int) stages.size();
    llamahip_model *first = stages[0], *last = stages[S - 1];
    if (first->host_only) { set_err(err, err_cap, "model was loaded with LLAMAHIP_FLAG_HOST_ONLY: no device state, cannot evaluate"); return LLAMAHIP_ERR_PREDICT; }
    if (!first->first_stage || !last->last_stage) { set_err(err, err_cap, "llamahip_decode_greedy_multi needs a whole-model or a pipeline handle"); return LLAMAHIP_ERR_PREDICT; }
    if (!n_past || !first_tokens || !out_tokens || n_seqs < 1 || n_steps < 1) { set_err(err, err_cap, "llamahip_decode_greedy_multi: bad arguments"); return LLAMAHIP_ERR_PREDICT; }
    if (n_seqs > first->n_seq) { set_err(err, err_cap, "llamahip_decode_greedy_multi: %d sequences on a handle with %d KV slots (llamahip_opts.n_seq)", n_seqs, first->n_seq); return LLAMAHIP_ERR_PREDICT; }
    int rc = 0;
    for (int i = 0; i < n_seqs; i++) {
        if ((rc = check_eval_args(first, n_past[i], first_tokens + i, 1, true, err, err_cap)) != 0) return rc;
        if (n_past[i] + n_steps > m->hp.n_ctx) { set_err(err, err_cap, "context overflow: n_past (%d) + n_steps (%d) > n_ctx (%d)", n_past[i], n_steps, m->hp.n_ctx); return LLAMAHIP_ERR_PREDICT; }
    }
    if (!multi_stage_steps(first))
        // no stage step to batch (Q4_1 files, f16 / f32 pipeline stages, LLAMAHIP_FLAG_UNFUSED): llamahip_decode_greedy on each slot in turn
        return each_slot(m, n_seqs, nullptr, err, err_cap, [&](int i) {
            return llamahip_decode_greedy(m, n_threads, n_past[i], first_tokens[i], n_steps, out_tokens + (size_t) i * n_steps, nullptr, err, err_cap); });
    const double t0 = now_ms();
    const std::vector<int> g0 = group_cut(n_seqs, S);
    const int G = (int) g0.size() - 1;
    if ((rc = multi_begin(stages, G, n_seqs, n_past, first_tokens, err, err_cap)) != 0) return rc;
    std::vector<int32_t> slots(n_seqs);
    for (int i = 0; i < n_seqs; i++) slots[i] = i;
    // (nobody waits for the last step's picks: the trace holds them)
    for (int t = 0; t < n_steps && rc == 0; t++)
        for (int g = 0; g < G && rc == 0; g++)
            rc = step_group(stages, { slots.data() + g0[g], g0[g + 1] - g0[g], g0[g], g0[g + 1] - g0[g], g }, n_threads, S > 1 && t > 0, t + 1 < n_steps, nullptr, err, err_cap);
    if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
    for (int i = 0; i < n_seqs; i++) {
        int32_t pos = 0;
        const int n = llamahip_stage_trace(last, i, &pos, out_tokens + (size_t) i * n_steps, n_steps, err, err_cap);
        if (n < 0) return n;
        if (n != n_steps || pos != n_past[i] + n_steps) { set_err(err, err_cap, "multi-sequence decode: sequence %d recorded %d of %d steps, position %d", i, n, n_steps, pos); return LLAMAHIP_ERR_PREDICT; }
    }
    m->n_evals += (int64_t) n_seqs * n_steps;
    m->t_eval_ms += now_ms() - t0;
    if (!m->stages.empty()) m->pipe_hand_off = 1;
    return LLAMAHIP_OK;
}

// Constrained greedy decoding for several sequences at once (llamahip.h): llamahip_decode_greedy_multi's loop -- sequence i
// bound to slot i, one set step per token for all of them, the captured set step exactly as it is -- with ONE k_pick_dfa launch over the
// step's rows behind it (step_group's hook).  That launch re-picks from the step's logits under each row's own table and state word and
// overwrites what the step's tail wrote: the trace entry at step - 1 and the slot's next-token word; the position stays as the tail advanced
// it.  A finished sequence stays in the set in DONE (its picks are stop tokens).  The host reads the {state, dead} words once per leg.
int llamahip_decode_greedy_constrained_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens,
                                             int32_t n_steps, llamahip_constraint *const *constraints, int32_t *states_io, int32_t *out_tokens,
                                             int32_t *n_out, int32_t *finished, char *err, size_t err_cap) {
    static const char *fn = "llamahip_decode_greedy_constrained_multi";
    if (!m || !n_past || !first_tokens || !constraints || !states_io || !out_tokens || !n_out || !finished) {
        set_err(err, err_cap, "%s: %s is NULL", fn, !m ? "model" : !n_past ? "n_past" : !first_tokens ? "first_tokens" : !constraints ? "constraints" : !states_io ? "states_io"
                : !out_tokens ? "out_tokens" : !n_out ? "n_out" : "finished");
        return LLAMAHIP_ERR_PREDICT;
    }
    if (n_seqs < 1 || n_seqs > SET_MAX) { set_err(err, err_cap, "%s: n_seqs %d outside 1 .. %d", fn, n_seqs, SET_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (n_steps < 1) { set_err(err, err_cap, "%s: n_steps must be >= 1 (got %d)", fn, n_steps); return LLAMAHIP_ERR_PREDICT; }
    const int V = m->hp.n_vocab;
    for (int i = 0; i < n_seqs; i++) {
        const llamahip_constraint *c = constraints[i];
        if (!c) { set_err(err, err_cap, "%s: constraints[%d] is NULL", fn, i); return LLAMAHIP_ERR_PREDICT; }
        if (c->m != m) { set_err(err, err_cap, "%s: constraints[%d] was made on another handle", fn, i); return LLAMAHIP_ERR_PREDICT; }
        if (states_io[i] < 0 || states_io[i] >= c->n_states) { set_err(err, err_cap, "%s: states_io[%d] = %d out of range [0, %d)", fn, i, states_io[i], c->n_states); return LLAMAHIP_ERR_PREDICT; }
        if (first_tokens[i] < 0 || first_tokens[i] >= V) { set_err(err, err_cap, "%s: token id %d out of range [0, %d)", fn, first_tokens[i], V); return LLAMAHIP_ERR_PREDICT; }
        if (n_past[i] < 0 || (int64_t) n_past[i] + n_steps > m->hp.n_ctx) {
            set_err(err, err_cap, "%s: context overflow: n_past (%d) + n_steps (%d) > n_ctx (%d)", fn, n_past[i], n_steps, m->hp.n_ctx);
            return LLAMAHIP_ERR_PREDICT;
        }
    }
    const std::vector<llamahip_model *> stages = stages_of(m);
    llamahip_model *first = stages[0], *last = stages.back();
    if (n_seqs > first->n_seq) { set_err(err, err_cap, "%s: %d sequences on a handle with %d KV slots (llamahip_opts.n_seq)", fn, n_seqs, first->n_seq); return LLAMAHIP_ERR_PREDICT; }
    if (first->host_only) { set_err(err, err_cap, "%s: model was loaded with LLAMAHIP_FLAG_HOST_ONLY: no device state, cannot evaluate", fn); return LLAMAHIP_ERR_PREDICT; }
    if (!first->first_stage || !last->last_stage) { set_err(err, err_cap, "%s: needs a whole-model or a pipeline handle", fn); return LLAMAHIP_ERR_PREDICT; }
    if (stages.size() > 1 || !multi_stage_steps(first))
        // pipeline handles, and handles with no stage step to batch (Q4_1 files, LLAMAHIP_FLAG_UNFUSED): the single-sequence call on each slot in turn
        return each_slot(m, n_seqs, nullptr, err, err_cap, [&](int i) {
            return llamahip_decode_greedy_constrained(m, n_threads, n_past[i], first_tokens[i], n_steps, constraints[i], states_io + i,
                                                      out_tokens + (size_t) i * n_steps, n_out + i, finished + i, nullptr, err, err_cap); });
    const double t0 = now_ms();
    int rc = 0;
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    for (int i = 0; i < n_seqs; i++) if ((rc = cst_ensure_dev(m, constraints[i], err, err_cap)) != 0) return rc;
    if ((rc = multi_begin(stages, 1, n_seqs, n_past, first_tokens, err, err_cap)) != 0) return rc;
    int32_t hc[2 * SET_MAX];
    for (int i = 0; i < n_seqs; i++) { hc[2 * i] = states_io[i]; hc[2 * i + 1] = 0; }
    HIP_TRY(hipMemcpy(m->d_cst, hc, (size_t) n_seqs * 8, hipMemcpyHostToDevice), LLAMAHIP_ERR_PREDICT);
    std::vector<int32_t> slots(n_seqs);
    for (int i = 0; i < n_seqs; i++) slots[i] = i;
    // rows [0, R) of the step's logits are slots j .. j + R - 1 (a set orders its rows by slot id; a single step leaves row 0)
    const std::function<int(int, int)> repick = [&](int j, int R) -> int {
        DfaRows rows = {};
        for (int r = 0; r < R; r++) {
            const int i = j + r;
            const llamahip_constraint *c = constraints[i];
            rows.r[r] = { m->logits + (size_t) r * V, c->dev, m->d_cst + 2 * i, m->d_slot_trace + (size_t) i * m->hp.n_ctx, m->mq_tok + i, m->d_slot_state + 2 * i,
                          c->n_states, c->stop_token, 0, 1 };
        }
        HIP_TRY(launch_pick_dfa(rows, R, V, m->stream), LLAMAHIP_ERR_PREDICT);
        return 0;
    };
    static const int leg_env = getenv("LLAMAHIP_CONSTRAIN_LEG") ? atoi(getenv("LLAMAHIP_CONSTRAIN_LEG")) : 0;
    const int32_t leg_steps = leg_env >= 1 && leg_env <= 64 ? leg_env : LLAMAHIP_CONSTRAIN_LEG;
    int32_t ran = 0;
    bool all_done = false;
    while (ran < n_steps && !all_done && rc == 0) {
        const int32_t leg = std::min<int32_t>(leg_steps, n_steps - ran);
        for (int32_t t = 0; t < leg && rc == 0; t++) rc = step_group(stages, { slots.data(), n_seqs, 0, n_seqs, 0 }, n_threads, false, false, repick, err, err_cap);
        if (rc) break;
        ran += leg;
        HIP_TRY(hipMemcpyAsync(hc, m->d_cst, (size_t) n_seqs * 8, hipMemcpyDeviceToHost, m->stream), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
        if ((rc = check_sync_timeout(m, err, err_cap)) != 0) break;
        all_done = true;
        for (int i = 0; i < n_seqs; i++) {
            if (hc[2 * i + 1] != 0 || hc[2 * i] < 0 || hc[2 * i] >= constraints[i]->n_states) {
                set_err(err, err_cap, "%s: a pick of sequence %d found no allowed token (state word %d, dead %d): the state does not come from its constraint", fn, i, hc[2 * i], hc[2 * i + 1]);
                rc = LLAMAHIP_ERR_PREDICT;
                break;
            }
            all_done = all_done && hc[2 * i] == constraints[i]->n_states - 1;
        }
    }
    if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
    for (int i = 0; i < n_seqs; i++) {
        int32_t pos = 0, *out = out_tokens + (size_t) i * n_steps;
        const int n = llamahip_stage_trace(last, i, &pos, out, ran, err, err_cap);
        if (n < 0) return n;
        if (n != ran || pos != n_past[i] + ran) { set_err(err, err_cap, "%s: sequence %d recorded %d of %d steps, position %d", fn, i, n, ran, pos); return LLAMAHIP_ERR_PREDICT; }
        const llamahip_constraint *c = constraints[i];
        const int32_t fin = hc[2 * i] == c->n_states - 1;
        int32_t k = ran;
        if (fin) { for (k = 0; k < ran && out[k] != c->stop_token; k++) {} k = std::min(k + 1, ran); }
        states_io[i] = hc[2 * i]; n_out[i] = k; finished[i] = fin;
    }
    m->n_evals += (int64_t) n_seqs * ran;
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}

// llamahip_eval_topk under a constraint (llamahip.h): the eval, k_mask_rows_dfa from the logits row into a scratch row, the candidate
// selection of llamahip_eval_topk on that row.  Where llamahip_eval_topk falls back to the logits row (pipeline handles, sizes the selection
// does not take) the row is masked on the host: *exact = 0, logits_out = the masked row.
int llamahip_eval_topk_constrained(llamahip_model *m, int32_t n_threads, int32_t n_past, const int32_t *tokens, int32_t n_tokens,
                                   const int32_t *last_n_tokens, int32_t n_last, double repeat_penalty, int32_t top_k, double temp,
                                   llamahip_constraint *c, int32_t state, double *cand_scores, int32_t *cand_ids, int32_t *exact, float *logits_out,
                                   char *err, size_t err_cap) {
    static const char *fn = "llamahip_eval_topk_constrained";
    if (!m || !c || !cand_scores || !cand_ids || !exact || !logits_out) { set_err(err, err_cap, "%s: null argument", fn); return LLAMAHIP_ERR_PREDICT; }
    if (c->m != m) { set_err(err, err_cap, "%s: the constraint was made on another handle", fn); return LLAMAHIP_ERR_PREDICT; }
    if (state < 0 || state >= c->n_states) { set_err(err, err_cap, "%s: state %d out of range [0, %d)", fn, state, c->n_states); return LLAMAHIP_ERR_PREDICT; }
    *exact = 0;
    const int V = m->hp.n_vocab;
    const int k = std::min(std::max(top_k, 1), V);
    const bool device_ok = m->stages.empty() && !m->host_only && V <= 32768 && k <= 64 && n_last >= 0 && n_last <= 1024 && (n_last == 0 || last_n_tokens);
    if (!device_ok) {
        const int rc = llamahip_eval(m, n_threads, n_past, tokens, n_tokens, logits_out, err, err_cap);
        if (rc) return rc;
        return llamahip_constraint_mask_row(c, state, logits_out, logits_out);
    }
    const double t0 = now_ms();
    int rc = eval_impl(m, n_threads, n_past, tokens, n_tokens, nullptr, nullptr, -1, nullptr, 0, nullptr, false, err, err_cap);   // logits stay on the device, no wait
    if (rc) return rc;
    if ((rc = cst_ensure_dev(m, c, err, err_cap)) != 0) return rc;
    if (!m->d_cst_row) HIP_TRY(m->own.alloc(&m->d_cst_row, (size_t) V), LLAMAHIP_ERR_PREDICT);
    if (!m->d_topk) HIP_TRY(m->own.alloc(&m->d_topk, 8192 + TOPK_WS_BYTES, true), LLAMAHIP_ERR_PREDICT);
    int32_t *d_win = (int32_t *) m->d_topk;
    double *d_sc = (double *) ((char *) m->d_topk + 4096);
    int32_t *d_id = (int32_t *) ((char *) m->d_topk + 4096 + 512), *d_fl = d_id + 64;
    const bool mapped = m->h_io != nullptr;
    if (mapped) {
        if (n_last > 0) memcpy(m->h_io->window, last_n_tokens, (size_t) n_last * 4);
        d_win = m->d_io->window; d_sc = m->d_io->sc; d_id = m->d_io->id; d_fl = m->d_io->fl;
    } else if (n_last > 0) HIP_TRY(hipMemcpyAsync(d_win, last_n_tokens, (size_t) n_last * 4, hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
    DfaMaskRows mr = {};
    mr.row[0] = c->dev + (size_t) state * V;
    HIP_TRY(launch_mask_rows_dfa(m->logits + (size_t) (n_tokens - 1) * V, m->d_cst_row, 1, V, mr, m->stream), LLAMAHIP_ERR_PREDICT);
    const float *row = m->d_cst_row;
    HIP_TRY(launch_topk_candidates(row, V, d_win, n_last, 1.0 / temp, repeat_penalty, k, d_sc, d_id, d_fl, m->stream, (char *) m->d_topk + 8192), LLAMAHIP_ERR_PREDICT);
    struct { double sc[64]; int32_t id[64]; int32_t fl[2]; } h;
    if (!mapped) HIP_TRY(hipMemcpyAsync(&h, d_sc, sizeof(h), hipMemcpyDeviceToHost, m->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
    if (mapped) { memcpy(h.sc, m->h_io->sc, sizeof(h.sc)); memcpy(h.id, m->h_io->id, sizeof(h.id)); memcpy(h.fl, m->h_io->fl, sizeof(h.fl)); }
    if ((rc = check_sync_timeout(m, err, err_cap)) != 0) return rc;
    m->t_eval_ms += now_ms() - t0;
    if (h.fl[0] == 1) {
        for (int i = 0; i < k; i++) { cand_scores[i] = h.sc[i]; cand_ids[i] = h.id[i]; }
        *exact = 1;
        return LLAMAHIP_OK;
    }
    HIP_TRY(hipMemcpy(logits_out, row, (size_t) V * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Drafted greedy decoding for SEVERAL sequences at once: llamahip_verify_greedy_multi / llamahip_decode_greedy_lookup_multi.  A set step has 16
// rows and costs what its weight stream costs; with 2 .. 8 sequences most rows are unused, and here they carry the sequences' drafts.  The rows
// of such a step are cut into SEGMENTS, one per sequence (VsetReq): segment i = [last token of slot i, its draft ...] at positions p_i, p_i + 1,
// ...  The kernels of the set path read three things per row -- position, KV offset, token -- and nothing in them requires the rows' slots to be
// distinct: rows r .. r + j that share one kv_off and hold positions p .. p + j make row r + j the single-token eval of that slot at p + j (its
// K / V rows are appended by the launch before the score launch, as in a multi-row eval; every row runs the V*P key split of its own
// single-token eval).  So the step is forward_set on a descriptor built on the host (VsetBlock), then k_verify_rows over all rows and
// k_accept_drafts_set, one wave per segment: 4 (rows + segments) bytes come back.  Eager, like every verify step.
// (Equality with single steps is BY TEST -- tests/test_gpu_lookup_multi.py -- not structural: the norm's one-pass against two-pass statistics,
//  as for set steps and verify steps.)
// ------------------------------------------------------------------------------------------------
// every stage takes set steps of 2 .. 16 rows with this n_threads (else: the callers' per-slot fall-back)
static bool vset_applies(const std::vector<llamahip_model *> &stages, int n_threads) {
    for (const llamahip_model *st : stages)
        for (int n = 2; n <= SET_MAX; n++) if (!llamahip_stage_set_applies(st, n, n_threads)) return false;
    return true;
}

static int vset_ensure(llamahip_model *st, bool first, char *err, size_t err_cap) {
    HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_PREDICT);
    int rc = ensure_workspace(st, SET_MAX, err, err_cap);
    if (rc) return rc;
    if ((rc = ensure_set_sc(st, err, err_cap)) != 0) return rc;
    if (!st->d_vset) HIP_TRY(st->own.alloc(&st->d_vset, 1, true), LLAMAHIP_ERR_PREDICT);
    if (!first && (rc = pipe_ensure_in(st, SET_MAX, err, err_cap)) != 0) return rc;
    return 0;
}

// The sampled step's device half (llamahip_verify_sample_multi): behind forward_set, in place of k_verify_rows / k_accept_drafts_set, the
// sampler's candidate selection over the R rows, row r's window = ids[row_off[r] .. + row_n_last[r]) of the id pool (launch_topk_slide_set).
// k == 0: the device cannot make candidates for any row (top_k > 64, n_vocab > 32768) -- nothing is launched.  out: R rows, valid after the step.
struct SlideSetReq { const int32_t *ids; int n_ids; int32_t row_off[VERIFY_ROWS_MAX], row_n_last[VERIFY_ROWS_MAX]; double scale, repeat_penalty; int k; TopkOut *out; };
static int slide_set_enqueue(llamahip_model *last, const SlideSetReq &ss, int R, char *err, size_t err_cap) {
    if (ss.k == 0) return 0;
    if (ss.n_ids < 0 || (size_t) ss.n_ids > SLIDE_SET_IDS) { set_err(err, err_cap, "sampled verify step over a set: an id pool of %d ids", ss.n_ids); return LLAMAHIP_ERR_PREDICT; }
    for (int r = 0; r < R; r++)      // (every window the kernel reads lies inside the pool)
        if (ss.row_n_last[r] < 0 || ss.row_off[r] < 0 || (ss.row_n_last[r] <= 1024 && ss.row_off[r] + ss.row_n_last[r] > ss.n_ids)) {
            set_err(err, err_cap, "sampled verify step over a set: row %d's window [%d, + %d) leaves the pool of %d ids", r, ss.row_off[r], ss.row_n_last[r], ss.n_ids);
            return LLAMAHIP_ERR_PREDICT;
        }
    int rc = slide_ensure(last, err, err_cap);
    if (rc) return rc;
    const int32_t *ids, *tab;
    TopkOut *out;
    if (last->h_io) {                       // (the stream is idle: every entry point synchronises before it returns)
        memcpy(last->h_io->pool, ss.ids, (size_t) ss.n_ids * 4);
        memcpy(last->h_io->row_tab, ss.row_off, sizeof(ss.row_off));
        memcpy(last->h_io->row_tab + VERIFY_ROWS_MAX, ss.row_n_last, sizeof(ss.row_n_last));
        ids = last->d_io->pool; tab = last->d_io->row_tab; out = last->d_io->rows;
    } else {
        if (!last->d_slide_set) HIP_TRY(last->own.alloc(&last->d_slide_set, SLIDE_SET_IDS + 2 * VERIFY_ROWS_MAX), LLAMAHIP_ERR_PREDICT);
        int32_t *d_tab = last->d_slide_set + SLIDE_SET_IDS;
        // (pageable sources: each copy has left the host buffer when the call returns)
        if (ss.n_ids > 0) HIP_TRY(hipMemcpyAsync(last->d_slide_set, ss.ids, (size_t) ss.n_ids * 4, hipMemcpyHostToDevice, last->stream), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipMemcpyAsync(d_tab, ss.row_off, sizeof(ss.row_off), hipMemcpyHostToDevice, last->stream), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipMemcpyAsync(d_tab + VERIFY_ROWS_MAX, ss.row_n_last, sizeof(ss.row_n_last), hipMemcpyHostToDevice, last->stream), LLAMAHIP_ERR_PREDICT);
        ids = last->d_slide_set; tab = d_tab; out = (TopkOut *) (last->d_slide + SLIDE_WS_BYTES + SLIDE_IDS_BYTES);
    }
    HIP_TRY(launch_topk_slide_set(last->logits, R, last->hp.n_vocab, ids, tab, tab + VERIFY_ROWS_MAX, ss.scale, ss.repeat_penalty, ss.k, out, last->stream, last->d_slide), LLAMAHIP_ERR_PREDICT);
    return 0;
}

// one verify step over a set on a Q4_0 handle, plain or pipeline; res: {n_accept[n_segs], picks[n_rows]}
// (ss != nullptr: the sampled step -- res unused, ss->out receives the rows' candidates, no slot word is touched)
static int vset_step(llamahip_model *m, const std::vector<llamahip_model *> &stages, int32_t n_threads, const VsetReq &rq, int32_t *res, char *err, size_t err_cap,
                     const SlideSetReq *ss = nullptr) {
    const double t0 = now_ms();
    const int S = (int) stages.size(), R = rq.n_rows, G = rq.n_segs;
    llamahip_model *first = stages[0], *last = stages[S - 1];
    const int C = m->hp.n_ctx, V = m->hp.n_vocab;
    const size_t d = m->hp.n_embd;
    const int nth = clamp_threads(n_threads);
    int rc, max_pos = 0;
    for (int g = 0; g < G; g++) max_pos = std::max(max_pos, rq.pos[g] + rq.seg_begin[g + 1] - rq.seg_begin[g] - 1);
    if (R < 2 || R > SET_MAX || G < 1 || G > R || max_pos >= C) { set_err(err, err_cap, "verify step over a set: %d rows in %d segments up to position %d", R, G, max_pos); return LLAMAHIP_ERR_PREDICT; }
    const int set_keys = set_key_bucket(C, max_pos);            // (llamahip_stage_step_set's key bucket, exact for this step)
    for (int s = 0; s < S; s++) if ((rc = vset_ensure(stages[s], s == 0, err, err_cap)) != 0) return rc;
    auto bail = [&](int r) { (void) pipe_sync_stages(stages, nullptr, 0); return r; };
    for (int s = 0; s < S; s++) {
        llamahip_model *st = stages[s];
        HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_PREDICT);
        VsetBlock *dv = st->d_vset;
        std::vector<char> pageable;
        VsetBlock *hb = st->h_io ? &st->h_io->vset : nullptr;      // (the stream is idle: every entry point synchronises before it returns)
        if (!hb) { pageable.resize(sizeof(VsetBlock)); hb = (VsetBlock *) pageable.data(); }
        memset(hb, 0, offsetof(VsetBlock, pick));
        hb->set.n = R;
        for (int g = 0; g < G; g++) {
            hb->seg_begin[g] = rq.seg_begin[g];
            hb->seg_slot[g] = rq.slot[g];
            for (int r = rq.seg_begin[g]; r < rq.seg_begin[g + 1]; r++) {
                hb->set.state[r] = dv->state[r];
                hb->set.tok_in[r] = &dv->tok[r];
                hb->set.hid_in[r] = s ? st->pipe_in + (size_t) r * d : nullptr;
                hb->set.kv_off[r] = (long) ((size_t) rq.slot[g] * (st->l1 - st->l0) * C * d);
                hb->state[r][0] = rq.pos[g] + (r - rq.seg_begin[g]);
                hb->tok[r] = rq.rows[r];
            }
        }
        hb->seg_begin[G] = R;
        // (pinned: stream-ordered; else the synchronous copy, done before the launches below are enqueued)
        if ((st->h_io ? hipMemcpyAsync(dv, hb, offsetof(VsetBlock, pick), hipMemcpyHostToDevice, st->stream)
                      : hipMemcpy(dv, hb, offsetof(VsetBlock, pick), hipMemcpyHostToDevice)) != hipSuccess) { set_err(err, err_cap, "HIP error copying the step descriptor"); return bail(LLAMAHIP_ERR_PREDICT); }
        if ((rc = forward_set(st, nth, &dv->set, R, st->stream, err, err_cap, set_keys, false)) != 0) return bail(rc);
        if (s + 1 < S && (rc = pipe_hand_off(st, stages[s + 1], stages[s + 1]->pipe_in, st->x, (size_t) R * d * 4, err, err_cap)) != 0) return bail(rc);
    }
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    VsetBlock *dv = last->d_vset;
    int32_t *d_res = last->h_io ? last->d_io->vset.res : dv->res;
    int32_t *next_tok = S == 1 ? first->mq_tok : last->mq_tok;
    if (rq.bound && (!last->d_slot_state || !last->d_slot_trace || !next_tok)) { set_err(err, err_cap, "verify step over a set: the slots are not bound"); return bail(LLAMAHIP_ERR_PREDICT); }
    if (ss) {
        if ((rc = slide_set_enqueue(last, *ss, R, err, err_cap)) != 0) return bail(rc);
        if ((rc = pipe_sync_stages(stages, err, err_cap)) != 0) return rc;
        HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
        if (ss->k > 0 && (rc = slide_fetch(last, ss->out, R, err, err_cap)) != 0) return rc;
        last->last_rows.clear();
        m->n_evals++;
        m->t_eval_ms += now_ms() - t0;
        return LLAMAHIP_OK;
    }
    if (launch_verify_rows(last->logits, R, V, dv->pick, last->stream) != hipSuccess ||
        launch_accept_drafts_set(dv->tok, dv->pick, dv->seg_begin, dv->seg_slot, G, R, rq.bound ? last->d_slot_state : nullptr, rq.bound ? last->d_slot_trace : nullptr,
                                 C, rq.bound ? next_tok : nullptr, d_res, last->stream) != hipSuccess) {
        set_err(err, err_cap, "HIP error launching the verify kernels of a set step");
        return bail(LLAMAHIP_ERR_PREDICT);
    }
    if ((rc = pipe_sync_stages(stages, err, err_cap)) != 0) return rc;
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    if (last->h_io) memcpy(res, last->h_io->vset.res, (size_t) (R + G) * 4);
    else HIP_TRY(hipMemcpy(res, dv->res, (size_t) (R + G) * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    for (int g = 0; g < G; g++) {
        const int nd = rq.seg_begin[g + 1] - rq.seg_begin[g] - 1;
        if (res[g] < 0 || res[g] > nd) { set_err(err, err_cap, "verify step over a set: the device reported %d accepted of %d drafted tokens for slot %d", res[g], nd, rq.slot[g]); return LLAMAHIP_ERR_PREDICT; }
    }
    last->last_rows.clear();
    m->n_evals++;
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}

static int check_multi_handle(llamahip_model *m, const char *fn, int32_t n_seqs, char *err, size_t err_cap) {
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    if (n_seqs > SET_MAX) { set_err(err, err_cap, "%s: n_seqs must be 1 .. %d (got %d): a step of %d rows has none to spare for drafts, use llamahip_decode_greedy_multi", fn, SET_MAX, n_seqs, SET_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (n_seqs < 1) { set_err(err, err_cap, "%s: n_seqs must be 1 .. %d (got %d)", fn, SET_MAX, n_seqs); return LLAMAHIP_ERR_PREDICT; }
    const int have = first_of(m)->n_seq;
    if (n_seqs > have) { set_err(err, err_cap, "%s: %d sequences on a handle with %d KV slots (llamahip_opts.n_seq)", fn, n_seqs, have); return LLAMAHIP_ERR_PREDICT; }
    return 0;
}

// the arguments of a verify step over a set (greedy and sampled), checked without a device, and the step they describe; the handle last
static int check_vset_args(llamahip_model *m, const char *fn, int32_t n_seqs, const int32_t *slots, const int32_t *n_past, const int32_t *tokens,
                           const int32_t *drafts, const int32_t *n_draft, VsetReq &rq, char *err, size_t err_cap) {
    const int V = m->hp.n_vocab, C = m->hp.n_ctx, have = first_of(m)->n_seq;
    int n_rows = 0, n_dr = 0;
    for (int i = 0; i < n_seqs; i++) {
        if (slots[i] < 0 || slots[i] >= have) { set_err(err, err_cap, "%s: sequence slot %d out of range [0, %d)", fn, slots[i], have); return LLAMAHIP_ERR_PREDICT; }
        for (int j = 0; j < i; j++) if (slots[j] == slots[i]) { set_err(err, err_cap, "%s: sequence slot %d appears twice in the step", fn, slots[i]); return LLAMAHIP_ERR_PREDICT; }
        if (n_draft[i] < 0 || n_draft[i] > VERIFY_ROWS_MAX - 1) { set_err(err, err_cap, "%s: n_draft must be 0 .. %d (got %d for slot %d): a verify step has at most %d rows", fn, VERIFY_ROWS_MAX - 1, n_draft[i], slots[i], VERIFY_ROWS_MAX); return LLAMAHIP_ERR_PREDICT; }
        if (n_past[i] < 0 || n_past[i] > C - n_draft[i] - 1) { set_err(err, err_cap, "%s: context overflow: n_past (%d) + n_draft (%d) + 1 > n_ctx (%d)", fn, n_past[i], n_draft[i], C); return LLAMAHIP_ERR_PREDICT; }
        if (tokens[i] < 0 || tokens[i] >= V) { set_err(err, err_cap, "%s: token id %d out of range [0, %d)", fn, tokens[i], V); return LLAMAHIP_ERR_PREDICT; }
        n_rows += n_draft[i] + 1;
        if (n_rows > VERIFY_ROWS_MAX) { set_err(err, err_cap, "%s: a verify step has at most %d rows (%d sequences with their drafts make more)", fn, VERIFY_ROWS_MAX, i + 1); return LLAMAHIP_ERR_PREDICT; }
        if (n_draft[i] > 0 && !drafts) { set_err(err, err_cap, "%s: null drafts", fn); return LLAMAHIP_ERR_PREDICT; }
        for (int j = 0; j < n_draft[i]; j++)
            if (drafts[n_dr + j] < 0 || drafts[n_dr + j] >= V) { set_err(err, err_cap, "%s: draft token id %d at %d out of range [0, %d)", fn, drafts[n_dr + j], n_dr + j, V); return LLAMAHIP_ERR_PREDICT; }
        rq.slot[i] = slots[i]; rq.pos[i] = n_past[i]; rq.seg_begin[i] = n_rows - n_draft[i] - 1;
        rq.rows[rq.seg_begin[i]] = tokens[i];
        for (int j = 0; j < n_draft[i]; j++) rq.rows[rq.seg_begin[i] + 1 + j] = drafts[n_dr + j];
        n_dr += n_draft[i];
    }
    rq.seg_begin[n_seqs] = n_rows; rq.n_segs = n_seqs; rq.n_rows = n_rows;
    if (m->stages.empty() && (!m->first_stage || !m->last_stage)) { set_err(err, err_cap, "%s on a pipeline-stage handle: load the whole model (or a device list)", fn); return LLAMAHIP_ERR_PREDICT; }
    return check_eval_args(first_of(m), n_past[0], tokens, 1, true, err, err_cap);      // (HOST_ONLY: refused here)
}

int llamahip_verify_greedy_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *slots, const int32_t *n_past, const int32_t *tokens,
                                 const int32_t *drafts, const int32_t *n_draft, int32_t *n_accept, int32_t *picks, char *err, size_t err_cap) {
    static const char *fn = "llamahip_verify_greedy_multi";
    int rc = check_multi_handle(m, fn, n_seqs, err, err_cap);
    if (rc) return rc;
    if (!slots || !n_past || !tokens || !n_draft) { set_err(err, err_cap, "%s: null slots / n_past / tokens / n_draft", fn); return LLAMAHIP_ERR_PREDICT; }
    if (!n_accept || !picks) { set_err(err, err_cap, "%s: null output", fn); return LLAMAHIP_ERR_PREDICT; }
    VsetReq rq;
    if ((rc = check_vset_args(m, fn, n_seqs, slots, n_past, tokens, drafts, n_draft, rq, err, err_cap)) != 0) return rc;
    const int n_rows = rq.n_rows;
    const std::vector<llamahip_model *> stages = stages_of(m);
    if (n_rows == 1 || lookup_dense(m) || (stages[0]->flags & LLAMAHIP_FLAG_UNFUSED) || !vset_applies(stages, n_threads))
        // no set step on this handle (or one row): llamahip_verify_greedy on each slot in turn (segment i's draft: rq.rows behind its first row)
        return each_slot(m, n_seqs, slots, err, err_cap, [&](int i) {
            return verify_greedy_impl(m, n_threads, n_past[i], tokens[i], rq.rows + rq.seg_begin[i] + 1, n_draft[i], n_past[i], &n_accept[i], picks + rq.seg_begin[i], nullptr, err, err_cap); });
    int32_t res[2 * SET_MAX];
    if ((rc = vset_step(m, stages, n_threads, rq, res, err, err_cap)) != 0) return rc;
    memcpy(n_accept, res, (size_t) n_seqs * 4);
    memcpy(picks, res + n_seqs, (size_t) n_rows * 4);
    return LLAMAHIP_OK;
}

// the arguments of the two multi-sequence lookup loops behind their own first refusals: the context offsets (run.open), every sequence's lookup
// arguments, the handle last
static int check_lookup_multi_args(llamahip_model *m, const char *fn, LookupRun &run, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens, int32_t n_steps,
                                   const int32_t *contexts, const int32_t *corpus, int32_t n_corpus, int32_t draft_len, int32_t ngram_min, int32_t ngram_max,
                                   const int32_t *out_tokens, const llamahip_lookup_stats *stats, char *err, size_t err_cap) {
    int rc = run.open(fn, m->hp.n_ctx, n_seqs, n_past, n_steps, err, err_cap);
    if (rc) return rc;
    for (int i = 0; i < n_seqs; i++)
        if ((rc = check_lookup_args(m, fn, n_past[i], first_tokens[i], n_steps, contexts ? contexts + run.coff[i] : nullptr, n_past[i], corpus, i == 0 ? n_corpus : 0, draft_len, ngram_min,
                                    ngram_max, out_tokens, stats ? stats + i : nullptr, err, err_cap, false)) != 0) return rc;
    if (m->stages.empty() && (!m->first_stage || !m->last_stage)) { set_err(err, err_cap, "%s on a pipeline-stage handle: load the whole model (or a device list)", fn); return LLAMAHIP_ERR_PREDICT; }
    return check_eval_args(first_of(m), n_past[0], first_tokens, 1, true, err, err_cap);      // (HOST_ONLY: refused here)
}

int llamahip_decode_greedy_lookup_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens, int32_t n_steps,
                                        const int32_t *contexts, const int32_t *corpus, int32_t n_corpus, int32_t draft_len, int32_t ngram_min, int32_t ngram_max,
                                        int32_t *out_tokens, llamahip_lookup_stats *stats, char *err, size_t err_cap) {
    static const char *fn = "llamahip_decode_greedy_lookup_multi";
    int rc = check_multi_handle(m, fn, n_seqs, err, err_cap);
    if (rc) return rc;
    if (!n_past || !first_tokens) { set_err(err, err_cap, "%s: null n_past / first_tokens", fn); return LLAMAHIP_ERR_PREDICT; }
    if (!out_tokens) { set_err(err, err_cap, "%s: null out_tokens", fn); return LLAMAHIP_ERR_PREDICT; }
    LookupRun run;
    if ((rc = check_lookup_multi_args(m, fn, run, n_seqs, n_past, first_tokens, n_steps, contexts, corpus, n_corpus, draft_len, ngram_min, ngram_max, out_tokens, stats, err, err_cap)) != 0) return rc;
    const std::vector<llamahip_model *> stages = stages_of(m);
    const int S = (int) stages.size();
    llamahip_model *first = stages[0], *last = stages[S - 1];
    if (n_seqs == 1 || lookup_dense(m) || (first->flags & LLAMAHIP_FLAG_UNFUSED) || !vset_applies(stages, n_threads))
        // one sequence, or no set step on this handle: llamahip_decode_greedy_lookup on each slot in turn
        return each_slot(m, n_seqs, nullptr, err, err_cap, [&](int i) {
            return llamahip_decode_greedy_lookup(m, n_threads, n_past[i], first_tokens[i], n_steps, contexts ? contexts + run.coff[i] : nullptr, n_past[i], corpus, n_corpus,
                                                 draft_len, ngram_min, ngram_max, out_tokens + (size_t) i * n_steps, nullptr, stats ? stats + i : nullptr, err, err_cap); });
    const double t0 = now_ms();
    // (llamahip_decode_greedy_multi's binding: sequence i in slot i, its token word fed by the last stage's pick)
    if ((rc = multi_begin(stages, 1, n_seqs, n_past, first_tokens, err, err_cap)) != 0) return rc;
    run.start(first_tokens, contexts, corpus, n_corpus, draft_len, ngram_min, ngram_max);
    std::vector<int32_t> act, words(n_seqs), st2((size_t) 2 * n_seqs);
    while (run.active(act)) {
        const int A = (int) act.size();
        int dealt = 0;
        if ((rc = run.draft_round(act, [](int) { return true; }, &dealt, err, err_cap)) != 0) return rc;
        if (dealt == 0) {
            // nothing is drafted: the captured set step (one active slot: the single step) on the bound slots.  Every slot's row / token word
            // travels: the words of the slots that sat the step out are not read before they are written again
            rc = step_group(stages, { act.data(), A, 0, n_seqs, 0 }, n_threads, false, true, nullptr, err, err_cap);
            if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
            HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(hipMemcpy(words.data(), last->mq_tok, (size_t) n_seqs * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
            for (int i : act) run.accept(i, 0, &words[i], nullptr, 1);
            continue;
        }
        VsetReq rq;
        rq.bound = true;
        run.segments(act, rq);
        int32_t res[2 * SET_MAX];
        if ((rc = vset_step(m, stages, n_threads, rq, res, err, err_cap)) != 0) return rc;
        // (mirror: the host's copy of the position the accept kernel advanced)
        for (int a = 0; a < A; a++) run.accept(act[a], run.give[a], res + A + rq.seg_begin[a], nullptr, res[a] + 1, &stages);
        if (S > 1) {
            // the last stage's accept kernel advanced ITS slot words; the other stages' positions and the first stage's token words follow from the host
            for (int i = 0; i < n_seqs; i++) { st2[2 * i] = run.pos(i); st2[2 * i + 1] = run.done[i]; words[i] = run.token(i); }
            for (int s = 0; s + 1 < S; s++) {
                HIP_TRY(hipSetDevice(stages[s]->device), LLAMAHIP_ERR_PREDICT);
                HIP_TRY(hipMemcpy(stages[s]->d_slot_state, st2.data(), st2.size() * 4, hipMemcpyHostToDevice), LLAMAHIP_ERR_PREDICT);
            }
            HIP_TRY(hipSetDevice(first->device), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(hipMemcpy(first->mq_tok, words.data(), (size_t) n_seqs * 4, hipMemcpyHostToDevice), LLAMAHIP_ERR_PREDICT);
        }
    }
    // the result is each slot's device log, checked against what the host saw step by step
    std::vector<int32_t> log(n_steps);
    for (int i = 0; i < n_seqs; i++) {
        int32_t pos = 0;
        const int n = llamahip_stage_trace(last, i, &pos, log.data(), n_steps, err, err_cap);
        if (n < 0) return n;
        if (run.done[i] != n_steps || n != n_steps || pos != n_past[i] + n_steps || memcmp(log.data(), run.hist[i].data() + n_past[i] + 1, (size_t) n_steps * 4) != 0) {
            set_err(err, err_cap, "%s: the device log of sequence %d holds %d tokens up to position %d, the host counted %d of %d up to %d", fn, i, n, pos, run.done[i], n_steps, n_past[i] + n_steps);
            return LLAMAHIP_ERR_PREDICT;
        }
        memcpy(out_tokens + (size_t) i * n_steps, log.data(), (size_t) n_steps * 4);
        if (stats) stats[i] = run.ls[i];
    }
    m->t_eval_ms += now_ms() - t0;
    if (!m->stages.empty()) m->pipe_hand_off = 1;
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// llamahip_decode_sample_multi: the schedule of llamahip_decode_greedy_multi (same groups, set steps, per-slot fall-back, stage hand-offs)
// with the reference's sampler in place of the argmax.  Behind the launch that produced a group's rows of logits, the last stage's stream
// runs the sampler's device half over those rows (step_group's hook -- launch_topk_rows: one launch pair for the group, then k_topk_spill
// copies the rows flagged inexact to the slots' spill rows) and records the group's event.  The host waits for that event only, finishes each
// slot's draw with the slot's own sampler (sample_draw: from the candidates, or on the spilled row), writes the token and the new window into
// the pinned block and enqueues the group's next step -- while the groups enqueued behind it keep the device (and the other stages) busy.
// The draw itself stays on the host: it is libstdc++'s std::discrete_distribution on the sampler's mt19937.
// ------------------------------------------------------------------------------------------------
// the selection of rows [0, R) of the last stage's logits under the windows at index i0 .. of the pinned block, results at the same index
// (no device half: the rows whole to the spill rows)
static int sample_select(llamahip_model *last, const SampleParams &sp, int i0, int R, char *err, size_t err_cap) {
    const llamahip_model::SampleIo &hl = last->smp_h, &dl = last->smp_d;
    const size_t V = last->hp.n_vocab;
    if (sp.dev_sel)
        HIP_TRY(launch_topk_rows(last->logits, R, (int) V, dl.win + (size_t) i0 * 1024, dl.n_last + i0, sp.scale, sp.repeat_penalty, sp.k, dl.out + i0,
                                 dl.spill + (size_t) i0 * V, last->stream, last->smp_ws), LLAMAHIP_ERR_PREDICT);
    else HIP_TRY(hipMemcpyAsync(hl.spill + (size_t) i0 * V, last->logits, (size_t) R * V * 4, hipMemcpyDeviceToHost, last->stream), LLAMAHIP_ERR_PREDICT);
    return 0;
}

int llamahip_decode_sample_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens,
                                 int32_t n_steps, llamahip_sampler *const *samplers, double repeat_penalty, int32_t top_k, double top_p,
                                 double temp, int32_t *out_tokens, int32_t *out_exact, char *err, size_t err_cap) {
    static const char *F = "llamahip_decode_sample_multi";
    if (!m) { set_err(err, err_cap, "null model"); return LLAMAHIP_ERR_PREDICT; }
    if (!n_past || !first_tokens || !samplers || !out_tokens) {
        set_err(err, err_cap, "%s: %s is NULL", F, !n_past ? "n_past" : !first_tokens ? "first_tokens" : !samplers ? "samplers" : "out_tokens"); return LLAMAHIP_ERR_PREDICT; }
    if (n_seqs < 1) { set_err(err, err_cap, "%s: n_seqs must be >= 1 (got %d)", F, n_seqs); return LLAMAHIP_ERR_PREDICT; }
    if (n_steps < 1) { set_err(err, err_cap, "%s: n_steps must be >= 1 (got %d)", F, n_steps); return LLAMAHIP_ERR_PREDICT; }
    for (int i = 0; i < n_seqs; i++) {
        if (!samplers[i]) { set_err(err, err_cap, "%s: samplers[%d] is NULL", F, i); return LLAMAHIP_ERR_PREDICT; }
        for (int j = 0; j < i; j++)
            if (samplers[j] == samplers[i]) { set_err(err, err_cap, "%s: samplers[%d] and samplers[%d] are the same sampler: every sequence draws with its own", F, j, i); return LLAMAHIP_ERR_PREDICT; }
    }
    const std::vector<llamahip_model *> stages = stages_of(m);
    const int S = (int) stages.size();
    llamahip_model *first = stages[0], *last = stages[S - 1];
    if (n_seqs > first->n_seq) { set_err(err, err_cap, "%s: %d sequences on a handle with %d KV slots (llamahip_opts.n_seq)", F, n_seqs, first->n_seq); return LLAMAHIP_ERR_PREDICT; }
    if (first->host_only) { set_err(err, err_cap, "model was loaded with LLAMAHIP_FLAG_HOST_ONLY: no device state, cannot evaluate"); return LLAMAHIP_ERR_PREDICT; }
    if (!first->first_stage || !last->last_stage) { set_err(err, err_cap, "%s needs a whole-model or a pipeline handle", F); return LLAMAHIP_ERR_PREDICT; }
    int rc = 0;
    for (int i = 0; i < n_seqs; i++) {
        if ((rc = check_eval_args(first, n_past[i], first_tokens + i, 1, true, err, err_cap)) != 0) return rc;
        if (n_past[i] + n_steps > m->hp.n_ctx) { set_err(err, err_cap, "context overflow: n_past (%d) + n_steps (%d) > n_ctx (%d)", n_past[i], n_steps, m->hp.n_ctx); return LLAMAHIP_ERR_PREDICT; }
    }
    // (the device half runs unless top_k > 64 or n_vocab > 32768 -- then every row is spilled; a window of more than 1024 ids spills its row only)
    const SampleParams sp = sample_params(m, repeat_penalty, top_k, top_p, temp);
    if (!multi_stage_steps(first)) {
        // no stage step to batch (Q4_1 files, f16 / f32 pipeline stages, LLAMAHIP_FLAG_UNFUSED): the single-sequence loop on each slot in turn
        std::vector<float> logits;
        std::vector<int32_t> win;
        return each_slot(m, n_seqs, nullptr, err, err_cap, [&](int i) {
            int32_t *out = out_tokens + (size_t) i * n_steps, ex = 0;
            int r = 0;
            for (int t = 0; t < n_steps && r == 0; t++)
                r = sample_single_step(m, n_threads, n_past[i] + t, t ? out[t - 1] : first_tokens[i], samplers[i], sp, win, logits, &out[t], out_exact ? &out_exact[(size_t) i * n_steps + t] : &ex, err, err_cap);
            return r; });
    }
    const double t0 = now_ms();
    const int V = m->hp.n_vocab;
    const std::vector<int> g0 = group_cut(n_seqs, S);
    const int G = (int) g0.size() - 1;
    if ((rc = multi_begin(stages, G, n_seqs, n_past, nullptr, err, err_cap)) != 0) return rc;
    const llamahip_model::SampleIo &hf = first->smp_h, &hl = last->smp_h;
    // (the stream of every stage is idle here: every entry point synchronises before it returns)
    auto publish = [&](int i, int32_t tok) {
        hf.tok[i] = tok;
        hl.n_last[i] = llamahip_sampler_window(samplers[i], hl.win + (size_t) i * 1024, 1024);
    };
    for (int i = 0; i < n_seqs; i++) publish(i, first_tokens[i]);
    std::vector<int32_t> slots(n_seqs);
    for (int i = 0; i < n_seqs; i++) slots[i] = i;
    // one step of group g through every stage, its selection (slot i's window and results at index i), and the group's event on the last stage
    auto enqueue = [&](int g) {
        return step_group(stages, { slots.data() + g0[g], g0[g + 1] - g0[g], g0[g], g0[g + 1] - g0[g], g }, n_threads, false, false,
                          [&, g](int j, int R) { return sample_select(last, sp, g0[g] + j, R, err, err_cap); }, err, err_cap);
    };
    for (int g = 0; g < G && rc == 0; g++) rc = enqueue(g);
    for (int t = 0; t < n_steps && rc == 0; t++) {
        for (int g = 0; g < G && rc == 0; g++) {
            if ((rc = pipe_wait_stage(last, S - 1, err, err_cap, last->mq_ev[g])) != 0) break;
            for (int i = g0[g]; i < g0[g + 1]; i++) {
                const TopkOut &c = hl.out[i];
                const int32_t tok = sample_draw(m, samplers[i], sp, sp.dev_sel && c.fl[0] == 1, c.sc, c.id, hl.spill + (size_t) i * V, out_exact ? &out_exact[(size_t) i * n_steps + t] : nullptr);
                out_tokens[(size_t) i * n_steps + t] = tok;
                if (t + 1 < n_steps) publish(i, tok);
            }
            if (t + 1 < n_steps) rc = enqueue(g);
        }
    }
    if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
    std::vector<int32_t> state((size_t) 2 * n_seqs);
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipMemcpy(state.data(), last->d_slot_state, state.size() * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    for (int i = 0; i < n_seqs; i++)
        if (state[2 * i] != n_past[i] + n_steps) { set_err(err, err_cap, "%s: sequence %d ended at position %d, not %d", F, i, state[2 * i], n_past[i] + n_steps); return LLAMAHIP_ERR_PREDICT; }
    m->n_evals += (int64_t) n_seqs * n_steps;
    m->t_eval_ms += now_ms() - t0;
    if (!m->stages.empty()) m->pipe_hand_off = 1;
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// llamahip_beam_search (llamahip.h): llamahip_decode_sample_multi's loop -- slots bound with host-written token words, one
// set step over the live slots, a device reduction behind it (step_group's hook: k_row_topn over the step's rows into pinned memory), one
// wait per step -- with the beams' bookkeeping between the steps: the step rule (llamahip_beam_select), the slots and the KV copies
// (llamahip_beam_slots; one k_kv_copy_rows launch per stage, stream-ordered in front of the step) and the token words.  One group whatever
// the stage count: the live set changes from step to step and every step waits for its candidates anyway.
// ------------------------------------------------------------------------------------------------
constexpr int BEAM_CAND_MAX = 2 * LLAMAHIP_BEAM_MAX;
static int beam_prepare(llamahip_model *last, char *err, size_t err_cap) {
    if (last->beam_blk) return 0;
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(last->own.alloc(&last->beam_blk, (size_t) LLAMAHIP_BEAM_MAX * BEAM_CAND_MAX * 12, true, MEM_PINNED), LLAMAHIP_ERR_PREDICT);
    const hipError_t e = hipHostGetDevicePointer((void **) &last->beam_dev, last->beam_blk, 0);
    if (e != hipSuccess) last->own.release(&last->beam_blk);
    HIP_TRY(e, LLAMAHIP_ERR_PREDICT);
    return 0;
}
// k_row_topn over R rows of the last stage's logits from `row` on, nc places each, results at index i0 .. of the pinned block
static int beam_topn(llamahip_model *last, const float *row, int R, int nc, int i0, char *err, size_t err_cap) {
    double *lp = (double *) last->beam_dev;
    int32_t *ids = (int32_t *) (last->beam_dev + (size_t) LLAMAHIP_BEAM_MAX * BEAM_CAND_MAX * 8);
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(launch_row_topn(row, R, last->hp.n_vocab, nc, ids + (size_t) i0 * nc, lp + (size_t) i0 * nc, last->stream), LLAMAHIP_ERR_PREDICT);
    return 0;
}

int llamahip_beam_search(llamahip_model *m, const llamahip_beam_opts *o, const int32_t *prompt, int32_t n_prompt, llamahip_beam_hyp *hyps_out,
                         int32_t *tokens_out, int32_t *n_hyps_out, llamahip_beam_stats *stats, char *err, size_t err_cap) {
    static const char *fn = "llamahip_beam_search";
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    int rc = beam_check(m->hp.n_ctx, m->hp.n_vocab, m->n_seq, o, prompt, n_prompt, hyps_out, tokens_out, n_hyps_out, err, err_cap);
    if (rc) return rc;
    if (m->sched) { set_err(err, err_cap, "%s: the handle has a live scheduler, which owns KV slots 0 .. %d: free it first", fn, sched_dev_max_active(m->sched) - 1); return LLAMAHIP_ERR_PREDICT; }
    if ((rc = decode_handle_check(m, fn, err, err_cap)) != 0) return rc;
    const std::vector<llamahip_model *> stages = stages_of(m);
    const int S = (int) stages.size();
    llamahip_model *first = stages[0], *last = stages[S - 1];
    const int B = o->n_beams, nc = 2 * B, P0 = n_prompt, T = o->n_predict, V = m->hp.n_vocab, nth = o->n_threads;
    const int n_return = o->n_return ? o->n_return : B;
    const size_t d = first->hp.n_embd;
    const bool set_path = multi_stage_steps(first);
    llamahip_beam_stats bs;
    memset(&bs, 0, sizeof(bs));
    bs.struct_size = (int32_t) sizeof(bs);
    *n_hyps_out = 0;
    if ((rc = beam_prepare(last, err, err_cap)) != 0) return rc;
    const double *h_lp = (const double *) last->beam_blk;
    const int32_t *h_ids = (const int32_t *) (last->beam_blk + (size_t) LLAMAHIP_BEAM_MAX * BEAM_CAND_MAX * 8);

    // the prompt on slot 0 (enqueued and waited for as the entry point it is); its last row stays where the last pass left it
    const int32_t zero = 0;
    const int chunk = o->chunk_tokens;
    rc = each_slot(m, 1, &zero, err, err_cap, [&](int) {
        return chunk > 0 ? eval_chunks_impl(m, nth, 0, prompt, P0, chunk, nullptr, true, err, err_cap) : llamahip_eval(m, nth, 0, prompt, P0, nullptr, err, err_cap); });
    if (rc) return rc;
    const int n_last_pass = (chunk > 0 && P0 > chunk && !chunks_in_one_pass(m, P0)) ? P0 - (P0 - 1) / chunk * chunk : P0;
    if ((rc = beam_topn(last, last->logits + (size_t) (n_last_pass - 1) * V, 1, nc, 0, err, err_cap)) != 0) return drain_stages(stages, rc, err, err_cap);
    if ((rc = drain_stages(stages, 0, err, err_cap)) != 0) return rc;

    struct Beam { std::vector<int32_t> tokens; double S; int32_t slot, row; };
    struct Fin { std::vector<int32_t> tokens; double S; int32_t reason, slot; };
    std::vector<Beam> live(1), next;
    live[0].S = 0.0; live[0].slot = 0; live[0].row = 0;
    std::vector<Fin> fin;
    bool bound = false;
    std::vector<int32_t> dev_pos((size_t) B, P0);      // the slots' device positions (set steps)
    // slot `slot` of every stage at position `pos`, multi_begin's pointers (the same ones: no graph is dropped)
    auto rebind = [&](int slot, int pos) {
        for (int s = 0; s < S; s++) {
            llamahip_model *st = stages[s];
            const int r = llamahip_stage_bind(st, slot, pos, s == 0 ? first->smp_d.tok + slot : nullptr, s ? st->mq_in + (size_t) slot * d : nullptr,
                                              s + 1 < S ? st->mq_out + (size_t) slot * d : nullptr, nullptr, err, err_cap);
            if (r) return r;
        }
        return 0;
    };
    const int save_seq = m->cur_seq;
    for (int t = 1; rc == 0; t++) {
        // ---- the step rule over the live beams' candidates
        const int L = (int) live.size();
        double sc[LLAMAHIP_BEAM_MAX], c_lp[LLAMAHIP_BEAM_MAX * BEAM_CAND_MAX], new_S[LLAMAHIP_BEAM_MAX], fin_S[LLAMAHIP_BEAM_MAX];
        int32_t c_id[LLAMAHIP_BEAM_MAX * BEAM_CAND_MAX], new_par[LLAMAHIP_BEAM_MAX], new_tok[LLAMAHIP_BEAM_MAX], fin_par[LLAMAHIP_BEAM_MAX], n_new = 0, n_fin = 0, n_dead = 0;
        for (int i = 0; i < L; i++) {
            sc[i] = live[i].S;
            memcpy(c_lp + (size_t) i * nc, h_lp + (size_t) live[i].row * nc, (size_t) nc * 8);
            memcpy(c_id + (size_t) i * nc, h_ids + (size_t) live[i].row * nc, (size_t) nc * 4);
        }
        if (llamahip_beam_select(L, sc, nc, c_id, c_lp, B, o->stop_token, new_par, new_tok, new_S, &n_new, fin_par, fin_S, &n_fin, &n_dead) != 0) {
            set_err(err, err_cap, "%s: llamahip_beam_select refused a step of %d beams", fn, L); rc = LLAMAHIP_ERR_PREDICT; break; }
        bs.n_dead += n_dead; bs.n_stop += n_fin;
        for (int k = 0; k < n_fin; k++) {
            Fin f = { live[fin_par[k]].tokens, fin_S[k], LLAMAHIP_DONE_STOP, -1 };
            f.tokens.push_back(o->stop_token);
            fin.push_back(std::move(f));
        }
        next.assign((size_t) n_new, Beam());
        for (int k = 0; k < n_new; k++) {
            next[k].tokens = live[new_par[k]].tokens;
            next[k].tokens.push_back(new_tok[k]);
            next[k].S = new_S[k];
        }
        if (t == T) {      // the last token is not evaluated: the hypothesis' rows are its parent's
            for (int k = 0; k < n_new; k++) fin.push_back({ std::move(next[k].tokens), next[k].S, LLAMAHIP_DONE_LENGTH, live[new_par[k]].slot });
            break;
        }
        if (n_new == 0) break;
        if (!o->length_norm && o->stop_token >= 0 && (int) fin.size() >= n_return) {
            std::vector<double> fs;
            for (const Fin &f : fin) fs.push_back(f.S);
            std::sort(fs.begin(), fs.end(), [](double a, double b) { return a > b; });
            if (fs[(size_t) n_return - 1] >= next[0].S) break;
        }
        // ---- the slots, and the forked beams' rows: rows [0, P) of the parent's slot
        const int P = P0 + t - 1;      // the position the new tokens are evaluated at = the rows a parent holds
        int32_t prev_slot[LLAMAHIP_BEAM_MAX], new_slot[LLAMAHIP_BEAM_MAX], c_src[LLAMAHIP_BEAM_MAX], c_dst[LLAMAHIP_BEAM_MAX];
        for (int i = 0; i < L; i++) prev_slot[i] = live[i].slot;
        const int n_copies = llamahip_beam_slots(L, prev_slot, n_new, new_par, B, new_slot, c_src, c_dst);
        if (n_copies < 0) { set_err(err, err_cap, "%s: llamahip_beam_slots refused a step of %d beams", fn, n_new); rc = LLAMAHIP_ERR_PREDICT; break; }
        if (n_copies > 0) {
            KvCopyTab tab = {};
            tab.n = n_copies;
            for (int c = 0; c < n_copies; c++) { tab.src[c] = c_src[c]; tab.dst[c] = c_dst[c]; tab.row_begin[c] = 0; tab.n_rows[c] = P; }
            if ((rc = kv_copy_enqueue(stages, tab, fn, err, err_cap)) != 0) break;
            bs.n_copy_launches += S; bs.n_copied_rows += (int64_t) n_copies * P;
        }
        // ---- the step: the live slots in ascending order (a set orders its rows by slot id), beam k's candidates at index next[k].row
        std::vector<int32_t> act((size_t) n_new);
        for (int k = 0; k < n_new; k++) { next[k].slot = new_slot[k]; act[k] = new_slot[k]; }
        std::sort(act.begin(), act.end());
        for (int k = 0; k < n_new; k++) next[k].row = (int32_t) (std::lower_bound(act.begin(), act.end(), next[k].slot) - act.begin());
        if (set_path) {
            if (!bound) {
                std::vector<int32_t> past((size_t) B, P0);
                if ((rc = multi_begin(stages, 1, B, past.data(), nullptr, err, err_cap)) != 0) break;
                bound = true;
            }
            for (int k = 0; k < n_new && rc == 0; k++) {
                const int sl = next[k].slot;
                if (dev_pos[sl] != P) rc = rebind(sl, P);      // (a slot that sat out a step)
                dev_pos[sl] = P + 1;
                first->smp_h.tok[sl] = next[k].tokens.back();
            }
            if (rc) break;
            rc = step_group(stages, { act.data(), n_new, 0, B, 0 }, nth, false, false,
                            [&](int j, int R) { return beam_topn(last, last->logits, R, nc, j, err, err_cap); }, err, err_cap);
            if (rc == 0) rc = pipe_wait_stage(last, S - 1, err, err_cap, last->mq_ev[0]);
            bs.n_set_steps++;
        } else {
            // no stage step to batch (Q4_1 files, f16 / f32 pipeline stages, LLAMAHIP_FLAG_UNFUSED): llamahip_eval on each live slot in turn, the
            // same kernel over its row (the copies above are on the stages' streams, ahead of the evals)
            for (int j = 0; j < n_new && rc == 0; j++) {
                int k = 0;
                while (next[k].row != j) k++;
                const int32_t tok = next[k].tokens.back();
                if ((rc = llamahip_set_seq(m, act[j], err, err_cap)) != 0) break;
                if ((rc = llamahip_eval(m, nth, P, &tok, 1, nullptr, err, err_cap)) != 0) break;
                rc = beam_topn(last, last->logits, 1, nc, j, err, err_cap);
                if (rc == 0 && hipStreamSynchronize(last->stream) != hipSuccess) { set_err(err, err_cap, "%s: HIP error waiting for k_row_topn", fn); rc = LLAMAHIP_ERR_PREDICT; }
                bs.n_fallback_steps++;
            }
        }
        bs.n_steps++; bs.n_rows += n_new;
        live.swap(next);
    }
    (void) llamahip_set_seq(m, save_seq, nullptr, 0);
    if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;

    // ---- the result: the finished list ranked
    const int nf = (int) fin.size();
    std::vector<double> fS((size_t) nf);
    std::vector<int32_t> fL((size_t) nf), order((size_t) nf);
    for (int k = 0; k < nf; k++) { fS[k] = fin[k].S; fL[k] = (int32_t) fin[k].tokens.size(); }
    beam_rank(nf, fS.data(), fL.data(), o->length_norm, order.data());
    const int n_out = std::min(nf, n_return);
    for (int k = 0; k < n_out; k++) {
        const Fin &f = fin[order[k]];
        hyps_out[k].length = (int32_t) f.tokens.size(); hyps_out[k].reason = f.reason; hyps_out[k].slot = f.slot; hyps_out[k].reserved = 0; hyps_out[k].score = f.S;
        int32_t *row = tokens_out + (size_t) k * T;
        for (int j = 0; j < T; j++) row[j] = j < (int) f.tokens.size() ? f.tokens[j] : -1;
    }
    *n_hyps_out = n_out;
    if (stats) { const int32_t n = std::min((size_t) std::max(stats->struct_size, 0), sizeof(bs)); if (n >= 4) { bs.struct_size = n; memcpy(stats, &bs, (size_t) n); } }
    if (!m->stages.empty()) m->pipe_hand_off = 1;
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Drafted SAMPLED decoding for SEVERAL sequences at once: llamahip_verify_sample_multi / llamahip_decode_sample_lookup_multi -- the two halves
// above put together.  ROWS: a verify step over a set (vset_step) evaluates rows cut into per-slot segments, every row the single-token eval
// of its slot at its own position.  SAMPLER: the reference's sampler is a deterministic function of (row logits, last_n_tokens window,
// mt19937 state), and the window at row j of a segment -- IF that sequence's draft tokens 0 .. j - 1 were accepted -- is known before the eval.
// So the device selects every row's candidates under that window (launch_topk_slide_set behind forward_set on the last stage's stream: the
// segments slide inside their own id streams of one pool) and the host walks every segment with that sequence's OWN sampler (sample_walk,
// as verify_sample_impl walks its rows).  The accept step therefore lives on the host: what a segment accepts depends on draws of a host-side
// mt19937 (std::discrete_distribution), so there is nothing for k_accept_drafts_set to compare; the loop keeps the slots' device words
// {position, cursor} in step from the host instead.
// (Equality with single steps is BY TEST -- tests/test_gpu_sample_lookup_multi.py -- not structural: the norm's one-pass against two-pass
//  statistics, as for set steps and verify steps.)
// ------------------------------------------------------------------------------------------------
// the id pool and the per-row table of a sampled step: segment g's stream = samplers[g]'s window, then its draft (rq.rows behind its first row);
// seg_sel[g]: the device makes candidates for the segment's rows
static void slide_set_build(const VsetReq &rq, llamahip_sampler *const *samplers, const SampleParams &sp, int32_t *pool, TopkOut *out, SlideSetReq &ss, bool *seg_sel) {
    ss.ids = pool; ss.n_ids = 0; ss.scale = sp.scale; ss.repeat_penalty = sp.repeat_penalty; ss.k = sp.dev_sel ? sp.k : 0; ss.out = out;
    memset(ss.row_off, 0, sizeof(ss.row_off));
    memset(ss.row_n_last, 0, sizeof(ss.row_n_last));
    for (int g = 0; g < rq.n_segs; g++) {
        const int rows = rq.seg_begin[g + 1] - rq.seg_begin[g];
        const int32_t nw = llamahip_sampler_window(samplers[g], nullptr, 0);
        seg_sel[g] = sp.dev_sel && nw <= 1024;
        if (!sp.dev_sel) continue;
        if (nw > 1024) {        // (no ids travel: the rows are flagged inexact by their length)
            for (int j = 0; j < rows; j++) ss.row_n_last[rq.seg_begin[g] + j] = 1025;
            continue;
        }
        int32_t *st = pool + ss.n_ids;
        (void) llamahip_sampler_window(samplers[g], st, nw);
        for (int j = 0; j + 1 < rows; j++) st[nw + j] = rq.rows[rq.seg_begin[g] + 1 + j];
        for (int j = 0; j < rows; j++) { ss.row_off[rq.seg_begin[g] + j] = ss.n_ids + j; ss.row_n_last[rq.seg_begin[g] + j] = nw; }
        ss.n_ids += nw + rows - 1;
    }
}

static int check_samplers(const char *fn, int32_t n_seqs, llamahip_sampler *const *samplers, double repeat_penalty, int32_t top_k, double top_p, double temp, char *err, size_t err_cap) {
    if (!samplers) { set_err(err, err_cap, "%s: null samplers", fn); return LLAMAHIP_ERR_PREDICT; }
    for (int i = 0; i < n_seqs; i++) {
        if (!samplers[i]) { set_err(err, err_cap, "%s: null sampler (samplers[%d])", fn, i); return LLAMAHIP_ERR_PREDICT; }
        int rc = check_sampler_params(fn, samplers[i], repeat_penalty, top_k, top_p, temp, err, err_cap);
        if (rc) return rc;
        for (int j = 0; j < i; j++)
            if (samplers[j] == samplers[i]) { set_err(err, err_cap, "%s: samplers[%d] and samplers[%d] are the same sampler: every sequence draws with its own", fn, j, i); return LLAMAHIP_ERR_PREDICT; }
    }
    return 0;
}

int llamahip_verify_sample_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *slots, const int32_t *n_past, const int32_t *tokens,
                                 const int32_t *drafts, const int32_t *n_draft, llamahip_sampler *const *samplers, double repeat_penalty, int32_t top_k,
                                 double top_p, double temp, int32_t *n_accept, int32_t *picks, int32_t *exact, char *err, size_t err_cap) {
    static const char *fn = "llamahip_verify_sample_multi";
    int rc = check_multi_handle(m, fn, n_seqs, err, err_cap);
    if (rc) return rc;
    if (!slots || !n_past || !tokens || !n_draft) { set_err(err, err_cap, "%s: null slots / n_past / tokens / n_draft", fn); return LLAMAHIP_ERR_PREDICT; }
    if (!n_accept || !picks) { set_err(err, err_cap, "%s: null output", fn); return LLAMAHIP_ERR_PREDICT; }
    if ((rc = check_samplers(fn, n_seqs, samplers, repeat_penalty, top_k, top_p, temp, err, err_cap)) != 0) return rc;
    VsetReq rq;
    if ((rc = check_vset_args(m, fn, n_seqs, slots, n_past, tokens, drafts, n_draft, rq, err, err_cap)) != 0) return rc;
    const std::vector<llamahip_model *> stages = stages_of(m);
    const SampleParams sp = sample_params(m, repeat_penalty, top_k, top_p, temp);
    std::vector<int32_t> win;
    std::vector<float> logits;
    if (rq.n_rows == 1 || sample_lookup_by_rows(m) || !vset_applies(stages, n_threads))
        // no set step on this handle (or one row): llamahip_verify_sample on each slot in turn (segment i's draft: rq.rows behind its first row)
        return each_slot(m, n_seqs, slots, err, err_cap, [&](int i) {
            return verify_sample_impl(m, n_threads, n_past[i], tokens[i], rq.rows + rq.seg_begin[i] + 1, n_draft[i], samplers[i], sp, &n_accept[i],
                                      picks + rq.seg_begin[i], exact ? exact + rq.seg_begin[i] : nullptr, win, logits, err, err_cap); });
    std::vector<int32_t> pool(SLIDE_SET_IDS);
    TopkOut out[VERIFY_ROWS_MAX];
    bool seg_sel[SET_MAX];
    SlideSetReq ss;
    slide_set_build(rq, samplers, sp, pool.data(), out, ss, seg_sel);
    if ((rc = vset_step(m, stages, n_threads, rq, nullptr, err, err_cap, &ss)) != 0) return rc;
    for (int r = 0; r < rq.n_rows; r++) { picks[r] = -1; if (exact) exact[r] = -1; }      // (-1 behind each segment's walk)
    for (int g = 0; g < n_seqs && rc == 0; g++)
        rc = sample_walk(m, stages.back(), rq.seg_begin[g], rq.rows + rq.seg_begin[g] + 1, n_draft[g], samplers[g], seg_sel[g], out, sp, &n_accept[g], picks + rq.seg_begin[g],
                         exact ? exact + rq.seg_begin[g] : nullptr, logits, err, err_cap);
    return rc;
}

int llamahip_decode_sample_lookup_multi(llamahip_model *m, int32_t n_threads, int32_t n_seqs, const int32_t *n_past, const int32_t *first_tokens, int32_t n_steps,
                                        const int32_t *contexts, const int32_t *corpus, int32_t n_corpus, int32_t draft_len, int32_t ngram_min, int32_t ngram_max,
                                        llamahip_sampler *const *samplers, double repeat_penalty, int32_t top_k, double top_p, double temp,
                                        int32_t *out_tokens, int32_t *out_exact, llamahip_lookup_stats *stats, char *err, size_t err_cap) {
    static const char *fn = "llamahip_decode_sample_lookup_multi";
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    if (n_seqs > SET_MAX) { set_err(err, err_cap, "%s: n_seqs must be 1 .. %d (got %d): a step of %d rows has none to spare for drafts, use llamahip_decode_sample_multi", fn, SET_MAX, n_seqs, SET_MAX); return LLAMAHIP_ERR_PREDICT; }
    int rc = check_multi_handle(m, fn, n_seqs, err, err_cap);
    if (rc) return rc;
    if (!n_past || !first_tokens) { set_err(err, err_cap, "%s: null n_past / first_tokens", fn); return LLAMAHIP_ERR_PREDICT; }
    if (!out_tokens) { set_err(err, err_cap, "%s: null out_tokens", fn); return LLAMAHIP_ERR_PREDICT; }
    if ((rc = check_samplers(fn, n_seqs, samplers, repeat_penalty, top_k, top_p, temp, err, err_cap)) != 0) return rc;
    LookupRun run;
    if ((rc = check_lookup_multi_args(m, fn, run, n_seqs, n_past, first_tokens, n_steps, contexts, corpus, n_corpus, draft_len, ngram_min, ngram_max, out_tokens, stats, err, err_cap)) != 0) return rc;
    const std::vector<llamahip_model *> stages = stages_of(m);
    llamahip_model *first = stages[0], *last = stages.back();
    if (n_seqs == 1 || sample_lookup_by_rows(m) || !vset_applies(stages, n_threads))
        // one sequence, or no set step on this handle: llamahip_decode_sample_lookup on each slot in turn
        return each_slot(m, n_seqs, nullptr, err, err_cap, [&](int i) {
            return llamahip_decode_sample_lookup(m, n_threads, n_past[i], first_tokens[i], n_steps, contexts ? contexts + run.coff[i] : nullptr, n_past[i], corpus, n_corpus,
                                                 draft_len, ngram_min, ngram_max, samplers[i], repeat_penalty, top_k, top_p, temp, out_tokens + (size_t) i * n_steps,
                                                 out_exact ? out_exact + (size_t) i * n_steps : nullptr, stats ? stats + i : nullptr, err, err_cap); });
    const double t0 = now_ms();
    const int V = m->hp.n_vocab;
    // the device half runs unless top_k > 64 or n_vocab > 32768: then every row is spilled and nobody drafts; a window of more than 1024 ids spills
    // its own rows only, and that sequence wants no draft
    const SampleParams sp = sample_params(m, repeat_penalty, top_k, top_p, temp);
    // (llamahip_decode_sample_multi's binding: sequence i in slot i, its token word in the pinned block, written by the host)
    if ((rc = multi_begin(stages, 1, n_seqs, n_past, nullptr, err, err_cap)) != 0) return rc;
    const llamahip_model::SampleIo &hf = first->smp_h, &hl = last->smp_h;
    run.start(first_tokens, contexts, corpus, n_corpus, draft_len, ngram_min, ngram_max);
    run.out_tokens = out_tokens; run.out_exact = out_exact;
    // a verify step advances no slot word on any device (what it accepts is known on the host only): before the next captured step the host writes
    // every slot's {position, cursor} on every stage -- through the pinned block where the stage has one; the first stage's token words are
    // written before every plain step anyway
    bool words_stale = false;
    auto push_words = [&]() -> int {
        int32_t w[2 * SET_MAX];
        for (int i = 0; i < n_seqs; i++) { w[2 * i] = run.pos(i); w[2 * i + 1] = run.done[i]; }
        for (llamahip_model *st : stages) {
            HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_PREDICT);
            if (st->h_io) {                 // (the stream is idle: the step before was waited for)
                memcpy(st->h_io->slot_words, w, (size_t) n_seqs * 8);
                HIP_TRY(hipMemcpyAsync(st->d_slot_state, st->h_io->slot_words, (size_t) n_seqs * 8, hipMemcpyHostToDevice, st->stream), LLAMAHIP_ERR_PREDICT);
            } else HIP_TRY(hipMemcpy(st->d_slot_state, w, (size_t) n_seqs * 8, hipMemcpyHostToDevice), LLAMAHIP_ERR_PREDICT);
        }
        words_stale = false;
        return 0;
    };
    // (the selection of a plain step: row a's window and results at index a of the pinned block)
    const std::function<int(int, int)> select = [&](int j, int R) { return sample_select(last, sp, j, R, err, err_cap); };
    std::vector<int32_t> act, pool(SLIDE_SET_IDS);
    std::vector<float> logits;
    while (run.active(act)) {
        const int A = (int) act.size();
        int dealt = 0;
        if ((rc = run.draft_round(act, [&](int i) { return sp.dev_sel && llamahip_sampler_window(samplers[i], nullptr, 0) <= 1024; }, &dealt, err, err_cap)) != 0) return rc;
        if (dealt == 0) {
            // llamahip_decode_sample_multi's step over the active slots: row a of the step = slot act[a] (a set orders its rows by slot id).  Every
            // slot's row travels: the rows of the slots that sat the step out are not read before they are written again
            if (words_stale) rc = push_words();
            for (int a = 0; a < A && rc == 0; a++) {
                hf.tok[act[a]] = run.token(act[a]);
                hl.n_last[a] = llamahip_sampler_window(samplers[act[a]], hl.win + (size_t) a * 1024, 1024);
            }
            if (rc == 0) rc = step_group(stages, { act.data(), A, 0, n_seqs, 0 }, n_threads, false, false, select, err, err_cap);
            if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
            for (int a = 0; a < A; a++) {
                const TopkOut &c = hl.out[a];
                int32_t ex = 0;
                const int32_t tok = sample_draw(m, samplers[act[a]], sp, sp.dev_sel && c.fl[0] == 1, c.sc, c.id, hl.spill + (size_t) a * V, &ex);
                run.accept(act[a], 0, &tok, &ex, 1);
            }
            m->n_evals += A;
            continue;
        }
        VsetReq rq;
        run.segments(act, rq);
        llamahip_sampler *seg_smp[SET_MAX];
        for (int a = 0; a < A; a++) seg_smp[a] = samplers[act[a]];
        TopkOut out[VERIFY_ROWS_MAX];
        bool seg_sel[SET_MAX];
        SlideSetReq ss;
        slide_set_build(rq, seg_smp, sp, pool.data(), out, ss, seg_sel);
        if ((rc = vset_step(m, stages, n_threads, rq, nullptr, err, err_cap, &ss)) != 0) return rc;
        for (int a = 0; a < A; a++) {
            int32_t na = 0, picks[VERIFY_ROWS_MAX], exact[VERIFY_ROWS_MAX];
            if ((rc = sample_walk(m, last, rq.seg_begin[a], rq.rows + rq.seg_begin[a] + 1, run.give[a], seg_smp[a], seg_sel[a], out, sp, &na, picks, exact, logits, err, err_cap)) != 0) return rc;
            run.accept(act[a], run.give[a], picks, exact, na + 1, &stages);      // (mirror: the host's copy of the slot's position)
        }
        words_stale = true;
    }
    // the slots end where a caller of the stage API expects them; the last stage's words are read back against the host's count
    if (words_stale) rc = push_words();
    if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
    std::vector<int32_t> state((size_t) 2 * n_seqs);
    HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipMemcpy(state.data(), last->d_slot_state, state.size() * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    for (int i = 0; i < n_seqs; i++) {
        if (run.done[i] != n_steps || state[2 * i] != n_past[i] + n_steps) { set_err(err, err_cap, "%s: sequence %d ended at position %d after %d of %d steps, not at %d", fn, i, state[2 * i], run.done[i], n_steps, n_past[i] + n_steps); return LLAMAHIP_ERR_PREDICT; }
        if (stats) stats[i] = run.ls[i];
    }
    m->t_eval_ms += now_ms() - t0;
    if (!m->stages.empty()) m->pipe_hand_off = 1;
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// The request scheduler's device half (sched.h; the queue, the slots and the step rule are sched.cpp's): what ONE planned step runs.
// MIXED PASS, some segment a prompt piece: llamahip_eval_multi's pass (RowsPass: a decode row is a one-token segment of it) on every stage,
// then on the last stage's stream the candidate selection over the sampled segments that emit (they are ordered first, so their logits
// rows are rows [0, ns): sample_select) and k_sched_pick over all segments -- greedy picks into the result block, the slots' {position,
// cursor} / next-token words / traces set on the device.  DECODE-ONLY STEP: step_group over the active slots, llamahip_decode_*_multi's step
// (the captured set step; one active slot: the single step), one wait, the picks read from the slots' token words.
// The slots [0, max_active) stay bound the greedy loops' way (multi_begin: token word = mq_tok[slot], fed by the last stage's pick); a
// sampled request's token word is written by the host before every decode-only step.  The host mirrors every slot's {position, cursor,
// token} and pushes them to every stage where the device cannot know them: after a (re)bind, and on a pipeline handle after a mixed pass
// (k_sched_pick runs on the last stage only -- llamahip_decode_sample_lookup_multi keeps its stages in step the same way).
// FALL-BACK, handles without the pass or without a set step: the contract's own per-slot calls, segment by segment.
// A STEP WITH DRAFTED TOKENS (some decoding segment carries a draft; include/llamahip.h) is the mixed pass whether or not
// anybody prefills: such a segment is [last token, draft ...], every row keyed as its own single-token eval, the lm head over every row of it
// and the last row of every other emitting segment -- at most 16 logits rows.  Behind it k_verify_rows + k_sched_accept for the greedy
// segments; for the sampled ones (still ordered first) the sliding-window candidate selection over their rows (slide_set_enqueue) and
// llamahip_verify_sample_multi's host walk, after which the slots' words are the host's to push (stale).
// ------------------------------------------------------------------------------------------------
extern "C++" {
namespace lh {
// the last stage's d_sched_tab: k_sched_pick's table and result as before, behind them a drafted step's k_sched_accept table | the logits
// rows' tokens | k_verify_rows' picks | the result {n_accept[16], pick[16]}
// (k_sched_pick_dfa's result is {pick[16], dead[16]}: the table's 64 words, then 32; a constrained drafted step's dead words lie at the end)
constexpr int SCHED_ACC_TAB = 6 * SET_MAX, SCHED_ACC_TOK = SCHED_ACC_TAB + SCHED_TAB_W * SET_MAX, SCHED_ACC_PICK = SCHED_ACC_TOK + VERIFY_ROWS_MAX,
              SCHED_ACC_RES = SCHED_ACC_PICK + VERIFY_ROWS_MAX, SCHED_ACC_DEAD = SCHED_ACC_RES + SET_MAX + VERIFY_ROWS_MAX, SCHED_TAB_WORDS = SCHED_ACC_DEAD + VERIFY_ROWS_MAX;
struct SchedDev {
    llamahip_model *m = nullptr;
    int n_threads = 1, max_active = 1, chunk = 0;
    double repeat_penalty = 0, top_p = 0, temp = 0;
    int32_t top_k = 0;
    bool decided = false, fallback = false, stale = true;
    int32_t pos[SET_MAX] = { 0 }, cur[SET_MAX] = { 0 }, tok[SET_MAX] = { 0 };      // host mirrors of the slots' words
    std::vector<float> logits;
    std::vector<int32_t> win, pool;          // pool: the id streams of a drafted step's sampled segments
};

int sched_handle_info(const llamahip_model *m, SchedHandleInfo *out, char *err, size_t err_cap) {
    const int rc = decode_handle_check(m, "llamahip_sched_new", err, err_cap);
    if (rc) return rc;
    const llamahip_model *first = m->stages.empty() ? m : m->stages[0];
    *out = { m->hp.n_ctx, m->hp.n_vocab, first->n_seq, (first->flags & LLAMAHIP_FLAG_FAST_PREFILL) ? 1 : 0, m->stages.empty() ? 0 : 1 };
    return 0;
}
int sched_sampler_check(double repeat_penalty, int32_t top_k, double top_p, double temp, char *err, size_t err_cap) {
    return check_sampling_rule("llamahip_sched_new", repeat_penalty, top_k, top_p, temp, err, err_cap);
}
// one scheduler per handle at a time: a second one would rebind and overwrite the first one's slots
int sched_dev_new(llamahip_model *m, const llamahip_sched_opts *o, SchedDev **out, char *err, size_t err_cap) {
    *out = nullptr;
    if (m->sched) { set_err(err, err_cap, "llamahip_sched_new: the handle already has a scheduler (one per handle at a time: llamahip_sched_free the other first)"); return LLAMAHIP_ERR_PREDICT; }
    SchedDev *d = new SchedDev();
    d->m = m; d->n_threads = o->n_threads; d->max_active = o->max_active; d->chunk = o->chunk_tokens;
    d->repeat_penalty = o->repeat_penalty; d->top_p = o->top_p; d->temp = o->temp; d->top_k = o->top_k;
    m->sched = d;
    *out = d;
    return 0;
}
// llamahip_eval_multi's and the multi-sequence decoders' own conditions: the pass, a stage step to batch, set steps of every size
static void sched_decide(SchedDev *d) {
    if (d->decided) return;
    const std::vector<llamahip_model *> stages = stages_of(d->m);
    d->fallback = !rows_pass_applies(d->m) || !multi_stage_steps(stages[0]) || !vset_applies(stages, d->n_threads);
    d->decided = true;
}
int sched_dev_drafts(SchedDev *d) {
    if (!d || !d->m) return 0;
    sched_decide(d);
    return d->fallback ? 0 : 1;
}
// one k_kv_copy_rows launch per stage, each on its own device and stream; nothing is waited for
int sched_dev_max_active(const SchedDev *d) { return d->max_active; }
int kv_copy_enqueue(const std::vector<llamahip_model *> &stages, const KvCopyTab &tab, const char *fn, char *err, size_t err_cap) {
    for (llamahip_model *st : stages) {
        HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_PREDICT);
        if (launch_kv_copy_rows(st->Kc, st->Vc, tab, st->n_seq, st->l1 - st->l0, st->hp.n_ctx, st->hp.n_embd, st->stream) != hipSuccess) {
            set_err(err, err_cap, "%s: HIP error launching k_kv_copy_rows on device %d", fn, st->device);
            return LLAMAHIP_ERR_PREDICT;
        }
    }
    return 0;
}
int sched_dev_copy_prefix(SchedDev *d, int32_t src, int32_t dst, int32_t row_begin, int32_t n_rows, int32_t *launches, char *err, size_t err_cap) {
    static const char *fn = "llamahip_sched_step";
    *launches = 0;
    llamahip_model *m = d->m;
    if (!m) { set_err(err, err_cap, "%s: the scheduler's model handle has been freed", fn); return LLAMAHIP_ERR_PREDICT; }
    if (src < 0 || src >= d->max_active || dst < 0 || dst >= d->max_active || src == dst || row_begin < 0 || n_rows < 1 || (int64_t) row_begin + n_rows > m->hp.n_ctx) {
        set_err(err, err_cap, "%s: a prefix copy of %d rows at %d from slot %d to slot %d is outside the scheduler's slots or the context (n_ctx %d)", fn, n_rows, row_begin, src, dst, m->hp.n_ctx);
        return LLAMAHIP_ERR_PREDICT;
    }
    const std::vector<llamahip_model *> stages = stages_of(m);
    KvCopyTab tab = {};
    tab.n = 1; tab.src[0] = src; tab.dst[0] = dst; tab.row_begin[0] = row_begin; tab.n_rows[0] = n_rows;
    const int rc = kv_copy_enqueue(stages, tab, fn, err, err_cap);
    if (rc) return drain_stages(stages, rc, err, err_cap);
    *launches = (int32_t) stages.size();
    return 0;
}
// the handle is being freed under a live scheduler: the scheduler forgets it (no device memory is the scheduler's own)
void sched_dev_orphan(SchedDev *d) { d->m = nullptr; }
void sched_dev_free(SchedDev *d) {
    if (!d) return;
    if (d->m) d->m->sched = nullptr;
    delete d;
}

// the slots bound the greedy loops' way on every stage, the table on the last stage; after a (re)bind every word is the host's to push
static int sched_bind(SchedDev *d, const std::vector<llamahip_model *> &stages, char *err, size_t err_cap) {
    llamahip_model *first = stages[0], *last = stages.back();
    bool bound = first->mq_tok != nullptr && last->mq_tok != nullptr;
    for (llamahip_model *st : stages)
        for (int i = 0; i < d->max_active && bound; i++)
            bound = i < (int) st->slots.size() && st->slots[i].bound && (st != first || st->slots[i].token_in == first->mq_tok + i) &&
                    (st != last || st->slots[i].token_out == last->mq_tok + i);
    if (!bound) {
        const std::vector<int32_t> zero((size_t) d->max_active, 0);
        const int rc = multi_begin(stages, 1, d->max_active, zero.data(), zero.data(), err, err_cap);
        if (rc) return rc;
        d->stale = true;
    }
    if (!last->d_sched_tab) {
        HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(last->own.alloc(&last->d_sched_tab, (size_t) SCHED_TAB_WORDS), LLAMAHIP_ERR_PREDICT);
    }
    return 0;
}
// every scheduler slot's {position, cursor} to every stage, its token to the first and the last stage's token words; the hosts' position mirrors
static int sched_push_words(SchedDev *d, const std::vector<llamahip_model *> &stages, char *err, size_t err_cap) {
    int32_t w[2 * SET_MAX];
    for (int i = 0; i < d->max_active; i++) { w[2 * i] = d->pos[i]; w[2 * i + 1] = d->cur[i]; }
    for (llamahip_model *st : stages) {
        HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipMemcpy(st->d_slot_state, w, (size_t) d->max_active * 8, hipMemcpyHostToDevice), LLAMAHIP_ERR_PREDICT);
        if (st == stages[0] || st == stages.back()) HIP_TRY(hipMemcpy(st->mq_tok, d->tok, (size_t) d->max_active * 4, hipMemcpyHostToDevice), LLAMAHIP_ERR_PREDICT);
        for (int i = 0; i < d->max_active; i++) st->slots[i].next_pos = d->pos[i];
    }
    d->stale = false;
    return 0;
}

static int sched_fallback_step(SchedDev *d, SchedSeg *segs, int n_segs, const SampleParams &sp, char *err, size_t err_cap) {
    llamahip_model *m = d->m;
    const int V = m->hp.n_vocab;
    d->logits.resize((size_t) V);
    for (int j = 0; j < n_segs; j++) {
        SchedSeg &g = segs[j];
        const int rc = each_slot(m, 1, &g.slot, err, err_cap, [&](int) {
            int r = 0;
            if (g.cst && g.emit) {
                // a constrained segment: the contract's own loop -- the eval (a decode row: the one-token llamahip_eval), the host pick
                r = g.n_out == 0 && d->chunk > 0 ? llamahip_eval_chunks(m, d->n_threads, g.pos, g.tokens, g.n_rows, d->chunk, d->logits.data(), err, err_cap)
                                                 : llamahip_eval(m, d->n_threads, g.pos, g.tokens, g.n_rows, d->logits.data(), err, err_cap);
                if (r) return r;
                g.exact = 1;
                g.token = llamahip_constraint_pick(g.cst, g.cst_state, d->logits.data());
                if (g.token < 0) { set_err(err, err_cap, "llamahip_sched_step: state %d of slot %d's constraint allows no token (the state does not come from this constraint)", g.cst_state, g.slot); return LLAMAHIP_ERR_PREDICT; }
                return 0;
            }
            if (g.n_rows == 1 && g.emit && g.pos > 0 && g.n_out > 0) {          // a decode row: the contract's single-token step
                if (!g.sampler) { g.exact = 1; return llamahip_decode_greedy(m, d->n_threads, g.pos, g.tokens[0], 1, &g.token, nullptr, err, err_cap); }
                return sample_single_step(m, d->n_threads, g.pos, g.tokens[0], g.sampler, sp, d->win, d->logits, &g.token, &g.exact, err, err_cap);
            }
            float *lo = g.emit ? d->logits.data() : nullptr;
            r = d->chunk > 0 ? llamahip_eval_chunks(m, d->n_threads, g.pos, g.tokens, g.n_rows, d->chunk, lo, err, err_cap)
                             : llamahip_eval(m, d->n_threads, g.pos, g.tokens, g.n_rows, lo, err, err_cap);
            if (r || !g.emit) return r;
            if (g.sampler) { g.token = sample_draw(m, g.sampler, sp, false, nullptr, nullptr, lo, &g.exact); return 0; }
            const int32_t one = 1;
            g.exact = 1;
            return llamahip_op_sched_pick(lo, 1, V, &one, &g.token, err, err_cap);          // (the device's pick rule, not restated here)
        });
        if (rc) return rc;
    }
    return 0;
}

int sched_dev_step(SchedDev *d, SchedSeg *segs, int32_t n_segs, bool mixed, int32_t *kind, int32_t *captures, char *err, size_t err_cap) {
    static const char *fn = "llamahip_sched_step";
    llamahip_model *m = d->m;
    *captures = 0;
    if (!m) { set_err(err, err_cap, "%s: the scheduler's model handle has been freed", fn); return LLAMAHIP_ERR_PREDICT; }
    if (n_segs < 1 || n_segs > SET_MAX) { set_err(err, err_cap, "%s: %d segments in a step (1 .. %d)", fn, n_segs, SET_MAX); return LLAMAHIP_ERR_PREDICT; }
    const int C = m->hp.n_ctx, V = m->hp.n_vocab;
    int64_t R = 0;
    int n_logit_rows = 0;
    bool drafted = false, constrained = false;
    for (int j = 0; j < n_segs; j++) {
        const SchedSeg &g = segs[j];
        if (g.slot < 0 || g.slot >= d->max_active || g.n_rows < 1 || g.pos < 0 || g.pos + g.n_rows > C || !g.tokens || (!mixed && (g.n_rows != 1 || !g.emit))) {
            set_err(err, err_cap, "%s: segment %d (slot %d, %d rows at %d) is outside the scheduler's slots or the context (n_ctx %d)", fn, j, g.slot, g.n_rows, g.pos, C);
            return LLAMAHIP_ERR_PREDICT;
        }
        if (g.n_draft < 0 || g.n_draft > VERIFY_ROWS_MAX - 1 || (g.n_draft > 0 && (!g.draft || g.n_rows != 1 || !g.emit || g.pos + 1 + g.n_draft > C))) {
            set_err(err, err_cap, "%s: segment %d (slot %d at %d) carries a draft of %d tokens (0 .. %d behind one decode row, inside n_ctx %d)", fn, j, g.slot, g.pos, g.n_draft, VERIFY_ROWS_MAX - 1, C);
            return LLAMAHIP_ERR_PREDICT;
        }
        for (int i = 0; i < g.n_draft; i++)
            if (g.draft[i] < 0 || g.draft[i] >= V) { set_err(err, err_cap, "%s: draft token id %d out of range [0, %d)", fn, g.draft[i], V); return LLAMAHIP_ERR_PREDICT; }
        for (int i = 0; i < j; i++) if (segs[i].slot == g.slot) { set_err(err, err_cap, "%s: slot %d has two segments in one step", fn, g.slot); return LLAMAHIP_ERR_PREDICT; }
        if (g.cst && (!g.emit || g.sampler || g.cst->m != m || !m->stages.empty() || g.cst_state < 0 || g.cst_state >= g.cst->n_states)) {
            set_err(err, err_cap, "%s: segment %d (slot %d) carries a constraint it cannot take (state %d; a greedy emitting segment of the constraint's own whole-model handle)", fn, j, g.slot, g.cst_state);
            return LLAMAHIP_ERR_PREDICT;
        }
        R += g.n_rows + g.n_draft;
        drafted = drafted || g.n_draft > 0;
        constrained = constrained || g.cst != nullptr;
        n_logit_rows += g.emit ? 1 + g.n_draft : 0;
    }
    if (drafted && n_logit_rows > VERIFY_ROWS_MAX) { set_err(err, err_cap, "%s: %d logits rows in a step with drafted tokens (at most %d)", fn, n_logit_rows, VERIFY_ROWS_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (R > LLAMAHIP_EVAL_MULTI_MAX_ROWS) { set_err(err, err_cap, "%s: %lld rows in one step, more than LLAMAHIP_EVAL_MULTI_MAX_ROWS (%d)", fn, (long long) R, LLAMAHIP_EVAL_MULTI_MAX_ROWS); return LLAMAHIP_ERR_PREDICT; }
    const std::vector<llamahip_model *> stages = stages_of(m);
    const int S = (int) stages.size();
    llamahip_model *first = stages[0], *last = stages[S - 1];
    const SampleParams sp = sample_params(m, d->repeat_penalty, d->top_k, d->top_p, d->temp);
    sched_decide(d);
    if (drafted && (d->fallback || !mixed)) { set_err(err, err_cap, "%s: a draft on a step or a handle that takes none", fn); return LLAMAHIP_ERR_PREDICT; }
    const double t0 = now_ms();
    if (d->fallback) {
        *kind = SCHED_STEP_FALLBACK;
        return sched_fallback_step(d, segs, n_segs, sp, err, err_cap);
    }
    int rc = sched_bind(d, stages, err, err_cap);
    if (rc) return rc;
    int64_t cap0 = 0;
    for (llamahip_model *st : stages) cap0 += st->n_set_captures;
    bool any_sampled = false;
    for (int j = 0; j < n_segs; j++) any_sampled = any_sampled || (segs[j].sampler && segs[j].emit);
    if (any_sampled) {
        if ((rc = sample_prepare(last, true, err, err_cap)) != 0) return rc;
        if (first != last && (rc = sample_prepare(first, false, err, err_cap)) != 0) return rc;
    }
    const llamahip_model::SampleIo &hl = last->smp_h;
    // a step with constrained segments: the tables on the device; the allow-list and the fallback token (the constraint's stop token) of every
    // logits row, filled where the rows are laid out.  A step without one launches exactly what it launched before
    DfaMaskRows allow = {};
    DfaFallback fb = {};
    int dead_at[SET_MAX], pick_at[SET_MAX];
    if (constrained) {
        HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
        for (int j = 0; j < n_segs; j++) if (segs[j].cst && (rc = cst_ensure_dev(m, segs[j].cst, err, err_cap)) != 0) return rc;
    }
    int order[SET_MAX], n_ord = 0;          // the step's rows: segment order[a] is row a of the logits
    if (mixed) {
        *kind = SCHED_STEP_MIXED;
        // the sampled segments that emit first: their logits rows are rows [0, ns), their windows and candidates index a of the pinned block
        for (int j = 0; j < n_segs; j++) if (segs[j].sampler && segs[j].emit) order[n_ord++] = j;
        const int ns = n_ord;
        for (int j = 0; j < n_segs; j++) if (!(segs[j].sampler && segs[j].emit)) order[n_ord++] = j;
        int32_t slots[SET_MAX], n_past[SET_MAX], n_tokens[SET_MAX], tab[4 * SET_MAX];
        // a drafted step: k_sched_accept's table and the logits rows' tokens (one upload), each segment's first logits row, the sampled rows' id pool
        int32_t acc[SCHED_TAB_W * SET_MAX + VERIFY_ROWS_MAX] = { 0 }, lrow0[SET_MAX] = { 0 }, *ltok = acc + SCHED_TAB_W * SET_MAX;
        int nl = 0, ns_rows = 0;
        std::vector<int32_t> tokens;
        tokens.reserve((size_t) R);
        RowsPass rp;
        for (int a = 0; a < n_segs; a++) {
            const SchedSeg &g = segs[order[a]];
            slots[a] = g.slot; n_past[a] = g.pos; n_tokens[a] = g.n_rows + g.n_draft;
            const int r0 = (int) tokens.size();
            tokens.insert(tokens.end(), g.tokens, g.tokens + g.n_rows);
            tokens.insert(tokens.end(), g.draft, g.draft + g.n_draft);
            tab[4 * a] = g.emit && !g.sampler; tab[4 * a + 1] = g.slot; tab[4 * a + 2] = g.pos + g.n_rows; tab[4 * a + 3] = g.n_out + (g.emit ? 1 : 0);
            if (!drafted) {
                if (g.cst) { allow.row[a] = g.cst->dev + (size_t) g.cst_state * V; fb.t[a] = g.cst->stop_token; }
                if (a < ns) hl.n_last[a] = llamahip_sampler_window(g.sampler, hl.win + (size_t) a * 1024, 1024);          // (the streams are idle: every step is waited for)
                continue;
            }
            // every row of a segment with a draft has a logits row, the last row of every other emitting segment, none of the rest.  A sampled
            // segment's words cannot be set by the device (the host draws): emit 0 with the words of a segment without a draft, the host's push follows
            rp.seg_single.push_back(g.n_draft > 0);
            lrow0[a] = nl;
            int32_t *t = acc + SCHED_TAB_W * a;
            t[0] = !g.emit || g.sampler ? 0 : g.n_draft > 0 ? 2 : 1; t[1] = g.slot; t[2] = g.pos; t[3] = g.n_out + (g.emit && g.sampler ? 1 : 0);
            t[4] = nl; t[5] = n_tokens[a];
            // (a constrained segment's logits row i is picked under the state behind the draft tokens in front of it)
            int32_t cs = g.cst ? g.cst_state : -1;
            for (int r = g.n_draft > 0 ? r0 : r0 + g.n_rows - 1, i = 0; g.emit && r < r0 + n_tokens[a]; r++, i++) {
                if (g.cst) {
                    if (cs < 0) { set_err(err, err_cap, "%s: draft token %d of slot %d is banned in its constraint's state", fn, g.draft[i - 1], g.slot); return LLAMAHIP_ERR_PREDICT; }
                    allow.row[nl] = g.cst->dev + (size_t) cs * V; fb.t[nl] = g.cst->stop_token;
                    if (i < g.n_draft) cs = llamahip_constraint_advance(g.cst, cs, g.draft[i]);
                }
                ltok[nl++] = tokens[(size_t) r]; rp.logit_rows.push_back(r);
            }
            if (a < ns) ns_rows = nl;
        }
        rp.n_seqs = n_segs; rp.chunk = d->chunk; rp.slots = slots; rp.n_past = n_past; rp.n_tokens = n_tokens; rp.R = (int) R;
        if (rows_pass_build(rp, C) != 0) { set_err(err, err_cap, "%s: the row table could not be built", fn); return LLAMAHIP_ERR_PREDICT; }
        // the sampled segments' id streams (drafted step): each segment slides inside its own -- its sampler's window, then its draft
        TopkOut cand[VERIFY_ROWS_MAX];
        bool seg_sel[SET_MAX] = { false };
        SlideSetReq ss;
        if (drafted && ns > 0) {
            VsetReq rq;
            llamahip_sampler *smp[SET_MAX];
            rq.n_segs = ns; rq.n_rows = ns_rows;
            for (int a = 0; a < ns; a++) { rq.seg_begin[a] = lrow0[a]; rq.slot[a] = slots[a]; rq.pos[a] = n_past[a]; smp[a] = segs[order[a]].sampler; }
            rq.seg_begin[ns] = ns_rows;
            memcpy(rq.rows, ltok, (size_t) ns_rows * 4);
            d->pool.resize(SLIDE_SET_IDS);
            slide_set_build(rq, smp, sp, d->pool.data(), cand, ss, seg_sel);
        }
        HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
        // (pageable: the table has left the host array when the call returns)
        if (!drafted) HIP_TRY(hipMemcpyAsync(last->d_sched_tab, tab, (size_t) n_segs * 16, hipMemcpyHostToDevice, last->stream), LLAMAHIP_ERR_PREDICT);
        else HIP_TRY(hipMemcpyAsync(last->d_sched_tab + SCHED_ACC_TAB, acc, sizeof(acc), hipMemcpyHostToDevice, last->stream), LLAMAHIP_ERR_PREDICT);
        int32_t *d_res = last->h_io ? last->d_io->vset.res : last->d_sched_tab + (drafted ? SCHED_ACC_RES : 4 * SET_MAX);
        rc = rows_pass_enqueue(stages, d->n_threads, rp, tokens.data(), err, err_cap);
        if (rc == 0 && hipSetDevice(last->device) != hipSuccess) { set_err(err, err_cap, "%s: hipSetDevice failed", fn); rc = LLAMAHIP_ERR_PREDICT; }
        if (rc == 0 && ns > 0) rc = drafted ? slide_set_enqueue(last, ss, ns_rows, err, err_cap) : sample_select(last, sp, 0, ns, err, err_cap);
        int32_t *d_dead = last->h_io ? last->d_io->vset.pick : last->d_sched_tab + SCHED_ACC_DEAD;          // (a constrained drafted step's dead words)
        if (rc == 0 && !drafted && (constrained ? launch_sched_pick_dfa(last->logits, n_segs, V, last->d_sched_tab, allow, fb, last->d_slot_state, last->d_slot_trace, C, last->mq_tok, d_res, last->stream)
                                                : launch_sched_pick(last->logits, n_segs, V, last->d_sched_tab, last->d_slot_state, last->d_slot_trace, C, last->mq_tok, d_res, last->stream)) != hipSuccess) {
            set_err(err, err_cap, "%s: HIP error launching k_sched_pick", fn); rc = LLAMAHIP_ERR_PREDICT;
        }
        if (rc == 0 && drafted && ((constrained ? launch_verify_rows_dfa(last->logits, nl, V, allow, fb, last->d_sched_tab + SCHED_ACC_PICK, d_dead, last->stream)
                                                : launch_verify_rows(last->logits, nl, V, last->d_sched_tab + SCHED_ACC_PICK, last->stream)) != hipSuccess ||
                                   launch_sched_accept(last->d_sched_tab + SCHED_ACC_PICK, last->d_sched_tab + SCHED_ACC_TOK, last->d_sched_tab + SCHED_ACC_TAB, n_segs, nl,
                                                       last->d_slot_state, last->d_slot_trace, C, last->mq_tok, d_res, last->stream) != hipSuccess)) {
            set_err(err, err_cap, "%s: HIP error launching k_verify_rows / k_sched_accept", fn); rc = LLAMAHIP_ERR_PREDICT;
        }
        if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
        HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
        int32_t res[SET_MAX + VERIFY_ROWS_MAX], dead[VERIFY_ROWS_MAX] = { 0 };
        const size_t n_res = (size_t) n_segs + (drafted ? (size_t) nl : constrained ? (size_t) n_segs : 0);
        if (last->h_io) memcpy(res, last->h_io->vset.res, n_res * 4);
        else HIP_TRY(hipMemcpy(res, d_res, n_res * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
        if (constrained && drafted) {
            if (last->h_io) memcpy(dead, last->h_io->vset.pick, (size_t) nl * 4);
            else HIP_TRY(hipMemcpy(dead, d_dead, (size_t) nl * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
        } else if (constrained) memcpy(dead, res + n_segs, (size_t) n_segs * 4);
        for (int r = 0; constrained && r < (drafted ? nl : n_segs); r++)
            if (dead[r] != 0) { set_err(err, err_cap, "%s: a pick found no allowed token (logits row %d): the state does not come from the request's constraint", fn, r); return LLAMAHIP_ERR_PREDICT; }
        if (drafted && ns > 0 && ss.k > 0 && (rc = slide_fetch(last, cand, ns_rows, err, err_cap)) != 0) return rc;
        for (int a = 0; a < n_segs; a++) {
            SchedSeg &g = segs[order[a]];
            g.n_accept = 0;
            if (drafted && g.emit && !g.sampler) {
                g.n_accept = res[a];
                if (g.n_accept < 0 || g.n_accept > g.n_draft) { set_err(err, err_cap, "%s: the device reported %d accepted of %d drafted tokens for slot %d", fn, g.n_accept, g.n_draft, g.slot); return LLAMAHIP_ERR_PREDICT; }
                for (int i = 0; i <= g.n_accept; i++) { g.toks[i] = res[n_segs + lrow0[a] + i]; g.exacts[i] = 1; }
                g.token = g.toks[0]; g.exact = 1;
            } else if (drafted && g.emit) {
                // llamahip_verify_sample_multi's walk: draw, accept, go on only while the draw is the draft's next token
                if ((rc = sample_walk(m, last, lrow0[a], g.draft, g.n_draft, g.sampler, seg_sel[a], cand, sp, &g.n_accept, g.toks, g.exacts, d->logits, err, err_cap)) != 0) return rc;
                g.token = g.toks[0]; g.exact = g.exacts[0];
                if (g.n_draft > 0) d->stale = true;          // (the device could not know the draws: the words are the host's to push)
            } else if (g.emit && !g.sampler) { g.token = res[a]; g.exact = 1; }
            else if (g.emit) {
                const TopkOut &c = hl.out[a];
                g.token = sample_draw(m, g.sampler, sp, sp.dev_sel && c.fl[0] == 1, c.sc, c.id, hl.spill + (size_t) a * V, &g.exact);
            }
            d->pos[g.slot] = g.pos + (g.n_draft > 0 ? g.n_accept + 1 : g.n_rows); d->cur[g.slot] = g.n_out + (g.emit ? g.n_accept + 1 : 0);
            if (g.emit) d->tok[g.slot] = g.n_draft > 0 ? g.toks[g.n_accept] : g.token;
            for (llamahip_model *st : stages) st->slots[g.slot].next_pos = d->pos[g.slot];
        }
        if (S > 1) d->stale = true;          // (k_sched_pick / k_sched_accept set the last stage's words only)
        last->last_rows.clear();
        m->last_rows.clear();
        m->n_evals++;
    } else {
        // a set orders its rows by slot id: row a of the step = the a-th slot in ascending order
        for (int j = 0; j < n_segs; j++) order[n_ord++] = j;
        std::sort(order, order + n_segs, [&](int x, int y) { return segs[x].slot < segs[y].slot; });
        int32_t act[SET_MAX];
        for (int a = 0; a < n_segs; a++) {
            const SchedSeg &g = segs[order[a]];
            act[a] = g.slot;
            if (d->pos[g.slot] != g.pos || d->tok[g.slot] != g.tokens[0]) { d->pos[g.slot] = g.pos; d->cur[g.slot] = g.n_out; d->tok[g.slot] = g.tokens[0]; d->stale = true; }
            if (any_sampled) hl.n_last[a] = g.sampler ? llamahip_sampler_window(g.sampler, hl.win + (size_t) a * 1024, 1024) : 0;
        }
        if (d->stale) { if ((rc = sched_push_words(d, stages, err, err_cap)) != 0) return rc; }
        else if (any_sampled) {
            // a sampled request's token word holds the step's greedy pick: the host writes the draws over them -- the mirror holds every
            // slot's token (a greedy slot's is what the device put there), so the whole array goes up in one copy
            HIP_TRY(hipSetDevice(first->device), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(hipMemcpy(first->mq_tok, d->tok, (size_t) d->max_active * 4, hipMemcpyHostToDevice), LLAMAHIP_ERR_PREDICT);
        }
        *kind = n_segs >= 2 ? SCHED_STEP_SET : SCHED_STEP_SINGLE;
        // constrained slots: the step exactly as it is, then ONE k_sched_pick_dfa launch over the step's logits rows (one per row where the
        // slots are stepped one by one) with the advanced {position, cursor} in its table -- it overwrites the trace entry and the next-token
        // word the step's own tail wrote, as llamahip_decode_greedy_constrained_multi does with k_pick_dfa's repick.  The stage step's tail
        // (k_argmax / k_argmax_set) only stores its pick: nothing has read the token word before the next step's embedding gather, which
        // runs behind this launch on the same stream.  Unconstrained rows emit nothing here: what the tail wrote stands
        int32_t *d_res = last->h_io ? last->d_io->vset.res : last->d_sched_tab + 4 * SET_MAX;
        if (constrained) {
            int32_t tab[4 * SET_MAX];
            for (int a = 0; a < n_segs; a++) {
                const SchedSeg &g = segs[order[a]];
                tab[4 * a] = g.cst ? 1 : 0; tab[4 * a + 1] = g.slot; tab[4 * a + 2] = g.pos + 1; tab[4 * a + 3] = g.n_out + 1;
                if (g.cst) { allow.row[a] = g.cst->dev + (size_t) g.cst_state * V; fb.t[a] = g.cst->stop_token; }
            }
            HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(hipMemcpyAsync(last->d_sched_tab, tab, (size_t) n_segs * 16, hipMemcpyHostToDevice, last->stream), LLAMAHIP_ERR_PREDICT);      // (pageable: gone when the call returns)
        }
        const std::function<int(int, int)> hook = [&](int j, int rows) -> int {
            if (any_sampled) { const int r = sample_select(last, sp, j, rows, err, err_cap); if (r) return r; }
            if (!constrained) return 0;
            DfaMaskRows al = {};
            DfaFallback f = {};
            for (int r = 0; r < rows; r++) { al.row[r] = allow.row[j + r]; f.t[r] = fb.t[j + r]; pick_at[j + r] = 2 * j + r; dead_at[j + r] = 2 * j + rows + r; }
            if (launch_sched_pick_dfa(last->logits, rows, V, last->d_sched_tab + 4 * j, al, f, last->d_slot_state, last->d_slot_trace, C, last->mq_tok, d_res + 2 * j, last->stream) != hipSuccess) {
                set_err(err, err_cap, "%s: HIP error launching k_sched_pick_dfa", fn); return LLAMAHIP_ERR_PREDICT;
            }
            return 0;
        };
        rc = step_group(stages, { act, n_segs, 0, d->max_active, 0 }, d->n_threads, false, true, any_sampled || constrained ? hook : nullptr, err, err_cap);
        if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
        HIP_TRY(hipSetDevice(last->device), LLAMAHIP_ERR_PREDICT);
        int32_t words[SET_MAX];
        HIP_TRY(hipMemcpy(words, last->mq_tok, (size_t) d->max_active * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
        if (constrained) {
            int32_t res[2 * SET_MAX];
            if (last->h_io) memcpy(res, last->h_io->vset.res, sizeof(res));
            else HIP_TRY(hipMemcpy(res, d_res, sizeof(res), hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
            for (int a = 0; a < n_segs; a++) {
                const SchedSeg &g = segs[order[a]];
                if (g.cst && (res[dead_at[a]] != 0 || res[pick_at[a]] != words[g.slot])) {
                    set_err(err, err_cap, "%s: a pick found no allowed token (slot %d, state %d): the state does not come from the request's constraint", fn, g.slot, g.cst_state);
                    return LLAMAHIP_ERR_PREDICT;
                }
            }
        }
        for (int a = 0; a < n_segs; a++) {
            SchedSeg &g = segs[order[a]];
            if (!g.sampler) { g.token = words[g.slot]; g.exact = 1; }
            else {
                const TopkOut &c = hl.out[a];
                g.token = sample_draw(m, g.sampler, sp, sp.dev_sel && c.fl[0] == 1, c.sc, c.id, hl.spill + (size_t) a * V, &g.exact);
            }
            d->pos[g.slot] = g.pos + 1; d->cur[g.slot] = g.n_out + 1; d->tok[g.slot] = g.token;
        }
        if (!m->stages.empty()) m->pipe_hand_off = 1;
    }
    for (llamahip_model *st : stages) cap0 -= st->n_set_captures;
    *captures = (int32_t) -cap0;
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}
}  // namespace lh
}  // extern "C++"

int llamahip_set_seq(llamahip_model *m, int32_t seq, char *err, size_t err_cap) {
    if (!m || seq < 0 || seq >= m->n_seq) { set_err(err, err_cap, "sequence slot %d out of range [0, %d)", seq, m ? m->n_seq : 0); return LLAMAHIP_ERR_PREDICT; }
    m->cur_seq = seq;
    for (llamahip_model *st : m->stages) st->cur_seq = seq;
    return LLAMAHIP_OK;
}

// the arguments first (a HOST_ONLY handle knows n_ctx and n_seq: the checks are the same without a device), then the handle, then its scheduler
static int kv_copy_check(llamahip_model *m, int32_t n_copies, const int32_t *src_slot, const int32_t *dst_slot, const int32_t *row_begin, const int32_t *n_rows,
                         lh::KvCopyTab &tab, const char *fn, char *err, size_t err_cap) {
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    const int C = m->hp.n_ctx, n_seq = first_of(m)->n_seq;
    if (n_copies < 1 || n_copies > LLAMAHIP_KV_COPY_MAX) { set_err(err, err_cap, "%s: n_copies (%d) outside 1 .. %d", fn, n_copies, LLAMAHIP_KV_COPY_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (!src_slot || !dst_slot || !row_begin || !n_rows) { set_err(err, err_cap, "%s: null array", fn); return LLAMAHIP_ERR_PREDICT; }
    tab = {};
    tab.n = n_copies;
    for (int i = 0; i < n_copies; i++) {
        if (src_slot[i] < 0 || src_slot[i] >= n_seq || dst_slot[i] < 0 || dst_slot[i] >= n_seq) {
            set_err(err, err_cap, "%s: copy %d from slot %d to slot %d: slot out of range [0, %d) (llamahip_opts.n_seq)", fn, i, src_slot[i], dst_slot[i], n_seq);
            return LLAMAHIP_ERR_PREDICT;
        }
        if (src_slot[i] == dst_slot[i]) { set_err(err, err_cap, "%s: copy %d: source and destination are the same slot (%d)", fn, i, src_slot[i]); return LLAMAHIP_ERR_PREDICT; }
        if (n_rows[i] < 0 || row_begin[i] < 0 || (int64_t) row_begin[i] + n_rows[i] > C) {
            set_err(err, err_cap, "%s: copy %d: rows [%d, %d + %d) outside [0, n_ctx (%d)]", fn, i, row_begin[i], row_begin[i], n_rows[i], C);
            return LLAMAHIP_ERR_PREDICT;
        }
        tab.src[i] = src_slot[i]; tab.dst[i] = dst_slot[i]; tab.row_begin[i] = row_begin[i]; tab.n_rows[i] = n_rows[i];
    }
    for (int i = 0; i < n_copies; i++)
        for (int o = 0; o < n_copies; o++)
            if (o != i && (dst_slot[i] == src_slot[o] || dst_slot[i] == dst_slot[o])) {
                set_err(err, err_cap, "%s: slot %d is the destination of copy %d and the %s of copy %d: a destination takes part in one copy of a call", fn, dst_slot[i], i,
                        dst_slot[i] == src_slot[o] ? "source" : "destination", o);
                return LLAMAHIP_ERR_PREDICT;
            }
    const int rc = lh::decode_handle_check(m, fn, err, err_cap);
    if (rc) return rc;
    if (m->sched)
        for (int i = 0; i < n_copies; i++)
            if (dst_slot[i] < lh::sched_dev_max_active(m->sched)) {
                set_err(err, err_cap, "%s: copy %d writes slot %d, which belongs to the handle's live scheduler (slots below its max_active, %d)", fn, i, dst_slot[i], lh::sched_dev_max_active(m->sched));
                return LLAMAHIP_ERR_PREDICT;
            }
    return 0;
}

int llamahip_kv_copy_rows(llamahip_model *m, int32_t n_copies, const int32_t *src_slot, const int32_t *dst_slot, const int32_t *row_begin,
                          const int32_t *n_rows, char *err, size_t err_cap) {
    static const char *fn = "llamahip_kv_copy_rows";
    lh::KvCopyTab tab;
    int rc = kv_copy_check(m, n_copies, src_slot, dst_slot, row_begin, n_rows, tab, fn, err, err_cap);
    if (rc) return rc;
    const std::vector<llamahip_model *> stages = stages_of(m);
    const double t0 = now_ms();
    rc = lh::kv_copy_enqueue(stages, tab, fn, err, err_cap);
    if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}

int llamahip_bench_kv_copy(llamahip_model *m, int32_t n_copies, const int32_t *src_slot, const int32_t *dst_slot, const int32_t *row_begin,
                           const int32_t *n_rows, int32_t how, int32_t iters, double *ms_per_call, char *err, size_t err_cap) {
    static const char *fn = "llamahip_bench_kv_copy";
    lh::KvCopyTab tab;
    int rc = kv_copy_check(m, n_copies, src_slot, dst_slot, row_begin, n_rows, tab, fn, err, err_cap);
    if (rc) return rc;
    if (!m->stages.empty() || iters < 1 || (how != 0 && how != 1) || !ms_per_call) { set_err(err, err_cap, "%s: a plain handle, iters >= 1, how 0 or 1", fn); return LLAMAHIP_ERR_PREDICT; }
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    const size_t d = m->hp.n_embd, layer = (size_t) m->hp.n_ctx * d, L = (size_t) (m->l1 - m->l0);
    double t0 = 0;
    for (int it = -1; it < iters; it++) {          // (it == -1: untimed)
        if (it == 0) t0 = now_ms();
        if (how == 0) rc = lh::kv_copy_enqueue({ m }, tab, fn, err, err_cap);
        else
            for (int c = 0; c < tab.n && rc == 0; c++)
                for (size_t il = 0; il < L && rc == 0 && tab.n_rows[c] > 0; il++)
                    for (float *base : { m->Kc, m->Vc }) {
                        const size_t in_slot = il * layer + (size_t) tab.row_begin[c] * d;
                        if (hipMemcpyAsync(base + (size_t) tab.dst[c] * L * layer + in_slot, base + (size_t) tab.src[c] * L * layer + in_slot, (size_t) tab.n_rows[c] * d * 4,
                                           hipMemcpyDeviceToDevice, m->stream) != hipSuccess) { set_err(err, err_cap, "%s: hipMemcpyAsync failed", fn); rc = LLAMAHIP_ERR_PREDICT; break; }
                    }
        if ((rc = drain_stages({ m }, rc, err, err_cap)) != 0) return rc;
    }
    *ms_per_call = (now_ms() - t0) / iters;
    return LLAMAHIP_OK;
}

static_assert(LLAMAHIP_KV_SHIFT_MAX == lh::KV_SHIFT_MAX && LLAMAHIP_KV_SHIFT_ROWS_IN_FLIGHT == lh::KV_SHIFT_U, "llamahip.h mirrors k_kv_shift_rows' limits");

// what llamahip_kv_shift_rows and llamahip_op_kv_shift refuse of a table of shifts, one set of messages (host_util.h); slots_of: what bounds the slots
extern "C++" int lh::kv_shift_table_check(int32_t n_slots, const char *slots_of, int32_t n_ctx, int32_t n_shifts, const int32_t *slot, const int32_t *row_begin, const int32_t *n_rows,
                             const int32_t *n_discard, KvShiftTab &tab, const char *fn, char *err, size_t err_cap) {
    if (n_shifts < 1 || n_shifts > LLAMAHIP_KV_SHIFT_MAX) { set_err(err, err_cap, "%s: n_shifts (%d) outside 1 .. %d", fn, n_shifts, LLAMAHIP_KV_SHIFT_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (!slot || !row_begin || !n_rows || !n_discard) { set_err(err, err_cap, "%s: null array", fn); return LLAMAHIP_ERR_PREDICT; }
    tab = {};
    tab.n = n_shifts;
    for (int i = 0; i < n_shifts; i++) {
        if (slot[i] < 0 || slot[i] >= n_slots) { set_err(err, err_cap, "%s: shift %d: slot %d out of range [0, %d)%s", fn, i, slot[i], n_slots, slots_of); return LLAMAHIP_ERR_PREDICT; }
        for (int o = 0; o < i; o++)
            if (slot[o] == slot[i]) { set_err(err, err_cap, "%s: slot %d is shifted by shift %d and by shift %d: a slot takes part in one shift of a call", fn, slot[i], o, i); return LLAMAHIP_ERR_PREDICT; }
        if (n_discard[i] < 1) { set_err(err, err_cap, "%s: shift %d: n_discard (%d) must be >= 1", fn, i, n_discard[i]); return LLAMAHIP_ERR_PREDICT; }
        if (n_rows[i] < 0 || row_begin[i] < 0 || (int64_t) row_begin[i] + n_rows[i] > n_ctx) {
            set_err(err, err_cap, "%s: shift %d: rows [%d, %d + %d) outside [0, n_ctx (%d)]", fn, i, row_begin[i], row_begin[i], n_rows[i], n_ctx);
            return LLAMAHIP_ERR_PREDICT;
        }
        if (row_begin[i] < n_discard[i]) {
            set_err(err, err_cap, "%s: shift %d: rows moved down from %d by n_discard %d would begin below row 0, outside [0, n_ctx (%d)]", fn, i, row_begin[i], n_discard[i], n_ctx);
            return LLAMAHIP_ERR_PREDICT;
        }
        tab.slot[i] = slot[i]; tab.row_begin[i] = row_begin[i]; tab.n_rows[i] = n_rows[i]; tab.n_discard[i] = n_discard[i];
    }
    return 0;
}

// llamahip_kv_copy_rows' order: the arguments, then the handle, then its scheduler
static int kv_shift_check(llamahip_model *m, int32_t n_shifts, const int32_t *slot, const int32_t *row_begin, const int32_t *n_rows, const int32_t *n_discard,
                          lh::KvShiftTab &tab, const char *fn, char *err, size_t err_cap) {
    if (!m) { set_err(err, err_cap, "%s: null model", fn); return LLAMAHIP_ERR_PREDICT; }
    int rc = lh::kv_shift_table_check(first_of(m)->n_seq, " (llamahip_opts.n_seq)", m->hp.n_ctx, n_shifts, slot, row_begin, n_rows, n_discard, tab, fn, err, err_cap);
    if (rc) return rc;
    if ((rc = lh::decode_handle_check(m, fn, err, err_cap)) != 0) return rc;
    if (m->sched)
        for (int i = 0; i < n_shifts; i++)
            if (slot[i] < lh::sched_dev_max_active(m->sched)) {
                set_err(err, err_cap, "%s: shift %d writes slot %d, which belongs to the handle's live scheduler (slots below its max_active, %d)", fn, i, slot[i], lh::sched_dev_max_active(m->sched));
                return LLAMAHIP_ERR_PREDICT;
            }
    return 0;
}
// one k_kv_shift_rows launch per stage, each on its own device and stream, with the stage's own angle table; nothing is waited for
static int kv_shift_enqueue(const std::vector<llamahip_model *> &stages, const lh::KvShiftTab &tab, const char *fn, char *err, size_t err_cap) {
    for (llamahip_model *st : stages) {
        HIP_TRY(hipSetDevice(st->device), LLAMAHIP_ERR_PREDICT);
        if (lh::launch_kv_shift_rows(st->Kc, st->Vc, st->sincos, tab, st->n_seq, st->l1 - st->l0, st->hp.n_ctx, st->hp.n_embd, st->hp.n_embd / st->hp.n_head, st->stream) != hipSuccess) {
            set_err(err, err_cap, "%s: HIP error launching k_kv_shift_rows on device %d", fn, st->device);
            return LLAMAHIP_ERR_PREDICT;
        }
    }
    return 0;
}

int32_t llamahip_cur_seq(const llamahip_model *m) { return m ? m->cur_seq : -1; }

int llamahip_kv_shift_rows(llamahip_model *m, int32_t n_shifts, const int32_t *slot, const int32_t *row_begin, const int32_t *n_rows,
                           const int32_t *n_discard, char *err, size_t err_cap) {
    static const char *fn = "llamahip_kv_shift_rows";
    lh::KvShiftTab tab;
    int rc = kv_shift_check(m, n_shifts, slot, row_begin, n_rows, n_discard, tab, fn, err, err_cap);
    if (rc) return rc;
    const std::vector<llamahip_model *> stages = stages_of(m);
    const double t0 = now_ms();
    rc = kv_shift_enqueue(stages, tab, fn, err, err_cap);
    if ((rc = drain_stages(stages, rc, err, err_cap)) != 0) return rc;
    m->t_eval_ms += now_ms() - t0;
    return LLAMAHIP_OK;
}

int llamahip_bench_kv_shift(llamahip_model *m, int32_t n_shifts, const int32_t *slot, const int32_t *row_begin, const int32_t *n_rows,
                            const int32_t *n_discard, int32_t iters, double *ms_per_launch, char *err, size_t err_cap) {
    static const char *fn = "llamahip_bench_kv_shift";
    lh::KvShiftTab tab;
    int rc = kv_shift_check(m, n_shifts, slot, row_begin, n_rows, n_discard, tab, fn, err, err_cap);
    if (rc) return rc;
    if (!m->stages.empty() || iters < 1 || !ms_per_launch) {
        set_err(err, err_cap, "%s: a plain handle, iters >= 1", fn);
        return LLAMAHIP_ERR_PREDICT;
    }
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    Events evs;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(evs.create(&e0), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(evs.create(&e1), LLAMAHIP_ERR_PREDICT);
    // whatever fails once a launch is enqueued, the stream is drained before the call returns
    auto record = [&](hipEvent_t ev) {
        if (hipEventRecord(ev, m->stream) == hipSuccess) return 0;
        (void) hipGetLastError();
        set_err(err, err_cap, "%s: hipEventRecord failed", fn);
        return (int) LLAMAHIP_ERR_PREDICT;
    };
    for (int it = -1; it < iters && rc == 0; it++) {          // (it == -1: untimed)
        if (it == 0) rc = record(e0);
        if (rc == 0) rc = kv_shift_enqueue({ m }, tab, fn, err, err_cap);
    }
    if (rc == 0) rc = record(e1);
    if ((rc = drain_stages({ m }, rc, err, err_cap)) != 0) return rc;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1), LLAMAHIP_ERR_PREDICT);
    *ms_per_launch = (double) ms / iters;
    return LLAMAHIP_OK;
}

int llamahip_kv_read(llamahip_model *m, int32_t il, int32_t n_pos, float *out_k, float *out_v, char *err, size_t err_cap) {
    if (m) for (llamahip_model *st : m->stages) if (il >= st->l0 && il < st->l1) return llamahip_kv_read(st, il, n_pos, out_k, out_v, err, err_cap);
    if (!m || m->host_only || il < m->l0 || il >= m->l1 || n_pos < 0 || n_pos > m->hp.n_ctx) { set_err(err, err_cap, "bad kv_read arguments"); return LLAMAHIP_ERR_PREDICT; }
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    const size_t d = m->hp.n_embd, off = ((size_t) m->cur_seq * (m->l1 - m->l0) + (il - m->l0)) * m->hp.n_ctx * d;
    HIP_TRY(hipMemcpy(out_k, m->Kc + off, (size_t) n_pos * d * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipMemcpy(out_v, m->Vc + off, (size_t) n_pos * d * 4, hipMemcpyDeviceToHost), LLAMAHIP_ERR_PREDICT);
    return LLAMAHIP_OK;
}

int64_t llamahip_tensor_bytes(llamahip_model *m, const char *name, void *out, int64_t cap) {
    if (!m || !name) return -1;
    auto it = m->file.tensors.find(name);
    if (it == m->file.tensors.end()) return -1;
    const int64_t n = it->second.nbytes();
    if (out && cap >= n) {
        std::string e;
        if (!m->file.read_tensor(name, (uint8_t *) out, e)) return -1;
    }
    return n;
}

// Phase-timing probe: arms the in-kernel s_memtime probe of k_gemv, runs `n_steps` greedy decode steps
// (graph replay, i.e. the real decode loop) and returns one record of 8 uint64 per GEMV launch:
// {entry, loads issued, prologue done, weights consumed, exit, ngroups, nchunks, PRE*16+EPI}.
// Returns the number of records written (<= cap).  Measurement tooling only.
int64_t llamahip_debug_decode_phases(llamahip_model *m, int32_t n_past, int32_t first_token, int32_t n_steps,
                                     uint64_t *records, int64_t cap, char *err, size_t err_cap) {
    if (!m || m->host_only || cap < 1) { set_err(err, err_cap, "bad arguments"); return -1; }
    if (hipSetDevice(m->device) != hipSuccess) return -1;
    DevOwner probe;                      // the records' buffer, for the length of this call
    unsigned long long *d_buf = nullptr;
    const size_t bytes = (size_t) (cap + 1) * 8 * sizeof(unsigned long long);
    if (probe.alloc(&d_buf, (size_t) (cap + 1) * 8, true) != 0) return -1;
    const unsigned long long hdr[2] = { 0, (unsigned long long) cap };
    (void) hipMemcpy(d_buf, hdr, sizeof(hdr), hipMemcpyHostToDevice);
    // warm the graph / caches first, unprobed
    std::vector<int32_t> toks(n_steps);
    int rc = llamahip_decode_greedy(m, 8, n_past, first_token, n_steps, toks.data(), nullptr, err, err_cap);
    if (rc == 0) {
        (void) set_phase_probe(d_buf);
        rc = llamahip_decode_greedy(m, 8, n_past, first_token, n_steps, toks.data(), nullptr, err, err_cap);
        (void) set_phase_probe(nullptr);
    }
    int64_t n = -1;
    if (rc == 0) {
        std::vector<unsigned long long> h((size_t) (cap + 1) * 8);
        if (hipMemcpy(h.data(), d_buf, bytes, hipMemcpyDeviceToHost) == hipSuccess) {
            n = (int64_t) std::min<unsigned long long>(h[0], (unsigned long long) cap);
            for (int64_t i = 0; i < n * 8; i++) records[i] = h[8 + i];
        }
    }
    return n;
}

// live registrations of every DevOwner of the process (handles, their slots and set descriptors, the single-op calls' scratch) and their
// bytes: what a leak check compares before and after (free device memory as the runtime reports it says nothing on a shared card)
void llamahip_debug_live_allocs(int64_t *n, int64_t *bytes) {
    if (n) *n = DevOwner::live_n.load();
    if (bytes) *bytes = DevOwner::live_bytes.load();
}

int32_t llamahip_debug_lut_math(void) { return g_lut_math; }

// Phase records of the few-row kernel (k_gemv_set; libllamahip_setprobe.so built with -DLH_SET_PROBE=1 and LLAMAHIP_SET_PROBE=<capacity>):
// copies up to `cap` records of 32 words and optionally clears the buffer.  Returns the number of records.  Measurement tooling only.
int64_t llamahip_debug_set_probe(uint64_t *records, int64_t cap, int32_t reset) {
    return (int64_t) set_probe_dump((unsigned long long *) records, (long) cap, reset != 0);
}

int32_t llamahip_debug_set_plan(int32_t m, int32_t k, int32_t interleaved, int32_t n_rows, int32_t epi, int64_t out[5]) {
    long o[5] = { 0, 0, 0, 0, 0 };
    if (m < 1 || k < 1 || !out || !gemv_set_plan_query(m, k, interleaved != 0, n_rows, epi, o)) return 0;
    for (int i = 0; i < 5; i++) out[i] = o[i];
    return 1;
}

int32_t llamahip_debug_gemv_plan(int32_t m, int32_t k, int32_t interleaved, int32_t pre, int32_t epi, int64_t out[6]) {
    if (m < 1 || k < 1 || !out) return 0;
    QMat w;
    w.set_shape(m, k);
    if (interleaved) w.gmapF8 = m / 16;
    const GemvPlan p = gemv_plan(w, pre, epi);
    if (!p.nw) return 0;
    const int64_t o[6] = { p.nw, p.pg, p.depth, p.ring, p.grid, (int64_t) p.lds };
    for (int i = 0; i < 6; i++) out[i] = o[i];
    return gemv_plan_has_kernel(pre, epi, p) ? 1 : -1;
}

int32_t llamahip_debug_gemm_paths(int64_t *out, int32_t cap) {
    for (int i = 0; out && i < cap && i < GEMM_PATH_COUNT; i++) out[i] = g_gemm_path_counts[i];
    return GEMM_PATH_COUNT;
}

int32_t llamahip_debug_dense_paths(int64_t *out, int32_t cap) {
    for (int i = 0; out && i < cap && i < DENSE_COUNT_N; i++) out[i] = g_dense_path_counts[i];
    return DENSE_COUNT_N;
}

int32_t llamahip_debug_dense_set_plan(int32_t m, int32_t k, int32_t wtype, int32_t n_rows, int64_t out[6]) {
    if (!out) return 0;
    const DenseSetPlan p = dense_set_plan(m, k, wtype, n_rows);
    if (!p.nr) return 0;
    const int64_t o[6] = { p.grid, p.hw * 32, p.rg, p.nr, p.slab, p.lds };
    for (int i = 0; i < 6; i++) out[i] = o[i];
    return dense_set_plan_has_kernel(p) ? 1 : -1;
}

int32_t llamahip_debug_q41_paths(int64_t *out, int32_t cap) {
    for (int i = 0; out && i < cap && i < Q41_COUNT_N; i++) out[i] = g_q41_path_counts[i];
    return Q41_COUNT_N;
}

int32_t llamahip_debug_q41_plan(int32_t m, int32_t k, int32_t n_rows, int64_t out[8]) {
    if (!out) return 0;
    const Q41Plan p = q41_plan(m, k, n_rows);
    if (!p.nr) return 0;
    const int64_t o[8] = { p.nr, p.rows, p.threads, p.grid_x, p.grid_y, p.slab, p.lds, p.chain };
    for (int i = 0; i < 8; i++) out[i] = o[i];
    return q41_plan_has_kernel(p) ? 1 : -1;
}

int32_t llamahip_debug_dense_mfma_plan(int32_t m, int32_t k, int32_t wtype, int32_t n_rows, int64_t out[6]) {
    if (!out) return 0;
    const DenseMfmaPlan p = dense_mfma_plan(m, k, wtype, n_rows);
    if (!p.ok) return 0;
    const int64_t o[6] = { (int64_t) p.grid_x * p.grid_y, p.threads, p.tile_rows, p.tile_cols, p.lds, p.auto_pick };
    for (int i = 0; i < 6; i++) out[i] = o[i];
    return dense_mfma_plan_has_kernel(p) ? 1 : -1;
}

int64_t llamahip_debug_dense_mfma_launches(void) { return g_dense_mfma_launches; }

int32_t llamahip_debug_dense_force(int32_t path) {
    if (path != 0 && path != LLAMAHIP_DENSE_MM && path != LLAMAHIP_DENSE_MFMA) return -1;
    const int32_t prev = g_dense_force;
    g_dense_force = path;
    return prev;
}

int llamahip_get_stats(const llamahip_model *m, llamahip_stats *out) {
    if (!m || !out) return LLAMAHIP_ERR_UNKNOWN;
    out->struct_size = (int32_t) sizeof(*out);
    out->weight_bytes_device = m->weight_bytes;
    out->kv_bytes_device = m->kv_bytes;
    out->n_evals = m->n_evals;
    out->t_load_ms = m->t_load_ms;
    out->t_eval_ms_total = m->t_eval_ms;
    for (const llamahip_model *st : m->stages) { out->weight_bytes_device += st->weight_bytes; out->kv_bytes_device += st->kv_bytes; }
    out->n_stages = m->stages.empty() ? 1 : (int32_t) m->stages.size();
    out->hand_off = m->pipe_hand_off;
    return LLAMAHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// the decode mat-vec on its own, timed (the single-op entry points llamahip_op_* are ops.cpp)
// ------------------------------------------------------------------------------------------------
int llamahip_bench_gemv(llamahip_model *m, int32_t which, int32_t layer, int32_t warmup, int32_t iters,
                        llamahip_gemv_bench *out, char *err, size_t err_cap) {
    if (!m || m->host_only || !out || iters < 1) { set_err(err, err_cap, "bad bench arguments"); return LLAMAHIP_ERR_PREDICT; }
    HIP_TRY(hipSetDevice(m->device), LLAMAHIP_ERR_PREDICT);
    // layer < 0: cycle over every resident layer so consecutive launches stream DIFFERENT weights
    // from HBM (one cycle of the smallest 7B matrix kind is 336 MB > the 256 MB Infinity Cache)
    const int variant = which >> 4;          // 0 QA/STORE (probe), 1 NORM/STORE, 2 NORM/SILU_QA, 3 QA/SILU_QA: prologue / epilogue ablation
    which &= 15;
    std::vector<const QMat *> mats;
    std::vector<const float *> norms;
    auto pick = [&](const Layer &L) -> const QMat * {
        norms.push_back(which == 2 ? L.ffn_norm : L.attention_norm);
        return which == 0 ? &L.qkv : which == 1 ? &L.wo : which == 2 ? &L.w13 : which == 3 ? &L.w2 : nullptr;
    };
    if (which == 4) { if (m->last_stage) mats.push_back(&m->output); }
    else if (which >= 0 && which < 4) {
        if (layer < 0) for (const Layer &L : m->layers) mats.push_back(pick(L));
        else if (layer >= m->l0 && layer < m->l1) mats.push_back(pick(m->layers[layer - m->l0]));
    }
    if (mats.empty()) { set_err(err, err_cap, "no such matrix (which=%d layer=%d)", which, layer); return LLAMAHIP_ERR_PREDICT; }
    const QMat *q = mats[0];
    int rc = ensure_workspace(m, 1, err, err_cap);
    if (rc) return rc;
    // a deterministic activation row, quantized once; the timed region is the decode GEMV kernel alone
    std::vector<float> hx(q->K);
    for (int i = 0; i < q->K; i++) hx[i] = (float) ((i * 2654435761u) >> 8 & 0xFFFF) / 32768.0f - 1.0f;
    HIP_TRY(hipMemcpyAsync(m->tmp, hx.data(), (size_t) q->K * 4, hipMemcpyHostToDevice, m->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(launch_prep(PREP_PLAIN, m->tmp, nullptr, q->K, 0, q->K, 1, m->qa_A, m->qa_d, nullptr, nullptr, m->T_silu, m->stream), LLAMAHIP_ERR_PREDICT);
    HIP_TRY(hipStreamSynchronize(m->stream), LLAMAHIP_ERR_PREDICT);
    float *yout = which == 4 ? m->logits : m->gu;     // gu (2F floats) is large enough for every layer matrix
    if (variant && (which == 4 || (variant >= 2 && which != 2) || (variant == 1 && which != 0 && which != 2))) { set_err(err, err_cap, "variant %d does not apply to matrix %d", variant, which); return LLAMAHIP_ERR_PREDICT; }
    size_t ri = 0;
    auto run = [&](const QMat *w) {
        const float *nw_ = norms.empty() ? nullptr : norms[ri++ % norms.size()];
        switch (variant) {
        case 1:  return launch_gemv(*w, PREP_NORM, EPI_STORE, nullptr, nullptr, m->tmp, nw_, yout, nullptr, m->T_silu, nullptr, nullptr, m->stream);
        case 2:  return launch_gemv(*w, PREP_NORM, EPI_SILU_QA, nullptr, nullptr, m->tmp, nw_, nullptr, nullptr, m->T_silu, m->qa2_A, m->qa2_d, m->stream);
        case 3:  return launch_gemv(*w, PRE_QA, EPI_SILU_QA, m->qa_A, m->qa_d, nullptr, nullptr, nullptr, nullptr, m->T_silu, m->qa2_A, m->qa2_d, m->stream);
        default: return launch_gemv(*w, PRE_QA, EPI_STORE, m->qa_A, m->qa_d, nullptr, nullptr, yout, nullptr, m->T_silu, nullptr, nullptr, m->stream);
        }
    };
    Scratch ev;              // destroys the events on every return
    const hipEvent_t e0 = ev.event(), e1 = ev.event();
    if (!ev.ok()) return ev.fail("llamahip_bench_gemv", err, err_cap);
    float ms_total = 0;
    int launches = 0;
    if (which == 4 && !m->layers.empty()) {
        // a single 82 MB matrix would be served from the Infinity Cache when re-launched: evict it
        // between timed launches by streaming > 256 MB of other weights (untimed)
        for (int it = 0; it < warmup + iters; it++) {
            size_t flushed = 0;
            for (const Layer &L : m->layers) {
                HIP_TRY(launch_gemv(L.w13, PRE_QA, EPI_STORE, m->qa_A, m->qa_d, nullptr, nullptr, m->gu, nullptr, m->T_silu, nullptr, nullptr, m->stream), LLAMAHIP_ERR_PREDICT);
                flushed += L.w13.bytes();
                if (flushed > (size_t) 400 << 20) break;
            }
            HIP_TRY(hipEventRecord(e0, m->stream), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(run(q), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(hipEventRecord(e1, m->stream), LLAMAHIP_ERR_PREDICT);
            HIP_TRY(hipEventSynchronize(e1), LLAMAHIP_ERR_PREDICT);
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, e0, e1), LLAMAHIP_ERR_PREDICT);
            if (it >= warmup) { ms_total += ms; launches++; }
        }
    } else {
        for (int it = 0; it < warmup; it++) for (const QMat *w : mats) HIP_TRY(run(w), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipEventRecord(e0, m->stream), LLAMAHIP_ERR_PREDICT);
        for (int it = 0; it < iters; it++) for (const QMat *w : mats) HIP_TRY(run(w), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipEventRecord(e1, m->stream), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipEventSynchronize(e1), LLAMAHIP_ERR_PREDICT);
        HIP_TRY(hipEventElapsedTime(&ms_total, e0, e1), LLAMAHIP_ERR_PREDICT);
        launches = iters * (int) mats.size();
    }
    out->M = q->M; out->K = q->K; out->iters = launches; out->ms_total = ms_total;
    out->algo_bytes = (double) q->M * (q->K / 32) * 20 + (double) (q->K / 32) * 20 + 4.0 * q->M;
    return LLAMAHIP_OK;
}

}  // extern "C"
