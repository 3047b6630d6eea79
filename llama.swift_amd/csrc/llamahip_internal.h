// llamahip_internal.h -- shared between the HIP kernels (kernels.hip) and the C-ABI host code.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "dec_attn_plan.h"
#include "q41_plan.h"
#include "set_plan.h"

namespace lh {

constexpr int MT4_TILE_BYTES = 4608;   // k_gemm_mfma4's weight tile: 32 rows x 4 Q4_0 blocks, one byte per weight + 128 fp32 scales
constexpr int TILE_BYTES = 1280;   // 8 rows x 8 Q4_0 blocks: 1024 B nibbles + 64 fp32 scales

// activation-preparation modes (also the fused-prologue selector of k_gemv)
// (PREP_NORMP: PREP_NORM with the row's {sum x, sum x^2} supplied by its producer -- k_gemv only, selected by launch_gemv)
// (the *_TAG forms: the operand arrives / the result leaves as 8-byte {fp32 bits, tag} granules that the consumer polls -- the
//  hand-offs inside k_qkv_attn, and the residual-stream row between pipeline stages through a device-side mailbox)
enum { PRE_QA = 0, PREP_PLAIN = 1, PREP_NORM = 2, PREP_SILU_MUL = 3, PREP_NORMP = 4, PREP_NORM_TAG = 6 };
enum { EPI_STORE = 0, EPI_RESID = 1, EPI_SILU_QA = 2, EPI_ROPE_KV = 3, EPI_STORE_TAG = 4, EPI_RESID_TAG = 5, EPI_STORE_PICK = 6, EPI_SILU_QAH = 7 };
// The rows of a BATCHED decode step (llamahip_stage_step_set): row b is the next token of sequence slot b' -- its own position (device
// resident, so a captured step replays unchanged), its own KV cache, its own token / pick / residual-stream buffers.  Lives in device
// memory; kernels that take a `const SeqSet *` treat null as "one sequence, consecutive positions" (the prompt-chunk meaning).
constexpr int SET_MAX = 16;
struct SeqSet {
    int32_t *state[SET_MAX];            // {position, step} of the row's slot
    const int32_t *tok_in[SET_MAX];     // first stage: where the row's token is read
    int32_t *tok_out[SET_MAX];          // last stage: where the greedy pick goes (may be null)
    int32_t *trace[SET_MAX];            // last stage: the slot's list of picks
    const float *hid_in[SET_MAX];       // stages after the first: the row of the residual stream coming in
    float *hid_out[SET_MAX];            // stages before the last: ... going out
    long kv_off[SET_MAX];               // elements from slot 0's KV cache to the row's slot's
    int32_t pos[SET_MAX];               // the rows' positions of THIS step (= *state[i]), gathered by the step's first launch (k_embed_set / k_rows_set): one
                                        // load instead of a pointer chase at the tail of the wq|wk|wv launch (written by the device, every step)
    int n;
};
// The score launch of a set step covers the key slices up to the set's highest position, in buckets of SET_KEY_BUCKET positions: what
// launch_attn_short takes as set_keys (max_pos < set_keys <= n_ctx).  Host only; llamahip_debug_set_keys reports it.
constexpr int SET_KEY_BUCKET = 128;
inline int set_key_bucket(int n_ctx, int max_pos) { const int k = (max_pos / SET_KEY_BUCKET + 1) * SET_KEY_BUCKET; return k < n_ctx ? k : n_ctx; }
// operands of the EPI_ROPE_KV epilogue (short evals, wq|wk|wv): rotate q / k, append k / v to the cache
// (set: row n is at position set->state[n][0] of the cache at Kc / Vc + set->kv_off[n] instead of n_past + n)
struct RopeKvArgs { const double *tab; float *qr, *Kc, *Vc; int n_past, d, dh; const SeqSet *set = nullptr; };
// what the half-block w1|w3 epilogue of k_gemv_set needs (EPI_SILU_QAH): granules for the partial amaxes, the epoch word its tags are made from
struct SiluHalfIO { uint64_t *amax_t = nullptr; const uint32_t *epoch = nullptr; int layer = 0; uint32_t *fault = nullptr; };

// a Q4_0 weight matrix resident in HBM in chain-major tile layout
struct QMat {
    uint8_t *tiles = nullptr;   // ngroups * (nchunks + 1) * TILE_BYTES; the last tile of a row-group is all-zero
    int M = 0, K = 0;           // logical rows / columns
    int ngroups = 0;            // ceil(M / 8)
    int nchunks = 0;            // ceil(K / 256)
    int gmapF8 = 0;             // F/8 for the interleaved w1|w3 matrix, else 0 (see k_repack_q4)
    // optional second copy for the prompt path: row-lane tiles, nrb * (nchunks + 1) * 10240 B (see k_gemm_rows);
    // rows are in LOGICAL order here (no w1|w3 interleave)
    uint8_t *rows = nullptr;
    int nrb = 0;                // ceil(M / 64)
    // optional third copy for long prompts: MFMA tiles, nrb32 * (2 * nchunks) * 2560 B (see k_gemm_mfma)
    uint8_t *mt = nullptr;      // int8 operand order (the opt-in fast path and LLAMAHIP_MFMA_I8)
    uint8_t *mt4 = nullptr;     // one byte per weight, four-chain operand order (k_gemm_mfma4: the exact path): nrb32 * (2 * nchunks) * 4608 B
    int nrb32 = 0;              // ceil(M / 32)
    // the tile geometry of an M x K matrix, every copy's (the one place that derives it)
    void set_shape(int m, int k) { M = m; K = k; ngroups = (M + 7) / 8; nchunks = (K + 255) / 256; nrb = (M + 63) / 64; nrb32 = (M + 31) / 32; }
    size_t mt_bytes() const { return (size_t) nrb32 * nchunks * 2 * 2560; }
    size_t mt4_bytes() const { return (size_t) nrb32 * nchunks * 2 * MT4_TILE_BYTES; }
    size_t rows_bytes() const { return (size_t) nrb * (nchunks + 1) * 10240; }
    size_t bytes() const { return (size_t) ngroups * (nchunks + 1) * TILE_BYTES; }
    int Kp() const { return nchunks * 256; }
};

// an f16 / f32 weight matrix (file layout: row-major [M][K]) of a dense model file (dense.hip)
struct DMat {
    void *w = nullptr;          // fp32 / fp16: the rows; Q4_1: {min, d} pairs [row-block of 64][block][lane] -- the one resident copy,
    void *w2 = nullptr;         // Q4_1: the 16 nibble bytes in the same order             read by k_q41_chain and k_q41_mm alike
    int M = 0, K = 0;
    int wtype = 0;              // 0 fp32, 1 fp16, 3 Q4_1
    size_t bytes() const { return wtype == 3 ? (size_t) ((M + 63) / 64) * 64 * (K / 32) * 8 : (size_t) M * K * (wtype == 1 ? 2 : 4); }
    size_t bytes2() const { return wtype == 3 ? (size_t) ((M + 63) / 64) * 64 * (K / 32) * 16 : 0; }
};
// The f16 / f32 mat-mul kernels (dense.hip), = LLAMAHIP_DENSE_* of llamahip.h: k_dense_mv (one row; forced with more rows: one launch per row),
// k_dense_mm (any row count, the rows on gridDim.y: the weights are streamed once per 8 rows), k_dense_set (1 .. 16 rows, the weights streamed
// once), k_dense_mfma (more than 16 rows, K a multiple of 128: the chains on the fp32 matrix cores, the weights streamed once per 64 rows).
// AUTO: one row MV, more by dense_auto_path (dense.hip).  Q4_1 ignores this path: launch_q41_mm and Q41_PATH_* below.
enum { DENSE_PATH_AUTO = 0, DENSE_PATH_MV = 1, DENSE_PATH_MM = 2, DENSE_PATH_SET = 3, DENSE_PATH_MFMA = 4 };
enum { DENSE_COUNT_MV = 0, DENSE_COUNT_MM = 1, DENSE_COUNT_SET = 2, DENSE_COUNT_N = 3 };
extern long g_dense_path_counts[DENSE_COUNT_N];      // launches per kernel (process-wide; tests)
constexpr int DENSE_SET_MAX_ROWS = 16;
// k_dense_set's launch plan: nr = the compiled row count the launch runs (0: the kernel does not take the shape), hw half-waves per workgroup
// of rg weight rows each, grid, slab = groups of 256 elements per activation row and LDS buffer, lds = static LDS bytes
struct DenseSetPlan { int nr, hw, rg, grid, slab, lds; };
DenseSetPlan dense_set_plan(int M, int K, int wtype, int N);
bool dense_set_plan_has_kernel(const DenseSetPlan &p);
// k_dense_mfma's launch plan: ok = the kernel takes the shape; grid (grid_x, grid_y) workgroups of `threads`, each tile_rows activation rows x
// tile_cols weight rows; lds = dynamic LDS bytes; auto_pick = AUTO takes the kernel at this row count (the measured rule)
struct DenseMfmaPlan { int ok, grid_x, grid_y, threads, tile_rows, tile_cols, lds, auto_pick; };
constexpr int DENSE_MFMA_K_UNIT = 128;               // K: whole groups of 256 elements plus at most one 4-step group
constexpr int DENSE_MFMA_AUTO_MIN_ROWS = 64;             // AUTO: k_dense_mfma from this many rows
constexpr int DENSE_ONE_PASS_MIN_ROWS = 36;          // llamahip_eval_chunks / _eval_logprobs on f16 / f32 files: one pass from this many rows
DenseMfmaPlan dense_mfma_plan(int M, int K, int wtype, int N);
bool dense_mfma_plan_has_kernel(const DenseMfmaPlan &p);
extern long g_dense_mfma_launches;                   // launches of k_dense_mfma (process-wide; tests)
extern int g_dense_force;                            // llamahip_debug_dense_force: 0, DENSE_PATH_MM or DENSE_PATH_MFMA for more than 16 rows
hipError_t init_attrs_dense();
// scratch: N * K floats (the permuted / rounded activation operand; Q4_1: the expanded one)
hipError_t launch_dense_mm(const DMat &w, int epi, const float *x, long x_stride, int N, float *y, long y_stride,
                           const float *resid, long resid_stride, hipStream_t st, float *scratch = nullptr,
                           int path = DENSE_PATH_AUTO, int *path_taken = nullptr);
hipError_t launch_q41_repack(const uint8_t *raw_rows, DMat &w, hipStream_t st);
// Q4_1 mat-mul: the paths, counters and k_q41_chain's launch plan are q41_plan.h's (host-only); scratch: N * K floats, the expanded operand
hipError_t launch_q41_mm(const DMat &w, int epi, const float *x, long x_stride, int N, float *y, long y_stride,
                         const float *resid, long resid_stride, hipStream_t st, float *scratch, int path, int *path_taken);
bool dense_prep_applies(int wtype, int mode, int K);
hipError_t launch_dense_prep(int mode, int wtype, const float *in0, const float *in1, long in_stride, long in1_stride,
                             int K, int N, float *scratch, const uint16_t *T_silu, hipStream_t st);
hipError_t launch_dense_perm_act(int wtype, const float *x, long x_stride, int K, int N, float *xp, hipStream_t st);
// which producer writes an f16 / f32 mat-mul's operand rows (dense.hip launch_dense_act), = LLAMAHIP_DENSE_PREP_* of llamahip.h
enum { DENSE_PREP_AUTO = 0, DENSE_PREP_FUSED = 1, DENSE_PREP_SPLIT = 2 };
int dense_prep_kernel(int kernel, int wtype, int mode, int K);      // the producer that runs, -1: refused
hipError_t launch_dense_act(int kernel, int mode, int wtype, const float *in0, const float *in1, long in_stride, long in1_stride, int K, int N,
                            float *xp, float *rows, uint32_t *qa_A, float *qa_d, const uint16_t *T_silu, hipStream_t st, int *taken = nullptr);
hipError_t launch_dense_perm_rows(const void *raw_rows, DMat &w, int row0, int rows, hipStream_t st);
hipError_t launch_quantize_q41_offline(const void *src, int f16, uint8_t *dst, long nrows, int nb, hipStream_t st);
hipError_t launch_embed_dense(const int32_t *tokens, const void *emb, int wtype, float *x, int d, int N, hipStream_t st);
// a batched decode step on an f16 / f32 file: the rows' embedding (+ SeqSet::pos, the step's first launch) and k_rope_kv per row of the set
hipError_t launch_embed_dense_set(SeqSet *set, int n, const void *emb, int wtype, float *x, int d, hipStream_t st);
hipError_t launch_rope_kv_set(const float *qkv, long qkv_stride, int d, int dh, const double *tab, float *qr, float *Kc, float *Vc,
                              const SeqSet *set, int N, hipStream_t st);

hipError_t init_kernel_attrs();
size_t prep_lds_bytes(int K);                                       // dynamic LDS of the LDS-staged activation preparation (prep.hip)
// exhaustive check (all 65 536 entries) that the device's double-precision formulas reproduce the host-built SiLU /
// exp tables; enables the gather-free paths of the decode kernels when they do (g_lut_math)
extern int g_lut_math;
hipError_t launch_check_lut_math(const uint16_t *T_silu, const uint16_t *T_exp, hipStream_t st);
hipError_t set_phase_probe(unsigned long long *dev_buf);

hipError_t launch_add(const float *a, const float *b, float *c, long n, hipStream_t st);
hipError_t launch_repack(const uint8_t *src_aos, uint8_t *dst, int M, int K, int gmap, int goff, hipStream_t st);
hipError_t launch_tiles_to_rows(const QMat &w, hipStream_t st);   // w.rows / w.nrb set by the caller
hipError_t launch_tiles_to_mtiles(const QMat &w, hipStream_t st); // w.mt / w.nrb32 set by the caller
hipError_t launch_tiles_to_mt4(const QMat &w, hipStream_t st);    // w.mt4 / w.nrb32 set by the caller
hipError_t launch_embed(const int32_t *tokens, const uint8_t *emb, float *x, int d, int N, hipStream_t st);
// The rule of launch_prep: the register-resident k_prep_fast unless a side output (y_out / raw_out) is wanted or a NORM row is wider than
// one workgroup's 1024 half-blocks; else the LDS-staged k_prep_qa.  force (llamahip_op_prep: per-op tests of both kernels on one shape):
// PREP_FORCE_FAST is refused with hipErrorInvalidValue where the rule's conditions for k_prep_fast do not hold; nothing is launched then.
// *launched (may be null): PREP_FORCE_FAST or PREP_FORCE_LDS, set on the branch that launches.
enum { PREP_FORCE_AUTO = 0, PREP_FORCE_FAST = 1, PREP_FORCE_LDS = 2 };      // = LLAMAHIP_PREP_KERNEL_* of llamahip.h
bool prep_fast_applies(int mode, int K, bool side_output);
hipError_t launch_prep(int mode, const float *in0, const float *in1, long in_stride, long in1_stride, int K, int N,
                       uint32_t *qa_A, float *qa_d, float *y_out, uint8_t *raw_out, const uint16_t *T_silu,
                       hipStream_t st, int force = PREP_FORCE_AUTO, int *launched = nullptr);
// Norm statistics handed from the producer of a residual-stream row to the norm-fused mat-vec that reads it
// (decode only): an EPI_RESID launch with `out` set writes one {sum y, sum y^2} pair of doubles per workgroup
// (gemv_resid_parts(w) of them); a PREP_NORM launch with `in` / `n_in` set folds them instead of reducing the
// row itself.  n_in <= NORM_PART_MAX.
constexpr int NORM_PART_MAX = 512;
struct NormPart { const double *in = nullptr; int n_in = 0; double *out = nullptr; };
// Pipeline mailbox on one side of a decode launch: the residual-stream row as tagged 8-byte granules in memory the NEIGHBOUR stage
// reads / writes (peer-mapped).  Tags are made from the sequence position (*pos_w + 1), which both stages know.
struct MailboxIO {
    const uint64_t *in_t = nullptr;      // the row the first layer's wq|wk|wv launch normalises arrives here ...
    const uint64_t *resid_t = nullptr;   // ... and the same granules are the residual operand of the first layer's wo launch
    uint64_t *out_t = nullptr;           // the last layer's w2 launch stores its row here (the next stage's inbox)
    const int32_t *pos_w = nullptr;      // device word holding the position (the slot's st[0])
    uint32_t *epoch = nullptr, *fault = nullptr;
    int test_bits = 0;                   // 0x1000 short polls, 0x2000 wrong tag on out_t (fault-injection tests)
};
// EPI_STORE_PICK (the lm head of the device-resident greedy loop): the launch that writes the logits also picks the token (k_argmax's
// rule: the largest value, the LOWEST index on ties, NaN never wins) -- every workgroup folds its rows into one 64-bit atomic max, the
// last workgroup to finish records the pick, advances the position and embeds the picked token for the next step (k_embed_part's
// arithmetic: row, {sum x, sum x^2}, epoch bump), so a decode step has no single-workgroup launches left.
struct PickIO {
    unsigned long long *key; uint32_t *count;       // key: one slot per workgroup of the launch; count: 8 shard tickets (16 dwords apart) + the top ticket at [128]; zeroed once, re-zeroed by the last workgroup
    int32_t *out; int32_t *next_token; int32_t *state;      // as launch_argmax: out[state[1]] = pick, *next_token = pick, state advances
    const uint8_t *emb; float *x_next; double *part_next; uint32_t *epoch; int n_vocab;      // the next step's embedding row
};
int gemv_resid_parts(const QMat &w);
// The launch plan of the single-row decode mat-vec (decode.hip gemv_plan, the one rule every launcher and predicate below derives from):
// waves per workgroup, operand granules per thread, ring depth, ring or whole row in flight, grid, dynamic LDS bytes.
struct GemvPlan { int nw, pg, depth; bool ring; int grid; size_t lds; };   // nw == 0: the kernel does not take this (matrix, pre, epi)
GemvPlan gemv_plan(const QMat &w, int pre, int epi);
bool gemv_plan_has_kernel(int pre, int epi, const GemvPlan &p);      // the plan names an instance of k_gemv that exists
// LLAMAHIP_NORM_MODE, read in one place: resolves (*pre, *np) to the prologue to launch (PREP_NORM / PREP_NORMP) and the kernel's
// part_in / npart; returns whether the mode is the default (pre == null: that question alone)
bool norm_mode_resolve(int *pre = nullptr, NormPart *np = nullptr);
// EPI_SILU_QAH: the w1|w3 decode mat-vec in HALF-block workgroups (4 waves: 16 gate rows + the same 16 up rows).  The 8-wave workgroups of
// EPI_SILU_QA are F / 32 = 344 on 256 CUs at 7B: 88 CUs stream two workgroups' weights, the others one, and a CU's load path bounds what
// it can pull -- the launch ends with a third of the chip streaming alone.  688 half-block workgroups spread 3 / 2 per CU.  The two halves
// of a Q4_0 activation block sit 8 blocks apart in the grid (one XCD: xcd_selftest) and exchange their partial amax as one tagged granule
// each way (fmaxf is exact in any order), then each writes its 16-bit halves of the block's eight QA dwords.
bool gemv_silu_half_applies(const QMat &w);
hipError_t launch_gemv_silu_half(const QMat &w, const float *in0, const float *in1, const uint16_t *T_silu, uint32_t *out_A, float *out_d, hipStream_t st,
                                 const NormPart *np, uint64_t *amax_t, uint32_t *epoch, int layer, uint32_t *fault);
bool gemv_pick_applies(const QMat &w);
hipError_t launch_gemv_pick(const QMat &w, const float *in0, const float *in1, float *y, const uint16_t *T_silu, hipStream_t st,
                            const NormPart *np, const PickIO &pick);
hipError_t launch_gemv(const QMat &w, int pre, int epi, const uint32_t *qa_A, const float *qa_d,
                       const float *in0, const float *in1, float *y, const float *resid,
                       const uint16_t *T_silu, uint32_t *out_A, float *out_d, hipStream_t st,
                       const NormPart *np = nullptr, const MailboxIO *mb = nullptr);
// embedding row of ONE token (decode) + its {sum x, sum x^2} pair for the first norm (part_out[0])
hipError_t launch_embed_part(const int32_t *token, const uint8_t *emb, float *x, int d, double *part_out, hipStream_t st, uint32_t *epoch = nullptr, uint64_t *xt = nullptr,
                             const uint64_t *token_mb = nullptr, const int32_t *state = nullptr, uint32_t *fault = nullptr, int n_vocab = 0);      // token_mb: the token arrives as a mailbox granule
// (GEMM_PATH_MFMA counts every matrix-core launch, the fast kernel's too; GEMM_PATH_FAST counts the fast kernel's alone)
enum { GEMM_PATH_MFMA = 0, GEMM_PATH_ROWS = 1, GEMM_PATH_LDS = 2, GEMM_PATH_GEMV = 3, GEMM_PATH_SET = 4, GEMM_PATH_FAST = 5, GEMM_PATH_COUNT = 6 };
extern long g_gemm_path_counts[GEMM_PATH_COUNT];     // launches per kernel family of launch_gemm (process-wide; tests)
// qb_ws: scratch for the int8 operand of the matrix-core path (N * nchunks * 256 B), or nullptr
hipError_t launch_gemm(const QMat &w, int epi, const uint32_t *qa_A, const float *qa_d, int N,
                       float *y, long y_stride, const float *resid, long resid_stride, hipStream_t st,
                       uint8_t *qb_ws = nullptr, bool fast = false);
// ONE kernel family of launch_gemm, forced whatever its selection rule would pick (llamahip_op_prompt_gemm_q4_0: per-op tests of every
// prompt GEMM).  The path values are LLAMAHIP_GEMM_* of llamahip.h; EPI_STORE / EPI_RESID only.  A family that cannot take the matrix
// (its copy is missing) or the shape is refused with hipErrorInvalidValue and the limit in *why; nothing is launched then.  Counts as
// launch_gemm does.
enum { GEMM_FORCE_MFMA4 = 1, GEMM_FORCE_MFMA_I8 = 2, GEMM_FORCE_FAST = 3, GEMM_FORCE_ROWS = 4, GEMM_FORCE_SET = 5, GEMM_FORCE_LDS = 6 };
hipError_t launch_gemm_forced(int path, const QMat &w, int epi, const uint32_t *qa_A, const float *qa_d, int N,
                              float *y, long y_stride, const float *resid, long resid_stride, hipStream_t st,
                              uint8_t *qb_ws, const char **why);
hipError_t launch_rope_kv(const float *qkv, long qkv_stride, int d, int dh, const double *tab,
                          float *qr, float *Kc, float *Vc, int n_past, int N, hipStream_t st);
// workspace of the many-row prompt attention (k_attnq_*): scores [H][T_cap][NB] fp32 + per-query max / 1/sum
struct AttnWs {
    float *S = nullptr, *pmax = nullptr, *inv = nullptr, *part = nullptr;   // part: [nth_cap][H][NB][128]
    int NB = 0;        // query rows per batch (multiple of 64)
    int T_cap = 0;     // keys the workspace can hold
    int KS_cap = 0;    // key slices of the score pass
    int nth_cap = 0;   // chunks of the V*P key split the workspace can hold (larger n_threads: per-row kernel)
};
// the one shape of that workspace, the model's and llamahip_op_attention's: n_ctx keys, NB query rows per batch (0: the model's 512) ...
inline void attn_ws_shape(AttnWs &w, int n_ctx, int NB = 0) { w.NB = NB ? NB : 512; w.T_cap = n_ctx; w.KS_cap = 32; w.nth_cap = 8; }
// ... and the bytes of its four buffers for H heads
struct AttnWsBytes { size_t S, pmax, inv, part; };
inline AttnWsBytes attn_ws_bytes(const AttnWs &w, int H) {
    const size_t h = (size_t) H;
    return { h * w.T_cap * w.NB * 4, h * w.KS_cap * w.NB * 4, h * w.NB * 4, (size_t) w.nth_cap * h * w.NB * 128 * 4 };
}
hipError_t launch_attn(const float *qr, const float *Kc, const float *Vc, float *merged, float *dbg_p, float *dbg_kqv,
                       int n_past, int N, int d, int H, int nth, const uint16_t *T_exp, const AttnWs *ws, hipStream_t st,
                       int chunk = 0,        // chunk > 0: the pass stands for successive evals of `chunk` rows (prompt_attn.hip split_keys)
                       long merged_stride = 0);      // floats between merged rows (0: d)
// The model's one rule for a multi-row eval's attention (forward and llamahip_op_attention's AUTO share it): ATTN_PATH_SHORT -- rope_kv,
// then launch_attn_short (k_decn_scores + k_dec_pv_blk<true>, N <= ATTN_SHORT_MAX) -- else launch_attn, which takes the matrix-core
// chain (k_attnq_*) where attn_mfma_applies and k_attn otherwise.  ws: the eval's workspace, NB == 0 before the first multi-row eval.
constexpr int ATTN_SHORT_MAX = 60;
enum { ATTN_PATH_MFMA = 1, ATTN_PATH_ROW = 2, ATTN_PATH_SHORT = 3 };      // = LLAMAHIP_ATTN_* of llamahip.h
bool attn_mfma_applies(const AttnWs *ws, int N, int dh, int T, int nth);
bool attn_short_applies(const AttnWs *ws, int N, int dh);
int attn_path_pick(const AttnWs *ws, int N, int dh, int T, int nth);
bool gemm_rope_kv_applies(const QMat &wqkv, int N, int d);
hipError_t launch_gemm_rope_kv(const QMat &wqkv, const uint32_t *qa_A, const float *qa_d, int N, const RopeKvArgs &ra, hipStream_t st);
bool gemm_silu_qa_applies(const QMat &w13, int N);
hipError_t launch_gemm_silu_qa(const QMat &w13, const uint32_t *qa_A, const float *qa_d, int N, const uint16_t *T_silu,
                               uint32_t *out_A, float *out_d, long out_strideA, long out_strideD, hipStream_t st,
                               const SiluHalfIO *hx = nullptr);      // hx: the half-block exchange of k_gemv_set may be used (2 .. 16 rows)
// k_gemv_set (gemv_set.hip): the mat-mul for 2 .. 16 activation rows -- a batched decode step's rows, the reference's 9-token evals.  The waves
// that share a row-group share its weight bytes through LDS, so every weight byte crosses a CU's load path once per launch.
//   gemv_set_applies(w, N, epi): EPI_STORE / EPI_RESID (launch_gemv_set), EPI_ROPE_KV (launch_gemv_set_rope_kv), EPI_SILU_QAH (launch_gemv_set_silu:
//   interleaved w1|w3 in half-block workgroups whose halves exchange their partial amax per column as tagged granules -- needs the XCD
//   placement xcd_selftest confirmed, the epoch word and SET_AMAX_GRANULES(F) * 16 zeroed granules)
inline size_t set_amax_granules(int F) { return (size_t) F / 16 + 16; }      // per column
bool gemv_set_applies(const QMat &w, int N, int epi);
// (SetForce, an override of the plan's rule; the plan itself: set_plan.h)
bool gemv_set_force_check(const QMat &w, int N, int epi, const SetForce &f, char *why, size_t why_cap);      // host-only; false: the reason in why
bool gemv_set_launch_query(const QMat &w, int N, int epi, const SetForce *force, long out[7]);      // host-only: { nc, cw, ncg, rgw, LDS, grid, threads } of the launch
bool gemv_set_silu_whole_blocks(const QMat &w13, int N, bool have_exchange);      // EPI_SILU_QA (whole-block workgroups, no exchange) instead of EPI_SILU_QAH
hipError_t launch_gemv_set(const QMat &w, int epi, const uint32_t *qa_A, const float *qa_d, int N,
                           float *y, long y_stride, const float *resid, long resid_stride, hipStream_t st, const SetForce *force = nullptr);
hipError_t launch_gemv_set_rope_kv(const QMat &wqkv, const uint32_t *qa_A, const float *qa_d, int N, const RopeKvArgs &ra, hipStream_t st, const SetForce *force = nullptr);
hipError_t launch_gemv_set_silu_epi(const QMat &w13, int epi, const uint32_t *qa_A, const float *qa_d, int N, const uint16_t *T_silu,
                                    uint32_t *out_A, float *out_d, long out_strideA, long out_strideD, const SiluHalfIO &hx, hipStream_t st, const SetForce *force = nullptr);
hipError_t launch_gemv_set_silu(const QMat &w13, const uint32_t *qa_A, const float *qa_d, int N, const uint16_t *T_silu,
                                uint32_t *out_A, float *out_d, long out_strideA, long out_strideD, const SiluHalfIO &hx, hipStream_t st);
hipError_t init_attrs_gemv_set();
long set_probe_dump(unsigned long long *out, long cap_records, bool reset);      // LH_SET_PROBE builds (tools/set_timeline.py): records of 32 words
hipError_t launch_attn_short(const float *qr, const float *Kc, const float *Vc, float *sc, float *merged,
                             uint32_t *qa_A, float *qa_d, int n_past, int N, int d, int H, int n_ctx, int nth,
                             const uint16_t *T_exp, hipStream_t st, int chunk = 0, const SeqSet *set = nullptr,      // set: N independent single-row evals (batched decode step)
                             int set_keys = 0,                                                                    // ... whose positions are all < set_keys (0: n_ctx): bounds the score grid
                             long merged_stride = 0);                                                             // floats between merged rows (0: d)
// The rows of a pass over SEVERAL KV slots (rows_attn.hip; llamahip_eval_multi, llamahip_op_attention_rows): row r is at position pos of the cache
// kv_off elements behind slot 0's (SeqSet::kv_off's meaning) and splits `keys` keys over the threads in V*P (prompt_attn.hip split_keys of the
// eval the row stands for).  Built and validated on the host (eval_multi.cpp), device resident, uploaded once per pass.
struct RowTab { int32_t pos, keys; long kv_off; };
hipError_t launch_rope_kv_rows(const float *qkv, long qkv_stride, int d, int dh, const double *tab, float *qr, float *Kc, float *Vc,
                               const RowTab *rows, int R, hipStream_t st);
hipError_t launch_attn_rows(const float *qr, const float *Kc, const float *Vc, float *sc, int sc_rows, float *merged, long merged_stride,
                            uint32_t *qa_A, float *qa_d, const RowTab *rows, const int32_t *idx /* may be null */, int n_rows, int max_keys,
                            int d, int H, int n_ctx, int nth, const uint16_t *T_exp, hipStream_t st);
hipError_t launch_gather_rows(const float *x, const int32_t *idx, int n, int d, float *out, hipStream_t st);      // out row i = x row idx[i]
// batched decode step: embedding rows / residual rows in and out / greedy picks of the set's rows
// (the step's FIRST launch -- embed, or rows with gather -- also writes set->pos and, given the epoch word, opens the step's epoch)
hipError_t launch_embed_set(SeqSet *set, int n, const uint8_t *emb, float *x, int d, hipStream_t st, uint32_t *epoch = nullptr);
hipError_t launch_rows_set(SeqSet *set, int n, float *x, int d, bool gather, hipStream_t st, uint32_t *epoch = nullptr);      // gather: hid_in -> x rows; else x rows -> hid_out
hipError_t launch_argmax_set(const float *logits, int V, const SeqSet *set, int n, hipStream_t st);   // + trace, tok_out, position advance
hipError_t launch_advance_set(const SeqSet *set, int n, hipStream_t st);
hipError_t launch_dec_attn(const float *qkv, int d, int H, int n_ctx, int nth, const double *tab, float *Kc, float *Vc,
                           float *sc, float *part, float *merged, uint32_t *qa_A, float *qa_d,
                           const uint16_t *T_exp, const int32_t *state, hipStream_t st,
                           uint32_t *xsync = nullptr, uint32_t *fault = nullptr,      // xsync: H * 32 zeroed dwords -> single-launch k_dec_attn_x
                           bool long_ctx = false,                                     // long_ctx: k_dec_scores + k_dec_pv_stream (pv_stream_applies) ...
                           uint64_t *xpart = nullptr, const uint32_t *epoch = nullptr, int layer = 0,       // ... its chains split over workgroups: [H dh/32][nth][32] granules, tag = (epoch, layer + 1)
                           const DecAttnForce *force = nullptr);                      // what runs is dec_attn_plan's answer (dec_attn_plan.h; pv_stream_applies lives there)
bool xcd_selftest(int H, int Y, hipStream_t st);
// wq|wk|wv mat-vec + decode attention as one launch (k_qkv_attn); xsync / fault as launch_dec_attn
constexpr int TAG_MAX_LAYERS = 250;                                 // hand-off tags carry the layer index in 8 bits (kernels.hip make_tag)
bool qkv_attn_applies(const QMat &w, int d, int H, int nth);
bool qkv_attn_launch_query(const QMat &w, const NormPart &np, int d, int H, int n_ctx, int nth, long out[5]);      // host-only: { prologue, depth, pg, grid, LDS } of the launch
hipError_t launch_qkv_attn(const QMat &w, const float *x, const float *norm_w, const NormPart &np, uint64_t *qkv2, uint64_t *sc2, uint32_t *epoch, int layer,
                           int d, int H, int n_ctx, int nth, const double *tab, float *Kc, float *Vc, float *merged, uint32_t *qa_A, float *qa_d,
                           const uint16_t *T_silu, const uint16_t *T_exp, const int32_t *state, uint32_t *fault, hipStream_t st,
                           const MailboxIO *mb = nullptr);      // mb->in_t: the row arrives as tagged granules (pipeline mailbox)
hipError_t launch_bump_epoch(uint32_t *epoch, hipStream_t st);
// a residual-stream row re-published as tagged granules, slot 0 of the current epoch (pipeline mailbox tests, single-GPU stage chains)
hipError_t launch_quantize_offline(const void *src, int f16, uint8_t *dst, long nblocks, hipStream_t st);
hipError_t launch_advance(int32_t *state, hipStream_t st);
// sampler front end (utils.cpp:345-395): the k best candidate scores of the last row of logits, on the device
hipError_t launch_topk_candidates(const float *logits, int V, const int32_t *window, int n_window, double scale, double repeat_penalty, int k,
                                  double *out_score, int32_t *out_id, int32_t *flags, hipStream_t st, void *ws = nullptr);      // ws: TOPK_WS_BYTES zeroed once -> the two-launch variant
constexpr size_t TOPK_WS_BYTES = 32768 * 8 + 64 * 8 + 64;
// the same selection over R rows [R][V] in one launch pair (llamahip_decode_sample_multi, llamahip_op_topk_rows): windows [R][1024], n_last [R]
// (> 1024: the row is flagged inexact), ws R * TOPK_WS_BYTES zeroed once, out [R]; spill (may be null) [R][V] receives the rows flagged inexact
struct TopkOut { double sc[64]; int32_t id[64]; int32_t fl[2]; };          // fl[0] = exact, fl[1] = values collected
hipError_t launch_topk_rows(const float *logits, int R, int V, const int32_t *windows, const int32_t *n_last, double scale, double repeat_penalty,
                            int k, TopkOut *out, float *spill, hipStream_t st, void *ws);
// ... with row r's window = ids[r .. r + n_last) of one id stream of n_last + R - 1 ids (llamahip_verify_sample, llamahip_op_topk_slide): refuses
// n_last > 1024, V > 32768, k > 64; ws and out as above, no spill (the rows stay on the device until the next eval)
hipError_t launch_topk_slide(const float *logits, int R, int V, const int32_t *ids, int n_last, double scale, double repeat_penalty, int k,
                             TopkOut *out, hipStream_t st, void *ws);
// ... with the R <= 16 rows cut into segments that slide inside their own id streams of one id pool (llamahip_verify_sample_multi,
// llamahip_op_topk_slide_set): row r's window = ids[row_off[r] .. + row_n_last[r]) -- two device words per row, resolved from the segments by the
// host, which also checks that every window lies inside the pool.  row_n_last[r] > 1024: the row reads no ids and is flagged inexact.
hipError_t launch_topk_slide_set(const float *logits, int R, int V, const int32_t *ids, const int32_t *row_off, const int32_t *row_n_last, double scale,
                                 double repeat_penalty, int k, TopkOut *out, hipStream_t st, void *ws);
// the id pool of such a step: per segment at most 1024 window ids + its rows - 1 draft ids; and its per-row table {row_off[16], row_n_last[16]}
constexpr size_t SLIDE_SET_IDS = 16 * 1024 + 16;
// next-token scoring of n_rows rows of logits (logprob.hip): per row the log-probability of targets[r] in double, the argmax (lowest index
// on ties) and the target's rank (entries strictly greater); target -1: not scored.  A row's result depends on its bits and V only.
hipError_t launch_row_logprob(const float *logits, int n_rows, int V, const int32_t *targets, double *lp_out, int32_t *am_out, int32_t *rk_out,
                              hipStream_t st);
// the n <= TOPN_MAX most probable entries of n_rows rows of logits (topn.hip): per row ids[n] (value descending, the lower index first on equal
// values) and logprob[n], bit for bit launch_row_logprob's for those targets; a row with a NaN or a +inf: ids -1, logprobs NaN.  A row's result
// depends on its bits, V and n only.  Refused (hipErrorInvalidValue, nothing launched): n_rows < 1, V < 1, n outside 1 .. TOPN_MAX, n > V.
constexpr int TOPN_MAX = 64;
hipError_t launch_row_topn(const float *logits, int n_rows, int V, int n, int32_t *ids_out, double *lp_out, hipStream_t st);
// a text's embedding (pool.hip): the final norm of n_rows rows x[n_rows][d] as plain fp32 rows y (k_dense_prep<PREP_NORM>'s arithmetic, no fp16
// rounding, no permutation); then out[s] = the last row (pool 0) or the mean in double over rows [seg_begin[s], seg_begin[s + 1]) of y in ascending
// row order (pool 1), and with normalize the row divided by its L2 length (64 lane sums folded by the xor butterfly; a zero row stays zero)
hipError_t launch_norm_rows_f32(const float *x, const float *w, int d, int n_rows, float *y, hipStream_t st);
hipError_t launch_pool_rows(const float *y, const int32_t *seg_begin /* device, n_segs + 1 */, int n_segs, int d, int pool, int normalize, float *out, hipStream_t st);
hipError_t launch_argmax(const float *logits, int V, int32_t *out, int out_idx, int32_t *next_token, int32_t *state, hipStream_t st, uint64_t *token_mb = nullptr);
// drafted greedy decoding (verify.hip): pick[r] = the greedy pick of row r (k_argmax's rule), 1 .. VERIFY_ROWS_MAX rows; then, for
// tokens = [last accepted token, draft ...] of those rows: n_accept = the number of leading draft tokens the picks reproduce,
// log[state[1] ..] (log_cap entries) receives pick[0 .. n_accept], state = {position, cursor} advances by n_accept + 1 and
// res = {n_accept, pick[0 .. n_rows)}.  pick == null: one row whose pick is pick_imm; restart_pos >= 0: state = {restart_pos, 0} first.
constexpr int VERIFY_ROWS_MAX = 16;
hipError_t launch_verify_rows(const float *logits, int n_rows, int V, int32_t *pick, hipStream_t st);
// a scheduler's mixed pass (k_sched_pick, one wave per segment): logits row s = segment s's last row, tab[s] = {emit, slot, position, cursor};
// res[s] = the greedy pick of an emitting segment (k_verify_rows' rule), -1 otherwise; state / log / next_tok (all or none): the slot's
// {position, cursor} words are set, an emitting segment's pick goes to the slot's next-token word and to log[slot][cursor - 1]
hipError_t launch_sched_pick(const float *logits, int n_segs, int V, const int32_t *tab, int32_t *state, int32_t *log, int log_cap, int32_t *next_tok,
                             int32_t *res, hipStream_t st);
hipError_t launch_accept_drafts(const int32_t *tokens, const int32_t *pick, int pick_imm, int n_rows, int restart_pos, int32_t *log, int log_cap,
                                int32_t *state, int32_t *res, hipStream_t st);
// ... for the rows of several sequences in one step: segment s = rows [seg_begin[s], seg_begin[s + 1]) of slot seg_slot[s] (seg_begin ascending from 0
// to n_rows: checked by the caller), res = {n_accept[n_segs], pick[n_rows]}.  state / log / next_tok (all or none): the bound slots' {position,
// cursor} [slot][2], token logs [slot][log_cap] and next-token words [slot], advanced / appended / set per segment.
hipError_t launch_accept_drafts_set(const int32_t *tokens, const int32_t *pick, const int32_t *seg_begin, const int32_t *seg_slot, int n_segs, int n_rows,
                                    int32_t *state, int32_t *log, int log_cap, int32_t *next_tok, int32_t *res, hipStream_t st);
// a scheduler's step with drafted tokens (k_sched_accept, one wave per segment, behind launch_verify_rows over the step's n_rows logits rows):
// tab[s] = {emit, slot, base position, base cursor, first logits row, row count} (SCHED_TAB_W words; emit 0 / 1 / 2: llamahip_op_sched_accept),
// tokens[r] = the token logits row r evaluated; res = {n_accept[n_segs], pick[n_rows]}.  state / log / next_tok (all or none): the slot's words.
// The caller has checked that every emitting segment's logits rows lie in [0, n_rows) and every slot inside state / log / next_tok.
constexpr int SCHED_TAB_W = 6;
hipError_t launch_sched_accept(const int32_t *pick, const int32_t *tokens, const int32_t *tab, int n_segs, int n_rows, int32_t *state, int32_t *log,
                               int log_cap, int32_t *next_tok, int32_t *res, hipStream_t st);
// KV rows from slot to slot (kv_copy.hip, k_kv_copy_rows): for every copy c < n the rows [row_begin[c], row_begin[c] + n_rows[c]) of every one of
// the n_layers layers of Kc and Vc ([n_slots][n_layers][n_ctx][d] fp32 each) go from slot src[c] to the same rows of slot dst[c].  The table
// travels by value in the kernel arguments.  ONE launch (none where every copy is empty).  Refused (hipErrorInvalidValue, nothing launched):
// a slot or a range outside the arrays, src == dst, a destination that is another copy's source or destination, d % 4 != 0.
constexpr int KV_COPY_MAX = 16;
struct KvCopyTab { int32_t n; int32_t src[KV_COPY_MAX], dst[KV_COPY_MAX], row_begin[KV_COPY_MAX], n_rows[KV_COPY_MAX]; };
hipError_t launch_kv_copy_rows(float *Kc, float *Vc, const KvCopyTab &tab, int n_slots, int n_layers, int n_ctx, int d, hipStream_t st);
// KV rows of a slot moved down in place, keys re-rotated (kv_shift.hip, k_kv_shift_rows; NOT the reference's arithmetic): for every shift c < n
// the rows [row_begin[c], row_begin[c] + n_rows[c]) of every one of the n_layers layers of Kc and Vc go to the rows n_discard[c] below, every K
// pair rotated by -n_discard[c] positions with (cos, sin) = sincos_tab[n_discard[c]][pair] ([n_ctx][dh / 2][2] doubles, device memory).  Any
// overlap of the two ranges is safe.  ONE launch (none where every shift is empty).  Refused (hipErrorInvalidValue, nothing launched): what
// launch_kv_copy_rows refuses of slots, ranges and d, a slot twice, n_discard < 1, row_begin - n_discard < 0, dh odd or not dividing d.
constexpr int KV_SHIFT_MAX = 16, KV_SHIFT_U = 8;
struct KvShiftTab { int32_t n; int32_t slot[KV_SHIFT_MAX], row_begin[KV_SHIFT_MAX], n_rows[KV_SHIFT_MAX], n_discard[KV_SHIFT_MAX]; };
hipError_t launch_kv_shift_rows(float *Kc, float *Vc, const double *sincos_tab, const KvShiftTab &tab, int n_slots, int n_layers, int n_ctx, int d, int dh,
                                hipStream_t st);
// constrained decoding (constrain.hip): the pick of 1 .. DFA_ROWS_MAX rows under their constraints' token tables, and the masked rows for the
// sampler front end.  A row of k_pick_dfa: its logits row, its table next[n_states][V] (DFA_BANNED_U16 = not allowed), its words
// cst = {state, dead}, the token picked where the state is out of range or nothing is allowed (dead := 1, state kept), and k_argmax's
// operands: out[st ? st[1] : out_idx] = pick (out may be null), *next_token = pick (may be null), st = {position, step} advanced (may be null).
// The rows travel by value in the kernel arguments, so a captured step replays them.
constexpr int DFA_ROWS_MAX = 16;
constexpr uint16_t DFA_BANNED_U16 = 0xFFFF;
struct DfaRow {
    const float *logits; const uint16_t *table; int32_t *cst; int32_t *out; int32_t *next_token; int32_t *st;
    int32_t n_states, fallback, out_idx, repick;      // repick: out[st[1] - 1] = pick, st stays (behind a step that has advanced it)
};
struct DfaRows { DfaRow r[DFA_ROWS_MAX]; };
struct DfaMaskRows { const uint16_t *row[DFA_ROWS_MAX]; };
hipError_t launch_pick_dfa(const DfaRows &rows, int n_rows, int V, hipStream_t st);
hipError_t launch_mask_rows_dfa(const float *logits, float *out, int n_rows, int V, const DfaMaskRows &rows, hipStream_t st);
// a scheduler step with constrained greedy segments (verify.hip): launch_verify_rows / launch_sched_pick with a per-row allow-list --
// rows.row[r] = the table row next[state] of logits row r (the host resolves the state), null = unconstrained (vr_row_pick); fb.t[r] = the
// range-checked token a row that allows nothing picks, its dead word then 1.  launch_sched_pick_dfa's res = {pick[n_segs], dead[n_segs]}.
struct DfaFallback { int32_t t[DFA_ROWS_MAX]; };
hipError_t launch_verify_rows_dfa(const float *logits, int n_rows, int V, const DfaMaskRows &rows, const DfaFallback &fb, int32_t *pick, int32_t *dead, hipStream_t st);
hipError_t launch_sched_pick_dfa(const float *logits, int n_segs, int V, const int32_t *tab, const DfaMaskRows &rows, const DfaFallback &fb, int32_t *state,
                                 int32_t *log, int log_cap, int32_t *next_tok, int32_t *res, hipStream_t st);

}  // namespace lh
