// ops.cpp -- the single-op entry points of include/llamahip.h (llamahip_op_*, llamahip_debug_attn_path): one or two kernel families on
// caller-supplied operands, for the per-op tests.  None of them touches a model handle: each uploads its operands into a Scratch
// (host_util.h), launches, copies back; the Scratch frees the device memory and the stream on every return.  No CPU fallback.
#include <algorithm>
#include <cstring>
#include <vector>

#include "host_util.h"
#include "llamahip_internal.h"

using namespace lh;

static_assert(LLAMAHIP_PREP_PLAIN == PREP_PLAIN && LLAMAHIP_PREP_NORM == PREP_NORM && LLAMAHIP_PREP_SILU_MUL == PREP_SILU_MUL, "llamahip.h mirrors the prep modes");
static_assert(LLAMAHIP_PREP_KERNEL_AUTO == PREP_FORCE_AUTO && LLAMAHIP_PREP_KERNEL_FAST == PREP_FORCE_FAST && LLAMAHIP_PREP_KERNEL_LDS == PREP_FORCE_LDS, "... and launch_prep's force values");

namespace lh {      // eval_multi.cpp
int rows_table_check(int32_t R, int32_t n_ctx, int32_t n_slots, const int32_t *row_slot, const int32_t *row_pos, const int32_t *row_keys, char *err, size_t err_cap);
int pool_rows_check(const float *x, int32_t R, int32_t d, const float *norm_w, const int32_t *seg_begin, int32_t n_segs, int32_t pool, int32_t normalize,
                    const float *out, char *err, size_t err_cap);
}

extern "C" {

int llamahip_op_mul_mat_q4_0(const void *w_q4_0, int32_t M, int32_t K, const float *x, int32_t N,
                             float *y, char *err, size_t err_cap) {
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    if (!w_q4_0 || !x || !y || M < 1 || N < 1 || K < 64 || K % 64 != 0) { set_err(err, err_cap, "bad mul_mat arguments (K must be a positive multiple of 64)"); return LLAMAHIP_ERR_PREDICT; }
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    QMat q;
    q.set_shape(M, K);
    const size_t wbytes = (size_t) M * (K / 32) * 20, Kp = (size_t) q.Kp();
    Scratch s;
    hipStream_t st = s.stream();
    uint8_t *d_w = s.alloc(wbytes, (const uint8_t *) w_q4_0);
    float *d_x = s.alloc((size_t) N * K, x), *d_y = s.alloc<float>((size_t) N * M);
    q.tiles = s.alloc<uint8_t>(q.bytes());
    uint32_t *d_qA = s.alloc<uint32_t>((size_t) N * Kp / 4);
    float *d_qd = s.alloc<float>((size_t) N * (Kp / 32));
    if (s.ok()) s.check(launch_repack(d_w, q.tiles, M, K, 0, 0, st));
    if (N >= 2) {          // the model path's prompt GEMM: row-lane copy
        q.rows = s.alloc<uint8_t>(q.rows_bytes());
        if (s.ok()) s.check(launch_tiles_to_rows(q, st));
    }
    if (s.ok()) s.check(launch_prep(PREP_PLAIN, d_x, nullptr, K, 0, K, N, d_qA, d_qd, nullptr, nullptr, nullptr, st));
    if (s.ok()) s.check(launch_gemm(q, EPI_STORE, d_qA, d_qd, N, d_y, M, nullptr, 0, st));
    s.download(y, d_y, (size_t) N * M * 4);
    s.sync();
    return s.ok() ? LLAMAHIP_OK : s.fail("llamahip_op_mul_mat_q4_0", err, err_cap);
}

static_assert(LLAMAHIP_GEMV_PRE_QA == PRE_QA && LLAMAHIP_GEMV_PRE_PLAIN == PREP_PLAIN && LLAMAHIP_GEMV_PRE_NORM == PREP_NORM && LLAMAHIP_GEMV_PRE_SILU_MUL == PREP_SILU_MUL, "llamahip.h mirrors the mat-vec prologues");
static_assert(LLAMAHIP_GEMV_EPI_STORE == EPI_STORE && LLAMAHIP_GEMV_EPI_RESID == EPI_RESID && LLAMAHIP_GEMV_EPI_SILU_QA == EPI_SILU_QA, "... and epilogues");
constexpr size_t GEMV_LDS_CAP = 160 * 1024;      // init_attrs_decode's dynamic-LDS attribute

// one launch of the single-row decode mat-vec (k_gemv) on caller-supplied operands (per-op tests of every instance gemv_plan can pick): see llamahip.h
int llamahip_op_gemv_q4_0(const void *w_q4_0, int32_t M, int32_t K, int32_t interleaved, int32_t pre, int32_t epi, const float *in0, const float *in1,
                          const double *part_in, int32_t n_part_in, const float *resid, float *y, int64_t y_floats, uint32_t *out_A, float *out_d,
                          int32_t out_rows, double *part_out, int32_t n_part_out, int32_t part_out_cap, int64_t *plan, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_gemv_q4_0";
    // the pairs that wait on other launches or other workgroups (tagged operands, the lm head's pick, half-block exchange): not an op's to launch
    const char *waits = pre == PREP_NORM_TAG ? "PREP_NORM_TAG" : epi == EPI_STORE_TAG ? "EPI_STORE_TAG" : epi == EPI_RESID_TAG ? "EPI_RESID_TAG"
                      : epi == EPI_STORE_PICK ? "EPI_STORE_PICK" : epi == EPI_SILU_QAH ? "EPI_SILU_QAH" : nullptr;
    if (waits) { set_err(err, err_cap, "%s: %s waits on other launches or workgroups: the op launches the untagged pairs only", fn, waits); return LLAMAHIP_ERR_PREDICT; }
    if (pre == PREP_NORMP) { set_err(err, err_cap, "%s: PREP_NORMP is pre NORM with part_in / n_part_in", fn); return LLAMAHIP_ERR_PREDICT; }
    if (pre < PRE_QA || pre > PREP_SILU_MUL) { set_err(err, err_cap, "%s: unknown prologue %d", fn, pre); return LLAMAHIP_ERR_PREDICT; }
    if (epi < EPI_STORE || epi > EPI_SILU_QA) { set_err(err, err_cap, "%s: unknown epilogue %d", fn, epi); return LLAMAHIP_ERR_PREDICT; }
    if (M < 1 || K < 64 || K % 64 != 0) { set_err(err, err_cap, "%s: bad shape (M %d >= 1; K %d must be a positive multiple of 64)", fn, M, K); return LLAMAHIP_ERR_PREDICT; }
    if (interleaved && M % 64 != 0) { set_err(err, err_cap, "%s: interleaved takes w1's F rows then w3's with F %% 32 == 0: M = 2F = %d is not a multiple of 64", fn, M); return LLAMAHIP_ERR_PREDICT; }
    const bool has1 = pre == PREP_NORM || pre == PREP_SILU_MUL, silu_qa = epi == EPI_SILU_QA;
    if (!w_q4_0 || !in0 || (has1 && !in1)) { set_err(err, err_cap, "%s: null operand (w, in0%s)", fn, has1 ? ", in1" : ""); return LLAMAHIP_ERR_PREDICT; }
    if (epi == EPI_RESID && !resid) { set_err(err, err_cap, "%s: EPI_RESID needs resid", fn); return LLAMAHIP_ERR_PREDICT; }
    const int64_t n_out = silu_qa ? M / 2 : M;      // floats the launch writes to y
    if (!silu_qa && !y) { set_err(err, err_cap, "%s: y is NULL (only EPI_SILU_QA may leave it out)", fn); return LLAMAHIP_ERR_PREDICT; }
    if (y && y_floats < n_out) { set_err(err, err_cap, "%s: y_floats %lld < the %lld outputs", fn, (long long) y_floats, (long long) n_out); return LLAMAHIP_ERR_PREDICT; }
    if (silu_qa && (!out_A || !out_d || out_rows < 1)) { set_err(err, err_cap, "%s: EPI_SILU_QA needs out_A, out_d and out_rows %d >= 1", fn, out_rows); return LLAMAHIP_ERR_PREDICT; }
    if (part_in && pre != PREP_NORM) { set_err(err, err_cap, "%s: part_in is the NORM prologue's", fn); return LLAMAHIP_ERR_PREDICT; }
    if (part_in && (n_part_in < 1 || n_part_in > NORM_PART_MAX)) { set_err(err, err_cap, "%s: n_part_in %d outside 1 .. %d (NORM_PART_MAX)", fn, n_part_in, NORM_PART_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (part_out && epi != EPI_RESID) { set_err(err, err_cap, "%s: part_out is the RESID epilogue's", fn); return LLAMAHIP_ERR_PREDICT; }
    QMat q;
    q.set_shape(M, K);
    if (interleaved) q.gmapF8 = M / 16;
    NormPart np;
    np.in = part_in; np.n_in = part_in ? n_part_in : 0;
    int pre_run = pre;
    norm_mode_resolve(&pre_run, &np);      // (the plan of what launch_gemv will launch: PREP_NORMP where the parts are taken)
    const GemvPlan p = gemv_plan(q, pre_run, epi);
    if (!gemv_plan_has_kernel(pre_run, epi, p)) {
        set_err(err, err_cap, "%s: k_gemv has no instance for prologue %d, epilogue %d on M %d, K %d%s (plan: %d waves, %d granules, depth %d, ring %d)", fn, pre_run, epi, M, K,
                interleaved ? " interleaved" : "", p.nw, p.pg, p.depth, (int) p.ring);
        return LLAMAHIP_ERR_PREDICT;
    }
    if (p.lds > GEMV_LDS_CAP) { set_err(err, err_cap, "%s: K %d needs %zu bytes of LDS, the kernels' cap is %zu", fn, K, p.lds, GEMV_LDS_CAP); return LLAMAHIP_ERR_PREDICT; }
    if (part_out && (p.grid > NORM_PART_MAX || n_part_out != p.grid || part_out_cap < n_part_out)) {
        set_err(err, err_cap, "%s: part_out takes %d pairs (one per workgroup: gemv_resid_parts), at most %d (NORM_PART_MAX); got %d in a buffer of %d", fn, p.grid, NORM_PART_MAX, n_part_out, part_out_cap);
        return LLAMAHIP_ERR_PREDICT;
    }
    if (plan) { const int64_t o[6] = { p.nw, p.pg, p.depth, p.ring, p.grid, (int64_t) p.lds }; for (int i = 0; i < 6; i++) plan[i] = o[i]; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    const size_t nb = (size_t) K / 32, Kp = (size_t) q.Kp(), F = (size_t) M / 2, Fp = (F + 255) / 256 * 256;
    const size_t oA = silu_qa ? (size_t) out_rows * Fp / 4 : 0, od = silu_qa ? (size_t) out_rows * (Fp / 32) : 0;
    const bool tables = pre == PREP_SILU_MUL || silu_qa;
    std::vector<uint16_t> ts, te;
    if (tables) { ts.resize(1 << 16); te.resize(1 << 16); lut_tables(ts, te); }
    Scratch s;
    hipStream_t st = s.stream();
    uint8_t *d_w = s.alloc((size_t) M * nb * 20, (const uint8_t *) w_q4_0);
    q.tiles = s.alloc<uint8_t>(q.bytes());
    float *d_in0 = s.alloc((size_t) K, in0), *d_in1 = has1 ? s.alloc((size_t) K, in1) : nullptr;
    float *d_r = epi == EPI_RESID ? s.alloc((size_t) M, resid) : nullptr;
    float *d_y = y ? s.alloc((size_t) y_floats, y) : nullptr;      // (the floats past the outputs keep the caller's bits; so do the buffers below)
    uint32_t *d_oA = silu_qa ? s.alloc(oA, out_A) : nullptr;
    float *d_od = silu_qa ? s.alloc(od, out_d) : nullptr;
    double *d_pi = part_in ? s.alloc((size_t) 2 * n_part_in, part_in) : nullptr;
    double *d_po = part_out ? s.alloc((size_t) 2 * part_out_cap, part_out) : nullptr;
    uint32_t *d_qA = pre == PRE_QA ? s.alloc<uint32_t>(Kp / 4) : nullptr;
    float *d_qd = pre == PRE_QA ? s.alloc<float>(Kp / 32) : nullptr;
    uint16_t *d_ts = tables ? s.alloc(ts.size(), ts.data()) : nullptr, *d_te = tables ? s.alloc(te.size(), te.data()) : nullptr;
    if (s.ok() && tables) s.check(launch_check_lut_math(d_ts, d_te, st));          // g_lut_math, as a model load leaves it
    if (s.ok() && !interleaved) s.check(launch_repack(d_w, q.tiles, M, K, 0, 0, st));
    if (s.ok() && interleaved) s.check(launch_repack(d_w, q.tiles, (int) F, K, 1, 0, st));                      // as the loader: w1's rows ...
    if (s.ok() && interleaved) s.check(launch_repack(d_w + F * nb * 20, q.tiles, (int) F, K, 1, 4, st));        // ... then w3's
    if (s.ok() && pre == PRE_QA) s.check(launch_prep(PREP_PLAIN, d_in0, nullptr, K, 0, K, 1, d_qA, d_qd, nullptr, nullptr, nullptr, st));
    np = NormPart();
    np.in = d_pi; np.n_in = d_pi ? n_part_in : 0; np.out = d_po;
    if (s.ok()) s.check(launch_gemv(q, pre, epi, d_qA, d_qd, pre == PRE_QA ? nullptr : d_in0, d_in1, d_y, d_r, d_ts, d_oA, d_od, st, &np));
    if (y) s.download(y, d_y, (size_t) y_floats * 4);
    if (silu_qa) { s.download(out_A, d_oA, oA * 4); s.download(out_d, d_od, od * 4); }
    if (part_out) s.download(part_out, d_po, (size_t) part_out_cap * 16);
    s.sync();
    return s.ok() ? LLAMAHIP_OK : s.fail(fn, err, err_cap);
}

static_assert(LLAMAHIP_GEMV_EPI_ROPE_KV == EPI_ROPE_KV && LLAMAHIP_GEMV_EPI_SILU_QAH == EPI_SILU_QAH, "llamahip.h mirrors the few-row epilogues");

// one launch of the few-row mat-mul (k_gemv_set) on caller-supplied operands (per-op tests of every (NC, CW) instance under every epilogue): see llamahip.h
int llamahip_op_gemv_set_q4_0(const void *w_q4_0, int32_t M, int32_t K, int32_t interleaved, int32_t epi, const float *x, int32_t N, const int32_t *force,
                              const float *resid, float *y, int32_t y_stride,
                              int32_t d, int32_t dh, int32_t n_ctx, int32_t n_slots, int32_t n_past, const int32_t *row_pos, const int32_t *row_slot,
                              float *qr, float *Kc, float *Vc,
                              uint32_t *out_A, float *out_d, int32_t out_rows, int32_t layer, const float *x_prev, uint32_t *fault,
                              int64_t *plan, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_gemv_set_q4_0";
    const bool plain = epi == EPI_STORE || epi == EPI_RESID, rope = epi == EPI_ROPE_KV, qah = epi == EPI_SILU_QAH, silu = qah || epi == EPI_SILU_QA;
    if (!plain && !rope && !silu) { set_err(err, err_cap, "%s: unknown epilogue %d (STORE, RESID, ROPE_KV, SILU_QA, SILU_QAH)", fn, epi); return LLAMAHIP_ERR_PREDICT; }
    if (N < 2 || N > 60) { set_err(err, err_cap, "%s: N %d outside 2 .. 60 rows", fn, N); return LLAMAHIP_ERR_PREDICT; }
    if (M < 1 || K < 64 || K % 64 != 0) { set_err(err, err_cap, "%s: bad shape (M %d >= 1; K %d must be a positive multiple of 64)", fn, M, K); return LLAMAHIP_ERR_PREDICT; }
    if (interleaved && M % 64 != 0) { set_err(err, err_cap, "%s: interleaved takes w1's F rows then w3's with F %% 32 == 0: M = 2F = %d is not a multiple of 64", fn, M); return LLAMAHIP_ERR_PREDICT; }
    if (silu != (interleaved != 0)) { set_err(err, err_cap, "%s: the SiLU epilogues take the interleaved w1|w3 matrix, the others a plain one (epilogue %d, interleaved %d)", fn, epi, interleaved); return LLAMAHIP_ERR_PREDICT; }
    if (!w_q4_0 || !x) { set_err(err, err_cap, "%s: null operand (w, x)", fn); return LLAMAHIP_ERR_PREDICT; }
    if (plain && !y) { set_err(err, err_cap, "%s: null operand (STORE / RESID need y)", fn); return LLAMAHIP_ERR_PREDICT; }
    if (epi == EPI_RESID && !resid) { set_err(err, err_cap, "%s: null operand (RESID needs resid)", fn); return LLAMAHIP_ERR_PREDICT; }
    if (plain && y_stride < M) { set_err(err, err_cap, "%s: y_stride %d < M %d", fn, y_stride, M); return LLAMAHIP_ERR_PREDICT; }
    if (rope && (!qr || !Kc || !Vc)) { set_err(err, err_cap, "%s: null operand (ROPE_KV needs qr, Kc, Vc)", fn); return LLAMAHIP_ERR_PREDICT; }
    if (silu && (!out_A || !out_d)) { set_err(err, err_cap, "%s: null operand (the SiLU epilogues need out_A, out_d)", fn); return LLAMAHIP_ERR_PREDICT; }
    if (silu && out_rows < N) { set_err(err, err_cap, "%s: out_rows %d < N %d", fn, out_rows, N); return LLAMAHIP_ERR_PREDICT; }
    if (qah && N > SET_MAX) { set_err(err, err_cap, "%s: SILU_QAH takes N <= %d rows (its exchange buffer), got %d", fn, SET_MAX, N); return LLAMAHIP_ERR_PREDICT; }
    if (qah && !fault) { set_err(err, err_cap, "%s: null operand (SILU_QAH returns its fault word)", fn); return LLAMAHIP_ERR_PREDICT; }
    if (qah && (layer < 0 || layer >= TAG_MAX_LAYERS)) { set_err(err, err_cap, "%s: layer %d outside 0 .. %d", fn, layer, TAG_MAX_LAYERS - 1); return LLAMAHIP_ERR_PREDICT; }
    if (x_prev && !qah) { set_err(err, err_cap, "%s: x_prev is SILU_QAH's (the launch before this one on the same exchange buffer)", fn); return LLAMAHIP_ERR_PREDICT; }
    const bool tables = rope && (row_pos || row_slot);
    if (rope) {
        if (d < 8 || d % 8 != 0 || M != 3 * d || dh < 2 || dh % 2 != 0 || d % dh != 0) {
            set_err(err, err_cap, "%s: ROPE_KV takes M = 3 d (M %d, d %d), d a multiple of 8 and of the even head size dh %d", fn, M, d, dh); return LLAMAHIP_ERR_PREDICT;
        }
        if (n_ctx < 1 || n_slots < 1) { set_err(err, err_cap, "%s: n_ctx (%d) and n_slots (%d) must be >= 1", fn, n_ctx, n_slots); return LLAMAHIP_ERR_PREDICT; }
        if (tables) {
            if (!row_pos || !row_slot) { set_err(err, err_cap, "%s: row_pos and row_slot come together", fn); return LLAMAHIP_ERR_PREDICT; }
            if (N > SET_MAX) { set_err(err, err_cap, "%s: a row table takes N <= %d rows (SeqSet), got %d", fn, SET_MAX, N); return LLAMAHIP_ERR_PREDICT; }
            for (int r = 0; r < N; r++) {
                if (row_slot[r] < 0 || row_slot[r] >= n_slots) { set_err(err, err_cap, "%s: row_slot[%d] = %d out of range [0, %d)", fn, r, row_slot[r], n_slots); return LLAMAHIP_ERR_PREDICT; }
                if (row_pos[r] < 0 || row_pos[r] >= n_ctx) { set_err(err, err_cap, "%s: row_pos[%d] = %d out of range [0, n_ctx = %d)", fn, r, row_pos[r], n_ctx); return LLAMAHIP_ERR_PREDICT; }
                for (int q = 0; q < r; q++)
                    if (row_slot[q] == row_slot[r] && row_pos[q] == row_pos[r]) {
                        set_err(err, err_cap, "%s: rows %d and %d both write position %d of slot %d", fn, q, r, row_pos[r], row_slot[r]); return LLAMAHIP_ERR_PREDICT;
                    }
            }
        } else if (n_past < 0 || n_past + N > n_ctx) {
            set_err(err, err_cap, "%s: n_past %d + N %d rows outside n_ctx %d", fn, n_past, N, n_ctx); return LLAMAHIP_ERR_PREDICT;
        }
    }
    QMat q;
    q.set_shape(M, K);
    if (interleaved) q.gmapF8 = M / 16;
    q.tiles = (uint8_t *) (uintptr_t) 16;      // (the plan's predicates ask for a tile copy; the real one follows below)
    SetForce sf;
    if (force) {
        sf.nc = force[0]; sf.cw = force[1]; sf.rgw = force[2]; sf.strict = true;
        char why[200] = "";
        if (!gemv_set_force_check(q, N, epi, sf, why, sizeof(why))) {
            set_err(err, err_cap, "%s: forced plan {nc %d, cw %d, rgw %d} refused for M %d, K %d, N %d, epilogue %d: %s", fn, sf.nc, sf.cw, sf.rgw, M, K, N, epi, why);
            return LLAMAHIP_ERR_PREDICT;
        }
    } else if (!gemv_set_applies(q, N, epi)) {
        set_err(err, err_cap, "%s: k_gemv_set does not take M %d, K %d, N %d under epilogue %d (a plan that is instantiated and fits its LDS: llamahip_debug_set_plan)", fn, M, K, N, epi);
        return LLAMAHIP_ERR_PREDICT;
    }
    const SetForce *fp = force ? &sf : nullptr;
    long lp[7];
    if (!gemv_set_launch_query(q, N, epi, fp, lp)) { set_err(err, err_cap, "%s: no launch for M %d, K %d, N %d under epilogue %d", fn, M, K, N, epi); return LLAMAHIP_ERR_PREDICT; }
    if (force && (lp[0] != sf.nc || lp[1] != sf.cw || (sf.rgw && lp[3] != sf.rgw))) {
        set_err(err, err_cap, "%s: forced plan {nc %d, cw %d, rgw %d} would launch as <%ld,%ld> rgw %ld", fn, sf.nc, sf.cw, sf.rgw, lp[0], lp[1], lp[3]); return LLAMAHIP_ERR_PREDICT;
    }
    if (plan) for (int i = 0; i < 7; i++) plan[i] = lp[i];
    q.tiles = nullptr;
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    const size_t nb = (size_t) K / 32, Kp = (size_t) q.Kp(), F = (size_t) M / 2, Fp = (F + 255) / 256 * 256;
    const size_t oA = silu ? (size_t) out_rows * Fp / 4 : 0, od = silu ? (size_t) out_rows * (Fp / 32) : 0;
    const size_t cache_f = rope ? (size_t) n_slots * n_ctx * d : 0;
    std::vector<uint16_t> ts, te;
    if (silu) { ts.resize(1 << 16); te.resize(1 << 16); lut_tables(ts, te); }
    std::vector<double> tab;
    if (rope) tab = rope_table(n_ctx, dh);
    Scratch s;
    hipStream_t st = s.stream();
    if (qah && s.ok() && !xcd_selftest(8, 4, st)) {
        set_err(err, err_cap, "%s: SILU_QAH needs workgroups 8 apart in the grid on one XCD; this device does not place them so", fn); return LLAMAHIP_ERR_PREDICT;
    }
    uint8_t *d_w = s.alloc((size_t) M * nb * 20, (const uint8_t *) w_q4_0);
    q.tiles = s.alloc<uint8_t>(q.bytes());
    float *d_x = s.alloc((size_t) N * K, x), *d_xp = x_prev ? s.alloc((size_t) N * K, x_prev) : nullptr;
    uint32_t *d_qA = s.alloc<uint32_t>((size_t) N * Kp / 4);
    float *d_qd = s.alloc<float>((size_t) N * (Kp / 32));
    float *d_y = plain ? s.alloc((size_t) N * y_stride, y) : nullptr;      // (the floats outside the N x M block keep the caller's bits; so do the buffers below)
    float *d_r = epi == EPI_RESID ? s.alloc((size_t) N * M, resid) : nullptr;
    float *d_qr = rope ? s.alloc((size_t) N * d, qr) : nullptr, *d_K = rope ? s.alloc(cache_f, Kc) : nullptr, *d_V = rope ? s.alloc(cache_f, Vc) : nullptr;
    double *d_tab = rope ? s.alloc(tab.size(), tab.data()) : nullptr;
    SeqSet *d_set = nullptr;
    if (tables) {
        // pos[] and kv_off[] filled, every other member null: as the step's first launch (k_embed_set) leaves the descriptor for this kernel
        SeqSet hs;
        memset(&hs, 0, sizeof(hs));
        hs.n = N;
        for (int r = 0; r < N; r++) { hs.pos[r] = row_pos[r]; hs.kv_off[r] = (long) row_slot[r] * n_ctx * d; }
        d_set = s.alloc(1, &hs);
        s.sync();                              // (hs leaves scope)
    }
    uint32_t *d_oA = silu ? s.alloc(oA, out_A) : nullptr;
    float *d_od = silu ? s.alloc(od, out_d) : nullptr;
    uint16_t *d_ts = silu ? s.alloc(ts.size(), ts.data()) : nullptr, *d_te = silu ? s.alloc(te.size(), te.data()) : nullptr;
    // SILU_QAH: the exchange granules, the epoch word and the fault word, zeroed ONCE (a model handle's: never cleared between launches)
    const size_t ng = (size_t) SET_MAX * set_amax_granules((int) F);
    uint64_t *d_am = qah ? s.alloc<uint64_t>(ng) : nullptr;
    uint32_t *d_words = qah ? s.alloc<uint32_t>(8) : nullptr;              // [0] epoch, [4] fault
    uint32_t *d_pA = x_prev ? s.alloc<uint32_t>((size_t) N * Fp / 4) : nullptr;      // the scratch operand rows of the launch on x_prev
    float *d_pd = x_prev ? s.alloc<float>((size_t) N * (Fp / 32)) : nullptr;
    if (qah) { s.fill(d_am, 0, ng * 8); s.fill(d_words, 0, 32); }
    if (x_prev) { s.fill(d_pA, 0, (size_t) N * Fp); s.fill(d_pd, 0, (size_t) N * (Fp / 32) * 4); }
    if (s.ok() && silu) s.check(launch_check_lut_math(d_ts, d_te, st));          // g_lut_math, as a model load leaves it
    if (s.ok() && !interleaved) s.check(launch_repack(d_w, q.tiles, M, K, 0, 0, st));
    if (s.ok() && interleaved) s.check(launch_repack(d_w, q.tiles, (int) F, K, 1, 0, st));                      // as the loader: w1's rows ...
    if (s.ok() && interleaved) s.check(launch_repack(d_w + F * nb * 20, q.tiles, (int) F, K, 1, 4, st));        // ... then w3's
    SiluHalfIO hx;
    if (qah) { hx.amax_t = d_am; hx.epoch = d_words; hx.layer = layer; hx.fault = d_words + 4; }
    if (x_prev) {
        if (s.ok()) s.check(launch_prep(PREP_PLAIN, d_xp, nullptr, K, 0, K, N, d_qA, d_qd, nullptr, nullptr, nullptr, st));
        if (s.ok()) s.check(launch_bump_epoch(d_words, st));
        if (s.ok()) s.check(launch_gemv_set_silu_epi(q, epi, d_qA, d_qd, N, d_ts, d_pA, d_pd, (long) (Fp / 4), (long) (Fp / 32), hx, st, fp));
    }
    if (s.ok()) s.check(launch_prep(PREP_PLAIN, d_x, nullptr, K, 0, K, N, d_qA, d_qd, nullptr, nullptr, nullptr, st));
    if (s.ok() && qah) s.check(launch_bump_epoch(d_words, st));
    if (s.ok() && plain) s.check(launch_gemv_set(q, epi, d_qA, d_qd, N, d_y, y_stride, d_r, M, st, fp));
    if (s.ok() && rope) {
        RopeKvArgs ra = { d_tab, d_qr, d_K, d_V, tables ? 0 : n_past, d, dh };
        ra.set = d_set;
        s.check(launch_gemv_set_rope_kv(q, d_qA, d_qd, N, ra, st, fp));
    }
    if (s.ok() && silu) s.check(launch_gemv_set_silu_epi(q, epi, d_qA, d_qd, N, d_ts, d_oA, d_od, (long) (Fp / 4), (long) (Fp / 32), hx, st, fp));
    if (plain) s.download(y, d_y, (size_t) N * y_stride * 4);
    if (rope) { s.download(qr, d_qr, (size_t) N * d * 4); s.download(Kc, d_K, cache_f * 4); s.download(Vc, d_V, cache_f * 4); }
    if (silu) { s.download(out_A, d_oA, oA * 4); s.download(out_d, d_od, od * 4); }
    if (qah) s.download(fault, d_words + 4, 4);
    s.sync();
    return s.ok() ? LLAMAHIP_OK : s.fail(fn, err, err_cap);
}

// one prompt GEMM kernel on caller-supplied operands (per-op tests of every kernel launch_gemm can pick): see llamahip.h
int llamahip_op_prompt_gemm_q4_0(const void *w_q4_0, int32_t M, int32_t K, const float *x, int32_t N, const float *resid,
                                 float *y, int32_t y_stride, int32_t path, int32_t *path_taken, char *err, size_t err_cap) {
    if (!w_q4_0 || !x || !y || M < 1 || N < 1 || K < 64 || K % 64 != 0) {
        set_err(err, err_cap, "llamahip_op_prompt_gemm_q4_0: bad arguments (M %d, N %d >= 1; K %d must be a positive multiple of 64)", M, N, K); return LLAMAHIP_ERR_PREDICT;
    }
    if (y_stride < M) { set_err(err, err_cap, "llamahip_op_prompt_gemm_q4_0: y_stride %d < M %d", y_stride, M); return LLAMAHIP_ERR_PREDICT; }
    if (path < LLAMAHIP_GEMM_AUTO || path > LLAMAHIP_GEMM_LDS) { set_err(err, err_cap, "llamahip_op_prompt_gemm_q4_0: unknown path %d", path); return LLAMAHIP_ERR_PREDICT; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    QMat q;
    q.set_shape(M, K);
    const size_t wbytes = (size_t) M * (K / 32) * 20, Kp = (size_t) q.Kp(), ybytes = (size_t) N * y_stride * 4;
    const bool auto_ = path == LLAMAHIP_GEMM_AUTO;
    const bool want_rows = auto_ || path == LLAMAHIP_GEMM_ROWS, want_mt4 = auto_ || path == LLAMAHIP_GEMM_MFMA4;
    const bool want_mt = path == LLAMAHIP_GEMM_MFMA_I8 || path == LLAMAHIP_GEMM_FAST;
    Scratch s;
    hipStream_t st = s.stream();
    uint8_t *d_w = s.alloc(wbytes, (const uint8_t *) w_q4_0);
    float *d_x = s.alloc((size_t) N * K, x);
    float *d_y = s.alloc((size_t) N * y_stride, y);      // (the floats between M and y_stride keep the caller's bits)
    float *d_r = resid ? s.alloc((size_t) N * M, resid) : nullptr;
    q.tiles = s.alloc<uint8_t>(q.bytes());
    if (want_rows) q.rows = s.alloc<uint8_t>(q.rows_bytes());
    if (want_mt4) q.mt4 = s.alloc<uint8_t>(q.mt4_bytes());
    if (want_mt) q.mt = s.alloc<uint8_t>(q.mt_bytes());
    uint32_t *d_qA = s.alloc<uint32_t>((size_t) N * Kp / 4);
    float *d_qd = s.alloc<float>((size_t) N * (Kp / 32));
    uint8_t *d_qb = s.alloc<uint8_t>((size_t) N * Kp * 2);      // as the model's workspace: the fp16 (or int8) operand
    if (s.ok()) s.check(launch_repack(d_w, q.tiles, M, K, 0, 0, st));
    if (s.ok() && want_rows) s.check(launch_tiles_to_rows(q, st));
    if (s.ok() && want_mt4) s.check(launch_tiles_to_mt4(q, st));
    if (s.ok() && want_mt) s.check(launch_tiles_to_mtiles(q, st));
    if (s.ok()) s.check(launch_prep(PREP_PLAIN, d_x, nullptr, K, 0, K, N, d_qA, d_qd, nullptr, nullptr, nullptr, st));
    const int epi = resid ? EPI_RESID : EPI_STORE;
    const char *why = nullptr;
    long before[GEMM_PATH_COUNT];
    for (int i = 0; i < GEMM_PATH_COUNT; i++) before[i] = g_gemm_path_counts[i];
    if (s.ok()) s.check(auto_ ? launch_gemm(q, epi, d_qA, d_qd, N, d_y, y_stride, d_r, M, st, d_qb, false)
                              : launch_gemm_forced(path, q, epi, d_qA, d_qd, N, d_y, y_stride, d_r, M, st, d_qb, &why));
    s.download(y, d_y, ybytes);
    s.sync();
    if (why) { set_err(err, err_cap, "llamahip_op_prompt_gemm_q4_0: path %d refused for M %d, K %d, N %d: %s", path, M, K, N, why); return LLAMAHIP_ERR_PREDICT; }
    if (!s.ok()) return s.fail("llamahip_op_prompt_gemm_q4_0", err, err_cap);
    if (path_taken) {
        // the kernel family whose count moved (the matrix-core count moves with the fast one; this handle has ONE matrix-core copy)
        auto moved = [&](int i) { return g_gemm_path_counts[i] != before[i]; };
        *path_taken = moved(GEMM_PATH_FAST) ? LLAMAHIP_GEMM_FAST : moved(GEMM_PATH_MFMA) ? (want_mt4 ? LLAMAHIP_GEMM_MFMA4 : LLAMAHIP_GEMM_MFMA_I8)
                    : moved(GEMM_PATH_ROWS) ? LLAMAHIP_GEMM_ROWS : moved(GEMM_PATH_SET) ? LLAMAHIP_GEMM_SET
                    : moved(GEMM_PATH_LDS) ? LLAMAHIP_GEMM_LDS : LLAMAHIP_GEMM_GEMV;
    }
    return LLAMAHIP_OK;
}

static_assert(LLAMAHIP_DENSE_AUTO == DENSE_PATH_AUTO && LLAMAHIP_DENSE_MV == DENSE_PATH_MV && LLAMAHIP_DENSE_MM == DENSE_PATH_MM && LLAMAHIP_DENSE_SET == DENSE_PATH_SET && LLAMAHIP_DENSE_MFMA == DENSE_PATH_MFMA, "llamahip.h mirrors the dense mat-mul paths");

// one f16 / f32 mat-mul kernel on caller-supplied operands (per-op tests of every kernel launch_dense_mm can pick): see llamahip.h
int llamahip_op_mul_mat_dense(const void *w, int32_t wtype, int32_t M, int32_t K, const float *x, int32_t N, const float *resid,
                              float *y, int32_t y_stride, int32_t path, int32_t *path_taken, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_mul_mat_dense";
    if (wtype != 0 && wtype != 1) { set_err(err, err_cap, "%s: wtype %d: 0 (fp32) or 1 (fp16) weights", fn, wtype); return LLAMAHIP_ERR_PREDICT; }
    if (K < 32 || K % 32 != 0) { set_err(err, err_cap, "%s: K %d must be a positive multiple of 32", fn, K); return LLAMAHIP_ERR_PREDICT; }
    if (path < LLAMAHIP_DENSE_AUTO || path > LLAMAHIP_DENSE_MFMA) { set_err(err, err_cap, "%s: unknown path %d", fn, path); return LLAMAHIP_ERR_PREDICT; }
    if (N < 1) { set_err(err, err_cap, "%s: N %d must be >= 1", fn, N); return LLAMAHIP_ERR_PREDICT; }
    if (path == LLAMAHIP_DENSE_SET && N > DENSE_SET_MAX_ROWS) { set_err(err, err_cap, "%s: path SET takes N 1 .. %d rows (got %d)", fn, DENSE_SET_MAX_ROWS, N); return LLAMAHIP_ERR_PREDICT; }
    if (y_stride < M) { set_err(err, err_cap, "%s: y_stride %d < M %d", fn, y_stride, M); return LLAMAHIP_ERR_PREDICT; }
    if (!w || !x || !y || M < 1) { set_err(err, err_cap, "%s: bad arguments (w, x, y not NULL; M %d >= 1)", fn, M); return LLAMAHIP_ERR_PREDICT; }
    // (up to 16 rows the paths are AUTO .. SET, as before the matrix-core kernel existed: it is a path of longer evals only)
    if (path == LLAMAHIP_DENSE_MFMA && N <= DENSE_SET_MAX_ROWS) {
        set_err(err, err_cap, "%s: unknown path %d for N %d rows: path MFMA takes N > %d rows", fn, path, N, DENSE_SET_MAX_ROWS);
        return LLAMAHIP_ERR_PREDICT;
    }
    if (path == LLAMAHIP_DENSE_MFMA && !dense_mfma_plan(M, K, wtype, N).ok) {
        set_err(err, err_cap, "%s: path MFMA takes N > %d rows, K a multiple of %d and N * K < 2^31 (got N %d, K %d)", fn, DENSE_SET_MAX_ROWS, DENSE_MFMA_K_UNIT, N, K);
        return LLAMAHIP_ERR_PREDICT;
    }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    DMat dm;
    dm.M = M; dm.K = K; dm.wtype = wtype;
    Scratch s;
    hipStream_t st = s.stream();
    uint8_t *d_raw = s.alloc(dm.bytes(), (const uint8_t *) w);
    dm.w = s.alloc<uint8_t>(dm.bytes());
    float *d_x = s.alloc((size_t) N * K, x);
    float *d_y = s.alloc((size_t) N * y_stride, y);      // (the floats between M and y_stride keep the caller's bits)
    float *d_r = resid ? s.alloc((size_t) N * M, resid) : nullptr;
    float *d_ws = s.alloc<float>((size_t) N * K);
    if (s.ok()) s.check(launch_dense_perm_rows(d_raw, dm, 0, M, st));
    int taken = 0;
    if (s.ok()) s.check(launch_dense_mm(dm, resid ? EPI_RESID : EPI_STORE, d_x, K, N, d_y, y_stride, d_r, M, st, d_ws, path, &taken));
    s.download(y, d_y, (size_t) N * y_stride * 4);
    s.sync();
    if (!s.ok()) return s.fail(fn, err, err_cap);
    if (path_taken) *path_taken = taken;
    return LLAMAHIP_OK;
}

// one Q4_1 mat-mul kernel on caller-supplied operands (per-op tests of both kernels launch_q41_mm can run): see llamahip.h
int llamahip_op_mul_mat_q4_1(const void *w_q4_1, int32_t M, int32_t K, const float *x, int32_t N, const float *resid,
                             float *y, int32_t y_stride, int32_t path, int32_t *path_taken, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_mul_mat_q4_1";
    if (q41_op_check(w_q4_1, M, K, x, N, y, y_stride, path, err, err_cap)) return LLAMAHIP_ERR_PREDICT;          // (q41_plan.cpp: host-only)
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    DMat dm;
    dm.M = M; dm.K = K; dm.wtype = 3;
    Scratch s;
    hipStream_t st = s.stream();
    uint8_t *d_raw = s.alloc((size_t) M * (K / 32) * 24, (const uint8_t *) w_q4_1);
    dm.w = s.alloc<uint8_t>(dm.bytes());
    dm.w2 = s.alloc<uint8_t>(dm.bytes2());
    float *d_x = s.alloc((size_t) N * K, x);
    float *d_y = s.alloc((size_t) N * y_stride, y);      // (the floats between M and y_stride keep the caller's bits)
    float *d_r = resid ? s.alloc((size_t) N * M, resid) : nullptr;
    float *d_ws = s.alloc<float>((size_t) N * K);
    if (s.ok()) s.check(launch_q41_repack(d_raw, dm, st));
    int taken = 0;
    if (s.ok()) s.check(launch_q41_mm(dm, resid ? EPI_RESID : EPI_STORE, d_x, K, N, d_y, y_stride, d_r, M, st, d_ws, path, &taken));
    s.download(y, d_y, (size_t) N * y_stride * 4);
    s.sync();
    if (!s.ok()) return s.fail(fn, err, err_cap);
    if (path_taken) *path_taken = taken;
    return LLAMAHIP_OK;
}

// one layer's attention on caller-supplied q|k|v rows and K / V caches, kernels chosen by the caller (per-op tests): see llamahip.h
int llamahip_op_attention(const float *qkv, int32_t N, int32_t d, int32_t H, int32_t n_past, int32_t n_ctx, float *Kc, float *Vc,
                          int32_t n_threads, int32_t chunk, int32_t path, int32_t ws_rows, float *merged, int32_t merged_stride,
                          void *wo_operand, int32_t *path_taken, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_attention";
    if (!qkv || !Kc || !Vc || N < 1 || d < 1 || H < 1 || d % H != 0 || n_past < 0 || chunk < 0) {
        set_err(err, err_cap, "%s: bad arguments (N %d >= 1, d %d a multiple of H %d, n_past %d >= 0, chunk %d >= 0)", fn, N, d, H, n_past, chunk);
        return LLAMAHIP_ERR_PREDICT;
    }
    const int dh = d / H, T = n_past + N, nth = n_threads;
    if (T > n_ctx) { set_err(err, err_cap, "%s: T = n_past + N = %d > n_ctx %d", fn, T, n_ctx); return LLAMAHIP_ERR_PREDICT; }
    if (merged && merged_stride < d) { set_err(err, err_cap, "%s: merged_stride %d < d %d", fn, merged_stride, d); return LLAMAHIP_ERR_PREDICT; }
    if (ws_rows < 0 || ws_rows % 64 != 0) { set_err(err, err_cap, "%s: ws_rows %d must be a positive multiple of 64 (0: 512)", fn, ws_rows); return LLAMAHIP_ERR_PREDICT; }
    if (nth < 1 || nth > 64) { set_err(err, err_cap, "%s: n_threads %d outside 1 .. 64 (the model's clamp)", fn, nth); return LLAMAHIP_ERR_PREDICT; }
    if (path < LLAMAHIP_ATTN_AUTO || path > LLAMAHIP_ATTN_DEC_STREAM) { set_err(err, err_cap, "%s: unknown path %d", fn, path); return LLAMAHIP_ERR_PREDICT; }
    if (d % 32 != 0) { set_err(err, err_cap, "%s: d %d must be a multiple of 32 (Q4_0 blocks of the wo operand)", fn, d); return LLAMAHIP_ERR_PREDICT; }
    AttnWs ws;                                       // the model's workspace, for ws_rows query rows per batch
    attn_ws_shape(ws, n_ctx, ws_rows);
    int run = path;
    if (path == LLAMAHIP_ATTN_AUTO) run = N >= 2 ? attn_path_pick(&ws, N, dh, T, nth) : -1;
    const char *why = nullptr;
    const bool dh_ok = dh % 32 == 0 && dh <= 256;
    switch (run) {
    case -1: why = "AUTO takes N >= 2 (one row is the decode step: paths DEC / DEC_STREAM)"; break;
    case LLAMAHIP_ATTN_MFMA: if (!attn_mfma_applies(&ws, N, dh, T, nth)) why = "MFMA takes N >= 2, head size 128 and n_threads <= 8"; break;
    case LLAMAHIP_ATTN_ROW: if (!dh_ok) why = "ROW takes head sizes that are multiples of 32 up to 256"; break;
    case LLAMAHIP_ATTN_SHORT: if (!attn_short_applies(&ws, N, dh)) why = "SHORT takes 2 <= N <= 60 and head sizes that are multiples of 32 up to 256"; break;
    case LLAMAHIP_ATTN_DEC: if (N != 1 || !dh_ok) why = "DEC takes N = 1 and head sizes that are multiples of 32 up to 256"; break;
    case LLAMAHIP_ATTN_DEC_STREAM:
        if (N != 1 || !dh_ok || !pv_stream_applies(dh, n_ctx, nth)) why = "DEC_STREAM takes N = 1, head sizes that are multiples of 32 up to 256, n_threads <= 32 and n_ctx <= 4096";
        break;
    }
    if (why) { set_err(err, err_cap, "%s: path %d refused for N %d, head size %d, n_threads %d: %s", fn, path, N, dh, nth, why); return LLAMAHIP_ERR_PREDICT; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    const bool dec = run == LLAMAHIP_ATTN_DEC || run == LLAMAHIP_ATTN_DEC_STREAM, quant = dec || run == LLAMAHIP_ATTN_SHORT;
    const int Kp = (d + 255) / 256 * 256;
    const size_t cache_b = (size_t) n_ctx * d * 4, qr_b = (size_t) N * d * 4;
    const size_t ms = merged ? (size_t) merged_stride : (size_t) d, mbytes = (size_t) N * ms * 4;
    const size_t qaA_b = (size_t) N * Kp, qad_b = (size_t) N * (Kp / 32) * 4;
    const AttnWsBytes wb = attn_ws_bytes(ws, H);
    std::vector<uint16_t> ts(1 << 16), te(1 << 16);
    lut_tables(ts, te);
    const std::vector<double> tab = rope_table(n_ctx, dh);
    const int32_t hs[2] = { n_past, 0 };
    Scratch s;
    hipStream_t st = s.stream();
    float *d_qr = s.alloc<float>(qr_b / 4), *d_m = s.alloc<float>(mbytes / 4), *d_qad = s.alloc<float>(qad_b / 4);
    uint32_t *d_qaA = s.alloc<uint32_t>(qaA_b / 4);
    ws.S = s.alloc<float>(wb.S / 4); ws.pmax = s.alloc<float>(wb.pmax / 4); ws.inv = s.alloc<float>(wb.inv / 4); ws.part = s.alloc<float>(wb.part / 4);
    // the op's own workspace, every byte NaN (0xFF): a read of something the launch did not write shows in the result
    s.fill(ws.S, 0xFF, wb.S); s.fill(ws.pmax, 0xFF, wb.pmax); s.fill(ws.inv, 0xFF, wb.inv); s.fill(ws.part, 0xFF, wb.part);
    s.fill(d_qr, 0xFF, qr_b);
    s.fill(d_qaA, 0xFF, qaA_b); s.fill(d_qad, 0xFF, qad_b);
    if (!merged) s.fill(d_m, 0xFF, mbytes);
    float *d_qkv = s.alloc((size_t) N * 3 * d, qkv), *d_K = s.alloc(cache_b / 4, Kc), *d_V = s.alloc(cache_b / 4, Vc);
    if (merged) s.upload(d_m, merged, mbytes);
    uint16_t *d_ts = s.alloc(ts.size(), ts.data()), *d_te = s.alloc(te.size(), te.data());
    double *d_tab = s.alloc(tab.size(), tab.data());
    int32_t *d_state = s.alloc(2, hs);
    if (s.ok()) s.check(launch_check_lut_math(d_ts, d_te, st));          // g_lut_math, as a model load leaves it
    float *mo = merged ? d_m : nullptr;
    if (s.ok() && dec) {
        s.check(launch_dec_attn(d_qkv, d, H, n_ctx, nth, d_tab, d_K, d_V, ws.S, nullptr, mo, d_qaA, d_qad, d_te, d_state, st,
                                nullptr, nullptr, run == LLAMAHIP_ATTN_DEC_STREAM));
    } else if (s.ok()) {
        s.check(launch_rope_kv(d_qkv, 3L * d, d, dh, d_tab, d_qr, d_K, d_V, n_past, N, st));
        if (s.ok() && run == LLAMAHIP_ATTN_SHORT)
            s.check(launch_attn_short(d_qr, d_K, d_V, ws.S, mo, d_qaA, d_qad, n_past, N, d, H, n_ctx, nth, d_te, st, chunk, nullptr, 0, (long) ms));
        else if (s.ok())
            s.check(launch_attn(d_qr, d_K, d_V, d_m, nullptr, nullptr, n_past, N, d, H, nth, d_te, run == LLAMAHIP_ATTN_MFMA ? &ws : nullptr, st, chunk, (long) ms));
    }
    s.download(Kc, d_K, cache_b);
    s.download(Vc, d_V, cache_b);
    if (merged) s.download(merged, d_m, mbytes);
    std::vector<uint32_t> qa(qaA_b / 4);
    std::vector<float> qd(qad_b / 4);
    if (quant && wo_operand) {
        s.download(qa.data(), d_qaA, qaA_b);
        s.download(qd.data(), d_qad, qad_b);
    }
    s.sync();
    if (!s.ok()) return s.fail(fn, err, err_cap);
    // (DEC: one row at offset 0; SHORT: rows Kp / 4 dwords and Kp / 32 scales apart)
    if (quant && wo_operand) qa_to_q4_0_blocks(qa.data(), qd.data(), N, d, (uint8_t *) wo_operand);
    if (path_taken) *path_taken = run;
    return LLAMAHIP_OK;
}

static_assert(LLAMAHIP_DEC_ATTN_X == 0 && LLAMAHIP_DEC_ATTN_STREAM == 1 && LLAMAHIP_DEC_ATTN_DMA == 2, "llamahip.h names the one-row hand-off paths");
static_assert(LLAMAHIP_DEC_KERNEL_PV_BLK == DEC_ATTN_PV_BLK && LLAMAHIP_DEC_KERNEL_X == DEC_ATTN_X && LLAMAHIP_DEC_KERNEL_PV_STREAM == DEC_ATTN_PV_STREAM &&
              LLAMAHIP_DEC_KERNEL_PV_DMA == DEC_ATTN_PV_DMA, "... and mirrors dec_attn_plan.h's kernels");

static void dec_attn_plan_out(const DecAttnPlan &p, int64_t out[8]) {
    const int64_t o[8] = { p.kernel, p.split, p.cpw, p.SR, p.NS, (int64_t) p.lds, (int64_t) p.gx * p.gy, p.threads };
    for (int i = 0; i < 8; i++) out[i] = o[i];
}
// the plan llamahip_op_dec_attention runs for (path, force): strict, the path decides long_ctx / which buffers exist / dma; the switches are not read
static DecAttnPlan dec_attn_op_plan(int d, int H, int n_ctx, int nth, int path, const int32_t *force, DecAttnForce &f) {
    if (force) { f.split = force[0]; f.stage_rows = force[1]; f.ns = force[2]; f.dma = force[3]; }
    f.strict = true;
    DecAttnPlan bad;
    const int want = path == LLAMAHIP_DEC_ATTN_X ? DEC_ATTN_X : path == LLAMAHIP_DEC_ATTN_STREAM ? DEC_ATTN_PV_STREAM : DEC_ATTN_PV_DMA;
    if (path != LLAMAHIP_DEC_ATTN_X) {
        const int dma = path == LLAMAHIP_DEC_ATTN_DMA ? 1 : 0;
        if (f.dma != -1 && f.dma != dma) { snprintf(bad.why, sizeof(bad.why), "force dma %d contradicts path %s", f.dma, dma ? "DMA" : "STREAM"); return bad; }
        f.dma = dma;
    }
    const bool lng = path != LLAMAHIP_DEC_ATTN_X;
    const DecAttnPlan p = dec_attn_plan(d, H, n_ctx, nth, lng, !lng, lng, &f);
    if (p.kernel >= 0 && p.kernel != want) {
        snprintf(bad.why, sizeof(bad.why), "%s", want == DEC_ATTN_X ? "path X takes H % 8 == 0, n_threads <= 8 and n_ctx <= 1024 (k_dec_attn_x)"
                                                                     : "paths STREAM / DMA take n_threads <= 32 and n_ctx <= 4096 (pv_stream_applies)");
        return bad;
    }
    return p;
}

int32_t llamahip_debug_dec_attn_plan(int32_t d, int32_t H, int32_t n_ctx, int32_t n_threads, int32_t long_ctx, int32_t have_sync, int32_t have_xpart,
                                     const int32_t *force, int64_t out[8], char *why, size_t why_cap) {
    DecAttnForce f;
    if (force) { f.split = force[0]; f.stage_rows = force[1]; f.ns = force[2]; f.dma = force[3]; f.strict = true; }
    const DecAttnPlan p = dec_attn_plan(d, H, n_ctx, n_threads, long_ctx != 0, have_sync != 0, have_xpart != 0, force ? &f : nullptr);
    if (why && why_cap) snprintf(why, why_cap, "%s", p.why);
    if (p.kernel < 0 || !out) return 0;
    dec_attn_plan_out(p, out);
    return 1;
}

int32_t llamahip_debug_qkv_attn_plan(int32_t d, int32_t H, int32_t n_ctx, int32_t n_threads, int32_t n_part_in, int64_t out[5], char *why, size_t why_cap) {
    char none[1];
    if (!why || !why_cap) { why = none; why_cap = sizeof(none); }
    why[0] = 0;
    if (d < 1 || H < 1 || n_ctx < 1 || n_threads < 1) { snprintf(why, why_cap, "d %d, H %d, n_ctx %d and n_threads %d must be >= 1", d, H, n_ctx, n_threads); return 0; }
    QMat w;
    w.set_shape(3 * d, d);
    if (!qkv_attn_shape_ok(d, H, n_threads, w.M, w.K, w.ngroups, w.gmapF8, why, why_cap)) return 0;
    NormPart np;
    // (a non-null marker: the query resolves the prologue, nothing is read)
    if (n_part_in > 0) { np.in = (const double *) (uintptr_t) 16; np.n_in = n_part_in; }
    long o[5];
    if (!qkv_attn_applies(w, d, H, n_threads) || !qkv_attn_launch_query(w, np, d, H, n_ctx, n_threads, o)) {
        snprintf(why, why_cap, "the wq|wk|wv mat-vec of d %d is not a 4-wave ring of depth 8 / 10 / 4 (or LLAMAHIP_NO_QKV_ATTN is set): no instance of k_qkv_attn", d);
        return 0;
    }
    for (int i = 0; out && i < 5; i++) out[i] = o[i];
    return 1;
}

// n_steps decode steps of one layer's attention through ONE of the hand-off kernels, on hand-off buffers that live across the steps: see llamahip.h
int llamahip_op_dec_attention(const float *qkv, int32_t n_steps, const int32_t *n_past, const int32_t *layer, const int32_t *bump_epoch, uint32_t epoch0,
                              int32_t d, int32_t H, int32_t n_ctx, float *Kc, float *Vc, int32_t n_threads, int32_t path, const int32_t *force,
                              float *merged, void *wo_operand, uint32_t *fault, int64_t *plan, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_dec_attention";
    if (!qkv || !n_past || !layer || !bump_epoch || !Kc || !Vc || !merged || !fault) { set_err(err, err_cap, "%s: null operand (qkv, n_past, layer, bump_epoch, Kc, Vc, merged, fault)", fn); return LLAMAHIP_ERR_PREDICT; }
    if (n_steps < 1 || n_steps > 64) { set_err(err, err_cap, "%s: n_steps %d outside 1 .. 64", fn, n_steps); return LLAMAHIP_ERR_PREDICT; }
    if (path < LLAMAHIP_DEC_ATTN_X || path > LLAMAHIP_DEC_ATTN_DMA) { set_err(err, err_cap, "%s: unknown path %d (X, STREAM, DMA)", fn, path); return LLAMAHIP_ERR_PREDICT; }
    if (d < 1 || H < 1 || d % H != 0 || d % 32 != 0) { set_err(err, err_cap, "%s: d %d must be a multiple of H %d and of 32", fn, d, H); return LLAMAHIP_ERR_PREDICT; }
    const int dh = d / H, nth = n_threads;
    DecAttnForce f;
    const DecAttnPlan p = dec_attn_op_plan(d, H, n_ctx, nth, path, force, f);
    if (p.kernel < 0) { set_err(err, err_cap, "%s: path %d refused for d %d, H %d, n_ctx %d, n_threads %d: %s", fn, path, d, H, n_ctx, nth, p.why); return LLAMAHIP_ERR_PREDICT; }
    const bool tags = path != LLAMAHIP_DEC_ATTN_X;
    bool used[TAG_MAX_LAYERS] = { false };      // layers whose tag (epoch, layer + 1) this epoch has spent
    for (int i = 0; i < n_steps; i++) {
        if (n_past[i] < 0 || n_past[i] >= n_ctx) { set_err(err, err_cap, "%s: step %d: n_past %d outside [0, n_ctx = %d)", fn, i, n_past[i], n_ctx); return LLAMAHIP_ERR_PREDICT; }
        if (layer[i] < 0 || layer[i] >= TAG_MAX_LAYERS) { set_err(err, err_cap, "%s: step %d: layer %d outside 0 .. %d", fn, i, layer[i], TAG_MAX_LAYERS - 1); return LLAMAHIP_ERR_PREDICT; }
        if (bump_epoch[i]) std::fill(used, used + TAG_MAX_LAYERS, false);
        if (tags && p.split > 1 && used[layer[i]]) {
            set_err(err, err_cap, "%s: step %d: layer %d again under one epoch: a forward pass spends each tag once (bump_epoch)", fn, i, layer[i]); return LLAMAHIP_ERR_PREDICT;
        }
        used[layer[i]] = true;
    }
    if (plan) dec_attn_plan_out(p, plan);
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    const int Kp = (d + 255) / 256 * 256;
    const size_t cache_b = (size_t) n_ctx * d * 4, qaA_b = (size_t) Kp, qad_b = (size_t) (Kp / 32) * 4, sc_b = (size_t) H * n_ctx * 4;
    std::vector<uint16_t> ts(1 << 16), te(1 << 16);
    lut_tables(ts, te);
    const std::vector<double> tab = rope_table(n_ctx, dh);
    std::vector<int32_t> hs((size_t) n_steps * 2, 0);
    for (int i = 0; i < n_steps; i++) hs[2 * i] = n_past[i];
    Scratch s;
    hipStream_t st = s.stream();
    // the placement every hand-off here relies on, asked as a model load asks (H x (column blocks + score slices) workgroups; head counts
    // that are no multiple of 8 -- no model handle splits those -- ask for the 1-D rule over as many workgroups)
    const int Y = dh / 32 + (n_ctx + 31) / 32;
    if (s.ok() && !(H % 8 == 0 ? xcd_selftest(H, Y, st) : xcd_selftest(8, (H * Y + 7) / 8, st))) {
        set_err(err, err_cap, "%s: the hand-off kernels need the workgroups of a head on one XCD; this device does not place them so", fn); return LLAMAHIP_ERR_PREDICT;
    }
    float *d_m = s.alloc<float>((size_t) d), *d_qad = s.alloc<float>(qad_b / 4), *d_sc = s.alloc<float>(sc_b / 4);
    uint32_t *d_qaA = s.alloc<uint32_t>(qaA_b / 4);
    // the op's own workspace, every byte NaN (0xFF): a read of something the launch did not write shows in the result
    s.fill(d_sc, 0xFF, sc_b); s.fill(d_qaA, 0xFF, qaA_b); s.fill(d_qad, 0xFF, qad_b);
    float *d_qkv = s.alloc((size_t) n_steps * 3 * d, qkv), *d_K = s.alloc(cache_b / 4, Kc), *d_V = s.alloc(cache_b / 4, Vc);
    uint16_t *d_ts = s.alloc(ts.size(), ts.data()), *d_te = s.alloc(te.size(), te.data());
    double *d_tab = s.alloc(tab.size(), tab.data());
    int32_t *d_state = s.alloc(hs.size(), hs.data());
    // the hand-off state, sized and zeroed ONCE as a model load does and never cleared between the steps: the heads' counters, the tagged
    // partial sums, the epoch word ([0]) and the fault word ([4])
    uint32_t *d_sync = s.alloc<uint32_t>((size_t) H * 32), *d_words = s.alloc<uint32_t>(8);
    uint64_t *d_xpart = s.alloc<uint64_t>((size_t) d * 32);
    s.fill(d_sync, 0, (size_t) H * 32 * 4); s.fill(d_xpart, 0, (size_t) d * 32 * 8); s.fill(d_words, 0, 32);
    s.upload(d_words, &epoch0, 4);
    if (s.ok()) s.check(launch_check_lut_math(d_ts, d_te, st));          // g_lut_math, as a model load leaves it
    std::vector<uint32_t> qa(qaA_b / 4);
    std::vector<float> qd(qad_b / 4);
    for (int i = 0; i < n_steps && s.ok(); i++) {
        fault[i] = 0xFFFFFFFFu;
        s.fill(d_m, 0xFF, (size_t) d * 4);
        if (bump_epoch[i]) s.check(launch_bump_epoch(d_words, st));
        if (s.ok()) s.check(launch_dec_attn(d_qkv + (size_t) i * 3 * d, d, H, n_ctx, nth, d_tab, d_K, d_V, d_sc, nullptr, d_m, d_qaA, d_qad, d_te, d_state + 2 * i, st,
                                            tags ? nullptr : d_sync, d_words + 4, tags, tags ? d_xpart : nullptr, d_words, layer[i], &f));
        s.download(merged + (size_t) i * d, d_m, (size_t) d * 4);
        s.download(fault + i, d_words + 4, 4);
        if (wo_operand) { s.download(qa.data(), d_qaA, qaA_b); s.download(qd.data(), d_qad, qad_b); }
        s.sync();
        if (!s.ok()) break;
        if (wo_operand) qa_to_q4_0_blocks(qa.data(), qd.data(), 1, d, (uint8_t *) wo_operand + (size_t) i * (d / 32) * 20);
        if (fault[i] != 0u) {      // a hand-off timed out: the results of that launch are invalid and nothing more is launched
            set_err(err, err_cap, "%s: step %d (n_past %d, layer %d): the fault word is %#x: a hand-off between workgroups timed out", fn, i, n_past[i], layer[i], fault[i]);
            return LLAMAHIP_ERR_PREDICT;
        }
    }
    s.download(Kc, d_K, cache_b);
    s.download(Vc, d_V, cache_b);
    s.sync();
    return s.ok() ? LLAMAHIP_OK : s.fail(fn, err, err_cap);
}

// n_steps decode steps of the fused wq|wk|wv + attention launch (k_qkv_attn) on hand-off buffers that live across the steps: see llamahip.h
int llamahip_op_qkv_attn(const void *w_q4_0, const float *norm_w, int32_t d, int32_t H, int32_t n_ctx, float *Kc, float *Vc, int32_t n_threads,
                         int32_t n_steps, const float *x, const double *part_in, const int32_t *n_part, int32_t part_stride,
                         const int32_t *n_past, const int32_t *layer, const int32_t *bump_epoch, uint32_t epoch0, int32_t tagged_in,
                         float *merged, void *wo_operand, uint32_t *fault, int64_t *plans, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_qkv_attn";
    if (tagged_in) { set_err(err, err_cap, "%s: PREP_NORM_TAG waits on another pipeline stage's mailbox: the op launches the NORM / NORMP prologues only", fn); return LLAMAHIP_ERR_PREDICT; }
    if (!w_q4_0 || !norm_w || !Kc || !Vc || !x || !n_part || !n_past || !layer || !bump_epoch || !merged || !fault) {
        set_err(err, err_cap, "%s: null operand (w, norm_w, Kc, Vc, x, n_part, n_past, layer, bump_epoch, merged, fault)", fn); return LLAMAHIP_ERR_PREDICT;
    }
    if (n_steps < 1 || n_steps > 64) { set_err(err, err_cap, "%s: n_steps %d outside 1 .. 64", fn, n_steps); return LLAMAHIP_ERR_PREDICT; }
    if (n_ctx < 1 || n_ctx > 4096) { set_err(err, err_cap, "%s: n_ctx %d outside 1 .. 4096", fn, n_ctx); return LLAMAHIP_ERR_PREDICT; }
    if (d < 1 || d % 256 != 0) { set_err(err, err_cap, "%s: d %d must be a positive multiple of 256", fn, d); return LLAMAHIP_ERR_PREDICT; }
    const int nth = n_threads;
    if (nth < 1) { set_err(err, err_cap, "%s: n_threads %d must be >= 1", fn, nth); return LLAMAHIP_ERR_PREDICT; }
    QMat q;
    q.set_shape(3 * d, d);
    char why[200] = "";
    if (!qkv_attn_shape_ok(d, H, nth, q.M, q.K, q.ngroups, q.gmapF8, why, sizeof(why))) { set_err(err, err_cap, "%s: k_qkv_attn does not take d %d, H %d, n_threads %d: %s", fn, d, H, nth, why); return LLAMAHIP_ERR_PREDICT; }
    if (!qkv_attn_applies(q, d, H, nth)) {
        set_err(err, err_cap, "%s: k_qkv_attn has no instance for d %d: its mat-vec role must be a 4-wave ring of (depth, granules) (8, 1), (10, 2) or (4, 2) (llamahip_debug_qkv_attn_plan)", fn, d);
        return LLAMAHIP_ERR_PREDICT;
    }
    bool used[TAG_MAX_LAYERS] = { false };      // layers whose tag (epoch, layer + 1) this epoch has spent
    int max_part = 0;
    for (int i = 0; i < n_steps; i++) {
        if (n_past[i] < 0 || n_past[i] >= n_ctx) { set_err(err, err_cap, "%s: step %d: n_past %d outside [0, n_ctx = %d)", fn, i, n_past[i], n_ctx); return LLAMAHIP_ERR_PREDICT; }
        if (layer[i] < 0 || layer[i] >= TAG_MAX_LAYERS) { set_err(err, err_cap, "%s: step %d: layer %d outside 0 .. %d", fn, i, layer[i], TAG_MAX_LAYERS - 1); return LLAMAHIP_ERR_PREDICT; }
        if (n_part[i] < 0 || n_part[i] > NORM_PART_MAX || (n_part[i] > 0 && (!part_in || part_stride < n_part[i]))) {
            set_err(err, err_cap, "%s: step %d: n_part %d outside 0 .. %d (NORM_PART_MAX), or part_in missing / part_stride %d too small", fn, i, n_part[i], NORM_PART_MAX, part_stride); return LLAMAHIP_ERR_PREDICT;
        }
        if (bump_epoch[i]) std::fill(used, used + TAG_MAX_LAYERS, false);
        if (used[layer[i]]) { set_err(err, err_cap, "%s: step %d: layer %d again under one epoch: a forward pass spends each tag once (bump_epoch)", fn, i, layer[i]); return LLAMAHIP_ERR_PREDICT; }
        used[layer[i]] = true;
        max_part = std::max(max_part, n_part[i]);
        long lp[5];
        NormPart np;
        if (n_part[i] > 0) { np.in = part_in + (size_t) i * part_stride * 2; np.n_in = n_part[i]; }
        if (!qkv_attn_launch_query(q, np, d, H, n_ctx, nth, lp)) { set_err(err, err_cap, "%s: step %d: no launch", fn, i); return LLAMAHIP_ERR_PREDICT; }
        if ((size_t) lp[4] > GEMV_LDS_CAP) { set_err(err, err_cap, "%s: %ld bytes of LDS, the kernels' cap is %zu", fn, lp[4], GEMV_LDS_CAP); return LLAMAHIP_ERR_PREDICT; }
        if (plans) for (int k = 0; k < 5; k++) plans[(size_t) i * 5 + k] = lp[k];
    }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    const int dh = d / H, Kp = q.Kp();
    const size_t nb = (size_t) d / 32, cache_b = (size_t) n_ctx * d * 4, qaA_b = (size_t) Kp, qad_b = (size_t) (Kp / 32) * 4;
    std::vector<uint16_t> ts(1 << 16), te(1 << 16);
    lut_tables(ts, te);
    const std::vector<double> tab = rope_table(n_ctx, dh);
    std::vector<int32_t> hs((size_t) n_steps * 2, 0);
    for (int i = 0; i < n_steps; i++) hs[2 * i] = n_past[i];
    Scratch s;
    hipStream_t st = s.stream();
    if (s.ok() && !xcd_selftest(H, dh / 32 + (n_ctx + 31) / 32, st)) {
        set_err(err, err_cap, "%s: k_qkv_attn needs the workgroups of a head on one XCD; this device does not place them so", fn); return LLAMAHIP_ERR_PREDICT;
    }
    uint8_t *d_w = s.alloc((size_t) q.M * nb * 20, (const uint8_t *) w_q4_0);
    q.tiles = s.alloc<uint8_t>(q.bytes());
    float *d_nw = s.alloc((size_t) d, norm_w), *d_x = s.alloc((size_t) n_steps * d, x);
    double *d_pi = max_part > 0 ? s.alloc((size_t) n_steps * part_stride * 2, part_in) : nullptr;
    float *d_m = s.alloc<float>((size_t) d), *d_qad = s.alloc<float>(qad_b / 4);
    uint32_t *d_qaA = s.alloc<uint32_t>(qaA_b / 4);
    s.fill(d_qaA, 0xFF, qaA_b); s.fill(d_qad, 0xFF, qad_b);
    float *d_K = s.alloc(cache_b / 4, Kc), *d_V = s.alloc(cache_b / 4, Vc);
    uint16_t *d_ts = s.alloc(ts.size(), ts.data()), *d_te = s.alloc(te.size(), te.data());
    double *d_tab = s.alloc(tab.size(), tab.data());
    int32_t *d_state = s.alloc(hs.size(), hs.data());
    // the hand-off state, sized and zeroed ONCE as a model load does and never cleared between the steps: the tagged q|k|v row, the tagged
    // scores, the epoch word ([0]) and the fault word ([4])
    uint64_t *d_qkv2 = s.alloc<uint64_t>((size_t) 3 * d), *d_sc2 = s.alloc<uint64_t>((size_t) H * n_ctx);
    uint32_t *d_words = s.alloc<uint32_t>(8);
    s.fill(d_qkv2, 0, (size_t) 3 * d * 8); s.fill(d_sc2, 0, (size_t) H * n_ctx * 8); s.fill(d_words, 0, 32);
    s.upload(d_words, &epoch0, 4);
    if (s.ok()) s.check(launch_check_lut_math(d_ts, d_te, st));          // g_lut_math, as a model load leaves it
    if (s.ok()) s.check(launch_repack(d_w, q.tiles, q.M, q.K, 0, 0, st));
    std::vector<uint32_t> qa(qaA_b / 4);
    std::vector<float> qd(qad_b / 4);
    for (int i = 0; i < n_steps && s.ok(); i++) {
        fault[i] = 0xFFFFFFFFu;
        s.fill(d_m, 0xFF, (size_t) d * 4);
        if (bump_epoch[i]) s.check(launch_bump_epoch(d_words, st));
        NormPart np;
        if (n_part[i] > 0) { np.in = d_pi + (size_t) i * part_stride * 2; np.n_in = n_part[i]; }
        if (s.ok()) s.check(launch_qkv_attn(q, d_x + (size_t) i * d, d_nw, np, d_qkv2, d_sc2, d_words, layer[i], d, H, n_ctx, nth, d_tab, d_K, d_V, d_m, d_qaA, d_qad,
                                            d_ts, d_te, d_state + 2 * i, d_words + 4, st, nullptr));
        s.download(merged + (size_t) i * d, d_m, (size_t) d * 4);
        s.download(fault + i, d_words + 4, 4);
        if (wo_operand) { s.download(qa.data(), d_qaA, qaA_b); s.download(qd.data(), d_qad, qad_b); }
        s.sync();
        if (!s.ok()) break;
        if (wo_operand) qa_to_q4_0_blocks(qa.data(), qd.data(), 1, d, (uint8_t *) wo_operand + (size_t) i * (d / 32) * 20);
        if (fault[i] != 0u) {      // a hand-off timed out: the results of that launch are invalid and nothing more is launched
            set_err(err, err_cap, "%s: step %d (n_past %d, layer %d): the fault word is %#x: a hand-off between workgroups timed out", fn, i, n_past[i], layer[i], fault[i]);
            return LLAMAHIP_ERR_PREDICT;
        }
    }
    s.download(Kc, d_K, cache_b);
    s.download(Vc, d_V, cache_b);
    s.sync();
    return s.ok() ? LLAMAHIP_OK : s.fail(fn, err, err_cap);
}

// the attention of llamahip_eval_multi's pass on caller-supplied rows, caches and row table (per-op tests of rows_attn.hip): see llamahip.h
int llamahip_op_attention_rows(const float *qkv, int32_t R, int32_t d, int32_t H, int32_t n_ctx, int32_t n_slots, float *Kc, float *Vc,
                               const int32_t *row_slot, const int32_t *row_pos, const int32_t *row_keys, int32_t n_threads,
                               float *merged, int32_t merged_stride, void *wo_operand, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_attention_rows";
    if (!qkv || !Kc || !Vc || d < 1 || H < 1 || d % H != 0) { set_err(err, err_cap, "%s: bad arguments (qkv, Kc, Vc not NULL; d %d a multiple of H %d)", fn, d, H); return LLAMAHIP_ERR_PREDICT; }
    const int dh = d / H, nth = n_threads;
    if (dh % 32 != 0 || dh > 256) { set_err(err, err_cap, "%s: head size %d: multiples of 32 up to 256", fn, dh); return LLAMAHIP_ERR_PREDICT; }
    if (nth < 1 || nth > 64) { set_err(err, err_cap, "%s: n_threads %d outside 1 .. 64 (the model's clamp)", fn, nth); return LLAMAHIP_ERR_PREDICT; }
    if (merged && merged_stride < d) { set_err(err, err_cap, "%s: merged_stride %d < d %d", fn, merged_stride, d); return LLAMAHIP_ERR_PREDICT; }
    if (rows_table_check(R, n_ctx, n_slots, row_slot, row_pos, row_keys, err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    std::vector<RowTab> tab_h((size_t) R);
    int max_keys = 1;
    for (int r = 0; r < R; r++) {
        tab_h[r] = { row_pos[r], row_keys[r], (long) row_slot[r] * n_ctx * d };
        max_keys = std::max(max_keys, row_pos[r] + 1);
    }
    const int Kp = (d + 255) / 256 * 256, sc_rows = 16;      // (a scratch of 16 rows: 29 and 64 rows walk it in batches)
    const size_t cache_b = (size_t) n_slots * n_ctx * d * 4, ms = merged ? (size_t) merged_stride : (size_t) d, mbytes = (size_t) R * ms * 4;
    const size_t qaA_b = (size_t) R * Kp, qad_b = (size_t) R * (Kp / 32) * 4, sc_b = (size_t) sc_rows * H * n_ctx * 4;
    std::vector<uint16_t> ts(1 << 16), te(1 << 16);
    lut_tables(ts, te);
    const std::vector<double> tab = rope_table(n_ctx, dh);
    Scratch s;
    hipStream_t st = s.stream();
    float *d_qr = s.alloc<float>((size_t) R * d), *d_m = s.alloc<float>(mbytes / 4), *d_qad = s.alloc<float>(qad_b / 4), *d_sc = s.alloc<float>(sc_b / 4);
    uint32_t *d_qaA = s.alloc<uint32_t>(qaA_b / 4);
    // the op's own workspace, every byte NaN (0xFF): a read of something the launches did not write shows in the result
    s.fill(d_sc, 0xFF, sc_b); s.fill(d_qr, 0xFF, (size_t) R * d * 4); s.fill(d_qaA, 0xFF, qaA_b); s.fill(d_qad, 0xFF, qad_b);
    if (!merged) s.fill(d_m, 0xFF, mbytes);
    float *d_qkv = s.alloc((size_t) R * 3 * d, qkv), *d_K = s.alloc(cache_b / 4, Kc), *d_V = s.alloc(cache_b / 4, Vc);
    if (merged) s.upload(d_m, merged, mbytes);
    uint16_t *d_ts = s.alloc(ts.size(), ts.data()), *d_te = s.alloc(te.size(), te.data());
    double *d_tab = s.alloc(tab.size(), tab.data());
    RowTab *d_rows = s.alloc(tab_h.size(), tab_h.data());
    if (s.ok()) s.check(launch_check_lut_math(d_ts, d_te, st));          // g_lut_math, as a model load leaves it
    if (s.ok()) s.check(launch_rope_kv_rows(d_qkv, 3L * d, d, dh, d_tab, d_qr, d_K, d_V, d_rows, R, st));
    if (s.ok()) s.check(launch_attn_rows(d_qr, d_K, d_V, d_sc, sc_rows, merged ? d_m : nullptr, (long) ms, d_qaA, d_qad, d_rows, nullptr, R, max_keys, d, H, n_ctx, nth, d_te, st));
    s.download(Kc, d_K, cache_b);
    s.download(Vc, d_V, cache_b);
    if (merged) s.download(merged, d_m, mbytes);
    std::vector<uint32_t> qa(qaA_b / 4);
    std::vector<float> qd(qad_b / 4);
    if (wo_operand) {
        s.download(qa.data(), d_qaA, qaA_b);
        s.download(qd.data(), d_qad, qad_b);
    }
    s.sync();
    if (!s.ok()) return s.fail(fn, err, err_cap);
    if (wo_operand) qa_to_q4_0_blocks(qa.data(), qd.data(), R, d, (uint8_t *) wo_operand);
    return LLAMAHIP_OK;
}

// one k_kv_shift_rows launch on caller-supplied caches [n_slots][n_layers][n_ctx][d] with rope_table(n_ctx, dh) (per-op tests of kv_shift.hip): see llamahip.h
int llamahip_op_kv_shift(float *Kc, float *Vc, int32_t n_slots, int32_t n_layers, int32_t n_ctx, int32_t d, int32_t dh, int32_t n_shifts,
                         const int32_t *slot, const int32_t *row_begin, const int32_t *n_rows, const int32_t *n_discard, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_kv_shift";
    if (!Kc || !Vc || n_slots < 1 || n_layers < 1 || n_ctx < 1) { set_err(err, err_cap, "%s: bad arguments (Kc, Vc not NULL; n_slots %d, n_layers %d, n_ctx %d all >= 1)", fn, n_slots, n_layers, n_ctx); return LLAMAHIP_ERR_PREDICT; }
    if (d < 4 || d % 4 != 0) { set_err(err, err_cap, "%s: d (%d) must be a positive multiple of 4 (rows move in 16-byte granules)", fn, d); return LLAMAHIP_ERR_PREDICT; }
    if (dh < 2 || dh % 2 != 0 || d % dh != 0) { set_err(err, err_cap, "%s: head size %d must be even and divide d (%d)", fn, dh, d); return LLAMAHIP_ERR_PREDICT; }
    KvShiftTab tab;
    if (kv_shift_table_check(n_slots, "", n_ctx, n_shifts, slot, row_begin, n_rows, n_discard, tab, fn, err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t cache = (size_t) n_slots * n_layers * n_ctx * d;
    const std::vector<double> rt = rope_table(n_ctx, dh);
    Scratch s;
    hipStream_t st = s.stream();
    float *d_K = s.alloc(cache, Kc), *d_V = s.alloc(cache, Vc);
    double *d_tab = s.alloc(rt.size(), rt.data());
    if (s.ok()) s.check(launch_kv_shift_rows(d_K, d_V, d_tab, tab, n_slots, n_layers, n_ctx, d, dh, st));
    s.download(Kc, d_K, cache * 4);
    s.download(Vc, d_V, cache * 4);
    s.sync();
    return s.ok() ? LLAMAHIP_OK : s.fail(fn, err, err_cap);
}

// host-only: the library's RoPE angle table [n_ctx][dh / 2][cos, sin] (rope_table: what a model load and the ops upload)
int32_t llamahip_debug_rope_table(int32_t n_ctx, int32_t dh, double *out) {
    if (n_ctx < 1 || dh < 2 || dh % 2 != 0 || !out) return -1;
    const std::vector<double> rt = rope_table(n_ctx, dh);
    memcpy(out, rt.data(), rt.size() * sizeof(double));
    return 0;
}

// host-only: the attention path a model's multi-row eval of N rows after n_past takes once its workspace exists (ensure_attn_ws)
int32_t llamahip_debug_attn_path(int32_t N, int32_t head_size, int32_t n_past, int32_t n_threads, int32_t n_ctx) {
    AttnWs ws;
    attn_ws_shape(ws, n_ctx);
    if (N < 2) return -1;
    return attn_path_pick(&ws, N, head_size, n_past + N, std::max(1, std::min((int) n_threads, 64)));
}

// the device half of the sampler on caller-supplied logits (parity tests): see llamahip_eval_topk
int llamahip_op_topk(const float *logits, int32_t n_vocab, const int32_t *last_n_tokens, int32_t n_last, double repeat_penalty,
                     int32_t top_k, double temp, double *cand_scores, int32_t *cand_ids, int32_t *exact, char *err, size_t err_cap) {
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    if (!logits || !cand_scores || !cand_ids || !exact || n_vocab < 1 || n_vocab > 32768 || top_k < 1 || top_k > 64 || top_k > n_vocab || n_last < 0 || n_last > 1024) {
        set_err(err, err_cap, "llamahip_op_topk: bad arguments"); return LLAMAHIP_ERR_PREDICT;
    }
    Scratch s;
    char *d_w = s.alloc<char>(8192 + TOPK_WS_BYTES);      // window [1024] | TopkOut at 4096 | from 8192: the selection's workspace
    s.fill(d_w, 0, 8192 + TOPK_WS_BYTES);
    float *d_l = s.alloc((size_t) n_vocab, logits);
    int32_t *d_win = (int32_t *) d_w;
    TopkOut *d_out = d_w ? (TopkOut *) (d_w + 4096) : nullptr;
    TopkOut h;
    if (n_last > 0) s.upload(d_win, last_n_tokens, (size_t) n_last * 4);
    if (s.ok()) s.check(launch_topk_candidates(d_l, n_vocab, d_win, n_last, 1.0 / temp, repeat_penalty, top_k, d_out->sc, d_out->id, d_out->fl, nullptr, d_w + 8192));
    s.download(&h, d_out, sizeof(h));
    if (!s.ok()) return s.fail("llamahip_op_topk", err, err_cap);
    *exact = h.fl[0];
    for (int i = 0; i < top_k; i++) { cand_scores[i] = h.sc[i]; cand_ids[i] = h.id[i]; }
    return LLAMAHIP_OK;
}

// the batched device half of the sampler on caller-supplied rows (parity tests): see llamahip_decode_sample_multi
int llamahip_op_topk_rows(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *windows, const int32_t *n_last, double repeat_penalty,
                          int32_t top_k, double temp, double *out_scores, int32_t *out_ids, int32_t *out_exact, float *out_spill, char *err, size_t err_cap) {
    if (!logits || !windows || !n_last || !out_scores || !out_ids || !out_exact || n_rows < 1 || n_vocab < 1 || n_vocab > 32768 || top_k < 1 || top_k > 64 || top_k > n_vocab) {
        set_err(err, err_cap, "llamahip_op_topk_rows: bad arguments (n_rows %d, n_vocab %d <= 32768, top_k %d in [1, min(64, n_vocab)])", n_rows, n_vocab, top_k); return LLAMAHIP_ERR_PREDICT;
    }
    for (int r = 0; r < n_rows; r++)
        if (n_last[r] < 0) { set_err(err, err_cap, "llamahip_op_topk_rows: n_last[%d] = %d", r, n_last[r]); return LLAMAHIP_ERR_PREDICT; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t R = n_rows, V = n_vocab;
    std::vector<TopkOut> h(R);
    Scratch s;
    char *d_ws = s.alloc<char>(R * TOPK_WS_BYTES);
    s.fill(d_ws, 0, R * TOPK_WS_BYTES);
    float *d_l = s.alloc(R * V, logits);
    int32_t *d_win = s.alloc<int32_t>(R * 1024 + R);      // the windows, then n_last
    s.upload(d_win, windows, R * 1024 * 4);
    if (s.ok()) s.upload(d_win + R * 1024, n_last, R * 4);
    float *d_sp = out_spill ? s.alloc(R * V, out_spill) : nullptr;      // (rows that are not spilled keep the caller's bits)
    TopkOut *d_out = s.alloc<TopkOut>(R);
    if (s.ok()) s.check(launch_topk_rows(d_l, n_rows, n_vocab, d_win, d_win + R * 1024, 1.0 / temp, repeat_penalty, top_k, d_out, d_sp, nullptr, d_ws));
    s.download(h.data(), d_out, R * sizeof(TopkOut));
    if (out_spill) s.download(out_spill, d_sp, R * V * 4);
    if (!s.ok()) return s.fail("llamahip_op_topk_rows", err, err_cap);
    for (size_t r = 0; r < R; r++) {
        out_exact[r] = h[r].fl[0];
        for (int i = 0; i < top_k; i++) { out_scores[r * 64 + i] = h[r].sc[i]; out_ids[r * 64 + i] = h[r].id[i]; }
    }
    return LLAMAHIP_OK;
}

// k_topk_keys_slide + k_topk_select_rows on caller-supplied rows (parity tests): see llamahip_verify_sample
int llamahip_op_topk_slide(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *ids, int32_t n_last, double repeat_penalty,
                           int32_t top_k, double temp, double *out_scores, int32_t *out_ids, int32_t *out_exact, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_topk_slide";
    if (n_rows < 1 || n_rows > VERIFY_ROWS_MAX) { set_err(err, err_cap, "%s: n_rows must be 1 .. %d (got %d): a verify step has at most %d rows", fn, VERIFY_ROWS_MAX, n_rows, VERIFY_ROWS_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (n_vocab < 1 || n_vocab > 32768) { set_err(err, err_cap, "%s: n_vocab must be 1 .. 32768 (got %d)", fn, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (top_k < 1 || top_k > 64 || top_k > n_vocab) { set_err(err, err_cap, "%s: top_k must be 1 .. min(64, n_vocab) (got %d, n_vocab %d)", fn, top_k, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (n_last < 0 || n_last > 1024) { set_err(err, err_cap, "%s: n_last must be 0 .. 1024 (got %d): the device takes windows of up to 1024 ids", fn, n_last); return LLAMAHIP_ERR_PREDICT; }
    const size_t R = n_rows, V = n_vocab, n_ids = (size_t) n_last + R - 1;
    if (!logits || !out_scores || !out_ids || !out_exact || (n_ids > 0 && !ids)) { set_err(err, err_cap, "%s: null argument", fn); return LLAMAHIP_ERR_PREDICT; }
    if (!(temp > 0.0) || !(repeat_penalty > 0.0)) { set_err(err, err_cap, "%s: temp (%g) and repeat_penalty (%g) must be positive", fn, temp, repeat_penalty); return LLAMAHIP_ERR_PREDICT; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    std::vector<TopkOut> h(R);
    Scratch s;
    char *d_ws = s.alloc<char>(R * TOPK_WS_BYTES);
    s.fill(d_ws, 0, R * TOPK_WS_BYTES);
    float *d_l = s.alloc(R * V, logits);
    int32_t *d_ids = s.alloc<int32_t>(n_ids + 1);
    if (n_ids > 0) s.upload(d_ids, ids, n_ids * 4);
    TopkOut *d_out = s.alloc<TopkOut>(R);
    if (s.ok()) s.check(launch_topk_slide(d_l, n_rows, n_vocab, d_ids, n_last, 1.0 / temp, repeat_penalty, top_k, d_out, nullptr, d_ws));
    s.download(h.data(), d_out, R * sizeof(TopkOut));
    if (!s.ok()) return s.fail(fn, err, err_cap);
    for (size_t r = 0; r < R; r++) {
        out_exact[r] = h[r].fl[0];
        for (int i = 0; i < top_k; i++) { out_scores[r * 64 + i] = h[r].sc[i]; out_ids[r * 64 + i] = h[r].id[i]; }
    }
    return LLAMAHIP_OK;
}

// k_topk_keys_slide_set + k_topk_select_rows on caller-supplied rows cut into segments (parity tests): see llamahip_verify_sample_multi
int llamahip_op_topk_slide_set(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *ids, int32_t n_ids, const int32_t *seg_begin, int32_t n_segs,
                               const int32_t *seg_ids_off, const int32_t *seg_n_last, double repeat_penalty, int32_t top_k, double temp,
                               double *out_scores, int32_t *out_ids, int32_t *out_exact, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_topk_slide_set";
    if (n_rows < 1 || n_rows > VERIFY_ROWS_MAX) { set_err(err, err_cap, "%s: n_rows must be 1 .. %d (got %d): a verify step has at most %d rows", fn, VERIFY_ROWS_MAX, n_rows, VERIFY_ROWS_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (n_vocab < 1 || n_vocab > 32768) { set_err(err, err_cap, "%s: n_vocab must be 1 .. 32768 (got %d)", fn, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (top_k < 1 || top_k > 64 || top_k > n_vocab) { set_err(err, err_cap, "%s: top_k must be 1 .. min(64, n_vocab) (got %d, n_vocab %d)", fn, top_k, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (!logits || !out_scores || !out_ids || !out_exact || !seg_begin || !seg_ids_off || !seg_n_last || n_ids < 0 || (n_ids > 0 && !ids)) { set_err(err, err_cap, "%s: null argument (or n_ids %d < 0)", fn, n_ids); return LLAMAHIP_ERR_PREDICT; }
    if (!(temp > 0.0) || !(repeat_penalty > 0.0)) { set_err(err, err_cap, "%s: temp (%g) and repeat_penalty (%g) must be positive", fn, temp, repeat_penalty); return LLAMAHIP_ERR_PREDICT; }
    if (n_segs < 1 || n_segs > n_rows) { set_err(err, err_cap, "%s: n_segs must be 1 .. n_rows (%d; got %d)", fn, n_rows, n_segs); return LLAMAHIP_ERR_PREDICT; }
    if (seg_begin[0] != 0 || seg_begin[n_segs] != n_rows) { set_err(err, err_cap, "%s: seg_begin must run from 0 to n_rows (%d; got %d .. %d)", fn, n_rows, seg_begin[0], seg_begin[n_segs]); return LLAMAHIP_ERR_PREDICT; }
    int32_t tab[2 * VERIFY_ROWS_MAX] = { 0 };          // row_off[16] | row_n_last[16]
    for (int s = 0; s < n_segs; s++) {
        if (seg_begin[s + 1] <= seg_begin[s]) { set_err(err, err_cap, "%s: seg_begin must ascend strictly (segment %d: %d .. %d)", fn, s, seg_begin[s], seg_begin[s + 1]); return LLAMAHIP_ERR_PREDICT; }
        const int rows = seg_begin[s + 1] - seg_begin[s];
        if (seg_ids_off[s] < 0 || seg_n_last[s] < 0) { set_err(err, err_cap, "%s: segment %d: seg_ids_off (%d) and seg_n_last (%d) must be >= 0", fn, s, seg_ids_off[s], seg_n_last[s]); return LLAMAHIP_ERR_PREDICT; }
        if ((int64_t) seg_ids_off[s] + seg_n_last[s] + rows - 1 > (int64_t) n_ids) {
            set_err(err, err_cap, "%s: segment %d's id stream does not fit: seg_ids_off (%d) + seg_n_last (%d) + rows (%d) - 1 > n_ids (%d)", fn, s, seg_ids_off[s], seg_n_last[s], rows, n_ids);
            return LLAMAHIP_ERR_PREDICT;
        }
        for (int r = seg_begin[s]; r < seg_begin[s + 1]; r++) { tab[r] = seg_ids_off[s] + (r - seg_begin[s]); tab[VERIFY_ROWS_MAX + r] = seg_n_last[s]; }
    }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t R = n_rows, V = n_vocab;
    std::vector<TopkOut> h(R);
    Scratch s;
    char *d_ws = s.alloc<char>(R * TOPK_WS_BYTES);
    s.fill(d_ws, 0, R * TOPK_WS_BYTES);
    float *d_l = s.alloc(R * V, logits);
    int32_t *d_ids = s.alloc<int32_t>((size_t) n_ids + 1);
    if (n_ids > 0) s.upload(d_ids, ids, (size_t) n_ids * 4);
    int32_t *d_tab = s.alloc((size_t) 2 * VERIFY_ROWS_MAX, tab);
    TopkOut *d_out = s.alloc<TopkOut>(R);
    if (s.ok()) s.check(launch_topk_slide_set(d_l, n_rows, n_vocab, d_ids, d_tab, d_tab + VERIFY_ROWS_MAX, 1.0 / temp, repeat_penalty, top_k, d_out, nullptr, d_ws));
    s.download(h.data(), d_out, R * sizeof(TopkOut));
    if (!s.ok()) return s.fail(fn, err, err_cap);
    for (size_t r = 0; r < R; r++) {
        out_exact[r] = h[r].fl[0];
        for (int i = 0; i < top_k; i++) { out_scores[r * 64 + i] = h[r].sc[i]; out_ids[r * 64 + i] = h[r].id[i]; }
    }
    return LLAMAHIP_OK;
}

// k_row_logprob on caller-supplied rows (parity tests): see llamahip_eval_logprobs
int llamahip_op_logprob(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *targets,
                        double *logprob_out, int32_t *argmax_out, int32_t *rank_out, char *err, size_t err_cap) {
    if (!logits || n_rows < 1 || n_vocab < 1) { set_err(err, err_cap, "llamahip_op_logprob: bad arguments (n_rows %d, n_vocab %d)", n_rows, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (targets)
        for (int i = 0; i < n_rows; i++)
            if (targets[i] < -1 || targets[i] >= n_vocab) { set_err(err, err_cap, "llamahip_op_logprob: target %d of row %d out of range [-1, %d)", targets[i], i, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t N = (size_t) n_rows;
    std::vector<char> h(N * 16);
    Scratch s;
    float *d_l = s.alloc(N * (size_t) n_vocab, logits);
    char *d_s = s.alloc<char>(N * 20);      // logprob [N] doubles | argmax [N] | rank [N] | targets [N]
    int32_t *d_t = d_s ? (int32_t *) (d_s + 16 * N) : nullptr;
    if (targets) s.upload(d_t, targets, N * 4);
    else s.fill(d_t, 0xFF, N * 4);      // (0xFFFFFFFF = -1)
    if (s.ok()) s.check(launch_row_logprob(d_l, n_rows, n_vocab, d_t, (double *) d_s, (int32_t *) (d_s + 8 * N), (int32_t *) (d_s + 12 * N), nullptr));
    s.download(h.data(), d_s, N * 16);
    if (!s.ok()) return s.fail("llamahip_op_logprob", err, err_cap);
    if (logprob_out) memcpy(logprob_out, h.data(), N * 8);
    if (argmax_out) memcpy(argmax_out, h.data() + N * 8, N * 4);
    if (rank_out) memcpy(rank_out, h.data() + N * 12, N * 4);
    return LLAMAHIP_OK;
}

// k_row_topn on caller-supplied rows (parity tests): see llamahip_eval_top_logprobs
int llamahip_op_top_logprobs(const float *logits, int32_t n_rows, int32_t n_vocab, int32_t n_top, int32_t *ids_out, double *logprob_out,
                             char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_top_logprobs";
    if (!logits || !ids_out || !logprob_out) { set_err(err, err_cap, "%s: %s is NULL", fn, !logits ? "logits" : !ids_out ? "ids_out" : "logprob_out"); return LLAMAHIP_ERR_PREDICT; }
    if (n_rows < 1) { set_err(err, err_cap, "%s: n_rows must be >= 1 (got %d)", fn, n_rows); return LLAMAHIP_ERR_PREDICT; }
    if (n_vocab < 1) { set_err(err, err_cap, "%s: n_vocab must be >= 1 (got %d)", fn, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (n_top < 1 || n_top > TOPN_MAX) { set_err(err, err_cap, "%s: n_top %d outside 1 .. %d", fn, n_top, TOPN_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (n_top > n_vocab) { set_err(err, err_cap, "%s: n_top %d > n_vocab %d", fn, n_top, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t N = (size_t) n_rows * (size_t) n_top;
    Scratch s;
    float *d_l = s.alloc((size_t) n_rows * (size_t) n_vocab, logits);
    double *d_lp = s.alloc<double>(N);
    int32_t *d_id = s.alloc<int32_t>(N);
    if (s.ok()) s.check(launch_row_topn(d_l, n_rows, n_vocab, n_top, d_id, d_lp, nullptr));
    std::vector<double> hl(N);
    std::vector<int32_t> hi(N);
    s.download(hl.data(), d_lp, N * 8);
    s.download(hi.data(), d_id, N * 4);
    if (!s.ok()) return s.fail(fn, err, err_cap);
    std::copy(hl.begin(), hl.end(), logprob_out);
    std::copy(hi.begin(), hi.end(), ids_out);
    return LLAMAHIP_OK;
}

// the tail of an embedding pass on caller-supplied rows (parity tests): see llamahip_text_embedding.  LAST: the segments' last rows gathered first,
// the norm over those rows alone -- forward_rows' launches
int llamahip_op_pool_rows(const float *x, int32_t R, int32_t d, const float *norm_w, const int32_t *seg_begin, int32_t n_segs, int32_t pool, int32_t normalize,
                          float *out, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_pool_rows";
    if (pool_rows_check(x, R, d, norm_w, seg_begin, n_segs, pool, normalize, out, err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const bool last = pool == LLAMAHIP_POOL_LAST;
    const size_t D = (size_t) d, ny = last ? (size_t) n_segs : (size_t) R;
    // LAST: idx = the segments' last rows, seg = 0 .. n_segs over the gathered rows
    std::vector<int32_t> idx((size_t) n_segs), seg(seg_begin, seg_begin + n_segs + 1);
    for (int s = 0; s < n_segs; s++) idx[(size_t) s] = seg_begin[s + 1] - 1;
    if (last) for (int s = 0; s <= n_segs; s++) seg[(size_t) s] = s;
    Scratch s;
    float *d_x = s.alloc((size_t) R * D, x), *d_w = s.alloc(D, norm_w);
    float *d_g = last ? s.alloc<float>(ny * D) : nullptr, *d_y = s.alloc<float>(ny * D), *d_o = s.alloc<float>((size_t) n_segs * D);
    int32_t *d_seg = s.alloc(seg.size(), seg.data()), *d_idx = s.alloc(idx.size(), idx.data());
    if (s.ok() && last) s.check(launch_gather_rows(d_x, d_idx, n_segs, d, d_g, nullptr));
    if (s.ok()) s.check(launch_norm_rows_f32(last ? d_g : d_x, d_w, d, (int) ny, d_y, nullptr));
    if (s.ok()) s.check(launch_pool_rows(d_y, d_seg, n_segs, d, pool, normalize, d_o, nullptr));
    s.download(out, d_o, (size_t) n_segs * D * 4);
    if (!s.ok()) return s.fail(fn, err, err_cap);
    return LLAMAHIP_OK;
}

// k_verify_rows + k_accept_drafts on caller-supplied rows (parity tests): see llamahip_verify_greedy
int llamahip_op_verify_rows(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *tokens,
                            int32_t *n_accept, int32_t *picks, char *err, size_t err_cap) {
    if (!logits || !tokens || n_rows < 1 || n_rows > VERIFY_ROWS_MAX || n_vocab < 1) {
        set_err(err, err_cap, "llamahip_op_verify_rows: bad arguments (n_rows %d of 1 .. %d, n_vocab %d)", n_rows, VERIFY_ROWS_MAX, n_vocab);
        return LLAMAHIP_ERR_PREDICT;
    }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t N = (size_t) n_rows;
    int32_t h[VERIFY_ROWS_MAX + 1] = { 0 };
    Scratch s;
    int32_t *d_v = s.alloc<int32_t>(80);      // {position, cursor} | tokens | picks | result | from [64]: a log of 16 entries
    s.fill(d_v, 0, 80 * 4);
    float *d_l = s.alloc(N * (size_t) n_vocab, logits);
    if (s.ok()) s.upload(d_v + 2, tokens, N * 4);
    if (s.ok()) s.check(launch_verify_rows(d_l, n_rows, n_vocab, d_v + 18, nullptr));
    if (s.ok()) s.check(launch_accept_drafts(d_v + 2, d_v + 18, 0, n_rows, 0, d_v + 64, VERIFY_ROWS_MAX, d_v, d_v + 34, nullptr));
    if (s.ok()) s.download(h, d_v + 34, (N + 1) * 4);
    if (!s.ok()) return s.fail("llamahip_op_verify_rows", err, err_cap);
    if (n_accept) *n_accept = h[0];
    if (picks) memcpy(picks, h + 1, N * 4);
    return LLAMAHIP_OK;
}

// what the two constrained-decoding ops refuse of their operands: 0, or LLAMAHIP_ERR_PREDICT with the limit in err
static int dfa_op_check(const char *fn, const float *logits, int32_t n_rows, int32_t n_vocab, const uint16_t *table, int32_t n_table_states, const int32_t *states,
                        char *err, size_t err_cap) {
    if (!logits || !table || !states) { set_err(err, err_cap, "%s: %s is NULL", fn, !logits ? "logits" : !table ? "table" : "states"); return LLAMAHIP_ERR_PREDICT; }
    if (n_rows < 1 || n_rows > DFA_ROWS_MAX) { set_err(err, err_cap, "%s: n_rows %d outside 1 .. %d", fn, n_rows, DFA_ROWS_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (n_vocab < 1) { set_err(err, err_cap, "%s: n_vocab must be >= 1 (got %d)", fn, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (n_table_states < 1 || n_table_states > 0xFFFF) { set_err(err, err_cap, "%s: n_table_states %d outside 1 .. %d", fn, n_table_states, 0xFFFF); return LLAMAHIP_ERR_PREDICT; }
    const size_t n = (size_t) n_table_states * (size_t) n_vocab;
    for (size_t i = 0; i < n; i++)
        if (table[i] != DFA_BANNED_U16 && table[i] >= n_table_states) {
            set_err(err, err_cap, "%s: table[%zu][%zu] = %d is neither a state below %d nor BANNED (65535)", fn, i / (size_t) n_vocab, i % (size_t) n_vocab, (int) table[i], n_table_states);
            return LLAMAHIP_ERR_PREDICT;
        }
    return 0;
}

// k_pick_dfa on caller-supplied rows (parity tests): see llamahip_decode_greedy_constrained
int llamahip_op_pick_dfa(const float *logits, int32_t n_rows, int32_t n_vocab, const uint16_t *table, int32_t n_table_states, int32_t *states_io,
                         int32_t fallback_token, int32_t *picks, int32_t *dead, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_pick_dfa";
    if (dfa_op_check(fn, logits, n_rows, n_vocab, table, n_table_states, states_io, err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    if (!picks || !dead) { set_err(err, err_cap, "%s: %s is NULL", fn, !picks ? "picks" : "dead"); return LLAMAHIP_ERR_PREDICT; }
    if (fallback_token < 0 || fallback_token >= n_vocab) { set_err(err, err_cap, "%s: fallback_token %d out of range [0, %d)", fn, fallback_token, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t N = (size_t) n_rows, V = (size_t) n_vocab;
    int32_t h[3 * DFA_ROWS_MAX];      // picks | {state, dead} per row: the caller's words go up and come back, so what the kernel leaves alone shows
    for (size_t r = 0; r < N; r++) { h[r] = picks[r]; h[DFA_ROWS_MAX + 2 * r] = states_io[r]; h[DFA_ROWS_MAX + 2 * r + 1] = dead[r]; }
    Scratch s;
    float *d_l = s.alloc(N * V, logits);
    uint16_t *d_t = s.alloc((size_t) n_table_states * V, table);
    int32_t *d_w = s.alloc(3 * (size_t) DFA_ROWS_MAX, h);
    DfaRows rows = {};
    for (size_t r = 0; r < N; r++) rows.r[r] = { d_l + r * V, d_t, d_w + DFA_ROWS_MAX + 2 * r, d_w, nullptr, nullptr, n_table_states, fallback_token, (int32_t) r, 0 };
    if (s.ok()) s.check(launch_pick_dfa(rows, n_rows, n_vocab, nullptr));
    s.download(h, d_w, sizeof(h));
    if (!s.ok()) return s.fail(fn, err, err_cap);
    for (size_t r = 0; r < N; r++) { picks[r] = h[r]; states_io[r] = h[DFA_ROWS_MAX + 2 * r]; dead[r] = h[DFA_ROWS_MAX + 2 * r + 1]; }
    return LLAMAHIP_OK;
}

// k_mask_rows_dfa on caller-supplied rows (parity tests): see llamahip_eval_topk_constrained
int llamahip_op_mask_rows_dfa(const float *logits, int32_t n_rows, int32_t n_vocab, const uint16_t *table, int32_t n_table_states, const int32_t *states,
                              float *out, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_mask_rows_dfa";
    if (dfa_op_check(fn, logits, n_rows, n_vocab, table, n_table_states, states, err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    if (!out) { set_err(err, err_cap, "%s: out is NULL", fn); return LLAMAHIP_ERR_PREDICT; }
    for (int32_t r = 0; r < n_rows; r++)
        if (states[r] < 0 || states[r] >= n_table_states) { set_err(err, err_cap, "%s: states[%d] = %d out of range [0, %d)", fn, r, states[r], n_table_states); return LLAMAHIP_ERR_PREDICT; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t N = (size_t) n_rows, V = (size_t) n_vocab;
    Scratch s;
    float *d_l = s.alloc(N * V, logits), *d_o = s.alloc(N * V, out);      // (the caller's bits go up: an entry the kernel skipped would show)
    uint16_t *d_t = s.alloc((size_t) n_table_states * V, table);
    DfaMaskRows rows = {};
    for (size_t r = 0; r < N; r++) rows.row[r] = d_t + (size_t) states[r] * V;
    if (s.ok()) s.check(launch_mask_rows_dfa(d_l, d_o, n_rows, n_vocab, rows, nullptr));
    s.download(out, d_o, N * V * 4);
    if (!s.ok()) return s.fail(fn, err, err_cap);
    return LLAMAHIP_OK;
}

// the pick half of k_sched_pick on caller-supplied rows, one segment per row, no slot words (parity tests): see llamahip_sched_step
int llamahip_op_sched_pick(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *emit, int32_t *picks, char *err, size_t err_cap) {
    if (!logits || !emit || !picks || n_rows < 1 || n_rows > SET_MAX || n_vocab < 1) {
        set_err(err, err_cap, "llamahip_op_sched_pick: bad arguments (n_rows %d of 1 .. %d, n_vocab %d)", n_rows, SET_MAX, n_vocab);
        return LLAMAHIP_ERR_PREDICT;
    }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t N = (size_t) n_rows;
    int32_t tab[4 * SET_MAX] = { 0 };
    for (size_t r = 0; r < N; r++) tab[4 * r] = emit[r] != 0;
    Scratch s;
    int32_t *d_tab = s.alloc<int32_t>(4 * N, tab), *d_res = s.alloc<int32_t>(N);
    float *d_l = s.alloc(N * (size_t) n_vocab, logits);
    if (s.ok()) s.check(launch_sched_pick(d_l, n_rows, n_vocab, d_tab, nullptr, nullptr, 0, nullptr, d_res, nullptr));
    if (s.ok()) s.download(picks, d_res, N * 4);
    if (!s.ok()) return s.fail("llamahip_op_sched_pick", err, err_cap);
    return LLAMAHIP_OK;
}

// what the two per-row allow-list ops refuse behind dfa_op_check: a state outside [-1, n_table_states), a fallback token out of range
static int dfa_rows_check(const char *fn, int32_t n_rows, int32_t n_vocab, int32_t n_table_states, const int32_t *states, const int32_t *fallback, const int32_t *picks,
                          const int32_t *dead, char *err, size_t err_cap) {
    if (!fallback || !picks || !dead) { set_err(err, err_cap, "%s: %s is NULL", fn, !fallback ? "fallback" : !picks ? "picks" : "dead"); return LLAMAHIP_ERR_PREDICT; }
    for (int32_t r = 0; r < n_rows; r++) {
        if (states[r] < -1 || states[r] >= n_table_states) { set_err(err, err_cap, "%s: states[%d] = %d out of range [-1, %d) (-1 = unconstrained)", fn, r, states[r], n_table_states); return LLAMAHIP_ERR_PREDICT; }
        if (fallback[r] < 0 || fallback[r] >= n_vocab) { set_err(err, err_cap, "%s: fallback[%d] = %d out of range [0, %d)", fn, r, fallback[r], n_vocab); return LLAMAHIP_ERR_PREDICT; }
    }
    return 0;
}

// k_verify_rows_dfa on caller-supplied rows (parity tests): see the request scheduler's "constrained requests" in llamahip.h
int llamahip_op_verify_rows_allow(const float *logits, int32_t n_rows, int32_t n_vocab, const uint16_t *table, int32_t n_table_states, const int32_t *states,
                                const int32_t *fallback, int32_t *picks, int32_t *dead, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_verify_rows_allow";
    if (dfa_op_check(fn, logits, n_rows, n_vocab, table, n_table_states, states, err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    if (dfa_rows_check(fn, n_rows, n_vocab, n_table_states, states, fallback, picks, dead, err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t N = (size_t) n_rows, V = (size_t) n_vocab;
    int32_t h[2 * DFA_ROWS_MAX];      // picks | dead: the caller's words go up and come back, so what the kernel leaves alone shows
    for (size_t r = 0; r < N; r++) { h[r] = picks[r]; h[DFA_ROWS_MAX + r] = dead[r]; }
    Scratch s;
    float *d_l = s.alloc(N * V, logits);
    uint16_t *d_t = s.alloc((size_t) n_table_states * V, table);
    int32_t *d_w = s.alloc(2 * (size_t) DFA_ROWS_MAX, h);
    DfaMaskRows rows = {};
    DfaFallback fb = {};
    for (size_t r = 0; r < N; r++) { rows.row[r] = states[r] < 0 ? nullptr : d_t + (size_t) states[r] * V; fb.t[r] = fallback[r]; }
    if (s.ok()) s.check(launch_verify_rows_dfa(d_l, n_rows, n_vocab, rows, fb, d_w, d_w + DFA_ROWS_MAX, nullptr));
    s.download(h, d_w, sizeof(h));
    if (!s.ok()) return s.fail(fn, err, err_cap);
    for (size_t r = 0; r < N; r++) { picks[r] = h[r]; dead[r] = h[DFA_ROWS_MAX + r]; }
    return LLAMAHIP_OK;
}

// k_sched_pick_dfa on caller-supplied rows, one segment per row, with or without slot words (parity tests)
int llamahip_op_sched_pick_allow(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *emit, const uint16_t *table, int32_t n_table_states,
                               const int32_t *states, const int32_t *fallback, const int32_t *seg_words, int32_t n_slots, int32_t log_cap, int32_t *state,
                               int32_t *log, int32_t *next_tok, int32_t *picks, int32_t *dead, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_sched_pick_allow";
    if (dfa_op_check(fn, logits, n_rows, n_vocab, table, n_table_states, states, err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    if (!emit) { set_err(err, err_cap, "%s: emit is NULL", fn); return LLAMAHIP_ERR_PREDICT; }
    if (dfa_rows_check(fn, n_rows, n_vocab, n_table_states, states, fallback, picks, dead, err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const bool words = state || log || next_tok || seg_words;
    if (words && (!state || !log || !next_tok || !seg_words)) { set_err(err, err_cap, "%s: the slot words state, log, next_tok and seg_words come all four or not at all", fn); return LLAMAHIP_ERR_PREDICT; }
    if (words && (n_slots < 1 || n_slots > 4096 || log_cap < 1 || log_cap > 1 << 20)) { set_err(err, err_cap, "%s: n_slots (%d) outside 1 .. 4096 or log_cap (%d) outside 1 .. 2^20", fn, n_slots, log_cap); return LLAMAHIP_ERR_PREDICT; }
    int32_t tab[4 * SET_MAX] = { 0 };
    for (int r = 0; r < n_rows; r++) {
        tab[4 * r] = emit[r] != 0;
        if (!words) continue;
        const int32_t *w = seg_words + 3 * r;
        if (w[0] < 0 || w[0] >= n_slots) { set_err(err, err_cap, "%s: segment %d: slot %d out of range [0, n_slots = %d)", fn, r, w[0], n_slots); return LLAMAHIP_ERR_PREDICT; }
        for (int q = 0; q < r; q++) if (seg_words[3 * q] == w[0]) { set_err(err, err_cap, "%s: slot %d has two segments (%d and %d): one segment per slot", fn, w[0], q, r); return LLAMAHIP_ERR_PREDICT; }
        if (w[1] < 0 || w[2] < 0) { set_err(err, err_cap, "%s: segment %d: position %d / cursor %d out of range", fn, r, w[1], w[2]); return LLAMAHIP_ERR_PREDICT; }
        tab[4 * r + 1] = w[0]; tab[4 * r + 2] = w[1]; tab[4 * r + 3] = w[2];
    }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t N = (size_t) n_rows, V = (size_t) n_vocab, NS = words ? (size_t) n_slots : 0;
    int32_t h[2 * SET_MAX];
    Scratch s;
    float *d_l = s.alloc(N * V, logits);
    uint16_t *d_t = s.alloc((size_t) n_table_states * V, table);
    int32_t *d_tab = s.alloc<int32_t>(4 * N, tab), *d_res = s.alloc<int32_t>(2 * N);
    // (the slot words go up and come back whole: what the launch does not write keeps the caller's bits)
    int32_t *d_state = words ? s.alloc<int32_t>(2 * NS, state) : nullptr, *d_log = words ? s.alloc<int32_t>(NS * (size_t) log_cap, log) : nullptr;
    int32_t *d_next = words ? s.alloc<int32_t>(NS, next_tok) : nullptr;
    DfaMaskRows rows = {};
    DfaFallback fb = {};
    for (size_t r = 0; r < N; r++) { rows.row[r] = states[r] < 0 ? nullptr : d_t + (size_t) states[r] * V; fb.t[r] = fallback[r]; }
    if (s.ok()) s.check(launch_sched_pick_dfa(d_l, n_rows, n_vocab, d_tab, rows, fb, d_state, d_log, log_cap, d_next, d_res, nullptr));
    if (s.ok()) s.download(h, d_res, 2 * N * 4);
    if (s.ok() && words) { s.download(state, d_state, 2 * NS * 4); s.download(log, d_log, NS * (size_t) log_cap * 4); s.download(next_tok, d_next, NS * 4); }
    if (!s.ok()) return s.fail(fn, err, err_cap);
    memcpy(picks, h, N * 4);
    memcpy(dead, h + N, N * 4);
    return LLAMAHIP_OK;
}

// k_verify_rows + k_sched_accept on caller-supplied rows and a caller's segment table, with or without slot words (parity tests): see the
// request scheduler's "drafted tokens" in llamahip.h
int llamahip_op_sched_accept(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *seg_tab, int32_t n_segs, const int32_t *tokens,
                             int32_t n_slots, int32_t log_cap, int32_t *state, int32_t *log, int32_t *next_tok,
                             int32_t *n_accept, int32_t *picks, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_sched_accept";
    if (!logits || !seg_tab || !tokens || !n_accept || !picks || n_vocab < 1) { set_err(err, err_cap, "%s: bad arguments (null pointer or n_vocab %d)", fn, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (n_rows < 1 || n_rows > VERIFY_ROWS_MAX) { set_err(err, err_cap, "%s: n_rows must be 1 .. %d (got %d): a step has at most %d logits rows", fn, VERIFY_ROWS_MAX, n_rows, VERIFY_ROWS_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (n_segs < 1 || n_segs > SET_MAX) { set_err(err, err_cap, "%s: n_segs must be 1 .. %d (got %d)", fn, SET_MAX, n_segs); return LLAMAHIP_ERR_PREDICT; }
    const bool words = state || log || next_tok;
    if (words && (!state || !log || !next_tok)) { set_err(err, err_cap, "%s: the slot words state, log and next_tok come all three or not at all", fn); return LLAMAHIP_ERR_PREDICT; }
    if (words && (n_slots < 1 || n_slots > 4096 || log_cap < 1 || log_cap > 1 << 20)) { set_err(err, err_cap, "%s: n_slots (%d) outside 1 .. 4096 or log_cap (%d) outside 1 .. 2^20", fn, n_slots, log_cap); return LLAMAHIP_ERR_PREDICT; }
    int next_row = 0;
    for (int s = 0; s < n_segs; s++) {
        const int32_t *t = seg_tab + SCHED_TAB_W * s;
        const int emit = t[0], slot = t[1], rows = t[5], N = emit == 2 ? rows : emit == 1 ? 1 : 0;
        if (emit < 0 || emit > 2) { set_err(err, err_cap, "%s: segment %d: emit %d outside 0 .. 2", fn, s, emit); return LLAMAHIP_ERR_PREDICT; }
        if (rows < 1 || (emit == 2 && rows > VERIFY_ROWS_MAX)) { set_err(err, err_cap, "%s: segment %d: row count %d (>= 1; at most %d where every row has a logits row)", fn, s, rows, VERIFY_ROWS_MAX); return LLAMAHIP_ERR_PREDICT; }
        if (t[2] < 0 || t[3] < 0 || t[2] > INT32_MAX - rows || t[3] > INT32_MAX - VERIFY_ROWS_MAX) { set_err(err, err_cap, "%s: segment %d: base position %d / base cursor %d out of range", fn, s, t[2], t[3]); return LLAMAHIP_ERR_PREDICT; }
        if (N > 0 && (t[4] != next_row || next_row + N > n_rows)) {
            set_err(err, err_cap, "%s: segment %d: logits rows [%d, %d + %d) -- the emitting segments' rows must tile [0, n_rows = %d) in segment order", fn, s, t[4], t[4], N, n_rows);
            return LLAMAHIP_ERR_PREDICT;
        }
        next_row += N;
        if (!words) continue;
        if (slot < 0 || slot >= n_slots) { set_err(err, err_cap, "%s: segment %d: slot %d out of range [0, n_slots = %d)", fn, s, slot, n_slots); return LLAMAHIP_ERR_PREDICT; }
        for (int q = 0; q < s; q++) if (seg_tab[SCHED_TAB_W * q + 1] == slot) { set_err(err, err_cap, "%s: slot %d has two segments (%d and %d): one segment per slot", fn, slot, q, s); return LLAMAHIP_ERR_PREDICT; }
    }
    if (next_row != n_rows) { set_err(err, err_cap, "%s: the segments name %d logits rows, n_rows is %d", fn, next_row, n_rows); return LLAMAHIP_ERR_PREDICT; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t N = (size_t) n_rows, S = (size_t) n_segs, NS = words ? (size_t) n_slots : 0;
    int32_t h[SET_MAX + VERIFY_ROWS_MAX] = { 0 };
    Scratch s;
    float *d_l = s.alloc(N * (size_t) n_vocab, logits);
    int32_t *d_tab = s.alloc<int32_t>(SCHED_TAB_W * S, seg_tab), *d_tok = s.alloc<int32_t>(N, tokens), *d_pick = s.alloc<int32_t>(N), *d_res = s.alloc<int32_t>(N + S);
    // (the slot words go up and come back whole: what the launch does not write keeps the caller's bits)
    int32_t *d_state = words ? s.alloc<int32_t>(2 * NS, state) : nullptr, *d_log = words ? s.alloc<int32_t>(NS * (size_t) log_cap, log) : nullptr;
    int32_t *d_next = words ? s.alloc<int32_t>(NS, next_tok) : nullptr;
    if (s.ok()) s.check(launch_verify_rows(d_l, n_rows, n_vocab, d_pick, nullptr));
    if (s.ok()) s.check(launch_sched_accept(d_pick, d_tok, d_tab, n_segs, n_rows, d_state, d_log, log_cap, d_next, d_res, nullptr));
    if (s.ok()) s.download(h, d_res, (N + S) * 4);
    if (s.ok() && words) { s.download(state, d_state, 2 * NS * 4); s.download(log, d_log, NS * (size_t) log_cap * 4); s.download(next_tok, d_next, NS * 4); }
    if (!s.ok()) return s.fail(fn, err, err_cap);
    memcpy(n_accept, h, S * 4);
    memcpy(picks, h + S, N * 4);
    return LLAMAHIP_OK;
}

// k_verify_rows + k_accept_drafts_set on caller-supplied rows cut into segments (parity tests): see llamahip_verify_greedy_multi
int llamahip_op_verify_rows_set(const float *logits, int32_t n_rows, int32_t n_vocab, const int32_t *tokens, const int32_t *seg_begin, int32_t n_segs,
                                int32_t *n_accept, int32_t *picks, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_verify_rows_set";
    if (!logits || !tokens || !seg_begin || n_vocab < 1) { set_err(err, err_cap, "%s: bad arguments (null pointer or n_vocab %d)", fn, n_vocab); return LLAMAHIP_ERR_PREDICT; }
    if (n_rows < 1 || n_rows > VERIFY_ROWS_MAX) { set_err(err, err_cap, "%s: n_rows must be 1 .. %d (got %d): a verify step has at most %d rows", fn, VERIFY_ROWS_MAX, n_rows, VERIFY_ROWS_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (n_segs < 1 || n_segs > n_rows) { set_err(err, err_cap, "%s: n_segs must be 1 .. n_rows (%d; got %d)", fn, n_rows, n_segs); return LLAMAHIP_ERR_PREDICT; }
    if (seg_begin[0] != 0 || seg_begin[n_segs] != n_rows) { set_err(err, err_cap, "%s: seg_begin must run from 0 to n_rows (%d; got %d .. %d)", fn, n_rows, seg_begin[0], seg_begin[n_segs]); return LLAMAHIP_ERR_PREDICT; }
    for (int s = 0; s < n_segs; s++)
        if (seg_begin[s + 1] <= seg_begin[s]) { set_err(err, err_cap, "%s: seg_begin must ascend strictly (segment %d: %d .. %d)", fn, s, seg_begin[s], seg_begin[s + 1]); return LLAMAHIP_ERR_PREDICT; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t N = (size_t) n_rows, S = (size_t) n_segs;
    int32_t h[2 * VERIFY_ROWS_MAX] = { 0 };
    Scratch s;
    int32_t *d_v = s.alloc<int32_t>(96);      // tokens | picks | seg_begin (17) at [32] | result at [64]
    s.fill(d_v, 0, 96 * 4);
    float *d_l = s.alloc(N * (size_t) n_vocab, logits);
    if (s.ok()) s.upload(d_v, tokens, N * 4);
    if (s.ok()) s.upload(d_v + 32, seg_begin, (S + 1) * 4);
    if (s.ok()) s.check(launch_verify_rows(d_l, n_rows, n_vocab, d_v + 16, nullptr));
    if (s.ok()) s.check(launch_accept_drafts_set(d_v, d_v + 16, d_v + 32, nullptr, n_segs, n_rows, nullptr, nullptr, 0, nullptr, d_v + 64, nullptr));
    if (s.ok()) s.download(h, d_v + 64, (N + S) * 4);
    if (!s.ok()) return s.fail(fn, err, err_cap);
    if (n_accept) memcpy(n_accept, h, S * 4);
    if (picks) memcpy(picks, h + S, N * 4);
    return LLAMAHIP_OK;
}

// one launch_prep on caller-supplied rows, the kernel family chosen by the caller (per-op tests of the activation producers): see llamahip.h
int llamahip_op_prep(int32_t mode, int32_t kernel, const float *buf, int64_t buf_floats, int64_t in0_offset, int64_t in_stride,
                     int64_t in1_offset, int64_t in1_stride, int32_t K, int32_t N, uint32_t *qa_A, float *qa_d, int32_t qa_rows,
                     float *y, int32_t *kernel_taken, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_prep";
    if (mode != LLAMAHIP_PREP_PLAIN && mode != LLAMAHIP_PREP_NORM && mode != LLAMAHIP_PREP_SILU_MUL) { set_err(err, err_cap, "%s: unknown mode %d", fn, mode); return LLAMAHIP_ERR_PREDICT; }
    if (kernel < LLAMAHIP_PREP_KERNEL_AUTO || kernel > LLAMAHIP_PREP_KERNEL_LDS) { set_err(err, err_cap, "%s: unknown kernel %d", fn, kernel); return LLAMAHIP_ERR_PREDICT; }
    if (!buf || !qa_A || !qa_d || N < 1 || qa_rows < N) { set_err(err, err_cap, "%s: bad arguments (N %d >= 1, qa_rows %d >= N)", fn, N, qa_rows); return LLAMAHIP_ERR_PREDICT; }
    if (K < 32 || K % 32 != 0 || K > 32768) { set_err(err, err_cap, "%s: K %d must be a multiple of 32 in 32 .. 32768", fn, K); return LLAMAHIP_ERR_PREDICT; }
    const bool rows1 = mode == LLAMAHIP_PREP_SILU_MUL, has1 = mode != LLAMAHIP_PREP_PLAIN;
    if (in_stride < K || (rows1 && in1_stride < K)) {
        set_err(err, err_cap, "%s: row stride %lld / %lld < K %d", fn, (long long) in_stride, (long long) in1_stride, K); return LLAMAHIP_ERR_PREDICT;
    }
    if (in_stride % 4 != 0 || in0_offset % 4 != 0 || (has1 && in1_offset % 4 != 0) || (rows1 && in1_stride % 4 != 0)) {
        set_err(err, err_cap, "%s: strides and offsets must be multiples of 4 floats (the kernels load 16 bytes at a time)", fn); return LLAMAHIP_ERR_PREDICT;
    }
    const int64_t end0 = in0_offset + (int64_t) (N - 1) * in_stride + K, end1 = !has1 ? 0 : in1_offset + (rows1 ? (int64_t) (N - 1) * in1_stride : 0) + K;
    if (in0_offset < 0 || (has1 && in1_offset < 0) || end0 > buf_floats || end1 > buf_floats) {
        set_err(err, err_cap, "%s: the operands end at float %lld / %lld of a buffer of %lld", fn, (long long) end0, (long long) end1, (long long) buf_floats); return LLAMAHIP_ERR_PREDICT;
    }
    if (kernel == LLAMAHIP_PREP_KERNEL_FAST && y) { set_err(err, err_cap, "%s: kernel FAST (k_prep_fast) has no fp32 output: y is the LDS kernel's", fn); return LLAMAHIP_ERR_PREDICT; }
    if (kernel == LLAMAHIP_PREP_KERNEL_FAST && !prep_fast_applies(mode, K, false)) {
        set_err(err, err_cap, "%s: kernel FAST refused for NORM with K %d: a row is one workgroup of K / 16 <= 1024 threads", fn, K); return LLAMAHIP_ERR_PREDICT;
    }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    const size_t Kp = ((size_t) K + 255) / 256 * 256, A_b = (size_t) qa_rows * Kp, d_b = (size_t) qa_rows * (Kp / 32) * 4;
    int launched = -1;      // the family launch_prep's own branch reports
    std::vector<uint16_t> ts, te;
    if (rows1) { ts.resize(1 << 16); te.resize(1 << 16); lut_tables(ts, te); }
    Scratch s;
    hipStream_t st = s.stream();
    float *d_buf = s.alloc((size_t) buf_floats, buf), *d_qd = s.alloc(d_b / 4, qa_d);      // (the QA buffers keep the caller's bits wherever the launch does not write)
    uint32_t *d_qA = s.alloc(A_b / 4, qa_A);
    float *d_y = y ? s.alloc((size_t) N * K, y) : nullptr;
    uint16_t *d_ts = rows1 ? s.alloc(ts.size(), ts.data()) : nullptr;
    if (s.ok()) s.check(launch_prep(mode, d_buf + in0_offset, has1 ? d_buf + in1_offset : nullptr, (long) in_stride, (long) in1_stride, K, N, d_qA, d_qd, d_y, nullptr,
                                    d_ts, st, kernel, &launched));
    s.download(qa_A, d_qA, A_b);
    s.download(qa_d, d_qd, d_b);
    if (y) s.download(y, d_y, (size_t) N * K * 4);
    s.sync();
    if (!s.ok()) return s.fail(fn, err, err_cap);
    if (kernel_taken) *kernel_taken = launched;
    return LLAMAHIP_OK;
}

// host-only: the QA operand llamahip_op_prep returns -> Q4_0 blocks in file layout (host_util.h qa_to_q4_0_blocks)
int llamahip_debug_qa_to_blocks(const uint32_t *qa_A, const float *qa_d, int32_t N, int32_t K, void *blocks) {
    if (!qa_A || !qa_d || !blocks || N < 1 || K < 32 || K % 32 != 0) return LLAMAHIP_ERR_PREDICT;
    qa_to_q4_0_blocks(qa_A, qa_d, N, K, (uint8_t *) blocks);
    return LLAMAHIP_OK;
}

// the embedding gather on a caller-supplied Q4_0 matrix: k_embed, or with stats k_embed_part (one token): see llamahip.h
int llamahip_op_embed(const int32_t *tokens, int32_t N, const void *emb_q4_0, int32_t V, int32_t d, float *x, int32_t x_stride,
                      double *stats, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_embed";
    if (!tokens || !emb_q4_0 || !x || N < 1 || V < 1 || d < 32 || d % 32 != 0) { set_err(err, err_cap, "%s: bad arguments (N %d, V %d >= 1; d %d a multiple of 32)", fn, N, V, d); return LLAMAHIP_ERR_PREDICT; }
    if (x_stride < d) { set_err(err, err_cap, "%s: x_stride %d < d %d", fn, x_stride, d); return LLAMAHIP_ERR_PREDICT; }
    if (stats && N != 1) { set_err(err, err_cap, "%s: stats are k_embed_part's, which takes one token (N %d)", fn, N); return LLAMAHIP_ERR_PREDICT; }
    for (int n = 0; n < N; n++)
        if (tokens[n] < 0 || tokens[n] >= V) { set_err(err, err_cap, "%s: token %d of row %d outside [0, %d)", fn, tokens[n], n, V); return LLAMAHIP_ERR_PREDICT; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t xfloats = (size_t) N * x_stride;
    Scratch s;
    hipStream_t st = s.stream();
    int32_t *d_tok = s.alloc((size_t) N, tokens);
    uint8_t *d_emb = s.alloc((size_t) V * (d / 32) * 20, (const uint8_t *) emb_q4_0);
    float *d_x = s.alloc(xfloats, x);      // (the floats between d and x_stride keep the caller's bits)
    float *d_rows = s.alloc<float>((size_t) N * d + 64);      // the kernels' dense [N][d] output, then 64 floats that must stay NaN
    s.fill(d_rows, 0xFF, ((size_t) N * d + 64) * 4);
    double *d_part = stats ? s.alloc<double>(2) : nullptr;
    if (s.ok()) s.check(stats ? launch_embed_part(d_tok, d_emb, d_rows, d, d_part, st) : launch_embed(d_tok, d_emb, d_rows, d, N, st));
    if (s.ok()) s.check(hipMemcpy2DAsync(d_x, (size_t) x_stride * 4, d_rows, (size_t) d * 4, (size_t) d * 4, N, hipMemcpyDeviceToDevice, st));
    uint32_t tail[64];
    s.download(tail, d_rows + (size_t) N * d, sizeof(tail));
    s.download(x, d_x, xfloats * 4);
    if (stats) s.download(stats, d_part, 16);
    s.sync();
    if (!s.ok()) return s.fail(fn, err, err_cap);
    for (uint32_t t : tail)
        if (t != 0xFFFFFFFFu) { set_err(err, err_cap, "%s: the kernel wrote past row N - 1 of its [N][d] output", fn); return LLAMAHIP_ERR_PREDICT; }
    return LLAMAHIP_OK;
}

static_assert(LLAMAHIP_DENSE_PREP_AUTO == DENSE_PREP_AUTO && LLAMAHIP_DENSE_PREP_FUSED == DENSE_PREP_FUSED && LLAMAHIP_DENSE_PREP_SPLIT == DENSE_PREP_SPLIT, "llamahip.h mirrors launch_dense_act's kernels");

// the producers of an f16 / f32 mat-mul's activation operand on caller-supplied rows (launch_dense_act: k_dense_prep, or launch_prep +
// k_dense_perm_act), the producer chosen by the caller: see llamahip.h
int llamahip_op_dense_prep(int32_t mode, int32_t wtype, int32_t kernel, const float *buf, int64_t buf_floats, int64_t in0_offset, int64_t in_stride,
                           int64_t in1_offset, int64_t in1_stride, int32_t K, int32_t N, float *xp, int32_t *kernel_taken, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_dense_prep";
    if (mode != LLAMAHIP_PREP_PLAIN && mode != LLAMAHIP_PREP_NORM && mode != LLAMAHIP_PREP_SILU_MUL) { set_err(err, err_cap, "%s: unknown mode %d", fn, mode); return LLAMAHIP_ERR_PREDICT; }
    if (wtype != 0 && wtype != 1) { set_err(err, err_cap, "%s: wtype %d: 0 (fp32) or 1 (fp16) weights", fn, wtype); return LLAMAHIP_ERR_PREDICT; }
    if (kernel < LLAMAHIP_DENSE_PREP_AUTO || kernel > LLAMAHIP_DENSE_PREP_SPLIT) { set_err(err, err_cap, "%s: unknown kernel %d", fn, kernel); return LLAMAHIP_ERR_PREDICT; }
    if (!buf || !xp || N < 1) { set_err(err, err_cap, "%s: bad arguments (buf, xp not NULL; N %d >= 1)", fn, N); return LLAMAHIP_ERR_PREDICT; }
    if (K < 32 || K % 32 != 0 || K > 32768) { set_err(err, err_cap, "%s: K %d must be a multiple of 32 in 32 .. 32768", fn, K); return LLAMAHIP_ERR_PREDICT; }
    const bool rows1 = mode == LLAMAHIP_PREP_SILU_MUL, has1 = mode != LLAMAHIP_PREP_PLAIN;
    if (in_stride < K || (rows1 && in1_stride < K)) {
        set_err(err, err_cap, "%s: row stride %lld / %lld < K %d", fn, (long long) in_stride, (long long) in1_stride, K); return LLAMAHIP_ERR_PREDICT;
    }
    if (in_stride % 4 != 0 || in0_offset % 4 != 0 || (has1 && in1_offset % 4 != 0) || (rows1 && in1_stride % 4 != 0)) {
        set_err(err, err_cap, "%s: strides and offsets must be multiples of 4 floats (the kernels load 16 bytes at a time)", fn); return LLAMAHIP_ERR_PREDICT;
    }
    const int64_t end0 = in0_offset + (int64_t) (N - 1) * in_stride + K, end1 = !has1 ? 0 : in1_offset + (rows1 ? (int64_t) (N - 1) * in1_stride : 0) + K;
    if (in0_offset < 0 || (has1 && in1_offset < 0) || end0 > buf_floats || end1 > buf_floats) {
        set_err(err, err_cap, "%s: the operands end at float %lld / %lld of a buffer of %lld", fn, (long long) end0, (long long) end1, (long long) buf_floats); return LLAMAHIP_ERR_PREDICT;
    }
    const int run = dense_prep_kernel(kernel, wtype, mode, K);
    if (run < 0) {
        set_err(err, err_cap, "%s: kernel FUSED (k_dense_prep) refused for NORM with K %d: a row is one workgroup of K / 16 <= 1024 threads", fn, K); return LLAMAHIP_ERR_PREDICT;
    }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    const size_t Kp = ((size_t) K + 255) / 256 * 256, xfloats = (size_t) N * K + 64;      // (64 guard floats behind row N - 1)
    const bool staged = run == DENSE_PREP_SPLIT && has1;      // launch_prep's fp32 rows and the Q4_0 operand it writes next to them
    int launched = -1;
    std::vector<uint16_t> ts, te;
    if (rows1) { ts.resize(1 << 16); te.resize(1 << 16); lut_tables(ts, te); }
    Scratch s;
    hipStream_t st = s.stream();
    float *d_buf = s.alloc((size_t) buf_floats, buf);
    float *d_xp = s.alloc(xfloats, xp);      // (whatever the launch does not write keeps the caller's bits)
    float *d_rows = staged ? s.alloc<float>((size_t) N * K) : nullptr, *d_qd = staged ? s.alloc<float>((size_t) N * (Kp / 32)) : nullptr;
    uint32_t *d_qA = staged ? s.alloc<uint32_t>((size_t) N * (Kp / 4)) : nullptr;
    uint16_t *d_ts = rows1 ? s.alloc(ts.size(), ts.data()) : nullptr;
    if (s.ok()) s.check(launch_dense_act(kernel, mode, wtype, d_buf + in0_offset, has1 ? d_buf + in1_offset : nullptr, (long) in_stride, (long) in1_stride, K, N,
                                         d_xp, d_rows, d_qA, d_qd, d_ts, st, &launched));
    s.download(xp, d_xp, xfloats * 4);
    s.sync();
    if (!s.ok()) return s.fail(fn, err, err_cap);
    if (kernel_taken) *kernel_taken = launched;
    return LLAMAHIP_OK;
}

// the embedding gather of an f16 / f32 / Q4_1 model file on a caller-supplied matrix (launch_embed_dense): see llamahip.h
int llamahip_op_embed_dense(const int32_t *tokens, int32_t N, const void *emb, int32_t wtype, int32_t V, int32_t d, float *x, int32_t x_stride,
                            char *err, size_t err_cap) {
    const char *fn = "llamahip_op_embed_dense";
    if (wtype != 0 && wtype != 1 && wtype != 3) { set_err(err, err_cap, "%s: wtype %d: 0 (fp32), 1 (fp16) or 3 (Q4_1) rows", fn, wtype); return LLAMAHIP_ERR_PREDICT; }
    if (!tokens || !emb || !x || N < 1 || V < 1 || d < 32 || d % 32 != 0) { set_err(err, err_cap, "%s: bad arguments (N %d, V %d >= 1; d %d a multiple of 32)", fn, N, V, d); return LLAMAHIP_ERR_PREDICT; }
    if (x_stride < d) { set_err(err, err_cap, "%s: x_stride %d < d %d", fn, x_stride, d); return LLAMAHIP_ERR_PREDICT; }
    for (int n = 0; n < N; n++)
        if (tokens[n] < 0 || tokens[n] >= V) { set_err(err, err_cap, "%s: token %d of row %d outside [0, %d)", fn, tokens[n], n, V); return LLAMAHIP_ERR_PREDICT; }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t xfloats = (size_t) N * x_stride;
    const size_t emb_bytes = wtype == 3 ? (size_t) V * (d / 32) * 24 : (size_t) V * d * (wtype == 1 ? 2 : 4);
    Scratch s;
    hipStream_t st = s.stream();
    int32_t *d_tok = s.alloc((size_t) N, tokens);
    uint8_t *d_emb = s.alloc(emb_bytes, (const uint8_t *) emb);
    float *d_x = s.alloc(xfloats, x);      // (the floats between d and x_stride keep the caller's bits)
    float *d_rows = s.alloc<float>((size_t) N * d + 64);      // the kernels' dense [N][d] output, then 64 floats that must stay NaN
    s.fill(d_rows, 0xFF, ((size_t) N * d + 64) * 4);
    if (s.ok()) s.check(launch_embed_dense(d_tok, d_emb, wtype, d_rows, d, N, st));
    if (s.ok()) s.check(hipMemcpy2DAsync(d_x, (size_t) x_stride * 4, d_rows, (size_t) d * 4, (size_t) d * 4, N, hipMemcpyDeviceToDevice, st));
    uint32_t tail[64];
    s.download(tail, d_rows + (size_t) N * d, sizeof(tail));
    s.download(x, d_x, xfloats * 4);
    s.sync();
    if (!s.ok()) return s.fail(fn, err, err_cap);
    for (uint32_t t : tail)
        if (t != 0xFFFFFFFFu) { set_err(err, err_cap, "%s: the kernel wrote past row N - 1 of its [N][d] output", fn); return LLAMAHIP_ERR_PREDICT; }
    return LLAMAHIP_OK;
}

// ---- the batched decode step (SeqSet) op by op: llamahip_op_set_attention, llamahip_op_set_entry, llamahip_op_set_exit (see llamahip.h) ----
// Row r's scattered words live in cell set_cell(r) of a pool (SET_CELL_W words: [1] token in, [2] pick out, [4] position, [5] step) and its
// row buffers (hid_in / hid_out / trace) in place set_place(r) of SET_MAX places: neither is the row order.  Every other word is 0xFF.
constexpr int SET_CELL_W = 8, SET_ROW_GUARD = 8;
constexpr uint32_t SET_POS_UNSET = 0x7F7F7F7Fu;
static inline int set_cell(int r) { return (5 * r + 3) % SET_MAX; }
static inline int set_place(int r) { return (7 * r + 2) % SET_MAX; }

int32_t llamahip_debug_set_keys(int32_t n_ctx, int32_t max_pos) {
    if (n_ctx < 1 || max_pos < 0 || max_pos >= n_ctx) return -1;
    return set_key_bucket(n_ctx, max_pos);
}

// what llamahip_op_set_attention refuses of its row table
static int set_rows_check(const char *fn, int B, int n_ctx, int n_slots, int set_keys, const int32_t *row_slot, const int32_t *row_pos, char *err, size_t err_cap) {
    for (int r = 0; r < B; r++) {
        if (row_slot[r] < 0 || row_slot[r] >= n_slots) { set_err(err, err_cap, "%s: row_slot[%d] = %d out of range [0, %d)", fn, r, row_slot[r], n_slots); return LLAMAHIP_ERR_PREDICT; }
        if (row_pos[r] < 0 || row_pos[r] >= n_ctx) { set_err(err, err_cap, "%s: row_pos[%d] = %d out of range [0, n_ctx = %d)", fn, r, row_pos[r], n_ctx); return LLAMAHIP_ERR_PREDICT; }
        if (set_keys > 0 && row_pos[r] >= set_keys) { set_err(err, err_cap, "%s: row_pos[%d] = %d is not below set_keys %d", fn, r, row_pos[r], set_keys); return LLAMAHIP_ERR_PREDICT; }
    }
    for (int r = 0; r < B; r++)
        for (int q = 0; q < r; q++)
            if (row_slot[q] == row_slot[r] && row_pos[q] == row_pos[r]) {
                set_err(err, err_cap, "%s: rows %d and %d are both at position %d of slot %d", fn, q, r, row_pos[r], row_slot[r]); return LLAMAHIP_ERR_PREDICT;
            }
    for (int r = 1; r < B; r++)
        for (int q = 0; q < r; q++)
            if (row_slot[q] == row_slot[r] && (row_slot[r - 1] != row_slot[r] || row_pos[r] != row_pos[r - 1] + 1)) {
                set_err(err, err_cap, "%s: the rows of slot %d are not one run of consecutive ascending positions in adjacent rows (row %d at %d, row %d of slot %d at %d)",
                        fn, row_slot[r], r, row_pos[r], r - 1, row_slot[r - 1], row_pos[r - 1]);
                return LLAMAHIP_ERR_PREDICT;
            }
    return 0;
}

int llamahip_op_set_attention(const float *qkv, int32_t B, int32_t d, int32_t H, int32_t n_ctx, int32_t n_slots, float *Kc, float *Vc,
                              const int32_t *row_slot, const int32_t *row_pos, int32_t n_threads, int32_t set_keys,
                              float *merged, int32_t merged_stride, void *wo_operand, uint32_t score_fill, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_set_attention";
    if (!qkv || !Kc || !Vc || !row_slot || !row_pos || d < 1 || H < 1 || d % H != 0 || n_ctx < 1 || n_slots < 1) {
        set_err(err, err_cap, "%s: bad arguments (qkv, Kc, Vc, row_slot, row_pos not NULL; d %d a multiple of H %d; n_ctx %d, n_slots %d >= 1)", fn, d, H, n_ctx, n_slots);
        return LLAMAHIP_ERR_PREDICT;
    }
    const int dh = d / H, nth = n_threads;
    if (dh % 32 != 0 || dh > 256) { set_err(err, err_cap, "%s: head size %d: multiples of 32 up to 256", fn, dh); return LLAMAHIP_ERR_PREDICT; }
    if (nth < 1 || nth > 32) { set_err(err, err_cap, "%s: n_threads %d outside 1 .. 32", fn, nth); return LLAMAHIP_ERR_PREDICT; }
    if (B < 2 || B > SET_MAX) { set_err(err, err_cap, "%s: B %d outside 2 .. %d rows (SeqSet)", fn, B, SET_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (set_keys < 0 || set_keys > n_ctx) { set_err(err, err_cap, "%s: set_keys %d outside 0 .. n_ctx = %d", fn, set_keys, n_ctx); return LLAMAHIP_ERR_PREDICT; }
    if (merged && merged_stride < d) { set_err(err, err_cap, "%s: merged_stride %d < d %d", fn, merged_stride, d); return LLAMAHIP_ERR_PREDICT; }
    if (set_rows_check(fn, B, n_ctx, n_slots, set_keys, row_slot, row_pos, err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    const int Kp = (d + 255) / 256 * 256;
    const size_t cache_b = (size_t) n_slots * n_ctx * d * 4, ms = merged ? (size_t) merged_stride : (size_t) d, mbytes = (size_t) B * ms * 4;
    const size_t qaA_b = (size_t) B * Kp, qad_b = (size_t) B * (Kp / 32) * 4, sc_w = (size_t) SET_MAX * H * n_ctx;
    std::vector<uint16_t> ts(1 << 16), te(1 << 16);
    lut_tables(ts, te);
    const std::vector<double> tab = rope_table(n_ctx, dh);
    std::vector<int32_t> pool((size_t) SET_MAX * SET_CELL_W, -1);
    for (int r = 0; r < B; r++) { pool[set_cell(r) * SET_CELL_W + 4] = row_pos[r]; pool[set_cell(r) * SET_CELL_W + 5] = 1000 + r; }
    SeqSet hs;
    memset(&hs, 0, sizeof(hs));
    Scratch s;
    hipStream_t st = s.stream();
    float *d_qr = s.alloc<float>((size_t) B * d), *d_m = s.alloc<float>(mbytes / 4), *d_qad = s.alloc<float>(qad_b / 4), *d_sc = s.alloc<float>(sc_w);
    float *d_hid = s.alloc<float>((size_t) B * d), *d_x = s.alloc<float>((size_t) B * d);      // the dummy rows the step's first launch gathers
    uint32_t *d_qaA = s.alloc<uint32_t>(qaA_b / 4);
    if (s.ok()) s.check(hipMemsetD32Async((hipDeviceptr_t) d_sc, (int) score_fill, sc_w, st));
    s.fill(d_qr, 0xFF, (size_t) B * d * 4); s.fill(d_qaA, 0xFF, qaA_b); s.fill(d_qad, 0xFF, qad_b);
    s.fill(d_hid, 0, (size_t) B * d * 4); s.fill(d_x, 0xFF, (size_t) B * d * 4);
    if (!merged) s.fill(d_m, 0xFF, mbytes);
    float *d_qkv = s.alloc((size_t) B * 3 * d, qkv), *d_K = s.alloc(cache_b / 4, Kc), *d_V = s.alloc(cache_b / 4, Vc);
    if (merged) s.upload(d_m, merged, mbytes);
    uint16_t *d_ts = s.alloc(ts.size(), ts.data()), *d_te = s.alloc(te.size(), te.data());
    double *d_tab = s.alloc(tab.size(), tab.data());
    int32_t *d_pool = s.alloc(pool.size(), pool.data());
    hs.n = B;
    for (int r = 0; r < B; r++) {
        hs.state[r] = d_pool + set_cell(r) * SET_CELL_W + 4;
        hs.hid_in[r] = d_hid + (size_t) r * d;
        hs.kv_off[r] = (long) row_slot[r] * n_ctx * d;
        // pos[] before the step's first launch: inside the cache (nothing is written out of place if it were used) and NOT the row's position
        hs.pos[r] = n_ctx < 2 ? 0 : (row_pos[r] + 1 + r % (n_ctx - 1)) % n_ctx;
    }
    SeqSet *d_set = s.alloc(1, &hs);
    if (s.ok()) s.check(launch_check_lut_math(d_ts, d_te, st));          // g_lut_math, as a model load leaves it
    if (s.ok()) s.check(launch_rows_set(d_set, B, d_x, d, true, st));      // fills SeqSet::pos, as the step's first launch
    if (s.ok()) s.check(launch_rope_kv_set(d_qkv, 3L * d, d, dh, d_tab, d_qr, d_K, d_V, d_set, B, st));
    if (s.ok()) s.check(launch_attn_short(d_qr, d_K, d_V, d_sc, merged ? d_m : nullptr, d_qaA, d_qad, 0, B, d, H, n_ctx, nth, d_te, st, 0, d_set, set_keys, (long) ms));
    s.download(Kc, d_K, cache_b);
    s.download(Vc, d_V, cache_b);
    if (merged) s.download(merged, d_m, mbytes);
    std::vector<uint32_t> qa(qaA_b / 4), qd(qad_b / 4);
    std::vector<int32_t> pool_after(pool.size());
    s.download(qa.data(), d_qaA, qaA_b);
    s.download(qd.data(), d_qad, qad_b);
    s.download(pool_after.data(), d_pool, pool.size() * 4);
    s.sync();
    if (!s.ok()) return s.fail(fn, err, err_cap);
    for (int r = 0; r < B; r++) {
        for (int pb = d / 32; pb < Kp / 32; pb++) {
            bool zero = qd[(size_t) r * (Kp / 32) + pb] == 0;
            for (int kk = 0; kk < 8; kk++) zero = zero && qa[(size_t) r * (Kp / 4) + ((pb >> 3) * 8 + kk) * 8 + (pb & 7)] == 0;
            if (!zero) { set_err(err, err_cap, "%s: row %d: operand block %d (padding d %d up to %d) is not all zero", fn, r, pb, d, Kp); return LLAMAHIP_ERR_PREDICT; }
        }
        for (int w = 4; w < 6; w++)
            if (pool_after[set_cell(r) * SET_CELL_W + w] != pool[set_cell(r) * SET_CELL_W + w]) {
                set_err(err, err_cap, "%s: row %d: state word %d changed (%d -> %d)", fn, r, w - 4, pool[set_cell(r) * SET_CELL_W + w], pool_after[set_cell(r) * SET_CELL_W + w]);
                return LLAMAHIP_ERR_PREDICT;
            }
    }
    if (pool_after != pool) { set_err(err, err_cap, "%s: a word of the state pool outside the rows' pairs changed", fn); return LLAMAHIP_ERR_PREDICT; }
    if (wo_operand) qa_to_q4_0_blocks(qa.data(), (const float *) qd.data(), B, d, (uint8_t *) wo_operand);
    return LLAMAHIP_OK;
}

int llamahip_op_set_entry(int32_t mode, const void *emb, int32_t V, int32_t d, const int32_t *tokens, const float *hid_in, int32_t B,
                          const int32_t *row_pos, uint32_t epoch_in, int32_t pass_epoch, float *x, int32_t x_stride,
                          int32_t *pos_out, uint32_t *epoch_out, int32_t *state_out, int32_t *pool_changed, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_set_entry";
    if (mode < LLAMAHIP_SET_ENTRY_EMBED_Q4_0 || mode > LLAMAHIP_SET_ENTRY_ROWS) { set_err(err, err_cap, "%s: unknown mode %d", fn, mode); return LLAMAHIP_ERR_PREDICT; }
    const bool embed = mode != LLAMAHIP_SET_ENTRY_ROWS, dense = mode == LLAMAHIP_SET_ENTRY_EMBED_F16 || mode == LLAMAHIP_SET_ENTRY_EMBED_F32;
    if (B < 2 || B > SET_MAX) { set_err(err, err_cap, "%s: B %d outside 2 .. %d rows (SeqSet)", fn, B, SET_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (d < 32 || d % 32 != 0) { set_err(err, err_cap, "%s: d %d must be a positive multiple of 32", fn, d); return LLAMAHIP_ERR_PREDICT; }
    if (!row_pos || !x || !pos_out || !epoch_out || !state_out || !pool_changed) { set_err(err, err_cap, "%s: null operand (row_pos, x, pos_out, epoch_out, state_out, pool_changed)", fn); return LLAMAHIP_ERR_PREDICT; }
    if (x_stride < d) { set_err(err, err_cap, "%s: x_stride %d < d %d", fn, x_stride, d); return LLAMAHIP_ERR_PREDICT; }
    if (embed && (!emb || !tokens || V < 1)) { set_err(err, err_cap, "%s: the embed modes need emb, tokens and V %d >= 1", fn, V); return LLAMAHIP_ERR_PREDICT; }
    if (!embed && !hid_in) { set_err(err, err_cap, "%s: mode ROWS needs hid_in", fn); return LLAMAHIP_ERR_PREDICT; }
    if (dense && pass_epoch) { set_err(err, err_cap, "%s: k_embed_dense_set takes no epoch word (pass_epoch with mode %d)", fn, mode); return LLAMAHIP_ERR_PREDICT; }
    for (int r = 0; r < B; r++) {
        if (embed && (tokens[r] < 0 || tokens[r] >= V)) { set_err(err, err_cap, "%s: token %d of row %d outside [0, %d)", fn, tokens[r], r, V); return LLAMAHIP_ERR_PREDICT; }
        if (row_pos[r] < 0) { set_err(err, err_cap, "%s: row_pos[%d] = %d is negative", fn, r, row_pos[r]); return LLAMAHIP_ERR_PREDICT; }
    }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t cells_w = (size_t) SET_MAX * SET_CELL_W, row_w = (size_t) d + SET_ROW_GUARD, pool_w = cells_w + (embed ? 0 : SET_MAX * row_w);
    std::vector<uint32_t> pool(pool_w, 0xFFFFFFFFu), after(pool_w);
    for (int r = 0; r < B; r++) {
        uint32_t *c = pool.data() + set_cell(r) * SET_CELL_W;
        if (embed) c[1] = (uint32_t) tokens[r];
        c[4] = (uint32_t) row_pos[r]; c[5] = (uint32_t) (7 + 3 * r);
        if (!embed) memcpy(pool.data() + cells_w + set_place(r) * row_w, hid_in + (size_t) r * d, (size_t) d * 4);
    }
    uint32_t ep[8], ep_after[8];
    for (uint32_t &w : ep) w = 0xFFFFFFFFu;
    ep[3] = epoch_in;
    const size_t emb_b = !embed ? 0 : mode == LLAMAHIP_SET_ENTRY_EMBED_Q4_0 ? (size_t) V * (d / 32) * 20 : (size_t) V * d * (mode == LLAMAHIP_SET_ENTRY_EMBED_F16 ? 2 : 4);
    const size_t xfloats = (size_t) B * x_stride;
    SeqSet hs, hs_after;
    memset(&hs, 0, sizeof(hs));
    Scratch s;
    hipStream_t st = s.stream();
    uint32_t *d_pool = s.alloc(pool_w, pool.data()), *d_ep = s.alloc(8, ep);
    uint8_t *d_emb = embed ? s.alloc(emb_b, (const uint8_t *) emb) : nullptr;
    float *d_x = s.alloc(xfloats, x);      // (the floats between d and x_stride keep the caller's bits)
    float *d_rows = s.alloc<float>((size_t) B * d + 64);      // the kernels' dense [B][d] output, then 64 floats that must stay NaN
    s.fill(d_rows, 0xFF, ((size_t) B * d + 64) * 4);
    hs.n = B;
    for (int r = 0; r < SET_MAX; r++) hs.pos[r] = (int32_t) SET_POS_UNSET;
    for (int r = 0; r < B; r++) {
        int32_t *c = (int32_t *) d_pool + set_cell(r) * SET_CELL_W;
        hs.state[r] = c + 4;
        if (embed) hs.tok_in[r] = c + 1;
        else hs.hid_in[r] = (const float *) (d_pool + cells_w + set_place(r) * row_w);
    }
    SeqSet *d_set = s.alloc(1, &hs);
    uint32_t *epw = pass_epoch ? d_ep + 3 : nullptr;
    if (s.ok() && mode == LLAMAHIP_SET_ENTRY_EMBED_Q4_0) s.check(launch_embed_set(d_set, B, d_emb, d_rows, d, st, epw));
    if (s.ok() && dense) s.check(launch_embed_dense_set(d_set, B, d_emb, mode == LLAMAHIP_SET_ENTRY_EMBED_F16 ? 1 : 0, d_rows, d, st));
    if (s.ok() && !embed) s.check(launch_rows_set(d_set, B, d_rows, d, true, st, epw));
    if (s.ok()) s.check(hipMemcpy2DAsync(d_x, (size_t) x_stride * 4, d_rows, (size_t) d * 4, (size_t) d * 4, B, hipMemcpyDeviceToDevice, st));
    uint32_t tail[64];
    s.download(tail, d_rows + (size_t) B * d, sizeof(tail));
    s.download(x, d_x, xfloats * 4);
    s.download(after.data(), d_pool, pool_w * 4);
    s.download(ep_after, d_ep, sizeof(ep_after));
    s.download(&hs_after, d_set, sizeof(SeqSet));
    s.sync();
    if (!s.ok()) return s.fail(fn, err, err_cap);
    for (uint32_t t : tail)
        if (t != 0xFFFFFFFFu) { set_err(err, err_cap, "%s: the kernel wrote past row B - 1 of its [B][d] output", fn); return LLAMAHIP_ERR_PREDICT; }
    for (int r = 0; r < SET_MAX; r++) pos_out[r] = hs_after.pos[r];
    *epoch_out = ep_after[3];
    bool changed = false;
    for (int r = 0; r < B; r++) {
        const size_t c = (size_t) set_cell(r) * SET_CELL_W;
        state_out[2 * r] = (int32_t) after[c + 4]; state_out[2 * r + 1] = (int32_t) after[c + 5];
        after[c + 4] = pool[c + 4]; after[c + 5] = pool[c + 5];
        hs_after.pos[r] = hs.pos[r];
    }
    for (int r = B; r < SET_MAX; r++) changed = changed || hs_after.pos[r] != (int32_t) SET_POS_UNSET;
    ep_after[3] = ep[3];
    changed = changed || after != pool || memcmp(ep_after, ep, sizeof(ep)) != 0 || memcmp(&hs_after, &hs, sizeof(SeqSet)) != 0;
    *pool_changed = changed ? 1 : 0;
    return LLAMAHIP_OK;
}

int llamahip_op_set_exit(int32_t mode, const float *logits, int32_t V, const float *x, int32_t d, int32_t B, int32_t n_ctx,
                         const int32_t *row_pos, const int32_t *row_step, const int32_t *tok_out_null,
                         int32_t *trace, int32_t *tok_out, float *hid_out, int32_t *state_out, char *err, size_t err_cap) {
    const char *fn = "llamahip_op_set_exit";
    if (mode < LLAMAHIP_SET_EXIT_ARGMAX || mode > LLAMAHIP_SET_EXIT_ARGMAX_ONE) { set_err(err, err_cap, "%s: unknown mode %d", fn, mode); return LLAMAHIP_ERR_PREDICT; }
    const bool one = mode == LLAMAHIP_SET_EXIT_ARGMAX_ONE, rows = mode == LLAMAHIP_SET_EXIT_ROWS_OUT;
    if (one && B != 1) { set_err(err, err_cap, "%s: mode ARGMAX_ONE takes B = 1 row (k_argmax), got %d", fn, B); return LLAMAHIP_ERR_PREDICT; }
    if (!one && (B < 2 || B > SET_MAX)) { set_err(err, err_cap, "%s: B %d outside 2 .. %d rows (SeqSet)", fn, B, SET_MAX); return LLAMAHIP_ERR_PREDICT; }
    if (!row_pos || !row_step || !tok_out_null || !trace || !tok_out || !state_out) { set_err(err, err_cap, "%s: null operand (row_pos, row_step, tok_out_null, trace, tok_out, state_out)", fn); return LLAMAHIP_ERR_PREDICT; }
    if (!rows && (!logits || V < 1)) { set_err(err, err_cap, "%s: the argmax modes need logits and V %d >= 1", fn, V); return LLAMAHIP_ERR_PREDICT; }
    if (rows && (!x || !hid_out || d < 1)) { set_err(err, err_cap, "%s: mode ROWS_OUT needs x, hid_out and d %d >= 1", fn, d); return LLAMAHIP_ERR_PREDICT; }
    if (n_ctx < 1) { set_err(err, err_cap, "%s: n_ctx %d must be >= 1", fn, n_ctx); return LLAMAHIP_ERR_PREDICT; }
    for (int r = 0; r < B; r++) {
        if (row_pos[r] < 0 || row_pos[r] >= n_ctx) { set_err(err, err_cap, "%s: row_pos[%d] = %d out of range [0, n_ctx = %d)", fn, r, row_pos[r], n_ctx); return LLAMAHIP_ERR_PREDICT; }
        if (row_step[r] < 0 || row_step[r] >= n_ctx) { set_err(err, err_cap, "%s: row_step[%d] = %d out of range [0, n_ctx = %d) (the trace row)", fn, r, row_step[r], n_ctx); return LLAMAHIP_ERR_PREDICT; }
    }
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    const size_t cells_w = (size_t) SET_MAX * SET_CELL_W, trace_w = (size_t) SET_MAX * n_ctx, row_w = rows ? (size_t) d + SET_ROW_GUARD : 0;
    const size_t pool_w = cells_w + trace_w + SET_MAX * row_w;
    std::vector<uint32_t> pool(pool_w, 0xFFFFFFFFu), after(pool_w);
    for (int r = 0; r < B; r++) {
        uint32_t *c = pool.data() + set_cell(r) * SET_CELL_W;
        c[4] = (uint32_t) row_pos[r]; c[5] = (uint32_t) row_step[r];
        memcpy(pool.data() + cells_w + (size_t) set_place(r) * n_ctx, trace + (size_t) r * n_ctx, (size_t) n_ctx * 4);
    }
    SeqSet hs;
    memset(&hs, 0, sizeof(hs));
    Scratch s;
    hipStream_t st = s.stream();
    uint32_t *d_pool = s.alloc(pool_w, pool.data());
    float *d_l = rows ? nullptr : s.alloc((size_t) B * V, logits), *d_x = rows ? s.alloc((size_t) B * d, x) : nullptr;
    hs.n = B;
    for (int r = 0; r < B; r++) {
        int32_t *c = (int32_t *) d_pool + set_cell(r) * SET_CELL_W;
        hs.state[r] = c + 4;
        hs.tok_out[r] = tok_out_null[r] ? nullptr : c + 2;
        hs.trace[r] = (int32_t *) d_pool + cells_w + (size_t) set_place(r) * n_ctx;
        if (rows) hs.hid_out[r] = (float *) (d_pool + cells_w + trace_w + set_place(r) * row_w);
        hs.pos[r] = row_pos[r];
    }
    SeqSet *d_set = s.alloc(1, &hs);
    if (s.ok() && mode == LLAMAHIP_SET_EXIT_ARGMAX) s.check(launch_argmax_set(d_l, V, d_set, B, st));
    if (s.ok() && one) s.check(launch_argmax(d_l, V, hs.trace[0], 0, hs.tok_out[0], hs.state[0], st));
    if (s.ok() && rows) s.check(launch_rows_set(d_set, B, d_x, d, false, st));
    if (s.ok() && rows) s.check(launch_advance_set(d_set, B, st));
    s.download(after.data(), d_pool, pool_w * 4);
    s.sync();
    if (!s.ok()) return s.fail(fn, err, err_cap);
    // the named words go to the caller and are put back as they were; everything else must be what it was
    for (int r = 0; r < B; r++) {
        const size_t c = (size_t) set_cell(r) * SET_CELL_W, t = cells_w + (size_t) set_place(r) * n_ctx, h = cells_w + trace_w + set_place(r) * row_w;
        state_out[2 * r] = (int32_t) after[c + 4]; state_out[2 * r + 1] = (int32_t) after[c + 5];
        after[c + 4] = pool[c + 4]; after[c + 5] = pool[c + 5];
        tok_out[r] = (int32_t) after[c + 2];
        if (!tok_out_null[r]) after[c + 2] = pool[c + 2];
        memcpy(trace + (size_t) r * n_ctx, after.data() + t, (size_t) n_ctx * 4);
        memcpy(after.data() + t, pool.data() + t, (size_t) n_ctx * 4);
        if (rows) { memcpy(hid_out + (size_t) r * d, after.data() + h, (size_t) d * 4); memcpy(after.data() + h, pool.data() + h, (size_t) d * 4); }
    }
    for (size_t i = 0; i < pool_w; i++)
        if (after[i] != pool[i]) {
            set_err(err, err_cap, "%s: word %zu of the pool (%s) changed: %#x -> %#x", fn, i, i < cells_w ? "the cells: a null tok_out's word or padding" : i < cells_w + trace_w ? "a trace row no row names" : "a guard around the hid_out rows",
                    pool[i], after[i]);
            return LLAMAHIP_ERR_PREDICT;
        }
    return LLAMAHIP_OK;
}

int llamahip_op_quantize_row_q4_0(const float *x, int32_t k, void *y, char *err, size_t err_cap) {
    if (need_device(err, err_cap)) return LLAMAHIP_ERR_PREDICT;
    if (!x || !y || k < 32 || k % 32 != 0) { set_err(err, err_cap, "bad quantize arguments"); return LLAMAHIP_ERR_PREDICT; }
    HIP_TRY(init_kernel_attrs(), LLAMAHIP_ERR_PREDICT);
    const size_t Kp = ((size_t) k + 255) / 256 * 256, raw_b = (size_t) (k / 32) * 20;
    Scratch s;
    float *d_x = s.alloc((size_t) k, x), *d_qd = s.alloc<float>(Kp / 32);
    uint32_t *d_qA = s.alloc<uint32_t>(Kp / 4);
    uint8_t *d_raw = s.alloc<uint8_t>(raw_b);
    if (s.ok()) s.check(launch_prep(PREP_PLAIN, d_x, nullptr, k, 0, k, 1, d_qA, d_qd, nullptr, d_raw, nullptr, nullptr));
    s.download(y, d_raw, raw_b);
    return s.ok() ? LLAMAHIP_OK : s.fail("llamahip_op_quantize_row_q4_0", err, err_cap);
}

}  // extern "C"
