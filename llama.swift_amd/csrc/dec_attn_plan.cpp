// dec_attn_plan.cpp -- the host half of the one-row decode attention (decode.hip launch_dec_attn / launch_qkv_attn): the one place that
// derives which kernel runs, the split of the key chains over workgroups, the rows per stage, the ring depth, the LDS size and the grid;
// the LLAMAHIP_PV_* switches; the check of a caller's forced plan.  Pure host code, no device: tools/host_sanitize runs it under ASan + UBSan.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "dec_attn_plan.h"

namespace lh {

bool pv_stream_applies(int dh, int n_ctx, int nth) { return nth >= 1 && nth <= 32 && n_ctx <= 4096 && dh % 32 == 0; }
bool pv_split_valid(int nth, int split) {
    if (split < 1 || split > nth) return false;
    const int cpw = (nth + split - 1) / split;
    return (split - 1) * cpw < nth;
}

// LLAMAHIP_PV_SPLIT / LLAMAHIP_PV_STAGE_ROWS / LLAMAHIP_PV_DMA are parsed once per process (the switches of this library are read once) into
// the same DecAttnForce a caller hands to dec_attn_plan (llamahip_op_dec_attention): one override path.  Not strict: a split the thread
// count cannot take is ignored.  (LLAMAHIP_PV_STAGE_ROWS shortens the stages so that small test contexts run many of them, and keeps
// k_dec_pv_stream; LLAMAHIP_PV_DMA=0 keeps k_dec_pv_stream.)
static DecAttnForce dec_attn_env_parse() {
    DecAttnForce f;
    const char *s = getenv("LLAMAHIP_PV_SPLIT"), *r = getenv("LLAMAHIP_PV_STAGE_ROWS"), *m = getenv("LLAMAHIP_PV_DMA");
    if (s && atoi(s) > 0) f.split = atoi(s);
    if (r) f.stage_rows = std::max(1, atoi(r));
    if (m && atoi(m) == 0) f.dma = 0;
    return f;
}
const DecAttnForce &dec_attn_env() {
    static const DecAttnForce env = dec_attn_env_parse();
    return env;
}

static DecAttnPlan refuse(const char *fmt, ...) {
    DecAttnPlan p;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.why, sizeof(p.why), fmt, ap);
    va_end(ap);
    return p;
}

DecAttnPlan dec_attn_plan(int d, int H, int n_ctx, int nth, bool long_ctx, bool have_sync, bool have_xpart, const DecAttnForce *force) {
    const DecAttnForce &f = force ? *force : dec_attn_env();
    if (d < 1 || H < 1 || nth < 1 || n_ctx < 1) return refuse("d %d, H %d, n_threads %d and n_ctx %d must be >= 1", d, H, nth, n_ctx);
    const int dh = d / H, nsl = (n_ctx + DEC_ATTN_TS - 1) / DEC_ATTN_TS;
    if (f.strict) {
        if (d % H != 0 || dh % 32 != 0 || dh > 256) return refuse("head size d / H = %d / %d: multiples of 32 up to 256", d, H);
        if (nth > 64) return refuse("n_threads %d outside 1 .. 64", nth);
        if (f.split < 0 || f.stage_rows < 0 || f.ns < 0 || f.dma < -1 || f.dma > 1)
            return refuse("force {split %d, stage_rows %d, ns %d, dma %d}: 0 (dma: -1) is the library's rule, dma is 0 or 1", f.split, f.stage_rows, f.ns, f.dma);
        if (f.split > 0 && !pv_split_valid(nth, f.split))
            return refuse("split %d is not valid for n_threads %d: every workgroup owns ceil(n_threads / split) chains and the last one at least one", f.split, nth);
    }
    DecAttnPlan p;
    // long contexts (the caller knows the position): scores, then the streaming soft_max . V
    if (long_ctx && pv_stream_applies(dh, n_ctx, nth)) {
        const int W = H * (dh / 32);
        // the LDS-DMA variant (k_dec_pv_dma): head size 128, a workgroup = (head, up to 3 chunks of the key split) over all 128 columns,
        // the heads' chunks split over as many workgroups as fill the chip once
        const bool dma_shape = dh == 128 && have_xpart && H % 8 == 0 && f.stage_rows == 0;
        if (f.strict && f.dma == 1 && !dma_shape)
            return refuse("k_dec_pv_dma takes head size 128 (got %d), H %% 8 == 0 (H %d), the partial-sum buffer and no stage_rows", dh, H);
        if (f.dma != 0 && dma_shape) {
            int sp = 1;
            if (f.split > 0 && pv_split_valid(nth, f.split)) sp = f.split;
            else while (H * sp * 2 <= 256 && pv_split_valid(nth, sp * 2)) sp *= 2;
            const int cpw = (nth + sp - 1) / sp;
            if (cpw <= PV_DMA_CPW_MAX) {
                const size_t fixed = 32 * sizeof(double) + ((size_t) ((n_ctx + 3) & ~3) + (size_t) nth * 128) * sizeof(float) + 64;
                int NS = (int) (((size_t) 156 * 1024 - fixed) / ((size_t) cpw * PV_DMA_SLOT_BYTES));
                NS = std::max(2, std::min(NS, PV_DMA_NS_MAX));
                if (f.ns > 0) {
                    if (f.strict && (f.ns < 2 || f.ns > PV_DMA_NS_MAX)) return refuse("ns %d outside 2 .. %d ring slots (a loader fills one slot while the owners read another)", f.ns, PV_DMA_NS_MAX);
                    NS = std::max(2, std::min(f.ns, PV_DMA_NS_MAX));
                }
                p.kernel = DEC_ATTN_PV_DMA; p.split = sp; p.cpw = cpw; p.NS = NS;
                p.lds = fixed + (size_t) NS * cpw * PV_DMA_SLOT_BYTES;
                p.gx = H * sp; p.threads = 512;
                if (f.strict && p.lds > DEC_ATTN_LDS_CAP) return refuse("ns %d x cpw %d: %zu bytes of LDS, the kernels' cap is %zu", NS, cpw, p.lds, DEC_ATTN_LDS_CAP);
                return p;
            }
            if (f.strict && f.dma == 1) return refuse("cpw = ceil(n_threads %d / split %d) = %d > %d chains per workgroup of k_dec_pv_dma", nth, sp, cpw, PV_DMA_CPW_MAX);
        }
        if (f.strict && f.ns > 0) return refuse("ns is the ring of k_dec_pv_dma; this shape runs k_dec_pv_stream");
        // chains of a (head, column block) over `split` workgroups until the chip is full (needs the XCD placement: the partial-sum buffer is
        // only passed when the load-time self-test confirmed it); every workgroup must own at least one chain
        int split = 1;
        if (have_xpart && W % 8 == 0) {
            if (f.split > 0) { if (pv_split_valid(nth, f.split)) split = f.split; }
            else while (W * split * 2 <= 256 && pv_split_valid(nth, split * 2)) split *= 2;       // (13B: 160 workgroups stay unsplit -- 320 would need two rounds: 322 against 298 tokens/s at 2 048 keys)
        } else if (f.strict && f.split > 1) {
            return refuse("split %d needs the partial-sum buffer and H dh / 32 = %d a multiple of 8 (the workgroups of a column block share an XCD)", f.split, W);
        }
        const int cpw = (nth + split - 1) / split;
        const int sr_max = PV_STREAM_QUADS / 8 / cpw;      // 16-byte loads per thread and stage: 64 KB stages, 128 KB of LDS, one workgroup per CU
        if (f.strict && f.stage_rows > sr_max) return refuse("stage_rows %d x cpw %d > %d rows per stage", f.stage_rows, cpw, PV_STREAM_QUADS / 8);
        p.kernel = DEC_ATTN_PV_STREAM; p.split = split; p.cpw = cpw;
        p.SR = f.stage_rows > 0 ? std::min(sr_max, f.stage_rows) : sr_max;
        p.lds = 32 * sizeof(double) + ((size_t) ((n_ctx + 3) & ~3) + (size_t) nth * 32) * sizeof(float) + (size_t) 2 * cpw * p.SR * 128;
        p.gx = W * split; p.threads = 1024;
        if (f.strict && p.lds > DEC_ATTN_LDS_CAP) return refuse("%zu bytes of LDS, the kernels' cap is %zu", p.lds, DEC_ATTN_LDS_CAP);
        return p;
    }
    if (f.strict && (f.split > 1 || f.stage_rows > 0 || f.ns > 0 || f.dma == 1))
        return refuse("split, stage_rows, ns and dma belong to the long-context kernels (n_threads <= 32, n_ctx <= 4096); this shape runs one workgroup per (head, column block)");
    p.cpw = nth;
    const size_t lds_pv = 32 * sizeof(double) + ((size_t) n_ctx + (size_t) nth * 32 + 16) * sizeof(float);
    // scores and soft_max . V in one launch with an XCD-local hand-off (k_dec_attn_x); the caller has the counters only after the self-test
    // confirmed the placement it relies on
    if (have_sync && nth <= 8 && dh % 32 == 0 && dh <= 256 && H % 8 == 0 && n_ctx <= DEC_ATTN_X_CTX_MAX) {
        p.kernel = DEC_ATTN_X;
        p.lds = std::max(lds_pv, (size_t) 2 * dh * sizeof(float));
        p.gx = H; p.gy = dh / 32 + nsl; p.threads = 256;
        return p;
    }
    p.kernel = DEC_ATTN_PV_BLK;
    p.lds = lds_pv;
    p.gx = H; p.gy = dh / 32;
    p.threads = (32 * (nth < 32 ? nth : 32) + 63) / 64 * 64;      // whole waves: the DPP reductions need every lane live
    if (f.strict && p.lds > DEC_ATTN_LDS_CAP) return refuse("%zu bytes of LDS, the kernels' cap is %zu", p.lds, DEC_ATTN_LDS_CAP);
    return p;
}

// head layouts whose workgroups line up with heads, on the plain wq|wk|wv matrix of the model
bool qkv_attn_shape_ok(int d, int H, int nth, int M, int K, int ngroups, int gmapF8, char *why, size_t why_cap) {
    char none[1];
    if (!why || !why_cap) { why = none; why_cap = sizeof(none); }
    if (d < 1 || H < 1 || H % 8 != 0 || d % H != 0) { snprintf(why, why_cap, "H %d must be a multiple of 8 that divides d %d", H, d); return false; }
    const int dh = d / H;
    if (dh % 32 != 0 || dh > 256) { snprintf(why, why_cap, "head size %d: multiples of 32 up to 256", dh); return false; }
    if (nth > 8) { snprintf(why, why_cap, "n_threads %d > 8 (256-thread workgroups: 32 lanes per chain)", nth); return false; }
    if (gmapF8 || M != 3 * d || K != d || ngroups != 3 * d / 8) { snprintf(why, why_cap, "the matrix must be the plain wq|wk|wv [3 d][d] of d %d, got [%d][%d]", d, M, K); return false; }
    return true;
}
bool qkv_attn_instance(int nw, bool ring, int depth, int pg) {
    return nw == 4 && ring && ((depth == 8 && pg == 1) || (depth == 10 && pg == 2) || (depth == 4 && pg == 2));
}
QkvAttnGeom qkv_attn_geom(int gemv_grid, size_t gemv_lds, int d, int H, int n_ctx, int nth) {
    const int dh = d / H, nsl = (n_ctx + DEC_ATTN_TS - 1) / DEC_ATTN_TS;
    const size_t lds_pv = 32 * sizeof(double) + ((size_t) n_ctx + (size_t) nth * 32 + 16) * sizeof(float);
    return { gemv_grid + H * (nsl + dh / 32), std::max(std::max(gemv_lds, lds_pv), (size_t) 2 * dh * sizeof(float)) };
}

}  // namespace lh
