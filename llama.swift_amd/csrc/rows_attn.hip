// rows_attn.hip -- RoPE + KV append and the short attention driven by a ROW TABLE (llamahip_eval_multi, llamahip_op_attention_rows): the R rows
// of one pass belong to several KV slots, cut into segments -- segment i is a multi-row eval of its own at n_past[i] on slot slots[i].  Every
// operator of the graph works row by row except these two, and all they need per row is {position, keys of the V*P split, cache offset}:
//   k_rope_kv_rows   k_rope_kv (prompt_attn.hip) / k_rope_kv_set (dense.hip) with the row's position and cache from the table
//   k_rows_scores    k_decn_scores (decode.hip) with np = pos[r], Kc += kv_off[r]
//   k_rows_pv        k_dec_pv_blk<true> (decode.hip) with T = pos[r] + 1, Tpv = keys[r], Vc += kv_off[r]
// One launch pair per layer covers every row of every segment, whatever their number.  The arithmetic is the named kernels', statement for
// statement; only where a row's three values come from differs.  The table is the same for every lane of a workgroup and is read with plain
// loads.  No hand-off between workgroups.  Conventions: decode.hip / DESIGN.md 12.17.
#include "kcommon.hip.h"

namespace lh {

__global__ void k_rope_kv_rows(const float *__restrict__ qkv, long qkv_stride, int d, int dh, const double *__restrict__ sincos_tab,
                               float *__restrict__ qr, float *__restrict__ Kc, float *__restrict__ Vc, const RowTab *__restrict__ rows) {
    const int n = blockIdx.x;
    const int pos = rows[n].pos;
    float *Kn = Kc + rows[n].kv_off, *Vn = Vc + rows[n].kv_off;
    const float *q = qkv + (size_t) n * qkv_stride, *k = q + d, *v = q + 2 * d;
    const double *tab = sincos_tab + (size_t) pos * dh;
    for (int i = threadIdx.x; i < d / 2; i += blockDim.x) {
        const int e = 2 * i;
        const int pr = (e % dh) >> 1;
        const double cs = tab[2 * pr], sn = tab[2 * pr + 1];
        {
            const double x0 = (double) q[e], x1 = (double) q[e + 1];
            qr[(size_t) n * d + e] = (float) (x0 * cs - x1 * sn);
            qr[(size_t) n * d + e + 1] = (float) (x0 * sn + x1 * cs);
        }
        {
            const double x0 = (double) k[e], x1 = (double) k[e + 1];
            Kn[(size_t) pos * d + e] = (float) (x0 * cs - x1 * sn);
            Kn[(size_t) pos * d + e + 1] = (float) (x0 * sn + x1 * cs);
        }
        Vn[(size_t) pos * d + e] = v[e];
        Vn[(size_t) pos * d + e + 1] = v[e + 1];
    }
}

constexpr int ROWS_TS = 32;      // keys per workgroup: 8 half-waves x 4 keys (decode.hip DEC_TS)

// blockIdx.z = entry z0 + z of the launch's row list (idx, null: the rows themselves); sc: [z][head][n_ctx], the batch's scratch
__global__ void __launch_bounds__(256)
k_rows_scores(const float *__restrict__ qr, int d, int dh, const float *__restrict__ Kc, float *__restrict__ sc,
              int n_ctx, float kq_scale, const RowTab *__restrict__ rows, const int32_t *__restrict__ idx, int z0) {
    const int h = blockIdx.x, z = blockIdx.z, H = gridDim.x;
    const int n = idx ? idx[z0 + z] : z0 + z;
    const int np = rows[n].pos;
    Kc += rows[n].kv_off;
    const int t0 = blockIdx.y * ROWS_TS;
    if (t0 > np) return;
    const int tid = threadIdx.x, hw = tid >> 5, l = tid & 31;
    constexpr int KPH = ROWS_TS / 8;
    const int tb = t0 + hw * KPH;
    const float *q = qr + (size_t) n * d + h * dh;
    float qv[8], kv[KPH][8];
#pragma unroll
    for (int i = 0; i < 8; i++) qv[i] = (i * 32 < dh) ? q[min(i * 32, dh - 32) + l] : 0.0f;
#pragma unroll
    for (int u = 0; u < KPH; u++) {
        const float *kr = Kc + (size_t) min(tb + u, np) * d + h * dh;
#pragma unroll
        for (int i = 0; i < 8; i++) kv[u][i] = (i * 32 < dh) ? kr[min(i * 32, dh - 32) + l] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < KPH; u++) {
        const int t = tb + u;
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (i * 32 < dh) s = fmaf(kv[u][i], qv[i], s);
        s = tree32_to_lane0(s);
        if (l == 0 && t <= np) sc[((size_t) z * H + h) * n_ctx + t] = s * kq_scale;
    }
}

// grid (H, dh/32, rows of the batch); block and dynamic LDS as k_dec_pv_blk: [32 doubles][n_ctx p][nth*32 partials].  merged (may be null) /
// QA rows are indexed by the ROW (strides m_stride floats, qa_strideA dwords, qa_strideD floats), the score scratch by the batch entry.
__global__ void __launch_bounds__(1024)
k_rows_pv(const float *__restrict__ sc, const float *__restrict__ Vc, int d, int dh, int n_ctx, int nth,
          float *__restrict__ merged, uint32_t *__restrict__ qa_A, float *__restrict__ qa_d, const uint16_t *__restrict__ T_exp,
          long qa_strideA, long qa_strideD, int lut_math, const RowTab *__restrict__ rows, const int32_t *__restrict__ idx, int z0, long m_stride) {
    extern __shared__ double smem_d[];
    double *red = smem_d;
    float *p = (float *) (smem_d + 32);
    float *part = p + n_ctx;
    const int h = blockIdx.x, cb = blockIdx.y, z = blockIdx.z, tid = threadIdx.x, nt = blockDim.x;
    const int n = idx ? idx[z0 + z] : z0 + z;
    const int n_past = rows[n].pos;
    Vc += rows[n].kv_off;
    const int T = n_past + 1;
    const float *row = sc + ((size_t) z * gridDim.x + h) * n_ctx;
    if (merged) merged += (size_t) n * m_stride;
    qa_A += (size_t) n * qa_strideA;
    qa_d += (size_t) n * qa_strideD;
    if (h == (int) gridDim.x - 1 && cb == (int) gridDim.y - 1)
        for (int pb = d / 32 + tid; pb < (int) qa_strideD; pb += nt) {
            const int pc = pb >> 3, pj = pb & 7;
#pragma unroll
            for (int kk = 0; kk < 8; kk++) qa_A[(pc * 8 + kk) * 8 + pj] = 0;
            qa_d[pb] = 0.0f;
        }
    pv_soft_max(row, p, T, tid, nt, red, T_exp, lut_math);
    // the row splits the keys of the eval it stands for (split_keys: its segment's n_past + rows, or up to the end of its chunk); the masked
    // tail [pos + 1, keys) -- rows of its own segment, appended by k_rope_kv_rows -- has weight 0 and is walked like the reference does
    const int Tpv = rows[n].keys;
    for (int t = T + tid; t < Tpv; t += nt) p[t] = 0.0f;
    __syncthreads();

    const int c = tid & 31, sub = tid >> 5, nsub = nt >> 5;
    const int dc = (Tpv + nth - 1) / nth;
    const int col = h * dh + cb * 32 + c;
    const float *vcol = Vc + col;
    for (int th = sub; th < nth; th += nsub) {
        const int t0 = dc * th, t1 = min(t0 + dc, Tpv);
        // (two register batches of 16 rows, the next in flight while the current one is consumed; rows past the chunk end are clamped
        //  re-reads weighted by 0: k_dec_pv_blk)
        float acc = 0.0f;
        float va[16], vb[16];
#pragma unroll
        for (int u = 0; u < 16; u++) va[u] = vcol[(size_t) min(t0 + u, t1 - 1) * d];
        for (int tb = t0; tb < t1; tb += 32) {
#pragma unroll
            for (int u = 0; u < 16; u++) vb[u] = vcol[(size_t) min(tb + 16 + u, t1 - 1) * d];
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const float pe = (tb + u < t1) ? p[min(tb + u, Tpv - 1)] : 0.0f;
                acc = fmaf(va[u], pe, acc);
            }
#pragma unroll
            for (int u = 0; u < 16; u++) va[u] = vcol[(size_t) min(tb + 32 + u, t1 - 1) * d];
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const float pe = (tb + 16 + u < t1) ? p[min(tb + 16 + u, Tpv - 1)] : 0.0f;
                acc = fmaf(vb[u], pe, acc);
            }
        }
        part[th * 32 + c] = acc;
    }
    __syncthreads();
    pv_store_block(part, nth, tid, col, h, dh, cb, merged, qa_A, qa_d);
}

hipError_t launch_rope_kv_rows(const float *qkv, long qkv_stride, int d, int dh, const double *tab, float *qr, float *Kc, float *Vc,
                               const RowTab *rows, int R, hipStream_t st) {
    hipLaunchKernelGGL(k_rope_kv_rows, dim3(R), dim3(256), 0, st, qkv, qkv_stride, d, dh, tab, qr, Kc, Vc, rows);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

// The table attention over n_rows entries of the row list (idx null: rows 0 .. n_rows - 1): scores -> soft_max + V*P + ordered combine + the
// Q4_0 quantization of the merged rows into the QA operand of wo (+ the fp32 rows, where `merged` is given).  sc: scratch of sc_rows * H * n_ctx
// floats; more rows than that are walked in batches.  max_keys: the host's bound on every listed row's position + 1 (bounds the score grid).
hipError_t launch_attn_rows(const float *qr, const float *Kc, const float *Vc, float *sc, int sc_rows, float *merged, long merged_stride,
                            uint32_t *qa_A, float *qa_d, const RowTab *rows, const int32_t *idx, int n_rows, int max_keys,
                            int d, int H, int n_ctx, int nth, const uint16_t *T_exp, hipStream_t st) {
    if (n_rows < 1 || sc_rows < 1 || max_keys < 1 || max_keys > n_ctx) return hipErrorInvalidValue;
    const int dh = d / H;
    const float kq_scale = 1.0f / sqrtf((float) d / (float) H);          // .mm:620
    const int Kp = (d + 255) / 256 * 256;
    const int nt = (32 * (nth < 32 ? nth : 32) + 63) / 64 * 64;
    const size_t lds = 32 * sizeof(double) + ((size_t) n_ctx + (size_t) nth * 32 + 16) * sizeof(float);
    for (int z0 = 0; z0 < n_rows; z0 += sc_rows) {
        const int nb = min(sc_rows, n_rows - z0);
        hipLaunchKernelGGL(k_rows_scores, dim3(H, (max_keys + ROWS_TS - 1) / ROWS_TS, nb), dim3(256), 0, st, qr, d, dh, Kc, sc, n_ctx, kq_scale, rows, idx, z0);
        LH_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rows_pv, dim3(H, dh / 32, nb), dim3(nt), lds, st, sc, Vc, d, dh, n_ctx, nth, merged, qa_A, qa_d, T_exp,
                           (long) Kp / 4, (long) Kp / 32, g_lut_math, rows, idx, z0, merged_stride > 0 ? merged_stride : (long) d);
        LH_LAUNCH_CHECK();
    }
    return hipSuccess;
}

// the last rows of the segments, side by side for the final norm and the lm head: out row i = x row idx[i]
__global__ void k_gather_rows(const float *__restrict__ x, const int32_t *__restrict__ idx, int d, float *__restrict__ out) {
    const int i = blockIdx.x;
    const float *src = x + (size_t) idx[i] * d;
    for (int e = blockIdx.y * blockDim.x + threadIdx.x; e < d; e += gridDim.y * blockDim.x) out[(size_t) i * d + e] = src[e];
}
hipError_t launch_gather_rows(const float *x, const int32_t *idx, int n, int d, float *out, hipStream_t st) {
    hipLaunchKernelGGL(k_gather_rows, dim3(n, (d + 1023) / 1024), dim3(256), 0, st, x, idx, d, out);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t init_attrs_rows_attn() {
    return hipFuncSetAttribute((const void *) k_rows_pv, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

}  // namespace lh
