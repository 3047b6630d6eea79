// flash_attn.hip -- k_flash_attn / k_flash_combine: the OPT-IN fused causal attention of long evals on the fp16 matrix cores
// (LLAMAHIP_FLAG_FAST_ATTN, llamahip_op_flash_attention).  NOT the reference's arithmetic: the exact path is the
// k_attnq_* chain (prompt_attn.hip).  One launch per layer instead of four, no score matrix in HBM.
//
//   merged[n][h * 128 + c] = sum_t softmax_t(kq_scale * q[n] . k[t]) * v[t][c]      t = 0 .. n_past + n, head size 128, q rotated, K / V the
//                                                                                  fp32 caches k_rope_kv has just appended to
//
// Stated arithmetic (the contract).
//   * q, k and v are each narrowed ONCE from fp32 to fp16, round to nearest even, SATURATING at +-65 504: no infinity is made from a finite input.
//   * Every product is exact in fp32; a score is one fp32 matrix-core sum over the 128 terms, multiplied in fp32 by c = kq_scale * log2(e)
//     (kq_scale as launch_attn computes it).  The weight is exp2(s - m) in fp32 (v_exp_f32) under the running maximum m.
//   * The weight is narrowed to fp16 for the P V instruction and the row sum l accumulates THE NARROWED weights in fp32: every output is a
//     convex combination of the narrowed v.
//   * O and l are rescaled by exp2(m_old - m_new) when the maximum moves; O is divided by l once at the end and stored as fp32.
//   * A masked key (past the query's position; that covers every key at or past T = n_past + N) has weight exactly 0: its score is replaced
//     by -inf before the maximum, and exp2(-inf - m) = +0 (a row with no visible key yet subtracts 0 instead of m = -inf).  Its operands are
//     never non-finite because of the cache: K / V rows at or past T are never loaded -- the row index is clamped to T - 1 -- so 0 * NaN
//     cannot arise from what lies behind the eval's last row.
//
// Work split.  A workgroup of four waves owns one (head, query tile, key split) and walks its share of the key tiles of 64 keys that the
// query tile sees (tiles wholly above the causal diagonal are never walked; the diagonal is masked per element).  A wave owns 16 TI
// queries: TI = 2 is the 128-query tile, TI = 1 the 64-query tile.  Query tiles are launched longest first (blockIdx.x 0 = the last tile).
//
// Which way round.  The kernel computes S^T = K Q^T and O^T = V^T P^T with v_mfma_f32_16x16x32_f16.  The A operand of a lane
// (r = lane & 15, g = lane >> 4) is row r, k-slots 8 g .. 8 g + 7; the B operand column r, the same slots; D register rr is row 4 g + rr,
// column r.  With keys as the ROWS of S^T a lane ends up with scores of ONE query (r) and keys 4 g .. 4 g + 3 of each 16-key block:
//   * the maximum and the sum of a query live in the four lanes r, r + 16, r + 32, r + 48 -- one ds_swizzle (xor 16) and one
//     ds_bpermute (xor 32), never LDS memory -- and in the SAME lanes that hold the query's O^T column, so rescaling needs no exchange;
//   * two 16-key blocks' registers, narrowed, ARE the B operand of O^T = V^T P^T for one 32-key step: P never leaves registers.  k-slot
//     8 g + 4 b + rr of the step stands for key 16 b + 4 g + rr; V is written to LDS under that same permutation.
// V needs the key index along the instruction's K dimension whichever way round, i.e. transposed against its [key][128] cache rows.  It is
// transposed on the LDS WRITE (a thread holds 4 keys x 4 columns from four 16-byte loads and writes four 8-byte key runs): the write is
// per key tile and shared by four waves, the read is per matrix instruction, so the read keeps the plain conflict-free ds_read_b128.
// (The LDS transpose read was not used: its lane layout could not be verified without a device at hand.)
//
// LDS.  K tile [64 keys][128 + 8] halves: rows 68 dwords = 4 (mod 64) apart, the 16 rows x 16 bytes of a quarter-wave's ds_read_b128 fall
// on 64 distinct banks (dense_fast.hip's argument).  V^T tile [128 columns][64 + 8] halves: rows 36 dwords apart, 16 consecutive rows
// start at banks 36 r mod 64 = { 0, 36, 8, 44, 16, 52, 24, 60, 32, 4, 40, 12, 48, 20, 56, 28 }, four dwords each: 64 distinct banks.  The
// V write: a half-wave is 8 key groups (dwords 0, 4, 8, 12, 2, 6, 10, 14 of a row, two each) x 4 column groups four rows = 144 = 16
// (mod 64) dwords apart: 64 distinct banks.  Two buffers (70 KB; two workgroups per CU) behind a register stage: tile t + 1's global
// loads are issued before tile t's matrix instructions and narrowed and written to the other buffer behind them -- one barrier per tile.
// On the 128-query tile every K / V operand read feeds two matrix instructions.
//
// Key splits.  Workgroup z of KS walks tiles [z nkt / KS, (z + 1) nkt / KS) of its query tile's nkt visible tiles and writes un-normalised
// O, m and l to the workspace ([KS][H][N][128] then [KS][H][N][2] floats); k_flash_combine merges them in split order.  A split with no
// visible key for a row reports l = 0, m = -inf; the combine gives it weight 0 without forming -inf - -inf.  KS = 1 writes merged itself.
//   grid (ceil(N / tile), H, KS), 256 threads, dynamic LDS FLASH_LDS_BYTES
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "llamahip_internal.h"

namespace lh {

namespace {

typedef _Float16 fh8 __attribute__((ext_vector_type(8)));
typedef _Float16 fh4 __attribute__((ext_vector_type(4)));
typedef float ff4 __attribute__((ext_vector_type(4)));
typedef uint32_t fu4 __attribute__((ext_vector_type(4)));
typedef uint32_t fu2 __attribute__((ext_vector_type(2)));

constexpr int BKEY = FLASH_KEY_TILE, LDK = FLASH_HEAD + 8, LDV = BKEY + 8;      // halves between LDS rows
constexpr int KBUF = BKEY * LDK, BUF = KBUF + FLASH_HEAD * LDV;                // halves: the K part, one whole buffer
static_assert(2 * BUF * 2 == FLASH_LDS_BYTES, "flash_attn_plan.h states the LDS size");

// fp32 -> fp16, round to nearest even, saturating at the largest finite half
__device__ __forceinline__ _Float16 sat16(float x) { return (_Float16) __builtin_amdgcn_fmed3f(x, -65504.0f, 65504.0f); }
__device__ __forceinline__ fu4 narrow8(const ff4 &a, const ff4 &b) {
    const fh8 h = { sat16(a.x), sat16(a.y), sat16(a.z), sat16(a.w), sat16(b.x), sat16(b.y), sat16(b.z), sat16(b.w) };
    return __builtin_bit_cast(fu4, h);
}
// the value of lane ^ 16 (ds_swizzle bit mode: and 0x1f, or 0, xor 0x10) and max / sum over the lane pair 32 apart (v_permlane32_swap)
__device__ __forceinline__ float xor16(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F)); }
// the value of lane ^ 32: ds_bpermute (the swizzle crossbar, no LDS memory).  (v_permlane32_swap would do, but this toolchain drops the second
// half of __builtin_amdgcn_permlane32_swap's result: measured, the reductions came back over lanes 0 .. 31 only)
__device__ __forceinline__ float xor32(float v) {
    const int lane = (int) __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ float max4(float v) {
    v = fmaxf(v, xor16(v));
    return fmaxf(v, xor32(v));
}
__device__ __forceinline__ float sum4(float v) {
    v = v + xor16(v);
    return v + xor32(v);
}

template <int TI>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))   // <= 256 registers: two workgroups per CU
k_flash_attn(const float *__restrict__ qr, const float *__restrict__ Kc, const float *__restrict__ Vc, float *__restrict__ merged, long m_stride,
             float *__restrict__ ws_o, float *__restrict__ ws_ml, int n_past, int N, int d, float c) {
    constexpr int QW = 16 * TI, TQ = 4 * QW;               // queries per wave, per workgroup
    extern __shared__ __attribute__((aligned(16))) uint16_t fa_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const int qt = gridDim.x - 1 - blockIdx.x, h = blockIdx.y, H = gridDim.y, z = blockIdx.z, KS = gridDim.z;
    const int q0 = qt * TQ, T = n_past + N;
    const int nkt = (n_past + min(q0 + TQ, N) + BKEY - 1) / BKEY;      // key tiles the query tile sees
    const int t0 = (int) ((long) z * nkt / KS), t1 = (int) ((long) (z + 1) * nkt / KS);
    const size_t hoff = (size_t) h * FLASH_HEAD;

    // Q: narrowed once, in registers for the whole walk.  A row past N is a clamped re-read, computed and never stored
    int qrow[TI];
    fh8 qreg[TI][4];
#pragma unroll
    for (int i = 0; i < TI; i++) {
        qrow[i] = min(q0 + wave * QW + 16 * i + r, N - 1);
        const float *p = qr + (size_t) qrow[i] * d + hoff + 8 * g;
#pragma unroll
        for (int s = 0; s < 4; s++) qreg[i][s] = __builtin_bit_cast(fh8, narrow8(*(const ff4 *) (p + 32 * s), *(const ff4 *) (p + 32 * s + 4)));
    }
    // staging.  K: chunk j of this thread is key row (tid >> 4) + 16 j, elements 8 (tid & 15) ..; V: unit j is keys 32 j + 4 kgl .. + 3, columns
    // 4 cg .. + 3, written as four key runs at k-slot 32 j + 8 (kgl & 3) + 4 (kgl >> 2) of rows 4 cg .. 4 cg + 3 (the permutation above)
    const int krow = tid >> 4, kcol = (tid & 15) * 8;
    const int kgl = tid & 7, cg = ((tid >> 5) & 7) * 4 + ((tid >> 3) & 3);
    const int kdst = krow * LDK + kcol, vdst = KBUF + 4 * cg * LDV + 8 * (kgl & 3) + 4 * (kgl >> 2);
    const float *ksrc = Kc + hoff + kcol, *vsrc = Vc + hoff + 4 * cg;
    ff4 ka[4], kb[4], vv[2][4];
    // tile TT's rows into the register stage; a row at or past T is a clamped re-read of row T - 1 (masked: weight 0, and finite if the eval's rows are)
#define FA_LOAD(TT)                                                                                \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < 4; j++) {                                                                  \
        const float *p = ksrc + (size_t) min((TT) * BKEY + krow + 16 * j, T - 1) * d;               \
        ka[j] = *(const ff4 *) p;                                                                  \
        kb[j] = *(const ff4 *) (p + 4);                                                            \
    }                                                                                              \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < 2; j++)                                                                    \
        _Pragma("unroll")                                                                          \
        for (int i = 0; i < 4; i++) vv[j][i] = *(const ff4 *) (vsrc + (size_t) min((TT) * BKEY + 32 * j + 4 * kgl + i, T - 1) * d);
#define FA_STAGE(B)                                                                                \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < 4; j++) *(fu4 *) (fa_lds + (B) * BUF + kdst + 16 * j * LDK) = narrow8(ka[j], kb[j]); \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < 2; j++)                                                                    \
        _Pragma("unroll")                                                                          \
        for (int cc = 0; cc < 4; cc++) {                                                           \
            const fh4 hv = { sat16(vv[j][0][cc]), sat16(vv[j][1][cc]), sat16(vv[j][2][cc]), sat16(vv[j][3][cc]) }; \
            *(fu2 *) (fa_lds + (B) * BUF + vdst + cc * LDV + 32 * j) = __builtin_bit_cast(fu2, hv); \
        }

    ff4 o[TI][8];
    float m[TI], l[TI];                                    // l: this lane's share of the row sum (its keys 4 g .. 4 g + 3 of every block)
#pragma unroll
    for (int i = 0; i < TI; i++) {
        m[i] = -INFINITY; l[i] = 0.0f;
#pragma unroll
        for (int db = 0; db < 8; db++) o[i][db] = ff4{ 0.0f, 0.0f, 0.0f, 0.0f };
    }
    const int wq_last = n_past + min(q0 + wave * QW + QW - 1, N - 1);      // the last key any query of this wave sees
    const int koff = r * LDK + 8 * g, voff = KBUF + r * LDV + 8 * g;
    if (t0 < t1) {                                         // (workgroup-uniform: an empty split runs no barrier at all)
        FA_LOAD(t0)
        FA_STAGE(0)
        __syncthreads();
    }
    for (int t = t0; t < t1; t++) {
        const int b = (t - t0) & 1, kt0 = t * BKEY;
        FA_LOAD(min(t + 1, t1 - 1))
        __builtin_amdgcn_sched_barrier(0);                 // the next tile goes out BEFORE this one is consumed
        if (kt0 <= wq_last) {                              // wave-uniform: a tile above this wave's diagonal is skipped, not its barrier
            const uint16_t *cur = fa_lds + b * BUF;
            ff4 s[4][TI];
#pragma unroll
            for (int kb4 = 0; kb4 < 4; kb4++)
#pragma unroll
                for (int i = 0; i < TI; i++) s[kb4][i] = ff4{ 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
            for (int st = 0; st < 4; st++)
#pragma unroll
                for (int kb4 = 0; kb4 < 4; kb4++) {
                    const fh8 a = *(const fh8 *) (cur + koff + 16 * kb4 * LDK + 32 * st);
#pragma unroll
                    for (int i = 0; i < TI; i++) s[kb4][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qreg[i][st], s[kb4][i], 0, 0, 0);
                }
            fh8 pk[TI][2];
#pragma unroll
            for (int i = 0; i < TI; i++) {
                const int lim = n_past + qrow[i];          // the query's own position: its last visible key
                float mx = -INFINITY;
#pragma unroll
                for (int kb4 = 0; kb4 < 4; kb4++)
#pragma unroll
                    for (int rr = 0; rr < 4; rr++) {
                        const float v = kt0 + 16 * kb4 + 4 * g + rr <= lim ? s[kb4][i][rr] * c : -INFINITY;
                        s[kb4][i][rr] = v;
                        mx = fmaxf(mx, v);
                    }
                mx = max4(mx);
                const float mn = fmaxf(m[i], mx), mref = mn == -INFINITY ? 0.0f : mn;      // no visible key yet: subtract 0, not -inf
                const float alpha = __builtin_amdgcn_exp2f(m[i] - mref);
                m[i] = mn;
                float ls = 0.0f;
#pragma unroll
                for (int ks = 0; ks < 2; ks++)
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const _Float16 ph = (_Float16) __builtin_amdgcn_exp2f(s[2 * ks + (e >> 2)][i][e & 3] - mref);
                        pk[i][ks][e] = ph;
                        ls = ls + (float) ph;
                    }
                l[i] = l[i] * alpha + ls;
#pragma unroll
                for (int db = 0; db < 8; db++) o[i][db] = o[i][db] * alpha;
            }
#pragma unroll
            for (int ks = 0; ks < 2; ks++)
#pragma unroll
                for (int db = 0; db < 8; db++) {
                    const fh8 a = *(const fh8 *) (cur + voff + 16 * db * LDV + 32 * ks);
#pragma unroll
                    for (int i = 0; i < TI; i++) o[i][db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pk[i][ks], o[i][db], 0, 0, 0);
                }
        }
        __builtin_amdgcn_sched_barrier(0);
        // the other buffer was last read in iteration t - 1, which every wave left through the barrier below
        FA_STAGE(b ^ 1)
        __syncthreads();
    }
#undef FA_LOAD
#undef FA_STAGE
    // D register rr of lane (r, g): column 16 db + 4 g + rr of query r
#pragma unroll
    for (int i = 0; i < TI; i++) {
        const int n = q0 + wave * QW + 16 * i + r;
        const float lt = sum4(l[i]);
        if (n >= N) continue;
        if (KS == 1) {
            float *dst = merged + (size_t) n * m_stride + hoff + 4 * g;
#pragma unroll
            for (int db = 0; db < 8; db++)
#pragma unroll
                for (int rr = 0; rr < 4; rr++) dst[16 * db + rr] = o[i][db][rr] / lt;
        } else {
            const size_t row = ((size_t) z * H + h) * N + n;
            float *dst = ws_o + row * FLASH_HEAD + 4 * g;
#pragma unroll
            for (int db = 0; db < 8; db++) *(ff4 *) (dst + 16 * db) = o[i][db];
            if (g == 0) { ws_ml[2 * row] = m[i]; ws_ml[2 * row + 1] = lt; }
        }
    }
}

// merged[n][h * 128 + c] = sum_z w_z O_z[c] / sum_z w_z l_z in split order, w_z = exp2(m_z - max m) -- 0 for a split that saw no key of the row
// (l_z = 0: its m_z = -inf never enters a subtraction).  grid (N, H), 128 threads
__global__ void __launch_bounds__(128)
k_flash_combine(const float *__restrict__ ws_o, const float *__restrict__ ws_ml, float *__restrict__ merged, long m_stride, int N, int KS) {
    const int n = blockIdx.x, h = blockIdx.y, H = gridDim.y, cc = threadIdx.x;
    float mx = -INFINITY;
    for (int z = 0; z < KS; z++) {
        const size_t row = ((size_t) z * H + h) * N + n;
        if (ws_ml[2 * row + 1] > 0.0f) mx = fmaxf(mx, ws_ml[2 * row]);
    }
    float num = 0.0f, den = 0.0f;
    for (int z = 0; z < KS; z++) {
        const size_t row = ((size_t) z * H + h) * N + n;
        const float lz = ws_ml[2 * row + 1];
        if (!(lz > 0.0f)) continue;
        const float w = __builtin_amdgcn_exp2f(ws_ml[2 * row] - mx);
        num = num + w * ws_o[row * FLASH_HEAD + cc];
        den = den + w * lz;
    }
    merged[(size_t) n * m_stride + (size_t) h * FLASH_HEAD + cc] = num / den;
}

}  // namespace

long g_flash_attn_launches = 0;

hipError_t init_attrs_flash_attn() {
    for (const void *kernel : { (const void *) k_flash_attn<1>, (const void *) k_flash_attn<2> }) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FLASH_LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// qr: the N rotated query rows; Kc / Vc: the layer's caches with rows n_past .. n_past + N - 1 appended (launch_rope_kv); ws: p.ws_bytes of
// workspace where the plan splits.  p: flash_attn_plan's answer for this (N, n_past + N, H)
hipError_t launch_flash_attn(const FlashAttnPlan &p, const float *qr, const float *Kc, const float *Vc, float *merged, long merged_stride,
                             int n_past, int N, int d, int H, float *ws, hipStream_t st) {
    if (!p.ok || !qr || !Kc || !Vc || !merged || d != H * FLASH_HEAD || n_past < 0 || (p.ks > 1 && !ws)) return hipErrorInvalidValue;
    const long ms = merged_stride > 0 ? merged_stride : d;
    const float kq_scale = 1.0f / sqrtf((float) d / (float) H);          // launch_attn's
    const float c = kq_scale * 1.44269504088896340736f;
    float *ws_o = p.ks > 1 ? ws : nullptr, *ws_ml = p.ks > 1 ? ws + (size_t) p.ks * H * N * FLASH_HEAD : nullptr;
    const dim3 grid(p.grid_x, p.grid_y, p.grid_z), block(256);
    if (p.tile == 128) hipLaunchKernelGGL(k_flash_attn<2>, grid, block, p.lds, st, qr, Kc, Vc, merged, ms, ws_o, ws_ml, n_past, N, d, c);
    else               hipLaunchKernelGGL(k_flash_attn<1>, grid, block, p.lds, st, qr, Kc, Vc, merged, ms, ws_o, ws_ml, n_past, N, d, c);
    g_flash_attn_launches++;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || p.ks == 1) return e;
    hipLaunchKernelGGL(k_flash_combine, dim3(N, H), dim3(128), 0, st, ws_o, ws_ml, merged, ms, N, p.ks);
    g_flash_attn_launches++;
    return hipGetLastError();
}

}  // namespace lh
