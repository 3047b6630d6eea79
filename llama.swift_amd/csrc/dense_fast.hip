// dense_fast.hip -- k_dense_f16_fast: the OPT-IN long-eval mat-mul of f16 model files on the fp16 matrix cores (LLAMAHIP_FLAG_FAST_DENSE,
// llamahip_op_mul_mat_f16_fast).  NOT the reference's arithmetic: the exact path is k_dense_mfma (dense.hip).
//
//   y[n][m] = sum_k W[m][k] * act(x[n][k])  (+ resid[n][m])        f16 weights, N >= 64 activation rows, fp32 accumulation
//
// Why stored order is enough.  The handle keeps every weight row in perm_index order (k_dense_perm_rows) and k_dense_prep /
// k_dense_perm_act leave every activation row in the SAME order: perm_index depends on the element index and K only, so position p of a
// stored weight row and position p of a stored activation row hold the same original element, in whole groups and in the tail group
// alike.  A dot product walked over stored positions 0 .. K - 1 therefore pairs the right elements; only the order in which fp32 adds
// the products differs from the reference's 32 chains, and that order is what this path does not promise.  No second copy of the weights.
//
// Why the operands are the exact path's.  ggml_vec_dot_f16 rounds every activation to fp16 once per row (WElem<1>::act): the fp32 words
// in the activation buffer already hold fp16 values, and narrowing them while staging is lossless.  Both operands are fp16, every
// product is exact in fp32 (11 x 11 significand bits), v_mfma_f32_16x16x32_f16 accumulates in fp32.  Nothing is rounded that act has
// not already rounded.
//
// The kernel.  A workgroup of four waves owns TN activation rows x TM weight rows and walks K in tiles of BK elements.  A thread stages
// 8-element chunks: one 16-byte load of a weight row, two 16-byte loads of an activation row narrowed to 8 halves; each chunk is one
// 16-byte LDS write at row * LD + chunk * 8.  LD = BK + 8 halves: rows are 4 (mod 64) dwords apart, so the 16 rows x 16 bytes of a
// quarter-wave's ds_read_b128 fall on 64 distinct banks.  A lane (r = lane & 15, q = lane >> 4) reads the 8 halves k = 8 q .. 8 q + 7
// of row r of a 16-row tile for A (activations) and B (weights) alike -- the pairing inside a 32-element step is the same on both
// sides, whatever it is.  A wave holds TI x TJ accumulator tiles: each A operand is used TJ times, each B operand TI times (wide
// instance: 8 LDS reads per 16 MFMAs).  Two LDS buffers and a register stage: tile t + 1's global loads are issued before tile t's
// MFMAs and written to the other buffer behind them -- one barrier per K tile.
// Edges.  No branch surrounds a load: rows past N, weight rows past M, chunks past K and the prefetch behind the last tile are clamped
// re-reads; chunks past K are replaced by zeros on BOTH sides before they reach LDS (0 * 0 adds +0 to a sum that no parity claim rests
// on: zero padding is harmless here, unlike in k_dense_mfma), so K need only be a multiple of 32 whatever BK is; rows past N and weight
// rows past M are computed and never stored; a wave whose rows lie wholly past N skips the arithmetic, not the barriers.
// No scratch, no cross-workgroup hand-off.
//   grid (ceil(N / TN), ceil(M / TM)) -- the workgroups that share a weight tile are neighbours in launch order -- 256 threads,
//   dynamic LDS 2 * (TN + TM) * (BK + 8) * 2 bytes
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "llamahip_internal.h"

namespace lh {

namespace {

typedef _Float16 fh8 __attribute__((ext_vector_type(8)));
typedef float ff4 __attribute__((ext_vector_type(4)));
typedef uint32_t fu4 __attribute__((ext_vector_type(4)));

// 8 fp32 words that hold fp16 values -> 8 halves (lossless), as the 16 bytes LDS takes
__device__ __forceinline__ fu4 narrow8(const ff4 &a, const ff4 &b) {
    const fh8 h = { (_Float16) a.x, (_Float16) a.y, (_Float16) a.z, (_Float16) a.w, (_Float16) b.x, (_Float16) b.y, (_Float16) b.z, (_Float16) b.w };
    return __builtin_bit_cast(fu4, h);
}

// TI x TJ accumulator tiles of 16 x 16 per wave, WN x WM waves (WN * WM == 4), BK elements per K tile
template <int TI, int TJ, int WN, int WM, int BK, int EPI>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))   // <= 256 registers: two workgroups per CU
k_dense_f16_fast(const uint16_t *__restrict__ w, int M, int K, const float *__restrict__ xp, int N,
                 float *__restrict__ y, long y_stride, const float *__restrict__ resid, long resid_stride) {
    static_assert(WN * WM == 4 && BK % 32 == 0, "four waves, whole MFMA steps");
    constexpr int NT = 256, TN = 16 * TI * WN, TM = 16 * TJ * WM;
    constexpr int LD = BK + 8;                             // halves between LDS rows
    constexpr int CPR = BK / 8;                            // 8-element chunks per row and K tile
    constexpr int XL = TN * CPR / NT, WL = TM * CPR / NT;  // chunks staged per thread
    static_assert(XL >= 1 && WL >= 1 && TN * CPR % NT == 0 && TM * CPR % NT == 0, "every thread stages whole chunks");
    constexpr int BUF = (TN + TM) * LD;                    // halves per LDS buffer
    extern __shared__ __attribute__((aligned(16))) uint16_t ff_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave / WM, wm = wave % WM;
    const int n0 = blockIdx.x * TN, m0 = blockIdx.y * TM;
    const int kc = K >> 3;                                 // chunks per row
    const int nkt = (K + BK - 1) / BK;
    // chunk j of this thread: row (tid + j * NT) / CPR of the tile, chunk (tid + j * NT) % CPR of the K tile
    const float *xsrc[XL];
    const uint16_t *wsrc[WL];
    int xdst[XL], xch[XL], wdst[WL], wch[WL];
#pragma unroll
    for (int j = 0; j < XL; j++) {
        const int idx = tid + j * NT, row = idx / CPR, c = idx % CPR;
        xsrc[j] = xp + (size_t) min(n0 + row, N - 1) * K;
        xch[j] = c;
        xdst[j] = row * LD + c * 8;
    }
#pragma unroll
    for (int j = 0; j < WL; j++) {
        const int idx = tid + j * NT, row = idx / CPR, c = idx % CPR;
        wsrc[j] = w + (size_t) min(m0 + row, M - 1) * K;
        wch[j] = c;
        wdst[j] = (TN + row) * LD + c * 8;
    }
    ff4 xa[XL], xb[XL];
    fu4 wq[WL];
    // tile T's chunks into the register stage; a chunk past K is a clamped re-read (replaced by zeros when it is written to LDS)
#define FF_LOAD(T)                                                                                 \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < XL; j++) {                                                                 \
        const float *p = xsrc[j] + (size_t) min((T) * CPR + xch[j], kc - 1) * 8;                   \
        xa[j] = *(const ff4 *) p;                                                                  \
        xb[j] = *(const ff4 *) (p + 4);                                                            \
    }                                                                                              \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < WL; j++)                                                                   \
        wq[j] = *(const fu4 *) (wsrc[j] + (size_t) min((T) * CPR + wch[j], kc - 1) * 8);      
#define FF_STAGE(T, B)                                                                             \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < XL; j++) {                                                                 \
        const fu4 v = narrow8(xa[j], xb[j]);                                                       \
        *(fu4 *) (ff_lds + (B) * BUF + xdst[j]) = (T) * CPR + xch[j] < kc ? v : fu4{ 0u, 0u, 0u, 0u }; \
    }                                                                                              \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < WL; j++)                                                                   \
        *(fu4 *) (ff_lds + (B) * BUF + wdst[j]) = (T) * CPR + wch[j] < kc ? wq[j] : fu4{ 0u, 0u, 0u, 0u };
    ff4 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
        for (int j = 0; j < TJ; j++) acc[i][j] = ff4{ 0.0f, 0.0f, 0.0f, 0.0f };
    const int r = lane & 15, q = lane >> 4;
    const bool live = n0 + wn * TI * 16 < N;               // wave-uniform
    const int aoff = (wn * TI * 16 + r) * LD + q * 8, boff = (TN + wm * TJ * 16 + r) * LD + q * 8;
    FF_LOAD(0)
    FF_STAGE(0, 0)
    __syncthreads();
    for (int t = 0; t < nkt; t++) {
        FF_LOAD(min(t + 1, nkt - 1))
        __builtin_amdgcn_sched_barrier(0);                 // the next tile goes out BEFORE this one is consumed
        if (live) {
            const uint16_t *cur = ff_lds + (t & 1) * BUF;
#pragma unroll
            for (int s = 0; s < BK / 32; s++) {
                fh8 a[TI], b[TJ];
#pragma unroll
                for (int i = 0; i < TI; i++) a[i] = *(const fh8 *) (cur + aoff + i * 16 * LD + s * 32);
#pragma unroll
                for (int j = 0; j < TJ; j++) b[j] = *(const fh8 *) (cur + boff + j * 16 * LD + s * 32);
#pragma unroll
                for (int i = 0; i < TI; i++)
#pragma unroll
                    for (int j = 0; j < TJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // the other buffer was last read in iteration t - 1, which every wave left through the barrier below
        FF_STAGE(t + 1, (t + 1) & 1)
        __syncthreads();
    }
#undef FF_LOAD
#undef FF_STAGE
    if (!live) return;
    // D register rr of lane (r, q): activation row 4 q + rr, weight row r of the tile
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int n = n0 + (wn * TI + i) * 16 + q * 4 + rr;
#pragma unroll
            for (int j = 0; j < TJ; j++) {
                const int m = m0 + (wm * TJ + j) * 16 + r;
                if (n < N && m < M) {
                    float s = acc[i][j][rr];
                    if (EPI == EPI_RESID) s = s + resid[(size_t) n * resid_stride + m];      // the residual last, in fp32
                    y[(size_t) n * y_stride + m] = s;
                }
            }
        }
}

// the three instances (dense_fast_plan): wide 128 x 128, mid 64 x 64, narrow 64 x 16
#define FF_WIDE(E)   (k_dense_f16_fast<4, 4, 2, 2, 64, E>)
#define FF_MID(E)    (k_dense_f16_fast<2, 2, 2, 2, 128, E>)
#define FF_NARROW(E) (k_dense_f16_fast<1, 1, 4, 1, 256, E>)

}  // namespace

long g_dense_fast_launches = 0;

// The instance rule, the one place that derives it.  Wider tiles re-read less (a workgroup streams (TN + TM) K elements for TN TM K
// products) but make fewer workgroups, and a 64-row eval is a race for HBM bytes in flight, not for MFMA issue: take the widest tile that
// still makes a workgroup for every one of the 256 CUs (wide) or for every second one (mid: two of its workgroups fit a CU, a weight tile
// of 16 KB in flight each), else the narrow one -- wo (4096 x 4096) against 64 rows is 32 / 64 / 256 workgroups.  K tiles grow as the
// tile narrows so that a workgroup keeps 8 .. 16 KB of weights in flight.
DenseFastPlan dense_fast_plan(int M, int K, int N) {
    DenseFastPlan p = { 0, 0, 0, 0, 0, 0, 0 };
    if (M < 1 || K < 32 || K % 32 != 0 || N < DENSE_FAST_MIN_ROWS) return p;
    auto wgs = [&](int tn, int tm) { return (long) ((N + tn - 1) / tn) * ((M + tm - 1) / tm); };
    if (wgs(128, 128) >= 256)    { p.tile_rows = 128; p.tile_cols = 128; p.k_tile = 64; }
    else if (wgs(64, 64) >= 128) { p.tile_rows = 64;  p.tile_cols = 64;  p.k_tile = 128; }
    else                         { p.tile_rows = 64;  p.tile_cols = 16;  p.k_tile = 256; }
    p.grid_x = (N + p.tile_rows - 1) / p.tile_rows;
    p.grid_y = (M + p.tile_cols - 1) / p.tile_cols;
    if (p.grid_y > 65535) return p;
    p.lds = 2 * (p.tile_rows + p.tile_cols) * (p.k_tile + 8) * 2;
    p.ok = 1;
    return p;
}

hipError_t init_attrs_dense_fast() {
    const int cap = 160 * 1024;          // two operand buffers: 68 .. 83 KB of dynamic LDS
    for (const void *kernel : { (const void *) FF_WIDE(EPI_STORE), (const void *) FF_WIDE(EPI_RESID), (const void *) FF_MID(EPI_STORE), (const void *) FF_MID(EPI_RESID),
                                (const void *) FF_NARROW(EPI_STORE), (const void *) FF_NARROW(EPI_RESID) }) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// xp: the N prepared activation rows (k_dense_prep / k_dense_perm_act for f16 weights); w: a handle's permuted f16 rows
hipError_t launch_dense_f16_fast(const DMat &w, int epi, const float *xp, int N, float *y, long y_stride,
                                 const float *resid, long resid_stride, hipStream_t st) {
    const DenseFastPlan p = dense_fast_plan(w.M, w.K, N);
    if (w.wtype != 1 || !p.ok || !xp || !y || (epi != EPI_STORE && epi != EPI_RESID) || (epi == EPI_RESID && !resid)) return hipErrorInvalidValue;
    const dim3 grid(p.grid_x, p.grid_y), block(256);
#define FF_GO(KERNEL) hipLaunchKernelGGL(KERNEL, grid, block, p.lds, st, (const uint16_t *) w.w, w.M, w.K, xp, N, y, y_stride, resid, resid_stride)
    if (p.tile_cols == 128)     { if (epi == EPI_RESID) FF_GO(FF_WIDE(EPI_RESID)); else FF_GO(FF_WIDE(EPI_STORE)); }
    else if (p.tile_cols == 64) { if (epi == EPI_RESID) FF_GO(FF_MID(EPI_RESID)); else FF_GO(FF_MID(EPI_STORE)); }
    else                        { if (epi == EPI_RESID) FF_GO(FF_NARROW(EPI_RESID)); else FF_GO(FF_NARROW(EPI_STORE)); }
#undef FF_GO
    g_dense_fast_launches++;
    return hipGetLastError();
}

}  // namespace lh
