// q41_fast.hip -- k_q41_act_f16 + k_q41_fast: the OPT-IN long-eval mat-mul of Q4_1 model files on the fp16 matrix cores
// (LLAMAHIP_FLAG_FAST_Q41, llamahip_op_mul_mat_q4_1_fast).  NOT the reference's arithmetic: the exact path is k_q41_chain
// (dense.hip), one ordered fp32 chain of K/2 dependent adds per output.
//
// The stated arithmetic (the contract; tests/test_gpu_q41_fast_op.py holds the kernel to it):
//   activations   a row is quantized with quantize_row_q4_1's min, d, id and code, bit for bit what k_q41_act computes, and expanded as
//                 a32 = fl(fl(d1 * code) + m1) in fp32, as the exact path expands it; then narrowed ONCE to fp16, round to nearest even,
//                 saturating at +-65504.
//   weights       f32 = fl(fl(d0 * q) + m0) in fp32 -- the exact path's two separately rounded operations, no contraction (the translation
//                 unit is compiled with -ffp-contract=off) -- narrowed once to fp16 the same way.
//   products, sum every product f16 * a16 is exact in fp32 (11 x 11 significand bits); an output is ONE fp32 sum of the K products in
//                 whatever order v_mfma_f32_16x16x32_f16 and the K tiling give; the residual is added last, in fp32.
//   what differs from the exact path: two 2^-11 narrowings and the summation order.  The quantization of the activations is unchanged
//   (min and max of a block do not depend on the order they are found in; only the sign of a zero min / max can, where a block holds
//   both -0 and +0).
//
// The within-chunk order, decided here once: inside every 8-element chunk of a row, BOTH operands are stored as elements
//   0, 2, 4, 6, 1, 3, 5, 7
// -- a 32-bit word of nibble bytes holds elements 8 c .. 8 c + 7 of its block, and w & 0x0F0F0F0F is elements 0, 2, 4, 6 (the low
// nibbles of its four bytes), (w >> 4) & 0x0F0F0F0F elements 1, 3, 5, 7.  The pairing inside a 32-element matrix-core step is free as long
// as A and B agree, so the weight side never shuffles a nibble and k_q41_act_f16 pays the permutation once per activation.
//
// k_q41_act_f16.  Eight lanes own a block of 32 activations: one coalesced 16-byte load each, min / max over the lane's four values and
// then across the eight lanes (xor 1, 2, 4), d, id and the four codes per lane with k_q41_act's own expressions.  A lane packs its
// elements of even and of odd index, swaps one packed pair with its neighbour and stores 8 bytes: the even lane of a chunk holds
// positions 0 .. 3 (elements 0, 2, 4, 6), the odd lane positions 4 .. 7.  Output: fp16 rows [N][K] in the scratch k_q41_act uses.
//
// k_q41_fast.  k_dense_f16_fast's structure (dense_fast.hip, 12.35): four waves own TN activation rows x TM weight rows and walk K in tiles
// of BK; a wave holds TI x TJ accumulator tiles; two LDS buffers and a register stage -- tile t + 1's global loads are issued before
// tile t's matrix instructions and land in the other buffer behind them, one barrier per K tile; LDS rows are BK + 8 halves apart, so
// the 16 rows x 16 bytes of a quarter-wave's ds_read_b128 (and of the staging writes) fall on 64 distinct banks.
// The weight staging is the new part.  It reads the load-time copy k_q41_chain reads, MD[row-block of 64][block][lane] = {min, d} and
// NB[..] = 16 nibble bytes: no second copy.  A staging item is one block of one weight row: a 16-byte and an 8-byte load, 6 dwords in
// flight for 32 weights; consecutive threads take consecutive rows of a row-block, so a wave reads 1 KiB (+ 512 B) contiguous.  The
// thread splits each word with the two masks, converts bytes to floats, applies d0, then m0 (two rounded operations), narrows, and
// writes four 16-byte chunks.  The activation side is one 16-byte load per chunk, no conversion.
// Edges.  No branch surrounds a load: rows past N are clamped re-reads, never stored; weight rows past M are the repack's zero rows (a
// 128-row tile's second row-block past the copy is a clamped re-read), never stored; a K tile's blocks past K and the prefetch behind
// the last tile are clamped re-reads replaced by zeros on BOTH sides before they reach LDS; a wave wholly past N skips the arithmetic,
// not the barriers.  No scratch, no cross-workgroup hand-off.
//   grid (ceil(N / TN), ceil(M / TM)) -- grid x walks the row tiles: the workgroups that share a weight tile are neighbours in launch
//   order -- 256 threads, dynamic LDS 2 * (TN + TM) * (BK + 8) * 2 bytes (q41_fast_plan, q41_fast_plan.cpp)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "llamahip_internal.h"

namespace lh {

namespace {

typedef _Float16 qh2 __attribute__((ext_vector_type(2)));
typedef _Float16 qh8 __attribute__((ext_vector_type(8)));
typedef float qf2 __attribute__((ext_vector_type(2)));
typedef float qf4 __attribute__((ext_vector_type(4)));
typedef uint32_t qu2 __attribute__((ext_vector_type(2)));
typedef uint32_t qu4 __attribute__((ext_vector_type(4)));

// fp32 -> fp16, round to nearest even, saturating: a value beyond +-65504 narrows to +-65504, never to an infinity
__device__ __forceinline__ uint32_t narrow2(float a, float b) {
    const qh2 h = { (_Float16) __builtin_fminf(__builtin_fmaxf(a, -65504.0f), 65504.0f), (_Float16) __builtin_fminf(__builtin_fmaxf(b, -65504.0f), 65504.0f) };
    return __builtin_bit_cast(uint32_t, h);
}

// x [N] rows of K floats, x_stride apart (a multiple of 4; 16-byte aligned) -> a fp16 [N][K], chunks in the file header's order
__global__ void __launch_bounds__(256)
k_q41_act_f16(const float *__restrict__ x, long x_stride, int K, long nblocks, uint16_t *__restrict__ a) {
    const long blk = ((long) blockIdx.x * 256 + threadIdx.x) >> 3;      // eight lanes per block of 32: they leave together
    if (blk >= nblocks) return;
    const int nb = K / 32, sub = threadIdx.x & 7;
    const long n = blk / nb;
    const int i = (int) (blk % nb);
    const qf4 v = *(const qf4 *) (x + (size_t) n * x_stride + i * 32 + sub * 4);
    float mn = fminf(fminf(v.x, v.y), fminf(v.z, v.w)), mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) { mn = fminf(mn, __shfl_xor(mn, s)); mx = fmaxf(mx, __shfl_xor(mx, s)); }
    const float d = (mx - mn) / 15.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    float e[4];
#pragma unroll
    for (int l = 0; l < 4; l++) {
        const uint32_t q = (uint32_t) (uint8_t) round((double) ((v[l] - mn) * id)) & 0xF;      // k_q41_act's code, to the letter
        e[l] = d * (float) q + mn;
    }
    // this lane: elements 4 sub .. 4 sub + 3 of the block = elements (sub & 1) * 4 .. + 3 of chunk sub >> 1
    const uint32_t even = narrow2(e[0], e[2]), odd = narrow2(e[1], e[3]);
    const uint32_t got = (uint32_t) __shfl_xor((int) (sub & 1 ? even : odd), 1);
    const qu2 o = sub & 1 ? qu2{ got, odd } : qu2{ even, got };
    *(qu2 *) (a + (size_t) n * K + i * 32 + sub * 4) = o;
}

// 4 nibble-code bytes -> 4 weights f = fl(fl(d * q) + m), narrowed: two dwords of halves in byte order
__device__ __forceinline__ qu2 dequant4(uint32_t b, float m, float d) {
    const float f0 = d * (float) (b & 0xFFu) + m, f1 = d * (float) ((b >> 8) & 0xFFu) + m;
    const float f2 = d * (float) ((b >> 16) & 0xFFu) + m, f3 = d * (float) (b >> 24) + m;
    return qu2{ narrow2(f0, f1), narrow2(f2, f3) };
}

// TI x TJ accumulator tiles of 16 x 16 per wave, WN x WM waves (WN * WM == 4), BK elements per K tile
template <int TI, int TJ, int WN, int WM, int BK, int EPI>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))   // <= 256 registers: two workgroups per CU
k_q41_fast(const qf2 *__restrict__ md, const qu4 *__restrict__ nbv, int M, int K, const uint16_t *__restrict__ xp, int N,
           float *__restrict__ y, long y_stride, const float *__restrict__ resid, long resid_stride) {
    static_assert(WN * WM == 4 && BK % 32 == 0, "four waves, whole MFMA steps");
    constexpr int NT = 256, TN = 16 * TI * WN, TM = 16 * TJ * WM;
    constexpr int LD = BK + 8;                             // halves between LDS rows
    constexpr int CPR = BK / 8;                            // 8-element chunks per row and K tile
    constexpr int BPT = BK / 32;                           // Q4_1 blocks per row and K tile
    constexpr int XL = TN * CPR / NT;                      // activation chunks staged per thread
    constexpr int ITEMS = TM * BPT;                        // weight staging items (one block of one row) per K tile
    constexpr int WL = ITEMS >= NT ? ITEMS / NT : 1;       // ... per thread (narrow: 128 items, threads 128 .. 255 stage none)
    constexpr int RL = TM < 64 ? TM : 64;                  // consecutive threads walk this many rows of one row-block
    static_assert(XL >= 1 && TN * CPR % NT == 0 && (ITEMS % NT == 0 || NT % ITEMS == 0) && 64 % RL == 0 && TM % RL == 0, "whole chunks and items");
    constexpr int BUF = (TN + TM) * LD;                    // halves per LDS buffer
    extern __shared__ __attribute__((aligned(16))) uint16_t qf_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave / WM, wm = wave % WM;
    const int n0 = blockIdx.x * TN, m0 = blockIdx.y * TM;
    const int kc = K >> 3, nb = K >> 5, nrb = (M + 63) >> 6;
    const int nkt = (K + BK - 1) / BK;
    // activation chunk j of this thread: row (tid + j * NT) / CPR of the tile, chunk (tid + j * NT) % CPR of the K tile
    const uint16_t *xsrc[XL];
    int xdst[XL], xch[XL];
#pragma unroll
    for (int j = 0; j < XL; j++) {
        const int idx = tid + j * NT, row = idx / CPR, c = idx % CPR;
        xsrc[j] = xp + (size_t) min(n0 + row, N - 1) * K;
        xch[j] = c;
        xdst[j] = row * LD + c * 8;
    }
    // weight item j of this thread: row l + 64 * sub of the tile (l walks a row-block first), block wbl[j] of the K tile
    size_t wsrc[WL];                                       // entry index of block 0 of the row in the load-time copy
    int wdst[WL], wbl[WL];
    const bool wstage = tid < ITEMS;
#pragma unroll
    for (int j = 0; j < WL; j++) {
        const int idx = (tid + j * NT) % ITEMS, l = idx % RL, rest = idx / RL, sub = rest % (TM / RL), blk = rest / (TM / RL);
        const int m = m0 + sub * 64 + l;                   // (TM 16: sub is 0 and m0 % 64 places the 16 rows inside their row-block)
        wsrc[j] = (size_t) min(m >> 6, nrb - 1) * nb * 64 + (m & 63);
        wbl[j] = blk;
        wdst[j] = (TN + sub * 64 + l) * LD + blk * 32;
    }
    qu4 xq[XL], wq[WL];
    qf2 wmd[WL];
    // tile T's chunks and blocks into the register stage; one past K is a clamped re-read (replaced by zeros when it is written to LDS)
#define QF_LOAD(T)                                                                                 \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < XL; j++)                                                                   \
        xq[j] = *(const qu4 *) (xsrc[j] + (size_t) min((T) * CPR + xch[j], kc - 1) * 8);           \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < WL; j++) {                                                                 \
        const size_t at = wsrc[j] + (size_t) min((T) * BPT + wbl[j], nb - 1) * 64;                 \
        wq[j] = nbv[at];                                                                           \
        wmd[j] = md[at];                                                                           \
    }
#define QF_STAGE(T, B)                                                                             \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < XL; j++)                                                                   \
        *(qu4 *) (qf_lds + (B) * BUF + xdst[j]) = (T) * CPR + xch[j] < kc ? xq[j] : qu4{ 0u, 0u, 0u, 0u }; \
    if (wstage) {                                                                                  \
        _Pragma("unroll")                                                                          \
        for (int j = 0; j < WL; j++) {                                                             \
            const bool in = (T) * BPT + wbl[j] < nb;                                               \
            _Pragma("unroll")                                                                      \
            for (int c = 0; c < 4; c++) {                                                          \
                const qu2 lo = dequant4(wq[j][c] & 0x0F0F0F0Fu, wmd[j].x, wmd[j].y);              \
                const qu2 hi = dequant4((wq[j][c] >> 4) & 0x0F0F0F0Fu, wmd[j].x, wmd[j].y);       \
                *(qu4 *) (qf_lds + (B) * BUF + wdst[j] + c * 8) = in ? qu4{ lo.x, lo.y, hi.x, hi.y } : qu4{ 0u, 0u, 0u, 0u }; \
            }                                                                                      \
        }                                                                                          \
    }
    qf4 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
        for (int j = 0; j < TJ; j++) acc[i][j] = qf4{ 0.0f, 0.0f, 0.0f, 0.0f };
    const int r = lane & 15, q = lane >> 4;
    const bool live = n0 + wn * TI * 16 < N;               // wave-uniform
    const int aoff = (wn * TI * 16 + r) * LD + q * 8, boff = (TN + wm * TJ * 16 + r) * LD + q * 8;
    QF_LOAD(0)
    QF_STAGE(0, 0)
    __syncthreads();
    for (int t = 0; t < nkt; t++) {
        QF_LOAD(min(t + 1, nkt - 1))
        __builtin_amdgcn_sched_barrier(0);                 // the next tile goes out BEFORE this one is consumed
        if (live) {
            const uint16_t *cur = qf_lds + (t & 1) * BUF;
#pragma unroll
            for (int s = 0; s < BK / 32; s++) {
                qh8 a[TI], b[TJ];
#pragma unroll
                for (int i = 0; i < TI; i++) a[i] = *(const qh8 *) (cur + aoff + i * 16 * LD + s * 32);
#pragma unroll
                for (int j = 0; j < TJ; j++) b[j] = *(const qh8 *) (cur + boff + j * 16 * LD + s * 32);
#pragma unroll
                for (int i = 0; i < TI; i++)
#pragma unroll
                    for (int j = 0; j < TJ; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // the other buffer was last read in iteration t - 1, which every wave left through the barrier below
        QF_STAGE(t + 1, (t + 1) & 1)
        __syncthreads();
    }
#undef QF_LOAD
#undef QF_STAGE
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

// the three instances (q41_fast_plan): wide 128 x 128, mid 64 x 64, narrow 64 x 16
#define QF_WIDE(E)   (k_q41_fast<4, 4, 2, 2, 64, E>)
#define QF_MID(E)    (k_q41_fast<2, 2, 2, 2, 128, E>)
#define QF_NARROW(E) (k_q41_fast<1, 1, 4, 1, 256, E>)

}  // namespace

hipError_t init_attrs_q41_fast() {
    const int cap = 160 * 1024;          // two operand buffers: 68 .. 83 KB of dynamic LDS
    for (const void *kernel : { (const void *) QF_WIDE(EPI_STORE), (const void *) QF_WIDE(EPI_RESID), (const void *) QF_MID(EPI_STORE), (const void *) QF_MID(EPI_RESID),
                                (const void *) QF_NARROW(EPI_STORE), (const void *) QF_NARROW(EPI_RESID) }) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// x: N fp32 rows, x_stride apart; scratch: N * K halves (the buffer k_q41_act fills on the exact path); w: a handle's load-time Q4_1 copy
hipError_t launch_q41_fast(const DMat &w, int epi, const float *x, long x_stride, int N, float *y, long y_stride,
                           const float *resid, long resid_stride, hipStream_t st, float *scratch) {
    const Q41FastPlan p = q41_fast_plan(w.M, w.K, N);
    if (w.wtype != 3 || !p.ok || !x || !y || !scratch || x_stride % 4 != 0 || (epi != EPI_STORE && epi != EPI_RESID) || (epi == EPI_RESID && !resid)) return hipErrorInvalidValue;
    const long nblocks = (long) N * (w.K / 32);
    hipLaunchKernelGGL(k_q41_act_f16, dim3((unsigned) ((nblocks + 31) / 32)), dim3(256), 0, st, x, x_stride, w.K, nblocks, (uint16_t *) scratch);
    const dim3 grid(p.grid_x, p.grid_y), block(256);
#define QF_GO(KERNEL) hipLaunchKernelGGL(KERNEL, grid, block, p.lds, st, (const qf2 *) w.w, (const qu4 *) w.w2, w.M, w.K, (const uint16_t *) scratch, N, y, y_stride, resid, resid_stride)
    if (p.tile_cols == 128)     { if (epi == EPI_RESID) QF_GO(QF_WIDE(EPI_RESID)); else QF_GO(QF_WIDE(EPI_STORE)); }
    else if (p.tile_cols == 64) { if (epi == EPI_RESID) QF_GO(QF_MID(EPI_RESID)); else QF_GO(QF_MID(EPI_STORE)); }
    else                        { if (epi == EPI_RESID) QF_GO(QF_NARROW(EPI_RESID)); else QF_GO(QF_NARROW(EPI_STORE)); }
#undef QF_GO
    g_q41_fast_launches++;
    return hipGetLastError();
}

}  // namespace lh
