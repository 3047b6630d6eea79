// q41_dot.hip -- k_q41_act_q + k_q41_dot: the OPT-IN few-row mat-mul of Q4_1 model files on the 4-bit integer dot instruction
// (LLAMAHIP_FLAG_FAST_Q41_DECODE, llamahip_op_mul_mat_q4_1_dot): decode and evals below 64 rows.  NOT the reference's
// arithmetic: the exact path is k_q41_chain (dense.hip), one ordered fp32 chain of K/2 dependent adds per output.
//
// The stated arithmetic (the contract; tests/test_gpu_q41_dot_op.py holds the kernel to it):
//   activations   a row is quantized with quantize_row_q4_1's min (m1), d (d1), id and code, bit for bit what k_q41_act computes.  The codes
//                 stay 4-bit codes, nibble-packed like a Q4_1 block (byte j = code[2j] | code[2j+1] << 4); per block the record also keeps
//                 d1, m1, the integer S_c = sum of the 32 codes (as a float: exact, <= 480) and E = fma(d1, S_c, 32 * m1), one rounding.
//   per block     with the exact integers S_qc = sum q * c (<= 7200) and S_q = sum q (<= 480) from v_dot8_u32_u4, converted exactly to fp32:
//                     inner = fma(d1, S_qc, fl(m1 * S_q))          2 roundings
//                     term  = fma(d0, inner, fl(m0 * E))           2 roundings + E's one: 5 in all
//                 which is d0 d1 S_qc + d0 m1 S_q + m0 d1 S_c + 32 m0 m1 = sum_k (d0 q + m0)(d1 c + m1) over the UN-rounded operands.
//   per output    K-lane l (0 .. 15) adds the terms of blocks l, l + 16, l + 32, ... in that order, sum = fl(sum + term) from +0; the 16 lane
//                 sums p0 .. p15 are added as the fixed tree (((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)))+(((p8+p9)+(p10+p11))+((p12+p13)+(p14+p15)));
//                 the residual is added last.  A term passes through at most ceil(K/512) + 3 <= K/32 - 1 rounded adds (K < 512: lanes
//                 without a block hold +0, and adding +0 rounds nothing).
//   what differs from the exact path: the per-element roundings fl(fl(d q) + m) of both operands are gone, and the order of summation.
// Two properties handles and tests rely on.  DETERMINISTIC: every output is written once, by one workgroup, sums in the order above; no
// atomics, nothing handed between workgroups.  INDEPENDENT OF N: the order above is a function of K alone; the row count of a launch, the
// compiled instance NR and a row's place in its tile change which registers hold a row, never an operation on it (the translation unit is
// compiled with -ffp-contract=off and every fused operation is written as fmaf).
//
// k_q41_act_q.  k_q41_act_f16's lane scheme: eight lanes own a block of 32 activations, one coalesced 16-byte load each, min / max over
// the lane's four values and across the eight lanes (xor 1, 2, 4), d, id and the four codes with k_q41_act's own expressions.  A lane
// packs its four codes into 16 bits and adds them; xor 1 makes the word of a chunk, xor 1, 2, 4 the block's S_c; lane 0 gathers the four
// words and stores the 16 code bytes, lane 1 stores { d1, m1, S_c, E }.  Output: [N][K/32] records of 32 bytes in the scratch k_q41_act uses.
//
// k_q41_dot<NR, EPI>.  A workgroup owns 16 weight rows -- the 256-byte run of the load-time copy k_q41_chain reads, MD[row-block of
// 64][block][lane] = {min, d}, NB[..] = 16 nibble bytes; no second copy -- x all of K x up to NR activation rows, as 16 rows x 16 K-lanes:
// thread (r = tid & 15, l = tid >> 4) walks blocks l, l + 16, ...  A word of NB holds elements 8 c .. 8 c + 7 low nibble first, the order
// v_dot8_u32_u4 wants, and the record's words are packed the same way: four dot instructions give S_qc, four more against 0x11111111 S_q
// (once per weight block, whatever NR).  K is taken in slabs of q41_dot_slab(NR) blocks (64 up to 4 rows, 32 at 8, 16 from 12: four, two or one per
// K-lane; the slab decides what is staged together, never the order of a sum): the records of a slab, the same for every weight row, are
// staged in LDS (two buffers) and read back as two 16-byte reads whose four distinct addresses per wave are 128 contiguous bytes; the
// weights of slab s + 1 (a 16-byte and an 8-byte load per block) and its record chunks are issued before slab s is consumed and the
// chunks land in the other buffer behind it, one barrier per slab.  The 16 lane sums of an output meet in LDS (the record buffers, free
// by then) and 16 NR threads add them in the fixed tree.
// Edges.  No branch surrounds a load: blocks past K and rows past N are clamped re-reads; a block past K adds nothing (predicated add),
// a row past N is never stored; weight rows past M are the repack's zero rows, never stored.  No scratch, no cross-workgroup hand-off.
//   grid (ceil(M / 16), row tiles of 16), 256 threads, static LDS 2 * NR * slab * 32 bytes (q41_dot_plan, q41_dot_plan.cpp)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "llamahip_internal.h"

namespace lh {

namespace {

typedef float tf2 __attribute__((ext_vector_type(2)));
typedef float tf4 __attribute__((ext_vector_type(4)));
typedef uint32_t tu4 __attribute__((ext_vector_type(4)));

// x [N] rows of K floats, x_stride apart (a multiple of 4; 16-byte aligned) -> rec [N][K/32] x { 16 code bytes, { d1, m1, S_c, E } }
__global__ void __launch_bounds__(256)
k_q41_act_q(const float *__restrict__ x, long x_stride, int K, long nblocks, tu4 *__restrict__ rec) {
    const long blk = ((long) blockIdx.x * 256 + threadIdx.x) >> 3;      // eight lanes per block of 32: they leave together
    if (blk >= nblocks) return;
    const int nb = K / 32, sub = threadIdx.x & 7;
    const long n = blk / nb;
    const int i = (int) (blk % nb);
    const tf4 v = *(const tf4 *) (x + (size_t) n * x_stride + i * 32 + sub * 4);
    float mn = fminf(fminf(v.x, v.y), fminf(v.z, v.w)), mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) { mn = fminf(mn, __shfl_xor(mn, s)); mx = fmaxf(mx, __shfl_xor(mx, s)); }
    const float d = (mx - mn) / 15.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    uint32_t h = 0, sc = 0;
#pragma unroll
    for (int l = 0; l < 4; l++) {
        const uint32_t q = (uint32_t) (uint8_t) round((double) ((v[l] - mn) * id)) & 0xF;      // k_q41_act's code, to the letter
        h |= q << (4 * l);                                  // elements 4 sub .. 4 sub + 3: bytes 2 sub, 2 sub + 1 of the block, low nibble first
        sc += q;
    }
    const uint32_t other = (uint32_t) __shfl_xor((int) h, 1);
    const uint32_t word = sub & 1 ? other | h << 16 : h | other << 16;      // word sub >> 1 of the block, in both lanes of the pair
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) sc += (uint32_t) __shfl_xor((int) sc, s);
    tu4 codes;
#pragma unroll
    for (int c = 0; c < 4; c++) codes[c] = (uint32_t) __shfl((int) word, 2 * c, 8);
    const float fsc = (float) sc;
    const tf4 tail = { d, mn, fsc, fmaf(d, fsc, 32.0f * mn) };
    if (sub == 0) rec[blk * 2] = codes;
    if (sub == 1) rec[blk * 2 + 1] = __builtin_bit_cast(tu4, tail);
}

__device__ __forceinline__ uint32_t dot32(tu4 a, tu4 b) {
    return __builtin_amdgcn_udot8(a.x, b.x, __builtin_amdgcn_udot8(a.y, b.y, __builtin_amdgcn_udot8(a.z, b.z, __builtin_amdgcn_udot8(a.w, b.w, 0u, false), false), false), false);
}

template <int NR, int EPI>
__global__ void __launch_bounds__(256)
k_q41_dot(const tf2 *__restrict__ md, const tu4 *__restrict__ nbv, int M, int nb, const tu4 *__restrict__ rec, int N, int n_base,
          float *__restrict__ y, long y_stride, const float *__restrict__ resid, long resid_stride) {
    constexpr int NT = 256, SLAB = q41_dot_slab(NR), G = SLAB / Q41_DOT_KLANES;      // blocks per slab, and per thread and slab
    constexpr int CH = NR * SLAB * 2;                       // 16-byte chunks per slab of records
    constexpr int CPT = (CH + NT - 1) / NT;                         // ... per thread (a thread whose chunk index is past CH stages none)
    static_assert(Q41_DOT_ROWS == 16 && Q41_DOT_KLANES == 16 && G >= 1 && SLAB % Q41_DOT_KLANES == 0 && NR * NT * 4 <= 2 * CH * 16, "16 x 16 threads; the lane sums fit the two record buffers");
    __shared__ tu4 lds[2][CH];
    const int tid = threadIdx.x, r = tid & 15, kl = tid >> 4;
    const int m0 = blockIdx.x * Q41_DOT_ROWS, n0 = n_base + blockIdx.y * Q41_DOT_TILE;
    const int nslab = (nb + SLAB - 1) / SLAB;
    const size_t wbase = (size_t) (m0 >> 6) * nb * 64 + (m0 & 63) + r;      // block 0 of this thread's weight row in the load-time copy
    // record chunk j of this thread: row idx / 128 of the tile, block (idx % 128) / 2 of the slab, half idx % 2
    const tu4 *csrc[CPT];
    int cblk[CPT];
#pragma unroll
    for (int j = 0; j < CPT; j++) {
        const int idx = (tid + j * NT) % CH, n = idx / (SLAB * 2);
        cblk[j] = (idx % (SLAB * 2)) >> 1;
        csrc[j] = rec + (size_t) min(n0 + n, N - 1) * nb * 2 + (idx & 1);
    }
    tu4 wq[G], wqn[G], cr[CPT];
    tf2 wm[G], wmn[G];
    // slab S's weights and record chunks into registers; a block past K is a clamped re-read (it adds nothing below)
#define QD_LOAD(S, WQ, WM)                                                                           \
    _Pragma("unroll")                                                                                \
    for (int i = 0; i < G; i++) {                                                                    \
        const size_t at = wbase + (size_t) min((S) * SLAB + i * Q41_DOT_KLANES + kl, nb - 1) * 64; \
        WQ[i] = nbv[at];                                                                             \
        WM[i] = md[at];                                                                              \
    }                                                                                                \
    _Pragma("unroll")                                                                                \
    for (int j = 0; j < CPT; j++) cr[j] = csrc[j][(size_t) min((S) * SLAB + cblk[j], nb - 1) * 2];
#define QD_STAGE(B)                                                                                  \
    _Pragma("unroll")                                                                                \
    for (int j = 0; j < CPT; j++)                                                                    \
        if (tid + j * NT < CH) lds[B][tid + j * NT] = cr[j];
    float acc[NR];
#pragma unroll
    for (int n = 0; n < NR; n++) acc[n] = 0.0f;
    QD_LOAD(0, wq, wm)
    QD_STAGE(0)
    __syncthreads();
    for (int s = 0; s < nslab; s++) {
        const bool more = s + 1 < nslab;                     // workgroup-uniform
        if (more) { QD_LOAD(s + 1, wqn, wmn) }
        __builtin_amdgcn_sched_barrier(0);                   // the next slab goes out BEFORE this one is consumed
        const tu4 *cur = lds[s & 1];
#pragma unroll
        for (int i = 0; i < G; i++) {
            const bool live = s * SLAB + i * Q41_DOT_KLANES + kl < nb;
            const tu4 w = wq[i];
            const float fsq = (float) dot32(w, tu4{ 0x11111111u, 0x11111111u, 0x11111111u, 0x11111111u });
            const float wmin = wm[i].x, wd = wm[i].y;
#pragma unroll
            for (int n = 0; n < NR; n++) {
                const int at = (n * SLAB + i * Q41_DOT_KLANES + kl) * 2;
                const tu4 c = cur[at];
                const tf4 t = __builtin_bit_cast(tf4, cur[at + 1]);      // { d1, m1, S_c, E }
                const float inner = fmaf(t.x, (float) dot32(w, c), t.y * fsq);
                const float term = fmaf(wd, inner, wmin * t.w);
                if (live) acc[n] = acc[n] + term;
                if (n % 8 == 7) __builtin_amdgcn_sched_barrier(0);      // at most eight rows' records in registers at a time
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // the other buffer was last read in iteration s - 1, which every wave left through the barrier below
        if (more) {
            QD_STAGE((s + 1) & 1)
#pragma unroll
            for (int i = 0; i < G; i++) { wq[i] = wqn[i]; wm[i] = wmn[i]; }
        }
        __syncthreads();
    }
#undef QD_LOAD
#undef QD_STAGE
    // every wave is past the last slab's reads: the 16 lane sums of an output meet in the record buffers
    float *red = (float *) lds[0];
#pragma unroll
    for (int n = 0; n < NR; n++) red[(n * Q41_DOT_KLANES + kl) * Q41_DOT_ROWS + r] = acc[n];
    __syncthreads();
    if (tid >= NR * Q41_DOT_ROWS) return;
    const int n = tid >> 4, row = n0 + n, m = m0 + r;
    float p[Q41_DOT_KLANES];
#pragma unroll
    for (int l = 0; l < Q41_DOT_KLANES; l++) p[l] = red[(n * Q41_DOT_KLANES + l) * Q41_DOT_ROWS + r];
#pragma unroll
    for (int w = 1; w < Q41_DOT_KLANES; w <<= 1)
#pragma unroll
        for (int l = 0; l < Q41_DOT_KLANES; l += 2 * w) p[l] = p[l] + p[l + w];
    if (row >= N || m >= M) return;
    float sum = p[0];
    if (EPI == EPI_RESID) sum = sum + resid[(size_t) row * resid_stride + m];      // the residual last, in fp32
    y[(size_t) row * y_stride + m] = sum;
}

static hipError_t go_q41_dot(const Q41DotPlan &p, int grid_y, int n_base, const DMat &w, int epi, const tu4 *rec, int N, float *y, long y_stride,
                             const float *resid, long resid_stride, hipStream_t st) {
    const dim3 grid(p.grid_x, grid_y), block(p.threads);
    bool found = false;
#define QD_GO(NR) if (p.nr == NR) { found = true; \
        if (epi == EPI_RESID) hipLaunchKernelGGL((k_q41_dot<NR, EPI_RESID>), grid, block, 0, st, (const tf2 *) w.w, (const tu4 *) w.w2, w.M, w.K / 32, rec, N, n_base, y, y_stride, resid, resid_stride); \
        else hipLaunchKernelGGL((k_q41_dot<NR, EPI_STORE>), grid, block, 0, st, (const tf2 *) w.w, (const tu4 *) w.w2, w.M, w.K / 32, rec, N, n_base, y, y_stride, resid, resid_stride); \
    }
    LH_Q41_INSTANCES(QD_GO)
#undef QD_GO
    return found ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace

// x: N fp32 rows, x_stride apart; scratch: N * K bytes of records (the buffer k_q41_act fills on the exact path); w: a handle's load-time
// Q4_1 copy.  Full row tiles of 16 are one launch on gridDim.y, a last tile of N % 16 rows a launch of its own on the plan of that row count.
hipError_t launch_q41_dot(const DMat &w, int epi, const float *x, long x_stride, int N, float *y, long y_stride,
                          const float *resid, long resid_stride, hipStream_t st, float *scratch) {
    if (w.wtype != 3 || !q41_dot_plan(w.M, w.K, N).ok || !x || !y || !scratch || x_stride % 4 != 0 || (epi != EPI_STORE && epi != EPI_RESID) || (epi == EPI_RESID && !resid)) return hipErrorInvalidValue;
    const long nblocks = (long) N * (w.K / 32);
    hipLaunchKernelGGL(k_q41_act_q, dim3((unsigned) ((nblocks + 31) / 32)), dim3(256), 0, st, x, x_stride, w.K, nblocks, (tu4 *) scratch);
    hipError_t e = hipGetLastError();
    const int full = N / Q41_DOT_TILE, rem = N % Q41_DOT_TILE;
    if (e == hipSuccess && full) e = go_q41_dot(q41_dot_plan(w.M, w.K, Q41_DOT_TILE), full, 0, w, epi, (const tu4 *) scratch, N, y, y_stride, resid, resid_stride, st);
    if (e == hipSuccess && rem) e = go_q41_dot(q41_dot_plan(w.M, w.K, rem), 1, full * Q41_DOT_TILE, w, epi, (const tu4 *) scratch, N, y, y_stride, resid, resid_stride, st);
    if (e == hipSuccess) g_q41_dot_launches++;
    return e;
}

}  // namespace lh
