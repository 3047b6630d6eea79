// q40_few.hip -- k_q40_few: the OPT-IN few-row mat-mul of Q4_0 model files on the int8 matrix cores (LLAMAHIP_FLAG_FAST_Q40_FEW,
// llamahip_op_mul_mat_q4_0_few): 1 .. 63 activation rows, a flagged handle's 16 .. 63 -- wide batched decode steps, verify steps, the scheduler's steps,
// beam search, the reference's 9-token prompt flow.  NOT the reference's arithmetic: the exact k_gemv_set reproduces the reference's
// eight fp32 chains per block at 22 VALU instructions per (lane, chunk, column) and is bound by them from about 8 rows on.
//
// The stated arithmetic (the contract; tests/test_gpu_q40_few_op.py holds the kernel to it).  q = the weight block's codes - 8, d_w its
// scale; c, d_a the codes - 8 and the scale of quantize_row_q4_0 on the activation block (the existing qa_A / qa_d rows, bit for bit):
//   isum  = sum over the block's 32 elements of q c                    an exact integer (|isum| <= 2048)
//   acc   = fma((float) isum, fl(d_w * d_a), acc)                      two roundings per block
//   K-slice s of S adds the blocks of chunks (256 elements) s, s + S, s + 2 S, ... in ascending order, starting from +0
//   y     = ((slice 0 + slice 1) + slice 2) + ... + slice S - 1  (+ resid, added last)
// S = q40_few_slices(M): 8 up to 8192 weight rows, 4 above -- (M, K) alone decide every order; N, the column tile and a row's place in it
// decide none, so row n of an N-row call is bit for bit the one-row call.  No atomics; each output is owned by one workgroup.  Blocks of
// the zero padding behind K (both operands pad a row to whole chunks with code 8 = value 0 and scale 0) add fma(0, 0, acc).
//
// Work split.  A workgroup owns 16 weight rows = two row-groups of the load-time chain-major tile copy (QMat::tiles, no other copy is
// read) and ALL columns: NT = ceil(N / 16) column tiles of 16.  Its S waves are the K-slices.  Per chunk a wave
//   * holds the two tiles' nibbles as the A operands of v_mfma_i32_16x16x32_i8: lane (i = lane % 16, g = lane / 16) loaded the 32 bytes
//     of chains 2 g, 2 g + 1 of weight row i -- the K-group g of all eight blocks of the chunk -- straight from HBM (two 16-byte loads,
//     every byte of the tiles read once by one lane), PF chunks ahead in a register ring;
//   * unpacks them ONCE for all NT tiles: the stored nibble is the signed code q & 15, so `w & 0xF0F0F0F0` (odd block) and
//     `(w << 4) & 0xF0F0F0F0` (even block) are four int8 values 16 q each: the +8 of the file format never has to be removed;
//   * stages the chunk's 128 weight scales in LDS transposed to [block][row] (lane (i, g) loaded blocks g and 4 + g of row i), so that the
//     four scales of an accumulator's rows 4 g .. 4 g + 3 are one 16-byte LDS read;
//   * per tile reads the B operand in place from qa_A: column n = lane % 16 of the tile, the same two chains = 64 contiguous bytes (a
//     code sits in the low nibble of its byte for even blocks, in the high nibble for odd ones: the byte is 16 c after at most a shift)
//     and the 8 scales of the column's blocks from qa_d, one (chunk, tile) item ahead in registers;
//   * per block and tile: one MFMA (256 block sums 256 q c), then per accumulator `>> 8` (exact), convert, the scale product, the FMA.
// Columns past N read the all-zero tile that closes row-group 0 instead of an operand row (codes 0, scales 0) and are never stored.
// The slices meet in LDS ([slice][column][row] fp32), one barrier, and thread o adds output o's partials in slice order.
//   grid ceil(M / 16), 64 S threads, static LDS 8 (NT + 1/2) KiB (q40_few_plan, q40_few_plan.cpp)
#include "kcommon.hip.h"
#include "q40_few_plan.h"

namespace lh {

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct Q40FewArgs {
    const uint8_t *wt; int ngroups, nchunks, M, gmapF8;
    const uint8_t *qa_A; const float *qa_d;         // [N] operand rows: nchunks * 256 bytes / nchunks * 8 floats apart
    int N;
    float *y; long y_stride; const float *resid; long resid_stride;
};

constexpr int Q40_FEW_PF = 2;                       // chunks of weights in flight per wave behind the one being multiplied

// the B operand of one (chunk, column tile) item as a lane holds it: chains 2 g, 2 g + 1 of its column, blocks 0 .. 7 each, and the blocks' scales
struct Q40FewB { u32x4 q[4]; f32x4 d[2]; };

template <int NT, int EPI>
__global__ void __launch_bounds__(64 * Q40_FEW_MAX_SLICES)
k_q40_few(const Q40FewArgs a) {
    constexpr int PF = Q40_FEW_PF;
    __shared__ __attribute__((aligned(16))) float sW[Q40_FEW_MAX_SLICES][128];            // per wave: the chunk's weight scales [block][row]
    __shared__ __attribute__((aligned(16))) float red[Q40_FEW_MAX_SLICES][NT * 256];      // [slice][column][row]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, S = blockDim.x >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int nchunks = a.nchunks;
    const int g0 = blockIdx.x * 2;
    // the lane's weight row: row i & 7 of tile group g0 + (i >> 3) (a last workgroup of one group reads it twice and stores it once)
    const uint8_t *wp = a.wt + (size_t) min(g0 + (i >> 3), a.ngroups - 1) * (nchunks + 1) * TILE_BYTES;
    const uint32_t woff = (uint32_t) (((i & 7) * 8 + 2 * g) * 16), soff = (uint32_t) (1024 + (i & 7) * 32 + g * 8);
    // the lane's column of every tile: its operand row, or the zero tile closing row-group 0
    const uint8_t *zero = a.wt + (size_t) nchunks * TILE_BYTES;
    const uint8_t *ap[NT];
    const float *dp[NT];
    int astep[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int col = t * 16 + i;
        const bool live = col < a.N;
        ap[t] = live ? a.qa_A + (size_t) col * nchunks * 256 + g * 64 : zero + g * 64;
        dp[t] = live ? a.qa_d + (size_t) col * nchunks * 8 : (const float *) (zero + 1024);
        astep[t] = live ? 1 : 0;
    }
    const int nmine = wave < nchunks ? (nchunks - wave + S - 1) / S : 0;      // chunks wave, wave + S, ...

    u32x4 wq[PF][2];
    f32x2 ws[PF];
#define LH_FEW_LOADW(SLOT, CH) do {                                                                         \
        const uint8_t *tp_ = wp + (size_t) min((CH), nchunks) * TILE_BYTES;      /* past the row: the zero tile */ \
        wq[SLOT][0] = __builtin_nontemporal_load((const u32x4 *) (tp_ + woff));                              \
        wq[SLOT][1] = __builtin_nontemporal_load((const u32x4 *) (tp_ + woff + 16));                         \
        ws[SLOT] = __builtin_nontemporal_load((const f32x2 *) (tp_ + soff));                                 \
    } while (0)
    auto load_b = [&](int ch, int t) {
        Q40FewB b;
        const int c = min(ch, nchunks - 1) * astep[t];
        const u32x4 *p = (const u32x4 *) (ap[t] + (size_t) c * 256);
        const f32x4 *d = (const f32x4 *) (dp[t] + (size_t) c * 8);
#pragma unroll
        for (int v = 0; v < 4; v++) b.q[v] = p[v];
        b.d[0] = d[0]; b.d[1] = d[1];
        return b;
    };

    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = f32x4{ 0.0f, 0.0f, 0.0f, 0.0f };

#pragma unroll
    for (int u = 0; u < PF; u++) LH_FEW_LOADW(u, wave + u * S);
    Q40FewB bn = load_b(wave, 0);
    float *sw = sW[wave];
    for (int k0 = 0; k0 < nmine; k0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; u++) {
            const int ch = wave + (k0 + u) * S;
            if (k0 + u < nmine) {
                // the chunk's scales -> LDS [block][row]; its nibbles -> the eight blocks' A operands; the ring slot is free again
                __builtin_amdgcn_wave_barrier();
                sw[g * 16 + i] = ws[u].x;
                sw[(4 + g) * 16 + i] = ws[u].y;
                __builtin_amdgcn_wave_barrier();
                long A[8];
#pragma unroll
                for (int j2 = 0; j2 < 4; j2++) {
                    const uint32_t w0 = wq[u][0][j2], w1 = wq[u][1][j2];
                    A[2 * j2] = (long) (((uint64_t) ((w1 << 4) & 0xF0F0F0F0u) << 32) | ((w0 << 4) & 0xF0F0F0F0u));
                    A[2 * j2 + 1] = (long) (((uint64_t) (w1 & 0xF0F0F0F0u) << 32) | (w0 & 0xF0F0F0F0u));
                }
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const Q40FewB b = bn;
                    bn = t + 1 < NT ? load_b(ch, t + 1) : load_b(ch + S, 0);      // (behind the wave's last item: one load nobody uses)
                    // loads return in order: requested BEHIND the next item's operand, the ring's refill stays in flight across that
                    // item's wait and has two items' time to arrive
                    if (t == 0) LH_FEW_LOADW(u, ch + PF * S);
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        uint32_t b0 = b.q[j >> 2][j & 3], b1 = b.q[2 + (j >> 2)][j & 3];
                        if ((j & 1) == 0) { b0 <<= 4; b1 <<= 4; }
                        const long B = (long) (((uint64_t) b1 << 32) | b0);
                        const i32x4 p = __builtin_amdgcn_mfma_i32_16x16x32_i8(A[j], B, i32x4{ 0, 0, 0, 0 }, 0, 0, 0);
                        const f32x4 dw = *(const f32x4 *) (sw + j * 16 + 4 * g);
                        const float da = b.d[j >> 2][j & 3];
#pragma unroll
                        for (int r = 0; r < 4; r++) acc[t][r] = __builtin_fmaf((float) (p[r] >> 8), dw[r] * da, acc[t][r]);
                    }
                }
            }
        }
    }
#undef LH_FEW_LOADW

    // the slices meet: [slice][column][row], then output o = column * 16 + row in slice order
#pragma unroll
    for (int t = 0; t < NT; t++) *(f32x4 *) (&red[wave][(t * 16 + i) * 16 + 4 * g]) = acc[t];
    __syncthreads();
    for (int o = threadIdx.x; o < NT * 256; o += blockDim.x) {
        const int row = o & 15, col = o >> 4, tg = g0 + (row >> 3);
        float s = red[0][o];
        for (int w = 1; w < S; w++) s = s + red[w][o];
        int lg = tg;
        if (a.gmapF8) { const int b8 = tg >> 3, w8 = tg & 7; lg = w8 < 4 ? b8 * 4 + w8 : a.gmapF8 + b8 * 4 + (w8 - 4); }
        const int m = lg * 8 + (row & 7);
        if (tg < a.ngroups && m < a.M && col < a.N) {
            if (EPI == EPI_RESID) s = s + a.resid[(size_t) col * a.resid_stride + m];
            a.y[(size_t) col * a.y_stride + m] = s;
        }
    }
}

template <int NT>
static hipError_t go_q40_few(const Q40FewPlan &p, int epi, const Q40FewArgs &a, hipStream_t st) {
    static_assert(sizeof(float) * Q40_FEW_MAX_SLICES * (NT * 256 + 128) == q40_few_lds(NT), "the plan reports the instance's static LDS");
    if (epi == EPI_RESID) hipLaunchKernelGGL((k_q40_few<NT, EPI_RESID>), dim3(p.grid), dim3(p.threads), 0, st, a);
    else                  hipLaunchKernelGGL((k_q40_few<NT, EPI_STORE>), dim3(p.grid), dim3(p.threads), 0, st, a);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_q40_few(const QMat &w, int epi, const uint32_t *qa_A, const float *qa_d, int N,
                          float *y, long y_stride, const float *resid, long resid_stride, hipStream_t st) {
    const Q40FewPlan p = q40_few_plan(w.M, w.K, N);
    if (!p.ok || !w.tiles || !qa_A || !qa_d || !y || (epi != EPI_STORE && epi != EPI_RESID) || (epi == EPI_RESID && !resid)) return hipErrorInvalidValue;
    const Q40FewArgs a = { w.tiles, w.ngroups, w.nchunks, w.M, w.gmapF8, (const uint8_t *) qa_A, qa_d, N, y, y_stride, resid, resid_stride };
    hipError_t e;
    switch (p.nt) {
    case 1:  e = go_q40_few<1>(p, epi, a, st); break;
    case 2:  e = go_q40_few<2>(p, epi, a, st); break;
    case 3:  e = go_q40_few<3>(p, epi, a, st); break;
    default: e = go_q40_few<4>(p, epi, a, st); break;
    }
    if (e == hipSuccess) g_q40_few_launches++;
    return e;
}

}  // namespace lh
