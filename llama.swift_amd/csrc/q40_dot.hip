// q40_dot.hip -- k_q40_dot: the OPT-IN K-split integer-dot mat-vec of Q4_0 model files (llamahip_opts.fast_decode = 1,
// llamahip_op_gemv_q4_0_dot): wo and w2 of the single-token decode step, y = W x + resid and the {sum y, sum y^2} pair of
// the workgroup's rows for the next launch's PREP_NORMP prologue.  NOT the reference's arithmetic: the exact k_gemv keeps one wave per
// row-group on these 4096-row matrices because the reference's eight fp32 chains per block forbid a split of K; that wave's 22 VALU
// instructions per chunk are the launch's floor whatever memory does.
//
// The stated arithmetic (the contract; tests/test_gpu_q40_dot_op.py holds the kernel to it, bit for bit) is k_q40_few's at one row.  q = the
// weight block's codes - 8, d_w its scale; c, d_a the codes - 8 and the scale of quantize_row_q4_0 on the activation block (the existing
// qa_A / qa_d row, bit for bit):
//   isum  = sum over the block's 32 elements of q c                    an exact integer (|isum| <= 2048)
//   acc   = fma((float) isum, fl(d_w * d_a), acc)                      two roundings per block
//   K-slice s of S adds the blocks of chunks (256 elements) s, s + S, s + 2 S, ... in ascending order, starting from +0
//   y     = ((slice 0 + slice 1) + slice 2) + ... + slice S - 1  (+ resid, added last)
// S = q40_dot_slices(M): 8 up to 8192 weight rows, 4 above -- (M, K) alone decide every order.  No atomics; each output is owned by one
// workgroup.  Blocks of the zero padding behind K (both operands pad a row to whole chunks with value 0 and scale 0) add fma(0, 0, acc).
// The pair: over the workgroup's 16 stored outputs in double, absent rows as 0, as the pairwise tree wave_sum_d runs (k_gemv's EPI_RESID
// form): ((y0 + y1) + (y2 + y3)) + ((y4 + y5) + (y6 + y7)), the same of rows 8 .. 15, the two halves added; y^2 likewise.
//
// Work split.  A workgroup owns 16 weight rows = two row-groups of the load-time chain-major tile copy (QMat::tiles, no other copy is
// read); its S waves are the K-slices.  Lane (i = lane / 4, g = lane % 4) streams the 32 bytes of chains 2 g, 2 g + 1 of weight row i of a
// chunk -- the K-group g of all eight blocks -- straight from HBM: two non-temporal 16-byte loads and the 8 bytes of two block scales, PF
// chunks ahead in a register ring.  A wave's loads of a chunk are two contiguous KiB; every byte of the tiles is read once by one lane.
// (The four g-lanes of a row are a DPP quad, so that their integer partials meet in two v_add_u32_dpp and a scale is a quad broadcast.)
//   * No unpacking: a tile dword holds the signed 4-bit codes of one block pair, even block in the low nibbles; the activation dword of
//     block j holds its codes in the low (even j) or high (odd j) nibbles and zeros in the others, so v_dot8_i32_i4 of the two IS the
//     block's partial sum of q c over the dword's four elements.  16 dots per lane and chunk.
//   * The activation row (codes and scales, 288 bytes per chunk) is staged in LDS once per workgroup, behind the ring's first loads.
//   * Lane g = 0 of a quad starts its dot chain on the bit pattern of 1.5 * 2^23, the others on 0: the quad's integer sum is then the
//     float 12582912 + isum, and (float) isum is one exact subtraction (k_gemv's LH_STEP trick) instead of a conversion.
//   * The block's weight scale sits in lane j % 4 of the quad (the tile stores a row's scales as s0 s4 s1 s5 ...): one DPP broadcast
//     into the product fl(d_w * d_a).  Every lane of the quad runs the row's FMA chain; lane g = 0 parks it.
// The slices meet in LDS ([slice][row] fp32) behind one barrier; wave 0 adds them in slice order, adds the residual (loaded at entry),
// stores y and reduces the pair.
//   grid ceil(M / 16), 64 S threads, dynamic LDS 288 nchunks + 512 bytes (q40_dot_plan, q40_dot_plan.cpp)
#include "kcommon.hip.h"
#include "q40_dot_plan.h"

namespace lh {

struct Q40DotArgs {
    const uint8_t *wt; int ngroups, nchunks, M;
    const uint8_t *qa_A; const float *qa_d;         // the operand row: nchunks * 256 bytes / nchunks * 8 floats
    float *y; const float *resid; f64x2 *part_out;  // part_out: one pair per workgroup, or null
    unsigned long long *count;                      // a handle's launch counter (the first thread of the grid adds one), or null
};

constexpr int Q40_DOT_PF = 4;                       // chunks of weights in flight per wave

template <int Q>
__device__ __forceinline__ int quad_xor_add(int v) {            // v + the value of lane ^ Q of the quad (Q = 1, 2): v_add_u32_dpp
    return v + __builtin_amdgcn_mov_dpp(v, Q == 1 ? DPP_QUAD_XOR1 : DPP_QUAD_XOR2, 0xF, 0xF, true);
}

// block J of a chunk: the quad's exact integer sum of q c as the float 12582912 + isum, the scale product, the FMA (see the header)
template <int J>
__device__ __forceinline__ float q40_dot_block(float acc, const u32x4 &w0, const u32x4 &w1, const u32x4 (&a0)[2], const u32x4 (&a1)[2],
                                               const f32x2 &sw, const f32x4 (&da)[2], int init) {
    int p = __builtin_amdgcn_sdot8((int) w0[J >> 1], (int) a0[J >> 2][J & 3], init, false);
    p = __builtin_amdgcn_sdot8((int) w1[J >> 1], (int) a1[J >> 2][J & 3], p, false);
    p = quad_xor_add<1>(p);
    p = quad_xor_add<2>(p);
    const float sc = quad_bcast<(J & 3)>(J < 4 ? sw.x : sw.y) * da[J >> 2][J & 3];
    return __builtin_fmaf(__builtin_bit_cast(float, p) - 12582912.0f, sc, acc);
}

template <int EPI>
__global__ void __launch_bounds__(64 * Q40_DOT_MAX_SLICES)
k_q40_dot(const Q40DotArgs a) {
    constexpr int PF = Q40_DOT_PF;
    extern __shared__ __attribute__((aligned(16))) uint8_t q40_dot_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nt = blockDim.x, S = nt >> 6;
    const int i = lane >> 2, g = lane & 3;
    const int nchunks = a.nchunks;
    uint8_t *sA = q40_dot_smem;                                             // [nchunks][256]: the row's codes, as qa_A holds them
    float *sD = (float *) (q40_dot_smem + (size_t) nchunks * 256);          // [nchunks][8]: the row's block scales
    float *red = sD + (size_t) nchunks * 8;                                 // [S][16]: the slices' partial outputs
    const int g0 = blockIdx.x * 2;
    // the lane's weight row: row i & 7 of tile group g0 + (i >> 3) (a last workgroup of one group reads it twice and stores it once)
    const uint8_t *wp = a.wt + (size_t) min(g0 + (i >> 3), a.ngroups - 1) * (nchunks + 1) * TILE_BYTES;
    const uint32_t woff = (uint32_t) (((i & 7) * 8 + 2 * g) * 16), soff = (uint32_t) (1024 + (i & 7) * 32 + g * 8);
    const int nmine = wave < nchunks ? (nchunks - wave + S - 1) / S : 0;      // chunks wave, wave + S, ...

    u32x4 wq[PF][2];
    f32x2 ws[PF];
#define LH_DOT_LOADW(SLOT, CH) do {                                                                         \
        const uint8_t *tp_ = wp + (size_t) min((CH), nchunks) * TILE_BYTES;      /* past the row: the zero tile */ \
        wq[SLOT][0] = __builtin_nontemporal_load((const u32x4 *) (tp_ + woff));                              \
        wq[SLOT][1] = __builtin_nontemporal_load((const u32x4 *) (tp_ + woff + 16));                         \
        ws[SLOT] = __builtin_nontemporal_load((const f32x2 *) (tp_ + soff));                                 \
    } while (0)
#pragma unroll
    for (int u = 0; u < PF; u++) LH_DOT_LOADW(u, wave + u * S);
    if (a.count && blockIdx.x == 0 && tid == 0) *a.count += 1ull;      // (launches of a handle are stream-ordered: one writer at a time)

    // the output this thread stores at the end (wave 0, lanes 0 .. 15: row `lane` of the workgroup) and its residual, asked for now
    const int om = (g0 + ((lane & 15) >> 3)) * 8 + (lane & 7);
    const bool olive = wave == 0 && lane < 16 && g0 + (lane >> 3) < a.ngroups && om < a.M;
    float r = 0.0f;
    if (EPI == EPI_RESID && olive) r = a.resid[om];

    // the activation row -> LDS, two 16-byte granules per thread in flight
    {
        const u32x4 *s4 = (const u32x4 *) a.qa_A;
        u32x4 *d4 = (u32x4 *) sA;
        const int nA = nchunks * 16;
        for (int base = tid; base < nA; base += 2 * nt) {
            const u32x4 v0 = s4[base], v1 = s4[min(base + nt, nA - 1)];
            d4[base] = v0;
            if (base + nt < nA) d4[base + nt] = v1;
        }
        const u32x4 *sd4 = (const u32x4 *) a.qa_d;
        u32x4 *dd4 = (u32x4 *) sD;
        for (int k = tid; k < nchunks * 2; k += nt) dd4[k] = sd4[k];
    }
    __syncthreads();

    const int init = g == 0 ? 0x4B400000 : 0;
    float acc = 0.0f;
    for (int k0 = 0; k0 < nmine; k0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; u++) {
            if (k0 + u < nmine) {
                const int ch = wave + (k0 + u) * S;
                const u32x4 *ap = (const u32x4 *) (sA + (size_t) ch * 256 + g * 64);
                const u32x4 a0[2] = { ap[0], ap[1] }, a1[2] = { ap[2], ap[3] };      // chains 2 g, 2 g + 1: blocks 0 .. 7 each
                const f32x4 *dp = (const f32x4 *) (sD + (size_t) ch * 8);
                const f32x4 da[2] = { dp[0], dp[1] };
                const u32x4 w0 = wq[u][0], w1 = wq[u][1];
                const f32x2 sw = ws[u];
                LH_DOT_LOADW(u, ch + PF * S);          // the ring slot is free again
                acc = q40_dot_block<0>(acc, w0, w1, a0, a1, sw, da, init);
                acc = q40_dot_block<1>(acc, w0, w1, a0, a1, sw, da, init);
                acc = q40_dot_block<2>(acc, w0, w1, a0, a1, sw, da, init);
                acc = q40_dot_block<3>(acc, w0, w1, a0, a1, sw, da, init);
                acc = q40_dot_block<4>(acc, w0, w1, a0, a1, sw, da, init);
                acc = q40_dot_block<5>(acc, w0, w1, a0, a1, sw, da, init);
                acc = q40_dot_block<6>(acc, w0, w1, a0, a1, sw, da, init);
                acc = q40_dot_block<7>(acc, w0, w1, a0, a1, sw, da, init);
            }
        }
    }
#undef LH_DOT_LOADW

    // the slices meet: [slice][row], then wave 0 adds output `lane`'s partials in slice order
    if (g == 0) red[wave * 16 + i] = acc;
    __syncthreads();
    if (wave == 0) {
        float s = red[lane & 15];
        for (int w = 1; w < S; w++) s = s + red[w * 16 + (lane & 15)];
        if (EPI == EPI_RESID) s = s + r;
        if (olive) a.y[om] = s;
        if (a.part_out) {
            // the workgroup's share of the next norm's statistics, as k_gemv's EPI_RESID leaves it: sum y and sum y^2 in double
            const double yd = olive ? (double) s : 0.0;
            const double s1 = wave_sum_d(yd), s2 = wave_sum_d(yd * yd);
            if (lane == 0) a.part_out[blockIdx.x] = f64x2{ s1, s2 };
        }
    }
}

hipError_t launch_q40_dot(const QMat &w, int epi, const uint32_t *qa_A, const float *qa_d, float *y, const float *resid, double *part_out, int part_cap, unsigned long long *count, hipStream_t st) {
    const Q40DotPlan p = q40_dot_plan(w.M, w.K);
    if (!p.ok || !w.tiles || w.gmapF8 || !qa_A || !qa_d || !y || (epi != EPI_STORE && epi != EPI_RESID) || (epi == EPI_RESID && !resid)) return hipErrorInvalidValue;
    if (part_out && p.grid > part_cap) return hipErrorInvalidValue;          // one pair per workgroup: the buffer must hold the grid
    static_assert(Q40_DOT_MAX_PARTS == NORM_PART_MAX, "the plan's `applies` bounds the grid by what a PREP_NORMP prologue folds");
    const Q40DotArgs a = { w.tiles, w.ngroups, w.nchunks, w.M, (const uint8_t *) qa_A, qa_d, y, resid, (f64x2 *) part_out, count };
    if (epi == EPI_RESID) hipLaunchKernelGGL(k_q40_dot<EPI_RESID>, dim3(p.grid), dim3(p.threads), p.lds, st, a);
    else                  hipLaunchKernelGGL(k_q40_dot<EPI_STORE>, dim3(p.grid), dim3(p.threads), p.lds, st, a);
    LH_LAUNCH_CHECK();
    g_q40_dot_launches++;
    return hipSuccess;
}

}  // namespace lh
