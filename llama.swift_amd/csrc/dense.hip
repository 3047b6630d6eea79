// dense.hip -- the other model file types: f16 / f32 (f16 = 1 / 0) and Q4_1 (f16 = 3; N2).
//
// Only the weight mat-muls and the embedding gather differ from a Q4_0 model; norm, RoPE, KV cache and
// attention are the same kernels (kernels.hip).  Reference semantics (x86 AVX2+F16C build):
//   f16 weights  ggml_compute_forward_mul_mat_f16_f32 (ggml.c:5681-5985): the activations are rounded to
//                fp16 (_cvtss_sh, RNE) once per mat-mul, then every output is ggml_vec_dot_f16
//                (ggml.c:1260-1297): 4 x 8 = 32 fp32 FMA chains over the widened halves (chain l =
//                elements l, l+32, ...), folded by GGML_F32x8_REDUCE (ggml.c:872-887).
//   f32 weights  ggml_compute_forward_mul_mat_f32 (ggml.c:5430-5680), ggml_vec_dot_f32 (:1223-1258): the
//                same 32 chains without any rounding of the inputs.
//   embedding    ggml_compute_forward_get_rows_f16 / _f32 (ggml.c:6787-6850): widen / copy.
// One half-wave (32 lanes = the 32 chains) owns RG weight rows x NC activation rows; the fold is the
// xor butterfly 8, 16, 4, 1, 2 (the reference's tree; float add commutes).  Weights and activations are kept
// in a chain-major order (perm_index) so that a lane's loads are 16 / 32 bytes wide.
// Four mat-mul kernels share that arithmetic: k_dense_mv (one row, software-pipelined), k_dense_set (2 .. 16 rows -- a set step's rows, the
// 9-token prompt evals -- the weights streamed once, the rows shared through LDS), k_dense_mm (any row count, 8 rows per pass over the
// weights) and k_dense_mfma (more than 16 rows: the chains on the fp32 matrix cores, 64 rows per pass); launch_dense_mm picks (DESIGN.md
// 12.16, 12.18).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <algorithm>

#include "llamahip_internal.h"

namespace lh {

namespace {

__device__ __forceinline__ uint16_t f2h_rne(float f) { return __builtin_bit_cast(uint16_t, (_Float16) f); }      // v_cvt_f16_f32: RNE
__device__ __forceinline__ float h2f(uint16_t h) { return (float) __builtin_bit_cast(_Float16, h); }

template <int WT> struct WElem;
template <> struct WElem<0> { typedef float T; static __device__ __forceinline__ float widen(float v) { return v; } static __device__ __forceinline__ float act(float x) { return x; } };
template <> struct WElem<1> { typedef uint16_t T; static __device__ __forceinline__ float widen(uint16_t v) { return h2f(v); } static __device__ __forceinline__ float act(float x) { return h2f(f2h_rne(x)); } };

// a lane's 8 consecutive operands of one group, kept as loaded (16 / 32 bytes) and widened at use: unpacked
// fp16 values would take one VGPR each (k_dense_mv: 170 VGPRs instead of 110)
typedef uint32_t du4 __attribute__((ext_vector_type(4)));
typedef float df4 __attribute__((ext_vector_type(4)));
template <int WT> struct WVec8;
// fp16 operands stay packed (two per VGPR) and are widened INSIDE the FMA: v_fma_mix_f32 reads its first
// source as the low / high half of a register (op_sel) and multiplies-adds in fp32 with one rounding --
// exactly fma((float) h, x, acc).  hipcc emits v_cvt_f32_f16 + v_fma_f32 for the C++ form and unpacks a
// whole batch first (246 VGPRs, or spills under a register cap), hence inline assembly.
template <> struct WVec8<1> {
    du4 v;
    __device__ __forceinline__ void load(const uint16_t *p) { v = __builtin_nontemporal_load((const du4 *) p); }
    __device__ __forceinline__ void fma_into(float &acc, int u, float x) const {
        const uint32_t word = u < 2 ? v.x : u < 4 ? v.y : u < 6 ? v.z : v.w;
        if (u & 1) asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(word), "v"(x));
        else       asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(word), "v"(x));
    }
};
template <> struct WVec8<0> {
    df4 a, b;
    __device__ __forceinline__ void load(const float *p) { a = __builtin_nontemporal_load((const df4 *) p); b = __builtin_nontemporal_load((const df4 *) p + 1); }
    __device__ __forceinline__ void fma_into(float &acc, int u, float x) const {
        const float wv = u == 0 ? a.x : u == 1 ? a.y : u == 2 ? a.z : u == 3 ? a.w : u == 4 ? b.x : u == 5 ? b.y : u == 6 ? b.z : b.w;
        acc = fmaf(wv, x, acc);
    }
};

constexpr int RG = 4;      // weight rows per half-wave

// Chain-major order inside groups of 256 elements (8 steps of the 32 chains): element g*256 + 32*s + l is stored
// at g*256 + l*st + s (st = steps in the group: 8, fewer in a tail group), so that lane l -- chain l -- finds
// its next 8 operands in ONE 16-byte (fp16) or 32-byte (fp32) load and a half-wave reads 512 / 1024 contiguous
// bytes.  The first version read 2 bytes per lane and step and reached 1.3 TB/s.
__device__ __forceinline__ long perm_index(long e, int K) {
    const long g = e >> 8;
    const int within = (int) (e & 255), l = within & 31, sidx = within >> 5;
    const int gs = (int) min((long) 256, (long) K - g * 256), st = gs >> 5;
    return g * 256 + (long) l * st + sidx;
}

// weights: raw rows -> permuted rows (load time)
template <int WT>
__global__ void k_dense_perm_rows(const void *__restrict__ src, void *__restrict__ dst, long M, int K) {
    typedef typename WElem<WT>::T T;
    const long gid = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= M * K) return;
    const long m = gid / K, e = gid % K;
    ((T *) dst)[m * K + perm_index(e, K)] = ((const T *) src)[gid];
}

// activations: round through fp16 where the weights are fp16 (ggml.c:5681-5985 INIT phase) and permute
template <int WT>
__global__ void k_dense_perm_act(const float *__restrict__ x, long x_stride, int K, float *__restrict__ xp) {
    const int n = blockIdx.x;
    for (int e = threadIdx.x; e < K; e += blockDim.x) xp[(size_t) n * K + perm_index(e, K)] = WElem<WT>::act(x[(size_t) n * x_stride + e]);
}

// Activation preparation fused with the rounding / permutation above (one launch instead of k_prep_qa with an
// fp32 side output + k_dense_perm_act: 16 instead of 61 us per layer at 7B shapes).  One thread per 16
// contiguous elements; NORM keeps a row in one workgroup (two block-wide double sums), the other modes are
// sliced over gridDim.y.  Arithmetic = make_y in kernels.hip:
//   MODE 1 plain    y = in0
//   MODE 2 norm     y = w * ((float)(x - mean) * scale)      ggml_norm + ggml_mul (ggml.c:5327-5385, :4555)
//   MODE 3 SiLU*up  y = silu_lut(in0) * in1                  (ggml.c:1956-1963, .mm:678-680)
__device__ __forceinline__ double dense_block_sum(double v, double *red) {
    for (int msk = 32; msk > 0; msk >>= 1) {
        int lo = __double2loint(v), hi = __double2hiint(v);
        lo = __shfl_xor(lo, msk); hi = __shfl_xor(hi, msk);
        v += __hiloint2double(hi, lo);
    }
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();                                       // (red may still be read by the previous call)
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nw; i++) s += red[i];
    return s;
}
template <int MODE, int WT>
__global__ void __launch_bounds__(1024)
k_dense_prep(const float *__restrict__ in0, const float *__restrict__ in1, long in_stride, long in1_stride, int K,
             float *__restrict__ xp, const uint16_t *__restrict__ T_silu) {
    __shared__ double red[16];
    const int n = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int nh = K >> 4;
    const int hi = blockIdx.y * nt + tid;
    const bool live = hi < nh;
    const int hc = min(hi, nh - 1);
    const df4 *a4 = (const df4 *) (in0 + (size_t) n * in_stride) + hc * 4;
    df4 xa[4], xb[4];
#pragma unroll
    for (int v = 0; v < 4; v++) xa[v] = a4[v];
    if (MODE == PREP_NORM) {
#pragma unroll
        for (int v = 0; v < 4; v++) xb[v] = ((const df4 *) in1)[hc * 4 + v];
    } else if (MODE == PREP_SILU_MUL) {
        const df4 *b4 = (const df4 *) (in1 + (size_t) n * in1_stride) + hc * 4;
#pragma unroll
        for (int v = 0; v < 4; v++) xb[v] = b4[v];
    }
    if (MODE == PREP_NORM) {
        double s1 = 0.0;
        if (live) {
#pragma unroll
            for (int v = 0; v < 4; v++) { s1 += (double) xa[v].x; s1 += (double) xa[v].y; s1 += (double) xa[v].z; s1 += (double) xa[v].w; }
        }
        const double mean = dense_block_sum(s1, red) / (double) K;
        double s2 = 0.0;
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const double v0 = (double) xa[v].x - mean, v1 = (double) xa[v].y - mean;
            const double v2 = (double) xa[v].z - mean, v3 = (double) xa[v].w - mean;
            xa[v].x = (float) v0; xa[v].y = (float) v1; xa[v].z = (float) v2; xa[v].w = (float) v3;
            if (live) { s2 += v0 * v0; s2 += v1 * v1; s2 += v2 * v2; s2 += v3 * v3; }
        }
        const double sum2 = dense_block_sum(s2, red);
        const float scale = (float) (1.0 / sqrt(sum2 / (double) K + (double) 1e-5f));
#pragma unroll
        for (int v = 0; v < 4; v++) {
            xa[v].x = xb[v].x * (xa[v].x * scale); xa[v].y = xb[v].y * (xa[v].y * scale);
            xa[v].z = xb[v].z * (xa[v].z * scale); xa[v].w = xb[v].w * (xa[v].w * scale);
        }
    } else if (MODE == PREP_SILU_MUL) {
#pragma unroll
        for (int v = 0; v < 4; v++) {
            xa[v].x = h2f(T_silu[f2h_rne(xa[v].x)]) * xb[v].x; xa[v].y = h2f(T_silu[f2h_rne(xa[v].y)]) * xb[v].y;
            xa[v].z = h2f(T_silu[f2h_rne(xa[v].z)]) * xb[v].z; xa[v].w = h2f(T_silu[f2h_rne(xa[v].w)]) * xb[v].w;
        }
    }
    if (!live) return;
    // The fp32 products above must exist as fp32 values before they are rounded to fp16: left alone, hipcc
    // folds `(_Float16) (a * b)` into v_fma_mixlo_f16 -- ONE rounding of the exact product -- while the
    // reference rounds the product to fp32 (ggml_mul) and that to fp16 (the mat-mul's INIT phase).  Rare
    // (a few elements per thousand rows), and enough to flip logits in the 4th digit.  tests/test_gpu_dense_prep_op.py holds this fence
    // in place: its f16_double_rounding rows are made of such products (64 and more per row), so the kernel without it fails them.
#pragma unroll
    for (int v = 0; v < 4; v++) asm volatile("" : "+v"(xa[v].x), "+v"(xa[v].y), "+v"(xa[v].z), "+v"(xa[v].w));
    // element e = hi*16 + i  ->  g*256 + l*st + sidx  (perm_index): the 16 elements share g and sidx
    const long e0 = (long) hi * 16;
    const long g = e0 >> 8;
    const int within = (int) (e0 & 255), l0 = within & 31, sidx = within >> 5;
    const int gs = (int) min((long) 256, (long) K - g * 256), stp = gs >> 5;
    float *o = xp + (size_t) n * K + g * 256 + sidx;
#pragma unroll
    for (int v = 0; v < 4; v++) {
        o[(size_t) (l0 + 4 * v + 0) * stp] = WElem<WT>::act(xa[v].x);
        o[(size_t) (l0 + 4 * v + 1) * stp] = WElem<WT>::act(xa[v].y);
        o[(size_t) (l0 + 4 * v + 2) * stp] = WElem<WT>::act(xa[v].z);
        o[(size_t) (l0 + 4 * v + 3) * stp] = WElem<WT>::act(xa[v].w);
    }
}

// y[n][m] (+ resid[n][m]) = dot(W[m][:], xp[n][:]) on permuted operands.  grid (ceil(M / (8 * RG)), ceil(N / NC)), 256 threads.
template <int WT, int NC, int EPI>
__global__ void __launch_bounds__(256)
k_dense_mm(const void *__restrict__ wv, int M, int K, const float *__restrict__ xp, int N,
           float *__restrict__ y, long y_stride, const float *__restrict__ resid, long resid_stride) {
    typedef typename WElem<WT>::T T;
    const T *w = (const T *) wv;
    const int l = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const int m0 = (blockIdx.x * 8 + hw) * RG, n0 = blockIdx.y * NC;
    const T *wr[RG];
#pragma unroll
    for (int r = 0; r < RG; r++) wr[r] = w + (size_t) min(m0 + r, M - 1) * K;
    const float *xr[NC];
#pragma unroll
    for (int n = 0; n < NC; n++) xr[n] = xp + (size_t) min(n0 + n, N - 1) * K;
    float acc[RG][NC];
#pragma unroll
    for (int r = 0; r < RG; r++)
#pragma unroll
        for (int n = 0; n < NC; n++) acc[r][n] = 0.0f;
    const int ng = K >> 8;
    // full groups: 8 steps per lane and group.  A decode launch is a few hundred waves each streaming its rows
    // once, so the bytes in flight per lane decide the rate: UG groups (UG x RG vector loads) are issued before
    // the first is consumed.  Groups past the end are clamped re-reads that are not accumulated.
    constexpr int UG = NC == 1 ? 4 : 1;
    for (int g0 = 0; g0 < ng; g0 += UG) {
        T wq[UG][RG][8];
        float xq[UG][NC][8];
#pragma unroll
        for (int v = 0; v < UG; v++) {
            const size_t at = (size_t) min(g0 + v, ng - 1) * 256 + l * 8;
#pragma unroll
            for (int r = 0; r < RG; r++)
#pragma unroll
                for (int u = 0; u < 8; u++) wq[v][r][u] = wr[r][at + u];
#pragma unroll
            for (int n = 0; n < NC; n++)
#pragma unroll
                for (int u = 0; u < 8; u++) xq[v][n][u] = xr[n][at + u];
        }
#pragma unroll
        for (int v = 0; v < UG; v++) {
            if (g0 + v < ng) {
#pragma unroll
                for (int u = 0; u < 8; u++)
#pragma unroll
                    for (int n = 0; n < NC; n++)
#pragma unroll
                        for (int r = 0; r < RG; r++) acc[r][n] = fmaf(WElem<WT>::widen(wq[v][r][u]), xq[v][n][u], acc[r][n]);
            }
        }
    }
    const int st = (K & 255) >> 5;                         // tail group: st < 8 steps
    for (int u = 0; u < st; u++) {
        const size_t at = (size_t) ng * 256 + l * st + u;
#pragma unroll
        for (int n = 0; n < NC; n++) {
            const float xa = xr[n][at];
#pragma unroll
            for (int r = 0; r < RG; r++) acc[r][n] = fmaf(WElem<WT>::widen(wr[r][at]), xa, acc[r][n]);
        }
    }
#pragma unroll
    for (int r = 0; r < RG; r++)
#pragma unroll
        for (int n = 0; n < NC; n++) {
            float s = acc[r][n];
            s += __shfl_xor(s, 8);
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 4);
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            if (l == 0 && m0 + r < M && n0 + n < N) {
                if (EPI == EPI_RESID) s = s + resid[(size_t) (n0 + n) * resid_stride + m0 + r];
                y[(size_t) (n0 + n) * y_stride + m0 + r] = s;
            }
        }
}

// Decode (one activation row): the same 32 chains per row, software-pipelined.  k_dense_mm issues a batch
// of loads, waits for all of it, consumes it, and only then issues the next: the memory pipe idles half
// the time (2.5 TB/s).  Here two register buffers of UG groups alternate -- the loads of batch b + 1 are in
// flight while batch b is consumed -- in a straight-line loop body (no branch around a load, so the
// compiler's vmcnt waits stay counted; the prefetch past the end is a clamped re-read that is never
// consumed); groups that do not fill a double batch and the tail group run un-pipelined afterwards.
//   grid ceil(M / (HW * RG)), block HW * 32 threads (HW half-waves of RG rows each)
template <int WT, int EPI>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))   // <= 128 VGPRs: keeps the operands packed until use
k_dense_mv(const void *__restrict__ wv, int M, int K, const float *__restrict__ xp,
           float *__restrict__ y, const float *__restrict__ resid) {
    typedef typename WElem<WT>::T T;
    const T *w = (const T *) wv;
    const int l = threadIdx.x & 31, hw = threadIdx.x >> 5, nhw = blockDim.x >> 5;
    const int m0 = (blockIdx.x * nhw + hw) * RG;
    const T *wr[RG];
#pragma unroll
    for (int r = 0; r < RG; r++) wr[r] = w + (size_t) min(m0 + r, M - 1) * K;
    float acc[RG];
#pragma unroll
    for (int r = 0; r < RG; r++) acc[r] = 0.0f;
    const int ng = K >> 8;
    constexpr int UG = WT == 1 ? 2 : 1;                    // groups per buffer (fp32 weights are twice the registers)
    WVec8<WT> wq[2][UG][RG];
    df4 xq[2][UG][2];
#define LD_LOADB(B, G0)                                                                            \
    _Pragma("unroll")                                                                              \
    for (int v = 0; v < UG; v++) {                                                                 \
        const size_t at = (size_t) min((G0) + v, ng - 1) * 256 + l * 8;                            \
        _Pragma("unroll")                                                                          \
        for (int r = 0; r < RG; r++) wq[B][v][r].load(wr[r] + at);                                 \
        xq[B][v][0] = *(const df4 *) (xp + at); xq[B][v][1] = *(const df4 *) (xp + at + 4);        \
    }
#define LD_CONSUMEB(B)                                                                             \
    _Pragma("unroll")                                                                              \
    for (int v = 0; v < UG; v++)                                                                   \
        _Pragma("unroll")                                                                          \
        for (int u = 0; u < 8; u++)                                                                \
            _Pragma("unroll")                                                                      \
            for (int r = 0; r < RG; r++) wq[B][v][r].fma_into(acc[r], u, xq[B][v][u >> 2][u & 3]);
    const int ngm = ng / (2 * UG) * (2 * UG);              // groups covered by whole double batches
    if (ngm) {
        LD_LOADB(0, 0)
        for (int g0 = 0; g0 < ngm; g0 += 2 * UG) {
            LD_LOADB(1, g0 + UG)
            __builtin_amdgcn_sched_barrier(0);             // the next batch goes out BEFORE the wait for this one
            LD_CONSUMEB(0)
            __builtin_amdgcn_sched_barrier(0);
            LD_LOADB(0, g0 + 2 * UG)
            __builtin_amdgcn_sched_barrier(0);
            LD_CONSUMEB(1)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef LD_LOADB
#undef LD_CONSUMEB
    for (int g = ngm; g < ng; g++) {                       // leftover full groups
        const size_t at = (size_t) g * 256 + l * 8;
        T wl[RG][8];
        float xl[8];
#pragma unroll
        for (int r = 0; r < RG; r++)
#pragma unroll
            for (int u = 0; u < 8; u++) wl[r][u] = wr[r][at + u];
#pragma unroll
        for (int u = 0; u < 8; u++) xl[u] = xp[at + u];
#pragma unroll
        for (int u = 0; u < 8; u++)
#pragma unroll
            for (int r = 0; r < RG; r++) acc[r] = fmaf(WElem<WT>::widen(wl[r][u]), xl[u], acc[r]);
    }
    const int st = (K & 255) >> 5;                         // tail group: st < 8 steps
    for (int u = 0; u < st; u++) {
        const size_t at = (size_t) ng * 256 + l * st + u;
        const float xa = xp[at];
#pragma unroll
        for (int r = 0; r < RG; r++) acc[r] = fmaf(WElem<WT>::widen(wr[r][at]), xa, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RG; r++) {
        float s = acc[r];
        s += __shfl_xor(s, 8);
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 4);
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        if (l == 0 && m0 + r < M) {
            if (EPI == EPI_RESID) s = s + resid[m0 + r];
            y[m0 + r] = s;
        }
    }
}

// 2 .. 16 activation rows, the weights streamed ONCE: k_dense_mv's chains and its software-pipelined weight loads, with
// NR accumulators per weight row.  A half-wave owns RGS weight rows x NR activation rows (RGS = RG, or 2 for the narrow matrices: twice
// the waves on the same bytes, see dense_set_plan); the activation rows reach the 8
// half-waves of a workgroup through LDS in slabs of UG groups (256 elements) per row -- 16 fp32 rows of K = 11 008 do not
// fit -- staged global -> registers -> LDS one slab ahead, into the buffer the previous slab was read from a barrier ago
// (two buffers, one barrier per slab).  Per slab and half-iteration, in issue order:
//   activation loads of slab b + 1 (registers) | weight loads of batch b + 1 (the other register buffer) |
//   consume batch b against LDS buffer b & 1 | write slab b + 1 into LDS buffer (b + 1) & 1 | barrier
// so the weight loads of the next batch are in flight while this one is consumed, and the wait of the LDS write is for
// the older activation loads only.  No branch surrounds a load: groups past the end are clamped re-reads that are never
// consumed, rows past N are clamped re-reads of row N - 1 whose sums are never stored.  The LDS image of a group keeps a
// lane's operands 0 .. 3 at [l] and 4 .. 7 at [32 + l] (16 bytes each): both reads are conflict-free and the two
// half-waves of a wave read the same addresses (broadcast).  The tail group (K % 256) is un-pipelined, its few activation
// operands read from global memory as k_dense_mv reads them.  Launch plan: dense_set_plan.
// 7B matrices in an 8-layer f16 file's set step, us per launch against k_dense_mm<WT, 8> (profiles/dense_set_probe.json): 2 rows
// 19.0 / 9.5 / 38.8 / 20.7 / 55.1 against 48.0 / 29.9 / 61.4 / 68.2 / 95.5 (wq|wk|wv, wo, w1|w3, w2, lm head; k_dense_mv: 18.0 / 8.3 /
// 37.6 / 20.2 / 52.2), 16 rows 43.0 / 31.6 / 71.8 / 63.3 / 93.0 against 57.9 / 40.0 / 105.2 / 85.0 / 144.1; a step of 16 sequences
// 2.30 ms against 15.34 ms one sequence after the other.
//   grid ceil(M / (8 * RGS)), block 256 threads
template <int WT, int NR> struct DenseSetShape { static constexpr int UG = (WT == 1 && NR <= 4) ? 2 : 1; };
template <int WT, int NR, int RGS>
__global__ void __launch_bounds__(256)
k_dense_set(const void *__restrict__ wv, int M, int K, const float *__restrict__ xp, int N,
            float *__restrict__ y, long y_stride, const float *__restrict__ resid, long resid_stride) {
    typedef typename WElem<WT>::T T;
    constexpr int UG = DenseSetShape<WT, NR>::UG, HW = 8, NT = HW * 32;
    constexpr int SLAB4 = UG * NR * 64;                    // 16-byte granules of one slab
    constexpr int ST = (SLAB4 + NT - 1) / NT;              // ... staged per thread
    __shared__ df4 xs[2][SLAB4];
    const T *w = (const T *) wv;
    const int tid = threadIdx.x, l = tid & 31, hw = tid >> 5;
    const int m0 = (blockIdx.x * HW + hw) * RGS;
    const T *wr[RGS];
#pragma unroll
    for (int r = 0; r < RGS; r++) wr[r] = w + (size_t) min(m0 + r, M - 1) * K;
    float acc[RGS][NR];
#pragma unroll
    for (int r = 0; r < RGS; r++)
#pragma unroll
        for (int n = 0; n < NR; n++) acc[r][n] = 0.0f;
    const int ng = K >> 8;
    WVec8<WT> wq[2][UG][RGS];
    df4 xst[ST];
    // granule j of this thread: slab index i = tid + j * NT = (v * NR + n) * 64 + q -- group v of the slab, row n, granule q of the
    // group's 64 (elements 4 q .. 4 q + 3: operands 4 (q & 1) .. of lane q >> 1)
    const float *xsrc[ST];
    int xv[ST], xdst[ST];
#pragma unroll
    for (int j = 0; j < ST; j++) {
        const int i = min(tid + j * NT, SLAB4 - 1);
        const int q = i & 63, vn = i >> 6, v = vn / NR, n = vn - v * NR;
        xsrc[j] = xp + (size_t) min(n, N - 1) * K + q * 4;
        xv[j] = v;
        xdst[j] = vn * 64 + (q & 1) * 32 + (q >> 1);
    }
#define LD_LOADX(G0)                                                                               \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < ST; j++) xst[j] = *(const df4 *) (xsrc[j] + (size_t) min((G0) + xv[j], ng - 1) * 256);
#define LD_STOREX(LB)                                                                              \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < ST; j++) if (tid + j * NT < SLAB4) xs[LB][xdst[j]] = xst[j];
#define LD_LOADB(B, G0)                                                                            \
    _Pragma("unroll")                                                                              \
    for (int v = 0; v < UG; v++) {                                                                 \
        const size_t at = (size_t) min((G0) + v, ng - 1) * 256 + l * 8;                            \
        _Pragma("unroll")                                                                          \
        for (int r = 0; r < RGS; r++) wq[B][v][r].load(wr[r] + at);                                 \
    }
#define LD_CONSUMEB(B, LB, G0)                                                                     \
    _Pragma("unroll")                                                                              \
    for (int v = 0; v < UG; v++) {                                                                 \
        if ((G0) + v < ng) {                                                                       \
            _Pragma("unroll")                                                                      \
            for (int n = 0; n < NR; n++) {                                                         \
                const df4 xa = xs[LB][(v * NR + n) * 64 + l], xb = xs[LB][(v * NR + n) * 64 + 32 + l]; \
                _Pragma("unroll")                                                                  \
                for (int u = 0; u < 8; u++)                                                        \
                    _Pragma("unroll")                                                              \
                    for (int r = 0; r < RGS; r++) wq[B][v][r].fma_into(acc[r][n], u, u < 4 ? xa[u & 3] : xb[u & 3]); \
            }                                                                                      \
        }                                                                                          \
    }
    if (ng) {
        LD_LOADX(0)
        LD_LOADB(0, 0)
        LD_STOREX(0)
        __syncthreads();
        for (int g0 = 0; g0 < ng; g0 += 2 * UG) {
            LD_LOADX(g0 + UG)
            LD_LOADB(1, g0 + UG)
            __builtin_amdgcn_sched_barrier(0);             // the next batch goes out BEFORE the wait for this one
            LD_CONSUMEB(0, 0, g0)
            __builtin_amdgcn_sched_barrier(0);
            LD_STOREX(1)
            __syncthreads();
            LD_LOADX(g0 + 2 * UG)
            LD_LOADB(0, g0 + 2 * UG)
            __builtin_amdgcn_sched_barrier(0);
            LD_CONSUMEB(1, 1, g0 + UG)
            __builtin_amdgcn_sched_barrier(0);
            LD_STOREX(0)
            __syncthreads();
        }
    }
#undef LD_LOADX
#undef LD_STOREX
#undef LD_LOADB
#undef LD_CONSUMEB
    const int st = (K & 255) >> 5;                         // tail group: st < 8 steps
    for (int u = 0; u < st; u++) {
        const size_t at = (size_t) ng * 256 + l * st + u;
        float wt[RGS];
#pragma unroll
        for (int r = 0; r < RGS; r++) wt[r] = WElem<WT>::widen(wr[r][at]);
#pragma unroll
        for (int n = 0; n < NR; n++) {
            const float xa = xp[(size_t) min(n, N - 1) * K + at];
#pragma unroll
            for (int r = 0; r < RGS; r++) acc[r][n] = fmaf(wt[r], xa, acc[r][n]);
        }
    }
#pragma unroll
    for (int r = 0; r < RGS; r++)
#pragma unroll
        for (int n = 0; n < NR; n++) {
            float s = acc[r][n];
            s += __shfl_xor(s, 8);
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 4);
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            if (l == 0 && m0 + r < M && n < N) {
                if (resid) s = s + resid[(size_t) n * resid_stride + m0 + r];
                y[(size_t) n * y_stride + m0 + r] = s;
            }
        }
}

// More than 16 activation rows, on the fp32 matrix cores.  v_mfma_f32_16x16x4_f32 is bit for bit the k-ordered chain
// fma(a3, b3, fma(a2, b2, fma(a1, b1, fma(a0, b0, C)))) per output (prompt_attn.hip), so with A = four consecutive steps of chain c of 16
// activation rows and B = the same steps of 16 weight rows, ONE accumulator tile per chain advances exactly as acc = fmaf(w, x, acc) does in
// the kernels above: 32 tiles = 128 registers per wave, all 32 chains of an output in one lane (D register r of lane (j, q): activation
// row 4 q + r, weight row j), the fold 31 in-lane adds in the butterfly's tree, no cross-lane traffic.  Consecutive MFMAs go to different
// chains, so the instruction's dependent latency is covered by the wave itself.
// A workgroup is 4 waves, one per SIMD = 64 activation rows x 16 MT weight rows (wave: its 16 activation rows against MT tiles of 16 weight
// rows, the A operand read once for them; MT = 2: 256 accumulator registers of the wave's 512): a weight byte is fetched once per 64
// activation rows.  Operands reach the MFMA lanes through LDS, a group of 256 elements per row at a time, in the permuted order
// as it is in memory (chain c's 8 steps at c * 8), weights widened on the way in: lane (i, kk) reads dword row * 260 + c * 8 + 4 h + kk.  Rows
// are 260 dwords apart: 16 rows x 4 steps fall on 64 distinct banks (256 apart they would share four).  One LDS buffer (two of 96 rows do
// not fit 160 KB), the next group's global loads in flight in registers while this one is consumed; two barriers per group.  No branch
// surrounds a load: the prefetch past the last group, rows past N and weight rows past M are clamped re-reads that are never stored; a
// wave whose tile lies wholly outside skips the arithmetic, not the barriers.  K % 256 == 128 ends in a 4-step group (chain c's steps at
// c * 4: one MFMA per chain); other K are refused (dense_mfma_plan) -- a padded step would have to leave -0.0 sums alone.
//   grid (ceil(M / (16 MT)), ceil(N / 64)), block 256 threads, dynamic LDS (64 + 16 MT) * 260 * 4 bytes
typedef float f32x4m __attribute__((ext_vector_type(4)));
constexpr int MF_TN = 64, MF_LD = 260;
template <int WT> __device__ __forceinline__ void mf_store_widened(float *dst, const WVec8<WT> &q);
template <> __device__ __forceinline__ void mf_store_widened<1>(float *dst, const WVec8<1> &q) {
    const uint32_t u[4] = { q.v.x, q.v.y, q.v.z, q.v.w };
    *(df4 *) dst = df4{ h2f((uint16_t) u[0]), h2f((uint16_t) (u[0] >> 16)), h2f((uint16_t) u[1]), h2f((uint16_t) (u[1] >> 16)) };
    *(df4 *) (dst + 4) = df4{ h2f((uint16_t) u[2]), h2f((uint16_t) (u[2] >> 16)), h2f((uint16_t) u[3]), h2f((uint16_t) (u[3] >> 16)) };
}
template <> __device__ __forceinline__ void mf_store_widened<0>(float *dst, const WVec8<0> &q) {
    *(df4 *) dst = q.a;
    *(df4 *) (dst + 4) = q.b;
}
template <int WT, int EPI, int MT>
__global__ void __launch_bounds__(256)
k_dense_mfma(const void *__restrict__ wv, int M, int K, const float *__restrict__ xp, int N,
             float *__restrict__ y, long y_stride, const float *__restrict__ resid, long resid_stride) {
    typedef typename WElem<WT>::T T;
    constexpr int NT = 256, WROWS = 16 * MT;
    constexpr int XG = MF_TN * 64 / NT;                    // 16-byte granules of the activation rows' group staged per thread
    constexpr int WC = WROWS * 32 / NT;                    // 8-element chunks of the weight rows' group staged per thread
    extern __shared__ __attribute__((aligned(16))) float mf_lds[];
    float *xs = mf_lds, *ws = mf_lds + MF_TN * MF_LD;
    const T *w = (const T *) wv;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = wave;
    const int m0 = blockIdx.x * WROWS, n0 = blockIdx.y * MF_TN;
    const int ng = K >> 8;
    // granule j of this thread: row (tid >> 6) + j * (NT / 64), elements 4 (tid & 63) .. + 3 of the group
    uint32_t xoff[XG];
    int xdst[XG];
#pragma unroll
    for (int j = 0; j < XG; j++) {
        const int row = (tid >> 6) + j * (NT / 64), q = tid & 63;
        xoff[j] = (uint32_t) min(n0 + row, N - 1) * (uint32_t) K + q * 4;
        xdst[j] = row * MF_LD + q * 4;
    }
    const T *wsrc[WC];
    int wdst[WC];
#pragma unroll
    for (int j = 0; j < WC; j++) {
        const int row = (tid >> 5) + j * (NT / 32), c = tid & 31;
        wsrc[j] = w + (size_t) min(m0 + row, M - 1) * K + c * 8;
        wdst[j] = row * MF_LD + c * 8;
    }
    f32x4m acc[MT][32];
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
        for (int c = 0; c < 32; c++) acc[t][c] = f32x4m{ 0.0f, 0.0f, 0.0f, 0.0f };
    const bool live = n0 + nt * 16 < N;                    // wave-uniform
    const float *ap = xs + (nt * 16 + (lane & 15)) * MF_LD + (lane >> 4);
    const float *bp = ws + (lane & 15) * MF_LD + (lane >> 4);
    df4 xst[XG];
    WVec8<WT> wst[WC];
#define LD_LOADG(G)                                                                                \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < XG; j++) xst[j] = *(const df4 *) (xp + xoff[j] + (size_t) (G) * 256);      \
    _Pragma("unroll")                                                                              \
    for (int j = 0; j < WC; j++) wst[j].load(wsrc[j] + (size_t) (G) * 256);
    if (ng) {
        LD_LOADG(0)
        for (int g = 0; g < ng; g++) {
#pragma unroll
            for (int j = 0; j < XG; j++) *(df4 *) (xs + xdst[j]) = xst[j];
#pragma unroll
            for (int j = 0; j < WC; j++) mf_store_widened<WT>(ws + wdst[j], wst[j]);
            __syncthreads();
            LD_LOADG(min(g + 1, ng - 1))
            __builtin_amdgcn_sched_barrier(0);             // the next group goes out BEFORE this one is consumed
            if (live) {
                // eight batches of 8 chains (half h = batch >> 2), the next batch's LDS reads issued before this one's MFMAs: left to itself
                // the compiler requests a whole half first and spills
                float af[2][8], bf[2][MT][8];
#define LD_READB(B, Q)                                                                             \
    _Pragma("unroll")                                                                              \
    for (int i = 0; i < 8; i++) {                                                                  \
        const int o = (((Q) & 3) * 8 + i) * 8 + 4 * ((Q) >> 2);                                    \
        af[B][i] = ap[o];                                                                          \
        _Pragma("unroll")                                                                          \
        for (int t = 0; t < MT; t++) bf[B][t][i] = bp[t * 16 * MF_LD + o];                         \
    }
                LD_READB(0, 0)
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    if (q + 1 < 8) { LD_READB((q + 1) & 1, q + 1) }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < 8; i++)
#pragma unroll
                        for (int t = 0; t < MT; t++)
                            acc[t][(q & 3) * 8 + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[q & 1][i], bf[q & 1][t][i], acc[t][(q & 3) * 8 + i], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
#undef LD_READB
            }
            __syncthreads();
        }
    }
#undef LD_LOADG
    if (K & 255) {                                         // the 4-step tail group (K % 256 == 128), un-pipelined
        const size_t at = (size_t) ng * 256;
        for (int i = tid; i < MF_TN * 32; i += NT) {
            const int row = i >> 5, q = i & 31;
            *(df4 *) (xs + row * MF_LD + q * 4) = *(const df4 *) (xp + (size_t) min(n0 + row, N - 1) * K + at + q * 4);
        }
        for (int i = tid; i < WROWS * 32; i += NT) {
            const int row = i >> 5, c = i & 31;
            const T *p = w + (size_t) min(m0 + row, M - 1) * K + at + c * 4;
            *(df4 *) (ws + row * MF_LD + c * 4) = df4{ WElem<WT>::widen(p[0]), WElem<WT>::widen(p[1]), WElem<WT>::widen(p[2]), WElem<WT>::widen(p[3]) };
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int c = 0; c < 32; c++) {
                const float a = ap[c * 4];
#pragma unroll
                for (int t = 0; t < MT; t++) acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[t * 16 * MF_LD + c * 4], acc[t][c], 0, 0, 0);
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int m = m0 + t * 16 + (lane & 15);
        // k_dense_mm's butterfly as lane 0 sees it: partners ^8, ^16, ^4, ^1, ^2
        float a[32], b[8], c4[4];
#pragma unroll
        for (int i = 0; i < 8; i++) { a[i] = acc[t][i][r] + acc[t][i + 8][r]; a[16 + i] = acc[t][16 + i][r] + acc[t][24 + i][r]; }
#pragma unroll
        for (int i = 0; i < 8; i++) b[i] = a[i] + a[16 + i];
#pragma unroll
        for (int i = 0; i < 4; i++) c4[i] = b[i] + b[i + 4];
        const float d0 = c4[0] + c4[1], d2 = c4[2] + c4[3];
        float s = d0 + d2;
        const int n = n0 + nt * 16 + (lane >> 4) * 4 + r;
        if (n < N && m < M) {
            if (EPI == EPI_RESID) s = s + resid[(size_t) n * resid_stride + m];
            y[(size_t) n * y_stride + m] = s;
        }
    }
}

template <int WT>
__global__ void k_embed_dense(const int32_t *__restrict__ tokens, const void *__restrict__ emb, float *__restrict__ x, int d) {
    typedef typename WElem<WT>::T T;
    const int n = blockIdx.x;
    const T *row = (const T *) emb + (size_t) tokens[n] * d;
    for (int i = threadIdx.x; i < d; i += blockDim.x) x[(size_t) n * d + i] = WElem<WT>::widen(row[i]);
}

// a batched decode step's rows (SeqSet): row n = the token at *set->tok_in[n]; the step's first launch also gathers the rows'
// positions into the descriptor (SeqSet::pos), as k_embed_set does
template <int WT>
__global__ void k_embed_dense_set(SeqSet *set, const void *__restrict__ emb, float *__restrict__ x, int d) {
    typedef typename WElem<WT>::T T;
    const int n = blockIdx.x;
    if (threadIdx.x == 0) set->pos[n] = set->state[n][0];
    const T *row = (const T *) emb + (size_t) *set->tok_in[n] * d;
    for (int i = threadIdx.x; i < d; i += blockDim.x) x[(size_t) n * d + i] = WElem<WT>::widen(row[i]);
}

// k_rope_kv (prompt_attn.hip) for the rows of a set: row n is at position set->pos[n] of the cache at + set->kv_off[n]
__global__ void k_rope_kv_set(const float *__restrict__ qkv, long qkv_stride, int d, int dh, const double *__restrict__ sincos_tab,
                              float *__restrict__ qr, float *__restrict__ Kc, float *__restrict__ Vc, const SeqSet *__restrict__ set) {
    const int n = blockIdx.x;
    const int pos = set->pos[n];
    float *Kn = Kc + set->kv_off[n], *Vn = Vc + set->kv_off[n];
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

template <int WT, int NR>
hipError_t go_set(const DenseSetPlan &p, const DMat &w, int N, float *y, long y_stride, const float *resid, long resid_stride, hipStream_t st, float *scratch) {
    if (p.rg == RG) hipLaunchKernelGGL((k_dense_set<WT, NR, RG>), dim3(p.grid), dim3(256), 0, st, w.w, w.M, w.K, scratch, N, y, y_stride, resid, resid_stride);
    else            hipLaunchKernelGGL((k_dense_set<WT, NR, 2>), dim3(p.grid), dim3(256), 0, st, w.w, w.M, w.K, scratch, N, y, y_stride, resid, resid_stride);
    return hipGetLastError();
}
template <int WT>
hipError_t go_set_rows(const DenseSetPlan &p, const DMat &w, int N, float *y, long y_stride, const float *resid, long resid_stride, hipStream_t st, float *scratch) {
    switch (p.nr) {
    case 2:  return go_set<WT, 2>(p, w, N, y, y_stride, resid, resid_stride, st, scratch);
    case 4:  return go_set<WT, 4>(p, w, N, y, y_stride, resid, resid_stride, st, scratch);
    case 6:  return go_set<WT, 6>(p, w, N, y, y_stride, resid, resid_stride, st, scratch);
    case 8:  return go_set<WT, 8>(p, w, N, y, y_stride, resid, resid_stride, st, scratch);
    case 10: return go_set<WT, 10>(p, w, N, y, y_stride, resid, resid_stride, st, scratch);
    case 12: return go_set<WT, 12>(p, w, N, y, y_stride, resid, resid_stride, st, scratch);
    case 14: return go_set<WT, 14>(p, w, N, y, y_stride, resid, resid_stride, st, scratch);
    case 16: return go_set<WT, 16>(p, w, N, y, y_stride, resid, resid_stride, st, scratch);
    }
    return hipErrorInvalidValue;
}

template <int WT, int NC>
hipError_t go(const DMat &w, int epi, const float *x, long x_stride, int N, float *y, long y_stride,
              const float *resid, long resid_stride, hipStream_t st, float *scratch, int path) {
    if (x) {                                               // x == nullptr: scratch already holds the prepared rows
        const hipError_t e = launch_dense_perm_act(WT, x, x_stride, w.K, N, scratch, st);
        if (e != hipSuccess) return e;
    }
    if (path == DENSE_PATH_MV) {
        // small matrices: 4 half-waves per workgroup so that every CU gets one (a 4096-row matrix is 256 workgroups)
        const int nhw = (w.M + 8 * RG - 1) / (8 * RG) >= 512 ? 8 : 4;
        const dim3 g1((w.M + nhw * RG - 1) / (nhw * RG));
        for (int n = 0; n < N; n++) {                      // (more than one row: forced, llamahip_op_mul_mat_dense -- one launch per row)
            const float *xn = scratch + (size_t) n * w.K, *rn = resid ? resid + (size_t) n * resid_stride : nullptr;
            float *yn = y + (size_t) n * y_stride;
            if (epi == EPI_RESID)
                hipLaunchKernelGGL((k_dense_mv<WT, EPI_RESID>), g1, dim3(nhw * 32), 0, st, w.w, w.M, w.K, xn, yn, rn);
            else
                hipLaunchKernelGGL((k_dense_mv<WT, EPI_STORE>), g1, dim3(nhw * 32), 0, st, w.w, w.M, w.K, xn, yn, rn);
            g_dense_path_counts[DENSE_COUNT_MV]++;
        }
        return hipGetLastError();
    }
    if (path == DENSE_PATH_SET) {
        const DenseSetPlan p = dense_set_plan(w.M, w.K, WT, N);
        if (!p.nr || !dense_set_plan_has_kernel(p)) return hipErrorInvalidValue;
        g_dense_path_counts[DENSE_COUNT_SET]++;
        return go_set_rows<WT>(p, w, N, y, y_stride, epi == EPI_RESID ? resid : nullptr, resid_stride, st, scratch);
    }
    if (path == DENSE_PATH_MFMA) {
        const DenseMfmaPlan p = dense_mfma_plan(w.M, w.K, WT, N);
        if (!p.ok || !dense_mfma_plan_has_kernel(p)) return hipErrorInvalidValue;
        g_dense_mfma_launches++;
        const dim3 grid(p.grid_x, p.grid_y), block(p.threads);
#define LD_MFMA(E, MTV) hipLaunchKernelGGL((k_dense_mfma<WT, E, MTV>), grid, block, p.lds, st, w.w, w.M, w.K, scratch, N, y, y_stride, resid, resid_stride)
        if (p.tile_cols == 32) { if (epi == EPI_RESID) LD_MFMA(EPI_RESID, 2); else LD_MFMA(EPI_STORE, 2); }
        else                   { if (epi == EPI_RESID) LD_MFMA(EPI_RESID, 1); else LD_MFMA(EPI_STORE, 1); }
#undef LD_MFMA
        return hipGetLastError();
    }
    g_dense_path_counts[DENSE_COUNT_MM]++;
    const dim3 grid((w.M + 8 * RG - 1) / (8 * RG), (N + NC - 1) / NC);
    if (epi == EPI_RESID)
        hipLaunchKernelGGL((k_dense_mm<WT, NC, EPI_RESID>), grid, dim3(256), 0, st, w.w, w.M, w.K, scratch, N, y, y_stride, resid, resid_stride);
    else
        hipLaunchKernelGGL((k_dense_mm<WT, NC, EPI_STORE>), grid, dim3(256), 0, st, w.w, w.M, w.K, scratch, N, y, y_stride, resid, resid_stride);
    return hipGetLastError();
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Q4_1 model files.  The reference's Q4_1 path is scalar C end to end (no SIMD branch exists):
//   row layout    [nb floats min][nb floats d][nb * 16 nibble bytes]   (struct of arrays PER ROW, ggml.c:606-615)
//   activations   quantize_row_q4_1 (ggml.c:606-648): min / max of 32, d = (max - min) / 15, id = d ? 1/d : 0,
//                 code = (uint8) round((x - min) * id)
//   dot product   ggml_vec_dot_q4_1 (ggml.c:1584-1626): ONE float accumulator per output, walked over all
//                 blocks and byte pairs in order:  sumf += (d0*q0 + m0) * (d1*p0 + m1) + (d0*q1 + m0) * (d1*p1 + m1)
//                 with every product and sum rounded separately (-std=c11: no contraction).
// The activation side (d1*p + m1, the same for every weight row) is expanded once per mat-mul by k_q41_act.
// Weights are regrouped at load into [row-block of 64][block][lane] so that a wave's loads are coalesced.
// Two kernels read that one copy:
//   k_q41_mm     a lane owns a whole weight row and does everything for it, one activation row per workgroup:
//                K/2 dependent additions behind a dozen instructions each.  Kept as the plain statement of the
//                arithmetic (llamahip_op_mul_mat_q4_1, path LANE); model handles no longer launch it.
//   k_q41_chain  the pair term p = f0*a0 + f1*a1 does not depend on the accumulator, so any lane may form it;
//                only sum = sum + p has to run in pair order.  Product waves form the terms of a slab for up to
//                16 activation rows from ONE dequantisation of the weights and park them in LDS; one chain lane
//                per output adds them up in order while the product waves fill the other buffer (q41_plan).
// ------------------------------------------------------------------------------------------------
typedef uint32_t du32x4 __attribute__((ext_vector_type(4)));
typedef float df32x2 __attribute__((ext_vector_type(2)));

namespace {

// raw rows -> MD[rb][block][lane] = {min, d}, NB[rb][block][lane] = 16 nibble bytes
__global__ void k_q41_repack(const uint8_t *__restrict__ raw, df32x2 *__restrict__ md, du32x4 *__restrict__ nbv, int M, int nb) {
    const long gid = (long) blockIdx.x * blockDim.x + threadIdx.x;
    const int nrb = (M + 63) / 64;
    if (gid >= (long) nrb * nb * 64) return;
    const int lane = (int) (gid & 63), i = (int) ((gid >> 6) % nb), rb = (int) ((gid >> 6) / nb);
    const int row = rb * 64 + lane;
    df32x2 o = { 0.0f, 0.0f };
    du32x4 q = { 0u, 0u, 0u, 0u };
    if (row < M) {
        const uint8_t *base = raw + (size_t) row * nb * 24;
        uint32_t b0, b1;
        memcpy(&b0, base + 4 * i, 4);
        memcpy(&b1, base + 4 * (nb + i), 4);
        o = df32x2{ __builtin_bit_cast(float, b0), __builtin_bit_cast(float, b1) };
        uint32_t t[4];
        memcpy(t, base + 8 * nb + 16 * i, 16);
        q = du32x4{ t[0], t[1], t[2], t[3] };
    }
    md[gid] = o;
    nbv[gid] = q;
}

// one activation row: quantize to Q4_1 and expand again (the operand ggml_vec_dot_q4_1 builds from src1)
__global__ void k_q41_act(const float *__restrict__ x, long x_stride, int K, float *__restrict__ a) {
    const int n = blockIdx.x;
    const float *xr = x + (size_t) n * x_stride;
    for (int i = threadIdx.x; i < K / 32; i += blockDim.x) {
        float mn = 3.402823466e+38f, mx = -3.402823466e+38f;
        float v[32];
#pragma unroll
        for (int l = 0; l < 32; l++) { v[l] = xr[i * 32 + l]; if (v[l] < mn) mn = v[l]; if (v[l] > mx) mx = v[l]; }
        const float d = (mx - mn) / 15.0f;
        const float id = d != 0.0f ? 1.0f / d : 0.0f;
#pragma unroll
        for (int l = 0; l < 32; l++) {
            const uint32_t q = (uint32_t) (uint8_t) round((double) ((v[l] - mn) * id)) & 0xF;     // pp = vi0 | vi1 << 4: 4 bits survive
            a[(size_t) n * K + i * 32 + l] = d * (float) q + mn;
        }
    }
}

template <int EPI>
__global__ void __launch_bounds__(64)
k_q41_mm(const df32x2 *__restrict__ md, const du32x4 *__restrict__ nbv, int M, int nb, const float *__restrict__ a, int K, int N,
         float *__restrict__ y, long y_stride, const float *__restrict__ resid, long resid_stride) {
    const int lane = threadIdx.x, rb = blockIdx.x, n = blockIdx.y;
    const float *ar = a + (size_t) n * K;                  // wave-uniform: scalar loads
    const size_t base = (size_t) rb * nb * 64 + lane;
    float sum = 0.0f;
    for (int i = 0; i < nb; i++) {
        const df32x2 w = md[base + (size_t) i * 64];
        const du32x4 q = nbv[base + (size_t) i * 64];
        const uint32_t qq[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t b = (qq[j >> 2] >> (8 * (j & 3))) & 0xFF;
            const float f0 = w.y * (float) (b & 0xF) + w.x;
            const float f1 = w.y * (float) (b >> 4) + w.x;
            const float t = f0 * ar[i * 32 + 2 * j], u = f1 * ar[i * 32 + 2 * j + 1];
            sum = sum + (t + u);
        }
    }
    const int m = rb * 64 + lane;
    if (m < M) {
        if (EPI == EPI_RESID) sum = sum + resid[(size_t) n * resid_stride + m];
        y[(size_t) n * y_stride + m] = sum;
    }
}

// k_q41_chain<NR, EPI>: Q41_R weight rows x up to NR activation rows (n_base ..) per workgroup, C = Q41_R * NR outputs, slabs of
// S = q41_slab_pairs(NR) byte pairs.
//   threads 0 .. 255 (waves 0 .. 3), product role: thread = (row r = t & 15, word slot (t >> 4) & 15).  A word is 4 nibble bytes = 4 byte pairs
//     of one row; the thread dequantises its 8 weights once and forms the 4 pair terms of each activation row, every product and sum
//     rounded on its own as k_q41_mm rounds them, then parks them as one 16-byte store at terms[word][n * Q41_R + r].  The 16 rows of
//     a word share their activations: the product threads stage the slab's NR x 2S floats in LDS with coalesced loads and read them
//     back as broadcasts.  Nothing a slab needs from global memory is waited for inside it: the words and the activation slab of
//     slab s + 1 are requested before slab s is computed, and land in registers / the other activation buffer behind it.
//     From 12 rows on the slab is 32 pairs = 8 words, so that two workgroups share a CU (72 KiB of LDS at 16 rows) and one's barriers
//     and LDS traffic overlap the other's arithmetic; the two halves of the product threads then split the activation rows of the
//     same words (the dequantisation is done twice).
//   the threads behind them, chain role: thread c < C owns output (n = c >> 4, r = c & 15) and adds its terms in pair order, 16-byte
//     reads issued three blocks of 16 pairs ahead of their use; sum lives in a register from slab to slab.
// A chain lane's 16 bytes sit next to its neighbours' (a wave reads 1 KiB contiguous: no bank conflict in any 16-lane group), and so
// do the 16 rows of a product store.  The roles meet at ONE __syncthreads() per slab on two buffers: at step s the product waves fill
// buffer s & 1 while the chain waves drain the other; nslab is a kernel argument, so every thread runs 1 + nslab barriers.  Row
// tails are predicated: weight rows past M are the repack's zero rows, activation rows past N re-read row N - 1, neither is stored.
// LDS: terms[2][S/4][C] float4, then act[2][NR][S/2] float4 (q41_plan's lds).
// (Q41_R = 16 weight rows, the product threads, the compiled NR and their slab: q41_plan.h)
template <int NR, int EPI>
__global__ void __launch_bounds__(q41_prod_threads(NR) + (Q41_R * NR + 63) / 64 * 64)
k_q41_chain(const df32x2 *__restrict__ md, const uint32_t *__restrict__ nbw, int M, int nb, const float *__restrict__ a, int K, int N, int n_base,
            int nslab, float *__restrict__ y, long y_stride, const float *__restrict__ resid, long resid_stride) {
    extern __shared__ __attribute__((aligned(16))) float q41_lds[];
    constexpr int C = Q41_R * NR, S = q41_slab_pairs(NR);
    constexpr int G = S / 4;                                 // words (16-byte term groups) per row and slab
    constexpr int PROD = q41_prod_threads(NR);               // product threads
    constexpr int WSLOTS = G < PROD / Q41_R ? G : PROD / Q41_R;      // word slots: 16, or the 8 words of a 32-pair slab ...
    constexpr int NSPLIT = PROD / (Q41_R * WSLOTS);          // ... whose product threads then split the activation rows in two halves
    constexpr int NH = NR / NSPLIT;                          // activation rows per product thread
    constexpr int WPT = G / WSLOTS;                          // words per product thread and slab
    constexpr int AROW = S / 2, AF4 = NR * AROW;             // float4 per activation row and slab, per slab
    constexpr int APT = (AF4 + PROD - 1) / PROD;             // ... per product thread
    static_assert(G % WSLOTS == 0 && WPT >= 1 && NR % NSPLIT == 0 && Q41_R * WSLOTS * NSPLIT == PROD, "a slab is whole rounds of the product threads");
    const int tid = threadIdx.x;
    const int P = nb * 16;                                   // byte pairs per row
    const int n0 = n_base + blockIdx.y * NR;
    float4 *terms = (float4 *) q41_lds, *act = (float4 *) q41_lds + 2 * G * C;
    if (tid < PROD) {
        const int r = tid & (Q41_R - 1), ws = (tid >> 4) & (WSLOTS - 1), nlo = tid / (Q41_R * WSLOTS) * NH;
        const size_t rowbase = (size_t) (blockIdx.x >> 2) * nb * 64 + (blockIdx.x & 3) * Q41_R + r;
        df32x2 wm[WPT], wm_next[WPT];
        uint32_t bits[WPT], bits_next[WPT];
        float4 areg[APT];
        // the words and the activations of slab s, guarded by what the slab holds (the last one may be short)
        auto fetch = [&](int s, df32x2 *m_, uint32_t *b_) {
            const int pairs = min(S, P - s * S);
#pragma unroll
            for (int k = 0; k < WPT; k++) {
                const int w = ws + k * WSLOTS;
                m_[k] = df32x2{ 0.0f, 0.0f }; b_[k] = 0u;
                if (4 * w < pairs) {
                    const int gw = s * G + w, i = gw >> 2, q = gw & 3;
                    m_[k] = md[rowbase + (size_t) i * 64];
                    b_[k] = nbw[(rowbase + (size_t) i * 64) * 4 + q];
                }
            }
#pragma unroll
            for (int k = 0; k < APT; k++) {
                const int e = tid + k * PROD, n = e / AROW, e4 = e % AROW;
                areg[k] = float4{ 0.0f, 0.0f, 0.0f, 0.0f };
                if (e < AF4 && 2 * e4 < pairs) areg[k] = *(const float4 *) (a + (size_t) min(n0 + n, N - 1) * K + (size_t) s * 2 * S + 4 * e4);
            }
        };
        auto park = [&](int s) {
#pragma unroll
            for (int k = 0; k < APT; k++) {
                const int e = tid + k * PROD;
                if (e < AF4) act[(s & 1) * AF4 + e] = areg[k];
            }
        };
        fetch(0, wm, bits);
        park(0);
        __syncthreads();
        for (int s = 0; s < nslab; s++) {
            if (s + 1 < nslab) fetch(s + 1, wm_next, bits_next);
            float4 *buf = terms + (s & 1) * G * C;
            const float4 *as = act + (s & 1) * AF4;
            const int pairs = min(S, P - s * S);
#pragma unroll
            for (int k = 0; k < WPT; k++) {
                const int w = ws + k * WSLOTS;
                if (4 * w < pairs) {
                    float f[8];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint32_t b = (bits[k] >> (8 * j)) & 0xFF;
                        f[2 * j] = wm[k].y * (float) (b & 0xF) + wm[k].x;
                        f[2 * j + 1] = wm[k].y * (float) (b >> 4) + wm[k].x;
                    }
#pragma unroll
                    for (int n = nlo; n < nlo + NH; n++) {
                        const float4 a0 = as[n * AROW + 2 * w], a1 = as[n * AROW + 2 * w + 1];
                        float4 p;
                        { const float t = f[0] * a0.x, u = f[1] * a0.y; p.x = t + u; }
                        { const float t = f[2] * a0.z, u = f[3] * a0.w; p.y = t + u; }
                        { const float t = f[4] * a1.x, u = f[5] * a1.y; p.z = t + u; }
                        { const float t = f[6] * a1.z, u = f[7] * a1.w; p.w = t + u; }
                        buf[w * C + n * Q41_R + r] = p;
                    }
                }
            }
            if (s + 1 < nslab) {
                park(s + 1);
#pragma unroll
                for (int k = 0; k < WPT; k++) { wm[k] = wm_next[k]; bits[k] = bits_next[k]; }
            }
            __syncthreads();
        }
    } else {
        const int c = tid - PROD;
        const bool live = c < C;
        float sum = 0.0f;
        __syncthreads();                                     // (the product role's first activation slab)
        for (int s = 0; s < nslab; s++) {
            __syncthreads();
            if (live) {
                const float4 *bp = terms + (s & 1) * G * C + c;
                const int nblk = (min(S, P - s * S)) >> 4;      // blocks of 16 pairs = 4 reads
                // Whole groups of 4 blocks (every slab but a short last one is made of them) run through a ring of 4 blocks in
                // registers, straight-line: block b + 3 is requested before block b is added up; the last three requests of a slab
                // re-read its last block and are dropped.
                const int nq4 = nblk & ~3;
                if (nq4) {
                    float4 ring[4][4];
#pragma unroll
                    for (int k = 0; k < 3; k++)
#pragma unroll
                        for (int j = 0; j < 4; j++) ring[k][j] = bp[(size_t) (4 * k + j) * C];
                    for (int b = 0; b < nq4; b += 4) {
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const int nx = min(b + k + 3, nq4 - 1);
#pragma unroll
                            for (int j = 0; j < 4; j++) ring[(k + 3) & 3][j] = bp[(size_t) (4 * nx + j) * C];
#pragma unroll
                            for (int j = 0; j < 4; j++) {
                                const float4 v = ring[k][j];
                                sum = sum + v.x; sum = sum + v.y; sum = sum + v.z; sum = sum + v.w;
                            }
                        }
                    }
                }
                if (S < 64) {                               // a slab of two blocks: both requested, then added (the second where it exists)
                    float4 v[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) v[j] = bp[j * C];
#pragma unroll
                    for (int j = 0; j < 4; j++) { sum = sum + v[j].x; sum = sum + v[j].y; sum = sum + v[j].z; sum = sum + v[j].w; }
                    if (nblk > 1) {
#pragma unroll
                        for (int j = 4; j < 8; j++) { sum = sum + v[j].x; sum = sum + v[j].y; sum = sum + v[j].z; sum = sum + v[j].w; }
                    }
                } else
                for (int b = nq4; b < nblk; b++) {          // a last slab's odd blocks
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const float4 v = bp[(size_t) (4 * b + j) * C];
                        sum = sum + v.x; sum = sum + v.y; sum = sum + v.z; sum = sum + v.w;
                    }
                }
            }
        }
        const int n = n0 + (c >> 4), m = blockIdx.x * Q41_R + (c & (Q41_R - 1));
        if (live && n < N && m < M) {
            if (EPI == EPI_RESID) sum = sum + resid[(size_t) n * resid_stride + m];
            y[(size_t) n * y_stride + m] = sum;
        }
    }
}

__global__ void k_embed_q41(const int32_t *__restrict__ tokens, const uint8_t *__restrict__ emb, float *__restrict__ x, int d) {
    const int n = blockIdx.x, nb = d / 32;
    const uint8_t *base = emb + (size_t) tokens[n] * nb * 24;             // dequantize_row_q4_1 (ggml.c:686-717)
    for (int e = threadIdx.x; e < d; e += blockDim.x) {
        const int i = e >> 5, l = e & 31;
        uint32_t b0, b1;
        memcpy(&b0, base + 4 * i, 4);
        memcpy(&b1, base + 4 * (nb + i), 4);
        const float mn = __builtin_bit_cast(float, b0), dd = __builtin_bit_cast(float, b1);
        const uint32_t byte = base[8 * nb + 16 * i + (l >> 1)];
        const int vi = (l & 1) ? (int) (byte >> 4) : (int) (byte & 0xF);
        x[(size_t) n * d + e] = (float) vi * dd + mn;
    }
}

// ggml_quantize_q4_1 (utils.cpp:487-544), one thread per block.  NOT quantize_row_q4_1: here `max` starts
// at std::numeric_limits<float>::min() (the smallest POSITIVE float), as the reference has it.
__global__ void k_quantize_q41_offline(const void *__restrict__ src, int f16, uint8_t *__restrict__ dst, long nrows, int nb) {
    const long gid = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= nrows * nb) return;
    const long row = gid / nb;
    const int i = (int) (gid % nb);
    float v[32];
    if (f16) { const uint16_t *p = (const uint16_t *) src + gid * 32; for (int l = 0; l < 32; l++) v[l] = h2f(p[l]); }
    else     { const float *p = (const float *) src + gid * 32; for (int l = 0; l < 32; l++) v[l] = p[l]; }
    float mn = 3.402823466e+38f, mx = 1.175494351e-38f;
    for (int l = 0; l < 32; l++) { if (v[l] < mn) mn = v[l]; if (v[l] > mx) mx = v[l]; }
    const float d = (mx - mn) / 15.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    uint8_t *base = dst + (size_t) row * nb * 24;
    const uint32_t bm = __builtin_bit_cast(uint32_t, mn), bd = __builtin_bit_cast(uint32_t, d);
    for (int k = 0; k < 4; k++) { base[4 * i + k] = (uint8_t) (bm >> (8 * k)); base[4 * (nb + i) + k] = (uint8_t) (bd >> (8 * k)); }
    for (int l = 0; l < 32; l += 2) {
        const uint8_t q0 = (uint8_t) round((double) ((v[l] - mn) * id)), q1 = (uint8_t) round((double) ((v[l + 1] - mn) * id));
        base[8 * nb + 16 * i + l / 2] = (uint8_t) (q0 | (q1 << 4));
    }
}

}  // namespace

// f16 / f32 rows [row0, row0 + rows) of `w` from raw file-layout rows (load time)
hipError_t launch_dense_perm_rows(const void *raw, DMat &w, int row0, int rows, hipStream_t st) {
    const long total = (long) rows * w.K;
    const size_t esz = w.wtype == 1 ? 2 : 4;
    void *dst = (uint8_t *) w.w + (size_t) row0 * w.K * esz;
    if (w.wtype == 1) hipLaunchKernelGGL(k_dense_perm_rows<1>, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, st, raw, dst, (long) rows, w.K);
    else              hipLaunchKernelGGL(k_dense_perm_rows<0>, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, st, raw, dst, (long) rows, w.K);
    return hipGetLastError();
}

hipError_t launch_q41_repack(const uint8_t *raw, DMat &w, hipStream_t st) {
    const int nb = w.K / 32;
    const long total = (long) ((w.M + 63) / 64) * nb * 64;
    hipLaunchKernelGGL(k_q41_repack, dim3((unsigned) ((total + 255) / 256)), dim3(256), 0, st, raw, (df32x2 *) w.w, (du32x4 *) w.w2, w.M, nb);
    return hipGetLastError();
}

hipError_t launch_quantize_q41_offline(const void *src, int f16, uint8_t *dst, long nrows, int nb, hipStream_t st) {
    const long total = nrows * nb;
    hipLaunchKernelGGL(k_quantize_q41_offline, dim3((unsigned) ((total + 127) / 128)), dim3(128), 0, st, src, f16, dst, nrows, nb);
    return hipGetLastError();
}

long g_dense_path_counts[DENSE_COUNT_N] = { 0, 0, 0 };

// The launch plan of k_dense_set, the one place that derives it: NR = the row count rounded up to the next compiled instance (even);
// workgroups of 8 half-waves; RG = 4 weight rows per half-wave where that still gives every CU two workgroups, and 2 rows for the narrower
// matrices -- at 7B wq|wk|wv, wo and w2: with 4 rows a 4096-row matrix is 512 waves on 1024 SIMDs, and from ~8 activation rows on the
// launch is bound by FMA issue, not by the stream; a slab of UG groups per activation row, two LDS buffers of it.
DenseSetPlan dense_set_plan(int M, int K, int wtype, int N) {
    DenseSetPlan p = { 0, 0, 0, 0, 0, 0 };
    if (M < 1 || K < 32 || K % 32 != 0 || (wtype != 0 && wtype != 1) || N < 1 || N > DENSE_SET_MAX_ROWS) return p;
    p.nr = std::max(2, (N + 1) & ~1);
    p.hw = 8;
    p.rg = (M + 8 * RG - 1) / (8 * RG) >= 512 ? RG : 2;
    p.grid = (M + p.hw * p.rg - 1) / (p.hw * p.rg);
    p.slab = (wtype == 1 && p.nr <= 4) ? 2 : 1;
    p.lds = 2 * p.slab * p.nr * 256 * 4;
    return p;
}
bool dense_set_plan_has_kernel(const DenseSetPlan &p) {
    return p.nr >= 2 && p.nr <= 16 && p.nr % 2 == 0 && p.hw == 8 && (p.rg == RG || p.rg == 2);      // go_set_rows / go_set
}

// The launch plan of k_dense_mfma, the one place that derives it.  The kernel takes more than 16 rows (fewer are k_dense_mv / k_dense_set's),
// K a multiple of 128 (whole groups of 256 plus at most one 4-step group) and operands it can index with 32 bits.  Workgroups of 64 activation
// rows x 32 weight rows (two accumulator tiles per wave) where that still gives every CU one, else x 16 weight rows: a 4096-row matrix
// against 64 rows would be 128 workgroups on 256 CUs.
long g_dense_mfma_launches = 0;
int g_dense_force = 0;
DenseMfmaPlan dense_mfma_plan(int M, int K, int wtype, int N) {
    DenseMfmaPlan p = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (M < 1 || K < DENSE_MFMA_K_UNIT || K % DENSE_MFMA_K_UNIT != 0 || (wtype != 0 && wtype != 1) || N <= DENSE_SET_MAX_ROWS) return p;
    if ((long) N * K >= (1L << 31) || (N + MF_TN - 1) / MF_TN > 65535) return p;
    p.ok = 1;
    p.tile_rows = MF_TN;
    p.grid_y = (N + MF_TN - 1) / MF_TN;
    p.tile_cols = (long) ((M + 31) / 32) * p.grid_y >= 256 ? 32 : 16;
    p.grid_x = (M + p.tile_cols - 1) / p.tile_cols;
    p.threads = 256;
    p.lds = (p.tile_rows + p.tile_cols) * MF_LD * 4;
    p.auto_pick = N >= DENSE_MFMA_AUTO_MIN_ROWS;
    return p;
}
bool dense_mfma_plan_has_kernel(const DenseMfmaPlan &p) {
    return p.ok && p.tile_rows == MF_TN && (p.tile_cols == 16 || p.tile_cols == 32) && p.threads == 256;      // go's LD_MFMA
}

// AUTO.  2 .. 16 rows: k_dense_set for the row counts at which it was not slower than k_dense_mm<WT, 8> on any of the five 7B
// matrices; more rows: k_dense_mfma where it takes the shape and from the row count at which it beat k_dense_mm on all
// five, else k_dense_mm.  LLAMAHIP_DENSE_MM=set / mm / mfma, or llamahip_debug_dense_force for more than 16 rows, sends
// every such row count to one kernel where that kernel takes the shape (measurement, tests)
static int dense_auto_path(int M, int K, int wtype, int N) {
    static const int env = [] {
        const char *e = getenv("LLAMAHIP_DENSE_MM");
        return !e ? 0 : !strcmp(e, "set") ? DENSE_PATH_SET : !strcmp(e, "mm") ? DENSE_PATH_MM : !strcmp(e, "mfma") ? DENSE_PATH_MFMA : 0;
    }();
    if (N == 1) return DENSE_PATH_MV;
    if (N > DENSE_SET_MAX_ROWS) {
        const int force = g_dense_force ? g_dense_force : env == DENSE_PATH_SET ? 0 : env;
        if (force == DENSE_PATH_MM) return DENSE_PATH_MM;
        const DenseMfmaPlan p = dense_mfma_plan(M, K, wtype, N);
        return p.ok && (force == DENSE_PATH_MFMA || p.auto_pick) ? DENSE_PATH_MFMA : DENSE_PATH_MM;
    }
    if (env == DENSE_PATH_SET || env == DENSE_PATH_MM) return env;
    return DENSE_PATH_SET;
}

hipError_t init_attrs_dense() {
    const int cap = 160 * 1024;          // k_dense_mfma's operand tile is 83 / 100 KB of dynamic LDS
#define LH_ATTR(KERNEL) do { hipError_t e_ = hipFuncSetAttribute((const void *) KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, cap); if (e_ != hipSuccess) return e_; } while (0)
    LH_ATTR((k_dense_mfma<0, EPI_STORE, 1>)); LH_ATTR((k_dense_mfma<0, EPI_RESID, 1>)); LH_ATTR((k_dense_mfma<0, EPI_STORE, 2>)); LH_ATTR((k_dense_mfma<0, EPI_RESID, 2>));
    LH_ATTR((k_dense_mfma<1, EPI_STORE, 1>)); LH_ATTR((k_dense_mfma<1, EPI_RESID, 1>)); LH_ATTR((k_dense_mfma<1, EPI_STORE, 2>)); LH_ATTR((k_dense_mfma<1, EPI_RESID, 2>));
#define LH_Q41_ATTR(NR) LH_ATTR((k_q41_chain<NR, EPI_STORE>)); LH_ATTR((k_q41_chain<NR, EPI_RESID>));
    LH_Q41_INSTANCES(LH_Q41_ATTR)          // k_q41_chain's two slab buffers: up to 128 KB
#undef LH_Q41_ATTR
#undef LH_ATTR
    return hipSuccess;
}

static hipError_t go_q41_chain(const Q41Plan &p, int grid_y, int n_base, const DMat &w, int epi, int N, float *y, long y_stride,
                               const float *resid, long resid_stride, hipStream_t st, const float *scratch) {
    if (!q41_plan_has_kernel(p)) return hipErrorInvalidValue;
    const dim3 grid(p.grid_x, grid_y);
    const int nb = w.K / 32, nslab = (nb * 16 + p.slab - 1) / p.slab;
#define LH_GO(NR) if (p.nr == NR) { \
        if (epi == EPI_RESID) hipLaunchKernelGGL((k_q41_chain<NR, EPI_RESID>), grid, dim3(p.threads), p.lds, st, (const df32x2 *) w.w, (const uint32_t *) w.w2, w.M, nb, scratch, w.K, N, n_base, nslab, y, y_stride, resid, resid_stride); \
        else hipLaunchKernelGGL((k_q41_chain<NR, EPI_STORE>), grid, dim3(p.threads), p.lds, st, (const df32x2 *) w.w, (const uint32_t *) w.w2, w.M, nb, scratch, w.K, N, n_base, nslab, y, y_stride, resid, resid_stride); \
    }
    LH_Q41_INSTANCES(LH_GO)
#undef LH_GO
    return hipGetLastError();
}

// Q4_1 mat-mul: k_q41_act, then k_q41_chain in row tiles of at most 16 (AUTO, CHAIN) or k_q41_mm (LANE: llamahip_op_mul_mat_q4_1 only)
hipError_t launch_q41_mm(const DMat &w, int epi, const float *x, long x_stride, int N, float *y, long y_stride,
                         const float *resid, long resid_stride, hipStream_t st, float *scratch, int path, int *path_taken) {
    if (w.wtype != 3 || w.K < 32 || w.K % 32 != 0 || !scratch || N < 1 || path < Q41_PATH_AUTO || path > Q41_PATH_LANE) return hipErrorInvalidValue;
    const int run = path == Q41_PATH_AUTO ? Q41_PATH_CHAIN : path;
    if (run == Q41_PATH_CHAIN && !q41_plan(w.M, w.K, N).nr) return hipErrorInvalidValue;
    if (path_taken) *path_taken = run;
    hipLaunchKernelGGL(k_q41_act, dim3(N), dim3(64), 0, st, x, x_stride, w.K, scratch);
    if (run == Q41_PATH_LANE) {
        g_q41_path_counts[Q41_COUNT_LANE]++;
        const dim3 grid((w.M + 63) / 64, N);
        if (epi == EPI_RESID)
            hipLaunchKernelGGL((k_q41_mm<EPI_RESID>), grid, dim3(64), 0, st, (const df32x2 *) w.w, (const du32x4 *) w.w2, w.M, w.K / 32, scratch, w.K, N, y, y_stride, resid, resid_stride);
        else
            hipLaunchKernelGGL((k_q41_mm<EPI_STORE>), grid, dim3(64), 0, st, (const df32x2 *) w.w, (const du32x4 *) w.w2, w.M, w.K / 32, scratch, w.K, N, y, y_stride, resid, resid_stride);
        return hipGetLastError();
    }
    g_q41_path_counts[Q41_COUNT_CHAIN]++;
    const int full = N / Q41_TILE, rem = N % Q41_TILE;
    if (full) {
        const hipError_t e = go_q41_chain(q41_plan(w.M, w.K, Q41_TILE), full, 0, w, epi, N, y, y_stride, resid, resid_stride, st, scratch);
        if (e != hipSuccess) return e;
    }
    if (rem) return go_q41_chain(q41_plan(w.M, w.K, rem), 1, full * Q41_TILE, w, epi, N, y, y_stride, resid, resid_stride, st, scratch);
    return hipSuccess;
}

hipError_t launch_dense_mm(const DMat &w, int epi, const float *x, long x_stride, int N, float *y, long y_stride,
                           const float *resid, long resid_stride, hipStream_t st, float *scratch, int path, int *path_taken) {
    if (w.wtype == 3) return launch_q41_mm(w, epi, x, x_stride, N, y, y_stride, resid, resid_stride, st, scratch, Q41_PATH_AUTO, nullptr);
    if (w.K % 32 != 0 || (w.wtype != 0 && w.wtype != 1) || !scratch) return hipErrorInvalidValue;
    if (N < 1 || path < DENSE_PATH_AUTO || path > DENSE_PATH_MFMA || (path == DENSE_PATH_SET && N > DENSE_SET_MAX_ROWS)) return hipErrorInvalidValue;
    if (path == DENSE_PATH_MFMA && !dense_mfma_plan(w.M, w.K, w.wtype, N).ok) return hipErrorInvalidValue;
    const int run = path == DENSE_PATH_AUTO ? dense_auto_path(w.M, w.K, w.wtype, N) : path;
    if (path_taken) *path_taken = run;
    if (w.wtype == 1) return go<1, 8>(w, epi, x, x_stride, N, y, y_stride, resid, resid_stride, st, scratch, run);
    return go<0, 8>(w, epi, x, x_stride, N, y, y_stride, resid, resid_stride, st, scratch, run);
}

hipError_t launch_embed_dense_set(SeqSet *set, int n, const void *emb, int wtype, float *x, int d, hipStream_t st) {
    if (wtype == 1) hipLaunchKernelGGL(k_embed_dense_set<1>, dim3(n), dim3(256), 0, st, set, emb, x, d);
    else if (wtype == 0) hipLaunchKernelGGL(k_embed_dense_set<0>, dim3(n), dim3(256), 0, st, set, emb, x, d);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_rope_kv_set(const float *qkv, long qkv_stride, int d, int dh, const double *tab, float *qr, float *Kc, float *Vc,
                              const SeqSet *set, int N, hipStream_t st) {
    hipLaunchKernelGGL(k_rope_kv_set, dim3(N), dim3(256), 0, st, qkv, qkv_stride, d, dh, tab, qr, Kc, Vc, set);
    return hipGetLastError();
}

// norm / plain / SiLU*up -> rounded, permuted activation rows in `scratch` (then launch_dense_mm with x = nullptr).
// false = not available for this weight type / row width: use launch_prep + launch_dense_mm.
bool dense_prep_applies(int wtype, int mode, int K) {
    return mode >= 1 && mode <= 3 && (wtype == 0 || wtype == 1) && K % 32 == 0 && (mode != PREP_NORM || K / 16 <= 1024);
}
hipError_t launch_dense_prep(int mode, int wtype, const float *in0, const float *in1, long in_stride, long in1_stride,
                             int K, int N, float *scratch, const uint16_t *T_silu, hipStream_t st) {
    const int nh = K / 16;
    const int nt = mode == PREP_NORM ? (nh + 63) / 64 * 64 : 256;
    const dim3 grid(N, mode == PREP_NORM ? 1 : (nh + nt - 1) / nt);
#define LD_PREP(MODE, WT) hipLaunchKernelGGL((k_dense_prep<MODE, WT>), grid, dim3(nt), 0, st, in0, in1, in_stride, in1_stride, K, scratch, T_silu)
    if (wtype == 1) {
        if (mode == PREP_NORM) LD_PREP(PREP_NORM, 1); else if (mode == PREP_SILU_MUL) LD_PREP(PREP_SILU_MUL, 1); else LD_PREP(PREP_PLAIN, 1);
    } else {
        if (mode == PREP_NORM) LD_PREP(PREP_NORM, 0); else if (mode == PREP_SILU_MUL) LD_PREP(PREP_SILU_MUL, 0); else LD_PREP(PREP_PLAIN, 0);
    }
#undef LD_PREP
    return hipGetLastError();
}

// fp32 rows -> the rounded (f16 weights), permuted operand rows: the second half of the split preparation, and what launch_dense_mm does
// with rows it is handed un-prepared
hipError_t launch_dense_perm_act(int wtype, const float *x, long x_stride, int K, int N, float *xp, hipStream_t st) {
    if (wtype == 1) hipLaunchKernelGGL(k_dense_perm_act<1>, dim3(N), dim3(256), 0, st, x, x_stride, K, xp);
    else if (wtype == 0) hipLaunchKernelGGL(k_dense_perm_act<0>, dim3(N), dim3(256), 0, st, x, x_stride, K, xp);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// The activation operand of an f16 / f32 mat-mul, the one place that picks its producer (a model's dense_prep_mm and
// llamahip_op_dense_prep both come here).  AUTO: FUSED -- k_dense_prep, one launch -- where dense_prep_applies, else SPLIT: launch_prep
// leaves the fp32 rows y in `rows` [N][K] (PLAIN has nothing to compute: in0 is read as it lies) and k_dense_perm_act rounds and permutes
// them.  FUSED asked for where it does not apply is refused with hipErrorInvalidValue, nothing launched.  qa_A / qa_d: the Q4_0 operand
// launch_prep always writes next to y (N rows of K rounded up to 256); *taken (may be null): DENSE_PREP_FUSED or DENSE_PREP_SPLIT.
int dense_prep_kernel(int kernel, int wtype, int mode, int K) {
    if (kernel < DENSE_PREP_AUTO || kernel > DENSE_PREP_SPLIT || (wtype != 0 && wtype != 1) || mode < PREP_PLAIN || mode > PREP_SILU_MUL || K < 32 || K % 32 != 0) return -1;
    const bool fused_ok = dense_prep_applies(wtype, mode, K);
    if (kernel == DENSE_PREP_FUSED && !fused_ok) return -1;
    return kernel == DENSE_PREP_AUTO ? (fused_ok ? DENSE_PREP_FUSED : DENSE_PREP_SPLIT) : kernel;
}
hipError_t launch_dense_act(int kernel, int mode, int wtype, const float *in0, const float *in1, long in_stride, long in1_stride, int K, int N,
                            float *xp, float *rows, uint32_t *qa_A, float *qa_d, const uint16_t *T_silu, hipStream_t st, int *taken) {
    const int run = dense_prep_kernel(kernel, wtype, mode, K);
    if (run < 0 || !xp) return hipErrorInvalidValue;
    if (taken) *taken = run;
    if (run == DENSE_PREP_FUSED) return launch_dense_prep(mode, wtype, in0, in1, in_stride, in1_stride, K, N, xp, T_silu, st);
    if (mode == PREP_PLAIN) return launch_dense_perm_act(wtype, in0, in_stride, K, N, xp, st);
    if (!rows || !qa_A || !qa_d) return hipErrorInvalidValue;
    const hipError_t e = launch_prep(mode, in0, in1, in_stride, in1_stride, K, N, qa_A, qa_d, rows, nullptr, T_silu, st);
    if (e != hipSuccess) return e;
    return launch_dense_perm_act(wtype, rows, K, K, N, xp, st);
}

hipError_t launch_embed_dense(const int32_t *tokens, const void *emb, int wtype, float *x, int d, int N, hipStream_t st) {
    if (wtype == 3) hipLaunchKernelGGL(k_embed_q41, dim3(N), dim3(256), 0, st, tokens, (const uint8_t *) emb, x, d);
    else if (wtype == 1) hipLaunchKernelGGL(k_embed_dense<1>, dim3(N), dim3(256), 0, st, tokens, emb, x, d);
    else            hipLaunchKernelGGL(k_embed_dense<0>, dim3(N), dim3(256), 0, st, tokens, emb, x, d);
    return hipGetLastError();
}

}  // namespace lh
