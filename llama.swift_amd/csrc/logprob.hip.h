// logprob.hip.h -- the row reductions k_row_logprob (logprob.hip) and k_row_topn (topn.hip) share, so that both give the same bits for a row:
// one workgroup of LP_THREADS = 256 threads (4 waves) per row.
//   lp_scan  the thread's own entries: the fp32 maximum with its LOWEST index on ties (k_argmax's rule, decode.hip argmax_take), the number
//            of entries strictly greater than `lt` and whether a NaN or a +inf was seen.  Vectorised when the rows are 16-byte aligned
//            (V % 4 == 0: thread t owns the float4s t, t + 256, ...), else thread t owns the entries t, t + 256, ...
//   lp_fold  the 256 threads' results folded to the row's: all order-free, hence exact.  (One __syncthreads.)
//   lp_sum   sum_j exp((double) l[j] - (double) max) in double.  Thread t adds j = t, t + 256, ... in ascending order, the 64 lanes of a wave
//            are folded by wave_sum_d's fixed DPP / readlane tree and the four waves as (w0 + w1) + (w2 + w3): the order depends on V alone.
//            (One __syncthreads; every thread gets the total.)
//   lp_value ((double) l - (double) max) - log_sum: the log-probability of an entry with logit l.
#pragma once
#include <cmath>

#include "kcommon.hip.h"

namespace lh {

constexpr int LP_THREADS = 256;

__device__ __forceinline__ void lp_take(float &v, int &i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
template <int CTRL>
__device__ __forceinline__ void lp_take_dpp(float &v, int &i) {
    const float ov = dpp_f<CTRL>(v);
    const int oi = __builtin_amdgcn_mov_dpp(i, CTRL, 0xF, 0xF, true);
    lp_take(v, i, ov, oi);
}
template <int CTRL>
__device__ __forceinline__ int lp_add_dpp(int v) { return v + __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true); }

struct LpAcc {
    float best = -INFINITY;
    int idx = 0x7fffffff, gt = 0;
    bool bad = false;
    __device__ __forceinline__ void visit(float x, int i, float lt) {
        lp_take(best, idx, x, i);         // (a NaN never wins: both comparisons are false)
        gt += x > lt;
        bad |= (x != x) || (x == INFINITY);
    }
};

__device__ __forceinline__ LpAcc lp_scan(const float *__restrict__ row, int V, float lt) {
    const int tid = threadIdx.x;
    LpAcc a;
    if ((V & 3) == 0) {
        const float4 *__restrict__ r4 = (const float4 *) row;
        const int V4 = V >> 2;
#pragma unroll 4
        for (int k = tid; k < V4; k += LP_THREADS) {
            const float4 x = r4[k];
            a.visit(x.x, 4 * k, lt); a.visit(x.y, 4 * k + 1, lt); a.visit(x.z, 4 * k + 2, lt); a.visit(x.w, 4 * k + 3, lt);
        }
    } else {
#pragma unroll 4
        for (int i = tid; i < V; i += LP_THREADS) a.visit(row[i], i, lt);
    }
    return a;
}

// the workgroup's pick of the threads' (v, i) under lp_take's order, on every thread.  s_v / s_i: 4 words each, free to be rewritten after the
// workgroup's NEXT barrier
__device__ __forceinline__ void lp_fold_take(float &v, int &i, float *s_v, int *s_i) {
    const int tid = threadIdx.x, wave = tid >> 6;
    lp_take_dpp<DPP_QUAD_XOR1>(v, i);
    lp_take_dpp<DPP_QUAD_XOR2>(v, i);
    lp_take_dpp<DPP_ROW_HALF_MIRROR>(v, i);
    lp_take_dpp<DPP_ROW_MIRROR>(v, i);           // every lane of a 16-lane row holds the row's pick
    const int vb = __builtin_bit_cast(int, v);
    float wv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 0));
    int wi = __builtin_amdgcn_readlane(i, 0);
    lp_take(wv, wi, __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 16)), __builtin_amdgcn_readlane(i, 16));
    lp_take(wv, wi, __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 32)), __builtin_amdgcn_readlane(i, 32));
    lp_take(wv, wi, __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 48)), __builtin_amdgcn_readlane(i, 48));
    if ((tid & 63) == 0) { s_v[wave] = wv; s_i[wave] = wi; }
    __syncthreads();
    v = s_v[0]; i = s_i[0];
    for (int w = 1; w < LP_THREADS / 64; w++) lp_take(v, i, s_v[w], s_i[w]);
}

struct LpRow { float mx; int am, gt; bool bad; };
struct LpShared {
    float best[4];
    int idx[4], gt[4], bad[4];
    double sum[4];
};

__device__ __forceinline__ LpRow lp_fold(LpAcc a, LpShared &sh) {
    const int tid = threadIdx.x, wave = tid >> 6;
    a.gt = lp_add_dpp<DPP_QUAD_XOR1>(a.gt);
    a.gt = lp_add_dpp<DPP_QUAD_XOR2>(a.gt);
    a.gt = lp_add_dpp<DPP_ROW_HALF_MIRROR>(a.gt);
    a.gt = lp_add_dpp<DPP_ROW_MIRROR>(a.gt);
    const bool wbad = __any(a.bad);
    const int wg = __builtin_amdgcn_readlane(a.gt, 0) + __builtin_amdgcn_readlane(a.gt, 16) + __builtin_amdgcn_readlane(a.gt, 32) + __builtin_amdgcn_readlane(a.gt, 48);
    if ((tid & 63) == 0) { sh.gt[wave] = wg; sh.bad[wave] = wbad; }
    LpRow r;
    r.mx = a.best; r.am = a.idx;
    lp_fold_take(r.mx, r.am, sh.best, sh.idx);      // (its barrier publishes gt / bad too)
    r.gt = sh.gt[0] + sh.gt[1] + sh.gt[2] + sh.gt[3];
    r.bad = sh.bad[0] | sh.bad[1] | sh.bad[2] | sh.bad[3];
    return r;
}

__device__ __forceinline__ double lp_sum(const float *__restrict__ row, int V, double mxd, LpShared &sh) {
    const int tid = threadIdx.x, wave = tid >> 6;
    double s = 0.0;
    int i = tid;
    for (; i + 3 * LP_THREADS < V; i += 4 * LP_THREADS) {
        const float x0 = row[i], x1 = row[i + LP_THREADS], x2 = row[i + 2 * LP_THREADS], x3 = row[i + 3 * LP_THREADS];
        s += exp((double) x0 - mxd);
        s += exp((double) x1 - mxd);
        s += exp((double) x2 - mxd);
        s += exp((double) x3 - mxd);
    }
    for (; i < V; i += LP_THREADS) s += exp((double) row[i] - mxd);
    s = wave_sum_d(s);
    if ((tid & 63) == 0) sh.sum[wave] = s;
    __syncthreads();
    return (sh.sum[0] + sh.sum[1]) + (sh.sum[2] + sh.sum[3]);
}

__device__ __forceinline__ double lp_value(float l, double mxd, double log_sum) { return ((double) l - mxd) - log_sum; }

}  // namespace lh
