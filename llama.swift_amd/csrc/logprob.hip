// logprob.hip -- next-token scoring of evaluated rows (llamahip_eval_logprobs / llamahip_perplexity / llamahip_op_logprob): every row of
// logits reduced on the device to the three numbers a perplexity or accuracy count needs, so N x 16 bytes cross to the host instead of
// N x n_vocab x 4.
//
// k_row_logprob: one workgroup of 256 threads (4 waves) per row, the row read twice.
//   pass 1  (vectorised when the rows are 16-byte aligned, i.e. n_vocab % 4 == 0): the fp32 maximum with its LOWEST index on ties
//           (k_argmax's rule, decode.hip argmax_take), the number of entries strictly greater than the target's logit (its rank) and
//           whether the row holds a NaN or a +inf.  All three are order-free, hence exact.
//   pass 2  (scored, finite rows only; the row is back from L2): sum_j exp((double) l[j] - (double) max) in double.  Thread t adds
//           j = t, t + 256, ... in ascending order, the 64 lanes of a wave are folded by wave_sum_d's fixed DPP / readlane tree and the
//           four waves as (w0 + w1) + (w2 + w3): the order depends on n_vocab alone, so a row's result is a pure function of its bits,
//           whatever the number of rows, the row's index, the handle or the stream.
//   logprob = ((double) l[t] - (double) max) - log(sum)
// Non-finite rows (a NaN or a +inf anywhere): logprob NaN, argmax -1, rank -1.  -inf entries are ordinary (their exp is 0).
// Unscored rows (target -1): logprob 0.0, rank -1, argmax as usual.
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

__global__ void __launch_bounds__(LP_THREADS)
k_row_logprob(const float *__restrict__ logits, int V, const int32_t *__restrict__ targets,
              double *__restrict__ lp_out, int32_t *__restrict__ am_out, int32_t *__restrict__ rk_out) {
    __shared__ float s_best[4];
    __shared__ int s_idx[4], s_gt[4], s_bad[4];
    __shared__ double s_sum[4];
    const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const float *__restrict__ row = logits + (size_t) r * V;
    const int t = targets ? targets[r] : -1;
    const bool scored = t >= 0 && t < V;
    const float lt = scored ? row[t] : INFINITY;          // (unscored: nothing is > +inf, the count stays 0 and is not reported)

    // ---- pass 1: max / argmax / rank / non-finite flag
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
    lp_take_dpp<DPP_QUAD_XOR1>(a.best, a.idx);
    lp_take_dpp<DPP_QUAD_XOR2>(a.best, a.idx);
    lp_take_dpp<DPP_ROW_HALF_MIRROR>(a.best, a.idx);
    lp_take_dpp<DPP_ROW_MIRROR>(a.best, a.idx);           // every lane of a 16-lane row holds the row's pick
    a.gt = lp_add_dpp<DPP_QUAD_XOR1>(a.gt);
    a.gt = lp_add_dpp<DPP_QUAD_XOR2>(a.gt);
    a.gt = lp_add_dpp<DPP_ROW_HALF_MIRROR>(a.gt);
    a.gt = lp_add_dpp<DPP_ROW_MIRROR>(a.gt);
    const bool wbad = __any(a.bad);
    {
        const int vb = __builtin_bit_cast(int, a.best);
        float wv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 0));
        int wi = __builtin_amdgcn_readlane(a.idx, 0);
        lp_take(wv, wi, __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 16)), __builtin_amdgcn_readlane(a.idx, 16));
        lp_take(wv, wi, __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 32)), __builtin_amdgcn_readlane(a.idx, 32));
        lp_take(wv, wi, __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 48)), __builtin_amdgcn_readlane(a.idx, 48));
        const int wg = __builtin_amdgcn_readlane(a.gt, 0) + __builtin_amdgcn_readlane(a.gt, 16) + __builtin_amdgcn_readlane(a.gt, 32) + __builtin_amdgcn_readlane(a.gt, 48);
        if ((tid & 63) == 0) { s_best[wave] = wv; s_idx[wave] = wi; s_gt[wave] = wg; s_bad[wave] = wbad; }
    }
    __syncthreads();
    float mx = s_best[0];
    int am = s_idx[0];
    for (int w = 1; w < LP_THREADS / 64; w++) lp_take(mx, am, s_best[w], s_idx[w]);
    const bool bad = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
    if (bad || !scored) {                                    // (uniform over the workgroup)
        if (tid == 0) {
            lp_out[r] = bad ? __builtin_nan("") : 0.0;
            am_out[r] = bad ? -1 : am;
            rk_out[r] = -1;
        }
        return;
    }

    // ---- pass 2: sum of exp(l - max) in double, in an order fixed by V
    const double mxd = (double) mx;
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
    if ((tid & 63) == 0) s_sum[wave] = s;
    __syncthreads();
    if (tid == 0) {
        const double tot = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        lp_out[r] = ((double) lt - mxd) - log(tot);
        am_out[r] = am;
        rk_out[r] = s_gt[0] + s_gt[1] + s_gt[2] + s_gt[3];
    }
}

hipError_t launch_row_logprob(const float *logits, int n_rows, int V, const int32_t *targets, double *lp_out, int32_t *am_out, int32_t *rk_out,
                              hipStream_t st) {
    if (n_rows < 1 || V < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_row_logprob, dim3((unsigned) n_rows), dim3(LP_THREADS), 0, st, logits, V, targets, lp_out, am_out, rk_out);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace lh
