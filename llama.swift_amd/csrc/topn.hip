// topn.hip -- the n most probable entries of evaluated rows with their log-probabilities (llamahip_op_top_logprobs / llamahip_eval_top_logprobs /
// llamahip_beam_search): every row of logits reduced on the device to n x 12 bytes, instead of n_vocab x 4 crossing to the host.
//
// k_row_topn: one workgroup of 256 threads (4 waves) per row, no hand-off between workgroups, no atomics.
//   ORDER    value descending, the LOWER index first on equal values (+0.0 == -0.0): lp_take's rule (k_argmax's), carried on to n places.
//   STATS    lp_scan / lp_fold / lp_sum of logprob.hip.h, the code k_row_logprob runs: the same maximum, the same double sum in the same order,
//            so logprob[j] = lp_value(l[ids[j]], max, log(sum)) is bit for bit k_row_logprob's for the target ids[j].
//   PLACES   lp_scan leaves every thread the best of its OWN entries (thread t owns the float4s t, t + 256, ... where V % 4 == 0, else the
//            entries t, t + 256, ...).  A round folds the 256 threads' candidates to the workgroup's pick (lp_fold_take: DPP, four words of
//            LDS, one barrier), which is the next place; then the ONE thread that owned it rescans its own entries (V / 256 of them, from L2: the
//            row has just been read twice) for its best entry that comes AFTER the pick in the order.  n rounds; a round costs a fold and, on
//            one thread, V / 256 loads.  The order is total on a finite row, so any scheme gives these places.
// Non-finite rows (a NaN or a +inf anywhere): every id -1, every logprob NaN, as k_row_logprob flags them.  -inf entries are ordinary: they
// come last, in index order.  A row's result depends on its bits, V and n alone.
#include "logprob.hip.h"

namespace lh {

// does (x, i) come after (pv, pi) in the order?
__device__ __forceinline__ bool topn_after(float x, int i, float pv, int pi) { return x < pv || (x == pv && i > pi); }

__global__ void __launch_bounds__(LP_THREADS)
k_row_topn(const float *__restrict__ logits, int V, int n, int32_t *__restrict__ ids_out, double *__restrict__ lp_out) {
    __shared__ LpShared sh;
    __shared__ float s_v[2][4];
    __shared__ int s_i[2][4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float *__restrict__ row = logits + (size_t) r * V;
    int32_t *__restrict__ ids = ids_out + (size_t) r * n;
    double *__restrict__ lps = lp_out + (size_t) r * n;

    const LpAcc mine = lp_scan(row, V, INFINITY);            // (.best / .idx: this thread's first candidate; idx 0x7fffffff = it owns nothing)
    const LpRow st = lp_fold(mine, sh);
    if (st.bad) {                                              // (uniform over the workgroup)
        for (int j = tid; j < n; j += LP_THREADS) { ids[j] = -1; lps[j] = __builtin_nan(""); }
        return;
    }
    const double mxd = (double) st.mx;
    const double tot = lp_sum(row, V, mxd, sh);
    const double log_sum = tid == 0 ? log(tot) : 0.0;

    float cv = mine.best;
    int ci = mine.idx;
    const bool vec = (V & 3) == 0;
    for (int j = 0; j < n; j++) {
        float wv = cv;
        int wi = ci;
        lp_fold_take(wv, wi, s_v[j & 1], s_i[j & 1]);        // (the words of round j are rewritten in round j + 2, behind round j + 1's barrier)
        if (tid == 0) { ids[j] = wi; lps[j] = lp_value(wv, mxd, log_sum); }
        if (ci == wi && j + 1 < n) {                         // the owner of the pick: its next candidate
            float nv = -INFINITY;
            int ni = 0x7fffffff;
            if (vec) {
                const float4 *__restrict__ r4 = (const float4 *) row;
                const int V4 = V >> 2;
#pragma unroll 4
                for (int k = tid; k < V4; k += LP_THREADS) {
                    const float4 x = r4[k];
                    if (topn_after(x.x, 4 * k, wv, wi)) lp_take(nv, ni, x.x, 4 * k);
                    if (topn_after(x.y, 4 * k + 1, wv, wi)) lp_take(nv, ni, x.y, 4 * k + 1);
                    if (topn_after(x.z, 4 * k + 2, wv, wi)) lp_take(nv, ni, x.z, 4 * k + 2);
                    if (topn_after(x.w, 4 * k + 3, wv, wi)) lp_take(nv, ni, x.w, 4 * k + 3);
                }
            } else {
#pragma unroll 4
                for (int i = tid; i < V; i += LP_THREADS) {
                    const float x = row[i];
                    if (topn_after(x, i, wv, wi)) lp_take(nv, ni, x, i);
                }
            }
            cv = nv; ci = ni;
        }
    }
}

hipError_t launch_row_topn(const float *logits, int n_rows, int V, int n, int32_t *ids_out, double *lp_out, hipStream_t st) {
    if (n_rows < 1 || V < 1 || n < 1 || n > TOPN_MAX || n > V) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_row_topn, dim3((unsigned) n_rows), dim3(LP_THREADS), 0, st, logits, V, n, ids_out, lp_out);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace lh
