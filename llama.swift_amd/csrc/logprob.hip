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
#include "logprob.hip.h"

namespace lh {

// (the reductions themselves: logprob.hip.h, shared with k_row_topn)
__global__ void __launch_bounds__(LP_THREADS)
k_row_logprob(const float *__restrict__ logits, int V, const int32_t *__restrict__ targets,
              double *__restrict__ lp_out, int32_t *__restrict__ am_out, int32_t *__restrict__ rk_out) {
    __shared__ LpShared sh;
    const int r = blockIdx.x, tid = threadIdx.x;
    const float *__restrict__ row = logits + (size_t) r * V;
    const int t = targets ? targets[r] : -1;
    const bool scored = t >= 0 && t < V;
    const float lt = scored ? row[t] : INFINITY;          // (unscored: nothing is > +inf, the count stays 0 and is not reported)

    // ---- pass 1: max / argmax / rank / non-finite flag
    const LpRow st = lp_fold(lp_scan(row, V, lt), sh);
    if (st.bad || !scored) {                                 // (uniform over the workgroup)
        if (tid == 0) {
            lp_out[r] = st.bad ? __builtin_nan("") : 0.0;
            am_out[r] = st.bad ? -1 : st.am;
            rk_out[r] = -1;
        }
        return;
    }

    // ---- pass 2: sum of exp(l - max) in double, in an order fixed by V
    const double mxd = (double) st.mx;
    const double tot = lp_sum(row, V, mxd, sh);
    if (tid == 0) {
        lp_out[r] = lp_value(lt, mxd, log(tot));
        am_out[r] = st.am;
        rk_out[r] = st.gt;
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
