// pool.hip -- a text's embedding (llamahip_text_embedding[_multi] / llamahip_op_pool_rows): the final norm of the hidden rows as plain fp32, the
// pooling over each segment's rows and the optional L2 normalisation -- the tail an embedding pass runs in place of the lm head.
//
// k_norm_rows_f32: one workgroup of 256 threads per row.  y[c] = w[c] * ((float) ((double) x[c] - mean) * scale), mean and sum2 in double in the
//   two-pass form, scale = (float) (1.0 / sqrt(sum2 / d + (double) 1e-5f)): k_dense_prep<PREP_NORM>'s arithmetic (ggml.c:5327-5385 + ggml_mul)
//   without the fp16 rounding and the permutation.  Thread t adds columns t, t + 256, ... in ascending order, block_sum_d folds the threads: the
//   association order of the two double sums is this kernel's own, equality with the reference's sequential sums is by test on order-proof rows.
// k_pool_rows: one thread per (segment, column).  LAST: the segment's last row.  MEAN: acc = 0.0; acc += (double) y[j][c] for j ascending over the
//   segment's rows; o[c] = (float) (acc / (double) n_rows).  Four loads are issued ahead of their adds; the adds stay in row order.
// k_l2_rows: one wave per segment, in place.  Lane l sums (double) o[c] * (double) o[c] over c = l, l + 64, ... ascending (every product is exact
//   in double), the 64 partials are folded by the xor butterfly 32, 16, 8, 4, 2, 1 (both operands of every add are the same two numbers on both
//   lanes, so every lane holds the same ss), o[c] = (float) ((double) o[c] / sqrt(ss)); ss == 0.0 leaves the row as it is.
// No workgroup reads what another wrote in the same launch, no polling, no atomics; a segment's output depends on that segment's rows alone.
#include <cmath>

#include "../../include/llamahip.h"
#include "kcommon.hip.h"

namespace lh {

constexpr int POOL_THREADS = 256;

__global__ void __launch_bounds__(POOL_THREADS)
k_norm_rows_f32(const float *__restrict__ x, const float *__restrict__ w, int d, float *__restrict__ y) {
    __shared__ double red[32];
    const int tid = threadIdx.x;
    const float *__restrict__ xr = x + (size_t) blockIdx.x * d;
    float *__restrict__ yr = y + (size_t) blockIdx.x * d;
    double s1 = 0.0;
    for (int c = tid; c < d; c += POOL_THREADS) s1 += (double) xr[c];
    const double mean = block_sum_d(s1, red, 0) / (double) d;
    double s2 = 0.0;
    for (int c = tid; c < d; c += POOL_THREADS) { const double v = (double) xr[c] - mean; s2 += v * v; }
    const double sum2 = block_sum_d(s2, red, 1);
    const float scale = (float) (1.0 / sqrt(sum2 / (double) d + (double) 1e-5f));
    for (int c = tid; c < d; c += POOL_THREADS) {
        const float v = (float) ((double) xr[c] - mean);
        yr[c] = w[c] * (v * scale);
    }
}

__global__ void __launch_bounds__(POOL_THREADS)
k_pool_rows(const float *__restrict__ y, const int32_t *__restrict__ seg_begin, int d, int pool, float *__restrict__ o) {
    const int s = blockIdx.y, c = blockIdx.x * POOL_THREADS + threadIdx.x;
    if (c >= d) return;
    const int b = seg_begin[s], e = seg_begin[s + 1];
    const float *__restrict__ col = y + c;
    if (pool == LLAMAHIP_POOL_LAST) { o[(size_t) s * d + c] = col[(size_t) (e - 1) * d]; return; }
    double acc = 0.0;
    int j = b;
    for (; j + 3 < e; j += 4) {
        const float y0 = col[(size_t) j * d], y1 = col[(size_t) (j + 1) * d], y2 = col[(size_t) (j + 2) * d], y3 = col[(size_t) (j + 3) * d];
        acc += (double) y0;
        acc += (double) y1;
        acc += (double) y2;
        acc += (double) y3;
    }
    for (; j < e; j++) acc += (double) col[(size_t) j * d];
    o[(size_t) s * d + c] = (float) (acc / (double) (e - b));
}

__global__ void __launch_bounds__(64)
k_l2_rows(float *__restrict__ o, int d) {
    float *__restrict__ row = o + (size_t) blockIdx.x * d;
    const int l = threadIdx.x;
    double ss = 0.0;
    for (int c = l; c < d; c += 64) { const double v = (double) row[c]; ss += v * v; }
    for (int msk = 32; msk > 0; msk >>= 1) {
        int lo = __double2loint(ss), hi = __double2hiint(ss);
        lo = __shfl_xor(lo, msk); hi = __shfl_xor(hi, msk);
        ss += __hiloint2double(hi, lo);
    }
    if (ss == 0.0) return;
    const double len = sqrt(ss);
    for (int c = l; c < d; c += 64) row[c] = (float) ((double) row[c] / len);
}

hipError_t launch_norm_rows_f32(const float *x, const float *w, int d, int n_rows, float *y, hipStream_t st) {
    if (n_rows < 1 || d < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_norm_rows_f32, dim3((unsigned) n_rows), dim3(POOL_THREADS), 0, st, x, w, d, y);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_pool_rows(const float *y, const int32_t *seg_begin, int n_segs, int d, int pool, int normalize, float *out, hipStream_t st) {
    if (n_segs < 1 || d < 1 || (pool != LLAMAHIP_POOL_LAST && pool != LLAMAHIP_POOL_MEAN)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pool_rows, dim3((unsigned) ((d + POOL_THREADS - 1) / POOL_THREADS), (unsigned) n_segs), dim3(POOL_THREADS), 0, st, y, seg_begin, d, pool, out);
    LH_LAUNCH_CHECK();
    if (normalize) {
        hipLaunchKernelGGL(k_l2_rows, dim3((unsigned) n_segs), dim3(64), 0, st, out, d);
        LH_LAUNCH_CHECK();
    }
    return hipSuccess;
}

}  // namespace lh
