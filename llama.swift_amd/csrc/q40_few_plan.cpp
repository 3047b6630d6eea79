// q40_few_plan.cpp -- the host half of the opt-in int8 matrix-core few-row mat-mul k_q40_few (q40_few.hip): its launch
// plan, the one place that derives column tiles, K-slices, threads, grid and LDS bytes, and what llamahip_op_mul_mat_q4_0_few (ops.cpp)
// refuses of its arguments.  Pure host code, no device: tools/host_sanitize runs it under ASan + UBSan.
#include <stdio.h>

#include "q40_few_plan.h"

namespace lh {

long g_q40_few_launches = 0;

// nt = column tiles of 16 activation rows against ONE unpacking of the weights (1 .. 4: every row count up to 63 is one launch and one
// pass over the weights).  What orders an output's sums -- the slice count and the chunks of a slice -- follows (M, K) alone.
Q40FewPlan q40_few_plan(int M, int K, int N) {
    Q40FewPlan p = { 0, 0, 0, 0, 0, 0 };
    if (M < 1 || K < 32 || K % 32 != 0 || N < 1 || N > Q40_FEW_MAX_ROWS) return p;
    p.nt = (N + Q40_FEW_TILE - 1) / Q40_FEW_TILE;
    p.slices = q40_few_slices(M);
    p.threads = 64 * p.slices;
    p.grid = (int) (((long) M + Q40_FEW_ROWS - 1) / Q40_FEW_ROWS);
    p.lds = q40_few_lds(p.nt);
    p.ok = 1;
    return p;
}

int q40_few_op_check(const void *w, int32_t M, int32_t K, const float *x, int32_t N, const float *y, int32_t y_stride, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_mul_mat_q4_0_few";
    if (!err) err_cap = 0;
    if (K < 32 || K % 32 != 0) { snprintf(err, err_cap, "%s: K %d must be a positive multiple of 32", fn, K); return -1; }
    if (N < 1 || N > Q40_FEW_MAX_ROWS) { snprintf(err, err_cap, "%s: N %d outside 1 .. %d rows", fn, N, Q40_FEW_MAX_ROWS); return -1; }
    if (M < 1) { snprintf(err, err_cap, "%s: M %d must be >= 1", fn, M); return -1; }
    if (y_stride < M) { snprintf(err, err_cap, "%s: y_stride %d < M %d", fn, y_stride, M); return -1; }
    if (!w || !x || !y) { snprintf(err, err_cap, "%s: bad arguments (w_q4_0, x, y not NULL)", fn); return -1; }
    return 0;
}

}  // namespace lh
