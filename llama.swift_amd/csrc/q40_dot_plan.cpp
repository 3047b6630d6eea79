// q40_dot_plan.cpp -- the host half of the opt-in K-split integer-dot mat-vec k_q40_dot (q40_dot.hip): its launch plan, the
// one place that derives K-slices, threads, grid and LDS bytes and that says which matrices of the decode step take the kernel, and what
// llamahip_op_gemv_q4_0_dot (ops.cpp) refuses of its arguments.  Pure host code, no device: tools/host_sanitize runs it under ASan + UBSan.
#include <stdio.h>

#include "q40_dot_plan.h"

namespace lh {

long g_q40_dot_launches = 0;

// What orders an output's sums -- the slice count and the chunks of a slice -- follows (M, K) alone.
// applies: a grid above Q40_DOT_MAX_PARTS cannot hand its statistics to the next launch's prologue, and the give-back rule of DESIGN.md
// 12.15 / 12.36 -- a matrix keeps the kernel only where its slowest of five processes beat the exact kernel's fastest.  Both 7B matrices
// LOST (in situ, 12.40: wo 4096 x 4096 6.28 us against k_gemv's 4.85, w2 4096 x 11008 9.18 against 7.47; decode 1.401 against 1.296 ms per
// token), and from 4096 rows on k_gemv only gains waves per workgroup: matrices of Q40_DOT_GIVE_BACK_ROWS rows and more stay on k_gemv --
// every LLaMA width.  Narrower matrices keep the kernel; they were NOT measured.
Q40DotPlan q40_dot_plan(int M, int K) {
    Q40DotPlan p = { 0, 0, 0, 0, 0, 0 };
    if (M < 1 || K < 32 || K % 32 != 0) return p;
    const int nchunks = (K + 255) / 256;
    if (q40_dot_lds(nchunks) > Q40_DOT_MAX_LDS) return p;
    p.slices = q40_dot_slices(M);
    p.threads = 64 * p.slices;
    p.grid = (int) (((long) M + Q40_DOT_ROWS - 1) / Q40_DOT_ROWS);
    p.lds = q40_dot_lds(nchunks);
    p.ok = 1;
    p.applies = p.grid <= Q40_DOT_MAX_PARTS && M < Q40_DOT_GIVE_BACK_ROWS;
    return p;
}

int q40_dot_op_check(const void *w, int32_t M, int32_t K, const float *x, const float *y, int32_t y_cap, const double *parts, int32_t parts_cap,
                     char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_gemv_q4_0_dot";
    if (!err) err_cap = 0;
    if (K < 32 || K % 32 != 0) { snprintf(err, err_cap, "%s: K %d must be a positive multiple of 32", fn, K); return -1; }
    if (M < 1) { snprintf(err, err_cap, "%s: M %d must be >= 1", fn, M); return -1; }
    if (!w || !x || !y || !parts) { snprintf(err, err_cap, "%s: bad arguments (w_q4_0, x, y, parts not NULL)", fn); return -1; }
    if (y_cap < M) { snprintf(err, err_cap, "%s: y_cap %d < M %d", fn, y_cap, M); return -1; }
    const Q40DotPlan p = q40_dot_plan(M, K);
    if (!p.ok) { snprintf(err, err_cap, "%s: K %d needs more than %d bytes of LDS for the activation row", fn, K, Q40_DOT_MAX_LDS); return -1; }
    if (parts_cap < p.grid) { snprintf(err, err_cap, "%s: parts_cap %d < %d pairs (one per workgroup of 16 rows: llamahip_debug_q40_dot_plan)", fn, parts_cap, p.grid); return -1; }
    return 0;
}

}  // namespace lh
