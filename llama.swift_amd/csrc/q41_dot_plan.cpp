// q41_dot_plan.cpp -- the host half of the opt-in integer-dot Q4_1 mat-mul k_q41_dot (q41_dot.hip): its launch plan, the one
// place that derives instance, threads, grid, slab and LDS bytes, and what llamahip_op_mul_mat_q4_1_dot (ops.cpp) refuses of its arguments.
// Pure host code, no device: tools/host_sanitize runs it under ASan + UBSan.
#include <stdio.h>

#include <algorithm>

#include "q41_plan.h"

namespace lh {

long g_q41_dot_launches = 0;

// nr = the compiled instance for a tile of N rows (N > 16: the full tiles of 16 on gridDim.y; the last tile of N % 16 rows is a launch of
// its own on q41_dot_plan(M, K, N % 16)) -- k_q41_chain's instances.  Everything that decides the order of an output's sums is a constant:
// 16 weight rows per workgroup (the narrowest 7B matrix is then 256 workgroups, one per CU) and 16 K-lanes.  Only nr, the slab that is
// staged together (q41_dot_slab), the LDS bytes (two record buffers of nr x slab x 32 bytes: 4 KiB at one row, 16 KiB at 4, 8 and 16 rows) and grid_y
// follow N.
Q41DotPlan q41_dot_plan(int M, int K, int N) {
    Q41DotPlan p = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (M < 1 || K < 32 || K % 32 != 0 || N < 1 || (N + Q41_DOT_TILE - 1) / Q41_DOT_TILE > 65535) return p;
    const int rows = std::min(N, Q41_DOT_TILE);
    p.nr = rows <= 2 ? rows : rows <= 4 ? 4 : rows <= 8 ? 8 : rows <= 12 ? 12 : 16;
    p.threads = Q41_DOT_ROWS * Q41_DOT_KLANES;
    p.grid_x = (int) (((long) M + Q41_DOT_ROWS - 1) / Q41_DOT_ROWS);
    p.grid_y = (N + Q41_DOT_TILE - 1) / Q41_DOT_TILE;
    p.klanes = Q41_DOT_KLANES;
    p.slab = q41_dot_slab(p.nr);
    p.lds = 2 * p.nr * p.slab * 32;
    p.ok = 1;
    return p;
}

int q41_dot_op_check(const void *w, int32_t M, int32_t K, const float *x, int32_t N, const float *y, int32_t y_stride, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_mul_mat_q4_1_dot";
    if (!err) err_cap = 0;
    if (K < 32 || K % 32 != 0) { snprintf(err, err_cap, "%s: K %d must be a positive multiple of 32", fn, K); return -1; }
    if (N < 1) { snprintf(err, err_cap, "%s: N %d must be >= 1", fn, N); return -1; }
    if (M < 1) { snprintf(err, err_cap, "%s: M %d must be >= 1", fn, M); return -1; }
    if (y_stride < M) { snprintf(err, err_cap, "%s: y_stride %d < M %d", fn, y_stride, M); return -1; }
    if (!w || !x || !y) { snprintf(err, err_cap, "%s: bad arguments (w_q4_1, x, y not NULL)", fn); return -1; }
    if (!q41_dot_plan(M, K, N).ok) { snprintf(err, err_cap, "%s: N %d is more than 65535 row tiles of 16", fn, N); return -1; }
    return 0;
}

}  // namespace lh
