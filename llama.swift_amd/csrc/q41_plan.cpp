// q41_plan.cpp -- the host half of the Q4_1 mat-mul: the launch plan of k_q41_chain (dense.hip), the one place that derives it, and what
// llamahip_op_mul_mat_q4_1 (ops.cpp) refuses of its arguments.  Pure host code, no device: tools/host_sanitize runs it under ASan + UBSan.
#include <stdio.h>

#include <algorithm>

#include "../../include/llamahip.h"
#include "q41_plan.h"

namespace lh {

static_assert(LLAMAHIP_Q41_AUTO == Q41_PATH_AUTO && LLAMAHIP_Q41_CHAIN == Q41_PATH_CHAIN && LLAMAHIP_Q41_LANE == Q41_PATH_LANE, "llamahip.h mirrors the Q4_1 mat-mul paths");

long g_q41_path_counts[Q41_COUNT_N] = { 0, 0 };

// nr = the compiled instance for a tile of N rows (N > 16: the full tiles of 16; the last tile of N % 16 rows is a launch of its own on
// q41_plan(M, K, N % 16)).  Q41_R = 16 weight rows per workgroup: the narrowest 7B matrix (4096 rows) is then 256 workgroups, one per CU, at
// any row count.  The slab is q41_slab_pairs(nr) (q41_plan.h); LDS holds two term buffers and two activation slabs of it: 34 KiB at one
// row, 72 KiB at 16.  Chain lanes = 16 * nr, in whole waves behind the 4 product waves.
Q41Plan q41_plan(int M, int K, int N) {
    Q41Plan p = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (M < 1 || K < 32 || K % 32 != 0 || N < 1 || (N + Q41_TILE - 1) / Q41_TILE > 65535) return p;
    const int rows = std::min(N, Q41_TILE);
    p.nr = rows <= 2 ? rows : rows <= 4 ? 4 : rows <= 8 ? 8 : rows <= 12 ? 12 : 16;
    p.rows = Q41_R;
    p.chain = Q41_R * p.nr;
    p.threads = q41_prod_threads(p.nr) + (p.chain + 63) / 64 * 64;
    p.grid_x = (M + Q41_R - 1) / Q41_R;
    p.grid_y = (N + Q41_TILE - 1) / Q41_TILE;
    p.slab = q41_slab_pairs(p.nr);
    p.lds = 2 * p.slab * 4 * (p.chain + 2 * p.nr);
    return p;
}

bool q41_plan_has_kernel(const Q41Plan &p) {
    bool nr = false;
#define LH_IS(NR) nr = nr || p.nr == NR;
    LH_Q41_INSTANCES(LH_IS)
#undef LH_IS
    // (the kernel takes slabs of two blocks of 16 pairs, or of whole groups of 4 blocks; only a matrix's last slab may be shorter)
    return nr && p.rows == Q41_R && p.chain == Q41_R * p.nr && p.threads == q41_prod_threads(p.nr) + (p.chain + 63) / 64 * 64 && p.threads <= 1024
        && p.slab == q41_slab_pairs(p.nr) && p.slab % 32 == 0 && p.lds == 2 * p.slab * 4 * (p.chain + 2 * p.nr) && p.lds <= 160 * 1024 && p.grid_x >= 1 && p.grid_y >= 1;
}

int q41_op_check(const void *w, int32_t M, int32_t K, const float *x, int32_t N, const float *y, int32_t y_stride, int32_t path, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_mul_mat_q4_1";
    if (!err) err_cap = 0;
    if (K < 32 || K % 32 != 0) { snprintf(err, err_cap, "%s: K %d must be a positive multiple of 32", fn, K); return -1; }
    if (path < Q41_PATH_AUTO || path > Q41_PATH_LANE) { snprintf(err, err_cap, "%s: unknown path %d", fn, path); return -1; }
    if (N < 1) { snprintf(err, err_cap, "%s: N %d must be >= 1", fn, N); return -1; }
    if (M < 1) { snprintf(err, err_cap, "%s: M %d must be >= 1", fn, M); return -1; }
    if (y_stride < M) { snprintf(err, err_cap, "%s: y_stride %d < M %d", fn, y_stride, M); return -1; }
    if (!w || !x || !y) { snprintf(err, err_cap, "%s: bad arguments (w_q4_1, x, y not NULL)", fn); return -1; }
    if (!q41_plan(M, K, N).nr) { snprintf(err, err_cap, "%s: N %d is more than 65535 row tiles of 16", fn, N); return -1; }
    return 0;
}

}  // namespace lh
