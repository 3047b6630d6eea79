// q41_fast_plan.cpp -- the host half of the opt-in fp16 matrix-core Q4_1 mat-mul k_q41_fast (q41_fast.hip): its launch plan,
// the one place that derives instance, grid and LDS bytes, and what llamahip_op_mul_mat_q4_1_fast (ops.cpp) refuses of its arguments.  Pure
// host code, no device: tools/host_sanitize runs it under ASan + UBSan.
#include <stdio.h>

#include "q41_plan.h"

namespace lh {

long g_q41_fast_launches = 0;

// Three instances: wide 128 x 128 (K tile 64), mid 64 x 64 (K tile 128), narrow 64 x 16 (K tile 256) -- activation rows x weight rows.  A
// weight tile of 16, 64 or 128 rows is a quarter, one or two of the load-time copy's 64-row blocks.  Unlike k_dense_f16_fast, whose short
// evals race for HBM bytes in flight, this kernel pays a dequantisation (about 5 VALU operations per weight and workgroup) whatever the
// tile: every weight is expanded once per ROW tile, so the wide tile halves that work and is taken wherever it fills the 256 CUs, and
// mid and narrow, which expand the same amount, differ only in how many CUs share it -- mid where it makes a workgroup for every CU,
// else narrow.  The five 7B matrices against 64 rows: wq|wk|wv 768 narrow, wo 256 narrow, w1|w3 344 mid, w2 256 narrow, lm head 500 mid
// workgroups -- none below one per CU.
Q41FastPlan q41_fast_plan(int M, int K, int N) {
    Q41FastPlan p = { 0, 0, 0, 0, 0, 0, 0 };
    if (M < 1 || K < 32 || K % 32 != 0 || N < 1) return p;
    auto wgs = [&](int tn, int tm) { return (long) ((N + tn - 1) / tn) * ((M + tm - 1) / tm); };
    if (wgs(128, 128) >= 256)    { p.tile_rows = 128; p.tile_cols = 128; p.k_tile = 64; }
    else if (wgs(64, 64) >= 256) { p.tile_rows = 64;  p.tile_cols = 64;  p.k_tile = 128; }
    else                         { p.tile_rows = 64;  p.tile_cols = 16;  p.k_tile = 256; }
    p.grid_x = (N + p.tile_rows - 1) / p.tile_rows;
    p.grid_y = (M + p.tile_cols - 1) / p.tile_cols;
    if (p.grid_y > 65535) return p;
    p.lds = 2 * (p.tile_rows + p.tile_cols) * (p.k_tile + 8) * 2;
    p.ok = 1;
    return p;
}

int q41_fast_op_check(const void *w, int32_t M, int32_t K, const float *x, int32_t N, const float *y, int32_t y_stride, char *err, size_t err_cap) {
    static const char *fn = "llamahip_op_mul_mat_q4_1_fast";
    if (!err) err_cap = 0;
    if (K < 32 || K % 32 != 0) { snprintf(err, err_cap, "%s: K %d must be a positive multiple of 32", fn, K); return -1; }
    if (N < 1) { snprintf(err, err_cap, "%s: N %d must be >= 1", fn, N); return -1; }
    if (M < 1) { snprintf(err, err_cap, "%s: M %d must be >= 1", fn, M); return -1; }
    if (y_stride < M) { snprintf(err, err_cap, "%s: y_stride %d < M %d", fn, y_stride, M); return -1; }
    if (!w || !x || !y) { snprintf(err, err_cap, "%s: bad arguments (w_q4_1, x, y not NULL)", fn); return -1; }
    if (!q41_fast_plan(M, K, N).ok) { snprintf(err, err_cap, "%s: M %d makes more than 65535 rows of workgroups", fn, M); return -1; }
    return 0;
}

}  // namespace lh
