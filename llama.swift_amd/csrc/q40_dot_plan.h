// q40_dot_plan.h -- the host-only half of the opt-in K-split integer-dot mat-vec of Q4_0 files k_q40_dot (q40_dot.hip; plan:
// q40_dot_plan.cpp): its launch plan and what llamahip_op_gemv_q4_0_dot refuses of its arguments.  No device header:
// tools/host_sanitize.cpp compiles it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lh {

// k_q40_dot: wo and w2 of the single-token decode step on llamahip_opts.fast_decode = 1 handles, and llamahip_op_gemv_q4_0_dot.  NOT the
// reference's arithmetic (k_q40_few's, at one row).  The plan: ok = the kernel takes the shape; a grid of `grid` workgroups of `threads` =
// 64 * slices threads, each Q40_DOT_ROWS weight rows (two row-groups of the chain-major tile copy); wave s of a workgroup is K-slice s: the
// chunks (256 elements) s, s + slices, s + 2 slices, ... in that order, the slices added 0, 1, 2, ... in LDS.  slices follows (M, K) alone.
// lds = dynamic LDS bytes: the activation row's codes and scales (288 bytes per chunk) and the slices' partial outputs.
// applies = ok, and the decode step takes the kernel for this matrix: its grid fits the norm statistics hand-off (one {sum, sum of squares}
// pair per workgroup, at most Q40_DOT_MAX_PARTS = NORM_PART_MAX) and the measured rule keeps it (q40_dot_plan.cpp): fewer than
// Q40_DOT_GIVE_BACK_ROWS weight rows -- the 7B matrices measured SLOWER than k_gemv, so no LLaMA width takes the kernel.
struct Q40DotPlan { int ok, slices, threads, grid, lds, applies; };
constexpr int Q40_DOT_ROWS = 16;
constexpr int Q40_DOT_MAX_SLICES = 8;
constexpr int Q40_DOT_MAX_PARTS = 512;
constexpr int Q40_DOT_MAX_LDS = 48 * 1024;
constexpr int Q40_DOT_GIVE_BACK_ROWS = 4096;
// 8 K-slices up to 8192 weight rows (the 4096-row matrices of the 7B file are 256 workgroups: one per CU, two waves per SIMD where the exact
// kernel has a half), 4 above -- k_q40_few's rule, so that the two kernels state one arithmetic
constexpr int q40_dot_slices(int M) { return (M + Q40_DOT_ROWS - 1) / Q40_DOT_ROWS <= 512 ? 8 : 4; }
constexpr int q40_dot_lds(int nchunks) { return nchunks * 288 + Q40_DOT_MAX_SLICES * Q40_DOT_ROWS * 4; }
Q40DotPlan q40_dot_plan(int M, int K);
extern long g_q40_dot_launches;                      // launches of k_q40_dot (process-wide; tests)
// llamahip_op_gemv_q4_0_dot's refusals, before any device is touched: 0, or -1 with the limit named in err
int q40_dot_op_check(const void *w, int32_t M, int32_t K, const float *x, const float *y, int32_t y_cap, const double *parts, int32_t parts_cap,
                     char *err, size_t err_cap);

}  // namespace lh
