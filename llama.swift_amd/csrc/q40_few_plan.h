// q40_few_plan.h -- the host-only half of the opt-in int8 matrix-core few-row mat-mul of Q4_0 files k_q40_few (q40_few.hip, DESIGN.md 12.39;
// plan: q40_few_plan.cpp): its launch plan and what llamahip_op_mul_mat_q4_0_few refuses of its arguments.  No device header:
// tools/host_sanitize.cpp compiles it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lh {

// k_q40_few: LLAMAHIP_FLAG_FAST_Q40_FEW handles' mat-muls of Q40_FEW_MIN_ROWS .. Q40_FEW_MAX_ROWS rows, and llamahip_op_mul_mat_q4_0_few
// (1 .. Q40_FEW_MAX_ROWS).  NOT the reference's arithmetic.  The plan: ok = the kernel takes the shape; a grid of `grid` workgroups of
// `threads` = 64 * slices threads, each Q40_FEW_ROWS weight rows (two row-groups of the chain-major tile copy) against nt column tiles of
// 16 activation rows; wave s of a workgroup is K-slice s: the chunks (256 elements) s, s + slices, s + 2 slices, ... in that order, the
// slices added 0, 1, 2, ... in LDS.  slices follows (M, K) alone -- never N --, so the bits of a row do not follow the rows around it.
// lds = static LDS bytes of the instance (the slices' partial tiles and one scale tile per wave).
struct Q40FewPlan { int ok, nt, slices, threads, grid, lds; };
constexpr int Q40_FEW_ROWS = 16, Q40_FEW_TILE = 16, Q40_FEW_MAX_NT = 4;
// the handle's gate (launch_gemm): 16 .. 63 rows.  2 .. 15 rows went back to the exact kernels by the give-back rule (7B, DESIGN.md 12.39: set
// steps of 2 / 4 / 8 sequences measured 38 / 25 / 5 % slower than k_gemv_set's fused schedule); the op takes 1 .. 63
constexpr int Q40_FEW_MIN_ROWS = 16, Q40_FEW_MAX_ROWS = 63;
constexpr int Q40_FEW_MAX_SLICES = 8;
// 8 K-slices where 16-row workgroups alone leave CUs short of two waves per SIMD (up to 512 workgroups: the 4096-row matrices of the 7B
// file are 256), 4 above
constexpr int q40_few_slices(int M) { return (M + Q40_FEW_ROWS - 1) / Q40_FEW_ROWS <= 512 ? 8 : 4; }
constexpr int q40_few_lds(int nt) { return Q40_FEW_MAX_SLICES * (nt * 1024 + 512); }
Q40FewPlan q40_few_plan(int M, int K, int N);
extern long g_q40_few_launches;                      // launches of k_q40_few (process-wide; tests)
// llamahip_op_mul_mat_q4_0_few's refusals, before any device is touched: 0, or -1 with the limit named in err
int q40_few_op_check(const void *w, int32_t M, int32_t K, const float *x, int32_t N, const float *y, int32_t y_stride, char *err, size_t err_cap);

}  // namespace lh
