// q41_plan.h -- the host-only half of the Q4_1 mat-mul (q41_plan.cpp): the launch plan of k_q41_chain (dense.hip) and the argument check of
// llamahip_op_mul_mat_q4_1 (ops.cpp).  No device header: tools/host_sanitize.cpp compiles it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lh {

// The Q4_1 mat-mul kernels, = LLAMAHIP_Q41_* of llamahip.h: k_q41_chain (product waves park the pair terms of up to 16 activation rows in LDS,
// one chain lane per output adds them in pair order: what AUTO and every model handle run) and k_q41_mm (a lane per weight row, one
// activation row per workgroup: the op entry point's LANE only).  Both read the same load-time copy and give the same bits.
enum { Q41_PATH_AUTO = 0, Q41_PATH_CHAIN = 1, Q41_PATH_LANE = 2 };
enum { Q41_COUNT_CHAIN = 0, Q41_COUNT_LANE = 1, Q41_COUNT_N = 2 };
extern long g_q41_path_counts[Q41_COUNT_N];         // mat-muls per kernel (process-wide; tests)

constexpr int Q41_R = 16;              // weight rows per workgroup: a quarter of the load-time copy's 64-row block
constexpr int Q41_TILE = 16;           // activation rows per row tile (gridDim.y) at most
#define LH_Q41_INSTANCES(X) X(1) X(2) X(4) X(8) X(12) X(16)      // the compiled NR (q41_plan rounds a tile's rows up to one of them)

// byte pairs per slab of the instance of nr rows: as long as two term buffers of it fit in 64 KiB, so that two workgroups share a CU
// (from 12 rows on that is 32 pairs: the product threads then split the activation rows of a word between them)
constexpr int q41_slab_pairs(int nr) { return nr <= 2 ? 256 : nr <= 4 ? 128 : nr <= 8 ? 64 : 32; }
// product threads (the chain lanes follow them in whole waves): 16 rows x 16 word slots, or 16 rows x 8 word slots x 2 halves of the rows
constexpr int q41_prod_threads(int) { return 256; }
// k_q41_chain's launch plan: nr = the compiled row count of a tile (0: bad shape), rows = weight rows per workgroup, threads, grid_x x grid_y
// workgroups (grid_y row tiles of at most 16; a last tile of N % 16 rows is launched on the plan of that row count), slab = byte pairs per
// term buffer, lds = dynamic LDS bytes (two term buffers of slab x chain floats and two activation slabs of nr x 2 slab floats), chain = chain lanes per workgroup
struct Q41Plan { int nr, rows, threads, grid_x, grid_y, slab, lds, chain; };
Q41Plan q41_plan(int M, int K, int N);
bool q41_plan_has_kernel(const Q41Plan &p);

// llamahip_op_mul_mat_q4_1's refusals, before any device is touched: 0, or -1 with the limit named in err
int q41_op_check(const void *w, int32_t M, int32_t K, const float *x, int32_t N, const float *y, int32_t y_stride, int32_t path, char *err, size_t err_cap);

// k_q41_fast (q41_fast.hip; plan: q41_fast_plan.cpp): the opt-in fp16 matrix-core mat-mul of Q4_1 files, LLAMAHIP_FLAG_FAST_Q41 handles' evals of
// >= Q41_FAST_MIN_ROWS rows and llamahip_op_mul_mat_q4_1_fast.  NOT the reference's arithmetic.  The plan: ok = the kernel takes the shape;
// grid (grid_x, grid_y) workgroups of 256 threads, each tile_rows activation rows x tile_cols weight rows, K in tiles of k_tile; lds = dynamic
// LDS bytes
struct Q41FastPlan { int ok, grid_x, grid_y, tile_rows, tile_cols, k_tile, lds; };
constexpr int Q41_FAST_MIN_ROWS = 64;                // the flag's row threshold
Q41FastPlan q41_fast_plan(int M, int K, int N);
extern long g_q41_fast_launches;                     // launches of k_q41_fast (process-wide; tests)
// llamahip_op_mul_mat_q4_1_fast's refusals, before any device is touched: 0, or -1 with the limit named in err
int q41_fast_op_check(const void *w, int32_t M, int32_t K, const float *x, int32_t N, const float *y, int32_t y_stride, char *err, size_t err_cap);

// k_q41_dot (q41_dot.hip; plan: q41_dot_plan.cpp): the opt-in integer-dot mat-mul of Q4_1 files, LLAMAHIP_FLAG_FAST_Q41_DECODE handles' decode
// steps and evals below Q41_FAST_MIN_ROWS rows, and llamahip_op_mul_mat_q4_1_dot.  NOT the reference's arithmetic.  The plan: ok = the kernel
// takes the shape; nr = the compiled row count of a tile (LH_Q41_INSTANCES); grid (grid_x, grid_y) workgroups of `threads` threads, each
// Q41_DOT_ROWS weight rows x klanes K-lanes (K-lane l adds the terms of blocks l, l + klanes, ... in that order); grid_y row tiles of at
// most Q41_DOT_TILE (a last tile of N % 16 rows is launched on the plan of that row count); slab = blocks whose activation records are
// staged in LDS at a time (it follows nr and orders no sum); lds = static LDS bytes.  grid_x and klanes do not depend on N: the bits of a
// row do not either.
struct Q41DotPlan { int ok, nr, threads, grid_x, grid_y, klanes, slab, lds; };
constexpr int Q41_DOT_ROWS = 16, Q41_DOT_KLANES = 16, Q41_DOT_TILE = 16;
// blocks per LDS slab of the instance of nr rows (whole walks of the 16 K-lanes): how much of the next slab a thread holds in registers --
// sized so that no instance parks registers in AGPRs or scratch and every one keeps two waves per SIMD or more
constexpr int q41_dot_slab(int nr) { return nr <= 4 ? 64 : nr <= 8 ? 32 : 16; }
Q41DotPlan q41_dot_plan(int M, int K, int N);
extern long g_q41_dot_launches;                      // mat-muls on k_q41_dot (process-wide; tests)
// llamahip_op_mul_mat_q4_1_dot's refusals, before any device is touched: 0, or -1 with the limit named in err
int q41_dot_op_check(const void *w, int32_t M, int32_t K, const float *x, int32_t N, const float *y, int32_t y_stride, char *err, size_t err_cap);

}  // namespace lh
