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

}  // namespace lh
