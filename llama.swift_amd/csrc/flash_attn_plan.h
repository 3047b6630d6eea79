// flash_attn_plan.h -- the host-only half of the opt-in fused prompt attention k_flash_attn (flash_attn.hip, LLAMAHIP_FLAG_FAST_ATTN): which
// query tile and how many key splits a launch takes, its grid, LDS and workspace bytes.  No device header: tools/host_sanitize.cpp can compile it.
#pragma once
#include <stddef.h>

namespace lh {

constexpr int FLASH_HEAD = 128;                      // the head size the kernel takes
constexpr int FLASH_KEY_TILE = 64;                   // keys per LDS tile
constexpr int FLASH_KS_CAP = 8;                      // key splits at most
constexpr int FLASH_CUS = 256;                       // workgroups the plan wants at least (one per CU of an MI355X)
// K [64][128 + 8] and V transposed [128][64 + 8] halves, two buffers
constexpr int FLASH_LDS_BYTES = 2 * (FLASH_KEY_TILE * (FLASH_HEAD + 8) + FLASH_HEAD * (FLASH_KEY_TILE + 8)) * 2;
// un-normalised O rows plus {m, l} per (split, head, query)
constexpr size_t FLASH_WS_ROW_FLOATS = FLASH_HEAD + 2;
// what a handle allocates once: the plan splits only while KS * H * ceil(N / 64) < 2 * FLASH_CUS (flash_attn_plan.cpp), rows of 64 queries
constexpr size_t FLASH_WS_CAP_BYTES = (size_t) 2 * FLASH_CUS * 64 * FLASH_WS_ROW_FLOATS * 4;

// ok = the kernel takes the shape; tile: queries per workgroup (128 or 64); ks: key splits (1: the kernel writes merged itself, no combine);
// grid (ceil(N / tile), H, ks) workgroups of 256 threads; ws_bytes: the workspace the splits need (0 at ks 1)
struct FlashAttnPlan { int ok, tile, ks, grid_x, grid_y, grid_z, lds; size_t ws_bytes; };
// N query rows at positions T - N .. T - 1 (T = n_past + N keys in all), H heads of 128.  tile / ks 0: the rule's choice; else as asked, or ok = 0
FlashAttnPlan flash_attn_plan(int N, int T, int H, int tile = 0, int ks = 0);

}  // namespace lh
