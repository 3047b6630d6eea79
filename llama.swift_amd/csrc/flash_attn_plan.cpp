// flash_attn_plan.cpp -- the launch plan of k_flash_attn (flash_attn.hip), the one place that derives it.  Host only.
#include "flash_attn_plan.h"

namespace lh {

// The rule.  A wider query tile re-reads K and V less (a workgroup streams every visible key once for `tile` queries) and feeds two matrix
// instructions from every LDS operand read, but makes fewer workgroups: take the 128-query tile where it still makes a workgroup for every
// CU, else the 64-query tile.  Where even that leaves CUs idle (a 64-row chunk at 7B: 32 workgroups), split the visible key tiles over the
// smallest number of workgroups per (head, query tile) that fills the chip -- every split costs a pass of k_flash_combine over its
// un-normalised rows, so no more than that -- capped by the key tiles there are and by FLASH_KS_CAP.
FlashAttnPlan flash_attn_plan(int N, int T, int H, int tile, int ks) {
    FlashAttnPlan p = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (N < 2 || T < N || H < 1 || H > 65535) return p;
    if (tile != 0 && tile != 64 && tile != 128) return p;
    const int key_tiles = (T + FLASH_KEY_TILE - 1) / FLASH_KEY_TILE;
    if (ks < 0 || ks > FLASH_KS_CAP) return p;
    auto wgs = [&](int t) { return (long) H * ((N + t - 1) / t); };
    p.tile = tile ? tile : wgs(128) >= FLASH_CUS ? 128 : 64;
    if (ks) p.ks = ks;
    else {
        const long w = wgs(p.tile);
        long want = w >= FLASH_CUS ? 1 : (FLASH_CUS + w - 1) / w;
        if (want > key_tiles) want = key_tiles;
        if (want > FLASH_KS_CAP) want = FLASH_KS_CAP;
        p.ks = (int) want;
    }
    p.grid_x = (N + p.tile - 1) / p.tile;
    p.grid_y = H;
    p.grid_z = p.ks;
    p.lds = FLASH_LDS_BYTES;
    p.ws_bytes = p.ks > 1 ? (size_t) p.ks * H * N * FLASH_WS_ROW_FLOATS * 4 : 0;
    p.ok = 1;
    return p;
}

}  // namespace lh
