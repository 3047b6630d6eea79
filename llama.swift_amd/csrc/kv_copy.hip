// kv_copy.hip -- k_kv_copy_rows: finished KV rows moved from one slot of a handle's cache to the same rows of another
// (llamahip_kv_copy_rows; the request scheduler's shared prompt prefixes, include/llamahip.h).
//
// The cache of a handle or stage is two fp32 arrays [slot][layer][n_ctx][n_embd].  One launch takes a table of at most KV_COPY_MAX copies
// {source slot, destination slot, first row, row count}, by value in the kernel arguments, and moves that row range of EVERY local layer, K
// and V, to the same rows of the destination slot: a K row carries its position's rotation, so the row index never changes.
// Per copy, layer and array the range is one contiguous RUN of rows * n_embd * 4 bytes, a multiple of 16 (n_embd is a multiple of 4; the
// launcher checks it and the arrays' alignment).  A run is cut into TILES of KV_COPY_TILE 16-byte granules; the tiles of all runs are
// numbered copy-major, and the workgroups walk that numbering grid-strided (the grid is capped at KV_COPY_GRID_MAX workgroups).  A thread
// moves KV_COPY_UNROLL granules of a tile, 256 granules apart, all loads issued before the first store: a wave has KV_COPY_UNROLL
// independent 1 KiB loads in flight.  Plain vector loads and stores only; a tile's last granules are masked by the run's length.
// Source and destination slots of one launch never coincide (the launcher refuses a table in which a destination is anybody's source or
// another copy's destination), so no granule is read and written by the same launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kcommon.hip.h"
#include "llamahip_internal.h"

namespace lh {

constexpr int KV_COPY_THREADS = 256, KV_COPY_UNROLL = 4, KV_COPY_TILE = KV_COPY_THREADS * KV_COPY_UNROLL, KV_COPY_GRID_MAX = 2048;

// tiles of one run of copy c (uniform over the launch); 0 for an empty copy
__host__ __device__ static inline long kv_copy_run_tiles(const KvCopyTab &tab, int c, int d) {
    return ((long) tab.n_rows[c] * (d / 4) + KV_COPY_TILE - 1) / KV_COPY_TILE;
}

__global__ void __launch_bounds__(KV_COPY_THREADS)
k_kv_copy_rows(float *Kc, float *Vc, const KvCopyTab tab, int n_layers, int n_ctx, int d, long n_tiles) {
    const long layer_f4 = (long) n_ctx * (d / 4), slot_f4 = layer_f4 * n_layers;      // 16-byte granules per layer / per slot
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        // tile t -> (copy c, run r = 2 * layer + {K, V}, tile k of the run): a scalar walk over at most KV_COPY_MAX copies
        long rest = t, per_run = 0;
        int c = 0;
        for (; c < tab.n; c++) {
            per_run = kv_copy_run_tiles(tab, c, d);
            const long of_copy = per_run * 2 * n_layers;
            if (rest < of_copy) break;
            rest -= of_copy;
        }
        if (c >= tab.n) return;                                    // (n_tiles is the launcher's sum of the same terms)
        const int r = (int) (rest / per_run);
        const long k = rest % per_run;
        const long run_f4 = (long) tab.n_rows[c] * (d / 4);
        const long in_slot = (long) (r >> 1) * layer_f4 + (long) tab.row_begin[c] * (d / 4);
        float4 *base = reinterpret_cast<float4 *>((r & 1) ? Vc : Kc);
        const float4 *src = base + (long) tab.src[c] * slot_f4 + in_slot;
        float4 *dst = base + (long) tab.dst[c] * slot_f4 + in_slot;
        const long i0 = k * KV_COPY_TILE + threadIdx.x;
        float4 v[KV_COPY_UNROLL];
#pragma unroll
        for (int u = 0; u < KV_COPY_UNROLL; u++) {
            const long i = i0 + (long) u * KV_COPY_THREADS;
            if (i < run_f4) v[u] = src[i];
        }
#pragma unroll
        for (int u = 0; u < KV_COPY_UNROLL; u++) {
            const long i = i0 + (long) u * KV_COPY_THREADS;
            if (i < run_f4) dst[i] = v[u];
        }
    }
}

hipError_t launch_kv_copy_rows(float *Kc, float *Vc, const KvCopyTab &tab, int n_slots, int n_layers, int n_ctx, int d, hipStream_t st) {
    if (!Kc || !Vc || n_slots < 1 || n_layers < 1 || n_ctx < 1 || d < 4 || d % 4 != 0 || tab.n < 1 || tab.n > KV_COPY_MAX) return hipErrorInvalidValue;
    if (((uintptr_t) Kc | (uintptr_t) Vc) & 15) return hipErrorInvalidValue;
    long n_tiles = 0;
    for (int c = 0; c < tab.n; c++) {
        // every range inside the cache, no slot both written and read (or written twice) by this launch
        if (tab.src[c] < 0 || tab.src[c] >= n_slots || tab.dst[c] < 0 || tab.dst[c] >= n_slots || tab.src[c] == tab.dst[c]) return hipErrorInvalidValue;
        if (tab.n_rows[c] < 0 || tab.row_begin[c] < 0 || (long) tab.row_begin[c] + tab.n_rows[c] > n_ctx) return hipErrorInvalidValue;
        for (int o = 0; o < tab.n; o++)
            if (o != c && (tab.dst[c] == tab.src[o] || tab.dst[c] == tab.dst[o])) return hipErrorInvalidValue;
        n_tiles += kv_copy_run_tiles(tab, c, d) * 2 * n_layers;
    }
    if (n_tiles == 0) return hipSuccess;          // nothing but empty copies
    const unsigned grid = (unsigned) (n_tiles < KV_COPY_GRID_MAX ? n_tiles : KV_COPY_GRID_MAX);
    hipLaunchKernelGGL(k_kv_copy_rows, dim3(grid), dim3(KV_COPY_THREADS), 0, st, Kc, Vc, tab, n_layers, n_ctx, d, n_tiles);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace lh
