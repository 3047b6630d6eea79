// kv_shift.hip -- k_kv_shift_rows: KV rows of a slot moved DOWN by n_discard positions in place, every key re-rotated by -n_discard
// positions (llamahip_kv_shift_rows; LLAMAHIP_CTX_SHIFT, the in-place way across the end of the context: include/llamahip.h).
// NOT the reference's arithmetic: a moved key is narrowed to fp32 a second time.  What the kernel computes is defined here, bit for bit.
//
// The cache of a handle or stage is two fp32 arrays [slot][layer][n_ctx][n_embd].  One launch takes a table of at most KV_SHIFT_MAX shifts
// {slot, first row, row count, n_discard}, by value in the kernel arguments, and for every shift and EVERY local layer moves the K and V rows
// [row_begin, row_begin + n_rows) to [row_begin - n_discard, row_begin - n_discard + n_rows).  V moves bytewise.  A K pair (x0, x1) at elements
// (e, e + 1), e even, becomes, with pr = (e % dh) / 2 and (c, s) = sincos[n_discard][pr] = (cos, sin) of the handle's own double table,
//     y0 = (float) __dadd_rn(__dmul_rn((double) x0, c), __dmul_rn((double) x1, s))
//     y1 = (float) __dsub_rn(__dmul_rn((double) x1, c), __dmul_rn((double) x0, s))
// -- explicit rounded operations, nothing contracted: a float64 restatement reproduces the bits.
//
// IN PLACE.  Source and destination of one shift overlap whenever n_rows > n_discard, and nothing here relies on any order between
// workgroups.  A thread OWNS one 16-byte column granule (two pairs) of one (shift, layer, array) run and walks the run's rows in ascending
// order, KV_SHIFT_U rows at a time: the U loads of source rows r .. r + U - 1 are all issued before the U stores to rows r - n_discard ..; the
// highest row a batch writes, r + U - 1 - n_discard, lies below every row a later batch reads (>= r + U) for every n_discard >= 1, and no
// other thread touches the column.  So no granule is read after the launch has overwritten it.  A wave reads and writes 1 KiB runs of a row.
// There is no row-band split: cutting a shift whose ranges do not alias into bands of 32 rows was measured on the 7B and bought nothing (the
// walk of whole columns already moves 5 TB/s and more at n_ctx 512 and 2048, aliasing or not: DESIGN.md 12.15), so every shift takes the one
// path.  Plain vector loads and stores only.  Slots of one table are distinct (the launcher refuses others).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kcommon.hip.h"
#include "llamahip_internal.h"

namespace lh {

constexpr int KV_SHIFT_THREADS = 256, U = KV_SHIFT_U;

__global__ void __launch_bounds__(KV_SHIFT_THREADS)
k_kv_shift_rows(float *Kc, float *Vc, const double *sincos_tab, const KvShiftTab tab, int n_layers, int n_ctx, int d, int dh, long n_items) {
    const int row_f4 = d / 4;
    const long layer_f4 = (long) n_ctx * row_f4, slot_f4 = layer_f4 * n_layers;      // 16-byte granules per layer / per slot
    // item -> (shift c, run = 2 * layer + {K, V}, column): columns fastest, so a wave walks 1 KiB of a row; an empty shift has no items
    long rest = (long) blockIdx.x * KV_SHIFT_THREADS + threadIdx.x;
    if (rest >= n_items) return;
    const long of_shift = (long) 2 * n_layers * row_f4;
    int c = 0;
    for (; c < tab.n; c++) {
        if (tab.n_rows[c] < 1) continue;
        if (rest < of_shift) break;
        rest -= of_shift;
    }
    if (c >= tab.n) return;                                       // (n_items is the launcher's sum of the same terms)
    const int col = (int) (rest % row_f4), run = (int) (rest / row_f4);
    const bool is_v = run & 1;
    const int nd = tab.n_discard[c], r_end = tab.n_rows[c];
    float4 *base = reinterpret_cast<float4 *>(is_v ? Vc : Kc) + (long) tab.slot[c] * slot_f4 + (long) (run >> 1) * layer_f4 + col;
    const float4 *src = base + (long) tab.row_begin[c] * row_f4;
    float4 *dst = base + (long) (tab.row_begin[c] - nd) * row_f4;
    double c0 = 1.0, s0 = 0.0, c1 = 1.0, s1 = 0.0;
    if (!is_v) {
        const double *t = sincos_tab + (size_t) nd * dh;
        const int e = 4 * col, p0 = (e % dh) >> 1, p1 = ((e + 2) % dh) >> 1;
        c0 = t[2 * p0]; s0 = t[2 * p0 + 1]; c1 = t[2 * p1]; s1 = t[2 * p1 + 1];
    }
    for (int r = 0; r < r_end; r += U) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++)
            v[u] = r + u < r_end ? src[(long) (r + u) * row_f4] : make_float4(0.f, 0.f, 0.f, 0.f);
        if (!is_v) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const double x0 = (double) v[u].x, x1 = (double) v[u].y, x2 = (double) v[u].z, x3 = (double) v[u].w;
                v[u].x = (float) __dadd_rn(__dmul_rn(x0, c0), __dmul_rn(x1, s0));
                v[u].y = (float) __dsub_rn(__dmul_rn(x1, c0), __dmul_rn(x0, s0));
                v[u].z = (float) __dadd_rn(__dmul_rn(x2, c1), __dmul_rn(x3, s1));
                v[u].w = (float) __dsub_rn(__dmul_rn(x3, c1), __dmul_rn(x2, s1));
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (r + u < r_end) dst[(long) (r + u) * row_f4] = v[u];
    }
}

hipError_t launch_kv_shift_rows(float *Kc, float *Vc, const double *sincos_tab, const KvShiftTab &tab, int n_slots, int n_layers, int n_ctx, int d, int dh,
                                hipStream_t st) {
    if (!Kc || !Vc || !sincos_tab || n_slots < 1 || n_layers < 1 || n_ctx < 1 || d < 4 || d % 4 != 0 || tab.n < 1 || tab.n > KV_SHIFT_MAX) return hipErrorInvalidValue;
    if (dh < 2 || dh % 2 != 0 || d % dh != 0) return hipErrorInvalidValue;
    if (((uintptr_t) Kc | (uintptr_t) Vc) & 15) return hipErrorInvalidValue;
    long n_items = 0;
    for (int c = 0; c < tab.n; c++) {
        // every range inside the cache on both sides (so n_discard < n_ctx, a row of the table, wherever a row moves), no slot twice
        if (tab.slot[c] < 0 || tab.slot[c] >= n_slots) return hipErrorInvalidValue;
        if (tab.n_discard[c] < 1 || tab.n_rows[c] < 0 || tab.row_begin[c] < 0 || (long) tab.row_begin[c] + tab.n_rows[c] > n_ctx) return hipErrorInvalidValue;
        if (tab.row_begin[c] - tab.n_discard[c] < 0) return hipErrorInvalidValue;
        for (int o = 0; o < c; o++)
            if (tab.slot[o] == tab.slot[c]) return hipErrorInvalidValue;
        if (tab.n_rows[c] > 0) n_items += (long) 2 * n_layers * (d / 4);
    }
    if (n_items == 0) return hipSuccess;          // nothing but empty shifts
    const long grid = (n_items + KV_SHIFT_THREADS - 1) / KV_SHIFT_THREADS;
    if (grid > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_kv_shift_rows, dim3((unsigned) grid), dim3(KV_SHIFT_THREADS), 0, st, Kc, Vc, sincos_tab, tab, n_layers, n_ctx, d, dh, n_items);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace lh
