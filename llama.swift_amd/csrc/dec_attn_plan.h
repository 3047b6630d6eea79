// dec_attn_plan.h -- the host-only half of the one-row decode attention (dec_attn_plan.cpp): which kernel launch_dec_attn runs for a shape,
// with which split of the key chains over workgroups, rows per stage, ring depth, LDS size and grid; the overrides of that rule (the
// LLAMAHIP_PV_* switches, llamahip_op_dec_attention's forced plans); and the geometry of the fused launch k_qkv_attn.  No device header:
// tools/host_sanitize.cpp compiles it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lh {

enum { DEC_ATTN_PV_BLK = 0, DEC_ATTN_X = 1, DEC_ATTN_PV_STREAM = 2, DEC_ATTN_PV_DMA = 3 };      // k_dec_scores + k_dec_pv_blk | k_dec_attn_x | k_dec_scores + k_dec_pv_stream | k_dec_scores + k_dec_pv_dma
constexpr int DEC_ATTN_TS = 32;                      // = DEC_TS of decode.hip (asserted there): keys per score workgroup
constexpr int DEC_ATTN_X_CTX_MAX = 1024;             // k_dec_attn_x: beyond, the two launches take over (launch_dec_attn explains)
constexpr int PV_STREAM_QUADS = 4 * 1024;            // k_dec_pv_stream<4>: 16-byte loads per stage (cpw * SR * 8 of them at most)
constexpr int PV_DMA_CPW_MAX = 3, PV_DMA_SLOT_BYTES = 4096, PV_DMA_NS_MAX = 256;      // k_dec_pv_dma: chains per workgroup, one chain-stage (8 rows x 128 floats), ring slots
constexpr size_t DEC_ATTN_LDS_CAP = 160 * 1024;      // init_attrs_decode's dynamic-LDS attribute

// An override of dec_attn_plan's rule: the LLAMAHIP_PV_* switches and llamahip_op_dec_attention's forced plans travel as this.  0 (dma: -1)
// = the library's rule.  dma 0: keep k_dec_pv_stream; 1: k_dec_pv_dma or nothing.  strict (the op): every value is taken as asked or the
// plan is refused with the reason; not strict (the switches): a value the shape cannot take falls back to the rule, as it always did.
struct DecAttnForce { int split = 0, stage_rows = 0, ns = 0, dma = -1; bool strict = false; };
// kernel < 0: refused, the reason in why.  split / cpw: workgroups per (head, column block) and chains per workgroup (one workgroup owns
// all nth chains in PV_BLK and X); SR: rows per chain and stage (PV_STREAM); NS: ring slots (PV_DMA); gx x gy workgroups of `threads`.
// The scores launch in front of PV_BLK / PV_STREAM / PV_DMA is always (H, ceil(n_ctx / 32)) x 256 threads with 2 dh floats of LDS.
struct DecAttnPlan {
    int kernel = -1, split = 1, cpw = 0, SR = 0, NS = 0;
    size_t lds = 0;
    int gx = 0, gy = 1, threads = 0;
    char why[200] = "";
};

bool pv_stream_applies(int dh, int n_ctx, int nth);
bool pv_split_valid(int nth, int split);             // every workgroup of the split owns at least one chain
const DecAttnForce &dec_attn_env();                  // the switches, parsed once per process
// force null: the switches.  have_sync: the caller has the zeroed counters and the fault word of k_dec_attn_x (the XCD placement confirmed);
// have_xpart: the tagged partial-sum buffer, the epoch and the fault word of the split soft_max . V
DecAttnPlan dec_attn_plan(int d, int H, int n_ctx, int nth, bool long_ctx, bool have_sync, bool have_xpart, const DecAttnForce *force = nullptr);

// ---- the fused launch (k_qkv_attn): the head layouts it takes, its three mat-vec instances, and grid / LDS next to the mat-vec role's
bool qkv_attn_shape_ok(int d, int H, int nth, int M, int K, int ngroups, int gmapF8, char *why = nullptr, size_t why_cap = 0);
bool qkv_attn_instance(int nw, bool ring, int depth, int pg);      // (4 waves, ring) x (depth, pg) in { (8, 1), (10, 2), (4, 2) }
struct QkvAttnGeom { int grid; size_t lds; };
QkvAttnGeom qkv_attn_geom(int gemv_grid, size_t gemv_lds, int d, int H, int n_ctx, int nth);

}  // namespace lh
