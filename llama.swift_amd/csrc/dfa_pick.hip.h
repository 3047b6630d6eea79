// dfa_pick.hip.h -- the ONE statement of the constrained scan: the pick of a logits row over the ALLOWED entries of a
// token-table row by one workgroup.  k_pick_dfa (constrain.hip: a sequence with a device-resident state word) and the scheduler's
// k_verify_rows_dfa / k_sched_pick_dfa (verify.hip: the host resolves the state, the table row travels in the kernel arguments) call it.
// The rule is k_argmax's (decode.hip argmax_take) over the entries whose table word is not DFA_BANNED_U16: the largest value, the LOWEST
// index on ties (+0.0 == -0.0), a NaN never taken; where every allowed entry is a NaN, the lowest allowed index.  The scan is k_argmax's --
// 32 loads in flight per thread, the DPP / readlane fold, one barrier -- with the table row read beside the logits at the same indices
// (plain 16-bit loads: with an odd n_vocab a table row is only 2-byte aligned, and nothing here is packed).  "Largest value, then lowest
// index" is a total order on the non-NaN entries, so the fold's shape and the workgroup's size do not matter.
#pragma once
#include <cmath>

#include "kcommon.hip.h"

namespace lh {

__device__ __forceinline__ void dfa_take(float &v, int &i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
template <int CTRL>
__device__ __forceinline__ void dfa_take_dpp(float &v, int &i, int &lo) {
    const float ov = dpp_f<CTRL>(v);
    const int oi = __builtin_amdgcn_mov_dpp(i, CTRL, 0xF, 0xF, true);
    dfa_take(v, i, ov, oi);
    lo = min(lo, __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, true));
}

constexpr int DFA_NONE = 0x7fffffff;

// the pick of `logits` [V] under the table row `tab` [V] by the whole workgroup (any whole number of waves up to 16; bv / bi / bl: 16 LDS
// entries each): valid in thread 0.  tab == null (uniform over the workgroup: a state word out of range) scans nothing.  DFA_NONE where
// nothing is allowed -- the caller then takes its range-checked fallback token.  One barrier, reached by every thread.
__device__ __forceinline__ int dfa_row_pick(const float *__restrict__ logits, const uint16_t *__restrict__ tab, int V, float *bv, int *bi, int *bl) {
    const int tid = threadIdx.x, nt = blockDim.x;
    float best = -INFINITY;
    int idx = DFA_NONE, lo = DFA_NONE;                            // lo: the thread's lowest allowed index (its indices ascend)
    if (tab) {
        for (int i0 = tid; i0 < V; i0 += 32 * nt) {
            float v[32];
            uint16_t t[32];
#pragma unroll
            for (int u = 0; u < 32; u++) { const int i = min(i0 + u * nt, V - 1); v[u] = logits[i]; t[u] = tab[i]; }
#pragma unroll
            for (int u = 0; u < 32; u++) {
                const int i = i0 + u * nt;
                if (i < V && t[u] != DFA_BANNED_U16) {
                    dfa_take(best, idx, v[u], i);                 // ascending i: a tie keeps the lower index
                    lo = min(lo, i);
                }
            }
        }
    }
    dfa_take_dpp<DPP_QUAD_XOR1>(best, idx, lo);
    dfa_take_dpp<DPP_QUAD_XOR2>(best, idx, lo);
    dfa_take_dpp<DPP_ROW_HALF_MIRROR>(best, idx, lo);
    dfa_take_dpp<DPP_ROW_MIRROR>(best, idx, lo);                  // every lane of a 16-lane row holds the row's pick
    {
        const int vb = __builtin_bit_cast(int, best);
        float wv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 0));
        int wi = __builtin_amdgcn_readlane(idx, 0), wl = __builtin_amdgcn_readlane(lo, 0);
        dfa_take(wv, wi, __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 16)), __builtin_amdgcn_readlane(idx, 16));
        dfa_take(wv, wi, __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 32)), __builtin_amdgcn_readlane(idx, 32));
        dfa_take(wv, wi, __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 48)), __builtin_amdgcn_readlane(idx, 48));
        wl = min(min(wl, __builtin_amdgcn_readlane(lo, 16)), min(__builtin_amdgcn_readlane(lo, 32), __builtin_amdgcn_readlane(lo, 48)));
        if ((tid & 63) == 0) { bv[tid >> 6] = wv; bi[tid >> 6] = wi; bl[tid >> 6] = wl; }
    }
    __syncthreads();
    float v = bv[0];
    int i = bi[0], l = bl[0];
    for (int w = 1; w < (nt >> 6); w++) { dfa_take(v, i, bv[w], bi[w]); l = min(l, bl[w]); }
    const int p = i != DFA_NONE ? i : l;                          // (nothing taken: every allowed entry a NaN -> the lowest allowed index)
    return p < 0 || p >= V ? DFA_NONE : p;
}

}  // namespace lh
