// constrain.hip -- the device half of constrained decoding (include/llamahip.h): the token table of a constraint is
// uint16 next[n_states][n_vocab], DFA_BANNED (0xFFFF) = not allowed; a sequence carries one device-resident word, the automaton's state.
//
// k_pick_dfa: one workgroup of 1024 threads per row, 1 .. 16 rows, each with its own logits row, state word and table.  The pick is
//   k_argmax's rule (decode.hip argmax_take) over the ALLOWED entries of next[state]: the largest value, the LOWEST index on ties
//   (+0.0 == -0.0), a NaN never taken; where every allowed entry is a NaN, the lowest allowed index.  The scan is k_argmax's -- 32 loads
//   in flight per thread, the DPP / readlane fold, one barrier -- with the table row read beside the logits at the same indices (plain
//   16-bit loads: rows are 2 * n_vocab bytes apart, so with an odd n_vocab a row is not 4-byte aligned, and nothing here is packed).
//   "Largest value, then lowest index" is a total order on the non-NaN entries, so the fold's shape does not matter.
//   Thread 0 then does what k_argmax does -- out[st ? st[1] : out_idx] = pick, *next_token = pick, {position, step} advanced -- and writes
//   state = next[state][pick].  With a row's `repick` set the launch stands behind a step whose own tail (k_argmax_set, k_argmax) has picked
//   from the same logits and advanced: the pick overwrites that tail's trace entry at st[1] - 1 and its next-token word, the position stays.
//   A state word outside [0, n_states), or a row with nothing allowed (neither occurs with a table of llamahip_constraint_new and a state
//   it handed out: DESIGN.md 12.33), indexes nothing: the pick is the row's fallback token, the state word stays, the row's `dead` word
//   (cst[1]) is set to 1.  The pick is an embedding read on the next step, so it is always a token id the host has range-checked.
// k_mask_rows_dfa: out[r][i] = next[state_r][i] == BANNED ? -inf : logits[r][i], bit copies otherwise; the sampler front end
//   (launch_topk_candidates) runs on the masked rows unchanged.
// Plain loads and stores, no hand-offs between workgroups.
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

__global__ void __launch_bounds__(1024)
k_pick_dfa(const DfaRows rows, int V) {
    __shared__ float bv[16];
    __shared__ int bi[16], bl[16];
    const DfaRow &R = rows.r[blockIdx.x];
    const int tid = threadIdx.x, nt = blockDim.x;
    const float *__restrict__ logits = R.logits;
    const int state = R.cst[0];                                   // (every thread reads it in front of the barrier; thread 0 writes behind it)
    const bool in_range = state >= 0 && state < R.n_states;       // uniform over the workgroup
    float best = -INFINITY;
    int idx = DFA_NONE, lo = DFA_NONE;                            // lo: the thread's lowest allowed index (its indices ascend)
    if (in_range) {
        const uint16_t *__restrict__ tab = R.table + (size_t) state * (size_t) V;
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
    if (tid == 0) {
        float v = bv[0];
        int i = bi[0], l = bl[0];
        for (int w = 1; w < (nt >> 6); w++) { dfa_take(v, i, bv[w], bi[w]); l = min(l, bl[w]); }
        const int p = i != DFA_NONE ? i : l;                      // (nothing taken: every allowed entry a NaN -> the lowest allowed index)
        const bool dead = !in_range || p == DFA_NONE || p < 0 || p >= V;
        const int r = dead ? R.fallback : p;
        int32_t *st = R.st;
        // repick (behind a set step, whose own tail has picked and advanced): the entry that tail wrote, and no advance
        const int at = st ? st[1] - (R.repick ? 1 : 0) : R.out_idx;
        if (R.out && at >= 0) R.out[at] = r;
        if (R.next_token) *R.next_token = r;
        if (st && !R.repick) { st[0] += 1; st[1] += 1; }
        if (dead) R.cst[1] = 1;
        else R.cst[0] = (int32_t) R.table[(size_t) state * (size_t) V + (size_t) r];
    }
}

__global__ void __launch_bounds__(256)
k_mask_rows_dfa(const uint32_t *__restrict__ logits, uint32_t *__restrict__ out, int V, const DfaMaskRows rows) {
    const int r = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const uint16_t *__restrict__ tab = rows.row[r];
    const size_t at = (size_t) r * (size_t) V + (size_t) i;
    out[at] = tab[i] == DFA_BANNED_U16 ? 0xFF800000u : logits[at];
}

// every row: logits, table, cst non-null, n_states >= 1, fallback in [0, V) -- the callers' business, re-checked here because a bad row is a
// wild store
hipError_t launch_pick_dfa(const DfaRows &rows, int n_rows, int V, hipStream_t st) {
    if (n_rows < 1 || n_rows > DFA_ROWS_MAX || V < 1) return hipErrorInvalidValue;
    for (int r = 0; r < n_rows; r++) {
        const DfaRow &R = rows.r[r];
        if (!R.logits || !R.table || !R.cst || R.n_states < 1 || R.fallback < 0 || R.fallback >= V) return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k_pick_dfa, dim3((unsigned) n_rows), dim3(1024), 0, st, rows, V);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

// rows.row[r] = the table row of logits row r's state (the host resolves the state: it is an argument of the entry points that mask)
hipError_t launch_mask_rows_dfa(const float *logits, float *out, int n_rows, int V, const DfaMaskRows &rows, hipStream_t st) {
    if (n_rows < 1 || n_rows > DFA_ROWS_MAX || V < 1 || !logits || !out) return hipErrorInvalidValue;
    for (int r = 0; r < n_rows; r++) if (!rows.row[r]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mask_rows_dfa, dim3((unsigned) ((V + 255) / 256), (unsigned) n_rows), dim3(256), 0, st, (const uint32_t *) logits, (uint32_t *) out, V, rows);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace lh
