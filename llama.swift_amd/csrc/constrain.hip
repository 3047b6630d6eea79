// constrain.hip -- the device half of constrained decoding (include/llamahip.h): the token table of a constraint is
// uint16 next[n_states][n_vocab], DFA_BANNED (0xFFFF) = not allowed; a sequence carries one device-resident word, the automaton's state.
//
// k_pick_dfa: one workgroup of 1024 threads per row, 1 .. 16 rows, each with its own logits row, state word and table.  The pick is
//   k_argmax's rule (decode.hip argmax_take) over the ALLOWED entries of next[state]: the largest value, the LOWEST index on ties
//   (+0.0 == -0.0), a NaN never taken; where every allowed entry is a NaN, the lowest allowed index.  The scan and the fold are the device
//   function dfa_row_pick (dfa_pick.hip.h: the one statement of them, shared with the scheduler's kernels in verify.hip) -- k_argmax's, 32 loads
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

#include "dfa_pick.hip.h"
#include "kcommon.hip.h"

namespace lh {

__global__ void __launch_bounds__(1024)
k_pick_dfa(const DfaRows rows, int V) {
    __shared__ float bv[16];
    __shared__ int bi[16], bl[16];
    const DfaRow &R = rows.r[blockIdx.x];
    const int state = R.cst[0];                                   // (every thread reads it in front of the barrier; thread 0 writes behind it)
    const bool in_range = state >= 0 && state < R.n_states;       // uniform over the workgroup
    // the scan and the fold: dfa_pick.hip.h, not restated
    const int p = dfa_row_pick(R.logits, in_range ? R.table + (size_t) state * (size_t) V : nullptr, V, bv, bi, bl);
    if (threadIdx.x == 0) {
        const bool dead = !in_range || p == DFA_NONE;
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
