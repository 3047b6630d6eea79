// verify.hip -- the device half of drafted greedy decoding (llamahip_verify_greedy / llamahip_decode_greedy_lookup / llamahip_op_verify_rows).
// A verify step evaluates the rows [last accepted token, draft ...] as ONE multi-row eval whose row j holds the logits of a single-token
// eval at n_past + j; the two kernels here turn those N rows into "how much of the draft the model itself would have produced", so that
// 4 (N + 1) bytes cross to the host instead of N x n_vocab x 4.
//
// k_verify_rows: one workgroup of 1024 threads per row, the row's greedy pick by k_argmax's rule (decode.hip argmax_take): the largest
//   value, the LOWEST index on ties; a NaN is never taken (both comparisons are false); a row of nothing but NaN picks 0.  The scan is
//   k_argmax's, thread for thread (each thread visits its indices in ascending order, the pairs are folded by the same DPP / readlane /
//   LDS tree) -- not that it matters: "largest value, then lowest index" is a total order on the non-NaN entries, so every reduction
//   tree gives the same pick.  The lm head's pick epilogue of the fused greedy step (decode.hip EPI_STORE_PICK, launch_gemv_pick) follows
//   the same rule through an order-preserving 64-bit key {value bits with -0 folded onto +0, ~index} under an unsigned max, key 0 for a
//   NaN and index 0 when no key is set: -0 == +0 ties go to the lower index and a row of -inf picks index 0 there as here.  So
//   llamahip_decode_greedy and a verify step never disagree on a row.
// k_accept_drafts: one wave, behind it on the stream.  tokens[0] is the last accepted token, tokens[1 .. N) the draft:
//   n_accept = the largest a <= N - 1 with pick[j] == tokens[j + 1] for all j < a
//   log[cursor .. cursor + n_accept] = pick[0 .. n_accept]; state = {position, cursor}, both advanced by n_accept + 1
//   res = {n_accept, pick[0 .. N)}      (res: the pinned, device-mapped host block where the handle has one)
// Plain loads and stores, no hand-offs between workgroups: the launch boundary orders the two kernels.
// k_accept_drafts_set: the same rule for the rows of SEVERAL sequences in one step (llamahip_verify_greedy_multi /
//   llamahip_decode_greedy_lookup_multi / llamahip_op_verify_rows_set), one wave per segment.  Segment s is the rows
//   [seg_begin[s], seg_begin[s + 1]) of KV slot seg_slot[s]: its first row the slot's last token, the rest its draft.  Per segment
//   n_accept as above; with slot words (state != null: the slots are bound, llamahip_stage_bind) the slot's token log receives
//   pick[0 .. n_accept] at the slot's cursor, the slot's {position, cursor} advance by n_accept + 1 and the slot's next-token word
//   receives pick[n_accept] -- an ordinary set step or single step continues the slot from there.
//   res = {n_accept[0 .. n_segs), pick[0 .. n_rows)}: 4 (n_rows + n_segs) bytes for the host.
// k_sched_pick: the device half of a request scheduler's mixed pass (llamahip_sched_step), one wave per segment behind the lm head -- the
//   greedy pick of every segment that emits, by the device function k_verify_rows picks with (vr_row_pick), into the result block, the
//   slot's next-token word and its trace; every segment's slot {position, cursor} set behind its rows.  4 bytes per segment come back.
// k_sched_accept: the same for a scheduler step that carries drafted tokens, behind k_verify_rows over all logits rows of the step -- per
//   segment n_accept by the rule above (one device function, vr_n_accept, for the three kernels), the slot's words advanced by what was
//   accepted.  4 (rows + segments) bytes come back.
// k_verify_rows_dfa / k_sched_pick_dfa: the two kernels above for a scheduler step in which some greedy segment decodes under a constraint
//   (include/llamahip.h "constrained requests").  Same geometry, same stores; every logits row carries a pointer to the table
//   row next[state] of the state the host resolved for it (null: the row is unconstrained and takes vr_row_pick, not restated) and a
//   range-checked fallback token.  A constrained row's pick is k_pick_dfa's rule (dfa_pick.hip.h, the one statement of that scan); a row that
//   allows nothing picks its fallback and sets its dead word.  Plain 16-bit loads, no hand-offs between workgroups.
#include <cmath>

#include "dfa_pick.hip.h"
#include "kcommon.hip.h"

namespace lh {

__device__ __forceinline__ void vr_take(float &v, int &i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
template <int CTRL>
__device__ __forceinline__ void vr_take_dpp(float &v, int &i) {
    const float ov = dpp_f<CTRL>(v);
    const int oi = __builtin_amdgcn_mov_dpp(i, CTRL, 0xF, 0xF, true);
    vr_take(v, i, ov, oi);
}

// the greedy pick of one row by the whole workgroup (any whole number of waves up to 16; bv / bi: 16 LDS entries each): valid in thread 0
__device__ __forceinline__ int vr_row_pick(const float *__restrict__ row, int V, float *bv, int *bi) {
    const int tid = threadIdx.x, nt = blockDim.x;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int i0 = tid; i0 < V; i0 += 32 * nt) {
        float v[32];
#pragma unroll
        for (int u = 0; u < 32; u++) v[u] = row[min(i0 + u * nt, V - 1)];
#pragma unroll
        for (int u = 0; u < 32; u++) {
            const int i = i0 + u * nt;
            if (i < V) vr_take(best, idx, v[u], i);           // ascending i: a tie keeps the lower index
        }
    }
    vr_take_dpp<DPP_QUAD_XOR1>(best, idx);
    vr_take_dpp<DPP_QUAD_XOR2>(best, idx);
    vr_take_dpp<DPP_ROW_HALF_MIRROR>(best, idx);
    vr_take_dpp<DPP_ROW_MIRROR>(best, idx);                   // every lane of a 16-lane row holds the row's pick
    {
        const int vb = __builtin_bit_cast(int, best);
        float wv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 0));
        int wi = __builtin_amdgcn_readlane(idx, 0);
        vr_take(wv, wi, __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 16)), __builtin_amdgcn_readlane(idx, 16));
        vr_take(wv, wi, __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 32)), __builtin_amdgcn_readlane(idx, 32));
        vr_take(wv, wi, __builtin_bit_cast(float, __builtin_amdgcn_readlane(vb, 48)), __builtin_amdgcn_readlane(idx, 48));
        if ((tid & 63) == 0) { bv[tid >> 6] = wv; bi[tid >> 6] = wi; }
    }
    __syncthreads();
    float v = bv[0];
    int i = bi[0];
    for (int w = 1; w < (nt >> 6); w++) vr_take(v, i, bv[w], bi[w]);
    return i == 0x7fffffff ? 0 : i;                           // (nothing taken: every entry a NaN)
}

// the accept rule of one segment of N rows by one wave: lane j < N holds row j's pick p, tokens = the tokens of the segment's rows (tokens[0]
// the last accepted token, tokens[j + 1] the draft token behind row j).  Lane j < N - 1 agrees if row j's pick is the draft's next token;
// the first lane where that fails (or N - 1) is n_accept.  N >= 1; every lane of the wave calls it.
__device__ __forceinline__ int vr_n_accept(int lane, int N, int p, const int32_t *__restrict__ tokens) {
    const bool agree = lane < N - 1 && p == tokens[lane + 1];
    const unsigned long long miss = ~__ballot(agree);
    return min((int) __builtin_ctzll(miss), N - 1);
}

__global__ void __launch_bounds__(1024)
k_verify_rows(const float *__restrict__ logits, int V, int32_t *__restrict__ pick) {
    __shared__ float bv[16];
    __shared__ int bi[16];
    const int p = vr_row_pick(logits + (size_t) blockIdx.x * V, V, bv, bi);
    if (threadIdx.x == 0) pick[blockIdx.x] = p;
}

// The device half of a scheduler's mixed pass (llamahip_sched_step), one wave per segment (blockIdx.x), behind the lm head: row s of the
// logits is segment s's last row.  tab[s] = {emit, slot, position, cursor}: a segment that emits takes its row's greedy pick by
// vr_row_pick -- k_verify_rows' rule, not restated -- and res[s] receives it (-1 where it does not emit: four bytes per segment for the
// host).  With slot words (state != null; all three or none): the slot's {position, cursor} become the segment's -- the position behind
// its rows, the tokens its request has produced with this step -- and an emitting segment's pick goes to the slot's next-token word and
// to its trace at cursor - 1, so that the next captured step continues the slot on the device.
__global__ void __launch_bounds__(64)
k_sched_pick(const float *__restrict__ logits, int V, const int32_t *__restrict__ tab, int32_t *__restrict__ state, int32_t *__restrict__ log,
             int log_cap, int32_t *__restrict__ next_tok, int32_t *__restrict__ res) {
    __shared__ float bv[16];
    __shared__ int bi[16];
    const int s = blockIdx.x;
    const int emit = tab[4 * s], slot = tab[4 * s + 1], pos = tab[4 * s + 2], cur = tab[4 * s + 3];
    int p = -1;
    if (emit) p = vr_row_pick(logits + (size_t) s * V, V, bv, bi);          // (emit is uniform over the workgroup)
    if (threadIdx.x != 0) return;
    res[s] = p;
    if (!state) return;
    state[2 * (size_t) slot] = pos;
    state[2 * (size_t) slot + 1] = cur;
    if (emit) {
        next_tok[slot] = p;
        if (cur >= 1 && cur <= log_cap) log[(size_t) slot * log_cap + cur - 1] = p;
    }
}

// k_verify_rows under per-row allow-lists: rows.row[r] = the table row of logits row r's state (null = unconstrained), fb.t[r] = the token
// a row that allows nothing picks (dead[r] = 1; 0 otherwise).  The pick is an embedding read on the next step: always a checked token id.
__global__ void __launch_bounds__(1024)
k_verify_rows_dfa(const float *__restrict__ logits, int V, const DfaMaskRows rows, const DfaFallback fb, int32_t *__restrict__ pick, int32_t *__restrict__ dead) {
    __shared__ float bv[16];
    __shared__ int bi[16], bl[16];
    const int r = blockIdx.x;
    const uint16_t *__restrict__ tab = rows.row[r];               // (uniform over the workgroup)
    const float *__restrict__ row = logits + (size_t) r * V;
    const int p = tab ? dfa_row_pick(row, tab, V, bv, bi, bl) : vr_row_pick(row, V, bv, bi);
    if (threadIdx.x == 0) {
        pick[r] = p == DFA_NONE ? fb.t[r] : p;
        dead[r] = p == DFA_NONE ? 1 : 0;
    }
}

// k_sched_pick under per-segment allow-lists: the stores are k_sched_pick's; res = {pick[n_segs], dead[n_segs]}
__global__ void __launch_bounds__(64)
k_sched_pick_dfa(const float *__restrict__ logits, int V, const int32_t *__restrict__ tab, const DfaMaskRows rows, const DfaFallback fb,
                 int32_t *__restrict__ state, int32_t *__restrict__ log, int log_cap, int32_t *__restrict__ next_tok, int32_t *__restrict__ res) {
    __shared__ float bv[16];
    __shared__ int bi[16], bl[16];
    const int s = blockIdx.x, n_segs = gridDim.x;
    const int emit = tab[4 * s], slot = tab[4 * s + 1], pos = tab[4 * s + 2], cur = tab[4 * s + 3];
    const uint16_t *__restrict__ allow = rows.row[s];
    const float *__restrict__ row = logits + (size_t) s * V;
    int p = -1, dead = 0;
    if (emit) {                                                   // (emit and allow are uniform over the workgroup)
        p = allow ? dfa_row_pick(row, allow, V, bv, bi, bl) : vr_row_pick(row, V, bv, bi);
        if (p == DFA_NONE) { p = fb.t[s]; dead = 1; }
    }
    if (threadIdx.x != 0) return;
    res[s] = p;
    res[n_segs + s] = dead;
    if (!state) return;
    state[2 * (size_t) slot] = pos;
    state[2 * (size_t) slot + 1] = cur;
    if (emit) {
        next_tok[slot] = p;
        if (cur >= 1 && cur <= log_cap) log[(size_t) slot * log_cap + cur - 1] = p;
    }
}

// pick == null: one row whose pick is pick_imm (a single-token step of the caller's loop, appended to the same log).
// restart_pos >= 0: the log starts over -- position restart_pos, cursor 0 -- before this step is appended.
// log_cap: entries the log holds; an append that would pass it is dropped (the host refuses such a call before it is launched).
__global__ void __launch_bounds__(64)
k_accept_drafts(const int32_t *__restrict__ tokens, const int32_t *__restrict__ pick, int pick_imm, int N, int restart_pos,
                int32_t *__restrict__ log, int log_cap, int32_t *__restrict__ state, int32_t *__restrict__ res) {
    const int lane = threadIdx.x;
    const int p = !pick ? pick_imm : lane < N ? pick[lane] : 0;
    const int n_accept = vr_n_accept(lane, N, p, tokens);
    const int pos = restart_pos >= 0 ? restart_pos : state[0], cur = restart_pos >= 0 ? 0 : state[1];
    if (lane <= n_accept && cur >= 0 && cur + lane < log_cap) log[cur + lane] = p;
    if (lane < N) res[1 + lane] = p;
    if (lane == 0) {
        res[0] = n_accept;
        state[0] = pos + n_accept + 1;
        state[1] = cur + n_accept + 1;
    }
}

// one wave per segment (blockIdx.x); slot words: state [slot][2], log [slot][log_cap], next_tok [slot] -- all three or none
__global__ void __launch_bounds__(64)
k_accept_drafts_set(const int32_t *__restrict__ tokens, const int32_t *__restrict__ pick, const int32_t *__restrict__ seg_begin,
                    const int32_t *__restrict__ seg_slot, int n_segs, int n_rows, int32_t *__restrict__ state, int32_t *__restrict__ log,
                    int log_cap, int32_t *__restrict__ next_tok, int32_t *__restrict__ res) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int b = seg_begin[s], N = seg_begin[s + 1] - b;
    if (b < 0 || N < 1 || b + N > n_rows) return;                 // (the host refuses such segments before the launch)
    const int p = lane < N ? pick[b + lane] : 0;
    const int n_accept = vr_n_accept(lane, N, p, tokens + b);
    if (lane < N) res[n_segs + b + lane] = p;
    if (lane == 0) res[s] = n_accept;
    if (!state) return;
    const int slot = seg_slot[s];
    int32_t *st = state + 2 * (size_t) slot;
    const int pos = st[0], cur = st[1];                           // (every lane reads before lane 0 writes: one wave, program order)
    if (lane <= n_accept && cur >= 0 && cur + lane < log_cap) log[(size_t) slot * log_cap + cur + lane] = p;
    if (lane == n_accept) next_tok[slot] = p;
    if (lane == 0) {
        st[0] = pos + n_accept + 1;
        st[1] = cur + n_accept + 1;
    }
}

// A scheduler's step with drafted tokens (llamahip_sched_step with draft_len > 0; llamahip_op_sched_accept), one wave per segment
// (blockIdx.x) behind k_verify_rows, which has picked every logits row of the step: k_sched_pick generalised to segments with several
// logits rows.  tab[s] = {emit, slot, base position, base cursor, first logits row b, row count}.  The segment's logits rows are
// [b, b + N): N = the row count where emit == 2 (a decode segment [last token, draft ...]: tokens[b ..] are its rows' tokens), 1 where
// emit == 1 (the last row of a prompt piece, a plain decode row), none where emit == 0.  n_accept by vr_n_accept -- the rule of
// k_accept_drafts_set, not restated -- where N > 1, else 0.  res = {n_accept[n_segs], pick[n_rows]}.  With slot words (state != null; all
// three or none): position = base + rows consumed (n_accept + 1 for emit 2, the row count otherwise), cursor = base cursor + tokens
// produced, the slot's next-token word = pick[n_accept], its trace receives pick[0 .. n_accept] at the base cursor.
// Plain loads and stores, program order inside the one wave, no hand-offs between workgroups.
__global__ void __launch_bounds__(64)
k_sched_accept(const int32_t *__restrict__ pick, const int32_t *__restrict__ tokens, const int32_t *__restrict__ tab, int n_segs, int n_rows,
               int32_t *__restrict__ state, int32_t *__restrict__ log, int log_cap, int32_t *__restrict__ next_tok, int32_t *__restrict__ res) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int32_t *t = tab + SCHED_TAB_W * s;
    const int emit = t[0], slot = t[1], pos = t[2], cur = t[3], b = t[4], rows = t[5];
    const int N = emit == 2 ? rows : emit == 1 ? 1 : 0;          // (uniform over the wave)
    if (N > 0 && (b < 0 || b + N > n_rows || N > 64)) return;    // (the host refuses such segments before the launch)
    const int p = lane < N ? pick[b + lane] : 0;
    const int n_accept = N > 1 ? vr_n_accept(lane, N, p, tokens + b) : 0;
    if (lane < N) res[n_segs + b + lane] = p;
    if (lane == 0) res[s] = n_accept;
    if (!state) return;
    const int made = N > 0 ? n_accept + 1 : 0;                   // the tokens the segment produced
    if (lane < made && cur >= 0 && cur + lane < log_cap) log[(size_t) slot * log_cap + cur + lane] = p;
    if (N > 0 && lane == n_accept) next_tok[slot] = p;
    if (lane == 0) {
        state[2 * (size_t) slot] = pos + (emit == 2 ? n_accept + 1 : rows);
        state[2 * (size_t) slot + 1] = cur + made;
    }
}

hipError_t launch_verify_rows(const float *logits, int n_rows, int V, int32_t *pick, hipStream_t st) {
    if (n_rows < 1 || n_rows > VERIFY_ROWS_MAX || V < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_verify_rows, dim3((unsigned) n_rows), dim3(1024), 0, st, logits, V, pick);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

// tab: n_segs x {emit, slot, position, cursor} on the device; the slots are checked by the caller (< the rows of state / log / next_tok)
hipError_t launch_sched_pick(const float *logits, int n_segs, int V, const int32_t *tab, int32_t *state, int32_t *log, int log_cap, int32_t *next_tok,
                             int32_t *res, hipStream_t st) {
    if (n_segs < 1 || n_segs > SET_MAX || V < 1 || !logits || !tab || !res) return hipErrorInvalidValue;
    if (state && (!log || !next_tok || log_cap < 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sched_pick, dim3((unsigned) n_segs), dim3(64), 0, st, logits, V, tab, state, log, log_cap, next_tok, res);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

// rows.row[r] null = unconstrained; every fallback token in [0, V) -- the callers' business, re-checked here because the pick is an index
hipError_t launch_verify_rows_dfa(const float *logits, int n_rows, int V, const DfaMaskRows &rows, const DfaFallback &fb, int32_t *pick, int32_t *dead, hipStream_t st) {
    if (n_rows < 1 || n_rows > VERIFY_ROWS_MAX || V < 1 || !logits || !pick || !dead) return hipErrorInvalidValue;
    for (int r = 0; r < n_rows; r++) if (fb.t[r] < 0 || fb.t[r] >= V) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_verify_rows_dfa, dim3((unsigned) n_rows), dim3(1024), 0, st, logits, V, rows, fb, pick, dead);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

// launch_sched_pick's operands; res receives {pick[n_segs], dead[n_segs]}
hipError_t launch_sched_pick_dfa(const float *logits, int n_segs, int V, const int32_t *tab, const DfaMaskRows &rows, const DfaFallback &fb, int32_t *state,
                                 int32_t *log, int log_cap, int32_t *next_tok, int32_t *res, hipStream_t st) {
    if (n_segs < 1 || n_segs > SET_MAX || V < 1 || !logits || !tab || !res) return hipErrorInvalidValue;
    if (state && (!log || !next_tok || log_cap < 1)) return hipErrorInvalidValue;
    for (int r = 0; r < n_segs; r++) if (fb.t[r] < 0 || fb.t[r] >= V) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sched_pick_dfa, dim3((unsigned) n_segs), dim3(64), 0, st, logits, V, tab, rows, fb, state, log, log_cap, next_tok, res);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_sched_accept(const int32_t *pick, const int32_t *tokens, const int32_t *tab, int n_segs, int n_rows, int32_t *state, int32_t *log,
                               int log_cap, int32_t *next_tok, int32_t *res, hipStream_t st) {
    if (n_segs < 1 || n_segs > SET_MAX || n_rows < 1 || n_rows > VERIFY_ROWS_MAX || !pick || !tokens || !tab || !res) return hipErrorInvalidValue;
    if (state && (!log || !next_tok || log_cap < 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sched_accept, dim3((unsigned) n_segs), dim3(64), 0, st, pick, tokens, tab, n_segs, n_rows, state, log, log_cap, next_tok, res);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_accept_drafts(const int32_t *tokens, const int32_t *pick, int pick_imm, int n_rows, int restart_pos, int32_t *log, int log_cap,
                                int32_t *state, int32_t *res, hipStream_t st) {
    if (n_rows < 1 || n_rows > VERIFY_ROWS_MAX || !log || !state || !res || (!pick && n_rows != 1) || (n_rows > 1 && !tokens)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_accept_drafts, dim3(1), dim3(64), 0, st, tokens, pick, pick_imm, n_rows, restart_pos, log, log_cap, state, res);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_accept_drafts_set(const int32_t *tokens, const int32_t *pick, const int32_t *seg_begin, const int32_t *seg_slot, int n_segs, int n_rows,
                                    int32_t *state, int32_t *log, int log_cap, int32_t *next_tok, int32_t *res, hipStream_t st) {
    if (n_rows < 1 || n_rows > VERIFY_ROWS_MAX || n_segs < 1 || n_segs > n_rows || !tokens || !pick || !seg_begin || !res) return hipErrorInvalidValue;
    if (state && (!log || !next_tok || !seg_slot || log_cap < 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_accept_drafts_set, dim3((unsigned) n_segs), dim3(64), 0, st, tokens, pick, seg_begin, seg_slot, n_segs, n_rows, state, log, log_cap,
                       next_tok, res);
    LH_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace lh
