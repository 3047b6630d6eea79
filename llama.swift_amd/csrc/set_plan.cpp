// set_plan.cpp -- the host half of the few-row Q4_0 mat-mul k_gemv_set (gemv_set.hip): the (NC, CW) plan per row count, the one place that
// derives it, the LLAMAHIP_SET_PLAN* switches, the check of a caller's forced plan, and the grid / threads arithmetic of a launch.  Pure host
// code, no device: tools/host_sanitize runs it under ASan + UBSan.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "set_plan.h"

namespace lh {

size_t set_lds_bytes(const SetShape &w, int ncols_group, int nc, int cw, int rgw) {
    const int steps = (w.nchunks + cw - 1) / cw, npad = steps * cw + SET_PF;
    size_t lds = (size_t) ncols_group * npad * 288 + (cw > 1 ? (size_t) rgw * SET_DR * cw * SET_TILE_BYTES : 0) + (LH_SET_PROBE ? 256 : 0);
    return std::max(lds, (size_t) nc * cw * 64 * 4);
}

// the (NC, CW) pairs k_gemv_set is instantiated for (launch_set_any's dispatch list)
bool set_plan_instantiated(int nc, int cw) {
    static const int pairs[][2] = { {1, 2}, {1, 3}, {1, 4}, {2, 1}, {2, 2}, {2, 3}, {2, 4}, {3, 1}, {3, 3}, {3, 4}, {4, 1}, {4, 2}, {4, 4}, {5, 1} };
    for (const auto &pr : pairs) if (pr[0] == nc && pr[1] == cw) return true;
    return false;
}

// LLAMAHIP_SET_PLAN[_BIG|_SMALL] are parsed once per process (the switches of this library are read once; set_plan runs several times per launch)
// into the same SetForce a caller hands to set_plan (llamahip_op_gemv_set_q4_0): one override path
static SetForce set_plan_env_parse(const char *name) {
    SetForce f;
    int nc = 0, cw = 0, ncg = 0, rgw = 0;
    const char *env = getenv(name);
    if (!env) return f;
    const int got = sscanf(env, "%d,%d,%d,%d", &nc, &cw, &ncg, &rgw);
    if (got < 2 || nc < 1 || nc > 5 || cw < 1 || cw > 4 || (nc == 5 && cw != 1)) return f;
    f.nc = nc; f.cw = cw; f.ncg = got >= 3 ? ncg : 0; f.rgw = got >= 4 ? rgw : 0;
    return f;
}
// the override onto (nc, cw, ncg, rgw); false (nothing changed): no override, or its column groups do not cover exactly the N rows
static bool set_force_apply(const SetForce &f, int N, int epi, int &nc, int &cw, int &ncg, int &rgw) {
    if (f.nc < 1 || f.cw < 1) return false;
    int f_ncg = f.ncg;
    if (f_ncg < 1) f_ncg = (N + f.nc * f.cw - 1) / (f.nc * f.cw);
    if (f.nc * f.cw * f_ncg < N || (f_ncg - 1) * f.nc * f.cw >= N) return false;
    nc = f.nc; cw = f.cw; ncg = f_ncg;
    if (f.rgw >= 1 && f.rgw <= 8 && epi != SET_EPI_SILU_QAH && epi != SET_EPI_SILU_QA) rgw = f.rgw;
    return true;
}
static const SetForce &set_plan_env(int which) {
    static const SetForce envs[3] = { set_plan_env_parse("LLAMAHIP_SET_PLAN_BIG"), set_plan_env_parse("LLAMAHIP_SET_PLAN_SMALL"), set_plan_env_parse("LLAMAHIP_SET_PLAN") };
    return envs[which];
}
// Columns per wave (nc), waves per row-group (cw) and column groups (ncg) for N rows.  What the in-kernel timelines say (profiles/r05_*):
// a wave spends ~0.07 - 0.09 us per (chunk, column) item whatever shares its SIMD, a step of a shared ring costs a barrier (~0.3 us in a
// 16-wave workgroup), and a launch ends when its longest wave does.  So: matrices with few row-groups (wo, w2: 512 at 7B) take cw waves per
// row-group with one or two columns each (items per wave = chunks x nc); matrices with >= 1 024 row-groups (wq|wk|wv, w1|w3, the lm head)
// have waves enough: up to four columns per wave, no sharing, and for more than four rows column GROUPS at grid level (the groups of a
// row block run side by side on one XCD; the second read of a tile is an L2 hit hidden behind arithmetic -- at 8 rows these launches
// are VALU bound: sharing the ring there AND streaming the operand rows through a second ring, k_gemv_set_ar of round 5, read the weights once
// and measured the same -- profiles/r05_o_operand_ring_ab.txt; removed).  LLAMAHIP_SET_PLAN[_BIG|_SMALL]="nc,cw[,ncg[,rgw]]" overrides (measurement; _BIG: the unshared class).
// force (may be null): the caller's override instead of the environment's; force->strict: the plan is launched as asked or not at all
// (gemv_set_force_check has admitted it), so the LDS rule below does not replace it
SetPlan set_plan(const SetShape &w, int N, int epi, const SetForce *force) {
    SetPlan p;
    // waves per row-group: enough to put about two waves on every SIMD of the chip (ngroups x cw >= ~2 000), w1|w3 always unshared (its
    // half-block workgroups are many); then <= 4 columns per wave, column groups at grid level beyond 4 cw columns
    const bool big = w.ngroups >= 1536 || epi == SET_EPI_SILU_QAH || epi == SET_EPI_SILU_QA;
    int cw = big ? 1 : w.ngroups >= 768 ? 2 : 4;
    if (cw > N) cw = N;
    const int ncmax = cw == 1 ? 5 : 4;                                // (five columns per wave are instantiated for unshared rings only: 9 rows = 5 + 4)
    int ncg = (N + ncmax * cw - 1) / (ncmax * cw);
    const int ng = (N + ncg - 1) / ncg;                               // columns per group, balanced (9 rows, unshared: 3 + 3 + 3)
    int nc = (ng + cw - 1) / cw, rgw = 0;
    cw = (ng + nc - 1) / nc;
    // the small class by row count, measured (7B wo / w2, fresh processes, profiles/r05_u_fresh_ab.txt, r05_v_small_plans.txt): three
    // column-waves leave 16 chunks a ragged last step (5 - 6 rows: <2,4> -1.5 %); from 9 rows on the launches are VALU bound and a step's
    // barrier is pure loss: unshared rings in column groups of 3 (9 - 12 rows: -4 ... -6 % per eval) or 4 (13 - 16: -2 %)
    // (the 768 .. 1 535 row-group class -- wo of the 30B / 65B -- takes the same rule from 9 rows on: the argument does not depend on the size)
    if (!big && N >= 5) {
        if (N <= 8) { if (w.ngroups < 768) { nc = 2; cw = 4; ncg = 1; } }
        else if (N <= 12) { nc = 3; cw = 1; ncg = (N + 2) / 3; }
        else { nc = 4; cw = 1; ncg = (N + 3) / 4; }
    }
    if (force) (void) set_force_apply(*force, N, epi, nc, cw, ncg, rgw);
    else (void) (set_force_apply(set_plan_env(big ? 0 : 1), N, epi, nc, cw, ncg, rgw) || set_force_apply(set_plan_env(2), N, epi, nc, cw, ncg, rgw));
    auto finish = [&]() {
        // (instantiated: <1,2> <1,3> <1,4> <2,1> <2,2> <2,3> <2,4> <3,1> <3,3> <3,4> <4,1> <4,2> <4,4> <5,1>)
        if (nc == 1 && cw == 1) nc = 2;
        if (nc == 3 && cw == 2) nc = 4;
        if (nc == 4 && cw == 3) cw = 4;
        ncg = (N + nc * cw - 1) / (nc * cw);                          // (the promotions above widen a group: no column group may start past row N)
        if (!rgw) rgw = epi == SET_EPI_SILU_QAH ? 4 : (cw >= 3 ? 2 : 4);
        if (epi == SET_EPI_SILU_QAH) rgw = 4;
        else if (epi == SET_EPI_SILU_QA) rgw = 8;
        else if (rgw * cw > 8) rgw = 8 / cw;                          // (set_max_threads)
        p.nc = nc; p.cw = cw; p.rgw = rgw; p.ncg = ncg;
        p.lds = set_lds_bytes(w, std::min(N, nc * cw), nc, cw, rgw);
    };
    finish();
    if (p.lds > SET_LDS_CAP && !(force && force->strict)) {
        // (a forced plan that cannot fit degrades to this rule for that shape too: a measurement variant never sends a shape to the generic kernel)
        // wide rows (w2 of the 13B / 65B: 54 / 86 chunks): the operand rows of a whole group do not fit next to a shared ring.  Unshared
        // column groups of as many columns (<= 4) as leave two workgroups' worth of LDS per CU where possible
        const size_t per_col = set_lds_bytes(w, 1, 1, 1, 4);
        int fit = (int) std::min<size_t>(4, (SET_LDS_CAP / 2) / per_col);
        if (fit < 2) fit = (int) std::min<size_t>(4, SET_LDS_CAP / per_col);
        if (fit >= 1) {
            cw = 1; rgw = 0;
            ncg = (N + fit - 1) / fit;
            nc = (N + ncg - 1) / ncg;
            finish();
        }
    }
    return p;
}

bool set_applies(const SetShape &w, int N, int epi) {
    if (N < 2 || N > SET_ROWS_MAX || !w.tiles) return false;
    if (epi == SET_EPI_ROPE_KV && w.gmapF8 != 0) return false;
    if ((epi == SET_EPI_SILU_QAH || epi == SET_EPI_SILU_QA) && (w.gmapF8 == 0 || w.ngroups % 8 != 0)) return false;
    if (epi != SET_EPI_STORE && epi != SET_EPI_RESID && epi != SET_EPI_ROPE_KV && epi != SET_EPI_SILU_QAH && epi != SET_EPI_SILU_QA) return false;
    const SetPlan p = set_plan(w, N, epi);
    if (epi == SET_EPI_SILU_QA && p.cw != 1) return false;                // (whole-block workgroups are instantiated for unshared rings)
    return p.lds <= SET_LDS_CAP && set_plan_instantiated(p.nc, p.cw);
}
// a caller's forced plan (llamahip_op_gemv_set_q4_0) is launched exactly as asked or refused here, on the host, with the reason in `why`:
// never promoted to a neighbouring pair, never clamped, never replaced by the LDS rule
bool set_force_check(const SetShape &w, int N, int epi, const SetForce &f, char *why, size_t why_cap) {
    const bool silu = epi == SET_EPI_SILU_QAH || epi == SET_EPI_SILU_QA;
    if (f.nc < 1 || f.cw < 1 || !set_plan_instantiated(f.nc, f.cw)) { snprintf(why, why_cap, "k_gemv_set<%d,%d> is not instantiated", f.nc, f.cw); return false; }
    if (f.rgw < 0 || f.rgw > 8) { snprintf(why, why_cap, "rgw %d outside 0 (derived) .. 8", f.rgw); return false; }
    if (silu && f.cw != 1) { snprintf(why, why_cap, "the SiLU epilogues take unshared rings only (cw 1, got %d)", f.cw); return false; }
    if (silu && f.rgw != 0 && f.rgw != (epi == SET_EPI_SILU_QAH ? 4 : 8)) {
        snprintf(why, why_cap, "the SiLU epilogues keep their rgw (%d), got %d", epi == SET_EPI_SILU_QAH ? 4 : 8, f.rgw); return false;
    }
    if (!silu && f.rgw * f.cw > 8) { snprintf(why, why_cap, "rgw %d x cw %d > 8 waves per workgroup", f.rgw, f.cw); return false; }
    const int want_ncg = (N + f.nc * f.cw - 1) / (f.nc * f.cw);
    if (f.ncg != 0 && f.ncg != want_ncg) { snprintf(why, why_cap, "ncg %d: %d rows in groups of %d x %d columns are %d groups", f.ncg, N, f.nc, f.cw, want_ncg); return false; }
    SetForce s = f;
    s.strict = true;
    const SetPlan p = set_plan(w, N, epi, &s);
    if (p.nc != f.nc || p.cw != f.cw || p.ncg != want_ncg || (f.rgw != 0 && p.rgw != f.rgw)) {
        snprintf(why, why_cap, "the plan would run as <%d,%d> ncg %d rgw %d", p.nc, p.cw, p.ncg, p.rgw); return false;
    }
    if (p.lds > SET_LDS_CAP) { snprintf(why, why_cap, "%zu bytes of LDS, the kernel's cap is %zu", p.lds, SET_LDS_CAP); return false; }
    return true;
}
// workgroups and threads of a plan's launch
void set_launch_shape(const SetShape &w, const SetPlan &p, int epi, int &grid, int &nthreads) {
    const int nwg = epi == SET_EPI_SILU_QAH ? (w.ngroups / 8 + 7) / 8 * 16 : (w.ngroups + p.rgw - 1) / p.rgw;      // (SET_EPI_SILU_QA: rgw = 8, a workgroup per block)
    grid = p.ncg == 1 ? nwg : (nwg + 7) / 8 * 8 * p.ncg;
    nthreads = p.rgw * p.cw * 64;
}
// host-only: what launch_set_any launches for (w, N, epi[, force]) -- out = { nc, cw, ncg, rgw, LDS bytes, grid, threads }; false = nothing
bool set_launch_query(const SetShape &w, int N, int epi, const SetForce *force, long out[7]) {
    const SetPlan p = set_plan(w, N, epi, force);
    if (p.lds > SET_LDS_CAP || !set_plan_instantiated(p.nc, p.cw)) return false;
    int grid = 0, nthreads = 0;
    set_launch_shape(w, p, epi, grid, nthreads);
    out[0] = p.nc; out[1] = p.cw; out[2] = p.ncg; out[3] = p.rgw; out[4] = (long) p.lds; out[5] = grid; out[6] = nthreads;
    return true;
}
// host-only query (tests, no device needed): the plan for N rows against an M x K matrix -- out = { nc, cw, ncg, rgw, LDS bytes }
bool gemv_set_plan_query(int M, int K, bool interleaved, int N, int epi, long out[5]) {
    SetShape w;
    w.tiles = true; w.M = M; w.K = K; w.ngroups = (M + 7) / 8; w.nchunks = (K + 255) / 256; w.gmapF8 = interleaved ? w.ngroups / 2 : 0;
    if (!set_applies(w, N, epi)) return false;
    const SetPlan p = set_plan(w, N, epi);
    out[0] = p.nc; out[1] = p.cw; out[2] = p.ncg; out[3] = p.rgw; out[4] = (long) p.lds;
    return true;
}

}  // namespace lh
