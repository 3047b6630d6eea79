// set_plan.h -- the host-only half of the few-row Q4_0 mat-mul k_gemv_set (set_plan.cpp): its launch plan, the overrides of the plan
// (the LLAMAHIP_SET_PLAN* switches, llamahip_op_gemv_set_q4_0's forced plans) and the launch's grid / threads.  No device header:
// tools/host_sanitize.cpp compiles it under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

// the ring depth, the operand prefetch distance and the timeline probe of k_gemv_set (gemv_set.hip explains them): measurement builds
// override them for the whole library, the kernel and its LDS arithmetic alike
#ifndef LH_SET_DR
#define LH_SET_DR 4
#endif
#ifndef LH_SET_PF
#define LH_SET_PF 1
#endif
#ifndef LH_SET_PROBE
#define LH_SET_PROBE 0
#endif

namespace lh {

constexpr int SET_DR = LH_SET_DR;
constexpr int SET_PF = LH_SET_PF, SET_NB = SET_PF + 1;
constexpr int SET_TILE_BYTES = 1280;                 // = TILE_BYTES of llamahip_internal.h (gemv_set.hip asserts it)
enum { SET_EPI_STORE = 0, SET_EPI_RESID = 1, SET_EPI_SILU_QA = 2, SET_EPI_ROPE_KV = 3, SET_EPI_SILU_QAH = 7 };      // = EPI_* (asserted there too)
// the short evals: up to 60 rows (measured crossover against the row-per-lane kernel at 7B shapes, round 1: +25 % at 33 rows, +7 % at 56, -1 % at
// 63; k_gemv_set against k_gemm_skinny at 20 / 24 / 32 / 48 / 60 rows: -5.5 / -5.5 / -0.7 / -5.2 / -6.3 % per eval, profiles/r05_y_rows_max.txt)
constexpr int SET_ROWS_MAX = 60;
constexpr size_t SET_LDS_CAP = 160 * 1024;

// what the plan needs of a QMat: its shape, the w1|w3 interleave and whether the tile copy exists
struct SetShape { int M = 0, K = 0, ngroups = 0, nchunks = 0, gmapF8 = 0; bool tiles = false; };
struct SetPlan { int nc = 0, cw = 0, rgw = 0, ncg = 1; size_t lds = 0; };
// An override of set_plan's rule: the LLAMAHIP_SET_PLAN* switches and llamahip_op_gemv_set_q4_0's forced plans travel as this.  ncg / rgw 0:
// derived.  strict (the op): set_force_check has admitted the plan and it runs as asked -- no neighbouring pair, no LDS fallback.
struct SetForce { int nc = 0, cw = 0, ncg = 0, rgw = 0; bool strict = false; };

size_t set_lds_bytes(const SetShape &w, int ncols_group, int nc, int cw, int rgw);
bool set_plan_instantiated(int nc, int cw);          // the (NC, CW) pairs k_gemv_set is instantiated for (launch_set_any's dispatch list)
SetPlan set_plan(const SetShape &w, int N, int epi, const SetForce *force = nullptr);
bool set_applies(const SetShape &w, int N, int epi);
bool set_force_check(const SetShape &w, int N, int epi, const SetForce &f, char *why, size_t why_cap);      // false: the reason in why
void set_launch_shape(const SetShape &w, const SetPlan &p, int epi, int &grid, int &nthreads);
bool set_launch_query(const SetShape &w, int N, int epi, const SetForce *force, long out[7]);      // { nc, cw, ncg, rgw, LDS, grid, threads } of the launch
bool gemv_set_plan_query(int M, int K, bool interleaved, int N, int epi, long out[5]);      // the (nc, cw, ncg, rgw, LDS) plan, false = the kernel does not take the shape

}  // namespace lh
