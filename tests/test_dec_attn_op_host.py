"""CPU: the host half of the one-row decode attention (csrc/dec_attn_plan.cpp) and of llamahip_op_dec_attention.

  * With no force and no switch set the plan equals a restatement of what launch_dec_attn / launch_qkv_attn computed inline before the plan
    became a function (parent_plan / parent_qkv_geom below, written from that source): every model handle launches what it launched.
  * A forced value the kernels cannot take, and every call the op must not launch, is refused with its reason before a device is looked for.
  * The CPU half of tests/test_gpu_dec_attn_op.py: the committed case tables equal what the searches of tests/dec_attn_cases.py return, every
    kernel, every chains-per-workgroup count and every named edge has its case, every case passes the op's host checks (the last refusal is
    the missing device), and every regime input has the property it is named for in the oracle's own arithmetic."""
import os
import subprocess

import numpy as np
import pytest

import attn_cases
import dec_attn_cases as dc
import synth
import variants

NO_DEVICE = "no HIP device available"
LLAMA = [(4096, 32), (5120, 40), (6656, 52), (8192, 64)]
SYNTH = [(d, H) for d, _ in variants.SYNTH_WIDTHS for H in range(1, d // 32 + 1) if d % H == 0 and (d // H) % 32 == 0 and d // H <= 256]
CTXS = (64, 192, 512, 1024, 2048, 4096)


def test_new_symbols_are_declared_and_exported(L):
    for fn in ("llamahip_op_dec_attention", "llamahip_op_qkv_attn", "llamahip_debug_dec_attn_plan", "llamahip_debug_qkv_attn_plan"):
        assert fn in L.declared_symbols() and hasattr(L.lib(), fn), fn


# ------------------------------------------------------------------------------------------------ the plan is unchanged
def parent_plan(d, H, n_ctx, nth, long_ctx, have_sync, have_xpart):
    """launch_dec_attn before dec_attn_plan existed, restated: (kernel, split, cpw, SR, NS, LDS, workgroups, threads) of the soft_max . V launch"""
    dh = d // H
    nsl = (n_ctx + 31) // 32

    def valid(s):
        cpw = (nth + s - 1) // s
        return 1 <= s <= nth and (s - 1) * cpw < nth
    if long_ctx and 1 <= nth <= 32 and n_ctx <= 4096 and dh % 32 == 0:
        W, split = H * (dh // 32), 1
        if have_xpart and W % 8 == 0:
            while W * split * 2 <= 256 and valid(split * 2):
                split *= 2
        cpw = (nth + split - 1) // split
        SR = 4 * 128 // cpw
        lds = 32 * 8 + (((n_ctx + 3) & ~3) + nth * 32) * 4 + 2 * cpw * SR * 128
        if dh == 128 and have_xpart and H % 8 == 0:
            sp = 1
            while H * sp * 2 <= 256 and valid(sp * 2):
                sp *= 2
            cpwd = (nth + sp - 1) // sp
            if cpwd <= 3:
                fixed = 32 * 8 + (((n_ctx + 3) & ~3) + nth * 128) * 4 + 64
                NS = max(2, min((156 * 1024 - fixed) // (cpwd * 4096), 256))
                return ("pv_dma", sp, cpwd, 0, NS, fixed + NS * cpwd * 4096, H * sp, 512)
        return ("pv_stream", split, cpw, SR, 0, lds, W * split, 1024)
    lds_pv = 32 * 8 + (n_ctx + nth * 32 + 16) * 4
    if have_sync and nth <= 8 and dh % 32 == 0 and dh <= 256 and H % 8 == 0 and n_ctx <= 1024:
        return ("attn_x", 1, nth, 0, 0, max(lds_pv, 2 * dh * 4), H * (dh // 32 + nsl), 256)
    return ("pv_blk", 1, nth, 0, 0, lds_pv, H * (dh // 32), (32 * min(nth, 32) + 63) // 64 * 64)


def handle_args(H, dh, n_ctx, nth, sched, placed):
    """(long_ctx, have_sync, have_xpart) as the decode step hands them to launch_dec_attn under attention schedule 0 / 1 / 2 on a handle whose
    load-time placement self-test passed (placed: it allocated the counters and the partial-sum buffer) or not"""
    placed = placed and H % 8 == 0
    long_attn = sched == 2 and 1 <= nth <= 32 and n_ctx <= 4096 and dh % 32 == 0
    two = sched == 1 or (sched == 2 and not long_attn)
    return long_attn, placed and not two, long_attn and placed


def test_the_rule_launches_what_launch_dec_attn_launched(L):
    n = 0
    kernels = set()
    for d, H in LLAMA + SYNTH:
        for n_ctx in CTXS:
            for nth in range(1, 65):
                for sched in (0, 1, 2):
                    for placed in (True, False):
                        args = handle_args(H, d // H, n_ctx, nth, sched, placed)
                        got = L.dec_attn_plan(d, H, n_ctx, nth, *args)
                        assert tuple(got) == parent_plan(d, H, n_ctx, nth, *args), (d, H, n_ctx, nth, sched, placed, got)
                        kernels.add(got.kernel)
                        n += 1
    assert kernels == set(L.DEC_ATTN_KERNELS) and n > 20000


def parent_qkv_geom(L, d, H, n_ctx, nth, n_part):
    """qkv_attn_applies + launch_qkv_attn before the geometry moved, restated on the mat-vec's own plan (llamahip_debug_gemv_plan)"""
    dh = d // H
    if H % 8 or d % H or dh % 32 or dh > 256 or nth > 8:
        return None
    p = L.gemv_plan(3 * d, d, 2, 0)                                             # (PREP_NORM, EPI_STORE)
    if p is None:
        return None
    nw, pg, depth, ring, grid, lds = p
    if nw != 4 or not ring or (depth, pg) not in ((8, 1), (10, 2), (4, 2)):
        return None
    lds_pv = 32 * 8 + (n_ctx + nth * 32 + 16) * 4
    return (4 if 0 < n_part <= 512 else 2, depth, pg, grid + H * ((n_ctx + 31) // 32 + dh // 32), max(lds, lds_pv, 2 * dh * 4))


def test_the_fused_launch_keeps_its_geometry(L):
    inst = set()
    for d, H in LLAMA + SYNTH + [(4096, 16), (4096, 64), (4096, 128), (8192, 32)]:
        for n_ctx in CTXS:
            for nth in (1, 3, 5, 8, 9):
                for n_part in (0, 1, 64, 512, 513):
                    got = L.qkv_attn_plan(d, H, n_ctx, nth, n_part)
                    assert got == parent_qkv_geom(L, d, H, n_ctx, nth, n_part), (d, H, n_ctx, nth, n_part, got)
                    if got:
                        inst.add(got[1:3])
    assert inst == {(8, 1), (10, 2), (4, 2)}
    assert L.qkv_attn_plan(4096, 32, 512, 8)[1:3] == (8, 1) and L.qkv_attn_plan(5120, 40, 512, 8)[1:3] == (10, 2) and L.qkv_attn_plan(8192, 64, 512, 8)[1:3] == (4, 2)
    assert L.qkv_attn_plan(6656, 52, 512, 8) is None                                # (52 heads: no multiple of 8)


# ------------------------------------------------------------------------------------------------ refusals
PLAN_REFUSALS = [
    (dict(d=1024, H=8, n_ctx=400, nth=5, long_ctx=True, force=dict(split=4)), "split 4 is not valid for n_threads 5"),
    (dict(d=1024, H=8, n_ctx=400, nth=5, long_ctx=True, force=dict(split=6)), "split 6 is not valid"),
    (dict(d=1024, H=8, n_ctx=400, nth=8, long_ctx=True, force=dict(split=2, dma=1)), "4 > 3 chains per workgroup"),
    (dict(d=1024, H=8, n_ctx=400, nth=3, long_ctx=True, force=dict(ns=1, dma=1)), "ns 1 outside 2 .. 256"),
    (dict(d=1024, H=8, n_ctx=400, nth=3, long_ctx=True, force=dict(ns=257, dma=1)), "ns 257 outside 2 .. 256"),
    (dict(d=1024, H=8, n_ctx=400, nth=3, long_ctx=True, force=dict(ns=256, dma=1)), "the kernels' cap is 163840"),
    (dict(d=1024, H=8, n_ctx=4096, nth=32, long_ctx=True, force=dict(split=16, ns=20, dma=1)), "the kernels' cap is 163840"),
    (dict(d=1024, H=8, n_ctx=400, nth=3, long_ctx=True, force=dict(ns=3, dma=0)), "ns is the ring of k_dec_pv_dma"),
    (dict(d=512, H=8, n_ctx=400, nth=3, long_ctx=True, force=dict(dma=1)), "k_dec_pv_dma takes head size 128 (got 64)"),
    (dict(d=512, H=4, n_ctx=400, nth=3, long_ctx=True, force=dict(dma=1)), "H % 8 == 0 (H 4)"),
    (dict(d=1024, H=8, n_ctx=400, nth=3, long_ctx=True, have_xpart=False, force=dict(dma=1)), "the partial-sum buffer"),
    (dict(d=1024, H=8, n_ctx=400, nth=3, long_ctx=True, force=dict(stage_rows=2, dma=1)), "no stage_rows"),
    (dict(d=1024, H=8, n_ctx=400, nth=4, long_ctx=True, force=dict(split=2, stage_rows=257, dma=0)), "stage_rows 257 x cpw 2 > 512"),
    (dict(d=1024, H=8, n_ctx=400, nth=4, long_ctx=True, have_xpart=False, force=dict(split=2, dma=0)), "split 2 needs the partial-sum buffer"),
    (dict(d=96, H=1, n_ctx=400, nth=4, long_ctx=True, force=dict(split=2, dma=0)), "H dh / 32 = 3 a multiple of 8"),
    (dict(d=1024, H=8, n_ctx=400, nth=5, force=dict(split=2)), "belong to the long-context kernels"),
    (dict(d=1024, H=8, n_ctx=400, nth=5, force=dict(ns=2)), "belong to the long-context kernels"),
    (dict(d=1024, H=8, n_ctx=4097, nth=5, long_ctx=True, force=dict(dma=1)), "belong to the long-context kernels"),
    (dict(d=1024, H=8, n_ctx=400, nth=33, long_ctx=True, force=dict(stage_rows=1)), "belong to the long-context kernels"),
    (dict(d=1024, H=8, n_ctx=400, nth=5, long_ctx=True, force=dict(split=-1)), "is the library's rule"),
    (dict(d=1024, H=8, n_ctx=400, nth=5, long_ctx=True, force=dict(dma=2)), "dma is 0 or 1"),
    (dict(d=1024, H=3, n_ctx=400, nth=5, force={}), "multiples of 32 up to 256"),
    (dict(d=1024, H=2, n_ctx=400, nth=5, force={}), "multiples of 32 up to 256"),
    (dict(d=1024, H=8, n_ctx=400, nth=65, force={}), "n_threads 65 outside 1 .. 64"),
    (dict(d=1024, H=8, n_ctx=50000, nth=8, have_sync=False, force={}), "the kernels' cap is 163840"),
    (dict(d=1024, H=8, n_ctx=0, nth=8), "must be >= 1"),
    (dict(d=1024, H=8, n_ctx=64, nth=0), "must be >= 1"),
]


@pytest.mark.parametrize("kw,msg", PLAN_REFUSALS, ids=[m for _, m in PLAN_REFUSALS])
def test_a_forced_value_the_kernels_cannot_take_is_refused_with_the_reason(L, kw, msg):
    kw = dict(kw)
    with pytest.raises(L.LlamaHipError) as e:
        L.dec_attn_plan(kw.pop("d"), kw.pop("H"), kw.pop("n_ctx"), kw.pop("nth"), **kw)
    assert msg in str(e.value), str(e.value)


def test_forced_plans_run_as_asked(L):
    """every forced value is the plan's own; the switches' lenient form (no force) is not consulted"""
    p = L.dec_attn_plan(1024, 8, 400, 7, long_ctx=True, force=dict(split=3, ns=2, dma=1))
    assert p == ("pv_dma", 3, 3, 0, 2, 32 * 8 + (400 + 7 * 128) * 4 + 64 + 2 * 3 * 4096, 24, 512)
    p = L.dec_attn_plan(256, 8, 100, 5, long_ctx=True, force=dict(split=3, stage_rows=3, dma=0))
    assert p == ("pv_stream", 3, 2, 3, 0, 32 * 8 + (100 + 5 * 32) * 4 + 2 * 2 * 3 * 128, 24, 1024)
    assert L.dec_attn_plan(1024, 8, 2048, 8, long_ctx=True, force=dict(dma=0)).kernel == "pv_stream"
    assert L.dec_attn_plan(1024, 8, 2048, 8, long_ctx=True, force={}).kernel == "pv_dma"


def call(L, path="x", H=8, dh=32, n_ctx=64, nth=2, steps=((0, 0, 1),), force=None, **kw):
    d = H * dh
    Kc, Vc = np.zeros((n_ctx, d), np.float32), np.zeros((n_ctx, d), np.float32)
    return L.op_dec_attention(path, [(np.zeros(3 * d, np.float32),) + tuple(s) for s in steps], H, Kc, Vc, nth, force=force, **kw)


OP_REFUSALS = [
    (dict(path=3), "unknown path 3"),
    (dict(steps=((0, 0, 0),) * 65), "n_steps 65 outside 1 .. 64"),
    (dict(steps=((64, 0, 0),)), "n_past 64 outside [0, n_ctx = 64)"),
    (dict(steps=((0, 0, 0), (-1, 0, 0))), "step 1: n_past -1 outside"),
    (dict(steps=((0, 250, 0),)), "layer 250 outside 0 .. 249"),
    (dict(steps=((0, -1, 0),)), "layer -1 outside 0 .. 249"),
    (dict(H=3, dh=32), "path 0 refused"),
    (dict(H=4, dh=32), "path X takes H % 8 == 0, n_threads <= 8 and n_ctx <= 1024"),
    (dict(nth=9), "path X takes H % 8 == 0, n_threads <= 8 and n_ctx <= 1024"),
    (dict(n_ctx=1025), "path X takes H % 8 == 0, n_threads <= 8 and n_ctx <= 1024"),
    (dict(force=dict(split=2)), "belong to the long-context kernels"),
    (dict(path="stream", nth=33), "paths STREAM / DMA take n_threads <= 32 and n_ctx <= 4096"),
    (dict(path="dma", dh=128, n_ctx=4100), "belong to the long-context kernels (n_threads <= 32, n_ctx <= 4096)"),
    (dict(path="stream", force=dict(dma=1)), "force dma 1 contradicts path STREAM"),
    (dict(path="dma", dh=128, force=dict(dma=0)), "force dma 0 contradicts path DMA"),
    (dict(path="dma", dh=64), "k_dec_pv_dma takes head size 128 (got 64)"),
    (dict(path="dma", dh=128, nth=8, force=dict(split=2)), "4 > 3 chains per workgroup"),
    (dict(path="dma", dh=128, nth=24, H=64), "> 3 chains per workgroup of k_dec_pv_dma"),      # (64 heads: the rule splits by 4 and the path refuses rather than fall back)
    (dict(path="dma", dh=128, nth=3, force=dict(ns=1)), "ns 1 outside 2 .. 256"),
    (dict(path="dma", dh=128, nth=3, force=dict(ns=200)), "the kernels' cap is 163840"),
    (dict(path="stream", nth=5, force=dict(split=4)), "split 4 is not valid for n_threads 5"),
    (dict(path="stream", nth=4, force=dict(split=2, stage_rows=300)), "stage_rows 300 x cpw 2 > 512"),
    (dict(path="stream", nth=4, force=dict(split=2), steps=((5, 1, 1), (6, 1, 0))), "layer 1 again under one epoch"),
    (dict(path="dma", dh=128, nth=4, force=dict(split=2), steps=((5, 0, 0), (6, 1, 0), (7, 0, 0))), "step 2: layer 0 again under one epoch"),
]


@pytest.mark.parametrize("kw,msg", OP_REFUSALS, ids=[m for _, m in OP_REFUSALS])
def test_the_op_refuses_before_it_looks_for_a_device(L, kw, msg):
    with pytest.raises(L.LlamaHipError) as e:
        call(L, **kw)
    assert msg in str(e.value) and NO_DEVICE not in str(e.value), str(e.value)


def test_null_operands_are_refused(L):
    import ctypes as C
    err = C.create_string_buffer(512)
    z = np.zeros(64 * 256, np.float32)
    i = np.zeros(4, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    full = [ptr(z), 1, ptr(i), ptr(i), ptr(i), 0, 256, 8, 64, ptr(z), ptr(z), 2, 0, None, ptr(z), None, ptr(i), None, err, len(err)]
    for k in (0, 2, 3, 4, 9, 10, 14, 16):
        a = list(full)
        a[k] = None
        assert L.lib().llamahip_op_dec_attention(*a) != 0 and b"null operand" in err.value, (k, err.value)
    full[1] = 0
    assert L.lib().llamahip_op_dec_attention(*full) != 0 and b"n_steps 0 outside 1 .. 64" in err.value, err.value


# ------------------------------------------------------------------------------------------------ the case tables
def all_cases():
    return dc.X_CASES + dc.STREAM_CASES + dc.DMA_CASES + dc.REGIME_CASES


def test_the_committed_tables_are_what_the_searches_return(L):
    plan_of = lambda c: dc.case_plan(L, c)
    assert dc.X_CASES == dc.find_x()
    assert dc.STREAM_CASES == dc.find_stream(plan_of)
    assert dc.DMA_CASES == dc.find_dma(plan_of)


def test_every_case_passes_the_host_checks(L):
    """... with the plan its table names it for; without a GPU the last refusal is the missing device"""
    want = {"x": "attn_x", "stream": "pv_stream", "dma": "pv_dma"}
    for c in all_cases():
        p = dc.case_plan(L, c)
        assert p is not None and p.kernel == want[c.path] and (c.path == "x" or p.grid <= dc.ONE_ROUND), (c, p)
        assert 0 <= c.n_past < c.n_ctx and c.regime in attn_cases.REGIMES
    for s in dc.SEQS:
        p = dc.case_plan(L, dc.Case(s.path, "plain", s.H, s.dh, s.n_ctx, 0, s.nth, s.force))
        assert p is not None and p.kernel == want[s.path], (s, p)
    for c in (dc.X_CASES[0], dc.STREAM_CASES[0], dc.DMA_CASES[0]):
        f = c.force or (0, 0, 0)
        try:
            call(L, c.path, c.H, c.dh, c.n_ctx, c.nth, steps=((c.n_past, 0, 1),), force=dict(split=f[0], stage_rows=f[1], ns=f[2]))
        except L.LlamaHipError as e:
            assert NO_DEVICE in str(e), f"{dc.case_id(c)}: {e}"          # the LAST refusal: everything before it passed


def test_coverage_tables(L):
    """every kernel, every chains-per-workgroup count of the DMA kernel and every edge has at least one case, named here"""
    fx = set().union(*(dc.x_features(c) for c in dc.X_CASES))
    for nth in dc.X_NTH:
        assert ("early", nth, True) in fx and ("early", nth, False) in fx, nth          # both sides of the early V prefetch
        assert nth == 1 or ("empty_chains", nth) in fx, nth                            # T < nth
    for sh in dc.X_SHAPES:
        for n_ctx in dc.X_CTX:
            assert ("shape", *sh) in fx and ("n_ctx", n_ctx) in fx
    assert {("n_past", p) for p in (0, 1, 30, 31, 32, 33, 63, 64, "last")} <= fx      # both sides of the slice edges 32 and 64
    assert {("slice", "last key of a slice"), ("slice", "first key of a slice"), ("slice", "second key of a slice")} <= fx
    assert any(c.n_ctx == 1024 and c.n_past == 1023 for c in dc.X_CASES)              # the kernel's limit

    fs = set().union(*(dc.stream_features(c, dc.case_plan(L, c)) for c in dc.STREAM_CASES))
    for nth in dc.STREAM_NTH:
        assert ("pair", nth, "rule") in fs
        for split in dc.STREAM_SPLITS:
            if dc.split_valid(nth, split):
                assert ("pair", nth, split) in fs, (nth, split)
    assert {("stage_rows", v) for v in (1, 2, 3, "rule")} <= fs and {("n_ctx", v) for v in dc.STREAM_CTX} <= fs
    assert {("n_past", v) for v in (0, "nth-2", 1023, 1024, "last")} <= fs and {("shape", *sh) for sh in dc.STREAM_SHAPES} <= fs
    assert ("ragged last workgroup",) in fs and ("empty_chains",) in fs and {("stages", v) for v in ("one", "two", "odd", "even")} <= fs

    plans = {c: dc.case_plan(L, c) for c in dc.DMA_CASES}
    fd = set().union(*(dc.dma_features(c, p) for c, p in plans.items()))
    assert {p.cpw for p in plans.values()} == {1, 2, 3}
    assert {("nth", n) for n in dc.DMA_NTH} <= fd and {("ns", v) for v in (2, 3, "rule")} <= fd and {("n_ctx", v) for v in dc.DMA_CTX} <= fd
    assert {("ring", "wrapped"), ("ring", "not wrapped"), ("tail clamp",), ("empty_chains",), ("n_past", 0)} <= fd
    assert {("tail clamp at the rule's NS", 2048), ("tail clamp at the rule's NS", 4096)} <= fd
    assert {("ragged last workgroup", 5, 2), ("ragged last workgroup", 7, 3)} <= fd
    for nloc in (1, 2, 3):                                                             # stage counts on both sides of F = 60 / (2 nloc)
        assert ("F", nloc, "more stages than F") in fd and ("F", nloc, "at most F stages") in fd, nloc
    # in production (2 048 keys, 8 threads) the ring wraps in every launch: that case is in the table with the rule's NS
    assert any(c.n_ctx >= 2048 and not (c.force and c.force[2]) and dc.dma_geometry(c, p)["wrapped"] for c, p in plans.items())
    # the regimes on the split kernels: one wrapped and one unwrapped ring each
    for r in ("negzero", "wide", "ties"):
        w = {dc.dma_geometry(c, dc.case_plan(L, c))["wrapped"] for c in dc.REGIME_CASES if c.path == "dma" and c.regime == r}
        assert w == {True, False}, (r, w)
    assert {c.regime for c in dc.REGIME_CASES if c.path == "x"} == set(attn_cases.REGIMES)
    # sequences: a lower position after a higher one on the same layer after a bump; two layers under one epoch; the epoch's wrap
    for s in dc.SEQS:
        if s.path != "x":
            assert any(b[2] == a[2] and b[1] < a[1] and b[3] for a, b in zip(s.steps, s.steps[1:])) or len({st[2] for st in s.steps}) > 1
    wraps = [s for s in dc.SEQS if s.epoch0 == 0x00FFFFFE]
    assert wraps and all(sum(st[3] for st in s.steps) >= 3 for s in wraps)
    e = 0x00FFFFFE
    seen = [e := dc.next_epoch(e) for _ in range(3)]
    assert seen == [0x00FFFFFF, 0x01000001, 0x01000002]


def test_regime_inputs_have_the_property_they_are_named_for(oracle):
    """ties: two keys at the maximum in every head; wide: an exp-table entry of 0 and a subnormal one; negzero: a merged column of -0;
    zeroq: q exactly 0 -- in the oracle's own result.  A case that loses its property must be replaced, not the GPU test loosened."""
    todo = [(c.regime, c.H, c.dh, c.n_ctx, c.n_past, c.nth, dc.case_id(c)) for c in dc.REGIME_CASES]
    seen = set()
    for regime, H, dh, n_ctx, n_past, nth, name in todo:
        if (regime, H, dh, n_ctx, n_past, nth) in seen:
            continue
        seen.add((regime, H, dh, n_ctx, n_past, nth))
        qkv, Kc, Vc = dc.first_inputs(regime, H, dh, n_ctx, n_past)
        ref, _, _ = dc.reference(oracle, [(qkv[0], n_past, 0, 1)], Kc, Vc, H, nth)
        want, _, qr, Kw, _ = ref[0]
        assert dc.regime_property(regime, qr, Kw, want, H, n_past) is None, (name, dc.regime_property(regime, qr, Kw, want, H, n_past))
        if regime == "leak":
            assert np.all(Kw[n_past + 1:].view(np.uint32) == attn_cases.CANARY)      # rows above the position hold the NaN canary


def test_fused_case_tables_and_properties(L, oracle):
    """the three instances have their smallest widths and a case each; the table is the search's; every activation row is order-proof under
    both forms of the second moment (NORM and NORMP then give one row); every regime input has its property in the oracle's result"""
    import prep_cases as pc
    assert dc.find_qkv_widths(lambda d, H: L.qkv_attn_plan(d, H, 1280, 8)) == dc.QKV_WIDTHS and dc.QKV_CASES == dc.find_qkv()
    cases = dc.QKV_CASES + dc.QKV_WIDE_CASES
    assert {L.qkv_attn_plan(c.d, c.H, c.n_ctx, c.nth, c.nparts)[1:3] for c in cases} == {(8, 1), (10, 2), (4, 2)}
    fq = set().union(*(dc.qkv_features(c) for c in dc.QKV_CASES))
    assert {("H", h) for h in (16, 32, 64, 128)} <= fq and {("nth", n) for n in (1, 3, 5, 8)} <= fq and {("parts", n) for n in (0, 1, 64, 512)} <= fq
    assert {("n_past", p) for p in (0, 31, 32, 33, 500, 1279)} <= fq and {("n_ctx", 1280), ("n_ctx", 2048)} <= fq and {("regime", r) for r in dc.QKV_REGIMES} <= fq
    for d in (4096, 4608, 6144):
        for step in range(3):
            assert pc.norm_proof_both(dc.qkv_x(d, step)), (d, step)
    seen = set()
    for c in cases:
        key = (c.regime, c.d, c.H, c.n_ctx, c.n_past)
        if c.regime == "plain" or key in seen:
            continue
        seen.add(key)
        w, norm_w, x, part_in, Kc, Vc, qkv = dc.qkv_inputs(oracle, c)
        ref, _, _ = dc.reference(oracle, [(qkv, c.n_past, 0, 1)], Kc, Vc, c.H, c.nth)
        want, _, qr, Kw, _ = ref[0]
        assert dc.qkv_regime_property(c, qkv, qr, Kw, want) is None, (dc.qkv_case_id(c), dc.qkv_regime_property(c, qkv, qr, Kw, want))
    for s in dc.QKV_SEQS:
        for a, b in zip(s.steps, s.steps[1:]):
            assert b[2] or b[1] != a[1]                                              # a tag is spent once per epoch


QKV_REFUSALS = [
    (dict(tagged_in=True), "PREP_NORM_TAG waits on another pipeline stage"),
    (dict(H=20), "H 20 must be a multiple of 8"),
    (dict(H=8), "head size 512"),
    (dict(nth=9), "n_threads 9 > 8"),
    (dict(d=256, H=8), "no instance for d 256"),
    (dict(d=128, H=4), "d 128 must be a positive multiple of 256"),
    (dict(n_ctx=5000), "n_ctx 5000 outside 1 .. 4096"),
    (dict(steps=((64, 0, 1, 0),)), "n_past 64 outside [0, n_ctx = 64)"),
    (dict(steps=((0, 250, 1, 0),)), "layer 250 outside 0 .. 249"),
    (dict(steps=((0, 0, 1, 513),)), "n_part 513 outside 0 .. 512"),
    (dict(steps=((0, 2, 1, 0), (1, 2, 0, 0))), "layer 2 again under one epoch"),
]


@pytest.mark.parametrize("kw,msg", QKV_REFUSALS, ids=[m for _, m in QKV_REFUSALS])
def test_the_fused_op_refuses_before_it_looks_for_a_device(L, kw, msg):
    kw = dict(kw)
    d, H, n_ctx, nth = kw.pop("d", 4096), kw.pop("H", 32), kw.pop("n_ctx", 64), kw.pop("nth", 8)
    steps = [(np.zeros(d, np.float32), np.zeros((n, 2)) if n else None, p, l, b) for p, l, b, n in kw.pop("steps", ((0, 0, 1, 0),))]
    w = np.zeros((3 * d, d // 32, 20), np.uint8)
    K = np.zeros((n_ctx, d), np.float32)
    with pytest.raises(L.LlamaHipError) as e:
        L.op_qkv_attn(w, np.ones(d, np.float32), steps, H, K, K.copy(), nth, **kw)
    assert msg in str(e.value) and NO_DEVICE not in str(e.value), str(e.value)


def test_sequences_step_through_evolving_caches(oracle):
    """a sequence's reference appends every step's row: after the steps the caches hold all of them, and a later step at a lower position
    sees the rows the earlier one left above it (not the canary)"""
    s = dc.SEQS[1]
    steps, Kc, Vc = dc.seq_inputs(s)
    ref, Kw, Vw = dc.reference(oracle, steps, Kc, Vc, s.H, s.nth)
    assert not np.any(Kw[[900, 3]].view(np.uint32) == attn_cases.CANARY) and np.all(Kw[901:].view(np.uint32) == attn_cases.CANARY)
    assert len(ref) == 2 and np.array_equal(ref[1][3][900], ref[0][3][900])           # the second step leaves the first one's row alone


def test_dec_attn_plan_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: dec_attn_plan.cpp (the rule over every head layout, thread count and context; every forced value admitted or refused on its
    own message buffer) compiled with -fsanitize=address,undefined into the stand-alone tools/host_sanitize and run there -- never loaded
    into python"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "asan"], check=True)
    src = open(os.path.join(csrc, "tools", "host_sanitize.cpp")).read()
    assert "dec_attn_plan(" in src and "qkv_attn_geom(" in src
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(csrc, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "decode attention host half" in r.stdout and "clean" in r.stdout, r.stdout + r.stderr
    assert "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
