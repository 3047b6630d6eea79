"""CPU: llamahip_op_gemv_set_q4_0 is exported and refuses, before it looks for a device, every call it must not launch, each naming its
limit.  Also the CPU half of tests/test_gpu_gemv_set_op.py: every case of tests/gemv_set_cases.py passes the op's host checks (the last refusal is the
missing device); the coverage tables of the `steps` and `auto` groups; the conditions on the inputs that make a misplaced
row, a lost exchange or a stale granule show in the reference; and the yardstick itself, on the base cases, tells each of those faults
from the right answer."""
import numpy as np
import pytest

import gemv_cases as gc
import gemv_set_cases as sc
import prep_cases as pc  # noqa: F401
from gemm_ref import Ref

NO_DEVICE = "no HIP device available"


def test_new_symbol_is_declared_and_exported(L):
    assert "llamahip_op_gemv_set_q4_0" in L.declared_symbols() and hasattr(L.lib(), "llamahip_op_gemv_set_q4_0")


def call(L, M=64, K=64, N=4, epi="store", x=True, **kw):
    """the op on zero operands of the given shape; what an epilogue needs is supplied unless the keyword says otherwise"""
    inter = kw.pop("interleaved", epi in ("silu_qa", "silu_qah", 2, 7))
    w = np.zeros((M, max(K, 0) // 32, 20), np.uint8)
    xs = np.zeros((max(N, 0), max(K, 0)), np.float32) if x is True else x
    if epi == "resid" and "resid" not in kw:
        kw["resid"] = np.zeros((N, M), np.float32)
    if epi == "rope_kv":
        d = kw.setdefault("d", M // 3)
        kw.setdefault("dh", 32)
        kw.setdefault("n_ctx", 64)
        for name in ("Kc", "Vc"):
            if name not in kw:
                kw[name] = np.zeros((kw.get("n_slots", 1), kw["n_ctx"], max(d, 1)), np.float32)
    if epi in ("silu_qa", "silu_qah"):
        Fp = (M // 2 + 255) // 256 * 256
        rows = kw.pop("out_rows", N + 1)
        kw.setdefault("out_A", np.zeros((rows, Fp // 4), np.uint32))
        kw.setdefault("out_d", np.zeros((rows, Fp // 32), np.float32))
    return L.op_gemv_set_q4_0(w, epi, xs, interleaved=inter, **kw)


POS9 = np.arange(9, dtype=np.int32)


@pytest.mark.parametrize("kw,msg", [
    (dict(epi=4), "unknown epilogue 4"), (dict(epi=6), "unknown epilogue 6"), (dict(epi=-1), "unknown epilogue -1"),
    (dict(N=1), "N 1 outside 2 .. 60 rows"), (dict(N=61), "N 61 outside 2 .. 60 rows"),
    (dict(K=0), "K 0 must be a positive multiple of 64"), (dict(K=96), "K 96 must be a positive multiple of 64"),
    (dict(M=96, epi="silu_qa"), "M = 2F = 96 is not a multiple of 64"),
    (dict(epi="silu_qa", interleaved=False), "SiLU epilogues take the interleaved"), (dict(interleaved=True), "SiLU epilogues take the interleaved"),
    (dict(epi="rope_kv", M=192, interleaved=True), "SiLU epilogues take the interleaved"),
    (dict(epi="resid", resid=None), "RESID needs resid"),
    (dict(y_stride=63), "y_stride 63 < M 64"), (dict(epi="resid", y_stride=0), "y_stride 0 < M 64"),
    (dict(epi="rope_kv", M=192, Kc=None), "ROPE_KV needs qr, Kc, Vc"), (dict(epi="rope_kv", M=192, Vc=None), "ROPE_KV needs qr, Kc, Vc"),
    (dict(epi="silu_qa", out_A=None), "SiLU epilogues need out_A, out_d"), (dict(epi="silu_qah", out_d=None), "SiLU epilogues need out_A, out_d"),
    (dict(epi="silu_qa", out_rows=3), "out_rows 3 < N 4"),
    (dict(epi="silu_qah", N=17), "SILU_QAH takes N <= 16 rows"),
    (dict(epi="silu_qah", layer=250), "layer 250 outside 0 .. 249"), (dict(epi="silu_qah", layer=-1), "layer -1 outside 0 .. 249"),
    (dict(x_prev=np.zeros((4, 64), np.float32)), "x_prev is SILU_QAH's"), (dict(epi="silu_qa", x_prev=np.zeros((4, 64), np.float32)), "x_prev is SILU_QAH's"),
    (dict(epi="rope_kv", M=192, d=32), "ROPE_KV takes M = 3 d .M 192, d 32."), (dict(epi="rope_kv", M=192, dh=48), "even head size dh 48"),
    (dict(epi="rope_kv", M=36, d=12, dh=4), "d a multiple of 8"),
    (dict(epi="rope_kv", M=192, n_ctx=0, Kc=np.zeros(1, np.float32), Vc=np.zeros(1, np.float32)), "n_ctx .0. and n_slots .1. must be >= 1"),
    (dict(epi="rope_kv", M=192, n_ctx=8, n_past=5), "n_past 5 \\+ N 4 rows outside n_ctx 8"), (dict(epi="rope_kv", M=192, n_past=-1), "n_past -1"),
    (dict(epi="rope_kv", M=192, row_pos=POS9[:4]), "row_pos and row_slot come together"),
    (dict(epi="rope_kv", M=192, N=17, row_pos=np.arange(17), row_slot=np.zeros(17)), "a row table takes N <= 16 rows"),
    (dict(epi="rope_kv", M=192, row_pos=POS9[:4], row_slot=[0, 1, 0, 0]), "row_slot.1. = 1 out of range .0, 1."),
    (dict(epi="rope_kv", M=192, n_ctx=8, row_pos=[0, 1, 8, 2], row_slot=[0, 0, 0, 0]), "row_pos.2. = 8 out of range .0, n_ctx = 8."),
    (dict(epi="rope_kv", M=192, n_slots=2, row_pos=[3, 1, 2, 3], row_slot=[1, 0, 0, 1]), "rows 0 and 3 both write position 3 of slot 1"),
    # forced plans: launched as asked or refused with the reason
    (dict(force=(1, 1)), "forced plan .nc 1, cw 1, rgw 0. refused .*k_gemv_set<1,1> is not instantiated"),
    (dict(force=(3, 2)), "k_gemv_set<3,2> is not instantiated"), (dict(force=(4, 3)), "k_gemv_set<4,3> is not instantiated"),
    (dict(force=(5, 2)), "k_gemv_set<5,2> is not instantiated"), (dict(force=(0, 0)), "k_gemv_set<0,0> is not instantiated"),
    (dict(force=(2, 2, 5)), "rgw 5 x cw 2 > 8 waves"), (dict(force=(1, 4, 3)), "rgw 3 x cw 4 > 8 waves"), (dict(force=(2, 1, 9)), "rgw 9 outside 0 .derived. .. 8"),
    (dict(epi="rope_kv", M=192, force=(2, 4, 4)), "rgw 4 x cw 4 > 8 waves"),
    (dict(epi="silu_qa", force=(2, 2)), "SiLU epilogues take unshared rings only .cw 1, got 2."), (dict(epi="silu_qah", force=(1, 4)), "unshared rings only"),
    (dict(epi="silu_qa", force=(2, 1, 4)), "SiLU epilogues keep their rgw .8., got 4"), (dict(epi="silu_qah", force=(2, 1, 8)), "keep their rgw .4., got 8"),
    (dict(K=22016, N=16, force=(4, 4)), "bytes of LDS, the kernel's cap is 163840"), (dict(K=13824, N=8, force=(2, 4)), "bytes of LDS, the kernel's cap is 163840"),
    # shapes gemv_set_applies refuses: a row so wide that not even one column fits the LDS
    (dict(K=147456), "k_gemv_set does not take M 64, K 147456, N 4 under epilogue 0"),
])
def test_refusals_need_no_device(L, kw, msg):
    with pytest.raises(L.LlamaHipError, match=msg) as e:
        call(L, **kw)
    assert NO_DEVICE not in str(e.value)


def test_null_weights_and_rows_are_refused(L):
    import ctypes as C
    x = np.zeros((4, 64), np.float32)
    xp = x.ctypes.data_as(C.c_void_p)
    for w, xs in ((None, xp), (xp, None)):
        err = C.create_string_buffer(256)
        rc = L.lib().llamahip_op_gemv_set_q4_0(w, 64, 64, 0, 0, xs, 4, None, None, xp, 64, 0, 0, 0, 0, 0, None, None, None, None, None,
                                               None, None, 0, 0, None, None, None, err, len(err))
        assert rc != 0 and b"null operand (w, x)" in err.value


def on_host(L, oracle, c):
    """the op on a case's own operands: the plan it reports (set before the device is looked for) or the refusal's text"""
    ops, want = sc.build(oracle, c)
    w, x = ops.pop("w"), ops.pop("x")
    try:
        return L.op_gemv_set_q4_0(w, x=x, **ops)["plan"], want
    except L.LlamaHipError as e:
        assert NO_DEVICE in str(e), f"{sc.case_id(c)}: {e}"          # the LAST refusal: everything before it passed
        return None, want


def test_every_case_passes_the_host_checks_and_the_limits_are_accepted(L, oracle):
    """what stops a case on a machine without a GPU is the device check, nothing earlier; ids are unique; every matrix holds a zero scale
    and the extreme codes; every activation holds its four kinds of row"""
    ids = [sc.case_id(c) for c in sc.CASES]
    assert len(set(ids)) == len(ids) and {c.group for c in sc.CASES} == set(sc.GROUPS)
    for c in sc.CASES:
        on_host(L, oracle, c)
        assert c.M * c.K <= (1 << 20) * 4 and (c.M < 6144 or c.K <= 1344), sc.case_id(c)          # the oracle's cost stays far below a second
    for M, K, wkind in sorted({(c.M, c.K, c.wkind) for c in sc.CASES}):
        if M * K >= 4096:          # (a matrix of a few blocks cannot hold everything; the generator is the same)
            assert all(gc.weight_properties(gc.weights(M, K, wkind))), (M, K, wkind)
    for c in sc.CASES[::7] + [sc.BASE]:
        assert all(sc.activation_properties(sc.activation(c))), sc.case_id(c)
    for kw in (dict(N=2), dict(N=60), dict(epi="silu_qah", N=16, layer=249), dict(M=1), dict(epi="rope_kv", M=192, n_ctx=8, n_past=4),
               dict(force=(2, 2, 4)), dict(force=(1, 4, 2)), dict(y_stride=64)):
        with pytest.raises(L.LlamaHipError, match=NO_DEVICE):
            call(L, **kw)


def forced_plans(L):
    """(case, (nc, cw, ncg, rgw, lds)) of every case, from the host-only query or the force"""
    for c in sc.CASES:
        if c.force:
            yield c, sc.expected_forced_plan(c)[:4]
        else:
            p = L.set_plan(c.M, c.K, c.N, sc.EPI[c.epi], c.epi.startswith("silu"))
            assert p is not None, sc.case_id(c)
            yield c, p[:4]


def test_steps_coverage_table():
    """for each cw every steps % 4 occurs, steps 1, 2 and 3 (fewer than the ring's prefill) occur, and so does a padded last chunk -- under
    both epilogues of the group"""
    for cw in (1, 2, 3, 4):
        for epi in ("store", "resid"):
            ks = [c.K for c in sc.CASES if c.group == "steps" and c.force[1] == cw and c.epi == epi]
            steps = [-(-(-(-K // 256)) // cw) for K in ks]
            assert {s % sc.SET_DR for s in steps} == {0, 1, 2, 3}, (cw, epi, steps)
            assert {1, 2, 3} <= set(steps) and max(steps) > sc.SET_DR, (cw, epi, steps)
            assert any(K % 256 for K in ks), (cw, ks)
    for c in sc.CASES:
        if c.group == "steps":
            assert c.M == 24 and c.N == c.force[0] * c.force[1]


def test_every_pair_is_launched_and_the_auto_cases_reach_the_ten_the_rule_can_produce(L):
    auto = {p[:2] for c, p in forced_plans(L) if c.group == "auto"}
    assert auto == sc.AUTO_PAIRS, sorted(auto ^ sc.AUTO_PAIRS)
    assert set(sc.PAIRS) - sc.AUTO_PAIRS == sc.FORCED_ONLY
    every_auto = {p[:2] for c, p in forced_plans(L) if not c.force}
    assert not (every_auto & sc.FORCED_ONLY), "a pair the rule never picked before is now picked: move it to AUTO_PAIRS and test it there"
    inst = {(c.epi, c.force) for c in sc.CASES if c.group == "inst"}
    for pair in sc.PAIRS:
        for epi in ("store", "resid", "rope_kv") + (("silu_qa", "silu_qah") if pair[1] == 1 else ()):
            assert (epi, pair) in inst, (epi, pair)
        ns = sorted({c.N for c in sc.CASES if c.group == "inst" and c.force == pair})
        g = pair[0] * pair[1]
        assert g in ns and 2 * g - 1 in ns and (g - 1 in ns or g == 2) and any(-(-n // g) >= 3 for n in ns), (pair, ns)
    # the class edges and the LDS fallback are where the issue puts them
    for c, p in forced_plans(L):
        if c.group == "auto" and c.K >= 13824:
            assert p[1] == 1 and L.set_plan(c.M, c.K, c.N, sc.EPI[c.epi])[4] <= sc.LDS_CAP, (sc.case_id(c), p)
    nine = [p for c, p in forced_plans(L) if c.group == "auto" and c.epi == "rope_kv"]
    assert nine and all(p[:3] == (5, 1, 2) for p in nine), nine
    # invalid workgroups: the inst shapes' row-groups are no multiple of rgw, and column groups pad the grid to eight per group
    for c in sc.CASES:
        if c.group == "inst" and c.epi in ("store", "resid"):
            nc, cw, ncg, rgw, grid, _ = sc.expected_forced_plan(c)
            assert ((c.M + 7) // 8) % rgw != 0 or c.M == 75 and rgw == 2
            assert ncg == 1 or grid == 8 * ncg > -(-((c.M + 7) // 8) // rgw) * ncg


def test_rope_inputs_make_a_misplaced_row_show(oracle):
    """every pair of columns differs in acc (q, k and v parts alike), and every pair of positions of a case differs in its rotation of the
    same (non-zero) row: a row written with another row's position or offset cannot reproduce the reference.  (The all-zero row rotates to
    zeros anywhere; it is caught by WHERE it lands: the caches are compared whole.)  Tables: distinct positions out of order, slot 1 never
    touched, rows 0 and 1 a drafted segment."""
    seen_tables = 0
    for c in sc.CASES + [sc.BASE_ROPE]:
        if c.epi != "rope_kv":
            continue
        ops, want = sc.build(oracle, c)
        d, dh, n_ctx, n_past, table = c.rope
        acc, pos, slot = want["acc"], want["pos"], want["slot"]
        for part in range(3):
            rows = {acc[n, part * d:(part + 1) * d].tobytes() for n in range(c.N)}
            assert len(rows) == c.N, (sc.case_id(c), part)
        assert len({(int(s), int(p)) for s, p in zip(slot, pos)}) == c.N and pos.min() >= 0 and pos.max() < n_ctx
        for n in range(c.N):
            k = acc[n, d:2 * d]
            if not k.any():
                assert c.N >= 3 and n == c.N - 1
                continue
            rot = oracle.rope(np.repeat(k[None, :], n_ctx, axis=0).reshape(n_ctx, d // dh, dh), 0, 0).reshape(n_ctx, d)      # row p: k at position p
            assert len({rot[p].tobytes() for p in pos}) == len(set(pos.tolist())), (sc.case_id(c), n)
            assert rot[pos[n]].tobytes() == want["Kc"][slot[n], pos[n]].tobytes()
        if table:
            seen_tables += 1
            assert len(set(pos.tolist())) == c.N and np.any(np.diff(pos) < 0) and 1 not in slot and ops["n_slots"] == 3, sc.case_id(c)
            if c.N >= 3:
                assert slot[0] == slot[1] and pos[1] == pos[0] + 1 and {0, 2} == set(slot.tolist())
            assert np.all(want["Kc"][1].view(np.uint32) == sc.CANARY) and np.all(want["Vc"][1].view(np.uint32) == sc.CANARY)
        else:
            assert n_past in (0, 3, 5, n_ctx - c.N) and np.array_equal(pos, np.arange(n_past, n_past + c.N))
    assert seen_tables >= 12


def test_silu_inputs_make_a_lost_exchange_show(oracle):
    """SILU_QAH: for each half there is a (column, block) where that half alone holds the strict block maximum -- never excused; the
    zero-gate and zero-up blocks of "silu_zero" give amax 0, d 0 and codes 0; the gates stay inside fp16; both epilogues get one x and one
    reference; the padded blocks of the expected rows are zero and the rows from N on keep the fill"""
    by_shape = {}
    for c in sc.CASES + [sc.BASE_SILU]:
        if not c.epi.startswith("silu"):
            continue
        ops, want = sc.build(oracle, c)
        F, Fp = c.M // 2, (c.M // 2 + 255) // 256 * 256
        if c.N <= sc.SET_MAX:
            assert sc.qah_condition(want["act"]), sc.case_id(c)
        assert np.isfinite(want["act"]).all() and np.abs(want["gate"]).max() < 6e4, sc.case_id(c)
        d = want["out_d"][:c.N].view(np.float32)
        assert not d[:, F // 32:].any() and np.all(want["out_d"][c.N:] == sc.FILL) and np.all(want["out_A"][c.N:] == sc.FILL)
        assert np.all(d[0, :F // 32] >= 0) and d[:c.N - 1].any()
        if c.wkind == "silu_zero":
            assert not d[:, :2].any() and np.all(d[:2, 2:F // 32] > 0), sc.case_id(c)
            assert not want["out_A"][:c.N].reshape(c.N, Fp // 256, 8, 8)[:, 0, :, :2].any()
        if c.x_prev:
            assert np.array_equal(ops["x_prev"], ops["x"] * np.float32(4.0)) and c.layer in (0, sc.TAG_MAX_LAYERS - 1)
        key = (c.M, c.K, c.N, c.wkind)
        blob = ops["x"].tobytes() + want["out_A"].tobytes() + want["out_d"].tobytes()
        assert by_shape.setdefault(key, blob) == blob, sc.case_id(c)
    both = {(c.M, c.K, c.N) for c in sc.CASES if c.epi == "silu_qah"} & {(c.M, c.K, c.N) for c in sc.CASES if c.epi == "silu_qa"}
    assert len(both) >= 30


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_yardstick_can_see_what_it_must(oracle):
    """conditions on the base cases' inputs, not on any kernel: each fault the kernel's structure invites differs from the reference in bits"""
    c = sc.BASE
    ops, want = sc.build(oracle, c)
    w, x, y = ops["w"], ops["x"], want["y"]
    live = [n for n in range(c.N - 1)]
    # a duplicated column (the clamped duplicates past ncols, written where a real column belongs)
    for n in live[1:]:
        assert np.count_nonzero(words(y[n]) != words(y[n - 1])) > c.M // 2, n
    # a column evaluated with its neighbour's operand row (the neighbour's codes under this column's scales): in float64 it lands further
    # from the reference than twice the bound every exact kernel is held to, so no arithmetic inside the bound can give the right bits
    ref = Ref(oracle, w, x, None)
    Wq = (ref.dw[:, :, None] * ref.cw).reshape(c.M, c.K)
    bound = ref.bound_exact()
    for n in live[1:]:
        mixed = (ref.da[n][:, None] * ref.ca[n - 1]).reshape(c.K) @ Wq.T
        assert np.count_nonzero(np.abs(mixed - ref.ystar[n]) > 2 * bound[n]) > c.M // 2, n
    assert np.all(ref.err(y) <= bound)
    # a dropped last chunk (1344 = five chunks and a padded sixth of two blocks)
    short = oracle.mul_mat_q4_0(np.ascontiguousarray(w[:, :40]), x[:, :1280], 1)
    assert np.count_nonzero(words(short[live]) != words(y[live])) > len(live) * c.M // 2
    # a block quantized with its own half's amax only (a lost or one-sided exchange), and with four times the amax (a stale granule)
    cs = sc.BASE_SILU
    ops, want = sc.build(oracle, cs)
    F = cs.M // 2
    lo, hi = sc.half_amax(want["act"])
    d = want["out_d"][:cs.N, :F // 32].view(np.float32)
    full = np.maximum(lo, hi)
    assert np.array_equal(words(d), words(full / np.float32(7.0)))
    assert np.count_nonzero(words(lo / np.float32(7.0)) != words(d)) >= 1 and np.count_nonzero(words(hi / np.float32(7.0)) != words(d)) >= 1
    assert np.count_nonzero(words(np.float32(4.0) * full / np.float32(7.0)) != words(d)) == np.count_nonzero(full)
    # a K row rotated at position + 1
    cr = sc.BASE_ROPE
    ops, want = sc.build(oracle, cr)
    d_, dh = cr.rope[0], cr.rope[1]
    for n in range(cr.N - 1):
        k = want["acc"][n, d_:2 * d_]
        off = oracle.rope(k.reshape(1, d_ // dh, dh), int(want["pos"][n]) + 1, 0).reshape(d_)
        assert np.count_nonzero(words(off) != words(want["Kc"][want["slot"][n], want["pos"][n]])) > d_ // 2, n


def test_set_plan_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: set_plan.cpp (the plan and launch shape of every LLaMA matrix at 2 .. 60 rows, every forced pair admitted or refused on
    exactly sized message buffers, what the rule refuses) compiled with -fsanitize=address,undefined into the stand-alone
    tools/host_sanitize and run there -- never loaded into python"""
    import os
    import subprocess
    import synth
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "asan"], check=True)
    src = open(os.path.join(csrc, "tools", "host_sanitize.cpp")).read()
    assert "set_force_check(" in src and "set_launch_query(" in src and "set_applies(" in src
    assert "set_plan.cpp" in open(os.path.join(csrc, "Makefile")).read().split("asan:")[1].split("tools:")[0]
    assert "hip_runtime" not in open(os.path.join(csrc, "set_plan.cpp")).read() + open(os.path.join(csrc, "set_plan.h")).read()
    path = str(tmp_path / "m.bin")
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(csrc, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "few-row mat-mul host half: 2655 plans" in r.stdout and "clean" in r.stdout, r.stdout + r.stderr
    assert "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
