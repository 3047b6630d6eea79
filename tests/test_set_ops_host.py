"""CPU: the op-level entry points of the batched decode step -- llamahip_op_set_attention, llamahip_op_set_entry, llamahip_op_set_exit -- are
exported and refuse, before they look for a device, every call they must not launch, each naming its limit; llamahip_debug_set_keys is the
one key-bucket rule, checked at its edges; the coverage tables of tests/set_attn_cases.py (every head size, position edge, set_keys form,
table kind, value regime, score fill and entry / exit mode the GPU tests are there for occurs in some case); and the conditions on the
inputs: each attention case's expected merged rows differ in at least one word from each of four wrong models (set_attn_cases.wrong_models),
so a kernel that did one of those things instead could not pass."""
import ctypes as C

import numpy as np
import pytest

import attn_cases
import set_attn_cases as sa

NO_DEVICE = "no HIP device available"
SYMS = ("llamahip_op_set_attention", "llamahip_op_set_entry", "llamahip_op_set_exit", "llamahip_debug_set_keys")


def test_new_symbols_are_declared_and_exported(L):
    for s in SYMS:
        assert s in L.declared_symbols() and hasattr(L.lib(), s), s
    assert L.SET_ENTRY_MODES == sa.ENTRY_MODES and L.SET_EXIT_MODES == sa.EXIT_MODES


# ------------------------------------------------------------------------------------------------ the key bucket
@pytest.mark.parametrize("n_ctx", [160, 288, 128, 512, 2048])
def test_key_bucket_rule(L, n_ctx):
    for max_pos in sorted({0, 127, 128, n_ctx - 1, 1, 126, 129, 255, 256} & set(range(n_ctx))):
        k = L.debug_set_keys(n_ctx, max_pos)
        assert max_pos < k <= n_ctx, (n_ctx, max_pos, k)
        assert k == min(n_ctx, (max_pos // 128 + 1) * 128) == sa.rule_keys(n_ctx, max_pos), (n_ctx, max_pos, k)
    assert L.debug_set_keys(n_ctx, 127) == min(128, n_ctx) and L.debug_set_keys(n_ctx, n_ctx - 1) == n_ctx
    for bad in ((n_ctx, n_ctx), (n_ctx, -1), (0, 0), (-5, 0)):
        assert L.debug_set_keys(*bad) is None, bad


# ------------------------------------------------------------------------------------------------ refusals
def attn_call(L, d=64, H=2, n_ctx=16, n_slots=3, row_slot=(0, 1), row_pos=(3, 4), **kw):
    B = len(row_slot)
    qkv = np.zeros((B, 3 * d), np.float32)
    Kc, Vc = np.zeros((n_slots, n_ctx, d), np.float32), np.zeros((n_slots, n_ctx, d), np.float32)
    return L.op_set_attention(qkv, H, Kc, Vc, row_slot, row_pos, **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(d=96, H=2), "head size 48: multiples of 32 up to 256"), (dict(d=288, H=1), "head size 288: multiples of 32 up to 256"),
    (dict(n_threads=33), "n_threads 33 outside 1 .. 32"), (dict(n_threads=0), "n_threads 0 outside 1 .. 32"),
    (dict(row_slot=(0,), row_pos=(1,)), "B 1 outside 2 .. 16 rows"), (dict(row_slot=[0] * 17, row_pos=list(range(17)), n_ctx=32), "B 17 outside 2 .. 16 rows"),
    (dict(set_keys=-1), "set_keys -1 outside 0 .. n_ctx = 16"), (dict(set_keys=17), "set_keys 17 outside 0 .. n_ctx = 16"),
    (dict(set_keys=4), "row_pos.1. = 4 is not below set_keys 4"), (dict(set_keys=3), "row_pos.0. = 3 is not below set_keys 3"),
    (dict(row_pos=(3, 16)), "row_pos.1. = 16 out of range .0, n_ctx = 16."), (dict(row_pos=(-1, 4)), "row_pos.0. = -1 out of range"),
    (dict(row_slot=(0, 3)), "row_slot.1. = 3 out of range .0, 3."), (dict(row_slot=(-1, 0)), "row_slot.0. = -1 out of range"),
    (dict(row_slot=(1, 1), row_pos=(5, 5)), "rows 0 and 1 are both at position 5 of slot 1"),
    (dict(row_slot=(2, 0, 2), row_pos=(7, 1, 7)), "rows 0 and 2 are both at position 7 of slot 2"),
    (dict(row_slot=(1, 1), row_pos=(5, 4)), "rows of slot 1 are not one run of consecutive ascending positions in adjacent rows"),
    (dict(row_slot=(1, 1), row_pos=(4, 6)), "rows of slot 1 are not one run"),
    (dict(row_slot=(1, 0, 1), row_pos=(4, 9, 5)), "rows of slot 1 are not one run"),
    (dict(merged_stride=63), "merged_stride 63 < d 64"),
])
def test_set_attention_refusals_need_no_device(L, kw, msg):
    with pytest.raises(L.LlamaHipError, match=msg) as e:
        attn_call(L, **kw)
    assert NO_DEVICE not in str(e.value)


def test_set_attention_null_operands_are_refused(L):
    err = C.create_string_buffer(512)
    z = np.zeros(8, np.int32).ctypes.data_as(C.c_void_p)
    rc = L.lib().llamahip_op_set_attention(None, 2, 64, 2, 16, 1, None, None, z, z, 8, 0, None, 0, None, 0, err, len(err))
    assert rc != 0 and b"bad arguments" in err.value


def entry_call(L, mode="embed_q4_0", d=32, B=2, **kw):
    emb = {"embed_q4_0": np.zeros((8, d // 32, 20), np.uint8), "embed_f16": np.zeros((8, d), np.float16), "embed_f32": np.zeros((8, d), np.float32)}.get(mode)
    kw.setdefault("row_pos", np.zeros(B, np.int32))
    if mode == "rows":
        kw.setdefault("hid_in", np.zeros((B, d), np.float32))
    else:
        kw.setdefault("emb", emb)
        kw.setdefault("tokens", np.zeros(B, np.int32))
    return L.op_set_entry(mode, **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(mode=4), "unknown mode 4"), (dict(mode=-1), "unknown mode -1"),
    (dict(B=1), "B 1 outside 2 .. 16 rows"), (dict(B=17), "B 17 outside 2 .. 16 rows"), (dict(mode="rows", B=17), "B 17 outside 2 .. 16 rows"),
    (dict(mode="embed_f32", d=48), "d 48 must be a positive multiple of 32"),
    (dict(x_stride=31), "x_stride 31 < d 32"),
    (dict(emb=None), "the embed modes need emb, tokens"), (dict(tokens=None), "the embed modes need emb, tokens"),
    (dict(mode="rows", hid_in=None), "d 0 must be a positive multiple of 32"),
    (dict(mode="embed_f16", pass_epoch=True), "k_embed_dense_set takes no epoch word"), (dict(mode="embed_f32", pass_epoch=True), "takes no epoch word"),
    (dict(tokens=[0, 8]), "token 8 of row 1 outside .0, 8."), (dict(mode="embed_f16", tokens=[-1, 0]), "token -1 of row 0 outside"),
    (dict(row_pos=[0, -1]), "row_pos.1. = -1 is negative"),
])
def test_set_entry_refusals_need_no_device(L, kw, msg):
    with pytest.raises(L.LlamaHipError, match=msg) as e:
        entry_call(L, **kw)
    assert NO_DEVICE not in str(e.value)


def test_set_entry_rows_without_rows_is_refused(L):
    err = C.create_string_buffer(512)
    z = np.zeros(64, np.int32).ctypes.data_as(C.c_void_p)
    rc = L.lib().llamahip_op_set_entry(3, None, 0, 32, None, None, 2, z, 0, 0, z, 32, z, z, z, z, err, len(err))
    assert rc != 0 and b"mode ROWS needs hid_in" in err.value
    rc = L.lib().llamahip_op_set_entry(3, None, 0, 32, None, z, 2, z, 0, 0, z, 32, None, z, z, z, err, len(err))
    assert rc != 0 and b"null operand" in err.value


def exit_call(L, mode="argmax", B=2, n_ctx=8, V=4, d=32, **kw):
    kw.setdefault("row_pos", np.zeros(B, np.int32))
    kw.setdefault("row_step", np.zeros(B, np.int32))
    if mode == "rows_out":
        kw.setdefault("x", np.zeros((B, d), np.float32))
    else:
        kw.setdefault("logits", np.zeros((B, V), np.float32))
    return L.op_set_exit(mode, n_ctx=n_ctx, **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(mode=3), "unknown mode 3"), (dict(mode=-1), "unknown mode -1"),
    (dict(mode="argmax_one", B=2), "mode ARGMAX_ONE takes B = 1 row .k_argmax., got 2"),
    (dict(B=1), "B 1 outside 2 .. 16 rows"), (dict(B=17, n_ctx=32), "B 17 outside 2 .. 16 rows"), (dict(mode="rows_out", B=1), "B 1 outside 2 .. 16 rows"),
    (dict(logits=None), "the argmax modes need logits and V 0 >= 1"), (dict(mode="argmax_one", B=1, logits=None), "the argmax modes need logits"),
    (dict(mode="rows_out", x=None), "mode ROWS_OUT needs x, hid_out"),
    (dict(n_ctx=0), "n_ctx 0 must be >= 1"),
    (dict(row_pos=[0, 8]), "row_pos.1. = 8 out of range .0, n_ctx = 8."), (dict(row_pos=[-1, 0]), "row_pos.0. = -1 out of range"),
    (dict(row_step=[8, 0]), "row_step.0. = 8 out of range .0, n_ctx = 8. .the trace row."), (dict(mode="rows_out", row_step=[0, -1]), "row_step.1. = -1 out of range"),
])
def test_set_exit_refusals_need_no_device(L, kw, msg):
    with pytest.raises(L.LlamaHipError, match=msg) as e:
        exit_call(L, **kw)
    assert NO_DEVICE not in str(e.value)


def test_binding_checks_its_own_shapes(L):
    with pytest.raises(ValueError):
        attn_call(L, row_slot=(0, 1), row_pos=(1, 2, 3))
    with pytest.raises(ValueError):
        entry_call(L, tokens=[0, 1, 2])
    with pytest.raises(ValueError):
        exit_call(L, row_step=[0])


def on_host(fn):
    """a call that passes every host check: the LAST refusal is the missing device (on a machine with a GPU it runs)"""
    import llama_swift_amd as L
    try:
        fn()
    except L.LlamaHipError as e:
        assert NO_DEVICE in str(e), e


# ------------------------------------------------------------------------------------------------ the cases
@pytest.fixture(scope="module")
def built_cases(oracle):
    """name -> (case, operands, expected merged, {wrong model: merged}); computed once"""
    out = {}
    for c in sa.CASES:
        ops = sa.build(c)
        right, wrong = sa.wrong_models(oracle, c, ops)
        out[c["name"]] = (c, ops, right, wrong)
    return out


def test_every_case_passes_the_host_checks(L, built_cases):
    for c, ops, _, _ in built_cases.values():
        for merged in (True, False):
            on_host(lambda: L.op_set_attention(ops["qkv"], c["H"], ops["Kc"].copy(), ops["Vc"].copy(), ops["row_slot"], ops["row_pos"], c["nth"],
                                               sa.set_keys_of(c), merged_stride=c["d"] + 8, want_merged=merged, score_fill=c["fill"]))
    emb = np.zeros((sa.V_EMB, 1, 20), np.uint8)
    for mode, d, B, e, p in sa.ENTRY_CASES:
        tokens, pos = sa.entry_rows(B)
        assert 0 <= tokens.min() and tokens.max() < sa.V_EMB
        if mode == "embed_q4_0" and d == 32:
            on_host(lambda: L.op_set_entry(mode, pos, emb=emb, tokens=tokens, epoch_in=e, pass_epoch=p))
    for mode in sa.EXIT_MODES:
        B = 1 if mode == "argmax_one" else 16
        pos, step, null = sa.exit_rows(B)
        on_host(lambda: L.op_set_exit(mode, pos, step, sa.EXIT_N_CTX, logits=np.zeros((B, 65), np.float32) if mode != "rows_out" else None,
                                      x=np.zeros((B, 32), np.float32) if mode == "rows_out" else None, tok_out_null=null))


def test_coverage_tables():
    cs = sa.CASES
    assert len({c["name"] for c in cs}) == len(cs)
    assert {c["d"] // c["H"] for c in cs} == {64, 96, 256, 128, 32} and {(c["d"], c["H"]) for c in cs} == set(sa.SHAPES)
    assert {c["d"] for c in cs if c["d"] % 256 != 0} == {128, 192, 320} and any(c["d"] % 256 == 0 for c in cs)          # with and without QA pad blocks
    assert {c["n_ctx"] for c in cs} == {160, 288}
    assert {len(sa.rows_of(c)[0]) for c in cs} == {2, 3, 16}
    assert {c["nth"] for c in cs} == {1, 3, 8, 32}
    # positions: 0 under 8 and 32 threads (empty chains), the slice edge, the bucket edge, n_ctx - 1, and 0 with n_ctx - 1 in one set
    pos = {c["name"]: set(sa.rows_of(c)[1].tolist()) for c in cs}
    for nth in (8, 32):
        assert any(c["nth"] == nth and 0 in pos[c["name"]] for c in cs), nth
    for p in (31, 32, 127, 128):
        assert any(p in v for v in pos.values()), p
    assert any(c["n_ctx"] - 1 in pos[c["name"]] for c in cs if c["n_ctx"] == 160) and any(c["n_ctx"] - 1 in pos[c["name"]] for c in cs if c["n_ctx"] == 288)
    assert any({0, c["n_ctx"] - 1} <= pos[c["name"]] for c in cs)
    # set_keys: 0, the rule's value, the exact bucket (highest row at 127 -> 128 keys)
    assert {c["keys"] for c in cs} == {"zero", "rule", "exact"}
    for c in cs:
        k, mx = sa.set_keys_of(c), int(sa.rows_of(c)[1].max())
        assert k == 0 or mx < k <= c["n_ctx"], c["name"]
        assert c["keys"] != "exact" or (mx == 127 and k == 128)
    assert any(c["keys"] == "rule" and sa.set_keys_of(c) < c["n_ctx"] for c in cs) and any(c["keys"] == "rule" and sa.set_keys_of(c) == c["n_ctx"] for c in cs)
    # tables
    assert {c["table"] for c in cs} == {"distinct", "segments", "one_slot"}
    for c in cs:
        slot, p = sa.rows_of(c)
        if c["table"] == "distinct":
            assert len(set(slot.tolist())) == len(slot) and any(slot[i] > slot[i + 1] for i in range(len(slot) - 1)), c["name"]
        elif c["table"] == "segments":
            runs = [(s, q, n) for s, q, n, _ in c["segs"] if n > 1]
            assert sorted((q, n) for _, q, n in runs) == [(30, 3), (125, 4)] and any(n == 1 for _, _, n, _ in c["segs"]), c["name"]
            assert all(any(q < e <= q + n - 1 for e in (32, 128)) for _, q, n in runs)          # both cross an edge (the slice's, the bucket's)
        else:
            assert len(slot) == 16 and len(set(slot.tolist())) == 1 and slot[0] != 0, c["name"]
        assert len({(int(a), int(b)) for a, b in zip(slot, p)}) == len(slot)
    assert any(0 in sa.rows_of(c)[0] for c in cs) and all((sa.rows_of(c)[0] != 0).any() for c in cs)
    # regimes: each in a single (N = 1) and the segment regimes in a run
    singles = {r for c in cs for _, _, n, r in c["segs"] if n == 1}
    runs = {r for c in cs for _, _, n, r in c["segs"] if n > 1}
    assert singles == set(attn_cases.REGIMES) and runs == set(attn_cases.REGIMES), (singles, runs)
    # score fills: NaN words and +1e30
    assert {c["fill"] for c in cs} == {sa.FILL_NAN, sa.FILL_1E30} and np.array([sa.FILL_1E30], np.uint32).view(np.float32)[0] == np.float32(1e30)
    # entry / exit
    assert {m for m, *_ in sa.ENTRY_CASES} == set(sa.ENTRY_MODES) and {d for _, d, *_ in sa.ENTRY_CASES} == {32, 320, 4096}
    assert {p for *_, p in sa.ENTRY_CASES} == {True, False} and all(not p or m in ("embed_q4_0", "rows") for m, _, _, _, p in sa.ENTRY_CASES)
    for B in (2, 3, 16):
        tokens, rp = sa.entry_rows(B)
        assert sa.V_EMB - 1 in tokens and len(set(tokens.tolist())) < B and (B == 2 or 0 in tokens)
    assert 0 in sa.entry_rows(16)[0]
    assert set(sa.EXIT_MODES) == {"argmax", "rows_out", "argmax_one"} and sa.EXIT_VOCABS == (1, 65, 1500, 32000)
    for B in (2, 16):
        _, step, null = sa.exit_rows(B)
        assert 0 in step and sa.EXIT_N_CTX - 1 in step and null.sum() == 1


def test_next_epoch_restated():
    assert sa.next_epoch(0) == 1 and sa.next_epoch(41) == 42
    assert sa.next_epoch(0x00FFFFFF) == 0x01000001 and sa.next_epoch(0xFFFFFFFF) == 1 and sa.next_epoch(0xFFFFFFFE) == 0xFFFFFFFF


@pytest.mark.parametrize("name", [c["name"] for c in sa.CASES])
def test_each_wrong_model_changes_the_expected_rows(built_cases, name):
    c, ops, right, wrong = built_cases[name]
    assert not np.isnan(right).any(), "the expected rows read nothing they should not"
    for k in "abc":
        assert wrong[k] is not None, (name, k)
    assert (wrong["d"] is not None) == (c["table"] != "distinct"), name
    for k, m in wrong.items():
        if m is not None:
            n = int((m.view(np.uint32) != right.view(np.uint32)).sum())
            assert n >= 1, f"{name}: wrong model {k} gives the expected merged rows: the case cannot tell them apart"


@pytest.mark.parametrize("name", [c["name"] for c in sa.CASES])
def test_expected_rows_stay_within_the_float64_bound(oracle, built_cases, name):
    """attn_ref.f64_reference's bound (as tests/test_gpu_attention.py asserts it) on the oracle's rows, one row at a time: the GPU test
    compares with these rows bit for bit"""
    from attn_ref import f64_reference
    c, ops, right, _ = built_cases[name]
    Kc, Vc = ops["Kc"].copy(), ops["Vc"].copy()
    for r in range(len(ops["row_pos"])):
        s, p = int(ops["row_slot"][r]), int(ops["row_pos"][r])
        m, Kc[s], Vc[s], qr = attn_cases.oracle_side(oracle, ops["qkv"][r:r + 1], Kc[s], Vc[s], c["H"], p, c["nth"])
        ref64, bound, _ = f64_reference(qr, Kc[s], Vc[s], c["H"], p, c["nth"])
        err = np.abs(m.astype(np.float64) - ref64)
        assert np.array_equal(m[0].view(np.uint32), right[r].view(np.uint32)) and np.all(err <= bound), (name, r, np.argwhere(err > bound)[:3])
