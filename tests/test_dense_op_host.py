"""CPU: the root of the f16 / f32 op tests.  The yardstick of tests/dense_cases.py -- 32 fmaf chains per output (orc_vec_dot_f32), the
activations rounded to fp16 once where the weights are fp16 -- agrees with what the reference build's own mat-mul computes
(ref_mul_mat_dense: a ggml graph with an F16 / F32 src0, run by the reference's ggml_graph_compute) for EVERY case the GPU tests run, at 1
and 8 threads; likewise the gather's expectation against the reference's ggml_get_rows (f32, f16, Q4_1).  The reference outputs are stored
in tests/golden/ref_outputs_dense_op.npz (tests/refgolden.py: re-checked wherever oracle/_ref is built).  Comparison rule: finite values bit
for bit, non-finite values by class.

Also here: the conditions on the INPUTS (the base case tells the reference's arithmetic from each neighbouring one in at least 8 outputs;
every row of the f16_double_rounding regime holds at least 64 elements whose two roundings differ from one; the value regimes contain
what their names say), perm_index against the operand order's definition, and the refusals of llamahip_op_dense_prep /
llamahip_op_embed_dense, which all happen before a device is looked for."""
import os

import numpy as np
import pytest

import dense_cases as dc
import prep_cases as pc
import refgolden

STORE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_outputs_dense_op.npz")
THREADS = (1, 8)


@refgolden.computed_by("dense_op.mul_mat", [(dc.mv_id(c), nth) for c in dc.MV_CASES for nth in THREADS], store=STORE)
def ref_mul_mat(ref, tmp_dir, cid, nth):
    w, x, _ = dc.mv_build(dc.MV_BY_ID[cid])
    with np.errstate(all="ignore"):
        return {"y": dc.stored(ref.mul_mat_dense(w, x, nth))}


@refgolden.computed_by("dense_op.get_rows", [(dc.embed_id(c),) for c in dc.EMBED_CASES], store=STORE)
def ref_get_rows(ref, tmp_dir, cid):
    wtype, d, N = next(c for c in dc.EMBED_CASES if dc.embed_id(c) == cid)
    return {"x": dc.stored(ref.get_rows(dc.embed_table(wtype, d), dc.EMBED_TOKENS[N], wtype=wtype))}


def live(ref):
    """the reference build where it has the two entry points (an oracle/_ref kept from an older tree has not: the store alone then)"""
    return ref if ref is not None and ref.has_dense_ops else None


# ------------------------------------------------------------------------------------------------ yardstick == reference
@pytest.mark.parametrize("cid", [dc.mv_id(c) for c in dc.MV_CASES])
def test_yardstick_equals_the_reference_mat_mul(oracle, ref, tmp_path, cid):
    case = dc.MV_BY_ID[cid]
    w, x, _ = dc.mv_build(case)
    y = dc.yardstick(oracle, w, x, None, case[0])
    assert y.shape == (case[3], case[2])
    for nth in THREADS:
        bad = dc.agrees_with_stored(y, refgolden.outputs("dense_op.mul_mat", live(ref), tmp_path, cid, nth)["y"])
        assert not bad, f"{cid}, {nth} threads: yardstick vs reference: {bad}"


@pytest.mark.parametrize("cid", [dc.embed_id(c) for c in dc.EMBED_CASES])
def test_gather_expectation_equals_the_reference_get_rows(ref, tmp_path, cid):
    wtype, d, N = next(c for c in dc.EMBED_CASES if dc.embed_id(c) == cid)
    rows = dc.embed_rows(wtype, dc.embed_table(wtype, d))[dc.EMBED_TOKENS[N]]
    bad = dc.agrees_with_stored(rows, refgolden.outputs("dense_op.get_rows", live(ref), tmp_path, cid)["x"])
    assert not bad, f"{cid}: expectation vs reference: {bad}"


def test_the_store_is_a_small_file():
    assert os.path.getsize(STORE) < (1 << 20)


# ------------------------------------------------------------------------------------------------ conditions on the inputs
@pytest.mark.parametrize("wtype", [1, 0], ids=["f16", "f32"])
def test_base_case_tells_the_reference_arithmetic_from_its_neighbours(oracle, wtype):
    """(a) the fold in lane order, (b) multiply and add rounded separately, (c) 16 / 64 chains, (d) f16: activations not rounded: each
    changes at least 8 of the base case's 120 outputs -- a kernel that computed any of them would fail tests/test_gpu_dense_mv_op.py.
    ((b) exists for f32 weights only: a product of two halves is exact in fp32, see below.)"""
    w, x, _ = dc.mv_build(dc.base_case(wtype))
    want = dc.yardstick(oracle, w, x, None, wtype)
    assert np.isfinite(want).all()
    mut = dc.mutations(oracle, w, x, wtype)
    assert np.array_equal(mut.pop("self").view(np.uint32), want.view(np.uint32)), "the variant with the reference's settings is not the yardstick"
    assert len(mut) == (5 if wtype == 1 else 4)
    for name, y in mut.items():
        n = int((y.view(np.uint32) != want.view(np.uint32)).sum())
        print(f"{dc.WNAMES[wtype]}: {name}: {n} of {want.size} outputs change")
        if wtype == 1 and name == "multiply and add rounded separately":
            # No seed can tell these apart: the product of two fp16 values has 11 + 11 = 22 significant bits and an exponent of at least
            # -48, so it is EXACT in fp32 and rounding it changes nothing -- for f16 weights (b) is the reference's arithmetic itself.
            assert n == 0
            continue
        assert n >= 8, f"{name} changes only {n} outputs of the base case: choose another seed"


def test_value_regimes_hold_what_their_names_say(oracle):
    # zeros: the cancellations are exact in the reference chain
    for wtype in (1, 0):
        w, x, _ = dc.mv_build((wtype, 1344, 40, 11, "zeros"))
        y = dc.yardstick(oracle, w, x, None, wtype)
        assert y[3, 2] == 0.0 and y[4, 3] == 0.0 and not np.signbit(y[3, 2]) and np.isfinite(y).all()
        assert not y[0].any() and not y[:, :2].any() and not np.signbit(y[:, :2]).any()    # (an accumulator that starts at +0 never turns -0)
    # midpoints: every activation is an exact tie and RNE goes to the even neighbour, from both parities
    rng = np.random.default_rng(1)
    xm, even = dc.fp16_midpoints(rng, 4096)
    assert np.array_equal(xm.astype(np.float16).view(np.uint16), even)
    assert (np.abs(xm) != np.abs(xm).astype(np.float16)).all()                              # no midpoint is itself a half
    w, x, _ = dc.mv_build((1, 1344, 40, 2, "midpoints"))
    up = np.abs(dc.act(x, 1)) > np.abs(x)
    assert up.any() and (~up).any()
    # overflow: 65519 stays finite, +-65520 become +-inf, and against the zero weights NaN appears
    w, x, _ = dc.mv_build((1, 1344, 40, 4, "overflow"))
    a = dc.act(x, 1)
    assert a[0, 5] == 65504.0 and a[0, 70] == -65504.0 and a[1, 7] == np.inf and a[2, 9] == -np.inf
    y = dc.yardstick(oracle, w, x, None, 1)
    assert np.isfinite(y[0]).all()
    assert np.isnan(y[1:]).any() and (y[1:] == np.inf).any() and (y[1:] == -np.inf).any()
    # tiny: the tie 2^-25 goes to zero, the next float to the smallest subnormal
    t = np.float32(2.0) ** -25
    assert dc.act(np.array([t, np.nextafter(t, np.float32(1)), 3 * t], np.float32), 1).tolist() == [0.0, 2.0 ** -24, 2.0 ** -23]
    w, x, _ = dc.mv_build((1, 1344, 40, 2, "tiny"))
    a = dc.act(x, 1)
    assert (a == 0).any() and (np.abs(a) == 2.0 ** -24).any() and (a != x).any()
    # underflow: subnormal sums, and sums of products that each underflow
    w, x, _ = dc.mv_build((0, 1344, 40, 2, "underflow"))
    y = dc.yardstick(oracle, w, x, None, 0)
    tiny = np.finfo(np.float32).tiny
    assert ((np.abs(y[0]) < tiny) & (y[0] != 0)).sum() >= 20
    with np.errstate(under="ignore"):
        assert ((w[0] * x[1]) == 0).any() and np.isfinite(y).all()


def test_double_rounding_rows_hold_at_least_64_such_elements(oracle):
    """f16_double_rounding: per row >= 64 elements whose exact product rounded once to fp16 differs from the reference's two roundings
    (fp32, then fp16) -- the elements a kernel that lost its fence in k_dense_prep gets wrong; NORM rows stay order-proof"""
    for mode, K, N, _, _ in dc.DR_CASES:
        x, b, mask = dc.dr_build(oracle, mode, K, N)
        first = oracle.unary_rows("silu" if mode == "silu_mul" else "norm", x)
        second = b if mode == "silu_mul" else np.broadcast_to(b, x.shape)
        hit = dc.rounds_twice(first, second) & mask
        print(f"{mode} K {K}: {hit.sum(axis=1).tolist()} elements per row")
        assert (hit.sum(axis=1) >= dc.DR_MIN_PER_ROW).all(), (mode, K, hit.sum(axis=1))
        y, _ = pc.reference(oracle, mode, x, b)
        with np.errstate(all="ignore"):
            once = (first.astype(np.float64) * second.astype(np.float64)).astype(np.float16).astype(np.float32)
        assert (dc.act(y, 1)[hit] != once[hit]).all() and np.isfinite(y).all()
        if mode == "norm":
            assert all(pc.norm_stats(r)["proof"] for r in x)


@pytest.mark.parametrize("K", [32, 224, 256, 288, 1344, 4128])
def test_perm_index_is_the_chain_major_order(K):
    """against the definition, element by element: inside a group of st steps chain l's steps s = 0 .. st - 1 are contiguous at l * st"""
    p = dc.perm_index(np.arange(K), K)
    assert sorted(p.tolist()) == list(range(K))
    for e in range(K):
        g, s, l = e // 256, (e % 256) // 32, e % 32
        st = 8 if (g + 1) * 256 <= K else (K % 256) // 32
        assert p[e] == g * 256 + l * st + s
    rows = np.arange(2 * K, dtype=np.float32).reshape(2, K)
    assert np.array_equal(dc.permute_rows(rows)[1, p], rows[1])


def test_gather_tables_hold_the_edges():
    q = dc.embed_table(3, 96)
    nb = 3
    codes = np.concatenate([q[:, 8 * nb:] & 0xF, q[:, 8 * nb:] >> 4], axis=1)
    mn, dd = q[:, :4 * nb].copy().view(np.float32), q[:, 4 * nb:8 * nb].copy().view(np.float32)
    assert set(np.unique(codes)) == set(range(16)) and (dd == 0).any() and (dd > 0).any() and (dd < 0).any() and (mn > 0).any() and (mn < 0).any()
    assert np.isfinite(dc.dequant_q41(q)).all()
    for d in dc.EMBED_DS:          # every Q4_1 case can tell two roundings from a fused multiply-add, the extreme rows alone included
        t = dc.embed_table(3, d)
        two, one = dc.dequant_q41(t), dc.dequant_q41_fused(t)
        for N in dc.EMBED_NS:
            n = int((two[dc.EMBED_TOKENS[N]] != one[dc.EMBED_TOKENS[N]]).sum())
            assert n >= 4, f"Q4_1 gather d {d} N {N}: only {n} elements tell a fused multiply-add from the reference's two roundings"
    h = dc.embed_table(1, 4096)[dc.EMBED_SPECIAL_ROW].view(np.uint16)
    assert set(range(1, 0x400)) <= set(h.tolist()) and set(range(0x8001, 0x8400)) <= set(h.tolist()) and {0, 0x8000, 0x7C00, 0xFC00, 0x7E00} <= set(h.tolist())
    for N in dc.EMBED_NS:
        t = dc.EMBED_TOKENS[N]
        assert len(t) == N and dc.EMBED_V - 1 in t and (N == 1 or 0 in t) and (N < 13 or (len(set(t)) < N and dc.EMBED_SPECIAL_ROW in t))


# ------------------------------------------------------------------------------------------------ the new ops' refusals
def test_new_symbols_are_exported(L):
    for s in ("llamahip_op_dense_prep", "llamahip_op_embed_dense"):
        assert s in L.declared_symbols() and hasattr(L.lib(), s), s


def dprep(L, mode="plain", wtype=1, K=64, N=2, n=None, **kw):
    return L.op_dense_prep(mode, wtype, np.zeros(4 * 64 * 8 if n is None else n, np.float32), K, N, **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(mode=0), "unknown mode 0"), (dict(mode=4), "unknown mode 4"), (dict(wtype=2), "wtype 2"), (dict(wtype=3), "wtype 3"), (dict(wtype=-1), "wtype -1"),
    (dict(kernel=3), "unknown kernel 3"), (dict(kernel=-1), "unknown kernel -1"),
    (dict(K=0), "K 0 must be a multiple of 32"), (dict(K=48), "K 48 must be a multiple of 32"), (dict(K=32800), "K 32800 must be"),
    (dict(N=0), "N 0 >= 1"),
    (dict(in_stride=32), "row stride 32 / 0 < K 64"), (dict(mode="silu_mul", in1_offset=128, in1_stride=60), "row stride 64 / 60 < K 64"),
    (dict(in_stride=66), "multiples of 4 floats"), (dict(in0_offset=2), "multiples of 4 floats"), (dict(mode="norm", in1_offset=130), "multiples of 4 floats"),
    (dict(mode="silu_mul", in1_offset=128, in1_stride=70), "multiples of 4 floats"),
    (dict(n=100), "end at float 128 / 0 of a buffer of 100"), (dict(mode="norm", in1_offset=2000), "end at float 128 / 2064 of a buffer of 2048"),
    (dict(mode="silu_mul", in1_offset=1920, in1_stride=128), "end at float 128 / 2112 of a buffer of 2048"), (dict(in0_offset=-4), "end at float"),
    (dict(mode="norm", kernel="fused", K=16416, n=40000, in1_offset=20000), "FUSED .k_dense_prep. refused for NORM with K 16416: .* K / 16 <= 1024"),
    (dict(mode="norm", kernel="fused", wtype=0, K=22016, N=1, n=50000, in1_offset=24000), "FUSED .k_dense_prep. refused for NORM with K 22016"),
])
def test_dense_prep_refusals_need_no_device(L, kw, msg):
    with pytest.raises(L.LlamaHipError, match=msg):
        dprep(L, **kw)


@pytest.mark.parametrize("kw,msg", [(dict(tokens=[0, 4]), "token 4 of row 1 outside .0, 4."), (dict(tokens=[-1]), "token -1 of row 0"),
                                    (dict(tokens=[1], x_stride=60), "x_stride 60 < d 64"), (dict(tokens=[]), "bad arguments"),
                                    (dict(tokens=[1], wtype=2), "wtype 2"), (dict(tokens=[1], wtype=4), "wtype 4")])
@pytest.mark.parametrize("table", ["f32", "f16", "q41"])
def test_embed_dense_refusals_need_no_device(L, table, kw, msg):
    emb = {"f32": np.zeros((4, 64), np.float32), "f16": np.zeros((4, 64), np.float16), "q41": np.zeros((4, 48), np.uint8)}[table]
    kw = dict(kw)
    with pytest.raises(L.LlamaHipError, match=msg):
        L.op_embed_dense(kw.pop("tokens"), emb, **kw)


def test_good_arguments_pass_every_host_check(L):
    """the limits themselves are accepted: what stops these calls on a machine without a GPU is the device check, nothing earlier"""
    for call in (lambda: dprep(L, mode="norm", K=16384, N=1, n=40000, in1_offset=20000, kernel="fused"),
                 lambda: dprep(L, mode="norm", K=16416, N=1, n=40000, in1_offset=20000, kernel="split"),
                 lambda: dprep(L, mode="norm", wtype=0, K=16416, N=1, n=40000, in1_offset=20000),
                 lambda: dprep(L, mode="silu_mul", in1_offset=64, in_stride=128, in1_stride=128),
                 lambda: L.op_embed_dense([0, 3], np.zeros((4, 64), np.float16), x_stride=64),
                 lambda: L.op_embed_dense([3], np.zeros((4, 48), np.uint8), x_stride=72)):
        try:
            call()
        except L.LlamaHipError as e:
            assert "no HIP device available" in str(e)
