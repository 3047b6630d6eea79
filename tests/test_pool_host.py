"""CPU: the host half of text embeddings -- llamahip_text_embedding, llamahip_text_embedding_multi, llamahip_op_pool_rows.  The symbols; every
refusal of the three entry points on a HOST_ONLY handle or with no handle (the arguments first, the limit and the function named, the handle
last); the argument checks under ASan + UBSan in the stand-alone program `make asan` builds; and the CPU half of tests/test_gpu_pool_op.py:
its cases cover the shapes and regimes they are meant to, every input row is order-proof for the norm, and the one row that is not is held
against the float64 bound instead."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pool_cases as cases
import pool_ref
import prep_cases as pc
import synth

HOST_ONLY = 4
HP = synth.HParams(n_vocab=96, n_embd=128, n_mult=64, n_head=2, n_layer=2)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
t = lambda n: np.arange(1, n + 1, dtype=np.int32)


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("pool") / "m.bin")
    synth.write_model(path, HP, synth.random_tensors(HP, seed=3))
    return path


@pytest.fixture(scope="module")
def host_model(L, model_path):
    with L.Model(model_path, n_ctx=48, flags=HOST_ONLY, n_seq=3) as m:
        yield m


def refused(L, call, fn, *words):
    with pytest.raises(L.LlamaHipError) as e:
        call()
    msg = e.value.message
    assert e.value.code == L.binding.ERR_PREDICT and msg.startswith(fn + ":") and all(w in msg for w in words), msg
    return msg


def test_new_symbols_are_declared_and_exported(L):
    names = L.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for fn in ("llamahip_text_embedding", "llamahip_text_embedding_multi", "llamahip_op_pool_rows"):
        assert fn in names and hasattr(L.lib(), fn) and fn in exported, fn
    assert not [s for s in exported if "embed_check" in s or "pool_rows_check" in s or "k_pool" in s or "k_norm_rows" in s]          # (lh:: internals stay local)
    assert hasattr(L.Model, "text_embedding") and hasattr(L.Model, "text_embedding_multi") and (L.POOL_LAST, L.POOL_MEAN) == (0, 1)
    assert "llamahip_op_embed" in names          # (the token-embedding gather keeps its own name)


def test_text_embedding_multi_refusals_touch_no_device(L, host_model):
    fn = "llamahip_text_embedding_multi"
    ok = dict(slots=[2, 0], n_past=[0, 5], token_lists=[t(4), t(9)], chunk_tokens=9, pool="mean", normalize=True)
    bad = [(dict(slots=[], n_past=[], token_lists=[]), ("n_seqs (0)", "1 .. 3")),
           (dict(slots=[0, 1, 2, 0], n_past=[0] * 4, token_lists=[t(1)] * 4), ("n_seqs (4)", "1 .. 3")),
           (dict(slots=[1, 1]), ("slot 1", "named twice")), (dict(slots=[3, 0]), ("out of range [0, 3)",)),
           (dict(token_lists=[t(4), t(0)]), ("n_tokens[1]", ">= 1")),
           (dict(n_past=[0, 40]), ("context overflow", "n_ctx (48)")), (dict(n_past=[-1, 5]), ("context overflow",)),
           (dict(token_lists=[t(4), np.array([1, 96], np.int32)]), ("token id 96", "[0, 96)")),
           (dict(chunk_tokens=-1), ("chunk_tokens (-1)", ">= 0")),
           (dict(pool=2), ("pool (2)", "LLAMAHIP_POOL_LAST (0)", "LLAMAHIP_POOL_MEAN (1)")), (dict(pool=-1), ("pool (-1)",)),
           (dict(normalize=2), ("normalize (2)", "0 or 1")), (dict(normalize=-1), ("normalize (-1)", "0 or 1"))]
    for change, words in bad:
        msg = refused(L, lambda: host_model.text_embedding_multi(**dict(ok, **change)), fn, *words)
        assert "HOST_ONLY" not in msg, msg
    # the arguments are fine -- a one-token segment among them -- and the handle is refused, last
    for change in (dict(), dict(pool="last", normalize=False), dict(token_lists=[t(1), t(43)], chunk_tokens=0)):
        refused(L, lambda: host_model.text_embedding_multi(**dict(ok, **change)), fn, "HOST_ONLY")
    with pytest.raises(ValueError):
        host_model.text_embedding_multi([0, 1], [0], [t(2), t(2)])


def test_text_embedding_refusals_touch_no_device(L, host_model):
    fn = "llamahip_text_embedding"
    ok = dict(tokens=t(9), n_past=5, chunk_tokens=9, pool="mean", normalize=True)
    bad = [(dict(tokens=[]), ("n_tokens[0]", ">= 1")), (dict(n_past=40), ("context overflow", "n_ctx (48)")), (dict(n_past=-1), ("context overflow",)),
           (dict(tokens=[1, 96]), ("token id 96", "[0, 96)")), (dict(tokens=[-1]), ("token id -1",)), (dict(chunk_tokens=-1), ("chunk_tokens (-1)", ">= 0")),
           (dict(pool=2), ("pool (2)",)), (dict(normalize=2), ("normalize (2)", "0 or 1"))]
    for change, words in bad:
        msg = refused(L, lambda: host_model.text_embedding(**dict(ok, **change)), fn, *words)
        assert "HOST_ONLY" not in msg, msg
    for change in (dict(), dict(tokens=[7], n_past=47, pool="last"), dict(tokens=t(48), n_past=0, chunk_tokens=0)):
        refused(L, lambda: host_model.text_embedding(**dict(ok, **change)), fn, "HOST_ONLY")


def test_row_cap_null_out_and_null_handle(L, model_path):
    """R = 2049 needs a context that holds it; a null out and a null handle are refused before anything is read"""
    with L.Model(model_path, n_ctx=1100, flags=HOST_ONLY, n_seq=2) as m:
        one = lambda n: np.ones(n, np.int32)
        refused(L, lambda: m.text_embedding_multi([0, 1], [0, 0], [one(1024), one(1025)]), "llamahip_text_embedding_multi", "LLAMAHIP_EVAL_MULTI_MAX_ROWS", "2049")
        refused(L, lambda: m.text_embedding_multi([0, 1], [0, 0], [one(1024), one(1024)]), "llamahip_text_embedding_multi", "HOST_ONLY")
        err = C.create_string_buffer(256)
        one1 = np.ones(1, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = L.lib().llamahip_text_embedding(m._h, 8, 0, p(one1), 1, 0, 0, 0, None, err, len(err))
        assert rc == L.binding.ERR_PREDICT and err.value == b"llamahip_text_embedding: null out"
        rc = L.lib().llamahip_text_embedding_multi(m._h, 8, 1, p(one1 * 0), p(one1 * 0), p(one1), p(one1), 0, 1, 1, None, None, err, len(err))
        assert rc == L.binding.ERR_PREDICT and err.value == b"llamahip_text_embedding_multi: null out"
    out = np.zeros(HP.n_embd, np.float32)
    rc = L.lib().llamahip_text_embedding(None, 8, 0, p(one1), 1, 0, 0, 0, p(out), err, len(err))
    assert rc == L.binding.ERR_PREDICT and err.value == b"llamahip_text_embedding: null model"
    rc = L.lib().llamahip_text_embedding_multi(None, 8, 1, p(one1 * 0), p(one1 * 0), p(one1), p(one1), 0, 0, 0, p(out), None, err, len(err))
    assert rc == L.binding.ERR_PREDICT and err.value == b"llamahip_text_embedding_multi: null model"


def test_op_pool_rows_refusals_need_no_device(L):
    fn = "llamahip_op_pool_rows"
    x = lambda R, d: np.zeros((R, d), np.float32)
    w = lambda d: np.ones(d, np.float32)
    bad = [((x(3, 16), w(16), [0, 3]), {}, ("d (16)", "multiple of 32")), ((x(3, 48), w(48), [0, 3]), {}, ("d (48)", "multiple of 32")),
           ((x(2049, 32), w(32), [0, 2049]), {}, ("R (2049)", "1 .. LLAMAHIP_EVAL_MULTI_MAX_ROWS (2048)")),
           ((x(0, 32), w(32), [0, 0]), {}, ("R (0)",)),
           ((x(3, 32), w(32), [0]), {}, ("n_segs (0)", "1 .. LLAMAHIP_POOL_MAX_SEGS (16)")),
           ((x(17, 32), w(32), list(range(18))), {}, ("n_segs (17)", "1 .. LLAMAHIP_POOL_MAX_SEGS (16)")),
           ((x(3, 32), w(32), [0, 3]), dict(pool=2), ("pool (2)",)), ((x(3, 32), w(32), [0, 3]), dict(normalize=2), ("normalize (2)", "0 or 1")),
           ((x(3, 32), w(32), [1, 3]), {}, ("from 0 to R (3)", "seg_begin[0] = 1")), ((x(3, 32), w(32), [0, 2]), {}, ("from 0 to R (3)", "seg_begin[1] = 2")),
           ((x(3, 32), w(32), [0, 2, 2, 3]), {}, ("rise strictly", "seg_begin[2] = 2")), ((x(3, 32), w(32), [0, 2, 1, 3]), {}, ("rise strictly",))]
    for args, kw, words in bad:
        refused(L, lambda: L.op_pool_rows(*args, **kw), fn, *words)
    err = C.create_string_buffer(256)
    seg = np.array([0, 1], np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((None, 1, 32, p(w(32)), p(seg), 1, 0, 0, p(x(1, 32))), (p(x(1, 32)), 1, 32, None, p(seg), 1, 0, 0, p(x(1, 32))),
                 (p(x(1, 32)), 1, 32, p(w(32)), None, 1, 0, 0, p(x(1, 32))), (p(x(1, 32)), 1, 32, p(w(32)), p(seg), 1, 0, 0, None)):
        rc = L.lib().llamahip_op_pool_rows(*args, err, len(err))
        assert rc == L.binding.ERR_PREDICT and err.value == b"llamahip_op_pool_rows: null x, norm_w, seg_begin or out"
    # the limits themselves pass every host check: what stops the call on a machine without a GPU is the device check, nothing earlier
    for call in (lambda: L.op_pool_rows(x(2048, 32), w(32), [0, 2048], "mean", True), lambda: L.op_pool_rows(x(16, 32), w(32), list(range(17)), "last")):
        try:
            call()
        except L.LlamaHipError as e:
            assert "no HIP device available" in str(e)


def test_embedding_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: eval_multi.cpp's embedding checks over exactly sized arrays and message buffers, compiled with -fsanitize=address,undefined
    into the stand-alone tools/host_sanitize and run there -- never loaded into python"""
    subprocess.run(["make", "-s", "-C", CSRC, "asan"], check=True)
    src = open(os.path.join(CSRC, "tools", "host_sanitize.cpp")).read()
    assert "lh::embed_check(" in src and "lh::pool_rows_check(" in src
    path = str(tmp_path / "m.bin")
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(CSRC, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout and "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if "text embeddings" in ln]
    assert len(line) == 1 and " 0 " not in line[0], r.stdout


# ------------------------------------------------------------------------------------------------ the CPU half of the GPU op test
def test_the_op_cases_cover_what_they_are_meant_to():
    ds = {c[1] for c in cases.CASES}
    assert ds == {32, 96, 256, 320, 4096}
    assert all(any(c[1] == d and c[2] == (1, 2, 7, 61, 300) for c in cases.CASES) for d in ds), "the mixed segments at every width"
    assert any(c[1] == 32 and c[2] == (2048,) for c in cases.CASES), "one segment of 2048 rows at d = 32"
    assert {len(c[2]) for c in cases.CASES} >= {1, 16}
    assert set(cases.VARIANTS) == {(p, n) for p in ("last", "mean") for n in (False, True)}
    seen = set()
    for c in cases.CASES:
        _, d, lens, nan = c
        assert d % 32 == 0 and 1 <= sum(lens) <= 2048 and 1 <= len(lens) <= 16
        x, w, sb, nan_seg = cases.build(c)
        assert x.shape == (sum(lens), d) and w.shape == (d,) and list(np.diff(sb)) == list(lens)
        reg = cases.row_regimes(lens)
        seen |= set(reg)
        for s, n in enumerate(lens):
            rows = x[sb[s]:sb[s + 1]]
            if n == 2:
                assert not rows.any(), "a whole all-zero segment"
                seen.add("zero_segment")
            if n == 7:
                assert not rows[-1].any() and rows[:-1].any(), "an all-zero row as a segment's last row"
                seen.add("zero_last_row")
        if np.signbit(x[x == 0]).any():
            seen.add("minus_zero")
        if np.abs(x[np.isfinite(x)]).max() > 1e17:
            seen.add("1e18")
        if nan:
            assert nan_seg >= 0 and np.isnan(x[sb[nan_seg]:sb[nan_seg + 1]]).sum() == 1 and np.isnan(x).sum() == 1 and len(lens) > 1
            seen.add("nan")
        else:
            assert nan_seg == -1 and np.isfinite(x).all()
    assert seen >= {"unit", "offset", "big", "zero", "zero_segment", "zero_last_row", "minus_zero", "1e18", "nan"}, seen


@pytest.mark.parametrize("c", cases.CASES, ids=cases.case_id)
def test_every_input_row_of_the_gpu_op_test_is_order_proof(c):
    x = cases.build(c)[0]
    for n, r in enumerate(x):
        if np.isnan(r).any():
            continue          # (the NaN row: its segment is held to NaN, not to bytes)
        assert pc.norm_stats(r)["proof"], (cases.case_id(c), n)


def test_the_reference_restatement_on_small_inputs(oracle):
    """pool_ref against definitions written out by hand: the mean of three rows, the butterfly against a plain lane sum where both are exact, a
    zero vector under the normalisation"""
    y = np.array([[1.0, -2.0] + [0.0] * 30, [3.0, 0.5] + [0.0] * 30, [5.0, 1.5] + [0.0] * 30], np.float32)
    assert np.array_equal(pool_ref.pool_segment(y, "last"), y[2]) and np.array_equal(pool_ref.pool_segment(y, "mean")[:2], np.array([3.0, 0.0], np.float32))
    o = np.zeros(96, np.float32)
    o[[0, 64, 65, 95]] = [3.0, 4.0, 12.0, 84.0]          # 9 + 16 + 144 + 7056 = 7225 = 85^2
    assert np.array_equal(pool_ref.l2_normalize(o), (o.astype(np.float64) / 85.0).astype(np.float32))
    z = np.zeros(32, np.float32)
    z[5] = -0.0
    assert np.array_equal(pool_ref.l2_normalize(z).view(np.uint32), z.view(np.uint32))
    x = np.random.default_rng(1).standard_normal((4, 64)).astype(np.float32)
    w = np.full(64, 2.0, np.float32)
    got = pool_ref.pool_rows(oracle, x, w, [0, 1, 4], "last", False)
    want = oracle.unary_rows("norm", x[[0, 3]]) * w
    assert np.array_equal(got, want.astype(np.float32))


def test_the_row_that_is_not_order_proof_meets_the_float64_bound(oracle):
    x, w = cases.cancel_input()
    assert not pc.norm_stats(x[0])["proof"]
    y64, B = pc.norm_f64_bound(x[0], w)
    y = pool_ref.norm_rows(oracle, x, w)[0]
    assert np.all(np.abs(y.astype(np.float64) - y64) <= B)


def test_embedding_tool_is_built(built):
    tool = os.path.join(CSRC, "tools", "embedding")
    assert os.access(tool, os.X_OK)
    r = subprocess.run([tool], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage: embedding MODEL" in r.stderr
