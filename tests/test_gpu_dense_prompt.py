"""GPU (-m gpu): long evals and chunked evals of f16 / f32 model files -- the matrix-core mat-mul k_dense_mfma inside a model handle and the one
pass that llamahip_eval_chunks / llamahip_eval_logprobs take on such files -- against the reference build's own evals (its outputs stored in
tests/golden/ref_outputs_dense_prompt.npz, tests/refgolden.py: last logits, and digests of every layer's KV rows).
  small         n_embd 256, n_ff 768 (both K multiples of 128: every mat-mul of a forced handle runs on k_dense_mfma), head size 128, 2 layers
  f16_7b_width  tests/test_gpu_dense_set.py's single 7B-width layer, with the kernel rule left alone
The reference evaluates a chunked prompt as the evals themselves, 9 tokens at a time."""
import os
import shutil

import numpy as np
import pytest

import refgolden
import synth
from test_gpu_dense_set import SHAPES as SET_SHAPES

HERE = os.path.dirname(os.path.abspath(__file__))
STORE = os.path.join(HERE, "golden", "ref_outputs_dense_prompt.npz")

SHAPES = {
    "small": synth.HParams(n_vocab=300, n_embd=256, n_mult=256, n_head=2, n_layer=2),
    "f16_7b_width": SET_SHAPES["f16_7b_width"],
}
CASES = [("small", "f16", 8), ("small", "f16", 3), ("small", "f32", 8), ("f16_7b_width", "f16", 8)]
N_CTX, CHUNK = 160, 9


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def write_model(tmp, shape, ftype):
    hp = SHAPES[shape]
    path = os.path.join(str(tmp), f"{shape}_{ftype}.bin")
    synth.write_model_unquantized(path, hp, synth.random_tensors(hp, seed=1601), 0 if ftype == "f32" else 1)
    return path


def tokens(hp, n, seed):
    return synth.synth_prompt(n, hp.n_vocab, seed=seed)


def _kv_digests(model, hp, n_pos, tag, out):
    for il in range(hp.n_layer):
        k, v = model.kv(il, n_pos)
        out[f"{tag}_k{il}"], out[f"{tag}_v{il}"] = refgolden.digest(k), refgolden.digest(v)


@refgolden.computed_by("gpu_dense_prompt.evals", CASES, store=STORE)
def _ref_evals(ref, tmp, shape, ftype, nth):
    hp = SHAPES[shape]
    rm = ref.load(write_model(tmp, shape, ftype), N_CTX)
    out = {}
    for n in ((131,) if shape == "f16_7b_width" else (70, 131)):
        out[f"e{n}"] = rm.eval(tokens(hp, n, 300 + n), 0, nth)["logits"]
        _kv_digests(rm, hp, n, f"e{n}", out)
    if shape == "small":
        t = tokens(hp, 70, 377)
        rm.eval(t[:30], 0, nth)
        out["e40p30"] = rm.eval(t[30:], 30, nth)["logits"]
        _kv_digests(rm, hp, 70, "e40p30", out)
        t = tokens(hp, 70, 388)
        for c in range(0, 70, CHUNK):                                           # the reference's prompt loop: the evals themselves
            out["c70"] = rm.eval(t[c:c + CHUNK], c, nth)["logits"]
        _kv_digests(rm, hp, 70, "c70", out)
    rm.close()
    return out


@pytest.fixture(scope="module")
def model_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense_prompt_models")
    made = {}

    def get(shape, ftype):
        if (shape, ftype) not in made:
            made[(shape, ftype)] = write_model(d, shape, ftype)
        return made[(shape, ftype)]
    yield get
    shutil.rmtree(str(d), ignore_errors=True)


@pytest.fixture(autouse=True)
def _the_measured_rule_again(L):
    yield
    L.dense_force(0)


def _check_kv(m, hp, n_pos, tag, want):
    got = {}
    _kv_digests(m, hp, n_pos, tag, got)
    bad = [k for k in got if not same(got[k], want[k])]
    assert not bad, f"KV rows differ from the reference's: {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("shape,ftype,nth", CASES[:3])
def test_forced_mfma_evals_vs_reference(L, ref, tmp_path, model_files, shape, ftype, nth):
    want = refgolden.outputs("gpu_dense_prompt.evals", ref, tmp_path, shape, ftype, nth)
    hp = SHAPES[shape]
    assert L.dense_force("mfma") == "auto"
    before = L.dense_mfma_launches()
    with L.Model(model_files(shape, ftype), n_ctx=N_CTX) as m:
        for n in (70, 131):
            assert same(m.eval(tokens(hp, n, 300 + n), 0, nth), want[f"e{n}"]), f"eval of {n} tokens"
            _check_kv(m, hp, n, f"e{n}", want)
        t = tokens(hp, 70, 377)
        m.eval(t[:30], 0, nth)
        assert same(m.eval(t[30:], 30, nth), want["e40p30"])
        _check_kv(m, hp, 70, "e40p30", want)
    # 4 evals of more than 16 rows x 2 layers x 4 mat-muls (the lm head takes the last row alone)
    assert L.dense_mfma_launches() - before == 4 * hp.n_layer * 4
    assert L.dense_force(0) == "mfma"


@pytest.mark.gpu
def test_the_rule_left_alone_on_a_7b_width_layer(L, ref, tmp_path, model_files):
    shape, ftype, nth = CASES[3]
    want = refgolden.outputs("gpu_dense_prompt.evals", ref, tmp_path, shape, ftype, nth)
    hp = SHAPES[shape]
    with L.Model(model_files(shape, ftype), n_ctx=N_CTX) as m:
        assert same(m.eval(tokens(hp, 131, 431), 0, nth), want["e131"])
        _check_kv(m, hp, 131, "e131", want)


def _chunk_loop_scores(m, t, nth):
    """eval_logprobs chunk by chunk: the evals themselves, each chunk's rows scored against the stream's next token"""
    tgt = np.concatenate([t[1:], [-1]]).astype(np.int32)
    parts = [m.eval_logprobs(t[c:c + CHUNK], c, n_threads=nth, targets=tgt[c:c + CHUNK]) for c in range(0, len(t), CHUNK)]
    return {k: np.concatenate([p[k] for p in parts]) for k in ("logprob", "argmax", "rank")}, parts[-1]["logits"]


@pytest.mark.gpu
@pytest.mark.parametrize("ftype", ["f16", "f32"])
def test_chunked_evals_take_one_pass(L, ref, tmp_path, model_files, ftype):
    """eval_chunks / eval_logprobs of 70 tokens, 9 at a time: the reference's chunk-by-chunk logits and KV rows, the same bits on either
    mat-mul kernel, on a plain handle and on a two-stage pipeline handle; the plain handle counts ONE eval for the eight chunks"""
    want = refgolden.outputs("gpu_dense_prompt.evals", ref, tmp_path, "small", ftype, 8)
    hp = SHAPES["small"]
    t = tokens(hp, 70, 388)
    path = model_files("small", ftype)
    with L.Model(path, n_ctx=N_CTX) as m:
        loop_scores, loop_last = _chunk_loop_scores(m, t, 8)
        assert same(loop_last, want["c70"])
    for opts in ({}, dict(devices=[0, 0])):
        for force in (0, "mfma", "mm"):
            L.dense_force(force)
            before = L.dense_mfma_launches()
            with L.Model(path, n_ctx=N_CTX, **opts) as m:
                e0 = m.stats()["n_evals"]
                assert same(m.eval_chunks(t, 0, CHUNK, 8), want["c70"]), (opts, force)
                if not opts:
                    assert m.stats()["n_evals"] - e0 == 1, "70 tokens in chunks of 9 on an f16 / f32 file: one pass"
                _check_kv(m, hp, 70, "c70", want)
                got = m.eval_logprobs(t, 0, n_threads=8, chunk_tokens=CHUNK)
                assert same(got["logits"], want["c70"]), (opts, force)
                for k in ("logprob", "argmax", "rank"):
                    assert same(got[k], loop_scores[k]), (opts, force, k)
                _check_kv(m, hp, 70, "c70", want)
            if force == "mfma":
                assert L.dense_mfma_launches() > before
            if force == "mm":
                assert L.dense_mfma_launches() == before


@pytest.mark.gpu
def test_a_q4_1_file_keeps_the_chunk_loop(L, tmp_path, model_files):
    hp = SHAPES["small"]
    path = str(tmp_path / "small_q41.bin")
    L.quantize_file(model_files("small", "f16"), path, 3)
    t = tokens(hp, 70, 388)
    L.dense_force("mfma")
    before = L.dense_mfma_launches()
    with L.Model(path, n_ctx=N_CTX) as m:
        for c in range(0, 70, CHUNK):
            last = m.eval(t[c:c + CHUNK], c, 8)
        kv = [m.kv(il, 70) for il in range(hp.n_layer)]
        e0 = m.stats()["n_evals"]
        assert same(m.eval_chunks(t, 0, CHUNK, 8), last)
        assert m.stats()["n_evals"] - e0 == 8
        for il in range(hp.n_layer):
            k, v = m.kv(il, 70)
            assert same(k, kv[il][0]) and same(v, kv[il][1])
    assert L.dense_mfma_launches() == before
