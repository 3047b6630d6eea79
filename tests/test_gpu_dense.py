"""GPU (-m gpu): f16 / f32 / Q4_1 model files (dense.hip) at the shapes where their kernels branch, against the reference build's own
arithmetic (its outputs stored in tests/golden/ref_outputs_dense.npz, tests/refgolden.py).  The goldens of test_gpu_parity.py use widths of 128 / 256
and at most 37-row evals; these shapes reach what a real f16 7B file takes:
  f16_7b_width  K = 4096 / 11008: the software-pipelined k_dense_mv loop (4 / 10 double batches) + 3 leftover groups, a 4-wave norm,
                SiLU * up sliced over 3 workgroups, k_dec_attn_x (H % 8 == 0, nth <= 8) and, at nth 12, k_dec_scores + k_dec_pv_blk
  odd_widths    K = 1344: pipelined loop, then a leftover group, then a 2-step tail group; 250 lm-head rows (row tails); a 2-wave norm
                with a partial wave; H = 21 (k_dec_scores + k_dec_pv_blk); a 600-token leg with decode attention over 600+ keys
  q41_odd       Q4_1 (the quantize tool's type 3, byte for byte the reference tool's file): 200 rows = a partial 64-row block, head size 32
Every case runs a 100-row prompt eval (the many-row attention kernels, ragged column tiles), a continuation in 9-token evals, single-token
evals, the device-resident greedy loop, and compares the KV rows of every layer -- bit for bit."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import refgolden
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
REFQ = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "quantize")
STORE = os.path.join(HERE, "golden", "ref_outputs_dense.npz")      # the reference's outputs for this module and the dense pipeline tests

SHAPES = {
    "f16_7b_width": synth.HParams(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=1),
    "odd_widths": synth.HParams(n_vocab=250, n_embd=1344, n_mult=64, n_head=21, n_layer=2),
    "q41_odd": synth.HParams(n_vocab=200, n_embd=320, n_mult=64, n_head=10, n_layer=2),
}
# (shape, file type, n_threads); f32 at the 7B width is left out (a 0.8 GB file for kernels the odd_widths f32 case already reaches)
CASES = [("f16_7b_width", "f16", nth) for nth in (8, 5, 12)] + [("odd_widths", ft, nth) for ft in ("f16", "f32") for nth in (8, 3)] + \
        [("q41_odd", "q41", nth) for nth in (8, 5)]
N_PROMPT, N_CONT, N_SINGLE, N_GREEDY, N_CTX = 100, 31, 4, 16, 160
LONG_PROMPT, LONG_GREEDY, LONG_CTX = 600, 24, 640


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def file_sha256(path) -> np.ndarray:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return np.frombuffer(h.digest(), np.uint8)


def write_model(tmp, shape, ftype, quantize=None, n_layer=None, seed=1601):
    """the model file of a case: f16 / f32 written directly; Q4_1 quantized from the f16 file by `quantize(src, dst)`"""
    hp = SHAPES[shape]
    if n_layer is not None:
        hp = synth.HParams(n_vocab=hp.n_vocab, n_embd=hp.n_embd, n_mult=hp.n_mult, n_head=hp.n_head, n_layer=n_layer)
    path = os.path.join(str(tmp), f"{shape}_{ftype}_{hp.n_layer}.bin")
    src = path + ".f16" if ftype == "q41" else path
    synth.write_model_unquantized(src, hp, synth.random_tensors(hp, seed=seed), 0 if ftype == "f32" else 1)
    if ftype == "q41":
        quantize(src, path)
        os.remove(src)
    return path


def ref_quantize(src, dst):
    subprocess.run([REFQ, src, dst, "3"], check=True, stdout=subprocess.DEVNULL)


def prompts(hp):
    return synth.synth_prompt(N_PROMPT, hp.n_vocab, seed=61), synth.synth_prompt(N_CONT, hp.n_vocab, seed=62)[1:]


@refgolden.computed_by("gpu_dense.branches", CASES, store=STORE)
def _ref_branches(ref, tmp, shape, ftype, nth):
    hp = SHAPES[shape]
    path = write_model(tmp, shape, ftype, ref_quantize)
    p, c = prompts(hp)
    rm = ref.load(path, N_CTX)
    r = rm.eval(p, 0, nth, all_logits=True)
    out = {"file_sha256": file_sha256(path), "prompt_all": refgolden.digest(r["logits_all"]), "prompt_last": r["logits"]}
    n_past = N_PROMPT
    for c0 in range(0, len(c), 9):
        lo = rm.eval(c[c0:c0 + 9], n_past, nth)["logits"]
        n_past += len(c[c0:c0 + 9])
    out["cont_last"] = lo
    single = []
    for i in range(N_SINGLE):
        lo = rm.eval(np.array([np.argmax(lo)], np.int32), n_past, nth)["logits"]
        single.append(lo); n_past += 1
    out["single"] = np.array(single)
    toks = [int(np.argmax(lo))]
    for i in range(N_GREEDY):
        lo = rm.eval(np.array([toks[-1]], np.int32), n_past, nth)["logits"]
        toks.append(int(np.argmax(lo))); n_past += 1
    out["greedy_tokens"], out["greedy_last"] = np.array(toks[1:], np.int32), lo
    for il in range(hp.n_layer):
        k, v = rm.kv(il, n_past)
        out[f"k{il}"], out[f"v{il}"] = refgolden.digest(k), refgolden.digest(v)
    rm.close()
    return out


@pytest.fixture(scope="module")
def model_files(tmp_path_factory, L):
    """one file per (shape, file type) for the whole module (the 7B-width f16 file is 0.4 GB), removed when the module is done"""
    d = tmp_path_factory.mktemp("dense_models")
    made = {}

    def get(shape, ftype):
        if (shape, ftype) not in made:
            made[(shape, ftype)] = write_model(d, shape, ftype, lambda s, t: L.quantize_file(s, t, 3))
        return made[(shape, ftype)]
    yield get
    shutil.rmtree(str(d), ignore_errors=True)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,ftype,nth", CASES)
def test_dense_kernel_branches_vs_reference(L, ref, tmp_path, model_files, shape, ftype, nth):
    want = refgolden.outputs("gpu_dense.branches", ref, tmp_path, shape, ftype, nth)
    hp = SHAPES[shape]
    path = model_files(shape, ftype)
    assert same(file_sha256(path), want["file_sha256"]), "model file differs from the reference's (Q4_1: the quantize tool's bytes)"
    p, c = prompts(hp)
    # 1: the greedy loop launched eagerly (NO_GRAPH); 16: FAST_PREFILL, which dense files never reach (it re-associates the Q4_0 prompt GEMMs only)
    for flags in ((0, 1) if (shape, ftype, nth) == ("odd_widths", "f16", 8) else (0,)) + ((16,) if nth == 8 else ()):
        with L.Model(path, n_ctx=N_CTX, flags=flags) as m:
            r = m.eval_debug(p, 0, nth, all_logits=True)
            assert same(r["logits"], want["prompt_last"]), f"flags {flags}: {N_PROMPT}-row prompt eval, last row"
            assert same(refgolden.digest(r["logits_all"]), want["prompt_all"]), f"flags {flags}: {N_PROMPT}-row prompt eval, all rows"
            lo = m.eval_chunks(c, N_PROMPT, 9, nth)
            assert same(lo, want["cont_last"]), f"flags {flags}: continuation in 9-token evals"
            n_past = N_PROMPT + len(c)
            for i in range(N_SINGLE):
                lo = m.eval(np.array([np.argmax(lo)], np.int32), n_past, nth)
                assert same(lo, want["single"][i]), f"flags {flags}: single-token eval {i}"
                n_past += 1
            toks, last = m.decode_greedy(int(np.argmax(lo)), n_past, N_GREEDY, nth, want_logits=True)
            assert toks.tolist() == want["greedy_tokens"].tolist(), f"flags {flags}: greedy tokens"
            assert same(last, want["greedy_last"]), f"flags {flags}: greedy loop, last logits"
            n_past += N_GREEDY
            for il in range(hp.n_layer):
                k, v = m.kv(il, n_past)
                assert same(refgolden.digest(k), want[f"k{il}"]) and same(refgolden.digest(v), want[f"v{il}"]), f"flags {flags}: KV rows of layer {il}"


@refgolden.computed_by("gpu_dense.long_context", store=STORE)
def _ref_long_context(ref, tmp):
    hp = SHAPES["odd_widths"]
    path = write_model(tmp, "odd_widths", "f16")
    p = synth.synth_prompt(LONG_PROMPT, hp.n_vocab, seed=63)
    rm = ref.load(path, LONG_CTX)
    lo = rm.eval(p, 0, 8)["logits"]
    out = {"prompt_last": lo}
    toks, n_past = [int(np.argmax(lo))], LONG_PROMPT
    for i in range(LONG_GREEDY):
        lo = rm.eval(np.array([toks[-1]], np.int32), n_past, 8)["logits"]
        toks.append(int(np.argmax(lo))); n_past += 1
    out["greedy_tokens"], out["greedy_last"] = np.array(toks[1:], np.int32), lo
    for il in range(hp.n_layer):
        k, v = rm.kv(il, n_past)
        out[f"k{il}"], out[f"v{il}"] = refgolden.digest(k), refgolden.digest(v)
    rm.close()
    return out


@pytest.mark.gpu
def test_dense_long_context_vs_reference(L, ref, tmp_path, model_files):
    """odd_widths, f16: a 600-row prompt eval, then 24 greedy steps whose decode attention covers 600+ keys on the dense path"""
    want = refgolden.outputs("gpu_dense.long_context", ref, tmp_path)
    hp = SHAPES["odd_widths"]
    p = synth.synth_prompt(LONG_PROMPT, hp.n_vocab, seed=63)
    with L.Model(model_files("odd_widths", "f16"), n_ctx=LONG_CTX) as m:
        lo = m.eval(p, 0, 8)
        assert same(lo, want["prompt_last"])
        toks, last = m.decode_greedy(int(np.argmax(lo)), LONG_PROMPT, LONG_GREEDY, 8, want_logits=True)
        assert toks.tolist() == want["greedy_tokens"].tolist() and same(last, want["greedy_last"])
        for il in range(hp.n_layer):
            k, v = m.kv(il, LONG_PROMPT + LONG_GREEDY)
            assert same(refgolden.digest(k), want[f"k{il}"]) and same(refgolden.digest(v), want[f"v{il}"]), f"KV rows of layer {il}"
