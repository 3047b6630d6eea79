"""GPU (-m gpu): a Q4_1 model file at widths the other Q4_1 model tests do not reach (K = 1344 and 3584: several slabs of k_q41_chain and a
short last one at every row count; 250 lm-head rows: a row tail against the workgroup edge), against the reference build's own arithmetic
(its outputs stored in tests/golden/ref_outputs_q41.npz, tests/refgolden.py), and on the kernel model handles are meant to run:
L.q41_paths() must show k_q41_chain launches and no k_q41_mm launch."""
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
STORE = os.path.join(HERE, "golden", "ref_outputs_q41.npz")

HP = synth.HParams(n_vocab=250, n_embd=1344, n_mult=64, n_head=21, n_layer=1)
N_EVAL, N_NINE, N_SINGLE, N_GREEDY, N_CTX, NTH = 20, 9, 4, 12, 64, 8


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def file_sha256(path) -> np.ndarray:
    with open(path, "rb") as f:
        return np.frombuffer(hashlib.sha256(f.read()).digest(), np.uint8)


def write_model(tmp, quantize):
    path = os.path.join(str(tmp), "q41_wide.bin")
    synth.write_model_unquantized(path + ".f16", HP, synth.random_tensors(HP, seed=1741), 1)
    quantize(path + ".f16", path)
    os.remove(path + ".f16")
    return path


def tokens():
    return synth.synth_prompt(N_EVAL, HP.n_vocab, seed=71), synth.synth_prompt(N_NINE + 1, HP.n_vocab, seed=72)[1:]


@refgolden.computed_by("gpu_q41_model.evals", store=STORE)
def _ref_evals(ref, tmp):
    path = write_model(tmp, lambda s, t: subprocess.run([REFQ, s, t, "3"], check=True, stdout=subprocess.DEVNULL))
    p, c = tokens()
    rm = ref.load(path, N_CTX)
    out = {"file_sha256": file_sha256(path), "eval20_last": rm.eval(p, 0, NTH)["logits"]}
    n_past = N_EVAL
    lo = rm.eval(c, n_past, NTH)["logits"]
    out["eval9_last"] = lo
    n_past += N_NINE
    single = []
    for i in range(N_SINGLE):
        lo = rm.eval(np.array([np.argmax(lo)], np.int32), n_past, NTH)["logits"]
        single.append(lo); n_past += 1
    out["single"] = np.array(single)
    toks = [int(np.argmax(lo))]
    for i in range(N_GREEDY):
        lo = rm.eval(np.array([toks[-1]], np.int32), n_past, NTH)["logits"]
        toks.append(int(np.argmax(lo))); n_past += 1
    out["greedy_tokens"], out["greedy_last"] = np.array(toks[1:], np.int32), lo
    for il in range(HP.n_layer):
        k, v = rm.kv(il, n_past)
        out[f"k{il}"], out[f"v{il}"] = refgolden.digest(k), refgolden.digest(v)
    rm.close()
    return out


@pytest.fixture(scope="module")
def model_file(tmp_path_factory, L):
    d = tmp_path_factory.mktemp("q41_models")
    yield write_model(d, lambda s, t: L.quantize_file(s, t, 3))
    shutil.rmtree(str(d), ignore_errors=True)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 1])      # 1: LLAMAHIP_FLAG_NO_GRAPH, the greedy loop launched eagerly
def test_q41_model_on_the_chain_kernel_vs_reference(L, ref, tmp_path, model_file, flags):
    want = refgolden.outputs("gpu_q41_model.evals", ref, tmp_path)
    assert same(file_sha256(model_file), want["file_sha256"]), "model file differs from the reference tool's"
    p, c = tokens()
    before = L.q41_paths()
    with L.Model(model_file, n_ctx=N_CTX, flags=flags) as m:
        assert same(m.eval(p, 0, NTH), want["eval20_last"]), "20-row eval (two row tiles, one partial)"
        n_past = N_EVAL
        lo = m.eval(c, n_past, NTH)
        assert same(lo, want["eval9_last"]), "9-token eval"
        n_past += N_NINE
        for i in range(N_SINGLE):
            lo = m.eval(np.array([np.argmax(lo)], np.int32), n_past, NTH)
            assert same(lo, want["single"][i]), f"single-token eval {i}"
            n_past += 1
        toks, last = m.decode_greedy(int(np.argmax(lo)), n_past, N_GREEDY, NTH, want_logits=True)
        assert toks.tolist() == want["greedy_tokens"].tolist(), "greedy tokens"
        assert same(last, want["greedy_last"]), "greedy loop, last logits"
        n_past += N_GREEDY
        for il in range(HP.n_layer):
            k, v = m.kv(il, n_past)
            assert same(refgolden.digest(k), want[f"k{il}"]) and same(refgolden.digest(v), want[f"v{il}"]), f"KV rows of layer {il}"
    after = L.q41_paths()
    assert after["chain"] > before["chain"] and after["lane"] == before["lane"], (before, after)
