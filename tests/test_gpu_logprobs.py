"""GPU (-m gpu): scoring a text -- llamahip_eval_logprobs / llamahip_perplexity / llamahip_op_logprob and the perplexity tool.

The logits of every row are the oracle's bit for bit (oracle.eval(..., all_logits=True)); the per-row results of k_row_logprob are checked
against numpy on those rows: argmax and rank exactly, the float64 log-probability within 1e-10 (a different summation order).  The KV cache
and the last row of logits an eval_logprobs call leaves are bit-identical to llamahip_eval's / llamahip_eval_chunks'.  f16 / Q4_1 files
have no oracle here: their rows are eval_debug's (bit-exact to the reference build by test_gpu_dense.py)."""
import math
import os
import subprocess

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "llama.swift_amd", "csrc", "tools", "perplexity")
NO_PREFILL_COPY, FAST_PREFILL = 8, 16
TOL = 1e-10


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def np_scores(rows, targets):
    """reference values: float64 log-softmax at the target (max = the row's fp32 maximum), first-index argmax, strict rank"""
    rows = np.asarray(rows, np.float32)
    t = np.asarray(targets, np.int64)
    n = rows.shape[0]
    r = rows.astype(np.float64)
    mx = rows.max(axis=1).astype(np.float64)
    lse = np.log(np.exp(r - mx[:, None]).sum(axis=1))
    tc = np.maximum(t, 0)
    lt = rows[np.arange(n), tc]
    lp = np.where(t >= 0, (lt.astype(np.float64) - mx) - lse, 0.0)
    rank = np.where(t >= 0, (rows > lt[:, None]).sum(axis=1), -1)
    return lp, rows.argmax(axis=1).astype(np.int32), rank.astype(np.int32)


def check_scores(got, rows, targets):
    lp, am, rk = np_scores(rows, targets)
    assert np.array_equal(got["argmax"], am)
    assert np.array_equal(got["rank"], rk)
    assert np.all(got["logprob"][np.asarray(targets) < 0] == 0.0)
    assert np.max(np.abs(got["logprob"] - lp)) <= TOL


def next_targets(toks):
    return np.append(np.asarray(toks[1:], np.int32), np.int32(-1))


def write_q4(tmp_path, hp, seed, name="m.bin"):
    path = str(tmp_path / name)
    synth.write_model(path, hp, synth.random_tensors(hp, seed=seed))
    return path


def test_big_vocabulary_rows_take_the_matrix_core_lm_head(L, oracle, tmp_path):
    hp = synth.HParams(n_vocab=32000, n_embd=256, n_mult=64, n_head=2, n_layer=2)
    path = write_q4(tmp_path, hp, seed=71)
    toks = synth.synth_prompt(511, hp.n_vocab, seed=72)
    om = oracle.load(path, 512)
    want = om.eval(toks, 0, 8, all_logits=True)
    okv = [om.kv(il, 511) for il in range(hp.n_layer)]
    om.close()
    with L.Model(path, n_ctx=512) as m:
        p0 = L.gemm_paths()
        got = m.eval_logprobs(toks, 0, n_threads=8)
        p1 = L.gemm_paths()
        kv = [m.kv(il, 511) for il in range(hp.n_layer)]
        last = m.eval(toks, 0, n_threads=8)
        p2 = L.gemm_paths()
        kv_eval = [m.kv(il, 511) for il in range(hp.n_layer)]
    # one more matrix-core launch than the plain eval: the all-rows lm head (k_gemm_mfma4)
    assert p1["mfma"] - p0["mfma"] == p2["mfma"] - p1["mfma"] + 1
    check_scores(got, want["logits_all"], next_targets(toks))
    assert same(got["logits"], last) and same(last, want["logits"])
    for il in range(hp.n_layer):
        assert same(kv[il][0], kv_eval[il][0]) and same(kv[il][1], kv_eval[il][1])
        assert same(kv[il][0], okv[il][0]) and same(kv[il][1], okv[il][1])
    with L.Model(path, n_ctx=512, flags=NO_PREFILL_COPY) as m:
        nc = m.eval_logprobs(toks, 0, n_threads=8)
    for k in ("logprob", "argmax", "rank", "logits"):
        assert same(nc[k], got[k]), k
    # a FAST_PREFILL handle has the int8 matrix-core copies instead of mt4: its all-rows lm head takes the int8 EXACT kernel (fast is for the
    # layers only), and no layer matrix of this width reaches the fast kernel's 512 workgroups -- so every field and KV row is the exact one
    with L.Model(path, n_ctx=512, flags=FAST_PREFILL) as m:
        p0 = L.gemm_paths()
        fa = m.eval_logprobs(toks, 0, n_threads=8)
        p1 = L.gemm_paths()
        fkv = [m.kv(il, 511) for il in range(hp.n_layer)]
        flast = m.eval(toks, 0, n_threads=8)
        p2 = L.gemm_paths()
        fkv_eval = [m.kv(il, 511) for il in range(hp.n_layer)]
    assert p1["mfma"] - p0["mfma"] == 1 and p2["mfma"] == p1["mfma"], (p0, p1, p2)       # the lm head alone, on k_gemm_mfma<*, false>
    assert p2["fast"] == p0["fast"], (p0, p2)
    for k in ("logprob", "argmax", "rank", "logits"):
        assert same(fa[k], got[k]), k
    assert same(flast, last)
    for il in range(hp.n_layer):
        for a, b in ((fkv[il], kv[il]), (fkv_eval[il], kv_eval[il])):
            assert same(a[0], b[0]) and same(a[1], b[1]), f"FAST handle: KV rows of layer {il}"


RAGGED = synth.HParams(n_vocab=250, n_embd=128, n_mult=64, n_head=2, n_layer=3)


@pytest.fixture
def ragged(tmp_path):
    return write_q4(tmp_path, RAGGED, seed=81)


def ragged_targets(n, seed):
    t = np.random.default_rng(seed).integers(0, RAGGED.n_vocab, size=n, dtype=np.int32)
    t[::5] = -1
    return t


def test_ragged_shapes_against_the_oracle(L, oracle, ragged):
    prefix = synth.synth_prompt(7, RAGGED.n_vocab, seed=82)
    om = oracle.load(ragged, 256)
    om.eval(prefix, 0, 8)
    with L.Model(ragged, n_ctx=256) as m:
        m.eval(prefix, 0, n_threads=8)
        for nth in (8, 3):
            for N in (1, 9, 33, 100):
                toks = synth.synth_prompt(N + 1, RAGGED.n_vocab, seed=83 + N)[1:]
                tgt = ragged_targets(N, N)
                want = om.eval(toks, 7, nth, all_logits=True)
                got = m.eval_logprobs(toks, 7, n_threads=nth, targets=tgt)
                check_scores(got, want["logits_all"], tgt)
                assert same(got["logits"], want["logits"])
                for il in range(RAGGED.n_layer):
                    k, v = m.kv(il, 7 + N)
                    ok, ov = om.kv(il, 7 + N)
                    assert same(k, ok) and same(v, ov), (nth, N, il)
        # chunk_tokens 9: the oracle evaluated chunk by chunk
        toks = synth.synth_prompt(101, RAGGED.n_vocab, seed=99)[1:]
        rows = [om.eval(toks[c:c + 9], 7 + c, 8, all_logits=True)["logits_all"] for c in range(0, 100, 9)]
        got = m.eval_logprobs(toks, 7, n_threads=8, chunk_tokens=9)
        check_scores(got, np.concatenate(rows), next_targets(toks))
        assert same(got["logits"], m.eval_chunks(toks, 7, chunk_tokens=9, n_threads=8))
        assert same(got["logits"], rows[-1][-1])
    om.close()


def test_scores_are_a_function_of_the_row_bits(L, ragged):
    toks = synth.synth_prompt(100, RAGGED.n_vocab, seed=91)
    tgt = ragged_targets(100, 92)
    with L.Model(ragged, n_ctx=128) as m:
        a = m.eval_logprobs(toks, 0, n_threads=8, targets=tgt)
        b = m.eval_logprobs(toks, 0, n_threads=8, targets=tgt)
        rows = m.eval_debug(toks, 0, n_threads=8)["logits_all"]
    for k in ("logprob", "argmax", "rank", "logits"):
        assert same(a[k], b[k]), k
    lp, am, rk = L.op_logprob(rows, tgt)
    assert same(lp, a["logprob"]) and same(am, a["argmax"]) and same(rk, a["rank"])
    # one row alone, or the rows in another order: the same bits
    lp1, _, _ = L.op_logprob(rows[37:38], tgt[37:38])
    assert same(lp1, a["logprob"][37:38])
    perm = np.random.default_rng(3).permutation(100)
    lpp, amp, rkp = L.op_logprob(rows[perm], tgt[perm])
    assert same(lpp, a["logprob"][perm]) and same(amp, a["argmax"][perm]) and same(rkp, a["rank"][perm])


def test_crafted_rows(L):
    rng = np.random.default_rng(5)
    for V in (1, 31, 250, 32001):
        rows = rng.standard_normal((6, V)).astype(np.float32) * 4
        tgt = rng.integers(0, V, size=6).astype(np.int32)
        if V > 3:
            rows[0, [2, V - 1, 1]] = 50.0                  # ties at the maximum: the lowest index
            rows[1, [0, V // 2, V - 2]] = 1.5              # a target tied with others: rank counts strictly greater only
            tgt[1] = V // 2
            rows[2] = rng.uniform(-1e30, 1e30, V).astype(np.float32)
            rows[3, ::3] = -np.inf
            tgt[3] = 1
        tgt[5] = -1                                         # unscored
        lp, am, rk = L.op_logprob(rows, tgt)
        check_scores({"logprob": lp, "argmax": am, "rank": rk}, rows, tgt)
        if V > 3:
            assert am[0] == 1 and rk[1] == (rows[1] > 1.5).sum()
        assert rk[5] == -1 and lp[5] == 0.0
    rows = rng.standard_normal((4, 300)).astype(np.float32)
    rows[0, 17] = np.nan
    rows[1, 250] = np.inf
    rows[2, 3] = np.nan
    lp, am, rk = L.op_logprob(rows, np.array([4, 5, -1, 6], np.int32))
    assert np.isnan(lp[0]) and np.isnan(lp[1]) and np.isnan(lp[2])
    assert list(am[:3]) == [-1, -1, -1] and list(rk[:3]) == [-1, -1, -1]
    check_scores({"logprob": lp[3:], "argmax": am[3:], "rank": rk[3:]}, rows[3:], [6])
    lp, am, rk = L.op_logprob(rows[3:])                    # no targets: nothing scored
    assert lp[0] == 0.0 and rk[0] == -1 and am[0] == rows[3].argmax()


DENSE = synth.HParams(n_vocab=200, n_embd=320, n_mult=64, n_head=10, n_layer=3)


def write_dense(L, tmp_path, ftype):
    path = str(tmp_path / f"dense_{ftype}.bin")
    src = path + ".f16" if ftype == "q41" else path
    synth.write_model_unquantized(src, DENSE, synth.random_tensors(DENSE, seed=1601), 1)
    if ftype == "q41":
        L.quantize_file(src, path, 3)
        os.remove(src)
    return path


@pytest.mark.parametrize("ftype", ["f16", "q41"])
def test_dense_file_types(L, tmp_path, ftype):
    path = write_dense(L, tmp_path, ftype)
    toks = synth.synth_prompt(70, DENSE.n_vocab, seed=101)
    with L.Model(path, n_ctx=128) as m:
        got = m.eval_logprobs(toks, 0, n_threads=8)
        kv = [m.kv(il, 70) for il in range(DENSE.n_layer)]
        dbg = m.eval_debug(toks, 0, n_threads=8)
        check_scores(got, dbg["logits_all"], next_targets(toks))
        assert same(got["logits"], m.eval(toks, 0, n_threads=8))
        for il in range(DENSE.n_layer):
            k, v = m.kv(il, 70)
            assert same(k, kv[il][0]) and same(v, kv[il][1])
        got = m.eval_logprobs(toks, 0, n_threads=8, chunk_tokens=16)
        rows = np.concatenate([m.eval_debug(toks[c:c + 16], c, n_threads=8)["logits_all"] for c in range(0, 70, 16)])
        check_scores(got, rows, next_targets(toks))
        assert same(got["logits"], m.eval_chunks(toks, 0, chunk_tokens=16, n_threads=8))


def test_pipeline_handles_are_bit_identical(L, tmp_path, ragged):
    dense = write_dense(L, tmp_path, "f16")
    for path, chunk in ((ragged, 0), (dense, 16)):
        hp_v = RAGGED.n_vocab if path == ragged else DENSE.n_vocab
        toks = synth.synth_prompt(100, hp_v, seed=111)
        stream = synth.synth_prompt(2 * 48 + 5, hp_v, seed=112)
        with L.Model(path, n_ctx=128) as m:
            want = m.eval_logprobs(toks, 0, n_threads=8, chunk_tokens=chunk)
            want_p = m.perplexity(stream, window=48, score_from=0, chunk_tokens=chunk)
        for devs in ([0, 0], [0, 0, 0]):
            with L.Model(path, n_ctx=128, devices=devs) as m:
                got = m.eval_logprobs(toks, 0, n_threads=8, chunk_tokens=chunk)
                got_p = m.perplexity(stream, window=48, score_from=0, chunk_tokens=chunk)
            for k in ("logprob", "argmax", "rank", "logits"):
                assert same(got[k], want[k]), (path, devs, k)
            assert got_p["nll_sum"] == want_p["nll_sum"] and got_p["n_scored"] == want_p["n_scored"]
            assert same(got_p["running"], want_p["running"])


def test_perplexity_windows_against_the_oracle(L, oracle, ragged):
    W = 128
    stream = synth.synth_prompt(3 * W + 57, RAGGED.n_vocab, seed=121)        # 3 windows + a partial tail (unused)
    om = oracle.load(ragged, W)
    rows = [om.eval(stream[k * W:(k + 1) * W - 1], 0, 8, all_logits=True)["logits_all"] for k in range(3)]
    om.close()
    with L.Model(ragged, n_ctx=W) as m:
        for sf in (-1, 0, 100):
            got = m.perplexity(stream, score_from=sf, n_threads=8)
            first = W // 2 if sf == -1 else sf
            nll, n, running = 0.0, 0, []
            for k in range(3):
                win = stream[k * W:(k + 1) * W]
                tgt = np.where(np.arange(W - 1) >= first, win[1:], -1).astype(np.int32)
                lp, _, _ = np_scores(rows[k], tgt)
                nll -= lp[first:].sum()
                n += W - 1 - first
                running.append(math.exp(nll / n))
            assert got["n_scored"] == n
            assert abs(got["nll_sum"] - nll) <= 1e-12 * abs(nll)
            assert np.allclose(got["running"], running, rtol=1e-12, atol=0)
            assert got["ppl"] == got["running"][-1]


def tool_text(n_words, seed):
    vocab = synth.make_vocab(RAGGED.n_vocab)
    rng = np.random.default_rng(seed)
    return "".join(vocab[i].decode() for i in rng.integers(3, RAGGED.n_vocab, size=n_words))


def run_tool(args, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=timeout, env=e)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    f = lines[-1].split()
    assert f[0] == "ppl" and f[2] == "n_scored" and f[4] == "windows" and f[6] == "ms"
    return float(f[1]), int(f[3]), int(f[5]), lines[0]


def test_tool_matches_the_python_api(L, ragged):
    text = tool_text(300, 131)
    with L.Model(ragged, n_ctx=64) as m:
        toks = m.tokenize(text, bos=True)
        want = m.perplexity(toks, n_threads=8)
    ppl, n, k, running = run_tool([ragged, "--prompt", text, "--ctx", "64", "--threads", "8"])
    assert ppl == want["ppl"] and n == want["n_scored"] and k == toks.size // 64 >= 3
    assert running.startswith("[1]") and f"[{k}]" in running
    ppl2, _, _, _ = run_tool([ragged, "--prompt", text, "--ctx", "64", "--threads", "8"], env={"LLAMAHIP_DEVICES": "0,0"})
    assert ppl2 == ppl


def test_tool_fast_prefill_gives_a_finite_perplexity(L, ragged, tmp_path):
    f = tmp_path / "text.txt"
    f.write_text(tool_text(700, 141))
    ppl, n, k, _ = run_tool([ragged, "--file", str(f), "--ctx", "128", "--fast-prefill"])
    assert math.isfinite(ppl) and ppl > 0 and n > 0 and k >= 2
    # ... and it is the library's FAST handle over the same windows, bit for bit (%.17g prints every bit of a double)
    with L.Model(ragged, n_ctx=128, flags=FAST_PREFILL) as m:
        want = m.perplexity(m.tokenize(f.read_text(), bos=True), n_threads=8)
    assert ppl == want["ppl"] and n == want["n_scored"], (ppl, want["ppl"], n, want["n_scored"])
