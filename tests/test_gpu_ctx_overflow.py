"""GPU (-m gpu): generating past the context window (llamahip_decode_greedy_window, the runner's overflow mode).

REEVAL is defined purely by llama_eval calls -- single-token steps, and at the wall the surviving tail fed again at n_past = n_keep -- so the
oracle making the same calls is the bit-for-bit yardstick: tokens, last logits, KV rows.  n_ctx 48 throughout: 130 steps cross the wall five times."""
import os
import subprocess

import numpy as np
import pytest

import refgolden
import synth
from conftest import synth_tool

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REFQ = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "quantize")
STORE = os.path.join(HERE, "golden", "ref_outputs_ctx_overflow.npz")      # the reference's outputs for the f16 / Q4_1 files (oracle.c reads Q4_0 only)

SMALL = dict(n_vocab=2000, n_embd=512, n_mult=256, n_head=4, n_layer=3)
W7B = dict(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=2)
SHAPES = {"small": SMALL, "7b_width": W7B}
DENSE_HP = synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=4, n_layer=2)
NO_GRAPH = 1
N_CTX, N_PROMPT, N_STEPS = 48, 20, 130
# (shape, n_keep, chunk_tokens, n_threads): both n_keep, both chunkings, the three thread counts; the oracle's 7B-width evals take 15 .. 60 ms
# a token on the CPU, so that shape runs at 8 and 3 threads
REEVAL_CASES = [("small", 0, 0, 1), ("small", 6, 9, 3), ("small", 6, 0, 8), ("small", 0, 9, 8), ("7b_width", 6, 9, 8), ("7b_width", 0, 0, 3)]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def plan(n_past, n_keep):
    nd = (n_past - n_keep) // 2
    assert nd >= 1
    return nd


def eval_loop_with_reeval(om, prompt, n_steps, n_keep, chunk, nth, n_ctx=N_CTX):
    """the yardstick: `om` (oracle / reference model: eval -> {"logits"}) evaluates the prompt, then single-token greedy steps; when the
    pending token has no room the tail is evaluated again at n_keep in chunks of `chunk` tokens (0: one eval)"""
    lg = om.eval(prompt, 0, nth)["logits"]
    toks, pos, pending, out = [int(t) for t in prompt], len(prompt), int(np.argmax(lg)), []
    first = pending
    while len(out) < n_steps:
        if pos == n_ctx:
            nd = plan(pos, n_keep)
            tail = toks[n_keep + nd:]
            c = chunk if chunk > 0 else len(tail)
            for c0 in range(0, len(tail), c):
                om.eval(np.array(tail[c0:c0 + c], np.int32), n_keep + c0, nth)
            toks, pos = toks[:n_keep] + tail, pos - nd
        lg = om.eval(np.array([pending], np.int32), pos, nth)["logits"]
        toks.append(pending)
        pos += 1
        pending = int(np.argmax(lg))
        out.append(pending)
    return first, np.array(out, np.int32), lg, pos


def check_reeval(h, om_result, kv_of, n_layer, prompt, n_keep, chunk, nth, note):
    first, want, want_lg, want_pos = om_result
    lg = h.eval(prompt, 0, nth)
    assert int(np.argmax(lg)) == first, note
    got, pos, got_lg = h.decode_greedy_window(first, N_STEPS, len(prompt), prompt, n_keep=n_keep, mode=1, chunk_tokens=chunk, n_threads=nth, want_logits=True)
    assert got.tolist() == want.tolist(), (note, "tokens")
    assert pos == want_pos and same(got_lg, want_lg), (note, "n_past_out / last logits")
    for il in range(n_layer):
        k, v = h.kv(il, pos)
        wk, wv = kv_of(il, pos)
        assert same(k, wk) and same(v, wv), (note, f"KV rows of layer {il}")


# ------------------------------------------------------------------------------------------------ 1. the greedy loop against the oracle
@pytest.mark.parametrize("shape,n_keep,chunk,nth", REEVAL_CASES)
def test_reeval_window_is_the_oracles_eval_sequence(L, oracle, tmp_path, shape, n_keep, chunk, nth):
    """130 steps from a 20-token context at n_ctx 48 on a plain, a NO_GRAPH and a two-stage in-process pipeline handle: tokens, last logits
    and KV rows [0, n_past_out) of every layer are the oracle's after the same sequence of evals"""
    kw = SHAPES[shape]
    path = synth_tool(tmp_path / "m.bin", seed=91, **kw)
    prompt = synth.synth_prompt(N_PROMPT, kw["n_vocab"], seed=5)
    om = oracle.load(path, n_ctx=N_CTX)
    res = eval_loop_with_reeval(om, prompt, N_STEPS, n_keep, chunk, nth)
    assert res[3] < N_CTX + 1 and N_STEPS > 2 * N_CTX          # (the run crossed the wall several times)
    for note, opts in (("plain", {}), ("no_graph", dict(flags=NO_GRAPH)), ("pipeline", dict(devices=[0, 0]))):
        with L.Model(path, n_ctx=N_CTX, **opts) as h:
            check_reeval(h, res, om.kv, kw["n_layer"], prompt, n_keep, chunk, nth, (shape, n_keep, chunk, nth, note))
    om.close()


def _dense_file(tmp, ftype, quantize):
    path = os.path.join(str(tmp), f"ctx_{ftype}.bin")
    src = path + ".f16" if ftype == "q41" else path
    synth.write_model_unquantized(src, DENSE_HP, synth.random_tensors(DENSE_HP, seed=1701), 1)
    if ftype == "q41":
        quantize(src, path)
        os.remove(src)
    return path


@refgolden.computed_by("gpu_ctx_overflow.dense_reeval", [("f16",), ("q41",)], store=STORE)
def _ref_dense_reeval(ref, tmp, ftype):
    path = _dense_file(tmp, ftype, lambda s, t: subprocess.run([REFQ, s, t, "3"], check=True, stdout=subprocess.DEVNULL))
    rm = ref.load(path, N_CTX)
    first, toks, lg, pos = eval_loop_with_reeval(rm, synth.synth_prompt(N_PROMPT, DENSE_HP.n_vocab, seed=5), N_STEPS, 6, 9, 8)
    out = {"first": np.int32(first), "tokens": toks, "last_logits": lg, "n_past": np.int32(pos)}
    for il in range(DENSE_HP.n_layer):
        k, v = rm.kv(il, pos)
        out[f"k{il}"], out[f"v{il}"] = refgolden.digest(k), refgolden.digest(v)
    rm.close()
    return out


@pytest.mark.parametrize("ftype", ["f16", "q41"])
def test_reeval_window_on_f16_and_q4_1_files(L, ref, tmp_path, ftype):
    """the same on an f16 and a Q4_1 file (n_keep 6, chunks of 9, 8 threads) against the reference build's own evals (stored with the tests)"""
    want = refgolden.outputs("gpu_ctx_overflow.dense_reeval", ref, tmp_path, ftype)
    path = _dense_file(tmp_path, ftype, lambda s, t: L.quantize_file(s, t, 3))
    prompt = synth.synth_prompt(N_PROMPT, DENSE_HP.n_vocab, seed=5)
    with L.Model(path, n_ctx=N_CTX) as h:
        first = int(np.argmax(h.eval(prompt, 0, 8)))
        assert first == int(want["first"])
        got, pos, lg = h.decode_greedy_window(first, N_STEPS, N_PROMPT, prompt, n_keep=6, mode=L.CTX_REEVAL, chunk_tokens=9, n_threads=8, want_logits=True)
        assert got.tolist() == want["tokens"].tolist() and pos == int(want["n_past"]) and same(lg, want["last_logits"]), ftype
        for il in range(DENSE_HP.n_layer):
            k, v = h.kv(il, pos)
            assert same(refgolden.digest(k), want[f"k{il}"]) and same(refgolden.digest(v), want[f"v{il}"]), (ftype, f"KV rows of layer {il}")


def test_window_starting_at_the_wall_and_a_single_step(L, tmp_path):
    """n_past == n_ctx on entry applies the plan first; one step at the wall"""
    path = synth_tool(tmp_path / "m.bin", seed=93, **SMALL)
    prompt = synth.synth_prompt(N_CTX, SMALL["n_vocab"], seed=11)
    with L.Model(path, n_ctx=N_CTX) as h:
        first = int(np.argmax(h.eval(prompt, 0, 8)))
        got, pos = h.decode_greedy_window(first, 1, N_CTX, prompt, n_keep=4, mode=L.CTX_REEVAL, chunk_tokens=9)
        assert got.size == 1 and pos == N_CTX - 22 + 1
        with pytest.raises(L.LlamaHipError):          # the plain loop still refuses the wall
            h.decode_greedy(first, N_CTX, 1)


# ------------------------------------------------------------------------------------------------ 2. the runner
def runner_tokens(L, path, prompt_text, n_tokens, overflow=None, lookup=None, greedy=False, seed=11, n_keep=-1):
    r = L.LlamaRunner(path)
    if overflow is not None:
        r.set_overflow(overflow, n_keep)
    if lookup is not None:
        r.set_lookup(lookup)
    try:
        return r.run(prompt_text, L.Config(numThreads=8, numTokens=n_tokens, n_ctx=N_CTX, greedy=greedy, seed=seed))
    finally:
        r.close()


def binding_loop(L, h, prompt_ids, n_tokens, greedy, seed, n_keep=-1):
    """the generation loop over the binding: eval_topk -> draw -> accept (greedy: eval -> argmax); at the wall the plan, then the
    tail again through eval_chunks in the runner's chunks of 9.  Returns the generated ids."""
    s = L.Sampler(seed, 64)
    P = len(prompt_ids)
    keep = min(P if n_keep < 0 else n_keep, N_CTX // 2)
    h.eval(np.array([0, 1, 2, 3], np.int32), 0, 8)
    for t in prompt_ids:
        s.accept(int(t))
    n_full = ((P - 1) // 9) * 9 if P > 9 else 0
    if n_full:
        h.eval_chunks(prompt_ids[:n_full], 0, 9, 8)
    toks, pos, pending, out = [int(t) for t in prompt_ids[:n_full]], n_full, np.asarray(prompt_ids[n_full:], np.int32), []
    while True:
        if pos + len(pending) > N_CTX:
            assert len(pending) == 1 and pos == N_CTX
            new, nd = L.ctx_overflow_plan(N_CTX, pos, keep)
            h.eval_chunks(np.array(toks[keep + nd:], np.int32), keep, 9, 8)
            toks, pos = toks[:keep] + toks[keep + nd:], new
        if greedy:
            tid = int(np.argmax(h.eval(pending, pos, 8)))
        else:
            exact, sc, ids, lg = h.eval_topk(pending, pos, s)
            tid = s.sample_from_candidates(sc, ids) if exact else s.sample(h, lg)
        toks += [int(t) for t in pending]
        pos += len(pending)
        s.accept(tid)
        out.append(tid)
        if len(out) == n_tokens:
            return out
        pending = np.array([tid], np.int32)


@pytest.fixture(scope="module")
def runner_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctx_runner")
    return synth_tool(d / "m.bin", seed=94, **SMALL)


def _prompt_text(h, V):
    ids = synth.synth_prompt(14, V, seed=21)[1:]
    text = b"".join(h.token_text(int(t)) for t in ids).decode(errors="ignore")
    return text, h.tokenize(text)


def test_runner_overflow_is_the_binding_loop(L, oracle, runner_model):
    """numberOfTokens 120 at n_ctx 48: the OUTPUT_TOKEN events are the prompt's tokens and then the ids of the Python loop over the binding on a
    second handle with the same seed; with lookup on the stream is the same; greedy runs are also the oracle's eval sequence"""
    with L.Model(runner_model, n_ctx=N_CTX) as h:
        text, ids = _prompt_text(h, SMALL["n_vocab"])
        P = len(ids)
        assert 2 <= P < N_CTX // 2
        for greedy in (False, True):
            want_ids = binding_loop(L, h, ids, 120, greedy, seed=11)
            want = [h.token_text(int(t)) for t in ids] + [h.token_text(t) for t in want_ids]
            got = runner_tokens(L, runner_model, text, 120, overflow=1, greedy=greedy)
            assert len(got) == P + 120 and got == want, greedy
            if not greedy:
                assert runner_tokens(L, runner_model, text, 120, overflow=1, lookup=4) == want, "lookup on"
            else:
                # the oracle: warm-up, the prompt in the runner's chunks, then the yardstick loop with n_keep = the prompt's length
                om = oracle.load(runner_model, n_ctx=N_CTX)
                om.eval(np.array([0, 1, 2, 3], np.int32), 0, 8)
                toks, pos = [int(t) for t in ids], 0
                n_full = ((P - 1) // 9) * 9 if P > 9 else 0
                for c0 in range(0, n_full, 9):
                    om.eval(ids[c0:c0 + 9], c0, 8)
                pending, pos, toks, out = ids[n_full:], n_full, toks[:n_full], []
                while len(out) < 120:
                    if pos + len(pending) > N_CTX:
                        nd = plan(pos, P)
                        tail = toks[P + nd:]
                        for c0 in range(0, len(tail), 9):
                            om.eval(np.array(tail[c0:c0 + 9], np.int32), P + c0, 8)
                        toks, pos = toks[:P] + tail, pos - nd
                    lg = om.eval(np.asarray(pending, np.int32), pos, 8)["logits"]
                    toks += [int(t) for t in pending]
                    pos += len(pending)
                    out.append(int(np.argmax(lg)))
                    pending = [out[-1]]
                om.close()
                assert out == want_ids, "greedy re-evaluation against the oracle"


def test_runner_without_a_mode_stops_at_the_wall(L, runner_model, monkeypatch):
    monkeypatch.delenv("LLAMAHIP_RUNNER_OVERFLOW", raising=False)
    with L.Model(runner_model, n_ctx=N_CTX) as h:
        text, ids = _prompt_text(h, SMALL["n_vocab"])
    for overflow in (None, 0):
        got = runner_tokens(L, runner_model, text, 120, overflow=overflow)
        assert len(got) == len(ids) + (N_CTX - len(ids)), overflow          # the prompt echoed, then n_ctx - n_inp tokens (.mm:812)
    past = runner_tokens(L, runner_model, text, 120, overflow=1)
    assert len(past) == len(ids) + 120 and got == past[:len(got)]          # the same stream up to the wall
    assert runner_tokens(L, runner_model, text, 120, overflow=2) == got          # a mode the runner does not have is mode 0
    # a bridge that never calls the setter takes the mode from the environment; the setter's 0 wins over it
    monkeypatch.setenv("LLAMAHIP_RUNNER_OVERFLOW", "reeval")
    assert runner_tokens(L, runner_model, text, 120) == past
    assert runner_tokens(L, runner_model, text, 120, overflow=0) == got
