"""The layer pipeline behind the reference's own surface (VERDICT r05 missing #3): ONE llamahip_model_load with a device
list (llamahip_opts.n_devices / LLAMAHIP_DEVICES) builds one stage handle per entry in ONE process, and llamahip_eval /
llamahip_eval_chunks / llamahip_decode_greedy / llamahip_eval_topk / the llama_runner_* driver walk the stages with stream-ordered peer
copies -- no Python, no torch.distributed.  Tested here on one GPU with every stage on device 0 (the copies are device copies, the
streams, events and stage launches are the multi-GPU ones) against the oracle: logits, greedy tokens, KV rows, the runner's events."""
import os
import subprocess
import sys

import numpy as np
import pytest

import refgolden
import synth
from conftest import synth_tool
from test_gpu_dense import STORE as DENSE_STORE, file_sha256, ref_quantize, write_model

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------------------------- host only
def test_device_list_validation_happens_before_any_device_work(L, tmp_path):
    """option errors of the pipeline handle are load failures (-1000) with a message, on a box without a GPU too"""
    hp = synth.HParams(n_vocab=64, n_embd=64, n_mult=32, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    with pytest.raises(L.LlamaHipError, match="layer range") as e:
        L.Model(path, n_ctx=32, devices=[0, 0], layer_begin=1, layer_end=2)
    assert e.value.code == -1000
    with pytest.raises(L.LlamaHipError, match="HOST_ONLY"):
        L.Model(path, n_ctx=32, devices=[0, 0], flags=4)
    with pytest.raises(L.LlamaHipError, match="3 pipeline stages for a model of 2 layers|no HIP device"):
        L.Model(path, n_ctx=32, devices=[0, 0, 0])
    with pytest.raises(L.LlamaHipError, match="negative"):
        L.Model(path, n_ctx=32, devices=[0, -1])
    with pytest.raises(ValueError):
        L.Model(path, n_ctx=32, devices=list(range(9)))
    # a missing file is the reader's own error (.mm:101-102), whatever the device list
    with pytest.raises(L.LlamaHipError, match="failed to open"):
        L.Model(str(tmp_path / "nope.bin"), n_ctx=32, devices=[0, 0])


def test_llamahip_devices_environment_is_parsed_and_never_applies_to_explicit_handles(tmp_path):
    """LLAMAHIP_DEVICES (what a caller that passes no options -- the replacement bridge -- uses): a bad value is a load error; a host-only
    handle or one with an explicit device / layer range ignores it"""
    hp = synth.HParams(n_vocab=64, n_embd=64, n_mult=32, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    code = ("import sys, llama_swift_amd as L\n"
            "try:\n"
            "    L.lib().llamahip_model_load  # noqa\n"
            "    import ctypes as C\n"
            "    h = C.c_void_p(); err = C.create_string_buffer(512)\n"
            "    rc = L.lib().llamahip_model_load(sys.argv[1].encode(), 32, None, C.byref(h), err, 512)\n"
            "    print('RC', rc, err.value.decode())\n"
            "    with L.Model(sys.argv[1], n_ctx=32, flags=4) as m: print('HOSTONLY', m.n_layer)\n"
            "except Exception as e:\n"
            "    print('EXC', type(e).__name__, e)\n")
    for env, want in (("0,x", "RC -1000 LLAMAHIP_DEVICES='0,x'"), ("0,1,2,3,4,5,6,7,8", "at most 8 pipeline stages"), ("0,0,0", "RC -1000")):
        r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, LLAMAHIP_DEVICES=env, PYTHONPATH=ROOT), capture_output=True, text=True, cwd=ROOT)
        assert want in r.stdout and "HOSTONLY 2" in r.stdout, (env, r.stdout, r.stderr[-800:])


# ---------------------------------------------------------------------------------------------- GPU
_SHAPES = {
    "small_3_stages": (dict(n_vocab=160, n_embd=512, n_mult=256, n_head=4, n_layer=5), [0, 0, 0], 8),            # uneven split 2 + 2 + 1
    "65b_width_2_stages": (dict(n_vocab=512, n_embd=8192, n_mult=256, n_head=64, n_layer=2, parts=8), [0, 0], 8),
    "65b_width_4_stages": (dict(n_vocab=512, n_embd=8192, n_mult=256, n_head=64, n_layer=4, parts=8), [0, 0, 0, 0], 5),
    "13b_width_2_stages": (dict(n_vocab=512, n_embd=5120, n_mult=256, n_head=40, n_layer=3, parts=2), [0, 0], 3),
    "7b_width_2_stages": (dict(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=3), [0, 0], 8),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(_SHAPES))
def test_pipeline_handle_equals_the_oracle(L, oracle, tmp_path, shape):
    """One handle, N stages: the bridge's flow -- 4-token warm-up eval, the prompt in nine-token evals (llamahip_eval_chunks and eval by
    eval), greedy tokens one llamahip_eval each and on the device-resident loop (llamahip_decode_greedy) -- against the oracle's
    llama_eval: logits bit for bit, tokens, and the KV rows of every layer (each read from the stage that owns the layer)."""
    kw, devices, nth = _SHAPES[shape]
    hp = synth.HParams(**{k: v for k, v in kw.items() if k != "parts"})
    path = synth_tool(tmp_path / "m.bin", seed=41, **kw)
    n_ctx = 96
    om = oracle.load(path, n_ctx)
    prompt = synth.synth_prompt(23, hp.n_vocab, seed=8)
    with L.Model(path, n_ctx=n_ctx, devices=devices) as pm:
        assert (pm.n_layer, pm.n_embd, pm.n_vocab) == (hp.n_layer, hp.n_embd, hp.n_vocab)
        warm = np.array([0, 1, 2, 3], np.int32)
        assert same(pm.eval(warm, 0, nth), om.eval(warm, 0, nth)["logits"])
        # the prompt eval by eval (9 + 9 + 5 rows: the few-row kernels on every stage) ...
        for c0 in range(0, len(prompt), 9):
            a, b = pm.eval(prompt[c0:c0 + 9], c0, nth), om.eval(prompt[c0:c0 + 9], c0, nth)["logits"]
            assert same(a, b), f"prompt eval at {c0}"
        # ... and again in one pass
        assert same(pm.eval_chunks(prompt, 0, 9, nth), b)
        # greedy: host-driven single-token evals, then the device loop
        t, n_past = int(np.argmax(b)), len(prompt)
        for i in range(4):
            a, b = pm.eval(np.array([t], np.int32), n_past, nth), om.eval(np.array([t], np.int32), n_past, nth)["logits"]
            assert same(a, b), f"single-token eval {i}"
            t = int(np.argmax(b)); n_past += 1
        first, want = t, []
        for i in range(10):
            b = om.eval(np.array([t], np.int32), n_past + i, nth)["logits"]
            t = int(np.argmax(b)); want.append(t)
        got, last = pm.decode_greedy(first, n_past, 10, nth, want_logits=True)
        assert got.tolist() == want and same(last, b), (got.tolist(), want)
        # a second loop continues from the device state the first one left (graphs replayed, same buffers)
        want2, t2 = [], want[-1]
        for i in range(5):
            b = om.eval(np.array([t2], np.int32), n_past + 10 + i, nth)["logits"]
            t2 = int(np.argmax(b)); want2.append(t2)
        got2, last2 = pm.decode_greedy(want[-1], n_past + 10, 5, nth, want_logits=True)
        assert got2.tolist() == want2 and same(last2, b)
        for il in range(hp.n_layer):
            gk, gv = pm.kv(il, n_past + 15)
            ok, ov = om.kv(il, n_past + 15)
            assert same(gk, ok) and same(gv, ov), f"KV cache layer {il}"
        st = pm.stats()
        assert st["weight_bytes_device"] > 0 and st["kv_bytes_device"] == 2 * 4 * hp.n_layer * n_ctx * hp.n_embd and st["n_evals"] >= 10
        assert st["n_stages"] == len(devices) and st["hand_off"] == 1, st
        # what a pipeline handle refuses, and the errors it shares with a plain handle
        with pytest.raises(L.LlamaHipError, match="pipeline handle"):
            pm.eval_stage(0, tokens=warm)
        with pytest.raises(L.LlamaHipError, match="pipeline handle"):
            pm.eval_debug(warm, 0, nth, dump_layer=0)
        with pytest.raises(L.LlamaHipError, match="context overflow") as e:
            pm.eval(warm, n_ctx - 2, nth)
        assert e.value.code == -1001
        with pytest.raises(L.LlamaHipError, match="out of range"):
            pm.eval(np.array([hp.n_vocab], np.int32), 0, nth)
    om.close()


@pytest.mark.gpu
def test_pipeline_handle_equals_the_single_device_handle_on_a_long_prompt(L, tmp_path):
    """70+ row evals take the matrix-core prompt kernels on every stage, and the sampler's device front end falls back to the logits row
    (exact = 0) on a pipeline handle: same bits as the plain handle."""
    kw = dict(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=4)
    path = synth_tool(tmp_path / "m.bin", seed=43, **kw)
    prompt = synth.synth_prompt(150, kw["n_vocab"], seed=9)
    with L.Model(path, n_ctx=256) as one, L.Model(path, n_ctx=256, devices=[0, 0, 0, 0]) as pm:
        a, b = one.eval(prompt, 0, 8), pm.eval(prompt, 0, 8)
        assert same(a, b)
        assert same(one.eval_chunks(prompt, 0, 9, 8), pm.eval_chunks(prompt, 0, 9, 8))
        s = L.Sampler(seed=-1, repeat_last_n=64)
        exact, sc, ids, lg = pm.eval_topk(np.array([5], np.int32), 150, s)
        assert not exact and same(lg, one.eval(np.array([5], np.int32), 150, 8))
        t = int(np.argmax(lg))
        assert one.decode_greedy(t, 151, 12, 8).tolist() == pm.decode_greedy(t, 151, 12, 8).tolist()


@pytest.mark.gpu
def test_fast_prefill_pipeline_handle_equals_the_fast_plain_handle(L, tmp_path):
    """LLAMAHIP_FLAG_FAST_PREFILL is not the reference's arithmetic, but it is deterministic and a stage runs its layers as the plain handle
    does: a FAST pipeline handle gives the FAST plain handle's bits -- a 129-token prompt (wq|wk|wv and w1|w3 on the fast kernel), every
    layer's KV rows, the greedy decode that follows."""
    kw = dict(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=2)
    path = synth_tool(tmp_path / "m.bin", seed=47, **kw)
    prompt = synth.synth_prompt(129, kw["n_vocab"], seed=10)
    with L.Model(path, n_ctx=256, flags=16) as one, L.Model(path, n_ctx=256, flags=16, devices=[0, 0]) as pm:
        p0 = L.gemm_paths()
        a = one.eval(prompt, 0, 8)
        p1 = L.gemm_paths()
        b = pm.eval(prompt, 0, 8)
        p2 = L.gemm_paths()
        assert p1["fast"] - p0["fast"] == 2 * kw["n_layer"] and p2["fast"] - p1["fast"] == 2 * kw["n_layer"], (p0, p1, p2)
        assert same(a, b)
        for il in range(kw["n_layer"]):
            (k1, v1), (k2, v2) = one.kv(il, 129), pm.kv(il, 129)
            assert same(k1, k2) and same(v1, v2), f"KV rows of layer {il}"
        t = int(np.argmax(a))
        ta, la = one.decode_greedy(t, 129, 12, 8, want_logits=True)
        tb, lb = pm.decode_greedy(t, 129, 12, 8, want_logits=True)
        assert ta.tolist() == tb.tolist() and same(la, lb)
        for il in range(kw["n_layer"]):
            (k1, v1), (k2, v2) = one.kv(il, 141), pm.kv(il, 141)
            assert same(k1, k2) and same(v1, v2), f"KV rows of layer {il} after the decode"


@pytest.mark.gpu
def test_runner_event_stream_through_the_pipeline_with_no_change_to_the_caller(tmp_path):
    """LLAMAHIP_DEVICES is all a caller that passes no options needs: the llama_runner_* driver (the C mirror of -[LlamaPredictOperation
    main], .mm:768-901) produces the same event stream -- prompt echo, tokens, completion -- through a 2-stage pipeline as through the
    plain handle, greedy and sampled (mt19937(-1); the sampler's host path on the logits row)."""
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=64, n_head=2, n_layer=4)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=21))
    res = _runner_streams(path, ("plain", "pipe", "pipe_count"))
    assert res["plain"]["True"]["states"] == ["notStarted", "initializing", "generatingOutput", "completed"]
    assert res["pipe"] == res["plain"] and res["pipe_count"] == res["plain"]
    assert len(res["plain"]["False"]["toks"]) == len(res["plain"]["True"]["toks"])


def _runner_streams(path, tags):
    """the llama_runner_* event stream of one greedy and one sampled run on `path`, in a fresh process per device setting"""
    code = ("import sys, json, llama_swift_amd as L\n"
            "out = {}\n"
            "for greedy in (True, False):\n"
            "    states, toks = [], []\n"
            "    r = L.LlamaRunner(sys.argv[1]).run('hello world abc tok00050 zz', L.Config(numThreads=8, numTokens=14, greedy=greedy, n_ctx=64), toks.append, lambda s, e: states.append(s.name))\n"
            "    tx = lambda v: [x.decode('latin-1') if isinstance(x, bytes) else x for x in v]\n"
            "    out[str(greedy)] = dict(states=states, toks=tx(toks), ret=tx(r))\n"
            "print('JSON' + json.dumps(out))\n")
    res = {}
    for tag, env in (("plain", {}), ("pipe", {"LLAMAHIP_DEVICES": "0,0"}), ("pipe_count", {"LLAMAHIP_DEVICES": "1"})):
        if tag not in tags:
            continue
        e = dict(os.environ, PYTHONPATH=ROOT, **env)
        e.pop("LLAMAHIP_DEVICES", None) if not env else None
        r = subprocess.run([sys.executable, "-c", code, path], env=e, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert "JSON" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
        import json
        res[tag] = json.loads(r.stdout.split("JSON", 1)[1])
    return res


# f16 / Q4_1 files and LLAMAHIP_FLAG_UNFUSED handles: no fused stage step, so the pipeline handle walks its stages with one eval per token
_DENSE_PIPES = {
    "f16_2_stages": ("odd_widths", "f16", [0, 0], 0),        # 2 + 1 layers; V 250, d 1344, H 21
    "q4_1_3_stages": ("q41_odd", "q41", [0, 0, 0], 0),       # 1 + 1 + 1 layers; V 200, d 320, H 10
    "q4_0_unfused_2_stages": (None, "q4_0", [0, 0], 2),      # LLAMAHIP_FLAG_UNFUSED, against the oracle
}
_DP_CTX, _DP_PROMPT, _DP_GREEDY = 96, 40, 12


def _chunked_flow(rm, prompt, nth=8):
    """what the bridge's flow leaves behind on a CPU model, one eval call at a time: the prompt in 9-token evals (last logits, every layer's
    KV rows), 12 greedy steps (tokens, last logits), one more single-token eval (its logits)"""
    for c0 in range(0, len(prompt), 9):
        lo = rm.eval(prompt[c0:c0 + 9], c0, nth)["logits"]
    out = {"prompt_last": lo}
    for il in range(rm.n_layer):
        k, v = rm.kv(il, len(prompt))
        out[f"k{il}"], out[f"v{il}"] = refgolden.digest(k), refgolden.digest(v)
    toks, n_past = [int(np.argmax(lo))], len(prompt)
    for i in range(_DP_GREEDY):
        lo = rm.eval(np.array([toks[-1]], np.int32), n_past, nth)["logits"]
        toks.append(int(np.argmax(lo))); n_past += 1
    out["greedy_tokens"], out["greedy_last"] = np.array(toks[1:], np.int32), lo
    out["next"] = rm.eval(np.array([toks[-1]], np.int32), n_past, nth)["logits"]
    return out


@refgolden.computed_by("inprocess_pipeline.dense", [("odd_widths", "f16"), ("q41_odd", "q41")], store=DENSE_STORE)
def _ref_dense_pipe(ref, tmp, shape, ftype):
    path = write_model(tmp, shape, ftype, ref_quantize, n_layer=3)
    rm = ref.load(path, _DP_CTX)
    out = _chunked_flow(rm, synth.synth_prompt(_DP_PROMPT, rm.n_vocab, seed=64))
    out["file_sha256"] = file_sha256(path)
    rm.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_DENSE_PIPES))
def test_dense_and_unfused_pipeline_handles_equal_the_plain_handle_and_the_reference(L, oracle, ref, tmp_path, case):
    """f16 / Q4_1 files (against the reference build's stored outputs) and a Q4_0 LLAMAHIP_FLAG_UNFUSED handle (against the oracle), 3 layers
    over 2 or 3 stages, next to a plain handle on the same file: eval_chunks = the reference's 9-token evals (logits, every layer's KV rows);
    decode_greedy (tokens, last logits); eval_topk falls back to the logits row (exact = 0); decode_greedy_multi over 3 slots with their own
    prompt lengths = decode_greedy on each slot alone, on both handles."""
    shape, ftype, devices, flags = _DENSE_PIPES[case]
    if ftype == "q4_0":
        kw = dict(n_vocab=160, n_embd=512, n_mult=256, n_head=4, n_layer=3)
        path = synth_tool(tmp_path / "m.bin", seed=53, **kw)
        om = oracle.load(path, _DP_CTX)
        want = _chunked_flow(om, synth.synth_prompt(_DP_PROMPT, kw["n_vocab"], seed=64))
        om.close()
    else:
        want = refgolden.outputs("inprocess_pipeline.dense", ref, tmp_path, shape, ftype)
        path = write_model(tmp_path, shape, ftype, lambda s, t: L.quantize_file(s, t, 3), n_layer=3)
        assert same(file_sha256(path), want["file_sha256"])
    with L.Model(path, n_ctx=_DP_CTX, flags=flags, n_seq=3) as one, L.Model(path, n_ctx=_DP_CTX, flags=flags, n_seq=3, devices=devices) as pm:
        V = one.n_vocab
        prompt = synth.synth_prompt(_DP_PROMPT, V, seed=64)
        for tag, h in (("plain", one), ("pipeline", pm)):
            lo = h.eval_chunks(prompt, 0, 9, 8)
            assert same(lo, want["prompt_last"]), f"{tag}: eval_chunks logits"
            for il in range(3):
                k, v = h.kv(il, _DP_PROMPT)
                assert same(refgolden.digest(k), want[f"k{il}"]) and same(refgolden.digest(v), want[f"v{il}"]), f"{tag}: KV rows of layer {il}"
            toks, last = h.decode_greedy(int(np.argmax(lo)), _DP_PROMPT, _DP_GREEDY, 8, want_logits=True)
            assert toks.tolist() == want["greedy_tokens"].tolist() and same(last, want["greedy_last"]), f"{tag}: decode_greedy"
            n_past = _DP_PROMPT + _DP_GREEDY
            if h is pm:
                exact, _, _, lg = pm.eval_topk(np.array([toks[-1]], np.int32), n_past, L.Sampler(seed=-1, repeat_last_n=64))
                assert not exact
            else:
                lg = one.eval(np.array([toks[-1]], np.int32), n_past, 8)
            assert same(lg, want["next"]), f"{tag}: eval_topk / eval logits"
        # three slots, three prompt lengths: slot 0 continues behind the eval above
        firsts, n_pasts = [int(np.argmax(lg))], [n_past + 1]
        for i, n in ((1, 13), (2, 22)):
            q = synth.synth_prompt(n, V, seed=65 + n)
            one.set_seq(i), pm.set_seq(i)
            lo = one.eval_chunks(q, 0, 9, 8)
            assert same(pm.eval_chunks(q, 0, 9, 8), lo), f"slot {i}: eval_chunks"
            firsts.append(int(np.argmax(lo))); n_pasts.append(n)
        alone = []
        for i in range(3):
            one.set_seq(i)
            alone.append(one.decode_greedy(firsts[i], n_pasts[i], 10, 8).tolist())
        for tag, h in (("pipeline", pm), ("plain", one)):
            h.set_seq(0)
            assert h.decode_greedy_multi(firsts, n_pasts, 10, 8).tolist() == alone, f"{tag}: decode_greedy_multi"


@pytest.mark.gpu
def test_runner_event_stream_through_a_dense_pipeline(L, tmp_path):
    """the llama_runner_* event stream of an f16 file through LLAMAHIP_DEVICES=0,0 (eval_chunks and decode_greedy of a dense pipeline
    handle) equals the plain handle's, greedy and sampled"""
    path = write_model(tmp_path, "odd_widths", "f16", n_layer=3)
    res = _runner_streams(path, ("plain", "pipe"))
    assert res["plain"]["True"]["states"] == ["notStarted", "initializing", "generatingOutput", "completed"]
    assert res["pipe"] == res["plain"]


_MULTI = {
    "plain_handle_5_sequences": ("small", None, 5, 8),                 # one stage: a single group, picks fed back in place
    "plain_handle_20_sequences": ("small", None, 20, 3),               # ... two groups of 10 stepped one after the other
    "3_stages_7_sequences": ("small", [0, 0, 0], 7, 3),                # groups of 3 + 2 + 2, one per stage
    "2_stages_40_sequences": ("small", [0, 0], 40, 8),                 # more than 16 per stage: three groups of 14 / 13 / 13
    "7b_width_2_stages_16_sequences": ("7b_width", [0, 0], 16, 8),     # two sets of 8: the pipeline bench's default set size
    "65b_width_2_stages_9_sequences": ("65b_width", [0, 0], 9, 5),     # 5 + 4 rows
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_MULTI))
def test_multi_sequence_greedy_decode_equals_one_stream_per_sequence_on_the_oracle(L, oracle, tmp_path, case):
    """llamahip_decode_greedy_multi: the micro-batched pipeline schedule behind the C ABI -- groups of sequences stepped as sets, the groups
    pipelined over the stages of a pipeline handle.  Every sequence (its own prompt length, its own KV slot) must produce bit for bit the
    tokens one llama_eval per token gives it on the oracle, through two consecutive calls (graphs replayed, slots re-bound), and leave the
    oracle's KV rows behind."""
    shape, devices, S, nth = _MULTI[case]
    kw = {"small": dict(n_vocab=160, n_embd=512, n_mult=256, n_head=4, n_layer=5),
          "7b_width": dict(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=2),
          "65b_width": dict(n_vocab=512, n_embd=8192, n_mult=256, n_head=64, n_layer=2, parts=8)}[shape]
    hp = synth.HParams(**{k: v for k, v in kw.items() if k != "parts"})
    path = synth_tool(tmp_path / "m.bin", seed=47, **kw)
    n_ctx, K1, K2 = 64, 7, 5
    prompts = [synth.synth_prompt(3 + (5 * i) % 23, hp.n_vocab, seed=70 + i) for i in range(S)]
    with L.Model(path, n_ctx=n_ctx, devices=devices, n_seq=S) as pm:
        firsts = []
        for i in range(S):
            pm.set_seq(i)
            firsts.append(int(np.argmax(pm.eval(prompts[i], 0, nth))))
        pm.set_seq(0)
        n_past = [len(p) for p in prompts]
        a = pm.decode_greedy_multi(firsts, n_past, K1, nth)
        b = pm.decode_greedy_multi(a[:, -1], [n + K1 for n in n_past], K2, nth)
        got = np.concatenate([a, b[:, :]], axis=1)
        assert got.shape == (S, K1 + K2)
        check = range(S) if S <= 9 else sorted(set([0, 1, S // 2, S - 2, S - 1, 13, 14, 15, 16]) & set(range(S)))      # (every group's edges; all of them when few)
        for i in check:
            om = oracle.load(path, n_ctx)
            lo = om.eval(prompts[i], 0, nth)["logits"]
            t = int(np.argmax(lo))
            assert t == firsts[i]
            want = [t]
            for k in range(K1 + K2):
                lo = om.eval(np.array([want[-1]], np.int32), n_past[i] + k, nth)["logits"]
                want.append(int(np.argmax(lo)))
            # (the second call is fed the first call's last pick at the position behind it: b continues a)
            assert a[i].tolist() == want[1:K1 + 1], f"sequence {i}: {a[i].tolist()} vs {want[1:K1 + 1]}"
            assert b[i].tolist() == want[K1 + 1:K1 + K2 + 1], f"sequence {i}, second call: {b[i].tolist()} vs {want[K1 + 1:]}"
            pm.set_seq(i)
            for il in (0, hp.n_layer - 1):
                gk, gv = pm.kv(il, n_past[i] + K1 + K2)
                ok, ov = om.kv(il, n_past[i] + K1 + K2)
                assert same(gk, ok) and same(gv, ov), f"sequence {i}: KV cache layer {il}"
            om.close()
        with pytest.raises(L.LlamaHipError, match="context overflow"):
            pm.decode_greedy_multi(firsts, [n_ctx - 2] * S, 3, nth)
    with L.Model(path, n_ctx=n_ctx, devices=devices, n_seq=2) as small:
        with pytest.raises(L.LlamaHipError, match="KV slots"):
            small.decode_greedy_multi([1, 2, 3], [0, 0, 0], 2, nth)


@pytest.mark.gpu
def test_pipeline_stage_wait_timeout_is_an_error_not_a_hang(tmp_path):
    """Waiting for a stage of a pipeline handle is bounded (LLAMAHIP_PIPE_WATCHDOG_S, default 600 s): with the bound set to a microsecond a
    600-token eval over four stages cannot have finished at the first look, and the call returns PredictionFailed naming the stage instead
    of blocking (the bound is read once per process: subprocess)."""
    kw = dict(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=4)
    path = synth_tool(tmp_path / "m.bin", seed=43, **kw)
    code = ("import sys, numpy as np, llama_swift_amd as L\n"
            "m = L.Model(sys.argv[1], n_ctx=640, devices=[0, 0, 0, 0])\n"
            "p = (np.arange(600) % 500 + 3).astype(np.int32)\n"
            "try:\n"
            "    m.eval(p, 0, 8); print('NO ERROR')\n"
            "except L.LlamaHipError as e:\n"
            "    print('ERR', e.code, str(e))\n")
    r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, PYTHONPATH=ROOT, LLAMAHIP_PIPE_WATCHDOG_S="0.000001"), capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert "ERR -1001" in r.stdout and "did not finish within" in r.stdout and "pipeline stage" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]

