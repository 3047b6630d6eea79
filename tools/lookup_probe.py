"""What drafted greedy decoding (llamahip_verify_greedy / llamahip_decode_greedy_lookup) costs and where it pays, on the full-depth synthetic
7B Q4_0 file bench.py makes.  Every leg runs in a fresh process (this script re-invoked with --leg), wall-clock around synchronous calls:

  step     ms per token of llamahip_decode_greedy over positions 16 .. 496, 5 repeats after a warm-up run: median and spread (max - min).
           --parent-lib NAME measures a second library file in csrc/ the same way (a build of the parent commit: plain decode is untouched
           if the two medians agree within the spread)
  verify   ms per llamahip_verify_greedy call of N = 1 .. 16 rows at positions 64, 256 and 448 (median of --reps calls; the draft is wrong
           on purpose: the cost of a step does not depend on what is accepted)
  breakeven[N] = (t_verify[N] / t_step - 1) / (N - 1): the share of drafted tokens that must be accepted for N rows to pay
  ceiling  tokens/s of llamahip_decode_greedy_lookup with the true stream as corpus (everything it drafts is accepted)
  floor    ... with a drafter that never hits (n-grams longer than the context: all single steps, one host round trip per token)

  sampled  (--sampled: the drafted SAMPLED loop, llamahip_verify_sample / llamahip_decode_sample_lookup, one process) ms per verify_sample call
           of 2 / 4 / 8 / 16 rows at the three positions next to verify_greedy calls of the same rows in the same run, ms per single
           llamahip_eval_topk step + draw (the loop with a drafter that never hits), breakeven against that step, and the loop's tokens/s
           with the true stream as corpus and with no corpus (drafts from the tokens seen so far only)

    python tools/lookup_probe.py [--out profiles/lookup_probe_7b.json] [--parent-lib libllamahip_parent.so] [--reps 20]
    python tools/lookup_probe.py --sampled [--out profiles/sample_lookup_probe_7b.json]
    python tools/lookup_probe.py --leg ceiling      (one leg in this process: for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_CTX, P, STEPS, NTH = 512, 16, 480, 8


def step_leg(path, lib_name):
    """the step leg through bare ctypes calls, so that a library file without the new entry points (the parent commit's) runs the same code"""
    import ctypes as C

    import numpy as np

    import synth
    lib = C.CDLL(os.path.join(ROOT, "llama.swift_amd", "csrc", lib_name))
    vp, i32, cp, sz = C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t
    lib.llamahip_model_load.argtypes = [cp, i32, vp, C.POINTER(vp), cp, sz]
    lib.llamahip_eval.argtypes = [vp, i32, i32, vp, i32, vp, cp, sz]
    lib.llamahip_decode_greedy.argtypes = [vp, i32, i32, i32, i32, vp, vp, cp, sz]
    lib.llamahip_model_free.argtypes = [vp]
    err, h = C.create_string_buffer(1024), vp()
    if lib.llamahip_model_load(path.encode(), N_CTX, None, C.byref(h), err, len(err)) != 0:
        raise RuntimeError(err.value.decode())
    prompt, logits, out = synth.synth_prompt(P, 32000, seed=4), np.empty(32000, np.float32), np.empty(STEPS, np.int32)
    if lib.llamahip_eval(h, NTH, 0, prompt.ctypes.data_as(vp), P, logits.ctypes.data_as(vp), err, len(err)) != 0:
        raise RuntimeError(err.value.decode())
    first, ts = int(np.argmax(logits)), []
    for r in range(6):                                  # (the first run is the warm-up: graph capture)
        t0 = time.perf_counter()
        if lib.llamahip_decode_greedy(h, NTH, P, first, STEPS, out.ctypes.data_as(vp), None, err, len(err)) != 0:
            raise RuntimeError(err.value.decode())
        if r:
            ts.append(1e3 * (time.perf_counter() - t0) / STEPS)
    lib.llamahip_model_free(h)
    return {"lib": lib_name, "t_step_ms": statistics.median(ts), "spread_ms": max(ts) - min(ts), "runs_ms": ts, "tokens_crc": int(np.bitwise_xor.reduce(out * np.arange(1, STEPS + 1, dtype=np.int32)))}


def leg(name, reps):
    import numpy as np

    import bench
    path = bench.model_path("7B", bench.MODELS["7B"], 20230312)
    if name == "sampled":
        return sampled_leg(reps)
    if name == "step":
        return step_leg(path, os.environ.get("LLAMAHIP_LIB", "libllamahip.so"))
    import llama_swift_amd as L
    import synth
    with L.Model(path, n_ctx=N_CTX) as m:
        prompt = synth.synth_prompt(P, m.n_vocab, seed=4)
        first = int(np.argmax(m.eval(prompt, 0, NTH)))
        if name == "verify":
            G = m.decode_greedy(first, P, STEPS, NTH)
            S = [first] + G.tolist()
            out = {}
            for pos in (64, 256, 448):
                i = pos - P
                for N in range(1, 17):
                    d = (np.array(S[i + 1:i + N], np.int32) + 1) % m.n_vocab          # wrong from the first token: rows [pos, ..) stay re-usable
                    m.verify_greedy(S[i], d, pos, NTH)
                    ts = []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        m.verify_greedy(S[i], d, pos, NTH)
                        ts.append(1e3 * (time.perf_counter() - t0))
                    out.setdefault(str(N), {})[str(pos)] = round(statistics.median(ts), 4)
                m.decode_greedy(S[i], pos, STEPS - i, NTH)                              # the true rows back
            return {"t_verify_ms": out}
        G = m.decode_greedy(first, P, STEPS, NTH)
        kw = dict(corpus=G) if name == "ceiling" else dict(ngram_min=4 * N_CTX, ngram_max=4 * N_CTX)
        out, st = m.decode_greedy_lookup(first, STEPS, P, prompt, n_threads=NTH, **kw)
        assert out.tolist() == G.tolist()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            m.decode_greedy_lookup(first, STEPS, P, prompt, n_threads=NTH, **kw)
            ts.append(time.perf_counter() - t0)
        t = statistics.median(ts)
        return {"tok_s": STEPS / t, "ms_per_token": 1e3 * t / STEPS, "spread_ms_per_token": 1e3 * (max(ts) - min(ts)) / STEPS, "stats": st}


def sampled_leg(reps):
    import numpy as np

    import bench
    import llama_swift_amd as L
    import synth
    path = bench.model_path("7B", bench.MODELS["7B"], 20230312)
    seed = 20230312

    def start(m, prompt, plg):
        s = L.Sampler(seed=seed, repeat_last_n=64)
        for t in prompt:
            s.accept(int(t))
        first = s.sample(m, plg)
        s.accept(first)
        return s, first

    def timed_loop(m, prompt, plg, G, **kw):
        ts, st = [], None
        for r in range(4):                              # (the first run is the warm-up)
            s, first = start(m, prompt, plg)
            t0 = time.perf_counter()
            out, _, st = m.decode_sample_lookup(first, STEPS, P, prompt, s, n_threads=NTH, **kw)
            if r:
                ts.append(time.perf_counter() - t0)
            assert G is None or out.tolist() == G
        t = statistics.median(ts)
        return out.tolist(), {"tok_s": STEPS / t, "ms_per_token": 1e3 * t / STEPS, "spread_ms_per_token": 1e3 * (max(ts) - min(ts)) / STEPS, "stats": st}

    with L.Model(path, n_ctx=N_CTX) as m:
        prompt = synth.synth_prompt(P, m.n_vocab, seed=4)
        plg = m.eval(prompt, 0, NTH)
        G, single = timed_loop(m, prompt, plg, None, ngram_min=4 * N_CTX, ngram_max=4 * N_CTX)      # never drafts: the eval_topk loop itself
        res = {"single": single}
        _, res["ceiling"] = timed_loop(m, prompt, plg, G, corpus=np.array(G, np.int32))
        _, res["no_corpus"] = timed_loop(m, prompt, plg, G)
        # verify steps, sampled next to greedy: wrong from the first draft token, so rows [pos, ..) stay re-usable
        first = start(m, prompt, plg)[1]
        S = [first] + G
        tv = {"sample": {}, "greedy": {}}
        s = L.Sampler(seed=seed, repeat_last_n=64)
        for pos in (64, 256, 448):
            i = pos - P
            for N in (2, 4, 8, 16):
                d = (np.array(S[i + 1:i + N], np.int32) + 1) % m.n_vocab
                for kind, call in (("sample", lambda: m.verify_sample(S[i], d, pos, s, n_threads=NTH)), ("greedy", lambda: m.verify_greedy(S[i], d, pos, NTH))):
                    call()
                    ts = []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        call()
                        ts.append(1e3 * (time.perf_counter() - t0))
                    tv[kind].setdefault(str(N), {})[str(pos)] = round(statistics.median(ts), 4)
        res["t_verify_sample_ms"], res["t_verify_greedy_ms"] = tv["sample"], tv["greedy"]
    t_step = res["single"]["ms_per_token"]
    res["selection_ms"] = {N: round(statistics.mean(tv["sample"][N].values()) - statistics.mean(tv["greedy"][N].values()), 4) for N in tv["sample"]}
    res["breakeven"] = {N: round((statistics.mean(tv["sample"][N].values()) / t_step - 1.0) / (int(N) - 1), 4) for N in tv["sample"]}
    for name in ("ceiling", "no_corpus"):
        res[name]["vs_single"] = round(res[name]["ms_per_token"] / t_step, 4)
    return res


def child(name, reps, lib=None):
    env = dict(os.environ)
    if lib:
        env["LLAMAHIP_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--reps", str(reps)], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"leg {name} failed ({r.returncode}):\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--sampled", action="store_true", help="the drafted sampled loop's leg alone (default --out profiles/sample_lookup_probe_7b.json)")
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.leg, a.reps)))
        return
    if a.sampled:
        res = {"model": "synthetic LLaMA-7B Q4_0, 32 layers", "n_ctx": N_CTX, "positions": [P, P + STEPS], "n_threads": NTH,
               "sampler": "repeat_penalty 1.3, top_k 40, top_p 0.95, temp 0.8, repeat_last_n 64"}
        res.update(child("sampled", a.reps))
        text = json.dumps(res, indent=1)
        print(text)
        with open(a.out or os.path.join(ROOT, "profiles", "sample_lookup_probe_7b.json"), "w") as f:
            f.write(text + "\n")
        return
    res = {"model": "synthetic LLaMA-7B Q4_0, 32 layers", "n_ctx": N_CTX, "positions": [P, P + STEPS], "n_threads": NTH}
    res["step"] = child("step", a.reps)
    if a.parent_lib:
        res["step_parent"] = child("step", a.reps, a.parent_lib)
        res["step_parent"]["agrees_within_spread"] = abs(res["step"]["t_step_ms"] - res["step_parent"]["t_step_ms"]) <= max(res["step"]["spread_ms"], res["step_parent"]["spread_ms"])
    res.update(child("verify", a.reps))
    t_step = res["step"]["t_step_ms"]
    be = {}
    for N in range(2, 17):
        tv = statistics.mean(res["t_verify_ms"][str(N)].values())
        be[str(N)] = round((tv / t_step - 1.0) / (N - 1), 4)
    res["breakeven"] = be
    best = min(be, key=lambda k: be[k])
    res["best_rows"], res["best_draft_len"], res["pays"] = int(best), int(best) - 1, be[best] < 1.0
    for name in ("ceiling", "floor"):
        res[name] = child(name, a.reps)
        res[name]["vs_step"] = round(res[name]["ms_per_token"] / t_step, 4)
    res["floor"]["loss_pct"] = round(100.0 * (res["floor"]["ms_per_token"] / t_step - 1.0), 2)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
