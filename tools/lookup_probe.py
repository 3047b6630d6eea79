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

  multi    (--multi: drafted greedy decoding for several sequences at once, llamahip_verify_greedy_multi / llamahip_decode_greedy_lookup_multi,
           one process) for 2 / 4 / 8 sequences: ms per step of llamahip_decode_greedy_multi (a captured set step, one row per sequence)
           against ms per llamahip_verify_greedy_multi call filled to 16 rows at the three positions (wrong drafts), and the loop's aggregate
           tokens/s with the true streams as corpus (every draft accepted) and with a drafter that never hits (set steps + one host wait
           each), next to llamahip_decode_greedy_multi of the same run for the same sequences.  --parent-lib NAME measures
           llamahip_decode_greedy_multi of a second library file in csrc/ (a build of the parent commit) the same way, in its own process

  multi sampled  (--multi --sampled: the drafted SAMPLED loop for several sequences, llamahip_verify_sample_multi /
           llamahip_decode_sample_lookup_multi, one process) for 2 / 4 / 8 sequences: llamahip_decode_sample_multi's aggregate tokens/s and ms per
           step, ms per llamahip_verify_sample_multi call filled to 16 rows at the three positions next to llamahip_verify_greedy_multi calls of
           the same rows (wrong drafts), and the loop's aggregate tokens/s with the true streams as corpus (every draft accepted) and with a
           drafter that never hits, all next to llamahip_decode_sample_multi of the same run for the same sequences and samplers

    python tools/lookup_probe.py [--out profiles/lookup_probe_7b.json] [--parent-lib libllamahip_parent.so] [--reps 20]
    python tools/lookup_probe.py --sampled [--out profiles/sample_lookup_probe_7b.json]
    python tools/lookup_probe.py --multi [--out profiles/lookup_multi_probe_7b.json] [--parent-lib libllamahip_parent.so]
    python tools/lookup_probe.py --multi --sampled [--out profiles/sample_lookup_multi_probe_7b.json]
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
    if name == "multi":
        return multi_leg(reps)
    if name == "multi_sampled":
        return multi_sampled_leg(reps)
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


MULTI_SEQS, MULTI_SLOTS = (2, 4, 8), 8


def multi_parent_leg(path, lib_name):
    """llamahip_decode_greedy_multi for 2 / 4 / 8 sequences through bare ctypes calls, so that a library file without the new entry points
    (the parent commit's) runs the same code"""
    import ctypes as C

    import numpy as np

    import synth
    lib = C.CDLL(os.path.join(ROOT, "llama.swift_amd", "csrc", lib_name))
    vp, i32, cp, sz = C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t

    class Opts(C.Structure):          # the head of llamahip_opts: struct_size says how much of it is there
        _fields_ = [("struct_size", i32), ("device", i32), ("layer_begin", i32), ("layer_end", i32), ("n_parts", i32), ("flags", i32), ("n_seq", i32)]
    lib.llamahip_model_load.argtypes = [cp, i32, vp, C.POINTER(vp), cp, sz]
    lib.llamahip_eval.argtypes = [vp, i32, i32, vp, i32, vp, cp, sz]
    lib.llamahip_set_seq.argtypes = [vp, i32, cp, sz]
    lib.llamahip_decode_greedy_multi.argtypes = [vp, i32, i32, vp, vp, i32, vp, cp, sz]
    lib.llamahip_model_free.argtypes = [vp]
    err, h = C.create_string_buffer(1024), vp()
    o = Opts(C.sizeof(Opts), -1, 0, -1, 0, 0, MULTI_SLOTS)
    if lib.llamahip_model_load(path.encode(), N_CTX, C.byref(o), C.byref(h), err, len(err)) != 0:
        raise RuntimeError(err.value.decode())
    logits, firsts = np.empty(32000, np.float32), []
    for i in range(MULTI_SLOTS):
        prompt = synth.synth_prompt(P, 32000, seed=4 + i)
        if lib.llamahip_set_seq(h, i, err, len(err)) != 0 or lib.llamahip_eval(h, NTH, 0, prompt.ctypes.data_as(vp), P, logits.ctypes.data_as(vp), err, len(err)) != 0:
            raise RuntimeError(err.value.decode())
        firsts.append(int(np.argmax(logits)))
    res = {"lib": lib_name}
    for n in MULTI_SEQS:
        ft, npast, out, ts = np.array(firsts[:n], np.int32), np.full(n, P, np.int32), np.empty((n, STEPS), np.int32), []
        for r in range(4):                              # (the first run is the warm-up: graph capture)
            t0 = time.perf_counter()
            if lib.llamahip_decode_greedy_multi(h, NTH, n, npast.ctypes.data_as(vp), ft.ctypes.data_as(vp), STEPS, out.ctypes.data_as(vp), err, len(err)) != 0:
                raise RuntimeError(err.value.decode())
            if r:
                ts.append(time.perf_counter() - t0)
        t = statistics.median(ts)
        res[str(n)] = {"tok_s": round(n * STEPS / t, 1), "ms_per_step": round(1e3 * t / STEPS, 4), "spread_ms_per_step": round(1e3 * (max(ts) - min(ts)) / STEPS, 4)}
    lib.llamahip_model_free(h)
    return res


def multi_leg(reps):
    import numpy as np

    import bench
    import llama_swift_amd as L
    import synth
    path = bench.model_path("7B", bench.MODELS["7B"], 20230312)
    if os.environ.get("LLAMAHIP_LIB"):
        return multi_parent_leg(path, os.environ["LLAMAHIP_LIB"])

    def timed(call, n):
        ts = []
        for r in range(4):                              # (the first run is the warm-up)
            t0 = time.perf_counter()
            ret = call()
            if r:
                ts.append(time.perf_counter() - t0)
        t = statistics.median(ts)
        return ret, {"tok_s": round(n * STEPS / t, 1), "ms_per_token": round(1e3 * t / (n * STEPS), 4), "spread_ms_per_token": round(1e3 * (max(ts) - min(ts)) / (n * STEPS), 4)}

    res = {}
    with L.Model(path, n_ctx=N_CTX, n_seq=MULTI_SLOTS) as m:
        prompts = [synth.synth_prompt(P, m.n_vocab, seed=4 + i) for i in range(MULTI_SLOTS)]
        firsts, S = [], []
        for i in range(MULTI_SLOTS):
            m.set_seq(i)
            firsts.append(int(np.argmax(m.eval(prompts[i], 0, NTH))))
            S.append([firsts[i]] + m.decode_greedy(firsts[i], P, STEPS, NTH).tolist())          # (the slot keeps the true rows)
        m.set_seq(0)
        for n in MULTI_SEQS:
            G = [s[1:] for s in S[:n]]
            npast, r = [P] * n, {}
            out, r["decode_greedy_multi"] = timed(lambda: m.decode_greedy_multi(firsts[:n], npast, STEPS, NTH), n)
            assert out.tolist() == G
            r["set_step_ms"] = round(r["decode_greedy_multi"]["ms_per_token"] * n, 4)
            # a verify step over the set filled to 16 rows: wrong from the first draft token, so rows [pos, ..) stay re-usable
            rows = [16 // n + (1 if i < 16 % n else 0) for i in range(n)]
            tv = {}
            for pos in (64, 256, 448):
                i0 = pos - P
                drafts = [(np.array(S[i][i0 + 1:i0 + rows[i]], np.int32) + 1) % m.n_vocab for i in range(n)]
                call = lambda: m.verify_greedy_multi(range(n), [S[i][i0] for i in range(n)], drafts, [pos] * n, NTH)
                call()
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    call()
                    ts.append(1e3 * (time.perf_counter() - t0))
                tv[str(pos)] = round(statistics.median(ts), 4)
                for i in range(n):                                                            # the true rows back
                    m.set_seq(i)
                    m.decode_greedy(S[i][i0], pos, STEPS - i0, NTH)
            m.set_seq(0)
            r["rows_per_sequence"], r["verify_set_step_16_rows_ms"] = rows, tv
            r["verify_set_over_set_step"] = round(statistics.mean(tv.values()) / r["set_step_ms"], 4)
            (out, st), r["loop_all_accepted"] = timed(lambda: m.decode_greedy_lookup_multi(firsts[:n], npast, STEPS, prompts[:n], corpus=np.concatenate([np.array(g, np.int32) for g in G]),
                                                                                           n_threads=NTH), n)
            assert out.tolist() == G
            r["loop_all_accepted"]["stats"] = st
            (out, st), r["loop_nothing_drafted"] = timed(lambda: m.decode_greedy_lookup_multi(firsts[:n], npast, STEPS, prompts[:n], ngram_min=4 * N_CTX, ngram_max=4 * N_CTX,
                                                                                              n_threads=NTH), n)
            assert out.tolist() == G and all(x["n_verify_steps"] == 0 for x in st)
            base = r["decode_greedy_multi"]["tok_s"]
            r["loop_all_accepted"]["vs_decode_greedy_multi"] = round(r["loop_all_accepted"]["tok_s"] / base, 4)
            r["loop_nothing_drafted"]["vs_decode_greedy_multi"] = round(r["loop_nothing_drafted"]["tok_s"] / base, 4)
            r["loop_nothing_drafted"]["slower_than_decode_greedy_multi"] = r["loop_nothing_drafted"]["tok_s"] < base      # (it pays one host wait per step)
            res[str(n)] = r
    return {"sequences": res}


def multi_sampled_leg(reps):
    import numpy as np

    import bench
    import llama_swift_amd as L
    import synth
    path = bench.model_path("7B", bench.MODELS["7B"], 20230312)
    seed = 20230312

    def timed(prep, call, n):
        """4 runs (the first is the warm-up), each on what prep() returns: fresh samplers are made outside the timed region"""
        ts = []
        for r in range(4):
            arg = prep()
            t0 = time.perf_counter()
            ret = call(arg)
            if r:
                ts.append(time.perf_counter() - t0)
        t = statistics.median(ts)
        return ret, {"tok_s": round(n * STEPS / t, 1), "ms_per_token": round(1e3 * t / (n * STEPS), 4), "spread_ms_per_token": round(1e3 * (max(ts) - min(ts)) / (n * STEPS), 4)}

    res = {}
    with L.Model(path, n_ctx=N_CTX, n_seq=MULTI_SLOTS) as m:
        prompts = [synth.synth_prompt(P, m.n_vocab, seed=4 + i) for i in range(MULTI_SLOTS)]
        plg = []
        for i in range(MULTI_SLOTS):
            m.set_seq(i)
            plg.append(m.eval(prompts[i], 0, NTH))
        m.set_seq(0)

        def fresh(n):
            """sampler i: seed + i, the prompt and the first token (drawn from the prompt's logits) accepted"""
            smp, firsts = [], []
            for i in range(n):
                s = L.Sampler(seed=seed + i, repeat_last_n=64)
                for t in prompts[i]:
                    s.accept(int(t))
                firsts.append(s.sample(m, plg[i]))
                s.accept(firsts[-1])
                smp.append(s)
            return smp, firsts

        for n in MULTI_SEQS:
            npast, r = [P] * n, {}
            firsts = fresh(n)[1]
            plain = lambda smp: m.decode_sample_multi(firsts, npast, STEPS, smp[0], n_threads=NTH)
            out, r["decode_sample_multi"] = timed(lambda: fresh(n), plain, n)
            G = out.tolist()
            S = [[firsts[i]] + G[i] for i in range(n)]
            r["set_step_ms"] = round(r["decode_sample_multi"]["ms_per_token"] * n, 4)
            # a verify step over the set filled to 16 rows, sampled next to greedy: wrong from the first draft token
            rows = [16 // n + (1 if i < 16 % n else 0) for i in range(n)]
            tv = {"sample": {}, "greedy": {}}
            smp = [L.Sampler(seed=seed + i, repeat_last_n=64) for i in range(n)]
            for pos in (64, 256, 448):
                i0 = pos - P
                drafts = [(np.array(S[i][i0 + 1:i0 + rows[i]], np.int32) + 1) % m.n_vocab for i in range(n)]
                toks = [S[i][i0] for i in range(n)]
                for kind, call in (("sample", lambda: m.verify_sample_multi(range(n), toks, drafts, [pos] * n, smp, n_threads=NTH)),
                                   ("greedy", lambda: m.verify_greedy_multi(range(n), toks, drafts, [pos] * n, NTH))):
                    call()
                    ts = []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        call()
                        ts.append(1e3 * (time.perf_counter() - t0))
                    tv[kind][str(pos)] = round(statistics.median(ts), 4)
                plain(fresh(n))                                                                # the true rows back
            r["rows_per_sequence"] = rows
            r["verify_sample_set_step_16_rows_ms"], r["verify_greedy_set_step_16_rows_ms"] = tv["sample"], tv["greedy"]
            r["verify_sample_set_over_set_step"] = round(statistics.mean(tv["sample"].values()) / r["set_step_ms"], 4)
            corpus = np.concatenate([np.array(g, np.int32) for g in G])
            (out, st), r["loop_all_accepted"] = timed(lambda: fresh(n), lambda a: m.decode_sample_lookup_multi(firsts, npast, STEPS, prompts[:n], a[0], corpus=corpus, n_threads=NTH), n)
            assert out.tolist() == G
            r["loop_all_accepted"]["stats"] = st
            (out, st), r["loop_nothing_drafted"] = timed(lambda: fresh(n), lambda a: m.decode_sample_lookup_multi(firsts, npast, STEPS, prompts[:n], a[0], ngram_min=4 * N_CTX,
                                                                                                                  ngram_max=4 * N_CTX, n_threads=NTH), n)
            assert out.tolist() == G and all(x["n_verify_steps"] == 0 for x in st)
            base = r["decode_sample_multi"]["tok_s"]
            r["loop_all_accepted"]["vs_decode_sample_multi"] = round(r["loop_all_accepted"]["tok_s"] / base, 4)
            r["loop_nothing_drafted"]["vs_decode_sample_multi"] = round(r["loop_nothing_drafted"]["tok_s"] / base, 4)
            res[str(n)] = r
    return {"sequences": res}


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
    ap.add_argument("--multi", action="store_true", help="the multi-sequence drafted loop's leg alone (default --out profiles/lookup_multi_probe_7b.json)")
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(leg(a.leg, a.reps)))
        return
    if a.multi and a.sampled:
        res = {"model": "synthetic LLaMA-7B Q4_0, 32 layers", "n_ctx": N_CTX, "positions": [P, P + STEPS], "n_threads": NTH, "kv_slots": MULTI_SLOTS,
               "sampler": "repeat_penalty 1.3, top_k 40, top_p 0.95, temp 0.8, repeat_last_n 64, seed 20230312 + sequence"}
        res.update(child("multi_sampled", a.reps))
        text = json.dumps(res, indent=1)
        print(text)
        with open(a.out or os.path.join(ROOT, "profiles", "sample_lookup_multi_probe_7b.json"), "w") as f:
            f.write(text + "\n")
        return
    if a.multi:
        res = {"model": "synthetic LLaMA-7B Q4_0, 32 layers", "n_ctx": N_CTX, "positions": [P, P + STEPS], "n_threads": NTH, "kv_slots": MULTI_SLOTS}
        res.update(child("multi", a.reps))
        if a.parent_lib:
            res["parent_decode_greedy_multi"] = child("multi", a.reps, a.parent_lib)
        text = json.dumps(res, indent=1)
        print(text)
        with open(a.out or os.path.join(ROOT, "profiles", "lookup_multi_probe_7b.json"), "w") as f:
            f.write(text + "\n")
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
