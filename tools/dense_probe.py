#!/usr/bin/env python3
"""Decode / prompt rate of an f16 model file with LLaMA-7B layer shapes (4 layers, so that the numpy writer
finishes in seconds): per-layer time extrapolates to the 32-layer model.
usage: dense_probe.py [n_layer]
       dense_probe.py [n_layer] --multi [--json OUT] [--repeats R] [--seqs 1,2,4,8,16] [--only-multi]
       dense_probe.py [n_layer] --prompt [--json OUT] [--repeats R] [--ftype f16|f32] [--force mm|mfma] [--evals 64,128,512]
                      [--chunks 18,36,72,144,504] [--trace-rows 17,32,64,128,512]
       dense_probe.py [n_layer] --q41 [--json OUT] [--repeats R] [--evals 9,16,17,64,512] [--trace-rows 1,16]
--multi (default 8 layers: 3.2 GB, larger than the Infinity Cache): ms per step and aggregate tokens/s of decode_greedy_multi for S sequences
from position 256 for 64 steps, the 9-token eval, and the single-stream greedy loop; every figure is the wall time of a call that
synchronises before it returns, after one untimed run of the same call (graph captures, first-touch allocations), R repeats each.
--prompt (default 8 layers): ms per call of eval of --evals rows and of eval_chunks(chunk 9) of --chunks tokens, the single-stream greedy loop and
the 16-sequence set step, timed the same way; --force sends every mat-mul of more than 16 rows to one kernel (dense_force).  --trace-rows:
nothing is timed -- per row count one untimed and R further eval_logprobs calls (the lm head over every row too) and exit, for a
rocprofv3 --kernel-trace run that tools/dense_trace_summary.py reads.
--q41 (default 8 layers): the f16 file of --prompt quantized with type 3 (Q4_1, kept next to it); ms per token of the single-stream greedy loop
from position 256 for 64 steps and ms per eval of --evals rows, timed the same way; q41_paths where the library has it.  --trace-rows: nothing
is timed -- per row count one untimed and R further evals (one row: a greedy loop of 1 + R steps, launched eagerly) and exit, for a rocprofv3
--kernel-trace run.  Run it once per library (LLAMAHIP_LIB), fresh processes, alternating.
LLAMAHIP_LIB / LLAMAHIP_DENSE_MM select the library / the mat-mul of 2 .. 16 rows as usual; the model file is kept for the next run."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import synth
import llama_swift_amd as L

args = sys.argv[1:]
multi = "--multi" in args
q41_mode = "--q41" in args
prompt_mode = "--prompt" in args or q41_mode
opt = lambda k, d: args[args.index(k) + 1] if k in args else d
nl = int(args[0]) if args and args[0].isdigit() else (8 if multi or prompt_mode else 4)
ftype = opt("--ftype", "f16")
hp = synth.HParams(n_vocab=32000, n_embd=4096, n_mult=256, n_head=32, n_layer=nl)
path = f"/tmp/dense7b_{ftype}_{nl}.bin" if multi or prompt_mode else "/tmp/dense7b_f16.bin"
rng = np.random.default_rng(1)
if not ((multi or prompt_mode) and os.path.exists(path)):
    t = {}
    for name, shape in synth.tensor_specs(hp):
        t[name] = (1.0 + 0.1 * rng.standard_normal(shape, dtype=np.float32)) if len(shape) == 1 else (0.02 * rng.standard_normal(shape, dtype=np.float32))
    synth.write_model_unquantized(path, hp, t, 0 if ftype == "f32" else 1)
    del t
prompt = np.concatenate([[1], np.random.default_rng(2).integers(3, 32000, 255)]).astype(np.int32)

if q41_mode:
    R = int(opt("--repeats", "3"))
    ints = lambda k, d: [int(x) for x in opt(k, d).split(",") if x]
    qpath = f"/tmp/dense7b_q41_{nl}.bin"
    if not os.path.exists(qpath):
        L.quantize_file(path, qpath, 3)
    stream = np.concatenate([[1], np.random.default_rng(2).integers(3, 32000, 511)]).astype(np.int32)
    tracing = "--trace-rows" in args
    m = L.Model(qpath, n_ctx=512, flags=1 if tracing else 0)          # (1 = LLAMAHIP_FLAG_NO_GRAPH: a kernel trace names the launches of a step)

    def timed(fn):
        fn()
        out = []
        for _ in range(R):
            t0 = time.perf_counter(); fn(); out.append(round((time.perf_counter() - t0) * 1e3, 4))
        return out
    res = {"library": L.LIB_PATH, "ftype": "q41", "n_layer": nl, "file_gb": round(os.path.getsize(qpath) / 1e9, 2)}
    if tracing:
        for n in ints("--trace-rows", ""):
            if n == 1:
                m.eval(stream[:8], 0)
                m.decode_greedy(int(stream[8]), 8, 1 + R)
            else:
                for _ in range(1 + R):
                    m.eval(stream[:n], 0)
        res["trace_rows"], res["repeats"] = ints("--trace-rows", ""), R
    else:
        first = int(np.argmax(m.eval(prompt, 0)))
        res["decode_greedy_ms_per_token"] = [round(x / 64, 4) for x in timed(lambda: m.decode_greedy(first, 256, 64))]
        res["eval_ms"] = {str(n): timed(lambda: m.eval(stream[:n], 0)) for n in ints("--evals", "9,16,17,64,512")}
    if hasattr(L, "q41_paths"):
        res["q41_paths"] = L.q41_paths()
    print(json.dumps(res))
    if "--json" in args:
        with open(opt("--json", ""), "w") as f:
            json.dump(res, f, indent=1)
    m.close()
    sys.exit(0)

if prompt_mode:
    R = int(opt("--repeats", "3"))
    ints = lambda k, d: [int(x) for x in opt(k, d).split(",") if x]
    force = opt("--force", "")
    if force:
        L.dense_force(force)
    stream = np.concatenate([[1], np.random.default_rng(2).integers(3, 32000, 511)]).astype(np.int32)
    m = L.Model(path, n_ctx=512, n_seq=16)

    def timed(fn):
        fn()
        out = []
        for _ in range(R):
            t0 = time.perf_counter(); fn(); out.append(round((time.perf_counter() - t0) * 1e3, 4))
        return out
    res = {"library": os.path.basename(L.LIB_PATH), "force": force, "ftype": ftype, "n_layer": nl, "file_gb": round(os.path.getsize(path) / 1e9, 2)}
    if "--trace-rows" in args:
        for n in ints("--trace-rows", ""):
            for _ in range(1 + R):
                m.eval_logprobs(stream[:n], 0)
        res["trace_rows"], res["repeats"] = ints("--trace-rows", ""), R
    else:
        res["eval_ms"] = {str(n): timed(lambda: m.eval(stream[:n], 0)) for n in ints("--evals", "64,128,512")}
        res["eval_chunks9_ms"] = {str(n): timed(lambda: m.eval_chunks(stream[:n], 0, 9)) for n in ints("--chunks", "18,36,72,144,504")}
        firsts = []
        for s_ in range(16):
            m.set_seq(s_)
            firsts.append(int(np.argmax(m.eval(np.concatenate([prompt[:255 - s_], prompt[:s_ + 1]]), 0))))
        m.set_seq(0)
        res["decode_greedy_ms_per_token"] = [round(x / 64, 4) for x in timed(lambda: m.decode_greedy(firsts[0], 256, 64))]
        res["set16_ms_per_step"] = [round(x / 64, 4) for x in timed(lambda: m.decode_greedy_multi(firsts, [256] * 16, 64))]
    if hasattr(L, "dense_paths"):
        res["dense_paths"] = L.dense_paths()
    if hasattr(L, "dense_mfma_launches"):
        res["dense_mfma_launches"] = L.dense_mfma_launches()
    print(json.dumps(res))
    if "--json" in args:
        with open(opt("--json", ""), "w") as f:
            json.dump(res, f, indent=1)
    m.close()
    sys.exit(0)

if multi:
    seqs = [int(s) for s in opt("--seqs", "1,2,4,8,16").split(",")]
    R, STEPS, POS = int(opt("--repeats", "3")), 64, 256
    m = L.Model(path, n_ctx=512, n_seq=max(seqs))
    firsts = []
    for s in range(max(seqs)):
        m.set_seq(s)
        firsts.append(int(np.argmax(m.eval(np.concatenate([prompt[:POS - s - 1], prompt[:s + 1]]), 0))))      # (a different context per slot)
    m.set_seq(0)

    def timed(fn):
        fn()
        out = []
        for _ in range(R):
            t0 = time.perf_counter(); fn(); out.append((time.perf_counter() - t0) * 1e3)
        return out
    res = {"library": os.path.basename(L.LIB_PATH), "dense_mm": os.environ.get("LLAMAHIP_DENSE_MM", ""), "n_layer": nl,
           "file_gb": round(os.path.getsize(path) / 1e9, 2), "steps": STEPS, "from_position": POS, "multi": {}}
    for S in seqs:
        ms = timed(lambda: m.decode_greedy_multi(firsts[:S], [POS] * S, STEPS))
        res["multi"][str(S)] = {"ms_per_step": [round(x / STEPS, 4) for x in ms], "tokens_per_s": [round(S * STEPS / (x / 1e3), 1) for x in ms]}
        print(f"S {S:2d}: {min(ms) / STEPS:.3f} ms/step, {S * STEPS / (min(ms) / 1e3):.0f} tokens/s ({nl} layers)", flush=True)
    if "--only-multi" not in args:                             # (a kernel trace of the set steps alone ends with them)
        res["eval9_ms"] = [round(x, 4) for x in timed(lambda: m.eval(prompt[:9], 0))]
        res["decode_greedy_ms_per_token"] = [round(x / STEPS, 4) for x in timed(lambda: m.decode_greedy(firsts[0], POS, STEPS))]
        print(f"9-token eval {min(res['eval9_ms']):.3f} ms; single stream {min(res['decode_greedy_ms_per_token']):.3f} ms/token")
    if hasattr(L, "dense_paths"):
        res["dense_paths"] = L.dense_paths()
    print(json.dumps(res))
    if "--json" in args:
        with open(opt("--json", ""), "w") as f:
            json.dump(res, f, indent=1)
    m.close()
    sys.exit(0)

t0 = time.perf_counter(); m = L.Model(path, n_ctx=512); print(f"loaded {os.path.getsize(path) / 1e9:.2f} GB in {time.perf_counter() - t0:.2f} s")
m.eval(prompt[:8], 0)
t0 = time.perf_counter(); lg = m.eval(prompt, 0); dt = time.perf_counter() - t0
print(f"prompt 256 tokens: {dt * 1e3:.1f} ms ({nl} layers) -> {256 / (dt * 32 / nl):.0f} tok/s at 32 layers")
tok = int(np.argmax(lg)); m.decode_greedy(tok, 256, 4)
t0 = time.perf_counter(); m.decode_greedy(tok, 260, 64); dt = time.perf_counter() - t0
per_layer = dt / 64 / nl
wbytes = (4 * 4096 * 4096 + 3 * 4096 * 11008) * 2
print(f"decode: {dt / 64 * 1e3:.3f} ms/token for {nl} layers + lm head = {per_layer * 1e6:.1f} us/layer-ish; 32 layers ~ {1 / (dt / 64 * 32 / nl):.0f} tok/s; "
      f"layer weights {wbytes / 1e6:.0f} MB -> {wbytes / per_layer / 1e12:.2f} TB/s upper bound")
m.close()
