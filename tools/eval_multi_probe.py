#!/usr/bin/env python3
"""llamahip_eval_multi against the per-slot loop it stands for (set_seq + eval_chunks / eval per slot), on the synthetic 7B file.
usage: eval_multi_probe.py [--json OUT] [--processes 3] [--repeats 3] [--seqs 2,4,8,16] [--lens 9,32,128,512] [--chunks 9,0]
       eval_multi_probe.py --child [...]          one process: a JSON line of raw times (what the parent starts, fresh, --processes times)
       eval_multi_probe.py --trace-child          one process for a kernel trace of its own: 8 x 9 rows, chunk 9 -- five one-pass calls, then five loops
Every figure is the wall time in ms of a call that synchronises before it returns, after one untimed run of the same call; inside a process
the two ways ALTERNATE (one pass, loop, one pass, loop ...) on the same handle.  Per shape the parent reports the median over the processes of
each process's minimum, the loop's own min .. max over all its timed runs, and `slower` where the one pass exceeds the loop by more than that
spread.  Shapes whose rows pass LLAMAHIP_EVAL_MULTI_MAX_ROWS (2048) are left out.
--short-max N (measurement: LLAMAHIP_EVAL_MULTI_SHORT_MAX=N in the children) lets segments of up to N rows join the table launch instead of
taking the long eval's attention launches on their own.  LLAMAHIP_LIB selects the library as usual."""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

args = sys.argv[1:]
opt = lambda k, d: args[args.index(k) + 1] if k in args else d
ints = lambda k, d: [int(x) for x in opt(k, d).split(",")]
SEQS, LENS, CHUNKS, R = ints("--seqs", "2,4,8,16"), ints("--lens", "9,32,128,512"), ints("--chunks", "9,0"), int(opt("--repeats", "3"))
MODEL = os.path.join(os.environ.get("LLAMAHIP_MODEL_DIR", "/tmp/llamahip_models"), "7B-seed20230312", "ggml-model-q4_0.bin")
MAX_ROWS, NTH = 2048, 8
shapes = [(s, n, c) for c in CHUNKS for n in LENS for s in SEQS if s * n <= MAX_ROWS]


def child(trace):
    import numpy as np
    import llama_swift_amd as L
    n_seq = 8 if trace else max(SEQS)
    m = L.Model(MODEL, n_ctx=(16 if trace else max(LENS)) + 8, n_seq=n_seq)
    rng = np.random.default_rng(5)
    toks = [np.concatenate([[1], rng.integers(3, m.n_vocab, (16 if trace else max(LENS)) - 1)]).astype(np.int32) for _ in range(n_seq)]

    def one_pass(s, n, c):
        return m.eval_multi(list(range(s)), [0] * s, [t[:n] for t in toks[:s]], chunk_tokens=c, n_threads=NTH)

    def loop(s, n, c):
        out = []
        for i in range(s):
            m.set_seq(i)
            out.append(m.eval_chunks(toks[i][:n], 0, c, NTH) if c > 0 else m.eval(toks[i][:n], 0, NTH))
        return np.stack(out)

    def timed(fn, *a):
        t0 = time.perf_counter(); r = fn(*a); return (time.perf_counter() - t0) * 1e3, r

    if trace:
        for fn in (one_pass, loop):
            for _ in range(6):
                fn(8, 9, 9)
        return
    res = []
    for s, n, c in shapes:
        _, a = timed(one_pass, s, n, c)
        _, b = timed(loop, s, n, c)
        same = bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))          # (faster and different is not faster)
        tm, tl = [], []
        for _ in range(R):
            tm.append(timed(one_pass, s, n, c)[0])
            tl.append(timed(loop, s, n, c)[0])
        res.append({"n_seqs": s, "n_tokens": n, "chunk": c, "same_bits": same, "one_pass_ms": tm, "loop_ms": tl})
    print("PROBE " + json.dumps({"library": os.path.basename(L.LIB_PATH), "shapes": res}), flush=True)
    m.close()


if "--child" in args or "--trace-child" in args:
    child("--trace-child" in args)
    sys.exit(0)

subprocess.run(["bash", os.path.join(ROOT, "tools", "ensure_7b.sh")], cwd=ROOT, check=True)
runs = []
for p in range(int(opt("--processes", "3"))):
    env = dict(os.environ, LLAMAHIP_EVAL_MULTI_SHORT_MAX=opt("--short-max", "0"))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args, capture_output=True, text=True, timeout=900, env=env)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("PROBE ")]
    if out.returncode != 0 or not line:
        sys.exit(f"process {p} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    runs.append(json.loads(line[0][6:]))
table = []
for k, (s, n, c) in enumerate(shapes):
    rows = [r["shapes"][k] for r in runs]
    one = statistics.median(min(r["one_pass_ms"]) for r in rows)
    lp = statistics.median(min(r["loop_ms"]) for r in rows)
    lo, hi = min(min(r["loop_ms"]) for r in rows), max(max(r["loop_ms"]) for r in rows)
    table.append({"n_seqs": s, "n_tokens": n, "chunk": c, "rows": s * n, "one_pass_ms": round(one, 3), "loop_ms": round(lp, 3),
                  "loop_min_ms": round(lo, 3), "loop_max_ms": round(hi, 3), "speedup": round(lp / one, 2),
                  "slower": bool(one - lp > hi - lo), "same_bits": all(r["same_bits"] for r in rows)})
    print(f"chunk {c} | {s:2d} x {n:3d} rows | one pass {one:8.3f} ms | loop {lp:8.3f} ms ({lo:.3f} .. {hi:.3f}) | x{lp / one:.2f}"
          f"{'  SLOWER' if table[-1]['slower'] else ''}{'' if table[-1]['same_bits'] else '  BITS DIFFER'}", flush=True)
res = {"model": "7B synthetic (seed 20230312), Q4_0", "short_max": int(opt("--short-max", "0")) or 60, "library": runs[0]["library"], "n_threads": NTH, "processes": len(runs), "repeats": R,
       "method": "fresh processes; in each, one pass and loop alternate on one handle after one untimed run each; ms per call = median over processes of the process minimum; loop_min .. loop_max over every timed loop run",
       "table": table, "raw": runs}
if "--json" in args:
    with open(opt("--json", ""), "w") as f:
        json.dump(res, f, indent=1)
