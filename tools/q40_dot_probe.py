#!/usr/bin/env python3
"""Single-stream decode of the 7B Q4_0 file with and without llamahip_opts.fast_decode (k_q40_dot on wo / w2): fresh
processes, the sides alternating, R a side, median (min .. max) -> profiles/q40_dot_probe.json.
Sides: exact (a default handle), fast (fast_decode = 1) and, where LLAMAHIP_PARENT_ROOT names a built checkout of the parent commit,
parent (a default handle of that tree's package and library).
  q40_dot_probe.py [--repeats 5] [--steps 128] [--n_ctx 512] [--trace] [--out profiles/q40_dot_probe.json]
    ms per token of decode_greedy from position 8 (one untimed call first: graph capture; the best of three timed calls per process).
    --trace: also R processes a side under `rocprofv3 --kernel-trace --stats`, nothing timed by the host; per process the mean in-situ
    microseconds of every decode mat-vec launch, grouped by (kernel, grid, LDS bytes) -- wo and w2 differ in their LDS bytes.
  q40_dot_probe.py --child SIDE [--trace-run]      one process of one side (what the above starts); prints one JSON line."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--child", default="")
ap.add_argument("--trace-run", action="store_true")
ap.add_argument("--trace", action="store_true")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--n_ctx", type=int, default=512)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q40_dot_probe.json"))
ap.add_argument("--trace-dir", default=os.path.join(tempfile.gettempdir(), "q40_dot_trace"), help="where the profiler writes (one folder per process)")
args = ap.parse_args()


def child():
    sys.path.insert(0, os.environ["LLAMAHIP_PARENT_ROOT"] if args.child == "parent" else ROOT)
    import numpy as np
    import bench
    import llama_swift_amd as L
    path = bench.model_path("7B", bench.MODELS["7B"], 20230312)
    m = L.Model(path, n_ctx=args.n_ctx, **(dict(fast_decode=1) if args.child == "fast" else {}))
    first = int(np.argmax(m.eval(bench.PROMPT, 0)))
    n0 = len(bench.PROMPT)
    toks = m.decode_greedy(first, n0, 33 if args.trace_run else args.steps)          # untimed: graph capture, first touches
    out = dict(side=args.child, crc=int(np.bitwise_xor.reduce(toks.astype(np.int64) * np.arange(1, toks.size + 1))), dot_launches=L.q40_dot_launches(m) if args.child != "parent" else 0)
    if not args.trace_run:
        best = 1e9
        for _ in range(3):
            t0 = time.perf_counter()
            m.decode_greedy(first, n0, args.steps)                                    # (synchronises before it returns)
            best = min(best, time.perf_counter() - t0)
        out["ms_per_token"] = best * 1e3 / args.steps
    print("PROBE " + json.dumps(out), flush=True)


def run_child(side, trace_dir=None):
    env = dict(os.environ)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--steps", str(args.steps), "--n_ctx", str(args.n_ctx)]
    if trace_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "--"] + cmd + ["--trace-run"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")]
    if r.returncode or not line:
        sys.exit(f"q40_dot_probe: side {side} failed (rc {r.returncode}): {r.stderr[-2000:]}")
    return json.loads(line[-1][6:])


def trace_groups(trace_dir):
    """mean microseconds per (kernel, grid, LDS bytes) of the decode mat-vecs in a rocprofv3 kernel trace"""
    groups = {}
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Kernel_Name", "")
            if "k_gemv<" not in name and "k_q40_dot" not in name:
                continue
            key = f'{name.split("(")[0][-70:]} grid {row.get("Grid_Size_X", row.get("Grid_Size", "?"))} lds {row.get("LDS_Block_Size", "?")}'
            groups.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: dict(n=len(v), mean_us=round(statistics.mean(v), 3), median_us=round(statistics.median(v), 3)) for k, v in sorted(groups.items())}


def summary(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4), all=[round(x, 4) for x in v])


if args.child:
    child()
    sys.exit(0)
sides = (["parent"] if os.environ.get("LLAMAHIP_PARENT_ROOT") else []) + ["exact", "fast"]
res = {s: [] for s in sides}
meta = {}
for r in range(args.repeats):
    for s in sides:
        o = run_child(s)
        res[s].append(o["ms_per_token"])
        meta[s] = dict(crc=o["crc"], dot_launches=o["dot_launches"])
        print(f"run {r} {s}: {o['ms_per_token']:.4f} ms/token, crc {o['crc']}, dot launches {o['dot_launches']}", flush=True)
report = dict(model="7B Q4_0 synthetic (bench.py seed)", n_ctx=args.n_ctx, steps=args.steps, repeats=args.repeats,
              decode_ms_per_token={s: dict(summary(res[s]), tokens_per_s=round(1e3 / statistics.median(res[s]), 1), **meta[s]) for s in sides})
if args.trace:
    report["trace_us"] = dict(exact=[], fast=[])
    for r in range(args.repeats):
        for s in ("exact", "fast"):
            d = os.path.join(args.trace_dir, f"{s}_{r}")
            run_child(s, d)
            report["trace_us"][s].append(trace_groups(d))
            print(f"trace {r} {s}: {json.dumps(report['trace_us'][s][-1])}", flush=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
json.dump(report, open(args.out, "w"), indent=1)
print(json.dumps(report["decode_ms_per_token"], indent=1))
