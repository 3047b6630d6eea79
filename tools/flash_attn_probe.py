#!/usr/bin/env python3
"""LLAMAHIP_FLAG_FAST_ATTN against the exact attention chain, end to end on the 7B Q4_0 file (measurement tooling): every figure is taken in
fresh processes, `--reps` a side, and reported as median with min .. max.  Per process: a 2 048-token eval; evals of 64 / 128 / 512 rows at
n_past 0 and of 64 rows behind 1 984 cached tokens; ms per greedy decode token behind them.  Writes profiles/flash_attn_probe.json.
usage: flash_attn_probe.py [--model 7B] [--reps 5] [--out profiles/flash_attn_probe.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bench  # noqa: E402
import llama_swift_amd as L  # noqa: E402

SIDES = {"exact": 0, "fast_attn": 64, "fast_prefill": 16, "fast_prefill+fast_attn": 16 | 64}
SHAPES = [(2048, 0), (512, 0), (128, 0), (64, 0), (64, 1984)]


def child(path, flags, n_vocab):
    toks = np.random.default_rng(9).integers(3, n_vocab, 2048).astype(np.int32)
    toks[0] = 1
    out = {}
    with L.Model(path, n_ctx=2560, flags=flags) as m:
        m.eval(toks, 0, 8)                                  # warm: code objects, workspaces, rows 0 .. 2047 of the cache
        for n, n_past in SHAPES:
            m.eval(toks[:n], n_past, 8)
            best = 1e9
            for _ in range(5):
                t0 = time.perf_counter(); m.eval(toks[:n], n_past, 8); best = min(best, time.perf_counter() - t0)
            out[f"eval_{n}_at_{n_past}_ms"] = best * 1e3
        m.decode_greedy(5, 2048, 8, 8)
        t0 = time.perf_counter(); m.decode_greedy(5, 2048, 64, 8); out["decode_ms_per_token"] = (time.perf_counter() - t0) * 1e3 / 64
    out["flash_launches"] = L.flash_attn_launches()
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7B")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flash_attn_probe.json"))
    ap.add_argument("--child", type=int, default=-1)
    args = ap.parse_args()
    cfg = bench.MODELS[args.model]
    path = bench.model_path(args.model, cfg, 20230312)
    if args.child >= 0:
        child(path, args.child, cfg["n_vocab"])
        sys.exit(0)
    runs = {name: [] for name in SIDES}
    for _ in range(args.reps):                              # the sides alternate: other work shares the machine
        for name, flags in SIDES.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--model", args.model, "--child", str(flags)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"{name}: child failed ({r.returncode}):\n{r.stderr[-2000:]}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    summary = {name: {k: {"median": statistics.median(x[k] for x in rs), "min": min(x[k] for x in rs), "max": max(x[k] for x in rs)} for k in rs[0]} for name, rs in runs.items()}
    for name, s in summary.items():
        print(name, {k: f"{v['median']:.3f} ({v['min']:.3f} .. {v['max']:.3f})" for k, v in s.items()}, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"model": args.model, "reps": args.reps, "what": __doc__.split("\n")[0], "sides": SIDES, "summary": summary, "runs": runs}, f, indent=1)
