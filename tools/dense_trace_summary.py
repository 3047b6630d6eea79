#!/usr/bin/env python3
"""Per-launch time of the f16 / f32 mat-mul of more than 16 rows from a rocprofv3 --kernel-trace run of
`tools/dense_probe.py N_LAYER --prompt --trace-rows A,B,.. --repeats R [--force mm|mfma]`.
usage: dense_trace_summary.py <dir-or-kernel_trace.csv> N_LAYER R A,B,..
The dispatches of k_dense_mm / k_dense_mfma are taken in start order: per row count 1 + R eval_logprobs calls (the first one untimed), per call
N_LAYER x (wq|wk|wv, wo, w1|w3, w2) then the lm head.  Prints one JSON object: per row count and matrix the median / min / max us over the R
calls x N_LAYER layers, and the FMA rate of the median in TF (2 M K N flop) for LLaMA-7B shapes."""
import csv, glob, json, os, statistics, sys

src, nl, R, rows_list = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), [int(x) for x in sys.argv[4].split(",")]
files = [src] if os.path.isfile(src) else glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True)
disp = []
for f in files:
    for r in csv.DictReader(open(f)):
        low = {k.lower(): v for k, v in r.items()}
        name = low.get("kernel_name", "")
        if "k_dense_mm" in name or "k_dense_mfma" in name:
            disp.append((int(low["start_timestamp"]), int(low["end_timestamp"]), "mfma" if "k_dense_mfma" in name else "mm"))
disp.sort()
per_call = nl * 4 + 1
want = len(rows_list) * (1 + R) * per_call
if len(disp) != want:
    sys.exit(f"{len(disp)} dispatches of the two kernels, expected {want}")
MATS = ("wqkv", "wo", "w13", "w2", "lm_head")
SHAPE = {"wqkv": (12288, 4096), "wo": (4096, 4096), "w13": (22016, 4096), "w2": (4096, 11008), "lm_head": (32000, 4096)}
out, at = {}, 0
for n in rows_list:
    us = {k: [] for k in MATS}
    kernels = set()
    for call in range(1 + R):
        for i in range(per_call):
            s, e, k = disp[at]; at += 1
            if call:
                us[MATS[i % 4] if i < nl * 4 else "lm_head"].append((e - s) / 1e3)
                kernels.add(k)
    out[str(n)] = {"kernel": sorted(kernels)}
    for k in MATS:
        med = statistics.median(us[k])
        M, K = SHAPE[k]
        out[str(n)][k] = {"us_median": round(med, 1), "us_min": round(min(us[k]), 1), "us_max": round(max(us[k]), 1), "tf": round(2.0 * M * K * n / med / 1e6, 1)}
print(json.dumps(out, indent=1))
