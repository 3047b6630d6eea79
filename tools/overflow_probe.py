#!/usr/bin/env python3
"""Crossing the end of the context: the in-place shift (LLAMAHIP_CTX_SHIFT) against the re-evaluation (LLAMAHIP_CTX_REEVAL), synthetic 7B file.
usage: overflow_probe.py [--json OUT] [--runs 5] [--ctx 512,2048] [--keep 0,1,63,64] [--window-keep 0,64]

DESIGN.md 12.15's rule: the shift mode is justified where the shift's max lies below the re-eval's min at both context sizes.
Every side runs in FRESH processes started in turn (shift, re-eval, shift, ... `--runs` of each per context size); a process loads the file
once and measures, for each n_keep:
  shift side    llamahip_bench_kv_shift of the plan's one shift at the wall (event-timed, 20 launches after one untimed); then
                decode_greedy_window(mode CTX_SHIFT) over 4 * n_ctx steps from a 32-token context, wall time (for the n_keep of --window-keep)
  re-eval side  the same tail fed again at n_keep: llamahip_eval_chunks in chunks of 9 (the runner's) and one llamahip_eval, wall time of the
                second of two calls each; then decode_greedy_window(mode CTX_REEVAL, one eval per crossing) over the same steps
An even n_keep gives n_rows == n_discard: the ranges do not alias.  An odd n_keep gives n_rows == n_discard + 1: one row of overlap, the
in-place hazard the kernel's row order exists for.  Both are measured, so the rule is checked on the aliasing case too.
Reported: median (min .. max) over the runs; the shift's bytes per second (read + write of every moved K and V row of every layer); the
verdict of the rule; and, as information with no threshold, the share of the first 256 tokens after the first crossing that the two
modes' end-to-end runs have in common."""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

args = sys.argv[1:]
opt = lambda k, d: args[args.index(k) + 1] if k in args else d
MODEL = os.path.join(os.environ.get("LLAMAHIP_MODEL_DIR", "/tmp/llamahip_models"), "7B-seed20230312", "ggml-model-q4_0.bin")
RUNS = int(opt("--runs", "5"))
CTXS = [int(x) for x in opt("--ctx", "512,2048").split(",")]
KEEPS = [int(x) for x in opt("--keep", "0,1,63,64").split(",")]
WINDOW_KEEPS = [int(x) for x in opt("--window-keep", "0,64").split(",")]
N_PROMPT, NTH = 32, 8


def one_side(side, n_ctx):
    """--side shift|reeval --n-ctx C: this fresh process's measurements, one JSON line"""
    import numpy as np
    import llama_swift_amd as L
    m = L.Model(MODEL, n_ctx=n_ctx)
    rng = np.random.default_rng(20240915)
    prompt = np.concatenate([[1], rng.integers(3, m.n_vocab, N_PROMPT - 1)]).astype(np.int32)
    out = {"side": side, "n_ctx": n_ctx, "keeps": {}}
    for keep in KEEPS:
        new, nd = L.ctx_overflow_plan(n_ctx, n_ctx, keep)
        rows = n_ctx - keep - nd
        r = {"n_discard": nd, "rows": rows}
        if side == "shift":
            r["aliasing"] = rows > nd
            r["shift_ms"] = m.bench_kv_shift([(0, keep + nd, rows, nd)], iters=20)
            r["bytes_moved"] = int(rows) * m.n_embd * 4 * 2 * m.n_layer * 2
        else:
            tail = rng.integers(3, m.n_vocab, rows).astype(np.int32)
            for name, fn in (("reeval_chunks9_ms", lambda: m.eval_chunks(tail, keep, 9, NTH)), ("reeval_one_eval_ms", lambda: m.eval(tail, keep, NTH))):
                fn()
                t0 = time.perf_counter()
                fn()
                r[name] = (time.perf_counter() - t0) * 1e3
        if keep in WINDOW_KEEPS:
            first = int(np.argmax(m.eval(prompt, 0, NTH)))
            mode = L.CTX_SHIFT if side == "shift" else L.CTX_REEVAL
            t0 = time.perf_counter()
            toks, _ = m.decode_greedy_window(first, 4 * n_ctx, N_PROMPT, prompt, n_keep=keep, mode=mode, chunk_tokens=0, n_threads=NTH)
            r["window_s"] = time.perf_counter() - t0
            cross = n_ctx - N_PROMPT          # the steps before the first crossing
            r["tokens_after_first_crossing"] = toks[cross:cross + 256].tolist()
        out["keeps"][str(keep)] = r
    m.close()
    print(json.dumps(out), flush=True)


def main():
    subprocess.run(["bash", os.path.join(ROOT, "tools", "ensure_7b.sh")], cwd=ROOT, check=True)
    spread = lambda xs: {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}
    res = {"model": "7B synthetic (seed 20230312), Q4_0", "n_threads": NTH, "runs": RUNS, "n_prompt": N_PROMPT,
           "method": "fresh processes started in turn (shift, re-eval, ...); shift: llamahip_bench_kv_shift, events around 20 back-to-back launches after one untimed "
                     "(no host wait inside the window; at n_ctx 512 part of the 0.5 GB working set can stay in the 256 MB Infinity Cache from launch to launch); "
                     "re-eval: wall time of the second of two calls; window: wall time of decode_greedy_window over 4 * n_ctx steps; median (min .. max)",
           "k_kv_copy_rows_bytes_per_s": "profiles/sched_prefix_probe_7b.json: about 5.4e12 on 256 rows, but as HOST wall time per enqueue + stream wait -- not measured alike", "cases": []}
    verdict = True
    for n_ctx in CTXS:
        got = {"shift": [], "reeval": []}
        for _ in range(RUNS):
            for side in ("shift", "reeval"):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--n-ctx", str(n_ctx), "--keep", ",".join(map(str, KEEPS)),
                                    "--window-keep", ",".join(map(str, WINDOW_KEEPS))],
                                   capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    sys.exit(f"{side} process at n_ctx {n_ctx} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
                got[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(f"n_ctx {n_ctx} {side}: done", flush=True)
        for keep in KEEPS:
            s = [g["keeps"][str(keep)] for g in got["shift"]]
            r = [g["keeps"][str(keep)] for g in got["reeval"]]
            case = {"n_ctx": n_ctx, "n_keep": keep, "n_discard": s[0]["n_discard"], "rows_moved": s[0]["rows"], "ranges_alias": s[0]["aliasing"],
                    "bytes_moved_read_plus_write": s[0]["bytes_moved"]}
            case["shift_ms"] = spread([x["shift_ms"] for x in s])
            case["shift_bytes_per_s"] = round(s[0]["bytes_moved"] / (case["shift_ms"]["median"] * 1e-3), 0)
            for k in ("reeval_chunks9_ms", "reeval_one_eval_ms"):
                case[k] = spread([x[k] for x in r])
            if keep in WINDOW_KEEPS:
                case["window_4n_ctx_steps_shift_s"] = spread([x["window_s"] for x in s])
                case["window_4n_ctx_steps_reeval_s"] = spread([x["window_s"] for x in r])
                a, b = s[0]["tokens_after_first_crossing"], r[0]["tokens_after_first_crossing"]
                case["tokens_in_common_first_256_after_crossing"] = round(sum(x == y for x, y in zip(a, b)) / max(len(a), 1), 4)
            case["shift_max_below_reeval_min"] = case["shift_ms"]["max"] < min(case["reeval_chunks9_ms"]["min"], case["reeval_one_eval_ms"]["min"])
            verdict = verdict and case["shift_max_below_reeval_min"]
            res["cases"].append(case)
    res["rule"] = "the shift mode is justified where the shift's max lies below the re-eval's min at both context sizes"
    res["shift_mode_justified"] = bool(verdict)
    text = json.dumps(res, indent=1)
    print(text)
    if "--json" in args:
        os.makedirs(os.path.dirname(os.path.abspath(opt("--json", ""))), exist_ok=True)
        open(opt("--json", ""), "w").write(text + "\n")


if __name__ == "__main__":
    if "--side" in args:
        one_side(opt("--side", ""), int(opt("--n-ctx", "512")))
    else:
        main()
