#!/usr/bin/env python3
"""Text embeddings over several KV slots against the eval they replace and the per-slot calls they stand for, on the synthetic 7B file.
usage: embed_probe.py [--json OUT] [--runs 5] [--repeats 3]
       embed_probe.py --child SIDE          one process: a JSON line of raw times (what the parent starts, fresh, --runs times per side)
Sides, each in processes of its own, started in turn (embed, logits, loop, embed, logits, loop ...):
  embed   llamahip_text_embedding_multi over the segments, MEAN + normalize and LAST + normalize
  logits  llamahip_eval_multi of the same segments with the logits rows copied back: what the lm head and the logits copy cost
  loop    set_seq + llamahip_text_embedding per segment, MEAN + normalize and LAST + normalize
Shapes: segments x rows of 4x10, 16x10, 16x32 and 4x128 at n_past 64.  Every figure is the wall time in ms of a call that synchronises before
it returns, after one untimed run of the same call; a run's figure is the minimum of its --repeats timed calls.  Per shape and side the parent
reports the median (min .. max) over the runs, whether embed and loop returned the same bytes, and `slower_than_loop` where the one pass is
slower than the loop by more than the loop's own min .. max spread.  LLAMAHIP_LIB selects the library as usual."""
import hashlib, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

args = sys.argv[1:]
opt = lambda k, d: args[args.index(k) + 1] if k in args else d
MODEL = os.path.join(os.environ.get("LLAMAHIP_MODEL_DIR", "/tmp/llamahip_models"), "7B-seed20230312", "ggml-model-q4_0.bin")
SEGS = [(4, 10), (16, 10), (16, 32), (4, 128)]
N_PAST, NTH, REPEATS = 64, 8, int(opt("--repeats", "3"))
SIDES = ("embed", "logits", "loop")
POOLS = ("mean", "last")


def child(side):
    import numpy as np
    import llama_swift_amd as L
    m = L.Model(MODEL, n_ctx=320, n_seq=16)
    rng = np.random.default_rng(5)
    draw = lambda n: rng.integers(3, m.n_vocab, n).astype(np.int32)
    prefix = [draw(N_PAST) for _ in range(16)]
    toks = [draw(128) for _ in range(16)]
    m.eval_multi(list(range(16)), [0] * 16, prefix, chunk_tokens=0, n_threads=NTH)          # the same 64 rows under every segment, on every side

    def embed(s, n, pool):
        return m.text_embedding_multi(list(range(s)), [N_PAST] * s, [t[:n] for t in toks[:s]], n_threads=NTH, pool=pool, normalize=True)

    def logits(s, n, pool):
        return m.eval_multi(list(range(s)), [N_PAST] * s, [t[:n] for t in toks[:s]], n_threads=NTH)

    def loop(s, n, pool):
        out = []
        for i in range(s):
            m.set_seq(i)
            out.append(m.text_embedding(toks[i][:n], N_PAST, NTH, 0, pool, True))
        return np.stack(out)

    def measure(fn, *a):
        out = fn(*a)          # (untimed)
        ts = []
        for _ in range(REPEATS):
            t0 = time.perf_counter(); fn(*a); ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms": ts, "sha1": hashlib.sha1(np.ascontiguousarray(out).tobytes()).hexdigest()}

    res = {}
    for s, n in SEGS:
        for pool in POOLS if side != "logits" else ("-",):
            res[f"{s}x{n} {pool}"] = measure({"embed": embed, "logits": logits, "loop": loop}[side], s, n, pool)
    print("PROBE " + json.dumps({"library": os.path.basename(L.LIB_PATH), "side": side, "shapes": res}), flush=True)
    m.close()


if "--child" in args:
    child(opt("--child", "embed"))
    sys.exit(0)

subprocess.run(["bash", os.path.join(ROOT, "tools", "ensure_7b.sh")], cwd=ROOT, check=True)
runs = {s: [] for s in SIDES}
for p in range(int(opt("--runs", "5"))):
    for side in SIDES:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", side, "--repeats", str(REPEATS)], capture_output=True, text=True, timeout=600)
        line = [ln for ln in out.stdout.splitlines() if ln.startswith("PROBE ")]
        if out.returncode != 0 or not line:
            sys.exit(f"run {p} of side {side} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
        runs[side].append(json.loads(line[0][6:]))
        print(f"run {p} {side}: " + "  ".join(f"{k} {min(v['ms']):.2f}" for k, v in runs[side][-1]["shapes"].items()), flush=True)
stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
table = []
for s, n in SEGS:
    lg = stat([min(r["shapes"][f"{s}x{n} -"]["ms"]) for r in runs["logits"]])
    for pool in POOLS:
        name = f"{s}x{n} {pool}"
        row = {"shape": f"{s}x{n}", "pool": pool, "eval_multi_with_logits": lg}
        for side in ("embed", "loop"):
            row[side] = stat([min(r["shapes"][name]["ms"]) for r in runs[side]])
        row["same_bits"] = len({r["shapes"][name]["sha1"] for side in ("embed", "loop") for r in runs[side]}) == 1
        row["saved_against_logits_ms"] = round(lg["median_ms"] - row["embed"]["median_ms"], 3)
        row["speedup_over_loop"] = round(row["loop"]["median_ms"] / row["embed"]["median_ms"], 2)
        row["slower_than_loop"] = bool(row["embed"]["median_ms"] - row["loop"]["median_ms"] > row["loop"]["max_ms"] - row["loop"]["min_ms"])
        table.append(row)
        print(f"{name:12s} | " + " | ".join(f"{k} {v['median_ms']:8.3f} ({v['min_ms']:.3f} .. {v['max_ms']:.3f})" for k, v in (("embed", row["embed"]), ("logits", lg), ("loop", row["loop"])))
              + f" | x{row['speedup_over_loop']:.2f} over the loop{'  SLOWER THAN THE LOOP' if row['slower_than_loop'] else ''}{'' if row['same_bits'] else '  BITS DIFFER'}", flush=True)
res = {"model": "7B synthetic (seed 20230312), Q4_0", "library": runs["embed"][0]["library"], "n_threads": NTH, "n_past": N_PAST, "runs_per_side": len(runs["embed"]), "repeats": REPEATS,
       "method": "every side in fresh processes started in turn; in a process one untimed call, then `repeats` timed calls, the run's figure their minimum; median (min .. max) over the runs, ms per call",
       "table": table, "raw": runs}
if "--json" in args:
    with open(opt("--json", ""), "w") as f:
        json.dump(res, f, indent=1)
