#!/usr/bin/env python3
"""Scoring over several KV slots against the per-slot calls it stands for, on the synthetic 7B file.
usage: score_probe.py [--json OUT] [--runs 5] [--repeats 3]
       score_probe.py --child SIDE          one process: a JSON line of raw times (what the parent starts, fresh, --runs times per side)
Sides, each in processes of its own, started in turn (multi, loop, whole, multi, loop, whole ...):
  multi   llamahip_eval_logprobs_multi over the segments; llamahip_score_choices
  loop    set_seq + llamahip_eval_logprobs per segment; the contract's per-choice sequence (context on the choice's slot, then one scoring eval)
  whole   score_choices only: one llamahip_eval_logprobs of context + ending per choice, the ending's rows scored
Shapes: segments x rows of 4x10, 8x10, 16x10, 16x32 and 4x128 at n_past 64, every row scored; a context of 64 and of 256 tokens with four
endings of 10 tokens.  Every figure is the wall time in ms of a call that synchronises before it returns, after one untimed run of the same
call; a run's figure is the minimum of its --repeats timed calls.  Per shape and side the parent reports the median (min .. max) over the
runs, whether multi and loop returned the same bytes, and `not_faster` where multi does not beat loop by more than loop's own min .. max spread.
LLAMAHIP_LIB selects the library as usual."""
import hashlib, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

args = sys.argv[1:]
opt = lambda k, d: args[args.index(k) + 1] if k in args else d
MODEL = os.path.join(os.environ.get("LLAMAHIP_MODEL_DIR", "/tmp/llamahip_models"), "7B-seed20230312", "ggml-model-q4_0.bin")
SEGS = [(4, 10), (8, 10), (16, 10), (16, 32), (4, 128)]
CHOICES = [(64, 4, 10), (256, 4, 10)]
N_PAST, NTH, REPEATS = 64, 8, int(opt("--repeats", "3"))
SIDES = ("multi", "loop", "whole")


def child(side):
    import numpy as np
    import llama_swift_amd as L
    m = L.Model(MODEL, n_ctx=320, n_seq=16)
    rng = np.random.default_rng(5)
    draw = lambda n: rng.integers(3, m.n_vocab, n).astype(np.int32)
    prefix = [draw(N_PAST) for _ in range(16)]
    toks, tgts = [draw(128) for _ in range(16)], [draw(128) for _ in range(16)]
    ctx, ends = draw(256), [draw(10) for _ in range(4)]
    m.eval_multi(list(range(16)), [0] * 16, prefix, chunk_tokens=0, n_threads=NTH)          # the same 64 rows under every segment, on every side

    def segs_multi(s, n):
        r = m.eval_logprobs_multi(list(range(s)), [N_PAST] * s, [t[:n] for t in toks[:s]], targets=[t[:n] for t in tgts[:s]], n_threads=NTH)
        return r["logprob"]

    def segs_loop(s, n):
        out = []
        for i in range(s):
            m.set_seq(i)
            out.append(m.eval_logprobs(toks[i][:n], N_PAST, NTH, targets=tgts[i][:n])["logprob"])
        return np.concatenate(out)

    def choices_multi(nc):
        return np.concatenate(m.score_choices(ctx[:nc], ends, n_threads=NTH)["rows"])

    def choices_loop(nc):
        out = []
        for i, e in enumerate(ends):
            m.set_seq(i)
            m.eval(ctx[:nc - 1], 0, NTH)
            out.append(m.eval_logprobs(np.concatenate([ctx[nc - 1:nc], e[:-1]]), nc - 1, NTH, targets=e)["logprob"])
        return np.concatenate(out)

    def choices_whole(nc):
        out = []
        for i, e in enumerate(ends):
            m.set_seq(i)
            tg = np.concatenate([np.full(nc - 1, -1, np.int32), e])
            out.append(m.eval_logprobs(np.concatenate([ctx[:nc], e[:-1]]), 0, NTH, targets=tg)["logprob"][nc - 1:])
        return np.concatenate(out)

    def measure(fn, *a):
        out = fn(*a)          # (untimed)
        ts = []
        for _ in range(REPEATS):
            t0 = time.perf_counter(); fn(*a); ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms": ts, "sha1": hashlib.sha1(np.ascontiguousarray(out).tobytes()).hexdigest()}

    res = {}
    if side != "whole":
        for s, n in SEGS:
            res[f"segs {s}x{n}"] = measure(segs_multi if side == "multi" else segs_loop, s, n)
    for nc, _, _ in CHOICES:
        res[f"choices ctx {nc}"] = measure({"multi": choices_multi, "loop": choices_loop, "whole": choices_whole}[side], nc)
    print("PROBE " + json.dumps({"library": os.path.basename(L.LIB_PATH), "side": side, "shapes": res}), flush=True)
    m.close()


if "--child" in args:
    child(opt("--child", "multi"))
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
table = []
names = [f"segs {s}x{n}" for s, n in SEGS] + [f"choices ctx {nc}" for nc, _, _ in CHOICES]
for name in names:
    row = {"shape": name}
    shas = set()
    for side in SIDES:
        per_run = [min(r["shapes"][name]["ms"]) for r in runs[side] if name in r["shapes"]]
        if not per_run:
            continue
        if side != "whole":          # (the whole-text eval splits the keys of V*P differently: close, not the same bytes)
            shas |= {r["shapes"][name]["sha1"] for r in runs[side]}
        row[side] = {"median_ms": round(statistics.median(per_run), 3), "min_ms": round(min(per_run), 3), "max_ms": round(max(per_run), 3)}
    row["same_bits"] = len(shas) == 1
    row["speedup_over_loop"] = round(row["loop"]["median_ms"] / row["multi"]["median_ms"], 2)
    row["not_faster"] = bool(row["loop"]["median_ms"] - row["multi"]["median_ms"] <= row["loop"]["max_ms"] - row["loop"]["min_ms"])
    table.append(row)
    print(f"{name:16s} | " + " | ".join(f"{side} {row[side]['median_ms']:8.3f} ({row[side]['min_ms']:.3f} .. {row[side]['max_ms']:.3f})" for side in SIDES if side in row)
          + f" | x{row['speedup_over_loop']:.2f}{'  NOT FASTER' if row['not_faster'] else ''}{'' if row['same_bits'] else '  BITS DIFFER'}", flush=True)
res = {"model": "7B synthetic (seed 20230312), Q4_0", "library": runs["multi"][0]["library"], "n_threads": NTH, "n_past": N_PAST, "runs_per_side": len(runs["multi"]), "repeats": REPEATS,
       "method": "every side in fresh processes started in turn; in a process one untimed call, then `repeats` timed calls, the run's figure their minimum; median (min .. max) over the runs, ms per call",
       "table": table, "raw": runs}
if "--json" in args:
    with open(opt("--json", ""), "w") as f:
        json.dump(res, f, indent=1)
