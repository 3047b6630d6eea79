"""What constrained greedy decoding (llamahip_decode_greedy_constrained) costs per token, on the full-depth synthetic 7B Q4_0 file bench.py
makes.  Every figure comes from fresh processes (this script re-invoked with --leg), wall-clock around synchronous calls, --runs processes
per leg: median and min .. max over the processes.

  greedy        ms per token of llamahip_decode_greedy as shipped (the lm head's pick epilogue), STEPS steps from position P
  unfolded      ... under LLAMAHIP_NO_PICK_FOLD=1: forward + k_argmax, structurally the constrained step without the table read
  cst_1         ms per token of llamahip_decode_greedy_constrained with the all-allowed constraint (1 byte-state), same positions
  cst_300       ... with "[a-z]{299}" (300 byte-states: every step reads another row of the table)
  leg sweep     LLAMAHIP_CONSTRAIN_LEG = 4 / 8 / 16 / 32 (the measurement switch of the same name): ms per CALL of a short answer
                (choices = ["abc"]: 4 tokens with the stop token; ["abcde"]: 6) and ms per token of the long one ("[a-z]{299}")

The constrained step is judged against `unfolded` of the same run: the difference is the table row read beside the logits and the 8-byte
look at {state, dead} once per leg.

    python tools/constrain_probe.py [--out profiles/constrain_probe_7b.json] [--runs 3]
    python tools/constrain_probe.py --leg cst_300      (one leg in this process)
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

N_CTX, P, STEPS, NTH, REPS = 512, 16, 299, 8, 3
LEGS = {"greedy": {}, "unfolded": {"LLAMAHIP_NO_PICK_FOLD": "1"}, "cst_1": {}, "cst_300": {}}
LEGS.update({f"leg{n}": {"LLAMAHIP_CONSTRAIN_LEG": str(n)} for n in (4, 8, 16, 32)})


def run_leg(name):
    import numpy as np

    import bench
    import llama_swift_amd as L
    import synth
    path = bench.model_path("7B", bench.MODELS["7B"], 20230312)
    prompt = synth.synth_prompt(P + 1, 32000, seed=3)
    out = {}
    with L.Model(path, n_ctx=N_CTX) as m:
        def timed(call, per):
            ts = []
            for r in range(REPS + 1):              # (the first repeat is the warm-up: graphs are captured in it)
                m.eval(prompt[:-1], 0)
                t0 = time.perf_counter()
                got = call()
                ts.append((time.perf_counter() - t0) * 1e3 / per)
            return got, statistics.median(ts[1:])

        first = int(prompt[-1])
        if name in ("greedy", "unfolded"):
            _, out["ms_per_token"] = timed(lambda: m.decode_greedy(first, P, STEPS, NTH), STEPS)
        elif name == "cst_1":
            with m.constraint(dfa=(np.zeros((1, 256), np.int32), np.ones(1, np.uint8), 0)) as c:
                got, out["ms_per_token"] = timed(lambda: m.decode_greedy_constrained(first, P, STEPS, c, n_threads=NTH), STEPS)
                out["tokens"] = int(got["tokens"].size)
        elif name == "cst_300":
            with m.constraint(regex="[a-z]{299}") as c:
                got, out["ms_per_token"] = timed(lambda: m.decode_greedy_constrained(first, P, STEPS + 1, c, n_threads=NTH), STEPS + 1)
                out["tokens"], out["finished"], out["n_states"] = int(got["tokens"].size), got["finished"], c.n_states
        else:
            with m.constraint(choices=["abc"]) as short, m.constraint(choices=["abcde"]) as short6, m.constraint(regex="[a-z]{299}") as long_:
                got, out["short_ms_per_call"] = timed(lambda: m.decode_greedy_constrained(first, P, 64, short, n_threads=NTH), 1)
                out["short_tokens"] = int(got["tokens"].size)
                got, out["short6_ms_per_call"] = timed(lambda: m.decode_greedy_constrained(first, P, 64, short6, n_threads=NTH), 1)
                out["short6_tokens"] = int(got["tokens"].size)
                got, out["long_ms_per_token"] = timed(lambda: m.decode_greedy_constrained(first, P, STEPS + 1, long_, n_threads=NTH), STEPS + 1)
                out["long_tokens"] = int(got["tokens"].size)
    print("LEG " + json.dumps(out))


def fresh(name, runs):
    rows = []
    for _ in range(runs):
        env = dict(os.environ, **LEGS[name])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], env=env, capture_output=True, text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
        if r.returncode != 0 or not line:
            raise RuntimeError(f"leg {name} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        rows.append(json.loads(line[0][4:]))
    res = dict(rows[0])
    for k in [k for k in rows[0] if "ms_per" in k]:
        v = [row[k] for row in rows]
        res[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrain_probe_7b.json"))
    ap.add_argument("--sweep-only", action="store_true", help="the leg sweep alone, merged into the --out file where it exists")
    args = ap.parse_args()
    if args.leg:
        return run_leg(args.leg)
    res = {"model": "synthetic LLaMA-7B Q4_0, 32 layers", "n_ctx": N_CTX, "positions": [P, P + STEPS], "n_threads": NTH, "processes_per_leg": args.runs,
           "repeats_per_process": REPS}
    if args.sweep_only and os.path.exists(args.out):
        res = json.load(open(args.out))
    for name in [n for n in LEGS if n.startswith("leg") or not args.sweep_only]:
        res[name] = fresh(name, args.runs)
        print(name, json.dumps(res[name]), flush=True)
    if all(k in res for k in ("unfolded", "cst_1", "cst_300")):
        u, c1, c300 = (res[k]["ms_per_token"]["median"] for k in ("unfolded", "cst_1", "cst_300"))
        res["constrained_minus_unfolded_ms"] = {"cst_1": c1 - u, "cst_300": c300 - u}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
