"""Cost of sampling on the multi-sequence path, on the synthetic 7B Q4_0 file bench.py makes: aggregate tokens/s of
llamahip_decode_greedy_multi against llamahip_decode_sample_multi (repeat penalty 1.3, top_k 40, top_p 0.95, temp 0.8, windows of 64)
for 1 .. 32 sequences, on a plain handle and on a 2-stage pipeline handle with both stages on GPU 0; alternated in one process.  Also the
share of draws that took the host path (exact = 0).  Prints one JSON line per handle and case, then a summary line.

    python tools/sample_multi_probe.py [--seqs 1,2,4,8,16,32] [--stages 1,2] [--steps 32] [--reps 5] [--out FILE]
    python tools/sample_multi_probe.py --one 16     (one plain-handle warm-up + one timed call of 16 sequences: for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import bench  # noqa: E402
import llama_swift_amd as L  # noqa: E402
import synth  # noqa: E402

N_CTX, PROMPT = 256, 8


def prepare(m, n):
    """every slot's 8-token prompt evaluated; first tokens = the prompts' argmax"""
    firsts = []
    for i in range(n):
        m.set_seq(i)
        firsts.append(int(np.argmax(m.eval(synth.synth_prompt(PROMPT, m.n_vocab, seed=100 + i), 0, 8))))
    m.set_seq(0)
    return firsts


def run_case(m, firsts, n, steps, reps):
    n_past = [PROMPT] * n
    samplers = [L.Sampler(seed=1000 + i, repeat_last_n=64) for i in range(n)]
    m.decode_greedy_multi(firsts[:n], n_past, steps, 8)                                  # warm-up: graph captures, workspaces
    m.decode_sample_multi(firsts[:n], n_past, steps, samplers)
    t_g, t_s, exact = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        m.decode_greedy_multi(firsts[:n], n_past, steps, 8)
        t_g.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        _, ex = m.decode_sample_multi(firsts[:n], n_past, steps, samplers, want_exact=True)
        t_s.append(time.perf_counter() - t0)
        exact.append(float(ex.mean()))
    g, s = n * steps / statistics.median(t_g), n * steps / statistics.median(t_s)
    return {"n_seqs": n, "steps": steps, "reps": reps, "greedy_tok_s": round(g, 1), "sample_tok_s": round(s, 1),
            "sample_cost_pct": round(100.0 * (1.0 - s / g), 2), "host_path_share": round(1.0 - statistics.mean(exact), 4),
            "greedy_ms_per_step": round(1e3 * statistics.median(t_g) / steps, 3), "sample_ms_per_step": round(1e3 * statistics.median(t_s) / steps, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", default="1,2,4,8,16,32")
    ap.add_argument("--stages", default="1,2")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--one", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    path = bench.model_path("7B", bench.MODELS["7B"], 20230312)
    if a.one:
        with L.Model(path, n_ctx=N_CTX, n_seq=a.one) as m:
            firsts = prepare(m, a.one)
            samplers = [L.Sampler(seed=1000 + i, repeat_last_n=64) for i in range(a.one)]
            m.decode_sample_multi(firsts, [PROMPT] * a.one, a.steps, samplers)
            _, ex = m.decode_sample_multi(firsts, [PROMPT] * a.one, a.steps, samplers, want_exact=True)
            print(json.dumps({"probe": "sample_multi_one", "n_seqs": a.one, "steps": a.steps, "exact_share": float(ex.mean())}))
        return
    seqs = [int(x) for x in a.seqs.split(",")]
    results = []
    for S in (int(x) for x in a.stages.split(",")):
        with L.Model(path, n_ctx=N_CTX, n_seq=max(seqs), devices=[0] * S if S > 1 else None) as m:
            firsts = prepare(m, max(seqs))
            for n in seqs:
                r = dict(probe="sample_multi_probe", handle="plain" if S == 1 else f"{S}_stages_one_gpu", **run_case(m, firsts, n, a.steps, a.reps))
                print(json.dumps(r), flush=True)
                results.append(r)
    line = json.dumps({"probe": "sample_multi_probe", "model": "7B synthetic Q4_0", "sampler": "repeat_penalty 1.3, top_k 40, top_p 0.95, temp 0.8, window 64",
                       "results": results})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
