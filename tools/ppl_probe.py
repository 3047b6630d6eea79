"""Cost of scoring a text on the synthetic 7B Q4_0 file bench.py makes: llamahip_perplexity over 512-token windows against the same
511 tokens through llamahip_eval_chunks (one eval, last row of logits only), alternated in one process.  Prints one JSON line.

    python tools/ppl_probe.py [--reps 12] [--out FILE]
    python tools/ppl_probe.py --one-window          (one warm-up window, then one window: for rocprofv3 --kernel-trace --stats)
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

import bench  # noqa: E402
import llama_swift_amd as L  # noqa: E402
import synth  # noqa: E402

W = 512


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--one-window", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    path = bench.model_path("7B", bench.MODELS["7B"], 20230312)
    m = L.Model(path, n_ctx=W)
    toks = synth.synth_prompt(W, m.n_vocab, seed=7)
    if a.one_window:
        m.perplexity(toks, window=W)
        r = m.perplexity(toks, window=W)
        print(json.dumps({"probe": "ppl_one_window", "ppl": r["ppl"], "n_scored": r["n_scored"]}))
        return
    # warm-up: workspaces, the prompt copies of the layer matrices and of the lm head
    m.perplexity(toks, window=W)
    m.eval_chunks(toks[:W - 1], 0, chunk_tokens=W - 1)
    t_ppl, t_eval = [], []
    r = None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        r = m.perplexity(toks, window=W)
        t_ppl.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        m.eval_chunks(toks[:W - 1], 0, chunk_tokens=W - 1)
        t_eval.append((time.perf_counter() - t0) * 1e3)
    scored = r["n_scored"]
    out = {
        "probe": "ppl_probe", "model": "7B synthetic Q4_0", "window": W, "n_scored_per_window": scored,
        "ms_per_window_perplexity": spread(t_ppl), "ms_eval_chunks_last_row": spread(t_eval),
        "scored_tokens_per_s": scored / (statistics.median(t_ppl) / 1e3),
        "ratio_perplexity_over_eval": statistics.median(t_ppl) / statistics.median(t_eval),
        "ppl": r["ppl"],
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    m.close()


if __name__ == "__main__":
    main()
