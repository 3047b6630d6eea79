#!/usr/bin/env python3
"""The request scheduler (llamahip_sched_*) against what the library offers without it, on the synthetic 7B file.
usage: sched_probe.py [--json OUT] [--budgets 16,32,64,128,256] [--repeats 3] [--requests 64]

Workload: n_ctx 512, 16 KV slots, chunks of 9, 8 threads, greedy.  64 requests from a fixed seed: prompt lengths cycle through 9, 18, 36, 72, 144
and 288 tokens; n_predict is a seeded permutation of 8, 16, 32, 64, 128 and 256 per cycle, capped at 224 = n_ctx - the longest prompt, so
that a static wave (below) fits the context whatever it holds.
Scheduler: all requests submitted at once, max_active 16, stepped until nothing is pending; every step is timed on its own.
Baseline, in the same process, on the same handle: waves of 16 requests in submission order -- llamahip_eval_multi over the wave's prompts,
then llamahip_decode_greedy_multi with n_steps = the wave's largest n_predict - 1 (every sequence is stepped to the end of the wave; only the
tokens a request asked for are counted).
The runs are interleaved (baseline, then every budget, `repeats` times over) after one untimed run of each.  Reported per configuration:
median and min .. max of the aggregate tokens/s, the longest single step (what a decoding conversation waits while a prompt is admitted), the
steps by kind, rows, graph captures; and what a capture costs: a set step that captured graphs against the next replayed set step of the same
row count in the same run.
LLAMAHIP_SCHED_ROW_BUDGET is the candidate with the highest median tokens/s; of candidates within the runs' spread of it, the smallest.

sched_probe.py --draft [--json OUT] [--repeats 3] [--alter 2,5] [--parent-root DIR] [--parent-runs 5]
Drafted tokens inside the scheduler (llamahip_sched_opts.draft_len) on the same workload at LLAMAHIP_SCHED_ROW_BUDGET: draft_len 0 against
LLAMAHIP_LOOKUP_DRAFT_LEN with three kinds of corpus -- none (the requests' own histories only); every request's own plain-run output (every
draft from it is accepted); that output with every k-th token altered, for each k of --alter.  One process, one handle, the configurations
interleaved `repeats` times after one untimed run of each; every run's tokens must be the plain run's.  Reported per configuration: aggregate
tokens/s, the longest step, steps, drafted / accepted, and the acceptance rate from which drafting pays (the plain run's tokens/s, interpolated
in acceptance rate between the configurations that draft from a corpus).
--parent-root DIR: a tree of the parent commit with its library built (python package and libllamahip.so).  The draft_len == 0 scheduler of
this tree against that tree's, each run in a fresh process (--one-plain-run, one untimed run, then the timed one), interleaved, --parent-runs
each: both medians, both min .. max spreads, and whether the medians differ by less than the parent's own spread.

sched_probe.py --shared-prefix N [--json OUT] [--repeats 5] [--parent-root DIR] [--parent-runs 5]
Shared prompt prefixes (llamahip_sched_opts.prefix_share): the same 64 requests with one common N-token system prompt in front of every
prompt, n_ctx raised by N to fit, row_budget LLAMAHIP_SCHED_ROW_BUDGET.  prefix_share off and on in one process on one handle, interleaved
`repeats` times after one untimed run of each, for two arrival patterns -- all 64 at once (the first 16 find nothing held; everybody later finds
the system prompt in the slot it takes) and the first request alone until its first token, then the other 63 (the next 15 copy its rows);
the tokens of every run must be the first run's.  Reported per configuration: aggregate
tokens/s, steps, the longest step, n_prompt_rows / n_shared_rows / n_copied_rows / n_copy_launches and the mean number of steps from
submit to a request's first token.  Before that, the copy itself against the obvious alternative (llamahip_bench_kv_copy): one
k_kv_copy_rows launch against a loop of hipMemcpyAsync calls over the same ranges of every layer, K and V, on the same stream -- one copy of 9
rows (launch-bound), one of 256 rows (bandwidth-bound), 256 rows broadcast to 15 destinations; interleaved, `repeats` runs of 20 calls each.
--parent-root DIR: as for --draft -- the standard workload (no shared prefix, prefix_share 0) of this tree against the parent's, fresh processes."""
import json, os, statistics, subprocess, sys, time
ROOT = os.environ.get("LLAMAHIP_PROBE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # (--one-plain-run on the parent's tree)
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

args = sys.argv[1:]
opt = lambda k, d: args[args.index(k) + 1] if k in args else d
BUDGETS = [int(x) for x in opt("--budgets", "16,32,64,128,256").split(",")]
REPEATS, N_REQ = int(opt("--repeats", "3")), int(opt("--requests", "64"))
MODEL = os.path.join(os.environ.get("LLAMAHIP_MODEL_DIR", "/tmp/llamahip_models"), "7B-seed20230312", "ggml-model-q4_0.bin")
N_CTX, SLOTS, CHUNK, NTH = 512, 16, 9, 8
LENS, PREDICTS = (9, 18, 36, 72, 144, 288), (8, 16, 32, 64, 128, 256)


def workload(np, n_vocab):
    rng = np.random.default_rng(20240611)
    reqs = []
    for i in range(N_REQ):
        if i % len(PREDICTS) == 0:
            perm = rng.permutation(PREDICTS)
        n = LENS[i % len(LENS)]
        prompt = np.concatenate([[1], rng.integers(3, n_vocab, n - 1)]).astype(np.int32)
        reqs.append((prompt, int(min(perm[i % len(PREDICTS)], N_CTX - max(LENS)))))
    return reqs


def timed_run(m, reqs, budget, **kw):
    """one scheduler run over the workload: (wall seconds, longest step in ms, stats, tokens per request)"""
    out, longest = {}, 0.0
    with m.scheduler(max_active=SLOTS, chunk_tokens=CHUNK, row_budget=budget, n_threads=NTH, **kw) as sc:
        ids = [sc.submit(p, k) for p, k in reqs]
        t_all = time.perf_counter()
        while sc.pending():
            t0 = time.perf_counter()
            ev = sc.step()
            longest = max(longest, (time.perf_counter() - t0) * 1e3)
            for e in ev:
                if e["kind"] == "token":
                    out.setdefault(e["id"], []).append(e["token"])
        wall = time.perf_counter() - t_all
        st = sc.stats()
    return wall, longest, st, [out[i] for i in ids]


def one_plain_run():
    """--one-plain-run: the draft_len == 0 scheduler of the tree at ROOT in this fresh process; one JSON line"""
    import numpy as np
    import llama_swift_amd as L
    m = L.Model(MODEL, n_ctx=N_CTX, n_seq=SLOTS)
    reqs = workload(np, m.n_vocab)
    timed_run(m, reqs, 256)
    wall, longest, st, toks = timed_run(m, reqs, 256)
    print(json.dumps({"tokens_per_s": sum(k for _, k in reqs) / wall, "longest_step_ms": longest, "n_steps": st["n_steps"], "library": L.LIB_PATH,
                      "tokens_crc": int(np.bitwise_xor.reduce(np.concatenate([np.asarray(t, np.int64) * (i + 1) for i, t in enumerate(toks)])))}), flush=True)
    m.close()


def main_draft():
    import numpy as np
    import llama_swift_amd as L
    subprocess.run(["bash", os.path.join(HERE, "tools", "ensure_7b.sh")], cwd=HERE, check=True)
    m = L.Model(MODEL, n_ctx=N_CTX, n_seq=SLOTS)
    reqs = workload(np, m.n_vocab)
    asked = sum(k for _, k in reqs)
    budget, draft_len = 256, 15          # LLAMAHIP_SCHED_ROW_BUDGET, LLAMAHIP_LOOKUP_DRAFT_LEN
    _, _, _, want = timed_run(m, reqs, budget)
    own = np.concatenate([np.concatenate([p[-1:], np.asarray(t, np.int32)]) for (p, _), t in zip(reqs, want)]).astype(np.int32)
    configs = [("draft_len 0", {}), ("no corpus", dict(draft_len=draft_len)), ("own output", dict(draft_len=draft_len, corpus=own))]
    for k in [int(x) for x in opt("--alter", "2,5").split(",")]:
        c = own.copy()
        c[k - 1::k] = (c[k - 1::k] + 1) % m.n_vocab
        configs.append((f"own output, every {k}th token altered", dict(draft_len=draft_len, corpus=c)))
    for name, kw in configs:          # one untimed run of each; the tokens are the plain run's whatever is drafted
        assert timed_run(m, reqs, budget, **kw)[3] == want, f"{name}: the tokens are not the plain run's"
    runs = {name: [] for name, _ in configs}
    for _ in range(REPEATS):
        for name, kw in configs:
            runs[name].append(timed_run(m, reqs, budget, **kw)[:3])
    spread = lambda xs: {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}
    res = {"model": "7B synthetic (seed 20230312), Q4_0", "n_ctx": N_CTX, "max_active": SLOTS, "chunk_tokens": CHUNK, "n_threads": NTH, "row_budget": budget,
           "draft_len": draft_len, "requests": N_REQ, "tokens_asked": int(asked), "repeats": REPEATS, "library": os.path.basename(L.LIB_PATH),
           "method": "one process, one handle; the configurations interleaved, `repeats` times, after one untimed run of each; wall time around the whole run and around every step",
           "configs": []}
    for name, _ in configs:
        st = runs[name][-1][2]
        row = {"corpus": name, "tokens_per_s": spread([asked / w for w, _, _ in runs[name]]), "longest_step_ms": spread([l for _, l, _ in runs[name]]),
               "steps": st["n_steps"], "draft_steps": st.get("n_draft_steps", 0), "drafted": st.get("n_drafted", 0), "accepted": st.get("n_accepted", 0),
               "acceptance": round(st.get("n_accepted", 0) / max(st.get("n_drafted", 0), 1), 4), "rows": st["n_rows"]}
        res["configs"].append(row)
        print(f"{name:40s} {row['tokens_per_s']} tokens/s | longest step {row['longest_step_ms']['median']} ms | {row['steps']} steps | "
              f"{row['accepted']} / {row['drafted']} accepted ({row['acceptance']})", flush=True)
    # from which acceptance rate drafting pays: the plain median, interpolated between the drafting configurations in acceptance rate
    plain = res["configs"][0]["tokens_per_s"]["median"]
    # (the corpus configurations only: they draft at every opportunity, so their cost per step is the same and the acceptance rate is what differs)
    pts = sorted((r["acceptance"], r["tokens_per_s"]["median"]) for r in res["configs"][2:] if r["drafted"] > 0)
    be = None
    for (a0, t0), (a1, t1) in zip(pts, pts[1:]):
        if (t0 - plain) * (t1 - plain) <= 0 and t1 != t0:
            be = round(a0 + (plain - t0) * (a1 - a0) / (t1 - t0), 3)
    res["break_even"] = {"plain_tokens_per_s": plain, "points": pts, "acceptance": be,
                         "note": "acceptance rate at which the interpolated tokens/s equals the plain run's; null: not bracketed by the measured points "
                                 + ("(drafting paid at every one)" if pts and min(t for _, t in pts) > plain else "(drafting paid at none)" if pts and max(t for _, t in pts) < plain else "")}
    print("break-even:", res["break_even"], flush=True)
    m.close()
    parent = opt("--parent-root", "")
    res["draft_len_0_against_parent"] = None
    if parent:
        n_runs = int(opt("--parent-runs", "5"))
        got = {"this": [], "parent": []}
        for _ in range(n_runs):
            for who, root in (("parent", os.path.abspath(parent)), ("this", HERE)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-plain-run"], env={**os.environ, "LLAMAHIP_PROBE_ROOT": root},
                                   capture_output=True, text=True, timeout=600)
                assert r.returncode == 0, r.stderr[-2000:]
                got[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
        assert len({x["tokens_crc"] for v in got.values() for x in v}) == 1, "the two libraries produced different tokens"
        assert got["parent"][0]["library"] != got["this"][0]["library"]
        tp, tt = spread([x["tokens_per_s"] for x in got["parent"]]), spread([x["tokens_per_s"] for x in got["this"]])
        res["draft_len_0_against_parent"] = {
            "method": f"fresh processes, interleaved, {n_runs} each; in each one untimed run, then the timed one", "parent_tokens_per_s": tp, "this_tokens_per_s": tt,
            "parent_longest_step_ms": spread([x["longest_step_ms"] for x in got["parent"]]), "this_longest_step_ms": spread([x["longest_step_ms"] for x in got["this"]]),
            "median_difference": round(tt["median"] - tp["median"], 3), "parent_spread": round(tp["max"] - tp["min"], 3),
            "unchanged_within_the_parents_spread": abs(tt["median"] - tp["median"]) <= tp["max"] - tp["min"]}
        print("draft_len 0 against the parent:", res["draft_len_0_against_parent"], flush=True)
    if "--json" in args:
        with open(opt("--json", ""), "w") as f:
            json.dump(res, f, indent=1)


def parent_comparison(spread):
    """the plain scheduler of this tree against the tree at --parent-root: fresh processes, interleaved (None without --parent-root)"""
    parent = opt("--parent-root", "")
    if not parent:
        return None
    n_runs = int(opt("--parent-runs", "5"))
    got = {"this": [], "parent": []}
    for _ in range(n_runs):
        for who, root in (("parent", os.path.abspath(parent)), ("this", HERE)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-plain-run"], env={**os.environ, "LLAMAHIP_PROBE_ROOT": root},
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            got[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert len({x["tokens_crc"] for v in got.values() for x in v}) == 1, "the two libraries produced different tokens"
    assert got["parent"][0]["library"] != got["this"][0]["library"]
    tp, tt = spread([x["tokens_per_s"] for x in got["parent"]]), spread([x["tokens_per_s"] for x in got["this"]])
    return {"method": f"fresh processes, interleaved, {n_runs} each; in each one untimed run, then the timed one", "parent_tokens_per_s": tp, "this_tokens_per_s": tt,
            "parent_longest_step_ms": spread([x["longest_step_ms"] for x in got["parent"]]), "this_longest_step_ms": spread([x["longest_step_ms"] for x in got["this"]]),
            "median_difference": round(tt["median"] - tp["median"], 3), "parent_spread": round(tp["max"] - tp["min"], 3),
            "unchanged_within_the_parents_spread": abs(tt["median"] - tp["median"]) <= tp["max"] - tp["min"]}


def main_prefix():
    import numpy as np
    import llama_swift_amd as L
    subprocess.run(["bash", os.path.join(HERE, "tools", "ensure_7b.sh")], cwd=HERE, check=True)
    n_sys, repeats, budget = int(opt("--shared-prefix", "256")), int(opt("--repeats", "5")), 256
    m = L.Model(MODEL, n_ctx=N_CTX + n_sys, n_seq=SLOTS)
    rng = np.random.default_rng(20250131)
    system = np.concatenate([[1], rng.integers(3, m.n_vocab, n_sys - 1)]).astype(np.int32)
    reqs = [(np.concatenate([system, p[1:] if len(p) > 1 else p]).astype(np.int32), k) for p, k in workload(np, m.n_vocab)]
    asked = sum(k for _, k in reqs)
    spread = lambda xs: {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}
    res = {"model": "7B synthetic (seed 20230312), Q4_0", "n_ctx": N_CTX + n_sys, "max_active": SLOTS, "chunk_tokens": CHUNK, "n_threads": NTH, "row_budget": budget,
           "shared_prefix_tokens": n_sys, "requests": N_REQ, "prompt_tokens": int(sum(len(p) for p, _ in reqs)), "tokens_asked": int(asked), "repeats": repeats,
           "library": os.path.basename(L.LIB_PATH)}
    # the copy alone: rows that hold something (one eval of the system prompt in slot 0), then each case both ways, interleaved
    m.set_seq(0)
    m.eval_chunks(system, 0, CHUNK, NTH)
    cases = [("one copy of 9 rows", [(0, 1, 0, 9)]), (f"one copy of {n_sys} rows", [(0, 1, 0, n_sys)]),
             (f"{n_sys} rows broadcast to 15 destinations", [(0, d, 0, n_sys) for d in range(1, SLOTS)])]
    res["copy"] = {"method": f"llamahip_bench_kv_copy: host wall time per enqueue + stream wait, the mean of 20 calls after one untimed call; kernel and loop interleaved, {repeats} runs each",
                   "cases": []}
    for name, copies in cases:
        t = {0: [], 1: []}
        for _ in range(repeats):
            for how in (0, 1):
                t[how].append(m.bench_kv_copy(copies, how, 20) * 1e3)
        rows = sum(c[3] for c in copies)
        nbytes = rows * m.n_embd * 4 * 2 * m.n_layer
        k, l = spread(t[0]), spread(t[1])
        row = {"case": name, "ranges": len(copies) * 2 * m.n_layer, "bytes_moved": int(nbytes), "k_kv_copy_rows_us": k, "hipMemcpyAsync_loop_us": l,
               "kernel_GBps_read_plus_write": round(2 * nbytes / (k["median"] * 1e-6) / 1e9, 1), "loop_spread_us": round(l["max"] - l["min"], 3),
               "kernel_not_slower_by_more_than_the_loops_spread": k["median"] <= l["median"] + (l["max"] - l["min"])}
        res["copy"]["cases"].append(row)
        print(f"{name:45s} kernel {k} us | memcpy loop {l} us | {row['kernel_GBps_read_plus_write']} GB/s", flush=True)

    def run(share, warm):
        """warm: the first request alone until its first token, then the other 63 at once (they find its rows and copy them); else all at once"""
        out, first, sub_at, longest, n_step = {}, {}, {}, 0.0, 0
        with m.scheduler(max_active=SLOTS, chunk_tokens=CHUNK, row_budget=budget, n_threads=NTH, prefix_share=share) as sc:
            ids = []
            todo = list(reqs)
            t_all = time.perf_counter()
            while todo or sc.pending():
                if todo and (not warm or not ids or ids[0] in first):
                    for p, k in (todo if ids or not warm else todo[:1]):
                        ids.append(sc.submit(p, k))
                        sub_at[ids[-1]] = n_step
                    todo = reqs[len(ids):]
                t0 = time.perf_counter()
                ev = sc.step()
                longest = max(longest, (time.perf_counter() - t0) * 1e3)
                n_step += 1
                for e in ev:
                    if e["kind"] == "token":
                        out.setdefault(e["id"], []).append(e["token"])
                        first.setdefault(e["id"], n_step - sub_at[e["id"]])
            wall = time.perf_counter() - t_all
            st = sc.stats()
        return wall, longest, st, [out[i] for i in ids], statistics.mean(first[i] for i in ids)

    configs = [(False, False), (True, False), (False, True), (True, True)]
    want = run(False, False)[3]
    for share, warm in configs[1:]:
        assert run(share, warm)[3] == want, "prefix_share or the arrival order changed a request's tokens"
    runs = {c: [] for c in configs}
    for _ in range(repeats):
        for c in configs:
            r = run(*c)
            assert r[3] == want, "a run's tokens are not the first run's"
            runs[c].append(r)
    res["scheduler"] = {"method": "one process, one handle; the configurations interleaved, `repeats` times, after one untimed run of each; wall time around the whole run "
                                  "(submissions included) and around every step",
                        "configs": []}
    for c in configs:
        st = runs[c][-1][2]
        row = {"prefix_share": int(c[0]), "arrival": "the first request alone until its first token, then the other 63" if c[1] else "all 64 at once",
               "tokens_per_s": spread([asked / r[0] for r in runs[c]]), "longest_step_ms": spread([r[1] for r in runs[c]]),
               "steps": st["n_steps"], "mixed_steps": st["n_mixed_steps"], "rows": st["n_rows"], "prompt_rows": st["n_prompt_rows"],
               "shared_rows": st["n_shared_rows"], "copied_rows": st["n_copied_rows"], "copy_launches": st["n_copy_launches"],
               "mean_steps_to_first_token": round(runs[c][-1][4], 2)}
        res["scheduler"]["configs"].append(row)
        print(f"prefix_share {row['prefix_share']}, {row['arrival']}: {row['tokens_per_s']} tokens/s | {row['steps']} steps | longest step {row['longest_step_ms']['median']} ms | "
              f"prompt rows {row['prompt_rows']} shared {row['shared_rows']} copied {row['copied_rows']} in {row['copy_launches']} launches | "
              f"{row['mean_steps_to_first_token']} steps to the first token", flush=True)
    m.close()
    res["prefix_share_0_against_parent"] = parent_comparison(spread)
    print("prefix_share 0, standard workload, against the parent:", res["prefix_share_0_against_parent"], flush=True)
    if "--json" in args:
        with open(opt("--json", ""), "w") as f:
            json.dump(res, f, indent=1)


def main():
    import numpy as np
    import llama_swift_amd as L
    subprocess.run(["bash", os.path.join(ROOT, "tools", "ensure_7b.sh")], cwd=ROOT, check=True)
    m = L.Model(MODEL, n_ctx=N_CTX, n_seq=SLOTS)
    reqs = workload(np, m.n_vocab)
    asked = sum(k for _, k in reqs)

    def run_sched(budget):
        steps, out = [], {}
        with m.scheduler(max_active=SLOTS, chunk_tokens=CHUNK, row_budget=budget, n_threads=NTH) as sc:
            ids = [sc.submit(p, k) for p, k in reqs]
            before = sc.stats()
            t_all = time.perf_counter()
            while sc.pending():
                t0 = time.perf_counter()
                ev = sc.step()
                dt = (time.perf_counter() - t0) * 1e3
                st = sc.stats()
                kind = next(k for k in ("mixed", "set", "single", "fallback") if st[f"n_{k}_steps"] != before[f"n_{k}_steps"])
                steps.append((kind, dt, st["n_graph_captures"] - before["n_graph_captures"], st["n_rows"] - before["n_rows"]))
                before = st
                for e in ev:
                    if e["kind"] == "token":
                        out.setdefault(e["id"], []).append(e["token"])
            wall = time.perf_counter() - t_all
        toks = [out[i] for i in ids]
        assert [len(t) for t in toks] == [k for _, k in reqs]
        return wall, steps, st, toks

    def run_waves():
        toks, t_eval, t_dec, n_steps_all = [], 0.0, 0.0, 0
        t_all = time.perf_counter()
        for w0 in range(0, N_REQ, SLOTS):
            wave = reqs[w0:w0 + SLOTS]
            t0 = time.perf_counter()
            lg = m.eval_multi(list(range(len(wave))), [0] * len(wave), [p for p, _ in wave], chunk_tokens=CHUNK, n_threads=NTH)
            t1 = time.perf_counter()
            first = [int(np.argmax(lg[i])) for i in range(len(wave))]
            n_steps = max(k for _, k in wave) - 1
            rest = m.decode_greedy_multi(first, [len(p) for p, _ in wave], n_steps, n_threads=NTH) if n_steps > 0 else np.zeros((len(wave), 0), np.int32)
            t_dec += time.perf_counter() - t1
            t_eval += t1 - t0
            n_steps_all += n_steps
            toks += [[first[i]] + rest[i, :k - 1].tolist() for i, (_, k) in enumerate(wave)]
        return time.perf_counter() - t_all, t_eval, t_dec, n_steps_all, toks

    # one untimed run of each (graphs captured, workspaces grown), and the two ways must produce the same tokens
    _, _, _, _, want = run_waves()
    for b in BUDGETS:
        _, _, _, got = run_sched(b)
        assert got == want, f"row_budget {b}: the scheduler's tokens are not the static waves'"
    base, runs = [], {b: [] for b in BUDGETS}
    for _ in range(REPEATS):
        base.append(run_waves()[:4])
        for b in BUDGETS:
            runs[b].append(run_sched(b)[:3])
    spread = lambda xs: {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}
    res = {"model": "7B synthetic (seed 20230312), Q4_0", "n_ctx": N_CTX, "max_active": SLOTS, "chunk_tokens": CHUNK, "n_threads": NTH,
           "requests": N_REQ, "prompt_tokens": int(sum(len(p) for p, _ in reqs)), "tokens_asked": int(asked), "repeats": REPEATS,
           "library": os.path.basename(L.LIB_PATH),
           "method": "one process, one handle; static waves and every budget interleaved, `repeats` times, after one untimed run of each; wall time around the whole run and around every scheduler step",
           "static_waves": {"tokens_per_s": spread([asked / w for w, _, _, _ in base]), "eval_multi_s": spread([e for _, e, _, _ in base]),
                            "decode_multi_s": spread([d for _, _, d, _ in base]), "set_steps": base[0][3]},
           "scheduler": []}
    print(f"static waves: {res['static_waves']['tokens_per_s']} tokens/s, {base[0][3]} set steps", flush=True)
    for b in BUDGETS:
        tps = [asked / w for w, _, _ in runs[b]]
        steps, st = runs[b][-1][1], runs[b][-1][2]
        by = {k: [dt for kk, dt, _, _ in steps if kk == k] for k in ("mixed", "set", "single")}
        # what a capture costs: a set step that captured graphs against the next replayed (already captured) set step of the same row count in the same run
        capt = []
        for r in runs[b]:
            ss = [x for x in r[1] if x[0] == "set"]
            for i, (_, dt, c, rows) in enumerate(ss):
                nxt = [x for x in ss[i + 1:i + 4] if x[2] == 0 and x[3] == rows]
                if c > 0 and nxt:
                    capt.append((dt - nxt[0][1]) / c)
        row = {"row_budget": b, "tokens_per_s": spread(tps), "longest_step_ms": spread([max(dt for _, dt, _, _ in r[1]) for r in runs[b]]),
               "steps": {k: len(v) for k, v in by.items()}, "step_ms_median": {k: round(statistics.median(v), 3) for k, v in by.items() if v},
               "mixed_step_rows_max": max([r for k, _, _, r in steps if k == "mixed"] or [0]),
               "rows": st["n_rows"], "prompt_rows": st["n_prompt_rows"], "graph_captures_per_run": [r[2]["n_graph_captures"] for r in runs[b]],
               "capture_ms": spread(capt) if capt else None, "captures_timed": len(capt),
               "capture_share_of_wall": round(sum(capt) / 1e3 / sum(w for w, _, _ in runs[b]), 4) if capt else 0.0}
        res["scheduler"].append(row)
        print(f"budget {b:3d}: {row['tokens_per_s']} tokens/s | longest step {row['longest_step_ms']['median']} ms | steps {row['steps']} "
              f"| captures {row['graph_captures_per_run']} at {row['capture_ms']} ms", flush=True)
    best = max(res["scheduler"], key=lambda r: r["tokens_per_s"]["median"])
    near = [r for r in res["scheduler"] if r["tokens_per_s"]["median"] >= best["tokens_per_s"]["median"] - (best["tokens_per_s"]["max"] - best["tokens_per_s"]["min"])]
    res["choice"] = {"row_budget": min(r["row_budget"] for r in near), "best_median": best["row_budget"],
                     "rule": "highest median tokens/s; of the candidates within the best one's min .. max spread of it, the smallest (shorter stalls)"}
    print("choice:", res["choice"], flush=True)
    if "--json" in args:
        with open(opt("--json", ""), "w") as f:
            json.dump(res, f, indent=1)
    m.close()


if __name__ == "__main__":
    one_plain_run() if "--one-plain-run" in args else main_prefix() if "--shared-prefix" in args else main_draft() if "--draft" in args else main()
