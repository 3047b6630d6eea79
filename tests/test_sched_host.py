"""CPU: the request scheduler's host half (csrc/sched.cpp; include/llamahip.h "request scheduler").

The step rule llamahip_sched_plan against a Python restatement of the issue's text over a grid, and its properties over whole drains
(progress, chunk alignment, a single overshoot of the budget per step); what llamahip_sched_new refuses, on a HOST_ONLY handle and
without a device (every argument first, the handle last -- so llamahip_sched_submit's refusals, which need a scheduler, are exercised in the
stand-alone sanitizer program against a stubbed device half, together with whole scheduler runs on exactly sized arrays); the exports;
`make asan`."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import synth

LENS = (0, 1, 3, 9, 10, 27, 61, 100)
CHUNKS = (0, 1, 4, 9)
BUDGETS = (1, 8, 16, 17, 64)


def plan_ref(left, c, budget):
    """the step rule restated (the yardstick): rows per sequence for sequences in admission order, left[i] prompt tokens to go, 0 = decoding"""
    rest = budget - sum(1 for x in left if x == 0)
    rows, given, stopped = [], False, False
    for x in left:
        if x == 0:
            rows.append(1)
            continue
        if stopped:
            rows.append(0)
            continue
        r = min(x, max(rest, 0) // c * c) if c > 0 else (x if x <= rest else 0)
        if r < 1:
            if not given:
                r = min(x, c) if c > 0 else x          # the progress guarantee: the only way past the budget
            else:
                stopped = True
                r = 0
        if r > 0:
            given = True
            rest -= r
        rows.append(r)
    return rows


def test_plan_is_the_restated_rule_over_the_grid(L):
    rng = np.random.default_rng(11)
    n_checked = 0
    for c, budget in itertools.product(CHUNKS, BUDGETS):
        for n in range(0, 17):
            for _ in range(12):
                left = [int(LENS[k]) for k in rng.integers(0, len(LENS), n)]
                total, rows = L.sched_plan(left, c, budget)
                want = plan_ref(left, c, budget)
                assert rows.tolist() == want and total == sum(want), (c, budget, left, rows.tolist(), want)
                n_checked += 1
        # every single length alone, and the all-decoding set
        for x in LENS:
            total, rows = L.sched_plan([x], c, budget)
            assert rows.tolist() == plan_ref([x], c, budget)
        assert L.sched_plan([0] * 16, c, budget)[1].tolist() == [1] * 16
    assert n_checked == len(CHUNKS) * len(BUDGETS) * 17 * 12


def test_plan_refuses_bad_arguments(L):
    assert L.sched_plan([3], 0, 0)[0] == -1            # row_budget < 1
    assert L.sched_plan([3], -1, 8)[0] == -1           # chunk_tokens < 0
    assert L.sched_plan([-1], 0, 8)[0] == -1           # a negative entry
    assert L.sched_plan([1] * 17, 0, 8)[0] == -1       # more than 16 sequences
    assert L.sched_plan([], 0, 8)[0] == 0              # nobody active: nothing to run
    assert L.lib().llamahip_sched_plan(1, None, 0, 8, None) == -1


@pytest.mark.parametrize("c", CHUNKS)
@pytest.mark.parametrize("budget", BUDGETS)
def test_a_whole_drain_makes_progress_aligned_and_overshoots_once(L, c, budget):
    """16 slots fed from a queue of prompts; every sequence decodes a few tokens after its prompt.  Every step: some row runs; every piece
    starts at a multiple of c and ends at one or at the prompt's end; the budget is exceeded only by the one piece of the progress
    guarantee (and then nobody else prefills); the oldest prefilling sequence is never starved; the drain terminates."""
    rng = np.random.default_rng(100 * c + budget)
    queue = [int(x) for x in rng.choice([x for x in LENS if x > 0], 40)]
    act = []          # [prompt_len, offset, tokens_to_decode]
    steps = 0
    while queue or act:
        while queue and len(act) < 16:
            act.append([queue.pop(0), 0, int(rng.integers(1, 6))])
        left = [a[0] - a[1] for a in act]
        total, rows = L.sched_plan(left, c, budget)
        rows = rows.tolist()
        assert total == sum(rows) and total >= 1, (left, rows)
        n_dec = sum(1 for x in left if x == 0)
        pre = [(i, r) for i, r in enumerate(rows) if left[i] > 0 and r > 0]
        if any(x > 0 for x in left):
            first = next(i for i, x in enumerate(left) if x > 0)
            assert rows[first] > 0, ("the oldest prefilling sequence got nothing", left, rows)
        if total > budget and n_dec < budget:
            assert len(pre) == 1 and pre[0][1] == (min(left[pre[0][0]], c) if c else left[pre[0][0]]), (left, rows)
        if total > budget and n_dec >= budget:
            assert len(pre) <= 1
        for i, r in pre:
            off = act[i][1]
            if c:
                assert off % c == 0 and ((off + r) % c == 0 or off + r == act[i][0]), (c, off, r, act[i])
            else:
                assert off == 0 and r == act[i][0]
        for i, r in enumerate(rows):
            if left[i] == 0:
                assert r == 1
                act[i][2] -= 1
            else:
                act[i][1] += r
                if act[i][1] == act[i][0]:
                    act[i][2] -= 1          # the piece that ends the prompt emits the first token
        act = [a for a in act if a[2] > 0]
        steps += 1
        assert steps < 5000
    assert steps > 0


def _opts(L, **kw):
    b = L.binding
    o = b._SchedOpts(C.sizeof(b._SchedOpts), 2, 2, 0, 0, 1.3, 0.95, 0.8, 40)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _new(L, model, o):
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    rc = L.lib().llamahip_sched_new(model._h if model is not None else None, C.byref(o), C.byref(h), err, len(err))
    return rc, h.value, err.value.decode()


@pytest.fixture(scope="module")
def host_only(L, tmp_path_factory):
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    path = str(tmp_path_factory.mktemp("sched") / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    return L.Model(path, n_ctx=64, flags=4, n_seq=4)          # LLAMAHIP_FLAG_HOST_ONLY: no device is touched


def test_sched_new_refusals_name_their_limit_and_touch_no_device(L, host_only):
    ERR = L.binding.ERR_PREDICT
    for kw, word in ((dict(max_active=0), "max_active"), (dict(max_active=17), "max_active"), (dict(chunk_tokens=-1), "chunk_tokens"),
                     (dict(row_budget=-1), "row_budget"), (dict(row_budget=2048 - 15), "row_budget"), (dict(top_k=0), "top_k"),
                     (dict(temp=0.0), "temp"), (dict(temp=-1.0), "temp"), (dict(repeat_penalty=0.0), "repeat_penalty"),
                     (dict(top_p=float("nan")), "top_p"), (dict(struct_size=8), "struct_size")):
        rc, h, msg = _new(L, host_only, _opts(L, **kw))
        assert rc == ERR and not h and word in msg, (kw, msg)
    # every argument in range: the handle is what is refused, last
    rc, h, msg = _new(L, host_only, _opts(L))
    assert rc == ERR and not h and "HOST_ONLY" in msg, msg
    rc, h, msg = _new(L, host_only, _opts(L, row_budget=2048 - 16))
    assert rc == ERR and "HOST_ONLY" in msg, msg
    rc, h, msg = _new(L, None, _opts(L))
    assert rc == ERR and "null model" in msg, msg
    with pytest.raises(L.LlamaHipError) as e:
        host_only.scheduler(max_active=2)
    assert e.value.code == ERR and "HOST_ONLY" in e.value.message
    # the entry points on a null scheduler
    lib = L.lib()
    err = C.create_string_buffer(256)
    n = C.c_int32(7)
    assert lib.llamahip_sched_submit(None, None, None, err, len(err)) == ERR
    assert lib.llamahip_sched_step(None, None, 64, C.byref(n), err, len(err)) == ERR and n.value == 0
    assert lib.llamahip_sched_cancel(None, 1) == -1 and lib.llamahip_sched_pending(None) == 0
    lib.llamahip_sched_free(None)


def test_new_symbols_are_declared_and_exported(L, built):
    names = L.declared_symbols()
    want = {"llamahip_sched_new", "llamahip_sched_submit", "llamahip_sched_step", "llamahip_sched_cancel", "llamahip_sched_pending",
            "llamahip_sched_get_stats", "llamahip_sched_free", "llamahip_sched_plan", "llamahip_op_sched_pick"}
    for fn in want:
        assert fn in names and hasattr(L.lib(), fn), fn
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert want <= exported
    assert not [s for s in exported if "sched" in s and not s.startswith("llamahip_")], "an internal of the scheduler is exported"
    assert hasattr(L.Model, "scheduler") and hasattr(L, "Scheduler") and hasattr(L, "sched_plan") and hasattr(L, "op_sched_pick")


def test_sched_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: sched.cpp as it is, against a stubbed device half, in the stand-alone tools/host_sanitize -- the plan over the grid on
    exactly sized arrays, whole scheduler runs replayed step by step against the rule, submit's and step's refusals, cancels -- never
    loaded into python"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "asan"], check=True)
    src = open(os.path.join(csrc, "tools", "host_sanitize.cpp")).read()
    assert "llamahip_sched_step(" in src and "llamahip_sched_submit(" in src and "llamahip_sched_plan(" in src and "llamahip_sched_cancel(" in src
    assert "LLAMAHIP_EVAL_MULTI_MAX_ROWS - max_active" in src and "g_sched_fail" in src          # submit's row limit at n_ctx 4096; a failing step
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(csrc, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout and "scheduler host half" in r.stdout, r.stdout + r.stderr
    assert "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
