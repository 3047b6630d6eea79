"""CPU: drafted tokens in the request scheduler's host half (csrc/sched.cpp; include/llamahip.h "request scheduler", drafted tokens).

The draft policy llamahip_sched_plan_drafts against a Python restatement over every case of up to four sequences, and its invariants; what
llamahip_sched_new refuses of the draft options, before the handle (a HOST_ONLY handle, no device); the event-capacity bound; the exports.
A scheduler that steps needs a device half, so whole drafting runs -- the old struct_size, the smallest event array, TOKEN events cut at stop
tokens and n_predict, the stats identity -- run in the stand-alone sanitizer program against the stubbed device half, as in
tests/test_sched_host.py."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import synth
from test_sched_host import _new, _opts

MAX_ROWS = 2048          # LLAMAHIP_EVAL_MULTI_MAX_ROWS


def deal_ref(want, spare):
    """llamahip_lookup_deal_rows' rule restated: the spare rows one draft token at a time, round-robin in order, while anybody wants more"""
    give = [0] * len(want)
    while spare > 0 and any(g < w for g, w in zip(give, want)):
        for i in range(len(want)):
            if spare > 0 and give[i] < want[i]:
                give[i] += 1
                spare -= 1
    return give


def plan_drafts_ref(left, rows, want):
    """the issue's text restated (the yardstick)"""
    emitting = sum(1 for x, r in zip(left, rows) if x == 0 or (r > 0 and r == x))
    spare = max(min(16 - emitting, MAX_ROWS - sum(rows)), 0)
    dec = [i for i, x in enumerate(left) if x == 0]
    give = [0] * len(left)
    for i, g in zip(dec, deal_ref([want[i] for i in dec], spare)):
        give[i] = g
    return give


def test_plan_drafts_is_the_restated_policy_over_every_small_case(L):
    n_checked = n_dealt = 0
    for n in range(0, 5):
        for left in itertools.product((0, 1, 5), repeat=n):
            dec = [i for i, x in enumerate(left) if x == 0]
            for c, budget in ((0, 16), (1, 1), (9, 64), (4, 3)):
                total, rows = L.sched_plan(list(left), c, budget)
                rows = rows.tolist()
                for wd in itertools.product((0, 1, 15), repeat=len(dec)):
                    want = [0] * n
                    for i, w in zip(dec, wd):
                        want[i] = w
                    got_n, give = L.sched_plan_drafts(list(left), rows, want)
                    give = give.tolist()
                    ref = plan_drafts_ref(left, rows, want)
                    assert give == ref and got_n == sum(ref), (left, rows, want, give, ref)
                    # the invariants
                    assert all(g <= w for g, w in zip(give, want))
                    assert all(g == 0 for g, x in zip(give, left) if x > 0), "a draft for a sequence that is not decoding"
                    emitting = sum(1 for x, r in zip(left, rows) if x == 0 or (r > 0 and r == x))
                    assert emitting + sum(give) <= 16, "more than 16 logits rows"
                    assert sum(give) <= 15
                    n_checked += 1
                    n_dealt += sum(give) > 0
    assert n_checked > 1000 and n_dealt > 300


def test_plan_drafts_round_robin_and_the_row_cap(L):
    # 16 spare rows less the emitting segments, one token at a time in admission order
    assert L.sched_plan_drafts([0, 0, 0], [1, 1, 1], [15, 15, 15])[1].tolist() == [5, 4, 4]
    assert L.sched_plan_drafts([0, 0, 0], [1, 1, 1], [2, 15, 1])[1].tolist() == [2, 10, 1]
    n, give = L.sched_plan_drafts([0] * 16, [1] * 16, [15] * 16)          # sixteen decode rows: nothing spare
    assert n == 0 and give.tolist() == [0] * 16
    assert L.sched_plan_drafts([0], [1], [15])[1].tolist() == [15]
    # a prompt piece that ends its prompt emits; one that does not leaves its logits row spare
    assert L.sched_plan_drafts([9, 0], [9, 1], [0, 15])[1].tolist() == [0, 14]
    assert L.sched_plan_drafts([9, 0], [4, 1], [0, 15])[1].tolist() == [0, 15]
    assert L.sched_plan_drafts([9, 0], [0, 1], [0, 15])[1].tolist() == [0, 15]
    # the pass takes LLAMAHIP_EVAL_MULTI_MAX_ROWS rows in all
    for room in (0, 1, 6, 15, 40):
        left, rows = [MAX_ROWS, 0, 0], [MAX_ROWS - 2 - room, 1, 1]
        n, give = L.sched_plan_drafts(left, rows, [0, 15, 15])
        assert n == min(room, 14) == int(give.sum()) and sum(rows) + n <= MAX_ROWS, (room, give)
        assert give.tolist() == [0] + deal_ref([15, 15], min(room, 14))


def test_plan_drafts_refuses_bad_arguments(L):
    assert L.sched_plan_drafts([], [], [])[0] == 0                             # nobody active: nothing to deal
    assert L.sched_plan_drafts([0] * 17, [1] * 17, [0] * 17)[0] == -1          # more than 16 sequences
    assert L.sched_plan_drafts([5], [5], [1])[0] == -1                         # a draft for a prefilling sequence
    assert L.sched_plan_drafts([0], [1], [16])[0] == -1                        # want outside 0 .. 15
    assert L.sched_plan_drafts([0], [1], [-1])[0] == -1
    assert L.sched_plan_drafts([-1], [1], [0])[0] == -1
    assert L.sched_plan_drafts([0], [2], [1])[0] == -1                         # a decoding sequence has one row
    assert L.sched_plan_drafts([3], [4], [0])[0] == -1                         # more rows than the prompt has left
    lib = L.lib()
    one = np.ones(1, np.int32)
    assert lib.llamahip_sched_plan_drafts(1, None, one.ctypes.data, one.ctypes.data, one.ctypes.data) == -1
    assert lib.llamahip_sched_plan_drafts(1, one.ctypes.data, one.ctypes.data, one.ctypes.data, None) == -1
    assert lib.llamahip_sched_plan_drafts(-1, None, None, None, None) == -1


@pytest.fixture(scope="module")
def host_only(L, tmp_path_factory):
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    path = str(tmp_path_factory.mktemp("sched_draft") / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    return L.Model(path, n_ctx=64, flags=4, n_seq=4)          # LLAMAHIP_FLAG_HOST_ONLY: no device is touched


def test_sched_new_refuses_the_draft_options_before_the_handle(L, host_only):
    ERR = L.binding.ERR_PREDICT
    good = np.array([1, 2, 95], np.int32)
    bad = np.array([1, 96, 2], np.int32)
    neg = np.array([-1], np.int32)
    cases = ((dict(draft_len=-1), "draft_len (-1) outside 0 .. 15"), (dict(draft_len=16), "draft_len (16) outside 0 .. 15"),
             (dict(draft_len=4, ngram_min=-1), "ngram_min (-1)"), (dict(draft_len=4, ngram_max=-2), "ngram_max (-2)"),
             (dict(draft_len=4, ngram_min=3, ngram_max=2), "ngram_max >= ngram_min"),
             (dict(draft_len=4, ngram_min=4), "ngram_max >= ngram_min"),          # above the default ngram_max (3)
             (dict(draft_len=4, n_corpus=-1), "n_corpus (-1)"), (dict(draft_len=4, n_corpus=3), "n_corpus (3)"),
             (dict(draft_len=4, corpus=bad.ctypes.data, n_corpus=3), "corpus token id 96 at 1 out of range [0, 96)"),
             (dict(draft_len=4, corpus=neg.ctypes.data, n_corpus=1), "corpus token id -1 at 0 out of range [0, 96)"))
    for kw, word in cases:
        rc, h, msg = _new(L, host_only, _opts(L, **kw))
        assert rc == ERR and not h and msg.startswith("llamahip_sched_new:") and word in msg and "HOST_ONLY" not in msg, (kw, msg)
    # every draft option in range: the handle is what is refused, last
    for kw in (dict(draft_len=15), dict(draft_len=1, ngram_min=1, ngram_max=1), dict(draft_len=4, ngram_max=7),
               dict(draft_len=4, corpus=good.ctypes.data, n_corpus=3), dict(draft_len=0, corpus=bad.ctypes.data, n_corpus=1)):
        rc, h, msg = _new(L, host_only, _opts(L, **kw))
        assert rc == ERR and not h and "HOST_ONLY" in msg, (kw, msg)
    with pytest.raises(L.LlamaHipError) as e:
        host_only.scheduler(max_active=2, draft_len=16)
    assert e.value.code == ERR and "draft_len" in e.value.message
    with pytest.raises(L.LlamaHipError) as e:
        host_only.scheduler(max_active=2, draft_len=4, corpus=[5, 200])
    assert "corpus token id 200 at 1" in e.value.message


def test_an_options_struct_of_the_old_size_does_not_read_the_draft_fields(L, host_only):
    b = L.binding
    old_size = b._SchedOpts.draft_len.offset
    assert old_size == b._SchedOpts.top_k.offset + 4 and C.sizeof(b._SchedOpts) > old_size
    # what lies behind struct_size is not the library's to read: a draft_len that would be refused is not even seen
    rc, h, msg = _new(L, host_only, _opts(L, struct_size=old_size, draft_len=99, ngram_min=-5, n_corpus=-1))
    assert rc == b.ERR_PREDICT and "HOST_ONLY" in msg, msg
    rc, h, msg = _new(L, host_only, _opts(L, struct_size=old_size + 4, draft_len=99, ngram_min=-5))          # draft_len covered, no more
    assert rc == b.ERR_PREDICT and "draft_len (99)" in msg, msg


def test_the_event_capacity_bound(L):
    for a in (1, 3, 16):
        assert L.sched_event_cap(a) == L.sched_event_cap(a, 0) == 2 * a + 1          # unchanged without drafts
        for dl in (1, 15):
            assert L.sched_event_cap(a, dl) == a + 17          # 16 logits rows, a DONE per request, one waiting DONE
    hdr = open(os.path.join(L.binding.INCLUDE, "llamahip.h")).read()
    m = re.search(r"#define LLAMAHIP_SCHED_EVENT_CAP\(max_active, draft_len\) (.*?)\s*/\*", hdr)
    assert m and m.group(1).replace(" ", "") == "((draft_len)>0?(max_active)+17:2*(max_active)+1)", m
    # the stats struct ends with the new counters, behind the old ones
    names = [k for k, _ in L.binding._SchedStats._fields_]
    assert names[-5:] == ["n_draft_steps", "n_drafted", "n_accepted", "n_emit_segs", "n_dropped"] and names[-6] == "n_done"


def test_new_symbols_are_declared_and_exported(L, built):
    names = L.declared_symbols()
    want = {"llamahip_sched_plan_drafts", "llamahip_op_sched_accept"}
    for fn in want:
        assert fn in names and hasattr(L.lib(), fn), fn
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert want <= exported
    assert not [s for s in exported if "sched" in s and not s.startswith("llamahip_")], "an internal of the scheduler is exported"
    assert hasattr(L, "sched_plan_drafts") and hasattr(L, "op_sched_accept") and hasattr(L, "sched_event_cap")
    import inspect
    assert {"draft_len", "ngram_min", "ngram_max", "corpus"} <= set(inspect.signature(L.Model.scheduler).parameters)
    assert inspect.signature(L.Model.scheduler).parameters["draft_len"].default == 0          # off unless asked for


def test_the_drafting_host_half_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: sched.cpp as it is against the stubbed device half, which accepts a scripted number of draft tokens per segment, in the
    stand-alone tools/host_sanitize (never loaded into python): drafting schedulers at draft_len 1 / 4 / 15 on an event array of exactly
    max_active + 17 entries (one fewer is refused), every draft checked against llamahip_lookup_draft on the request's history, every event
    against the stub's tokens, the stream cut at stop tokens and n_predict, the stats identity; a handle that takes no drafts; the refusals;
    an options struct that ends before draft_len"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "asan"], check=True)
    src = open(os.path.join(csrc, "tools", "host_sanitize.cpp")).read()
    for word in ("g_sched_accept", "sched_dev_drafts", "LLAMAHIP_SCHED_EVENT_CAP(max_active, draft_len)", "offsetof(llamahip_sched_opts, draft_len)",
                 "ss.n_tokens == ss.n_emit_segs + ss.n_accepted - ss.n_dropped", "max_active + 17"):
        assert word in src, word
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(csrc, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout and "scheduler with drafted tokens" in r.stdout, r.stdout + r.stderr
    assert "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
