"""CPU: shared prompt prefixes in the request scheduler (include/llamahip.h "Evaluated prompt prefixes shared between KV slots").

The prefix policy llamahip_sched_plan_prefix against a brute-force restatement over a grid -- chunks 0, 1, 4, 9; prompts of 1 .. 40 tokens;
common prefixes of 0 .. 40; records shorter than, equal to and longer than the prefix; all slots free, some free, an active donor -- and its
properties; its refusals; what llamahip_kv_copy_rows refuses without a device (every argument first, the handle last); llamahip_sched_new
on prefix_share; the exports; the stand-alone sanitizer program (never loaded into python)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import synth

CHUNKS = (0, 1, 4, 9)


def lcp(a, b):
    n = 0
    while n < len(a) and n < len(b) and a[n] == b[n]:
        n += 1
    return n


def share_ref(held, prompt, c):
    """rows of the record a new prompt may take over: whole chunks of the common prefix, never the prompt's last token"""
    return min(lcp(prompt, held), len(held), len(prompt) - 1) // c * c if c > 0 else 0


def plan_prefix_ref(free, held, prompt, c):
    """the policy restated (the yardstick): (P, slot, donor, in place)"""
    sh = [share_ref(h, prompt, c) for h in held]
    slot = min((s for s in range(len(held)) if free[s]), key=lambda s: (-sh[s], len(held[s]), s))
    others = [t for t in range(len(held)) if t != slot]
    donor = min(others, key=lambda t: (-sh[t], t)) if others else -1
    if donor >= 0 and sh[donor] > sh[slot]:
        return sh[donor], slot, donor, sh[slot]
    return sh[slot], slot, -1, sh[slot]


def _record(rng, prompt, common, rel):
    """a record that agrees with the prompt on exactly `common` tokens (or is the prompt's whole prefix where it ends first), its length
    shorter than / equal to / longer than the common prefix asks for"""
    n = {"shorter": max(common - int(rng.integers(1, 5)), 0), "equal": common, "longer": common + int(rng.integers(1, 9))}[rel]
    h = [int(t) for t in prompt[:min(n, common)]]
    while len(h) < n:
        k = len(h)
        t = int(rng.integers(0, 50))
        if k == common and k < len(prompt) and t == int(prompt[k]):
            t = (t + 1) % 50          # the record leaves the prompt exactly here
        h.append(t)
    return h


def test_plan_prefix_is_the_restated_policy_over_the_grid(L):
    rng = np.random.default_rng(23)
    n_checked = n_donors = n_inplace = 0
    for c in CHUNKS:
        for n_prompt in range(1, 41):
            prompt = [int(t) for t in rng.integers(0, 50, n_prompt)]
            for common in sorted({0, 1, c, n_prompt - 1, n_prompt, 40, int(rng.integers(0, 41))}):
                common = min(common, n_prompt)
                for rel in ("shorter", "equal", "longer"):
                    for occupancy in ("all_free", "some_free", "donor_active"):
                        n_slots = int(rng.integers(1, 6)) if occupancy == "all_free" else int(rng.integers(2, 6))
                        held = [_record(rng, prompt, common if s == n_slots - 1 else int(rng.integers(0, common + 1)), rel) if rng.integers(0, 4) else []
                                for s in range(n_slots)]
                        free = [1] * n_slots
                        if occupancy == "some_free":
                            free = [int(x) for x in rng.integers(0, 2, n_slots)]
                            free[int(rng.integers(0, n_slots))] = 1
                        if occupancy == "donor_active":
                            free[n_slots - 1] = 0          # the slot with the longest common prefix is busy: it can only give
                        got = L.sched_plan_prefix(free, held, prompt, c)
                        want = plan_prefix_ref(free, held, prompt, c)
                        assert got == want, (c, prompt, held, free, got, want)
                        P, slot, donor, inplace = got
                        # the properties, stated on their own
                        assert free[slot] and 0 <= inplace <= P <= n_prompt - 1
                        assert P == 0 if c == 0 else P % c == 0 and inplace % c == 0
                        src = held[donor] if donor >= 0 else held[slot]
                        assert P <= len(src) and src[:P] == prompt[:P]
                        assert held[slot][:inplace] == prompt[:inplace]
                        assert donor != slot and (donor == -1) == (P == inplace)
                        assert all(share_ref(h, prompt, c) <= P for h in held)          # nobody holds more
                        n_checked += 1
                        n_donors += donor >= 0
                        n_inplace += inplace > 0
    assert n_checked > 5000 and n_donors > 300 and n_inplace > 300, (n_checked, n_donors, n_inplace)


def test_plan_prefix_tie_breaks_and_the_empty_case(L):
    p = list(range(1, 21))
    # nothing held anywhere: the lowest free slot, as without the option
    assert L.sched_plan_prefix([1, 1, 1], [[], [], []], p, 4) == (0, 0, -1, 0)
    assert L.sched_plan_prefix([0, 1, 1], [[], [], []], p, 4) == (0, 1, -1, 0)
    # the largest in-place share wins; ties go to the smallest record (an empty slot loses nothing), then to the lowest index
    assert L.sched_plan_prefix([1, 1, 1], [p[:4], p[:12], p[:8]], p, 4) == (12, 1, -1, 12)
    assert L.sched_plan_prefix([1, 1, 1], [p[:8] + [99] * 5, p[:8], p[:8] + [99]], p, 4) == (8, 1, -1, 8)
    assert L.sched_plan_prefix([1, 1, 1], [[77] * 9, [], [78]], p, 4) == (0, 1, -1, 0)
    assert L.sched_plan_prefix([1, 1, 1], [[77], [78], [79]], p, 4) == (0, 0, -1, 0)
    # the donor: the largest share among the OTHER slots, free or active, ties to the lowest index; only if it beats what is in place
    assert L.sched_plan_prefix([1, 0, 0], [p[:4], p[:16], p[:16]], p, 4) == (16, 0, 1, 4)
    assert L.sched_plan_prefix([1, 0, 1], [[], p[:12], p[:9]], p, 4) == (12, 2, 1, 8)
    assert L.sched_plan_prefix([1, 0], [p[:8], p[:8]], p, 4) == (8, 0, -1, 8)
    # whole chunks only, never the last token, never more than the record holds as prompt rows
    assert L.sched_plan_prefix([1, 0], [[], p], p, 9) == (18, 0, 1, 0)
    assert L.sched_plan_prefix([1, 0], [[], p], p, 1) == (19, 0, 1, 0)          # an exact resubmission: everything but the last token
    assert L.sched_plan_prefix([1, 0], [[], p], p, 4) == (16, 0, 1, 0)
    assert L.sched_plan_prefix([1, 0], [[], p[:7]], p, 4) == (4, 0, 1, 0)
    assert L.sched_plan_prefix([1, 0], [[], p], p[:9], 9) == (0, 0, -1, 0)        # a prompt no longer than one chunk
    assert L.sched_plan_prefix([1, 0], [[], p], p, 0) == (0, 0, -1, 0)            # chunk_tokens 0 shares nothing


def test_plan_prefix_refuses_bad_arguments(L):
    p = [1, 2, 3]
    assert L.sched_plan_prefix([1], [[1, 2]], p, 1)[0] == 2
    assert L.sched_plan_prefix([1] * 17, [[]] * 17, p, 1)[0] == -1        # n_slots outside 1 .. 16
    assert L.sched_plan_prefix([], [], p, 1)[0] == -1
    assert L.sched_plan_prefix([0, 0], [[], []], p, 1)[0] == -1           # no free slot
    assert L.sched_plan_prefix([1], [[]], [], 1)[0] == -1                 # n_prompt < 1
    assert L.sched_plan_prefix([1], [[]], p, -1)[0] == -1                 # chunk_tokens < 0
    assert L.sched_plan_prefix([-1, 1], [[], []], p, 1)[0] == -1          # a negative entry
    assert L.sched_plan_prefix([1], [[1, -2]], p, 1)[0] == -1
    assert L.sched_plan_prefix([1], [[]], [1, -2], 1)[0] == -1
    lib = L.lib()
    one, two, neg = (C.c_int32 * 1)(1), (C.c_int32 * 1)(2), (C.c_int32 * 1)(-1)
    tok = (C.c_int32 * 3)(1, 2, 3)
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    args = [1, one, tok, two, tok, 3, 1, C.byref(a), C.byref(b), C.byref(c)]
    assert lib.llamahip_sched_plan_prefix(*args) == 2
    for k in (1, 2, 3, 4, 7, 8, 9):          # a null array or output
        bad = list(args)
        bad[k] = None
        assert lib.llamahip_sched_plan_prefix(*bad) == -1, k
    bad = list(args)
    bad[3] = neg
    assert lib.llamahip_sched_plan_prefix(*bad) == -1          # a negative record length


@pytest.fixture(scope="module")
def host_only(L, tmp_path_factory):
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    path = str(tmp_path_factory.mktemp("prefix") / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    return L.Model(path, n_ctx=64, flags=4, n_seq=4)          # LLAMAHIP_FLAG_HOST_ONLY: no device is touched


def test_kv_copy_rows_refusals_name_their_limit_and_touch_no_device(L, host_only):
    ERR = L.binding.ERR_PREDICT
    for copies, word in (([(0, 4, 0, 1)], "n_seq"), ([(-1, 1, 0, 1)], "n_seq"), ([(4, 0, 0, 1)], "n_seq"),
                         ([(2, 2, 0, 1)], "same slot"),
                         ([(0, 1, 0, -1)], "n_ctx"), ([(0, 1, -1, 1)], "n_ctx"), ([(0, 1, 60, 5)], "n_ctx"), ([(0, 1, 65, 0)], "n_ctx"),
                         ([(0, 1, 0, 2147483647)], "n_ctx"),
                         ([(0, 1, 0, 4), (1, 2, 0, 4)], "destination of copy"),          # a destination that is another copy's source
                         ([(1, 2, 0, 4), (0, 1, 0, 4)], "destination of copy"),
                         ([(0, 2, 0, 4), (1, 2, 8, 4)], "destination of copy"),          # ... or another copy's destination
                         ([(0, 1, 0, 1)] * 17, "1 .. 16")):
        with pytest.raises(L.LlamaHipError) as e:
            host_only.kv_copy_rows(copies)
        assert e.value.code == ERR and word in e.value.message, (copies, e.value.message)
    # every argument in range -- one source feeding many destinations, an empty entry, the whole context: the handle is what is refused, last
    for copies in ([(0, 1, 0, 64)], [(0, 1, 0, 8), (0, 2, 0, 8), (0, 3, 4, 0)], [(0, 1, 64, 0)]):
        with pytest.raises(L.LlamaHipError) as e:
            host_only.kv_copy_rows(copies)
        assert e.value.code == ERR and "HOST_ONLY" in e.value.message, (copies, e.value.message)
    lib = L.lib()
    err = C.create_string_buffer(256)
    one = (C.c_int32 * 1)(1)
    zero = (C.c_int32 * 1)(0)
    assert lib.llamahip_kv_copy_rows(None, 1, zero, one, zero, one, err, len(err)) == ERR and b"null model" in err.value
    assert lib.llamahip_kv_copy_rows(host_only._h, 0, zero, one, zero, one, err, len(err)) == ERR and b"1 .. 16" in err.value
    for k in range(4):
        arrs = [zero, one, zero, one]
        arrs[k] = None
        assert lib.llamahip_kv_copy_rows(host_only._h, 1, *arrs, err, len(err)) == ERR and b"null array" in err.value
    assert lib.llamahip_kv_copy_rows(host_only._h, 1, zero, one, zero, one, None, 0) == ERR


def _new(L, model, o):
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    rc = L.lib().llamahip_sched_new(model._h, C.byref(o), C.byref(h), err, len(err))
    return rc, h.value, err.value.decode()


def test_sched_new_on_prefix_share(L, host_only):
    b = L.binding
    ERR = b.ERR_PREDICT
    assert b._SchedOpts.prefix_share.offset >= b._SchedOpts.n_corpus.offset + 4          # appended behind n_corpus
    for v in (2, -1, 7):
        o = b._SchedOpts(C.sizeof(b._SchedOpts), 2, 2, 9, 0, 1.3, 0.95, 0.8, 40, prefix_share=v)
        rc, h, msg = _new(L, host_only, o)
        assert rc == ERR and not h and "prefix_share" in msg, (v, msg)
    # 0 and 1 are taken: the handle is what is refused; a struct that ends before the field means off, whatever lies behind it
    for v, size in ((0, C.sizeof(b._SchedOpts)), (1, C.sizeof(b._SchedOpts)), (2, b._SchedOpts.prefix_share.offset)):
        o = b._SchedOpts(size, 2, 2, 9, 0, 1.3, 0.95, 0.8, 40, prefix_share=v)
        rc, h, msg = _new(L, host_only, o)
        assert rc == ERR and not h and "HOST_ONLY" in msg, (v, size, msg)
    with pytest.raises(L.LlamaHipError) as e:
        host_only.scheduler(max_active=2, chunk_tokens=9, prefix_share=True)
    assert "HOST_ONLY" in e.value.message
    # the stats struct ends with the new counters, behind the old ones
    assert [k for k, _ in b._SchedStatsPrefix._fields_] == ["n_shared_rows", "n_copied_rows", "n_copy_launches"]
    assert b._SchedStatsPrefix.n_shared_rows.offset == C.sizeof(b._SchedStats) and C.sizeof(b._SchedStatsPrefix) == C.sizeof(b._SchedStats) + 24


def test_new_symbols_are_declared_and_exported(L, built):
    names = L.declared_symbols()
    want = {"llamahip_sched_plan_prefix", "llamahip_kv_copy_rows"}
    for fn in want:
        assert fn in names and hasattr(L.lib(), fn), fn
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert want <= exported
    assert not [s for s in exported if "kv_copy" in s and not s.startswith("llamahip_")], "an internal of the copy is exported"
    assert hasattr(L.Model, "kv_copy_rows") and hasattr(L, "sched_plan_prefix")


def test_prefix_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: sched.cpp as it is against a stubbed device half in the stand-alone tools/host_sanitize -- the prefix policy over a grid on
    exactly sized arrays, whole runs with prefix_share on against a shadow cache, a copy and a step that fail -- never loaded into python"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "asan"], check=True)
    src = open(os.path.join(csrc, "tools", "host_sanitize.cpp")).read()
    assert "llamahip_sched_plan_prefix(" in src and "prefix_share = share" in src and "sched_dev_copy_prefix(" in src and "g_sched_copy_fail" in src
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(csrc, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout and "scheduler with shared prefixes" in r.stdout, r.stdout + r.stderr
    assert "scheduler host half" in r.stdout and "scheduler with drafted tokens" in r.stdout          # (what the tool printed before)
    assert "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
