"""CPU: the host side of constrained requests in the request scheduler (include/llamahip.h) without a device.
llamahip_forced_run against tests/sched_dfa_ref.py's restatement on the regular expressions and choice sets of tests/test_gpu_constrain.py
and a choice set with long forced tails; what llamahip_sched_new refuses of forced_drafts and the two sizes of llamahip_sched_opts it takes; what
the two allow-list op entry points refuse, each with its message, before any device is asked for; the op tests' own cases held to their
conditions; and `make asan`: sched.cpp and constrain.cpp as they are, against a stubbed device half whose constrained segments get the rule's
pick, in the stand-alone tools/host_sanitize -- llamahip_sched_submit's refusals (which need a scheduler), both sizes of llamahip_request, forced
drafts off and on, a cancel, a stop token inside an accepted draft.  Nothing is loaded into python under a sanitizer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dfa_ref
import sched_dfa_ref as R
import synth

HOST_ONLY = 4
HP = synth.HParams(n_vocab=300, n_embd=128, n_mult=64, n_head=2, n_layer=1)
VOCAB = synth.make_vocab(HP.n_vocab)
STOP = 2
SHORT = "(ab|ba){1,3} tok0003[0-9]"
LONG = "[a-e]{20}"
CHOICES = [b"cab", b"cabbage", b"tok00100", b"d tok00200 e"]
SPECS = (SHORT, LONG, CHOICES, R.TAILS)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")


@pytest.fixture(scope="module")
def host_only(L, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("schedcst") / "m.bin")
    synth.write_model(path, HP, synth.random_tensors(HP, seed=7))
    return L.Model(path, n_ctx=16, flags=HOST_ONLY, n_seq=4)


def constraint_of(m, spec):
    return m.constraint(choices=spec) if isinstance(spec, list) else m.constraint(regex=spec)


@pytest.mark.parametrize("spec", SPECS, ids=["short", "long", "choices", "tails"])
def test_forced_is_the_restated_run_from_every_state(L, host_only, spec):
    with constraint_of(host_only, spec) as c:
        table = c.table()
        n_forced_states = longest = 0
        for state in range(c.n_states):
            for cap in (0, 1, 15):
                got = c.forced(state, cap).tolist()
                assert got == R.forced(table, state, cap), (state, cap)
                assert len(got) <= cap
            run, st = c.forced(state, 15).tolist(), state
            for t in run:          # every forced token is the single allowed entry of its state's row
                assert st != c.done and np.flatnonzero(table[st] != dfa_ref.BANNED).tolist() == [t]
                st = int(table[st][t])
            n_forced_states += len(run) > 0
            longest = max(longest, len(run))
            if len(run) < 15 and st != c.done:          # the run ends where the state allows several tokens
                assert (table[st] != dfa_ref.BANNED).sum() != 1
        assert c.forced(c.done, 15).size == 0          # DONE itself yields nothing
        # an accepting state with only the stop token allowed: the stop token, DONE, and the run ends there
        only_stop = [s for s in range(c.n_states - 1) if np.flatnonzero(table[s] != dfa_ref.BANNED).tolist() == [STOP]]
        assert only_stop or spec == SHORT or spec == LONG
        for s in only_stop:
            assert c.forced(s, 15).tolist() == [STOP] and int(table[s][STOP]) == c.done
        if spec is R.TAILS:          # "yes please" is forced from its second letter on: nine letters and the stop token
            y = c.advance(c.start, VOCAB.index(b"y"))
            assert c.forced(y, 15).tolist() == [VOCAB.index(bytes([b])) for b in b"es please"] + [STOP] and longest >= 10
        assert n_forced_states > 0
        lib = L.lib()
        out = np.zeros(4, np.int32)
        assert lib.llamahip_forced_run(None, 0, out.ctypes.data, 4) == -1 and lib.llamahip_forced_run(c._c, -1, out.ctypes.data, 4) == -1
        assert lib.llamahip_forced_run(c._c, c.n_states, out.ctypes.data, 4) == -1 and lib.llamahip_forced_run(c._c, 0, out.ctypes.data, -1) == -1
        assert lib.llamahip_forced_run(c._c, 0, None, 0) == 0 and lib.llamahip_forced_run(c._c, 0, None, 3) == -1


def test_struct_sizes_and_forced_drafts_refusals(L, host_only):
    b = L.binding
    ERR = b.ERR_PREDICT
    assert C.sizeof(b._SchedOptsForced) == C.sizeof(b._SchedOpts) + 8 and b._SchedOptsForced.forced_drafts.offset == C.sizeof(b._SchedOpts)
    assert b._RequestCst.constraint.offset == C.sizeof(b._Request) and C.sizeof(b._RequestCst) == C.sizeof(b._Request) + 16
    assert C.sizeof(b._SchedStatsDfa) == C.sizeof(b._SchedStatsPrefix) + 24

    def new(size, forced):
        o = b._SchedOptsForced(size, 2, 2, 0, 0, 1.3, 0.95, 0.8, 40)
        o.forced_drafts = forced
        h, err = C.c_void_p(), C.create_string_buffer(1024)
        rc = L.lib().llamahip_sched_new(host_only._h, C.byref(o), C.byref(h), err, len(err))
        return rc, h.value, err.value.decode()
    for bad in (2, -1):
        rc, h, msg = new(C.sizeof(b._SchedOptsForced), bad)
        assert rc == ERR and not h and f"forced_drafts ({bad}) must be 0 (off) or 1" in msg, msg
    # in range, or behind the end of the old struct: the handle is what is refused, last
    for size, forced in ((C.sizeof(b._SchedOptsForced), 1), (C.sizeof(b._SchedOptsForced), 0), (C.sizeof(b._SchedOpts), 2)):
        rc, h, msg = new(size, forced)
        assert rc == ERR and not h and "HOST_ONLY" in msg, (size, forced, msg)
    with pytest.raises(L.LlamaHipError, match="HOST_ONLY"):
        host_only.scheduler(max_active=2, forced_drafts=True)
    assert b.sched_event_cap(4, 1) == 4 + 17          # what a scheduler with forced_drafts and draft_len 0 requires


def test_op_refusals_name_their_limit_before_any_device(L):
    lib = L.lib()
    ERR = L.binding.ERR_PREDICT
    V, S, N = 8, 3, 2
    lg = np.zeros((N, V), np.float32)
    tab = np.zeros((S, V), np.uint16)
    st, fb, em = np.zeros(N, np.int32), np.zeros(N, np.int32), np.ones(N, np.int32)
    pk, dd = np.zeros(N, np.int32), np.zeros(N, np.int32)
    p = lambda a: None if a is None else a.ctypes.data

    def verify(logits=lg, n=N, v=V, table=tab, s=S, states=st, fallback=fb, picks=pk, dead=dd):
        err = C.create_string_buffer(512)
        rc = lib.llamahip_op_verify_rows_allow(p(logits), n, v, p(table), s, p(states), p(fallback), p(picks), p(dead), err, len(err))
        return rc, err.value.decode()

    def sched(logits=lg, n=N, v=V, emit=em, table=tab, s=S, states=st, fallback=fb, picks=pk, dead=dd, words=None, n_slots=0, log_cap=0, state=None, log=None, nxt=None):
        err = C.create_string_buffer(512)
        rc = lib.llamahip_op_sched_pick_allow(p(logits), n, v, p(emit), p(table), s, p(states), p(fallback), p(words), n_slots, log_cap, p(state), p(log), p(nxt),
                                            p(picks), p(dead), err, len(err))
        return rc, err.value.decode()
    bad_tab = tab.copy()
    bad_tab[1, 5] = S          # neither a state nor BANNED
    for call, fn in ((verify, "llamahip_op_verify_rows_allow"), (sched, "llamahip_op_sched_pick_allow")):
        for kw, words in ((dict(logits=None), "logits is NULL"), (dict(table=None), "table is NULL"), (dict(states=None), "states is NULL"),
                          (dict(fallback=None), "fallback is NULL"), (dict(picks=None), "picks is NULL"), (dict(dead=None), "dead is NULL"),
                          (dict(n=0), "n_rows 0 outside 1 .. 16"), (dict(n=17), "n_rows 17 outside 1 .. 16"), (dict(v=0), "n_vocab must be >= 1 (got 0)"),
                          (dict(s=0), "n_table_states 0 outside 1 .. 65535"), (dict(s=65536), "n_table_states 65536 outside 1 .. 65535"),
                          (dict(table=bad_tab), "table[1][5] = 3 is neither a state below 3 nor BANNED (65535)"),
                          (dict(states=np.array([0, S], np.int32)), "states[1] = 3 out of range [-1, 3) (-1 = unconstrained)"),
                          (dict(states=np.array([-2, 0], np.int32)), "states[0] = -2 out of range [-1, 3) (-1 = unconstrained)"),
                          (dict(fallback=np.array([0, V], np.int32)), "fallback[1] = 8 out of range [0, 8)"),
                          (dict(fallback=np.array([-1, 0], np.int32)), "fallback[0] = -1 out of range [0, 8)")):
            rc, msg = call(**kw)
            assert rc == ERR and msg == f"{fn}: {words}", (kw, msg)
    rc, msg = sched(emit=None)
    assert rc == ERR and msg == "llamahip_op_sched_pick_allow: emit is NULL"
    words = np.array([[0, 1, 1], [1, 2, 2]], np.int32)
    state, log, nxt = np.zeros((2, 2), np.int32), np.zeros((2, 4), np.int32), np.zeros(2, np.int32)
    rc, msg = sched(words=words, n_slots=2, log_cap=4, state=state, log=None, nxt=nxt)
    assert rc == ERR and "come all four or not at all" in msg
    rc, msg = sched(words=words, n_slots=0, log_cap=4, state=state, log=log, nxt=nxt)
    assert rc == ERR and "n_slots (0) outside 1 .. 4096" in msg
    rc, msg = sched(words=np.array([[0, 1, 1], [2, 2, 2]], np.int32), n_slots=2, log_cap=4, state=state, log=log, nxt=nxt)
    assert rc == ERR and "segment 1: slot 2 out of range [0, n_slots = 2)" in msg
    rc, msg = sched(words=np.array([[1, 1, 1], [1, 2, 2]], np.int32), n_slots=2, log_cap=4, state=state, log=log, nxt=nxt)
    assert rc == ERR and "slot 1 has two segments (0 and 1)" in msg
    rc, msg = sched(words=np.array([[0, -1, 1], [1, 2, 2]], np.int32), n_slots=2, log_cap=4, state=state, log=log, nxt=nxt)
    assert rc == ERR and "segment 0: position -1 / cursor 1 out of range" in msg


def test_the_op_cases_hold_their_own_conditions():
    seen = set()
    for V in R.OP_VOCABS:
        for rows in R.OP_ROWS:
            for seed in range(len(R.KINDS) if rows == 1 else 2 if rows == 5 else 1):
                case = R.op_case(V, rows, seed)
                picks, dead = R.op_expected(case)
                assert len(case["kinds"]) == rows
                for r, kind in enumerate(case["kinds"]):
                    row, st = case["logits"][r], int(case["states"][r])
                    seen.add((kind, V >= 3))
                    if kind == "free":
                        assert st == -1 and dead[r] == 0 and picks[r] == int(np.argmax(row))
                        continue
                    allowed = np.flatnonzero(case["table"][st] != dfa_ref.BANNED)
                    assert (case["table"][st][allowed] <= rows).all()
                    if kind == "none":
                        assert allowed.size == 0 and dead[r] == 1 and picks[r] == case["fallback"][r]
                        continue
                    assert dead[r] == 0 and picks[r] in allowed
                    if kind in ("max_banned", "tie_across_banned"):          # the best value is banned: the unconstrained argmax is another token
                        assert R.free_pick(row) not in allowed and R.free_pick(row) != picks[r]
                    if kind in ("tie_allowed", "tie_across_banned", "zeros"):          # two allowed entries hold the maximum; the lower index wins
                        best = row[allowed][~np.isnan(row[allowed])].max()
                        holders = allowed[row[allowed] == best]
                        assert holders.size >= 2 and picks[r] == holders[0]
                    if kind == "zeros":
                        assert np.signbit(row[picks[r]]) and row[picks[r]] == 0 and not np.signbit(row[allowed[row[allowed] == 0][-1]])
                    if kind == "nan_among":
                        assert np.isnan(row[allowed]).any() and not np.isnan(row[picks[r]])
                    if kind == "all_nan":
                        assert np.isnan(row[allowed]).all() and picks[r] == allowed[0]
                    if kind == "one_first":
                        assert allowed.tolist() == [0]
                    if kind == "one_last":
                        assert allowed.tolist() == [V - 1]
    assert {k for k, big in seen if big} == set(R.KINDS)          # every kind at the sizes that have room for it


def test_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    subprocess.run(["make", "-s", "-C", CSRC, "asan"], check=True)
    src = open(os.path.join(CSRC, "tools", "host_sanitize.cpp")).read()
    for word in ("forced_drafts", "llamahip_forced_run(", "rq.constraint = ", "offsetof(llamahip_request, constraint)", "n_forced_accepted == ss.n_forced_drafted",
                 "llamahip_sched_cancel(sc, ids[4])", "ss.n_dropped > 0", "another handle", "constraint_state"):
        assert word in src, word
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(CSRC, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout and "scheduler with constrained requests" in r.stdout, r.stdout + r.stderr
    assert "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
