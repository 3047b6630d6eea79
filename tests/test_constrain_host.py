"""CPU: the host half of constrained decoding (csrc/constrain.cpp, llama.swift_amd/regex_dfa.py) -- the symbols; the lift and the prune
against tests/dfa_ref.py with the whole uint16 table compared, on synth.make_vocab vocabularies and hand-made ones (multi-byte tokens across
several byte-states, tokens that die midway, bytes >= 0x80, empty tokens, the stop token in and out of accepting states, the DONE row, a
byte-state only bytes no token supplies would reach, a start state that is not live); the choices builder against the trie built in Python;
advance / pick / mask_row against numpy at ties, signed zeros, NaN, -inf and all-NaN rows; regex_dfa against re.fullmatch on every byte
string up to length 4 over a 4-letter alphabet; every refusal with the limit named; and the host code under ASan + UBSan in the stand-alone
program `make asan` builds.  Everything is exact: integers and bit patterns."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import dfa_ref
import synth

HOST_ONLY = 4
BANNED = dfa_ref.BANNED
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
NEW = ("llamahip_constraint_new", "llamahip_constraint_new_choices", "llamahip_constraint_free", "llamahip_constraint_n_states",
       "llamahip_constraint_start", "llamahip_constraint_done", "llamahip_constraint_table", "llamahip_constraint_advance",
       "llamahip_constraint_pick", "llamahip_constraint_mask_row", "llamahip_decode_greedy_constrained", "llamahip_decode_greedy_constrained_multi",
       "llamahip_eval_topk_constrained", "llamahip_op_pick_dfa",
       "llamahip_op_mask_rows_dfa")


def model_with(L, tmp_path, vocab, name="m.bin"):
    hp = synth.HParams(n_vocab=len(vocab), n_embd=128, n_mult=64, n_head=2, n_layer=1)
    path = str(tmp_path / name)
    synth.write_model(path, hp, synth.random_tensors(hp, seed=7), vocab=vocab)
    return L.Model(path, n_ctx=16, flags=HOST_ONLY)


def dfa_of(n_states, edges, accept):
    """edges: {(state, byte): next}"""
    trans = np.full((n_states, 256), -1, np.int32)
    for (s, b), q in edges.items():
        trans[s, b] = q
    acc = np.zeros(n_states, np.uint8)
    acc[list(accept)] = 1
    return trans, acc


def check_lift(L, m, vocab, trans, accept, start, stop):
    want = dfa_ref.lift(vocab, trans, accept, start, stop)
    assert want is not None
    with m.constraint(dfa=(trans, accept, start), stop_token=stop) as c:
        got = c.table()
        assert (c.n_states, c.start, c.done) == (trans.shape[0] + 1, start, trans.shape[0])
        assert got.dtype == np.uint16 and got.shape == want.shape and got.tobytes() == want.tobytes()
        # advance is the table, and -1 outside it
        rng = np.random.default_rng(1)
        for s, t in zip(rng.integers(0, c.n_states, 200), rng.integers(0, len(vocab), 200)):
            assert c.advance(s, t) == (-1 if want[s, t] == BANNED else int(want[s, t]))
        assert c.advance(-1, 3) == -1 and c.advance(c.n_states, 3) == -1 and c.advance(0, -1) == -1 and c.advance(0, len(vocab)) == -1
    return want


def test_new_symbols_are_declared_and_exported(L):
    names = L.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for fn in NEW:
        assert fn in names and fn in exported, fn
    assert callable(L.op_pick_dfa) and callable(L.op_mask_rows_dfa) and callable(L.Model.constraint) and callable(L.Model.decode_greedy_constrained)
    assert callable(L.Model.decode_greedy_constrained_multi) and callable(L.Model.eval_topk_constrained) and callable(L.Model.decode_sample_constrained)
    assert {s for s in exported if "constrain" in s or "dfa" in s} == set(NEW)


def test_lift_on_hand_made_vocabularies(L, tmp_path):
    # 0 -a-> 1 -b-> 2 -c-> 3(acc); 3 -\xc3-> 4 -\xa9-> 3 (an e-acute behind the answer); 0 -z-> 5 (5 leads nowhere: not live);
    # 1 -q-> 6 -q-> 3: state 6 is entered only by the byte q, which no token supplies on its own
    edges = {(0, ord("a")): 1, (1, ord("b")): 2, (2, ord("c")): 3, (3, 0xC3): 4, (4, 0xA9): 3, (0, ord("z")): 5, (5, ord("z")): 5,
             (1, ord("q")): 6, (6, ord("q")): 3}
    trans, accept = dfa_of(7, edges, [3])
    vocab = [b"", b"", b"", b"a", b"b", b"c", b"abc", b"ab", b"bc", b"abd", b"\xc3\xa9", b"\xc3", b"\xa9", b"c\xc3\xa9c", b"z", b"zz", b"STOP", b"abcabc",
             b"qq", b"bqq"]
    stop = 16
    with model_with(L, tmp_path, vocab) as m:
        t = check_lift(L, m, vocab, trans, accept, 0, stop)
        V = {w: i for i, w in enumerate(vocab) if w}
        assert t[0, V[b"abc"]] == 3 and t[0, V[b"ab"]] == 2 and t[1, V[b"bc"]] == 3                     # multi-byte tokens across several byte-states
        assert t[0, V[b"abd"]] == BANNED and t[0, V[b"abcabc"]] == BANNED and t[3, V[b"c\xc3\xa9c"]] == BANNED      # ... that die midway
        assert t[3, V[b"\xc3\xa9"]] == 3 and t[3, V[b"\xc3"]] == 4 and t[4, V[b"\xa9"]] == 3             # bytes >= 0x80
        assert (t[:, :3] == BANNED).all()                                                             # empty tokens, everywhere
        assert t[3, stop] == 7 and all(t[s, stop] == BANNED for s in (0, 1, 2, 4, 5, 6))               # the stop token in / out of accepting states
        assert t[7, stop] == 7 and (np.delete(t[7], stop) == BANNED).all()                            # the DONE row
        assert t[0, V[b"z"]] == BANNED and t[0, V[b"zz"]] == BANNED and (t[5] == BANNED).all()          # into a state that is not live
        assert t[1, V[b"qq"]] == 3 and not (t[:7] == 6).any()                                           # state 6: never a token's target ...
        assert t[6, V[b"qq"]] == BANNED                                                                # ... and its own row leads nowhere by tokens
        # every state a token can enter from the start has an allowed token (the prune's consequence)
        seen, todo = {0}, [0]
        while todo:
            for q in t[todo.pop()]:
                if q != BANNED and int(q) not in seen:
                    seen.add(int(q)), todo.append(int(q))
        assert all((t[s] != BANNED).any() for s in seen) and 7 in seen
        # (the stop token's own text does not matter: "STOP" would die in every state)
        # a start state that is not live: refused; so is one that only byte-state 6's bytes would save
        for start in (5, 6):
            assert dfa_ref.lift(vocab, trans, accept, start, stop) is None
            with pytest.raises(L.LlamaHipError) as e:
                m.constraint(dfa=(trans, accept, start), stop_token=stop)
            assert e.value.message == f"llamahip_constraint_new: start state {start} is not live: no sequence of tokens leads from it to an accepting state"
        # a stop token whose text is empty (the end-of-text id of these files)
        check_lift(L, m, vocab, trans, accept, 0, 2)
        # the one-state case: a static allow-list of the tokens made of a / b / c
        allow, acc1 = dfa_of(1, {(0, ord(x)): 0 for x in "abc"}, [0])
        t1 = check_lift(L, m, vocab, allow, acc1, 0, stop)
        assert sorted(np.flatnonzero(t1[0] != BANNED).tolist()) == sorted([V[w] for w in (b"a", b"b", b"c", b"abc", b"ab", b"bc", b"abcabc")] + [stop])


def test_lift_on_synth_vocabularies_and_random_automata(L, tmp_path):
    rng = np.random.default_rng(11)
    for V in (40, 300):
        vocab = synth.make_vocab(V)
        with model_with(L, tmp_path, vocab, f"v{V}.bin") as m:
            done = 0
            for it in range(12):
                S = int(rng.integers(1, 9))
                trans = np.full((S, 256), -1, np.int32)
                alphabet = list(b"abct ok0123")
                for s in range(S):
                    for b in alphabet:
                        if rng.random() < 0.6:
                            trans[s, b] = rng.integers(0, S)
                accept = (rng.random(S) < 0.3).astype(np.uint8)
                accept[int(rng.integers(0, S))] = 1
                start, stop = int(rng.integers(0, S)), int(rng.integers(0, V))
                if dfa_ref.lift(vocab, trans, accept, start, stop) is None:
                    with pytest.raises(L.LlamaHipError, match="is not live"):
                        m.constraint(dfa=(trans, accept, start), stop_token=stop)
                    continue
                check_lift(L, m, vocab, trans, accept, start, stop)
                done += 1
            assert done >= 6
            # a regex over the vocabulary's words: tok000NN is one token, its letters t / o / k are tokens too, its digits are not
            c = m.constraint(regex="(ab|ba)+ tok0003[0-9]", stop_token=2) if V == 300 else m.constraint(regex="(ab|ba)+ c", stop_token=2)
            from llama_swift_amd import regex_dfa
            tr, ac, st = regex_dfa.compile("(ab|ba)+ tok0003[0-9]" if V == 300 else "(ab|ba)+ c")
            assert c.table().tobytes() == dfa_ref.lift(vocab, tr, ac, st, 2).tobytes()
            c.close()


def test_choices_builder_is_the_trie(L, tmp_path):
    vocab = synth.make_vocab(64)
    with model_with(L, tmp_path, vocab) as m:
        for strings in ([b"yes", b"no"], [b"a"], [b"ab", b"abc", b"ab", b"b"], [b"tok00040", b"tok00041 a", b"to"], [b"\xff\x00z", b"\xffa"]):
            tr, ac, st = dfa_ref.trie(strings)
            want = dfa_ref.lift(vocab, tr, ac, st, 2)
            if want is None:      # (the \xff strings: no token supplies their bytes)
                with pytest.raises(L.LlamaHipError) as e:
                    m.constraint(choices=strings)
                assert e.value.message.startswith("llamahip_constraint_new_choices: start state 0 is not live")
                continue
            with m.constraint(choices=strings) as c:
                assert c.n_states == tr.shape[0] + 1 and c.start == 0 and c.table().tobytes() == want.tobytes()
        with m.constraint(choices=["ab", "abc"]) as c:      # a prefix of another: both ends accepting
            t = c.table()
            assert t[2, 2] == c.done and t[3, 2] == c.done and t[0, 2] == BANNED and t[1, 2] == BANNED


def test_advance_pick_and_mask_row_against_numpy(L, tmp_path):
    vocab = synth.make_vocab(300)
    nan, inf = np.float32("nan"), np.float32("inf")
    with model_with(L, tmp_path, vocab) as m, m.constraint(regex="[a-e]+|tok0010[0-9]", stop_token=2) as c:
        t = c.table()
        rng = np.random.default_rng(3)
        rows, empty_rows = [], 0
        for s in range(c.n_states):
            allowed = np.flatnonzero(t[s] != BANNED)
            base = rng.standard_normal(300).astype(np.float32)
            if allowed.size == 0:      # a byte-state inside "tok0010": no token enters it, its row allows nothing, the host pick says -1
                assert not (t == s).any() and c.pick(s, base) == -1 and np.isneginf(c.mask_row(s, base)).all()
                empty_rows += 1
                continue
            rows.append((s, base))
            x = base.copy(); x[np.argmax(np.where(t[s] == BANNED, base, -inf))] = 100.0; rows.append((s, x))      # the global argmax banned
            x = base.copy(); x[allowed] = 1.5; rows.append((s, x))                                              # a tie among all allowed
            x = base.copy(); x[allowed[-1]] = 7.0; x[allowed[0]] = 7.0; rows.append((s, x))                      # a tie of two
            x = np.full(300, -0.0, np.float32); x[allowed[-1]] = 0.0; rows.append((s, x))                        # -0.0 == +0.0: the lower index
            x = base.copy(); x[allowed[0]] = nan; rows.append((s, x))                                            # a NaN on an allowed entry
            x = base.copy(); x[allowed] = nan; rows.append((s, x))                                               # every allowed entry NaN
            x = base.copy(); x[allowed] = -inf; rows.append((s, x))                                              # only -inf allowed
            x = base.copy(); x[t[s] == BANNED] = inf; rows.append((s, x))                                        # +inf banned
            x = np.full(300, nan, np.float32); rows.append((s, x))
        assert empty_rows >= 1 and len(rows) >= 30
        for s, x in rows:
            assert c.pick(s, x) == dfa_ref.pick(t[s], x), s
            assert c.mask_row(s, x).tobytes() == dfa_ref.mask(t[s], x).tobytes()
        x = rows[0][1].copy()
        x.view(np.uint32)[5] = 0x7FC12345                               # a NaN payload on an allowed entry survives the mask bit for bit
        s = int(np.flatnonzero(t[:, 5] != BANNED)[0])
        assert c.mask_row(s, x).view(np.uint32)[5] == 0x7FC12345
        assert c.pick(-1, x) == -1 and c.pick(c.n_states, x) == -1
        with pytest.raises(L.LlamaHipError):
            c.mask_row(c.n_states, x)


PATTERNS = ["a", "ab", "a|b", "a*", "a+", "a?b", "(ab)*", "(a|b)*c", "a{2}", "a{1,3}", "a{2,}", "(ab|ba)+", "[ab]c", "[^a]", "[a-c]+d?", "a.c", ".*",
            "(a|bc)*d", "a(b|)c", "(?:ab){0,2}", "[^ab]*", "a\\.b|\\.", "(a*b*)*", "((a|b)(c|d))+", "a||b", "[a\\]]", "\\x61b", "[\\x61-\\x63]", "(ab?){2}",
            "(a+)(b+)?", "[.]a", "\\w+", "[\\w.]"]


def test_regex_dfa_against_re_fullmatch(L):
    from llama_swift_amd import regex_dfa
    words = [bytes(w) for n in range(5) for w in itertools.product(b"abc.", repeat=n)] + [bytes(w) for n in range(4) for w in itertools.product(b"abcd", repeat=n)]
    words += [b"]", b"a]", b"\n", b"a\nc", b"_", b"a_9"]
    for pat in PATTERNS:
        dfa = regex_dfa.compile(pat)
        rx = re.compile(pat.encode())
        assert dfa[0].dtype == np.int32 and dfa[0].shape[1] == 256 and dfa[2] == 0
        for w in words:
            assert regex_dfa.matches(dfa, w) == (rx.fullmatch(w) is not None), (pat, w)
    assert regex_dfa.matches(regex_dfa.compile("(é)+x"), "ééx".encode())      # (a str pattern is its UTF-8 bytes)
    for bad in ("(", "a)", "*a", "a**", "a*?", "[a", "a{2,1}", "a{x}", "\\", "(?=a)", "^a", "a$", "\\b", "[b-a]", "a{5000}", "(a{4000}){4000}"):
        with pytest.raises(regex_dfa.RegexError):
            regex_dfa.compile(bad)


def test_every_refusal_names_its_limit(L, tmp_path):
    vocab = synth.make_vocab(48)
    trans, accept = dfa_of(2, {(0, ord("a")): 1, (1, ord("b")): 0}, [1])
    with model_with(L, tmp_path, vocab) as m:
        def refused(text, trans=trans, accept=accept, start=0, stop=2, n_states=None):
            import ctypes as C
            err, c = C.create_string_buffer(512), C.c_void_p()
            tr = None if trans is None else np.ascontiguousarray(trans, np.int32)
            ac = None if accept is None else np.ascontiguousarray(accept, np.uint8)
            p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
            n = n_states if n_states is not None else tr.shape[0]
            rc = L.lib().llamahip_constraint_new(m._h, n, p(tr), p(ac), start, stop, C.byref(c), err, len(err))
            assert rc == -1001 and not c.value and err.value.decode() == "llamahip_constraint_new: " + text, err.value
        refused("trans is NULL", trans=None, n_states=2)
        refused("accept is NULL", accept=None)
        refused("n_states 0 outside 1 .. 4096", n_states=0)
        refused("n_states 4097 outside 1 .. 4096", n_states=4097)
        bad = trans.copy(); bad[1, 7] = 2
        refused("trans[1][7] = 2 outside [-1, 2)", trans=bad)
        bad = trans.copy(); bad[0, 255] = -2
        refused("trans[0][255] = -2 outside [-1, 2)", trans=bad)
        refused("start 2 out of range [0, 2)", start=2)
        refused("start -1 out of range [0, 2)", start=-1)
        refused("stop_token 48 out of range [0, 48)", stop=48)
        refused("stop_token -1 out of range [0, 48)", stop=-1)
        refused("no accepting state among the 2", accept=np.zeros(2, np.uint8))
        import ctypes as C
        err, c = C.create_string_buffer(512), C.c_void_p()
        assert L.lib().llamahip_constraint_new(None, 2, trans.ctypes.data_as(C.c_void_p), accept.ctypes.data_as(C.c_void_p), 0, 2, C.byref(c), err, len(err)) == -1001
        assert err.value.decode() == "llamahip_constraint_new: model is NULL"
        assert L.lib().llamahip_constraint_new(m._h, 2, trans.ctypes.data_as(C.c_void_p), accept.ctypes.data_as(C.c_void_p), 0, 2, None, err, len(err)) == -1001
        assert err.value.decode() == "llamahip_constraint_new: out is NULL"
        for strings, text in (([], "n must be >= 1 (got 0)"), ([b"a", b""], "strings[1] is empty (length 0): a choice has at least one byte"),
                              ([b"x" * 5000], "the trie of the choices has more than 4096 states (n_states outside 1 .. 4096)")):
            with pytest.raises(L.LlamaHipError) as e:
                m.constraint(choices=strings)
            assert e.value.message == "llamahip_constraint_new_choices: " + text
        with pytest.raises(L.LlamaHipError) as e:
            m.constraint(choices=[b"a"], stop_token=48)
        assert e.value.message == "llamahip_constraint_new_choices: stop_token 48 out of range [0, 48)"
        # the decode entry point: the arguments first, the handle last (HOST_ONLY)
        with m.constraint(dfa=(trans, accept, 0)) as c1:
            for kw, text in ((dict(state=3), "state 3 out of range [0, 3)"), (dict(state=-1), "state -1 out of range [0, 3)"),
                             (dict(first_token=48), "token id 48 out of range [0, 48)"), (dict(n_steps=0), "n_steps must be >= 1 (got 0)"),
                             (dict(n_past=10, n_steps=7), "context overflow: n_past (10) + n_steps (7) > n_ctx (16)"),
                             (dict(n_past=-1), "context overflow: n_past (-1) + n_steps (4) > n_ctx (16)")):
                args = dict(first_token=3, n_past=0, n_steps=4, constraint=c1)
                args.update(kw)
                with pytest.raises(L.LlamaHipError) as e:
                    m.decode_greedy_constrained(**args)
                assert e.value.message == "llamahip_decode_greedy_constrained: " + text
            with pytest.raises(L.LlamaHipError, match="llamahip_decode_greedy_constrained: .*HOST_ONLY"):
                m.decode_greedy_constrained(3, 0, 16, c1)
            with model_with(L, tmp_path, vocab, "other.bin") as m2:
                with pytest.raises(L.LlamaHipError) as e:
                    m2.decode_greedy_constrained(3, 0, 4, c1)
                assert e.value.message == "llamahip_decode_greedy_constrained: the constraint was made on another handle"
    # a table over 256 MiB: 4096 states x 32 768 tokens x 2 bytes is the limit itself; one more token is over it
    big = synth.make_vocab(32770)
    with model_with(L, tmp_path, big, "big.bin") as mb:
        tr = np.full((4096, 256), -1, np.int32)
        with pytest.raises(L.LlamaHipError) as e:
            mb.constraint(dfa=(tr, np.ones(4096, np.uint8), 0))
        assert e.value.message == "llamahip_constraint_new: table of (4096 + 1) states x 32770 tokens x 2 bytes = 268517380 bytes over the limit of 268435456 (256 MiB)"
    # the per-op entry points refuse their operands before they look for a device
    lg, tab = np.zeros((2, 8), np.float32), np.zeros((3, 8), np.uint16)
    for call, text in ((lambda: L.op_pick_dfa(np.zeros((17, 8), np.float32), tab, [0] * 17, 0), "llamahip_op_pick_dfa: n_rows 17 outside 1 .. 16"),
                       (lambda: L.op_pick_dfa(lg, tab, [0, 0], 8), "llamahip_op_pick_dfa: fallback_token 8 out of range [0, 8)"),
                       (lambda: L.op_pick_dfa(lg, tab, [0, 0], -1), "llamahip_op_pick_dfa: fallback_token -1 out of range [0, 8)"),
                       (lambda: L.op_pick_dfa(lg, np.full((3, 8), 3, np.uint16), [0, 0], 0), "llamahip_op_pick_dfa: table[0][0] = 3 is neither a state below 3 nor BANNED (65535)"),
                       (lambda: L.op_mask_rows_dfa(lg, tab, [0, 3]), "llamahip_op_mask_rows_dfa: states[1] = 3 out of range [0, 3)"),
                       (lambda: L.op_mask_rows_dfa(lg, tab, [-1, 0]), "llamahip_op_mask_rows_dfa: states[0] = -1 out of range [0, 3)")):
        with pytest.raises(L.LlamaHipError) as e:
            call()
        assert e.value.message == text


def test_constrain_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: constrain.cpp (the lift on the model file's vocabulary against the rule restated, a prune case, every refusal at short and
    missing message buffers, the choices builder, pick / mask_row / advance) compiled with -fsanitize=address,undefined into the stand-alone
    tools/host_sanitize and run there -- never loaded into python"""
    subprocess.run(["make", "-s", "-C", CSRC, "asan"], check=True)
    src = open(os.path.join(CSRC, "tools", "host_sanitize.cpp")).read()
    for fn in ("llamahip_constraint_new(", "llamahip_constraint_new_choices(", "llamahip_constraint_pick(", "llamahip_constraint_mask_row(",
               "llamahip_constraint_advance(", "llamahip_constraint_table(", "llamahip_constraint_free("):
        assert fn in src, fn
    assert "constrain.cpp" in open(os.path.join(CSRC, "Makefile")).read().split("asan:")[1].split("tools:")[0]
    path = str(tmp_path / "m.bin")
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(CSRC, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout and "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if "constraints:" in ln]
    assert len(line) == 1 and " 0 " not in line[0], r.stdout
