"""GPU (-m gpu): the in-place KV shift at model level -- llamahip_kv_shift_rows, decode_greedy_window(mode=CTX_SHIFT), the runner's mode 4.

The shift is NOT the reference's arithmetic, so nothing here is compared with the oracle's evals.  What is claimed is tested bit for bit:
kv_shift_rows leaves the float64 numpy restatement's bytes (tests/kv_shift_ref.py) and touches nothing else; the window loop equals
decode_greedy legs with kv_shift_rows calls between them; the runner equals the loop over the binding that shifts at the wall.  Two checks
need no restatement: a layer-0 row depends on its own token and position only, so after one crossing a shift handle and a re-eval handle
hold byte-equal layer-0 V rows and layer-0 K rows within the derived rounding bound -- and a deeper layer must differ, or the shift mode
would be the re-eval in disguise.  Small synthetic files, n_ctx 48; n_ctx 96 for crossings of more than 32 rows whose ranges do not alias."""
import os

import numpy as np
import pytest

import kv_shift_ref as R
import synth
from conftest import synth_tool

pytestmark = pytest.mark.gpu
N_CTX, N_SEQ, N_PROMPT, N_STEPS = 48, 3, 20, 140
NO_GRAPH = 1
HP256 = synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=4, n_layer=3)
HP384 = synth.HParams(n_vocab=1500, n_embd=384, n_mult=64, n_head=3, n_layer=2)
SMALL = dict(n_vocab=2000, n_embd=512, n_mult=256, n_head=4, n_layer=3)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def model_file(L, tmp, kind):
    """q4_0 files of both widths, and an f16 and a Q4_1 file of width 256"""
    hp = HP384 if kind == "w384" else HP256
    path = os.path.join(str(tmp), f"{kind}.bin")
    if kind in ("f16", "q41"):
        src = path + ".f16" if kind == "q41" else path
        synth.write_model_unquantized(src, hp, synth.random_tensors(hp, seed=1701), 1)
        if kind == "q41":
            L.quantize_file(src, path, 3)
            os.remove(src)
    else:
        synth.write_model(path, hp, synth.random_tensors(hp, seed=211))
    return hp, path


def read_all(hm, hp, n_seq, n_ctx=N_CTX):
    """(K, V) f32 [slot, layer, n_ctx, d]; the handle's current slot is put back"""
    cur = hm.cur_seq
    K = np.empty((n_seq, hp.n_layer, n_ctx, hp.n_embd), np.float32)
    V = np.empty_like(K)
    for s in range(n_seq):
        hm.set_seq(s)
        for il in range(hp.n_layer):
            K[s, il], V[s, il] = hm.kv(il, n_ctx)
    hm.set_seq(cur)
    return K, V


def fill(hm, hp, n_seq, seed, n_ctx=N_CTX):
    for s in range(n_seq):
        hm.set_seq(s)
        hm.eval(synth.synth_prompt(n_ctx + 1, hp.n_vocab, seed=seed + 17 * s)[1:], 0, 8)
    hm.set_seq(1)
    return read_all(hm, hp, n_seq, n_ctx)


# ------------------------------------------------------------------------------------------------ 1. kv_shift_rows against the restatement
HANDLES = {"plain": ("w256", {}), "pipe2": ("w256", dict(devices=[0, 0])), "width384": ("w384", {}), "f16": ("f16", {}), "q41": ("q41", {})}
SHIFTS = [[(1, 24, 24, 24)],                        # the plan's even case: disjoint
          [(0, 24, 24, 23)],                        # its odd case: one row of overlap
          [(2, 1, 47, 1), (0, 10, 0, 4)],           # maximal overlap beside an empty entry
          [(0, 47, 1, 47), (1, 11, 37, 7), (2, 30, 5, 10)]]


@pytest.mark.parametrize("kind", list(HANDLES))
def test_kv_shift_rows_leaves_the_restatements_bytes_and_nothing_else(L, tmp_path, kind):
    file_kind, opts = HANDLES[kind]
    hp, path = model_file(L, tmp_path, file_kind)
    tab = L.rope_table(N_CTX, hp.n_embd // hp.n_head)
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, **opts) as hm:
        K, V = fill(hm, hp, N_SEQ, 4000)
        assert R.no_subnormals(K) and R.no_subnormals(V)
        for shifts in SHIFTS:
            R.shift_restated(K, V, tab, hp.n_embd // hp.n_head, shifts)
            assert R.no_subnormals(K)
            hm.kv_shift_rows(shifts)
            assert hm.cur_seq == 1          # the current slot is left alone
            gotK, gotV = read_all(hm, hp, N_SEQ)
            for s in range(N_SEQ):
                for il in range(hp.n_layer):
                    assert same(gotK[s, il], K[s, il]), (kind, shifts, f"K slot {s} layer {il}", np.flatnonzero(np.any(gotK[s, il] != K[s, il], axis=1))[:8])
                    assert same(gotV[s, il], V[s, il]), (kind, shifts, f"V slot {s} layer {il}", np.flatnonzero(np.any(gotV[s, il] != V[s, il], axis=1))[:8])


BANDS_CTX = 96
BAND_SHIFTS = [[(1, 48, 48, 48)],                                  # the plan's crossing at n_ctx 96, n_keep 0: 48 rows, disjoint ranges
               [(0, 53, 43, 53), (2, 33, 63, 33)],                 # n_keep 10: 43 rows beside an aliasing shift
               [(2, 48, 33, 40), (1, 1, 95, 1)]]


@pytest.mark.parametrize("kind", ["plain", "pipe2"])
def test_kv_shift_rows_of_long_disjoint_ranges(L, tmp_path, kind):
    """n_ctx 96: shifts of more than 32 rows whose ranges do not alias -- what every crossing at a real context size is -- against the
    restatement's bytes, nothing else changed"""
    file_kind, opts = HANDLES[kind]
    hp, path = model_file(L, tmp_path, file_kind)
    dh = hp.n_embd // hp.n_head
    tab = L.rope_table(BANDS_CTX, dh)
    assert any(32 < n <= nd for sh in BAND_SHIFTS for _, _, n, nd in sh)
    with L.Model(path, n_ctx=BANDS_CTX, n_seq=N_SEQ, **opts) as hm:
        K, V = fill(hm, hp, N_SEQ, 4200, BANDS_CTX)
        for shifts in BAND_SHIFTS:
            R.shift_restated(K, V, tab, dh, shifts)
            assert R.no_subnormals(K)
            hm.kv_shift_rows(shifts)
            gotK, gotV = read_all(hm, hp, N_SEQ, BANDS_CTX)
            for s in range(N_SEQ):
                for il in range(hp.n_layer):
                    assert same(gotK[s, il], K[s, il]), (kind, shifts, f"K slot {s} layer {il}", np.flatnonzero(np.any(gotK[s, il] != K[s, il], axis=1))[:8])
                    assert same(gotV[s, il], V[s, il]), (kind, shifts, f"V slot {s} layer {il}", np.flatnonzero(np.any(gotV[s, il] != V[s, il], axis=1))[:8])


# ------------------------------------------------------------------------------------------------ 2. refusals on a live handle
def test_refusals_on_a_live_handle(L, tmp_path):
    hp, path = model_file(L, tmp_path, "w256")
    ERR = L.binding.ERR_PREDICT
    with L.Model(path, n_ctx=N_CTX, n_seq=5) as hm:
        K, V = fill(hm, hp, 5, 4100)
        for shifts, word in (([(0, 4, 2, 1), (0, 20, 2, 2)], "one shift of a call"), ([(5, 4, 2, 1)], "n_seq"), ([(0, N_CTX - 1, 2, 1)], "n_ctx"),
                             ([(0, 4, 2, 0)], "n_discard"), ([(0, 4, 2, 5)], "below row 0"), ([], "1 .. 16")):
            with pytest.raises(L.LlamaHipError) as e:
                hm.kv_shift_rows(shifts)
            assert e.value.code == ERR and word in e.value.message, (shifts, e.value.message)
        # a live scheduler owns the slots below its max_active: nothing may be written there; above them the caller shifts as before
        with hm.scheduler(max_active=3, chunk_tokens=9):
            for slot in (0, 2):
                with pytest.raises(L.LlamaHipError) as e:
                    hm.kv_shift_rows([(slot, 8, 4, 2)])
                assert e.value.code == ERR and "max_active" in e.value.message, e.value.message
            with pytest.raises(L.LlamaHipError) as e:
                hm.kv_shift_rows([(4, 8, 4, 2), (1, 8, 4, 2)])
            assert "max_active" in e.value.message
            gotK, gotV = read_all(hm, hp, 5)
            assert same(gotK, K) and same(gotV, V)          # (nothing moved by what was refused)
            shifts = [(3, 30, 12, 30), (4, 5, 20, 3)]
            R.shift_restated(K, V, L.rope_table(N_CTX, 64), 64, shifts)
            hm.kv_shift_rows(shifts)
            gotK, gotV = read_all(hm, hp, 5)
            assert same(gotK, K) and same(gotV, V), "beside a live scheduler"
        shifts = [(0, 11, 21, 11)]
        R.shift_restated(K, V, L.rope_table(N_CTX, 64), 64, shifts)
        hm.kv_shift_rows(shifts)
        gotK, gotV = read_all(hm, hp, 5)
        assert same(gotK, K) and same(gotV, V), "after the scheduler is gone"


# ------------------------------------------------------------------------------------------------ 3. the loop against its parts
def legs_with_shifts(L, h, first, n_steps, n_past, n_keep, n_ctx=N_CTX):
    """decode_greedy in legs; at the wall the plan and ONE kv_shift_rows call of the surviving rows of the current slot"""
    pos, pending, out, lg = n_past, first, [], None
    while len(out) < n_steps:
        if pos == n_ctx:
            new, nd = L.ctx_overflow_plan(n_ctx, pos, n_keep)
            assert new > 0
            h.kv_shift_rows([(h.cur_seq, n_keep + nd, pos - n_keep - nd, nd)])
            pos = new
        leg = min(n_steps - len(out), n_ctx - pos)
        if len(out) + leg == n_steps:
            toks, lg = h.decode_greedy(pending, pos, leg, want_logits=True)
        else:
            toks = h.decode_greedy(pending, pos, leg)
        out += toks.tolist()
        pending, pos = int(toks[-1]), pos + leg
    return np.array(out, np.int32), pos, lg


LOOPS = {"graph": ("w256", {}), "no_graph": ("w256", dict(flags=NO_GRAPH)), "pipe2": ("w256", dict(devices=[0, 0])), "f16": ("f16", {})}


@pytest.mark.parametrize("kind", list(LOOPS))
def test_shift_window_is_decode_greedy_legs_with_kv_shift_rows_between(L, tmp_path, kind):
    """140 steps from a 20-token context at n_ctx 48 (the wall is crossed five times or more) at n_keep 0, 6 and 5 (an odd remainder: one row
    of overlap at every crossing): tokens, last logits, n_past_out and KV rows [0, n_past_out) of every layer, byte for byte"""
    file_kind, opts = LOOPS[kind]
    hp, path = model_file(L, tmp_path, file_kind)
    prompt = synth.synth_prompt(N_PROMPT, hp.n_vocab, seed=5)
    with L.Model(path, n_ctx=N_CTX, **opts) as a, L.Model(path, n_ctx=N_CTX, **opts) as b:
        for n_keep in (0, 6, 5):
            first = int(np.argmax(a.eval(prompt, 0, 8)))
            assert int(np.argmax(b.eval(prompt, 0, 8))) == first
            got, pos, lg = a.decode_greedy_window(first, N_STEPS, N_PROMPT, prompt, n_keep=n_keep, mode=L.CTX_SHIFT, chunk_tokens=9, n_threads=8, want_logits=True)
            want, want_pos, want_lg = legs_with_shifts(L, b, first, N_STEPS, N_PROMPT, n_keep)
            assert got.tolist() == want.tolist(), (kind, n_keep, "tokens")
            assert pos == want_pos and same(lg, want_lg), (kind, n_keep, "n_past_out / last logits")
            for il in range(hp.n_layer):
                ka, va = a.kv(il, pos)
                kb, vb = b.kv(il, pos)
                assert same(ka, kb) and same(va, vb), (kind, n_keep, f"KV rows of layer {il}")


def test_shift_window_with_longer_crossings(L, tmp_path):
    """the same at n_ctx 96 over 250 steps, n_keep 0 (48 rows move) and 10 (43 rows); the bytes the moved rows must hold are
    test_kv_shift_rows_of_long_disjoint_ranges'"""
    hp, path = model_file(L, tmp_path, "w256")
    prompt = synth.synth_prompt(N_PROMPT, hp.n_vocab, seed=5)
    with L.Model(path, n_ctx=BANDS_CTX) as a, L.Model(path, n_ctx=BANDS_CTX) as b:
        for n_keep in (0, 10):
            first = int(np.argmax(a.eval(prompt, 0, 8)))
            assert int(np.argmax(b.eval(prompt, 0, 8))) == first
            got, pos, lg = a.decode_greedy_window(first, 250, N_PROMPT, prompt, n_keep=n_keep, mode=L.CTX_SHIFT, chunk_tokens=0, n_threads=8, want_logits=True)
            want, want_pos, want_lg = legs_with_shifts(L, b, first, 250, N_PROMPT, n_keep, BANDS_CTX)
            assert got.tolist() == want.tolist() and pos == want_pos and same(lg, want_lg), n_keep
            for il in range(hp.n_layer):
                ka, va = a.kv(il, pos)
                kb, vb = b.kv(il, pos)
                assert same(ka, kb) and same(va, vb), (n_keep, f"KV rows of layer {il}")


# ------------------------------------------------------------------------------------------------ 4. / 5. against the re-eval, one crossing
def test_one_crossing_against_the_reeval_layer_0_agrees_deeper_layers_differ(L, tmp_path):
    """29 steps from 20 tokens at n_keep 6: 28 steps fill the cache, the plan drops 21 rows, one more step.  Both handles then hold the same
    28 tokens at the same positions.  Layer 0: V byte-equal; K byte-equal in the kept rows and in the row evaluated after the crossing, within
    3.5 * 2^-24 * ||pair|| in the moved rows (||pair|| taken from the re-eval handle's key: a rotation keeps it up to 2^-24).  A deeper layer's
    moved K rows attended to the dropped tokens when they were computed: at least one differs from the re-eval's"""
    hp, path = model_file(L, tmp_path, "w256")
    prompt = synth.synth_prompt(N_PROMPT, hp.n_vocab, seed=5)
    n_keep, n_steps = 6, N_CTX - N_PROMPT + 1
    res = {}
    for mode in (L.CTX_SHIFT, L.CTX_REEVAL):
        with L.Model(path, n_ctx=N_CTX) as h:
            first = int(np.argmax(h.eval(prompt, 0, 8)))
            toks, pos = h.decode_greedy_window(first, n_steps, N_PROMPT, prompt, n_keep=n_keep, mode=mode, chunk_tokens=0)
            res[mode] = (toks, pos, [h.kv(il, pos) for il in range(hp.n_layer)])
    (ts, ps, kvs), (tr, pr, kvr) = res[L.CTX_SHIFT], res[L.CTX_REEVAL]
    new, nd = L.ctx_overflow_plan(N_CTX, N_CTX, n_keep)
    assert ps == pr == new + 1 and ts[:-1].tolist() == tr[:-1].tolist()          # (the last pick comes after the crossing: it may differ)
    moved = slice(n_keep, new)
    (k0s, v0s), (k0r, v0r) = kvs[0], kvr[0]
    assert same(v0s, v0r), "layer 0 V rows"
    assert same(k0s[:n_keep], k0r[:n_keep]) and same(k0s[new:], k0r[new:]), "layer 0 K rows that did not move"
    worst = R.within_bound(k0s[moved], k0r[moved], k0r[moved])
    print(f"layer 0 moved K rows: worst |shift - re-eval| / (2^-24 ||pair||) = {worst:.3f} (bound 3.5)")
    assert worst < 3.5
    assert not same(k0s[moved], k0r[moved]), "the moved keys were narrowed twice: some bits differ"
    differ = [il for il in range(1, hp.n_layer) if np.any(kvs[il][0][moved] != kvr[il][0][moved])]
    assert differ, "a shift mode that runs the re-eval"


# ------------------------------------------------------------------------------------------------ 6. the runner
def runner_tokens(L, path, prompt_text, n_tokens, overflow=None, lookup=None, greedy=False, seed=11, n_keep=-1):
    r = L.LlamaRunner(path)
    if overflow is not None:
        r.set_overflow(overflow, n_keep)
    if lookup is not None:
        r.set_lookup(lookup)
    try:
        return r.run(prompt_text, L.Config(numThreads=8, numTokens=n_tokens, n_ctx=N_CTX, greedy=greedy, seed=seed))
    finally:
        r.close()


def binding_loop_with_shift(L, h, prompt_ids, n_tokens, greedy, seed, n_keep=-1):
    """the generation loop over the binding: eval_topk -> draw -> accept (greedy: eval -> argmax); at the wall the plan, then ONE
    kv_shift_rows call.  Returns the generated ids."""
    s = L.Sampler(seed, 64)
    P = len(prompt_ids)
    keep = min(P if n_keep < 0 else n_keep, N_CTX // 2)
    h.eval(np.array([0, 1, 2, 3], np.int32), 0, 8)
    for t in prompt_ids:
        s.accept(int(t))
    n_full = ((P - 1) // 9) * 9 if P > 9 else 0
    if n_full:
        h.eval_chunks(prompt_ids[:n_full], 0, 9, 8)
    pos, pending, out = n_full, np.asarray(prompt_ids[n_full:], np.int32), []
    while True:
        if pos + len(pending) > N_CTX:
            assert len(pending) == 1 and pos == N_CTX
            new, nd = L.ctx_overflow_plan(N_CTX, pos, keep)
            h.kv_shift_rows([(0, keep + nd, pos - keep - nd, nd)])
            pos = new
        if greedy:
            tid = int(np.argmax(h.eval(pending, pos, 8)))
        else:
            exact, sc, ids, lg = h.eval_topk(pending, pos, s)
            tid = s.sample_from_candidates(sc, ids) if exact else s.sample(h, lg)
        pos += len(pending)
        s.accept(tid)
        out.append(tid)
        if len(out) == n_tokens:
            return out
        pending = np.array([tid], np.int32)


@pytest.fixture(scope="module")
def runner_model(tmp_path_factory):
    return synth_tool(tmp_path_factory.mktemp("shift_runner") / "m.bin", seed=94, **SMALL)


def _prompt_text(h, V):
    ids = synth.synth_prompt(14, V, seed=21)[1:]
    text = b"".join(h.token_text(int(t)) for t in ids).decode(errors="ignore")
    return text, h.tokenize(text)


def test_runner_in_shift_mode_is_the_binding_loop_that_shifts(L, runner_model, monkeypatch):
    """numberOfTokens 120 at n_ctx 48: the OUTPUT_TOKEN events are the prompt's tokens and then the ids of the Python loop over the binding on
    a second handle with the same seed -- sampled, sampled with lookup steps, greedy, and with an explicit n_keep; mode 2 is still mode 0"""
    monkeypatch.delenv("LLAMAHIP_RUNNER_OVERFLOW", raising=False)
    with L.Model(runner_model, n_ctx=N_CTX) as h:
        text, ids = _prompt_text(h, SMALL["n_vocab"])
        P = len(ids)
        assert 2 <= P < N_CTX // 2
        echo = [h.token_text(int(t)) for t in ids]
        for greedy, n_keep in ((False, -1), (True, -1), (False, 3)):
            want = echo + [h.token_text(t) for t in binding_loop_with_shift(L, h, ids, 120, greedy, seed=11, n_keep=n_keep)]
            got = runner_tokens(L, runner_model, text, 120, overflow=L.CTX_SHIFT, greedy=greedy, n_keep=n_keep)
            assert len(got) == P + 120 and got == want, (greedy, n_keep)
            if not greedy:
                assert runner_tokens(L, runner_model, text, 120, overflow=L.CTX_SHIFT, lookup=4, n_keep=n_keep) == want, ("lookup on", n_keep)
            if (greedy, n_keep) == (False, -1):
                sampled = want
    stop = runner_tokens(L, runner_model, text, 120, overflow=0)
    assert len(stop) == P + (N_CTX - P)
    assert runner_tokens(L, runner_model, text, 120, overflow=2) == stop          # a mode the runner does not have is mode 0
    assert sampled[:len(stop)] == stop                                           # the same stream up to the wall
    # a bridge that never calls the setter takes the mode from the environment
    monkeypatch.setenv("LLAMAHIP_RUNNER_OVERFLOW", "shift")
    assert runner_tokens(L, runner_model, text, 120) == sampled
