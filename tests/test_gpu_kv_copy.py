"""GPU (-m gpu): llamahip_kv_copy_rows / k_kv_copy_rows -- KV rows of every layer, K and V, from one slot to the same rows of another.

Every slot of a handle is filled with a full-context eval of its own random prompt and every row of every slot and layer is read; after a
copy everything is read again: the destination ranges hold the source's bits and EVERY OTHER ROW OF EVERY SLOT AND LAYER IS UNCHANGED.
Shapes: 3 layers of width 256 (the odd count catches layer x K/V indexing), width 384 with three heads of 128 (a row that is not a
power-of-two number of bytes), a 2-stage pipeline handle with both stages on device 0.  n_ctx 160, 5 slots; the case of 16 copies in one
call needs 16 destinations (a destination takes part in one copy of a call) and runs on a handle with 20 slots."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
N_CTX, N_SEQ = 160, 5


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


SHAPES = {
    "layers3": (synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=4, n_layer=3), {}),
    "width384": (synth.HParams(n_vocab=1500, n_embd=384, n_mult=64, n_head=3, n_layer=2), {}),
    "pipe2": (synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=2, n_layer=3), dict(devices=[0, 0])),
}


def read_all(hm, hp, n_seq):
    """[slot][layer] -> (K, V), all n_ctx rows; the handle's current slot is put back to the last one"""
    out = []
    for s in range(n_seq):
        hm.set_seq(s)
        out.append([hm.kv(il, N_CTX) for il in range(hp.n_layer)])
    hm.set_seq(n_seq - 1)
    return out


def fill(hm, hp, n_seq, seed):
    for s in range(n_seq):
        hm.set_seq(s)
        hm.eval(synth.synth_prompt(N_CTX + 1, hp.n_vocab, seed=seed + 17 * s)[1:], 0, 8)          # (without the BOS: row 0 differs too)
    hm.set_seq(n_seq - 1)
    kv = read_all(hm, hp, n_seq)
    for s in range(n_seq):          # the slots differ from each other: a copy from the wrong slot shows (a row of the last layer depends on
        for t in range(s):          # every token up to it: at most row 0 can coincide, where two prompts begin with the same token)
            assert np.count_nonzero(np.all(kv[s][-1][0] == kv[t][-1][0], axis=1)) <= 1
    return kv


def copy_and_check(hm, hp, n_seq, before, copies, note):
    """the copy, then every row of every slot and layer against `before` with the named ranges replaced; returns the new state"""
    hm.kv_copy_rows(copies)
    after = read_all(hm, hp, n_seq)
    for s in range(n_seq):
        for il in range(hp.n_layer):
            for w in (0, 1):
                want = before[s][il][w].copy()
                for src, dst, r0, n in copies:
                    if dst == s:
                        want[r0:r0 + n] = before[src][il][w][r0:r0 + n]
                assert same(after[s][il][w], want), (note, f"slot {s} layer {il} {'KV'[w]}", np.flatnonzero(np.any(after[s][il][w] != want, axis=1))[:8])
    return after


@pytest.fixture(scope="module", params=list(SHAPES), ids=list(SHAPES))
def filled(request, L, tmp_path_factory):
    hp, opts = SHAPES[request.param]
    path = str(tmp_path_factory.mktemp("kvcopy") / f"{request.param}.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=211))
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, **opts) as hm:
        yield request.param, hp, path, hm, {"kv": fill(hm, hp, N_SEQ, 4000)}


CASES = [
    ("one row at row 0", [(0, 1, 0, 1)]),
    ("one row at n_ctx - 1", [(2, 3, N_CTX - 1, 1)]),
    ("37 rows from row 5", [(4, 0, 5, 37)]),          # a byte count that is no multiple of any tile
    ("a broadcast to four destinations", [(3, 0, 9, 40), (3, 1, 9, 40), (3, 2, 9, 40), (3, 4, 9, 40)]),
    ("an empty entry beside a copy", [(0, 1, 20, 0), (2, 4, 100, 60)]),
    ("all n_ctx rows", [(1, 2, 0, N_CTX)]),
]


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0].replace(" ", "_") for c in CASES])
def test_copied_rows_are_the_sources_bits_and_nothing_else_changes(L, filled, case):
    kind, hp, _, hm, state = filled
    note, copies = CASES[case]
    state["kv"] = copy_and_check(hm, hp, N_SEQ, state["kv"], copies, (kind, note))


def test_sixteen_copies_in_one_call(L, tmp_path):
    """16 copies of different lengths, a zero among them, from four sources into 16 destinations: a destination takes part in one copy of a
    call, so the handle has 20 slots"""
    hp, n_seq = SHAPES["layers3"][0], 20
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=211))
    lens = [1, 2, 0, 9, 37, 160, 5, 64, 3, 100, 17, 33, 8, 127, 50, 11]
    copies = [(i % 4, 4 + i, (N_CTX - n) * (i % 3) // 2, n) for i, n in enumerate(lens)]
    assert len(copies) == 16 and all(r + n <= N_CTX for _, _, r, n in copies)
    with L.Model(path, n_ctx=N_CTX, n_seq=n_seq) as hm:
        before = fill(hm, hp, n_seq, 5000)
        copy_and_check(hm, hp, n_seq, before, copies, "16 copies")


def test_refusals_on_a_live_handle(L, filled):
    kind, hp, _, hm, state = filled
    ERR = L.binding.ERR_PREDICT
    for copies, word in (([(0, 1, 0, 4), (1, 2, 0, 4)], "destination of copy"),          # slot 1: written and read by one call
                         ([(0, 2, 0, 4), (1, 2, 8, 4)], "destination of copy"),
                         ([(0, 0, 0, 4)], "same slot"), ([(0, N_SEQ, 0, 4)], "n_seq"), ([(0, 1, N_CTX - 3, 4)], "n_ctx")):
        with pytest.raises(L.LlamaHipError) as e:
            hm.kv_copy_rows(copies)
        assert e.value.code == ERR and word in e.value.message, (kind, copies, e.value.message)
    # a live scheduler owns the slots below its max_active: nothing may be written there; above them the caller copies as before
    with hm.scheduler(max_active=3, chunk_tokens=9):
        for dst in (0, 2):
            with pytest.raises(L.LlamaHipError) as e:
                hm.kv_copy_rows([(4, dst, 0, 4)])
            assert e.value.code == ERR and "max_active" in e.value.message, (kind, e.value.message)
        with pytest.raises(L.LlamaHipError) as e:
            hm.kv_copy_rows([(0, 3, 0, 4), (4, 1, 0, 4)])
        assert "max_active" in e.value.message
        now = read_all(hm, hp, N_SEQ)          # (nothing moved by what was refused)
        for s in range(N_SEQ):
            for il in range(hp.n_layer):
                assert same(now[s][il][0], state["kv"][s][il][0]) and same(now[s][il][1], state["kv"][s][il][1]), (kind, s, il)
        state["kv"] = copy_and_check(hm, hp, N_SEQ, state["kv"], [(1, 3, 30, 12), (0, 4, 0, 5)], (kind, "beside a live scheduler"))
    state["kv"] = copy_and_check(hm, hp, N_SEQ, state["kv"], [(4, 0, 11, 21)], (kind, "after the scheduler is gone"))
