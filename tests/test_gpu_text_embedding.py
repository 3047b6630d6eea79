"""GPU (-m gpu): llamahip_text_embedding and llamahip_text_embedding_multi -- a text's pooled final-norm rows, several texts per weight pass.

Against the oracle: its hidden rows after the last layer (the evals of `chunk_tokens` rows one after the other, the last layer's output rows
from the per-layer dump), the reference's norm times norm.weight and tests/pool_ref.py.  Every hidden row is asserted order-proof for the
norm, so the comparison is by bytes.  The multi call against set_seq + text_embedding per slot on a second handle, its KV rows against
llamahip_eval_multi's on a third; KV rows outside the appended ranges, slots the call does not name and the current slot keep what they had.
No tolerance anywhere."""
import os

import numpy as np
import pytest

import pool_ref
import prep_cases as pc
import synth

pytestmark = pytest.mark.gpu
N_CTX, N_SEQ = 192, 6
NO_GRAPH = 1
HP = synth.HParams(n_vocab=2000, n_embd=256, n_mult=64, n_head=4, n_layer=2)
MODEL_SEED = 44
TEXT_LENS = (1, 9, 10, 17, 64)
PREFIX = 5          # the n_past > 0 of the single-text cases
VARIANTS = [(pool, normalize) for pool in ("last", "mean") for normalize in (False, True)]
# the mixed segments of the multi call: rows, n_past, slots (never ascending); slot 5 is named by no call
LENS, PAST, SLOTS = [1, 9, 10, 17, 3], [0, 5, 0, 20, 40], [3, 0, 4, 1, 2]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def text_of(n, seed):
    return synth.synth_prompt(max(n, 2), HP.n_vocab, seed=seed)[:n]


def tokens_of(lens, seed):
    return [text_of(n, seed + 7 * i) for i, n in enumerate(lens)]


def prefix_of(slot, n):
    return synth.synth_prompt(max(n, 2), HP.n_vocab, seed=900 + slot)[:n]


def kv_all(h, slots):
    out = {}
    for s in slots:
        h.set_seq(s)
        out[s] = [h.kv(il, N_CTX) for il in range(HP.n_layer)]
    return out


def prefill(handles, slots, n_past, nth=8):
    for h in handles:
        for s, p in zip(slots, n_past):
            if p > 0:
                h.set_seq(s)
                h.eval(prefix_of(s, p), 0, nth)


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("embed") / "m.bin")
    synth.write_model(path, HP, synth.random_tensors(HP, seed=MODEL_SEED))
    return path


@pytest.fixture(scope="module")
def om(oracle, model_path):
    m = oracle.load(model_path, n_ctx=N_CTX)
    yield m
    m.close()


@pytest.fixture(scope="module")
def norm_w(om):
    return om.tensor_bytes("norm.weight").view(np.float32).copy()


def oracle_hidden(om, toks, n_past, chunk, nth):
    """the hidden rows after the last layer: evals of `chunk` rows one after the other (chunk 0: one eval), the prefix first"""
    if n_past > 0:
        om.eval(prefix_of(0, n_past), 0, nth)
    step = chunk if chunk > 0 else len(toks)
    rows = []
    for c0 in range(0, len(toks), step):
        part = toks[c0:c0 + step]
        rows.append(om.eval(part, n_past + c0, nth, dump_layer=HP.n_layer - 1)["layer_out"].reshape(len(part), HP.n_embd))
    return np.ascontiguousarray(np.concatenate(rows), np.float32)


@pytest.mark.parametrize("nth", [8, 5])
@pytest.mark.parametrize("chunk", [0, 9])
@pytest.mark.parametrize("n_past", [0, PREFIX])
def test_text_embedding_against_the_oracle(L, oracle, om, norm_w, model_path, n_past, chunk, nth):
    with L.Model(model_path, n_ctx=N_CTX, n_seq=N_SEQ) as h:
        if n_past > 0:
            h.eval(prefix_of(0, n_past), 0, nth)
        for n in TEXT_LENS:
            toks = text_of(n, 100 + n)
            hid = oracle_hidden(om, toks, n_past, chunk, nth)
            assert all(pc.norm_stats(r)["proof"] for r in hid), ("a hidden row that is not order-proof: choose another text seed", n, n_past, chunk, nth)
            y = pool_ref.norm_rows(oracle, hid, norm_w)
            for pool, normalize in VARIANTS:
                want = pool_ref.pool_normed(y, [0, n], pool, normalize)[0]
                got = h.text_embedding(toks, n_past, nth, chunk, pool, normalize)
                bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                assert bad.size == 0, (n, n_past, chunk, nth, pool, normalize, f"{bad.size} elements differ, first at {bad[:4]}", got[bad[:4]], want[bad[:4]])
                if normalize:
                    assert abs(float(np.sqrt((got.astype(np.float64) ** 2).sum())) - 1.0) < 1e-6
            for il in range(HP.n_layer):
                assert all(same(a, b) for a, b in zip(h.kv(il, n_past + n), om.kv(il, n_past + n))), (n, n_past, chunk, nth, f"KV rows of layer {il}")


def check_multi(hm, hl, he, lens, n_past, slots, chunk, nth, pool, normalize, seed, note, n_passes=1):
    """one text_embedding_multi on hm against set_seq + text_embedding per slot on hl, and its KV rows against eval_multi's on he"""
    toks = tokens_of(lens, seed)
    before = kv_all(hm, range(N_SEQ))
    cur = slots[-1]
    hm.set_seq(cur)
    got, st = hm.text_embedding_multi(slots, n_past, toks, chunk_tokens=chunk, n_threads=nth, pool=pool, normalize=normalize, want_stats=True)
    k_cur, v_cur = hm.kv(0, N_CTX)          # (read through the handle's current slot, which the call must leave alone)
    assert got.shape == (len(lens), HP.n_embd)
    for i, s in enumerate(slots):
        hl.set_seq(s)
        want = hl.text_embedding(toks[i], n_past[i], nth, chunk, pool, normalize)
        assert same(got[i], want), (note, f"segment {i} (slot {s}, {lens[i]} rows at {n_past[i]})")
        assert np.isfinite(got[i]).all() and got[i].any()
    he.eval_multi(slots, n_past, toks, chunk_tokens=chunk, n_threads=nth)
    after, want_kv, single_kv = kv_all(hm, range(N_SEQ)), kv_all(he, slots), kv_all(hl, slots)
    assert same(k_cur, after[cur][0][0]) and same(v_cur, after[cur][0][1]), (note, "the handle's current slot moved")
    for s in range(N_SEQ):
        for il in range(HP.n_layer):
            for w in (0, 1):
                g, was = after[s][il][w], before[s][il][w]
                if s not in slots:
                    assert same(g, was), (note, f"slot {s} layer {il}: a slot the call does not name")
                    continue
                i = slots.index(s)
                end = n_past[i] + lens[i]
                assert same(g[:end], want_kv[s][il][w][:end]), (note, f"slot {s} layer {il} {'KV'[w]} rows [0, {end}) against eval_multi's")
                assert same(g[:end], single_kv[s][il][w][:end]), (note, f"slot {s} layer {il} {'KV'[w]} rows [0, {end}) against text_embedding's")
                assert same(g[:n_past[i]], was[:n_past[i]]) and same(g[end:], was[end:]), (note, f"slot {s} layer {il}: rows outside [{n_past[i]}, {end})")
    assert st["n_rows"] == sum(lens) and st["n_passes"] == n_passes, (note, st)
    return st


@pytest.fixture(scope="module")
def trio(L, model_path):
    with L.Model(model_path, n_ctx=N_CTX, n_seq=N_SEQ) as hm, L.Model(model_path, n_ctx=N_CTX, n_seq=N_SEQ) as hl, \
            L.Model(model_path, n_ctx=N_CTX, n_seq=N_SEQ) as he:
        prefill((hm, hl, he), SLOTS, PAST)
        yield hm, hl, he


@pytest.mark.parametrize("pool,normalize", VARIANTS, ids=lambda v: str(v))
def test_multi_is_the_per_slot_call(L, trio, pool, normalize):
    hm, hl, he = trio
    for chunk, nth in ((9, 8), (0, 5)):
        st = check_multi(hm, hl, he, LENS, PAST, SLOTS, chunk, nth, pool, normalize, seed=300 + chunk, note=(pool, normalize, chunk, nth))
        assert st["n_short_segs"] == 5 and st["n_long_segs"] == 0


def test_multi_with_a_long_segment_and_one_segment_alone(L, trio):
    """a segment of 70 rows takes attention launches of its own; one segment alone is the single-text call (n_passes = its evals)"""
    hm, hl, he = trio
    st = check_multi(hm, hl, he, [70, 9, 2], [0, 5, 40], [4, 0, 2], 9, 8, "mean", True, seed=400, note="long")
    assert st["n_long_segs"] == 1 and st["n_short_segs"] == 2
    st = check_multi(hm, hl, he, [23], [20], [1], 9, 8, "mean", False, seed=410, note="one segment")
    assert st["n_short_segs"] == 0 and st["n_long_segs"] == 0


def test_multi_against_the_oracle(L, oracle, om, norm_w, trio):
    """the one pass held to the reference directly, not only to the per-slot call: two fresh texts at n_past 0"""
    hm = trio[0]
    lens, slots = [10, 17], [5, 3]
    toks = tokens_of(lens, 500)
    for pool, normalize in VARIANTS:
        got = hm.text_embedding_multi(slots, [0, 0], toks, chunk_tokens=0, n_threads=8, pool=pool, normalize=normalize)
        for i, n in enumerate(lens):
            hid = oracle_hidden(om, toks[i], 0, 0, 8)
            assert all(pc.norm_stats(r)["proof"] for r in hid)
            want = pool_ref.pool_normed(pool_ref.norm_rows(oracle, hid, norm_w), [0, n], pool, normalize)[0]
            assert same(got[i], want), (pool, normalize, i)
    prefill((hm,), [3], [20])          # (slot 3's prefix back for the tests that follow)


@pytest.mark.parametrize("kind", ["pipe2", "no_graph", "f16", "q41"])
def test_other_handle_shapes(L, model_path, tmp_path, kind):
    """a two-stage in-process pipeline (both stages on device 0) and a NO_GRAPH handle take the one pass; f16 / Q4_1 files run the per-slot loop
    and report its eval count"""
    path, kw = model_path, {}
    if kind in ("f16", "q41"):
        path = str(tmp_path / f"d_{kind}.bin")
        src = path + ".f16" if kind == "q41" else path
        synth.write_model_unquantized(src, HP, synth.random_tensors(HP, seed=1701), 1)
        if kind == "q41":
            L.quantize_file(src, path, 3)
            os.remove(src)
    elif kind == "pipe2":
        kw = dict(devices=[0, 0])
    else:
        kw = dict(flags=NO_GRAPH)
    dense = kind in ("f16", "q41")
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, **kw) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hl, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as he:
        prefill((hm, hl, he), SLOTS, PAST)
        for chunk, nth, pool, normalize in ((9, 8, "mean", True), (0, 5, "last", False), (9, 8, "last", True), (0, 8, "mean", False)):
            # (f16 / Q4_1 files below 36 rows: one eval per chunk of 9; else one eval per segment)
            n_evals = (sum((n + 8) // 9 for n in LENS) if chunk else len(LENS)) if dense else 1
            e0 = hm.stats()["n_evals"]
            st = check_multi(hm, hl, he, LENS, PAST, SLOTS, chunk, nth, pool, normalize, seed=600 + chunk, note=(kind, chunk, nth, pool, normalize), n_passes=n_evals)
            assert hm.stats()["n_evals"] - e0 == n_evals
            assert (st["n_short_segs"], st["n_long_segs"]) == ((0, 0) if dense else (5, 0))


def test_eval_and_decode_after_an_embedding_call_give_the_bits_they_give_without_it(L, model_path):
    """the logits buffer, the logits row map and the captured graphs: an embedding call between an eval and a greedy decode changes nothing"""
    before = L.live_allocs()
    prompt = text_of(12, 700)
    with L.Model(model_path, n_ctx=N_CTX, n_seq=N_SEQ) as ha, L.Model(model_path, n_ctx=N_CTX, n_seq=N_SEQ) as hb:
        for h in (ha, hb):
            h.set_seq(2)
            first = h.eval(prompt, 0, 8)
            t0 = h.decode_greedy(int(np.argmax(first)), len(prompt), 4, 8)          # (captures the decode graphs)
        row = ha.stage_logits(0)          # (the texts below are no longer than the prompt: the workspace, which holds the logits, does not grow)
        e1 = ha.text_embedding(text_of(9, 701), len(prompt) + 4, 8, 0, "mean", True)          # on the current slot, behind the context
        e2 = ha.text_embedding_multi([4, 0], [0, 0], tokens_of([10, 3], 702), chunk_tokens=9, pool="last", normalize=True)
        assert np.isfinite(e1).all() and np.isfinite(e2).all()
        assert same(ha.stage_logits(0), row), "an embedding call wrote logits or moved the logits row map"
        outs = []
        for h in (ha, hb):
            tok, lg = h.decode_greedy(int(t0[-1]), len(prompt) + 4, 6, 8, want_logits=True)
            outs.append((tok, lg, h.eval(text_of(11, 703), len(prompt) + 10, 8)))
        assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1]) and same(outs[0][2], outs[1][2])
        # ... and the embedding of the same text again, after all that, has the same bits
        ha.set_seq(1)
        e3 = ha.text_embedding_multi([4, 0], [0, 0], tokens_of([10, 3], 702), chunk_tokens=9, pool="last", normalize=True)
        assert same(e2, e3)
    assert L.live_allocs() == before


def test_a_live_scheduler_keeps_its_slots(L, model_path):
    with L.Model(model_path, n_ctx=N_CTX, n_seq=N_SEQ) as h:
        toks = tokens_of([3, 4], 800)
        with L.Scheduler(h, max_active=2):
            with pytest.raises(L.LlamaHipError) as e:
                h.text_embedding_multi([1, 4], [0, 0], toks)
            assert e.value.message.startswith("llamahip_text_embedding_multi:") and "scheduler" in e.value.message
            h.set_seq(0)
            with pytest.raises(L.LlamaHipError) as e:
                h.text_embedding(toks[0])
            assert e.value.message.startswith("llamahip_text_embedding:") and "scheduler" in e.value.message
            assert h.text_embedding_multi([5, 4], [0, 0], toks).shape == (2, HP.n_embd)
        assert h.text_embedding_multi([1, 4], [0, 0], toks).shape == (2, HP.n_embd)


def test_the_embedding_tool_matches_the_python_api(L, model_path, tmp_path):
    """csrc/tools/embedding: 19 lines of text, 16 per pass and the rest in a second one; the vectors it prints are text_embedding's, the
    similarity matrix is symmetric with ones on its diagonal"""
    import subprocess
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc", "tools", "embedding")
    vocab = synth.make_vocab(HP.n_vocab)
    rng = np.random.default_rng(31)
    lines = ["".join(vocab[i].decode() for i in rng.integers(3, HP.n_vocab, size=2 + (5 * k) % 13)).replace("\n", " ").replace("\r", " ") for k in range(19)]
    lines = [ln for ln in lines if ln.strip()]
    f = tmp_path / "texts.txt"
    f.write_text("\n".join(lines) + "\n")
    r = subprocess.run([tool, model_path, "--file", str(f), "--pool", "mean", "--ctx", "64"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.array([[float(v) for v in ln.split()] for ln in r.stdout.strip().splitlines()], np.float64)
    assert got.shape == (len(lines), HP.n_embd) and f"texts {len(lines)} passes {(len(lines) + 15) // 16}" in r.stderr, r.stderr
    with L.Model(model_path, n_ctx=64) as m:
        for i, ln in enumerate(lines):
            want = m.text_embedding(m.tokenize(ln.encode(), bos=True)[:64], pool="mean", normalize=True)
            assert np.array_equal(got[i].astype(np.float32), want), i          # (%.9g round-trips a float32)
    r = subprocess.run([tool, model_path, "--file", str(f), "--pool", "last", "--cosine", "--ctx", "64", "--batch", "4"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    sim = np.array([[float(v) for v in ln.split()] for ln in r.stdout.strip().splitlines()])
    assert sim.shape == (len(lines), len(lines)) and np.allclose(np.diag(sim), 1.0, atol=2e-6) and np.array_equal(sim, sim.T) and (np.abs(sim) <= 1.000002).all()
