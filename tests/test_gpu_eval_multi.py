"""GPU (-m gpu): llamahip_eval_multi -- the prompts of several KV slots in one weight pass -- against the per-slot loop it stands for.

Yardstick: a second handle on the same file doing set_seq + eval / eval_chunks per slot (code this entry point does not touch), and for one case
per model the oracle making the same llama_eval calls per slot.  Logits rows and the KV rows of every layer and slot are compared bit for bit;
KV rows outside the appended ranges must keep the bits they had.  n_ctx 160, 5 KV slots, d 256 with head sizes 64 and 128."""
import os

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
N_CTX, N_SEQ = 160, 5
NO_GRAPH, UNFUSED, NO_PREFILL_COPY = 1, 2, 8
SHORT_MAX = 60          # ATTN_SHORT_MAX: longer segments take attention launches of their own
# name: (segment lengths, n_past, slots -- never ascending)
CASES = {
    "a_mixed_short": ([1, 2, 9, 17, 33], [0, 0, 12, 0, 40], [3, 0, 4, 1, 2]),          # R = 62
    "b_long": ([61, 70], [0, 20], [4, 1]),                                             # R = 131, one segment of 64 rows or more
    "c_60_and_61": ([60, 61], [5, 0], [2, 0]),                                          # the short path's limit beside a long segment
    "e_to_n_ctx": ([20, 9, 3], [140, 3, 157], [1, 4, 0]),                               # two segments end exactly at n_ctx
}
COMBOS = [(c, t) for c in (0, 1, 9) for t in (1, 3, 8)]


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def hparams(n_head, n_layer=2):
    return synth.HParams(n_vocab=1500, n_embd=256, n_mult=64, n_head=n_head, n_layer=n_layer)


@pytest.fixture(scope="module", params=[4, 2], ids=["head64", "head128"])
def pair(request, L, tmp_path_factory):
    """(hparams, path, the handle under test, the yardstick handle) -- one pair per head size for the whole module"""
    hp = hparams(request.param)
    path = str(tmp_path_factory.mktemp("evm") / f"m{request.param}.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=40 + request.param))
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hl:
        yield hp, path, hm, hl


def tokens_of(hp, lens, seed):
    return [synth.synth_prompt(n, hp.n_vocab, seed=seed + 7 * i)[:n] for i, n in enumerate(lens)]


def prefix_of(hp, slot, n):
    return synth.synth_prompt(max(n, 1), hp.n_vocab, seed=900 + slot)[:n]


def loop_eval(h, slot, toks, n_past, chunk, nth):
    h.set_seq(slot)
    return h.eval_chunks(toks, n_past, chunk, nth) if chunk > 0 else h.eval(toks, n_past, nth)


def kv_all(h, n_layer, slots=range(N_SEQ)):
    out = {}
    for s in slots:
        h.set_seq(s)
        out[s] = [h.kv(il, N_CTX) for il in range(n_layer)]
    return out


def check_call(hm, hl, hp, lens, n_past, slots, chunk, nth, seed, note, prefill=True, cur=None):
    """one eval_multi on hm against the per-slot loop on hl, both after the same per-slot prefixes; returns (logits, stats)"""
    toks = tokens_of(hp, lens, seed)
    if prefill:
        for h in (hm, hl):
            for s, p in zip(slots, n_past):
                if p > 0:
                    h.set_seq(s)
                    h.eval(prefix_of(hp, s, p), 0, nth)
    before = kv_all(hm, hp.n_layer)
    cur = slots[-1] if cur is None else cur
    hm.set_seq(cur)
    lg, st = hm.eval_multi(slots, n_past, toks, chunk_tokens=chunk, n_threads=nth, want_stats=True)
    k_cur, v_cur = hm.kv(0, N_CTX)          # (read through the handle's current slot, which the call must leave alone)
    assert lg.shape == (len(slots), hp.n_vocab)
    for i, s in enumerate(slots):
        want = loop_eval(hl, s, toks[i], n_past[i], chunk, nth)
        assert same(lg[i], want), (note, f"logits row {i} (slot {s}, {lens[i]} rows at {n_past[i]})")
    after, want_kv = kv_all(hm, hp.n_layer), kv_all(hl, hp.n_layer, slots)
    assert same(k_cur, after[cur][0][0]) and same(v_cur, after[cur][0][1]), (note, "the handle's current slot moved")
    for s in range(N_SEQ):
        for il in range(hp.n_layer):
            for w in (0, 1):
                got, was = after[s][il][w], before[s][il][w]
                if s not in slots:
                    assert same(got, was), (note, f"slot {s} layer {il}: a slot the call does not name")
                    continue
                i = slots.index(s)
                end = n_past[i] + lens[i]
                assert same(got[:end], want_kv[s][il][w][:end]), (note, f"slot {s} layer {il} {'KV'[w]} rows [0, {end})")
                assert same(got[:n_past[i]], was[:n_past[i]]) and same(got[end:], was[end:]), (note, f"slot {s} layer {il}: rows outside [{n_past[i]}, {end})")
    n_long = sum(n > SHORT_MAX for n in lens)
    assert st == dict(n_rows=sum(lens), n_passes=1, n_short_segs=len(lens) - n_long, n_long_segs=n_long, attn_groups=(1 if n_long < len(lens) else 0) + n_long), (note, st)
    return lg, st


@pytest.mark.parametrize("case", list(CASES))
def test_one_pass_is_the_per_slot_loop(L, pair, case):
    """cases (a) (b) (c) (e) at every chunk 0 / 1 / 9 x n_threads 1 / 3 / 8"""
    hp, _, hm, hl = pair
    lens, n_past, slots = CASES[case]
    for k, (chunk, nth) in enumerate(COMBOS):
        check_call(hm, hl, hp, lens, n_past, slots, chunk, nth, seed=100 + k, note=(case, chunk, nth), prefill=(k == 0))


def test_a_slot_continued_by_successive_calls(L, pair):
    """case (d): two slots continued twice, the later calls starting where the earlier ones ended (short, then short + long segments)"""
    hp, _, hm, hl = pair
    slots = [3, 1]
    for chunk, nth in ((9, 8), (0, 3)):
        check_call(hm, hl, hp, [9, 5], [0, 0], slots, chunk, nth, seed=300, note=("d1", chunk, nth), prefill=False)
        check_call(hm, hl, hp, [10, 61], [9, 5], slots, chunk, nth, seed=301, note=("d2", chunk, nth), prefill=False)
        check_call(hm, hl, hp, [1, 30], [19, 66], slots, chunk, nth, seed=302, note=("d3", chunk, nth), prefill=False)


def test_attn_groups_do_not_grow_with_the_number_of_short_segments(L, pair):
    hp, _, hm, hl = pair
    for n_seqs in (2, 5):
        _, st = check_call(hm, hl, hp, [9] * n_seqs, [0] * n_seqs, list(range(n_seqs))[::-1], 9, 8, seed=400, note=("groups", n_seqs), prefill=False)
        assert st["attn_groups"] == 1 and st["n_short_segs"] == n_seqs


def test_against_the_oracles_evals_per_slot(L, oracle, pair):
    """case (a), chunks of 9, 8 threads: the oracle makes the llama_eval calls of every slot in turn (it holds one conversation)"""
    hp, path, hm, _ = pair
    lens, n_past, slots = CASES["a_mixed_short"]
    toks = tokens_of(hp, lens, seed=500)
    for s, p in zip(slots, n_past):
        if p > 0:
            hm.set_seq(s)
            hm.eval(prefix_of(hp, s, p), 0, 8)
    lg = hm.eval_multi(slots, n_past, toks, chunk_tokens=9, n_threads=8)
    om = oracle.load(path, n_ctx=N_CTX)
    for i, s in enumerate(slots):
        if n_past[i] > 0:
            om.eval(prefix_of(hp, s, n_past[i]), 0, 8)
        for c0 in range(0, lens[i], 9):
            want = om.eval(toks[i][c0:c0 + 9], n_past[i] + c0, 8)["logits"]
        assert same(lg[i], want), ("oracle", i)
        hm.set_seq(s)
        for il in range(hp.n_layer):
            k, v = hm.kv(il, n_past[i] + lens[i])
            wk, wv = om.kv(il, n_past[i] + lens[i])
            assert same(k, wk) and same(v, wv), ("oracle", i, il)
    om.close()


@pytest.mark.parametrize("opts", [dict(devices=[0, 0]), dict(devices=[0, 0, 0]), dict(flags=NO_GRAPH), dict(flags=UNFUSED), dict(flags=NO_PREFILL_COPY)],
                         ids=["pipe2", "pipe3", "no_graph", "unfused", "no_prefill_copy"])
def test_pipeline_handles_and_flags_take_the_one_pass(L, tmp_path, opts):
    """a two- and a three-stage in-process pipeline on one GPU (three layers), and the flags that do not change a multi-row eval: short and
    mixed tables against a plain handle's per-slot loop"""
    hp = hparams(4, n_layer=3)
    path = str(tmp_path / "m3.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=61))
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, **opts) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hl:
        for case, chunk, nth in (("a_mixed_short", 9, 8), ("c_60_and_61", 0, 3), ("e_to_n_ctx", 1, 1)):
            lens, n_past, slots = CASES[case]
            check_call(hm, hl, hp, lens, n_past, slots, chunk, nth, seed=600, note=(str(opts), case))


@pytest.mark.parametrize("ftype", ["f16", "q41"])
def test_f16_and_q4_1_files_run_the_loop(L, tmp_path, ftype):
    """no one-pass eval on these files: the per-slot loop runs, the results are the loop's, n_passes is the number of evals it made"""
    hp = hparams(4)
    path = str(tmp_path / f"d_{ftype}.bin")
    src = path + ".f16" if ftype == "q41" else path
    synth.write_model_unquantized(src, hp, synth.random_tensors(hp, seed=1701), 1)
    if ftype == "q41":
        L.quantize_file(src, path, 3)
        os.remove(src)
    lens, n_past, slots = [1, 9, 20, 10], [0, 0, 4, 0], [3, 0, 2, 1]
    toks = tokens_of(hp, lens, seed=700)
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hm, L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as hl:
        for h in (hm, hl):
            h.set_seq(2)
            h.eval(prefix_of(hp, 2, 4), 0, 8)
        for chunk, n_evals in ((9, 1 + 1 + 3 + 2), (0, 4)):
            e0 = hm.stats()["n_evals"]
            lg, st = hm.eval_multi(slots, n_past, toks, chunk_tokens=chunk, n_threads=8, want_stats=True)
            assert st["n_passes"] == n_evals == hm.stats()["n_evals"] - e0 and st["n_rows"] == sum(lens), (ftype, chunk, st)
            for i, s in enumerate(slots):
                assert same(lg[i], loop_eval(hl, s, toks[i], n_past[i], chunk, 8)), (ftype, chunk, i)
                hm.set_seq(s)
                for il in range(hp.n_layer):
                    end = n_past[i] + lens[i]
                    assert all(same(a, b) for a, b in zip(hm.kv(il, end), hl.kv(il, end))), (ftype, chunk, i, il)


def test_one_segment_is_the_eval_itself(L, pair):
    """n_seqs == 1 runs llamahip_eval / llamahip_eval_chunks on that slot: one pass reported"""
    hp, _, hm, hl = pair
    toks = tokens_of(hp, [23], seed=800)
    lg, st = hm.eval_multi([2], [0], toks, chunk_tokens=9, n_threads=8, want_stats=True)
    assert st["n_passes"] == 1 and st["n_rows"] == 23 and same(lg[0], loop_eval(hl, 2, toks[0], 0, 9, 8))


def test_decode_greedy_multi_continues_from_the_slots(L, pair):
    """after eval_multi, the multi-sequence greedy loop gives the tokens it gives after per-slot prompts"""
    hp, _, hm, hl = pair
    lens, slots = [9, 17, 2], [2, 0, 1]
    toks = tokens_of(hp, lens, seed=850)
    lg = hm.eval_multi(slots, [0, 0, 0], toks, chunk_tokens=9, n_threads=8)
    want_lg = [loop_eval(hl, s, toks[i], 0, 9, 8) for i, s in enumerate(slots)]
    by_slot = sorted(range(3), key=lambda i: slots[i])
    first = [int(np.argmax(lg[i])) for i in by_slot]
    assert first == [int(np.argmax(want_lg[i])) for i in by_slot]
    n_past = [lens[i] for i in by_slot]
    got = hm.decode_greedy_multi(first, n_past, 6, n_threads=8)
    want = hl.decode_greedy_multi(first, n_past, 6, n_threads=8)
    assert got.tolist() == want.tolist()


@pytest.mark.parametrize("n_head", [4, 2], ids=["head64", "head128"])
def test_segments_of_512_rows_and_the_measured_loop_rule(L, tmp_path, n_head):
    """2 x 512 rows take the one pass (each segment the long eval's attention on its own rows, in batches of its workspace); more than 1024 rows in
    segments of 512 rows or more each take the per-slot loop (the measured rule) -- the bits are the loop's either way"""
    hp, C = hparams(n_head), 520
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=77))
    with L.Model(path, n_ctx=C, n_seq=2) as hm, L.Model(path, n_ctx=C, n_seq=2) as hl:
        for lens, n_passes in (([512, 512], 1), ([513, 512], 2), ([513, 511], 1)):
            toks = tokens_of(hp, lens, seed=950)
            lg, st = hm.eval_multi([1, 0], [0, 0], toks, chunk_tokens=9, n_threads=8, want_stats=True)
            assert st["n_passes"] == n_passes and st["n_rows"] == sum(lens), (lens, st)
            assert (st["n_long_segs"], st["attn_groups"]) == ((2, 2) if n_passes == 1 else (0, 0)), (lens, st)
            for i, s in enumerate([1, 0]):
                assert same(lg[i], loop_eval(hl, s, toks[i], 0, 9, 8)), (lens, i)
                hm.set_seq(s)
                for il in range(hp.n_layer):
                    end = lens[i]
                    assert all(same(a, b) for a, b in zip(hm.kv(il, end), hl.kv(il, end))), (lens, i, il)
