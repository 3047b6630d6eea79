"""CPU (-m "not gpu"): the host half of drafted sampled decoding -- every refusal of llamahip_verify_sample, llamahip_decode_sample_lookup and
llamahip_op_topk_slide names its limit and comes before any device work (a HOST_ONLY handle knows n_vocab and n_ctx), the runner's lookup
setter and stats getter work on a bridge that never ran, the symbols are declared and exported."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import synth

HOST_ONLY = 4
NEW = {"llamahip_verify_sample", "llamahip_decode_sample_lookup", "llamahip_op_topk_slide", "llama_runner_bridge_set_lookup",
       "llama_runner_bridge_lookup_stats"}


@pytest.fixture()
def host_model(L, tmp_path):
    hp = synth.HParams(n_vocab=64, n_embd=64, n_mult=32, n_head=2, n_layer=1)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    with L.Model(path, n_ctx=32, flags=HOST_ONLY) as m:
        yield m


def _refused(L, cases):
    for call, what in cases:
        with pytest.raises(L.LlamaHipError, match=what) as e:
            call()
        assert e.value.code == -1001


def test_verify_sample_refusals_name_their_limit(L, host_model):
    m, s = host_model, L.Sampler(seed=1)
    _refused(L, ((lambda: m.verify_sample(5, np.arange(16), 0, s), r"n_draft must be 0 \.\. 15 \(got 16\)"),
                 (lambda: m.verify_sample(5, [1, 2, 3], 29, s), r"n_past \(29\) \+ n_draft \(3\) \+ 1 > n_ctx \(32\)"),
                 (lambda: m.verify_sample(5, [1, 2, 3], -1, s), r"context overflow"),
                 (lambda: m.verify_sample(64, [1], 0, s), r"token id 64 out of range \[0, 64\)"),
                 (lambda: m.verify_sample(5, [1, -2], 0, s), r"draft token id -2 at 1 out of range \[0, 64\)"),
                 (lambda: m.verify_sample(5, [1, 2], 3, None), r"llamahip_verify_sample: null sampler"),
                 (lambda: m.verify_sample(5, [1, 2], 3, s, top_k=0), r"top_k must be >= 1 \(got 0\)"),
                 (lambda: m.verify_sample(5, [1, 2], 3, s, temp=0.0), r"temp must be > 0"),
                 (lambda: m.verify_sample(5, [1, 2], 3, s, repeat_penalty=-1.0), r"repeat_penalty must be > 0"),
                 (lambda: m.verify_sample(5, [1, 2], 3, s), r"HOST_ONLY")))
    assert s.window().tolist() == [0] * 64          # nothing was drawn or accepted


def test_decode_sample_lookup_refusals_name_their_limit(L, host_model):
    m, s = host_model, L.Sampler(seed=1)
    ctx = np.arange(8, dtype=np.int32)
    _refused(L, ((lambda: m.decode_sample_lookup(5, 30, 8, ctx, s), r"n_past \(8\) \+ n_steps \(30\) > n_ctx \(32\)"),
                 (lambda: m.decode_sample_lookup(5, 0, 8, ctx, s), r"context overflow"),
                 (lambda: m.decode_sample_lookup(5, 2**31 - 1, 8, ctx, s), r"context overflow"),
                 (lambda: m.decode_sample_lookup(99, 4, 8, ctx, s), r"token id 99 out of range \[0, 64\)"),
                 (lambda: m.decode_sample_lookup(5, 4, 9, ctx, s), r"n_context \(8\) must equal n_past \(9\)"),
                 (lambda: m.decode_sample_lookup(5, 4, 8, ctx + 60, s), r"context token id 64 at 4 out of range"),
                 (lambda: m.decode_sample_lookup(5, 4, 8, ctx, s, corpus=[1, 2, 64]), r"corpus token id 64 at 2 out of range"),
                 (lambda: m.decode_sample_lookup(5, 4, 8, ctx, s, draft_len=16), r"draft_len must be 1 \.\. 15"),
                 (lambda: m.decode_sample_lookup(5, 4, 8, ctx, s, draft_len=-1), r"draft_len must be 1 \.\. 15"),
                 (lambda: m.decode_sample_lookup(5, 4, 8, ctx, s, ngram_min=4), r"ngram_min \(4\) / ngram_max \(0\)"),
                 (lambda: m.decode_sample_lookup(5, 4, 8, ctx, s, stats_size=8), r"stats->struct_size \(8\) is not sizeof\(llamahip_lookup_stats\) \(32\)"),
                 (lambda: m.decode_sample_lookup(5, 4, 8, ctx, None), r"llamahip_decode_sample_lookup: null sampler"),
                 (lambda: m.decode_sample_lookup(5, 4, 8, ctx, s, top_k=0), r"top_k must be >= 1"),
                 (lambda: m.decode_sample_lookup(5, 4, 8, ctx, s), r"HOST_ONLY")))
    assert s.window().tolist() == [0] * 64


def test_op_topk_slide_refusals_name_their_limit(L):
    lg = np.zeros((2, 100), np.float32)
    _refused(L, ((lambda: L.op_topk_slide(lg, np.zeros(1026, np.int32), 1025), r"n_last must be 0 \.\. 1024 \(got 1025\)"),
                 (lambda: L.op_topk_slide(np.zeros((0, 100), np.float32), np.zeros(3, np.int32), 4), r"n_rows must be 1 \.\. 16 \(got 0\)"),
                 (lambda: L.op_topk_slide(np.zeros((17, 100), np.float32), np.zeros(16, np.int32), 0), r"n_rows must be 1 \.\. 16 \(got 17\)"),
                 (lambda: L.op_topk_slide(lg, np.zeros(5, np.int32), 4, top_k=65), r"top_k must be 1 \.\. min\(64, n_vocab\) \(got 65"),
                 (lambda: L.op_topk_slide(lg, np.zeros(5, np.int32), 4, top_k=0), r"top_k must be 1 \.\. min\(64, n_vocab\) \(got 0"),
                 (lambda: L.op_topk_slide(np.zeros((1, 32769), np.float32), np.zeros(4, np.int32), 4), r"n_vocab must be 1 \.\. 32768 \(got 32769\)"),
                 (lambda: L.op_topk_slide(lg, np.zeros(5, np.int32), 4, temp=0.0), r"temp \(0\) and repeat_penalty")))
    with pytest.raises(ValueError):
        L.op_topk_slide(lg, np.zeros(4, np.int32), 4)          # 2 rows with windows of 4 ids: a stream of 5


def test_runner_lookup_setter_and_stats_on_a_bridge_that_never_ran(L, tmp_path):
    zero = dict(n_verify_steps=0, n_single_steps=0, n_drafted=0, n_accepted=0)
    r = L.LlamaRunner(str(tmp_path / "missing.bin"))
    assert r.lookup_stats() == zero
    for k in (15, 0, 7, 99, -3):
        r.set_lookup(k)
        assert r.lookup_stats() == zero
    # a load failure with lookup on is still the bridge's load failure, and the counts stay zero
    r.set_lookup(15)
    with pytest.raises(L.LlamaHipError) as e:
        r.run("hello", L.Config(numTokens=4))
    assert e.value.code == -1000 and r.lookup_stats() == zero
    # the C getter refuses a null argument and a struct of another size
    lib = L.lib()
    lib.llama_runner_bridge_lookup_stats.restype = C.c_int32
    lib.llama_runner_bridge_lookup_stats.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.llama_runner_bridge_lookup_stats(r._bridge, None) == -1
    buf = (C.c_int32 * 8)(8)
    assert lib.llama_runner_bridge_lookup_stats(r._bridge, buf) == -1
    lib.llama_runner_bridge_set_lookup.argtypes = [C.c_void_p, C.c_int32]
    lib.llama_runner_bridge_set_lookup.restype = None
    lib.llama_runner_bridge_set_lookup(None, 3)          # a null bridge is ignored
    r.close()


def test_the_sampled_lookup_entry_points_are_declared_and_exported(L):
    so = L.LIB_PATH
    if not (shutil.which("nm") and os.path.exists(so)):
        pytest.fail("needs binutils' nm and the built libllamahip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NEW <= exported and NEW <= set(L.declared_symbols())
