"""CPU: the host half of sampled decode with drafted tokens for several sequences at once -- every refusal of llamahip_verify_sample_multi /
llamahip_decode_sample_lookup_multi on a HOST_ONLY handle and of llamahip_op_topk_slide_set without a device (the arguments are checked
before any device work), and the new symbols in the header and the library's dynamic table."""
import ctypes as C
import fnmatch
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import synth

HOST_ONLY = 4


@pytest.fixture()
def host_model(L, tmp_path):
    hp = synth.HParams(n_vocab=64, n_embd=64, n_mult=32, n_head=2, n_layer=1)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    with L.Model(path, n_ctx=32, n_seq=20, flags=HOST_ONLY) as m:
        yield m


def _smp(L, n, rln=64):
    return [L.Sampler(seed=100 + i, repeat_last_n=rln) for i in range(n)]


def test_verify_sample_multi_refusals_name_their_limit(L, host_model):
    m = host_model
    v = m.verify_sample_multi
    s = _smp(L, 17)
    for call, what in ((lambda: v(range(17), [5] * 17, [[]] * 17, [0] * 17, s), r"n_seqs must be 1 \.\. 16 \(got 17\)"),
                       (lambda: v([], [], [], [], []), r"n_seqs must be 1 \.\. 16 \(got 0\)"),
                       (lambda: v([0, 20], [5, 5], [[], []], [0, 0], s[:2]), r"sequence slot 20 out of range \[0, 20\)"),
                       (lambda: v([0, 3, 0], [5, 5, 5], [[], [], []], [0, 0, 0], s[:3]), r"sequence slot 0 appears twice"),
                       (lambda: v([0, 1, 2], [5, 5, 5], [[], [], []], [0, 0, 0], [s[0], s[1], s[0]]), r"samplers\[0\] and samplers\[2\] are the same sampler"),
                       (lambda: v([0, 1], [5, 5], [[], []], [0, 0], [s[0], None]), r"null sampler \(samplers\[1\]\)"),
                       (lambda: v([0, 1], [5, 5], [[1], []], [0, 0], s[:2], top_k=0), r"top_k must be >= 1 \(got 0\)"),
                       (lambda: v([0, 1], [5, 5], [[1], []], [0, 0], s[:2], temp=0.0), r"temp must be > 0 \(got 0\)"),
                       (lambda: v([0, 1], [5, 5], [[1], []], [0, 0], s[:2], repeat_penalty=-1.0), r"repeat_penalty must be > 0 \(got -1\)"),
                       (lambda: v([0, 1], [5, 5], [[1], []], [0, 0], s[:2], top_p=float("nan")), r"top_p is NaN"),
                       (lambda: v([0], [5], [np.arange(16)], [0], s[:1]), r"n_draft must be 0 \.\. 15 \(got 16 for slot 0\)"),
                       (lambda: v([0, 1, 2], [5, 5, 5], [[1] * 7, [1] * 6, [1]], [0, 0, 0], s[:3]), r"at most 16 rows \(3 sequences"),
                       (lambda: v([0, 1], [5, 5], [[1], [1, 2, 3]], [0, 29], s[:2]), r"n_past \(29\) \+ n_draft \(3\) \+ 1 > n_ctx \(32\)"),
                       (lambda: v([0, 1], [5, 5], [[1], [1]], [0, -1], s[:2]), r"context overflow"),
                       (lambda: v([0, 1], [5, 64], [[1], [1]], [0, 0], s[:2]), r"token id 64 out of range \[0, 64\)"),
                       (lambda: v([0, 1], [5, 5], [[1], [1, -2]], [0, 0], s[:2]), r"draft token id -2 at 2 out of range \[0, 64\)"),
                       (lambda: v([0, 1], [5, 5], [[1, 2], []], [3, 4], s[:2]), r"HOST_ONLY")):
        with pytest.raises(L.LlamaHipError, match=what) as e:
            call()
        assert e.value.code == -1001
    # null pointers
    f, err = L.lib().llamahip_verify_sample_multi, C.create_string_buffer(512)
    a = np.zeros(4, np.int32)
    p = a.ctypes.data
    sp = (C.c_void_p * 1)(s[0]._s.value)
    tail = (1.3, 40, 0.95, 0.8)
    for args, out, what in (((None, p, p, p, p), (p, p, p), "null slots"), ((p, None, p, p, p), (p, p, p), "null slots"), ((p, p, p, p, None), (p, p, p), "null slots"),
                            ((p, p, p, p, p), (None, p, p), "null output"), ((p, p, p, p, p), (p, None, p), "null output")):
        assert f(m._h, 8, 1, *args, sp, *tail, *out, err, len(err)) == -1001 and what in err.value.decode()
    assert f(m._h, 8, 1, p, p, p, p, p, None, *tail, p, p, p, err, len(err)) == -1001 and "null samplers" in err.value.decode()
    assert f(None, 8, 1, p, p, p, p, p, sp, *tail, p, p, p, err, len(err)) == -1001 and "null model" in err.value.decode()


def test_decode_sample_lookup_multi_refusals_name_their_limit(L, host_model):
    m = host_model
    g = m.decode_sample_lookup_multi
    s = _smp(L, 17)
    ctx = [np.arange(8, dtype=np.int32), np.arange(3, dtype=np.int32)]
    for call, what in ((lambda: g([5] * 17, [0] * 17, 4, [[]] * 17, s), r"n_seqs must be 1 \.\. 16 \(got 17\).*llamahip_decode_sample_multi"),
                       (lambda: g([], [], 4, [], []), r"n_seqs must be 1 \.\. 16 \(got 0\)"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, [s[0], s[0]]), r"samplers\[0\] and samplers\[1\] are the same sampler"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, [None, s[0]]), r"null sampler \(samplers\[0\]\)"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, s[:2], top_k=0), r"top_k must be >= 1 \(got 0\)"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, s[:2], temp=-0.5), r"temp must be > 0 \(got -0.5\)"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, s[:2], repeat_penalty=0.0), r"repeat_penalty must be > 0 \(got 0\)"),
                       (lambda: g([5, 5], [8, 3], 30, ctx, s[:2]), r"n_past \(8\) \+ n_steps \(30\) > n_ctx \(32\)"),
                       (lambda: g([5, 5], [8, 3], 0, ctx, s[:2]), r"context overflow"),
                       (lambda: g([5, 5], [8, -3], 4, ctx, s[:2]), r"context overflow"),
                       (lambda: g([5, 99], [8, 3], 4, ctx, s[:2]), r"token id 99 out of range \[0, 64\)"),
                       (lambda: g([5, 5], [8, 3], 4, [ctx[0], ctx[1] + 62], s[:2]), r"context token id 64 at 2 out of range"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, s[:2], corpus=[1, 2, 64]), r"corpus token id 64 at 2 out of range"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, s[:2], draft_len=16), r"draft_len must be 1 \.\. 15"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, s[:2], ngram_min=4), r"ngram_min \(4\) / ngram_max \(0\)"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, s[:2], stats_size=8), r"stats->struct_size \(8\)"),
                       (lambda: g([5, 5], [8, 3], 4, ctx, s[:2]), r"HOST_ONLY")):
        with pytest.raises(L.LlamaHipError, match=what) as e:
            call()
        assert e.value.code == -1001
    f, err = L.lib().llamahip_decode_sample_lookup_multi, C.create_string_buffer(512)
    a = np.zeros(4, np.int32)
    p = a.ctypes.data
    sp = (C.c_void_p * 1)(s[0]._s.value)
    tail = (1.3, 40, 0.95, 0.8)
    assert f(m._h, 8, 1, None, p, 4, None, None, 0, 0, 0, 0, sp, *tail, p, None, None, err, len(err)) == -1001 and "null n_past" in err.value.decode()
    assert f(m._h, 8, 1, p, p, 4, None, None, 0, 0, 0, 0, sp, *tail, None, None, None, err, len(err)) == -1001 and "null out_tokens" in err.value.decode()
    assert f(m._h, 8, 1, p, p, 4, None, None, 0, 0, 0, 0, None, *tail, p, None, None, err, len(err)) == -1001 and "null samplers" in err.value.decode()
    assert f(None, 8, 1, p, p, 4, None, None, 0, 0, 0, 0, sp, *tail, p, None, None, err, len(err)) == -1001 and "null model" in err.value.decode()


def test_more_sequences_than_kv_slots_are_refused(L, tmp_path):
    hp = synth.HParams(n_vocab=64, n_embd=64, n_mult=32, n_head=2, n_layer=1)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    s = _smp(L, 3)
    with L.Model(path, n_ctx=32, n_seq=2, flags=HOST_ONLY) as m:
        with pytest.raises(L.LlamaHipError, match=r"llamahip_decode_sample_lookup_multi: 3 sequences on a handle with 2 KV slots"):
            m.decode_sample_lookup_multi([5, 5, 5], [0, 0, 0], 4, [[], [], []], s)
        with pytest.raises(L.LlamaHipError, match=r"llamahip_verify_sample_multi: 3 sequences on a handle with 2 KV slots"):
            m.verify_sample_multi([0, 1, 0], [5, 5, 5], [[], [], []], [0, 0, 0], s)


def test_op_topk_slide_set_refusals_name_their_limit(L):
    """every refusal comes before the device is asked for: each message is the argument's, not "no HIP device" """
    z = np.zeros((6, 8), np.float32)
    ids = np.zeros(40, np.int32)
    o = L.op_topk_slide_set
    for call, what in ((lambda: o(np.zeros((17, 8), np.float32), ids, [0, 17], [0], [4]), r"n_rows must be 1 \.\. 16 \(got 17\): a verify step has at most 16 rows"),
                       (lambda: o(np.zeros((2, 32769), np.float32), ids, [0, 2], [0], [4]), r"n_vocab must be 1 \.\. 32768 \(got 32769\)"),
                       (lambda: o(z, ids, [0, 6], [0], [4], top_k=65), r"top_k must be 1 \.\. min\(64, n_vocab\) \(got 65, n_vocab 8\)"),
                       (lambda: o(z, ids, [0, 6], [0], [4], top_k=9), r"top_k must be 1 \.\. min\(64, n_vocab\) \(got 9, n_vocab 8\)"),
                       (lambda: o(z, ids, [0, 6], [0], [4], top_k=0), r"top_k must be 1 \.\. min\(64, n_vocab\) \(got 0"),
                       (lambda: o(z, ids, [0, 6], [0], [4], top_k=4, temp=0.0), r"temp \(0\) and repeat_penalty \(1\.3\) must be positive"),
                       (lambda: o(z, ids, [0, 4, 2, 6], [0, 0, 0], [4, 4, 4], top_k=4), r"seg_begin must ascend strictly \(segment 1: 4 \.\. 2\)"),
                       (lambda: o(z, ids, [0, 3, 3, 6], [0, 0, 0], [4, 4, 4], top_k=4), r"ascend strictly"),
                       (lambda: o(z, ids, [1, 6], [0], [4], top_k=4), r"seg_begin must run from 0 to n_rows \(6; got 1 \.\. 6\)"),
                       (lambda: o(z, ids, [0, 5], [0], [4], top_k=4), r"must run from 0 to n_rows"),
                       (lambda: o(z, ids, list(range(8)), [0] * 7, [4] * 7, top_k=4), r"n_segs must be 1 \.\. n_rows \(6; got 7\)"),
                       (lambda: o(z, ids, [0, 2, 6], [0, -1], [4, 4], top_k=4), r"segment 1: seg_ids_off \(-1\) and seg_n_last \(4\) must be >= 0"),
                       (lambda: o(z, ids, [0, 2, 6], [0, 3], [4, -4], top_k=4), r"segment 1: seg_ids_off \(3\) and seg_n_last \(-4\) must be >= 0"),
                       (lambda: o(z, ids, [0, 2, 6], [0, 30], [4, 8], top_k=4), r"segment 1's id stream does not fit: seg_ids_off \(30\) \+ seg_n_last \(8\) \+ rows \(4\) - 1 > n_ids \(40\)"),
                       (lambda: o(z, ids, [0, 6], [0], [1025], top_k=4), r"segment 0's id stream does not fit: seg_ids_off \(0\) \+ seg_n_last \(1025\)"),
                       (lambda: o(z, ids, [0, 2, 6], [2**31 - 8, 0], [2**31 - 8, 4], top_k=4), r"segment 0's id stream does not fit")):
        with pytest.raises(L.LlamaHipError, match=what) as e:
            call()
        assert e.value.code == -1001 and "llamahip_op_topk_slide_set" in str(e.value)
    f, err = L.lib().llamahip_op_topk_slide_set, C.create_string_buffer(512)
    a, sc = np.zeros(64, np.int32), np.zeros(6 * 64, np.float64)
    p = a.ctypes.data
    ok = [z.ctypes.data, 6, 8, p, 40, p, 1, p, p, 1.3, 4, 0.8, sc.ctypes.data, p, p]
    for hole in (0, 3, 5, 7, 8, 12, 13, 14):
        args = list(ok)
        args[hole] = None
        assert f(*args, err, len(err)) == -1001 and "null argument" in err.value.decode(), hole


def test_the_new_entry_points_are_declared_and_exported(L):
    so = L.LIB_PATH
    if not (shutil.which("nm") and os.path.exists(so)):
        pytest.fail("needs binutils' nm and the built libllamahip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    want = {"llamahip_verify_sample_multi", "llamahip_decode_sample_lookup_multi", "llamahip_op_topk_slide_set"}
    assert want <= exported and want <= set(L.declared_symbols())
    # the version script exports by prefix: every new name falls under one of its global patterns
    text = open(os.path.join(os.path.dirname(so), "exports.map")).read()
    pats = re.search(r"global:(.*?)local:", text, re.S).group(1).replace(";", " ").split()
    assert all(any(fnmatch.fnmatchcase(s, p) for p in pats) for s in want)
