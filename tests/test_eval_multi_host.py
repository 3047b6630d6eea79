"""CPU: the host half of llamahip_eval_multi -- the row table (llamahip_eval_multi_rows) against a restatement of its rule, every refusal of
the entry point and of llamahip_op_attention_rows' table check before any device is touched, the new symbols, and the host code under
ASan + UBSan in the stand-alone program `make asan` builds."""
import os
import subprocess

import numpy as np
import pytest

import synth

HOST_ONLY = 4
HP = synth.HParams(n_vocab=96, n_embd=128, n_mult=64, n_head=2, n_layer=2)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")


def rows_ref(n_ctx, n_past, n_tokens, chunk):
    """the rule, restated: row j of segment i sits at n_past[i] + j and splits the keys of the eval it belongs to"""
    if chunk < 0 or not len(n_past) or any(n < 1 or p < 0 or p + n > n_ctx for p, n in zip(n_past, n_tokens)) or sum(n_tokens) > 2048:
        return None
    seg, pos, keys = [], [], []
    for i, (p, n) in enumerate(zip(n_past, n_tokens)):
        for j in range(n):
            seg.append(i)
            pos.append(p + j)
            keys.append(p + (min(n, (j // chunk + 1) * chunk) if chunk > 0 else n))
    return seg, pos, keys


def test_row_table_is_its_rule(L):
    pasts, lens = (0, 3, 37), (1, 2, 9, 10, 18, 61)
    rng = np.random.default_rng(11)
    n_cases = n_refused = 0
    for n_ctx in (64, 128):
        for n_seqs in range(1, 6):
            for chunk in (0, 1, 9):
                # every (n_past, n_tokens) pair in the first segment, random draws from the grid in the others
                for p0 in pasts:
                    for n0 in lens:
                        n_past = [p0] + [int(rng.choice(pasts)) for _ in range(n_seqs - 1)]
                        n_tok = [n0] + [int(rng.choice(lens)) for _ in range(n_seqs - 1)]
                        want = rows_ref(n_ctx, n_past, n_tok, chunk)
                        got = L.eval_multi_rows(n_ctx, n_past, n_tok, chunk)
                        n_cases += 1
                        if want is None:
                            n_refused += 1
                            assert got is None, (n_ctx, n_past, n_tok, chunk)
                            continue
                        assert got is not None and [a.tolist() for a in got] == [list(w) for w in want], (n_ctx, n_past, n_tok, chunk)
    assert n_cases == 2 * 5 * 3 * 18 and 0 < n_refused < n_cases          # (37 + 61 > 64: the grid holds segments that do not fit)
    assert L.eval_multi_rows(4096, [0], [2049]) is None and L.eval_multi_rows(4096, [0, 0], [1024, 1024])[0].size == 2048
    assert L.eval_multi_rows(64, [0], [4], -1) is None and L.eval_multi_rows(0, [0], [1]) is None


@pytest.fixture(scope="module")
def host_model(L, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("evm") / "m.bin")
    synth.write_model(path, HP, synth.random_tensors(HP, seed=3))
    with L.Model(path, n_ctx=48, flags=HOST_ONLY, n_seq=3) as m:
        yield m


def test_eval_multi_refusals_touch_no_device(L, host_model):
    t = lambda n: np.arange(1, n + 1, dtype=np.int32)
    ok = dict(slots=[2, 0], n_past=[0, 5], token_lists=[t(4), t(9)], chunk_tokens=9)
    bad = [(dict(slots=[], n_past=[], token_lists=[]), "n_seqs"),
           (dict(slots=[0, 1, 2, 0], n_past=[0] * 4, token_lists=[t(1)] * 4), "n_seqs"),
           (dict(slots=[3, 0]), "out of range"), (dict(slots=[-1, 0]), "out of range"), (dict(slots=[1, 1]), "named twice"),
           (dict(token_lists=[t(4), t(0)]), "n_tokens"), (dict(n_past=[-1, 5]), "context overflow"), (dict(n_past=[0, 40]), "context overflow"),
           (dict(token_lists=[t(4), np.array([1, 96], np.int32)]), "token id"), (dict(token_lists=[np.array([-1], np.int32), t(2)]), "token id"),
           (dict(chunk_tokens=-1), "chunk_tokens")]
    for change, word in bad:
        with pytest.raises(L.LlamaHipError) as e:
            host_model.eval_multi(**dict(ok, **change))
        assert e.value.code == L.binding.ERR_PREDICT and "llamahip_eval_multi" in e.value.message and word in e.value.message, (change, e.value.message)
        assert "HOST_ONLY" not in e.value.message
    # the arguments are fine: the handle is refused, last
    with pytest.raises(L.LlamaHipError) as e:
        host_model.eval_multi(**ok)
    assert e.value.code == L.binding.ERR_PREDICT and "HOST_ONLY" in e.value.message and "llamahip_eval_multi" in e.value.message


def test_eval_multi_row_cap_and_null_handle(L, tmp_path):
    """R > LLAMAHIP_EVAL_MULTI_MAX_ROWS needs a context that holds it; a null handle is refused before anything is read"""
    path = str(tmp_path / "m.bin")
    synth.write_model(path, HP, synth.random_tensors(HP, seed=3))
    with L.Model(path, n_ctx=1100, flags=HOST_ONLY, n_seq=2) as m:
        with pytest.raises(L.LlamaHipError) as e:
            m.eval_multi([0, 1], [0, 0], [np.ones(1024, np.int32), np.ones(1025, np.int32)])
        assert "LLAMAHIP_EVAL_MULTI_MAX_ROWS" in e.value.message and "2049" in e.value.message
        with pytest.raises(L.LlamaHipError) as e:
            m.eval_multi([0, 1], [0, 0], [np.ones(1024, np.int32), np.ones(1024, np.int32)])
        assert "HOST_ONLY" in e.value.message
    import ctypes as C
    err = C.create_string_buffer(256)
    one = np.ones(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.lib().llamahip_eval_multi(None, 8, 1, p(one * 0), p(one * 0), p(one), p(one), 0, None, None, err, len(err))
    assert rc == L.binding.ERR_PREDICT and b"null model" in err.value


def test_op_attention_rows_table_refusals(L):
    d, H, C, S = 64, 2, 16, 3
    Kc, Vc = np.zeros((S, C, d), np.float32), np.zeros((S, C, d), np.float32)
    q = lambda R: np.zeros((R, 3 * d), np.float32)
    ok = dict(row_slot=[2, 2, 0], row_pos=[3, 4, 0], row_keys=[5, 5, 1])
    bad = [(dict(row_slot=[3, 3, 0]), "row_slot"), (dict(row_slot=[-1, 2, 0]), "row_slot"), (dict(row_slot=[2, 0, 2], row_pos=[3, 0, 4], row_keys=[4, 1, 5]), "not consecutive"),
           (dict(row_pos=[3, 5, 0]), "consecutive positions"), (dict(row_pos=[4, 3, 0]), "consecutive positions"), (dict(row_pos=[15, 16, 0]), "row_pos"),
           (dict(row_pos=[-1, 0, 0]), "row_pos"), (dict(row_keys=[3, 5, 1]), "row_keys"), (dict(row_keys=[5, 6, 1]), "row_keys"), (dict(row_keys=[5, 5, 0]), "row_keys")]
    for change, word in bad:
        with pytest.raises(L.LlamaHipError) as e:
            L.op_attention_rows(q(3), H, Kc, Vc, **dict(ok, **change))
        assert "llamahip_op_attention_rows" in e.value.message and word in e.value.message, (change, e.value.message)
    for kw, word in ((dict(n_threads=0), "n_threads"), (dict(n_threads=65), "n_threads"), (dict(merged_stride=d - 1), "merged_stride")):
        with pytest.raises(L.LlamaHipError) as e:
            L.op_attention_rows(q(3), H, Kc, Vc, **ok, **kw)
        assert word in e.value.message
    with pytest.raises(L.LlamaHipError) as e:          # head size 16
        L.op_attention_rows(q(3), 4, Kc, Vc, **ok)
    assert "head size" in e.value.message
    # a run that ends exactly at n_ctx is inside the cache: accepted by the table check (the next refusal, if any, is the missing device's)
    try:
        L.op_attention_rows(q(2), H, Kc, Vc, [1, 1], [14, 15], [16, 16])
    except L.LlamaHipError as e:
        assert "llamahip_op_attention_rows: row" not in e.message and "device" in e.message.lower(), e.message


def test_new_symbols_are_declared_and_exported(L):
    names = L.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for fn in ("llamahip_eval_multi", "llamahip_eval_multi_rows", "llamahip_op_attention_rows"):
        assert fn in names and hasattr(L.lib(), fn) and fn in exported, fn
    assert not [s for s in exported if "rows_table_check" in s or "eval_multi_check" in s]          # (lh:: internals stay local)
    assert hasattr(L.Model, "eval_multi") and callable(L.eval_multi_rows) and callable(L.op_attention_rows)


def test_eval_multi_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: eval_multi.cpp (the table over the grid on exactly sized arrays, the argument and table checks, accepted and refused) compiled
    with -fsanitize=address,undefined into the stand-alone tools/host_sanitize and run there -- never loaded into python"""
    subprocess.run(["make", "-s", "-C", CSRC, "asan"], check=True)
    src = open(os.path.join(CSRC, "tools", "host_sanitize.cpp")).read()
    assert "llamahip_eval_multi_rows(" in src and "lh::eval_multi_check(" in src and "lh::rows_table_check(" in src
    assert "eval_multi.cpp" in open(os.path.join(CSRC, "Makefile")).read().split("asan:")[1].split("tools:")[0]
    path = str(tmp_path / "m.bin")
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(CSRC, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout and "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
