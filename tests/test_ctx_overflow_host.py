"""CPU: generating past the context window -- the plan (llamahip_ctx_overflow_plan) against its formula, the refusals of
llamahip_decode_greedy_window that happen before any device is touched, and the new host code (the plan, the
greedy loop in legs, the driver's overflow mode) under ASan + UBSan in the stand-alone program `make asan` builds."""
import os
import subprocess

import numpy as np
import pytest

import synth

HOST_ONLY = 4
HP = synth.HParams(n_vocab=96, n_embd=128, n_mult=64, n_head=2, n_layer=2)


@pytest.fixture(scope="module")
def host_model(L, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ctx") / "m.bin")
    synth.write_model(path, HP, synth.random_tensors(HP, seed=3))
    with L.Model(path, n_ctx=48, flags=HOST_ONLY) as m:
        yield m


def test_plan_is_its_formula(L):
    """n_discard = (n_past - n_keep) // 2, new context n_past - n_discard; -1 where that discards nothing or the arguments are out of range"""
    for n_ctx in (1, 2, 3, 4, 7, 48, 512, 2048):
        for n_past in sorted({-1, 0, 1, 2, 3, n_ctx // 2, n_ctx - 1, n_ctx, n_ctx + 1}):
            for n_keep in sorted({-1, 0, 1, 2, n_past - 3, n_past - 2, n_past - 1, n_past, n_past + 1, n_ctx // 2}):
                new, nd = L.ctx_overflow_plan(n_ctx, n_past, n_keep)
                ok = 0 <= n_keep <= n_past <= n_ctx and (n_past - n_keep) // 2 >= 1
                want = (n_past - (n_past - n_keep) // 2, (n_past - n_keep) // 2) if ok else (-1, 0)
                assert (new, nd) == want, (n_ctx, n_past, n_keep)
    # spans of 1, 2 and 3 tokens behind n_keep: nothing to drop, one of two, one of three
    assert L.ctx_overflow_plan(48, 48, 47) == (-1, 0)
    assert L.ctx_overflow_plan(48, 48, 46) == (47, 1)
    assert L.ctx_overflow_plan(48, 48, 45) == (47, 1)
    assert L.ctx_overflow_plan(48, 48, 0) == (24, 24)
    assert L.ctx_overflow_plan(48, 47, 0) == (24, 23)          # odd span: M = n_discard + 1 rows survive


def test_decode_greedy_window_refusals_touch_no_device(L, host_model):
    ctx = np.arange(3, 13, dtype=np.int32)
    ok = dict(first_token=5, n_steps=100, n_past=10, context=ctx, n_keep=4, mode=L.CTX_REEVAL, chunk_tokens=9)
    bad = [(dict(mode=0), "mode"), (dict(mode=2), "mode"), (dict(mode=3), "mode"), (dict(n_steps=0), "n_steps"), (dict(n_past=-1, context=ctx[:0]), "n_past"),
           (dict(n_past=49, context=np.zeros(49, np.int32)), "n_past"), (dict(context=ctx[:9]), "n_context"), (dict(first_token=96), "token id"),
           (dict(first_token=-1), "token id"), (dict(context=np.full(10, 96, np.int32)), "context token id"), (dict(chunk_tokens=-1), "chunk_tokens"),
           (dict(n_keep=-1), "n_keep"), (dict(n_keep=47), "n_keep"), (dict(n_keep=48), "n_keep")]
    for change, word in bad:
        with pytest.raises(L.LlamaHipError) as e:
            host_model.decode_greedy_window(**dict(ok, **change))
        assert e.value.code == L.binding.ERR_PREDICT and "llamahip_decode_greedy_window" in e.value.message and word in e.value.message, (change, e.value.message)
    for mode in (L.CTX_REEVAL,):
        for start in (dict(), dict(n_past=48, context=np.ones(48, np.int32))):          # ... a start at the wall included
            with pytest.raises(L.LlamaHipError) as e:
                host_model.decode_greedy_window(**dict(ok, mode=mode, **start))
            assert e.value.code == L.binding.ERR_PREDICT and "HOST_ONLY" in e.value.message, e.value.message


def test_new_symbols_are_declared_and_exported(L):
    names = L.declared_symbols()
    for fn in ("llamahip_ctx_overflow_plan", "llamahip_decode_greedy_window", "llama_runner_bridge_set_overflow"):
        assert fn in names and hasattr(L.lib(), fn), fn
    assert L.CTX_REEVAL == 1
    assert hasattr(L.LlamaRunner, "set_overflow")


def test_overflow_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: ctx_overflow.cpp (the plan over a grid, the greedy loop in legs on exactly sized arrays its refusals) and the
    driver's overflow modes in runner.cpp, compiled with -fsanitize=address,undefined into the stand-alone tools/host_sanitize (device entry
    points stubbed) and run there -- never loaded into python"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "asan"], check=True)
    src = open(os.path.join(csrc, "tools", "host_sanitize.cpp")).read()
    assert "llamahip_decode_greedy_window(" in src and "llama_runner_bridge_set_overflow(" in src and "llamahip_ctx_overflow_plan(" in src
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(csrc, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout and "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
