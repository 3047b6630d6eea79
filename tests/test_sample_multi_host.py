"""CPU: the batched sampling entry points (llamahip_decode_sample_multi, llamahip_op_topk_rows) are exported and declared, a HOST_ONLY handle
refuses decode_sample_multi with a message, and bad arguments -- null samplers, n_steps < 1, more sequences than KV slots -- are rejected with a
message naming the argument before any device work (a HOST_ONLY handle knows n_seq, n_vocab and n_ctx, so the checks run here without a GPU)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import synth

HOST_ONLY = 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("llamahip_decode_sample_multi", "llamahip_op_topk_rows")


def test_sample_multi_symbols_are_declared_and_exported(L):
    assert all(s in L.declared_symbols() for s in NEW)
    so = os.path.join(ROOT, "llama.swift_amd", "csrc", "libllamahip.so")
    if not (shutil.which("nm") and os.path.exists(so)):
        pytest.skip("needs binutils' nm and the built libllamahip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert all(s in exported for s in NEW)


@pytest.fixture
def host_model(L, tmp_path):
    hp = synth.HParams(n_vocab=96, n_embd=64, n_mult=32, n_head=2, n_layer=1)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=5))
    with L.Model(path, n_ctx=32, flags=HOST_ONLY, n_seq=3) as m:
        yield m


def _err(L, fn, *a, **kw):
    with pytest.raises(L.LlamaHipError) as e:
        fn(*a, **kw)
    assert e.value.code == -1001 and e.value.message
    return e.value.message


def _samplers(L, n):
    return [L.Sampler(seed=i, repeat_last_n=64) for i in range(n)]


def test_host_only_handle_refuses_decode_sample_multi(L, host_model):
    msg = _err(L, host_model.decode_sample_multi, [1, 2], [4, 5], 3, _samplers(L, 2))
    assert "HOST_ONLY" in msg


def test_bad_arguments_are_rejected_before_device_work(L, host_model):
    m = host_model
    msg = _err(L, m.decode_sample_multi, [1, 2], [4, 5], 3, [L.Sampler(seed=1), None])
    assert "samplers[1] is NULL" in msg, msg
    s = L.Sampler(seed=1)
    assert "same sampler" in _err(L, m.decode_sample_multi, [1, 2], [4, 5], 3, [s, s])
    msg = _err(L, m.decode_sample_multi, [1, 2], [4, 5], 0, _samplers(L, 2))
    assert "n_steps must be >= 1 (got 0)" in msg, msg
    msg = _err(L, m.decode_sample_multi, [1, 2, 3, 4], [4, 5, 6, 7], 2, _samplers(L, 4))
    assert "4 sequences" in msg and "3 KV slots" in msg, msg
    with pytest.raises(ValueError):
        m.decode_sample_multi([1, 2], [4], 2, _samplers(L, 2))


def test_null_arrays_are_rejected_through_the_c_abi(L, host_model):
    import ctypes as C
    err = C.create_string_buffer(512)
    ft, npast, out = np.array([1], np.int32), np.array([2], np.int32), np.zeros(4, np.int32)
    sp = (C.c_void_p * 1)(L.Sampler(seed=3)._s.value)
    f = L.lib().llamahip_decode_sample_multi
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert f(host_model._h, 8, 1, p(npast), p(ft), 4, None, 1.3, 40, 0.95, 0.8, p(out), None, err, len(err)) == -1001
    assert b"samplers is NULL" in err.value
    assert f(host_model._h, 8, 1, None, p(ft), 4, sp, 1.3, 40, 0.95, 0.8, p(out), None, err, len(err)) == -1001
    assert b"n_past is NULL" in err.value
    assert f(host_model._h, 8, 1, p(npast), p(ft), 4, sp, 1.3, 40, 0.95, 0.8, None, None, err, len(err)) == -1001
    assert b"out_tokens is NULL" in err.value


def test_op_topk_rows_rejects_bad_arguments_before_device_work(L):
    lg = np.zeros((2, 100), np.float32)
    for kw in (dict(top_k=0), dict(top_k=65), dict(top_k=101)):
        with pytest.raises(L.LlamaHipError, match="bad arguments"):
            L.op_topk_rows(np.zeros((2, 100), np.float32) if kw["top_k"] != 101 else lg, [[], []], **kw)
    with pytest.raises(L.LlamaHipError, match="bad arguments"):
        L.op_topk_rows(np.zeros((1, 32769), np.float32), [[]])
    with pytest.raises(ValueError):
        L.op_topk_rows(lg, [[]])
