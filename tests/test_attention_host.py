"""CPU: the op-level attention entry point (llamahip_op_attention) is declared and exported, refuses bad arguments and shapes its path
cannot take with a message before any device work, and without a GPU fails loudly; the model's attention rule, queried host-only
(llamahip_debug_attn_path), picks what forward() launches."""
import os
import shutil
import subprocess

import numpy as np
import pytest

SYMS = ("llamahip_op_attention", "llamahip_debug_attn_path")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_attention_symbols_are_declared_and_exported(L):
    assert set(SYMS) <= set(L.declared_symbols())
    so = os.path.join(ROOT, "llama.swift_amd", "csrc", "libllamahip.so")
    if not (shutil.which("nm") and os.path.exists(so)):
        pytest.skip("needs binutils' nm and the built libllamahip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert set(SYMS) <= {line.split()[-1] for line in out.splitlines() if line.strip()}


def _args(N=9, H=2, dh=128, n_past=0, n_ctx=16):
    d = H * dh
    return np.ones((N, 3 * d), np.float32), H, n_past, np.zeros((n_ctx, d), np.float32), np.zeros((n_ctx, d), np.float32)


def _refused(L, *a, **kw):
    with pytest.raises(L.LlamaHipError) as e:
        L.op_attention(*a, **kw)
    assert e.value.code == -1001
    return e.value.message


def test_bad_arguments_are_refused_before_device_work(L):
    qkv, H, n_past, K, V = _args()
    assert "d 256 a multiple of H 3" in _refused(L, qkv, 3, n_past, K, V)
    assert "T = n_past + N = 17 > n_ctx 16" in _refused(L, qkv, H, 8, K, V)
    assert "merged_stride 255 < d 256" in _refused(L, qkv, H, n_past, K, V, merged_stride=255)
    for bad in (-64, 32, 100):
        assert f"ws_rows {bad} must be a positive multiple of 64" in _refused(L, qkv, H, n_past, K, V, ws_rows=bad)
    for bad in (0, 65):
        assert f"n_threads {bad} outside 1 .. 64" in _refused(L, qkv, H, n_past, K, V, n_threads=bad)
    for bad in (-1, 6, 99):
        assert f"unknown path {bad}" in _refused(L, qkv, H, n_past, K, V, path=bad)
    assert "N 0 >= 1" in _refused(L, np.ones((0, 768), np.float32), H, n_past, K, V)


def test_paths_refuse_shapes_they_cannot_take(L):
    assert "MFMA takes N >= 2, head size 128 and n_threads <= 8" in _refused(L, *_args(dh=64), path="mfma")
    assert "MFMA takes N >= 2, head size 128 and n_threads <= 8" in _refused(L, *_args(), path="mfma", n_threads=9)
    assert "MFMA takes" in _refused(L, *_args(N=1), path="mfma")
    assert "ROW takes head sizes that are multiples of 32 up to 256" in _refused(L, *_args(dh=512), path="row")
    assert "ROW takes" in _refused(L, *_args(H=4, dh=48, n_ctx=16), path="row")
    assert "SHORT takes 2 <= N <= 60" in _refused(L, *_args(N=61, n_ctx=64), path="short")
    assert "SHORT takes 2 <= N <= 60" in _refused(L, *_args(N=1), path="short")
    assert "DEC takes N = 1" in _refused(L, *_args(N=2), path="dec")
    assert "DEC_STREAM takes N = 1, head sizes that are multiples of 32 up to 256, n_threads <= 32 and n_ctx <= 4096" in \
        _refused(L, *_args(N=1), path="dec_stream", n_threads=33)
    assert "n_ctx <= 4096" in _refused(L, *_args(N=1, n_ctx=4097), path="dec_stream")
    assert "AUTO takes N >= 2" in _refused(L, *_args(N=1))


def test_attention_fails_loudly_without_a_gpu(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for path in ("auto", "mfma", "row", "short"):
        assert "no CPU fallback" in _refused(L, *_args(), path=path)
    assert "no CPU fallback" in _refused(L, *_args(N=1), path="dec")


def test_auto_rule_table(L):
    """the model's rule: the short path for 2 .. 60 rows (head sizes multiples of 32 up to 256), the matrix-core chain for longer evals
    at head size 128 and n_threads <= 8, k_attn otherwise"""
    want = {}
    for N in (2, 9, 60, 61, 512):
        for dh in (64, 128):
            for nth in (8, 9):
                want[(N, dh, nth)] = "short" if N <= 60 else ("mfma" if dh == 128 and nth <= 8 else "row")
    got = {k: L.debug_attn_path(k[0], k[1], 0, k[2], 1024) for k in want}
    assert got == want
    assert L.debug_attn_path(1, 128, 5, 8, 1024) is None
    assert L.debug_attn_path(61, 128, 1000, 8, 1024) == "row"             # T beyond the workspace's keys
    assert L.debug_attn_path(9, 512, 0, 8, 1024) == "row"
    assert L.debug_attn_path(9, 128, 0, 64, 1024) == L.debug_attn_path(9, 128, 0, 200, 1024) == "short"   # n_threads clamped as forward() does
