"""CPU: the op-level prompt GEMM entry point (llamahip_op_prompt_gemm_q4_0) is declared and exported, refuses bad arguments with a message
before any device work, and without a GPU fails loudly; the launch counters name the fast kernel's family."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "llamahip_op_prompt_gemm_q4_0"


def test_prompt_gemm_symbol_is_declared_and_exported(L):
    assert SYM in L.declared_symbols()
    so = os.path.join(ROOT, "llama.swift_amd", "csrc", "libllamahip.so")
    if not (shutil.which("nm") and os.path.exists(so)):
        pytest.skip("needs binutils' nm and the built libllamahip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert SYM in {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_launch_counters_include_the_fast_kernel(L):
    p = L.gemm_paths()
    assert list(p) == ["mfma", "rows", "lds", "gemv", "set", "fast"]
    assert all(v >= 0 for v in p.values()) and p["fast"] <= p["mfma"]


def _refused(L, *a, **kw):
    with pytest.raises(L.LlamaHipError) as e:
        L.op_prompt_gemm_q4_0(*a, **kw)
    assert e.value.code == -1001
    return e.value.message


def test_bad_arguments_are_refused_before_device_work(L):
    w = synth.quantize_q4_0_offline(np.ones((8, 256), np.float32))
    x = np.ones((3, 256), np.float32)
    assert "multiple of 64" in _refused(L, synth.quantize_q4_0_offline(np.ones((8, 96), np.float32)), np.ones((3, 96), np.float32))
    assert "y_stride 7 < M 8" in _refused(L, w, x, y_stride=7)
    for bad in (-1, 7, 99):                                  # 7 (the mat-vec) is reported, never requested
        assert f"unknown path {bad}" in _refused(L, w, x, path=bad)


def test_prompt_gemm_fails_loudly_without_a_gpu(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    w = synth.quantize_q4_0_offline(np.ones((8, 256), np.float32))
    for path in ("auto", "fast"):
        assert "no CPU fallback" in _refused(L, w, np.ones((65, 256), np.float32), path=path)
