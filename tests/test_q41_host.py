"""CPU: the Q4_1 mat-mul (k_q41_chain) from the host side -- its three symbols, its launch plan over every mat-mul shape of the four LLaMA
widths and over the shapes of tests/test_gpu_q41_op.py (LDS budget, grid coverage, every plan names a compiled instance), the single-op
entry point llamahip_op_mul_mat_q4_1 refusing bad arguments with a message naming the limit before any device is touched, and the
yardstick of tests/q41_cases.py telling a reversed chain and a fused pair term from the reference's arithmetic on the base case."""
import numpy as np
import pytest

import q41_cases as qc

LDS_BYTES = 163840           # one CU's LDS (gfx950)
# (n_embd, n_ff) of LLaMA 7B / 13B / 30B / 65B; n_vocab 32000
WIDTHS = [(4096, 11008), (5120, 13824), (6656, 17920), (8192, 22016)]
OP_KS, OP_MS = (32, 64, 224, 256, 288, 320, 544, 896, 1376, 4096, 11008), (1, 15, 16, 17, 64, 65, 200)      # tests/test_gpu_q41_op.py
ROWS = list(range(1, 17)) + [17, 100]


def _shapes():
    out = []
    for d, F in WIDTHS:
        out += [(3 * d, d), (d, d), (2 * F, d), (d, F), (32000, d)]
    out += [(M, K) for K in OP_KS for M in OP_MS]
    return out


def test_new_symbols_are_declared_and_exported(L):
    for sym in ("llamahip_op_mul_mat_q4_1", "llamahip_debug_q41_plan", "llamahip_debug_q41_paths"):
        assert sym in L.declared_symbols()
        assert hasattr(L.lib(), sym)
    assert list(L.q41_paths()) == ["chain", "lane"]


def test_plan_over_model_and_test_shapes(L):
    for M, K in _shapes():
        for N in ROWS:
            # (q41_plan raises where the plan names an instance that was never compiled); the tiles of an N-row mat-mul: full ones on the
            # plan of N, a last one of N % 16 rows on the plan of that row count
            tiles = [(N, min(N, 16))] + ([(N % 16, N % 16)] if N > 16 and N % 16 else [])
            for n, tile_rows in tiles:
                p = L.q41_plan(M, K, n)
                assert p is not None, (M, K, n)
                assert p["lds_bytes"] <= LDS_BYTES, (M, K, n, p)
                assert p["grid_x"] * p["rows_per_workgroup"] >= M > (p["grid_x"] - 1) * p["rows_per_workgroup"], (M, K, n, p)      # covers M, no idle workgroup
                assert p["grid_y"] == (n + 15) // 16
                assert tile_rows <= p["rows"] <= 16, (M, K, n, p)
                assert p["chain_lanes"] == p["rows"] * p["rows_per_workgroup"]
                assert p["threads"] % 64 == 0 and p["threads"] <= 1024 and p["threads"] - 256 >= p["chain_lanes"]
                assert p["slab_pairs"] % 16 == 0 and p["lds_bytes"] == 2 * p["slab_pairs"] * 4 * (p["chain_lanes"] + 2 * p["rows"])
    # the 7B matrices give every one of the 256 CUs work at one row
    for M in (4096, 11008, 12288, 22016, 32000):
        assert L.q41_plan(M, 4096, 1)["grid_x"] >= 256


def test_plan_refuses_what_the_kernel_does_not_take(L):
    assert L.q41_plan(64, 48, 4) is None             # K not a multiple of 32
    assert L.q41_plan(64, 0, 4) is None
    assert L.q41_plan(64, 256, 0) is None
    assert L.q41_plan(0, 256, 4) is None


def _refused(L, *a, **kw):
    with pytest.raises(L.LlamaHipError) as e:
        L.op_mul_mat_q4_1(*a, **kw)
    assert e.value.code == -1001
    return e.value.message


def test_bad_arguments_are_refused_before_any_device_is_touched(L):
    w = np.zeros((8, 256 // 32 * 24), np.uint8)
    x = np.ones((2, 256), np.float32)
    assert "K 48 must be a positive multiple of 32" in _refused(L, w, np.ones((2, 48), np.float32), K=48)
    assert "K 0 must be a positive multiple of 32" in _refused(L, w, x, K=0)
    assert "N 0 must be >= 1" in _refused(L, w, np.ones((0, 256), np.float32))
    assert "M 0 must be >= 1" in _refused(L, np.zeros((0, 192), np.uint8), x)
    assert "y_stride 7 < M 8" in _refused(L, w, x, y_stride=7)
    assert "unknown path 3" in _refused(L, w, x, path=3)
    assert "unknown path -1" in _refused(L, w, x, path=-1)
    import torch
    if not torch.cuda.is_available():          # good arguments get as far as the device, and there is no other way to compute
        assert "no CPU fallback" in _refused(L, w, x)


def test_the_yardstick_can_see_what_it_must():
    """conditions on the base case's inputs (seeds 4101 / 4102), not on any kernel: a chain walked backwards and a fused pair term must show"""
    w, x = qc.base_inputs()
    terms = qc.pair_terms(w, x)
    y = qc.chain(terms)
    assert np.isfinite(y).all() and (np.abs(y) > 1e-30).all()
    rev = qc.chain(terms, reverse=True)
    changed = np.count_nonzero(y.view(np.uint32) != rev.view(np.uint32))
    assert changed > y.size // 2, f"the reversed chain changes {changed} of {y.size} outputs"
    fused = qc.chain(qc.pair_terms(w, x, fused=True))
    assert np.count_nonzero(y.view(np.uint32) != fused.view(np.uint32)) >= 1
    assert y.tobytes() == qc.yardstick(w, x).tobytes()


def test_q41_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: q41_plan.cpp (the plan over the model and test shapes, every refusal of the op on exactly sized message buffers) compiled
    with -fsanitize=address,undefined into the stand-alone tools/host_sanitize and run there -- never loaded into python"""
    import os
    import subprocess
    import synth
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "asan"], check=True)
    src = open(os.path.join(csrc, "tools", "host_sanitize.cpp")).read()
    assert "q41_plan(" in src and "q41_op_check(" in src
    assert "q41_plan.cpp" in open(os.path.join(csrc, "Makefile")).read().split("asan:")[1].split("tools:")[0]
    path = str(tmp_path / "m.bin")
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(csrc, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "Q4_1 mat-mul host half" in r.stdout and "clean" in r.stdout, r.stdout + r.stderr
    assert "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
