"""CPU: the in-place KV shift (include/llamahip.h "generating past the context window", LLAMAHIP_CTX_SHIFT) without a device.

The new symbols; every refusal of llamahip_kv_shift_rows on a HOST_ONLY handle and of llamahip_op_kv_shift's argument checks (the limit
named, no device touched); decode_greedy_window(mode=4) passing the argument checks mode 1 passes; llamahip_debug_rope_table against a C
restatement; the numpy restatement's own properties on the GPU file's cases (tests/kv_shift_ref.py): no subnormal expected output, and the
derived rounding bound against oracle.rope at the new positions; the stand-alone sanitizer program's shift section."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kv_shift_ref as R
import synth

HOST_ONLY = 4
HP = synth.HParams(n_vocab=96, n_embd=128, n_mult=64, n_head=2, n_layer=2)
N_CTX, N_SEQ = 48, 3
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")


@pytest.fixture(scope="module")
def host_only(L, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("kvshift") / "m.bin")
    synth.write_model(path, HP, synth.random_tensors(HP, seed=3))
    with L.Model(path, n_ctx=N_CTX, flags=HOST_ONLY, n_seq=N_SEQ) as m:
        yield m


def test_new_symbols_are_declared_and_exported(L):
    want = {"llamahip_kv_shift_rows", "llamahip_op_kv_shift", "llamahip_debug_rope_table", "llamahip_bench_kv_shift", "llamahip_cur_seq"}
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert want <= exported and want <= set(L.declared_symbols())
    assert not [s for s in exported if "kv_shift" in s and not s.startswith("llamahip_")], "an internal of the shift is exported"
    assert L.CTX_SHIFT == 4 and L.CTX_REEVAL == 1 and L.KV_SHIFT_MAX == 16
    header = open(os.path.join(L.binding.INCLUDE, "llamahip.h")).read()
    assert "#define LLAMAHIP_CTX_SHIFT 4" in header and f"#define LLAMAHIP_KV_SHIFT_ROWS_IN_FLIGHT {L.KV_SHIFT_ROWS_IN_FLIGHT}" in header
    assert R.U == L.KV_SHIFT_ROWS_IN_FLIGHT          # (the batch edges of the op cases are the kernel's)
    # ... and some op case has a long shift whose ranges do not alias beside an aliasing one
    assert any(any(n <= nd and n > R.BAND for _, _, n, nd in c[6]) and any(n > nd for _, _, n, nd in c[6]) for c in R.op_cases())
    assert "NOT the reference's arithmetic" in header.split("LLAMAHIP_CTX_SHIFT   ")[1][:200]
    for name in ("kv_shift_rows", "bench_kv_shift"):
        assert hasattr(L.Model, name)
    assert callable(L.op_kv_shift) and callable(L.rope_table) and hasattr(L.LlamaRunner, "set_overflow")


def test_kv_shift_rows_refusals_name_their_limit_and_touch_no_device(L, host_only):
    ERR = L.binding.ERR_PREDICT
    bad = [([], "1 .. 16"), ([(i % N_SEQ, 4, 1, 1) for i in range(17)], "1 .. 16"),
           ([(-1, 4, 2, 1)], "n_seq"), ([(N_SEQ, 4, 2, 1)], "n_seq"),
           ([(0, 4, 2, 1), (1, 9, 2, 3), (0, 20, 2, 2)], "one shift of a call"),
           ([(0, 4, 2, 0)], "n_discard"), ([(0, 4, 2, -3)], "n_discard"),
           ([(0, 4, -1, 1)], "n_ctx"), ([(0, -1, 2, 1)], "n_ctx"), ([(0, N_CTX - 1, 2, 1)], "n_ctx"), ([(0, N_CTX + 1, 0, 1)], "n_ctx"),
           ([(0, 4, 2, 5)], "below row 0"), ([(1, 0, 1, 1)], "below row 0"), ([(2, N_CTX, 0, N_CTX + 1)], "below row 0")]
    for shifts, word in bad:
        with pytest.raises(L.LlamaHipError) as e:
            host_only.kv_shift_rows(shifts)
        assert e.value.code == ERR and "llamahip_kv_shift_rows" in e.value.message and word in e.value.message, (shifts, e.value.message)
    # the arguments are in order: the handle is refused last, as HOST_ONLY (an empty entry beside a real one, the largest rotation)
    for shifts in ([(0, 4, 2, 1)], [(1, 10, 0, 3), (2, N_CTX - 1, 1, N_CTX - 1)], [(0, N_CTX, 0, N_CTX)]):
        with pytest.raises(L.LlamaHipError) as e:
            host_only.kv_shift_rows(shifts)
        assert e.value.code == ERR and "HOST_ONLY" in e.value.message, e.value.message
    lib, err = L.lib(), C.create_string_buffer(256)
    one = (C.c_int32 * 1)(4)
    zero = (C.c_int32 * 1)(0)
    assert lib.llamahip_kv_shift_rows(None, 1, zero, one, one, one, err, len(err)) == ERR and b"null model" in err.value
    for k in range(4):
        arrs = [zero, one, one, one]
        arrs[k] = None
        assert lib.llamahip_kv_shift_rows(host_only._h, 1, *arrs, err, len(err)) == ERR and b"null array" in err.value
    assert lib.llamahip_kv_shift_rows(host_only._h, 1, zero, one, one, one, None, 0) == ERR
    ms = C.c_double(0)
    assert lib.llamahip_bench_kv_shift(host_only._h, 1, zero, one, one, one, 5, C.byref(ms), err, len(err)) == ERR and b"HOST_ONLY" in err.value
    assert lib.llamahip_cur_seq(host_only._h) == 0 and lib.llamahip_cur_seq(None) == -1


def test_op_kv_shift_argument_checks_name_their_limit(L):
    """every check comes before the device is asked for: they read the same on a machine without one"""
    K = np.zeros((2, 2, 16, 8), np.float32)
    V = np.zeros_like(K)
    ok = [(1, 4, 2, 1)]
    for shifts, word in (([], "1 .. 16"), ([(i, 4, 1, 1) for i in range(17)], "1 .. 16"), ([(2, 4, 2, 1)], "out of range [0, 2)"), ([(-1, 4, 2, 1)], "out of range"),
                         ([(0, 4, 2, 1), (0, 9, 2, 1)], "one shift of a call"), ([(0, 4, 2, 0)], "n_discard"), ([(0, 15, 2, 1)], "n_ctx"),
                         ([(0, 4, -2, 1)], "n_ctx"), ([(0, 4, 2, 5)], "below row 0")):
        with pytest.raises(L.LlamaHipError) as e:
            L.op_kv_shift(K, V, 4, shifts)
        assert "llamahip_op_kv_shift" in e.value.message and word in e.value.message, (shifts, e.value.message)
    for dh, word in ((3, "head size"), (1, "head size"), (6, "head size"), (0, "head size")):
        with pytest.raises(L.LlamaHipError) as e:
            L.op_kv_shift(K, V, dh, ok)
        assert word in e.value.message, e.value.message
    with pytest.raises(L.LlamaHipError) as e:
        L.op_kv_shift(np.zeros((2, 2, 16, 6), np.float32), np.zeros((2, 2, 16, 6), np.float32), 2, ok)
    assert "multiple of 4" in e.value.message
    lib, err = L.lib(), C.create_string_buffer(256)
    a = (C.c_int32 * 1)(1)
    assert lib.llamahip_op_kv_shift(None, None, 2, 2, 16, 8, 4, 1, a, a, a, a, err, len(err)) == L.binding.ERR_PREDICT and b"Kc, Vc not NULL" in err.value
    assert lib.llamahip_op_kv_shift(K.ctypes.data, V.ctypes.data, 2, 2, 16, 8, 4, 1, None, a, a, a, err, len(err)) == L.binding.ERR_PREDICT and b"null array" in err.value
    assert not K.any() and not V.any()


def test_decode_greedy_window_takes_the_shift_mode(L, host_only):
    """mode 4 passes every argument check mode 1 passes (the HOST_ONLY handle is refused last) and is refused where mode 1 is"""
    ctx = np.arange(3, 13, dtype=np.int32)
    ok = dict(first_token=5, n_steps=100, n_past=10, context=ctx, n_keep=4, mode=L.CTX_SHIFT, chunk_tokens=9)
    for start in (dict(), dict(chunk_tokens=0), dict(n_keep=0), dict(n_keep=46), dict(n_past=48, context=np.ones(48, np.int32))):
        for mode in (L.CTX_REEVAL, L.CTX_SHIFT):
            with pytest.raises(L.LlamaHipError) as e:
                host_only.decode_greedy_window(**dict(ok, mode=mode, **start))
            assert e.value.code == L.binding.ERR_PREDICT and "HOST_ONLY" in e.value.message, (mode, start, e.value.message)
    bad = [(dict(mode=5), "mode"), (dict(mode=-4), "mode"), (dict(n_steps=0), "n_steps"), (dict(n_past=49, context=np.zeros(49, np.int32)), "n_past"),
           (dict(context=ctx[:9]), "n_context"), (dict(first_token=96), "token id"), (dict(chunk_tokens=-1), "chunk_tokens"), (dict(n_keep=47), "n_keep")]
    for change, word in bad:
        with pytest.raises(L.LlamaHipError) as e:
            host_only.decode_greedy_window(**dict(ok, **change))
        assert "llamahip_decode_greedy_window" in e.value.message and word in e.value.message, (change, e.value.message)


TABLE_C = r"""
#define _GNU_SOURCE
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char **argv) {
    const int n_ctx = atoi(argv[1]), dh = atoi(argv[2]);
    FILE *f = fopen(argv[3], "wb");
    if (!f) return 1;
    for (int p = 0; p < n_ctx; p++)
        for (int i0 = 0; i0 < dh; i0 += 2) {
            const double theta = pow(10000.0, ((double) -i0) / dh);
            double out[2], sn, cs;
            sincos(p * theta, &sn, &cs);
            out[0] = cs; out[1] = sn;
            if (fwrite(out, sizeof(double), 2, f) != 2) return 1;
        }
    return fclose(f) != 0;
}
"""


def test_debug_rope_table_is_the_c_restatement(L, tmp_path):
    """[n_ctx][dh / 2][cos, sin] of position * 10000^(-2 pair / dh) by the C library's pow and sincos, bit for bit; row 0 is (1, 0)"""
    src, exe = tmp_path / "table.c", tmp_path / "table"
    src.write_text(TABLE_C)
    subprocess.run(["cc", "-O2", "-o", str(exe), str(src), "-lm"], check=True)
    for n_ctx, dh in ((40, 64), (64, 128), (2048, 128), (7, 2)):
        out = tmp_path / f"t_{n_ctx}_{dh}.bin"
        subprocess.run([str(exe), str(n_ctx), str(dh), str(out)], check=True)
        want = np.fromfile(str(out), np.float64).reshape(n_ctx, dh // 2, 2)
        got = L.rope_table(n_ctx, dh)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n_ctx, dh)
        assert np.all(got[0, :, 0] == 1.0) and np.all(got[0, :, 1] == 0.0)
    out = np.zeros(4, np.float64)
    for n_ctx, dh, buf in ((0, 4, out), (2, 3, out), (2, 0, out), (1, 4, None)):
        assert L.lib().llamahip_debug_rope_table(n_ctx, dh, None if buf is None else buf.ctypes.data) == -1
    assert not out.any()


@pytest.mark.parametrize("case", R.op_cases(), ids=[c[0] for c in R.op_cases()])
def test_restatement_has_no_subnormal_output_and_keeps_the_bound(L, oracle, case):
    """on every case of tests/test_gpu_kv_shift_op.py: the expected outputs are zero or normal fp32 (the contract's condition on the inputs),
    the moved V rows are the source's bits, the moved K rows lie within 3.5 * 2^-24 * ||pair|| of oracle.rope at the new positions, and
    nothing outside the destination rows changes"""
    _, n_slots, n_layers, n_ctx, d, dh, shifts = case
    raw, K0, V0 = R.make_caches(oracle, 77, n_slots, n_layers, n_ctx, d, dh)
    K, V = K0.copy(), V0.copy()
    R.shift_restated(K, V, L.rope_table(n_ctx, dh), dh, shifts)
    assert R.no_subnormals(K) and R.no_subnormals(V)
    changed = np.zeros((n_slots, n_ctx), bool)
    worst = 0.0
    for slot, rb, n, nd in shifts:
        changed[slot, rb - nd:rb - nd + n] = True
        for il in range(n_layers):
            assert np.array_equal(V[slot, il, rb - nd:rb - nd + n].view(np.uint32), V0[slot, il, rb:rb + n].view(np.uint32))
            if n:
                worst = max(worst, R.within_bound(K[slot, il, rb - nd:rb - nd + n], R.direct_keys(oracle, raw[slot, il, rb:rb + n], rb - nd, dh), raw[slot, il, rb:rb + n]))
    print(f"worst |shifted - direct| / (2^-24 ||pair||) = {worst:.3f} (bound 3.5)")
    assert worst < 3.5
    keep = ~changed[:, None, :, None]
    assert np.array_equal(np.where(keep, K.view(np.uint32), 0), np.where(keep, K0.view(np.uint32), 0))
    assert np.array_equal(np.where(keep, V.view(np.uint32), 0), np.where(keep, V0.view(np.uint32), 0))


def test_bound_over_random_positions_and_magnitudes(L, oracle):
    """200 random (position, n_discard) at head size 128, one row each in the three magnitude regimes"""
    rng = np.random.default_rng(5)
    n_ctx, d, dh = 2048, 256, 128
    tab = L.rope_table(n_ctx, dh)
    worst = 0.0
    for _ in range(200):
        pos = int(rng.integers(1, n_ctx))
        nd = int(rng.integers(1, pos + 1))
        raw = (rng.standard_normal((3, d)).astype(np.float32) * np.asarray(R.MAGS, np.float32)[:, None]).astype(np.float32)
        k_pos = np.concatenate([R.direct_keys(oracle, raw[i:i + 1], pos, dh) for i in range(3)])
        direct = np.concatenate([R.direct_keys(oracle, raw[i:i + 1], pos - nd, dh) for i in range(3)])
        worst = max(worst, R.within_bound(R.rotate_down(k_pos, tab, nd, dh), direct, raw))
    print(f"worst ratio over 200 draws: {worst:.3f}")
    assert worst < 3.5


def test_shift_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: the greedy loop in legs and the driver in shift mode against a stubbed llamahip_kv_shift_rows, the stub's call sequence
    replayed against the plan, in the stand-alone tools/host_sanitize -- never loaded into python"""
    subprocess.run(["make", "-s", "-C", CSRC, "asan"], check=True)
    src = open(os.path.join(CSRC, "tools", "host_sanitize.cpp")).read()
    assert "int llamahip_kv_shift_rows(" in src and "LLAMAHIP_CTX_SHIFT" in src
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(CSRC, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout and "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if "shift mode:" in ln]
    assert len(line) == 1, r.stdout
    counts = [int(w) for w in line[0].split() if w.isdigit()]
    assert len(counts) == 2 and min(counts) > 0, line[0]          # (shifts replayed in the loop's legs / in the driver's runs)
