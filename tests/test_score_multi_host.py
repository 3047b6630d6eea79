"""CPU: the host half of llamahip_eval_logprobs_multi and llamahip_score_choices -- the symbols, every refusal of the two entry points on a
HOST_ONLY handle (the arguments first, the limit and the function named, the handle last), and the host code (argument checks, the scored
rows, the scatter of compacted results back to row order) under ASan + UBSan in the stand-alone program `make asan` builds."""
import os
import subprocess

import numpy as np
import pytest

import synth

HOST_ONLY = 4
HP = synth.HParams(n_vocab=96, n_embd=128, n_mult=64, n_head=2, n_layer=2)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
t = lambda n: np.arange(1, n + 1, dtype=np.int32)


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("score") / "m.bin")
    synth.write_model(path, HP, synth.random_tensors(HP, seed=3))
    return path


@pytest.fixture(scope="module")
def host_model(L, model_path):
    with L.Model(model_path, n_ctx=48, flags=HOST_ONLY, n_seq=3) as m:
        yield m


def refused(L, call, fn, *words):
    with pytest.raises(L.LlamaHipError) as e:
        call()
    msg = e.value.message
    assert e.value.code == L.binding.ERR_PREDICT and fn in msg and all(w in msg for w in words), msg
    return msg


def test_new_symbols_are_declared_and_exported(L):
    names = L.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for fn in ("llamahip_eval_logprobs_multi", "llamahip_score_choices"):
        assert fn in names and hasattr(L.lib(), fn) and fn in exported, fn
    assert not [s for s in exported if "score_multi" in s or "score_scatter" in s or "score_choices_check" in s]          # (lh:: internals stay local)
    assert hasattr(L.Model, "eval_logprobs_multi") and hasattr(L.Model, "score_choices") and L.SCORE_CHOICES_MAX == 16


def test_eval_logprobs_multi_refusals_touch_no_device(L, host_model):
    fn = "llamahip_eval_logprobs_multi"
    ok = dict(slots=[2, 0], n_past=[0, 5], token_lists=[t(4), t(9)], chunk_tokens=9)
    tg = lambda last: [np.full(4, -1, np.int32), np.array([1, 2, 3, 4, 5, 6, 7, 8, last], np.int32)]
    bad = [(dict(slots=[], n_past=[], token_lists=[]), ("n_seqs (0)", "1 .. 3")),
           (dict(slots=[0, 1, 2, 0], n_past=[0] * 4, token_lists=[t(1)] * 4), ("n_seqs (4)", "1 .. 3")),
           (dict(slots=[1, 1]), ("slot 1", "named twice")), (dict(slots=[3, 0]), ("out of range [0, 3)",)),
           (dict(token_lists=[t(4), t(0)]), ("n_tokens[1]", ">= 1")),
           (dict(n_past=[0, 40]), ("context overflow", "n_ctx (48)")), (dict(n_past=[-1, 5]), ("context overflow",)),
           (dict(token_lists=[t(4), np.array([1, 96], np.int32)]), ("token id 96", "[0, 96)")),
           (dict(targets=tg(96)), ("target 96", "[-1, 96)")), (dict(targets=tg(-2)), ("target -2", "[-1, 96)")),
           (dict(chunk_tokens=-1), ("chunk_tokens (-1)", ">= 0"))]
    for change, words in bad:
        msg = refused(L, lambda: host_model.eval_logprobs_multi(**dict(ok, **change)), fn, *words)
        assert "HOST_ONLY" not in msg, msg
    # targets of -1 and of n_vocab - 1 are inside the range; the arguments are fine, the handle is refused, last
    for targets in (None, tg(95), np.concatenate(tg(-1))):
        refused(L, lambda: host_model.eval_logprobs_multi(**ok, targets=targets), fn, "HOST_ONLY")
    with pytest.raises(ValueError):
        host_model.eval_logprobs_multi(**ok, targets=np.zeros(12, np.int32))


def test_row_cap_and_null_handle(L, model_path):
    """R = 2049 needs a context that holds it; a null handle is refused before anything is read"""
    with L.Model(model_path, n_ctx=1100, flags=HOST_ONLY, n_seq=2) as m:
        one = lambda n: np.ones(n, np.int32)
        refused(L, lambda: m.eval_logprobs_multi([0, 1], [0, 0], [one(1024), one(1025)]), "llamahip_eval_logprobs_multi", "LLAMAHIP_EVAL_MULTI_MAX_ROWS", "2049")
        refused(L, lambda: m.eval_logprobs_multi([0, 1], [0, 0], [one(1024), one(1024)]), "llamahip_eval_logprobs_multi", "HOST_ONLY")
    import ctypes as C
    err = C.create_string_buffer(256)
    one = np.ones(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.lib().llamahip_eval_logprobs_multi(None, 8, 1, p(one * 0), p(one * 0), p(one), p(one), 0, None, None, None, None, None, err, len(err))
    assert rc == L.binding.ERR_PREDICT and b"llamahip_eval_logprobs_multi: null model" in err.value
    rc = L.lib().llamahip_score_choices(None, 8, p(one), 1, 1, p(one), p(one), 0, None, None, None, err, len(err))
    assert rc == L.binding.ERR_PREDICT and b"llamahip_score_choices: null model" in err.value


def test_score_choices_refusals_touch_no_device(L, host_model, model_path):
    fn = "llamahip_score_choices"
    ok = dict(context=t(10), endings=[t(3), t(5), t(1)], chunk_tokens=9)
    bad = [(dict(endings=[]), ("n_choices (0)", "1 .. 3")), (dict(endings=[t(1)] * 4), ("n_choices (4)", "1 .. 3")),
           (dict(endings=[t(1)] * 17), ("n_choices (17)", "LLAMAHIP_SCORE_CHOICES_MAX 16")),
           (dict(context=[]), ("n_context (0)", ">= 1")), (dict(endings=[t(3), t(0), t(1)]), ("n_ending[1]", ">= 1")),
           (dict(endings=[t(3), t(40)]), ("context overflow", "n_ctx (48)")),
           (dict(context=[1, 96]), ("context token id 96", "[0, 96)")), (dict(endings=[t(3), [5, -1]]), ("ending token id -1", "[0, 96)")),
           (dict(chunk_tokens=-1), ("chunk_tokens (-1)", ">= 0"))]
    for change, words in bad:
        msg = refused(L, lambda: host_model.score_choices(**dict(ok, **change)), fn, *words)
        assert "HOST_ONLY" not in msg, msg
    refused(L, lambda: host_model.score_choices(**ok), fn, "HOST_ONLY")
    refused(L, lambda: host_model.score_choices(t(10), [t(39)]), fn, "HOST_ONLY")          # 9 + 39 = n_ctx: fits
    # 16 choices pass the argument check on a handle with the slots for them; 17 never do
    with L.Model(model_path, n_ctx=48, flags=HOST_ONLY, n_seq=20) as m:
        refused(L, lambda: m.score_choices(t(10), [t(2)] * 16), fn, "HOST_ONLY")
        refused(L, lambda: m.score_choices(t(10), [t(2)] * 17), fn, "n_choices (17)", "1 .. 16")


def test_score_host_code_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: eval_multi.cpp's scoring half (the argument checks over exactly sized arrays and message buffers, the scored rows, the
    scatter of compacted results from a buffer of exactly 16 bytes per scored row) compiled with -fsanitize=address,undefined into the
    stand-alone tools/host_sanitize and run there -- never loaded into python"""
    subprocess.run(["make", "-s", "-C", CSRC, "asan"], check=True)
    src = open(os.path.join(CSRC, "tools", "host_sanitize.cpp")).read()
    assert "lh::score_multi_check(" in src and "lh::score_scatter(" in src and "lh::score_multi_rows(" in src and "lh::score_choices_check(" in src
    assert "eval_multi.cpp" in open(os.path.join(CSRC, "Makefile")).read().split("asan:")[1].split("tools:")[0]
    path = str(tmp_path / "m.bin")
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(CSRC, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout and "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
    line = [ln for ln in r.stdout.splitlines() if "scoring over KV slots" in ln]
    assert len(line) == 1 and " 0 " not in line[0], r.stdout
