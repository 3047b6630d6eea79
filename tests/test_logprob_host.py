"""CPU: the scoring entry points (llamahip_eval_logprobs, llamahip_perplexity, llamahip_op_logprob) are exported and declared, a
HOST_ONLY handle refuses them with a message, and bad arguments are rejected -- with a message naming the argument -- before any
device work (a HOST_ONLY handle knows n_vocab and n_ctx, so the checks run here without a GPU)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import synth

HOST_ONLY = 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("llamahip_eval_logprobs", "llamahip_perplexity", "llamahip_op_logprob")


def test_scoring_symbols_are_declared_and_exported(L):
    assert all(s in L.declared_symbols() for s in NEW)
    so = os.path.join(ROOT, "llama.swift_amd", "csrc", "libllamahip.so")
    if not (shutil.which("nm") and os.path.exists(so)):
        pytest.skip("needs binutils' nm and the built libllamahip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert all(s in exported for s in NEW)


def test_perplexity_tool_is_built():
    tool = os.path.join(ROOT, "llama.swift_amd", "csrc", "tools", "perplexity")
    assert os.access(tool, os.X_OK)
    r = subprocess.run([tool], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage: perplexity MODEL" in r.stderr


@pytest.fixture
def host_model(L, tmp_path):
    hp = synth.HParams(n_vocab=96, n_embd=64, n_mult=32, n_head=2, n_layer=1)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=5))
    with L.Model(path, n_ctx=32, flags=HOST_ONLY) as m:
        yield m


def _err(L, fn, *a, **kw):
    with pytest.raises(L.LlamaHipError) as e:
        fn(*a, **kw)
    assert e.value.code == -1001 and e.value.message
    return e.value.message


def test_host_only_handle_refuses_every_scoring_call(L, host_model):
    toks = synth.synth_prompt(20, host_model.n_vocab, seed=1)
    assert "HOST_ONLY" in _err(L, host_model.eval_logprobs, toks, 0)
    assert "HOST_ONLY" in _err(L, host_model.eval_logprobs, toks, 0, chunk_tokens=9, targets=np.full(20, -1, np.int32))
    assert "HOST_ONLY" in _err(L, host_model.perplexity, toks, window=8)
    assert "HOST_ONLY" in _err(L, host_model.perplexity, synth.synth_prompt(70, host_model.n_vocab, seed=4), window=0, score_from=0)


def test_bad_arguments_are_rejected_before_device_work(L, host_model):
    m, V = host_model, host_model.n_vocab
    toks = synth.synth_prompt(20, V, seed=2)
    tgt = np.full(20, -1, np.int32)
    tgt[3] = V
    assert "target" in _err(L, m.eval_logprobs, toks, 0, targets=tgt)
    tgt[3] = -2
    assert "target" in _err(L, m.eval_logprobs, toks, 0, targets=tgt)
    assert "context overflow" in _err(L, m.eval_logprobs, toks, 20)
    assert "chunk_tokens" in _err(L, m.eval_logprobs, toks, 0, chunk_tokens=-1)
    bad = toks.copy()
    bad[5] = V
    assert "token id" in _err(L, m.eval_logprobs, bad, 0)
    assert "window" in _err(L, m.perplexity, toks, window=1)
    assert "window" in _err(L, m.perplexity, toks, window=-3)
    long = synth.synth_prompt(80, V, seed=3)
    assert "n_ctx" in _err(L, m.perplexity, long, window=34)               # 33 evaluated tokens > n_ctx 32
    assert "shorter than one window" in _err(L, m.perplexity, toks, window=21)
    assert "shorter than one window" in _err(L, m.perplexity, toks)       # window 0 = n_ctx = 32 > 20 tokens
    assert "score_from" in _err(L, m.perplexity, toks, window=8, score_from=7)
    assert "score_from" in _err(L, m.perplexity, toks, window=8, score_from=-2)
    assert "token id" in _err(L, m.perplexity, bad, window=10)


def test_op_logprob_rejects_bad_arguments(L):
    rows = np.zeros((2, 5), np.float32)
    msg = _err(L, L.op_logprob, rows, np.array([0, 5], np.int32))
    assert "target" in msg
