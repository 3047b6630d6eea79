"""bench.py's own logic, without a GPU: the parser that turns a rocprofv3 kernel trace of the decode loop into the in-situ
per-launch table `roofline` is computed from must recognise every launch layout the library can run; a plain run (no --full)
does the timed steps and nothing else."""
import csv
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CFG = dict(bench.MODELS["7B"], n_layer=3)          # three layers keep the synthetic traces short

LAYOUTS = {
    "fused": ["lh::k_qkv_attn<4, 8, 1, false>(args)", "void lh::k_gemv<0, 1, 16, false, 4>(a)", "void lh::k_gemv<4, 2, 4, true, 1>(a)", "void lh::k_gemv<0, 1, 10, true, 12>(a)"],
    "attn_x": ["void lh::k_gemv<4, 0, 8, true, 1>(a)", "lh::k_dec_attn_x(a)", "void lh::k_gemv<0, 1, 16, false, 4>(a)", "void lh::k_gemv<4, 2, 4, true, 1>(a)",
               "void lh::k_gemv<0, 1, 10, true, 12>(a)"],
    "two": ["void lh::k_gemv<4, 0, 8, true, 1>(a)", "lh::k_dec_scores(a)", "void lh::k_dec_pv_blk<false>(a)", "void lh::k_gemv<0, 1, 16, false, 4>(a)",
            "void lh::k_gemv<4, 2, 4, true, 1>(a)", "void lh::k_gemv<0, 1, 10, true, 12>(a)"],
    "stream": ["void lh::k_gemv<4, 0, 8, true, 1>(a)", "lh::k_dec_scores(a)", "void lh::k_dec_pv_stream<4>(a)", "void lh::k_gemv<0, 1, 16, false, 4>(a)",
               "void lh::k_gemv<4, 2, 4, true, 1>(a)", "void lh::k_gemv<0, 1, 10, true, 12>(a)"],
}


def write_trace(path, layer, tokens):
    t = 1000
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Kind", "Agent_Id", "Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        w.writerow(["KERNEL_DISPATCH", 1, "lh::k_repack_q4(a)", t, t + 500]); t += 1000          # load-time noise before the loop
        for _ in range(tokens):
            seq = ["lh::k_embed_part(a)"] + layer * CFG["n_layer"] + ["void lh::k_gemv<4, 0, 4, true, 1>(a)", "void lh::k_argmax<1>(a)"]
            for i, name in enumerate(seq):
                dur = 1000 * (1 + i % 7)
                w.writerow(["KERNEL_DISPATCH", 1, name, t, t + dur]); t += dur + 300


@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_insitu_trace_parser_knows_every_decode_layout(tmp_path, kind):
    d = tmp_path / kind
    d.mkdir()
    write_trace(str(d / "x_kernel_trace.csv"), LAYOUTS[kind], tokens=5)
    prof = bench.parse_kernel_trace(str(d), CFG)
    assert prof and prof["tokens"] == 5
    roles = set(prof["us"])
    assert {"w1|w3", "w2", "wo", "output", "embed", "argmax", "token_span"} <= roles
    if kind == "fused":
        assert "wq|wk|wv+attention" in roles and "k_qkv_attn" in prof["kernel"]["wq|wk|wv+attention"]
    elif kind == "attn_x":
        assert {"wq|wk|wv", "attention"} <= roles
    else:
        assert {"wq|wk|wv", "attn_scores", "attn_softmax_pv"} <= roles
        assert ("k_dec_pv_stream" if kind == "stream" else "k_dec_pv_blk") in prof["kernel"]["attn_softmax_pv"]
    assert "k_gemv<4, 2, 4" in prof["kernel"]["w1|w3"]


def test_insitu_trace_parser_rejects_a_foreign_sequence(tmp_path):
    d = tmp_path / "bad"
    d.mkdir()
    write_trace(str(d / "x_kernel_trace.csv"), ["lh::k_something_else(a)"] * 4, tokens=3)
    assert bench.parse_kernel_trace(str(d), CFG) is None


def test_token_bytes_follow_the_survey_formula():
    cfg = bench.MODELS["7B"]
    d, F, V, Lr = cfg["n_embd"], bench.n_ff(cfg), cfg["n_vocab"], cfg["n_layer"]
    W = (Lr * (4 * d * d + 3 * d * F) + V * d) // 32 * 20
    assert abs(W - 4.129e9) / 4.129e9 < 0.01                      # 4.129 GB of Q4_0 weights per 7B token
    assert bench.token_bytes(cfg, 100) - bench.token_bytes(cfg, 99) == Lr * 2 * d * 4          # one more K and V row per layer


class _RecordingModel:
    """Stands in for llama_swift_amd.Model in a plain single-GPU bench run: records every call and answers with made-up tokens; any
    other entry point (probes, prompt evaluations, ...) is not part of a plain run and fails the test."""
    calls = []
    n_vocab = 512

    def __init__(self, path, n_ctx=512, **kw):
        assert not kw, kw
        type(self).calls.append(("load", n_ctx))

    def stats(self):
        return {}

    def eval(self, tokens, n_past, n_threads=8):
        type(self).calls.append(("eval", len(tokens), n_past))
        lg = np.zeros(self.n_vocab, np.float32)
        lg[7] = 1.0
        return lg

    def decode_greedy(self, first_token, n_past, n_steps, n_threads=8, want_logits=False):
        type(self).calls.append(("decode_greedy", n_past, n_steps, want_logits))
        toks = ((np.arange(n_steps) + first_token + 1) % self.n_vocab).astype(np.int32)
        return (toks, np.full(self.n_vocab, n_steps, np.float32)) if want_logits else toks

    def close(self):
        type(self).calls.append(("close",))

    def __getattr__(self, name):
        raise AssertionError(f"a plain bench run called Model.{name}")


def _plain_run(monkeypatch, capsys, argv):
    import types

    import torch
    _RecordingModel.calls = []
    monkeypatch.setitem(sys.modules, "llama_swift_amd", types.SimpleNamespace(Model=_RecordingModel))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(bench, "model_path", lambda name, cfg, seed: "model.bin")
    for k in ("RANK", "WORLD_SIZE", "LLAMAHIP_FORCE_PIPELINE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    bench.main()
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1
    return json.loads(out[0]), _RecordingModel.calls


def test_plain_run_times_the_steps_and_nothing_else(monkeypatch, capsys, tmp_path):
    """Without --full a single-GPU run loads, evaluates the prompt, warms up, times exactly --steps steps (past the context end the
    window repeats), writes --dump-outputs and prints one line: no other call reaches the model."""
    line, calls = _plain_run(monkeypatch, capsys, ["--gpus", "1", "--steps", "600", "--warmup", "5", "--model", "tiny", "--dump-outputs", str(tmp_path)])
    window = 512 - len(bench.PROMPT) - 5
    assert calls == [("load", 512), ("eval", len(bench.PROMPT), 0), ("decode_greedy", len(bench.PROMPT), 5, False),
                     ("decode_greedy", len(bench.PROMPT) + 5, window, True), ("decode_greedy", len(bench.PROMPT) + 5, 600 - window, True), ("close",)]
    assert line["steps"] == 600 and line["warmup"] == 5 and line["n_gpus"] == 1 and line["unit"] == "tokens/s" and line["higher_is_better"] is True
    assert line["metric"] == "decode tokens/sec LLaMA-7B Q4_0 @1 GPU; % HBM-roofline on Q4_0 GEMV"
    assert abs(line["ms_per_step"] * line["value"] - 1e3) < 1e-6 * 1e3
    assert "end_to_end_frac" in line["roofline"] and line["parity"]["checked"] is False
    assert line["full_context"]["workload"].startswith("the timed run IS configs[1]")
    for k in ("value_pcie", "cpu_baseline", "prefill", "concurrent_sequences", "batched_sequences", "inprocess_pipeline", "runner"):
        assert k not in line
    toks = np.load(tmp_path / "tokens.npy")
    assert toks.dtype == np.float64 and len(toks) == 600 - window and np.load(tmp_path / "logits.npy").dtype == np.float32


def test_plain_short_run_points_at_full_for_the_full_context(monkeypatch, capsys):
    line, calls = _plain_run(monkeypatch, capsys, ["--steps", "20", "--warmup", "5", "--model", "tiny"])
    assert [c[0] for c in calls] == ["load", "eval", "decode_greedy", "decode_greedy", "close"] and calls[3][1:3] == (len(bench.PROMPT) + 5, 20)
    assert "full_context" not in line and "bench.py --full" in line["config"]["workload"]
    assert "positions 13 .. 32" in line["config"]["workload"]
