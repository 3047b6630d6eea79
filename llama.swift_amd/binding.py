"""ctypes binding of include/llamahip.h (no torch types cross the boundary)."""
from __future__ import annotations

import collections
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.path.join(CSRC, os.environ.get("LLAMAHIP_LIB", "libllamahip.so"))     # LLAMAHIP_LIB=libllamahip_probe.so: measurement build
INCLUDE = os.path.join(ROOT, "include")

ERR_LOAD, ERR_PREDICT = -1000, -1001
CTX_REEVAL = 1          # LLAMAHIP_CTX_REEVAL: what to do when the KV cache is full
CTX_SHIFT = 4           # LLAMAHIP_CTX_SHIFT: ... the in-place shift (NOT the reference's arithmetic: opt-in)
KV_SHIFT_MAX = 16       # LLAMAHIP_KV_SHIFT_MAX: the shifts of one Model.kv_shift_rows / op_kv_shift call
KV_SHIFT_ROWS_IN_FLIGHT = 8   # LLAMAHIP_KV_SHIFT_ROWS_IN_FLIGHT: rows a thread of k_kv_shift_rows loads before it stores them
SCORE_CHOICES_MAX = 16  # LLAMAHIP_SCORE_CHOICES_MAX: the endings of one Model.score_choices call
POOL_LAST, POOL_MEAN = 0, 1  # LLAMAHIP_POOL_*: how Model.text_embedding pools a text's final-norm rows
_POOLS = {"last": POOL_LAST, "mean": POOL_MEAN}
DUMP_NAMES = [
    "layer_in", "attn_normed", "q", "k", "v", "q_roped", "kq_softmax", "kqv", "kqv_merged",
    "wo_out", "ffn_in", "ffn_normed", "w3_out", "w1_out", "silu_mul", "w2_out", "layer_out",
]
bench_gemv_names = {0: "wq|wk|wv", 1: "wo", 2: "w1|w3", 3: "w2", 4: "output"}


DONE_LENGTH, DONE_STOP = 1, 2      # LLAMAHIP_DONE_*


class LlamaHipError(RuntimeError):
    """Mirrors NSError(domain LlamaErrorDomain, code) (Sources/llamaObjCxx/headers/LlamaError.h:12-19)."""

    domain = "com.alexrozanski.llama.error"

    def __init__(self, code: int, message: str):
        super().__init__(f"[{self.domain} {code}] {message}")
        self.code = code
        self.message = message


def build(verbose: bool = False) -> str:
    """Compile libllamahip.so + tools in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", CSRC, "all"], capture_output=not verbose, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libllamahip.so failed:\n" + (r.stdout or "") + (r.stderr or ""))
    return LIB_PATH


_lib = None


class _BeamOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "n_threads", "n_beams", "n_predict", "stop_token", "n_return", "length_norm", "chunk_tokens")]


class _BeamHyp(C.Structure):
    _fields_ = [("length", C.c_int32), ("reason", C.c_int32), ("slot", C.c_int32), ("reserved", C.c_int32), ("score", C.c_double)]


class _BeamStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32)] + [(n, C.c_int64) for n in (
        "n_steps", "n_rows", "n_set_steps", "n_fallback_steps", "n_copy_launches", "n_copied_rows", "n_stop", "n_dead")]


class _Opts(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("layer_begin", C.c_int32),
                ("layer_end", C.c_int32), ("n_parts", C.c_int32), ("flags", C.c_int32), ("n_seq", C.c_int32),
                ("n_devices", C.c_int32), ("devices", C.c_int32 * 8)]


class _GemvBench(C.Structure):
    _fields_ = [("M", C.c_int32), ("K", C.c_int32), ("iters", C.c_int32), ("ms_total", C.c_float),
                ("algo_bytes", C.c_double)]


class _EvalMultiStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_rows", C.c_int32), ("n_passes", C.c_int32), ("n_short_segs", C.c_int32),
                ("n_long_segs", C.c_int32), ("attn_groups", C.c_int32)]


class _ScoreMultiStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_rows", C.c_int32), ("n_scored_rows", C.c_int32), ("n_passes", C.c_int32),
                ("n_short_segs", C.c_int32), ("n_long_segs", C.c_int32)]


class _LookupStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_verify_steps", C.c_int32), ("n_single_steps", C.c_int32), ("n_drafted", C.c_int64), ("n_accepted", C.c_int64)]


class _SchedOpts(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_threads", C.c_int32), ("max_active", C.c_int32), ("chunk_tokens", C.c_int32),
                ("row_budget", C.c_int32), ("repeat_penalty", C.c_double), ("top_p", C.c_double), ("temp", C.c_double), ("top_k", C.c_int32),
                ("draft_len", C.c_int32), ("ngram_min", C.c_int32), ("ngram_max", C.c_int32), ("corpus", C.c_void_p), ("n_corpus", C.c_int32),
                ("prefix_share", C.c_int32)]


class _Request(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("prompt", C.c_void_p), ("n_prompt", C.c_int32), ("n_predict", C.c_int32),
                ("stop_token", C.c_int32), ("sampler", C.c_void_p)]


class _RequestCst(_Request):
    """llamahip_request as it is now: the constraint fields appended behind _Request's (the struct is size-versioned; the old size is still taken)"""
    _fields_ = [("constraint", C.c_void_p), ("constraint_state", C.c_int32)]


class _SchedOptsForced(_SchedOpts):
    """llamahip_sched_opts as it is now: forced_drafts appended behind _SchedOpts' fields"""
    _fields_ = [("forced_drafts", C.c_int32)]


class _SchedEvent(C.Structure):
    _fields_ = [("id", C.c_int64), ("kind", C.c_int32), ("token", C.c_int32), ("exact", C.c_int32), ("slot", C.c_int32),
                ("position", C.c_int32), ("reason", C.c_int32)]


class _SchedStats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_graph_captures", C.c_int32), ("n_steps", C.c_int64), ("n_mixed_steps", C.c_int64),
                ("n_set_steps", C.c_int64), ("n_single_steps", C.c_int64), ("n_fallback_steps", C.c_int64), ("n_rows", C.c_int64),
                ("n_prompt_rows", C.c_int64), ("n_tokens", C.c_int64), ("n_submitted", C.c_int64), ("n_done", C.c_int64),
                ("n_draft_steps", C.c_int64), ("n_drafted", C.c_int64), ("n_accepted", C.c_int64), ("n_emit_segs", C.c_int64), ("n_dropped", C.c_int64)]


class _SchedStatsPrefix(_SchedStats):
    """llamahip_sched_stats as it is now: the counters of shared prompt prefixes appended behind _SchedStats' (the struct is size-versioned)"""
    _fields_ = [("n_shared_rows", C.c_int64), ("n_copied_rows", C.c_int64), ("n_copy_launches", C.c_int64)]


class _SchedStatsDfa(_SchedStatsPrefix):
    """... and the counters of constrained requests behind those"""
    _fields_ = [("n_dfa_rows", C.c_int64), ("n_forced_drafted", C.c_int64), ("n_forced_accepted", C.c_int64)]


class _Stats(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("weight_bytes_device", C.c_int64), ("kv_bytes_device", C.c_int64),
                ("n_evals", C.c_int64), ("t_load_ms", C.c_double), ("t_eval_ms_total", C.c_double), ("n_stages", C.c_int32), ("hand_off", C.c_int32)]


def lib() -> C.CDLL:
    """Load the HIP library; never falls back to anything else."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the HIP path)")
    # PyTorch-ROCm bundles its own libamdhip64.so.7 + libhsa-runtime64; whichever HIP runtime is
    # loaded first serves the whole process (same SONAME).  If this library pulled in the system
    # runtime first, a later torch.cuda init would pair it with torch's bundled HSA runtime and find
    # no GPUs -- so when torch is installed, let it load its runtime first (torch is only plumbing
    # here: device tensors for the pipeline hand-off and torch.distributed).
    if not os.environ.get("LLAMAHIP_NO_TORCH"):          # (measurement tools that never touch torch skip its slow import)
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    vp, i32, cp, sz = C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t
    L.llamahip_version.restype = cp
    L.llamahip_model_load.argtypes = [cp, i32, C.POINTER(_Opts), C.POINTER(vp), cp, sz]
    L.llamahip_eval.argtypes = [vp, i32, i32, vp, i32, vp, cp, sz]
    L.llamahip_eval_chunks.argtypes = [vp, i32, i32, vp, i32, i32, vp, cp, sz]
    L.llamahip_eval_logprobs.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, cp, sz]
    L.llamahip_perplexity.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, vp, vp, cp, sz]
    L.llamahip_model_free.argtypes = [vp]
    for fn in ("n_vocab", "n_ctx", "n_embd", "n_head", "n_layer", "n_ff", "n_parts"):
        getattr(L, "llamahip_" + fn).argtypes = [vp]
        getattr(L, "llamahip_" + fn).restype = i32
    L.llamahip_token_text.argtypes = [vp, i32, C.POINTER(C.c_uint32)]
    L.llamahip_token_text.restype = vp
    L.llamahip_tokenize.argtypes = [vp, cp, i32, vp, i32]
    L.llamahip_tokenize.restype = i32
    L.llamahip_sampler_new.argtypes = [i32, i32]
    L.llamahip_sampler_new.restype = vp
    L.llamahip_sampler_free.argtypes = [vp]
    L.llamahip_sampler_accept.argtypes = [vp, i32]
    L.llamahip_eval_topk.argtypes = [vp, i32, i32, vp, i32, vp, i32, C.c_double, i32, C.c_double, vp, vp, vp, vp, cp, sz]
    L.llamahip_sample_from_candidates.argtypes = [vp, vp, vp, i32, C.c_double]
    L.llamahip_sample_from_candidates.restype = i32
    L.llamahip_sampler_window.argtypes = [vp, vp, i32]
    L.llamahip_sampler_window.restype = i32
    L.llamahip_sampler_random_prompt.argtypes = [vp]
    L.llamahip_sampler_random_prompt.restype = cp
    L.llamahip_sample_top_p_top_k.argtypes = [vp, vp, vp, C.c_double, i32, C.c_double, C.c_double]
    L.llamahip_sample_top_p_top_k.restype = i32
    L.llamahip_decode_greedy.argtypes = [vp, i32, i32, i32, i32, vp, vp, cp, sz]
    L.llamahip_verify_greedy.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp, vp, cp, sz]
    L.llamahip_decode_greedy_lookup.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp, i32, i32, i32, i32, vp, vp, C.POINTER(_LookupStats), cp, sz]
    L.llamahip_verify_sample.argtypes = [vp, i32, i32, i32, vp, i32, vp, C.c_double, i32, C.c_double, C.c_double, vp, vp, vp, cp, sz]
    L.llamahip_decode_sample_lookup.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp, i32, i32, i32, i32, vp, C.c_double, i32, C.c_double, C.c_double, vp, vp,
                                                C.POINTER(_LookupStats), cp, sz]
    L.llamahip_op_topk_slide.argtypes = [vp, i32, i32, vp, i32, C.c_double, i32, C.c_double, vp, vp, vp, cp, sz]
    L.llamahip_lookup_draft.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp]
    L.llamahip_lookup_draft.restype = i32
    L.llamahip_op_verify_rows.argtypes = [vp, i32, i32, vp, vp, vp, cp, sz]
    L.llamahip_op_verify_rows_set.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, cp, sz]
    L.llamahip_verify_greedy_multi.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, cp, sz]
    L.llamahip_decode_greedy_lookup_multi.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, i32, i32, i32, i32, vp, vp, cp, sz]
    L.llamahip_verify_sample_multi.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, C.c_double, i32, C.c_double, C.c_double, vp, vp, vp, cp, sz]
    L.llamahip_decode_sample_lookup_multi.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, i32, i32, i32, i32, vp, C.c_double, i32, C.c_double, C.c_double, vp, vp, vp, cp, sz]
    L.llamahip_op_topk_slide_set.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, vp, C.c_double, i32, C.c_double, vp, vp, vp, cp, sz]
    L.llamahip_lookup_deal_rows.argtypes = [vp, i32, i32, vp]
    L.llamahip_lookup_deal_rows.restype = i32
    L.llamahip_decode_greedy_multi.argtypes = [vp, i32, i32, vp, vp, i32, vp, cp, sz]
    L.llamahip_decode_sample_multi.argtypes = [vp, i32, i32, vp, vp, i32, vp, C.c_double, i32, C.c_double, C.c_double, vp, vp, cp, sz]
    L.llamahip_eval_debug.argtypes = [vp, i32, i32, vp, i32, vp, vp, i32, vp, C.c_int64, vp, cp, sz]
    L.llamahip_eval_stage.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, cp, sz]
    L.llamahip_stage_bind.argtypes = [vp, i32, i32, vp, vp, vp, vp, cp, sz]
    L.llamahip_stage_step.argtypes = [vp, i32, i32, vp, cp, sz]
    L.llamahip_stage_trace.argtypes = [vp, i32, vp, vp, i32, cp, sz]
    L.llamahip_stage_step_set.argtypes = [vp, vp, i32, i32, vp, cp, sz]
    L.llamahip_stage_set_applies.argtypes = [vp, i32, i32]
    L.llamahip_stage_set_applies.restype = i32
    L.llamahip_stage_logits.argtypes = [vp, i32, vp, cp, sz]
    L.llamahip_stage_mailbox.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), vp, vp, cp, sz]
    L.llamahip_stage_mailbox_connect.argtypes = [vp, i32, vp, vp, vp, vp, cp, sz]
    L.llamahip_quantize_file.argtypes = [cp, cp, i32, cp, sz]
    L.llamahip_kv_read.argtypes = [vp, i32, i32, vp, vp, cp, sz]
    L.llamahip_set_seq.argtypes = [vp, i32, cp, sz]
    L.llamahip_ctx_overflow_plan.argtypes = [i32, i32, i32, C.POINTER(i32)]
    L.llamahip_ctx_overflow_plan.restype = i32
    L.llamahip_decode_greedy_window.argtypes = [vp, i32, i32, i32, i32, vp, i32, i32, i32, i32, vp, vp, C.POINTER(i32), cp, sz]
    L.llamahip_tensor_bytes.argtypes = [vp, cp, vp, C.c_int64]
    L.llamahip_tensor_bytes.restype = C.c_int64
    L.llamahip_op_mul_mat_q4_0.argtypes = [vp, i32, i32, vp, i32, vp, cp, sz]
    L.llamahip_op_quantize_row_q4_0.argtypes = [vp, i32, vp, cp, sz]
    L.llamahip_op_prompt_gemm_q4_0.argtypes = [vp, i32, i32, vp, i32, vp, vp, i32, i32, vp, cp, sz]
    L.llamahip_op_attention.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, cp, sz]
    L.llamahip_op_attention_rows.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, i32, vp, cp, sz]
    L.llamahip_op_set_attention.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, i32, vp, C.c_uint32, cp, sz]
    L.llamahip_op_set_entry.argtypes = [i32, vp, i32, i32, vp, vp, i32, vp, C.c_uint32, i32, vp, i32, vp, vp, vp, vp, cp, sz]
    L.llamahip_op_set_exit.argtypes = [i32, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, cp, sz]
    L.llamahip_debug_set_keys.argtypes = [i32, i32]
    L.llamahip_debug_set_keys.restype = i32
    L.llamahip_op_dec_attention.argtypes = [vp, i32, vp, vp, vp, C.c_uint32, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, vp, cp, sz]
    L.llamahip_debug_dec_attn_plan.argtypes = [i32, i32, i32, i32, i32, i32, i32, vp, vp, cp, sz]
    L.llamahip_debug_dec_attn_plan.restype = i32
    L.llamahip_debug_qkv_attn_plan.argtypes = [i32, i32, i32, i32, i32, vp, cp, sz]
    L.llamahip_debug_qkv_attn_plan.restype = i32
    L.llamahip_op_qkv_attn.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, C.c_uint32, i32, vp, vp, vp, vp, cp, sz]
    L.llamahip_eval_multi.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, C.POINTER(_EvalMultiStats), cp, sz]
    L.llamahip_eval_multi_rows.argtypes = [i32, i32, vp, vp, i32, vp, vp, vp]
    L.llamahip_eval_multi_rows.restype = i32
    L.llamahip_eval_logprobs_multi.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, C.POINTER(_ScoreMultiStats), cp, sz]
    L.llamahip_score_choices.argtypes = [vp, i32, vp, i32, i32, vp, vp, i32, vp, vp, vp, cp, sz]
    L.llamahip_sched_new.argtypes = [vp, C.POINTER(_SchedOpts), C.POINTER(vp), cp, sz]
    L.llamahip_sched_submit.argtypes = [vp, C.POINTER(_Request), C.POINTER(C.c_int64), cp, sz]
    L.llamahip_sched_step.argtypes = [vp, vp, i32, C.POINTER(i32), cp, sz]
    L.llamahip_sched_cancel.argtypes = [vp, C.c_int64]
    L.llamahip_sched_pending.argtypes = [vp]
    L.llamahip_sched_pending.restype = i32
    L.llamahip_sched_get_stats.argtypes = [vp, vp]          # (size-versioned: _SchedStats or _SchedStatsPrefix)
    L.llamahip_sched_free.argtypes = [vp]
    L.llamahip_sched_free.restype = None
    L.llamahip_sched_plan.argtypes = [i32, vp, i32, i32, vp]
    L.llamahip_sched_plan.restype = i32
    L.llamahip_op_sched_pick.argtypes = [vp, i32, i32, vp, vp, cp, sz]
    L.llamahip_sched_plan_drafts.argtypes = [i32, vp, vp, vp, vp]
    L.llamahip_sched_plan_drafts.restype = i32
    L.llamahip_op_sched_accept.argtypes = [vp, i32, i32, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, cp, sz]
    L.llamahip_sched_plan_prefix.argtypes = [i32, vp, vp, vp, vp, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.llamahip_sched_plan_prefix.restype = i32
    L.llamahip_kv_copy_rows.argtypes = [vp, i32, vp, vp, vp, vp, cp, sz]
    L.llamahip_bench_kv_copy.argtypes = [vp, i32, vp, vp, vp, vp, i32, i32, C.POINTER(C.c_double), cp, sz]
    L.llamahip_kv_shift_rows.argtypes = [vp, i32, vp, vp, vp, vp, cp, sz]
    L.llamahip_bench_kv_shift.argtypes = [vp, i32, vp, vp, vp, vp, i32, C.POINTER(C.c_double), cp, sz]
    L.llamahip_op_kv_shift.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, cp, sz]
    L.llamahip_debug_rope_table.argtypes = [i32, i32, vp]
    L.llamahip_debug_rope_table.restype = i32
    L.llamahip_cur_seq.argtypes = [vp]
    L.llamahip_cur_seq.restype = i32
    L.llamahip_debug_attn_path.argtypes = [i32, i32, i32, i32, i32]
    L.llamahip_debug_attn_path.restype = i32
    L.llamahip_op_topk.argtypes = [vp, i32, vp, i32, C.c_double, i32, C.c_double, vp, vp, vp, cp, sz]
    L.llamahip_op_topk_rows.argtypes = [vp, i32, i32, vp, vp, C.c_double, i32, C.c_double, vp, vp, vp, vp, cp, sz]
    L.llamahip_op_logprob.argtypes = [vp, i32, i32, vp, vp, vp, vp, cp, sz]
    L.llamahip_op_top_logprobs.argtypes = [vp, i32, i32, i32, vp, vp, cp, sz]
    L.llamahip_eval_top_logprobs.argtypes = [vp, i32, i32, vp, i32, i32, i32, vp, vp, vp, cp, sz]
    L.llamahip_beam_search.argtypes = [vp, C.POINTER(_BeamOpts), vp, i32, vp, vp, C.POINTER(i32), C.POINTER(_BeamStats), cp, sz]
    L.llamahip_beam_select.argtypes = [i32, vp, i32, vp, vp, i32, i32, vp, vp, vp, C.POINTER(i32), vp, vp, C.POINTER(i32), C.POINTER(i32)]
    L.llamahip_beam_select.restype = i32
    L.llamahip_beam_slots.argtypes = [i32, vp, i32, vp, i32, vp, vp, vp]
    L.llamahip_beam_slots.restype = i32
    L.llamahip_text_embedding.argtypes = [vp, i32, i32, vp, i32, i32, i32, i32, vp, cp, sz]
    L.llamahip_text_embedding_multi.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, i32, i32, vp, C.POINTER(_EvalMultiStats), cp, sz]
    L.llamahip_op_pool_rows.argtypes = [vp, i32, i32, vp, vp, i32, i32, i32, vp, cp, sz]
    L.llamahip_op_prep.argtypes = [i32, i32, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, i32, i32, vp, vp, i32, vp, vp, cp, sz]
    L.llamahip_debug_qa_to_blocks.argtypes = [vp, vp, i32, i32, vp]
    L.llamahip_op_embed.argtypes = [vp, i32, vp, i32, i32, vp, i32, vp, cp, sz]
    L.llamahip_op_dense_prep.argtypes = [i32, i32, i32, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, i32, i32, vp, vp, cp, sz]
    L.llamahip_op_embed_dense.argtypes = [vp, i32, vp, i32, i32, i32, vp, i32, cp, sz]
    L.llamahip_op_gemv_q4_0.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, C.c_int64, vp, vp, i32, vp, i32, i32, vp, cp, sz]
    L.llamahip_op_gemv_set_q4_0.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, cp, sz]
    L.llamahip_bench_gemv.argtypes = [vp, i32, i32, i32, i32, C.POINTER(_GemvBench), cp, sz]
    L.llamahip_get_stats.argtypes = [vp, C.POINTER(_Stats)]
    L.llamahip_debug_lut_math.restype = i32
    L.llamahip_debug_gemm_paths.argtypes = [vp, i32]
    L.llamahip_debug_gemm_paths.restype = i32
    L.llamahip_op_mul_mat_dense.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp, i32, i32, vp, cp, sz]
    L.llamahip_debug_dense_paths.argtypes = [vp, i32]
    L.llamahip_debug_dense_paths.restype = i32
    L.llamahip_debug_dense_set_plan.argtypes = [i32, i32, i32, i32, vp]
    L.llamahip_debug_dense_set_plan.restype = i32
    L.llamahip_debug_dense_mfma_plan.argtypes = [i32, i32, i32, i32, vp]
    L.llamahip_debug_dense_mfma_plan.restype = i32
    L.llamahip_debug_dense_mfma_launches.argtypes = []
    L.llamahip_debug_dense_mfma_launches.restype = C.c_int64
    L.llamahip_debug_dense_force.argtypes = [i32]
    L.llamahip_op_mul_mat_q4_1.argtypes = [vp, i32, i32, vp, i32, vp, vp, i32, i32, vp, cp, sz]
    L.llamahip_debug_q41_paths.argtypes = [vp, i32]
    L.llamahip_debug_q41_paths.restype = i32
    L.llamahip_debug_q41_plan.argtypes = [i32, i32, i32, vp]
    L.llamahip_debug_q41_plan.restype = i32
    L.llamahip_debug_dense_force.restype = i32
    L.llamahip_constraint_new.argtypes = [vp, i32, vp, vp, i32, i32, C.POINTER(vp), cp, sz]
    L.llamahip_constraint_new_choices.argtypes = [vp, vp, vp, i32, i32, C.POINTER(vp), cp, sz]
    L.llamahip_constraint_free.argtypes = [vp]
    L.llamahip_constraint_free.restype = None
    for name in ("n_states", "start", "done"):
        getattr(L, "llamahip_constraint_" + name).argtypes = [vp]
        getattr(L, "llamahip_constraint_" + name).restype = i32
    L.llamahip_constraint_table.argtypes = [vp, vp, C.c_int64]
    L.llamahip_constraint_table.restype = C.c_int64
    L.llamahip_constraint_advance.argtypes = [vp, i32, i32]
    L.llamahip_constraint_advance.restype = i32
    L.llamahip_constraint_pick.argtypes = [vp, i32, vp]
    L.llamahip_constraint_pick.restype = i32
    L.llamahip_forced_run.argtypes = [vp, i32, vp, i32]
    L.llamahip_forced_run.restype = i32
    L.llamahip_op_verify_rows_allow.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, vp, cp, sz]
    L.llamahip_op_sched_pick_allow.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, cp, sz]
    L.llamahip_constraint_mask_row.argtypes = [vp, i32, vp, vp]
    L.llamahip_decode_greedy_constrained.argtypes = [vp, i32, i32, i32, i32, vp, C.POINTER(i32), vp, C.POINTER(i32), C.POINTER(i32), vp, cp, sz]
    L.llamahip_decode_greedy_constrained_multi.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, cp, sz]
    L.llamahip_eval_topk_constrained.argtypes = [vp, i32, i32, vp, i32, vp, i32, C.c_double, i32, C.c_double, vp, i32, vp, vp, C.POINTER(i32), vp, cp, sz]
    L.llamahip_op_pick_dfa.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, vp, cp, sz]
    L.llamahip_op_mask_rows_dfa.argtypes = [vp, i32, i32, vp, i32, vp, vp, cp, sz]
    L.llamahip_debug_live_allocs.argtypes = [vp, vp]
    L.llamahip_debug_live_allocs.restype = None
    _lib = L
    return L


def set_plan(m: int, k: int, n_rows: int, epi: int, interleaved: bool = False):
    """Host-only: the few-row kernel's plan (nc, cw, ncg, rgw, lds_bytes) for n_rows against an m x k matrix, or None (llamahip_debug_set_plan)."""
    a = np.zeros(5, np.int64)
    f = lib().llamahip_debug_set_plan
    f.restype = C.c_int32
    f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    return tuple(int(x) for x in a) if f(m, k, int(interleaved), n_rows, epi, a.ctypes.data_as(C.c_void_p)) else None


def gemv_plan(m: int, k: int, pre: int, epi: int, interleaved: bool = False):
    """Host-only: the single-row decode mat-vec's launch plan (nw, pg, depth, ring, grid, lds_bytes) for an m x k matrix under a
    (prologue, epilogue) pair, or None where the kernel does not take it (llamahip_debug_gemv_plan); a plan that names an instance
    that does not exist is an error."""
    a = np.zeros(6, np.int64)
    f = lib().llamahip_debug_gemv_plan
    f.restype = C.c_int32
    f.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    rc = f(m, k, int(interleaved), pre, epi, a.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise LlamaHipError(rc, f"gemv_plan({m}, {k}, pre={pre}, epi={epi}): the plan {a.tolist()} names a kernel instance that does not exist")
    return tuple(int(x) for x in a) if rc else None


def gemm_paths() -> dict:
    """Launch counts of the multi-row mat-mul kernel families since process start (llamahip_debug_gemm_paths)."""
    a = np.zeros(8, np.int64)
    n = lib().llamahip_debug_gemm_paths(a.ctypes.data_as(C.c_void_p), 8)
    return dict(zip(("mfma", "rows", "lds", "gemv", "set", "fast"), a[:n].tolist()))


def dense_paths() -> dict:
    """Launch counts of the f16 / f32 mat-mul kernels since process start (llamahip_debug_dense_paths)."""
    a = np.zeros(4, np.int64)
    n = lib().llamahip_debug_dense_paths(a.ctypes.data_as(C.c_void_p), 4)
    return dict(zip(("mv", "mm", "set"), a[:n].tolist()))


def dense_set_plan(m: int, k: int, wtype: int, n_rows: int):
    """Host-only: the launch plan of the few-row f16 / f32 mat-mul k_dense_set (llamahip_debug_dense_set_plan) for n_rows rows against an
    m x k matrix of wtype (0 fp32, 1 fp16): a dict, or None where the kernel does not take the shape; a plan that names an instance that
    does not exist is an error."""
    a = np.zeros(6, np.int64)
    rc = lib().llamahip_debug_dense_set_plan(m, k, wtype, n_rows, a.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise LlamaHipError(rc, f"dense_set_plan({m}, {k}, wtype={wtype}, n_rows={n_rows}): the plan {a.tolist()} names a kernel instance that does not exist")
    return dict(zip(("grid", "threads", "rows_per_half_wave", "rows", "slab_groups", "lds_bytes"), (int(x) for x in a))) if rc else None


def q41_paths() -> dict:
    """Q4_1 mat-muls per kernel since process start (llamahip_debug_q41_paths): chain = k_q41_chain, lane = k_q41_mm."""
    a = np.zeros(4, np.int64)
    n = lib().llamahip_debug_q41_paths(a.ctypes.data_as(C.c_void_p), 4)
    return dict(zip(("chain", "lane"), a[:n].tolist()))


def q41_plan(m: int, k: int, n_rows: int):
    """Host-only: the launch plan of the Q4_1 mat-mul k_q41_chain (llamahip_debug_q41_plan) for n_rows rows against an m x k matrix: a dict,
    or None where the kernel does not take the shape; a plan that names an instance that does not exist is an error.  For n_rows > 16 the
    plan is that of the full tiles of 16; a last tile of n_rows % 16 rows runs on q41_plan(m, k, n_rows % 16)."""
    a = np.zeros(8, np.int64)
    rc = lib().llamahip_debug_q41_plan(m, k, n_rows, a.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise LlamaHipError(rc, f"q41_plan({m}, {k}, n_rows={n_rows}): the plan {a.tolist()} names a kernel instance that does not exist")
    names = ("rows", "rows_per_workgroup", "threads", "grid_x", "grid_y", "slab_pairs", "lds_bytes", "chain_lanes")
    return dict(zip(names, (int(x) for x in a))) if rc else None


def dense_mfma_plan(m: int, k: int, wtype: int, n_rows: int):
    """Host-only: the launch plan of the matrix-core f16 / f32 mat-mul k_dense_mfma (llamahip_debug_dense_mfma_plan) for n_rows rows against
    an m x k matrix of wtype (0 fp32, 1 fp16): a dict, or None where the kernel does not take the shape; a plan that names an instance that
    does not exist is an error."""
    a = np.zeros(6, np.int64)
    rc = lib().llamahip_debug_dense_mfma_plan(m, k, wtype, n_rows, a.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise LlamaHipError(rc, f"dense_mfma_plan({m}, {k}, wtype={wtype}, n_rows={n_rows}): the plan {a.tolist()} names a kernel instance that does not exist")
    return dict(zip(("grid", "threads", "tile_rows", "tile_cols", "lds_bytes", "auto"), (int(x) for x in a))) if rc else None


def dense_mfma_launches() -> int:
    """Launches of k_dense_mfma since process start (llamahip_debug_dense_mfma_launches)."""
    return int(lib().llamahip_debug_dense_mfma_launches())


def dense_force(path=0) -> str:
    """Process-wide: send every f16 / f32 mat-mul of more than 16 rows of a model handle to "mm" or "mfma" (where the kernel takes the shape);
    0 / "auto": the measured rule again (llamahip_debug_dense_force).  Returns the previous setting as a name of DENSE_PATHS."""
    code = DENSE_PATHS.index(path) if path in DENSE_PATHS else int(path)
    prev = lib().llamahip_debug_dense_force(code)
    if prev < 0:
        raise ValueError(f"dense_force({path!r}): 0 / 'auto', 'mm' or 'mfma'")
    return DENSE_PATHS[prev]


def live_allocs() -> tuple:
    """(allocations, bytes) of device / pinned memory the library holds right now, process-wide (llamahip_debug_live_allocs): its own exact
    count, so a leak check compares it before a handle's load and after its free."""
    n, b = C.c_int64(0), C.c_int64(0)
    lib().llamahip_debug_live_allocs(C.byref(n), C.byref(b))
    return int(n.value), int(b.value)


def version() -> str:
    return lib().llamahip_version().decode()


def declared_symbols() -> list[str]:
    """Every function name declared in include/*.h (used by the CPU-side ABI test)."""
    names: list[str] = []
    for h in sorted(os.listdir(INCLUDE)):
        if not h.endswith(".h"):
            continue
        text = open(os.path.join(INCLUDE, h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names += re.findall(r"\b(llamahip_[a-z0-9_]+|llama_runner_[a-z0-9_]+)\s*\(", text)
    seen, out = set(), []
    for n in names:
        if n not in seen and n not in ("llamahip_opts", "llamahip_model", "llamahip_sampler", "llamahip_stats", "llamahip_gemv_bench"):
            seen.add(n)
            out.append(n)
    return out


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(rc: int, err) -> None:
    if rc != 0:
        raise LlamaHipError(rc, err.value.decode(errors="replace"))


def quantize_file(fname_inp: str, fname_out: str, itype: int = 2) -> None:
    """f32 / f16 model file -> Q4_0 model file (replaces llama_model_quantize, quantize.cpp:32-286)."""
    err = C.create_string_buffer(1024)
    _check(lib().llamahip_quantize_file(fname_inp.encode(), fname_out.encode(), itype, err, len(err)), err)


class Model:
    """Opaque model handle (llama_model + gpt_vocab of the reference, .mm:71-88, utils.h:49-55)."""

    def __init__(self, path: str, n_ctx: int = 512, device: int = -1, layer_begin: int = 0,
                 layer_end: int = -1, n_parts: int = 0, flags: int = 0, n_seq: int = 1, devices=None):
        """devices: a list of HIP device ordinals = an in-process layer pipeline, one stage per entry (include/llamahip.h);
        the same entry points work on it (eval, eval_chunks, eval_topk, decode_greedy, kv, stats)."""
        L = lib()
        err = C.create_string_buffer(1024)
        h = C.c_void_p()
        devices = list(devices or [])
        if len(devices) > 8:
            raise ValueError("at most 8 pipeline stages")
        opts = _Opts(C.sizeof(_Opts), device, layer_begin, layer_end, n_parts, flags, n_seq, len(devices), (C.c_int32 * 8)(*devices))
        self.layer_begin, self.n_seq = layer_begin, n_seq
        rc = L.llamahip_model_load(path.encode(), n_ctx, C.byref(opts), C.byref(h), err, len(err))
        _check(rc, err)
        self._h = h
        self.path = path
        self.n_vocab = L.llamahip_n_vocab(h)
        self.n_ctx = L.llamahip_n_ctx(h)
        self.n_embd = L.llamahip_n_embd(h)
        self.n_head = L.llamahip_n_head(h)
        self.n_layer = L.llamahip_n_layer(h)
        self.n_ff = L.llamahip_n_ff(h)
        self.n_parts = L.llamahip_n_parts(h)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().llamahip_model_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # --- llama_eval ---------------------------------------------------------------------------
    def eval(self, tokens, n_past: int, n_threads: int = 8) -> np.ndarray:
        tokens = np.ascontiguousarray(tokens, np.int32)
        logits = np.empty(self.n_vocab, np.float32)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_eval(self._h, n_threads, n_past, _ptr(tokens), tokens.size, _ptr(logits), err, len(err))
        _check(rc, err)
        return logits

    def eval_chunks(self, tokens, n_past: int, chunk_tokens: int = 9, n_threads: int = 8) -> np.ndarray:
        """The reference's prompt loop (successive llama_eval calls of `chunk_tokens` tokens, .mm:880-888) in one pass, bit for bit."""
        tokens = np.ascontiguousarray(tokens, np.int32)
        logits = np.empty(self.n_vocab, np.float32)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_eval_chunks(self._h, n_threads, n_past, _ptr(tokens), tokens.size, chunk_tokens, _ptr(logits), err, len(err))
        _check(rc, err)
        return logits

    def eval_logprobs(self, tokens, n_past: int, n_threads: int = 8, targets=None, chunk_tokens: int = 0) -> dict:
        """eval / eval_chunks (chunk_tokens 0 = one eval) + every row's next-token score, reduced on the device: logprob (float64; 0.0 for
        an unscored row), argmax, rank (logits strictly greater than the target's; -1 unscored), logits (the last row's).  targets: one id
        per row, -1 = not scored; None = the next token of every row but the last."""
        tokens = np.ascontiguousarray(tokens, np.int32)
        N = tokens.size
        if targets is not None:
            targets = np.ascontiguousarray(targets, np.int32)
            if targets.size != N:
                raise ValueError(f"targets: {targets.size} ids for {N} rows")
        lp, am, rk = np.empty(N, np.float64), np.empty(N, np.int32), np.empty(N, np.int32)
        last = np.empty(self.n_vocab, np.float32)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_eval_logprobs(self._h, n_threads, n_past, _ptr(tokens), N, chunk_tokens, _ptr(targets), _ptr(lp), _ptr(am), _ptr(rk),
                                          _ptr(last), err, len(err))
        _check(rc, err)
        return {"logprob": lp, "argmax": am, "rank": rk, "logits": last}

    def eval_top_logprobs(self, tokens, n_past: int, n_top: int, n_threads: int = 8, chunk_tokens: int = 0) -> dict:
        """llamahip_eval_top_logprobs: eval / eval_chunks (chunk_tokens 0 = one eval) + every row's n_top most probable tokens, reduced on the
        device: ids int32 [N, n_top] (value descending, the lower index first on ties), logprob float64 [N, n_top], logits (the last row's)."""
        tokens = np.ascontiguousarray(tokens, np.int32)
        N, n = tokens.size, max(int(n_top), 0)
        ids, lp = np.empty((N, n), np.int32), np.empty((N, n), np.float64)
        last = np.empty(self.n_vocab, np.float32)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_eval_top_logprobs(self._h, n_threads, n_past, _ptr(tokens), N, chunk_tokens, n_top, _ptr(ids), _ptr(lp), _ptr(last), err, len(err))
        _check(rc, err)
        return {"ids": ids, "logprob": lp, "logits": last}

    def beam_search(self, prompt, n_beams: int, n_predict: int, stop_token: int = -1, n_return: int = 0, length_norm: bool = False,
                    chunk_tokens: int = 0, n_threads: int = 8, with_stats: bool = False):
        """llamahip_beam_search: the best continuations of `prompt` searched over KV slots [0, n_beams) (include/llamahip.h states the contract).
        Returns a list of dicts, best first: tokens (int32 array), length, reason ("stop" / "length"), slot (-1 for a stop hypothesis),
        score (the summed log-probability, float64); with_stats: (that list, the llamahip_beam_stats counters as a dict)."""
        prompt = np.ascontiguousarray(prompt, np.int32)
        o = _BeamOpts(C.sizeof(_BeamOpts), n_threads, n_beams, n_predict, stop_token, n_return, int(length_norm), chunk_tokens)
        cap = max(n_return or n_beams, 1)
        hyps = (_BeamHyp * cap)()
        toks = np.full((cap, max(n_predict, 1)), -1, np.int32)
        n = C.c_int32(0)
        st = _BeamStats()
        st.struct_size = C.sizeof(_BeamStats)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_beam_search(self._h, C.byref(o), _ptr(prompt), prompt.size, C.cast(hyps, C.c_void_p), _ptr(toks), C.byref(n), C.byref(st), err, len(err))
        _check(rc, err)
        out = [{"tokens": toks[k, : hyps[k].length].copy(), "length": int(hyps[k].length), "reason": "stop" if hyps[k].reason == DONE_STOP else "length",
                "slot": int(hyps[k].slot), "score": float(hyps[k].score)} for k in range(n.value)]
        if not with_stats:
            return out
        return out, {f: int(getattr(st, f)) for f, _ in _BeamStats._fields_ if f.startswith("n_")}

    def perplexity(self, tokens, window: int = 0, score_from: int = -1, n_threads: int = 8, chunk_tokens: int = 0) -> dict:
        """Perplexity of a token stream over windows of `window` tokens (0 = n_ctx; the partial tail is unused), rows from score_from
        (-1 = window / 2) scored: ppl, nll_sum, n_scored, running (the ppl after each window).  Overwrites the KV cache."""
        tokens = np.ascontiguousarray(tokens, np.int32)
        w = window or self.n_ctx
        running = np.zeros(max(tokens.size // w, 1) if w > 0 else 1, np.float64)
        nll, n = C.c_double(0.0), C.c_int64(0)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_perplexity(self._h, n_threads, _ptr(tokens), tokens.size, window, score_from, chunk_tokens, C.byref(nll), C.byref(n),
                                       _ptr(running), err, len(err))
        _check(rc, err)
        return {"ppl": math.exp(nll.value / n.value), "nll_sum": nll.value, "n_scored": n.value, "running": running[: tokens.size // w]}

    def eval_debug(self, tokens, n_past: int, n_threads: int = 8, all_logits: bool = True, dump_layer: int = -1) -> dict:
        tokens = np.ascontiguousarray(tokens, np.int32)
        N = tokens.size
        last = np.empty(self.n_vocab, np.float32)
        allb = np.empty((N, self.n_vocab), np.float32) if all_logits else None
        dump = sizes = None
        cap = 0
        if dump_layer >= 0:
            T = n_past + N
            cap = N * (14 * self.n_embd + 3 * self.n_ff) + T * N * self.n_head + 1024
            dump = np.zeros(cap, np.float32)
            sizes = np.zeros(len(DUMP_NAMES), np.int64)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_eval_debug(self._h, n_threads, n_past, _ptr(tokens), N, _ptr(last), _ptr(allb),
                                       dump_layer, _ptr(dump), cap, _ptr(sizes), err, len(err))
        _check(rc, err)
        res = {"logits": last}
        if all_logits:
            res["logits_all"] = allb
        if dump is not None:
            off = 0
            for i, name in enumerate(DUMP_NAMES):
                n = int(sizes[i])
                res[name] = dump[off:off + n].copy()
                off += n
        return res

    def eval_topk(self, tokens, n_past: int, sampler: "Sampler", repeat_penalty: float = 1.3, top_k: int = 40,
                  temp: float = float(np.float32(0.8)), n_threads: int = 8):
        """llamahip_eval_topk: returns (exact, scores[k], ids[k], logits or None)."""
        tokens = np.ascontiguousarray(tokens, np.int32)
        win = np.zeros(1024, np.int32)
        nw = lib().llamahip_sampler_window(sampler._s, _ptr(win), 1024)
        sc, ids = np.zeros(64, np.float64), np.zeros(64, np.int32)
        exact = C.c_int32(0)
        logits = np.empty(self.n_vocab, np.float32)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_eval_topk(self._h, n_threads, n_past, _ptr(tokens), tokens.size, _ptr(win), nw, repeat_penalty, top_k, temp,
                                      _ptr(sc), _ptr(ids), C.byref(exact), _ptr(logits), err, len(err))
        _check(rc, err)
        k = min(top_k, self.n_vocab)
        return bool(exact.value), sc[:k], ids[:k], (None if exact.value else logits)

    def set_seq(self, seq: int) -> None:
        err = C.create_string_buffer(1024)
        _check(lib().llamahip_set_seq(self._h, seq, err, len(err)), err)

    def eval_stage(self, n_past: int, tokens=None, n_tokens: int = 0, hidden_in: int = 0, hidden_out: int = 0,
                   want_logits: bool = False, n_threads: int = 8):
        """Pipeline-stage eval.  hidden_in / hidden_out are DEVICE addresses (e.g. torch tensor
        .data_ptr()) of n_tokens * n_embd fp32; tokens is given on the first stage only."""
        tk = np.ascontiguousarray(tokens, np.int32) if tokens is not None else None
        N = tk.size if tk is not None else n_tokens
        logits = np.empty(self.n_vocab, np.float32) if want_logits else None
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_eval_stage(self._h, n_threads, n_past, _ptr(tk), N, C.c_void_p(hidden_in), C.c_void_p(hidden_out),
                                       _ptr(logits), err, len(err))
        _check(rc, err)
        return logits

    def stage_bind(self, seq: int, n_past: int, token_in: int = 0, hidden_in: int = 0, hidden_out: int = 0, token_out: int = 0):
        """Fix slot `seq`'s next position and its DEVICE i/o buffers (addresses) for stage_step."""
        err = C.create_string_buffer(1024)
        _check(lib().llamahip_stage_bind(self._h, seq, n_past, C.c_void_p(token_in), C.c_void_p(hidden_in), C.c_void_p(hidden_out),
                                         C.c_void_p(token_out), err, len(err)), err)

    def stage_mailbox(self, seq: int):
        """Create (once) slot `seq`'s device-side inboxes.  Returns (hidden_ptr, token_ptr, hidden_handle, token_handle): device
        addresses (0 where the stage has no such inbox) for same-process neighbours, 64-byte IPC handles (bytes) for other processes."""
        hp, tp = C.c_void_p(0), C.c_void_p(0)
        hh, th = C.create_string_buffer(64), C.create_string_buffer(64)
        err = C.create_string_buffer(1024)
        _check(lib().llamahip_stage_mailbox(self._h, seq, C.byref(hp), C.byref(tp), hh, th, err, len(err)), err)
        return (hp.value or 0), (tp.value or 0), (hh.raw if hp.value else None), (th.raw if tp.value else None)

    def stage_mailbox_connect(self, seq: int, next_hidden_handle: bytes = None, next_hidden_ptr: int = 0, token_handle: bytes = None, token_ptr: int = 0):
        """Give slot `seq` the next stage's hidden inbox and / or (last stage) the first stage's token inbox: an IPC handle (bytes) or a
        device address each."""
        err = C.create_string_buffer(1024)
        _check(lib().llamahip_stage_mailbox_connect(self._h, seq, next_hidden_handle, C.c_void_p(next_hidden_ptr or None),
                                                    token_handle, C.c_void_p(token_ptr or None), err, len(err)), err)

    def stage_step(self, seq: int, n_threads: int = 8, stream: int = 0):
        """Enqueue one token step of this stage on `stream` (hipStream_t address, 0 = the null stream); asynchronous."""
        err = C.create_string_buffer(256)
        _check(lib().llamahip_stage_step(self._h, seq, n_threads, C.c_void_p(stream), err, len(err)), err)

    def stage_set_applies(self, n_seqs: int, n_threads: int = 8) -> bool:
        """Whether stage_step_set can step n_seqs slots as one set on this handle (else: stage_step per slot)."""
        return bool(lib().llamahip_stage_set_applies(self._h, n_seqs, n_threads))

    def stage_step_set(self, seqs, n_threads: int = 8, stream: int = 0):
        """One decode step for all the slots in `seqs` at once (bit-identical to stepping them one by one; the weights are
        streamed once for the whole set); asynchronous like stage_step."""
        err = C.create_string_buffer(1024)
        sq = np.ascontiguousarray(seqs, dtype=np.int32)
        _check(lib().llamahip_stage_step_set(self._h, _ptr(sq), len(sq), n_threads, C.c_void_p(stream), err, len(err)), err)

    def stage_logits(self, row: int = 0) -> np.ndarray:
        """Row `row` of the logits of the most recent step (waits for the device)."""
        err = C.create_string_buffer(1024)
        out = np.empty(self.n_vocab, np.float32)
        _check(lib().llamahip_stage_logits(self._h, row, _ptr(out), err, len(err)), err)
        return out

    def stage_trace(self, seq: int, cap: int = 0):
        """Waits for the device.  Returns (steps taken since bind, current position, tokens picked [last stage])."""
        toks = np.zeros(max(cap, 1), np.int32)
        pos = C.c_int32(0)
        err = C.create_string_buffer(1024)
        n = lib().llamahip_stage_trace(self._h, seq, C.byref(pos), _ptr(toks), cap, err, len(err))
        _check(min(n, 0), err)
        return n, pos.value, toks[:min(n, cap)]

    def decode_greedy(self, first_token: int, n_past: int, n_steps: int, n_threads: int = 8, want_logits: bool = False):
        out = np.empty(n_steps, np.int32)
        logits = np.empty(self.n_vocab, np.float32) if want_logits else None
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_decode_greedy(self._h, n_threads, n_past, int(first_token), n_steps, _ptr(out), _ptr(logits), err, len(err))
        _check(rc, err)
        return (out, logits) if want_logits else out

    # --- constrained decoding (include/llamahip.h) ---------------------------------
    def constraint(self, dfa=None, choices=None, regex=None, stop_token: int = 2) -> "Constraint":
        """One of: dfa = (trans int32[n_states, 256] with -1 = dead, accept[n_states], start) -- a byte automaton; choices = byte strings (or
        str, taken as UTF-8) -- "answer with one of these"; regex = a pattern for regex_dfa.compile (full-match semantics).  stop_token ends
        an answer: it is allowed exactly where the text so far is accepted."""
        if (dfa is not None) + (choices is not None) + (regex is not None) != 1:
            raise ValueError("constraint: exactly one of dfa=, choices=, regex=")
        if regex is not None:
            from . import regex_dfa
            dfa = regex_dfa.compile(regex)
        return Constraint(self, dfa=dfa, choices=choices, stop_token=stop_token)

    def decode_greedy_constrained(self, first_token: int, n_past: int, n_steps: int, constraint: "Constraint", state: int | None = None,
                                  n_threads: int = 8, want_logits: bool = False) -> dict:
        """llamahip_decode_greedy_constrained: tokens (up to and including the stop token), finished, state (behind the last reported token:
        pass it back to resume) and with want_logits the logits the last reported token was picked from."""
        out = np.full(max(n_steps, 1), -1, np.int32)
        logits = np.empty(self.n_vocab, np.float32) if want_logits else None
        st = C.c_int32(constraint.start if state is None else int(state))
        n_out, fin = C.c_int32(0), C.c_int32(0)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_decode_greedy_constrained(self._h, n_threads, n_past, int(first_token), n_steps, constraint._c, C.byref(st), _ptr(out),
                                                      C.byref(n_out), C.byref(fin), _ptr(logits), err, len(err))
        _check(rc, err)
        return {"tokens": out[:n_out.value].copy(), "finished": bool(fin.value), "state": st.value, "logits": logits}

    def decode_greedy_constrained_multi(self, first_tokens, n_past, n_steps: int, constraints, states=None, n_threads: int = 8) -> list:
        """llamahip_decode_greedy_constrained_multi: sequence i in KV slot i under constraints[i] from states[i] (default: each start state).
        Returns one dict per sequence: tokens (up to and including the stop token), finished, state."""
        first_tokens = np.ascontiguousarray(first_tokens, np.int32).ravel()
        n_past = np.ascontiguousarray(n_past, np.int32).ravel()
        n = first_tokens.size
        if n_past.size != n or len(constraints) != n:
            raise ValueError(f"{n} first tokens, {n_past.size} positions, {len(constraints)} constraints")
        st = np.array([c.start for c in constraints] if states is None else states, np.int32).ravel()
        if st.size != n:
            raise ValueError(f"states: {st.size} for {n} sequences")
        cs = (C.c_void_p * max(n, 1))(*[c._c.value for c in constraints])
        out = np.full((max(n, 1), max(n_steps, 1)), -1, np.int32)
        n_out, fin = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_decode_greedy_constrained_multi(self._h, n_threads, n, _ptr(n_past), _ptr(first_tokens), n_steps, cs, _ptr(st), _ptr(out),
                                                            _ptr(n_out), _ptr(fin), err, len(err))
        _check(rc, err)
        return [{"tokens": out[i, :n_out[i]].copy(), "finished": bool(fin[i]), "state": int(st[i])} for i in range(n)]

    def eval_topk_constrained(self, tokens, n_past: int, sampler: "Sampler", constraint: "Constraint", state: int, repeat_penalty: float = 1.3,
                              top_k: int = 40, temp: float = float(np.float32(0.8)), n_threads: int = 8):
        """llamahip_eval_topk_constrained: (exact, scores[k], ids[k], masked logits or None) -- eval_topk's results for the row masked by
        the constraint's state."""
        tokens = np.ascontiguousarray(tokens, np.int32)
        win = np.zeros(1024, np.int32)
        nw = lib().llamahip_sampler_window(sampler._s, _ptr(win), 1024)
        sc, ids = np.zeros(64, np.float64), np.zeros(64, np.int32)
        exact = C.c_int32(0)
        logits = np.empty(self.n_vocab, np.float32)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_eval_topk_constrained(self._h, n_threads, n_past, _ptr(tokens), tokens.size, _ptr(win), nw, repeat_penalty, top_k, temp,
                                                  constraint._c, int(state), _ptr(sc), _ptr(ids), C.byref(exact), _ptr(logits), err, len(err))
        _check(rc, err)
        k = min(top_k, self.n_vocab)
        return bool(exact.value), sc[:k], ids[:k], (None if exact.value else logits)

    def decode_sample_constrained(self, first_token: int, n_past: int, n_steps: int, constraint: "Constraint", sampler: "Sampler", state: int | None = None,
                                  repeat_penalty: float = 1.3, top_k: int = 40, top_p: float = float(np.float32(0.95)),
                                  temp: float = float(np.float32(0.8)), n_threads: int = 8) -> dict:
        """Sampled decoding under a constraint: eval_topk_constrained -> draw -> accept -> advance, until the stop token or n_steps.  Token
        for token, and in the sampler's window and rng state, the loop eval -> Constraint.mask_row -> Sampler.sample -> accept.  Returns
        tokens, finished, state and n_exact (the steps whose candidates came from the device)."""
        state = constraint.start if state is None else int(state)
        tok, out, n_exact = int(first_token), [], 0
        while len(out) < n_steps and state != constraint.done:
            exact, sc, ids, masked = self.eval_topk_constrained([tok], n_past + len(out), sampler, constraint, state, repeat_penalty, top_k, temp, n_threads)
            tok = sampler.sample_from_candidates(sc, ids, top_p) if exact else sampler.sample(self, masked, repeat_penalty, top_k, top_p, temp)
            n_exact += int(exact)
            sampler.accept(tok)
            state = constraint.advance(state, tok)
            if state < 0:
                raise LlamaHipError(ERR_PREDICT, f"decode_sample_constrained: the sampler drew token {tok}, which the constraint bans")
            out.append(tok)
        return {"tokens": np.array(out, np.int32), "finished": state == constraint.done, "state": state, "n_exact": n_exact}

    def verify_greedy(self, token: int, draft, n_past: int, n_threads: int = 8, want_logits: bool = False):
        """llamahip_verify_greedy: the rows [token, draft ...] at n_past as one eval.  Returns (n_accept, picks[len(draft) + 1]) -- the new
        context is n_past + n_accept + 1, the next token picks[n_accept] -- and with want_logits the logits that token was picked from."""
        draft = np.ascontiguousarray(draft, np.int32).ravel()
        picks = np.full(draft.size + 1, -1, np.int32)
        n_acc = C.c_int32(-1)
        logits = np.empty(self.n_vocab, np.float32) if want_logits else None
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_verify_greedy(self._h, n_threads, n_past, int(token), _ptr(draft), draft.size, C.byref(n_acc), _ptr(picks), _ptr(logits), err, len(err))
        _check(rc, err)
        return (n_acc.value, picks, logits) if want_logits else (n_acc.value, picks)

    def decode_greedy_lookup(self, first_token: int, n_steps: int, n_past: int, context, corpus=None, draft_len: int = 0, ngram_min: int = 0,
                             ngram_max: int = 0, n_threads: int = 8, want_logits: bool = False):
        """llamahip_decode_greedy_lookup: decode_greedy's tokens, drafted from context (the n_past tokens already evaluated) + what is produced,
        then from corpus.  Returns (tokens[n_steps], stats dict) and with want_logits the last step's logits too."""
        context = np.ascontiguousarray(context, np.int32).ravel()
        corpus = None if corpus is None else np.ascontiguousarray(corpus, np.int32).ravel()
        out = np.empty(max(n_steps, 0), np.int32)
        logits = np.empty(self.n_vocab, np.float32) if want_logits else None
        st = _LookupStats(C.sizeof(_LookupStats))
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_decode_greedy_lookup(self._h, n_threads, n_past, int(first_token), n_steps, _ptr(context), context.size, _ptr(corpus),
                                                 0 if corpus is None else corpus.size, draft_len, ngram_min, ngram_max, _ptr(out), _ptr(logits),
                                                 C.byref(st), err, len(err))
        _check(rc, err)
        stats = {k: getattr(st, k) for k, _ in _LookupStats._fields_ if k != "struct_size"}
        return (out, stats, logits) if want_logits else (out, stats)

    def verify_sample(self, token: int, draft, n_past: int, sampler: "Sampler", repeat_penalty: float = 1.3, top_k: int = 40,
                      top_p: float = float(np.float32(0.95)), temp: float = float(np.float32(0.8)), n_threads: int = 8):
        """llamahip_verify_sample: the rows [token, draft ...] at n_past as one eval, walked by `sampler` (which has accepted `token`).  Returns
        (n_accept, picks[len(draft) + 1], exact[len(draft) + 1]); -1 in both for the rows the walk did not reach."""
        draft = np.ascontiguousarray(draft, np.int32).ravel()
        picks, exact = np.full(draft.size + 1, -2, np.int32), np.full(draft.size + 1, -2, np.int32)
        n_acc = C.c_int32(-1)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_verify_sample(self._h, n_threads, n_past, int(token), _ptr(draft), draft.size, None if sampler is None else sampler._s,
                                          repeat_penalty, top_k, top_p, temp, C.byref(n_acc), _ptr(picks), _ptr(exact), err, len(err))
        _check(rc, err)
        return n_acc.value, picks, exact

    def decode_sample_lookup(self, first_token: int, n_steps: int, n_past: int, context, sampler: "Sampler", corpus=None, draft_len: int = 0,
                             ngram_min: int = 0, ngram_max: int = 0, repeat_penalty: float = 1.3, top_k: int = 40,
                             top_p: float = float(np.float32(0.95)), temp: float = float(np.float32(0.8)), n_threads: int = 8, stats_size: int | None = None):
        """llamahip_decode_sample_lookup: the eval_topk -> draw -> accept loop's tokens, drafted from context (the n_past tokens already
        evaluated) + what is produced, then from corpus.  Returns (tokens[n_steps], exact[n_steps], stats dict)."""
        context = np.ascontiguousarray(context, np.int32).ravel()
        corpus = None if corpus is None else np.ascontiguousarray(corpus, np.int32).ravel()
        out, exact = np.empty(max(n_steps, 0), np.int32), np.empty(max(n_steps, 0), np.int32)
        st = _LookupStats(C.sizeof(_LookupStats) if stats_size is None else stats_size)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_decode_sample_lookup(self._h, n_threads, n_past, int(first_token), n_steps, _ptr(context), context.size, _ptr(corpus),
                                                 0 if corpus is None else corpus.size, draft_len, ngram_min, ngram_max,
                                                 None if sampler is None else sampler._s, repeat_penalty, top_k, top_p, temp, _ptr(out), _ptr(exact),
                                                 C.byref(st), err, len(err))
        _check(rc, err)
        return out, exact, {k: getattr(st, k) for k, _ in _LookupStats._fields_ if k != "struct_size"}

    def eval_multi(self, slots, n_past, token_lists, chunk_tokens: int = 0, n_threads: int = 8, want_stats: bool = False):
        """llamahip_eval_multi: token_lists[i] evaluated at n_past[i] on KV slot slots[i], all in one weight pass.  Returns the segments' last
        rows of logits [n_seqs][n_vocab] (with want_stats: (logits, the llamahip_eval_multi_stats fields as a dict))."""
        slots = np.ascontiguousarray(slots, np.int32).ravel()
        npast = np.ascontiguousarray(n_past, np.int32).ravel()
        toks = [np.ascontiguousarray(t, np.int32).ravel() for t in token_lists]
        if not (slots.size == npast.size == len(toks)):
            raise ValueError(f"eval_multi: {slots.size} slots, {npast.size} n_past, {len(toks)} token lists")
        nt = np.array([t.size for t in toks], np.int32)
        flat = np.ascontiguousarray(np.concatenate(toks), np.int32) if int(nt.sum()) else np.zeros(1, np.int32)
        logits = np.empty((max(slots.size, 1), self.n_vocab), np.float32)
        st = _EvalMultiStats(C.sizeof(_EvalMultiStats))
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_eval_multi(self._h, n_threads, slots.size, _ptr(slots), _ptr(npast), _ptr(flat), _ptr(nt), int(chunk_tokens),
                                       _ptr(logits), C.byref(st), err, len(err))
        _check(rc, err)
        logits = logits[:slots.size]
        return (logits, {k: getattr(st, k) for k, _ in _EvalMultiStats._fields_ if k != "struct_size"}) if want_stats else logits

    def text_embedding(self, tokens, n_past: int = 0, n_threads: int = 8, chunk_tokens: int = 0, pool="last", normalize: bool = False) -> np.ndarray:
        """llamahip_text_embedding: the text's embedding [n_embd] -- the final-norm hidden state of its last row (pool "last") or the mean over its
        rows (pool "mean"), optionally divided by its L2 length; the eval of llamahip_eval_chunks without the lm head, no logits written."""
        toks = np.ascontiguousarray(tokens, np.int32).ravel()
        out = np.empty(self.n_embd, np.float32)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_text_embedding(self._h, n_threads, int(n_past), _ptr(toks if toks.size else np.zeros(1, np.int32)), toks.size, int(chunk_tokens),
                                           _pool_id(pool), int(normalize), _ptr(out), err, len(err))
        _check(rc, err)
        return out

    def text_embedding_multi(self, slots, n_past, token_lists, chunk_tokens: int = 0, n_threads: int = 8, pool="last", normalize: bool = False,
                             want_stats: bool = False):
        """llamahip_text_embedding_multi: token_lists[i] evaluated at n_past[i] on KV slot slots[i], all in one weight pass; returns the texts'
        embeddings [n_seqs][n_embd] (with want_stats: (embeddings, the llamahip_eval_multi_stats fields as a dict))."""
        slots = np.ascontiguousarray(slots, np.int32).ravel()
        npast = np.ascontiguousarray(n_past, np.int32).ravel()
        toks = [np.ascontiguousarray(t, np.int32).ravel() for t in token_lists]
        if not (slots.size == npast.size == len(toks)):
            raise ValueError(f"text_embedding_multi: {slots.size} slots, {npast.size} n_past, {len(toks)} token lists")
        nt = np.array([t.size for t in toks], np.int32) if toks else np.zeros(1, np.int32)
        flat = np.ascontiguousarray(np.concatenate(toks), np.int32) if toks and int(nt.sum()) else np.zeros(1, np.int32)
        out = np.empty((max(slots.size, 1), self.n_embd), np.float32)
        st = _EvalMultiStats(C.sizeof(_EvalMultiStats))
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_text_embedding_multi(self._h, n_threads, slots.size, _ptr(slots), _ptr(npast), _ptr(flat), _ptr(nt), int(chunk_tokens),
                                                 _pool_id(pool), int(normalize), _ptr(out), C.byref(st), err, len(err))
        _check(rc, err)
        out = out[:slots.size]
        return (out, {k: getattr(st, k) for k, _ in _EvalMultiStats._fields_ if k != "struct_size"}) if want_stats else out

    def eval_logprobs_multi(self, slots, n_past, token_lists, targets=None, chunk_tokens: int = 0, n_threads: int = 8, want_stats: bool = False) -> dict:
        """llamahip_eval_logprobs_multi: token_lists[i] evaluated at n_past[i] on KV slot slots[i] and scored, all in one weight pass.  targets:
        one id per row over all segments (a flat array or one list per segment), -1 = not scored; None = the next token inside the row's
        segment.  Returns logprob / argmax / rank [R] in row order (an unscored row: 0.0 / -1 / -1) and seg_begin, the segments' first rows
        (with want_stats: + stats, the llamahip_score_multi_stats fields)."""
        slots = np.ascontiguousarray(slots, np.int32).ravel()
        npast = np.ascontiguousarray(n_past, np.int32).ravel()
        toks = [np.ascontiguousarray(t, np.int32).ravel() for t in token_lists]
        if not (slots.size == npast.size == len(toks)):
            raise ValueError(f"eval_logprobs_multi: {slots.size} slots, {npast.size} n_past, {len(toks)} token lists")
        nt = np.array([t.size for t in toks], np.int32)
        R = int(nt.sum())
        flat = np.ascontiguousarray(np.concatenate(toks), np.int32) if R else np.zeros(1, np.int32)
        if targets is not None:
            if len(targets) and not np.isscalar(targets[0]):
                targets = np.concatenate([np.ascontiguousarray(t, np.int32).ravel() for t in targets])
            targets = np.ascontiguousarray(targets, np.int32).ravel()
            if targets.size != R:
                raise ValueError(f"eval_logprobs_multi: {targets.size} targets for {R} rows")
            if not R:
                targets = np.zeros(1, np.int32)
        lp, am, rk = np.empty(max(R, 1), np.float64), np.empty(max(R, 1), np.int32), np.empty(max(R, 1), np.int32)
        st = _ScoreMultiStats(C.sizeof(_ScoreMultiStats))
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_eval_logprobs_multi(self._h, n_threads, slots.size, _ptr(slots), _ptr(npast), _ptr(flat), _ptr(nt), int(chunk_tokens),
                                                _ptr(targets), _ptr(lp), _ptr(am), _ptr(rk), C.byref(st), err, len(err))
        _check(rc, err)
        out = {"logprob": lp[:R], "argmax": am[:R], "rank": rk[:R], "seg_begin": [int(b) for b in np.cumsum(nt) - nt]}
        if want_stats:
            out["stats"] = {k: getattr(st, k) for k, _ in _ScoreMultiStats._fields_ if k != "struct_size"}
        return out

    def score_choices(self, context, endings, chunk_tokens: int = 0, n_threads: int = 8) -> dict:
        """llamahip_score_choices: one context, len(endings) endings on KV slots 0 .. len(endings) - 1 (overwritten) -- the context evaluated
        once, its rows copied to the other slots, the endings scored in one weight pass.  Returns logprob_sum [n] (float64), n_greedy [n]
        (rows whose target was the greedy pick) and rows, the per-ending arrays of log-probabilities."""
        ctx = np.ascontiguousarray(context, np.int32).ravel()
        ends = [np.ascontiguousarray(e, np.int32).ravel() for e in endings]
        ne = np.array([e.size for e in ends], np.int32) if ends else np.zeros(1, np.int32)
        E = int(ne.sum()) if ends else 0
        flat = np.ascontiguousarray(np.concatenate(ends), np.int32) if E else np.zeros(1, np.int32)
        sums, greedy = np.zeros(max(len(ends), 1), np.float64), np.zeros(max(len(ends), 1), np.int32)
        rows = np.zeros(max(E, 1), np.float64)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_score_choices(self._h, n_threads, _ptr(ctx) if ctx.size else None, ctx.size, len(ends), _ptr(flat), _ptr(ne), int(chunk_tokens),
                                          _ptr(sums), _ptr(greedy), _ptr(rows), err, len(err))
        _check(rc, err)
        at = np.cumsum(ne) - ne
        return {"logprob_sum": sums[:len(ends)], "n_greedy": greedy[:len(ends)], "rows": [rows[int(a):int(a) + int(n)].copy() for a, n in zip(at, ne)]}

    def decode_greedy_multi(self, first_tokens, n_past, n_steps: int, n_threads: int = 8) -> np.ndarray:
        """llamahip_decode_greedy_multi: sequences in KV slots 0 .. len(first_tokens) - 1 decoded together; returns [n_seqs][n_steps]."""
        ft = np.ascontiguousarray(first_tokens, np.int32)
        npast = np.ascontiguousarray(n_past, np.int32)
        out = np.empty((ft.size, n_steps), np.int32)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_decode_greedy_multi(self._h, n_threads, ft.size, _ptr(npast), _ptr(ft), n_steps, _ptr(out), err, len(err))
        _check(rc, err)
        return out

    def verify_greedy_multi(self, slots, tokens, drafts, n_past, n_threads: int = 8):
        """llamahip_verify_greedy_multi: one step whose rows are, per sequence i, [tokens[i], *drafts[i]] of KV slot slots[i] at n_past[i]
        (drafts: one sequence of ids per slot, empty allowed).  Returns (n_accept int32[n_seqs], picks: one int32 array per sequence)."""
        slots = np.ascontiguousarray(slots, np.int32).ravel()
        tokens = np.ascontiguousarray(tokens, np.int32).ravel()
        npast = np.ascontiguousarray(n_past, np.int32).ravel()
        drafts = [np.ascontiguousarray(d, np.int32).ravel() for d in drafts]
        if not (slots.size == tokens.size == npast.size == len(drafts)):
            raise ValueError(f"verify_greedy_multi: {slots.size} slots, {tokens.size} tokens, {npast.size} n_past, {len(drafts)} drafts")
        nd = np.array([d.size for d in drafts], np.int32)
        flat = np.concatenate(drafts).astype(np.int32) if int(nd.sum()) else np.zeros(1, np.int32)
        n_acc = np.full(slots.size, -1, np.int32)
        picks = np.full(int(nd.sum()) + slots.size, -1, np.int32)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_verify_greedy_multi(self._h, n_threads, slots.size, _ptr(slots), _ptr(npast), _ptr(tokens), _ptr(flat), _ptr(nd), _ptr(n_acc),
                                                _ptr(picks), err, len(err))
        _check(rc, err)
        cut = np.cumsum(nd + 1)[:-1]
        return n_acc, np.split(picks, cut)

    def decode_greedy_lookup_multi(self, first_tokens, n_past, n_steps: int, contexts, corpus=None, draft_len: int = 0, ngram_min: int = 0,
                                   ngram_max: int = 0, n_threads: int = 8, stats_size: int | None = None):
        """llamahip_decode_greedy_lookup_multi: sequences in KV slots 0 .. len(first_tokens) - 1 decoded together, the spare rows of every step
        carrying drafts (contexts: one sequence of n_past[i] ids per sequence).  Returns (tokens [n_seqs][n_steps], one stats dict per sequence)."""
        ft = np.ascontiguousarray(first_tokens, np.int32).ravel()
        npast = np.ascontiguousarray(n_past, np.int32).ravel()
        ctx = [np.ascontiguousarray(c, np.int32).ravel() for c in contexts]
        flat = np.concatenate(ctx).astype(np.int32) if sum(c.size for c in ctx) else None
        corpus = None if corpus is None else np.ascontiguousarray(corpus, np.int32).ravel()
        out = np.empty((ft.size, max(n_steps, 0)), np.int32)
        st = (_LookupStats * max(ft.size, 1))()
        for x in st:
            x.struct_size = C.sizeof(_LookupStats) if stats_size is None else stats_size
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_decode_greedy_lookup_multi(self._h, n_threads, ft.size, _ptr(npast), _ptr(ft), n_steps, _ptr(flat), _ptr(corpus),
                                                       0 if corpus is None else corpus.size, draft_len, ngram_min, ngram_max, _ptr(out),
                                                       C.cast(st, C.c_void_p), err, len(err))
        _check(rc, err)
        return out, [{k: getattr(x, k) for k, _ in _LookupStats._fields_ if k != "struct_size"} for x in st[:ft.size]]

    def decode_sample_multi(self, first_tokens, n_past, n_steps: int, samplers, repeat_penalty: float = 1.3, top_k: int = 40,
                            top_p: float = float(np.float32(0.95)), temp: float = float(np.float32(0.8)), n_threads: int = 8,
                            want_exact: bool = False):
        """llamahip_decode_sample_multi: sequence i (KV slot i) continues at n_past[i] with first_tokens[i] and draws with samplers[i] (one
        Sampler per sequence; every pick is accepted into it).  Returns [n_seqs][n_steps] int32, and with want_exact the [n_seqs][n_steps]
        flags too (1 = drawn from the device's candidates, 0 = from the full logits row on the host)."""
        ft = np.ascontiguousarray(first_tokens, np.int32)
        npast = np.ascontiguousarray(n_past, np.int32)
        if npast.size != ft.size or len(samplers) != ft.size:
            raise ValueError(f"{ft.size} first tokens, {npast.size} positions, {len(samplers)} samplers")
        sp = (C.c_void_p * max(ft.size, 1))(*[s._s.value if s is not None else None for s in samplers])
        out = np.empty((ft.size, n_steps), np.int32)
        exact = np.empty((ft.size, n_steps), np.int32) if want_exact else None
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_decode_sample_multi(self._h, n_threads, ft.size, _ptr(npast), _ptr(ft), n_steps, sp, repeat_penalty, top_k, top_p, temp,
                                                _ptr(out), _ptr(exact), err, len(err))
        _check(rc, err)
        return (out, exact) if want_exact else out

    def verify_sample_multi(self, slots, tokens, drafts, n_past, samplers, repeat_penalty: float = 1.3, top_k: int = 40,
                            top_p: float = float(np.float32(0.95)), temp: float = float(np.float32(0.8)), n_threads: int = 8):
        """llamahip_verify_sample_multi: one step whose rows are, per sequence i, [tokens[i], *drafts[i]] of KV slot slots[i] at n_past[i], walked
        by samplers[i] (which has accepted tokens[i]).  Returns (n_accept int32[n_seqs], picks, exact: one int32 array per sequence each; -1 in
        both for the rows a walk did not reach)."""
        slots = np.ascontiguousarray(slots, np.int32).ravel()
        tokens = np.ascontiguousarray(tokens, np.int32).ravel()
        npast = np.ascontiguousarray(n_past, np.int32).ravel()
        drafts = [np.ascontiguousarray(d, np.int32).ravel() for d in drafts]
        if not (slots.size == tokens.size == npast.size == len(drafts) == len(samplers)):
            raise ValueError(f"verify_sample_multi: {slots.size} slots, {tokens.size} tokens, {npast.size} n_past, {len(drafts)} drafts, {len(samplers)} samplers")
        nd = np.array([d.size for d in drafts], np.int32)
        flat = np.concatenate(drafts).astype(np.int32) if int(nd.sum()) else np.zeros(1, np.int32)
        sp = (C.c_void_p * max(slots.size, 1))(*[s._s.value if s is not None else None for s in samplers])
        n_acc = np.full(slots.size, -1, np.int32)
        picks, exact = np.full(int(nd.sum()) + slots.size, -2, np.int32), np.full(int(nd.sum()) + slots.size, -2, np.int32)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_verify_sample_multi(self._h, n_threads, slots.size, _ptr(slots), _ptr(npast), _ptr(tokens), _ptr(flat), _ptr(nd), sp,
                                                repeat_penalty, top_k, top_p, temp, _ptr(n_acc), _ptr(picks), _ptr(exact), err, len(err))
        _check(rc, err)
        cut = np.cumsum(nd + 1)[:-1]
        return n_acc, np.split(picks, cut), np.split(exact, cut)

    def decode_sample_lookup_multi(self, first_tokens, n_past, n_steps: int, contexts, samplers, corpus=None, draft_len: int = 0, ngram_min: int = 0,
                                   ngram_max: int = 0, repeat_penalty: float = 1.3, top_k: int = 40, top_p: float = float(np.float32(0.95)),
                                   temp: float = float(np.float32(0.8)), n_threads: int = 8, want_exact: bool = False, stats_size: int | None = None):
        """llamahip_decode_sample_lookup_multi: sequence i (KV slot i) continues at n_past[i] with first_tokens[i] and draws with samplers[i], the
        spare rows of every step carrying drafts (contexts: one sequence of n_past[i] ids per sequence).  Returns (tokens [n_seqs][n_steps],
        one stats dict per sequence), and with want_exact (tokens, exact [n_seqs][n_steps], stats)."""
        ft = np.ascontiguousarray(first_tokens, np.int32).ravel()
        npast = np.ascontiguousarray(n_past, np.int32).ravel()
        if len(samplers) != ft.size:
            raise ValueError(f"{ft.size} first tokens, {len(samplers)} samplers")
        ctx = [np.ascontiguousarray(c, np.int32).ravel() for c in contexts]
        flat = np.concatenate(ctx).astype(np.int32) if sum(c.size for c in ctx) else None
        corpus = None if corpus is None else np.ascontiguousarray(corpus, np.int32).ravel()
        sp = (C.c_void_p * max(ft.size, 1))(*[s._s.value if s is not None else None for s in samplers])
        out = np.empty((ft.size, max(n_steps, 0)), np.int32)
        exact = np.empty((ft.size, max(n_steps, 0)), np.int32) if want_exact else None
        st = (_LookupStats * max(ft.size, 1))()
        for x in st:
            x.struct_size = C.sizeof(_LookupStats) if stats_size is None else stats_size
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_decode_sample_lookup_multi(self._h, n_threads, ft.size, _ptr(npast), _ptr(ft), n_steps, _ptr(flat), _ptr(corpus),
                                                       0 if corpus is None else corpus.size, draft_len, ngram_min, ngram_max, sp, repeat_penalty, top_k,
                                                       top_p, temp, _ptr(out), _ptr(exact), C.cast(st, C.c_void_p), err, len(err))
        _check(rc, err)
        stats = [{k: getattr(x, k) for k, _ in _LookupStats._fields_ if k != "struct_size"} for x in st[:ft.size]]
        return (out, exact, stats) if want_exact else (out, stats)

    def decode_greedy_window(self, first_token: int, n_steps: int, n_past: int, context, n_keep: int = 0, mode: int = CTX_REEVAL,
                             chunk_tokens: int = 0, n_threads: int = 8, want_logits: bool = False):
        """llamahip_decode_greedy_window: decode_greedy in legs that never stop at n_ctx -- at the wall the first n_keep tokens stay, the older
        half of the rest is dropped (ctx_overflow_plan) and the tail is re-evaluated (CTX_REEVAL, exact; chunk_tokens 0 = one eval) or, with
        mode CTX_SHIFT, the surviving rows are moved down in place by kv_shift_rows (NOT the reference's arithmetic; chunk_tokens ignored).
        context: the n_past tokens already evaluated.  Returns (tokens[n_steps], n_past afterwards) and with
        want_logits the last step's logits too."""
        context = np.ascontiguousarray(context, np.int32).ravel()
        out = np.empty(max(n_steps, 0), np.int32)
        logits = np.empty(self.n_vocab, np.float32) if want_logits else None
        np_out = C.c_int32(-1)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_decode_greedy_window(self._h, n_threads, n_past, int(first_token), n_steps, _ptr(context), context.size, n_keep, mode,
                                                 chunk_tokens, _ptr(out), _ptr(logits), C.byref(np_out), err, len(err))
        _check(rc, err)
        return (out, np_out.value, logits) if want_logits else (out, np_out.value)

    def scheduler(self, max_active: int, chunk_tokens: int = 0, row_budget: int = 0, n_threads: int = 8, repeat_penalty: float = 1.3,
                  top_k: int = 40, top_p: float = float(np.float32(0.95)), temp: float = float(np.float32(0.8)), draft_len: int = 0,
                  ngram_min: int = 0, ngram_max: int = 0, corpus=None, prefix_share: bool = False, forced_drafts: bool = False) -> "Scheduler":
        """llamahip_sched_new: a request scheduler over KV slots [0, max_active) of this handle (include/llamahip.h "request scheduler").
        draft_len > 0: drafted tokens ride in the rows a step leaves spare (prompt lookup in each request's history, then `corpus`).
        prefix_share: a request takes over the evaluated prompt rows it has in common with a slot's record instead of evaluating them.
        forced_drafts: a constrained greedy request's forced tokens ride as its draft (works with draft_len 0)."""
        return Scheduler(self, max_active, chunk_tokens, row_budget, n_threads, repeat_penalty, top_k, top_p, temp, draft_len, ngram_min, ngram_max, corpus,
                         prefix_share, forced_drafts)

    def kv_copy_rows(self, copies) -> None:
        """llamahip_kv_copy_rows: copies = [(src slot, dst slot, first row, row count), ...], 1 .. 16 of them -- those KV rows of every layer, K
        and V, from the source slot to the same rows of the destination slot, in one launch per stage."""
        c = np.ascontiguousarray(copies, np.int32).reshape(-1, 4)
        cols = [np.ascontiguousarray(c[:, k]) for k in range(4)]
        err = C.create_string_buffer(1024)
        _check(lib().llamahip_kv_copy_rows(self._h, len(c), *(_ptr(a) for a in cols), err, len(err)), err)

    def kv_shift_rows(self, shifts) -> None:
        """llamahip_kv_shift_rows (NOT the reference's arithmetic): shifts = [(slot, first row, row count, n_discard), ...], 1 .. 16 of them --
        those KV rows of every layer move down by n_discard rows in place, the keys re-rotated by -n_discard positions, one launch per stage."""
        c = np.ascontiguousarray(shifts, np.int32).reshape(-1, 4)
        cols = [np.ascontiguousarray(c[:, k]) for k in range(4)]
        err = C.create_string_buffer(1024)
        _check(lib().llamahip_kv_shift_rows(self._h, len(c), *(_ptr(a) for a in cols), err, len(err)), err)

    @property
    def cur_seq(self) -> int:
        """llamahip_cur_seq: the handle's current KV slot"""
        return int(lib().llamahip_cur_seq(self._h))

    def kv(self, il: int, n_pos: int):
        k = np.empty((n_pos, self.n_embd), np.float32)
        v = np.empty((n_pos, self.n_embd), np.float32)
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_kv_read(self._h, il, n_pos, _ptr(k), _ptr(v), err, len(err))
        _check(rc, err)
        return k, v

    def tensor_bytes(self, name: str) -> np.ndarray:
        n = lib().llamahip_tensor_bytes(self._h, name.encode(), None, 0)
        if n < 0:
            raise KeyError(name)
        out = np.empty(n, np.uint8)
        if lib().llamahip_tensor_bytes(self._h, name.encode(), _ptr(out), n) != n:
            raise LlamaHipError(ERR_LOAD, f"failed to read tensor {name}")
        return out

    # --- vocab / text -------------------------------------------------------------------------
    def token_text(self, tid: int) -> bytes:
        ln = C.c_uint32(0)
        p = lib().llamahip_token_text(self._h, tid, C.byref(ln))
        if not p:
            raise IndexError(tid)
        return C.string_at(p, ln.value)

    def tokenize(self, text: str | bytes, bos: bool = True) -> np.ndarray:
        raw = text.encode() if isinstance(text, str) else text
        cap = len(raw) + 2
        out = np.empty(cap, np.int32)
        n = lib().llamahip_tokenize(self._h, raw, int(bos), _ptr(out), cap)
        return out[:n].copy()

    # --- measurement ----------------------------------------------------------------------------
    def bench_gemv(self, which: int, layer: int = 0, warmup: int = 5, iters: int = 50) -> dict:
        b = _GemvBench()
        err = C.create_string_buffer(1024)
        rc = lib().llamahip_bench_gemv(self._h, which, layer, warmup, iters, C.byref(b), err, len(err))
        _check(rc, err)
        us = b.ms_total * 1e3 / b.iters
        return {"name": bench_gemv_names[which], "M": b.M, "K": b.K, "iters": b.iters, "us_per_launch": us,
                "algo_bytes": b.algo_bytes, "GBps": b.algo_bytes / (us * 1e-6) / 1e9}

    def bench_kv_copy(self, copies, how: int, iters: int = 20) -> float:
        """llamahip_bench_kv_copy: milliseconds per enqueue + wait of `copies` (as kv_copy_rows takes them) -- how 0: one k_kv_copy_rows launch,
        1: a loop of hipMemcpyAsync calls over the same ranges on the same stream."""
        c = np.ascontiguousarray(copies, np.int32).reshape(-1, 4)
        cols = [np.ascontiguousarray(c[:, k]) for k in range(4)]
        ms = C.c_double(0)
        err = C.create_string_buffer(1024)
        _check(lib().llamahip_bench_kv_copy(self._h, len(c), *(_ptr(a) for a in cols), int(how), int(iters), C.byref(ms), err, len(err)), err)
        return float(ms.value)

    def bench_kv_shift(self, shifts, iters: int = 20) -> float:
        """llamahip_bench_kv_shift: milliseconds per k_kv_shift_rows launch of `shifts` (as kv_shift_rows takes them), event-timed over `iters`
        launches after one untimed launch."""
        c = np.ascontiguousarray(shifts, np.int32).reshape(-1, 4)
        cols = [np.ascontiguousarray(c[:, k]) for k in range(4)]
        ms = C.c_double(0)
        err = C.create_string_buffer(1024)
        _check(lib().llamahip_bench_kv_shift(self._h, len(c), *(_ptr(a) for a in cols), int(iters), C.byref(ms), err, len(err)), err)
        return float(ms.value)

    def stats(self) -> dict:
        s = _Stats()
        lib().llamahip_get_stats(self._h, C.byref(s))
        return {k: getattr(s, k) for k, _ in _Stats._fields_ if k != "struct_size"}


class Constraint:
    """A token-level constraint of one Model (llamahip_constraint_*): owns the handle's constraint -- close it (or leave the `with` block)
    before the model is closed."""

    def __init__(self, model: Model, dfa=None, choices=None, stop_token: int = 2):
        L = lib()
        err = C.create_string_buffer(1024)
        c = C.c_void_p()
        self._c = None
        self.model, self.stop_token = model, int(stop_token)
        if choices is not None:
            bs = [x.encode() if isinstance(x, str) else bytes(x) for x in choices]
            bufs = [C.create_string_buffer(b, max(len(b), 1)) for b in bs]
            ptrs = (C.c_void_p * max(len(bs), 1))(*[C.cast(b, C.c_void_p).value for b in bufs])
            lens = np.array([len(b) for b in bs], np.int32)
            rc = L.llamahip_constraint_new_choices(model._h, ptrs, _ptr(lens), len(bs), self.stop_token, C.byref(c), err, len(err))
        else:
            trans, accept, start = dfa
            trans = np.ascontiguousarray(trans, np.int32)
            if trans.ndim != 2 or trans.shape[1] != 256:
                raise ValueError("constraint: trans is int32 [n_states, 256]")
            accept = np.ascontiguousarray(accept, np.uint8).ravel()
            if accept.size != trans.shape[0]:
                raise ValueError(f"constraint: accept has {accept.size} entries for {trans.shape[0]} states")
            rc = L.llamahip_constraint_new(model._h, trans.shape[0], _ptr(trans), _ptr(accept), int(start), self.stop_token, C.byref(c), err, len(err))
        _check(rc, err)
        self._c = c
        self.n_states, self.start, self.done = L.llamahip_constraint_n_states(c), L.llamahip_constraint_start(c), L.llamahip_constraint_done(c)
        self.n_vocab = model.n_vocab

    def close(self) -> None:
        if getattr(self, "_c", None):
            lib().llamahip_constraint_free(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def table(self) -> np.ndarray:
        """uint16 [n_states, n_vocab]; 0xFFFF = banned"""
        out = np.empty((self.n_states, self.n_vocab), np.uint16)
        n = lib().llamahip_constraint_table(self._c, _ptr(out), out.size)
        assert n == out.size
        return out

    def advance(self, state: int, token: int) -> int:
        return lib().llamahip_constraint_advance(self._c, int(state), int(token))

    def pick(self, state: int, logits) -> int:
        logits = np.ascontiguousarray(logits, np.float32)
        if logits.size != self.n_vocab:
            raise ValueError(f"pick: {logits.size} logits for n_vocab {self.n_vocab}")
        return lib().llamahip_constraint_pick(self._c, int(state), _ptr(logits))

    def forced(self, state: int, cap: int = 15) -> np.ndarray:
        """llamahip_forced_run: the tokens forced from `state` on (each the single allowed token of its state), at most cap"""
        out = np.empty(max(int(cap), 1), np.int32)
        n = lib().llamahip_forced_run(self._c, int(state), _ptr(out) if cap > 0 else None, int(cap))
        if n < 0:
            raise LlamaHipError(ERR_PREDICT, f"llamahip_forced_run: state {state} out of range [0, {self.n_states}) or cap {cap} < 0")
        return out[:n].copy()

    def mask_row(self, state: int, logits) -> np.ndarray:
        logits = np.ascontiguousarray(logits, np.float32)
        if logits.size != self.n_vocab:
            raise ValueError(f"mask_row: {logits.size} logits for n_vocab {self.n_vocab}")
        out = np.empty_like(logits)
        if lib().llamahip_constraint_mask_row(self._c, int(state), _ptr(logits), _ptr(out)) != 0:
            raise LlamaHipError(ERR_PREDICT, f"llamahip_constraint_mask_row: state {state} out of range [0, {self.n_states})")
        return out


class Sampler:
    """mt19937 + last_n_tokens window (LlamaPredictOperation.mm:773, 827-829)."""

    def __init__(self, seed: int = -1, repeat_last_n: int = 64):
        self._s = C.c_void_p(lib().llamahip_sampler_new(seed, repeat_last_n))

    def accept(self, tid: int) -> None:
        lib().llamahip_sampler_accept(self._s, int(tid))

    def sample_from_candidates(self, scores, ids, top_p: float = float(np.float32(0.95))) -> int:
        scores, ids = np.ascontiguousarray(scores, np.float64), np.ascontiguousarray(ids, np.int32)
        return int(lib().llamahip_sample_from_candidates(self._s, _ptr(scores), _ptr(ids), len(ids), top_p))

    def window(self) -> np.ndarray:
        """the last_n_tokens window, oldest first (llamahip_sampler_window)"""
        n = lib().llamahip_sampler_window(self._s, None, 0)
        out = np.zeros(max(n, 1), np.int32)
        lib().llamahip_sampler_window(self._s, _ptr(out), n)
        return out[:n]

    def random_prompt(self) -> str:
        """gpt_random_prompt on this sampler's rng (utils.cpp:102-119; .mm:774-776)."""
        return lib().llamahip_sampler_random_prompt(self._s).decode()

    def sample(self, model: Model, logits: np.ndarray, repeat_penalty: float = 1.3, top_k: int = 40,
               top_p: float = float(np.float32(0.95)), temp: float = float(np.float32(0.8))) -> int:
        logits = np.ascontiguousarray(logits, np.float32)
        return int(lib().llamahip_sample_top_p_top_k(model._h, self._s, _ptr(logits), repeat_penalty, top_k, top_p, temp))

    def __del__(self):
        try:
            if self._s:
                lib().llamahip_sampler_free(self._s)
                self._s = None
        except Exception:
            pass


EV_TOKEN, EV_DONE = 1, 2
DONE_REASONS = {1: "length", 2: "stop", 3: "cancelled"}


class Scheduler:
    """llamahip_sched_*: requests wait in a queue, take a free KV slot, have their prompt evaluated inside the running decode's weight
    passes, decode, and leave at their stop token or their length.  A context manager; one step() = one weight pass."""

    def __init__(self, model: Model, max_active: int, chunk_tokens: int = 0, row_budget: int = 0, n_threads: int = 8,
                 repeat_penalty: float = 1.3, top_k: int = 40, top_p: float = float(np.float32(0.95)), temp: float = float(np.float32(0.8)),
                 draft_len: int = 0, ngram_min: int = 0, ngram_max: int = 0, corpus=None, prefix_share: bool = False, forced_drafts: bool = False):
        self._s = None
        self.model, self.max_active, self.draft_len = model, int(max_active), int(draft_len)
        self.forced_drafts = bool(forced_drafts)
        self._cap_len = max(self.draft_len, int(self.forced_drafts))          # (forced drafts need a drafting scheduler's event capacity)
        self._samplers = {}          # id -> Sampler: kept alive while the request may draw
        self._constraints = {}       # id -> Constraint: kept alive while the request lives
        c = np.ascontiguousarray(corpus if corpus is not None else [], np.int32).ravel()          # (copied by llamahip_sched_new)
        o = _SchedOptsForced(C.sizeof(_SchedOptsForced), n_threads, max_active, chunk_tokens, row_budget, repeat_penalty, top_p, temp, top_k,
                             int(draft_len), int(ngram_min), int(ngram_max), c.ctypes.data if c.size else None, c.size, int(prefix_share), int(forced_drafts))
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        _check(lib().llamahip_sched_new(model._h, C.byref(o), C.byref(h), err, len(err)), err)
        self._s = h
        self._ev = (_SchedEvent * (sched_event_cap(self.max_active, self._cap_len) + 63))()          # (room for waiting DONE events)

    def close(self) -> None:
        if self._s:
            lib().llamahip_sched_free(self._s)
            self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def submit(self, prompt, n_predict: int, stop_token: int = -1, sampler: "Sampler | None" = None, constraint: "Constraint | None" = None,
               constraint_state: int = -1) -> int:
        """llamahip_sched_submit: returns the request's id (sampler None = greedy; constraint: every pick under it, from constraint_state,
        -1 = its start; the scheduler keeps the Constraint alive while the request lives)."""
        p = np.ascontiguousarray(prompt, np.int32).ravel()
        r = _RequestCst(C.sizeof(_RequestCst), p.ctypes.data if p.size else None, p.size, int(n_predict), int(stop_token), None if sampler is None else sampler._s.value,
                        None if constraint is None else constraint._c.value, int(constraint_state))
        rid = C.c_int64(0)
        err = C.create_string_buffer(1024)
        _check(lib().llamahip_sched_submit(self._s, C.byref(r), C.byref(rid), err, len(err)), err)
        if sampler is not None:
            self._samplers[rid.value] = sampler
        if constraint is not None:
            self._constraints[rid.value] = constraint
        return int(rid.value)

    def step(self, cap: int | None = None) -> list[dict]:
        """llamahip_sched_step: one weight pass; the step's events as dicts {id, kind ("token" / "done"), token, exact, slot, position, reason}."""
        n = C.c_int32(0)
        err = C.create_string_buffer(1024)
        assert len(self._ev) >= sched_event_cap(self.max_active, self._cap_len)
        _check(lib().llamahip_sched_step(self._s, C.cast(self._ev, C.c_void_p), len(self._ev) if cap is None else int(cap), C.byref(n), err, len(err)), err)
        out = []
        for e in self._ev[:n.value]:
            done = e.kind == EV_DONE
            out.append({"id": int(e.id), "kind": "done" if done else "token", "token": int(e.token), "exact": int(e.exact), "slot": int(e.slot),
                        "position": int(e.position), "reason": DONE_REASONS.get(e.reason) if done else None})
            if done:
                self._samplers.pop(int(e.id), None)
                self._constraints.pop(int(e.id), None)
        return out

    def cancel(self, rid: int) -> bool:
        return lib().llamahip_sched_cancel(self._s, int(rid)) == 0

    def pending(self) -> int:
        return int(lib().llamahip_sched_pending(self._s))

    def stats(self) -> dict:
        st = _SchedStatsDfa(C.sizeof(_SchedStatsDfa))
        lib().llamahip_sched_get_stats(self._s, C.byref(st))
        return {k: int(getattr(st, k)) for k, _ in _SchedStats._fields_ + _SchedStatsPrefix._fields_ + _SchedStatsDfa._fields_ if k != "struct_size"}

    def run(self, on_done=None) -> dict:
        """step until nothing is pending; returns {id: tokens}.  on_done(event), if given, is called at each DONE event -- while the
        request's KV rows are still in its slot (the slot is reused from the next step)."""
        out: dict = {}
        while self.pending():
            for e in self.step():
                if e["kind"] == "token":
                    out.setdefault(e["id"], []).append(e["token"])
                else:
                    out.setdefault(e["id"], [])
                    if on_done is not None:
                        on_done(e)
        return out


def sched_event_cap(max_active: int, draft_len: int = 0) -> int:
    """LLAMAHIP_SCHED_EVENT_CAP: the smallest event capacity llamahip_sched_step takes."""
    return max_active + 17 if draft_len > 0 else 2 * max_active + 1


def sched_plan_drafts(prompt_left, rows, want):
    """llamahip_sched_plan_drafts (host only): (draft rows dealt, draft tokens per sequence) for sequences in admission order -- prompt_left and
    rows as llamahip_sched_plan takes and gives them, want[i] the draft tokens sequence i could use; -1 = bad arguments."""
    left, rows, want = (np.ascontiguousarray(a, np.int32).ravel() for a in (prompt_left, rows, want))
    if not left.size == rows.size == want.size:
        raise ValueError(f"sched_plan_drafts: {left.size} / {rows.size} / {want.size} entries")
    give = np.full(max(left.size, 1), -1, np.int32)
    n = lib().llamahip_sched_plan_drafts(left.size, *((_ptr(left), _ptr(rows), _ptr(want)) if left.size else (None, None, None)), _ptr(give))
    return int(n), give[:left.size]


def op_sched_accept(logits2d, seg_tab, tokens, state=None, log=None, next_tok=None):
    """k_verify_rows + k_sched_accept on host rows (llamahip_op_sched_accept): seg_tab [n_segs][6] = {emit, slot, base position, base cursor,
    first logits row, row count}, tokens [n_rows]; the slot words state [n_slots][2], log [n_slots][log_cap], next_tok [n_slots] -- all three
    or none -- are updated in place (int32, C-contiguous).  Returns (n_accept [n_segs], picks [n_rows])."""
    logits2d = np.ascontiguousarray(logits2d, np.float32)
    R, V = logits2d.shape
    tab = np.ascontiguousarray(seg_tab, np.int32).reshape(-1, 6)
    tokens = np.ascontiguousarray(tokens, np.int32).ravel()
    if tokens.size != R:
        raise ValueError(f"op_sched_accept: {R} rows, {tokens.size} tokens")
    words = [a for a in (state, log, next_tok) if a is not None]
    for a in words:
        if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous):
            raise ValueError("op_sched_accept: the slot words are int32 C-contiguous arrays, updated in place")
    n_slots = int(next_tok.size) if next_tok is not None else 0
    log_cap = int(log.size // max(n_slots, 1)) if log is not None else 0
    if len(words) == 3 and (state.size != 2 * n_slots or log.size != n_slots * log_cap):
        raise ValueError("op_sched_accept: state [n_slots][2], log [n_slots][log_cap], next_tok [n_slots]")
    n_acc = np.full(max(len(tab), 1), -7, np.int32)
    picks = np.full(max(R, 1), -7, np.int32)
    err = C.create_string_buffer(1024)
    _check(lib().llamahip_op_sched_accept(_ptr(logits2d), R, V, _ptr(tab), len(tab), _ptr(tokens), n_slots, log_cap,
                                          *(None if a is None else _ptr(a) for a in (state, log, next_tok)), _ptr(n_acc), _ptr(picks), err, len(err)), err)
    return n_acc[:len(tab)], picks[:R]


def sched_plan_prefix(slot_free, held, prompt, chunk_tokens: int):
    """llamahip_sched_plan_prefix (host only): held[s] = the prompt tokens whose KV rows slot s holds as prompt rows, slot_free[s] whether the
    slot is free.  Returns (shared rows P, slot, donor or -1, rows already in place in that slot); P == -1 = bad arguments."""
    free = np.ascontiguousarray(slot_free, np.int32).ravel()
    recs = [np.ascontiguousarray(h, np.int32).ravel() for h in held]
    if len(recs) != free.size:
        raise ValueError(f"sched_plan_prefix: {free.size} slots, {len(recs)} records")
    n_held = np.array([h.size for h in recs], np.int32)
    cat = np.concatenate(recs + [np.zeros(1, np.int32)]).astype(np.int32)          # (the last entry is never read: a non-null array where nothing is held)
    prompt = np.ascontiguousarray(prompt, np.int32).ravel()
    slot, donor, inplace = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    P = lib().llamahip_sched_plan_prefix(free.size, _ptr(free) if free.size else None, _ptr(cat), _ptr(n_held) if free.size else None,
                                         _ptr(prompt) if prompt.size else None, prompt.size, int(chunk_tokens), C.byref(slot), C.byref(donor), C.byref(inplace))
    return int(P), int(slot.value), int(donor.value), int(inplace.value)


def sched_plan(prompt_left, chunk_tokens: int, row_budget: int):
    """llamahip_sched_plan (host only): (total rows, rows per sequence) of the next step for sequences in admission order with prompt_left[i]
    prompt tokens still to evaluate (0 = decoding); total -1 = bad arguments."""
    left = np.ascontiguousarray(prompt_left, np.int32).ravel()
    rows = np.full(max(left.size, 1), -1, np.int32)
    total = lib().llamahip_sched_plan(left.size, _ptr(left) if left.size else None, int(chunk_tokens), int(row_budget), _ptr(rows))
    return int(total), rows[:left.size]


def op_sched_pick(logits2d, emit) -> np.ndarray:
    """k_sched_pick's pick half on host rows: picks[r] = the greedy pick of row r where emit[r], -1 elsewhere (llamahip_op_sched_pick)."""
    logits2d = np.ascontiguousarray(logits2d, np.float32)
    R, V = logits2d.shape
    emit = np.ascontiguousarray(emit, np.int32).ravel()
    if emit.size != R:
        raise ValueError(f"op_sched_pick: {R} rows, {emit.size} emit flags")
    picks = np.full(max(R, 1), -7, np.int32)
    err = C.create_string_buffer(1024)
    _check(lib().llamahip_op_sched_pick(_ptr(logits2d), R, V, _ptr(emit), _ptr(picks), err, len(err)), err)
    return picks[:R]


def ctx_overflow_plan(n_ctx: int, n_past: int, n_keep: int):
    """llamahip_ctx_overflow_plan (host only): (new context, n_discard) with n_discard = (n_past - n_keep) // 2, or (-1, 0) where nothing can be dropped."""
    nd = C.c_int32(-1)
    new = lib().llamahip_ctx_overflow_plan(n_ctx, n_past, n_keep, C.byref(nd))
    return int(new), int(nd.value)


def op_topk(logits, window, repeat_penalty: float = 1.3, top_k: int = 40, temp: float = float(np.float32(0.8))):
    """Device half of the sampler on host logits: returns (exact, scores[top_k], ids[top_k])."""
    logits = np.ascontiguousarray(logits, np.float32)
    window = np.ascontiguousarray(window, np.int32)
    sc, ids, exact = np.zeros(64, np.float64), np.zeros(64, np.int32), C.c_int32(0)
    err = C.create_string_buffer(512)
    rc = lib().llamahip_op_topk(_ptr(logits), logits.size, _ptr(window), window.size, repeat_penalty, top_k, temp, _ptr(sc), _ptr(ids), C.byref(exact), err, len(err))
    _check(rc, err)
    return bool(exact.value), sc[:top_k], ids[:top_k]


def op_topk_rows(logits2d, windows, repeat_penalty: float = 1.3, top_k: int = 40, temp: float = float(np.float32(0.8)), want_spill: bool = False):
    """The batched device half of the sampler on host rows f32 [R, n_vocab]; windows: R id lists (up to 1024 ids each; longer: the row is
    reported inexact).  Returns (exact bool[R], scores float64[R][top_k], ids int32[R][top_k]), and with want_spill the [R, n_vocab] rows the
    kernel copied out (the rows reported inexact; NaN elsewhere)."""
    logits2d = np.ascontiguousarray(logits2d, np.float32)
    if logits2d.ndim == 1:
        logits2d = logits2d.reshape(1, -1)
    R, V = logits2d.shape
    if len(windows) != R:
        raise ValueError(f"{len(windows)} windows for {R} rows")
    win = np.zeros((R, 1024), np.int32)
    n_last = np.zeros(R, np.int32)
    for r, w in enumerate(windows):
        w = np.asarray(w, np.int32).ravel()
        n_last[r] = w.size
        win[r, :min(w.size, 1024)] = w[:1024]
    sc, ids, exact = np.zeros((R, 64), np.float64), np.zeros((R, 64), np.int32), np.zeros(R, np.int32)
    spill = np.full((R, V), np.nan, np.float32) if want_spill else None
    err = C.create_string_buffer(512)
    rc = lib().llamahip_op_topk_rows(_ptr(logits2d), R, V, _ptr(win), _ptr(n_last), repeat_penalty, top_k, temp, _ptr(sc), _ptr(ids), _ptr(exact),
                                     _ptr(spill), err, len(err))
    _check(rc, err)
    res = (exact.astype(bool), sc[:, :top_k].copy(), ids[:, :top_k].copy())
    return res + (spill,) if want_spill else res


def op_topk_slide(logits2d, ids, n_last: int, repeat_penalty: float = 1.3, top_k: int = 40, temp: float = float(np.float32(0.8))):
    """k_topk_keys_slide + k_topk_select_rows on host rows f32 [R, n_vocab] (1 .. 16 rows): ids is ONE stream of n_last + R - 1 ids, row r's
    window = ids[r : r + n_last].  Returns (exact bool[R], scores float64[R][top_k], ids int32[R][top_k])."""
    logits2d = np.ascontiguousarray(logits2d, np.float32)
    if logits2d.ndim == 1:
        logits2d = logits2d.reshape(1, -1)
    R, V = logits2d.shape
    ids = np.ascontiguousarray(ids, np.int32).ravel()
    if ids.size != max(n_last + R - 1, 0):
        raise ValueError(f"ids: {ids.size} ids for {R} rows with windows of {n_last} (want {n_last + R - 1})")
    sc, out_ids, exact = np.zeros((max(R, 1), 64), np.float64), np.zeros((max(R, 1), 64), np.int32), np.zeros(max(R, 1), np.int32)
    err = C.create_string_buffer(512)
    rc = lib().llamahip_op_topk_slide(_ptr(logits2d), R, V, _ptr(ids), n_last, repeat_penalty, top_k, temp, _ptr(sc), _ptr(out_ids), _ptr(exact), err, len(err))
    _check(rc, err)
    return exact[:R].astype(bool), sc[:R, :top_k].copy(), out_ids[:R, :top_k].copy()


def op_topk_slide_set(logits2d, ids, seg_begin, seg_ids_off, seg_n_last, repeat_penalty: float = 1.3, top_k: int = 40, temp: float = float(np.float32(0.8))):
    """k_topk_keys_slide_set + k_topk_select_rows on host rows f32 [R, n_vocab] (1 .. 16 rows) cut into the segments [seg_begin[s], seg_begin[s + 1]):
    row j of segment s has the window ids[seg_ids_off[s] + j : + seg_n_last[s]] of the id pool `ids` (seg_n_last[s] > 1024: its rows are
    reported inexact).  Returns (exact bool[R], scores float64[R][top_k], ids int32[R][top_k])."""
    logits2d = np.ascontiguousarray(logits2d, np.float32)
    if logits2d.ndim == 1:
        logits2d = logits2d.reshape(1, -1)
    R, V = logits2d.shape
    ids = np.ascontiguousarray(ids, np.int32).ravel()
    seg_begin = np.ascontiguousarray(seg_begin, np.int32).ravel()
    off, nl = np.ascontiguousarray(seg_ids_off, np.int32).ravel(), np.ascontiguousarray(seg_n_last, np.int32).ravel()
    if seg_begin.size < 2 or off.size != seg_begin.size - 1 or nl.size != off.size:
        raise ValueError(f"op_topk_slide_set: {seg_begin.size} segment bounds, {off.size} offsets, {nl.size} window lengths")
    sc, out_ids, exact = np.zeros((max(R, 1), 64), np.float64), np.zeros((max(R, 1), 64), np.int32), np.zeros(max(R, 1), np.int32)
    err = C.create_string_buffer(512)
    rc = lib().llamahip_op_topk_slide_set(_ptr(logits2d), R, V, _ptr(ids) if ids.size else None, ids.size, _ptr(seg_begin), seg_begin.size - 1, _ptr(off), _ptr(nl),
                                          repeat_penalty, top_k, temp, _ptr(sc), _ptr(out_ids), _ptr(exact), err, len(err))
    _check(rc, err)
    return exact[:R].astype(bool), sc[:R, :top_k].copy(), out_ids[:R, :top_k].copy()


def op_logprob(logits2d, targets=None):
    """k_row_logprob on host rows f32 [n_rows, n_vocab]: returns (logprob float64, argmax int32, rank int32) per row; targets -1 = not scored."""
    logits2d = np.ascontiguousarray(logits2d, np.float32)
    if logits2d.ndim == 1:
        logits2d = logits2d.reshape(1, -1)
    R, V = logits2d.shape
    if targets is not None:
        targets = np.ascontiguousarray(targets, np.int32)
        if targets.size != R:
            raise ValueError(f"targets: {targets.size} ids for {R} rows")
    lp, am, rk = np.empty(R, np.float64), np.empty(R, np.int32), np.empty(R, np.int32)
    err = C.create_string_buffer(512)
    rc = lib().llamahip_op_logprob(_ptr(logits2d), R, V, _ptr(targets), _ptr(lp), _ptr(am), _ptr(rk), err, len(err))
    _check(rc, err)
    return lp, am, rk


def op_top_logprobs(logits2d, n_top: int):
    """k_row_topn on host rows f32 [n_rows, n_vocab]: returns (ids int32 [n_rows, n_top], logprob float64 [n_rows, n_top]) -- per row the n_top
    entries by value descending (the lower index first on ties) with their log-probabilities; a row with a NaN or a +inf: ids -1, logprobs NaN."""
    logits2d = np.ascontiguousarray(logits2d, np.float32)
    if logits2d.ndim == 1:
        logits2d = logits2d.reshape(1, -1)
    R, V = logits2d.shape
    n = min(max(int(n_top), 0), 1024)
    ids, lp = np.empty((R, n), np.int32), np.empty((R, n), np.float64)
    err = C.create_string_buffer(512)
    rc = lib().llamahip_op_top_logprobs(_ptr(logits2d), R, V, n_top, _ptr(ids), _ptr(lp), err, len(err))
    _check(rc, err)
    return ids, lp


def beam_select(live_score, cand_ids, cand_logprob, n_beams: int, stop_token: int = -1) -> dict:
    """llamahip_beam_select, the step rule of llamahip_beam_search (host only): live_score [n_live], cand_ids / cand_logprob [n_live, n_cand].
    Returns parent / token / score of the new live beams in rank order, fin_parent / fin_score of the walk's finished entries, n_dead."""
    sc = np.ascontiguousarray(live_score, np.float64).reshape(-1)
    ids = np.ascontiguousarray(cand_ids, np.int32).reshape(sc.size, -1)
    lp = np.ascontiguousarray(cand_logprob, np.float64).reshape(sc.size, -1)
    if ids.shape != lp.shape:
        raise ValueError("cand_ids and cand_logprob differ in shape")
    cap = max(n_beams, 1)
    par, tok, nsc = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
    fpar, fsc = np.zeros(max(sc.size, 1), np.int32), np.zeros(max(sc.size, 1), np.float64)
    nn, nf, nd = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = lib().llamahip_beam_select(sc.size, _ptr(sc), ids.shape[1], _ptr(ids), _ptr(lp), n_beams, stop_token, _ptr(par), _ptr(tok), _ptr(nsc), C.byref(nn),
                                    _ptr(fpar), _ptr(fsc), C.byref(nf), C.byref(nd))
    if rc != 0:
        raise LlamaHipError(-1, f"llamahip_beam_select refused its arguments (n_live {sc.size}, n_cand {ids.shape[1]}, n_beams {n_beams})")
    return {"parent": par[: nn.value].copy(), "token": tok[: nn.value].copy(), "score": nsc[: nn.value].copy(),
            "fin_parent": fpar[: nf.value].copy(), "fin_score": fsc[: nf.value].copy(), "n_dead": nd.value}


def beam_slots(prev_slot, parent, n_beams: int):
    """llamahip_beam_slots (host only): the slots of a step's new beams and the KV copies [(src slot, dst slot), ...] they need."""
    prev = np.ascontiguousarray(prev_slot, np.int32).reshape(-1)
    par = np.ascontiguousarray(parent, np.int32).reshape(-1)
    cap = max(par.size, 1)
    ns, cs, cd = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    n = lib().llamahip_beam_slots(prev.size, _ptr(prev), par.size, _ptr(par), n_beams, _ptr(ns), _ptr(cs), _ptr(cd))
    if n < 0:
        raise LlamaHipError(-1, f"llamahip_beam_slots refused its arguments (n_prev {prev.size}, n_new {par.size}, n_beams {n_beams})")
    return ns[: par.size].copy(), [(int(cs[k]), int(cd[k])) for k in range(n)]


def _pool_id(pool) -> int:
    return _POOLS[pool] if isinstance(pool, str) else int(pool)


def op_pool_rows(x, norm_w, seg_begin, pool="last", normalize: bool = False, out=None) -> np.ndarray:
    """The tail of an embedding pass (k_norm_rows_f32, k_pool_rows, the L2 normalisation) on host rows x f32 [R, d]: the final norm with norm_w,
    rows [seg_begin[s], seg_begin[s + 1]) pooled per segment; returns [n_segs, d].  out: a caller's float32 buffer of at least n_segs * d
    floats, written in place (what lies behind the result keeps its bits)."""
    x = np.ascontiguousarray(x, np.float32)
    norm_w = np.ascontiguousarray(norm_w, np.float32)
    seg = np.ascontiguousarray(seg_begin, np.int32).ravel()
    R, d = x.shape
    n_segs = seg.size - 1
    if out is None:
        out = np.empty(max(n_segs, 1) * d, np.float32)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_pool_rows(_ptr(x), R, d, _ptr(norm_w), _ptr(seg), n_segs, _pool_id(pool), int(normalize), _ptr(out), err, len(err))
    _check(rc, err)
    return out.ravel()[:max(n_segs, 0) * d].reshape(max(n_segs, 0), d)


def lookup_draft(history, corpus=None, draft_len: int = 0, ngram_min: int = 0, ngram_max: int = 0) -> np.ndarray:
    """llamahip_lookup_draft (host only): the tokens that followed the most recent earlier occurrence of history's last n tokens -- in history,
    else in corpus -- for the longest n of ngram_max .. ngram_min that occurs; empty = no hit.  0 = the header's defaults."""
    history = np.ascontiguousarray(history, np.int32).ravel()
    corpus = None if corpus is None else np.ascontiguousarray(corpus, np.int32).ravel()
    out = np.empty(max(draft_len, 16), np.int32)
    n = lib().llamahip_lookup_draft(_ptr(history), history.size, _ptr(corpus), 0 if corpus is None else corpus.size, draft_len, ngram_min, ngram_max, _ptr(out))
    if n < 0:
        raise ValueError(f"lookup_draft: bad arguments (draft_len {draft_len}, ngram_min {ngram_min}, ngram_max {ngram_max})")
    return out[:n].copy()


def lookup_deal_rows(want, budget: int = 16) -> np.ndarray:
    """llamahip_lookup_deal_rows (host only): the draft tokens each sequence of a step gets -- every sequence has its base row, the
    budget - n_seqs spare rows go one at a time, round-robin in ascending order, to the sequences that still want more."""
    want = np.ascontiguousarray(want, np.int32).ravel()
    give = np.zeros(max(want.size, 1), np.int32)
    n = lib().llamahip_lookup_deal_rows(_ptr(want), want.size, budget, _ptr(give))
    if n < 0:
        raise ValueError(f"lookup_deal_rows: bad arguments ({want.size} sequences, budget {budget}, want {want.tolist()})")
    return give[:want.size].copy()


def op_verify_rows_set(logits2d, tokens, seg_begin):
    """k_verify_rows + k_accept_drafts_set on host rows f32 [n_rows, n_vocab] (1 .. 16 rows) cut into the segments [seg_begin[s], seg_begin[s + 1]):
    a segment's first token its last token, the rest its draft.  Returns (n_accept int32[n_segs], picks int32[n_rows])."""
    logits2d = np.ascontiguousarray(logits2d, np.float32)
    if logits2d.ndim == 1:
        logits2d = logits2d.reshape(1, -1)
    R, V = logits2d.shape
    tokens = np.ascontiguousarray(tokens, np.int32).ravel()
    seg_begin = np.ascontiguousarray(seg_begin, np.int32).ravel()
    if tokens.size != R:
        raise ValueError(f"tokens: {tokens.size} ids for {R} rows")
    if seg_begin.size < 2:
        raise ValueError("seg_begin: at least one segment")
    n_segs = seg_begin.size - 1
    picks, n_acc = np.full(R, -1, np.int32), np.full(n_segs, -1, np.int32)
    err = C.create_string_buffer(512)
    rc = lib().llamahip_op_verify_rows_set(_ptr(logits2d), R, V, _ptr(tokens), _ptr(seg_begin), n_segs, _ptr(n_acc), _ptr(picks), err, len(err))
    _check(rc, err)
    return n_acc, picks


def _dfa_operands(logits2d, table, states):
    logits2d = np.ascontiguousarray(logits2d, np.float32)
    if logits2d.ndim == 1:
        logits2d = logits2d.reshape(1, -1)
    R, V = logits2d.shape
    table = np.ascontiguousarray(table, np.uint16)
    if table.ndim != 2 or table.shape[1] != V:
        raise ValueError(f"table: uint16 [n_states, {V}]")
    states = np.array(states, np.int32).ravel()
    if states.size != R:
        raise ValueError(f"states: {states.size} for {R} rows")
    return logits2d, R, V, table, states


def _dfa_rows_args(logits2d, table, states, fallback):
    logits2d = np.ascontiguousarray(logits2d, np.float32)
    table = np.ascontiguousarray(table, np.uint16)
    R, V = logits2d.shape
    if table.ndim != 2 or table.shape[1] != V:
        raise ValueError(f"table is uint16 [n_states, n_vocab = {V}]")
    states = np.ascontiguousarray(states, np.int32).ravel()
    fallback = np.ascontiguousarray(np.broadcast_to(np.asarray(fallback, np.int32), (R,)), np.int32)
    if states.size != R:
        raise ValueError(f"{states.size} states for {R} rows")
    return logits2d, table, states, fallback, R, V


def op_verify_rows_dfa(logits2d, table, states, fallback, picks=None, dead=None):
    """k_verify_rows_dfa on host rows (llamahip_op_verify_rows_allow): states[r] = the table row of logits row r, -1 = unconstrained;
    returns (picks, dead).  picks / dead, if given, go up first: what the kernel leaves alone keeps their values."""
    logits2d, table, states, fallback, R, V = _dfa_rows_args(logits2d, table, states, fallback)
    picks = np.full(R, -7, np.int32) if picks is None else np.ascontiguousarray(picks, np.int32).copy()
    dead = np.full(R, -7, np.int32) if dead is None else np.ascontiguousarray(dead, np.int32).copy()
    err = C.create_string_buffer(1024)
    _check(lib().llamahip_op_verify_rows_allow(_ptr(logits2d), R, V, _ptr(table), table.shape[0], _ptr(states), _ptr(fallback), _ptr(picks), _ptr(dead), err, len(err)), err)
    return picks, dead


def op_sched_pick_dfa(logits2d, emit, table, states, fallback, seg_words=None, state=None, log=None, next_tok=None):
    """k_sched_pick_dfa on host rows, one segment per row (llamahip_op_sched_pick_allow): returns (picks, dead), picks[r] = -1 where emit[r] == 0.
    With slot words -- seg_words [R, 3] = {slot, position, cursor}, state [n_slots, 2], log [n_slots, log_cap], next_tok [n_slots] -- the
    three arrays are updated in place as the kernel leaves them."""
    logits2d, table, states, fallback, R, V = _dfa_rows_args(logits2d, table, states, fallback)
    emit = np.ascontiguousarray(emit, np.int32).ravel()
    if emit.size != R:
        raise ValueError(f"{emit.size} emit flags for {R} rows")
    picks, dead = np.full(R, -7, np.int32), np.full(R, -7, np.int32)
    n_slots = log_cap = 0
    if seg_words is not None:
        seg_words = np.ascontiguousarray(seg_words, np.int32)
        for a in (state, log, next_tok):
            if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous):
                raise ValueError("state, log and next_tok are contiguous int32 arrays (updated in place)")
        n_slots, log_cap = log.shape
        if seg_words.shape != (R, 3) or state.shape != (n_slots, 2) or next_tok.shape != (n_slots,):
            raise ValueError("seg_words [R, 3], state [n_slots, 2], log [n_slots, log_cap], next_tok [n_slots]")
    err = C.create_string_buffer(1024)
    _check(lib().llamahip_op_sched_pick_allow(_ptr(logits2d), R, V, _ptr(emit), _ptr(table), table.shape[0], _ptr(states), _ptr(fallback),
                                            None if seg_words is None else _ptr(seg_words), n_slots, log_cap,
                                            None if seg_words is None else _ptr(state), None if seg_words is None else _ptr(log),
                                            None if seg_words is None else _ptr(next_tok), _ptr(picks), _ptr(dead), err, len(err)), err)
    return picks, dead


def op_pick_dfa(logits2d, table, states, fallback_token: int, picks=None, dead=None):
    """k_pick_dfa on host rows f32 [n_rows, n_vocab] (1 .. 16 rows) under ONE table uint16 [n_states, n_vocab] (0xFFFF = banned) with per-row
    states.  picks / dead: what the words hold before the launch (default -1 / 0).  Returns (picks, next states, dead), int32[n_rows] each."""
    logits2d, R, V, table, states = _dfa_operands(logits2d, table, states)
    picks = np.full(R, -1, np.int32) if picks is None else np.array(picks, np.int32).ravel()
    dead = np.zeros(R, np.int32) if dead is None else np.array(dead, np.int32).ravel()
    err = C.create_string_buffer(512)
    rc = lib().llamahip_op_pick_dfa(_ptr(logits2d), R, V, _ptr(table), table.shape[0], _ptr(states), int(fallback_token), _ptr(picks), _ptr(dead), err, len(err))
    _check(rc, err)
    return picks, states, dead


def op_mask_rows_dfa(logits2d, table, states, out=None):
    """k_mask_rows_dfa on host rows: f32 [n_rows, n_vocab] with the banned entries of each row's state at -inf, the others bit for bit.
    out: what the result buffer holds before the launch."""
    logits2d, R, V, table, states = _dfa_operands(logits2d, table, states)
    out = np.zeros((R, V), np.float32) if out is None else np.array(out, np.float32).reshape(R, V)
    err = C.create_string_buffer(512)
    rc = lib().llamahip_op_mask_rows_dfa(_ptr(logits2d), R, V, _ptr(table), table.shape[0], _ptr(states), _ptr(out), err, len(err))
    _check(rc, err)
    return out


def op_verify_rows(logits2d, tokens):
    """k_verify_rows + k_accept_drafts on host rows f32 [n_rows, n_vocab] (1 .. 16 rows); tokens = [last token, draft ...], one per row.
    Returns (n_accept, picks int32[n_rows])."""
    logits2d = np.ascontiguousarray(logits2d, np.float32)
    if logits2d.ndim == 1:
        logits2d = logits2d.reshape(1, -1)
    R, V = logits2d.shape
    tokens = np.ascontiguousarray(tokens, np.int32).ravel()
    if tokens.size != R:
        raise ValueError(f"tokens: {tokens.size} ids for {R} rows")
    picks, n_acc = np.full(R, -1, np.int32), C.c_int32(-1)
    err = C.create_string_buffer(512)
    rc = lib().llamahip_op_verify_rows(_ptr(logits2d), R, V, _ptr(tokens), C.byref(n_acc), _ptr(picks), err, len(err))
    _check(rc, err)
    return n_acc.value, picks


def op_mul_mat_q4_0(wq: np.ndarray, x: np.ndarray) -> np.ndarray:
    """wq uint8 [M, K/32, 20] (file layout), x f32 [N, K] -> f32 [N, M] on the GPU."""
    wq = np.ascontiguousarray(wq, np.uint8)
    M, nb, _ = wq.shape
    K = nb * 32
    x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
    N = x.shape[0]
    y = np.empty((N, M), np.float32)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_mul_mat_q4_0(_ptr(wq), M, K, _ptr(x), N, _ptr(y), err, len(err))
    _check(rc, err)
    return y


GEMM_PATHS = ("auto", "mfma4", "mfma_i8", "fast", "rows", "set", "lds", "gemv")      # LLAMAHIP_GEMM_* of llamahip.h, in order


def op_prompt_gemm_q4_0(wq: np.ndarray, x: np.ndarray, resid=None, path: str = "auto", y_stride: int | None = None, y_init=None):
    """One prompt GEMM kernel (llamahip_op_prompt_gemm_q4_0): wq uint8 [M, K/32, 20] (file layout), x f32 [N, K], resid f32 [N, M] or None.
    path: one of GEMM_PATHS[:7].  Returns (y f32 [N, y_stride], the path taken): the whole buffer as the device left it -- y_init
    (default: NaN everywhere) is what columns M .. y_stride - 1 and any output a kernel skips keep."""
    wq = np.ascontiguousarray(wq, np.uint8)
    M, nb, _ = wq.shape
    K = nb * 32
    x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
    N = x.shape[0]
    ys = M if y_stride is None else int(y_stride)
    y = np.full((N, ys), np.nan, np.float32) if y_init is None else np.array(y_init, np.float32, order="C").reshape(N, ys)
    if resid is not None:
        resid = np.ascontiguousarray(resid, np.float32).reshape(N, M)
    code = GEMM_PATHS.index(path) if path in GEMM_PATHS else int(path)
    taken = C.c_int32(-1)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_prompt_gemm_q4_0(_ptr(wq), M, K, _ptr(x), N, _ptr(resid), _ptr(y), ys, code, C.byref(taken), err, len(err))
    _check(rc, err)
    return y, GEMM_PATHS[taken.value]


DENSE_PATHS = ("auto", "mv", "mm", "set", "mfma")      # LLAMAHIP_DENSE_* of llamahip.h, in order


def op_mul_mat_dense(w: np.ndarray, x: np.ndarray, resid=None, path: str = "auto", y_stride: int | None = None, y_init=None, wtype: int | None = None):
    """One f16 / f32 mat-mul kernel (llamahip_op_mul_mat_dense): w float16 or float32 [M, K] (file layout; wtype overrides the dtype's 1 / 0),
    x f32 [N, K], resid f32 [N, M] or None.  path: one of DENSE_PATHS.  Returns (y f32 [N, y_stride], the path taken): the whole buffer as the
    device left it -- y_init (default: NaN everywhere) is what columns M .. y_stride - 1 keep."""
    w = np.ascontiguousarray(w)
    if w.dtype not in (np.float16, np.float32):
        w = w.astype(np.float32)
    wt = (1 if w.dtype == np.float16 else 0) if wtype is None else int(wtype)
    M, K = w.shape
    x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
    N = x.shape[0]
    ys = M if y_stride is None else int(y_stride)
    y = np.full((N, max(ys, 0)), np.nan, np.float32) if y_init is None else np.array(y_init, np.float32, order="C").reshape(N, ys)
    if resid is not None:
        resid = np.ascontiguousarray(resid, np.float32).reshape(N, M)
    code = DENSE_PATHS.index(path) if path in DENSE_PATHS else int(path)
    taken = C.c_int32(-1)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_mul_mat_dense(_ptr(w), wt, M, K, _ptr(x), N, _ptr(resid), _ptr(y), ys, code, C.byref(taken), err, len(err))
    _check(rc, err)
    return y, DENSE_PATHS[taken.value]


Q41_PATHS = ("auto", "chain", "lane")      # LLAMAHIP_Q41_* of llamahip.h, in order


def op_mul_mat_q4_1(w: np.ndarray, x: np.ndarray, resid=None, path: str = "auto", y_stride: int | None = None, y_init=None, K: int | None = None):
    """One Q4_1 mat-mul kernel (llamahip_op_mul_mat_q4_1): w uint8 [M, K/32 * 24], the rows in file layout ([K/32 f32 min][K/32 f32 d][K/32 * 16
    nibble bytes]); x f32 [N, K], resid f32 [N, M] or None.  path: one of Q41_PATHS.  Returns (y f32 [N, y_stride], the path taken): the
    whole buffer as the device left it -- y_init (default: NaN everywhere) is what columns M .. y_stride - 1 keep.  K overrides the row
    length the shape of w implies (refusal tests)."""
    w = np.ascontiguousarray(w, np.uint8)
    M, rb = w.shape
    x = np.ascontiguousarray(x, np.float32)
    if K is None:
        K = rb // 24 * 32
        x = x.reshape(-1, K)
    N = x.shape[0]
    ys = M if y_stride is None else int(y_stride)
    y = np.full((N, max(ys, 0)), np.nan, np.float32) if y_init is None else np.array(y_init, np.float32, order="C").reshape(N, ys)
    if resid is not None:
        resid = np.ascontiguousarray(resid, np.float32).reshape(N, M)
    code = Q41_PATHS.index(path) if path in Q41_PATHS else int(path)
    taken = C.c_int32(-1)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_mul_mat_q4_1(_ptr(w), M, K, _ptr(x), N, _ptr(resid), _ptr(y), ys, code, C.byref(taken), err, len(err))
    _check(rc, err)
    return y, Q41_PATHS[taken.value]


ATTN_PATHS = ("auto", "mfma", "row", "short", "dec", "dec_stream")      # LLAMAHIP_ATTN_* of llamahip.h, in order


def op_attention(qkv: np.ndarray, H: int, n_past: int, Kc: np.ndarray, Vc: np.ndarray, n_threads: int = 8, chunk: int = 0,
                 path: str = "auto", ws_rows: int = 0, merged_stride: int | None = None, merged_init=None, want_wo: bool = True):
    """One layer's attention (llamahip_op_attention): qkv f32 [N, 3d] un-rotated, Kc / Vc f32 [n_ctx, d] (updated in place: the device's
    whole copy comes back).  Returns (merged f32 [N, merged_stride] -- merged_init, default NaN, where nothing was written --, the wo
    operand uint8 [N, d/32, 20] or None, the path taken)."""
    qkv = np.ascontiguousarray(qkv, np.float32)
    N, d3 = qkv.shape
    d = d3 // 3
    for a in (Kc, Vc):
        if a.dtype != np.float32 or not a.flags.c_contiguous or a.ndim != 2 or a.shape[1] != d or a.shape[0] != Kc.shape[0]:
            raise ValueError("Kc / Vc must be C-contiguous float32 [n_ctx, d]")
    ms = d if merged_stride is None else int(merged_stride)
    merged = np.full((N, ms), np.nan, np.float32) if merged_init is None else np.array(merged_init, np.float32, order="C").reshape(N, ms)
    wo = np.full((N, max(d // 32, 1), 20), 0xEE, np.uint8) if want_wo else None
    code = ATTN_PATHS.index(path) if path in ATTN_PATHS else int(path)
    taken = C.c_int32(-1)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_attention(_ptr(qkv), N, d, int(H), int(n_past), Kc.shape[0], _ptr(Kc), _ptr(Vc), int(n_threads), int(chunk),
                                     code, int(ws_rows), _ptr(merged), ms, _ptr(wo), C.byref(taken), err, len(err))
    _check(rc, err)
    name = ATTN_PATHS[taken.value]
    return merged, (wo if name in ("short", "dec", "dec_stream") else None), name


DEC_ATTN_PATHS = ("x", "stream", "dma")                                # LLAMAHIP_DEC_ATTN_* of llamahip.h, in order
DEC_ATTN_KERNELS = ("pv_blk", "attn_x", "pv_stream", "pv_dma")         # LLAMAHIP_DEC_KERNEL_*, in order
DecAttnPlan = collections.namedtuple("DecAttnPlan", "kernel split cpw SR NS lds grid threads")


def _dec_force(force):
    """None, or int32 [4] = (split, stage_rows, ns, dma) from a tuple or a dict of some of them (0, dma -1: the library's rule)"""
    if force is None:
        return None
    if isinstance(force, dict):
        force = (force.get("split", 0), force.get("stage_rows", 0), force.get("ns", 0), force.get("dma", -1))
    return np.ascontiguousarray(force, np.int32).reshape(4)


def _dec_plan(a) -> DecAttnPlan:
    return DecAttnPlan(DEC_ATTN_KERNELS[int(a[0])], *(int(v) for v in a[1:]))


def dec_attn_plan(d: int, H: int, n_ctx: int, n_threads: int, long_ctx: bool = False, have_sync: bool = True, have_xpart: bool = True, force=None):
    """Host-only: the launch plan of the one-row decode attention (llamahip_debug_dec_attn_plan) as DecAttnPlan(kernel, split, cpw, SR, NS, lds,
    grid, threads).  force None: what a model handle launches (the rule under the LLAMAHIP_PV_* switches); else (split, stage_rows, ns, dma) or
    a dict of some of them, taken exactly or refused: LlamaHipError with the reason."""
    a = np.zeros(8, np.int64)
    why = C.create_string_buffer(256)
    if not lib().llamahip_debug_dec_attn_plan(int(d), int(H), int(n_ctx), int(n_threads), int(long_ctx), int(have_sync), int(have_xpart),
                                              _ptr(_dec_force(force)), _ptr(a), why, len(why)):
        raise LlamaHipError(-1, why.value.decode(errors="replace"))
    return _dec_plan(a)


def qkv_attn_plan(d: int, H: int, n_ctx: int, n_threads: int, n_part_in: int = 0):
    """Host-only: (prologue, depth, pg, grid, lds) of the fused wq|wk|wv + attention launch of a model of head layout (d, H), or None where
    k_qkv_attn does not take it (llamahip_debug_qkv_attn_plan)."""
    a = np.zeros(5, np.int64)
    return tuple(int(v) for v in a) if lib().llamahip_debug_qkv_attn_plan(int(d), int(H), int(n_ctx), int(n_threads), int(n_part_in), _ptr(a), None, 0) else None


def op_dec_attention(path: str, steps, H: int, Kc: np.ndarray, Vc: np.ndarray, n_threads: int = 8, force=None, epoch0: int = 0, want_wo: bool = True):
    """Decode steps of one layer's attention through a hand-off kernel (llamahip_op_dec_attention), on hand-off buffers the op zeroes once and
    keeps across the steps.  path "x" | "stream" | "dma"; steps: [(qkv f32 [3d] un-rotated, n_past, layer, bump_epoch), ...]; Kc / Vc f32
    [n_ctx, d] (updated in place: the device's whole copy comes back); force as dec_attn_plan's.  Returns (merged f32 [n_steps, d], the wo
    operand uint8 [n_steps, d/32, 20] or None, fault uint32 [n_steps], the DecAttnPlan that ran)."""
    n = len(steps)
    qkv = np.ascontiguousarray(np.stack([np.asarray(s[0], np.float32).ravel() for s in steps]), np.float32) if n else np.zeros((0, 3), np.float32)
    d = qkv.shape[1] // 3
    for a in (Kc, Vc):
        if a.dtype != np.float32 or not a.flags.c_contiguous or a.ndim != 2 or a.shape[1] != d or a.shape[0] != Kc.shape[0]:
            raise ValueError("Kc / Vc must be C-contiguous float32 [n_ctx, d]")
    cols = [np.ascontiguousarray([int(s[k]) for s in steps], np.int32) for k in (1, 2, 3)]
    merged = np.full((n, d), np.nan, np.float32)
    wo = np.full((n, max(d // 32, 1), 20), 0xEE, np.uint8) if want_wo else None
    fault = np.full(max(n, 1), 0xFFFFFFFF, np.uint32)
    plan = np.full(8, -1, np.int64)
    code = DEC_ATTN_PATHS.index(path) if path in DEC_ATTN_PATHS else int(path)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_dec_attention(_ptr(qkv), n, _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), int(epoch0) & 0xFFFFFFFF, d, int(H), Kc.shape[0],
                                         _ptr(Kc), _ptr(Vc), int(n_threads), code, _ptr(_dec_force(force)), _ptr(merged), _ptr(wo), _ptr(fault),
                                         _ptr(plan), err, len(err))
    _check(rc, err)
    return merged, wo, fault[:n], _dec_plan(plan)


def op_qkv_attn(wq: np.ndarray, norm_w, steps, H: int, Kc: np.ndarray, Vc: np.ndarray, n_threads: int = 8, epoch0: int = 0, tagged_in: bool = False,
                want_wo: bool = True):
    """Decode steps of the fused wq|wk|wv + attention launch (llamahip_op_qkv_attn).  wq uint8 [3d, d/32, 20] in file layout; norm_w f32 [d];
    steps: [(x f32 [d], part_in float64 [n, 2] or None, n_past, layer, bump_epoch), ...]; Kc / Vc f32 [n_ctx, d] (updated in place).  Returns
    (merged f32 [n_steps, d], the wo operand uint8 [n_steps, d/32, 20] or None, fault uint32 [n_steps], plans [(pre, depth, pg, grid, lds)])."""
    wq = np.ascontiguousarray(wq, np.uint8)
    d = wq.shape[1] * 32
    n = len(steps)
    x = np.ascontiguousarray(np.stack([np.asarray(s[0], np.float32).ravel() for s in steps]), np.float32)
    parts = [None if s[1] is None else np.ascontiguousarray(s[1], np.float64).reshape(-1, 2) for s in steps]
    n_part = np.ascontiguousarray([0 if p is None else p.shape[0] for p in parts], np.int32)
    stride = int(n_part.max()) if n else 0
    pin = None
    if stride:
        pin = np.zeros((n, stride, 2), np.float64)
        for i, p in enumerate(parts):
            if p is not None:
                pin[i, :p.shape[0]] = p
    for a in (Kc, Vc):
        if a.dtype != np.float32 or not a.flags.c_contiguous or a.ndim != 2 or a.shape[1] != d or a.shape[0] != Kc.shape[0]:
            raise ValueError("Kc / Vc must be C-contiguous float32 [n_ctx, d]")
    cols = [np.ascontiguousarray([int(s[k]) for s in steps], np.int32) for k in (2, 3, 4)]
    merged = np.full((n, d), np.nan, np.float32)
    wo = np.full((n, max(d // 32, 1), 20), 0xEE, np.uint8) if want_wo else None
    fault = np.full(max(n, 1), 0xFFFFFFFF, np.uint32)
    plans = np.full((max(n, 1), 5), -1, np.int64)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_qkv_attn(_ptr(wq), _ptr(np.ascontiguousarray(norm_w, np.float32)), d, int(H), Kc.shape[0], _ptr(Kc), _ptr(Vc), int(n_threads),
                                    n, _ptr(x), _ptr(pin), _ptr(n_part), stride, _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), int(epoch0) & 0xFFFFFFFF,
                                    int(tagged_in), _ptr(merged), _ptr(wo), _ptr(fault), _ptr(plans), err, len(err))
    _check(rc, err)
    return merged, wo, fault[:n], [tuple(int(v) for v in p) for p in plans[:n]]


def eval_multi_rows(n_ctx: int, n_past, n_tokens, chunk_tokens: int = 0):
    """llamahip_eval_multi_rows (host only): the row table of an eval_multi pass -- (row_seg, row_pos, row_keys) int32 [R] -- or None where the
    arguments are refused."""
    npast = np.ascontiguousarray(n_past, np.int32).ravel()
    nt = np.ascontiguousarray(n_tokens, np.int32).ravel()
    if npast.size != nt.size:
        raise ValueError(f"eval_multi_rows: {npast.size} n_past, {nt.size} n_tokens")
    cap = max(int(np.clip(nt.astype(np.int64), 0, None).sum()), 1)
    seg, pos, keys = (np.full(cap, -1, np.int32) for _ in range(3))
    R = lib().llamahip_eval_multi_rows(int(n_ctx), npast.size, _ptr(npast), _ptr(nt), int(chunk_tokens), _ptr(seg), _ptr(pos), _ptr(keys))
    return None if R < 0 else (seg[:R], pos[:R], keys[:R])


def op_attention_rows(qkv: np.ndarray, H: int, Kc: np.ndarray, Vc: np.ndarray, row_slot, row_pos, row_keys, n_threads: int = 8,
                      merged_stride: int | None = None, merged_init=None, want_wo: bool = True):
    """The row-table attention of eval_multi's pass (llamahip_op_attention_rows): qkv f32 [R, 3d] un-rotated, Kc / Vc f32 [n_slots, n_ctx, d]
    (updated in place).  Returns (merged f32 [R, merged_stride], the wo operand uint8 [R, d/32, 20] or None)."""
    qkv = np.ascontiguousarray(qkv, np.float32)
    R, d3 = qkv.shape
    d = d3 // 3
    for a in (Kc, Vc):
        if a.dtype != np.float32 or not a.flags.c_contiguous or a.ndim != 3 or a.shape[2] != d or a.shape != Kc.shape:
            raise ValueError("Kc / Vc must be C-contiguous float32 [n_slots, n_ctx, d]")
    tab = [np.ascontiguousarray(a, np.int32).ravel() for a in (row_slot, row_pos, row_keys)]
    if any(a.size != R for a in tab):
        raise ValueError(f"op_attention_rows: the table must have R = {R} entries")
    ms = d if merged_stride is None else int(merged_stride)
    merged = np.full((R, ms), np.nan, np.float32) if merged_init is None else np.array(merged_init, np.float32, order="C").reshape(R, ms)
    wo = np.full((R, max(d // 32, 1), 20), 0xEE, np.uint8) if want_wo else None
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_attention_rows(_ptr(qkv), R, d, int(H), Kc.shape[1], Kc.shape[0], _ptr(Kc), _ptr(Vc), _ptr(tab[0]), _ptr(tab[1]),
                                          _ptr(tab[2]), int(n_threads), _ptr(merged), ms, _ptr(wo), err, len(err))
    _check(rc, err)
    return merged, wo


def debug_set_keys(n_ctx: int, max_pos: int) -> int | None:
    """Host-only: the key bucket (set_keys) of a batched decode step whose highest row position is max_pos (llamahip_debug_set_keys);
    None where the arguments are refused."""
    r = lib().llamahip_debug_set_keys(int(n_ctx), int(max_pos))
    return None if r < 0 else r


def op_set_attention(qkv: np.ndarray, H: int, Kc: np.ndarray, Vc: np.ndarray, row_slot, row_pos, n_threads: int = 8, set_keys: int = 0,
                     merged_stride: int | None = None, merged_init=None, want_merged: bool = True, want_wo: bool = True, score_fill: int = 0xFFFFFFFF):
    """The attention of a batched decode step (llamahip_op_set_attention): qkv f32 [B, 3d] un-rotated, Kc / Vc f32 [n_slots, n_ctx, d]
    (updated in place).  want_merged False: the launch gets a null merged (Q4_0 handles).  Returns (merged f32 [B, merged_stride] or None,
    the wo operand uint8 [B, d/32, 20] or None)."""
    qkv = np.ascontiguousarray(qkv, np.float32)
    B, d3 = qkv.shape
    d = d3 // 3
    for a in (Kc, Vc):
        if a.dtype != np.float32 or not a.flags.c_contiguous or a.ndim != 3 or a.shape[2] != d or a.shape != Kc.shape:
            raise ValueError("Kc / Vc must be C-contiguous float32 [n_slots, n_ctx, d]")
    tab = [np.ascontiguousarray(a, np.int32).ravel() for a in (row_slot, row_pos)]
    if any(a.size != B for a in tab):
        raise ValueError(f"op_set_attention: the table must have B = {B} entries")
    ms = d if merged_stride is None else int(merged_stride)
    merged = None
    if want_merged:
        merged = np.full((B, ms), np.nan, np.float32) if merged_init is None else np.array(merged_init, np.float32, order="C").reshape(B, ms)
    wo = np.full((B, max(d // 32, 1), 20), 0xEE, np.uint8) if want_wo else None
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_set_attention(_ptr(qkv), B, d, int(H), Kc.shape[1], Kc.shape[0], _ptr(Kc), _ptr(Vc), _ptr(tab[0]), _ptr(tab[1]),
                                         int(n_threads), int(set_keys), _ptr(merged), ms, _ptr(wo), int(score_fill) & 0xFFFFFFFF, err, len(err))
    _check(rc, err)
    return merged, wo


SET_ENTRY_MODES = ("embed_q4_0", "embed_f16", "embed_f32", "rows")      # LLAMAHIP_SET_ENTRY_* of llamahip.h, in order
SET_EXIT_MODES = ("argmax", "rows_out", "argmax_one")                  # LLAMAHIP_SET_EXIT_*, in order


def op_set_entry(mode, row_pos, emb=None, tokens=None, hid_in=None, epoch_in: int = 0, pass_epoch: bool = False, x_stride: int | None = None, x_init=None):
    """The first launch of a batched decode step (llamahip_op_set_entry).  mode "embed_q4_0" (emb uint8 [V, d/32, 20]), "embed_f16" /
    "embed_f32" (emb [V, d]) with tokens int32 [B]; "rows" with hid_in f32 [B, d].  Returns dict(x f32 [B, x_stride], pos int32 [16] -- the
    descriptor's pos[] --, epoch, state int32 [B, 2], changed: whether anything else moved)."""
    code = SET_ENTRY_MODES.index(mode) if mode in SET_ENTRY_MODES else int(mode)
    row_pos = np.ascontiguousarray(row_pos, np.int32).ravel()
    B = row_pos.size
    V = 0
    if code == 3:
        hid_in = None if hid_in is None else np.ascontiguousarray(hid_in, np.float32)
        d = 0 if hid_in is None else hid_in.shape[1]
        if hid_in is not None and hid_in.shape[0] != B:
            raise ValueError(f"op_set_entry: {hid_in.shape[0]} hid_in rows for {B} positions")
    else:
        if emb is not None:
            emb = np.ascontiguousarray(emb, (np.uint8, np.float16, np.float32)[code] if code in (0, 1, 2) else None)
            V, d = emb.shape[0], emb.shape[1] * (32 if code == 0 else 1)
        else:
            d = 32
        tokens = None if tokens is None else np.ascontiguousarray(tokens, np.int32).ravel()
        if tokens is not None and tokens.size != B:
            raise ValueError(f"op_set_entry: {tokens.size} tokens for {B} positions")
    xs = d if x_stride is None else int(x_stride)
    x = np.full((B, max(xs, 0)), np.nan, np.float32) if x_init is None else np.array(x_init, np.float32, order="C").reshape(B, xs)
    pos, state = np.full(16, -2, np.int32), np.full((max(B, 1), 2), -2, np.int32)
    epoch, changed = C.c_uint32(0), C.c_int32(-1)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_set_entry(code, _ptr(emb) if code != 3 else None, V, d, _ptr(tokens) if code != 3 else None, _ptr(hid_in) if code == 3 else None, B,
                                     _ptr(row_pos), int(epoch_in) & 0xFFFFFFFF, int(bool(pass_epoch)), _ptr(x), xs, _ptr(pos), C.byref(epoch), _ptr(state),
                                     C.byref(changed), err, len(err))
    _check(rc, err)
    return dict(x=x, pos=pos, epoch=epoch.value, state=state, changed=bool(changed.value))


def op_set_exit(mode, row_pos, row_step, n_ctx: int, logits=None, x=None, tok_out_null=None):
    """The last launches of a batched decode step (llamahip_op_set_exit).  mode "argmax" / "argmax_one" on logits f32 [B, V]; "rows_out" on
    x f32 [B, d].  Returns dict(trace int32 [B, n_ctx] (started as -1), tok_out int32 [B] (-1: not written), hid_out f32 [B, d] or None,
    state int32 [B, 2])."""
    code = SET_EXIT_MODES.index(mode) if mode in SET_EXIT_MODES else int(mode)
    row_pos = np.ascontiguousarray(row_pos, np.int32).ravel()
    row_step = np.ascontiguousarray(row_step, np.int32).ravel()
    B = row_pos.size
    if row_step.size != B:
        raise ValueError(f"op_set_exit: {row_step.size} steps for {B} positions")
    null = np.zeros(B, np.int32) if tok_out_null is None else np.ascontiguousarray(tok_out_null, np.int32).ravel()
    if null.size != B:
        raise ValueError(f"op_set_exit: {null.size} tok_out flags for {B} rows")
    V = d = 0
    hid = None
    if logits is not None:
        logits = np.ascontiguousarray(logits, np.float32).reshape(B, -1)
        V = logits.shape[1]
    if x is not None:
        x = np.ascontiguousarray(x, np.float32).reshape(B, -1)
        d = x.shape[1]
        hid = np.full((B, d), np.nan, np.float32)
    trace = np.full((B, max(int(n_ctx), 1)), -1, np.int32)
    tok, state = np.full(B, -2, np.int32), np.full((B, 2), -2, np.int32)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_set_exit(code, _ptr(logits), V, _ptr(x), d, B, int(n_ctx), _ptr(row_pos), _ptr(row_step), _ptr(null), _ptr(trace), _ptr(tok),
                                    _ptr(hid), _ptr(state), err, len(err))
    _check(rc, err)
    return dict(trace=trace, tok_out=tok, hid_out=hid, state=state)


def op_kv_shift(Kc: np.ndarray, Vc: np.ndarray, dh: int, shifts) -> None:
    """One k_kv_shift_rows launch (llamahip_op_kv_shift; NOT the reference's arithmetic) on Kc / Vc f32 [n_slots, n_layers, n_ctx, d], updated
    in place: shifts = [(slot, first row, row count, n_discard), ...] as Model.kv_shift_rows takes them; the angle table is rope_table(n_ctx, dh)."""
    for a in (Kc, Vc):
        if a.dtype != np.float32 or not a.flags.c_contiguous or a.ndim != 4 or a.shape != Kc.shape:
            raise ValueError("Kc / Vc must be C-contiguous float32 [n_slots, n_layers, n_ctx, d]")
    c = np.ascontiguousarray(shifts, np.int32).reshape(-1, 4)
    cols = [np.ascontiguousarray(c[:, k]) for k in range(4)]
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_kv_shift(_ptr(Kc), _ptr(Vc), Kc.shape[0], Kc.shape[1], Kc.shape[2], Kc.shape[3], int(dh), len(c), *(_ptr(a) for a in cols), err, len(err))
    _check(rc, err)


def rope_table(n_ctx: int, dh: int) -> np.ndarray:
    """Host-only: the library's RoPE angle table float64 [n_ctx, dh // 2, 2] = (cos, sin) (llamahip_debug_rope_table)."""
    if n_ctx < 1 or dh < 2 or dh % 2:
        raise ValueError(f"rope_table: n_ctx {n_ctx} >= 1 and an even head size {dh} >= 2")
    out = np.empty((n_ctx, dh // 2, 2), np.float64)
    if lib().llamahip_debug_rope_table(int(n_ctx), int(dh), _ptr(out)) != 0:
        raise ValueError("llamahip_debug_rope_table refused its arguments")
    return out


def debug_attn_path(N: int, head_size: int, n_past: int, n_threads: int, n_ctx: int) -> str | None:
    """Host-only: the attention path a model's multi-row eval takes for the shape (llamahip_debug_attn_path); None for one row."""
    r = lib().llamahip_debug_attn_path(N, head_size, n_past, n_threads, n_ctx)
    return None if r < 0 else ATTN_PATHS[r]


PREP_MODES = {"plain": 1, "norm": 2, "silu_mul": 3}      # LLAMAHIP_PREP_* of llamahip.h
PREP_KERNELS = ("auto", "fast", "lds")                    # LLAMAHIP_PREP_KERNEL_*, in order


def op_prep(mode: str, buf: np.ndarray, K: int, N: int, in_stride: int | None = None, in0_offset: int = 0, in1_offset: int = 0,
            in1_stride: int = 0, kernel: str = "auto", want_y: bool = False, qa_rows: int | None = None, fill: int = 0xFF):
    """One activation-preparation launch (llamahip_op_prep).  buf: ONE float32 buffer holding every operand as the caller laid it out: in0
    rows at in0_offset + n * in_stride (default stride K); in1 = the K norm weights at in1_offset ("norm") or rows at in1_offset + n *
    in1_stride ("silu_mul").  Returns (qa_A uint32 [qa_rows, Kp/4], qa_d float32 [qa_rows, Kp/32], y float32 [N, K] or None, the kernel
    taken): the raw operand buffers as the device left them, every byte `fill` where the launch wrote nothing (y: likewise)."""
    buf = np.ascontiguousarray(buf, np.float32).ravel()
    Kp = (int(K) + 255) // 256 * 256
    rows = int(N) if qa_rows is None else int(qa_rows)
    qa_A = np.full((max(rows, 0), Kp // 4), fill * 0x01010101, np.uint32)
    qa_d = np.full((max(rows, 0), Kp // 32), fill * 0x01010101, np.uint32).view(np.float32)
    y = np.full((max(int(N), 0), max(int(K), 0)), fill * 0x01010101, np.uint32).view(np.float32) if want_y else None
    mcode = PREP_MODES[mode] if mode in PREP_MODES else int(mode)
    kcode = PREP_KERNELS.index(kernel) if kernel in PREP_KERNELS else int(kernel)
    taken = C.c_int32(-1)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_prep(mcode, kcode, _ptr(buf), buf.size, int(in0_offset), int(K if in_stride is None else in_stride), int(in1_offset),
                                int(in1_stride), int(K), int(N), _ptr(qa_A), _ptr(qa_d), rows, _ptr(y), C.byref(taken), err, len(err))
    _check(rc, err)
    return qa_A, qa_d, y, PREP_KERNELS[taken.value]


GEMV_PRE = {"qa": 0, "plain": 1, "norm": 2, "silu_mul": 3}      # LLAMAHIP_GEMV_PRE_* of llamahip.h
GEMV_EPI = {"store": 0, "resid": 1, "silu_qa": 2}                # LLAMAHIP_GEMV_EPI_*


def op_gemv_q4_0(wq: np.ndarray, pre, epi, in0, in1=None, resid=None, interleaved: bool = False, part_in=None, n_part_in: int | None = None,
                 y_init=None, want_y: bool = True, out_rows: int = 2, out_fill: int = 0xFF, part_out=None, n_part_out: int | None = None):
    """One launch of the single-row decode mat-vec (llamahip_op_gemv_q4_0).  wq uint8 [M, K/32, 20] in file layout (interleaved: w1's F rows
    then w3's); pre / epi: a name of GEMV_PRE / GEMV_EPI or the library's own code; in0 / in1 / resid float32 as the pair takes them;
    part_in float64 [n, 2]; y_init: the y buffer before the launch (default: NaN, one float per output); part_out: the buffer of pairs
    before the launch (float64 [cap, 2]), n_part_out of which the launch is told about (default: all).  Returns dict(y, out_A, out_d,
    part_out, plan): the buffers as the device left them (out_A / out_d [out_rows, Fp/4] / [out_rows, Fp/32] start as `out_fill` bytes with
    the padded blocks of row 0 zero, as a model's workspace has them), plan = (nw, pg, depth, ring, grid, lds)."""
    wq = np.ascontiguousarray(wq, np.uint8)
    M, nb, _ = wq.shape
    K = nb * 32
    pcode = GEMV_PRE[pre] if pre in GEMV_PRE else int(pre)
    ecode = GEMV_EPI[epi] if epi in GEMV_EPI else int(epi)
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ravel()
    in0, in1, resid = f32(in0), f32(in1), f32(resid)
    silu_qa = ecode == GEMV_EPI["silu_qa"]
    F = M // 2
    y = None
    if want_y or y_init is not None:
        y = np.full(F if silu_qa else M, np.nan, np.float32) if y_init is None else np.array(y_init, np.float32, order="C").ravel()
    out_A = out_d = None
    if silu_qa:
        Fp = (F + 255) // 256 * 256
        out_A = np.full((out_rows, Fp // 4), out_fill * 0x01010101, np.uint32)
        out_d = np.full((out_rows, Fp // 32), out_fill * 0x01010101, np.uint32)
        for b in range(F // 32, Fp // 32 if out_rows > 0 else 0):      # (dword (c * 8 + k) * 8 + j holds chain k of block c * 8 + j)
            out_d[0, b] = 0
            out_A[0].reshape(Fp // 256, 8, 8)[b >> 3, :, b & 7] = 0
        out_d = out_d.view(np.float32)
    pin = None if part_in is None else np.ascontiguousarray(part_in, np.float64).reshape(-1, 2)
    npin = (0 if pin is None else pin.shape[0]) if n_part_in is None else int(n_part_in)
    pout = None if part_out is None else np.array(part_out, np.float64, order="C").reshape(-1, 2)
    cap = 0 if pout is None else pout.shape[0]
    npout = cap if n_part_out is None else int(n_part_out)
    plan = np.zeros(6, np.int64)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_gemv_q4_0(_ptr(wq), M, K, int(interleaved), pcode, ecode, _ptr(in0), _ptr(in1), _ptr(pin), npin, _ptr(resid),
                                     _ptr(y), 0 if y is None else y.size, _ptr(out_A), _ptr(out_d), int(out_rows), _ptr(pout), npout, cap,
                                     _ptr(plan), err, len(err))
    _check(rc, err)
    return dict(y=y, out_A=out_A, out_d=out_d, part_out=pout, plan=tuple(int(v) for v in plan))


GEMV_SET_EPI = {"store": 0, "resid": 1, "silu_qa": 2, "rope_kv": 3, "silu_qah": 7}      # LLAMAHIP_GEMV_EPI_*


def op_gemv_set_q4_0(wq: np.ndarray, epi, x, force=None, interleaved: bool = False, resid=None, y_init=None, y_stride: int | None = None,
                     d: int = 0, dh: int = 0, n_ctx: int = 0, n_slots: int = 1, n_past: int = 0, row_pos=None, row_slot=None,
                     qr_init=None, Kc=None, Vc=None, out_A=None, out_d=None, layer: int = 0, x_prev=None):
    """One launch of the few-row mat-mul k_gemv_set (llamahip_op_gemv_set_q4_0).  wq uint8 [M, K/32, 20] in file layout (interleaved: w1's F
    rows then w3's); epi: a name of GEMV_SET_EPI or the library's own code; x float32 [N, K]; force None (the library's rule) or
    (nc, cw[, rgw]).  store / resid: resid [N, M], y_init [N, y_stride] (default NaN).  rope_kv: d, dh, n_ctx, n_slots, n_past or
    row_pos / row_slot [N], qr_init [N, d] (default NaN), Kc / Vc [n_slots, n_ctx, d] (copied, not modified).  silu_qa / silu_qah: out_A
    uint32 [rows, Fp/4] / out_d float32 or uint32 [rows, Fp/32] as the buffers are before the launch (copied); layer; x_prev [N, K].
    Returns dict(y, qr, Kc, Vc, out_A, out_d (uint32 view kept as float32), fault, plan): the buffers as the device left them,
    plan = (nc, cw, ncg, rgw, lds, grid, threads)."""
    wq = np.ascontiguousarray(wq, np.uint8)
    M, nb, _ = wq.shape
    K = nb * 32
    ecode = GEMV_SET_EPI[epi] if epi in GEMV_SET_EPI else int(epi)
    x = None if x is None else np.ascontiguousarray(x, np.float32)
    N = 0 if x is None else (x.shape[0] if x.ndim == 2 else 1)
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    i32a = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ravel()
    resid, x_prev, row_pos, row_slot = f32(resid), f32(x_prev), i32a(row_pos), i32a(row_slot)
    fc = None
    if force is not None:
        fc = np.zeros(3, np.int32)
        fc[:len(force)] = force
    y = qr = None
    ys = M if y_stride is None else int(y_stride)
    if ecode in (0, 1):
        y = np.full((N, max(ys, 0)), np.nan, np.float32) if y_init is None else np.array(y_init, np.float32, order="C")
    if ecode == 3:
        qr = np.full((N, max(d, 0)), np.nan, np.float32) if qr_init is None else np.array(qr_init, np.float32, order="C")
        Kc = None if Kc is None else np.array(Kc, np.float32, order="C")
        Vc = None if Vc is None else np.array(Vc, np.float32, order="C")
    else:
        Kc = Vc = None
    out_rows = 0
    if ecode in (2, 7):
        out_A = None if out_A is None else np.array(out_A, np.uint32, order="C")
        out_d = None if out_d is None else np.array(np.asarray(out_d).view(np.float32), np.float32, order="C")
        out_rows = 0 if out_A is None else out_A.shape[0]
    else:
        out_A = out_d = None
    fault = np.full(1, 0xFFFFFFFF, np.uint32)
    plan = np.zeros(7, np.int64)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_gemv_set_q4_0(_ptr(wq), M, K, int(interleaved), ecode, _ptr(x), N, _ptr(fc), _ptr(resid), _ptr(y), ys,
                                         int(d), int(dh), int(n_ctx), int(n_slots), int(n_past), _ptr(row_pos), _ptr(row_slot), _ptr(qr), _ptr(Kc), _ptr(Vc),
                                         _ptr(out_A), _ptr(out_d), out_rows, int(layer), _ptr(x_prev), _ptr(fault), _ptr(plan), err, len(err))
    _check(rc, err)
    return dict(y=y, qr=qr, Kc=Kc, Vc=Vc, out_A=out_A, out_d=out_d, fault=int(fault[0]) if ecode == 7 else None, plan=tuple(int(v) for v in plan))


def qa_to_blocks(qa_A: np.ndarray, qa_d: np.ndarray, N: int, K: int) -> np.ndarray:
    """Host-only: rows 0 .. N-1 of a raw QA operand (op_prep) -> uint8 [N, K/32, 20] Q4_0 blocks in file layout (llamahip_debug_qa_to_blocks)."""
    qa_A, qa_d = np.ascontiguousarray(qa_A, np.uint32), np.ascontiguousarray(qa_d, np.float32)
    Kp = (K + 255) // 256 * 256
    if qa_A.size < N * Kp // 4 or qa_d.size < N * Kp // 32:
        raise ValueError(f"qa_to_blocks: {qa_A.size} dwords / {qa_d.size} scales for {N} rows of K {K}")
    out = np.empty((N, K // 32, 20), np.uint8)
    if lib().llamahip_debug_qa_to_blocks(_ptr(qa_A), _ptr(qa_d), N, K, _ptr(out)) != 0:
        raise ValueError(f"qa_to_blocks: bad arguments (N {N}, K {K})")
    return out


def op_embed(tokens, emb: np.ndarray, x_stride: int | None = None, x_init=None, want_stats: bool = False):
    """The embedding gather (llamahip_op_embed): tokens int32 [N], emb uint8 [V, d/32, 20] -> x float32 [N, x_stride] as the device left it
    (x_init, default NaN, where nothing was written).  want_stats (N = 1): k_embed_part instead of k_embed; returns (x, float64 [2])."""
    tokens = np.ascontiguousarray(tokens, np.int32).ravel()
    emb = np.ascontiguousarray(emb, np.uint8)
    V, nb, _ = emb.shape
    d, N = nb * 32, tokens.size
    xs = d if x_stride is None else int(x_stride)
    x = np.full((N, max(xs, 0)), np.nan, np.float32) if x_init is None else np.array(x_init, np.float32, order="C").reshape(N, xs)
    stats = np.full(2, np.nan, np.float64) if want_stats else None
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_embed(_ptr(tokens), N, _ptr(emb), V, d, _ptr(x), xs, _ptr(stats), err, len(err))
    _check(rc, err)
    return (x, stats) if want_stats else x


DENSE_PREP_KERNELS = ("auto", "fused", "split")          # LLAMAHIP_DENSE_PREP_*, in order
DENSE_XP_GUARD = 64                                       # floats behind row N - 1 of op_dense_prep's operand


def op_dense_prep(mode: str, wtype: int, buf: np.ndarray, K: int, N: int, in_stride: int | None = None, in0_offset: int = 0, in1_offset: int = 0,
                  in1_stride: int = 0, kernel: str = "auto", xp_init=None):
    """The activation operand of an f16 / f32 mat-mul (llamahip_op_dense_prep).  buf and the offsets / strides as op_prep takes them; wtype 1
    (fp16 weights) or 0 (fp32).  Returns (xp float32 [N * K + DENSE_XP_GUARD], the kernel taken): the operand rows in the kernels' permuted
    order followed by the guard floats, as the device left them -- xp_init (default: 0xFF in every byte) wherever nothing was written."""
    buf = np.ascontiguousarray(buf, np.float32).ravel()
    n = max(int(N), 0) * max(int(K), 0) + DENSE_XP_GUARD
    xp = np.full(n, 0xFFFFFFFF, np.uint32).view(np.float32) if xp_init is None else np.array(xp_init, np.float32, order="C").reshape(n)
    mcode = PREP_MODES[mode] if mode in PREP_MODES else int(mode)
    kcode = DENSE_PREP_KERNELS.index(kernel) if kernel in DENSE_PREP_KERNELS else int(kernel)
    taken = C.c_int32(-1)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_dense_prep(mcode, int(wtype), kcode, _ptr(buf), buf.size, int(in0_offset), int(K if in_stride is None else in_stride),
                                      int(in1_offset), int(in1_stride), int(K), int(N), _ptr(xp), C.byref(taken), err, len(err))
    _check(rc, err)
    return xp, DENSE_PREP_KERNELS[taken.value]


def op_embed_dense(tokens, emb: np.ndarray, x_stride: int | None = None, x_init=None, wtype: int | None = None):
    """The embedding gather of an f16 / f32 / Q4_1 file (llamahip_op_embed_dense): tokens int32 [N]; emb float32 / float16 [V, d] (wtype 0 / 1)
    or uint8 [V, d/32 * 24] Q4_1 rows in file layout (wtype 3); wtype overrides what the dtype implies.  Returns x float32 [N, x_stride] as
    the device left it (x_init, default NaN, where nothing was written)."""
    tokens = np.ascontiguousarray(tokens, np.int32).ravel()
    emb = np.ascontiguousarray(emb)
    if emb.dtype not in (np.float16, np.float32, np.uint8):
        emb = emb.astype(np.float32)
    wt = {np.dtype(np.float32): 0, np.dtype(np.float16): 1, np.dtype(np.uint8): 3}[emb.dtype] if wtype is None else int(wtype)
    V = emb.shape[0]
    d = emb.shape[1] // 24 * 32 if emb.dtype == np.uint8 else emb.shape[1]
    N = tokens.size
    xs = d if x_stride is None else int(x_stride)
    x = np.full((N, max(xs, 0)), np.nan, np.float32) if x_init is None else np.array(x_init, np.float32, order="C").reshape(N, xs)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_embed_dense(_ptr(tokens), N, _ptr(emb), wt, V, d, _ptr(x), xs, err, len(err))
    _check(rc, err)
    return x


def op_quantize_row_q4_0(x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32).ravel()
    out = np.empty(x.size // 32 * 20, np.uint8)
    err = C.create_string_buffer(1024)
    rc = lib().llamahip_op_quantize_row_q4_0(_ptr(x), x.size, _ptr(out), err, len(err))
    _check(rc, err)
    return out
