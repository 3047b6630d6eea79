"""llama.swift_amd -- MI355X (gfx950) drop-in for the quantized-LLaMA hot path of
alexrozanski/llama.swift.

The product is ``csrc/libllamahip.so`` (hand-written HIP kernels behind the C ABI of
``include/llamahip.h``).  This package is only the thin host-side glue the tests and the benchmark
use: a ctypes binding of that C ABI (:mod:`.binding`) and a Python mirror of the reference's Swift
surface ``LlamaRunner`` / ``Config`` / ``RunState`` (:mod:`.runner`,
Sources/llama/LlamaRunner.swift:11-124).

There is no CPU fallback: importing works anywhere (so the symbol table can be checked without a
GPU), but every compute call fails loudly if the shared library or a HIP device is missing.

The directory is literally named ``llama.swift_amd``; import it as ``llama_swift_amd`` through the
shim module at the repository root.
"""
from .binding import (  # noqa: F401
    CTX_REEVAL,
    DEC_ATTN_KERNELS,
    DEC_ATTN_PATHS,
    DecAttnPlan,
    CTX_SHIFT,
    KV_SHIFT_MAX,
    KV_SHIFT_ROWS_IN_FLIGHT,
    LIB_PATH,
    LlamaHipError,
    Model,
    POOL_LAST,
    POOL_MEAN,
    SCORE_CHOICES_MAX,
    Sampler,
    Scheduler,
    bench_gemv_names,
    build,
    ctx_overflow_plan,
    debug_attn_path,
    dec_attn_plan,
    declared_symbols,
    dense_paths,
    dense_set_plan,
    dense_mfma_plan,
    dense_mfma_launches,
    dense_force,
    eval_multi_rows,
    gemm_paths,
    lib,
    live_allocs,
    lookup_deal_rows,
    lookup_draft,
    op_attention,
    op_attention_rows,
    op_dec_attention,
    op_embed,
    op_gemv_q4_0,
    op_gemv_set_q4_0,
    op_kv_shift,
    op_logprob,
    op_mul_mat_dense,
    op_pool_rows,
    op_mul_mat_q4_1,
    op_mul_mat_q4_0,
    op_prep,
    op_prompt_gemm_q4_0,
    op_qkv_attn,
    op_quantize_row_q4_0,
    op_sched_accept,
    op_sched_pick,
    op_topk,
    op_topk_rows,
    op_topk_slide,
    op_topk_slide_set,
    op_verify_rows,
    op_verify_rows_set,
    q41_paths,
    q41_plan,
    qa_to_blocks,
    qkv_attn_plan,
    quantize_file,
    rope_table,
    sched_event_cap,
    sched_plan,
    sched_plan_drafts,
    sched_plan_prefix,
    gemv_plan,
    set_plan,
    version,
)
from .runner import Config, LlamaRunner, RunState  # noqa: F401
