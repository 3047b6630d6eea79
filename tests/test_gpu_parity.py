"""GPU (-m gpu): the HIP path, called through the C ABI, against (a) the committed golden vectors
produced by the reference build, (b) the oracle on seeded inputs, (c) size-independent properties at
the full LLaMA-7B size.  Everything is compared BIT FOR BIT (fp32 logits included): the kernels
reproduce the arithmetic order of the reference's AVX2 build, so the tolerance the north star allows
(1e-3 on logits) is not needed; the only documented exception is the double-precision sum order in
the norm statistics: tests/test_gpu_prep.py shows for its rows that no summation order can
change a float (and requires bit-equality there), and bounds a row where it can."""
import os

import numpy as np
import pytest

import refgolden
import synth
from conftest import synth_tool

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def describe(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return f"shape {a.shape} vs {b.shape}"
    bad = np.flatnonzero(a.ravel() != b.ravel())
    return f"{bad.size}/{a.size} differ, first at {bad[:4]}, got {a.ravel()[bad[:3]]} want {b.ravel()[bad[:3]]}"


# ------------------------------------------------------------------------------------------------ golden vectors
def test_quantizer_golden(L):
    g = np.load(os.path.join(G, "q4_blocks.npz"))
    x = g["x"]
    got = L.op_quantize_row_q4_0(x.reshape(-1)).reshape(len(x), 20)
    assert same(got, g["runtime_q"]), describe(got, g["runtime_q"])


@pytest.mark.parametrize("tag", list("abcde"))
def test_mul_mat_golden(L, tag):
    g = np.load(os.path.join(G, "mul_mat.npz"))
    y = L.op_mul_mat_q4_0(g[f"{tag}_w"], g[f"{tag}_x"])
    assert same(y, g[f"{tag}_y"]), describe(y, g[f"{tag}_y"])


@pytest.mark.parametrize("nth", [1, 8])
@pytest.mark.parametrize("flags", [0, 1, 3])          # graph+fused, eager+fused, eager+unfused
def test_tiny_model_golden(L, tmp_path, nth, flags):
    g = np.load(os.path.join(G, "tiny_model.npz"))
    path = str(tmp_path / "tiny.bin")
    g["model_file"].tofile(path)
    with L.Model(path, n_ctx=int(g["n_ctx"][0]), flags=flags) as m:
        assert same(m.eval(np.array([0, 1, 2, 3], np.int32), 0, nth), g[f"nth{nth}_warmup_logits"])
        r = m.eval_debug(g["prompt"], 0, nth, dump_layer=1)
        for k, v in r.items():
            assert same(v, g[f"nth{nth}_prompt_{k}"]), f"{k}: " + describe(v, g[f"nth{nth}_prompt_{k}"])
        tok, n_past = int(np.argmax(r["logits"])), 9
        for i in range(16):                                # host-driven single-token evals
            lg = m.eval(np.array([tok], np.int32), n_past, nth)
            assert same(lg, g[f"nth{nth}_decode_logits"][i]), f"decode step {i}: " + describe(lg, g[f"nth{nth}_decode_logits"][i])
            tok = int(np.argmax(lg)); n_past += 1
        k, v = m.kv(1, n_past)
        assert same(k, g[f"nth{nth}_kcache_l1"]) and same(v, g[f"nth{nth}_vcache_l1"])
    with L.Model(path, n_ctx=64, flags=flags) as m:       # device-resident greedy loop
        lg = m.eval(g["prompt"], 0, nth)
        toks, last = m.decode_greedy(int(np.argmax(lg)), 9, 16, nth, want_logits=True)
        assert toks.tolist() == g[f"nth{nth}_greedy_tokens"].tolist()
        assert same(last, g[f"nth{nth}_decode_logits"][15])


# ------------------------------------------------------------------------------------------------ oracle, seeded inputs
@pytest.mark.parametrize("M,K,N", [(8, 64, 1), (40, 256, 1), (64, 704, 2), (256, 4096, 1), (256, 4096, 9), (64, 11008, 1),
                                   (64, 11008, 5), (24, 5120, 3), (16, 8192, 1), (100, 4096, 17), (8, 13824, 1), (8, 22016, 2),
                                   (520, 4096, 32), (72, 11008, 13), (40, 22016, 4), (2056, 4096, 8),
                                   # every (columns per wave, waves per row-group) plan of the few-row kernel (k_gemv_set): small matrices ...
                                   (264, 4096, 3), (264, 4096, 4), (264, 4096, 6), (264, 4096, 7), (264, 4096, 11), (264, 4096, 16), (200, 11008, 9), (136, 1280, 12),
                                   # ... and matrices with >= 1 024 row-groups (two columns per wave up to four rows)
                                   (8200, 512, 2), (8200, 512, 3), (8200, 768, 4),
                                   # ... more rows on those: up to five columns per wave, then column groups at grid level (5: one group, 7: 4 + 3, 9: 5 + 4, 16: 4 x 4)
                                   (8200, 512, 5), (8200, 512, 7), (8200, 512, 9), (8200, 768, 16),
                                   # ... the row-group classes in between (768 .. 1 535 row-groups: two waves per row-group) and wider K
                                   (6200, 1280, 6), (6200, 1280, 8), (6200, 1792, 10), (12296, 1024, 9)])
def test_mul_mat_vs_oracle(L, oracle, M, K, N):
    rng = np.random.default_rng(M + K + N)
    w = synth.quantize_q4_0_offline((0.02 * rng.standard_normal((M, K))).astype(np.float32))
    x = (rng.standard_normal((N, K)) * rng.uniform(0.1, 4)).astype(np.float32)
    x[0, :32] = 0                                          # an all-zero activation block (d = 0, id = 0)
    got, want = L.op_mul_mat_q4_0(w, x), oracle.mul_mat_q4_0(w, x, 8)
    assert same(got, want), describe(got, want)


@pytest.mark.parametrize("parts,nth", [(1, 8), (2, 3), (4, 64)])
def test_model_vs_oracle_with_multipart_files(L, oracle, tmp_path, parts, nth):
    hp = synth.HParams(n_vocab=160, n_embd=512, n_mult=256, n_head=4, n_layer=3)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=100 + parts), n_parts=parts)
    om = oracle.load(path, 96, parts)
    with L.Model(path, n_ctx=96, n_parts=parts) as gm:
        assert gm.n_parts == parts
        toks = synth.synth_prompt(40, hp.n_vocab, seed=parts)
        n_past = 0
        for chunk in (toks[:9], toks[9:18], toks[18:22], toks[22:39], toks[39:40]):     # 9, 9, 4, 17, 1 tokens
            a = gm.eval_debug(chunk, n_past, nth, dump_layer=2)
            b = om.eval(chunk, n_past, nth, all_logits=True, dump_layer=2)
            for k in b:
                assert same(a[k], b[k]), f"n_past {n_past} {k}: " + describe(a[k], b[k])
            n_past += len(chunk)
        tok = int(np.argmax(b["logits"]))
        want = []
        t = tok
        for i in range(24):
            lo = om.eval(np.array([t], np.int32), n_past + i, nth)["logits"]
            t = int(np.argmax(lo)); want.append(t)
        got = gm.decode_greedy(tok, n_past, 24, nth)
        assert got.tolist() == want
        for il in range(hp.n_layer):
            gk, gv = gm.kv(il, n_past + 23)
            ok, ov = om.kv(il, n_past + 23)
            assert same(gk, ok) and same(gv, ov), f"KV cache layer {il}"


def test_long_prompt_in_one_eval(L, oracle, tmp_path):
    """n_ctx is a load parameter here (the reference hard-codes 512, .mm:790): a 1100-token prompt in a
    single eval (k_gemm_rows column groups, three 512-row batches of k_attnq_* over up to 1100 keys), then
    decode at the far end of a 1280-token context."""
    hp = synth.HParams(n_vocab=256, n_embd=256, n_mult=64, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=77))
    om = oracle.load(path, 1280)
    with L.Model(path, n_ctx=1280) as gm:
        prompt = synth.synth_prompt(1100, hp.n_vocab, seed=8)
        a = gm.eval_debug(prompt, 0, 8, all_logits=True)
        b = om.eval(prompt, 0, 8, all_logits=True)
        assert same(a["logits_all"], b["logits_all"]), describe(a["logits_all"], b["logits_all"])
        tok = int(np.argmax(b["logits"]))
        want, t = [], tok
        for i in range(40):
            lo = om.eval(np.array([t], np.int32), 1100 + i, 8)["logits"]
            t = int(np.argmax(lo)); want.append(t)
        got, last = gm.decode_greedy(tok, 1100, 40, 8, want_logits=True)
        assert got.tolist() == want and same(last, lo)


@pytest.mark.parametrize("nth", [8, 3, 5])
def test_prompt_continuation_and_ragged_batches(L, oracle, tmp_path, nth):
    """The many-row prompt kernels (row-per-lane GEMM, lane = query attention) away from the easy case:
    evals that start at n_past > 0, row counts that are not multiples of the 64-query blocks or of the
    GEMM column groups, a row count just under / over the per-row-kernel threshold (32), thread counts
    whose V*P key split is uneven, then decode on top of that cache.  Also the handle without the
    second weight copy (LLAMAHIP_FLAG_NO_PREFILL_COPY = 8: LDS-staged GEMM) must agree bit for bit."""
    hp = synth.HParams(n_vocab=128, n_embd=256, n_mult=64, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=123))
    om = oracle.load(path, 400)
    prompt = synth.synth_prompt(330, hp.n_vocab, seed=3)
    with L.Model(path, n_ctx=400) as gm, L.Model(path, n_ctx=400, flags=8) as gl:
        n_past = 0
        for n in (31, 33, 100, 2, 64, 97):                  # 327 tokens in ragged pieces
            chunk = prompt[n_past:n_past + n]
            a = gm.eval_debug(chunk, n_past, nth, all_logits=True)
            b = om.eval(chunk, n_past, nth, all_logits=True)
            c = gl.eval_debug(chunk, n_past, nth, all_logits=True)
            assert same(a["logits_all"], b["logits_all"]), (n_past, n, describe(a["logits_all"], b["logits_all"]))
            assert same(c["logits_all"], b["logits_all"]), (n_past, n, "no prefill copy")
            n_past += n
        for il in range(hp.n_layer):
            gk, gv = gm.kv(il, n_past)
            ok, ov = om.kv(il, n_past)
            assert same(gk, ok) and same(gv, ov), f"kv cache layer {il}"
        tok, want = int(np.argmax(b["logits"])), []
        t = tok
        for i in range(12):
            lo = om.eval(np.array([t], np.int32), n_past + i, nth)["logits"]
            t = int(np.argmax(lo)); want.append(t)
        assert gm.decode_greedy(tok, n_past, 12, nth).tolist() == want


@pytest.mark.parametrize("shape,nth,chunk,n_prompt", [("small", 8, 9, 23), ("small", 3, 9, 200), ("small_dh64", 5, 4, 77), ("small_dh64", 8, 9, 30),
                                                     ("7b_width", 8, 9, 23), ("7b_width", 8, 9, 150), ("7b_width", 3, 9, 197), ("7b_width", 8, 5, 131)])
def test_prompt_chunks_in_one_pass_vs_chunk_by_chunk_oracle(L, oracle, tmp_path, shape, nth, chunk, n_prompt):
    """llamahip_eval_chunks: the reference's prompt loop -- successive llama_eval calls of n_batch + 1 = 9 tokens (.mm:880-888) -- as ONE
    pass over all rows.  The KV cache of every layer and the logits after the last token must be bit for bit what the chunk-by-chunk
    evals of the oracle leave behind: the one eval-dependent piece of arithmetic, the V*P key split over n_threads (ggml.c:5459-5480),
    is applied per row.  Starts at n_past = 4 behind a 4-token eval (the warm-up of the reference's driver), row counts on both sides of
    the per-row / lane-per-query attention threshold (60) and of the 64-query blocks, ragged last chunk, uneven thread counts, another
    chunk size; head size 128 (matrix-core attention kernels) and 64 (per-row kernels); decode on top of the cache."""
    if shape != "7b_width":
        hp = synth.HParams(n_vocab=128, n_embd=256, n_mult=64, n_head=2 if shape == "small" else 4, n_layer=2)
        path = str(tmp_path / "m.bin")
        synth.write_model(path, hp, synth.random_tensors(hp, seed=77))
        n_vocab, n_layer = hp.n_vocab, hp.n_layer
    else:
        path = synth_tool(tmp_path / "m.bin", seed=13, n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=2)
        n_vocab, n_layer = 512, 2
    n_ctx = n_prompt + 24
    om = oracle.load(path, n_ctx)
    prompt = synth.synth_prompt(n_prompt, n_vocab, seed=5)
    warm = np.array([0, 1, 2, 3], np.int32)
    om.eval(warm, 0, nth)
    n_past = 4
    for c0 in range(0, n_prompt, chunk):
        want = om.eval(prompt[c0:c0 + chunk], n_past + c0, nth)["logits"]
    with L.Model(path, n_ctx=n_ctx) as gm:
        gm.eval(warm, 0, nth)
        got = gm.eval_chunks(prompt, n_past, chunk, nth)
        assert same(got, want), describe(got, want)
        T = n_past + n_prompt
        for il in range(n_layer):
            gk, gv = gm.kv(il, T)
            ok, ov = om.kv(il, T)
            assert same(gk, ok) and same(gv, ov), f"kv cache layer {il}"
        tok, seq = int(np.argmax(want)), []
        t = tok
        for i in range(6):
            lo = om.eval(np.array([t], np.int32), T + i, nth)["logits"]
            t = int(np.argmax(lo)); seq.append(t)
        assert gm.decode_greedy(tok, T, 6, nth).tolist() == seq
        # and the one-pass eval of the same rows as ONE eval differs from it where the split differs (the test would be vacuous otherwise)
        if n_prompt > 60 and nth > 1:
            with L.Model(path, n_ctx=n_ctx) as g1:
                g1.eval(warm, 0, nth)
                one = g1.eval(prompt, n_past, nth)
                assert not same(one, want)


@pytest.mark.parametrize("nth", [1, 4, 8])
def test_short_chunks_vs_oracle(L, oracle, tmp_path, nth):
    """The reference feeds a prompt n_batch = 8 tokens at a time, so short evals are THE prompt path of the
    drop-in: 2..60 rows take the few-row kernel (k_gemv_set, with RoPE + KV append and
    SiLU * up -> QA in its epilogues) and the per-row attention that quantizes its output for wo
    (k_decn_scores / k_dec_pv_blk<true>); 61 is the first size past both.  n_embd 320 / n_ff 896 leave padded QA blocks (K not a multiple of 256) that these
    kernels must zero themselves."""
    hp = synth.HParams(n_vocab=96, n_embd=320, n_mult=64, n_head=5, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=77))
    om = oracle.load(path, 352)
    prompt = synth.synth_prompt(348, hp.n_vocab, seed=5)
    with L.Model(path, n_ctx=352) as gm:
        n_past = 0
        for n in (8, 8, 2, 3, 4, 5, 7, 9, 12, 16, 17, 24, 32, 33, 47, 60, 61):     # 348 tokens
            chunk = prompt[n_past:n_past + n]
            a = gm.eval_debug(chunk, n_past, nth, all_logits=True)
            b = om.eval(chunk, n_past, nth, all_logits=True)
            assert same(a["logits_all"], b["logits_all"]), (n_past, n, describe(a["logits_all"], b["logits_all"]))
            n_past += n
        for il in range(hp.n_layer):
            gk, gv = gm.kv(il, n_past)
            ok, ov = om.kv(il, n_past)
            assert same(gk, ok) and same(gv, ov), f"kv cache layer {il}"


@pytest.mark.parametrize("n_embd,n_head", [(128, 4), (128, 2), (256, 1), (512, 2)])       # head sizes 32, 64, 256, 256
def test_other_head_sizes_vs_oracle(L, oracle, tmp_path, n_embd, n_head):
    """The loader accepts head sizes 32 / 64 / 128 / 256; only 128 has the lane = query prompt attention, the
    others take the per-row kernel.  Prompt (all-row logits), decode (graph and eager) and KV rows vs the oracle."""
    hp = synth.HParams(n_vocab=96, n_embd=n_embd, n_mult=64, n_head=n_head, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=n_embd + n_head))
    om = oracle.load(path, 64)
    prompt = synth.synth_prompt(37, hp.n_vocab, seed=5)
    b = om.eval(prompt, 0, 8, all_logits=True)
    tok, want, t = int(np.argmax(b["logits"])), [], None
    t = tok
    for i in range(10):
        lo = om.eval(np.array([t], np.int32), 37 + i, 8)["logits"]
        t = int(np.argmax(lo)); want.append(t)
    for flags in (0, 1):
        with L.Model(path, n_ctx=64, flags=flags) as gm:
            a = gm.eval_debug(prompt, 0, 8, all_logits=True)
            assert same(a["logits_all"], b["logits_all"]), describe(a["logits_all"], b["logits_all"])
            got, last = gm.decode_greedy(tok, 37, 10, 8, want_logits=True)
            assert got.tolist() == want and same(last, lo)
            for il in range(hp.n_layer):
                gk, gv = gm.kv(il, 47)
                ok, ov = om.kv(il, 47)
                assert same(gk, ok) and same(gv, ov)


@pytest.mark.parametrize("nested_tag", ["matrix_core_prompt_gemm_forced"], ids=["mfma_min_32"])
def test_matrix_core_prompt_gemm_forced_on_small_models(nested_tag):
    """k_gemm_mfma4 (the exact long-prompt kernel: fp16 K = 4 matrix instructions, four chains per issue, four waves per SIMD,
    DMA-staged operands) is only selected when its workgroups fill the chip, which the small test models never do: re-run the
    prompt tests with LLAMAHIP_MFMA_MIN=32 (read once per process, hence the subprocess) so that every eval of >= 32 rows
    goes through the matrix cores -- ragged row and column counts, odd numbers of 32-row blocks, the wider models' shapes."""
    from conftest import nested
    nested(nested_tag)


def _nested_params(prefix):
    import variants           # (ONE registry of variants: tests/variants.py; tests/test_host.py walks the forced few-row plans host-only)
    return [pytest.param(t, id=t.split(":", 1)[1]) for t in variants.NESTED if t.startswith(prefix)]


@pytest.mark.parametrize("nested_tag", _nested_params("attn:"))
def test_decode_attention_fallback_paths(nested_tag):
    """The decode step runs wq|wk|wv + attention as one launch with in-launch hand-offs (k_qkv_attn) where the shapes allow;
    the paths it replaces stay in the library for every other shape: the single-launch attention with per-head counters
    (k_dec_attn_x: LLAMAHIP_NO_QKV_ATTN=1) and the two-launch attention (LLAMAHIP_NO_ATTN_X=1).  The schedule also changes with
    the POSITION (llamahip.cpp attn_sched_at; defaults = measured crossovers, far beyond these tests' contexts): separate mat-vec +
    k_dec_scores + k_dec_pv_blk from LLAMAHIP_ATTN_TWO_FROM, + the streaming soft_max . V (k_dec_pv_stream, its chains split over
    workgroups with tagged partial sums) from LLAMAHIP_ATTN_LONG_FROM -- run here from position 0, and with both switch points
    inside the thread-split test's one decode call (27 -> 71: three captured graphs replayed in turn), with stages of 3 / 2 rows per
    chain so that these small contexts walk the whole load / LDS pipeline (many stages, both buffers, ragged last stage).
    The w1|w3 mat-vec runs in half-block workgroups where that balances the CUs (7B; EPI_SILU_QAH: the halves of a Q4_0 activation block
    exchange their partial amax inside one XCD) -- LLAMAHIP_NO_W13_HALF keeps the 8-wave block workgroups everywhere, LLAMAHIP_W13_HALF=1
    forces the halves onto the 13B / 65B widths (their two-granule prologue variant).
    The switches are read once per process, hence the subprocess; same parity tests, same oracle."""
    from conftest import nested
    nested(nested_tag)



@pytest.mark.parametrize("nth", [8, 3, 5])
def test_7b_width_decode_at_ragged_contexts_thread_splits(L, oracle, tmp_path, nth):
    """7B-width rows (n_embd 4096, 32 heads of 128: the shapes every decode attention schedule is instantiated for -- the fused launch,
    and with LLAMAHIP_ATTN_LONG_FROM=0 the LDS-DMA soft_max . V, k_dec_pv_dma: head size 128, chunks split over 8 / 2 / 2 workgroups
    of a head) decoded from position 137 to 185 with n_threads 8 / 3 / 5: chunk lengths that are not multiples of the 8-row stages, a
    last chunk shorter than the others, the ring wrapping never / the tail clamp at the cache's end (n_ctx 192)."""
    kw = dict(n_vocab=256, n_embd=4096, n_mult=256, n_head=32, n_layer=2)
    path = synth_tool(tmp_path / "w7b.bin", seed=29, **kw)
    prompt = synth.synth_prompt(137, kw["n_vocab"], seed=2)
    om = oracle.load(path, 192)
    lo = om.eval(prompt, 0, nth)["logits"]
    with L.Model(path, n_ctx=192) as gm:
        a = gm.eval(prompt, 0, nth)
        assert same(a, lo), describe(a, lo)
        t = int(np.argmax(lo)); first, want = t, []
        for i in range(48):
            lo = om.eval(np.array([t], np.int32), 137 + i, nth)["logits"]
            t = int(np.argmax(lo)); want.append(t)
        got, last = gm.decode_greedy(first, 137, 48, nth, want_logits=True)
        assert got.tolist() == want and same(last, lo), (got.tolist(), want)
    om.close()


@pytest.mark.parametrize("shape", ["small", "7b_width"])
def test_norm_statistics_branches_with_dc_offset_rows(L, oracle, tmp_path, shape):
    """The decode kernels' norm prologue computes the second moment in one pass (S2 - mean * S1, from the producer's partial sums)
    and switches to the reference's two-pass form (ggml.c:5355-5381) when the mean dominates (K mean^2 > S2 / 4).  Random weights
    have mean ~ 0, so this model's embedding rows carry a constant: row r gets 0.0115 * (r % 4) / 2 added -- means of 0, 0.29, 0.58
    and 0.86 sigma / ... i.e. rows well inside the fast branch, rows within 3 % of the threshold on either side (r % 4 == 2) and rows
    well inside the two-pass branch; the residual stream keeps the offset through the layers, so every norm of the step sees it.
    Single-token evals (both norm-fused mat-vecs, the lm head) and the captured greedy loop, against the oracle."""
    kw = dict(n_vocab=64, n_embd=256, n_mult=64, n_head=2, n_layer=2) if shape == "small" else dict(n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=2)
    path = synth_tool(tmp_path / "dc.bin", seed=5, emb_offset=0.0115, **kw)
    om = oracle.load(path, 64)
    with L.Model(path, n_ctx=64) as gm:
        toks = [1, 2, 3, 6, 7, 10, 5, 4, 14, 11]           # residues 1, 2, 3, 2, 3, 2, 1, 0, 2, 3
        for pos, t in enumerate(toks):
            a, b = gm.eval(np.array([t], np.int32), pos, 8), om.eval(np.array([t], np.int32), pos, 8)["logits"]
            assert same(a, b), (shape, pos, t, describe(a, b))
        t, want = int(np.argmax(b)), []
        first = t
        for i in range(12):
            lo = om.eval(np.array([t], np.int32), len(toks) + i, 8)["logits"]
            t = int(np.argmax(lo)); want.append(t)
        got, last = gm.decode_greedy(first, len(toks), 12, 8, want_logits=True)
        assert got.tolist() == want and same(last, lo), (shape, got.tolist(), want)
        # a prompt chunk as well (the prompt path's norm is the reference's two-pass form throughout)
        pr = np.array(toks[:9], np.int32)
        a, b = gm.eval(pr, 0, 8), om.eval(pr, 0, 8)["logits"]
        assert same(a, b), describe(a, b)
    om.close()


@pytest.mark.parametrize("nested_tag", _nested_params("plan:"))
def test_few_row_kernel_selectable_epilogues_and_plans(nested_tag):
    """The few-row mat-mul (k_gemv_set) runs w1|w3 in half-block workgroups with a tagged amax exchange for one column group and in
    whole-block workgroups (no exchange) from two column groups on; LLAMAHIP_SET_W13_BLOCKS=0 / 1 forces either epilogue onto every row
    count it can serve, LLAMAHIP_SET_PLAN[_SMALL] another (columns per wave, column-waves) plan than the measured default -- the short-eval
    and set-step parity tests re-run under each (switches are read once per process, hence the subprocess; same tests, same oracle)."""
    from conftest import nested
    nested(nested_tag)


@pytest.mark.parametrize("nested_tag", _nested_params("prod:"))
def test_production_fallbacks_and_selectable_variants(nested_tag):
    """Arithmetic that ships in libllamahip.so but that the default configuration of this box never selects:
    NO_LUT_MATH -- the SiLU / exp fp16 tables GATHERED (ggml.c:1956-1963, 7024-7036) instead of evaluated, what a device whose
    double-precision exp failed the exhaustive load-time check would run; NORM_MODE 0 / 1 -- the reference's two-pass statistics /
    the one-pass statistics reduced inside every prologue instead of handed over by the producer; NO_HOST_IO + HOST_SAMPLER -- blit
    copies and the host-side candidate selection; MFMA_I8 -- the int8 matrix-core prompt GEMM of round 1; EAGER_PREFILL_COPY -- the
    prompt-only weight copies built at load.  Switches are read once
    per process, hence the subprocess; same parity tests, same oracle."""
    from conftest import nested
    nested(nested_tag)


@pytest.mark.parametrize("which", [{"LLAMAHIP_HANDOFF_FAULT_TEST": "1"}, {"LLAMAHIP_HANDOFF_FAULT_TEST": "4", "LLAMAHIP_ATTN_LONG_FROM": "0"},
                                   {"LLAMAHIP_HANDOFF_FAULT_TEST": "6"}])
def test_in_launch_handoff_timeout_is_an_error_not_a_hang(model7b, which):
    """The tagged hand-offs of the decode step are bounded polls; one that runs out raises a sticky fault word in
    pinned host memory and the next synchronisation returns PredictionFailed.  LLAMAHIP_HANDOFF_FAULT_TEST=1 makes the
    mat-vec role of k_qkv_attn publish a tag nobody waits for and shortens the polls (read once per process: subprocess);
    =4 does the same to the split workgroups of the long-context soft_max . V (k_dec_pv_stream / k_dec_pv_dma), run here from position 0;
    =6 to the half-block workgroups of the w1|w3 mat-vec (EPI_SILU_QAH: a partial amax published under a tag its partner does not wait for)."""
    import subprocess
    import sys
    code = (
        "import sys, time, numpy as np\n"
        "import llama_swift_amd as L\n"
        "m = L.Model(sys.argv[1], n_ctx=64)\n"
        "m.eval(np.array([1, 5, 9, 13], np.int32), 0, 8)\n"          # a 4-row eval: not the decode path, must still work
        "t0 = time.time()\n"
        "try:\n"
        "    m.eval(np.array([7], np.int32), 4, 8)\n"
        "    print('NO ERROR')\n"
        "except L.LlamaHipError as e:\n"
        "    print('ERR', e.code, str(e)); print('SECONDS', time.time() - t0)\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, **which)
    r = subprocess.run([sys.executable, "-c", code, model7b], env=env, capture_output=True, text=True, cwd=root, timeout=300)
    assert "ERR -1001" in r.stdout and "hand-off" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(r.stdout.split("SECONDS")[1].split()[0]) < 30.0, r.stdout


def test_few_row_handoff_timeout_is_an_error_not_a_hang(model7b):
    """The same for the few-row kernel (k_gemv_set): its half-block w1|w3 workgroups exchange a partial amax per column as tagged
    granules.  LLAMAHIP_HANDOFF_FAULT_TEST=7 publishes them under a tag the partner does not wait for and shortens the polls: a 4-row
    eval (the set step's kernels) returns PredictionFailed within seconds instead of hanging."""
    import subprocess
    import sys
    code = (
        "import sys, time, numpy as np\n"
        "import llama_swift_amd as L\n"
        "m = L.Model(sys.argv[1], n_ctx=64)\n"
        "m.eval(np.array([7], np.int32), 0, 8)\n"                    # single-token decode does not use the few-row kernel: works
        "t0 = time.time()\n"
        "try:\n"
        "    m.eval(np.array([1, 5, 9, 13], np.int32), 1, 8)\n"
        "    print('NO ERROR')\n"
        "except L.LlamaHipError as e:\n"
        "    print('ERR', e.code, str(e)); print('SECONDS', time.time() - t0)\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, LLAMAHIP_HANDOFF_FAULT_TEST="7")
    r = subprocess.run([sys.executable, "-c", code, model7b], env=env, capture_output=True, text=True, cwd=root, timeout=300)
    assert "ERR -1001" in r.stdout and "hand-off" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert float(r.stdout.split("SECONDS")[1].split()[0]) < 30.0, r.stdout


def test_context_overflow_and_bad_tokens_are_errors(L, tmp_path):
    hp = synth.HParams(n_vocab=64, n_embd=256, n_mult=64, n_head=2, n_layer=1)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=1))
    with L.Model(path, n_ctx=16) as m:
        m.eval(np.arange(3, 19, dtype=np.int32) % 64, 0)                 # exactly fills the context
        with pytest.raises(L.LlamaHipError) as e:
            m.eval([5], 16)
        assert e.value.code == -1001 and "context overflow" in e.value.message
        with pytest.raises(L.LlamaHipError):
            m.eval([64], 0)
        with pytest.raises(L.LlamaHipError):
            m.decode_greedy(5, 10, 7)


def test_runner_event_stream_matches_the_reference_driver(L, oracle, tmp_path):
    """-[LlamaPredictOperation main] (.mm:768-901): prompt echoed first, chunks of 9, warm-up eval,
    exactly len(prompt tokens) + n_predict tokens, greedy = argmax."""
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=64, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=21))
    states, toks = [], []
    text = "hello world abc tok00050 zz"
    out = L.LlamaRunner(path).run(text, L.Config(numThreads=8, numTokens=12, greedy=True, n_ctx=64), toks.append,
                                  lambda s, e: states.append(s))
    assert states == [L.RunState.notStarted, L.RunState.initializing, L.RunState.generatingOutput, L.RunState.completed]
    with L.Model(path, n_ctx=64, flags=4) as hm:
        ids = hm.tokenize(text, True)
        vocab = [hm.token_text(i) for i in range(hp.n_vocab)]
    assert len(out) == len(ids) + 12 and out == toks
    assert out[:len(ids)] == [vocab[i] for i in ids]
    om = oracle.load(path, 64)
    om.eval(np.array([0, 1, 2, 3], np.int32), 0, 8)                      # warm-up (.mm:822)
    n_past, lo = 0, None
    for c0 in range(0, len(ids), 9):
        lo = om.eval(ids[c0:c0 + 9], n_past, 8)["logits"]; n_past += len(ids[c0:c0 + 9])
    want = []
    for i in range(12):
        t = int(np.argmax(lo)); want.append(vocab[t])
        if i < 11:
            lo = om.eval(np.array([t], np.int32), n_past, 8)["logits"]; n_past += 1
    assert out[len(ids):] == want


@pytest.mark.parametrize("tag", ["f16", "f32"])
def test_quantize_file_matches_the_reference_tool(L, oracle, tmp_path, tag):
    """llamahip_quantize_file against the file the reference's own quantize tool wrote
    for the same input (tests/golden/quantize_file.npz): byte-identical, crafted .5 ties / zero blocks /
    outliers included; the result loads and evaluates like any other Q4_0 model; bad requests fail."""
    import subprocess
    g = np.load(os.path.join(G, "quantize_file.npz"))
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    g[f"in_{tag}"].tofile(src)
    L.quantize_file(src, dst, 2)
    got = np.fromfile(dst, np.uint8)
    assert got.size == g[f"out_{tag}"].size and np.array_equal(got, g[f"out_{tag}"])
    toks = np.array([1, 5, 9, 30, 2], np.int32)
    with L.Model(dst, n_ctx=16) as gm:
        assert same(gm.eval(toks, 0, 8), oracle.load(dst, 16).eval(toks, 0, 8)["logits"])
    tool = os.path.join(os.path.dirname(G), os.pardir, "llama.swift_amd", "csrc", "tools", "quantize")
    dst2 = str(tmp_path / "out2.bin")
    assert subprocess.run([tool, src, dst2, "2"], capture_output=True).returncode == 0
    assert np.array_equal(np.fromfile(dst2, np.uint8), g[f"out_{tag}"])
    with pytest.raises(L.LlamaHipError, match="invalid quantization type"):
        L.quantize_file(src, dst2, 4)
    with pytest.raises(L.LlamaHipError, match="unsupported ftype"):
        L.quantize_file(dst, dst2, 2)                                  # already quantized
    with pytest.raises(L.LlamaHipError, match="failed to open"):
        L.quantize_file(str(tmp_path / "missing.bin"), dst2, 2)
    open(str(tmp_path / "junk.bin"), "wb").write(b"not a model file at all")
    with pytest.raises(L.LlamaHipError, match="bad magic"):
        L.quantize_file(str(tmp_path / "junk.bin"), dst2, 2)


@pytest.mark.parametrize("tag,ftype", [("f16", 1), ("f32", 0)])
def test_dense_model_files_golden(L, tmp_path, tag, ftype):
    """f16 / f32 model files (dense.hip) against vectors the reference itself produced
    (tests/golden/make_dense_golden.py): all-row prompt logits from an empty and from a non-empty context,
    13 greedy tokens, the last logits and one layer's KV rows -- bit for bit, for two thread counts."""
    g = np.load(os.path.join(G, "dense_model.npz"))
    v, e, mult, h, nl = (int(x) for x in g["hp"])
    hp = synth.HParams(n_vocab=v, n_embd=e, n_mult=mult, n_head=h, n_layer=nl)
    path = str(tmp_path / "m.bin")
    synth.write_model_unquantized(path, hp, synth.random_tensors(hp, seed=int(g["seed"][0])), ftype)
    prompt = g["prompt"]
    for nth in (8, 3):
        with L.Model(path, n_ctx=64) as m:
            a = m.eval_debug(prompt[:28], 0, nth, all_logits=True)["logits_all"]
            b = m.eval_debug(prompt[28:], 28, nth, all_logits=True)
            assert same(a, g[f"{tag}_nth{nth}_logits_a"]) and same(b["logits_all"], g[f"{tag}_nth{nth}_logits_b"])
            want = g[f"{tag}_nth{nth}_tokens"]
            assert int(np.argmax(b["logits"])) == want[0]
            got, last = m.decode_greedy(int(want[0]), len(prompt), 12, nth, want_logits=True)
            assert got.tolist() == want[1:].tolist() and same(last, g[f"{tag}_nth{nth}_logits_last"])
            k, vv = m.kv(1, len(prompt) + 12)
            assert same(k, g[f"{tag}_nth{nth}_k1"]) and same(vv, g[f"{tag}_nth{nth}_v1"])


def test_q4_1_model_file_golden(L, tmp_path):
    """Q4_1 files (f16 = 3): the quantize tool with type 3 reproduces the file the reference's tool wrote from
    the same f16 input (the offline quantizer's FLT_MIN quirk included), and that file evaluates bit for bit
    like the reference's scalar Q4_1 path: all-row logits from an empty / non-empty context, 11 greedy tokens,
    last logits, KV rows, two thread counts."""
    g = np.load(os.path.join(G, "q41_model.npz"))
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "q41.bin")
    g["in_f16"].tofile(src)
    L.quantize_file(src, dst, 3)
    assert np.array_equal(np.fromfile(dst, np.uint8), g["q41_file"])
    prompt = g["prompt"]
    for nth in (8, 3):
        with L.Model(dst, n_ctx=64) as m:
            a = m.eval_debug(prompt[:20], 0, nth, all_logits=True)["logits_all"]
            b = m.eval_debug(prompt[20:], 20, nth, all_logits=True)
            assert same(a, g[f"nth{nth}_logits_a"]), describe(a, g[f"nth{nth}_logits_a"])
            assert same(b["logits_all"], g[f"nth{nth}_logits_b"])
            want = g[f"nth{nth}_tokens"]
            assert int(np.argmax(b["logits"])) == want[0]
            got, last = m.decode_greedy(int(want[0]), len(prompt), 10, nth, want_logits=True)
            assert got.tolist() == want[1:].tolist() and same(last, g[f"nth{nth}_logits_last"])
            k, vv = m.kv(1, len(prompt) + 10)
            assert same(k, g[f"nth{nth}_k1"]) and same(vv, g[f"nth{nth}_v1"])


def _dense_multipart_model(tmp):
    hp = synth.HParams(n_vocab=64, n_embd=256, n_mult=128, n_head=2, n_layer=1)
    path = str(tmp) + "/m.bin"
    t = synth.random_tensors(hp, seed=77)
    synth.write_model_unquantized(path, hp, t, 1, n_parts=2)
    return path, t, synth.synth_prompt(35, hp.n_vocab, seed=2)


@refgolden.computed_by("gpu_parity.dense_multipart")
def _ref_dense_multipart(ref, tmp):
    path, _, prompt = _dense_multipart_model(tmp)
    rm = ref.load(path, 48, 2)
    out = {"logits_all": rm.eval(prompt, 0, 8, all_logits=True)["logits_all"]}
    rm.close()
    return out


def test_dense_multipart_files_vs_reference(L, ref, tmp_path):
    """An f16 model in two part files (column / row shards merged at load, .mm:358-388, 467-487) against
    the reference library on the same files (its logits stored in tests/golden/ref_outputs.npz); refusals: per-layer dumps, the fused
    stage step."""
    want = refgolden.outputs("gpu_parity.dense_multipart", ref, tmp_path)
    path, t, prompt = _dense_multipart_model(tmp_path)
    with L.Model(path, n_ctx=48, n_parts=2) as m:
        assert same(m.eval_debug(prompt, 0, 8, all_logits=True)["logits_all"], want["logits_all"])
        for name in ("layers.0.attention.wo.weight", "layers.0.feed_forward.w1.weight", "tok_embeddings.weight"):
            assert m.tensor_bytes(name).tobytes() == np.ascontiguousarray(t[name], np.float16).tobytes(), name
        with pytest.raises(L.LlamaHipError, match="Q4_0 models only"):
            m.eval_debug(prompt[:4], 0, 8, dump_layer=0)
        with pytest.raises(L.LlamaHipError, match="llamahip_eval_stage"):
            m.stage_bind(0, 0, token_in=1)


def test_runner_keeps_the_model_between_runs_when_asked(L, tmp_path):
    """the reference reloads the model on every run (.mm:790, :900).  With
    Config.keepModel the bridge reuses the loaded handle; a second run on the stale KV cache must give
    exactly the tokens of a freshly loaded model, sampled path included (mt19937 seeded per run)."""
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=64, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=21))
    prompts = ["hello world abc tok00050 zz", "tok00007 a much longer second prompt tok00011 tok00012 xyz", "b"]
    for greedy in (True, False):
        fresh = [L.LlamaRunner(path).run(p, L.Config(numTokens=10, greedy=greedy, n_ctx=64, seed=5)) for p in prompts]
        kept = L.LlamaRunner(path)
        states = []
        got = [kept.run(p, L.Config(numTokens=10, greedy=greedy, n_ctx=64, seed=5, keepModel=True), None,
                        lambda s, e: states.append(s)) for p in prompts]
        assert got == fresh
        assert kept.loads == 1
        assert states.count(L.RunState.initializing) == 3 and states.count(L.RunState.completed) == 3
        kept.run(prompts[0], L.Config(numTokens=4, greedy=greedy, n_ctx=32, seed=5, keepModel=True))     # other n_ctx: reload
        assert kept.loads == 2
        kept.run(prompts[0], L.Config(numTokens=4, greedy=greedy, n_ctx=32, seed=5))                      # reference behaviour again
        assert kept.loads == 3
        kept.close()


@pytest.mark.parametrize("name,kw,parts", [
    ("13B-shaped", dict(n_vocab=32000, n_embd=5120, n_mult=256, n_head=40, n_layer=2), 2),      # K = 5120 / 13824, two part files
    ("30B-shaped", dict(n_vocab=4000, n_embd=6656, n_mult=256, n_head=52, n_layer=1), 4),       # K = 6656 / 17920, four part files
    ("65B-shaped", dict(n_vocab=4000, n_embd=8192, n_mult=256, n_head=64, n_layer=1), 8),       # K = 8192 / 22016, eight part files
])
def test_wider_models_vs_oracle(L, oracle, tmp_path, name, kw, parts):
    """The other widths of the family (LLAMA_N_PARTS, .mm:33-38): different chunk counts exercise other
    ring depths / prologue budgets of the GEMV, and the part counts the loader derives from n_embd."""
    path = synth_tool(tmp_path / "m.bin", seed=5, parts=parts, **kw)
    om = oracle.load(path, 48)
    with L.Model(path, n_ctx=48) as gm:
        assert gm.n_parts == parts == om.n_parts
        prompt = synth.synth_prompt(9, kw["n_vocab"], seed=3)
        a, b = gm.eval_debug(prompt, 0, 8, dump_layer=kw["n_layer"] - 1), om.eval(prompt, 0, 8, all_logits=True, dump_layer=kw["n_layer"] - 1)
        for k in b:
            assert same(a[k], b[k]), f"{name} {k}: " + describe(a[k], b[k])
        tok, want = int(np.argmax(b["logits"])), []
        t = tok
        for i in range(5):
            lo = om.eval(np.array([t], np.int32), 9 + i, 8)["logits"]
            t = int(np.argmax(lo)); want.append(t)
        got, last = gm.decode_greedy(tok, 9, 5, 8, want_logits=True)
        assert got.tolist() == want and same(last, lo), name


@pytest.mark.parametrize("nth", [1, 3, 5, 8])
def test_fused_decode_launch_thread_splits_and_slice_boundaries(L, oracle, tmp_path, nth):
    """k_qkv_attn (wq|wk|wv mat-vec + attention in one launch, tagged hand-offs) at the 7B width for every n_threads the
    V*P split can take (the chunk boundaries dc = ceil(T / n_threads) move with it), decoding across the 32-key slice
    boundaries of its score workgroups (context 27 -> 71: slices 1, 2 and 3 come alive at 32 and 64) -- tokens, final
    logits and the KV rows the launch appended, against the oracle."""
    path = synth_tool(tmp_path / "m.bin", seed=11, n_vocab=512, n_embd=4096, n_mult=256, n_head=32, n_layer=2)
    om = oracle.load(path, 96)
    with L.Model(path, n_ctx=96) as gm:
        # a single token at position 0 (one key, every V*P chain but the first empty), then one at position 1
        for pos, t in ((0, 1), (1, 17)):
            a, b = gm.eval(np.array([t], np.int32), pos, nth), om.eval(np.array([t], np.int32), pos, nth)["logits"]
            assert same(a, b), (pos, describe(a, b))
        prompt = synth.synth_prompt(27, 512, seed=4)
        a, b = gm.eval(prompt, 0, nth), om.eval(prompt, 0, nth)["logits"]
        assert same(a, b), describe(a, b)
        tok, want = int(np.argmax(b)), []
        t = tok
        for i in range(44):
            lo = om.eval(np.array([t], np.int32), 27 + i, nth)["logits"]
            t = int(np.argmax(lo)); want.append(t)
        got, last = gm.decode_greedy(tok, 27, 44, nth, want_logits=True)
        assert got.tolist() == want and same(last, lo), (nth, got.tolist(), want)
        for il in range(2):
            gk, gv = gm.kv(il, 71)
            ok, ov = om.kv(il, 71)
            assert same(gk, ok) and same(gv, ov), f"kv cache layer {il}"


# ------------------------------------------------------------------------------------------------ full LLaMA-7B size
@pytest.fixture(scope="module")
def model7b():
    import bg_expect
    return bg_expect.model("7B")


def test_7b_logits_and_greedy_tokens_vs_oracle(L, oracle, model7b):
    om = oracle.load(model7b, 512)
    with L.Model(model7b, n_ctx=512) as gm:
        prompt = synth.synth_prompt(9, 32000, seed=1)
        a, b = gm.eval_debug(prompt, 0, 8, dump_layer=31), om.eval(prompt, 0, 8, all_logits=True, dump_layer=31)
        for k in b:
            assert same(a[k], b[k]), f"{k}: " + describe(a[k], b[k])
        tok, want, t = int(np.argmax(b["logits"])), [], None
        t = tok
        for i in range(6):
            lo = om.eval(np.array([t], np.int32), 9 + i, 8)["logits"]
            t = int(np.argmax(lo)); want.append(t)
        got, last = gm.decode_greedy(tok, 9, 6, 8, want_logits=True)
        assert got.tolist() == want
        assert same(last, lo), describe(last, lo)


@pytest.fixture(scope="module")
def trace7b(model7b):
    """BASELINE.json configs[0] / [1]: greedy generation on the 7B file at n_ctx 512 by the CPU path, 8 threads --
    the reference's own ggml.c (oracle/_ref) when it travelled with the snapshot, else the standalone
    restatement.  One token per llama_eval, as the bridge does (.mm:834-896): 504 tokens after an 8-token prompt
    fill the context; the first 128 of them are configs[0].  Keeps the top-2 logit margin of every step."""
    import bg_expect
    x = bg_expect.get("trace7b")           # (a child process started at collection, tests/bg_expect.py; nested variant runs read its .npz)
    return dict(prompt=x["prompt"], first=int(x["first"]), toks=x["want"], margins=x["margins"], last=x["lo"])


def _trace_report(got, want, margins):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want)[:len(got)])
    if not bad.size:
        return "identical"
    i = int(bad[0])
    return (f"first divergence at generated token {i} (context position {8 + i}): gpu {int(got[i])} vs cpu {int(want[i])}; "
            f"cpu top-2 logit margin there {margins[i]:.3e}; smallest margin before it {margins[:i + 1].min():.3e}")


def test_7b_greedy_trace_128_tokens_vs_cpu_path(L, model7b, trace7b):
    """configs[0]: LLaMA-7B, 8 threads, greedy 128 tokens -- token for token, one host-driven llama_eval per token
    (the drop-in boundary), logits of the last step bit for bit."""
    with L.Model(model7b, n_ctx=512) as gm:
        lg = gm.eval(trace7b["prompt"], 0, 8)
        t = int(np.argmax(lg))
        assert t == trace7b["first"]
        got = []
        for i in range(128):
            lg = gm.eval(np.array([t], np.int32), 8 + i, 8)
            t = int(np.argmax(lg)); got.append(t)
        assert got == trace7b["toks"][:128].tolist(), _trace_report(got, trace7b["toks"], trace7b["margins"])


def test_7b_greedy_trace_512_context_vs_cpu_path(L, model7b, trace7b):
    """configs[1]: LLaMA-7B single-token decode over the whole 512-token context on the device-resident greedy
    loop (hipGraph replay, on-device argmax) -- all 504 generated tokens and the final logits against the CPU path."""
    with L.Model(model7b, n_ctx=512) as gm:
        lg = gm.eval(trace7b["prompt"], 0, 8)
        assert int(np.argmax(lg)) == trace7b["first"]
        got, last = gm.decode_greedy(trace7b["first"], 8, 504, 8, want_logits=True)
        assert got.tolist() == trace7b["toks"].tolist(), _trace_report(got, trace7b["toks"], trace7b["margins"])
        assert same(last, trace7b["last"]), describe(last, trace7b["last"])


def test_7b_width_2048_token_prefill_vs_oracle(L, oracle, tmp_path):
    """configs[2]: a 2048-token prompt in ONE eval at n_ctx 2560 on LLaMA-7B's matrix shapes (n_embd 4096, n_ff
    11008, 32 heads; 2 layers and a 4000-entry vocabulary so that the CPU side stays at ~15 s): every mat-mul
    takes the matrix-core kernel by the production selection rule (no LLAMAHIP_MFMA_MIN), attention the
    lane-per-query kernels at T = 2048.  All 2048 rows of logits, bit for bit."""
    kw = dict(n_vocab=4000, n_embd=4096, n_mult=256, n_head=32, n_layer=2)
    path = synth_tool(tmp_path / "w7b.bin", seed=11, **kw)
    prompt = synth.synth_prompt(2048, kw["n_vocab"], seed=5)
    om = oracle.load(path, 2560)
    want = om.eval(prompt, 0, 8, all_logits=True)
    om.close()
    before = L.gemm_paths()
    with L.Model(path, n_ctx=2560) as gm:
        got = gm.eval_debug(prompt, 0, 8)
        after = L.gemm_paths()
        assert after["mfma"] - before["mfma"] >= 4 * kw["n_layer"], (before, after)      # wq|wk|wv, wo, w1|w3, w2 of every layer
        # (only the lm head over all 2048 rows -- a debug-eval extra, it has no prompt copies -- takes another kernel)
        assert after["rows"] == before["rows"] and after["lds"] - before["lds"] <= 1, (before, after)
        assert same(got["logits"], want["logits"]), "last row: " + describe(got["logits"], want["logits"])
        for r in (0, 1, 63, 64, 777, 1500, 2046):
            assert same(got["logits_all"][r], want["logits_all"][r]), f"row {r}: " + describe(got["logits_all"][r], want["logits_all"][r])
        assert same(got["logits_all"], want["logits_all"]), describe(got["logits_all"], want["logits_all"])
        # ... and decode continues from that context exactly as the CPU path does
        om = oracle.load(path, 2560)
        om.eval(prompt, 0, 8)
        t = int(np.argmax(want["logits"]))
        toks = gm.decode_greedy(t, 2048, 3, 8)
        for i in range(3):
            lo = om.eval(np.array([t], np.int32), 2048 + i, 8)["logits"]
            t = int(np.argmax(lo))
            assert int(toks[i]) == t, f"decode step {i} after the 2048-token prompt"
        om.close()


def _topk_model(tmp):
    hp = synth.HParams(n_vocab=1200, n_embd=256, n_mult=64, n_head=2, n_layer=2)
    path = str(tmp) + "/m.bin"
    synth.write_model(path, hp, synth.random_tensors(hp, seed=21))
    return path, synth.synth_prompt(9, hp.n_vocab, seed=4)


@refgolden.computed_by("gpu_parity.topk_sampled")
def _ref_topk_sampled(ref, tmp):
    """60 steps of the reference's own llama_sample_top_p_top_k, fed with the reference's logits of every step"""
    path, toks = _topk_model(tmp)
    rm = ref.load(path, 128)
    rs = ref.L.refllama_sampler_new(-1, 64)
    n_past, ids = 0, []
    for _ in range(60):
        full = rm.eval(toks, n_past, 8)["logits"]
        ids.append(int(ref.L.refllama_sampler_sample(rm.h, rs, full, 1.3, 40, float(np.float32(0.95)), float(np.float32(0.8)))))
        ref.L.refllama_sampler_accept(rs, ids[-1])
        n_past += len(toks)
        toks = np.array([ids[-1]], np.int32)
    ref.L.refllama_sampler_free(rs)
    rm.close()
    return {"ids": np.array(ids)}


def test_device_topk_candidates_vs_the_reference_sampler(L, ref, tmp_path):
    """The sampler's front half on the device (scores + top-k, utils.cpp:345-395).  (1) On logits without ties the k
    (score, id) pairs are the host formula's, sorted -- checked against float64 numpy.  (2) On tie-heavy logits the kernel
    must flag every case where an equality could matter (exact = 0), and where it claims exactness the pairs must again
    be the unique answer.  (3) End to end: a sampled generation through llamahip_eval_topk + sample_from_candidates
    (fallback to the host path when flagged) draws the same ids, with the same mt19937 state, as the reference's own
    llama_sample_top_p_top_k fed with the logits of every step (the reference's logits, bit for bit the library's; stored in
    tests/golden/ref_outputs.npz)."""
    rng = np.random.default_rng(77)
    V = 32000

    def host_scores(lg, window, pen=1.3, temp=float(np.float32(0.8))):
        sc = lg.astype(np.float64) * (1.0 / temp)
        seen = np.zeros(V, bool); seen[window] = True
        neg = lg < 0
        sc[seen & neg] = (lg[seen & neg].astype(np.float64) * (1.0 / temp)) * pen
        sc[seen & ~neg] = (lg[seen & ~neg].astype(np.float64) * (1.0 / temp)) / pen
        return sc
    n_exact = 0
    for trial in range(40):
        ties = trial >= 20
        lg = (rng.integers(-40, 41, V) * 0.25).astype(np.float32) if ties else (rng.standard_normal(V) * 3).astype(np.float32)
        if ties and trial % 2:
            lg += (rng.standard_normal(V) * 1e-3).astype(np.float32) * (rng.random(V) < 0.5)        # half the entries stay tied
        window = rng.integers(0, V, 64).astype(np.int32)
        k = int(rng.integers(1, 41)) if trial % 3 else 40
        exact, sc, ids = L.op_topk(lg, window, top_k=k)
        want = host_scores(lg, window)
        order = np.argsort(-want, kind="stable")
        kth = want[order[k - 1]]
        unambiguous = np.count_nonzero(want >= kth) == k and np.unique(want[order[:k]]).size == k
        assert exact == unambiguous, (trial, exact, unambiguous)
        if exact:
            n_exact += 1
            assert ids.tolist() == order[:k].tolist(), trial
            assert np.array_equal(sc, want[order[:k]]), trial
    assert n_exact >= 20
    # end to end on a model
    want_ids = refgolden.outputs("gpu_parity.topk_sampled", ref, tmp_path)["ids"].tolist()
    path, prompt = _topk_model(tmp_path)
    s = L.Sampler(seed=-1, repeat_last_n=64)
    with L.Model(path, n_ctx=128) as m:
        toks, n_past, hits = prompt, 0, 0
        for step, want in enumerate(want_ids):
            exact, sc, ids, lg = m.eval_topk(toks, n_past, s)
            got = s.sample_from_candidates(sc, ids) if exact else s.sample(m, lg)
            hits += exact
            assert got == want, (step, exact, got, want)
            s.accept(got)
            n_past += len(toks)
            toks = np.array([got], np.int32)
        assert hits >= 50


def test_fast_prefill_is_opt_in_and_close(L, tmp_path):
    """LLAMAHIP_FLAG_FAST_PREFILL (one integer sum and one fp32 chain per Q4_0 block on the matrix cores) is NOT the
    reference's arithmetic: it must be off by default and leave decode and short evals untouched.  How close it stays is
    bounded loosely on purpose: the reference quantizes activations to 4 bits before every mat-mul (ggml.c:6134-6152), so a
    last-bit difference in one mat-mul flips codes in the next and the difference grows to the size of that quantization
    noise within a layer or two -- measured on this random-weight model: max |delta logit| 0.83 after 2 layers of 7B width
    (4.4 after the 32 layers of the synthetic 7B, tools/prefill_fast_probe.py; logit std 1.3) -- the same floor the
    reference's own NEON and AVX2 builds sit apart at, since their activation quantizers round differently
    (ggml.c:415-452 vs 456-523).  The logits stay the same function: cosine similarity 0.986 here, bound 0.97."""
    kw = dict(n_vocab=4000, n_embd=4096, n_mult=256, n_head=32, n_layer=2)
    path = synth_tool(tmp_path / "w7b.bin", seed=11, **kw)
    prompt = synth.synth_prompt(512, kw["n_vocab"], seed=5)
    with L.Model(path, n_ctx=640) as ex, L.Model(path, n_ctx=640, flags=16) as fa:
        a, b = ex.eval(prompt, 0, 8), fa.eval(prompt, 0, 8)
        d = float(np.abs(a - b).max())
        cos = float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
        print(f"fast prefill vs exact, 512 tokens, 2 layers of 7B width: max |delta logit| = {d:.3e}, cosine {cos:.5f}, logit std {a.std():.3f}")
        assert not same(a, b), "the fast path did not run (or is, unexpectedly, bit-identical)"
        assert d <= 2.0 and cos > 0.97, (d, cos)
        # short evals and decode take the exact kernels under the flag too
        c9 = synth.synth_prompt(9, kw["n_vocab"], seed=6)
        assert same(ex.eval(c9, 512, 8), ex.eval(c9, 512, 8))
        ex2 = ex.eval(c9, 0, 8); fa2 = fa.eval(c9, 0, 8)
        assert same(ex2, fa2), "a 9-token eval must not take the fast kernel"
        t = int(np.argmax(ex2))
        assert ex.decode_greedy(t, 9, 8, 8).tolist() == fa.decode_greedy(t, 9, 8, 8).tolist()
        # ragged prompt lengths: the fast kernel takes exactly the matrices whose 64 x 64 workgroups reach 512 (launch_gemm:
        # ceil(M / 64) row pairs x ceil(N / 64) column tiles) -- at 65 and 100 rows w1|w3 alone, at 129 also wq|wk|wv, from 449 all four
        de, F = kw["n_embd"], synth.n_ff_of(kw["n_embd"], kw["n_mult"])
        for n in (65, 100, 129, 449, 512):
            p = synth.synth_prompt(n, kw["n_vocab"], seed=20 + n)
            want_fast = kw["n_layer"] * sum(1 for rows in (3 * de, de, 2 * F, de) if (rows + 63) // 64 * ((n + 63) // 64) >= 512)
            p0 = L.gemm_paths()
            b = fa.eval(p, 0, 8)
            p1 = L.gemm_paths()
            assert p1["fast"] - p0["fast"] == want_fast, (n, p0, p1)
            assert p1["mfma"] - p0["mfma"] >= want_fast, (n, p0, p1)
            a = ex.eval(p, 0, 8)
            d_, cos = float(np.abs(a - b).max()), float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))
            print(f"fast prefill vs exact, {n} tokens: max |delta logit| = {d_:.3e}, cosine {cos:.5f}")
            assert np.all(np.isfinite(b)) and d_ <= 2.0 and cos > 0.97, (n, d_, cos)
            p2 = L.gemm_paths()
            assert p2["fast"] == p1["fast"], "the exact handle took the fast kernel"


def test_7b_full_context_properties(L, model7b):
    """Size-independent properties over the whole 512-token context (no oracle in the loop):
    the graph-replayed device loop, the eager fused path and the unfused per-op path must agree
    token for token and bit for bit, and a rerun must reproduce itself."""
    prompt = synth.synth_prompt(8, 32000, seed=2)
    runs = {}
    for flags in (0, 1, 3):
        with L.Model(model7b, n_ctx=512, flags=flags) as m:
            lg = m.eval(prompt, 0, 8)
            steps = 504 if flags == 0 else 96
            toks, last = m.decode_greedy(int(np.argmax(lg)), 8, steps, 8, want_logits=True)
            runs[flags] = (toks, last)
            if flags == 0:
                lg2 = m.eval(prompt, 0, 8)
                toks2, last2 = m.decode_greedy(int(np.argmax(lg2)), 8, steps, 8, want_logits=True)
                assert same(lg, lg2) and toks.tolist() == toks2.tolist() and same(last, last2)      # idempotent
                assert len(set(toks.tolist())) > 8                                                   # not a degenerate loop
    assert runs[1][0].tolist() == runs[0][0][:96].tolist()
    assert runs[3][0].tolist() == runs[0][0][:96].tolist()
    assert same(runs[1][1], runs[3][1])
