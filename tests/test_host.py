"""CPU: the C-ABI library loads and exports every symbol include/*.h declares; loader validation and
error strings (file parsing happens before any device work); host-only handles: multi-part merge,
tokenizer and sampler against the golden vectors; the runner's event order on failure.
No compute call is made (there is no GPU here)."""
import os
import pathlib
import struct

import numpy as np
import pytest

import refgolden
import synth

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOST_ONLY = 4


def test_library_exports_every_declared_symbol(L):
    lib = L.lib()
    missing = [s for s in L.declared_symbols() if not hasattr(lib, s)]
    assert not missing
    assert len(L.declared_symbols()) >= 25
    assert {"llamahip_op_dense_prep", "llamahip_op_embed_dense"} <= set(L.declared_symbols())
    assert L.version().startswith("llamahip")


def test_library_exports_nothing_but_the_declared_c_abi(L):
    """A drop-in library linked into someone's application exports llamahip_* / llama_runner_* only (the declarations of include/*.h):
    no lh:: internals, no kernel host stubs, no stray helpers -- `nm -D --defined-only` against the headers."""
    import shutil
    import subprocess
    so = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc", "libllamahip.so")
    if not (shutil.which("nm") and os.path.exists(so)):
        pytest.skip("needs binutils' nm and the built libllamahip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    declared = set(L.declared_symbols())
    stray = [s for s in exported if s not in declared]
    assert not stray, f"exported but not declared in include/*.h: {stray[:20]}"
    assert all(s.startswith(("llamahip_", "llama_runner_")) for s in exported)


def test_load_errors_follow_the_reference_messages(L, tmp_path):
    with pytest.raises(L.LlamaHipError) as e:
        L.Model(str(tmp_path / "nope.bin"))
    assert e.value.code == -1000 and "failed to open" in e.value.message           # .mm:101-102
    bad = tmp_path / "bad.bin"
    bad.write_bytes(b"\x00" * 64)
    with pytest.raises(L.LlamaHipError) as e:
        L.Model(str(bad))
    assert e.value.code == -1000 and "bad magic" in e.value.message                 # .mm:111-112
    f16 = tmp_path / "f16.bin"
    f16.write_bytes(struct.pack("<I7i", synth.MAGIC, 4, 64, 32, 1, 1, 64, 7) + b"\x00" * 64)
    with pytest.raises(L.LlamaHipError) as e:
        L.Model(str(f16))
    assert "bad f16 value 7" in e.value.message                                      # .mm:176-177


def _write(tmp_path, hp, parts=1, mutate=None, seed=3):
    path = str(tmp_path / "m.bin")
    t = synth.random_tensors(hp, seed=seed)
    synth.write_model(path, hp, t, n_parts=parts)
    if mutate:
        mutate(path)
    return path, t


def test_unknown_and_misshapen_tensors_are_rejected(L, tmp_path):
    hp = synth.HParams(n_vocab=32, n_embd=128, n_mult=64, n_head=1, n_layer=1)
    path, _ = _write(tmp_path, hp)
    raw = bytearray(open(path, "rb").read())
    at = raw.find(b"norm.weight")
    raw[at:at + 4] = b"nor_"
    open(path, "wb").write(raw)
    with pytest.raises(L.LlamaHipError) as e:
        L.Model(path, flags=HOST_ONLY)
    assert "unknown tensor 'nor_.weight' in model file" in e.value.message         # .mm:353-354
    path, _ = _write(tmp_path, hp)
    raw = bytearray(open(path, "rb").read())
    at = raw.find(b"tok_embeddings.weight")
    ne0 = struct.unpack_from("<i", raw, at - 8)[0]
    assert ne0 == 128
    struct.pack_into("<i", raw, at - 8, 64)
    open(path, "wb").write(raw)
    with pytest.raises(L.LlamaHipError) as e:
        L.Model(path, flags=HOST_ONLY)
    assert "has wrong size in model file" in e.value.message                        # .mm:394-395


MERGE_TENSORS = ("tok_embeddings.weight", "output.weight", "norm.weight", "layers.0.attention.wq.weight",
                 "layers.1.attention.wo.weight", "layers.0.feed_forward.w1.weight", "layers.1.feed_forward.w2.weight",
                 "layers.1.feed_forward.w3.weight", "layers.0.ffn_norm.weight")


def _merge_model(tmp, parts):
    hp = synth.HParams(n_vocab=64, n_embd=256, n_mult=256, n_head=2, n_layer=2)      # n_ff 768: shards stay multiples of 64
    return _write(tmp, hp, parts=parts, seed=11)[0]


@refgolden.computed_by("host.multipart_merge", [(1,), (2,), (4,)])
def _ref_multipart_merge(ref, tmp, parts):
    r = ref.load(_merge_model(pathlib.Path(tmp), parts), 32, parts)
    out = {"hparams": np.array([r.n_vocab, r.n_embd, r.n_head, r.n_layer, r.n_ff])}
    out.update({f"tensor/{name}": refgolden.digest(r.tensor_bytes(name)) for name in MERGE_TENSORS})
    r.close()
    return out


@pytest.mark.parametrize("parts", [1, 2, 4])
def test_multipart_merge_matches_the_reference_loader(L, ref, tmp_path, parts):
    want = refgolden.outputs("host.multipart_merge", ref, tmp_path, parts)
    path = _merge_model(tmp_path, parts)
    m = L.Model(path, n_ctx=32, n_parts=parts, flags=HOST_ONLY)
    assert (m.n_vocab, m.n_embd, m.n_head, m.n_layer, m.n_ff, m.n_parts) == tuple(want["hparams"].tolist()) + (parts,)
    for name in MERGE_TENSORS:
        assert np.array_equal(refgolden.digest(m.tensor_bytes(name)), want[f"tensor/{name}"]), name
    with pytest.raises(L.LlamaHipError) as e:          # no device state behind a host-only handle
        m.eval([1], 0)
    assert e.value.code == -1001


def test_multipart_equals_single_part(L, tmp_path):
    hp = synth.HParams(n_vocab=64, n_embd=256, n_mult=256, n_head=2, n_layer=1)
    t = synth.random_tensors(hp, seed=5)
    p1, p2 = str(tmp_path / "one.bin"), str(tmp_path / "two.bin")
    synth.write_model(p1, hp, t, 1)
    synth.write_model(p2, hp, t, 2)
    a = L.Model(p1, flags=HOST_ONLY)
    b = L.Model(p2, n_parts=2, flags=HOST_ONLY)
    # row-sharded tensors quantize identically per shard; column shards too (32-aligned slices)
    for name in ("layers.0.attention.wq.weight", "layers.0.attention.wo.weight", "layers.0.feed_forward.w2.weight", "output.weight", "tok_embeddings.weight"):
        assert np.array_equal(a.tensor_bytes(name), b.tensor_bytes(name)), name


def _golden_model(L, tmp_path):
    g = np.load(os.path.join(G, "tiny_model.npz"))
    path = str(tmp_path / "tiny.bin")
    g["model_file"].tofile(path)
    return L.Model(path, n_ctx=64, flags=HOST_ONLY), g


def test_tokenizer_matches_reference_vectors(L, tmp_path):
    m, _ = _golden_model(L, tmp_path)
    t = np.load(os.path.join(G, "text.npz"))
    prompts = bytes(t["prompts_joined"]).split(b"\x00")
    for i, p in enumerate(prompts):
        assert np.array_equal(m.tokenize(p, True), t[f"tok_{i}_bos"]), p
        assert np.array_equal(m.tokenize(p, False), t[f"tok_{i}_nobos"]), p
    assert m.token_text(3) == b"a" and m.token_text(1) == b""
    with pytest.raises(IndexError):
        m.token_text(10 ** 6)


def test_tokenizer_equals_the_whole_vocabulary_scan(L, tmp_path):
    """The tokenizer buckets the vocabulary by first byte; the reference (utils.cpp:275-311) tries every token at
    every position.  Same result by construction -- checked here against a literal restatement of the
    reference loop on a vocabulary built to be nasty: duplicate strings (the highest id must win), prefixes of
    one another, empty entries, multi-byte UTF-8, and text with bytes no token starts with (tokenization stops)."""
    import synth
    rng = np.random.default_rng(11)
    alphabet = [b"a", b"b", b"ab", b"abc", b"abcd", b"b", b"bc", b"", b"c", b"ca", b"\xc3\xa9", b"\xc3", b"ab", b" ", b" a", b"abca"]
    vocab = [b"", b"", b""] + alphabet
    while len(vocab) < 64:
        k = int(rng.integers(1, 5))
        vocab.append(b"".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), k)))
    hp = synth.HParams(n_vocab=64, n_embd=64, n_mult=32, n_head=1, n_layer=1)
    path = str(tmp_path / "v.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=1), vocab=vocab)
    m = L.Model(path, n_ctx=16, flags=HOST_ONLY)

    def reference(text: bytes, bos: bool):
        res = [1] if bos else []
        pos = 0
        while True:
            best_len, best_id = 0, 0
            for tid, tok in enumerate(vocab):                     # ascending id, only strictly shorter tokens are skipped
                if len(tok) < best_len or len(tok) > len(text) - pos:
                    continue
                if text[pos:pos + len(tok)] == tok:
                    best_len, best_id = len(tok), tid
            if best_len == 0:
                break
            res.append(best_id)
            pos += best_len
        return res

    texts = [b"", b"abcabcd abca", b"ab ab\xc3\xa9c", b"abzab", b"\xc3\xa9\xc3", b" a a  abcdabcd" * 40]
    for _ in range(40):
        k = int(rng.integers(1, 30))
        texts.append(b"".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), k)))
    for t in texts:
        if b"\x00" in t:
            continue
        for bos in (True, False):
            assert m.tokenize(t, bos).tolist() == reference(t, bos), (t, bos)


def test_sampler_matches_reference_sequence(L, tmp_path):
    m, _ = _golden_model(L, tmp_path)
    t = np.load(os.path.join(G, "text.npz"))
    s = L.Sampler(seed=-1, repeat_last_n=64)
    for tok in t["sampler_window_init"]:
        s.accept(int(tok))
    got = []
    for lg in t["sampler_logits"]:
        tid = s.sample(m, lg)
        s.accept(tid)
        got.append(tid)
    assert got == t["sampler_ids"].tolist()


def _tokenizer_sampler_inputs(m):
    """random texts over the golden model's vocabulary, then 400 (logits, top_k) sampling steps with many exact ties"""
    rng = np.random.default_rng(2024)
    pieces = [m.token_text(i) for i in range(m.n_vocab)]
    pieces = [p for p in pieces if p and b"\x00" not in p]
    texts = []
    for _ in range(60):
        text = b"".join(pieces[int(i)] for i in rng.integers(0, len(pieces), int(rng.integers(1, 40))))
        try:
            text.decode()
        except UnicodeDecodeError:
            continue
        texts.append(text)
    steps = []
    for step in range(400):
        lg = (rng.integers(-6, 7, m.n_vocab) * 0.5).astype(np.float32)           # 13 distinct values: ties everywhere
        if step % 3 == 0:
            lg += rng.standard_normal(m.n_vocab).astype(np.float32) * np.float32(0.01)
        steps.append((lg, int(min(m.n_vocab, rng.integers(1, 41)))))
    return texts, steps


SAMPLE_KW = dict(repeat_penalty=1.3, top_p=float(np.float32(0.95)), temp=float(np.float32(0.8)))


@refgolden.computed_by("host.tokenizer_and_sampler")
def _ref_tokenizer_and_sampler(ref, tmp):
    import llama_swift_amd as L
    tmp = pathlib.Path(tmp)
    m, _ = _golden_model(L, tmp)
    texts, steps = _tokenizer_sampler_inputs(m)
    rm = ref.load(str(tmp / "tiny.bin"), 64)
    out = {}
    for bos in (True, False):
        toks = [rm.tokenize(t.decode(), bos) for t in texts]
        out[f"tokens_bos{int(bos)}"] = np.concatenate(toks)
        out[f"lengths_bos{int(bos)}"] = np.array([len(t) for t in toks])
    rs = ref.L.refllama_sampler_new(-1, 64)
    ids = []
    for lg, top_k in steps:
        ids.append(int(ref.L.refllama_sampler_sample(rm.h, rs, lg, SAMPLE_KW["repeat_penalty"], top_k, SAMPLE_KW["top_p"], SAMPLE_KW["temp"])))
        ref.L.refllama_sampler_accept(rs, ids[-1])
    ref.L.refllama_sampler_free(rs)
    rm.close()
    out["sampled_ids"] = np.array(ids)
    return out


def test_tokenizer_and_sampler_against_the_reference_build(L, ref, tmp_path):
    """The host utilities next to the reference's OWN utils.cpp (oracle/_ref; its results stored in tests/golden/ref_outputs.npz): random
    texts over the model's vocabulary, and 400 sampling steps on logits with many exact ties (so that std::partial_sort's handling of
    equal scores at the top_k boundary matters) and repeated tokens in the penalty window -- same ids, same
    mt19937 draws.  (The sampler's window lookup is a byte map here, std::find per logit there.)"""
    want = refgolden.outputs("host.tokenizer_and_sampler", ref, tmp_path)
    m, g = _golden_model(L, tmp_path)
    texts, steps = _tokenizer_sampler_inputs(m)
    assert len(texts) > 40
    for bos in (True, False):
        ends = np.cumsum(want[f"lengths_bos{int(bos)}"])
        assert len(ends) == len(texts)
        for text, e, n in zip(texts, ends, want[f"lengths_bos{int(bos)}"]):
            assert np.array_equal(m.tokenize(text, bos), want[f"tokens_bos{int(bos)}"][e - n:e]), text
    s = L.Sampler(seed=-1, repeat_last_n=64)
    for step, ((lg, top_k), b) in enumerate(zip(steps, want["sampled_ids"].tolist())):
        a = s.sample(m, lg, top_k=top_k, **SAMPLE_KW)
        assert a == b, (step, a, b)
        s.accept(a)


EMPTY_PROMPT_SEEDS = (-1, 0, 1, 7, 12345)


def _empty_prompt_logits(n_vocab):
    rng = np.random.default_rng(5)
    return [[rng.standard_normal(n_vocab).astype(np.float32) for _ in range(8)] for _ in EMPTY_PROMPT_SEEDS]


@refgolden.computed_by("host.empty_prompt")
def _ref_empty_prompt(ref, tmp):
    import ctypes as C
    path = os.path.join(tmp, "tiny.bin")
    np.load(os.path.join(G, "tiny_model.npz"))["model_file"].tofile(path)
    rm = ref.load(path, 64)
    out = {}
    for seed, lgs in zip(EMPTY_PROMPT_SEEDS, _empty_prompt_logits(rm.n_vocab)):
        rs = ref.L.refllama_sampler_new(seed, 64)
        buf = C.create_string_buffer(64)
        ref.L.refllama_sampler_random_prompt(rs, buf, 64)
        out[f"prompt_{seed}"] = np.frombuffer(buf.value, np.uint8)
        ids = []
        for lg in lgs:
            ids.append(int(ref.L.refllama_sampler_sample(rm.h, rs, lg, 1.3, 40, float(np.float32(0.95)), float(np.float32(0.8)))))
            ref.L.refllama_sampler_accept(rs, ids[-1])
        ref.L.refllama_sampler_free(rs)
        out[f"ids_{seed}"] = np.array(ids)
    rm.close()
    return out


def test_empty_prompt_draws_the_reference_random_prompt(L, ref, tmp_path):
    """-[LlamaPredictOperation main] replaces an empty prompt by gpt_random_prompt(rng) (.mm:774-776), which
    consumes one draw of the rng the sampler uses afterwards: same prompt, same sampled ids after it."""
    want = refgolden.outputs("host.empty_prompt", ref, tmp_path)
    m, _ = _golden_model(L, tmp_path)
    for seed, lgs in zip(EMPTY_PROMPT_SEEDS, _empty_prompt_logits(m.n_vocab)):
        s = L.Sampler(seed=seed, repeat_last_n=64)
        assert s.random_prompt() == want[f"prompt_{seed}"].tobytes().decode()
        for lg, b in zip(lgs, want[f"ids_{seed}"].tolist()):
            a = s.sample(m, lg)
            assert a == b
            s.accept(a)


def test_sampler_clamps_top_k_to_the_vocabulary(L, tmp_path):
    """top_k larger than the vocabulary (the bridge hard-codes 40; the reference reads past its candidate
    array there, utils.cpp:389-395) must still return a valid id."""
    import synth
    hp = synth.HParams(n_vocab=32, n_embd=128, n_mult=64, n_head=1, n_layer=1)
    path = str(tmp_path / "v32.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=2))
    rng = np.random.default_rng(1)
    with L.Model(path, n_ctx=8, flags=4) as m:
        s = L.Sampler(seed=3, repeat_last_n=64)
        for _ in range(50):
            tid = s.sample(m, rng.standard_normal(32).astype(np.float32), top_k=40)
            assert 0 <= tid < 32
            s.accept(tid)
        assert 0 <= s.sample(m, rng.standard_normal(32).astype(np.float32), top_k=0) < 32


def test_corrupt_headers_are_load_errors_not_aborts(L, tmp_path):
    """A header with an absurd n_vocab used to reach std::vector::resize and abort the host process through
    the C ABI.  The header's n_rot is NOT validated: the reference reads it (.mm:130) and then rotates
    n_embd / n_head dims regardless (.mm:528), so any value loads and evaluates identically."""
    import synth
    hp = synth.HParams(n_vocab=64, n_embd=128, n_mult=64, n_head=1, n_layer=1)
    path = str(tmp_path / "ok.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=2))
    raw = bytearray(open(path, "rb").read())
    bad = bytearray(raw); bad[4:8] = (0x7fffffff).to_bytes(4, "little")           # n_vocab
    open(str(tmp_path / "bad_vocab.bin"), "wb").write(bad)
    with pytest.raises(L.LlamaHipError, match="bad hyper-parameters") as e:
        L.Model(str(tmp_path / "bad_vocab.bin"), n_ctx=8, flags=4)
    assert e.value.code == -1000
    bad = bytearray(raw); bad[4:8] = (1 << 23).to_bytes(4, "little")              # plausible count, file far too short
    open(str(tmp_path / "bad_vocab2.bin"), "wb").write(bad)
    with pytest.raises(L.LlamaHipError):
        L.Model(str(tmp_path / "bad_vocab2.bin"), n_ctx=8, flags=4)
    odd = bytearray(raw); odd[24:28] = (7).to_bytes(4, "little")                  # n_rot (6th hparam): ignored as in the reference
    open(str(tmp_path / "odd_rot.bin"), "wb").write(odd)
    with L.Model(str(tmp_path / "odd_rot.bin"), n_ctx=8, flags=4) as m:
        assert m.n_embd == 128


def test_host_half_is_clean_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: model-file reader, shard merge, tokenizer, sampler, the bridge's failure path and its whole control flow compiled with
    -fsanitize=address,undefined (device entry points stubbed) and run on a one-part and a two-part file, on corrupted
    headers and on truncated files (memory-error detection for the host shim)."""
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "asan"], check=True)
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    t = synth.random_tensors(hp, seed=3)
    for parts in (1, 2):
        path = str(tmp_path / f"m{parts}.bin")
        synth.write_model(path, hp, t, n_parts=parts)
        r = subprocess.run([os.path.join(csrc, "tools", "host_sanitize"), path, str(parts)], capture_output=True, text=True)
        assert r.returncode == 0 and "clean" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr
        if parts == 1:
            # ... and the generation driver end to end with evals that succeed on made-up logits: the prompt is taken at once, everything but
            # its last nine-token chunk goes through ONE llamahip_eval_chunks call, the last chunk's logits are sampled, one eval per
            # generated token, prompt + generated tokens echoed (the harness checks the call sequence itself; here: that it ran)
            assert "driver with a 40-token prompt: 8 evals (36 tokens in one chunk-exact pass, 4 in the last chunk), 46 token events" in r.stdout, r.stdout
            assert "driver with a 9-token prompt: 7 evals (0 tokens in one chunk-exact pass, 9 in the last chunk)" in r.stdout, r.stdout


def test_device_memory_owner_is_all_or_nothing_under_asan_and_ubsan(built, tmp_path):
    """`make asan`: csrc/dev_owner.h as it is, on counting stub allocators over malloc / free that fail at the k-th call, in the stand-alone
    tools/host_sanitize -- alloc_all over groups of 1, 2 and 12 at every failing call (every slot null, the live count unchanged, the same
    group succeeds afterwards), release, destruction through the release function of each entry's kind; LeakSanitizer clean at exit --
    never loaded into python"""
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.swift_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "asan"], check=True)
    src = open(os.path.join(csrc, "tools", "host_sanitize.cpp")).read()
    assert '#include "../dev_owner.h"' in src and "own.alloc_all(" in src and "own.release(" in src and "g_own_fail_at = k" in src and "{ 1, 2, 12 }" in src
    assert "hip/hip_runtime.h" not in open(os.path.join(csrc, "dev_owner.h")).read()          # the owner compiles without the runtime
    hp = synth.HParams(n_vocab=96, n_embd=256, n_mult=256, n_head=2, n_layer=2)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    r = subprocess.run([os.path.join(csrc, "tools", "host_sanitize"), path, "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout and "device-memory owner: groups of 1, 2 and 12" in r.stdout, r.stdout + r.stderr
    assert "FAILED" not in r.stderr and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stdout + r.stderr


def test_live_allocs_is_exported_and_counts_no_device_memory_for_a_host_only_handle(L, tmp_path):
    hp = synth.HParams(n_vocab=96, n_embd=128, n_mult=64, n_head=1, n_layer=1)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    assert "llamahip_debug_live_allocs" in L.declared_symbols()
    before = L.live_allocs()
    with L.Model(path, n_ctx=8, flags=4):
        assert L.live_allocs() == before
    assert L.live_allocs() == before and before[0] >= 0 and before[1] >= 0


def test_runner_reports_load_failure_like_the_bridge(L, tmp_path):
    states, tokens = [], []
    r = L.LlamaRunner(str(tmp_path / "missing.bin"))
    with pytest.raises(L.LlamaHipError) as e:
        r.run("hello", L.Config(numThreads=8, numTokens=4), tokens.append, lambda s, err: states.append(s))
    assert e.value.code == -1000 and e.value.domain == "com.alexrozanski.llama.error"
    assert states == [L.RunState.notStarted, L.RunState.initializing, L.RunState.failed] and tokens == []
    assert L.Config.default == L.Config(8, 512, None)


def test_compute_entry_points_fail_loudly_without_a_gpu(L):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(L.LlamaHipError) as e:
        L.op_quantize_row_q4_0(np.zeros(32, np.float32))
    assert "no CPU fallback" in e.value.message


def test_eval_entry_points_refuse_a_host_only_handle(L, tmp_path):
    """llamahip_eval / llamahip_eval_chunks / greedy decode on a handle that has no device state (LLAMAHIP_FLAG_HOST_ONLY: the file
    reader alone) are PredictionFailed, never a silent CPU path."""
    hp = synth.HParams(n_vocab=64, n_embd=64, n_mult=32, n_head=2, n_layer=1)
    path = str(tmp_path / "m.bin")
    synth.write_model(path, hp, synth.random_tensors(hp, seed=3))
    with L.Model(path, n_ctx=32, flags=4) as m:          # 4 = LLAMAHIP_FLAG_HOST_ONLY
        for call in (lambda: m.eval(np.arange(3, 8, dtype=np.int32), 0), lambda: m.eval_chunks(np.arange(3, 23, dtype=np.int32), 0, 9),
                     lambda: m.decode_greedy(5, 0, 2)):
            with pytest.raises(L.LlamaHipError) as e:
                call()
            assert e.value.code == -1001


def test_dense_model_files_parse_on_the_host(L, tmp_path):
    """f16 / f32 model files (f16 = 1 / 0) are accepted by the reader; a HOST_ONLY handle serves their
    merged tensors byte for byte (two part files: column and row shards); a header / tensor type mismatch is an error."""
    import synth
    hp = synth.HParams(n_vocab=64, n_embd=256, n_mult=128, n_head=2, n_layer=1)
    t = synth.random_tensors(hp, seed=5)
    for ftype, dt in ((1, np.float16), (0, np.float32)):
        path = str(tmp_path / f"m{ftype}.bin")
        synth.write_model_unquantized(path, hp, t, ftype, n_parts=2)
        with L.Model(path, n_ctx=16, n_parts=2, flags=4) as m:
            for name in ("tok_embeddings.weight", "output.weight", "layers.0.attention.wq.weight", "layers.0.attention.wo.weight",
                         "layers.0.feed_forward.w2.weight", "layers.0.feed_forward.w3.weight"):
                assert m.tensor_bytes(name).tobytes() == np.ascontiguousarray(t[name], dt).tobytes(), (ftype, name)
            assert m.tensor_bytes("norm.weight").tobytes() == np.ascontiguousarray(t["norm.weight"], np.float32).tobytes()
    raw = bytearray(open(str(tmp_path / "m1.bin"), "rb").read())
    raw[28:32] = (3).to_bytes(4, "little")                  # header says Q4_1, tensors are f16: sizes cannot match
    open(str(tmp_path / "q41.bin"), "wb").write(raw)
    with pytest.raises(L.LlamaHipError, match="wrong size"):
        L.Model(str(tmp_path / "q41.bin"), n_ctx=16, n_parts=1, flags=4)


def test_few_row_kernel_plans_every_llama_shape_and_row_count(L):
    """Host-only walk of the few-row mat-mul's plan (csrc/gemv_set.hip set_plan; no device needed): for every matrix of the four LLaMA
    sizes and every row count a short eval or a batched decode step can have (2 .. 60), the kernel takes the shape -- so no eval silently
    falls to the slow generic path -- with an instantiated (columns per wave, column-waves) pair, column groups that cover the rows
    exactly, and operand rows + weight ring inside the CU's 160 KB of LDS (13B / 65B w2 rows are 54 / 86 chunks long: they take
    unshared column groups).  The walk itself lives in tests/variants.py."""
    import variants
    assert variants.walk_set_plans(L) == 4 * 6 * 59
    EPI_RESID, EPI_SILU_QAH = variants.EPI_RESID, variants.EPI_SILU_QAH
    assert L.set_plan(4096, 4096, 1, EPI_RESID) is None and L.set_plan(4096, 4096, 61, EPI_RESID) is None       # one row: k_gemv; 61+: the prompt kernels
    assert L.set_plan(2 * 11008, 4096, 4, EPI_SILU_QAH, False) is None                                           # not the interleaved layout


def _variant_params():
    import variants
    return [pytest.param(env, id=tag) for env, tag in variants.SET_PLAN_VARIANTS]


@pytest.mark.parametrize("env", _variant_params())
def test_few_row_kernel_forced_plans_take_every_shape_too(built, env):
    """The same walk under every environment tests/test_gpu_parity.py::test_few_row_kernel_selectable_epilogues_and_plans forces (one
    list, tests/variants.py): a forced plan that does not fit a shape's LDS budget degrades to the default rule for that shape, it never
    sends the shape to a generic kernel -- the GPU tests assert exactly that through the path counters (switches are read once per
    process, hence the subprocess)."""
    import subprocess
    import sys
    import variants
    r = subprocess.run([sys.executable, os.path.join(variants.HERE, "variants.py"), "walk"], env=dict(os.environ, **env), capture_output=True, text=True, cwd=variants.ROOT)
    assert r.returncode == 0 and "plans walked: 1416" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def _gemv_plan_table():
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemv_plans.json")) as f:
        return json.load(f)


def test_decode_matvec_plan_table_does_not_move(L):
    """The launch plan of the single-row decode mat-vec (csrc/decode.hip gemv_plan: waves, operand budget, ring depth, ring or whole row
    in flight, grid, LDS bytes -- host only) equals, entry for entry, the table recorded from the launchers before they shared one plan
    function (tests/golden/gemv_plans.json; the sweep is tests/variants.py gemv_plan_sweep): every decode matrix of the four LLaMA widths
    and of the synthetic models' widths, the edges of every rule, under every (prologue, epilogue) pair a launcher dispatches.
    Refusals are part of the table."""
    import variants
    table = _gemv_plan_table()
    assert [tuple(r[:5]) for r in table] == [(M, K, int(inter), pre, epi) for M, K, inter, pre, epi in variants.gemv_plan_sweep()]
    assert len(table) > 2000 and sum(r[5] is None for r in table) > 100
    for M, K, inter, pre, epi, want in table:
        got = L.gemv_plan(M, K, pre, epi, bool(inter))
        assert got == (tuple(want) if want else None), (M, K, inter, pre, epi, want, got)


def test_decode_matvec_plans_of_the_llama_sizes(L):
    """The same plans against rows worked out by hand from the launch rules (they agree with the instances
    profiles/r06_kernel_scratch_report.txt recorded on the hardware): nw / pg / depth / ring / grid of every decode mat-vec."""
    import variants as v
    R, W = True, False          # ring | whole row in flight
    want = {
        "7B":  {"wq|wk|wv": (4, 1, 8, R, 384), "wo": (2, 4, 16, W, 256), "w1|w3": (8, 1, 4, R, 344), "w2": (2, 12, 10, R, 256), "output": (4, 1, 4, R, 1000)},
        "13B": {"wq|wk|wv": (4, 2, 10, R, 480), "wo": (2, 4, 10, R, 320), "w1|w3": (8, 1, 4, R, 432), "w2": (2, 12, 10, R, 320), "output": (4, 2, 4, R, 1000)},
        "30B": {"wq|wk|wv": (4, 2, 4, R, 624), "wo": (2, 4, 10, R, 416), "w1|w3": (8, 1, 4, R, 560), "w2": (2, 12, 10, R, 416), "output": (4, 2, 4, R, 1000)},
        "65B": {"wq|wk|wv": (4, 2, 4, R, 768), "wo": (4, 4, 8, R, 256), "w1|w3": (8, 1, 4, R, 688), "w2": (4, 12, 10, R, 256), "output": (4, 2, 4, R, 1000)},
    }
    pairs = {"wq|wk|wv": (v.PREP_NORM, v.EPI_STORE), "wo": (v.PRE_QA, v.EPI_RESID), "w1|w3": (v.PREP_NORM, v.EPI_SILU_QA), "w2": (v.PRE_QA, v.EPI_RESID),
             "output": (v.PREP_NORM, v.EPI_STORE)}
    for size, d in v.LLAMA_WIDTHS.items():
        for name, (M, K, inter) in v.llama_matrices(d).items():
            pre, epi = pairs[name]
            p = L.gemv_plan(M, K, pre, epi, inter)
            assert p is not None and p[:5] == tuple(int(x) for x in want[size][name]), (size, name, p, want[size][name])


def test_decode_matvec_plans_name_kernels_that_exist(L):
    """Every plan of the table names an instance of k_gemv that was compiled: the launchers look their kernel up by the plan, so a plan
    without one would be refused at launch (llamahip_debug_gemv_plan returns -1 for it) -- the single-row counterpart of the few-row walk."""
    import ctypes as C
    f = L.lib().llamahip_debug_gemv_plan
    f.restype, f.argtypes = C.c_int32, [C.c_int32] * 5 + [C.c_void_p]
    out = np.zeros(6, np.int64)
    n = 0
    for M, K, inter, pre, epi, want in _gemv_plan_table():
        rc = f(M, K, inter, pre, epi, out.ctypes.data_as(C.c_void_p))
        assert rc == (1 if want else 0), (M, K, inter, pre, epi, want, rc, out.tolist())
        n += rc
    assert n > 1000
