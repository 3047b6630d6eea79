"""GPU: the handle's device memory, captured steps and events have one owner each (csrc/dev_owner.h, host_util.h GraphCache / Events).

What the ownership has to guarantee and a reader of the code cannot see from a passing parity test: a workspace that grows drops every
captured step that holds its old pointers (the decode loop's and a bound slot's), the least recently used set step is evicted and
captured again without disturbing any slot, and a handle that is freed gives back every allocation it made -- counted by the library
itself (llamahip_debug_live_allocs), since free device memory as the runtime reports it moves with every other process on the card.
Out-of-memory behaviour is checked on the CPU (tools/host_sanitize, test_host.py); nothing here tries to exhaust the device.

One tiny synthetic Q4_0 model: 2 layers, n_embd 256 with head size 128 (the fused decode launch and the set steps apply), n_ctx 64, 6 slots."""
import itertools

import numpy as np
import pytest

import synth

N_CTX, N_SEQ, NTH = 64, 6, 8
HP = synth.HParams(n_vocab=96, n_embd=256, n_mult=64, n_head=2, n_layer=2)
PROMPT = synth.synth_prompt(5, HP.n_vocab, seed=11)
LONG = synth.synth_prompt(17, HP.n_vocab, seed=12)          # one row more than the workspace a load allocates: the eval regrows it
K = 6


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("own") / "m.bin")
    synth.write_model(p, HP, synth.random_tensors(HP, seed=41))
    return p


def _stage_steps(gm, torch, buf, first, n_past, k):
    """slot 0 bound at n_past to the token word `buf` holding `first`, k single steps: (picks, logits of the last step)"""
    buf.fill_(first)
    torch.cuda.synchronize()
    gm.stage_bind(0, n_past, token_in=buf.data_ptr(), token_out=buf.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(k):
        gm.stage_step(0, NTH, st)
    n, pos, got = gm.stage_trace(0, k)
    assert n == k and pos == n_past + k
    return got.copy(), gm.stage_logits(0)


@pytest.fixture(scope="module")
def fresh(L, path):
    """what a handle that never regrew anything gives: the first token, decode_greedy's K tokens and last logits, a bound slot's K steps"""
    import torch
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as gm:
        first = int(np.argmax(gm.eval(PROMPT, 0, NTH)))
        toks, logits = gm.decode_greedy(first, len(PROMPT), K, NTH, want_logits=True)
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as gm:
        assert int(np.argmax(gm.eval(PROMPT, 0, NTH))) == first
        s_toks, s_logits = _stage_steps(gm, torch, torch.zeros(1, dtype=torch.int32, device="cuda"), first, len(PROMPT), K)
    return {"first": first, "toks": toks, "logits": logits, "s_toks": s_toks, "s_logits": s_logits}


def _regrow(gm):
    """a 17-token eval in another KV slot: the workspace grows, slot 0's cache stays as it is"""
    gm.set_seq(1)
    gm.eval(LONG, 0, NTH)
    gm.set_seq(0)


@pytest.mark.gpu
def test_regrown_workspace_drops_the_captured_decode_step(L, path, fresh):
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as gm:
        assert int(np.argmax(gm.eval(PROMPT, 0, NTH))) == fresh["first"]
        t0, l0 = gm.decode_greedy(fresh["first"], len(PROMPT), K, NTH, want_logits=True)          # captures
        _regrow(gm)
        t1, l1 = gm.decode_greedy(fresh["first"], len(PROMPT), K, NTH, want_logits=True)          # same key: a stale exec would replay on freed buffers
    assert same(t0, fresh["toks"]) and same(l0, fresh["logits"])
    assert same(t1, fresh["toks"]), (t1.tolist(), fresh["toks"].tolist())
    assert same(l1, fresh["logits"])


@pytest.mark.gpu
def test_regrown_workspace_drops_a_bound_slots_captured_step(L, path, fresh):
    import torch
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as gm:
        assert int(np.argmax(gm.eval(PROMPT, 0, NTH))) == fresh["first"]
        buf = torch.zeros(1, dtype=torch.int32, device="cuda")
        t0, l0 = _stage_steps(gm, torch, buf, fresh["first"], len(PROMPT), K)          # captures
        _regrow(gm)
        t1, l1 = _stage_steps(gm, torch, buf, fresh["first"], len(PROMPT), K)          # bound to the same buffers again: the bind drops nothing itself
    assert same(t0, fresh["s_toks"]) and same(l0, fresh["s_logits"])
    assert same(t1, fresh["s_toks"]), (t1.tolist(), fresh["s_toks"].tolist())
    assert same(l1, fresh["s_logits"])
    assert same(fresh["s_toks"], fresh["toks"])          # (the slot's steps are the greedy loop's)


def _bind_all(gm, torch, firsts, prompts):
    bufs = [torch.tensor([firsts[s]], dtype=torch.int32, device="cuda") for s in range(N_SEQ)]
    for s in range(N_SEQ):
        gm.stage_bind(s, len(prompts[s]), token_in=bufs[s].data_ptr(), token_out=bufs[s].data_ptr())
    return bufs


@pytest.mark.gpu
def test_set_step_eviction_and_recapture_leave_every_slot_as_stepped_alone(L, path):
    """33 distinct sets of 2 .. 3 of the 6 slots, one step each -- one more than the cache of captured set steps holds, so the first set is
    evicted -- then the first set again (captured again).  Every slot's picks equal stepping that slot alone on a second handle.
    (The capture count behind llamahip_sched_get_stats covers a scheduler's own steps only; from the binding the traces are what shows.)"""
    import torch
    prompts = [synth.synth_prompt(2 + s, HP.n_vocab, seed=70 + s) for s in range(N_SEQ)]
    sets = [list(c) for c in itertools.combinations(range(N_SEQ), 2)] + [list(c) for c in itertools.combinations(range(N_SEQ), 3)]
    sets = sets[:33] + [sets[0]]
    assert len({tuple(s) for s in sets[:33]}) == 33 and all(2 <= len(s) <= 3 for s in sets)
    n_steps = [sum(s in st for st in sets) for s in range(N_SEQ)]
    assert all(len(prompts[s]) + n_steps[s] < N_CTX for s in range(N_SEQ))

    def prepare(gm):
        firsts = []
        for s in range(N_SEQ):
            gm.set_seq(s)
            firsts.append(int(np.argmax(gm.eval(prompts[s], 0, NTH))))
        gm.set_seq(0)
        return firsts

    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as gm:
        assert gm.stage_set_applies(2, NTH) and gm.stage_set_applies(3, NTH)
        firsts = prepare(gm)
        bufs = _bind_all(gm, torch, firsts, prompts)
        st = torch.cuda.current_stream().cuda_stream
        for sq in sets:
            gm.stage_step_set(sq, NTH, st)
        got = [gm.stage_trace(s, n_steps[s]) for s in range(N_SEQ)]
    with L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ) as alone:
        assert prepare(alone) == firsts
        bufs2 = _bind_all(alone, torch, firsts, prompts)
        st = torch.cuda.current_stream().cuda_stream
        for s in range(N_SEQ):
            for _ in range(n_steps[s]):
                alone.stage_step(s, NTH, st)
        want = [alone.stage_trace(s, n_steps[s]) for s in range(N_SEQ)]
    del bufs, bufs2
    for s in range(N_SEQ):
        assert got[s][0] == want[s][0] == n_steps[s] and got[s][1] == want[s][1] == len(prompts[s]) + n_steps[s]
        assert got[s][2].tolist() == want[s][2].tolist(), f"slot {s}"


def _walk_the_surface(L, gm, pipeline):
    """one call of every family at its smallest arguments: whatever each allocates lazily is allocated"""
    import torch
    V = gm.n_vocab
    first = int(np.argmax(gm.eval(PROMPT, 0, NTH)))
    gm.eval_chunks(LONG, 0, 9, NTH)
    gm.eval_topk(PROMPT[:2], 0, L.Sampler(seed=1), n_threads=NTH)
    gm.eval_logprobs(PROMPT, 0, NTH)
    gm.decode_greedy(first, len(PROMPT), 2, NTH)
    if not pipeline:          # (stage steps are a stage handle's: an in-process pipeline handle steps its own stages)
        buf = [torch.tensor([first], dtype=torch.int32, device="cuda") for _ in range(2)]
        for s in range(2):
            gm.stage_bind(s, 1, token_in=buf[s].data_ptr(), token_out=buf[s].data_ptr())
        st = torch.cuda.current_stream().cuda_stream
        gm.stage_step(0, NTH, st)
        gm.stage_step_set([0, 1], NTH, st)
        gm.stage_trace(0, 1)
    gm.verify_greedy(first, [1, 2], len(PROMPT), NTH)
    gm.decode_sample_multi([first, first], [1, 1], 2, [L.Sampler(seed=2), L.Sampler(seed=3)], n_threads=NTH)
    gm.eval_multi([0, 1], [0, 0], [PROMPT, PROMPT[:3]], n_threads=NTH)
    with gm.scheduler(2, n_threads=NTH) as sc:
        sc.submit(PROMPT[:3], 2)
        sc.step()
    assert 0 <= first < V


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [False, True], ids=["plain", "two_stages_one_device"])
def test_a_freed_handle_gives_back_every_allocation(L, path, pipeline):
    before = L.live_allocs()
    gm = L.Model(path, n_ctx=N_CTX, n_seq=N_SEQ, devices=[0, 0] if pipeline else None)
    loaded = L.live_allocs()
    assert loaded[0] > before[0] and loaded[1] > before[1]
    _walk_the_surface(L, gm, pipeline)
    assert L.live_allocs()[0] > loaded[0]          # the lazily allocated groups are counted too
    gm.close()
    assert L.live_allocs() == before


@pytest.mark.gpu
def test_single_op_calls_give_back_their_scratch(L):
    before = L.live_allocs()
    rng = np.random.default_rng(5)
    logits = rng.standard_normal(96).astype(np.float32)
    L.op_topk(logits, np.array([1, 2, 3], np.int32))
    L.op_logprob(rng.standard_normal((3, 96)).astype(np.float32), np.array([1, 2, 3], np.int32))
    assert L.live_allocs() == before
