"""GPU (-m gpu): k_kv_shift_rows op by op (llamahip_op_kv_shift) against the float64 numpy restatement, bit for bit.

Caches of n_ctx 40, 3 layers (an odd count), 3 slots, at d 128 / dh 64 and d 384 / dh 128 (three heads; a row that is not a power of two in
bytes): K is oracle.rope of random rows at their positions in three magnitude regimes with some exact +-0.0 pairs, V random, so no byte is a
constant fill (tests/kv_shift_ref.py, whose own properties tests/test_kv_shift_host.py checks on the CPU).  In every case the destination
rows equal the restatement's bytes, EVERY OTHER BYTE of every slot, layer and array is unchanged, and the moved K rows stay within the
derived bound of oracle.rope at the new positions.  The geometry covers the in-place hazard from disjoint ranges down to n_discard = 1,
the kernel's own batch edges (rows in flight U), long shifts whose ranges do not alias at n_ctx 160 (33 .. 80 rows: what every crossing
at a real context size is), alone, beside an aliasing shift and among 16 shifts in one call, and one case at d 4096."""
import numpy as np
import pytest

import kv_shift_ref as R

pytestmark = pytest.mark.gpu
_CACHES = {}


def caches(oracle, n_slots, n_layers, n_ctx, d, dh):
    """computed once per shape, shared and left unchanged"""
    key = (n_slots, n_layers, n_ctx, d, dh)
    if key not in _CACHES:
        _CACHES[key] = R.make_caches(oracle, 77, *key)
        for a in _CACHES[key]:
            a.setflags(write=False)
    return _CACHES[key]


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("case", R.op_cases(), ids=[c[0] for c in R.op_cases()])
def test_shifted_rows_are_the_restatements_bytes_and_nothing_else_changes(L, oracle, case):
    assert R.U == L.KV_SHIFT_ROWS_IN_FLIGHT
    _, n_slots, n_layers, n_ctx, d, dh, shifts = case
    raw, K0, V0 = caches(oracle, n_slots, n_layers, n_ctx, d, dh)
    wantK, wantV = K0.copy(), V0.copy()
    R.shift_restated(wantK, wantV, L.rope_table(n_ctx, dh), dh, shifts)
    K, V = K0.copy(), V0.copy()
    L.op_kv_shift(K, V, dh, shifts)
    for slot, rb, n, nd in shifts:
        for il in range(n_layers):
            dst = slice(rb - nd, rb - nd + n)
            assert same(K[slot, il, dst], wantK[slot, il, dst]), (case[0], "K", slot, il, np.flatnonzero(np.any(K[slot, il, dst] != wantK[slot, il, dst], axis=1))[:8])
            assert same(V[slot, il, dst], wantV[slot, il, dst]), (case[0], "V", slot, il)
            if n:
                worst = R.within_bound(K[slot, il, dst], R.direct_keys(oracle, raw[slot, il, rb:rb + n], rb - nd, dh), raw[slot, il, rb:rb + n])
                assert worst < 3.5, (case[0], slot, il, worst)
    # every byte, the destinations included: outside them the restatement left the original
    assert same(K, wantK) and same(V, wantV), case[0]
