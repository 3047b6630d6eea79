"""GPU (-m gpu): llamahip_op_sched_pick -- the pick half of k_sched_pick, one wave per row -- against llamahip_op_verify_rows' picks on the
same rows (k_verify_rows: the rule both kernels take from one device function), and against the rule written out on the host: the largest
value, the lowest index on ties, +0 == -0, a NaN never, index 0 where nothing can be taken.  picks[r] = -1 where emit[r] == 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROWS = (1, 2, 16)
VOCABS = (1, 65, 1500, 32000)


def rule(row):
    """k_argmax's rule on the host"""
    ok = ~np.isnan(row)          # (a NaN is never taken)
    if not ok.any():
        return 0
    return int(np.flatnonzero(ok & (row == row[ok].max()))[0])          # (+0 == -0: the lower index)


def rows_of(rng, R, V):
    """R rows: plain; ties at the first and the last index; +0 / -0; a NaN among finite values; all -inf; a +inf; all NaN -- in turn"""
    lg = (rng.standard_normal((R, V)) * 3).astype(np.float32)
    for r in range(R):
        kind = r % 8
        if kind == 1:          # the maximum at the first and the last index (and once in between)
            lg[r] = np.minimum(lg[r], 5.0)
            lg[r, 0] = lg[r, V - 1] = lg[r, V // 2] = 7.5
        elif kind == 2:        # the maximum at the last index only, a tie of lower values at the front
            lg[r] = np.minimum(lg[r], 5.0)
            lg[r, 0] = lg[r, min(1, V - 1)] = 6.0
            lg[r, V - 1] = 6.5
        elif kind == 3:        # nothing above zero: -0 first, +0 later -- equal values, the lower index wins
            lg[r] = -np.abs(lg[r]) - 1.0
            lg[r, V // 3] = -0.0
            lg[r, V - 1] = 0.0
        elif kind == 4:        # a NaN among finite values, in front of the maximum
            lg[r, 0] = np.nan
            lg[r, V // 2] = np.nan
        elif kind == 5:
            lg[r] = -np.inf
        elif kind == 6:
            lg[r, (2 * V) // 3] = np.inf
        elif kind == 7:
            lg[r] = np.nan
    return lg


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("R", ROWS)
def test_picks_are_verify_rows_picks(L, R, V):
    rng = np.random.default_rng(1000 * R + V)
    for rep in range(8 // R if R < 8 else 1):
        lg = rows_of(rng, max(R, 8), V)
        if R < 8:          # few rows: walk the eight kinds over the repetitions
            lg = np.ascontiguousarray(lg[[(rep * R + r) % 8 for r in range(R)]])
        _, want = L.op_verify_rows(lg, np.zeros(R, np.int32))
        host = [rule(lg[r]) for r in range(R)]
        assert want.tolist() == host, (R, V, "the yardstick kernel against the rule")
        for name, emit in (("all", np.ones(R, np.int32)), ("none", np.zeros(R, np.int32)), ("alternating", (np.arange(R) % 2 == 0).astype(np.int32)),
                           ("alternating_odd", (np.arange(R) % 2 == 1).astype(np.int32))):
            got = L.op_sched_pick(lg, emit)
            for r in range(R):
                assert got[r] == (want[r] if emit[r] else -1), (R, V, name, r, got.tolist(), want.tolist())


def test_every_kind_of_row_at_every_vocabulary(L):
    """each of the eight kinds as the only row, and all eight together with emit flags of 2 (any non-zero value emits)"""
    rng = np.random.default_rng(7)
    for V in VOCABS:
        lg = rows_of(rng, 8, V)
        want = [rule(lg[r]) for r in range(8)]
        assert L.op_sched_pick(lg, np.full(8, 2, np.int32)).tolist() == want, V
        for r in range(8):
            assert L.op_sched_pick(lg[r:r + 1], [1]).tolist() == [want[r]], (V, r)
    # what the kinds are there for
    lg = rows_of(rng, 8, 1500)
    got = L.op_sched_pick(lg, np.ones(8, np.int32)).tolist()
    assert got[1] == 0 and got[2] == 1499 and got[3] == 500 and got[5] == 0 and got[6] == 1000 and got[7] == 0 and got[4] not in (0, 750)


def test_refusals(L):
    lg = np.zeros((17, 8), np.float32)
    with pytest.raises(L.LlamaHipError):
        L.op_sched_pick(lg, np.ones(17, np.int32))          # more than 16 rows
    with pytest.raises(ValueError):
        L.op_sched_pick(lg[:2], [1])
    err = __import__("ctypes").create_string_buffer(256)
    assert L.lib().llamahip_op_sched_pick(None, 1, 8, None, None, err, len(err)) == L.binding.ERR_PREDICT
