"""GPU (-m gpu): the embedding gathers of f16 / f32 / Q4_1 model files alone -- k_embed_dense<f32>, k_embed_dense<f16>, k_embed_q41
(llamahip_op_embed_dense) -- against what ggml_get_rows leaves: f32 a copy, f16 the exact widening (every fp16 subnormal, +-0, +-inf and a
NaN in one row), Q4_1 the reference build's own dequantize_row_q4_1, read from tests/golden/ref_outputs_dense_op.npz: the store, not this
file, decides whether `(float) code * d + m` is one rounding or two (tests/test_dense_op_host.py holds dense_cases.dequant_q41 against the
same store for every case, so a difference here names the element).  Finite values bit for bit, non-finite ones by class.

V 37; d 32, 96, 288 (nine blocks), 4096, 4128 (not a multiple of 256: the last block of the 256-thread loop is partial); N 1, 2, 13 with
tokens 0, V - 1 and repeats; rows d and d + 8 apart.  The kernels write dense [N][d] rows on the device, which the op places x_stride apart;
behind them the op keeps 64 guard floats and fails if one changed."""
import numpy as np
import pytest

import dense_cases as dc
import refgolden
import test_dense_op_host as host

pytestmark = pytest.mark.gpu
CANARY = np.uint32(0x7FC0BEEF)


@pytest.fixture(scope="module")
def tables():
    """(wtype, d) -> (table, its rows as the gather must leave them [V, d]); computed once"""
    out = {}
    for wtype in dc.EMBED_WTYPES:
        for d in dc.EMBED_DS:
            t = dc.embed_table(wtype, d)
            out[(wtype, d)] = (t, dc.embed_rows(wtype, t))
    return out


@pytest.mark.parametrize("N", dc.EMBED_NS)
@pytest.mark.parametrize("d", dc.EMBED_DS)
@pytest.mark.parametrize("wtype", dc.EMBED_WTYPES, ids=[dc.ENAMES[w] for w in dc.EMBED_WTYPES])
def test_embed_dense(L, ref, tmp_path, tables, wtype, d, N):
    table, rows = tables[(wtype, d)]
    tokens = np.array(dc.EMBED_TOKENS[N], np.int32)
    want = rows[tokens]
    if wtype == 3:          # the reference build's own rows decide
        stored = refgolden.outputs("dense_op.get_rows", host.live(ref), tmp_path, dc.embed_id((wtype, d, N)))["x"]
        assert not dc.agrees_with_stored(want, stored), "dense_cases.dequant_q41 is not the reference's dequantize_row_q4_1"
        if want.size <= dc.FULL_MAX:
            want = stored
    for stride in (d, d + 8):
        x = L.op_embed_dense(tokens, table, stride, np.full((N, stride), CANARY, np.uint32).view(np.float32))
        assert x.shape == (N, stride)
        assert np.all(x[:, d:].view(np.uint32) == CANARY), "the floats between the rows were written"
        assert np.all(x[:, :d].view(np.uint32) != CANARY), "a float of a row was not written"
        assert not len(dc.differ(x[:, :d], want)), f"{dc.embed_id((wtype, d, N))} stride {stride}: {dc.first_diff(x[:, :d], want)}"


def test_out_of_range_tokens_are_refused_without_a_launch(L, tables):
    for wtype in dc.EMBED_WTYPES:
        table, _ = tables[(wtype, 32)]
        for bad in ([dc.EMBED_V], [0, -1], [3, 2 ** 31 - 1]):
            with pytest.raises(L.LlamaHipError, match=r"outside \[0, 37\)"):
                L.op_embed_dense(bad, table)
