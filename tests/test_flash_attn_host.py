"""CPU: what llamahip_op_flash_attention refuses before any device is touched, each with the limit in its message; the launch plan of
k_flash_attn (flash_attn_plan) over the 7B / 13B / 65B head counts; the flag and the counter as the package exports them."""
import numpy as np
import pytest

CUS, KEY_TILE, KS_CAP = 256, 64, 8


def test_refusals_name_their_limit(L):
    qkv = np.zeros((64, 3 * 256), np.float32)
    cache = lambda: (np.zeros((128, 256), np.float32), np.zeros((128, 256), np.float32))
    with pytest.raises(L.LlamaHipError, match=r"head size 64: the kernel takes head size 128"):
        L.op_flash_attention(qkv, 4, 0, *cache())
    with pytest.raises(L.LlamaHipError, match=r"N 1: the kernel takes N >= 2 rows"):
        L.op_flash_attention(qkv[:1], 2, 0, *cache())
    with pytest.raises(L.LlamaHipError, match=r"T = n_past \+ N = 129 > n_ctx 128"):
        L.op_flash_attention(qkv, 2, 65, *cache())
    with pytest.raises(L.LlamaHipError, match=r"tile 32 is not an instance"):
        L.op_flash_attention(qkv, 2, 0, *cache(), tile=32)
    with pytest.raises(L.LlamaHipError, match=r"key_splits 9 outside 0 \.\. 8"):
        L.op_flash_attention(qkv, 2, 0, *cache(), key_splits=9)
    with pytest.raises(L.LlamaHipError, match=r"merged_stride 255 < d 256"):
        L.op_flash_attention(qkv, 2, 0, *cache(), merged_stride=255)


@pytest.mark.parametrize("H", [32, 40, 64])
@pytest.mark.parametrize("N", [64, 128, 512, 2048])
@pytest.mark.parametrize("n_past", [0, 1984])
def test_the_plan_rule(L, H, N, n_past):
    T = n_past + N
    p = L.flash_attn_plan(N, T, H)
    wgs = lambda tile: H * -(-N // tile)
    assert p["tile"] == (128 if wgs(128) >= CUS else 64)                      # the widest tile that still makes a workgroup for every CU
    w, key_tiles, ks = wgs(p["tile"]), -(-T // KEY_TILE), p["key_splits"]
    assert 1 <= ks <= min(key_tiles, KS_CAP)
    assert ks == 1 or w * (ks - 1) < CUS                                      # ... then the smallest split count that does
    assert w * ks >= CUS or ks == min(key_tiles, KS_CAP)                      # (short of it only at a cap)
    assert p["query_tiles"] == -(-N // p["tile"]) and p["workgroups"] == w * ks
    assert p["lds_bytes"] * 2 <= 160 * 1024                                   # two workgroups per CU
    assert p["ws_bytes"] >= (ks * H * N * (128 + 2) * 4 if ks > 1 else 0)


def test_no_plan_and_the_exports(L):
    assert L.flash_attn_plan(1, 1, 32) is None and L.flash_attn_plan(64, 63, 32) is None and L.flash_attn_plan(64, 64, 0) is None
    assert L.FAST_ATTN == 64 and L.FAST_ATTN & (L.FAST_DENSE | 16) == 0
    assert isinstance(L.flash_attn_launches(), int) and L.flash_attn_launches() >= 0
