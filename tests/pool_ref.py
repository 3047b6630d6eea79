"""The float64 numpy restatement of csrc/pool.hip -- the tail an embedding pass runs in place of the lm head -- for the tests of
llamahip_op_pool_rows and llamahip_text_embedding[_multi].

  norm   the reference's sequential form: the oracle's unary_rows("norm", x) (ggml.c:5327-5385) times norm_w in float32 (ggml_mul).  The
         kernel folds its two double sums in its own order, so equality is asked only on rows that are order-proof (prep_cases.norm_stats).
  LAST   the segment's last row.
  MEAN   acc = 0.0; acc += float64(y[j][c]) for j ascending over the segment's rows; o[c] = float32(acc / float64(n_rows)).
  L2     lane l of 64 sums float64(o[c]) * float64(o[c]) over c = l, l + 64, ... ascending; the 64 partials are folded by the xor butterfly
         32, 16, 8, 4, 2, 1 (lane l takes s[l] + s[l ^ m]); out[c] = float32(float64(o[c]) / sqrt(ss)); ss == 0.0 leaves the row."""
import numpy as np

POOL_LAST, POOL_MEAN = 0, 1
POOLS = {"last": POOL_LAST, "mean": POOL_MEAN}


def norm_rows(oracle, x, w):
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(oracle.unary_rows("norm", x) * np.asarray(w, np.float32)[None, :], np.float32)


def pool_segment(y, pool):
    """y float32 [n, d]: the rows of one segment, already normed"""
    if POOLS.get(pool, pool) == POOL_LAST:
        return y[-1].copy()
    acc = np.zeros(y.shape[1], np.float64)
    with np.errstate(all="ignore"):
        for j in range(y.shape[0]):
            acc = acc + y[j].astype(np.float64)
        return (acc / np.float64(y.shape[0])).astype(np.float32)


def l2_normalize(o):
    d = o.size
    od = o.astype(np.float64)
    with np.errstate(all="ignore"):
        s = np.zeros(64, np.float64)
        for c0 in range(0, d, 64):          # ascending per lane
            blk = od[c0:c0 + 64]
            s[:blk.size] = s[:blk.size] + blk * blk
        lanes = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            s = s + s[lanes ^ m]
        ss = s[0]
        if ss == 0.0:
            return o.copy()
        return (od / np.sqrt(ss)).astype(np.float32)


def pool_normed(y, seg_begin, pool, normalize):
    """y float32 [R, d] normed rows -> [n_segs, d]"""
    out = np.stack([pool_segment(y[seg_begin[s]:seg_begin[s + 1]], pool) for s in range(len(seg_begin) - 1)])
    if normalize:
        out = np.stack([l2_normalize(r) for r in out])
    return np.ascontiguousarray(out, np.float32)


def pool_rows(oracle, x, w, seg_begin, pool, normalize):
    """x float32 [R, d] hidden rows -> the embeddings [n_segs, d]"""
    return pool_normed(norm_rows(oracle, x, w), seg_begin, pool, normalize)
