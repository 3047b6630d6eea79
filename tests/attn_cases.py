"""Inputs of one layer's attention for the op-level attention tests (test_oracle_vs_ref.py, test_gpu_attention.py).

make() returns the un-rotated q|k|v rows of an eval ([N][3d], as the wq|wk|wv product) and K / V caches of n_ctx rows: rows below n_past
hold earlier (rotated) keys and values, rows from n_past + N on hold CANARY, a NaN the reference never reads.  oracle_side() runs what the
model does with them on the CPU: RoPE (orc_rope, mode 0 for q, mode 1 for the new cache rows), the append and orc_attention.

Value regimes (numbers the random model weights never produce):
  plain    random values
  wide     score spreads of ~40: exp table entries become subnormal or 0
  ties     scores 0 at the row maximum on several keys (the first visible key and every new key among them), negative elsewhere
  leak     keys beyond a query's position score higher the later they are: a leaked mask changes the maximum
  negzero  V columns of -2^-149 (products round to -0, chains end in -0), of -0, of subnormals of both signs, and of -2^-149 up to a
           key and positive values after it (the masked tail of a row decides the sign of its sum)
  zeroq    q rows all zero (uniform weights)"""
import numpy as np

CANARY = np.uint32(0x7FC0BEEF)
REGIMES = ("plain", "wide", "ties", "leak", "negzero", "zeroq")


def _f(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def make(regime, N, d, H, n_past, n_ctx, seed=0):
    dh = d // H
    T = n_past + N
    assert T <= n_ctx
    rng = np.random.default_rng([seed, N, d, H, n_past, REGIMES.index(regime)])
    q = rng.standard_normal((N, d)).astype(np.float32)
    k = rng.standard_normal((N, d)).astype(np.float32)
    v = rng.standard_normal((N, d)).astype(np.float32)
    Kc = np.full((n_ctx, d), _f(CANARY), np.float32)
    Vc = np.full((n_ctx, d), _f(CANARY), np.float32)
    Kc[:n_past] = rng.standard_normal((n_past, d))
    Vc[:n_past] = rng.standard_normal((n_past, d))
    if regime == "wide":
        q *= np.float32(6.0 * np.sqrt(dh) / np.sqrt(dh / 2))          # scores of standard deviation ~8: spreads well beyond 20
    elif regime in ("ties", "leak"):
        # only the last rotation pair (the slowest angle: < 0.25 rad at position 2 048) carries q and k, so signs survive RoPE
        lp = [h * dh + dh - 2 for h in range(H)]
        q[:] = 0
        k[:] = 0
        Kc[:n_past] = 0
        for c in lp:
            q[:, c] = rng.uniform(0.5, 3.0, N)
            if regime == "ties":
                # old keys: 0 (a tie at the maximum, key 0 always among them) or negative; new keys: 0 (each query's own key ties)
                loser = rng.random(n_past) < 0.5
                loser[0] = False
                Kc[:n_past, c] = np.where(loser, -rng.uniform(0.1, 2.0, n_past), 0.0)
            else:
                Kc[:n_past, c] = rng.uniform(-2.0, 0.0, n_past)
                k[:, c] = 0.5 + 0.25 * np.arange(N)                      # later keys score higher
    elif regime == "negzero":
        q *= np.float32(0.05)                                           # near-uniform weights: every p <= 1/2 once a row sees two keys
        Vall = np.concatenate([Vc[:n_past], v])
        cols = np.arange(d)
        kind = cols % 5
        tiny_neg, tiny_pos = _f(0x80000001), _f(0x00000001)
        Vall[:, kind == 0] = tiny_neg
        Vall[:, kind == 1] = _f(0x80000000)
        sub = rng.integers(1, 1 << 23, (T, d)).astype(np.uint32) | (rng.integers(0, 2, (T, d)).astype(np.uint32) << 31)
        Vall[:, kind == 2] = _f(sub)[:, kind == 2]
        # -2^-149 up to key b, then values >= +0: a row whose visible keys all lie below b ends in -0 only if its masked tail is not walked
        b = n_past + (37 * cols + 11) % N
        tail = np.arange(T)[:, None] >= b[None, :]
        later = np.where(cols % 10 == 3, np.float32(1.0), np.where(cols % 10 == 8, _f(0x00000000), tiny_pos))
        m3 = kind == 3
        Vall[:, m3] = np.where(tail[:, m3], later[None, m3], tiny_neg)
        Vc[:n_past], v = Vall[:n_past], Vall[n_past:]
    elif regime == "zeroq":
        q[::2] = 0
        q[-1] = 0
    qkv = np.ascontiguousarray(np.concatenate([q, k, v], axis=1), np.float32)
    return qkv, Kc, Vc


def oracle_side(oracle, qkv, Kc, Vc, H, n_past, n_threads, chunk=0):
    """(merged [N][d], Kc, Vc after the append) as the model computes them, on the CPU"""
    N, d3 = qkv.shape
    d = d3 // 3
    dh = d // H
    T = n_past + N
    qr = oracle.rope(qkv[:, :d].reshape(N, H, dh), n_past, 0).reshape(N, d)
    Kc, Vc = Kc.copy(), Vc.copy()
    Kc[n_past:T] = qkv[:, d:2 * d]
    Vc[n_past:T] = qkv[:, 2 * d:]
    Kc[:T] = oracle.rope(Kc[:T].reshape(T, H, dh), n_past, 1).reshape(T, d)
    return oracle.attention(qr, Kc, Vc, H, n_past, n_threads, chunk), Kc, Vc, qr
