"""The float64 reference of one layer's attention and its error bound, shared by the op-level attention tests (test_gpu_attention.py,
test_gpu_dec_attn_op.py).  tests/test_gpu_attention.py's docstring derives the bound; the 1.25 factor is part of it."""
import numpy as np

EPS = 2.0 ** -24


def f64_reference(qr, K, V, H, n_past, nth):
    """(float64 attention [N][d], its error bound [N][d], the change of dropping each row's largest key [N][d])"""
    N, d = qr.shape
    dh, T = d // H, n_past + N
    scale = np.float64(np.float32(1.0) / np.sqrt(np.float32(d / H)))
    q = qr.astype(np.float64).reshape(N, H, dh)
    k = K[:T].astype(np.float64).reshape(T, H, dh)
    v = V[:T].astype(np.float64).reshape(T, H, dh)
    gamma = lambda m: m * EPS / (1 - m * EPS)
    s = np.einsum("nhi,thi->hnt", q, k) * scale
    ds = gamma(dh // 32 + 6) * scale * np.einsum("nhi,thi->hnt", np.abs(q), np.abs(k)) + 2 * EPS * np.abs(s)
    vis = np.arange(T)[None, :] <= (n_past + np.arange(N))[:, None]
    s = np.where(vis[None], s, -np.inf)
    ds = np.where(vis[None], ds, 0.0)
    m = s.max(axis=2, keepdims=True)
    dsm = np.take_along_axis(ds, s.argmax(axis=2)[..., None], axis=2)
    x = s - m
    e = np.where(vis[None], np.exp(x), 0.0)
    dx = np.where(vis[None], 2.0 ** -11 * (np.abs(np.where(vis[None], x, 0.0)) + ds + dsm) + ds + dsm, 0.0)
    r = np.expm1(dx) + 2.0 ** -11 + 2.0 ** -23
    se = e.sum(axis=2, keepdims=True)
    E = (e * r + np.where(vis[None], 2.0 ** -25, 0.0)).sum(axis=2, keepdims=True)
    p = e / se
    dp = p * (r + E / (se - E) + 2.0 ** -22) + np.where(vis[None], 2.0 ** -25 / se, 0.0)
    out = np.einsum("hnt,thc->nhc", p, v)
    av = np.abs(v)
    bound = 1.25 * (np.einsum("hnt,thc->nhc", dp, av) + gamma(T + nth) * np.einsum("hnt,thc->nhc", p, av) + (T + nth) * 2.0 ** -150)
    top = p.argmax(axis=2)                                                   # [H][N]
    vtop = np.stack([v[top[h], h] for h in range(H)])                        # [H][N][dh]
    ptop = np.take_along_axis(p, top[..., None], axis=2)                     # [H][N][1]
    drop = np.abs(ptop * (vtop - out.transpose(1, 0, 2))).transpose(1, 0, 2)
    return out.reshape(N, d), bound.reshape(N, d), drop.reshape(N, d)
