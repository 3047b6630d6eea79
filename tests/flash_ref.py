"""The float64 statement of causal soft_max attention on the UN-ROUNDED fp32 rotated q, K and V, and the derived error bound of the opt-in
fused kernel k_flash_attn (csrc/flash_attn.hip states the arithmetic), shared by tests/test_gpu_flash_attn_op.py.

The bound, per output o[n][c] of one head.  u = 2^-11 (fp16), U = 2^-24 and gamma(k) = k U / (1 - k U) (fp32, tests/gemm_ref.py),
eta = 2^-25 (half the spacing of the fp16 subnormals), T keys in all, nt = ceil(T / 64) key tiles, a_t = kq (q . k_t) the exact score,
A_t = sum_i |q_i k_ti|.
  scores   q and k are narrowed once: |q^ - q| <= dq = u |q| + eta, the same for k, so the 128 exact products move by
           E_t = sum_i dq_i (|k_ti| + dk_ti) + |q_i| dk_ti    [= (2 u + u^2) A_t when nothing is subnormal];
           the matrix core sums them once in fp32 (gamma(129)), c = fl(kq * fl(log2 e)) and the multiplication by it round three times
           (gamma(3)), and s - m, m_old - m_new round once each with |s - m| <= 2 max |s| (4 U kq max A in all, in natural-log units):
               Delta = max_t kq (E_t + gamma(132) (A_t + E_t)) + 4 U kq max_t (A_t + E_t)       over the keys t the row sees.
  weights  the kernel's un-normalised weight is C w_t e^(d_t) with |d_t| <= Delta and one C per row (the running maximum and the rescales
           multiply numerator and denominator by the SAME fp32 numbers), times (1 + eps_exp) per exp2 it went through -- its own and at most
           nt rescales; eps_exp = 2^-22 is the stated accuracy taken for v_exp_f32 (1 ulp, doubled) -- times (1 + u) for its narrowing to
           fp16, or +- eta absolutely where it falls into the fp16 subnormals.
  sums     numerator and denominator are each one fp32 sum of T terms taken by the matrix core / the lanes, rescaled at most nt times, merged
           over at most 8 key splits (2 roundings per split) and divided once: g = gamma(T + nt + 20).  v moves by (1 + u) (+ eta).
  So numerator / C = sum w v (1 + theta), |1 + theta| <= R_N = e^Delta (1 + eps_exp)^(nt + 1) (1 + u)^2 (1 + g), denominator / C = W (1 + e_D)
  with |e_D| <= R_D - 1, R_D = R_N / (1 + u), and for o64 = sum p_t v_tc, B = sum p_t |v_tc|:
      |o - o64| <= B ((R_N - 1) + (R_D - 1)) / (2 - R_D) + (T 2^-24 max |v| + 2^-24) / (2 - R_D) + one fp32 ulp of o64.
  The absolute term: T subnormal weights, eta each, against |v^| in the numerator and against |o64| <= max |v| in the denominator (W >= 1).
Derived, not fitted: if the measured error exceeds it, the kernel or this derivation is wrong."""
import numpy as np

from gemm_ref import U, gamma

u = 2.0 ** -11
ETA = 2.0 ** -25
EPS_EXP = 2.0 ** -22


def flash_reference(qr, K, V, H, n_past):
    """qr f32 [N][d] rotated queries, K / V f32 caches whose rows 0 .. n_past + N - 1 are the eval's keys.  Returns (o64 [N][d], bound [N][d])."""
    N, d = qr.shape
    dh, T = d // H, n_past + N
    nt = (T + 63) // 64
    kq = np.float64(np.float32(1.0) / np.sqrt(np.float32(d / H)))
    q = qr.astype(np.float64).reshape(N, H, dh)
    k = K[:T].astype(np.float64).reshape(T, H, dh)
    v = V[:T].astype(np.float64).reshape(T, H, dh)
    vis = (np.arange(T)[None, :] <= (n_past + np.arange(N))[:, None])[None]            # [1][N][T]
    a = np.where(vis, kq * np.einsum("nhi,thi->hnt", q, k), -np.inf)
    w = np.exp(a - a.max(axis=2, keepdims=True))
    p = w / w.sum(axis=2, keepdims=True)
    out = np.einsum("hnt,thc->nhc", p, v)
    B = np.einsum("hnt,thc->nhc", p, np.abs(v))
    aq, ak = np.abs(q), np.abs(k)
    dq, dk = u * aq + ETA, u * ak + ETA
    A = np.einsum("nhi,thi->hnt", aq, ak)
    E = np.einsum("nhi,thi->hnt", dq, ak + dk) + np.einsum("nhi,thi->hnt", aq, dk)
    AE = np.where(vis, A + E, 0.0)
    delta = (kq * np.where(vis, E + gamma(132) * (A + E), 0.0)).max(axis=2) + 4 * U * kq * AE.max(axis=2)      # [H][N]
    g = gamma(T + nt + 20)
    R_N = np.exp(delta) * (1 + EPS_EXP) ** (nt + 1) * (1 + u) ** 2 * (1 + g)
    R_D = R_N / (1 + u)
    if (R_D >= 2).any():
        raise ValueError("the score perturbation is too large for the bound to say anything: scale the operands down")
    rel = (((R_N - 1) + (R_D - 1)) / (2 - R_D)).T[:, :, None]                                                   # [N][H][1]
    absolute = ((T * 2.0 ** -24 * np.abs(v).max() + 2.0 ** -24) / (2 - R_D)).T[:, :, None]
    bound = rel * B + absolute + np.spacing(np.abs(out).astype(np.float32)).astype(np.float64)
    return out.reshape(N, d), bound.reshape(N, d)
