"""The float64 yardstick of a Q4_0 x Q4_0 product, shared by the per-op mat-mul tests (test_gpu_prompt_gemm.py, test_gpu_gemv_set_op.py):
y* = sum_b t_b in float64 (t_b = d_w,b * d_a,b * s_b, s_b the exact integer dot product of block b) and the proven bounds on a kernel's
distance from it -- gamma_k = k u / (1 - k u), u = 2^-24; the exact kernels chain n = Kp / 32 blocks through eight chains and a depth-3
tree: |y - y*| <= gamma_{n+4} * sum |w| |x| (+ u |y* + r| and the float64 slack with a residual).  Nothing here needs a GPU."""
import numpy as np

U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


def split(blocks):
    """Q4_0 blocks [R, nb, 20] -> (scales float64 [R, nb], codes int8 [R, nb, 32])"""
    d = blocks[:, :, :4].copy().view(np.float32)[..., 0].astype(np.float64)
    qs = blocks[:, :, 4:]
    c = np.empty(qs.shape[:2] + (32,), np.int8)
    c[..., 0::2] = (qs & 0xF).astype(np.int8) - 8
    c[..., 1::2] = (qs >> 4).astype(np.int8) - 8
    return d, c


class Ref:
    """float64 reference of one product: y*, sum |t_b| (exact per block where it is cheap), sum |w| |x|, and the bounds"""

    def __init__(self, oracle, w, x, resid):
        M, nb, _ = w.shape
        N, K = x.shape
        self.n = (K + 255) // 256 * 8                                   # blocks the kernels chain, padded ones included
        self.dw, self.cw = split(w)
        self.da, self.ca = split(oracle.quantize_row(x).reshape(N, nb, 20))
        Wq = (self.dw[:, :, None] * self.cw).reshape(M, K)            # exact in float64
        Xq = (self.da[:, :, None] * self.ca).reshape(N, K)
        self.sabs_wx = np.abs(Xq) @ np.abs(Wq).T
        if N * M * nb <= 40_000_000:
            ys, st = np.zeros((N, M)), np.zeros((N, M))
            for b in range(nb):
                t = np.outer(self.da[:, b], self.dw[:, b]) * (self.ca[:, b, :].astype(np.float64) @ self.cw[:, b, :].T.astype(np.float64))
                ys += t
                st += np.abs(t)
            self.ystar, self.sabs_t, slack_n = ys, st, self.n
        else:
            self.ystar, self.sabs_t, slack_n = Xq @ Wq.T, None, K
        self.r = None if resid is None else resid.astype(np.float64)
        self.slack = slack_n * 2.0 ** -52 * self.sabs_wx

    def _with_resid(self, chain):
        if self.r is None:
            return chain + self.slack
        tot = np.abs(self.ystar + self.r)
        return chain * (1 + U) + U * tot + self.slack + 2.0 ** -52 * tot

    def bound_fast(self):
        return self._with_resid(gamma(self.n + 1) * (self.sabs_t if self.sabs_t is not None else self.sabs_wx))

    def bound_exact(self):
        return self._with_resid(gamma(self.n + 4) * self.sabs_wx)

    def err(self, y):
        want = self.ystar if self.r is None else self.ystar + self.r
        return np.abs(y.astype(np.float64) - want)

    def lost_block_margin(self, rows_w, rows_x, rng, k=64):
        """on k ordinary outputs: the exact-sum bound of the fast kernel against the output's median single-block |t_b| (a block the kernel
        lost or paired with another block's scale moves the output by about that much)"""
        nb_real = self.cw.shape[1]
        worst = 0.0
        for _ in range(k):
            n, m = int(rng.choice(rows_x)), int(rng.choice(rows_w))
            t = self.da[n] * self.dw[m] * (self.ca[n].astype(np.int64) * self.cw[m].astype(np.int64)).sum(axis=1)
            med = np.median(np.abs(t[:nb_real]))
            b = gamma(self.n + 1) * np.abs(t).sum()
            assert med > 0 and b < med / 20, f"output (n {n}, m {m}): bound {b:.3e} vs median block |t_b| {med:.3e}"
            worst = max(worst, b / med)
        return worst
