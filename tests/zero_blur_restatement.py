"""The zero-boundary Gaussian blur (GaussianDeblurring with any mode but "fft", pnpflow/degradations.py:72-76, 82-86) for the tests: the
oracle's class asserts mode == "fft", so this subclass supplies H = H_adj = F.conv2d(padding='same') and drives the oracle's solver
restatements (O.pnp_flow_restore, O.ot_ode_restore with its generic GMRES branch, O.gmres) and the *_restatement.py modules; plus fp64
forms of the operator (any taps: H is the correlation, H_adj the convolution) and of the reference's GMRES, which the GPU tests and
tools/make_golden_spatial.py measure fp32 results against."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import pnpflow_oracle as O


class ZeroBlur(O.GaussianDeblurring):
    def __init__(self, sigma_blur, kernel_size, num_channels=3, dim_image=128):
        super().__init__(sigma_blur, kernel_size, "fft", num_channels, dim_image)
        self.mode = "spatial"

    def H(self, x):
        k = self.kernel.to(x.dtype).repeat(x.shape[1], 1, 1, 1)
        return F.conv2d(x, k, stride=1, padding="same", groups=x.shape[1])

    H_adj = H


def corr_matrix(taps, n):
    """(n, n) fp64 matrix of the 1-D zero-boundary correlation out[i] = sum_k taps[k] in[i + k - r], r = len(taps) // 2"""
    g = np.asarray(taps, dtype=np.float64)
    r = len(g) // 2
    T = np.zeros((n, n))
    for k, gk in enumerate(g):
        i = np.arange(max(0, r - k), min(n, n + r - k))
        T[i, i + k - r] = gk
    return T


def blur64(x, taps, adjoint=False):
    """fp64 zero-boundary separable blur of x [..., H, W] with outer(taps, taps): correlation (H), or its transpose (H_adj)"""
    x = np.asarray(x, dtype=np.float64)
    Th, Tw = corr_matrix(taps, x.shape[-2]), corr_matrix(taps, x.shape[-1])
    if adjoint:
        Th, Tw = Th.T, Tw.T
    return Th @ x @ Tw.T


def grad_step64(x, y, coef, taps, laplace=False):
    """z = x - coef[b] H_adj(H x - y)  (or of sgn(H x - y) in {-1, +1}: 2 heaviside(., 0) - 1)"""
    r = blur64(x, taps) - np.asarray(y, dtype=np.float64)
    if laplace:
        r = np.where(r > 0, 1.0, -1.0)
    return np.asarray(x, dtype=np.float64) - np.asarray(coef, dtype=np.float64).reshape(-1, 1, 1, 1) * blur64(r, taps, adjoint=True)


def gmres64(avp, b, max_iter, tol=1e-6, atol=1e-6):
    """pnpflow/utils.py:972-1109 with x0 = 0 in fp64 -> (solution, Krylov vectors used; 0 for the |b| < 1e-8 return of b itself)"""
    b = np.asarray(b, dtype=np.float64)
    bnorm = np.linalg.norm(b)
    if max_iter == 0 or bnorm < 1e-8:
        return b.copy(), 0
    eps = float(np.finfo(np.float64).eps)
    V = [b / bnorm if bnorm > eps else np.zeros_like(b)]
    Hm = np.zeros((max_iter + 1, max_iter + 1)); cs = np.zeros(max_iter); ss = np.zeros(max_iter)
    beta = np.zeros(max_iter + 1); beta[0] = bnorm
    j = 0
    for j in range(max_iter):
        w = avp(V[j])
        for i in range(j + 1):
            Hm[i, j] = w @ V[i]; w = w - Hm[i, j] * V[i]
        wn = np.linalg.norm(w); Hm[j + 1, j] = wn
        V.append(w / wn if wn > eps else np.zeros_like(w))
        for i in range(j):
            tmp = cs[i] * Hm[i, j] - ss[i] * Hm[i + 1, j]
            Hm[i + 1, j] = cs[i] * Hm[i + 1, j] + ss[i] * Hm[i, j]
            Hm[i, j] = tmp
        r = np.hypot(Hm[j, j], Hm[j + 1, j])
        cs[j], ss[j] = Hm[j, j] / r, -Hm[j + 1, j] / r
        Hm[j, j] = cs[j] * Hm[j, j] - ss[j] * Hm[j + 1, j]; Hm[j + 1, j] = 0
        beta[j + 1] = ss[j] * beta[j]; beta[j] = cs[j] * beta[j]
        if abs(beta[j + 1]) < tol * bnorm or abs(beta[j + 1]) < atol:
            break
    y = np.linalg.solve(np.triu(Hm[:j + 1, :j + 1]), beta[:j + 1])
    return np.stack(V[:j + 1], axis=1) @ y, j + 1


# ---- the Krylov cases of tests/golden/zero_blur_gmres.npz (tools/make_golden_spatial.py) -------------------------------------------
KRYLOV_SHAPE = (3, 3, 20, 24)           # B, C, H, W
KRYLOV_RT2 = (0.9, 0.15, 0.5)           # per image: different conditioning, different iteration counts
KRYLOV_SIGMA2 = 0.04                    # 0.2 ** 2
KRYLOV_BLUR = (1.0, 61)                 # blur sigma, K


def krylov_rhs():
    """det_normal right-hand sides; image 2 is zero (the |rhs| < 1e-8 return)"""
    g = np.random.Generator(np.random.Philox(key=[7300, 0]))
    rhs = g.standard_normal(size=KRYLOV_SHAPE, dtype=np.float32)
    rhs[2] = 0.0
    return rhs


def krylov_solve64(rhs, taps, max_iter):
    """fp64 restatement of the batched solve -> (sol [B, C, H, W], Krylov vectors per image)"""
    sols, its = [], []
    for b in range(rhs.shape[0]):
        shp = rhs.shape[1:]
        avp = lambda z, b=b: (KRYLOV_RT2[b] * blur64(blur64(z.reshape(shp), taps, adjoint=True), taps) + KRYLOV_SIGMA2 * z.reshape(shp)).reshape(-1)
        s, k = gmres64(avp, rhs[b].reshape(-1), max_iter)
        sols.append(s.reshape(shp)); its.append(k)
    return np.stack(sols), np.array(its)
