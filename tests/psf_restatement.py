"""Blur with an arbitrary 2-D point-spread function for the tests: `PsfBlur` carries a PSF in the oracle's GaussianDeblurring (`.kernel`, `.filter`)
and drives the oracle's solver restatements and the *_restatement.py modules like zero_blur_restatement.ZeroBlur does; plus fp64 direct sums of
both operator kinds for any (H, W), the bound of an fp32 multiply-add chain on them, and the seeded asymmetric kernels the tests use.

  mode "fft" (PF_DEG_PSF_BLUR):        H = circular convolution  y[i] = sum_j k[j] x[i - (j - r)],  H_adj = circular correlation  (the reference's FFT pair)
  any other (PF_DEG_PSF_BLUR_ZERO):    H = F.conv2d(padding='same'), the zero-boundary correlation; H_adj = the zero-boundary convolution, its true
                                       adjoint (the reference's spatial H_adj is the correlation again, which is not the adjoint of an asymmetric kernel)
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import pnpflow_oracle as O


class PsfBlur(O.GaussianDeblurring):
    def __init__(self, kernel, mode="fft", num_channels=3, dim_image=128):
        k = torch.as_tensor(np.asarray(kernel, dtype=np.float32))
        K = k.shape[0]
        assert k.ndim == 2 and k.shape[1] == K and K % 2 == 1
        self.sigma, self.kernel_size, self.mode = None, K, mode
        self.kernel = k.view(1, 1, K, K)
        if K <= dim_image:
            f = torch.zeros((1, num_channels, dim_image, dim_image))
            f[..., :K, :K] = k
            s = -(K - 1) // 2
            self.filter = torch.roll(f, shifts=(s, s), dims=(2, 3))      # degradations.py:62-68

    def _conv(self, x, k):
        return F.conv2d(x, k.to(x.dtype).repeat(x.shape[1], 1, 1, 1), stride=1, padding="same", groups=x.shape[1])

    def H(self, x):
        return super().H(x) if self.mode == "fft" else self._conv(x, self.kernel)

    def H_adj(self, x):
        return super().H_adj(x) if self.mode == "fft" else self._conv(x, torch.flip(self.kernel, dims=(2, 3)))


def apply64(x, k, zero, adjoint=False, absolute=False):
    """fp64 direct sum of one operator application on x [..., H, W]: kind 7 (zero False) H = convolution, H_adj = correlation; kind 8 (zero True) the
    other way round.  absolute: sum |k| |x| instead, the scale of the rounding-error bound.  Zero taps are skipped (they add exactly 0)."""
    x = np.asarray(x, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    if absolute:
        x, k = np.abs(x), np.abs(k)
    K = k.shape[0]
    r = K // 2
    conv = (not zero) != bool(adjoint)
    g = k[::-1, ::-1] if conv else k                 # both directions as the correlation out[i] = sum_t g[t] in[i - r + t]
    Hh, Ww = x.shape[-2:]
    pad = [(0, 0)] * (x.ndim - 2) + [(r, r), (r, r)]
    xp = np.pad(x, pad, mode="constant") if zero else np.pad(x, pad, mode="wrap")
    out = np.zeros_like(x)
    for a, b in zip(*np.nonzero(g)):
        out += g[a, b] * xp[..., a:a + Hh, b:b + Ww]
    return out


def chain_bound(x, k, zero, adjoint=False):
    """Forward error bound of the kernel's fp32 fmaf chain, derived: the nnz non-zero taps are nnz roundings, the zero taps add exactly nothing, the
    inputs and taps are exact fp32; (nnz + 2) 2^-24 S with S = max over outputs of sum |g| |x| covers the chain (gamma_nnz) and the comparison's own
    rounding of the fp64 reference to the fp32 grid."""
    nnz = int(np.count_nonzero(k))
    return (nnz + 2) * 2.0 ** -24 * float(apply64(x, k, zero, adjoint, absolute=True).max())


def grad_step32(x, y, coef, hx, hadj_of, laplace=False):
    """The engine's gradient step composed in numpy fp32 from its own operator outputs: hx = H(x) as the engine returned it, hadj_of(r) = the engine's
    H_adj of the fp32 residual r -> (residual, z)"""
    r = hx.astype(np.float32) - y.astype(np.float32)
    if laplace:
        r = np.where(r > 0, np.float32(1), np.float32(-1)).astype(np.float32)
    v = hadj_of(r).astype(np.float32)
    z = x.astype(np.float32) - coef.astype(np.float32).reshape(-1, 1, 1, 1) * v
    return r, v, z.astype(np.float32)


def psf_kernel(K, seed=0):
    """Seeded, non-negative, asymmetric, sum 1.  K < 63: uniform draws plus one dominant off-centre tap.  K = 63: sparse, about 40 non-zero taps with
    the four corners among them."""
    g = np.random.Generator(np.random.Philox(key=[9100 + seed, K]))
    if K == 1:
        return np.ones((1, 1), dtype=np.float32)
    if K == 63:
        k = np.zeros((K, K))
        idx = g.choice(K * K, size=36, replace=False)
        k.reshape(-1)[idx] = g.uniform(0.2, 1.0, size=36)
        k[0, 0], k[0, -1], k[-1, 0], k[-1, -1] = 0.9, 0.5, 0.7, 0.3
    else:
        k = g.uniform(0.0, 1.0, size=(K, K))
        k[K // 2 - 1, min(K - 1, K // 2 + 1)] += 0.25 * K * K      # off the centre on both axes
    k = (k / k.sum()).astype(np.float32)
    assert not np.array_equal(k, k[::-1, ::-1])
    return k


def unit_tap(K, ty, tx):
    k = np.zeros((K, K), dtype=np.float32)
    k[ty, tx] = 1.0
    return k


def shift_exact(x, dy, dx, zero):
    """x moved by (dy, dx): out[i, j] = x[i - dy, j - dx], wrapped (np.roll) or zero-filled"""
    if not zero:
        return np.roll(x, (dy, dx), axis=(-2, -1))
    out = np.zeros_like(x)
    Hh, Ww = x.shape[-2:]
    ys, yd = (slice(0, Hh - dy), slice(dy, Hh)) if dy >= 0 else (slice(-dy, Hh), slice(0, Hh + dy))
    xs, xd = (slice(0, Ww - dx), slice(dx, Ww)) if dx >= 0 else (slice(-dx, Ww), slice(0, Ww + dx))
    out[..., yd, xd] = x[..., ys, xs]
    return out


def power_spectrum64(k, Hh, Ww):
    """|fft2(filter)|^2 in fp64, the filter being k zero-padded to (Hh, Ww) and rolled so that tap (K/2, K/2) sits at (0, 0)"""
    K = k.shape[0]
    f = np.zeros((Hh, Ww))
    f[:K, :K] = np.asarray(k, dtype=np.float64)
    f = np.roll(f, (-(K // 2), -(K // 2)), axis=(0, 1))
    return np.abs(np.fft.fft2(f)) ** 2


def ot_ode_vec64(k, x, vt, y, omt, rt2, sigma2):
    """fp64: vec = H_adj(ifft2(fft2(y - H(x + (1-t) v)) / (rt2 |fft2 filter|^2 + sigma2))) for the circular kind (ot_ode.py:108-118, 130)"""
    x, vt, y = (np.asarray(a, dtype=np.float64) for a in (x, vt, y))
    o = np.asarray(omt, dtype=np.float64).reshape(-1, 1, 1, 1)
    r2 = np.asarray(rt2, dtype=np.float64).reshape(-1, 1, 1, 1)
    d = y - apply64(x + o * vt, k, zero=False)
    P = power_spectrum64(k, *x.shape[-2:])
    sol = np.real(np.fft.ifft2(np.fft.fft2(d) / (r2 * P + float(sigma2))))
    return apply64(sol, k, zero=False, adjoint=True)
