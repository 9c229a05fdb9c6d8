"""Superresolution through a blur kernel, y = (k (*) x) decimated by sf (PF_DEG_PSF_SR = 9; PF_DEG_SR_FILTERED = 5 with separable taps), restated in
numpy fp64 for the tests: direct sums of H and H_adj for any (H, W, sf), the bound of an fp32 multiply-add chain on them, the aliased spectrum, the
closed-form OT-ODE vector and the exact prox.

    H x [i, j]     = sum_t k[t] x[(i sf - (t - r)) mod N]            (the circular convolution of PF_DEG_PSF_BLUR, sampled at multiples of sf; r = K // 2)
    H_adj y [m, n] = sum_t k[t] z[(m + (t - r)) mod N],  z = zero-fill(y)      (only the taps with m + t - r = 0 mod sf meet a sample)
    H H_adj        = ifft2_l( fft2_l(.) lam ),  lam[u, v] = 1/sf^2 sum_{a, b < sf} |fft2 filter|^2 [u + a Hl, v + b Wl]        (circulant on the low grid)
    prox(z)        = argmin_x alpha/2 |H x - y|^2 + 1/2 |x - z|^2 = r - alpha H_adj( ifft2_l( fft2_l(H r) / (alpha lam + 1) ) ),  r = z + alpha H_adj(y)

For an even tap count (the bicubic filter of kind 5, 4 sf taps) r = K // 2 is the tap the engine puts at offset 0 (pnpflow_hip.h), and the reference's
roll by -(K - 1) // 2 puts there too."""
import numpy as np

import psf_restatement as P


def _taps2d(k):
    k = np.asarray(k, dtype=np.float64)
    return np.outer(k, k) if k.ndim == 1 else k


def blur64(x, k, adjoint=False, absolute=False):
    """the circular blur with tap (K // 2, K // 2) at offset 0, any K (even included): convolution, or correlation when adjoint"""
    x = np.asarray(x, dtype=np.float64)
    k = _taps2d(k)
    if absolute:
        x, k = np.abs(x), np.abs(k)
    r = k.shape[0] // 2
    out = np.zeros_like(x)
    for a, b in zip(*np.nonzero(k)):
        s = (a - r, b - r) if not adjoint else (r - a, r - b)      # out[i] = x[i - (a - r)]  /  x[i + (a - r)]
        out += k[a, b] * np.roll(x, s, axis=(-2, -1))
    return out


def zero_fill(y, sf):
    y = np.asarray(y)
    z = np.zeros(y.shape[:-2] + (y.shape[-2] * sf, y.shape[-1] * sf), dtype=y.dtype)
    z[..., ::sf, ::sf] = y
    return z


def H64(x, k, sf, absolute=False):
    return blur64(x, k, False, absolute)[..., ::sf, ::sf]


def Hadj64(y, k, sf, absolute=False):
    return blur64(zero_fill(np.asarray(y, dtype=np.float64), sf), k, True, absolute)


def phase_counts(k, sf):
    """non-zero taps an H_adj output of phase (m mod sf, n mod sf) sums: those with (m + a - r) = 0 and (n + b - r) = 0 mod sf -> [sf, sf]"""
    k = _taps2d(k)
    r = k.shape[0] // 2
    out = np.zeros((sf, sf), dtype=np.int64)
    for a, b in zip(*np.nonzero(k)):
        out[(r - a) % sf, (r - b) % sf] += 1
    return out


def chain_bound(a, k, sf, adjoint=False):
    """(nnz + 2) 2^-24 max sum |g| |x| (psf_restatement.chain_bound) with nnz the taps actually summed: all non-zero taps for H, the largest phase's
    count for H_adj"""
    k2 = _taps2d(k)
    nnz = int(phase_counts(k2, sf).max()) if adjoint else int(np.count_nonzero(k2))
    S = float((Hadj64(a, k2, sf, absolute=True) if adjoint else H64(a, k2, sf, absolute=True)).max())
    return (nnz + 2) * 2.0 ** -24 * S


def power_spectrum64(k, Hh, Ww):
    k = _taps2d(k)
    K = k.shape[0]
    f = np.zeros((Hh, Ww))
    f[:K, :K] = k
    f = np.roll(f, (-(K // 2), -(K // 2)), axis=(0, 1))
    return np.abs(np.fft.fft2(f)) ** 2


def aliased_spectrum64(k, Hh, Ww, sf):
    """lam[Hl, Wl]: the eigenvalues of H H_adj"""
    Pw = power_spectrum64(k, Hh, Ww)
    Hl, Wl = Hh // sf, Ww // sf
    return Pw.reshape(sf, Hl, sf, Wl).sum(axis=(0, 2)) / sf ** 2


def ot_ode_vec64(k, sf, x, vt, y, omt, rt2, sigma2):
    """vec = H_adj( ifft2_l( fft2_l(y - H(x + (1-t) v)) / (rt2 lam + sigma2) ) )"""
    x, vt, y = (np.asarray(a, dtype=np.float64) for a in (x, vt, y))
    o = np.asarray(omt, dtype=np.float64).reshape(-1, 1, 1, 1)
    r2 = np.asarray(rt2, dtype=np.float64).reshape(-1, 1, 1, 1)
    d = y - H64(x + o * vt, k, sf)
    lam = aliased_spectrum64(k, x.shape[-2], x.shape[-1], sf)
    sol = np.real(np.fft.ifft2(np.fft.fft2(d) / (r2 * lam + float(sigma2))))
    return Hadj64(sol, k, sf)


def prox64(k, sf, z, y, alpha):
    z, y = np.asarray(z, dtype=np.float64), np.asarray(y, dtype=np.float64)
    r = z + alpha * Hadj64(y, k, sf)
    lam = aliased_spectrum64(k, z.shape[-2], z.shape[-1], sf)
    sol = np.real(np.fft.ifft2(np.fft.fft2(H64(r, k, sf)) / (alpha * lam + 1.0)))
    return r - alpha * Hadj64(sol, k, sf)


def strided_shift(x, dy, dx, sf):
    """H of a unit tap at offset (dy, dx) from the centre: x[i sf - dy, j sf - dx], wrapped"""
    return np.roll(x, (dy, dx), axis=(-2, -1))[..., ::sf, ::sf]


psf_kernel, unit_tap, grad_step32 = P.psf_kernel, P.unit_tap, P.grad_step32


# ---- torch: the operator object and the hqs iteration the solver restatements drive ---------------------------------------------------------------
import torch  # noqa: E402

from oracle import pnpflow_oracle as O  # noqa: E402


class SrBlur(O.Superresolution):
    """The oracle's Superresolution(mode="bicubic") with `.filter` replaced by the rolled, zero-padded PSF (what the fixtures of
    tools/make_golden_sr_blur.py do to the reference's object); kernel=None keeps the bicubic filter.  H / H_adj work in the dtype of their argument."""
    def __init__(self, kernel, sf, num_channels=3, dim_image=64):
        super().__init__(sf, dim_image, mode="bicubic")
        if kernel is not None:
            k = torch.as_tensor(np.asarray(kernel, dtype=np.float32))
            K = k.shape[0]
            f = torch.zeros((1, num_channels, dim_image, dim_image))
            f[..., :K, :K] = k
            s = -(K - 1) // 2
            self.filter = torch.roll(f, shifts=(s, s), dims=(2, 3))
        else:
            self.filter = self.filter[:, :1].repeat(1, num_channels, 1, 1)

    def _fk(self, x):
        return torch.fft.fft2(self.filter.to(x.dtype))

    def H(self, x):
        return self._down(torch.real(torch.fft.ifft2(torch.fft.fft2(x) * self._fk(x))))

    def H_adj(self, x):
        return torch.real(torch.fft.ifft2(torch.fft.fft2(self._up(x)) * torch.conj(self._fk(x))))

    def _up(self, x):
        z = torch.zeros((x.shape[0], x.shape[1], x.shape[2] * self.sf, x.shape[3] * self.sf), dtype=x.dtype)
        z[..., ::self.sf, ::self.sf] = x
        return z

    def lam(self, dtype=torch.float64):
        k2 = torch.fft.fft2(self.filter.to(dtype)).abs() ** 2
        D, sf = k2.shape[-1], self.sf
        return k2.reshape(1, k2.shape[1], sf, D // sf, sf, D // sf).sum(dim=(2, 4)) / sf ** 2

    def prox(self, z, y, alpha):
        """the exact prox of alpha/2 |H x - y|^2 at z"""
        r = z + alpha * self.H_adj(y)
        sol = torch.real(torch.fft.ifft2(torch.fft.fft2(self.H(r)) / (alpha * self.lam(z.dtype) + 1.0)))
        return r - alpha * self.H_adj(sol)

    def ot_ode_sol(self, d, rt2, sigma2):
        """(rt2 H H^T + sigma2)^-1 d in closed form on the low-resolution grid"""
        return torch.real(torch.fft.ifft2(torch.fft.fft2(d) / (rt2.view(-1, 1, 1, 1) * self.lam(d.dtype) + sigma2)))


def hqs_iterate(net, d, x, noisy, sigma_noise, alpha):
    """One iteration of the schedule of pnp_gs.py:180-200 with the exact prox -> (x_next, J^T r for the tolerance)"""
    import pnp_gs_restatement as R
    sig = torch.ones(x.shape[0], dtype=x.dtype) * (2.0 * sigma_noise)
    Dg, _, _, JN = R.calculate_grad(net, x, sig)
    Dx = x - Dg
    z = 0.065 * alpha * Dx + alpha * (1 - alpha * 0.065) * x
    return d.prox(z, noisy, alpha), JN


def ot_ode_restore64(sd, cfg, d, noisy, sigma_noise, steps, start_time, init_noise, record=None):
    """The loop of ot_ode.py:49-52, 63-147 (gamma constant) in fp64 with the closed-form solve on the low-resolution grid where the reference's generic
    branch runs its GMRES"""
    import flow_priors_restatement as FR
    vel = FR.oracle_vel(sd, cfg, torch.float64)
    noisy, init_noise = noisy.double(), init_noise.double()
    x = start_time * d.H_adj(noisy) + (1 - start_time) * init_noise
    delta = 1 / steps
    for it in range(int(steps * start_time), int(steps)):
        t1 = torch.ones(len(x), dtype=torch.float64) * delta * it
        vt = vel(x, t1)
        omt = (1 - t1).view(-1, 1, 1, 1)
        rt2 = (1 - t1) ** 2 / ((1 - t1) ** 2 + t1 ** 2)
        vec = d.H_adj(d.ot_ode_sol(noisy - d.H(x + omt * vt), rt2, sigma_noise ** 2))
        g = vec + omt * vel.vjp(x, t1, vec)
        x = x + delta * (vt + omt / t1.view(-1, 1, 1, 1) * g)
        if record is not None:
            record(it, x)
    return x
