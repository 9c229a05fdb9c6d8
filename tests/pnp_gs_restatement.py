"""CPU restatement of Prox-PnP with the gradient-step denoiser (pnpflow/methods/pnp_gs.py, pnpflow/train_denoiser.py:39-57) that the
pnp_gs tests lean on: calculate_grad by autograd, the initialisations, the denoiser-level schedule and the three iteration forms.

`net(x, sigma)` is the denoiser U-Net: the oracle `lambda x, s: O.unet_forward(sd, cfg, x, s)`.  `d` is an oracle degradation.
tests/test_pnp_gs_host.py pins this file to goldens of the real reference (tools/make_golden_pnp_gs.py).
"""
import numpy as np
import torch

from oracle import pnpflow_oracle as O


def det_laplace(shape, seed, idx=0):
    """Deterministic unit-scale Laplace sample (inverse CDF of a numpy Philox uniform): the draw tools/make_golden_pnp_gs.py puts in
    place of torch.distributions.laplace.Laplace(...).sample()."""
    g = np.random.Generator(np.random.Philox(key=[seed, idx]))
    u = g.random(size=shape, dtype=np.float32) - np.float32(0.5)
    return torch.from_numpy((-np.sign(u) * np.log1p(-2 * np.abs(u))).astype(np.float32))


def calculate_grad(net, x, sigma):
    """(Dg, N, g, J^T (x - N)):  N = net(x, sigma),  Dg = (x - N) - J_N(x)^T (x - N),  g = 0.5 sum (x - N)^2 over the batch."""
    x = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        N = net(x, sigma)
        (JN,) = torch.autograd.grad(N, x, grad_outputs=(x - N).detach())
    x, N = x.detach(), N.detach()
    r = x - N
    return r - JN, N, 0.5 * torch.sum(r.reshape(x.shape[0], -1) ** 2), JN


def algo_code(algo, problem):
    if algo == "pgd":
        return 0
    return {"random_inpainting": 1, "gaussian_deblurring_FFT": 2}[problem]


def level(code, it, sigma_noise, sigma_factor=1.0):
    """Denoiser level of iteration `it`: hqs random inpainting 0.2 for it < 20 then sigma_noise, hqs deblurring 1.8 sigma_noise, pgd
    sigma_factor sigma_noise."""
    if code == 1:
        return 0.2 if it < 20 else sigma_noise
    if code == 2:
        return 1.8 * sigma_noise
    return sigma_factor * sigma_noise


def initialise(problem, noisy, d):
    if problem == "random_inpainting":
        return 1.5 * noisy.clone() - d.H(noisy)
    if problem == "superresolution":
        S = noisy.shape[-1] * d.sf
        return O.Superresolution(2 if S == 128 else 4, S, mode="bicubic").H_adj(noisy.clone())
    return d.H_adj(noisy.clone())


def grad_datafit(x, y, d, sigma_noise, noise_type):
    if noise_type == "gaussian":
        return d.H_adj(d.H(x) - y) / (sigma_noise ** 2)
    r = d.H(x) - y
    return d.H_adj(2 * torch.heaviside(r, torch.zeros_like(r)) - 1) / sigma_noise


def prox_blur(v, y, d, alpha):
    """argmin_x alpha/2 |H x - y|^2 + 1/2 |x - v|^2 for the circular blur, in the Fourier domain."""
    fk = torch.fft.fft2(d.filter.to(v.dtype))
    return torch.real(torch.fft.ifft2(torch.fft.fft2(alpha * d.H_adj(y) + v) / (alpha * torch.conj(fk) * fk + 1.)))


def iterate(net, d, x, noisy, it, *, algo, problem, max_iter, sigma_noise, alpha, lr=None, sigma_factor=1.0, noise_type="gaussian"):
    """One iteration on the entering iterate x -> (x_next, alpha_next, info).  info: 'JN' (for tolerances), 'gap', 'thr' (hqs deblurring)."""
    code = algo_code(algo, problem)
    B = x.shape[0]
    sig = torch.ones(B, dtype=x.dtype) * level(code, it, sigma_noise, sigma_factor)
    info = {}
    if code == 0:
        lr = sigma_noise ** 2 if lr is None else lr
        z = x - lr * grad_datafit(x, noisy, d, sigma_noise, noise_type) if (problem != "denoising" or noise_type == "laplace") else x
        Dg, _, _, info["JN"] = calculate_grad(net, z, sig)
        return (1 - alpha) * z + alpha * (z - Dg), alpha, info
    Dg, _, g, info["JN"] = calculate_grad(net, x, sig)
    Dx = x - Dg
    if code == 1:
        if it < max_iter - 1:
            return d.H(noisy) - d.H(Dx) + Dx, alpha, info
        return x, alpha, info
    v = 0.1 * alpha * Dx + alpha * (1 - alpha * 0.1) * x
    xn = prox_blur(v, noisy, d, alpha)
    obj = lambda a: 0.5 * torch.linalg.norm(d.H(a) - noisy) ** 2 + 0.1 * g
    info["gap"] = float(obj(xn) - obj(x))
    info["thr"] = float(0.1 / alpha * torch.linalg.norm(xn - x) ** 2)
    return xn, (0.9 * alpha if info["gap"] < info["thr"] else alpha), info


def solve(net, d, noisy, *, x0=None, alpha, first=0, stop=None, **kw):
    """Free-running iterations [first, stop): ([x entering first, ..., x after stop - 1], [alpha entering first, ..., alpha after], infos)."""
    x = initialise(kw["problem"], noisy, d) if x0 is None else x0
    stop = kw["max_iter"] if stop is None else stop
    xs, alphas, infos = [x], [alpha], []
    for it in range(first, stop):
        x, alpha, info = iterate(net, d, x, noisy, it, alpha=alpha, **kw)
        xs.append(x); alphas.append(alpha); infos.append(info)
    return xs, alphas, infos
