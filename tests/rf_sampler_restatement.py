"""CPU restatement, line by line, of the reference's rectified-flow samplers - pnpflow/image_generation/sampling.py:69-153 (euler_sampler,
rk45_sampler) and sde_lib.py:37-94 (RectifiedFlow.ode, euler_ode) - over any `model_fn(x, label) -> velocity` (the oracles' forwards).
Torch on the CPU and SciPy's own solve_ivp; no reference import, no engine.  tools/make_golden_rf_sampler.py runs the REAL samplers on the
REAL NCSN++ module and stores their outputs; tests/test_rf_sampler_host.py holds this file to them.

The label a sampler feeds the net is t * label_scale: 999 in the reference (the NCSN++ net), 1 for a U-Net that takes t as it is.
"""
import numpy as np
import torch

EPS = 1e-3


def sigma_t(t, sigma_var):
    return (1. - t) * sigma_var


def euler_sampler(model_fn, z, sample_N, sigma_var=0.0, noise_scale=1.0, noise=None, T=1., label_scale=999, eps=EPS):
    """sampling.py:69-109 from the latent z -> (x, nfe).  noise[i]: the draw torch.randn_like makes in step i (needed when sigma_var > 0)."""
    if noise is None and sigma_var != 0.0:
        raise ValueError("sigma_var > 0 needs the steps' normal draws")
    x = z
    dt = 1. / sample_N
    for i in range(sample_N):
        num_t = i / sample_N * (T - eps) + eps
        t = torch.ones(z.shape[0], dtype=z.dtype) * num_t
        pred = model_fn(x, t * label_scale)
        s_t = sigma_t(num_t, sigma_var)
        pred_sigma = pred + (s_t ** 2) / (2 * (noise_scale ** 2) * ((1. - num_t) ** 2)) * (0.5 * num_t * (1. - num_t) * pred - 0.5 * (2. - num_t) * x.detach().clone())
        n_i = noise[i] if noise is not None else torch.zeros_like(pred_sigma)
        x = x.detach().clone() + pred_sigma * dt + s_t * np.sqrt(dt) * n_i
    return x, sample_N


def solve(model_fn, x, t_span, rtol, atol, label_scale=999, dtype=torch.float32):
    """The solve_ivp call of sampling.py:135-149 and sde_lib.py:54-69: the state flattened to ONE fp64 vector (the whole batch), the net
    evaluated in `dtype` (the reference: fp32) -> (the state at the end, fp64 numpy of x's shape; SciPy's OdeResult)."""
    from scipy import integrate
    shape = tuple(x.shape)

    def ode_func(t, y):
        xx = torch.from_numpy(y.reshape(shape)).type(dtype)
        vec_t = torch.ones(shape[0], dtype=dtype) * t
        drift = model_fn(xx, vec_t * label_scale)
        return drift.detach().cpu().numpy().reshape((-1,))

    sol = integrate.solve_ivp(ode_func, t_span, x.detach().cpu().numpy().reshape((-1,)), rtol=rtol, atol=atol, method='RK45')
    assert sol.success, sol.message
    return sol.y[:, -1].reshape(shape), sol


def rk45_sampler(model_fn, z, ode_tol=1e-5, T=1., label_scale=999, dtype=torch.float32, eps=EPS):
    """sampling.py:111-153 -> (x fp64 numpy, nfev, accepted steps)."""
    y, sol = solve(model_fn, z, (eps, T), ode_tol, ode_tol, label_scale, dtype)
    return y, sol.nfev, sol.t.size - 1


def ode(model_fn, init_input, reverse=False, T=1., label_scale=999, dtype=torch.float32, rtol=1e-5, atol=1e-5, eps=EPS):
    """sde_lib.py:37-72 -> (x fp64 numpy, nfev, accepted steps)."""
    y, sol = solve(model_fn, init_input, (T, eps) if reverse else (eps, T), rtol, atol, label_scale, dtype)
    return y, sol.nfev, sol.t.size - 1


def euler_ode(model_fn, init_input, reverse=False, N=100, T=1., label_scale=999, eps=EPS):
    """sde_lib.py:74-94; `reverse` is ignored there, and here."""
    x = init_input.detach().clone()
    dt = 1. / N
    for i in range(N):
        num_t = i / N * (T - eps) + eps
        t = torch.ones(x.shape[0], dtype=x.dtype) * num_t
        pred = model_fn(x, t * label_scale)
        x = x.detach().clone() + pred * dt
    return x
