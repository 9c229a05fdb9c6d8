"""CPU restatement of Flow-Priors (pnpflow/methods/flow_priors.py) that the Flow-Priors tests and tools/make_golden_flow_priors.py lean on.

The method's loss contains the Hutchinson trace term eps . J(x) eps; its gradient with respect to x is taken here by EXACT double
autograd (torch.autograd.functional.jvp(create_graph=True), then autograd.grad - what the reference's hut_estimator + autograd.grad do),
in fp32 or fp64.  The engine instead takes the central difference of two first-order VJPs,
    grad_x (eps . J(x) eps) = d/ds [J(x + s eps)^T eps] at s = 0  ~  (J(x + h eps)^T eps - J(x - h eps)^T eps) / (2 h),
which `fd_grad_trace` restates on the oracle's first-order VJP (O.unet_vjp).

`vel(x, t)` is a velocity field of the working dtype: `oracle_vel(sd, cfg, dtype)`.  fp64 needs the state dict cast and the oracle's
sinusoidal embedding and FIR taps (which are fp32) cast to the weights' dtype; both happen in here, nothing under oracle/ is touched.
Probes are +-1 from a numpy Philox generator (`probe`).
"""
import contextlib

import numpy as np
import torch

from oracle import pnpflow_oracle as O


@contextlib.contextmanager
def _embedding_as(dtype):
    emb, fir = O.sinusoidal_embedding, O.fir_kernel_2d
    O.sinusoidal_embedding = lambda t, dim: emb(t, dim).to(dtype)
    O.fir_kernel_2d = lambda k, gain=1.0: fir(k, gain).to(dtype)          # the NCSN++ oracle's FIR taps (exact in fp32)
    try:
        yield
    finally:
        O.sinusoidal_embedding, O.fir_kernel_2d = emb, fir


def cast_state_dict(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def oracle_vel(sd, cfg, dtype=torch.float32):
    """v(x, t) of the oracle U-Net in `dtype` (sd: the fp32 synthetic state dict); .vjp(x, t, vec) = O.unet_vjp in the same dtype."""
    sdd = cast_state_dict(sd, dtype)

    def vel(x, t):
        with _embedding_as(dtype):
            return O.unet_forward(sdd, cfg, x.to(dtype), t)

    def vjp(x, t, vec):
        with _embedding_as(dtype):
            return O.unet_vjp(sdd, cfg, x, t, vec)
    vel.vjp, vel.dtype = vjp, dtype
    return vel


def ncsnpp_vel(sd, cfg, dtype=torch.float32, scale=999.0):
    """The `rectified` net: model_forward(x, t) = NCSNpp(x, t * 999) (flow_priors.py:22-25) on oracle/ncsnpp_oracle.py."""
    from oracle import ncsnpp_oracle as NO
    sdd = cast_state_dict(sd, dtype)

    def vel(x, t):
        with _embedding_as(dtype):
            return NO._forward(sdd, cfg, x.to(dtype), t * scale, None)

    def vjp(x, t, vec):
        with _embedding_as(dtype):
            return NO.ncsnpp_vjp(sdd, cfg, x, t * scale, vec)
    vel.vjp, vel.dtype = vjp, dtype
    return vel


def probe(shape, seed, idx=0, dtype=torch.float32):
    """Rademacher probe number `idx` of stream `seed`: numpy Philox, +1 where the drawn bit is set."""
    g = np.random.Generator(np.random.Philox(key=[seed, idx]))
    return torch.from_numpy(g.integers(0, 2, size=shape, dtype=np.int8).astype(np.float32) * 2 - 1).to(dtype)


def schedule(N, start_time, i):
    """(num_t, dt) of outer iteration i, the reference's Python doubles (flow_priors.py:63-69, 83)."""
    if start_time > 0.0:
        eps0 = 1 * start_time
        dt = (1 - eps0) / N
    else:
        dt = 1. / N
        eps0 = 1e-3
    return i / N * (1 - eps0) + eps0, dt


def _data_loss(vel, H, x, x_init, y, num_t, dt, lmbda, noise_type):
    t1 = torch.ones(len(x), dtype=x.dtype) * num_t
    t = t1.view(-1, 1, 1, 1)
    pred = vel(x, t1)
    x_next = x + pred * dt
    y_next = (t + dt) * y + (1 - (t + dt)) * H(x_init)
    r = H(x_next) - y_next
    if noise_type == "gaussian":
        loss = lmbda * torch.sum(r ** 2, dim=(1, 2, 3))
    elif noise_type == "laplace":
        loss = lmbda * torch.sum(torch.abs(r), dim=(1, 2, 3))
    else:
        raise ValueError("Noise type not supported")
    return loss, pred, y_next, r


def trace_value(vel, x, num_t, eps, create_graph=False):
    """hut_estimator(1, v, x, num_t) with the probe given: eps . (J eps) per image, by forward-over-reverse autograd."""
    t1 = torch.ones(len(x), dtype=x.dtype) * num_t
    prod = torch.autograd.functional.jvp(lambda a: vel(a, t1), x, eps, create_graph=create_graph)[1]
    return (prod * eps).sum(dim=(1, 2, 3))


def grad(vel, H, x, x_init, y, eps, i, N, lmbda, noise_type="gaussian", start_time=0.0, zero_trace=False):
    """One inner step's gradient at x -> (g, g_data, g_trace, g_extra, pred, info); the exact (autograd) trace gradient.
    info: y_next, the residual r, the data loss value (summed over the batch)."""
    num_t, dt = schedule(N, start_time, i)
    x = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        loss, pred, y_next, r = _data_loss(vel, H, x, x_init, y, num_t, dt, lmbda, noise_type)
        (g_data,) = torch.autograd.grad(loss.sum(), x)
        if zero_trace:
            g_trace = torch.zeros_like(g_data)
        else:
            tr = trace_value(vel, x, num_t, eps, create_graph=True) * dt
            (g_trace,) = torch.autograd.grad(tr.sum(), x)
    xd, pred = x.detach(), pred.detach()
    g_extra = xd.clone() if i == 0 else (- 1.0 / (1.0 - num_t) * (-xd + num_t * pred))
    g = g_data + g_trace + g_extra
    return g, g_data, g_trace, g_extra, pred, dict(y_next=y_next.detach(), r=r.detach(), loss=float(loss.detach().sum()), num_t=num_t, dt=dt)


def fd_grad_trace(vel, x, eps, i, N, h, start_time=0.0):
    """dt (J(x + h eps)^T eps - J(x - h eps)^T eps) / (2 h) on the oracle's first-order VJP (O.unet_vjp)."""
    num_t, dt = schedule(N, start_time, i)
    t1 = torch.ones(len(x), dtype=x.dtype) * num_t
    return dt * (vel.vjp(x + h * eps, t1, eps) - vel.vjp(x - h * eps, t1, eps)) / (2 * h)


def vjp(vel, x, num_t, vec):
    return vel.vjp(x, torch.ones(len(x), dtype=x.dtype) * num_t, vec)


def step(vel, H, x, x_init, y, eps_list, i, N, lmbda, eta, noise_type="gaussian", start_time=0.0, zero_trace=False):
    """One outer iteration: a fresh Adam, len(eps_list) inner steps, then x + v(x, t) dt.  Returns (x_new, x after the Adam steps, first g)."""
    num_t, dt = schedule(N, start_time, i)
    x = x.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=eta)
    g0 = None
    for eps in eps_list:
        g = grad(vel, H, x.detach(), x_init, y, eps, i, N, lmbda, noise_type, start_time, zero_trace)[0]
        g0 = g if g0 is None else g0
        opt.zero_grad()
        x.grad = g
        opt.step()
    xa = x.detach().clone()
    with torch.no_grad():
        t1 = torch.ones(len(xa), dtype=xa.dtype) * num_t
        x_new = xa + vel(xa, t1) * dt
    return x_new, xa, g0


def solve(vel, H, x_init, y, probes, N, K, lmbda, eta, noise_type="gaussian", start_time=0.0, zero_trace=False):
    """The whole N x K loop from x = x_init; probes(i, k) -> eps.  Returns the final iterate."""
    x = x_init.clone()
    for i in range(N):
        x = step(vel, H, x, x_init, y, [probes(i, k) for k in range(K)], i, N, lmbda, eta, noise_type, start_time, zero_trace)[0]
    return x


# ---- the fixture cases (tools/make_golden_flow_priors.py writes them, the tests re-make their inputs from the same seeds) ------------------
N_STEP, LMBDA, ETA = 100, 1000.0, 0.01          # config/method_config/flow_priors.yaml
FD_STEPS = (3e-3, 1e-2, 3e-2)
FREE_N = 24
# name -> (problem, noise type, outer iteration, sigma_noise (main.py's table), seed)
CASES = {"inpainting_it0": ("inpainting", "gaussian", 0, 0.05, 11),
         "inpainting_it50": ("inpainting", "gaussian", 50, 0.05, 12),
         "inpainting_laplace": ("inpainting", "laplace", 30, 0.3, 13),
         "random_inpainting": ("random_inpainting", "gaussian", 20, 0.01, 14),
         "superresolution": ("superresolution", "gaussian", 40, 0.05, 15),
         "gaussian_deblurring_FFT": ("gaussian_deblurring_FFT", "gaussian", 60, 0.05, 16),
         "denoising_laplace": ("denoising", "laplace", 70, 0.3, 17)}
FREE_CASE = ("inpainting", "gaussian", 0, 0.05, 21)
NCSNPP_CASE = ("inpainting", "gaussian", 50, 0.05, 31)


def det_normal(shape, seed, idx=0):
    g = np.random.Generator(np.random.Philox(key=[seed, idx]))
    return torch.from_numpy(g.standard_normal(size=shape, dtype=np.float32))


def det_image(shape, seed):
    """The synthetic clean image of tools/make_golden.py / tests/conftest.py."""
    x = det_normal(shape, seed, 7)
    k = torch.ones(shape[1], 1, 3, 3) / 9.0
    for _ in range(5):
        x = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), k, groups=shape[1])
    lo = x.amin(dim=(1, 2, 3), keepdim=True); hi = x.amax(dim=(1, 2, 3), keepdim=True)
    return ((x - lo) / (hi - lo) * 2 - 1).contiguous()


def det_laplace(shape, seed, idx=0):
    """Laplace(0, 1) draws by inverse CDF from numpy Philox uniforms."""
    g = np.random.Generator(np.random.Philox(key=[seed, idx]))
    u = g.uniform(-0.5, 0.5, size=shape)
    return torch.from_numpy((-np.sign(u) * np.log1p(-2 * np.abs(u))).astype(np.float32))


def oracle_degradation(problem, S, half=10):
    return {"denoising": lambda: O.Denoising(), "inpainting": lambda: O.BoxInpainting(half), "random_inpainting": lambda: O.RandomInpainting(0.7),
            "superresolution": lambda: O.Superresolution(2, S), "gaussian_deblurring_FFT": lambda: O.GaussianDeblurring(1.0, 61, "fft", 3, S)}[problem]()


def case_inputs(case, S=64, B=2, half=10):
    """(operator, noise type, iteration, dict(clean, x_init, x, y, eps)) of a case, fp32, from its seed alone.  x is x_init on iteration 0 and a
    point near the straight path from x_init to the clean image otherwise."""
    problem, noise_type, it, sigma, seed = case
    shape = (B, 3, S, S)
    op = oracle_degradation(problem, S, half)
    clean = det_image(shape, seed)
    x_init = det_normal(shape, seed, 1)
    num_t, _ = schedule(N_STEP, 0.0, it)
    x = x_init.clone() if it == 0 else ((1 - num_t) * x_init + num_t * clean + 0.05 * det_normal(shape, seed, 2)).float()
    hx = op.H(clean)
    noise = det_normal(tuple(hx.shape), seed, 3) if noise_type == "gaussian" else det_laplace(tuple(hx.shape), seed, 3)
    y = (hx + sigma * noise).float()
    return op, noise_type, it, dict(clean=clean, x_init=x_init, x=x, y=y, eps=probe(shape, seed, 4))


def tolerances(g, h, lmbda=LMBDA, dt=1.0 / N_STEP, laplace=False):
    """The bounds of the GPU tests from a fixture's stored maxima (the project's constants: forward 2e-5 of max, VJP 2e-5 + 5e-5 max|.|):
    (TOL_fwd, TOL_data, TOL_trace, TOL_g)."""
    tol_fwd = 2e-5 * float(g["pred_max"])
    vjp = lambda m: 2e-5 + 5e-5 * float(m)
    c = lmbda if laplace else 2 * lmbda
    tol_data = c * dt * tol_fwd + dt * vjp(g["jtw_max"])
    k = list(FD_STEPS).index(h)
    tol_trace = float(g["trunc64"][k]) + dt * vjp(g["jteps_max"]) / h
    return tol_fwd, tol_data, tol_trace, tol_data + tol_trace + 1e-6 * float(g["g_extra_max"])


# ---- torch.optim.Adam as the yardstick of csrc/adam_step.h (CPU test on the host shim, GPU test on pf_adam_step) ---------------------------
def adam_inputs(n, seed):
    """x and three gradients of n values: normal entries at several scales plus exact zeros, denormals and +-1e30."""
    g = np.random.Generator(np.random.Philox(key=[seed, 0]))
    x = g.standard_normal(n).astype(np.float32) * 3
    gs = []
    for k in range(3):
        a = (g.standard_normal(n) * 10.0 ** g.integers(-6, 4, n)).astype(np.float32)
        a[k::17] = 0.0
        a[5 + k::29] = np.float32(1e-41) * (1 + k)          # denormal
        a[7 + k::31] = np.float32(1e30) * (-1) ** k
        gs.append(a)
    return x, gs


def torch_adam_reference(x, gs, lr):
    """(x, exp_avg, exp_avg_sq) after every step of torch.optim.Adam (CPU, fp32) on the gradients gs."""
    p = torch.from_numpy(x.copy()).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=lr)
    out = []
    for g in gs:
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
    return out


def check_adam_bound(x, m, v, rx, rm, rv, lr, what):
    """x within 2 ulp(|x|) + 1e-6 lr of torch's, m and v within 2 ulp (an overflowed v must be torch's inf)."""
    ulp = lambda a: np.spacing(np.abs(a).astype(np.float32))
    fin = np.isfinite(rv)
    assert np.array_equal(fin, np.isfinite(v)), what
    assert np.all(np.abs(x - rx) <= 2 * ulp(rx) + 1e-6 * lr), (what, float(np.abs(x - rx).max()))
    assert np.all(np.abs(m - rm) <= 2 * ulp(rm)), (what, "m")
    assert np.all(np.abs(v[fin] - rv[fin]) <= 2 * ulp(rv[fin])), (what, "v")
    assert np.array_equal(v[~fin], rv[~fin]), (what, "overflowed v")
