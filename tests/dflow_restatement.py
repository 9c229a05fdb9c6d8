"""CPU restatement of D-Flow (pnpflow/methods/d_flow.py) that the D-Flow tests lean on: T(z), the closure's value and its autograd
gradient, the hand-written adjoint recursion the engine implements, a dopri5 that follows the engine's step-control rules
(include/pnpflow_hip.h pf_flow_ode_dopri5; torchdiffeq 0.2.x dopri5 as we understand it) and the full LBFGS solve.

`vel(x, t)` is any velocity field: the oracle net `lambda x, t: O.unet_forward(sd, cfg, x, t)` or a smooth stand-in.
"""
import numpy as np
import torch

f32 = np.float32


def schedule(steps_euler, start_time=0.0):
    """(t_i, t_i + delta/2, delta) with the reference's fp32 expressions (d_flow.py:43-47)."""
    delta = (1 - start_time) / (steps_euler - 1)
    t = [torch.ones(1) * delta * i + start_time for i in range(steps_euler - 1)]
    return [float(a[0]) for a in t], [float((a + delta / 2)[0]) for a in t], delta


def T(z, vel, steps_euler=6, start_time=0.0):
    """forward_flow_matching (d_flow.py:41-49)."""
    delta = (1 - start_time) / (steps_euler - 1)
    for i in range(steps_euler - 1):
        t1 = torch.ones(len(z), dtype=z.dtype) * delta * i + start_time
        z = z + delta * vel(z + delta / 2 * vel(z, t1), t1 + delta / 2)
    return z


def loss_per_image(z, y, H, vel, lmbda, steps_euler=6, start_time=0.0):
    """The closure's terms per image (d_flow.py:110-121)."""
    d = z.shape[1] * z.shape[2] * z.shape[3]
    nrm = torch.sqrt((z ** 2).sum([1, 2, 3]))
    reg = 0.5 * torch.clamp(nrm ** 2, min=-1e6, max=1e6) - (d - 1) * torch.log(nrm + 1e-5)
    return torch.sum((H(T(z, vel, steps_euler, start_time)) - y) ** 2, dim=(1, 2, 3)) + lmbda * reg


def value_and_grad(z, y, H, vel, lmbda, steps_euler=6, start_time=0.0):
    """(loss per image, d sum(loss) / dz) by autograd through T."""
    z = z.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        per = loss_per_image(z, y, H, vel, lmbda, steps_euler, start_time)
        (g,) = torch.autograd.grad(per.sum(), z)
    return per.detach(), g


def adjoint_grad(z, y, H, H_adj, vel, lmbda, steps_euler=6, start_time=0.0):
    """The engine's gradient, written out: forward with saved inputs z_i, u_i; seed g = 2 H_adj(H(T z) - y); per midpoint step in
    reverse  h = delta J_v(u_i)^T g,  g <- g + h + (delta/2) J_v(z_i)^T h;  plus lmbda (z [|z|^2 in +-1e6] - (d-1)/(|z|+1e-5) z/|z|).
    The J^T products are autograd VJPs of single velocity evaluations."""
    delta = (1 - start_time) / (steps_euler - 1)
    zs, us, ts, tms = [], [], [], []
    x = z.detach()
    with torch.no_grad():
        for i in range(steps_euler - 1):
            t1 = torch.ones(len(z), dtype=z.dtype) * delta * i + start_time
            u = x + delta / 2 * vel(x, t1)
            zs.append(x); us.append(u); ts.append(t1); tms.append(t1 + delta / 2)
            x = x + delta * vel(u, t1 + delta / 2)

    def vjp(a, t, vec):
        a = a.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            (ga,) = torch.autograd.grad(vel(a, t), a, vec)
        return ga
    g = 2 * H_adj(H(x) - y)
    for i in reversed(range(steps_euler - 1)):
        h = delta * vjp(us[i], tms[i], g)
        g = g + h + delta / 2 * vjp(zs[i], ts[i], h)
    d = z.shape[1] * z.shape[2] * z.shape[3]
    s = (z ** 2).sum([1, 2, 3]).view(-1, 1, 1, 1)
    nrm = torch.sqrt(s)
    mask = ((s >= -1e6) & (s <= 1e6)).to(z.dtype)
    return g + lmbda * (mask * z - (d - 1) / (nrm + 1e-5) * z / nrm)


# ---- dopri5 --------------------------------------------------------------------------------------------------------------------------
DP_ALPHA = [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1., 1.]
DP_BETA = [[1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9], [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
           [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656], [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]]
DP_ERR = [35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 - -12231 / 42400, 11 / 84 - 649 / 6300, -1 / 60]
DP_MID = [6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2, 187940372067 / 1594534317056 / 2,
          -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2]


def dopri5(vel, y0, t0=1.0, t1=0.0, rtol=1e-5, atol=1e-5, max_steps=1000):
    """dx/dt = vel(x, t) from t0 to t1 (fp32 state; fp64 time and step sizes; time rounded to fp32 for the net):
      * decreasing time as s = -t, f(s, y) = -vel(y, -s);
      * initial step: Hairer's rule with order 4 (one extra evaluation);
      * error norm: RMS over the whole tensor of err / (atol + rtol max(|y0|, |y1|)); accept if ratio <= 1;
      * next step: dt min(10, max(0.9 ratio^(-1/5), 0.2)), the 0.2 floor replaced by 1 when ratio < 1, dt 10 when ratio == 0;
      * FSAL; the result is the 4th-order dense output at t1.
    Returns (y(t1), dict(accepted, rejected, nfev)); raises past max_steps attempts."""
    rev = t1 < t0
    sg = -1.0 if rev else 1.0
    s0, send = (-t0, -t1) if rev else (t0, t1)
    y = y0.detach().float().clone()
    B, N = y.shape[0], y.numel()
    st = dict(accepted=0, rejected=0, nfev=0)

    def f(s, x):
        st["nfev"] += 1
        tt = float(-f32(s)) if rev else float(f32(s))
        return sg * vel(x, torch.full((B,), tt, dtype=torch.float32))

    def rms(q):
        return float(f32(np.sqrt(float((q * q).double().sum()) / N)))

    def combine(base, coefs, ks):
        acc = torch.zeros_like(base)
        for c, k in zip(coefs, ks):
            acc = acc + float(c) * k
        return base + acc

    with torch.no_grad():
        k = [None] * 7
        k[0] = f(s0, y)
        scale = atol + torch.abs(y) * rtol
        d0, d1 = rms(y / scale), rms(k[0] / scale)
        h0 = f32(1e-6) if (d0 < 1e-5 or d1 < 1e-5) else f32(f32(f32(0.01) * f32(d0)) / f32(d1))
        fh = f(f32(f32(s0) + h0), y + float(h0) * k[0])
        d2 = abs(f32(rms((fh - k[0]) / scale)) / h0)
        if d1 <= 1e-15 and d2 <= 1e-15:
            h1 = max(f32(1e-6), f32(h0 * f32(1e-3)))
        else:
            h1 = np.power(f32(f32(0.01) / f32(max(d1, d2))), f32(0.2))
        dt = float(min(f32(100) * h0, h1))
        t = s0
        out = None
        while send > t:
            if st["accepted"] + st["rejected"] >= max_steps:
                raise RuntimeError(f"dopri5: step cap of {max_steps} attempts exceeded")
            assert t + dt > t, "step size underflow"
            tn = t + dt
            tf, dtf = f32(t), f32(dt)
            ys = None
            for i in range(6):
                ti = f32(tn) if DP_ALPHA[i] == 1. else f32(tf + f32(f32(DP_ALPHA[i]) * dtf))
                ys = combine(y, [f32(f32(b) * dtf) for b in DP_BETA[i]], k[:i + 1])
                k[i + 1] = f(ti, ys)
            y1 = ys
            err = combine(torch.zeros_like(y), [f32(f32(c) * dtf) for c in DP_ERR], k)
            ratio = rms(err / (atol + rtol * torch.maximum(y.abs(), y1.abs())))
            if not np.isfinite(ratio):
                raise RuntimeError("dopri5: non-finite error estimate")
            if ratio <= 1:
                st["accepted"] += 1
                if send <= tn:
                    ymid = combine(y, [f32(dtf * f32(m)) for m in DP_MID], k)
                    f0, f1 = k[0], k[6]
                    a = float(f32(2) * dtf) * (f1 - f0) - 8 * (y1 + y) + 16 * ymid
                    b = float(dtf) * (5 * f0 - 3 * f1) + 18 * y + 14 * y1 - 32 * ymid
                    c = float(dtf) * (f1 - 4 * f0) - 11 * y - 5 * y1 + 16 * ymid
                    d = float(dtf) * f0
                    x = float(f32((send - t) / (tn - t)))
                    out = y + x * d + x ** 2 * c + x ** 3 * b + x ** 4 * a
                t = tn
                y = y1
                k[0] = k[6]
            else:
                st["rejected"] += 1
            if ratio == 0:
                dt = dt * 10.0
            else:
                dt = dt * min(10.0, max(0.9 / ratio ** (1 / 5), 1.0 if ratio < 1 else 0.2))
    return out, st


# ---- the full solve --------------------------------------------------------------------------------------------------------------------
def solve(z_init, y, H, vel, lmbda, lbfgs_iter, max_iter, steps_euler=6):
    """The LBFGS stage of solve_ip (d_flow.py:93-128) from the blended latent z_init: torch.optim.LBFGS with the reference's arguments.
    Returns (T(z) after every outer step, closure calls of every outer step)."""
    z = z_init.detach().clone().requires_grad_(True)
    opt = torch.optim.LBFGS([z], max_iter=lbfgs_iter, history_size=100, line_search_fn='strong_wolfe')
    restored, calls = [], []

    def closure():
        opt.zero_grad()
        per, g = value_and_grad(z.detach(), y, H, vel, lmbda, steps_euler)
        z.grad = g
        n[0] += 1
        return per.sum()
    for _ in range(max_iter):
        n = [0]
        opt.step(closure)
        calls.append(n[0])
        with torch.no_grad():
            restored.append(T(z.detach(), vel, steps_euler))
    return restored, calls
