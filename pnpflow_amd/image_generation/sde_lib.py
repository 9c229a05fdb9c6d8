"""`RectifiedFlow` with the constructor and sampling surface of pnpflow/image_generation/sde_lib.py (reference :7-104), on the HIP engine.

    sde = RectifiedFlow(init_type='gaussian', noise_scale=1.0, use_ode_sampler='rk45', sigma_var=0.0, ode_tol=1e-5, sample_N=100)
    x1 = sde.ode(z0, model)                      # z0 -> data, SciPy's RK45 rules at rtol = atol = 1e-5 (pf_flow_ode_rk45)
    z0 = sde.ode(x1, model, reverse=True)        # data -> latent
    x1 = sde.euler_ode(z0, model, N=100)         # N Euler steps (pf_rf_euler_sampler at sigma_var = 0)

The reference moves the state to the host and back for every evaluation of solve_ivp; here each solve is one engine call with the state on
the device.  Training (the reflow losses and time schedules) is out of scope: reflow_flag=True raises NotImplementedError.
"""
from __future__ import annotations

import torch

EPS = 1e-3          # the start time of every sampler of the reference (sde_lib.py:45, 77; sampling.py:91, 123)
LABEL_SCALE = 999.0  # model_fn(x, t * 999) (sde_lib.py:57, 90; sampling.py:97, 140)


def engine_net(model, who):
    """The engine net behind `model` (a DataParallel-style wrapper's `.module`, or the net itself)."""
    net = getattr(model, "module", model)
    if not hasattr(net, "rf_euler") or not hasattr(net, "ode_rk45"):
        raise TypeError(f"{who} needs an engine net (pnpflow_amd UNet / NCSNpp)")
    return net


def set_label_scale(net):
    """The samplers feed a net that takes a scaled label (NCSN++: it has set_solver_time_scale) t * 999; a U-Net is fed t as it is, so its
    engine's scale is put (back) to 1.  -> the scale set."""
    if hasattr(net, "set_solver_time_scale"):
        net.set_solver_time_scale(LABEL_SCALE)
        return LABEL_SCALE
    lib = getattr(net, "_lib", None)
    if lib is not None:
        from .. import _lib
        _lib.check(lib.pf_engine_set_solver_time_scale(net.handle, 1.0), net.handle, "pf_engine_set_solver_time_scale")
    return 1.0


class RectifiedFlow():
    def __init__(self, init_type='gaussian', noise_scale=1.0, reflow_flag=False, reflow_t_schedule='uniform', reflow_loss='l2', use_ode_sampler='rk45',
                 sigma_var=0.0, ode_tol=1e-5, sample_N=None):
        if reflow_flag:
            raise NotImplementedError("reflow training (reflow_flag=True: the reflow time schedules and losses) is not implemented by this engine (inference only)")
        if sample_N is not None:
            self.sample_N = sample_N
            print('Number of sampling steps:', self.sample_N)
        self.init_type = init_type
        self.noise_scale = noise_scale
        self.use_ode_sampler = use_ode_sampler
        self.ode_tol = ode_tol
        self.sigma_var = sigma_var
        self.sigma_t = lambda t: (1. - t) * sigma_var
        print('Init. Distribution Variance:', self.noise_scale)
        print('SDE Sampler Variance:', sigma_var)
        print('ODE Tolerence:', self.ode_tol)
        self.reflow_flag = False
        self.last_ode_stats = None

    @property
    def T(self):
        return 1.

    @torch.no_grad()
    def ode(self, init_input, model, reverse=False):
        """solve_ivp(ode_func, (eps, T) or, reversed, (T, eps), method='RK45', rtol = atol = 1e-5) of sde_lib.py:37-72 -> the state at the end.
        The error norm runs over the whole batch (SciPy sees it flattened into one vector): the images of a batch share one step sequence."""
        net = engine_net(model, "RectifiedFlow.ode")
        set_label_scale(net)
        t0, t1 = (self.T, EPS) if reverse else (EPS, self.T)
        x, self.last_ode_stats = net.ode_rk45(init_input, t0, t1, 1e-5, 1e-5)
        return x

    @torch.no_grad()
    def euler_ode(self, init_input, model, reverse=False, N=100):
        """N Euler steps x += v(x, num_t) / N at num_t = i/N (T - eps) + eps (sde_lib.py:74-94).  `reverse` IS IGNORED, as in the reference:
        its loop is the same for both values (the time always runs from eps towards T)."""
        net = engine_net(model, "RectifiedFlow.euler_ode")
        set_label_scale(net)
        return net.rf_euler(init_input, int(N), t_begin=EPS, t_end=self.T, sigma_var=0.0, noise_scale=1.0)

    def get_z0(self, batch, train=True):
        """A CPU torch.randn draw of the batch's shape times noise_scale, as the reference draws it: torch.manual_seed reproduces it."""
        n, c, h, w = batch.shape
        if self.init_type == 'gaussian':
            cur_shape = (n, c, h, w)
            return torch.randn(cur_shape) * self.noise_scale
        else:
            raise NotImplementedError("INITIALIZATION TYPE NOT IMPLEMENTED")
