"""The rectified-flow samplers with the API of pnpflow/image_generation/sampling.py (reference :36-161), on the HIP engine.

    sde = sde_lib.RectifiedFlow(init_type=c.init_type, noise_scale=c.init_noise_scale, use_ode_sampler=c.use_ode_sampler,
                                sigma_var=c.sigma_variance, ode_tol=c.ode_tol, sample_N=c.sample_N)          # c = config.sampling
    sampling_fn = get_sampling_fn(config, sde, shape, inverse_scaler, eps)
    x, nfe = sampling_fn(model)                  # or sampling_fn(model, z=latent)

euler_sampler is one engine call (pf_rf_euler_sampler: N forwards and N fused updates, no host synchronisation), rk45_sampler one
pf_flow_ode_rk45 solve (SciPy's RK45 step control on the host from an 8-byte error norm per attempt, the state on the device).  The
reference moves the state to the host and back for every evaluation.  `PriorSampler` gives a rectified checkpoint the sampling surface
compute_metric.ComputeMetric and tools/prior_report.py take from FLOW_MATCHING.
"""
from __future__ import annotations

import torch

from . import sde_lib
from .sde_lib import EPS, engine_net, set_label_scale


def get_sampling_fn(config, sde, shape, inverse_scaler, eps):
    """sampling.py:36-59.  `eps` is accepted and, as in the reference, not used: the samplers start at their own 1e-3."""
    sampler_name = config.sampling.method
    if sampler_name.lower() == 'rectified_flow':
        sampling_fn = get_rectified_flow_sampler(sde=sde, shape=shape, inverse_scaler=inverse_scaler, device=getattr(config, "device", 'cuda'))
    else:
        raise ValueError(f"Sampler name {sampler_name} unknown.")
    return sampling_fn


def _philox_key():
    """(seed, stream) of an in-kernel noise draw: torch.initial_seed() (what torch.manual_seed set) and the process's draw counter."""
    from .. import utils
    stream = utils._device_draws
    utils._device_draws += 1
    return torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, stream


def get_rectified_flow_sampler(sde, shape, inverse_scaler, device='cuda'):
    """sampling.py:62-161 -> euler_sampler or rk45_sampler, by sde.use_ode_sampler; each returns (inverse_scaler(x), evaluations).
    Both feed the net t * 999 where it takes a scaled label (NCSN++) and t as it is otherwise (the U-Net)."""

    def initial(z):
        if z is None:
            return sde.get_z0(torch.zeros(shape, device='cpu'), train=False).to(device).detach().clone()
        return z

    def euler_sampler(model, z=None, noise=None):
        """sde.sample_N steps from t = 1e-3 with dt = 1 / sample_N (sampling.py:69-109); the Euler-Maruyama form when the SDE's sigma_var > 0.
        `noise` (sample_N, B, C, H, W): the normal draws of the steps, injected; otherwise the engine's Philox normals, drawn in the kernel."""
        with torch.no_grad():
            net = engine_net(model, "euler_sampler")
            x = initial(z)
            set_label_scale(net)
            sigma_var = float(getattr(sde, "sigma_var", sde.sigma_t(0.0)))          # sigma_t(0) = sigma_var
            seed, stream = (0, 0) if (noise is not None or sigma_var == 0.0) else _philox_key()
            x = net.rf_euler(x, int(sde.sample_N), t_begin=EPS, t_end=sde.T, sigma_var=sigma_var, noise_scale=float(sde.noise_scale), noise=noise,
                             seed=seed, stream_id=stream)
            x = inverse_scaler(x)
            nfe = sde.sample_N
            return x, nfe

    def rk45_sampler(model, z=None):
        """solve_ivp(ode_func, (1e-3, sde.T), method='RK45', rtol = atol = sde.ode_tol) (sampling.py:111-153).  The error norm runs over the whole
        batch, as SciPy's does over the flattened state: the images of a batch share one step sequence."""
        with torch.no_grad():
            net = engine_net(model, "rk45_sampler")
            x = initial(z)
            set_label_scale(net)
            x, stats = net.ode_rk45(x, EPS, sde.T, sde.ode_tol, sde.ode_tol)
            rk45_sampler.last_stats = stats
            x = inverse_scaler(x)
            return x, stats["nfev"]

    rk45_sampler.last_stats = None
    print('Type of Sampler:', sde.use_ode_sampler)
    if sde.use_ode_sampler == 'rk45':
        return rk45_sampler
    elif sde.use_ode_sampler == 'euler':
        return euler_sampler
    else:
        assert False, 'Not Implemented!'


def rectified_flow_from_config(config, **overrides):
    """RectifiedFlow from a rectified-flow config's `config.sampling`; overrides: use_ode_sampler, sample_N, sigma_variance, ode_tol."""
    c = dict(config.sampling)
    unknown = set(overrides) - {"use_ode_sampler", "sample_N", "sigma_variance", "ode_tol"}
    if unknown:
        raise ValueError(f"unknown sampling overrides {sorted(unknown)}")
    c.update({k: v for k, v in overrides.items() if v is not None})
    return sde_lib.RectifiedFlow(init_type=c["init_type"], noise_scale=c["init_noise_scale"], use_ode_sampler=c["use_ode_sampler"],
                                 sigma_var=float(c["sigma_variance"]), ode_tol=float(c["ode_tol"]), sample_N=int(c["sample_N"]))


class PriorSampler:
    """The sampling surface ComputeMetric and the prior report take from FLOW_MATCHING, for a rectified-flow net:

        PriorSampler(model, sde, (B, C, H, W)).apply_flow_matching(n)                       # (n, C, H, W)
        PriorSampler(model, sde, shape).generate_samples(n_samples, batch_size)             # (n_samples, C, H, W)

    Samples come back in the loaders' data range [-1, 1] (the inverse scaler is the identity), so ComputeMetric sees what it sees from
    FLOW_MATCHING.  `shape[0]` is the default batch size; only the image dimensions of `shape` bind.
    The reference's own compute_metrics path for `model rectified` would call the net through FLOW_MATCHING's cnf, i.e. WITHOUT the * 999
    label scale the net was trained with; that is not reproduced here: the samples come from the reference's sampler (sampling.py)."""

    def __init__(self, model, sde, shape, device='cuda'):
        self.model, self.sde, self.shape, self.device = model, sde, tuple(shape), device
        self.last_nfe = None
        self._fns = {}          # batch size -> sampling function

    @staticmethod
    def batch_sizes(n_samples, batch_size):
        """Full batches, then the remainder (FLOW_MATCHING.sample_schedule's split)."""
        if batch_size is None or batch_size <= 0:
            batch_size = n_samples
        sizes = [batch_size] * (n_samples // batch_size) if batch_size else []
        if batch_size and n_samples % batch_size:
            sizes.append(n_samples % batch_size)
        return sizes

    def _draw(self, n, z=None):
        if n not in self._fns:
            self._fns[n] = get_rectified_flow_sampler(self.sde, (n,) + self.shape[1:], inverse_scaler=lambda x: x, device=self.device)
        x, self.last_nfe = self._fns[n](self.model, z=z)
        return x

    def apply_flow_matching(self, NO_samples, latent=None):
        if latent is not None and latent.shape[0] != NO_samples:
            raise ValueError(f"latent holds {latent.shape[0]} samples, NO_samples is {NO_samples}")
        if NO_samples == 0:
            return torch.empty((0,) + self.shape[1:], device=self.device)
        return self._draw(NO_samples, latent)

    def generate_samples(self, n_samples, batch_size=None, latent=None):
        if latent is not None and latent.shape[0] != n_samples:
            raise ValueError(f"latent holds {latent.shape[0]} samples, n_samples is {n_samples}")
        out, first = [], 0
        for b in self.batch_sizes(n_samples, batch_size if batch_size is not None else self.shape[0]):
            out.append(self._draw(b, None if latent is None else latent[first:first + b].to(self.device)))
            first += b
        return torch.cat(out, dim=0) if out else torch.empty((0,) + self.shape[1:], device=self.device)
