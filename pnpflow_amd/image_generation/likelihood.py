"""Log-likelihood in bits/dim under the rectified-flow prior, with the API of pnpflow/image_generation/likelihood.py (reference :116-195).

    likelihood_fn = get_likelihood_fn_rf()
    bpd, z, nfe = likelihood_fn(model, data)

The reference integrates the augmented state (x, logp), d logp/dt = eps . (J_v^T eps), from t = sde.T to t = eps with
scipy.integrate.solve_ivp(method='RK45'), moving the whole state to the host and back for every evaluation.  Here the solve is one engine
call (pf_flow_likelihood_rk45): the state stays on the device, the velocity and the Hutchinson term come from one retained forward and one
hand-written backward per evaluation, and SciPy's step control runs on the host from an 8-byte error norm per attempt.
"""
from __future__ import annotations

import torch

from .. import utils


def get_div_fn(fn):
    raise NotImplementedError("get_div_fn differentiates an arbitrary Python function with autograd; the engine evaluates the divergence of its own "
                              "velocity net (model.divergence / pnpflow_amd.utils.hut_estimator)")


def get_likelihood_fn(sde, inverse_scaler, hutchinson_type='Rademacher', rtol=1e-5, atol=1e-5, method='RK45', eps=1e-5):
    raise NotImplementedError("the SDE form (score model + reverse-time SDE drift) is not implemented by this engine; "
                              "use get_likelihood_fn_rf for the rectified-flow velocity nets")


def get_likelihood_fn_rf(sde=None, inverse_scaler=None, hutchinson_type='Rademacher', rtol=1e-5, atol=1e-5, method='RK45', eps=1e-5):
    """likelihood_fn(model, data, epsilon=None) -> (bpd (B,), z like data, nfe) of likelihood.py:150-193.

    sde: read for `.T` only (default 1).  inverse_scaler: the inverse data normaliser, default x -> (x + 1) / 2; offset = 7 - inverse_scaler(-1).
    hutchinson_type: 'Rademacher' (pf_fill_rademacher) or 'Gaussian' (pf_fill_normal); `epsilon` injects the probe vector instead.
    The net is fed t * 999 where it takes a scaled label (the NCSN++ net; the OT U-Net takes t as it is)."""
    if method != 'RK45':
        raise NotImplementedError(f"ODE method {method!r} is not implemented by this engine (only scipy's 'RK45' rules are)")
    if hutchinson_type not in ('Rademacher', 'Gaussian'):
        raise NotImplementedError(f"Hutchinson type {hutchinson_type} unknown.")
    T = float(getattr(sde, "T", 1.0)) if sde is not None else 1.0
    if inverse_scaler is None:
        inverse_scaler = lambda x: (x + 1.) / 2.
    offset = 7. - float(inverse_scaler(-1.))

    def likelihood_fn(model, data, epsilon=None):
        net = getattr(model, "module", model)
        if not hasattr(net, "likelihood_ode"):
            raise TypeError("likelihood_fn needs an engine net (pnpflow_amd UNet / NCSNpp)")
        if epsilon is None:
            epsilon = utils.device_draw("rademacher" if hutchinson_type == 'Rademacher' else "gaussian", data.shape, data.device)
        if hasattr(net, "set_solver_time_scale"):
            net.set_solver_time_scale(999.0)          # likelihood.py:175-176: vec_t * 999
        z, delta_logp, bpd, stats = net.likelihood_ode(data, epsilon, t0=T, t1=eps, rtol=rtol, atol=atol, offset=offset)
        likelihood_fn.last_stats = stats
        likelihood_fn.last_delta_logp = delta_logp
        return bpd, z, stats["nfev"]

    likelihood_fn.last_stats = None
    likelihood_fn.last_delta_logp = None
    return likelihood_fn
