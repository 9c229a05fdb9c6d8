"""CPU checks of the D-Flow method (pnpflow/methods/d_flow.py): the C ABI surface, the config / CLI wiring, the adjoint recursion the
engine implements (fp64, against autograd), the restatement's dopri5 and the restatement against goldens of the REAL reference
(tests/golden/d_flow_tiny4_*.npz, tools/make_golden_dflow.py).  No GPU needed.
"""
import os
import re

import numpy as np
import pytest
import torch

from conftest import CFGS, det_image, det_normal
from oracle import pnpflow_oracle as O
import dflow_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("pf_d_flow_forward", "pf_d_flow_value_and_grad", "pf_flow_ode_dopri5")
PROBLEMS = ["denoising", "inpainting", "superresolution", "gaussian_deblurring_FFT"]
LATENT_SEED, NOISE_SEED = 71, 73        # tools/make_golden_dflow.py


def test_new_symbols_declared_exported_and_typed():
    import pnpflow_amd._lib as L
    header = open(os.path.join(ROOT, "include", "pnpflow_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in include/pnpflow_hip.h"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
    if os.path.isfile(L.LIB_PATH):
        lib = L.load()
        for name in NEW_SYMBOLS:
            assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    import __graft_entry__ as G
    assert "flow_solvers.hip" in G.SOURCES


def test_config_and_cli_dispatch():
    from pnpflow_amd.utils import load_cfg_from_cfg_file
    cfg = load_cfg_from_cfg_file(os.path.join(ROOT, "config", "method_config", "d_flow.yaml"))
    # the reference's config/method_config/d_flow.yaml: keys in this order (they name the results directory), these values
    assert list(cfg.keys()) == ["steps_euler", "lmbda", "alpha", "max_iter", "LBFGS_iter", "start_time"]
    assert dict(cfg) == dict(steps_euler=6, lmbda=0.01, alpha=0.1, max_iter=20, LBFGS_iter=20, start_time=0.0)
    src = open(os.path.join(ROOT, "main.py")).read()
    assert "args.method == 'd_flow'" in src and "D_FLOW(model, device, args)" in src
    from pnpflow.methods.d_flow import D_FLOW
    from pnpflow_amd.methods.d_flow import D_FLOW as D2
    assert D_FLOW is D2
    for m in ("model_forward", "gaussian", "forward_flow_matching", "inverse_flow_matching", "compute_norm", "solve_ip", "run_method"):
        assert callable(getattr(D_FLOW, m))


def _smooth_field(x, t):
    """A smooth stand-in velocity with a non-trivial Jacobian (couples pixels and channels) and time dependence."""
    return torch.sin(x) * (1 + t.view(-1, 1, 1, 1)) + 0.3 * torch.roll(x, 1, dims=3) * t.view(-1, 1, 1, 1) - 0.2 * torch.tanh(x.flip(1))


def _check_adjoint(vel, shape, H, H_adj, y, lmbda=0.01):
    z = det_normal(shape, 61).double() * 3
    _, g_ref = R.value_and_grad(z, y, H, vel, lmbda)
    g = R.adjoint_grad(z, y, H, H_adj, vel, lmbda)
    np.testing.assert_allclose(g.numpy(), g_ref.numpy(), rtol=1e-10, atol=1e-10 * float(g_ref.abs().max()))


@pytest.mark.parametrize("op", ["denoising", "box", "sr2"])
def test_adjoint_recursion_matches_autograd_fp64_smooth_field(op):
    S = 16
    d = {"denoising": O.Denoising(), "box": O.BoxInpainting(3), "sr2": O.Superresolution(2, S)}[op]
    shape = (2, 3, S, S)
    y = d.H(det_normal(shape, 62).double())
    _check_adjoint(_smooth_field, shape, d.H, d.H_adj, y)


def test_adjoint_recursion_matches_autograd_fp64_tiny4(monkeypatch):
    c = CFGS["tiny4"]; cfg = O.unet_config(**c)
    sd = {k: v.double() for k, v in O.synthetic_state_dict(cfg, 0).items()}
    emb = O.sinusoidal_embedding
    monkeypatch.setattr(O, "sinusoidal_embedding", lambda t, dim: emb(t, dim).double())
    d = O.BoxInpainting(10)
    shape = (1, 3, 64, 64)
    y = d.H(det_image(shape, 63).double())
    _check_adjoint(lambda x, t: O.unet_forward(sd, cfg, x, t), shape, d.H, d.H_adj, y, lmbda=0.001)


def test_regulariser_clamp_gradient_switches_off_outside_the_clamp():
    """|z|^2 > 1e6: the clamp passes no gradient (torch.clamp's rule), only the log term remains."""
    zero = lambda x, t: 0.0 * x
    ident = lambda x: x
    z = torch.full((1, 1, 40, 40), 30.0, dtype=torch.float64)          # |z|^2 = 1.44e6
    _, g_ref = R.value_and_grad(z, torch.zeros_like(z), ident, zero, 0.5)
    g = R.adjoint_grad(z, torch.zeros_like(z), ident, ident, zero, 0.5)
    np.testing.assert_allclose(g.numpy(), g_ref.numpy(), rtol=1e-12)
    d = z[0].numel(); n = float(z.norm())
    np.testing.assert_allclose(g.numpy(), (2 * z - 0.5 * (d - 1) / (n + 1e-5) * z / n).numpy(), rtol=1e-12)      # data term: T = id, y = 0


def test_dopri5_linear_system_against_expm():
    import scipy.linalg
    g = np.random.Generator(np.random.Philox(key=[64, 0]))
    n = 16
    A = g.standard_normal((n, n)) * 0.5 - 1.0 * np.eye(n)
    At = torch.from_numpy(A.astype(np.float32))
    vel = lambda x, t: (x.reshape(x.shape[0], -1) @ At.T).reshape(x.shape)
    y0 = torch.from_numpy(g.standard_normal((1, 4, 2, 2)).astype(np.float32))
    rtol = atol = 1e-5
    out, st = R.dopri5(vel, y0, 1.0, 0.0, rtol, atol)
    exact = scipy.linalg.expm(-A) @ y0.reshape(-1).double().numpy()
    err = np.abs(out.reshape(-1).double().numpy() - exact)
    assert (err <= 10 * (atol + rtol * np.abs(exact))).all(), (err.max(), st)
    assert st["accepted"] < 40 and st["nfev"] == 2 + 6 * (st["accepted"] + st["rejected"]), st
    # increasing time as well
    out2, _ = R.dopri5(vel, y0, 0.0, 1.0, rtol, atol)
    exact2 = scipy.linalg.expm(A) @ y0.reshape(-1).double().numpy()
    assert (np.abs(out2.reshape(-1).double().numpy() - exact2) <= 10 * (atol + rtol * np.abs(exact2))).all()


def test_dopri5_step_cap_is_loud():
    vel = lambda x, t: -50.0 * x
    with pytest.raises(RuntimeError, match="step cap"):
        R.dopri5(vel, torch.ones(1, 1, 2, 2), 1.0, 0.0, 1e-5, 1e-5, max_steps=3)


def test_dopri5_tiny4_flow_against_dop853():
    """The restatement's dopri5 on the tiny4 flow (t 1 -> 0) against a DOP853 solve at rtol = atol = 1e-10 (golden, fp64 oracle)."""
    c = CFGS["tiny4"]; cfg = O.unet_config(**c); sd = O.synthetic_state_dict(cfg, 0)
    x0 = det_image((2, 3, 64, 64), 41)
    out, st = R.dopri5(lambda x, t: O.unet_forward(sd, cfg, x, t), x0)
    tight = torch.from_numpy(np.load(os.path.join(GOLD, "d_flow_dop853_tiny4.npz"))["x"])
    err = float((out - tight).abs().max())
    # rtol = atol = 1e-5 bounds the local error per step; measured 1.4e-3 global on this flow (8 accepted steps, 0 rejected)
    assert err < 5e-3, (err, st)
    assert st["rejected"] + st["accepted"] < 30


@pytest.mark.parametrize("problem", PROBLEMS)
def test_restatement_reproduces_reference_goldens(problem):
    g = np.load(os.path.join(GOLD, f"d_flow_tiny4_{problem}.npz"))
    c = CFGS["tiny4"]; cfg = O.unet_config(**c); sd = O.synthetic_state_dict(cfg, 0)
    vel = lambda x, t: O.unet_forward(sd, cfg, x, t)
    S = 64
    d = {"denoising": O.Denoising(), "inpainting": O.BoxInpainting(10), "superresolution": O.Superresolution(2, S),
         "gaussian_deblurring_FFT": O.GaussianDeblurring(1.0, 61, "fft", 3, S)}[problem]
    shape = (2, 3, S, S)
    clean = det_image(shape, 31)
    noisy = d.H(clean) + det_normal(tuple(g["noisy"].shape), NOISE_SEED, 0) * float(g["sigma"])
    np.testing.assert_allclose(noisy.numpy(), g["noisy"], atol=1e-6)
    alpha, lmbda = float(g["alpha"]), float(g["lmbda"])
    z0 = np.sqrt(alpha) * det_normal(shape, LATENT_SEED) + np.sqrt(1 - alpha) * det_normal(shape, NOISE_SEED, 1)
    per, grad = R.value_and_grad(z0, noisy, d.H, vel, lmbda)
    np.testing.assert_allclose(per.numpy(), g["loss0_per_image"], rtol=1e-5)
    np.testing.assert_allclose(grad.numpy(), g["grad0"], atol=1e-4 * float(np.abs(g["grad0"]).max()))
    restored, calls = R.solve(z0, noisy, d.H, vel, lmbda, int(g["lbfgs_iter"]), 2)
    assert calls == list(g["calls_per_step"]), (calls, g["calls_per_step"])
    np.testing.assert_allclose(restored[0].numpy(), g["restored_it1"], atol=1e-3)
    np.testing.assert_allclose(restored[1].numpy(), g["restored_it2"], atol=1e-3)
