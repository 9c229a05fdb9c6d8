"""Host side of the zero-boundary Gaussian blur (GaussianDeblurring with any mode but "fft"): the tests' restatement
(tests/zero_blur_restatement.py) reproduces the real reference's fixtures (tools/make_golden_spatial.py) for the operator, GMRES and both
solvers; the Python surface and the C ABI declare the new kind and the Krylov entry points.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import CFGS, det_image, det_normal
from oracle import pnpflow_oracle as O
import zero_blur_restatement as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny4():
    cfg = O.unet_config(**CFGS["tiny4"])
    sd = O.synthetic_state_dict(cfg, 0)
    return cfg, sd


def test_restatement_operator_matches_reference(golden):
    g = golden("zero_blur_op")
    x = det_image((2, 3, 64, 64), 31)
    for sig in (1.0, 3.0):
        d = Z.ZeroBlur(sig, 61, 3, 64)
        np.testing.assert_allclose(d.H(x).numpy(), g[f"blur{sig}_H"], atol=1e-6)
        np.testing.assert_allclose(d.H_adj(x).numpy(), g[f"blur{sig}_Hadj"], atol=1e-6)
        # the fp64 separable form with the 1-D taps is the same operator: zero extension commutes with the two passes
        np.testing.assert_allclose(Z.blur64(x.numpy(), O.gaussian_1d_taps(sig, 61)), g[f"blur{sig}_H"], atol=2e-6)
    # it is not the circular blur: the two differ at the border and agree in the interior
    circ = O.GaussianDeblurring(1.0, 61, "fft", 3, 64).H(x).numpy()
    zero = Z.ZeroBlur(1.0, 61, 3, 64).H(x).numpy()
    assert np.abs(circ - zero)[..., :3, :].max() > 1e-2 and np.abs(circ - zero)[..., 10:-10, 10:-10].max() < 1e-5


def test_restatement_adjoint_and_small_images():
    taps = np.array([0.1, 0.5, 0.25, 0.1, 0.05])           # asymmetric: correlation and convolution differ
    x, y = det_normal((2, 1, 3, 7), 5).numpy(), det_normal((2, 1, 3, 7), 6).numpy()
    assert abs((Z.blur64(x, taps) * y).sum() - (x * Z.blur64(y, taps, adjoint=True)).sum()) < 1e-12
    k = torch.from_numpy(np.outer(taps, taps)).view(1, 1, 5, 5)
    ref = torch.nn.functional.conv2d(torch.from_numpy(x).double(), k, padding="same")       # the radius (2) reaches past the 3-row image
    np.testing.assert_allclose(Z.blur64(x, taps), ref.numpy(), atol=1e-14)


def test_restatement_gmres_matches_reference(golden):
    """O.gmres (fp32, the reference's algorithm) reproduces the reference's solutions; the fp64 restatement is within the stored distance."""
    g = golden("zero_blur_gmres")
    rhs = torch.from_numpy(Z.krylov_rhs())
    np.testing.assert_array_equal(g["rhs"], rhs.numpy())
    d = Z.ZeroBlur(Z.KRYLOV_BLUR[0], Z.KRYLOV_BLUR[1], 3, 128)
    rt2 = torch.tensor(Z.KRYLOV_RT2, dtype=torch.float32)
    for tag, max_iter in (("A", 100), ("B", 5)):
        for b in range(rhs.shape[0]):
            avp = lambda z, b=b: (rt2[b].unsqueeze(0) * d.H(d.H_adj(z.reshape(rhs.shape[1:]).unsqueeze(0))) + 0.2 ** 2 * z.reshape(rhs.shape[1:]).unsqueeze(0)).reshape(-1)
            sol = O.gmres(avp, rhs[b].reshape(-1), max_iter=max_iter).reshape(rhs.shape[1:])
            np.testing.assert_allclose(sol.numpy(), g[f"sol_{tag}"][b], atol=4 * float(g[f"dist_fp64_{tag}"]))
        sol64, its = Z.krylov_solve64(rhs.numpy(), O.gaussian_1d_taps(*Z.KRYLOV_BLUR), max_iter)
        assert np.abs(its - g[f"iters_{tag}"]).max() <= 1
        assert np.abs(sol64 - g[f"sol_{tag}"]).max() <= 1.01 * float(g[f"dist_fp64_{tag}"])
    assert g["iters_A"].tolist()[2] == 0 and g["iters_A"][0] != g["iters_A"][1] and g["iters_A"].max() < 100
    assert g["iters_B"].tolist() == [5, 5, 0]


@pytest.mark.parametrize("tag,noise_type", [("zero_blur", "gaussian"), ("laplace_zero_blur", "laplace")])
def test_restatement_pnp_flow_matches_reference(golden, tag, noise_type):
    g = golden("pnp_traj_" + tag)
    cfg, sd = tiny4()
    steps, ns, sigma = int(g["steps"]), int(g["num_samples"]), float(g["sigma"])
    its = {}
    O.pnp_flow_restore(lambda a, t: O.unet_forward(sd, cfg, a, t), Z.ZeroBlur(1.0, 61, 3, 64), torch.from_numpy(g["noisy"]), sigma, steps=steps, num_samples=ns,
                       alpha=float(g["alpha"]), noise_fn=lambda it, s, like: det_normal(tuple(like.shape), 41, 1 + it * ns + s),
                       record=lambda it, x: its.__setitem__(it, x.clone()), noise_type=noise_type)
    for it in (0, 1, 4, 9):
        np.testing.assert_allclose(its[it].numpy(), g[f"x_it{it}"], atol=2e-5, err_msg=f"iterate {it}")


def test_restatement_ot_ode_matches_reference(golden):
    g = golden("ot_ode_traj_zero_blur")
    cfg, sd = tiny4()
    steps, t0, sigma = int(g["steps"]), float(g["start_time"]), float(g["sigma"])
    assert g["gmres_vectors"].shape == (steps - int(g["first"]), 2) and 0 < g["gmres_vectors"].min() and g["gmres_vectors"].max() < 100
    its = {}
    O.ot_ode_restore(lambda a, t: O.unet_forward(sd, cfg, a, t), lambda x, t, v: O.unet_vjp(sd, cfg, x, t, v), Z.ZeroBlur(1.0, 61, 3, 64), "gaussian_deblurring",
                     torch.from_numpy(g["noisy"]), sigma, steps=steps, start_time=t0, gamma="constant", init_noise=det_normal((2, 3, 64, 64), 61, 1),
                     record=lambda it, x: its.__setitem__(it, x.clone()))
    first = int(g["first"])
    for it in (first, first + 1, steps - 1):
        ref = g[f"x_it{it}"]
        np.testing.assert_allclose(its[it].numpy(), ref, atol=1e-4 * max(1.0, float(np.abs(ref).max())), err_msg=f"iterate {it}")


def test_python_surface():
    import main as M
    import pnpflow_amd._lib as L
    import pnpflow_amd.degradations as D
    for dim, sig in ((128, 1.0), (256, 3.0)):
        for noise, sn in (("gaussian", 0.05), ("laplace", 0.3)):
            d, s = M.make_degradation("gaussian_deblurring", dim, 3, noise, "cpu")
            assert type(d).__name__ == "GaussianDeblurring" and d.kind == L.PF_DEG_GAUSSIAN_BLUR_ZERO == 6
            assert (d.sigma, d.kernel_size, d.mode, s) == (sig, 61, "spatial", sn)
    d, _ = M.make_degradation("gaussian_deblurring_FFT", 128, 3, "gaussian", "cpu")
    assert d.kind == L.PF_DEG_GAUSSIAN_BLUR == 4
    with pytest.raises(ValueError):
        M.make_degradation("nope", 128, 3, "gaussian", "cpu")
    with pytest.raises(ValueError, match="odd"):
        D.GaussianDeblurring(1.0, 60, "spatial")
    D.GaussianDeblurring(1.0, 60, "fft")                       # the circular mode keeps accepting what it accepted
    a, b = D.GaussianDeblurring(1.0, 61, "spatial"), D.GaussianDeblurring(1.0, 61, "fft")
    assert np.array_equal(a.taps_eff, b.taps_eff) and len(a.taps_eff) == 15      # the same visible-tap truncation
    assert len(D.GaussianDeblurring(3.0, 61, "anything-but-fft").taps_eff) == 43


def test_abi_declares_the_kind_and_the_krylov_entry_points():
    import pnpflow_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "pnpflow_hip.h")).read()
    assert re.search(r"PF_DEG_GAUSSIAN_BLUR_ZERO\s*=\s*6\b", hdr) and re.search(r"#define\s+PF_ABI_VERSION\s+6\b", hdr)
    assert L.PF_ABI_VERSION == 6 and L.PF_DEG_GAUSSIAN_BLUR_ZERO == 6
    for name in ("pf_krylov_workspace_floats", "pf_krylov_solve", "pf_ot_ode_krylov_iterations"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in L.SIGNATURES
    lib = L.load()
    assert lib.pf_abi_version() == 6
    # the workspace is the basis + two operator temporaries + the small per-image state
    B, Cc, H, W, m = 3, 3, 20, 24, 100
    n = lib.pf_krylov_workspace_floats(B, Cc, H, W, m)
    assert (m + 3) * B * Cc * H * W <= n <= (m + 3) * B * Cc * H * W + 2 * B * (m * m + 8 * m + 16) + 64
    assert lib.pf_krylov_workspace_floats(0, Cc, H, W, m) == 0
