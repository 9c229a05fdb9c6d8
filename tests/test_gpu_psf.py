"""Blur with any 2-D point-spread function (PF_DEG_PSF_BLUR = 7 circular, PF_DEG_PSF_BLUR_ZERO = 8 zero boundary) through the C ABI and on every solver.
Needs a real MI355X:  python -m pytest tests/test_gpu_psf.py -m gpu

References: the fp64 direct sums and restatements of tests/psf_restatement.py and the real reference's fixtures of tools/make_golden_psf.py.

Every instantiation and launcher branch of csrc/psf.hip and of the spectrum / Fourier-solve additions of csrc/fft2.hip, and the case that takes it:

  psf2d_kernel<32, false> (kind 7) / psf2d_kernel<32, true> (kind 8), flip = 0 / 1 (H and H_adj of each kind), mode 0: the operator table
      (B, C, H, W) x K:  (2, 3, 20, 24), (1, 1, 8, 8), (2, 2, 37, 70), (2, 3, 64, 64), (1, 2, 70, 37)  x  1, 3, 9, 17, 31, 63 (kind 7: K <= min(H, W)
      only), and (2, 2, 37, 70) x 37 for kind 7: K == min(H, W)
      a tile is 32 columns x 64 rows.  ragged tiles on both axes: 20 x 24, 37 x 70, 70 x 37;   more than one tile along x: 37 x 70, 64 x 64;   along y:
      70 x 37;   a single partial tile: 8 x 8
      the staged neighbourhood wraps several times (TS + r >= 2 min(H, W), the true-modulo staging): every kind-7 case at 8 x 8 and 20 x 24
      kernel radius beyond the image (only zeros staged on one side): kind 8, K = 17, 31, 63 at 8 x 8 and K = 63 at 20 x 24
      sparse PSF with the four corner taps: K = 63
  modes 1, 3, 2 (epilogues of pf_grad_step / pf_grad_step_laplace): the gradient-step cases
  launch_psf2d's refusals (even K, K > 63, NULL taps, K > min(H, W) for kind 7, in == out): test_refusals_launch_nothing
  psf_power_spectrum_kernel and fft_cols_solve_kernel's table branch, with radix-2 / DFT line kernels, (H, W): (32, 24) radix-2 columns / DFT rows,
      (24, 32) DFT / radix-2, (20, 28) DFT / DFT, (64, 32) radix-2 / radix-2
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import CFGS, det_image, det_normal
from oracle import pnpflow_oracle as O
import psf_restatement as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAJ_ATOL = 1e-4          # tests/test_gpu_parity.py
INVALID = -1              # PF_ERR_INVALID
SHAPES = [(2, 3, 20, 24), (1, 1, 8, 8), (2, 2, 37, 70), (2, 3, 64, 64), (1, 2, 70, 37)]
SIDES = [1, 3, 9, 17, 31, 63]
COEF = np.array([0.7, 0.25], dtype=np.float32)


@pytest.fixture(scope="module")
def hip():
    import pnpflow_amd._lib as L
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    L.load()
    return L


_MODELS = {}


def model_for(name="tiny4"):
    from pnpflow_amd.models import UNet
    if name not in _MODELS:
        c = CFGS[name]
        cfg = O.unet_config(**c)
        sd = O.synthetic_state_dict(cfg, 0)
        m = UNet(c["input_channels"], c["input_height"], c["ch"], ch_mult=c["ch_mult"], num_res_blocks=c["num_res_blocks"], attn_resolutions=c["attn_resolutions"])
        m.load_state_dict(sd)
        _MODELS[name] = (m, cfg, sd)
    return _MODELS[name]


def engine_op(k, mode, S=64):
    import pnpflow_amd.degradations as D
    return D.PSFDeblurring(k, "fft" if mode == "fft" else "spatial", 3, S)


# ---------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------
def descriptor(L, kind, k):
    t = torch.from_numpy(np.ascontiguousarray(k, dtype=np.float32)).cuda()
    d = L.PfDegradation(); d.kind = kind; d.ntaps = int(k.shape[0]); d.taps = t.data_ptr()
    return d, t


def run_op(L, kind, shape, k, what, a, y=None, coef=None, want_scratch=False):
    """one ABI call -> (status, output[, scratch]); H / H_adj get no scratch at all (the PSF kinds need none)"""
    lib = L.load()
    B, Cc, H, W = shape
    d, keep = descriptor(L, kind, k)
    out = torch.full(shape, float("nan"), device="cuda")
    st = L.current_stream_ptr()
    ad = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    scr = None
    if what == "H":
        rc = lib.pf_degradation_H(C.byref(d), ad.data_ptr(), out.data_ptr(), B, Cc, H, W, None, st)
    elif what == "H_adj":
        rc = lib.pf_degradation_H_adj(C.byref(d), ad.data_ptr(), out.data_ptr(), B, Cc, H, W, None, st)
    else:
        scr = torch.full((int(np.prod(shape)),), float("nan"), device="cuda")        # B*C*H*W floats: the residual
        yd, cd = torch.from_numpy(y).cuda(), torch.from_numpy(coef).cuda()
        fn = lib.pf_grad_step if what == "grad" else lib.pf_grad_step_laplace
        rc = fn(C.byref(d), ad.data_ptr(), yd.data_ptr(), cd.data_ptr(), out.data_ptr(), B, Cc, H, W, scr.data_ptr(), st)
    torch.cuda.synchronize()
    if want_scratch:
        return rc, out.cpu().numpy(), scr.cpu().numpy().reshape(shape)
    return rc, out.cpu().numpy()


def table():
    cases = []
    for kind in (7, 8):
        for si, shape in enumerate(SHAPES):
            for K in SIDES + ([37] if (kind == 7 and shape == (2, 2, 37, 70)) else []):
                if kind == 7 and K > min(shape[2:]):
                    continue
                cases.append((kind, si, K))
    return cases


_DATA = {}


def op_data(si):
    if si not in _DATA:
        _DATA[si] = tuple(det_normal(SHAPES[si], 8100 + si, i).numpy() for i in range(3))
    return _DATA[si]


# ---------------------------------------------------------------------------------------------
# operator: fp64 direct sums, adjoint identity, run-to-run
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,si,K", table())
def test_operator_matches_fp64_direct_sums(hip, kind, si, K):
    """Tolerance, derived: the forward error bound of an fp32 multiply-add chain over the nnz non-zero taps, (nnz + 2) 2^-24 S, S = the largest
    sum |g| |x| over the outputs (psf_restatement.chain_bound).  Then <H x, w> = <x, H_adj w> on the kernels' own outputs within 2e-4 of the
    product (the criterion of tests/test_gpu_zero_blur.py::test_adjoint_identity_on_the_kernels_outputs), and a second call returns the same bits."""
    shape, zero = SHAPES[si], kind == 8
    k = P.psf_kernel(K)
    if K == 63:
        assert 36 <= np.count_nonzero(k) <= 40 and k[0, 0] and k[0, -1] and k[-1, 0] and k[-1, -1]
    x, w, _ = op_data(si)
    got = {}
    for what, a, adj in (("H", x, False), ("H_adj", w, True)):
        rc, out = run_op(hip, kind, shape, k, what, a)
        assert rc == 0, (what, rc)
        ref, tol = P.apply64(a, k, zero, adj), P.chain_bound(a, k, zero, adj)
        err = float(np.abs(out.astype(np.float64) - ref).max())
        print(f"psf kind {kind} {shape} K {K} {what}: max|hip - fp64| = {err:.3e} (bound {tol:.3e})")
        assert np.isfinite(out).all() and err <= tol, (what, err, tol)
        rc2, out2 = run_op(hip, kind, shape, k, what, a)
        assert rc2 == 0 and np.array_equal(out, out2), f"{what}: two calls differ"
        got[what] = out.astype(np.float64)
    lhs, rhs = float((got["H"] * w).sum()), float((x.astype(np.float64) * got["H_adj"]).sum())
    assert abs(lhs - rhs) <= 2e-4 * float(np.abs(got["H"] * w).sum()), (lhs, rhs)


@pytest.mark.parametrize("kind", [7, 8])
@pytest.mark.parametrize("shape,K,ty,tx", [((2, 2, 37, 70), 9, 1, 7), ((1, 1, 8, 8), 5, 4, 0), ((2, 3, 20, 24), 17, 16, 3), ((1, 2, 70, 37), 9, 8, 2)])
def test_orientation_is_exact(hip, kind, shape, K, ty, tx):
    """A single off-centre unit tap reproduces the shifted image bit for bit: np.roll for the circular kind, a zero-filled shift for the other; H and
    H_adj shift in opposite directions, and the two kinds' H shift in opposite directions (convolution against correlation)."""
    x = det_normal(shape, 8200, K).numpy()
    k, r = P.unit_tap(K, ty, tx), K // 2
    dy, dx = ty - r, tx - r
    assert (dy, dx) != (0, 0)
    sy, sx = (dy, dx) if kind == 7 else (-dy, -dx)           # kind 7: H x [i] = x[i - (j - r)]
    rc, h = run_op(hip, kind, shape, k, "H", x)
    rc2, ha = run_op(hip, kind, shape, k, "H_adj", x)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(h, P.shift_exact(x, sy, sx, zero=kind == 8))
    assert np.array_equal(ha, P.shift_exact(x, -sy, -sx, zero=kind == 8))
    assert not np.array_equal(h, ha)


def test_separable_kernel_agrees_with_the_gaussian_kind(hip):
    """Kind 7 with outer(g, g) of the sigma-3 Gaussian's 43 visible taps against kind 4 on the same input, within the sum of the two bounds: the
    PSF chain's (43^2 + 2) 2^-24 S, and for the two 43-tap passes of the separable kind plus the rounding of outer(g, g) to fp32 (2 x 43 + 4) 2^-24 S."""
    import pnpflow_amd.degradations as D
    lib = hip.load()
    g = np.ascontiguousarray(D.GaussianDeblurring(3.0, 61, "fft").taps_eff, dtype=np.float32)
    assert len(g) == 43
    shape = (2, 3, 64, 64)
    x = det_normal(shape, 8300).numpy()
    k = np.outer(g, g).astype(np.float32)
    S = float(P.apply64(x, k, zero=False, absolute=True).max())
    bound = (43 * 43 + 2 + 2 * 43 + 4) * 2.0 ** -24 * S
    for what in ("H", "H_adj"):
        rc, psf = run_op(hip, 7, shape, k, what, x)
        assert rc == 0
        t = torch.from_numpy(g).cuda()
        d = hip.PfDegradation(); d.kind = hip.PF_DEG_GAUSSIAN_BLUR; d.ntaps = 43; d.taps = t.data_ptr()
        xd, out, scr = torch.from_numpy(x).cuda(), torch.full(shape, float("nan"), device="cuda"), torch.empty(int(np.prod(shape)), device="cuda")
        fn = lib.pf_degradation_H if what == "H" else lib.pf_degradation_H_adj
        assert fn(C.byref(d), xd.data_ptr(), out.data_ptr(), *shape, scr.data_ptr(), hip.current_stream_ptr()) == 0
        torch.cuda.synchronize()
        err = float(np.abs(psf.astype(np.float64) - out.cpu().numpy()).max())
        print(f"separable cross-check {what}: max|psf - gaussian| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound


@pytest.mark.parametrize("kind", [7, 8])
def test_refusals_launch_nothing(hip, kind):
    """PF_ERR_INVALID with the output untouched: an even side, a side above 63, NULL taps, in == out, and for the circular kind a kernel larger
    than the image (the zero-boundary kind has no size rule)"""
    lib = hip.load()
    shape = (1, 1, 8, 8)
    x = det_normal(shape, 8400).numpy()
    for K in (4, 65):
        rc, out = run_op(hip, kind, (1, 1, 80, 80), np.ones((K, K), dtype=np.float32), "H", det_normal((1, 1, 80, 80), 8401).numpy())
        assert rc == INVALID and np.isnan(out).all(), K
    rc, out = run_op(hip, kind, shape, P.psf_kernel(9), "H", x)
    assert (rc == INVALID and np.isnan(out).all()) if kind == 7 else rc == 0
    rc, out, _ = run_op(hip, kind, shape, P.psf_kernel(9), "grad", x, y=x, coef=COEF[:1], want_scratch=True)
    assert (rc == INVALID and np.isnan(out).all()) if kind == 7 else rc == 0
    d = hip.PfDegradation(); d.kind = kind; d.ntaps = 3; d.taps = None
    xd, out = torch.from_numpy(x).cuda(), torch.full(shape, float("nan"), device="cuda")
    assert lib.pf_degradation_H(C.byref(d), xd.data_ptr(), out.data_ptr(), *shape, None, hip.current_stream_ptr()) == INVALID
    d, keep = descriptor(hip, kind, P.psf_kernel(3))
    before = xd.clone()
    assert lib.pf_degradation_H(C.byref(d), xd.data_ptr(), xd.data_ptr(), *shape, None, hip.current_stream_ptr()) == INVALID      # in == out
    assert lib.pf_degradation_H_adj(C.byref(d), xd.data_ptr(), xd.data_ptr(), *shape, None, hip.current_stream_ptr()) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(xd, before) and torch.isnan(out).all()


# ---------------------------------------------------------------------------------------------
# gradient steps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("laplace", [False, True])
@pytest.mark.parametrize("kind,si,K", [(7, 0, 9), (8, 0, 31), (7, 2, 17), (8, 2, 9), (7, 3, 63), (8, 1, 17), (7, 4, 31), (8, 4, 9)])
def test_gradient_steps_match_the_composed_operators(hip, kind, si, K, laplace):
    """pf_grad_step / pf_grad_step_laplace against the same step composed in numpy fp32 from the engine's own H and H_adj outputs, per-image
    coefficients (0.7, 0.25).  The residual the first application leaves in the scratch - H x - y, or its sign in {-1, +1} - is one fp32
    subtraction (or comparison) of the same chain: exact.  The update x - coef H_adj(r) is at most one contracted multiply-subtract away from the
    two-rounding numpy form: elementwise 2^-23 (|x| + |coef v|)."""
    shape = SHAPES[si]
    k = P.psf_kernel(K)
    x, _, y = op_data(si)
    coef = COEF[:shape[0]]
    rc, hx = run_op(hip, kind, shape, k, "H", x)
    assert rc == 0
    hadj = lambda r: run_op(hip, kind, shape, k, "H_adj", r)[1]
    r, v, z = P.grad_step32(x, y, coef, hx, hadj, laplace)
    rc, got, scr = run_op(hip, kind, shape, k, "laplace" if laplace else "grad", x, y=y, coef=coef, want_scratch=True)
    assert rc == 0
    assert np.array_equal(scr, r), "the residual (or its sign) is not exact"
    if laplace:
        assert set(np.unique(scr)) <= {-1.0, 1.0}
    bound = 2.0 ** -23 * (np.abs(x.astype(np.float64)) + np.abs(coef.astype(np.float64).reshape(-1, 1, 1, 1) * v))
    err = np.abs(got.astype(np.float64) - z)
    print(f"psf grad step kind {kind} {shape} K {K} laplace {laplace}: max err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert float(np.abs(got - x).max()) > 1e-3               # the step moved the image


# ---------------------------------------------------------------------------------------------
# spectrum and Fourier solve
# ---------------------------------------------------------------------------------------------
FOURIER = [((32, 24), 15), ((24, 32), 9), ((20, 28), 17), ((64, 32), 31)]


@pytest.mark.parametrize("hw,K", FOURIER)
def test_power_spectrum_matches_fp64(hip, hw, K):
    """|fft2(filter)|^2 against numpy fp64: 2^-23 max P absolute (the value is computed in fp64 and rounded once to fp32: 2^-24 max P, doubled for
    the fp64 twiddles' own error, which is far below it)"""
    lib = hip.load()
    H, W = hw
    k = P.psf_kernel(K)
    d, keep = descriptor(hip, 7, k)
    out = torch.full((H, W), float("nan"), device="cuda")
    assert lib.pf_psf_power_spectrum(C.byref(d), H, W, out.data_ptr(), hip.current_stream_ptr()) == 0
    torch.cuda.synchronize()
    ref = P.power_spectrum64(k, H, W)
    err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
    print(f"psf spectrum {hw} K {K}: max err {err:.3e} (bound {2.0 ** -23 * ref.max():.3e})")
    assert err <= 2.0 ** -23 * float(ref.max())
    d.kind = 8
    assert lib.pf_psf_power_spectrum(C.byref(d), H, W, out.data_ptr(), hip.current_stream_ptr()) == INVALID      # the circular kind's alone


@pytest.mark.parametrize("hw,K", FOURIER)
def test_ot_ode_vec_fourier_solve_matches_fp64(hip, hw, K):
    """pf_ot_ode_vec with the circular PSF against fp64: the project's Fourier-solve bound, 5e-5 max|ref| (tests/test_gpu_operator_paths.py); the
    zero-boundary kind is refused there, as PF_DEG_GAUSSIAN_BLUR_ZERO is"""
    lib = hip.load()
    H, W = hw
    shape = (2, 2 if hw != (20, 28) else 1, H, W)
    B, Cc = shape[:2]
    k = P.psf_kernel(K)
    x, vt, w = (det_normal(shape, 8500 + K, i).numpy() for i in range(3))
    y = (P.apply64(w, k, zero=False) + 0.05 * det_normal(shape, 8500 + K, 3).numpy()).astype(np.float32)
    omt, rt2, sigma2 = np.array([0.6, 0.3], dtype=np.float32), np.array([0.55, 0.2], dtype=np.float32), 0.05 ** 2
    ref = P.ot_ode_vec64(k, x, vt, y, omt, rt2, np.float32(sigma2))
    S = int(np.prod(shape))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    xd, vd, yd, od, rd = dev(x), dev(vt), dev(y), dev(omt), dev(rt2)
    for kind in (7, 8, hip.PF_DEG_GAUSSIAN_BLUR_ZERO):
        d, keep = descriptor(hip, kind, k)
        if kind == hip.PF_DEG_GAUSSIAN_BLUR_ZERO:
            d, keep = descriptor(hip, kind, k[0:1].T.copy())           # 1-D taps for the Gaussian kind
            d.ntaps = K
        out = torch.full(shape, float("nan"), device="cuda")
        scr = torch.full((4 * S + H * W,), float("nan"), device="cuda")
        rc = lib.pf_ot_ode_vec(C.byref(d), xd.data_ptr(), vd.data_ptr(), yd.data_ptr(), od.data_ptr(), rd.data_ptr(), float(sigma2), out.data_ptr(), B, Cc, H, W,
                               scr.data_ptr(), hip.current_stream_ptr())
        torch.cuda.synchronize()
        if kind != 7:
            assert rc == INVALID and torch.isnan(out).all(), kind
            continue
        assert rc == 0
        err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
        print(f"psf Fourier solve {shape} K {K}: max|hip - fp64| = {err:.3e} (bound {5e-5 * np.abs(ref).max():.3e})")
        assert err <= 5e-5 * float(np.abs(ref).max())


# ---------------------------------------------------------------------------------------------
# the Python operator against the reference's fixture
# ---------------------------------------------------------------------------------------------
def test_python_operator_matches_reference_golden(hip, golden):
    g = golden("psf_op")
    x = det_image((2, 3, 64, 64), 31)[:1]
    for K in (9, 21):
        for mode in ("fft", "zero"):
            d = engine_op(g[f"psf{K}"], mode)
            assert d.kind == (7 if mode == "fft" else 8)
            np.testing.assert_allclose(d.H(x.cuda()).cpu().numpy(), g[f"k{K}_{mode}_H"], rtol=0, atol=1e-5)
            np.testing.assert_allclose(d.H_adj(x.cuda()).cpu().numpy(), g[f"k{K}_{mode}_Hadj"], rtol=0, atol=1e-5)


# ---------------------------------------------------------------------------------------------
# PnP-Flow
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,mode,noise_type", [("psf_fft", "fft", "gaussian"), ("laplace_psf_zero", "zero", "laplace")])
def test_pnp_flow_matches_reference(hip, golden, tag, mode, noise_type):
    from pnpflow_amd.methods.pnp_flow import PNP_FLOW
    from pnpflow_amd.utils import CfgNode
    g = golden("pnp_traj_" + tag)
    m, cfg, sd = model_for("tiny4")
    sigma, steps, ns = float(g["sigma"]), int(g["steps"]), int(g["num_samples"])
    problem = "psf_deblurring_FFT" if mode == "fft" else "psf_deblurring"
    args = CfgNode(dict(method="pnp_flow", model="ot", problem=problem, noise_type=noise_type, num_samples=ns, steps_pnp=steps, lr_pnp=1.0,
                        gamma_style="alpha_1_minus_t", alpha=float(g["alpha"]), max_batch=1, compute_time=False, compute_memory=False, save_results=False,
                        batch=0, sigma_noise=sigma))
    solver = PNP_FLOW(m, torch.device("cuda"), args)
    solver.noise = torch.stack([det_normal((2, 3, 64, 64), 41, 1 + i) for i in range(steps * ns)]).cuda()
    its = {}
    solver.restore_batch(torch.from_numpy(g["noisy"]).cuda(), engine_op(g["psf"], mode), sigma, lr=sigma ** 2 if noise_type == "gaussian" else sigma * 1.0,
                         iter_cb=lambda it, xx: its.__setitem__(it, xx.clone().cpu()))
    for it in (0, 1, 4, 9):
        print(f"pnp_flow {tag} iterate {it}: max|hip - reference| = {float(np.abs(its[it].numpy() - g[f'x_it{it}']).max()):.3e}")
    for it in (0, 1, 4, 9):
        np.testing.assert_allclose(its[it].numpy(), g[f"x_it{it}"], atol=TRAJ_ATOL, err_msg=f"iterate {it}")


# ---------------------------------------------------------------------------------------------
# OT-ODE: the engine loop, Fourier solve (circular) and Krylov halves (zero boundary)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,mode", [("psf_fft", "fft"), ("psf_zero", "zero")])
def test_ot_ode_engine_loop_matches_reference(hip, golden, monkeypatch, tag, mode):
    from pnpflow_amd.methods.ot_ode import OT_ODE
    from pnpflow_amd.utils import CfgNode, psnr_per_image
    g = golden("ot_ode_traj_" + tag)
    m, cfg, sd = model_for("tiny4")
    S, steps, t0, sigma, first = cfg["input_height"], int(g["steps"]), float(g["start_time"]), float(g["sigma"]), int(g["first"])
    args = CfgNode(dict(method="ot_ode", model="ot", problem="psf_deblurring_FFT" if mode == "fft" else "psf_deblurring", steps_ode=steps, start_time=t0,
                        gamma="constant", max_batch=1, compute_time=False, compute_memory=False, save_results=False, batch=0))
    solver = OT_ODE(m, torch.device("cuda"), args)

    def no_host_loop(*a, **k):
        raise AssertionError("the host GMRES loop ran")
    monkeypatch.setattr(solver, "_restore_batch_generic", no_host_loop)
    solver.init_noise = det_normal((2, 3, S, S), 61, 1).cuda()
    its = {}
    x = solver.restore_batch(torch.from_numpy(g["noisy"]).cuda(), engine_op(g["psf"], mode), sigma, iter_cb=lambda it, xx: its.__setitem__(it, xx.clone().cpu()))
    if mode == "zero":
        # Krylov vectors: every solve of the reference stopped below the cap; the engine's per-step count is its slowest image's, within one of the
        # fixture's, rounded up to the next poll of the done flags (every 8 iterations)
        vec = g["gmres_vectors"]
        assert int(vec.max()) < 100
        lo, hi = int((vec.max(axis=1) - 1).sum()), int(((vec.max(axis=1) + 1 + 7) // 8 * 8).sum())
        print(f"ot_ode psf zero: {solver.last_krylov_iterations} Krylov iterations enqueued (fixture's slowest image per step: {vec.max(axis=1).tolist()})")
        assert lo <= solver.last_krylov_iterations <= hi, (lo, solver.last_krylov_iterations, hi)
    else:
        assert solver.last_krylov_iterations == 0
    for it in (first, first + 1):
        ref = g[f"x_it{it}"]
        print(f"ot_ode {tag} iterate {it}: max|hip - reference| / max|ref| = {float(np.abs(its[it].numpy() - ref).max() / np.abs(ref).max()):.3e}")
        np.testing.assert_allclose(its[it].numpy(), ref, atol=1e-3 * float(np.abs(ref).max()), err_msg=f"iterate {it}")
    clean = det_image((2, 3, S, S), 31)
    p_hip = psnr_per_image(x, clean.cuda()).cpu()
    p_ref = O.psnr_per_image(torch.from_numpy(g[f"x_it{steps - 1}"]), clean)
    assert float((p_hip - p_ref).abs().max()) <= 0.05, (p_hip, p_ref)


# ---------------------------------------------------------------------------------------------
# Prox-PnP
# ---------------------------------------------------------------------------------------------
def gs_solver(m, **kw):
    from pnpflow_amd.methods.pnp_gs import PROX_PNP
    from pnpflow_amd.train_denoiser import GRADIENT_STEP_DENOISER
    from pnpflow_amd.utils import CfgNode
    a = dict(method="pnp_gs", model="gradient_step", problem="psf_deblurring_FFT", noise_type="gaussian", algo="hqs", max_iter=3, lr_pnp=1.0, alpha=0.5,
             sigma_factor=1.0, max_batch=1, compute_time=False, compute_memory=False, save_results=False, batch=0, dim_image=m.input_height,
             num_channels=m.input_channels)
    a.update(kw)
    args = CfgNode(a)
    return PROX_PNP(GRADIENT_STEP_DENOISER(m, torch.device("cuda"), args), torch.device("cuda"), args)


def GS_TOL(jn_max):
    return 2e-5 + 2 * 5e-5 * float(jn_max)            # TOL of tests/test_gpu_pnp_gs.py


def test_pnp_gs_hqs_matches_reference_golden(hip, golden):
    """teacher-forced single iterations at TOL, then free-running from the initialisation at TOL growth^(k-1) (tests/test_gpu_pnp_gs.py)"""
    g = golden("pnp_gs_tiny4_hqs_psf_fft")
    m, _, _ = model_for("tiny4")
    dg = engine_op(g["psf"], "fft")
    sigma, growth = float(g["sigma"]), float(g["growth"])
    noisy = torch.from_numpy(g["noisy"]).cuda()
    s = gs_solver(m)
    for k in range(3):
        x = s.restore_batch(noisy, dg, sigma, first=k, stop=k + 1, x0=torch.from_numpy(g["iterates"][k]).cuda(), alpha=float(g["alpha"][k]))
        err = float(np.abs(x.cpu().numpy() - g["iterates"][k + 1]).max())
        print(f"pnp_gs hqs psf teacher-forced {k}: err / TOL = {err / GS_TOL(g['jn_max'][k]):.4f}")
        assert s.last_alpha == float(g["alpha"][k + 1]), (s.last_alpha, g["alpha"])
        np.testing.assert_allclose(s.last_gap_log[k], g["gap"][k], rtol=1e-2)
        np.testing.assert_allclose(x.cpu().numpy(), g["iterates"][k + 1], atol=GS_TOL(g["jn_max"][k]))
    bound = lambda k: max(GS_TOL(j) for j in g["jn_max"][:k]) * growth ** (k - 1)
    for k in (1, 2, 3):
        x = s.restore_batch(noisy, dg, sigma, first=0, stop=k, lr=sigma ** 2, alpha=0.5)
        err = float(np.abs(x.cpu().numpy() - g["iterates"][k]).max())
        print(f"pnp_gs hqs psf free-running after iteration {k}: err / bound = {err / bound(k):.4f}")
        assert s.last_alpha == float(g["alpha"][k])
        np.testing.assert_allclose(x.cpu().numpy(), g["iterates"][k], atol=bound(k), err_msg=f"after iteration {k}")


def test_pnp_gs_pgd_iteration_matches_restatement_and_hqs_zero_is_refused(hip):
    import pnp_gs_restatement as R
    m, cfg, sd = model_for("tiny4")
    k = P.psf_kernel(9)
    do = P.PsfBlur(k, "zero", 3, 64)
    sigma, shape = 0.05, (2, 3, 64, 64)
    noisy = do.H(det_image(shape, 93)) + sigma * det_normal(shape, 94)
    kw = dict(algo="pgd", problem="gaussian_deblurring", max_iter=2, sigma_noise=sigma)
    xs, alphas, infos = R.solve(lambda x, s: O.unet_forward(sd, cfg, x, s), do, noisy, alpha=0.5, stop=1, **kw)
    s = gs_solver(m, algo="pgd", problem="psf_deblurring", max_iter=2)
    x = s.restore_batch(noisy.cuda(), engine_op(k, "zero"), sigma, first=0, stop=1, x0=xs[0].cuda(), alpha=alphas[0])
    np.testing.assert_allclose(x.cpu().numpy(), xs[1].numpy(), atol=GS_TOL(infos[0]["JN"].abs().max()))
    # hqs: the prox is a Fourier solve of the circular operator - refused by the solver (naming pgd) and by the engine
    with pytest.raises(ValueError, match="pgd"):
        gs_solver(m, algo="hqs", problem="psf_deblurring").restore_batch(noisy.cuda(), engine_op(k, "zero"), sigma)
    with pytest.raises(hip.PnpFlowHipError, match="(?i)circular"):
        gs_solver(m, algo="hqs", problem="psf_deblurring_FFT").restore_batch(noisy.cuda(), engine_op(k, "zero"), sigma)


# ---------------------------------------------------------------------------------------------
# D-Flow, Flow-Priors: one evaluation each against the solver's own restatement, both kinds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fft", "zero"])
def test_d_flow_value_and_grad_matches_restatement(hip, mode):
    import dflow_restatement as R
    from pnpflow_amd.methods.d_flow import D_FLOW
    from pnpflow_amd.utils import CfgNode
    LOSS_RTOL, GRAD_RTOL = 1e-5, 2e-4        # tests/test_gpu_d_flow.py
    m, cfg, sd = model_for("tiny4")
    k = P.psf_kernel(9)
    do = P.PsfBlur(k, mode, 3, 64)
    z = det_normal((2, 3, 64, 64), 82)
    y = do.H(det_image((2, 3, 64, 64), 83)) + 0.05 * det_normal((2, 3, 64, 64), 84)
    per, gref = R.value_and_grad(z, y, do.H, lambda x, t: O.unet_forward(sd, cfg, x, t), 0.001)
    s = D_FLOW(m, torch.device("cuda"), CfgNode(dict(method="d_flow", model="ot", problem="psf_deblurring", steps_euler=6, lmbda=0.001, alpha=0.1, max_iter=1,
                                                    LBFGS_iter=3, start_time=0.0, max_batch=1, compute_time=False, compute_memory=False, save_results=False, batch=0)))
    loss, grad = s.value_and_grad(z.cuda(), y.cuda(), engine_op(k, mode), 0.001)
    np.testing.assert_allclose(loss.cpu().numpy(), per.numpy(), rtol=LOSS_RTOL)
    np.testing.assert_allclose(grad.cpu().numpy(), gref.numpy(), atol=GRAD_RTOL * float(gref.abs().max()))


@pytest.mark.parametrize("mode", ["fft", "zero"])
def test_flow_priors_data_gradient_matches_fp64_restatement(hip, mode):
    """TOL_data = 2 lmbda dt 2e-5 max|pred| + dt (2e-5 + 5e-5 max|J^T w|) (tests/test_gpu_flow_priors.py)"""
    import flow_priors_restatement as R
    from pnpflow_amd.methods.flow_priors import FLOW_PRIORS
    from pnpflow_amd.utils import CfgNode
    m, cfg, sd = model_for("tiny4")
    it, sigma, seed = 60, 0.05, 16
    _, _, _, inp = R.case_inputs(("denoising", "gaussian", it, sigma, seed))
    k = P.psf_kernel(9)
    do = P.PsfBlur(k, mode, 3, 64)
    y = (do.H(inp["clean"]) + sigma * R.det_normal((2, 3, 64, 64), seed, 3)).float()
    f64 = lambda t: t.double()
    vel = R.oracle_vel(sd, cfg, torch.float64)
    _, g_data, _, _, pred, info = R.grad(vel, do.H, f64(inp["x"]), f64(inp["x_init"]), f64(y), f64(inp["eps"]), it, R.N_STEP, R.LMBDA, "gaussian", zero_trace=True)
    dt = 1.0 / R.N_STEP
    w = 2 * R.LMBDA * do.H_adj(info["r"])
    jtw_max = float(((g_data - w) / dt).abs().max())
    tol = 2 * R.LMBDA * dt * 2e-5 * float(pred.abs().max()) + dt * (2e-5 + 5e-5 * jtw_max)
    s = FLOW_PRIORS(m, torch.device("cuda"), CfgNode(dict(method="flow_priors", model="ot", problem="psf_deblurring", noise_type="gaussian", N=R.N_STEP, K=1,
                                                         lmbda=R.LMBDA, eta=R.ETA, start_time=0.0, max_batch=1, compute_time=False, compute_memory=False,
                                                         save_results=False, batch=0)))
    _, eg_data, _, epred = s.gradient(inp["x"].cuda(), inp["x_init"].cuda(), y.cuda(), engine_op(k, mode), inp["eps"].cuda(), it)
    err = float((eg_data.cpu().double() - g_data).abs().max())
    print(f"flow_priors psf {mode}: g_data err {err:.3e} (TOL {tol:.3e}, max {float(g_data.abs().max()):.3e})")
    assert float(g_data.abs().max()) > 20 * tol
    assert err <= tol


# ---------------------------------------------------------------------------------------------
# main.py
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,problem,extra", [("pnp_flow", "psf_deblurring_FFT", ("steps_pnp", "10", "num_samples", "2")),
                                                  ("ot_ode", "psf_deblurring", ("steps_ode", "10", "start_time", "0.5", "psf", "disk", "psf_size", "9"))])
def test_main_end_to_end(hip, tmp_path, method, problem, extra):
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--opts", "dataset", "celeba", "problem", problem, "method", method, "synthetic", "True",
           "max_batch", "1", "batch_size_ip", "2", *extra, "output_root", str(tmp_path) + "/"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    base = tmp_path / "results_synthetic" / "celeba" / "ot" / problem / method
    files = [p for p in base.rglob("psnr_rec_batch0.txt")]
    assert files, [str(p) for p in base.rglob("*")]
    vals = [float(l.split()[1]) for l in open(files[0]).read().strip().splitlines()]
    assert vals and all(np.isfinite(v) for v in vals), vals
