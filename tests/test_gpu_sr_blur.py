"""Superresolution through a blur kernel (PF_DEG_PSF_SR = 9: y = (k (*) x) decimated by sf) through the C ABI and on every solver, and the low-resolution
Fourier solve it shares with the bicubic PF_DEG_SR_FILTERED = 5.  Needs a real MI355X:  python -m pytest tests/test_gpu_sr_blur.py -m gpu

References: the fp64 restatements of tests/sr_blur_restatement.py (pinned on the host by tests/test_sr_blur_host.py) and the real reference's fixtures of
tools/make_golden_sr_blur.py.

Shapes (B, C, H, W, sf, K), the smallest at which each branch of csrc/psf.hip / csrc/fft2.hip can go wrong:
  (1, 1,  8,   8, 2,  5)   the image wraps through the staged tile (forward tile: 32 x 4 low-resolution outputs; adjoint tile: 64 x 32 pixels)
  (2, 3, 24,  40, 2,  9)   non-square; the low-resolution grid is 12 x 20: direct-DFT line kernels
  (2, 2, 36,  60, 3,  7)   odd factor, K no multiple of sf: the phases have 3 x 3, 3 x 2, 2 x 2 taps; 9 phases on 4 waves
  (1, 3, 64,  64, 4, 17)   radix-2 FFT at 16
  (1, 2, 64, 128, 4, 63)   largest K, ragged tiles (low-resolution 16 x 32 against 64-row forward tiles, 16 x 32 adjoint grids)
  (2, 1, 20,  24, 1,  9)   sf 1: agrees with PF_DEG_PSF_BLUR
  (1, 1,  6,   6, 2,  3)   (Fourier solve and prox only) 117 floats of scratch precede the complex plane: it is realigned to 8 bytes
  (1, 1, 80, 160, 2,  9)   more than one workgroup along both axes in both kernels (low-resolution 40 x 80: adjoint grids 16 x 32; forward rows 40 of 64, columns 80 of 32)
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
import sr_blur_restatement as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAJ_ATOL = 1e-4          # tests/test_gpu_parity.py
INVALID = -1              # PF_ERR_INVALID
SHAPES = [(1, 1, 8, 8, 2, 5), (2, 3, 24, 40, 2, 9), (2, 2, 36, 60, 3, 7), (1, 3, 64, 64, 4, 17), (1, 2, 64, 128, 4, 63), (2, 1, 20, 24, 1, 9), (1, 1, 80, 160, 2, 9)]
FOURIER = SHAPES[:5]      # the Fourier-solve cases (the sf-1 shape is PF_DEG_PSF_BLUR's own solve on the full grid)
# ... and one where 3 S + Sl floats, the scratch before the complex plane, is an odd count (even sf, odd B C H W / sf^2): the plane is moved to the next 8-byte boundary
SOLVES = FOURIER + [(1, 1, 6, 6, 2, 3)]
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


def engine_op(k, sf, S_=64):
    import pnpflow_amd.degradations as D
    return D.PSFSuperresolution(k, sf, 3, S_)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


# ---------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------
def descriptor(L, k, sf, kind=9):
    t = dev(k)
    d = L.PfDegradation(); d.kind = kind; d.sf = sf; d.ntaps = int(np.asarray(k).shape[0]); d.taps = t.data_ptr()
    return d, t


def run_op(L, shape, sf, k, what, a, y=None, coef=None, want_scratch=False, kind=9, scratch_floats=0):
    """one ABI call -> (status, output[, scratch]).  shape: the full-resolution (B, C, H, W); H / H_adj of kind 9 get no scratch at all"""
    lib = L.load()
    B, Cc, H, W = shape
    low = (B, Cc, H // sf, W // sf) if (H % sf == 0 and W % sf == 0) else (B, Cc, max(H // sf, 1), max(W // sf, 1))
    d, keep = descriptor(L, k, sf, kind)
    out = torch.full(low if what == "H" else shape, float("nan"), device="cuda")
    st = L.current_stream_ptr()
    ad = dev(a)
    scr = torch.full((scratch_floats,), float("nan"), device="cuda") if scratch_floats else None
    sp = scr.data_ptr() if scr is not None else None
    if what == "H":
        rc = lib.pf_degradation_H(C.byref(d), ad.data_ptr(), out.data_ptr(), B, Cc, H, W, sp, st)
    elif what == "H_adj":
        rc = lib.pf_degradation_H_adj(C.byref(d), ad.data_ptr(), out.data_ptr(), B, Cc, H, W, sp, st)
    else:
        scr = torch.full((int(np.prod(low)),), float("nan"), device="cuda")        # B*C*H*W / sf^2 floats: the low-resolution residual
        yd, cd = dev(y), dev(coef)
        fn = lib.pf_grad_step if what == "grad" else lib.pf_grad_step_laplace
        rc = fn(C.byref(d), ad.data_ptr(), yd.data_ptr(), cd.data_ptr(), out.data_ptr(), B, Cc, H, W, scr.data_ptr(), st)
    torch.cuda.synchronize()
    if want_scratch:
        return rc, out.cpu().numpy(), scr.cpu().numpy().reshape(low)
    return rc, out.cpu().numpy()


_DATA = {}


def op_data(si):
    """(x full resolution, w low resolution, y low resolution), computed once per shape"""
    if si not in _DATA:
        B, Cc, H, W, sf, K = SHAPES[si]
        low = (B, Cc, H // sf, W // sf)
        _DATA[si] = (det_normal((B, Cc, H, W), 9400 + si, 0).numpy(), det_normal(low, 9400 + si, 1).numpy(), det_normal(low, 9400 + si, 2).numpy())
    return _DATA[si]


# ---------------------------------------------------------------------------------------------
# 1. operator: fp64 direct sums, adjoint identity, run-to-run
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_operator_matches_fp64_direct_sums(hip, si):
    """Tolerance, derived (tests/test_gpu_psf.py): the forward error bound of an fp32 multiply-add chain over the nnz taps actually summed,
    (nnz + 2) 2^-24 max sum |g| |x| - every non-zero tap for H, the largest phase's count for H_adj.  Then <H x, w> = <x, H_adj w> on the kernels' own
    outputs in fp64 within 2e-4 of the product (tests/test_gpu_psf.py), and a second call returns the same bits."""
    B, Cc, H, W, sf, K = SHAPES[si]
    shape = (B, Cc, H, W)
    k = P.psf_kernel(K)
    x, w, _ = op_data(si)
    got = {}
    for what, a, adj in (("H", x, False), ("H_adj", w, True)):
        rc, out = run_op(hip, shape, sf, k, what, a)
        assert rc == 0, (what, rc)
        ref = S.Hadj64(a, k, sf) if adj else S.H64(a, k, sf)
        tol = S.chain_bound(a, k, sf, adj)
        err = float(np.abs(out.astype(np.float64) - ref).max())
        print(f"sr blur {SHAPES[si]} {what}: max|hip - fp64| = {err:.3e} (bound {tol:.3e})")
        assert out.shape == ref.shape and np.isfinite(out).all() and err <= tol, (what, err, tol)
        rc2, out2 = run_op(hip, shape, sf, k, what, a)
        assert rc2 == 0 and np.array_equal(out, out2), f"{what}: two calls differ"
        got[what] = out.astype(np.float64)
    lhs, rhs = float((got["H"] * w).sum()), float((x.astype(np.float64) * got["H_adj"]).sum())
    assert abs(lhs - rhs) <= 2e-4 * float(np.abs(got["H"] * w).sum()), (lhs, rhs)


def test_sf_1_agrees_with_the_psf_blur_kind(hip):
    """sf 1 against PF_DEG_PSF_BLUR on the same taps, within the sum of the two chains' bounds (both sum the same nnz taps, in another order)"""
    import test_gpu_psf as TP
    B, Cc, H, W, sf, K = SHAPES[5]
    assert sf == 1
    k = P.psf_kernel(K)
    x, w, _ = op_data(5)
    for what, a, adj in (("H", x, False), ("H_adj", w, True)):
        rc, sr = run_op(hip, (B, Cc, H, W), 1, k, what, a)
        rc7, blur = TP.run_op(hip, 7, (B, Cc, H, W), k, what, a)
        assert rc == 0 and rc7 == 0
        bound = S.chain_bound(a, k, 1, adj) + P.chain_bound(a, k, False, adj)
        assert float(np.abs(sr.astype(np.float64) - blur).max()) <= bound


# ---------------------------------------------------------------------------------------------
# 2. orientation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,sf,K,ty,tx", [((2, 2, 36, 72), 2, 9, 1, 7), ((1, 1, 8, 8), 2, 5, 4, 0), ((2, 3, 24, 36), 3, 7, 6, 2), ((1, 2, 72, 36), 3, 9, 8, 3),
                                               ((1, 1, 80, 160), 2, 17, 0, 16)])
def test_orientation_is_exact(hip, shape, sf, K, ty, tx):
    """A single off-centre unit tap is a strided shift, bit for bit: H x [i, j] = x[i sf - dy, j sf - dx]; H_adj puts y[i, j] at (i sf - dy, j sf - dx)
    and zeros elsewhere"""
    x = det_normal(shape, 9500, K).numpy()
    B, Cc, H, W = shape
    y = det_normal((B, Cc, H // sf, W // sf), 9500, K + 1).numpy()
    k, r = P.unit_tap(K, ty, tx), K // 2
    dy, dx = ty - r, tx - r
    assert (dy, dx) != (0, 0)
    rc, h = run_op(hip, shape, sf, k, "H", x)
    rc2, ha = run_op(hip, shape, sf, k, "H_adj", y)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(h, S.strided_shift(x, dy, dx, sf))
    assert np.array_equal(ha, np.roll(S.zero_fill(y, sf), (-dy, -dx), axis=(-2, -1)))
    assert not np.array_equal(h, S.strided_shift(x, -dy, -dx, sf))


# ---------------------------------------------------------------------------------------------
# 3. separable kernel against the two-pass kind
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sf,K", [(2, 9), (4, 17)])
def test_separable_kernel_agrees_with_the_filtered_kind(hip, sf, K):
    """Kind 9 with outer(w, w), K odd, against kind 5 (two 1-D passes, then decimation / zero-fill first) on the same taps, within the sum of the two
    bounds: the PSF chain's (K^2 + 2) 2^-24 S and, for the two K-tap passes plus the rounding of outer(w, w) to fp32, (2 K + 4) 2^-24 S"""
    lib = hip.load()
    g = np.random.Generator(np.random.Philox(key=[9600, K]))
    w1 = g.uniform(0.1, 1.0, size=K); w1[K // 2 + 1] += 2.0
    w1 = (w1 / w1.sum()).astype(np.float32)
    shape = (2, 3, 64, 64)
    low = (2, 3, 64 // sf, 64 // sf)
    k = np.outer(w1, w1).astype(np.float32)
    for what, a in (("H", det_normal(shape, 9601).numpy()), ("H_adj", det_normal(low, 9602).numpy())):
        rc, sr = run_op(hip, shape, sf, k, what, a)
        assert rc == 0
        rc5, filt = run_op(hip, shape, sf, w1, what, a, kind=5, scratch_floats=2 * int(np.prod(shape)))
        assert rc5 == 0
        Sx = float((S.Hadj64(a, k, sf, absolute=True) if what == "H_adj" else S.H64(a, k, sf, absolute=True)).max())
        bound = (K * K + 2 + 2 * K + 4) * 2.0 ** -24 * Sx
        err = float(np.abs(sr.astype(np.float64) - filt).max())
        print(f"separable cross-check sf {sf} K {K} {what}: max|psf_sr - filtered| = {err:.3e} (bound {bound:.3e})")
        assert err <= bound


# ---------------------------------------------------------------------------------------------
# 4. gradient steps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("laplace", [False, True])
@pytest.mark.parametrize("si", [0, 1, 2, 3, 4, 6])
def test_gradient_steps_match_the_composed_operators(hip, si, laplace):
    """pf_grad_step / pf_grad_step_laplace against the same step composed in numpy fp32 from the engine's own H and H_adj outputs (the comparison of
    tests/test_gpu_psf.py): the low-resolution residual in the scratch is exact, the update within 2^-23 (|x| + |coef v|) elementwise"""
    B, Cc, H, W, sf, K = SHAPES[si]
    shape = (B, Cc, H, W)
    k = P.psf_kernel(K)
    x, _, y = op_data(si)
    coef = COEF[:B]
    rc, hx = run_op(hip, shape, sf, k, "H", x)
    assert rc == 0
    hadj = lambda r: run_op(hip, shape, sf, k, "H_adj", r)[1]
    r, v, z = P.grad_step32(x, y, coef, hx, hadj, laplace)
    rc, got, scr = run_op(hip, shape, sf, k, "laplace" if laplace else "grad", x, y=y, coef=coef, want_scratch=True)
    assert rc == 0
    assert scr.shape == y.shape and np.array_equal(scr, r), "the low-resolution residual (or its sign) is not exact"
    if laplace:
        assert set(np.unique(scr)) <= {-1.0, 1.0}
    bound = 2.0 ** -23 * (np.abs(x.astype(np.float64)) + np.abs(coef.astype(np.float64).reshape(-1, 1, 1, 1) * v))
    err = np.abs(got.astype(np.float64) - z)
    print(f"sr blur grad step {SHAPES[si]} laplace {laplace}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    assert float(np.abs(got - x).max()) > 1e-3               # the step moved the image


# ---------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------
def refused_everywhere(hip, d, shape, sf):
    """every entry point that takes the operator returns PF_ERR_INVALID for the descriptor d and leaves outputs and scratch poisoned"""
    lib = hip.load()
    st = hip.current_stream_ptr()
    B, Cc, H, W = shape
    s_eff = max(sf, 1)
    low = (B, Cc, max(H // s_eff, 1), max(W // s_eff, 1))
    xd, yd, cd = dev(det_normal(shape, 9702).numpy()), dev(np.zeros(low)), dev(COEF[:1])
    ad = torch.tensor([0.8], dtype=torch.float64, device="cuda")
    full, lowo = torch.full(shape, float("nan"), device="cuda"), torch.full(low, float("nan"), device="cuda")
    scr = torch.full((4 * int(np.prod(shape)) + H * W + 8,), float("nan"), device="cuda")
    rcs = dict(
        H=lib.pf_degradation_H(C.byref(d), xd.data_ptr(), lowo.data_ptr(), B, Cc, H, W, None, st),
        H_adj=lib.pf_degradation_H_adj(C.byref(d), yd.data_ptr(), full.data_ptr(), B, Cc, H, W, None, st),
        grad=lib.pf_grad_step(C.byref(d), xd.data_ptr(), yd.data_ptr(), cd.data_ptr(), full.data_ptr(), B, Cc, H, W, scr.data_ptr(), st),
        laplace=lib.pf_grad_step_laplace(C.byref(d), xd.data_ptr(), yd.data_ptr(), cd.data_ptr(), full.data_ptr(), B, Cc, H, W, scr.data_ptr(), st),
        vec=lib.pf_ot_ode_vec(C.byref(d), xd.data_ptr(), xd.data_ptr(), yd.data_ptr(), cd.data_ptr(), cd.data_ptr(), 0.01, full.data_ptr(), B, Cc, H, W,
                              scr.data_ptr(), st),
        spectrum=lib.pf_sr_aliased_spectrum(C.byref(d), H, W, lowo.data_ptr(), scr.data_ptr(), st),
        prox=lib.pf_sr_prox(C.byref(d), xd.data_ptr(), ad.data_ptr(), yd.data_ptr(), full.data_ptr(), B, Cc, H, W, scr.data_ptr(), st))
    torch.cuda.synchronize()
    assert all(rc == INVALID for rc in rcs.values()), rcs
    assert torch.isnan(full).all() and torch.isnan(lowo).all() and torch.isnan(scr).all()


def test_refusals_launch_nothing(hip):
    """PF_ERR_INVALID with the output untouched on every entry point (H, H_adj, both gradient steps, pf_ot_ode_vec, pf_sr_aliased_spectrum, pf_sr_prox): sf not
    dividing H or W, sf out of 1 .. 8, even K, K > 63, NULL taps, K larger than the image; in == out on the calls that have one input and one output (H, H_adj,
    pf_sr_prox), at sf 1 where the two have one size and at sf 2; pf_krylov_solve refuses the kind like the other superresolution kinds"""
    lib = hip.load()
    st = hip.current_stream_ptr()
    bad = [((1, 1, 80, 80), 3, P.psf_kernel(9)),                               # sf does not divide
           ((1, 1, 80, 90), 4, P.psf_kernel(9)),                               # ... W only
           ((1, 1, 80, 80), 0, P.psf_kernel(9)), ((1, 1, 80, 80), 16, P.psf_kernel(9)),
           ((1, 1, 80, 80), 2, np.ones((4, 4), dtype=np.float32)), ((1, 1, 80, 80), 2, np.ones((65, 65), dtype=np.float32)),
           ((1, 1, 8, 8), 2, P.psf_kernel(9))]                                 # K larger than the image
    for shape, sf, k in bad:
        d, keep = descriptor(hip, k, sf)
        refused_everywhere(hip, d, shape, sf)
    shape = (1, 1, 8, 8)
    d = hip.PfDegradation(); d.kind = 9; d.sf = 2; d.ntaps = 3; d.taps = None                                           # NULL taps
    refused_everywhere(hip, d, shape, 2)
    xd = dev(det_normal(shape, 9703).numpy())
    before = xd.clone()
    ad, lam, scr = torch.tensor([0.8], dtype=torch.float64, device="cuda"), torch.ones(64, device="cuda"), torch.full((1024,), float("nan"), device="cuda")
    for sf in (1, 2):                                                                                                   # in == out
        d, keep = descriptor(hip, P.psf_kernel(3), sf)
        assert lib.pf_degradation_H(C.byref(d), xd.data_ptr(), xd.data_ptr(), *shape, None, st) == INVALID
        assert lib.pf_degradation_H_adj(C.byref(d), xd.data_ptr(), xd.data_ptr(), *shape, None, st) == INVALID
        assert lib.pf_sr_prox(C.byref(d), xd.data_ptr(), ad.data_ptr(), lam.data_ptr(), xd.data_ptr(), *shape, scr.data_ptr(), st) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(xd, before) and torch.isnan(scr).all()
    # the Krylov solve: the measurement must have the image's shape
    d, keep = descriptor(hip, P.psf_kernel(3), 2)
    n = lib.pf_krylov_workspace_floats(1, 1, 8, 8, 5)
    ws, sol, rt2 = torch.full((n,), float("nan"), device="cuda"), torch.full(shape, float("nan"), device="cuda"), dev(COEF[:1])
    assert lib.pf_krylov_solve(C.byref(d), rt2.data_ptr(), 0.04, xd.data_ptr(), sol.data_ptr(), 1, 1, 8, 8, 5, 1e-6, 1e-6, ws.data_ptr(), n, None, st) == INVALID
    torch.cuda.synchronize()
    assert torch.isnan(sol).all() and torch.isnan(ws).all()


# ---------------------------------------------------------------------------------------------
# 6. the aliased spectrum
# ---------------------------------------------------------------------------------------------
def spectrum(hip, k, sf, H, W, kind):
    lib = hip.load()
    d, keep = descriptor(hip, k, sf, kind)
    out = torch.full((H // sf, W // sf), float("nan"), device="cuda")
    tmp = torch.empty((max(H * W, 2 * (H + W) + 2),), device="cuda")
    rc = lib.pf_sr_aliased_spectrum(C.byref(d), H, W, out.data_ptr(), tmp.data_ptr(), hip.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("B,Cc,H,W,sf,K", FOURIER)
def test_aliased_spectrum_matches_fp64(hip, B, Cc, H, W, sf, K):
    """lam against numpy fp64 under the rule of tests/test_gpu_psf.py::test_power_spectrum_matches_fp64: 2^-23 max lam absolute (the table entries are fp64
    values rounded once to fp32, their fp64 mean is rounded once more)"""
    k = P.psf_kernel(K)
    rc, got = spectrum(hip, k, sf, H, W, 9)
    assert rc == 0
    ref = S.aliased_spectrum64(k, H, W, sf)
    err = float(np.abs(got - ref).max())
    print(f"aliased spectrum {(H, W, sf, K)}: max err {err:.3e} (bound {2.0 ** -23 * ref.max():.3e})")
    assert err <= 2.0 ** -23 * float(ref.max())


@pytest.mark.parametrize("H,W,sf", [(64, 64, 2), (64, 128, 4), (24, 36, 3)])
def test_aliased_spectrum_of_the_bicubic_kind_matches_fp64(hip, H, W, sf):
    from pnpflow_amd.degradations import bicubic_taps
    w1 = bicubic_taps(sf)
    rc, got = spectrum(hip, w1, sf, H, W, 5)
    assert rc == 0
    ref = S.aliased_spectrum64(w1, H, W, sf)
    err = float(np.abs(got - ref).max())
    print(f"aliased spectrum bicubic {(H, W, sf)}: max err {err:.3e} (bound {2.0 ** -23 * ref.max():.3e})")
    assert err <= 2.0 ** -23 * float(ref.max())


# ---------------------------------------------------------------------------------------------
# 7. pf_ot_ode_vec
# ---------------------------------------------------------------------------------------------
def ot_ode_vec_case(hip, shape, sf, k, kind, seed):
    lib = hip.load()
    B, Cc, H, W = shape
    low = (B, Cc, H // sf, W // sf)
    x, vt, w = (det_normal(shape, seed, i).numpy() for i in range(3))
    y = (S.H64(w, k, sf) + 0.05 * det_normal(low, seed, 3).numpy()).astype(np.float32)
    omt, rt2, sigma2 = np.array([0.6, 0.3], dtype=np.float32)[:B], np.array([0.55, 0.2], dtype=np.float32)[:B], 0.05 ** 2
    ref = S.ot_ode_vec64(k, sf, x, vt, y, omt, rt2, np.float32(sigma2))
    d, keep = descriptor(hip, k, sf, kind)
    n = lib.pf_sr_solve_scratch_floats(B, Cc, H, W, sf)
    assert n > 0
    out, scr = torch.full(shape, float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
    xd, vd, yd, od, rd = dev(x), dev(vt), dev(y), dev(omt), dev(rt2)
    rc = lib.pf_ot_ode_vec(C.byref(d), xd.data_ptr(), vd.data_ptr(), yd.data_ptr(), od.data_ptr(), rd.data_ptr(), float(sigma2), out.data_ptr(), B, Cc, H, W,
                           scr.data_ptr(), hip.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return out.cpu().numpy().astype(np.float64), ref


@pytest.mark.parametrize("B,Cc,H,W,sf,K", SOLVES)
def test_ot_ode_vec_fourier_solve_matches_fp64(hip, B, Cc, H, W, sf, K):
    """pf_ot_ode_vec of kind 9 against the fp64 closed form: the project's Fourier-solve bound, 5e-5 max|ref|
    (tests/test_gpu_psf.py::test_ot_ode_vec_fourier_solve_matches_fp64)"""
    got, ref = ot_ode_vec_case(hip, (B, Cc, H, W), sf, P.psf_kernel(K), 9, 9800 + K)
    err = float(np.abs(got - ref).max())
    print(f"sr blur Fourier solve {(B, Cc, H, W, sf, K)}: max|hip - fp64| = {err:.3e} (bound {5e-5 * np.abs(ref).max():.3e})")
    assert err <= 5e-5 * float(np.abs(ref).max())


@pytest.mark.parametrize("sf", [2, 4])
def test_ot_ode_vec_of_the_bicubic_kind_matches_fp64(hip, sf):
    from pnpflow_amd.degradations import bicubic_taps
    got, ref = ot_ode_vec_case(hip, (2, 3, 64, 64), sf, bicubic_taps(sf), 5, 9850 + sf)
    err = float(np.abs(got - ref).max())
    print(f"bicubic sf {sf} Fourier solve: max|hip - fp64| = {err:.3e} (bound {5e-5 * np.abs(ref).max():.3e})")
    assert err <= 5e-5 * float(np.abs(ref).max())


# ---------------------------------------------------------------------------------------------
# 8. the prox alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Cc,H,W,sf,K", SOLVES)
def test_prox_satisfies_the_optimality_condition(hip, B, Cc, H, W, sf, K):
    """x = pf_sr_prox(z + alpha H_adj(y)) satisfies x + alpha H_adj(H x - y) = z against the engine's own H / H_adj, and agrees with the fp64 prox, both
    within the Fourier-solve bound of test_ot_ode_vec_fourier_solve_matches_fp64, 5e-5 max|ref| with ref the fp64 prox; two calls return the same bits"""
    lib = hip.load()
    shape, low = (B, Cc, H, W), (B, Cc, H // sf, W // sf)
    k = P.psf_kernel(K)
    z, y = det_normal(shape, 9900 + K, 0).numpy(), det_normal(low, 9900 + K, 1).numpy()
    alpha = 0.8
    hadj = lambda a: run_op(hip, shape, sf, k, "H_adj", a)[1].astype(np.float64)
    Hf = lambda a: run_op(hip, shape, sf, k, "H", a)[1].astype(np.float64)
    r = (z.astype(np.float64) + alpha * hadj(y)).astype(np.float32)
    rc, lam = spectrum(hip, k, sf, H, W, 9)
    assert rc == 0
    d, keep = descriptor(hip, k, sf)
    n = lib.pf_sr_solve_scratch_floats(B, Cc, H, W, sf)
    rd, ld, ad = dev(r), dev(lam), torch.tensor([alpha], dtype=torch.float64, device="cuda")
    outs = []
    for _ in range(2):
        out, scr = torch.full(shape, float("nan"), device="cuda"), torch.full((n,), float("nan"), device="cuda")
        assert lib.pf_sr_prox(C.byref(d), rd.data_ptr(), ad.data_ptr(), ld.data_ptr(), out.data_ptr(), B, Cc, H, W, scr.data_ptr(), hip.current_stream_ptr()) == 0
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]), "two calls differ"
    x = outs[0]
    res = x.astype(np.float64) + alpha * hadj((Hf(x) - y).astype(np.float32)) - z
    ref = S.prox64(k, sf, z, y, alpha)
    scale = float(np.abs(ref).max())
    print(f"sr prox {(B, Cc, H, W, sf, K)}: optimality residual {np.abs(res).max():.3e}, max|hip - fp64| {np.abs(x - ref).max():.3e} (bound {5e-5 * scale:.3e})")
    assert float(np.abs(res).max()) <= 5e-5 * scale
    assert float(np.abs(x - ref).max()) <= 5e-5 * scale
    assert lib.pf_sr_prox(C.byref(d), rd.data_ptr(), ad.data_ptr(), ld.data_ptr(), rd.data_ptr(), B, Cc, H, W, scr.data_ptr(), hip.current_stream_ptr()) == INVALID


# ---------------------------------------------------------------------------------------------
# 9. solvers
# ---------------------------------------------------------------------------------------------
def gs_solver(m, **kw):
    from pnpflow_amd.methods.pnp_gs import PROX_PNP
    from pnpflow_amd.train_denoiser import GRADIENT_STEP_DENOISER
    from pnpflow_amd.utils import CfgNode
    a = dict(method="pnp_gs", model="gradient_step", problem="superresolution_blur", noise_type="gaussian", algo="hqs", max_iter=3, lr_pnp=1.0, alpha=0.5,
             sigma_factor=1.0, max_batch=1, compute_time=False, compute_memory=False, save_results=False, batch=0, dim_image=m.input_height,
             num_channels=m.input_channels)
    a.update(kw)
    args = CfgNode(a)
    return PROX_PNP(GRADIENT_STEP_DENOISER(m, torch.device("cuda"), args), torch.device("cuda"), args)


def GS_TOL(jn_max):
    return 2e-5 + 2 * 5e-5 * float(jn_max)            # TOL of tests/test_gpu_pnp_gs.py


def test_python_operator_matches_reference_golden(hip, golden):
    g = golden("sr_blur_op")
    x = torch.from_numpy(g["clean"])
    d = engine_op(g["psf"], int(g["sf"]))
    np.testing.assert_allclose(d.H(x.cuda()).cpu().numpy(), g["H"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(d.H_adj(torch.from_numpy(g["H"]).cuda()).cpu().numpy(), g["Hadj"], rtol=0, atol=1e-5)


def test_pnp_flow_matches_reference(hip, golden):
    from pnpflow_amd.methods.pnp_flow import PNP_FLOW
    from pnpflow_amd.utils import CfgNode
    g = golden("pnp_traj_sr_blur")
    m, cfg, sd = model_for("tiny4")
    sigma, steps, ns = float(g["sigma"]), int(g["steps"]), int(g["num_samples"])
    args = CfgNode(dict(method="pnp_flow", model="ot", problem="superresolution_blur", noise_type="gaussian", num_samples=ns, steps_pnp=steps, lr_pnp=1.0,
                        gamma_style="alpha_1_minus_t", alpha=float(g["alpha"]), max_batch=1, compute_time=False, compute_memory=False, save_results=False,
                        batch=0, sigma_noise=sigma))
    solver = PNP_FLOW(m, torch.device("cuda"), args)
    solver.noise = torch.stack([det_normal((2, 3, 64, 64), 41, 1 + i) for i in range(steps * ns)]).cuda()
    its = {}
    solver.restore_batch(torch.from_numpy(g["noisy"]).cuda(), engine_op(g["psf"], int(g["sf"])), sigma, lr=sigma ** 2,
                         iter_cb=lambda it, xx: its.__setitem__(it, xx.clone().cpu()))
    for it in (0, 1, 4, 9):
        print(f"pnp_flow sr blur iterate {it}: max|hip - reference| = {float(np.abs(its[it].numpy() - g[f'x_it{it}']).max()):.3e}")
    for it in (0, 1, 4, 9):
        np.testing.assert_allclose(its[it].numpy(), g[f"x_it{it}"], atol=TRAJ_ATOL, err_msg=f"iterate {it}")


def test_ot_ode_engine_loop_matches_reference_gmres_trajectory(hip, golden, monkeypatch):
    """The engine's closed-form loop against the reference's GMRES trajectory (every solve stopped on its tolerance): 1e-3 of max|ref|, the fixture's own
    fp32-vs-fp64-closed-form distance (first two iterates and last) under a quarter of that"""
    from pnpflow_amd.methods.ot_ode import OT_ODE
    from pnpflow_amd.utils import CfgNode, psnr_per_image
    g = golden("ot_ode_traj_sr_blur")
    m, cfg, sd = model_for("tiny4")
    S_, steps, t0, sigma, first = cfg["input_height"], int(g["steps"]), float(g["start_time"]), float(g["sigma"]), int(g["first"])
    assert int(g["gmres_vectors"].max()) < 100 and int(g["gmres_vectors"].min()) > 0
    assert float(g["dist_fp64"]) < 0.25 * 1e-3 and float(g["dist_fp64_last"]) < 0.25 * 1e-3
    args = CfgNode(dict(method="ot_ode", model="ot", problem="superresolution_blur", steps_ode=steps, start_time=t0, gamma="constant", max_batch=1,
                        compute_time=False, compute_memory=False, save_results=False, batch=0))
    solver = OT_ODE(m, torch.device("cuda"), args)

    def no_host_loop(*a, **k):
        raise AssertionError("the host GMRES loop ran")
    monkeypatch.setattr(solver, "_restore_batch_generic", no_host_loop)
    solver.init_noise = det_normal((2, 3, S_, S_), 61, 1).cuda()
    its = {}
    x = solver.restore_batch(torch.from_numpy(g["noisy"]).cuda(), engine_op(g["psf"], int(g["sf"])), sigma, iter_cb=lambda it, xx: its.__setitem__(it, xx.clone().cpu()))
    assert solver.last_krylov_iterations == 0
    for it in (first, first + 1, steps - 1):
        ref = g[f"x_it{it}"]
        print(f"ot_ode sr blur iterate {it}: max|hip - reference| / max|ref| = {float(np.abs(its[it].numpy() - ref).max() / np.abs(ref).max()):.3e}")
    # first: the eager step; first + 1: the step the graph is captured on; steps - 1: after the replays of the captured graph
    assert first + 1 < steps - 1
    for it in (first, first + 1, steps - 1):
        ref = g[f"x_it{it}"]
        np.testing.assert_allclose(its[it].numpy(), ref, atol=1e-3 * float(np.abs(ref).max()), err_msg=f"iterate {it}")
    clean = det_image((2, 3, S_, S_), 31)
    p_hip = psnr_per_image(x, clean.cuda()).cpu()
    p_ref = O.psnr_per_image(torch.from_numpy(g[f"x_it{steps - 1}"]), clean)
    assert float((p_hip - p_ref).abs().max()) <= 0.05, (p_hip, p_ref)             # tests/test_gpu_psf.py


def test_ot_ode_bicubic_step_matches_fp64_closed_form(hip, monkeypatch):
    """OT-ODE with Superresolution(mode="bicubic") runs on the engine loop (it returned PF_ERR_INVALID) and its first Euler step equals an fp64 closed-form
    restatement of ot_ode.py:63-147 within the engine loop's 1e-3 of max|ref|"""
    import pnpflow_amd.degradations as D
    from pnpflow_amd.methods.ot_ode import OT_ODE
    from pnpflow_amd.utils import CfgNode
    m, cfg, sd = model_for("tiny4")
    sf, steps, t0, sigma, shape = 2, 10, 0.9, 0.05, (2, 3, 64, 64)
    do = S.SrBlur(None, sf, 3, 64)
    noisy = (do.H(det_image(shape, 31)) + sigma * det_normal((2, 3, 32, 32), 71)).float()
    init = det_normal(shape, 72)
    assert int(steps * t0) == steps - 1                      # one Euler step
    ref = S.ot_ode_restore64(sd, cfg, do, noisy, sigma, steps, t0, init).numpy()
    args = CfgNode(dict(method="ot_ode", model="ot", problem="superresolution_bicubic", steps_ode=steps, start_time=t0, gamma="constant", max_batch=1,
                        compute_time=False, compute_memory=False, save_results=False, batch=0))
    solver = OT_ODE(m, torch.device("cuda"), args)
    monkeypatch.setattr(solver, "_restore_batch_generic", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the host GMRES loop ran")))
    solver.init_noise = init.cuda()
    got = solver.restore_batch(noisy.cuda(), D.Superresolution(sf, 64, mode="bicubic"), sigma).cpu().numpy()
    err = float(np.abs(got - ref).max())
    print(f"ot_ode bicubic one step: max|hip - fp64| / max|ref| = {err / np.abs(ref).max():.3e}")
    assert err <= 1e-3 * float(np.abs(ref).max())


def test_pnp_gs_hqs_matches_reference_golden(hip, golden):
    """algo 3: teacher-forced single iterations at GS_TOL, then free-running from the initialisation at GS_TOL growth^(k-1) (tests/test_gpu_pnp_gs.py)"""
    g = golden("pnp_gs_tiny4_hqs_sr_blur")
    m, _, _ = model_for("tiny4")
    dg = engine_op(g["psf"], int(g["sf"]))
    sigma, growth = float(g["sigma"]), float(g["growth"])
    noisy = torch.from_numpy(g["noisy"]).cuda()
    s = gs_solver(m)
    for k in range(3):
        x = s.restore_batch(noisy, dg, sigma, first=k, stop=k + 1, x0=torch.from_numpy(g["iterates"][k]).cuda(), alpha=0.5)
        err = float(np.abs(x.cpu().numpy() - g["iterates"][k + 1]).max())
        print(f"pnp_gs hqs sr blur teacher-forced {k}: err / TOL = {err / GS_TOL(g['jn_max'][k]):.4f}")
        assert s.last_alpha == 0.5 and s.last_gap_log is None              # alpha never decays, no gap log
        np.testing.assert_allclose(x.cpu().numpy(), g["iterates"][k + 1], atol=GS_TOL(g["jn_max"][k]))
    bound = lambda k: max(GS_TOL(j) for j in g["jn_max"][:k]) * growth ** (k - 1)
    for k in (1, 2, 3):
        x = s.restore_batch(noisy, dg, sigma, first=0, stop=k, lr=sigma ** 2, alpha=0.5)
        err = float(np.abs(x.cpu().numpy() - g["iterates"][k]).max())
        print(f"pnp_gs hqs sr blur free-running after iteration {k}: err / bound = {err / bound(k):.4f}")
        np.testing.assert_allclose(x.cpu().numpy(), g["iterates"][k], atol=bound(k), err_msg=f"after iteration {k}")
    with pytest.raises(ValueError, match="pgd only"):
        gs_solver(m, noise_type="laplace").restore_batch(noisy, dg, sigma)


def test_pnp_gs_pgd_iteration_matches_restatement(hip):
    import pnp_gs_restatement as R
    m, cfg, sd = model_for("tiny4")
    k, sf = P.psf_kernel(9), 2
    do = S.SrBlur(k, sf, 3, 64)
    sigma, shape = 0.05, (2, 3, 64, 64)
    noisy = do.H(det_image(shape, 93)) + sigma * det_normal((2, 3, 32, 32), 94)
    kw = dict(algo="pgd", problem="superresolution_blur", max_iter=2, sigma_noise=sigma)
    xs, alphas, infos = R.solve(lambda x, s: O.unet_forward(sd, cfg, x, s), do, noisy, alpha=0.5, stop=1, **kw)
    s = gs_solver(m, algo="pgd", max_iter=2)
    x = s.restore_batch(noisy.cuda(), engine_op(k, sf), sigma, first=0, stop=1, x0=xs[0].cuda(), alpha=alphas[0])
    np.testing.assert_allclose(x.cpu().numpy(), xs[1].numpy(), atol=GS_TOL(infos[0]["JN"].abs().max()))


def test_d_flow_value_and_grad_matches_restatement(hip):
    import dflow_restatement as R
    from pnpflow_amd.methods.d_flow import D_FLOW
    from pnpflow_amd.utils import CfgNode
    LOSS_RTOL, GRAD_RTOL = 1e-5, 2e-4        # tests/test_gpu_d_flow.py
    m, cfg, sd = model_for("tiny4")
    k, sf = P.psf_kernel(9), 2
    do = S.SrBlur(k, sf, 3, 64)
    z = det_normal((2, 3, 64, 64), 82)
    y = do.H(det_image((2, 3, 64, 64), 83)) + 0.05 * det_normal((2, 3, 32, 32), 84)
    per, gref = R.value_and_grad(z, y, do.H, lambda x, t: O.unet_forward(sd, cfg, x, t), 0.001)
    s = D_FLOW(m, torch.device("cuda"), CfgNode(dict(method="d_flow", model="ot", problem="superresolution_blur", steps_euler=6, lmbda=0.001, alpha=0.1, max_iter=1,
                                                    LBFGS_iter=3, start_time=0.0, max_batch=1, compute_time=False, compute_memory=False, save_results=False, batch=0)))
    loss, grad = s.value_and_grad(z.cuda(), y.cuda(), engine_op(k, sf), 0.001)
    np.testing.assert_allclose(loss.cpu().numpy(), per.numpy(), rtol=LOSS_RTOL)
    np.testing.assert_allclose(grad.cpu().numpy(), gref.numpy(), atol=GRAD_RTOL * float(gref.abs().max()))


def test_flow_priors_data_gradient_matches_fp64_restatement(hip):
    """TOL_data = 2 lmbda dt 2e-5 max|pred| + dt (2e-5 + 5e-5 max|J^T w|) (tests/test_gpu_flow_priors.py)"""
    import flow_priors_restatement as R
    from pnpflow_amd.methods.flow_priors import FLOW_PRIORS
    from pnpflow_amd.utils import CfgNode
    m, cfg, sd = model_for("tiny4")
    it, sigma, seed = 60, 0.05, 16
    _, _, _, inp = R.case_inputs(("denoising", "gaussian", it, sigma, seed))
    k, sf = P.psf_kernel(9), 2
    do = S.SrBlur(k, sf, 3, 64)
    y = (do.H(inp["clean"]) + sigma * R.det_normal((2, 3, 32, 32), seed, 3)).float()
    f64 = lambda t: t.double()
    vel = R.oracle_vel(sd, cfg, torch.float64)
    _, g_data, _, _, pred, info = R.grad(vel, do.H, f64(inp["x"]), f64(inp["x_init"]), f64(y), f64(inp["eps"]), it, R.N_STEP, R.LMBDA, "gaussian", zero_trace=True)
    dt = 1.0 / R.N_STEP
    w = 2 * R.LMBDA * do.H_adj(info["r"])
    jtw_max = float(((g_data - w) / dt).abs().max())
    tol = 2 * R.LMBDA * dt * 2e-5 * float(pred.abs().max()) + dt * (2e-5 + 5e-5 * jtw_max)
    s = FLOW_PRIORS(m, torch.device("cuda"), CfgNode(dict(method="flow_priors", model="ot", problem="superresolution_blur", noise_type="gaussian", N=R.N_STEP, K=1,
                                                         lmbda=R.LMBDA, eta=R.ETA, start_time=0.0, max_batch=1, compute_time=False, compute_memory=False,
                                                         save_results=False, batch=0)))
    _, eg_data, _, epred = s.gradient(inp["x"].cuda(), inp["x_init"].cuda(), y.cuda(), engine_op(k, sf), inp["eps"].cuda(), it)
    err = float((eg_data.cpu().double() - g_data).abs().max())
    print(f"flow_priors sr blur: g_data err {err:.3e} (TOL {tol:.3e}, max {float(g_data.abs().max()):.3e})")
    assert float(g_data.abs().max()) > 20 * tol
    assert err <= tol


# ---------------------------------------------------------------------------------------------
# 10. main.py
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,problem,extra", [("pnp_flow", "superresolution_blur", ("steps_pnp", "10", "num_samples", "2", "psf_size", "9")),
                                                  ("ot_ode", "superresolution_blur", ("steps_ode", "10", "start_time", "0.5", "psf", "disk", "psf_size", "9")),
                                                  ("pnp_gs", "superresolution_blur", ("model", "gradient_step", "algo", "hqs", "max_iter", "3", "psf_size", "9")),
                                                  ("ot_ode", "superresolution_bicubic", ("steps_ode", "10", "start_time", "0.5"))])
def test_main_end_to_end(hip, tmp_path, method, problem, extra):
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--opts", "dataset", "celeba", "problem", problem, "method", method, "synthetic", "True",
           "max_batch", "1", "batch_size_ip", "2", *extra, "output_root", str(tmp_path) + "/"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    files = [p for p in tmp_path.rglob("psnr_rec_batch0.txt")]
    assert files, [str(p) for p in tmp_path.rglob("*")]
    vals = [float(l.split()[1]) for l in open(files[0]).read().strip().splitlines()]
    assert vals and all(np.isfinite(v) for v in vals), vals
