"""Host side of the point-spread-function blur (PSFDeblurring; PF_DEG_PSF_BLUR circular, PF_DEG_PSF_BLUR_ZERO zero boundary): the tests' restatement
(tests/psf_restatement.py) reproduces the real reference's fixtures (tools/make_golden_psf.py) for the operator and the solvers, at the bounds
tests/test_zero_blur_host.py and tests/test_pnp_gs_host.py use for the Gaussian twins; the Python surface (PSFDeblurring, pnpflow_amd.psf,
main.make_degradation, the solvers' problem names) and the C ABI declare the two kinds and pf_psf_power_spectrum.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import CFGS, det_image, det_normal
from oracle import pnpflow_oracle as O
import psf_restatement as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny4():
    cfg = O.unet_config(**CFGS["tiny4"])
    sd = O.synthetic_state_dict(cfg, 0)
    return cfg, sd


# ---- 1. the restatement against the real reference -----------------------------------------------------------------------------------
def test_restatement_operator_matches_reference(golden):
    g = golden("psf_op")
    x = det_image((2, 3, 64, 64), 31)[:1]
    for K in (9, 21):
        k = g[f"psf{K}"]
        np.testing.assert_array_equal(k, P.psf_kernel(K))
        assert not np.array_equal(k, k[::-1, ::-1])              # asymmetric: H and H_adj differ
        for mode in ("fft", "zero"):
            d = P.PsfBlur(k, mode, 3, 64)
            np.testing.assert_allclose(d.H(x).numpy(), g[f"k{K}_{mode}_H"], atol=1e-6)
            np.testing.assert_allclose(d.H_adj(x).numpy(), g[f"k{K}_{mode}_Hadj"], atol=1e-6)
            np.testing.assert_allclose(P.apply64(x.numpy(), k, mode == "zero"), g[f"k{K}_{mode}_H"], atol=2e-6)
            np.testing.assert_allclose(P.apply64(x.numpy(), k, mode == "zero", adjoint=True), g[f"k{K}_{mode}_Hadj"], atol=2e-6)
            assert np.abs(g[f"k{K}_{mode}_H"] - g[f"k{K}_{mode}_Hadj"]).max() > 1e-2
        # the two boundary rules differ at the border and agree in the interior
        assert np.abs(g[f"k{K}_fft_H"] - g[f"k{K}_zero_Hadj"])[..., :2, :].max() > 1e-2
        r = K // 2
        np.testing.assert_allclose(g[f"k{K}_fft_H"][..., r:-r, r:-r], g[f"k{K}_zero_Hadj"][..., r:-r, r:-r], atol=2e-6)


def test_restatement_direct_sums_and_adjoints():
    """apply64 on non-square images against an index-by-index sum; both pairs are adjoint in fp64; the kernel radius may reach past the image"""
    k = P.psf_kernel(5).astype(np.float64)
    x, y = det_normal((1, 1, 6, 7), 5).numpy().astype(np.float64), det_normal((1, 1, 6, 7), 6).numpy().astype(np.float64)
    Hh, Ww, r = 6, 7, 2
    circ, zero = np.zeros((Hh, Ww)), np.zeros((Hh, Ww))
    for i in range(Hh):
        for j in range(Ww):
            for a in range(5):
                for b in range(5):
                    circ[i, j] += k[a, b] * x[0, 0, (i - (a - r)) % Hh, (j - (b - r)) % Ww]          # H of kind 7: the convolution
                    ii, jj = i + a - r, j + b - r
                    if 0 <= ii < Hh and 0 <= jj < Ww:
                        zero[i, j] += k[a, b] * x[0, 0, ii, jj]                                      # H of kind 8: the correlation
    np.testing.assert_allclose(P.apply64(x, k, zero=False)[0, 0], circ, atol=1e-14)
    np.testing.assert_allclose(P.apply64(x, k, zero=True)[0, 0], zero, atol=1e-14)
    for z in (False, True):
        assert abs((P.apply64(x, k, z) * y).sum() - (x * P.apply64(y, k, z, adjoint=True)).sum()) < 1e-12
    big = P.psf_kernel(17)
    small = det_normal((1, 1, 8, 8), 7).numpy()
    ref = torch.nn.functional.conv2d(torch.from_numpy(small).double(), torch.from_numpy(big).double().view(1, 1, 17, 17), padding="same")
    np.testing.assert_allclose(P.apply64(small, big, zero=True), ref.numpy(), atol=1e-14)
    # a unit tap is a shift, in opposite directions for H and H_adj
    u = P.unit_tap(5, 1, 4)                    # (j - r) = (-1, +2)
    np.testing.assert_array_equal(P.apply64(x, u, zero=False), P.shift_exact(x, -1, 2, zero=False))
    np.testing.assert_array_equal(P.apply64(x, u, zero=False, adjoint=True), P.shift_exact(x, 1, -2, zero=False))
    np.testing.assert_array_equal(P.apply64(x, u, zero=True), P.shift_exact(x, 1, -2, zero=True))
    np.testing.assert_array_equal(P.apply64(x, u, zero=True, adjoint=True), P.shift_exact(x, -1, 2, zero=True))


@pytest.mark.parametrize("tag,mode,noise_type", [("psf_fft", "fft", "gaussian"), ("laplace_psf_zero", "zero", "laplace")])
def test_restatement_pnp_flow_matches_reference(golden, tag, mode, noise_type):
    g = golden("pnp_traj_" + tag)
    cfg, sd = tiny4()
    steps, ns, sigma = int(g["steps"]), int(g["num_samples"]), float(g["sigma"])
    its = {}
    O.pnp_flow_restore(lambda a, t: O.unet_forward(sd, cfg, a, t), P.PsfBlur(g["psf"], mode, 3, 64), torch.from_numpy(g["noisy"]), sigma, steps=steps, num_samples=ns,
                       alpha=float(g["alpha"]), noise_fn=lambda it, s, like: det_normal(tuple(like.shape), 41, 1 + it * ns + s),
                       record=lambda it, x: its.__setitem__(it, x.clone()), noise_type=noise_type)
    for it in (0, 1, 4, 9):
        np.testing.assert_allclose(its[it].numpy(), g[f"x_it{it}"], atol=2e-5, err_msg=f"iterate {it}")


@pytest.mark.parametrize("tag,mode,problem", [("psf_fft", "fft", "gaussian_deblurring_FFT"), ("psf_zero", "zero", "gaussian_deblurring")])
def test_restatement_ot_ode_matches_reference(golden, tag, mode, problem):
    g = golden("ot_ode_traj_" + tag)
    cfg, sd = tiny4()
    steps, t0, sigma = int(g["steps"]), float(g["start_time"]), float(g["sigma"])
    if mode == "zero":
        assert g["gmres_vectors"].shape == (steps - int(g["first"]), 2) and 0 < g["gmres_vectors"].min() and g["gmres_vectors"].max() < 100
    its = {}
    O.ot_ode_restore(lambda a, t: O.unet_forward(sd, cfg, a, t), lambda x, t, v: O.unet_vjp(sd, cfg, x, t, v), P.PsfBlur(g["psf"], mode, 3, 64), problem,
                     torch.from_numpy(g["noisy"]), sigma, steps=steps, start_time=t0, gamma="constant", init_noise=det_normal((2, 3, 64, 64), 61, 1),
                     record=lambda it, x: its.__setitem__(it, x.clone()))
    first = int(g["first"])
    for it in (first, first + 1, steps - 1):
        ref = g[f"x_it{it}"]
        np.testing.assert_allclose(its[it].numpy(), ref, atol=1e-4 * max(1.0, float(np.abs(ref).max())), err_msg=f"iterate {it}")


def test_restatement_pnp_gs_hqs_matches_reference(golden):
    """the procedure of tests/test_pnp_gs_host.py::test_restatement_reproduces_reference_goldens on the PSF fixture"""
    import pnp_gs_restatement as R
    g = golden("pnp_gs_tiny4_hqs_psf_fft")
    cfg, sd = tiny4()
    net = lambda x, s: O.unet_forward(sd, cfg, x, s)
    d = P.PsfBlur(g["psf"], "fft", 3, 64)
    MAX_ITER, ALPHA = 3, 0.5
    sigma = float(g["sigma"])
    its = [torch.from_numpy(a) for a in g["iterates"]]
    assert len(its) == MAX_ITER + 1 and len(g["alpha"]) == MAX_ITER + 1
    hc = d.H(det_image((2, 3, 64, 64), 33))
    np.testing.assert_allclose((hc + det_normal(tuple(hc.shape), int(g["noise_seed"]), 0) * sigma).numpy(), g["noisy"], atol=1e-6)
    noisy = torch.from_numpy(g["noisy"])
    kw = dict(algo="hqs", problem="gaussian_deblurring_FFT", noise_type="gaussian", max_iter=MAX_ITER, sigma_noise=sigma)
    scale = lambda a: float(a.abs().max())
    np.testing.assert_allclose(R.initialise("gaussian_deblurring_FFT", noisy, d).numpy(), its[0].numpy(), atol=1e-4 * scale(its[0]))
    for k in range(MAX_ITER):
        xn, an, info = R.iterate(net, d, its[k], noisy, k, alpha=float(g["alpha"][k]), **kw)
        np.testing.assert_allclose(xn.numpy(), its[k + 1].numpy(), atol=1e-4 * scale(its[k + 1]), err_msg=f"iteration {k}")
        assert an == float(g["alpha"][k + 1]), (k, an, g["alpha"])
        np.testing.assert_allclose([info["gap"], info["thr"]], g["gap"][k], rtol=1e-3)
    xs, alphas, _ = R.solve(net, d, noisy, alpha=ALPHA, **kw)
    assert alphas == [float(a) for a in g["alpha"]]
    growth = float(g["growth"])
    assert growth >= 1.0 and growth ** 2 * 2e-4 <= 0.05
    for k in range(1, MAX_ITER + 1):
        np.testing.assert_allclose(xs[k].numpy(), its[k].numpy(), atol=2e-4 * growth ** (k - 1) * scale(its[k]), err_msg=f"after iteration {k}")
    gap, thr = g["gap"][:, 0], g["gap"][:, 1]
    assert (np.abs(gap - thr) >= 0.01 * np.maximum(np.abs(gap), np.abs(thr))).all()       # no decision can flip on rounding


def test_fixtures_are_small_and_carry_the_psf(golden):
    from pnpflow_amd.psf import motion_psf
    for name in ("pnp_traj_psf_fft", "pnp_traj_laplace_psf_zero", "ot_ode_traj_psf_fft", "ot_ode_traj_psf_zero", "pnp_gs_tiny4_hqs_psf_fft"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= 460 * 1024
        np.testing.assert_array_equal(golden(name)["psf"], motion_psf(21, 1 if name == "ot_ode_traj_psf_zero" else 0))


# ---- 2. the Python surface ---------------------------------------------------------------------------------------------------------------
def test_psf_deblurring_kinds_padding_cropping_and_refusals():
    import pnpflow_amd._lib as L
    import pnpflow_amd.degradations as D
    k = P.psf_kernel(9)
    a, b = D.PSFDeblurring(k, "fft", 3, 64, "cpu"), D.PSFDeblurring(k, "spatial", 3, 64, "cpu")
    assert (a.kind, b.kind) == (L.PF_DEG_PSF_BLUR, L.PF_DEG_PSF_BLUR_ZERO) == (7, 8)
    assert D.PSFDeblurring(k, "anything-but-fft", 3, 64, "cpu").kind == 8
    assert (a.kernel_size, a.mode, b.mode) == (9, "fft", "spatial") and a.out_side(64) == 64
    np.testing.assert_array_equal(a.kernel.numpy(), k)
    # .filter is the reference's rolled (1, C, dim, dim) attribute
    np.testing.assert_array_equal(a.filter.cpu().numpy(), P.PsfBlur(k, "fft", 3, 64).filter.numpy())
    assert tuple(a.filter.shape) == (1, 3, 64, 64) and float(a.filter[0, 0, 0, 0]) == float(k[4, 4])
    # rectangular: zero-padded, centred, to a square
    rect = np.arange(1, 16, dtype=np.float32).reshape(3, 5)
    sq = D.PSFDeblurring(rect, "fft", 1, 32, "cpu")
    assert sq.kernel_size == 5
    np.testing.assert_array_equal(sq.taps_host[1:4], rect)
    assert not sq.taps_host[0].any() and not sq.taps_host[4].any()
    # all-zero border rings are cropped, the centre stays the centre, no non-zero tap is dropped
    pad = np.zeros((13, 13), dtype=np.float32); pad[2:11, 2:11] = k
    c = D.PSFDeblurring(pad, "spatial", 3, 64, "cpu")
    assert c.kernel_size == 9
    np.testing.assert_array_equal(c.taps_host, k)
    lone = np.zeros((7, 7), dtype=np.float32); lone[3, 0] = 1.0          # one non-zero tap on the outer ring: nothing can go
    assert D.PSFDeblurring(lone, "fft", 1, 32, "cpu").kernel_size == 7
    assert D.PSFDeblurring(np.zeros((5, 5)), "fft", 1, 32, "cpu").kernel_size == 1
    assert D.PSFDeblurring(torch.from_numpy(k), "fft", 3, 64, "cpu").kernel_size == 9
    # descriptor fields (a device of "cpu" keeps the taps on the host: the layout is what is checked)
    d = a.descriptor(2, 64, 64, "cpu")
    assert (d.kind, d.ntaps) == (7, 9) and d.taps
    for bad, msg in ((np.ones((4, 5)), "odd"), (np.ones((5, 4)), "odd"), (np.ones((65, 65)), "63"), (np.ones(5), "2-D"), (np.ones((3, 3), dtype=complex), "real"),
                     (np.full((3, 3), np.nan), "finite")):
        with pytest.raises(ValueError, match=msg):
            D.PSFDeblurring(bad, "fft", 3, 64, "cpu")
    with pytest.raises(ValueError, match="fit"):
        D.PSFDeblurring(P.psf_kernel(31), "fft", 3, 16, "cpu")
    assert D.PSFDeblurring(P.psf_kernel(31), "spatial", 3, 16, "cpu").kernel_size == 31       # no size rule for the zero boundary


def test_psf_generators():
    from pnpflow_amd import psf
    for size in (9, 31, 61):
        for seed in (0, 3):
            k = psf.motion_psf(size, seed)
            assert k.dtype == np.float32 and k.shape == (size, size) and (k >= 0).all()
            assert abs(float(k.astype(np.float64).sum()) - 1.0) < 1e-6
            ax = np.arange(size) - size // 2
            cy, cx = float((k.sum(axis=1) * ax).sum()), float((k.sum(axis=0) * ax).sum())
            assert abs(cy) <= 0.5 and abs(cx) <= 0.5, (size, seed, cy, cx)
            assert not np.array_equal(k, k[::-1, ::-1])
            np.testing.assert_array_equal(k, psf.motion_psf(size, seed))           # seeded
        assert not np.array_equal(psf.motion_psf(size, 0), psf.motion_psf(size, 1))
    d = psf.disk_psf(31, 7.5)
    assert d.dtype == np.float32 and d.shape == (31, 31) and (d >= 0).all() and abs(float(d.astype(np.float64).sum()) - 1.0) < 1e-6
    np.testing.assert_array_equal(d, d[::-1, ::-1]); np.testing.assert_array_equal(d, d.T)
    assert d[15, 15] == d.max() and d[15, 15 + 6] == d.max() and d[15, 15 + 9] == 0 and d[0, 0] == 0
    assert abs(float(np.count_nonzero(d)) - np.pi * 7.5 ** 2) < 0.35 * np.pi * 7.5 ** 2
    for bad in (0, 4, -3):
        with pytest.raises(ValueError):
            psf.motion_psf(bad)
    with pytest.raises(ValueError):
        psf.disk_psf(9, 0.0)


def test_load_psf(tmp_path):
    from pnpflow_amd import psf
    k = P.psf_kernel(9)
    np.save(tmp_path / "k.npy", k.astype(np.float64))
    got = psf.load_psf(str(tmp_path / "k.npy"))
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, k)
    np.save(tmp_path / "bad.npy", np.ones(5))
    with pytest.raises(ValueError, match="2-D"):
        psf.load_psf(str(tmp_path / "bad.npy"))


def test_make_degradation_and_problem_names(tmp_path):
    import inspect
    import main as M
    import pnpflow_amd._lib as L
    from pnpflow_amd import psf
    assert list(inspect.signature(M.make_degradation).parameters)[:5] == ["problem", "dim_image", "num_channels", "noise_type", "device"]
    for dim, size in ((128, 31), (256, 61)):
        for noise, sn in (("gaussian", 0.05), ("laplace", 0.3)):
            d, s = M.make_degradation("psf_deblurring_FFT", dim, 3, noise, "cpu")
            assert type(d).__name__ == "PSFDeblurring" and d.kind == L.PF_DEG_PSF_BLUR and s == sn
            assert d.kernel_size <= size and d.dim_image == dim
            np.testing.assert_array_equal(d.taps_host.sum(), np.float32(psf.motion_psf(size, 0).sum()))
            d, s = M.make_degradation("psf_deblurring", dim, 3, noise, "cpu")
            assert d.kind == L.PF_DEG_PSF_BLUR_ZERO and d.mode != "fft" and s == sn
    d, _ = M.make_degradation("psf_deblurring", 128, 3, "gaussian", "cpu", psf="disk", psf_size=9)
    np.testing.assert_array_equal(d.taps_host, psf.disk_psf(9, 4.0))
    a, _ = M.make_degradation("psf_deblurring", 128, 3, "gaussian", "cpu", psf_size=21, psf_seed=0)
    b, _ = M.make_degradation("psf_deblurring", 128, 3, "gaussian", "cpu", psf_size=21, psf_seed=5)
    assert not np.array_equal(a.taps_host, b.taps_host)
    np.save(tmp_path / "k.npy", P.psf_kernel(9))
    d, _ = M.make_degradation("psf_deblurring_FFT", 128, 3, "gaussian", "cpu", psf=str(tmp_path / "k.npy"))
    np.testing.assert_array_equal(d.taps_host, P.psf_kernel(9))
    # the Gaussian problems are what they were
    g, _ = M.make_degradation("gaussian_deblurring_FFT", 128, 3, "gaussian", "cpu")
    assert g.kind == L.PF_DEG_GAUSSIAN_BLUR


def test_pnp_gs_problem_rules():
    from pnpflow_amd.methods.pnp_gs import PROX_PNP
    from pnpflow_amd.utils import CfgNode
    mk = lambda algo, problem: PROX_PNP.__new__(PROX_PNP).__class__.algo_code(type("S", (), {"args": CfgNode(dict(algo=algo, problem=problem))})())
    assert mk("hqs", "psf_deblurring_FFT") == 2 == mk("hqs", "gaussian_deblurring_FFT")
    assert mk("pgd", "psf_deblurring") == 0 == mk("pgd", "psf_deblurring_FFT")
    with pytest.raises(ValueError, match="pgd"):
        mk("hqs", "psf_deblurring")
    with pytest.raises(ValueError, match="pgd"):
        mk("hqs", "gaussian_deblurring")


# ---- 3. the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_kinds_and_the_spectrum_entry_point():
    import __graft_entry__ as G
    import pnpflow_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "pnpflow_hip.h")).read()
    assert re.search(r"PF_DEG_PSF_BLUR\s*=\s*7\b", hdr) and re.search(r"PF_DEG_PSF_BLUR_ZERO\s*=\s*8\b", hdr)
    assert re.search(r"#define\s+PF_ABI_VERSION\s+6\b", hdr)          # additive: the layout of pf_degradation is what it was
    assert (L.PF_ABI_VERSION, L.PF_DEG_PSF_BLUR, L.PF_DEG_PSF_BLUR_ZERO, L.PSF_MAX_SIDE) == (6, 7, 8, 63)
    assert re.search(r"\bpf_psf_power_spectrum\s*\(", hdr) and "pf_psf_power_spectrum" in L.SIGNATURES
    assert [f[0] for f in L.PfDegradation._fields_] == ["kind", "half_size_mask", "sf", "ntaps", "mask", "taps"]
    common = open(os.path.join(ROOT, "pnpflow_amd", "csrc", "deg_rules.h")).read()
    assert re.search(r"DEG_PSF_BLUR\s*=\s*7\b", common) and re.search(r"DEG_PSF_BLUR_ZERO\s*=\s*8\b", common)
    assert "psf.hip" in G.SOURCES
    lib = L.load()
    assert lib.pf_abi_version() == 6 and hasattr(lib, "pf_psf_power_spectrum")
