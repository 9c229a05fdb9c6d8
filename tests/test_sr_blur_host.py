"""Host side of superresolution through a blur kernel (PSFSuperresolution, PF_DEG_PSF_SR = 9; the bicubic PF_DEG_SR_FILTERED on the same solves): the
ABI declarations, the Python surface and the problem table, and the math the GPU tests compare against - the tests' fp64 restatement
(tests/sr_blur_restatement.py) must satisfy the aliased-spectrum identity and the prox optimality condition on its own.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import psf_restatement as P
import sr_blur_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, C, H, W, sf, K) of tests/test_gpu_sr_blur.py
SHAPES = [(1, 1, 8, 8, 2, 5), (2, 3, 24, 40, 2, 9), (2, 2, 36, 60, 3, 7), (1, 3, 64, 64, 4, 17), (1, 2, 64, 128, 4, 63), (2, 1, 20, 24, 1, 9)]


def rnd(shape, seed):
    return np.random.Generator(np.random.Philox(key=[9300, seed])).standard_normal(size=shape)


# ---- 1. the math ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W,sf,K", SHAPES)
def test_restatement_adjoint_and_aliased_spectrum_identity(B, C, H, W, sf, K):
    """<H x, w> = <x, H_adj w>, and H H_adj = ifft2(fft2(.) lam) on the low-resolution grid, both to fp64 rounding"""
    k = P.psf_kernel(K).astype(np.float64)
    x, w = rnd((B, C, H, W), 1), rnd((B, C, H // sf, W // sf), 2)
    hx, hw = S.H64(x, k, sf), S.Hadj64(w, k, sf)
    assert hx.shape == w.shape and hw.shape == x.shape
    assert abs((hx * w).sum() - (x * hw).sum()) <= 1e-12 * np.abs(hx * w).sum()
    lam = S.aliased_spectrum64(k, H, W, sf)
    assert lam.shape == (H // sf, W // sf) and (lam >= 0).all()
    circ = np.real(np.fft.ifft2(np.fft.fft2(w) * lam))
    np.testing.assert_allclose(S.H64(hw, k, sf), circ, rtol=0, atol=1e-13 * max(1.0, np.abs(circ).max()))
    if sf == 1:
        np.testing.assert_allclose(hx, P.apply64(x, k, zero=False), rtol=0, atol=1e-14)
        np.testing.assert_allclose(lam, P.power_spectrum64(k, H, W), rtol=0, atol=1e-14)


@pytest.mark.parametrize("sf", [2, 4])
def test_restatement_identity_holds_for_the_even_bicubic_taps(sf):
    from pnpflow_amd.degradations import bicubic_taps
    w1 = bicubic_taps(sf).astype(np.float64)
    assert len(w1) == 4 * sf
    H = W = 16 * sf
    y = rnd((1, 2, H // sf, W // sf), 3)
    lam = S.aliased_spectrum64(w1, H, W, sf)
    circ = np.real(np.fft.ifft2(np.fft.fft2(y) * lam))
    np.testing.assert_allclose(S.H64(S.Hadj64(y, w1, sf), w1, sf), circ, rtol=0, atol=1e-13)
    # the separable fold the engine uses for kind 5: the sum of the products is the product of the folded factors
    p1 = np.abs(np.fft.fft(np.roll(np.concatenate([w1, np.zeros(H - len(w1))]), -(len(w1) // 2)))) ** 2
    f1 = p1.reshape(sf, H // sf).sum(axis=0)
    np.testing.assert_allclose(lam, np.outer(f1, f1) / sf ** 2, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("B,C,H,W,sf,K", SHAPES)
def test_restatement_prox_satisfies_the_optimality_condition(B, C, H, W, sf, K):
    """x = prox(z) minimises alpha/2 |H x - y|^2 + 1/2 |x - z|^2:  x + alpha H_adj(H x - y) = z"""
    k = P.psf_kernel(K).astype(np.float64)
    z, y = rnd((B, C, H, W), 4), rnd((B, C, H // sf, W // sf), 5)
    for alpha in (0.3, 1.0, 7.0):
        x = S.prox64(k, sf, z, y, alpha)
        res = x + alpha * S.Hadj64(S.H64(x, k, sf) - y, k, sf) - z
        assert np.abs(res).max() <= 1e-12 * max(1.0, np.abs(z).max()) * (1 + alpha), (alpha, np.abs(res).max())


def test_reference_prox_of_the_dead_branch_is_not_a_prox():
    """What pnp_gs.py:63-76 computes (its `below` multiplies the aliased power spectrum by the data spectrum), restated in numpy, misses the optimality
    condition by O(1) where the exact form meets it to rounding: why the engine does not reproduce it"""
    sf, H = 2, 16
    k = P.psf_kernel(5).astype(np.float64)
    z, y, alpha = rnd((1, 1, H, H), 6), rnd((1, 1, H // sf, H // sf), 7), 1.0
    f = np.zeros((H, H)); f[:5, :5] = k; f = np.roll(f, (-2, -2), axis=(0, 1))
    fk = np.fft.fft2(f)
    hat_z = S.Hadj64(y, k, sf) + z / alpha
    fz = np.fft.fft2(hat_z)
    fold = lambda a: a.reshape(a.shape[:-2] + (sf, H // sf, sf, H // sf)).mean(axis=(-4, -2))
    top, below = fold(fk * fz), fold(np.conj(fk) * fk * fz) + 1 / alpha
    sol = np.real(np.fft.ifft2(np.conj(fk) * np.tile(top / below, (sf, sf))))
    x_ref = (hat_z - sol) * alpha
    res = lambda x: np.abs(x + alpha * S.Hadj64(S.H64(x, k, sf) - y, k, sf) - z).max()
    assert res(x_ref) > 1e-2 and res(S.prox64(k, sf, z, y, alpha)) < 1e-12


def test_phase_counts_cover_every_tap_once():
    for K, sf in ((5, 2), (7, 3), (17, 4), (63, 4), (9, 1), (1, 2)):
        k = np.ones((K, K))
        c = S.phase_counts(k, sf)
        assert c.sum() == K * K and c.max() == (-(-K // sf)) ** 2


# ---- 2. the Python surface ---------------------------------------------------------------------------------------------------------------
def test_psf_superresolution_surface_and_sanitising():
    import pnpflow_amd._lib as L
    import pnpflow_amd.degradations as D
    k = P.psf_kernel(9)
    a = D.PSFSuperresolution(k, 2, 3, 64, "cpu")
    assert a.kind == L.PF_DEG_PSF_SR == 9 and a.sf == 2 and a.kernel_size == 9
    assert a.out_side(64) == 32 and D.PSFSuperresolution(k, 4, 3, 64, "cpu").out_side(64) == 16 and D.PSFSuperresolution(k, 1, 3, 64, "cpu").out_side(64) == 64
    np.testing.assert_array_equal(a.kernel.numpy(), k)
    # .filter is the reference's rolled (1, C, dim, dim) attribute, the layout PSFDeblurring has
    np.testing.assert_array_equal(a.filter.cpu().numpy(), P.PsfBlur(k, "fft", 3, 64).filter.numpy())
    np.testing.assert_array_equal(a.filter.cpu().numpy(), D.PSFDeblurring(k, "fft", 3, 64, "cpu").filter.cpu().numpy())
    assert tuple(a.filter.shape) == (1, 3, 64, 64) and float(a.filter[0, 0, 0, 0]) == float(k[4, 4])
    d = a.descriptor(2, 64, 64, "cpu")
    assert (d.kind, d.sf, d.ntaps) == (9, 2, 9) and d.taps
    # the same sanitising as PSFDeblurring: rectangular -> centred square, zero rings cropped, tensors accepted
    rect = np.arange(1, 16, dtype=np.float32).reshape(3, 5)
    sq = D.PSFSuperresolution(rect, 2, 1, 32, "cpu")
    np.testing.assert_array_equal(sq.taps_host, D.PSFDeblurring(rect, "fft", 1, 32, "cpu").taps_host)
    pad = np.zeros((13, 13), dtype=np.float32); pad[2:11, 2:11] = k
    c = D.PSFSuperresolution(pad, 2, 3, 64, "cpu")
    assert c.kernel_size == 9
    np.testing.assert_array_equal(c.taps_host, k)
    assert D.PSFSuperresolution(torch.from_numpy(k), 2, 3, 64, "cpu").kernel_size == 9
    for bad, msg in ((np.ones((4, 5)), "odd"), (np.ones((65, 65)), "63"), (np.ones(5), "2-D"), (np.ones((3, 3), dtype=complex), "real"),
                     (np.full((3, 3), np.nan), "finite")):
        with pytest.raises(ValueError, match=msg):
            D.PSFSuperresolution(bad, 2, 3, 64, "cpu")
    with pytest.raises(ValueError, match="fit"):
        D.PSFSuperresolution(P.psf_kernel(31), 2, 3, 16, "cpu")
    with pytest.raises(ValueError, match="divide"):
        D.PSFSuperresolution(k, 3, 3, 64, "cpu")
    for sf in (0, 9, 2.5):
        with pytest.raises(ValueError, match="sf"):
            D.PSFSuperresolution(k, sf, 3, 72, "cpu")
    # the reference's operator classes are still all that degradations defines itself
    assert "PSFSuperresolution" not in vars(D) or D.PSFSuperresolution.__module__.endswith("psf_superresolution")


def test_make_degradation_builds_both_problems(tmp_path):
    import main as M
    import pnpflow_amd._lib as L
    from pnpflow_amd import psf
    for dim, size, sf in ((128, 31, 2), (256, 61, 4)):
        for noise, sn in (("gaussian", 0.05), ("laplace", 0.3)):
            assert M.make_degradation("superresolution", dim, 3, noise, "cpu")[1] == sn
            d, s = M.make_degradation("superresolution_blur", dim, 3, noise, "cpu")
            assert type(d).__name__ == "PSFSuperresolution" and d.kind == L.PF_DEG_PSF_SR and s == sn and d.sf == sf and d.dim_image == dim
            np.testing.assert_array_equal(d.taps_host.sum(), np.float32(psf.motion_psf(size, 0).sum()))
            d, s = M.make_degradation("superresolution_bicubic", dim, 3, noise, "cpu")
            assert type(d).__name__ == "Superresolution" and d.kind == L.PF_DEG_SR_FILTERED and d.mode == "bicubic" and d.sf == sf and s == sn
    d, _ = M.make_degradation("superresolution_blur", 128, 3, "gaussian", "cpu", psf="disk", psf_size=9, sf=4)
    assert d.sf == 4
    np.testing.assert_array_equal(d.taps_host, psf.disk_psf(9, 4.0))
    np.save(tmp_path / "k.npy", P.psf_kernel(9))
    d, _ = M.make_degradation("superresolution_blur", 128, 3, "gaussian", "cpu", psf=str(tmp_path / "k.npy"))
    np.testing.assert_array_equal(d.taps_host, P.psf_kernel(9))
    assert M.make_degradation("superresolution", 128, 3, "gaussian", "cpu")[0].kind == L.PF_DEG_SUPERRESOLUTION      # what it was


def test_pnp_gs_algo_code_and_level_table():
    from pnpflow_amd.methods import pnp_gs
    from pnpflow_amd.methods.pnp_gs import PROX_PNP
    from pnpflow_amd.utils import CfgNode

    def solver(algo, problem):
        s = PROX_PNP.__new__(PROX_PNP)
        s.args = CfgNode(dict(algo=algo, problem=problem, max_iter=5, sigma_factor=1.5))
        return s
    for problem in ("superresolution_blur", "superresolution_bicubic"):
        assert solver("hqs", problem).algo_code() == 3 and solver("pgd", problem).algo_code() == 0
        tab = solver("hqs", problem).level_table(0.05)
        assert tab.dtype == np.float32 and list(tab) == [np.float32(2.0 * 0.05)] * 5          # pnp_gs.py:182-183
        assert list(solver("pgd", problem).level_table(0.05)) == [np.float32(1.5 * 0.05)] * 5
    assert solver("hqs", "gaussian_deblurring_FFT").algo_code() == 2 and solver("hqs", "random_inpainting").algo_code() == 1
    with pytest.raises(ValueError, match="not supported"):
        solver("hqs", "superresolution").algo_code()
    assert "superresolution_blur" in pnp_gs.SUPPORTED and "superresolution_bicubic" in pnp_gs.SUPPORTED
    assert "not a proximal map" in pnp_gs.__doc__


def test_python_prox_datafit_is_the_exact_prox():
    """PROX_PNP.prox_datafit for the new problems (torch FFTs, any device) against the fp64 restatement, with a CPU stand-in for the operator"""
    from pnpflow_amd.methods.pnp_gs import PROX_PNP
    from pnpflow_amd.utils import CfgNode
    k, sf, H = P.psf_kernel(5), 2, 16

    class Op:
        pass
    op = Op(); op.sf = sf
    f = torch.zeros((1, 2, H, H), dtype=torch.float64); f[:, :, :5, :5] = torch.from_numpy(k.astype(np.float64)); op.filter = torch.roll(f, (-2, -2), (2, 3))
    Hf = lambda x: torch.from_numpy(S.H64(x.numpy(), k, sf))
    Ha = lambda y: torch.from_numpy(S.Hadj64(y.numpy(), k, sf))
    s = PROX_PNP.__new__(PROX_PNP); s.args = CfgNode(dict(noise_type="gaussian", problem="superresolution_blur"))
    z, y = torch.from_numpy(rnd((1, 2, H, H), 8)), torch.from_numpy(rnd((1, 2, H // sf, H // sf), 9))
    got = s.prox_datafit(z, y, Hf, Ha, op, 0.8).numpy()
    np.testing.assert_allclose(got, S.prox64(k.astype(np.float64), sf, z.numpy(), y.numpy(), 0.8), rtol=0, atol=1e-12)


# ---- 3. the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_declares_kind_9_additively():
    import pnpflow_amd._lib as L
    hdr = open(os.path.join(ROOT, "include", "pnpflow_hip.h")).read()
    assert re.search(r"PF_DEG_PSF_SR\s*=\s*9\b", hdr)
    assert re.search(r"#define\s+PF_ABI_VERSION\s+6\b", hdr)          # additive: the layout of pf_degradation is what it was
    assert (L.PF_ABI_VERSION, L.PF_DEG_PSF_SR, L.PSF_MAX_SIDE, L.PSF_SR_MAX_SF) == (6, 9, 63, 8)
    assert [f[0] for f in L.PfDegradation._fields_] == ["kind", "half_size_mask", "sf", "ntaps", "mask", "taps"]
    for name in ("pf_sr_aliased_spectrum", "pf_sr_solve_scratch_floats", "pf_sr_prox"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in L.SIGNATURES
    common = open(os.path.join(ROOT, "pnpflow_amd", "csrc", "deg_rules.h")).read()
    assert re.search(r"DEG_PSF_SR\s*=\s*9\b", common) and re.search(r"PSF_SR_MAX_SF\s*=\s*8\b", common)
    lib = L.load()
    assert lib.pf_abi_version() == 6 and hasattr(lib, "pf_sr_prox")
    # the scratch rule of the low-resolution Fourier solve: 3 S + 3 S / sf^2 + 1 (alignment of the complex plane) + Hl Wl + max(H W, 2 (H + W) + 2) + B
    assert lib.pf_sr_solve_scratch_floats(2, 3, 64, 64, 2) == 3 * 24576 + 3 * 6144 + 1 + 32 * 32 + 64 * 64 + 2
    assert lib.pf_sr_solve_scratch_floats(0, 3, 64, 64, 2) == 0


# ---- 4. the fixtures ------------------------------------------------------------------------------------------------------------------
def test_fixtures_are_small_and_carry_the_psf(golden):
    from pnpflow_amd.psf import motion_psf
    for name in ("sr_blur_op", "pnp_traj_sr_blur", "ot_ode_traj_sr_blur", "pnp_gs_tiny4_hqs_sr_blur"):
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= 460 * 1024
        np.testing.assert_array_equal(golden(name)["psf"], motion_psf(9, 0))
        assert int(golden(name)["sf"]) == 2
    g = golden("ot_ode_traj_sr_blur")
    assert 0 < int(g["gmres_vectors"].min()) and int(g["gmres_vectors"].max()) < 100          # every solve of the reference stopped on its tolerance
    assert float(g["dist_fp64"]) < 0.25 * 1e-3 and float(g["dist_fp64_last"]) < 0.25 * 1e-3
    op = golden("sr_blur_op")
    np.testing.assert_allclose(op["H"], S.H64(op["clean"], op["psf"], 2), rtol=0, atol=5e-6)
    np.testing.assert_allclose(op["Hadj"], S.Hadj64(op["H"], op["psf"], 2), rtol=0, atol=5e-6)
    assert op["noisy"].shape == op["H"].shape and 0.5 * float(op["sigma"]) < float((op["noisy"] - op["H"]).std()) < 2 * float(op["sigma"])


def test_hqs_fixture_steps_are_the_exact_prox_schedule(golden):
    """the restatement of algo 3 (tests/sr_blur_restatement.hqs_iterate, oracle U-Net) reproduces the reference loop's stored iterates, teacher-forced"""
    from conftest import CFGS
    from oracle import pnpflow_oracle as O
    g = golden("pnp_gs_tiny4_hqs_sr_blur")
    cfg = O.unet_config(**CFGS["tiny4"])
    sd = O.synthetic_state_dict(cfg, 0)
    d = S.SrBlur(g["psf"], int(g["sf"]), 3, 64)
    its, noisy = torch.from_numpy(g["iterates"]), torch.from_numpy(g["noisy"])
    np.testing.assert_allclose(d.H_adj(noisy).numpy(), its[0].numpy(), atol=1e-5)
    xn, _ = S.hqs_iterate(lambda x, s: O.unet_forward(sd, cfg, x, s), d, its[0], noisy, float(g["sigma"]), 0.5)
    np.testing.assert_allclose(xn.numpy(), its[1].numpy(), atol=1e-4 * float(its[1].abs().max()))
