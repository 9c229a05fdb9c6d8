"""Fixtures of superresolution through a blur kernel (PF_DEG_PSF_SR: y = (k (*) x) decimated by sf) from the REAL reference on the CPU.

Run in the build container only:   python tools/make_golden_sr_blur.py [op] [pnp] [ot_ode] [pnp_gs]
Writes data only, under tests/golden/.  The operator is the reference's own Superresolution(2, 64, mode="bicubic") object with `.filter` replaced by
the rolled, zero-padded PSF (its H / H_adj read nothing else: degradations.py:113-127).  PSF: pnpflow_amd.psf.motion_psf(9, 0); net tiny4 (64^2,
C = 3); sf 2; B = 2.  The loops are the generators of tools/make_golden_spatial.py and tools/make_golden_pnp_gs.py, handed a degradations module
whose GaussianDeblurring builds that object; every fixture stores the PSF and sf.

  sr_blur_op.npz                 clean (one image), H(clean), H_adj(H(clean)) - checked against the fp64 direct sums of tests/sr_blur_restatement.py - and
                                 the measurement noisy = H(clean) + sigma n with its sigma
  pnp_traj_sr_blur.npz           PNP_FLOW.solve_ip, 10 x 2, Gaussian noise; iterates 0 / 1 / 4 / 9
  ot_ode_traj_sr_blur.npz        OT_ODE.solve_ip with the problem name superresolution_blur: the reference has no branch for it and takes its GMRES
                                 path (ot_ode.py:119-127).  Stores the Krylov vectors of every solve - the tool fails unless every solve stops on its
                                 tolerance below the cap of 100 - and dist_fp64 / dist_fp64_last, the distance (relative to max|iterate|) of the stored
                                 first two iterates / of the last one from an fp64 rerun with the closed-form solve on the low-resolution grid, each
                                 of which must stay under a quarter of the engine test's 1e-3
  pnp_gs_tiny4_hqs_sr_blur.npz   PROX_PNP.solve_ip, algo hqs, problem superresolution_bicubic: the reference's own loop body (pnp_gs.py:180-200)
                                 with prox_datafit replaced on the class by the exact proximal map (torch FFTs; the reference's :45-76 is not one),
                                 in the format of pnp_gs_tiny4_hqs_psf_fft.npz (iterates entering every iteration, jn_max, growth from the fp64 rerun)
"""
import os
import shutil
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden as MG  # noqa: E402
import make_golden_spatial as MS  # noqa: E402
from make_golden import CFGS, OUT, det_image, det_normal  # noqa: E402
from make_golden_psf import rehome, with_out  # noqa: E402
import sr_blur_restatement as S  # noqa: E402
from oracle import pnpflow_oracle as O  # noqa: E402
from pnpflow_amd.psf import motion_psf  # noqa: E402

SF, SIDE = 2, 64
PSF = motion_psf(9, 0)


def sr_object(degr, kernel=PSF, sf=SF, dim_image=SIDE):
    """the reference's Superresolution(sf, dim, mode="bicubic") carrying `kernel` in `.filter`"""
    d = degr.Superresolution(sf, dim_image, mode="bicubic", device="cpu")
    K = kernel.shape[0]
    f = torch.zeros((1, 3, dim_image, dim_image))
    f[..., :K, :K] = torch.from_numpy(np.ascontiguousarray(kernel, dtype=np.float32))
    d.filter = torch.roll(f, shifts=(-(K - 1) // 2, -(K - 1) // 2), dims=(2, 3))      # degradations.py:103-109
    return d


def degr_with(degr):
    ns = types.SimpleNamespace(**{n: getattr(degr, n) for n in dir(degr) if not n.startswith("_")})
    ns.GaussianDeblurring = lambda *a, **k: sr_object(degr)
    return ns


def renamed_problem(cls, name):
    """the reference's solver class with a constructor that writes `name` into the generator's problem field; returns the constructor to put back"""
    real = cls.__init__

    def init(self, model, device, args):
        args.problem = name
        real(self, model, device, args)
    cls.__init__ = init
    return real


EXTRA = dict(psf=PSF, sf=np.array(SF))


def gen_op(degr):
    d = sr_object(degr)
    x = det_image((2, 3, SIDE, SIDE), 31)[:1]
    h = d.H(x); ha = d.H_adj(h)
    for got, ref in ((h, S.H64(x.numpy(), PSF, SF)), (ha, S.Hadj64(h.numpy(), PSF, SF))):
        err = float(np.abs(got.numpy() - ref).max())
        assert got.shape == ref.shape and err < 5e-6, err
    w = det_normal(tuple(h.shape), 32)
    lhs, rhs = float((h.double() * w.double()).sum()), float((x.double() * d.H_adj(w).double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * float((h * w).abs().sum()), (lhs, rhs)
    sigma = 0.05
    noisy = h + sigma * det_normal(tuple(h.shape), 33)
    path = os.path.join(OUT, "sr_blur_op.npz")
    np.savez_compressed(path, clean=x.numpy(), noisy=noisy.numpy(), sigma=np.array(sigma), H=h.numpy(), Hadj=ha.numpy(), **EXTRA)
    print("sr_blur_op.npz", os.path.getsize(path), "bytes")


def gen_pnp(models, degr, utils, pnp):
    real = renamed_problem(pnp.PNP_FLOW, "superresolution_blur")
    try:
        tmp = with_out([MS], lambda: MS.gen_pnp(models, degr_with(degr), utils, pnp))
    finally:
        pnp.PNP_FLOW.__init__ = real
    rehome(tmp, "pnp_traj_zero_blur.npz", "pnp_traj_sr_blur.npz", EXTRA)          # the generator's Gaussian-noise case
    shutil.rmtree(tmp)


def gen_ot_ode(models, degr, utils):
    import pnpflow.methods.ot_ode as ot
    real = renamed_problem(ot.OT_ODE, "superresolution_blur")
    try:
        tmp = with_out([MS], lambda: MS.gen_ot_ode(models, degr_with(degr), utils))      # asserts 0 < Krylov vectors < 100 for every solve
    finally:
        ot.OT_ODE.__init__ = real
    g = np.load(os.path.join(tmp, "ot_ode_traj_zero_blur.npz"))
    steps, t0, sigma, first = int(g["steps"]), float(g["start_time"]), float(g["sigma"]), int(g["first"])
    cfg = O.unet_config(**CFGS["tiny4"])
    sd = O.synthetic_state_dict(cfg, 0)
    its = {}
    S.ot_ode_restore64(sd, cfg, S.SrBlur(PSF, SF, 3, SIDE), torch.from_numpy(g["noisy"]), sigma, steps, t0, det_normal((2, 3, SIDE, SIDE), 61, 1),
                       record=lambda it, x: its.__setitem__(it, x.numpy()))
    rel = {it: float(np.abs(g[f"x_it{it}"] - its[it]).max() / np.abs(its[it]).max()) for it in (first, first + 1, steps - 1)}
    dist = max(rel[first], rel[first + 1])
    assert rel[steps - 1] < 0.25 * 1e-3, rel
    print("ot_ode sr_blur: Krylov vectors", g["gmres_vectors"].tolist(), "fp32 GMRES trajectory vs fp64 closed form, relative:", rel)
    assert dist < 0.25 * 1e-3, rel
    rehome(tmp, "ot_ode_traj_zero_blur.npz", "ot_ode_traj_sr_blur.npz", dict(EXTRA, dist_fp64=np.array(dist), dist_fp64_last=np.array(rel[steps - 1])))
    shutil.rmtree(tmp)


def exact_prox(self, x, y, H, H_adj, degradation=None, alpha=None):
    """argmin_u alpha/2 |H u - y|^2 + 1/2 |u - x|^2 by the Woodbury identity on the low-resolution grid"""
    r = x + alpha * H_adj(y)
    k2 = torch.fft.fft2(degradation.filter.to(x.dtype)).abs() ** 2
    sf, D = degradation.sf, k2.shape[-1]
    lam = k2.reshape(1, k2.shape[1], sf, D // sf, sf, D // sf).sum(dim=(2, 4)) / sf ** 2
    sol = torch.real(torch.fft.ifft2(torch.fft.fft2(H(r)) / (alpha * lam + 1.0)))
    return r - alpha * H_adj(sol)


def gen_pnp_gs(models, degr, utils):
    import make_golden_pnp_gs as PG
    PG._stub("skimage").io = PG._stub("skimage.io")
    PG._stub("torchmetrics.image", PeakSignalNoiseRatio=lambda **k: types.SimpleNamespace(to=lambda d: None))
    import pnpflow.methods.pnp_gs as pg
    import pnpflow.train_denoiser as td
    m, cfg, sd = PG.build_ref_unet(models, "tiny4")
    m64, _, _ = PG.build_ref_unet(models, "tiny4"); m64 = m64.double()
    clean = det_image((PG.B, 3, SIDE, SIDE), PG.CLEAN_SEED)
    sigma, emb = 0.05, models.get_sinusoidal_positional_embedding
    saved = pg.PROX_PNP.prox_datafit
    pg.PROX_PNP.prox_datafit = exact_prox
    try:
        r32 = PG.run_case(pg, td, utils, m, "hqs", "superresolution_bicubic", "gaussian", sr_object(degr), sigma, clean, torch.float32, PG.NOISE_SEED)
        models.get_sinusoidal_positional_embedding = lambda t, dim: emb(t, dim).double()
        try:
            r64 = PG.run_case(pg, td, utils, m64, "hqs", "superresolution_bicubic", "gaussian", sr_object(degr), sigma, clean, torch.float64, PG.NOISE_SEED)
        finally:
            models.get_sinusoidal_positional_embedding = emb
    finally:
        pg.PROX_PNP.prox_datafit = saved
    assert r32["alpha_prox"] == [PG.ALPHA] * PG.MAX_ITER            # alpha never decays
    xs = [x.float() for x in r32["iterates"]]
    spread = [float((a.double() - b.double()).abs().max() / b.double().abs().max()) for a, b in zip(r32["iterates"], r64["iterates"])]
    eps, growth = float(np.finfo(np.float32).eps), 1.0
    for k in range(2, len(spread)):
        growth = max(growth, max(spread[k], eps) / max(spread[k - 1], eps))
    assert growth ** 2 * 2e-4 <= 0.05, (growth, spread)
    # every stored step is the exact prox: optimality of x_{k+1} against its z cannot be checked without Dg, but the first iterate is H_adj(noisy)
    d = sr_object(degr)
    assert float((xs[0] - d.H_adj(r32["noisy"])).abs().max()) == 0.0
    out = dict(sigma=np.array(sigma), noise_seed=np.array(PG.NOISE_SEED), alpha=np.array([PG.ALPHA] * (PG.MAX_ITER + 1)), noisy=r32["noisy"].numpy(),
               iterates=torch.stack(xs).numpy(), jn_max=np.array(r32["jn_max"]), growth=np.array(growth), spread=np.array(spread), **EXTRA)
    assert all(np.isfinite(v).all() for v in out.values())
    path = os.path.join(OUT, "pnp_gs_tiny4_hqs_sr_blur.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 460 * 1024, os.path.getsize(path)
    print("pnp_gs hqs sr_blur growth %.2f" % growth, "spread", ["%.1e" % s for s in spread], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    which = sys.argv[1:] or ["op", "pnp", "ot_ode", "pnp_gs"]
    os.makedirs(OUT, exist_ok=True)
    models, degr, utils, pnp = MG.import_reference()
    if "op" in which:
        gen_op(degr)
    if "pnp" in which:
        gen_pnp(models, degr, utils, pnp)
    if "ot_ode" in which:
        gen_ot_ode(models, degr, utils)
    if "pnp_gs" in which:
        gen_pnp_gs(models, degr, utils)
