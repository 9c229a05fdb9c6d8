"""Generate tests/golden/pnp_gs_tiny4_*.npz by running the REAL reference PROX_PNP.solve_ip (pnpflow/methods/pnp_gs.py) on its
GRADIENT_STEP_DENOISER (pnpflow/train_denoiser.py) here, on CPU.

Run in the build container only:   python tools/make_golden_pnp_gs.py
Net: the 4-level test U-Net `tiny4` (64x64, synthetic weights of oracle/pnpflow_oracle.py), B = 2, max_iter 3, alpha 0.5, lr_pnp 1,
sigma_factor 1.  Replaced, in the style of tools/make_golden_dflow.py:
  * the absent skimage and torchmetrics.image (imported at module top by train_denoiser.py, unused at inference) -> empty stubs;
  * torch.randn_like -> det_normal(NOISE_SEED, call index); torch.distributions.laplace.Laplace(loc, scale).sample() ->
    loc + scale * det_laplace(NOISE_SEED, 0);
  * the metric functions -> capture of the final image.
The denoiser's calculate_grad, and the solver's grad_datafit, prox_datafit and objective are wrapped to record the iterate entering
every iteration, the alpha each prox sees and the two objective values of every backtracking test.
Every case runs a second time in fp64 (model.double(), the time embedding cast to double, Tensor.float mapped to double for the
`x.float()` of calculate_grad): `growth` is the largest ratio of successive max|x32_k - x64_k| / max|x64_k| over the stored iterates
k >= 1 (those that have been through the net; see gen), floored at 1 - the factor by which the synthetic-weight net (no contraction)
amplifies a rounding-level perturbation per iteration.
The fixtures hold numeric arrays only.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ref_import import import_reference, _stub  # noqa: E402
from make_golden import OUT, build_ref_unet, det_image, det_normal, CFGS  # noqa: E402
from pnp_gs_restatement import det_laplace  # noqa: E402

torch.set_num_threads(8)

CLEAN_SEED, NOISE_SEED, GRAD_SEED = 33, 75, 77
B, MAX_ITER, ALPHA, LR_PNP, SIGMA_FACTOR = 2, 3, 0.5, 1.0, 1.0
# per-case measurement-noise seeds where the default fails the tool's conditions: the Laplace data term's gradient is a sign, so a residual
# that sits within rounding of zero at some pixel flips between the fp32 and the fp64 run and the spread jumps by 2 lr / sigma
NOISE_SEEDS = {"pgd_laplace_denoising": 92, "pgd_laplace_inpainting": 76}
GRAD_SIGMA = (0.05, 0.2)        # two different denoiser levels in the calculate_grad golden


def cases(degr, S):
    # (name, algo, problem, noise_type, (degradation, sigma_noise of the reference's main.py table))
    return [("pgd_denoising", "pgd", "denoising", "gaussian", lambda: (degr.Denoising(), 0.2)),
            ("pgd_inpainting", "pgd", "inpainting", "gaussian", lambda: (degr.BoxInpainting(10), 0.05)),
            ("pgd_superresolution", "pgd", "superresolution", "gaussian", lambda: (degr.Superresolution(4, S, device="cpu"), 0.05)),
            ("pgd_gaussian_deblurring_FFT", "pgd", "gaussian_deblurring_FFT", "gaussian",
             lambda: (degr.GaussianDeblurring(1.0, 61, "fft", 3, S, device="cpu"), 0.05)),
            ("pgd_laplace_denoising", "pgd", "denoising", "laplace", lambda: (degr.Denoising(), 0.3)),
            ("pgd_laplace_inpainting", "pgd", "inpainting", "laplace", lambda: (degr.BoxInpainting(10), 0.3)),
            ("hqs_random_inpainting", "hqs", "random_inpainting", "gaussian", lambda: (degr.RandomInpainting(0.7), 0.01)),
            ("hqs_gaussian_deblurring_FFT", "hqs", "gaussian_deblurring_FFT", "gaussian",
             lambda: (degr.GaussianDeblurring(1.0, 61, "fft", 3, S, device="cpu"), 0.05))]


def fake_laplace(noise_seed):
    class FakeLaplace:
        def __init__(self, loc, scale):
            self.loc, self.scale = loc, scale

        def sample(self):
            return self.loc + self.scale * det_laplace(tuple(self.loc.shape), noise_seed, 0).to(self.loc.dtype)
    return FakeLaplace


def run_case(pg, td, utils, model, algo, problem, noise_type, degradation, sigma, clean, dtype, noise_seed):
    """One solve_ip of the reference; returns the record."""
    S = clean.shape[-1]
    args = utils.CfgNode(dict(method="pnp_gs", model="gradient_step", dataset="celeba", problem=problem, noise_type=noise_type, algo=algo,
                              max_iter=MAX_ITER, lr_pnp=LR_PNP, alpha=ALPHA, sigma_factor=SIGMA_FACTOR, max_batch=1, dim_image=S, num_channels=3,
                              lr=1e-4, batch=0, save_path_ip="/tmp", eval_split="test"))
    den = td.GRADIENT_STEP_DENOISER(model, torch.device("cpu"), args)
    solver = pg.PROX_PNP(den, torch.device("cpu"), args)
    rec = {"enter": [], "grad_in": [], "jn_max": [], "alpha_prox": [], "obj": [], "final": None, "noisy": None}
    seq = {"n": 0}

    def fake_randn_like(like, **kw):
        i = seq["n"]; seq["n"] += 1
        return det_normal(tuple(like.shape), noise_seed, i).to(like.dtype)

    calc = den.calculate_grad

    def rec_calc(x, sigma_, compute_g=False):
        out = calc(x, sigma_, compute_g=compute_g)
        xin = x.detach().clone()
        rec["grad_in"].append(xin)
        rec["jn_max"].append(float((xin - out[1].detach() - out[0].detach()).abs().max()))
        return out
    den.calculate_grad = rec_calc
    gdf, prox, obj = solver.grad_datafit, solver.prox_datafit, solver.objective

    def rec_gdf(x, y, H, H_adj):
        rec["enter"].append(x.detach().clone())
        return gdf(x, y, H, H_adj)

    def rec_prox(x, y, H, H_adj, degradation=None, alpha=None):
        rec["alpha_prox"].append(alpha)
        return prox(x, y, H, H_adj, degradation, alpha)

    def rec_obj(*a):
        v = obj(*a)
        rec["obj"].append(float(v))
        return v
    solver.grad_datafit, solver.prox_datafit, solver.objective = rec_gdf, rec_prox, rec_obj

    def cap_psnr(clean_img, noisy_img, rec_img, a, H_adj, iter="final"):
        rec["noisy"] = noisy_img.detach().clone(); rec["final"] = rec_img.detach().clone(); rec["final_iter"] = iter
    noop = lambda *a, **k: None
    saved = (torch.randn_like, torch.distributions.laplace.Laplace, utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images,
             utils.compute_average_psnr, utils.compute_average_ssim, utils.compute_average_lpips, torch.Tensor.float)
    torch.randn_like = fake_randn_like
    torch.distributions.laplace.Laplace = fake_laplace(noise_seed)
    utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images = cap_psnr, noop, noop, noop
    utils.compute_average_psnr = utils.compute_average_ssim = utils.compute_average_lpips = noop
    if dtype == torch.float64:
        torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        solver.solve_ip([(clean.to(dtype), torch.zeros(B))], degradation, sigma)
    finally:
        (torch.randn_like, torch.distributions.laplace.Laplace, utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images,
         utils.compute_average_psnr, utils.compute_average_ssim, utils.compute_average_lpips, torch.Tensor.float) = saved
    assert rec["final_iter"] == MAX_ITER - 1            # the final metrics carry the last loop index
    assert args.lr_pnp == sigma ** 2 * LR_PNP           # multiplied in place
    # the iterate entering every iteration: grad_datafit's argument where pgd takes a gradient step, calculate_grad's otherwise
    enter = rec["enter"] if rec["enter"] else rec["grad_in"]
    assert len(enter) == MAX_ITER and len(rec["grad_in"]) == MAX_ITER
    rec["iterates"] = enter + [rec["final"]]
    return rec


def gen(models, degr, utils):
    _stub("skimage").io = _stub("skimage.io")
    _stub("torchmetrics.image", PeakSignalNoiseRatio=lambda **k: types.SimpleNamespace(to=lambda d: None))
    import pnpflow.methods.pnp_gs as pg
    import pnpflow.train_denoiser as td
    m, cfg, sd = build_ref_unet(models, "tiny4")
    m64, _, _ = build_ref_unet(models, "tiny4"); m64 = m64.double()
    c = CFGS["tiny4"]; S = c["input_height"]; shape = (B, c["input_channels"], S, S)
    clean = det_image(shape, CLEAN_SEED)
    assert float((clean[0] - clean[1]).abs().max()) > 0.1          # distinct per-image clean images
    emb = models.get_sinusoidal_positional_embedding

    # calculate_grad at one point with two different denoiser levels
    gargs = utils.CfgNode(dict(dim_image=S, num_channels=3, lr=1e-4))
    den = td.GRADIENT_STEP_DENOISER(m, torch.device("cpu"), gargs)
    xg = det_image(shape, GRAD_SEED) + 0.1 * det_normal(shape, GRAD_SEED, 1)
    Dg, N, g = den.calculate_grad(xg.clone(), torch.tensor(GRAD_SIGMA), compute_g=True)
    out = dict(sigma=np.array(GRAD_SIGMA, dtype=np.float32), Dg=Dg.detach().numpy(), N=N.detach().numpy(), g=np.array(float(g.detach())))
    assert all(np.isfinite(v).all() for v in out.values())
    path = os.path.join(OUT, "pnp_gs_tiny4_calculate_grad.npz")
    np.savez_compressed(path, **out)
    print("calculate_grad g", float(g), os.path.getsize(path), "bytes")

    for name, algo, problem, noise_type, mk in cases(degr, S):
        degradation, sigma = mk()
        seed = NOISE_SEEDS.get(name, NOISE_SEED)
        r32 = run_case(pg, td, utils, m, algo, problem, noise_type, degradation, sigma, clean, torch.float32, seed)
        models.get_sinusoidal_positional_embedding = lambda t, dim: emb(t, dim).double()
        try:
            degradation64, _ = mk()
            r64 = run_case(pg, td, utils, m64, algo, problem, noise_type, degradation64, sigma, clean, torch.float64, seed)
        finally:
            models.get_sinusoidal_positional_embedding = emb
        xs = [x.float() for x in r32["iterates"]]
        spread = [float((a.double() - b.double()).abs().max() / b.double().abs().max()) for a, b in zip(r32["iterates"], r64["iterates"])]
        # ratios between iterates that have been through the net: the initialisation is exact up to the rounding of the data in both runs, so
        # the step from it to x_1 injects the net's rounding afresh instead of amplifying an earlier error (the tests use the factor from
        # iteration 1 on: bound(k) = TOL growth^(k-1))
        eps = float(np.finfo(np.float32).eps)
        growth = 1.0
        for k in range(2, len(spread)):
            growth = max(growth, max(spread[k], eps) / max(spread[k - 1], eps))
        alphas = [ALPHA] * (MAX_ITER + 1)
        gaps = np.zeros((MAX_ITER, 2))
        if algo == "hqs" and problem == "gaussian_deblurring_FFT":
            assert len(r32["alpha_prox"]) == MAX_ITER and len(r32["obj"]) == 2 * MAX_ITER
            alphas = list(r32["alpha_prox"])
            for k in range(MAX_ITER):
                gap = r32["obj"][2 * k] - r32["obj"][2 * k + 1]
                thr = float(0.1 / alphas[k] * torch.linalg.norm(xs[k + 1] - xs[k]) ** 2)
                gaps[k] = (gap, thr)
                nxt = 0.9 * alphas[k] if gap < thr else alphas[k]
                if k + 1 < MAX_ITER:
                    assert nxt == alphas[k + 1], (k, nxt, alphas)
                else:
                    alphas.append(nxt)
                # the alpha decision cannot flip on rounding
                assert abs(gap - thr) >= 0.01 * max(abs(gap), abs(thr)), (name, k, gap, thr)
        out = dict(sigma=np.array(sigma), noise_seed=np.array(seed), alpha=np.array(alphas, dtype=np.float64), noisy=r32["noisy"].numpy(),
                   iterates=torch.stack(xs).numpy(), jn_max=np.array(r32["jn_max"]), gap=gaps, growth=np.array(growth), spread=np.array(spread))
        if problem == "random_inpainting":
            out["mask"] = np.random.RandomState(42).binomial(n=1, p=1 - 0.7, size=(B, S, S)).astype(np.uint8)
            assert np.array_equal(degradation.H(torch.ones(shape)).numpy(), np.broadcast_to(out["mask"][:, None], shape).astype(np.float32))
        assert all(np.isfinite(v).all() for v in out.values()), name
        if noise_type == "laplace":
            # the sign pattern of H(x_k) - y cannot flip on rounding: every residual of an iterate that has been through the net stays four times
            # the fp32-vs-fp64 distance of that iterate away from zero
            for k in range(1, MAX_ITER):
                margin = float((degradation.H(xs[k]) - r32["noisy"]).abs().min())
                dist = float((r32["iterates"][k].double() - r64["iterates"][k]).abs().max())
                if os.environ.get("PNP_GS_SEED_SEARCH"):
                    print(name, "seed", seed, "iterate", k, "margin %.2e" % margin, "4 x distance %.2e" % (4 * dist))
                assert margin >= 4 * dist or os.environ.get("PNP_GS_SEED_SEARCH"), (name, k, margin, dist)
        if os.environ.get("PNP_GS_SEED_SEARCH") and growth ** 2 * 2e-4 > 0.05:
            print(name, "seed", seed, "fails: growth", growth); continue
        assert growth ** 2 * 2e-4 <= 0.05, (name, growth, spread)
        path = os.path.join(OUT, f"pnp_gs_tiny4_{name}.npz")
        np.savez_compressed(path, **out)
        print(name, "alpha", alphas, "gap", gaps.tolist(), "growth %.2f" % growth, "spread", ["%.1e" % s for s in spread], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    models, degr, utils, _ = import_reference()
    gen(models, degr, utils)
