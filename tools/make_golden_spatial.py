"""Fixtures of the zero-boundary Gaussian blur (GaussianDeblurring with mode != "fft") from the REAL reference on the CPU.

Run in the build container only:   python tools/make_golden_spatial.py [op] [gmres] [gmres_paths] [pnp] [ot_ode]
Writes data only, under tests/golden/:
  zero_blur_op.npz        H (= H_adj) of det_image at 2 x 3 x 64 x 64 for blur sigma 1 and 3, K = 61
  zero_blur_gmres.npz     utils.GMRES on r_t^2 H H^T + sigma^2 I (cases of tests/zero_blur_restatement.py: max_iter 100 and 5), its iteration
                          counts, and the measured distance between that fp32 result and the fp64 restatement
  krylov_paths.npz        (target gmres_paths, only when named) utils.GMRES in fp32 on every case of tests/krylov_reference.py: its Krylov vector
                          counts and zero_blur_restatement.gmres64's, per image max|ref32 - exact fp64 solution| (capped cases: - gmres64's iterate
                          at the cap) and max|exact|.  Scalars and small integer arrays only; the right-hand sides are regenerated from seeds
  pnp_traj_zero_blur.npz / pnp_traj_laplace_zero_blur.npz     PNP_FLOW.solve_ip, tiny4, 10 x 2
  ot_ode_traj_zero_blur.npz                                   OT_ODE.solve_ip, tiny4, B = 2, 10 steps from 0.3, sigma 0.2, gamma constant: first
                          two iterates, last iterate, the Krylov vectors of every GMRES call (all below the cap of 100: asserted)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden as MG  # noqa: E402
from make_golden import CFGS, OUT, build_ref_unet, det_image, det_normal  # noqa: E402
import zero_blur_restatement as Z  # noqa: E402


def gen_op(degr):
    x = det_image((2, 3, 64, 64), 31)
    rec = {}
    for sig in (1.0, 3.0):
        d = degr.GaussianDeblurring(sig, 61, "spatial", 3, 64, "cpu")
        rec[f"blur{sig}_H"] = d.H(x).numpy(); rec[f"blur{sig}_Hadj"] = d.H_adj(x).numpy()
    np.savez_compressed(os.path.join(OUT, "zero_blur_op.npz"), **rec)
    print("op ok")


def gen_gmres(degr, utils):
    sig, K = Z.KRYLOV_BLUR
    B, C, H, W = Z.KRYLOV_SHAPE
    d = degr.GaussianDeblurring(sig, K, "spatial", C, 128, "cpu")       # (dim_image only sizes the circular mode's filter, which must hold the kernel)
    rhs = torch.from_numpy(Z.krylov_rhs())
    rt2 = torch.tensor(Z.KRYLOV_RT2, dtype=torch.float32)
    sigma_noise = 0.2
    assert abs(sigma_noise ** 2 - Z.KRYLOV_SIGMA2) < 1e-12
    taps = np.exp(-(np.arange(-K // 2 + 1.0, K // 2 + 1.0) ** 2) / (2 * sig ** 2))
    taps = taps / taps.sum()
    rec = dict(rhs=rhs.numpy(), rt2=rt2.numpy(), sigma2=np.array(sigma_noise ** 2))
    for tag, max_iter in (("A", 100), ("B", 5)):
        sols, its = [], []
        for i in range(B):
            def C_ope(z, i=i):        # ot_ode.py:121-124
                z = z.reshape(rhs.shape[1:]).unsqueeze(0)
                return (rt2[i].unsqueeze(0) * d.H(d.H_adj(z)) + sigma_noise ** 2 * z).reshape(-1)
            out = utils.GMRES(C_ope, rhs[i].reshape(-1), max_iter=max_iter)
            if isinstance(out, tuple):
                sols.append(out[0].reshape(rhs.shape[1:]).numpy()); its.append(out[1][0] + 1)
            else:                      # |b| < 1e-8: b itself (utils.py:995-996)
                sols.append(out.reshape(rhs.shape[1:]).numpy()); its.append(0)
        sol32 = np.stack(sols)
        sol64, its64 = Z.krylov_solve64(rhs.numpy(), taps, max_iter)
        dist = float(np.abs(sol32.astype(np.float64) - sol64).max())
        rec[f"sol_{tag}"] = sol32; rec[f"iters_{tag}"] = np.array(its); rec[f"iters64_{tag}"] = its64
        rec[f"dist_fp64_{tag}"] = np.array(dist); rec[f"solmax_{tag}"] = np.array(float(np.abs(sol64).max()))
        print(f"gmres case {tag}: iterations {its} (fp64 {its64.tolist()}), max|ref32 - fp64| = {dist:.3e}, max|sol| = {np.abs(sol64).max():.3e}")
    assert len(set(rec["iters_A"][:2].tolist())) == 2 and max(rec["iters_A"]) < 100 and rec["iters_A"][2] == 0
    np.savez_compressed(os.path.join(OUT, "zero_blur_gmres.npz"), **rec)


def ref_closures(degr, utils, name):
    """(H, H_adj) on (1, C, H, W) fp32 CPU tensors of image b -> closures(b): the reference's own degradation class where it has one for the case's
    operator, fp32 torch forms of the same operator otherwise"""
    import torch.nn.functional as F
    import krylov_reference as K
    c = K.CASES[name]
    B, C, Hh, Ww = c["shape"]
    kind = c["kind"]
    if kind == 0:
        d = degr.Denoising()
        return lambda b: (d.H, d.H_adj)
    if kind == 1:
        d = degr.BoxInpainting(c["half"])
        return lambda b: (d.H, d.H_adj)
    if kind == 2:            # RandomInpainting draws its own mask from the batch shape on every call: a given per-image mask has no class
        m = torch.from_numpy(K.mask_of(c).astype(np.float32))
        return lambda b: ((lambda x: m[b][None, None] * x),) * 2
    if kind == 6:            # (dim_image only sizes the circular mode's filter, which must hold the kernel)
        d = degr.GaussianDeblurring(c["blur"], 61, "spatial", C, 128, "cpu")
        return lambda b: (d.H, d.H_adj)
    if kind == 7 and Hh == Ww:      # the reference's circular pair with `.kernel` / `.filter` holding the PSF (make_golden_psf.py)
        k = torch.from_numpy(K.taps_of(c))
        Kk = k.shape[0]
        d = degr.GaussianDeblurring(1.0, Kk, "fft", C, Hh, "cpu")
        f = torch.zeros((1, C, Hh, Ww)); f[..., :Kk, :Kk] = k
        d.kernel = k; d.filter = torch.roll(f, shifts=(-(Kk - 1) // 2, -(Kk - 1) // 2), dims=(2, 3))
        return lambda b: (d.H, d.H_adj)
    if kind == 4:            # not square: the class's filter is dim x dim.  The same FFT pair on the reference's own 2-D kernel
        k = utils.gaussian_2d_kernel(c["blur"], 61)
        f = torch.zeros((1, C, Hh, Ww)); f[..., :61, :61] = k
        ff = torch.fft.fft2(torch.roll(f, shifts=(-30, -30), dims=(2, 3)))
        return lambda b: ((lambda x: torch.real(torch.fft.ifft2(torch.fft.fft2(x) * ff))), (lambda x: torch.real(torch.fft.ifft2(torch.fft.fft2(x) * torch.conj(ff)))))
    if kind == 8:            # the reference's spatial H_adj is the correlation again, not the adjoint of an asymmetric kernel: conv2d with the flipped kernel
        k = torch.from_numpy(K.taps_of(c))[None, None].repeat(C, 1, 1, 1)
        return lambda b: ((lambda x: F.conv2d(x, k, padding="same", groups=C)), (lambda x: F.conv2d(x, torch.flip(k, dims=(2, 3)), padding="same", groups=C)))
    raise ValueError(name)


def gen_gmres_paths(degr, utils):
    """tests/golden/krylov_paths.npz.  Asserts what tests/test_gpu_krylov_paths.py relies on, so that the reference alone satisfies each condition."""
    import krylov_reference as K
    rec = {}
    for name, c in K.CASES.items():
        B = c["shape"][0]
        rhs = torch.from_numpy(np.array(K.rhs(name)))
        rt2 = torch.from_numpy(K.rt2_of(name))
        sigma2 = float(np.float32(c["sigma2"]))
        closures = ref_closures(degr, utils, name)
        sols, its = [], []
        for i in range(B):
            Hf, Ha = closures(i)

            def C_ope(z, i=i, Hf=Hf, Ha=Ha):        # ot_ode.py:121-124
                z = z.reshape(rhs.shape[1:]).unsqueeze(0)
                return (rt2[i].unsqueeze(0) * Hf(Ha(z)) + sigma2 * z).reshape(-1)
            out = utils.GMRES(C_ope, rhs[i].reshape(-1), max_iter=c["max_iter"], tol=K.TOL, atol=K.ATOL)
            if isinstance(out, tuple):
                sols.append(out[0].reshape(rhs.shape[1:]).numpy()); its.append(out[1][0] + 1)
            else:                                    # |b| < 1e-8: b itself (utils.py:995-996)
                sols.append(out.reshape(rhs.shape[1:]).numpy()); its.append(0)
        sol32, its = np.stack(sols).astype(np.float64), np.array(its)
        sol64, its64 = K.gmres64(name)
        target = sol64 if c["capped"] else K.exact(name)
        per = lambda a: np.abs(a).reshape(B, -1).max(axis=1)
        dref, solmax = per(sol32 - target), per(target)
        ret = K.returns_rhs(name)
        dref[ret] = 0.0                              # (the right-hand side is returned: compared bit for bit, not with the solution)
        print(f"gmres_paths {name}: vectors {its.tolist()} (fp64 {its64.tolist()}), d_ref {['%.3e' % v for v in dref]}, max|sol| {['%.3e' % v for v in solmax]}")
        assert np.array_equal(its == 0, ret) and np.array_equal(its64 == 0, ret), (name, its, its64)
        if c["capped"]:
            assert (its == c["max_iter"]).all() and (its64 == c["max_iter"]).all(), (name, its, its64)
        else:
            assert its.max() < c["max_iter"] and its64.max() < c["max_iter"], (name, its, its64)
            if c["counts"]:
                assert np.abs(its - its64).max() <= 1, (name, its, its64)
        rec[f"{name}_iters32"], rec[f"{name}_iters64"], rec[f"{name}_dref"], rec[f"{name}_solmax"] = its, its64, dref, solmax
    assert sorted(rec) == K.fixture_keys()
    np.savez_compressed(os.path.join(OUT, "krylov_paths.npz"), **rec)


def gen_pnp(models, degr, utils, pnp):
    steps, num_samples, B, alpha = 10, 2, 2, 0.01
    for tag, laplace, sigma in (("zero_blur", False, 0.05), ("laplace_zero_blur", True, 0.3)):
        m, cfg, sd = build_ref_unet(models, "tiny4")
        S = CFGS["tiny4"]["input_height"]
        degradation = degr.GaussianDeblurring(1.0, 61, "spatial", 3, S, "cpu")
        clean = det_image((B, 3, S, S), 31)
        args = utils.CfgNode(dict(method="pnp_flow", model="ot", dataset="celeba", problem="gaussian_deblurring",
                                  noise_type="laplace" if laplace else "gaussian", num_samples=num_samples, steps_pnp=steps, lr_pnp=1.0,
                                  gamma_style="alpha_1_minus_t", alpha=alpha, max_batch=1, compute_time=False,
                                  compute_memory=False, save_results=True, batch=0, save_path_ip="/tmp"))
        iterates, seq = {}, {"n": 0}

        def fake_randn_like(like, **kw):
            i = seq["n"]; seq["n"] += 1
            return det_normal(tuple(like.shape), 41, i)   # call 0 = measurement noise, then (it, sample) order

        def fake_laplace_sample(self_, sample_shape=torch.Size()):
            seq["n"] += 1
            g = np.random.Generator(np.random.Philox(key=[41, 0]))
            u = torch.from_numpy(g.uniform(-0.5, 0.5, size=tuple(self_.loc.shape)).astype(np.float32))
            return self_.loc - self_.scale * torch.sign(u) * torch.log1p(-2 * u.abs())

        def cap_psnr(clean_img, noisy_img, rec_img, a, H_adj, iter="final"):
            iterates.setdefault(int(iter), rec_img.clone()); iterates["noisy"] = noisy_img.clone()
        noop = lambda *a, **k: None
        saved_lap = torch.distributions.laplace.Laplace.sample
        saved = (torch.randn_like, utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images,
                 utils.compute_average_psnr, utils.compute_average_ssim, utils.compute_average_lpips)
        torch.distributions.laplace.Laplace.sample = fake_laplace_sample
        torch.randn_like = fake_randn_like
        utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images = cap_psnr, noop, noop, noop
        utils.compute_average_psnr = utils.compute_average_ssim = utils.compute_average_lpips = noop
        try:
            pnp.PNP_FLOW(m, torch.device("cpu"), args).solve_ip([(clean, torch.zeros(B))], degradation, sigma)
        finally:
            (torch.randn_like, utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images,
             utils.compute_average_psnr, utils.compute_average_ssim, utils.compute_average_lpips) = saved
            torch.distributions.laplace.Laplace.sample = saved_lap
        assert seq["n"] == 1 + steps * num_samples
        rec = dict(steps=np.array(steps), num_samples=np.array(num_samples), alpha=np.array(alpha), sigma=np.array(sigma),
                   noisy=iterates["noisy"].numpy())
        for it in (0, 1, 4, 9):
            rec[f"x_it{it}"] = iterates[it].numpy()
        np.savez_compressed(os.path.join(OUT, f"pnp_traj_{tag}.npz"), **rec)
        print("pnp", tag, iterates[9].abs().mean().item())


def gen_ot_ode(models, degr, utils):
    import pnpflow.methods.ot_ode as ot
    steps, B, t0, sigma = 10, 2, 0.3, 0.2
    m, cfg, sd = build_ref_unet(models, "tiny4")
    S = CFGS["tiny4"]["input_height"]
    degradation = degr.GaussianDeblurring(1.0, 61, "spatial", 3, S, "cpu")
    clean = det_image((B, 3, S, S), 31)
    args = utils.CfgNode(dict(method="ot_ode", model="ot", dataset="celeba", problem="gaussian_deblurring", steps_ode=steps, start_time=t0,
                              gamma="constant", max_batch=1, compute_time=False, compute_memory=False, save_results=True, batch=0,
                              save_path_ip="/tmp"))
    iterates, seq, counts = {}, {"n": 0}, []

    def fake_randn_like(like, **kw):
        i = seq["n"]; seq["n"] += 1
        return det_normal(tuple(like.shape), 61, i)        # call 0: measurement noise, call 1: initialisation noise

    def cap_psnr(clean_img, noisy_img, rec_img, a, H_adj, iter="final"):
        iterates.setdefault(int(iter), rec_img.clone()); iterates["noisy"] = noisy_img.clone()
    real_gmres = utils.GMRES

    def counting_gmres(*a, **k):
        out = real_gmres(*a, **k)
        counts.append(out[1][0] + 1 if isinstance(out, tuple) else 0)
        return out
    noop = lambda *a, **k: None
    saved = (torch.randn_like, utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images,
             utils.compute_average_psnr, utils.compute_average_ssim, utils.compute_average_lpips)
    torch.randn_like = fake_randn_like
    utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images = cap_psnr, noop, noop, noop
    utils.compute_average_psnr = utils.compute_average_ssim = utils.compute_average_lpips = noop
    utils.GMRES = counting_gmres
    try:
        ot.OT_ODE(m, torch.device("cpu"), args).solve_ip([(clean, torch.zeros(B))], degradation, sigma)
    finally:
        (torch.randn_like, utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images,
         utils.compute_average_psnr, utils.compute_average_ssim, utils.compute_average_lpips) = saved
        utils.GMRES = real_gmres
    assert seq["n"] == 2
    first = int(steps * t0)
    counts = np.array(counts).reshape(steps - first, B)
    assert counts.max() < 100 and counts.min() > 0, counts        # every solve stopped on its tolerance, below the cap
    rec = dict(steps=np.array(steps), start_time=np.array(t0), sigma=np.array(sigma), noisy=iterates["noisy"].numpy(), first=np.array(first),
               gmres_vectors=counts)
    for it in (first, first + 1, steps - 1):
        rec[f"x_it{it}"] = iterates[it].numpy()
    np.savez_compressed(os.path.join(OUT, "ot_ode_traj_zero_blur.npz"), **rec)
    print("ot_ode zero_blur", iterates[steps - 1].abs().mean().item(), "Krylov vectors per (step, image):", counts.tolist())


if __name__ == "__main__":
    which = sys.argv[1:] or ["op", "gmres", "pnp", "ot_ode"]
    models, degr, utils, pnp = MG.import_reference()
    if "op" in which:
        gen_op(degr)
    if "gmres" in which:
        gen_gmres(degr, utils)
    if "gmres_paths" in which:
        gen_gmres_paths(degr, utils)
    if "pnp" in which:
        gen_pnp(models, degr, utils, pnp)
    if "ot_ode" in which:
        gen_ot_ode(models, degr, utils)
