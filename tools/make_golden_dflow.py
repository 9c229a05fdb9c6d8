"""Generate tests/golden/d_flow_*.npz by running the REAL reference D_FLOW.solve_ip (pnpflow/methods/d_flow.py) here, on CPU.

Run in the build container only:   python tools/make_golden_dflow.py
Net: the 4-level test U-Net `tiny4` (64x64, synthetic weights of oracle/pnpflow_oracle.py), B = 2, lmbda 0.001, alpha 0.1, LBFGS_iter 3,
max_iter 2.  Three things are replaced, in the style of tools/make_golden.py gen_ot_ode:
  * inverse_flow_matching (the torchdiffeq dopri5 solve; torchdiffeq is not installed here and is stubbed) -> the latent
    det_normal(LATENT_SEED), so the fixtures pin the LBFGS stage alone;
  * torch.randn_like -> det_normal(NOISE_SEED, call index): call 0 the measurement noise, call 1 the blend noise;
  * the metric functions -> capture of the restored image.
torch.optim.LBFGS is wrapped to record the first closure's loss and z.grad (the reference's own value and gradient at the initial
latent) and the number of closure calls of every outer step; forward_flow_matching is wrapped to capture T(z) after every outer step
and the per-image loss at that step's latent.
The fixtures hold numeric arrays only; inputs are re-made by recipe (det_image / det_normal) in the tests.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ref_import import import_reference  # noqa: E402
from make_golden import OUT, build_ref_unet, det_image, det_normal, CFGS  # noqa: E402

torch.set_num_threads(8)

CLEAN_SEED, LATENT_SEED, NOISE_SEED = 31, 71, 73
B, LMBDA, ALPHA, LBFGS_ITER, MAX_ITER = 2, 0.001, 0.1, 3, 2


def cases(degr, S):
    return [("denoising", lambda: (degr.Denoising(), 0.2)),
            ("inpainting", lambda: (degr.BoxInpainting(10), 0.05)),
            ("superresolution", lambda: (degr.Superresolution(2, S, device="cpu"), 0.05)),
            ("gaussian_deblurring_FFT", lambda: (degr.GaussianDeblurring(1.0, 61, "fft", 3, S, device="cpu"), 0.05))]


def gen(models, degr, utils):
    stub = types.ModuleType("torchdiffeq")
    stub.odeint_adjoint = stub.odeint = None          # inverse_flow_matching is replaced below
    sys.modules.setdefault("torchdiffeq", stub)
    import pnpflow.methods.d_flow as dfl
    m, cfg, sd = build_ref_unet(models, "tiny4")
    c = CFGS["tiny4"]; S = c["input_height"]; shape = (B, c["input_channels"], S, S)
    for problem, mk in cases(degr, S):
        degradation, sigma = mk()
        clean = det_image(shape, CLEAN_SEED)
        args = utils.CfgNode(dict(method="d_flow", model="ot", dataset="celeba", problem=problem, steps_euler=6, lmbda=LMBDA, alpha=ALPHA,
                                  max_iter=MAX_ITER, LBFGS_iter=LBFGS_ITER, start_time=0.0, max_batch=1, compute_time=False, compute_memory=False,
                                  save_results=True, batch=0, save_path_ip="/tmp"))
        rec = {"calls": [], "loss0": None, "grad0": None, "restored": [], "noisy": None, "latents": []}
        seq = {"n": 0}

        def fake_randn_like(like, **kw):
            i = seq["n"]; seq["n"] += 1
            return det_normal(tuple(like.shape), NOISE_SEED, i)

        class RecLBFGS(torch.optim.LBFGS):
            def step(self, closure):
                n0 = len(rec["calls"])

                def wrapped():
                    loss = closure()
                    if rec["loss0"] is None:
                        rec["loss0"] = float(loss)
                        rec["grad0"] = self.param_groups[0]["params"][0].grad.detach().clone()
                    rec["calls"].append(1)
                    return loss
                out = super().step(wrapped)
                rec.setdefault("per_step", []).append(len(rec["calls"]) - n0)
                return out

        solver = dfl.D_FLOW(m, torch.device("cpu"), args)
        solver.inverse_flow_matching = lambda x: det_normal(tuple(x.shape), LATENT_SEED)
        fwd = solver.forward_flow_matching

        def cap_forward(z):
            out = fwd(z)
            if not z.requires_grad:
                rec["restored"].append(out.detach().clone())
                rec["latents"].append(z.detach().clone())
            return out
        solver.forward_flow_matching = cap_forward

        def cap_psnr(clean_img, noisy_img, rec_img, a, H_adj, iter="final"):
            rec["noisy"] = noisy_img.clone()
        noop = lambda *a, **k: None
        saved = (torch.randn_like, torch.optim.LBFGS, utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images,
                 utils.compute_average_psnr, utils.compute_average_ssim, utils.compute_average_lpips)
        torch.randn_like = fake_randn_like
        torch.optim.LBFGS = RecLBFGS
        utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images = cap_psnr, noop, noop, noop
        utils.compute_average_psnr = utils.compute_average_ssim = utils.compute_average_lpips = noop
        try:
            solver.solve_ip([(clean, torch.zeros(B))], degradation, sigma)
        finally:
            (torch.randn_like, torch.optim.LBFGS, utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images,
             utils.compute_average_psnr, utils.compute_average_ssim, utils.compute_average_lpips) = saved
        assert seq["n"] == 2 and len(rec["restored"]) == MAX_ITER + 1
        # the per-image value at the initial latent, with the reference's own building blocks (its closure returns only the sum)
        noisy = rec["noisy"]
        z0 = (np.sqrt(ALPHA) * det_normal(shape, LATENT_SEED) + np.sqrt(1 - ALPHA) * det_normal(shape, NOISE_SEED, 1)).detach()
        def per_image(z):
            with torch.no_grad():
                d = z.shape[1] * z.shape[2] * z.shape[3]
                nrm = solver.compute_norm(z)
                reg = 0.5 * torch.clamp(nrm ** 2, min=-1e6, max=1e6) - (d - 1) * torch.log(nrm + 1e-5)
                return torch.sum((degradation.H(fwd(z)) - noisy) ** 2, dim=(1, 2, 3)) + LMBDA * reg
        per = per_image(z0)
        assert abs(float(per.sum()) - rec["loss0"]) <= 1e-5 * abs(rec["loss0"]), (float(per.sum()), rec["loss0"])
        out = dict(sigma=np.array(sigma), lmbda=np.array(LMBDA), alpha=np.array(ALPHA), lbfgs_iter=np.array(LBFGS_ITER), noisy=noisy.numpy(),
                   loss0=np.array(rec["loss0"]), loss0_per_image=per.numpy(), grad0=rec["grad0"].numpy(),
                   calls_per_step=np.array(rec["per_step"]), restored_it1=rec["restored"][0].numpy(), restored_it2=rec["restored"][1].numpy(),
                   loss_it1=per_image(rec["latents"][0]).numpy(), loss_it2=per_image(rec["latents"][1]).numpy())
        path = os.path.join(OUT, f"d_flow_tiny4_{problem}.npz")
        np.savez_compressed(path, **out)
        print("d_flow", problem, "loss0", rec["loss0"], "calls", rec["per_step"], os.path.getsize(path), "bytes")


DOPRI_SEED = 41


def gen_dop853():
    """A tight solution of the flow ODE the dopri5 initialisation integrates (dx/dt = v(x, t), t 1 -> 0) on the tiny4 oracle net in fp64:
    scipy.integrate.solve_ivp(method='DOP853', rtol = atol = 1e-10).  Oracle-only (no reference code): the yardstick the dopri5 tests
    measure their distance to, since torchdiffeq itself is not installed here."""
    from scipy.integrate import solve_ivp
    from oracle import pnpflow_oracle as O
    c = CFGS["tiny4"]; S = c["input_height"]; shape = (B, c["input_channels"], S, S)
    cfg = O.unet_config(**c)
    sd = {k: v.double() for k, v in O.synthetic_state_dict(cfg, seed=0).items()}
    emb = O.sinusoidal_embedding
    O.sinusoidal_embedding = lambda t, dim: emb(t, dim).double()
    x0 = det_image(shape, DOPRI_SEED)
    nfev = [0]

    def f(t, y):
        nfev[0] += 1
        with torch.no_grad():
            v = O.unet_forward(sd, cfg, torch.from_numpy(y).view(shape), torch.full((B,), t, dtype=torch.float64))
        return v.reshape(-1).numpy()
    try:
        sol = solve_ivp(f, (1.0, 0.0), x0.double().reshape(-1).numpy(), method="DOP853", rtol=1e-10, atol=1e-10)
    finally:
        O.sinusoidal_embedding = emb
    assert sol.success, sol.message
    x = sol.y[:, -1].reshape(shape).astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "d_flow_dop853_tiny4.npz"), x=x, nfev=np.array(nfev[0]))
    print("dop853", nfev[0], "evaluations", float(np.abs(x).mean()))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    which = sys.argv[1:] or ["lbfgs", "dop853"]
    if "lbfgs" in which:
        models, degr, utils, _ = import_reference()
        gen(models, degr, utils)
    if "dop853" in which:
        gen_dop853()
