"""Generate tests/golden/flow_priors_*.npz.

Run in the build container only:   python tools/make_golden_flow_priors.py [pin] [steps] [free] [ncsnpp]

The reference's hut_estimator (pnpflow/utils.py:243-270) hard-codes device 'cuda' and cannot run here, so - as with
tools/make_golden_prior_eval.py - the fixtures come from the CPU restatement tests/flow_priors_restatement.py (exact double autograd on the
oracle, fp32 and fp64).  What CAN run here pins the restatement's first-order parts to the REAL reference first (`pin`): FLOW_PRIORS.solve_ip
(pnpflow/methods/flow_priors.py) on the `tiny4` reference U-Net for N = 3, K = 1, box inpainting, with utils.hut_estimator replaced by a zero
function in this process, torch.randn / torch.randn_like by the det_normal recipe and torch.autograd.grad / torch.optim.Adam wrapped to record the loss
value, the autograd gradient and the gradient handed to Adam (which carries grad_xt_lik from iteration 1 on).  The tool asserts that the
restatement with zero_trace=True reproduces every recorded loss, gradient and the final image (x_init, y_next, the data loss and grad_xt_lik all
enter them).

Single-step cases (B = 2, 3 x 64 x 64, N = 100, lmbda = 1000, eta = 0.01; flow_priors_restatement.CASES): per case g64, g_data64, g_trace64,
x_new64 (one outer iteration with K = 1, from x) as fp32, the maxima the tolerances need (pred_max, jtw_max, jteps_max, g_extra_max),
g32_err = max|g32 - g64|, trunc64[h] = max|fd64(h) - g_trace64| for h in FD_STEPS, and for laplace the indices of the residuals within
dt * TOL_fwd of zero.  Inputs are re-made from seeds by the tests.  The gate condition is checked on the reference alone: the share of pixels
with |g64| <= 4 TOL_g must be at most 0.5 % for every h in GATE_STEPS (otherwise: change the case's seed).
Free run: box inpainting, N = 24, K = 1, fp32 and fp64: final iterates, per-image PSNR, d32 (share of pixels where fp32 is further than eta / 2
from fp64), m32 (largest distance among the rest), fwd32_rel (the fp32 oracle's own forward error relative to max|v|), the largest max|pred|, and the iterates after the first outer
iteration (what the CPU test repeats).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pnpflow_oracle as O  # noqa: E402
import flow_priors_restatement as R  # noqa: E402

torch.set_num_threads(8)
OUT = os.path.join(ROOT, "tests", "golden")
TINY4 = dict(input_channels=3, input_height=64, ch=32, ch_mult=(1, 2, 4, 8), num_res_blocks=1, attn_resolutions=(16, 8))
NCSNPP_TINY = dict(image_size=32, nf=32, ch_mult=(1, 1, 2), num_res_blocks=2, attn_resolutions=(16,))
GATE_SHARE = 0.005
GATE_STEPS = (3e-3, 1e-2)       # the candidates for the default fd_step; 3e-2 (ten times the truncation error of 1e-2) is measured and printed only
D = torch.float64


def to64(d):
    return {k: v.double() for k, v in d.items()}


def pin_to_reference():
    from ref_import import import_reference
    from make_golden import build_ref_unet
    models, degr, utils, _ = import_reference()
    import pnpflow.methods.flow_priors as fp
    m, cfg, sd = build_ref_unet(models, "tiny4")
    Bn, S, N, seed, sigma = 2, 64, 3, 5, 0.05
    shape = (Bn, 3, S, S)
    clean = R.det_image(shape, seed)
    args = utils.CfgNode(dict(method="flow_priors", model="ot", dataset="celeba", problem="inpainting", noise_type="gaussian", N=N, K=1, lmbda=R.LMBDA,
                              eta=R.ETA, start_time=0.0, max_batch=1, compute_time=False, compute_memory=False, save_results=True, batch=0,
                              save_path_ip="/tmp"))
    rec = {"loss": [], "grad": [], "adam_grad": [], "final": None, "noisy": None}

    def cap_psnr(clean_img, noisy_img, rec_img, a, H_adj, iter="final"):
        rec["noisy"], rec["final"] = noisy_img.detach().clone(), rec_img.detach().clone()
    noop = lambda *a, **k: None
    real_grad, RealAdam = torch.autograd.grad, torch.optim.Adam

    def rec_grad(loss, x, **kw):
        out = real_grad(loss, x, **kw)
        rec["loss"].append(float(loss.detach())); rec["grad"].append(out[0].detach().clone())
        return out

    class RecAdam(RealAdam):
        def step(self, *a, **k):
            rec["adam_grad"].append(self.param_groups[0]["params"][0].grad.detach().clone())
            return super().step(*a, **k)
    saved = (torch.randn, torch.randn_like, torch.autograd.grad, torch.optim.Adam, utils.hut_estimator, utils.compute_psnr, utils.compute_ssim,
             utils.compute_lpips, utils.save_images, utils.compute_average_psnr, utils.compute_average_ssim, utils.compute_average_lpips)
    torch.randn = lambda *a, **k: R.det_normal(tuple(a[0]) if len(a) == 1 else tuple(a), seed, 1)
    torch.randn_like = lambda like, **k: R.det_normal(tuple(like.shape), seed, 3)
    torch.autograd.grad, torch.optim.Adam = rec_grad, RecAdam
    utils.hut_estimator = lambda NO_test, v, inp, t: torch.zeros(inp.shape[0])
    utils.compute_psnr, utils.compute_ssim, utils.compute_lpips, utils.save_images = cap_psnr, noop, noop, noop
    utils.compute_average_psnr = utils.compute_average_ssim = utils.compute_average_lpips = noop
    try:
        fp.FLOW_PRIORS(m, torch.device("cpu"), args).solve_ip([(clean, torch.zeros(Bn))], degr.BoxInpainting(10), sigma)
    finally:
        (torch.randn, torch.randn_like, torch.autograd.grad, torch.optim.Adam, utils.hut_estimator, utils.compute_psnr, utils.compute_ssim,
         utils.compute_lpips, utils.save_images, utils.compute_average_psnr, utils.compute_average_ssim, utils.compute_average_lpips) = saved
    assert len(rec["loss"]) == N and len(rec["adam_grad"]) == N
    op = O.BoxInpainting(10)
    x_init = R.det_normal(shape, seed, 1)
    y = op.H(clean) + R.det_normal(shape, seed, 3) * sigma
    assert torch.equal(y, rec["noisy"]), "the restatement's measurement differs from the reference's"
    vel = R.oracle_vel(sd, cfg)
    x = x_init.clone()
    for i in range(N):
        g, g_data, _, g_extra, _, info = R.grad(vel, op.H, x, x_init, y, None, i, N, R.LMBDA, zero_trace=True)
        tol = 1e-5 * float(rec["grad"][i].abs().max())
        loss = info["loss"] + (0.5 * float((x ** 2).sum()) if i == 0 else 0.0)          # the reference's loss carries the prior term on iteration 0
        assert abs(loss - rec["loss"][i]) <= 1e-5 * abs(rec["loss"][i]), (i, loss, rec["loss"][i])
        # iteration 0: the reference's autograd gradient contains the 0.5 x^2 term's x
        ref_auto = g_data + g_extra if i == 0 else g_data
        assert float((ref_auto - rec["grad"][i]).abs().max()) <= tol, (i, float((ref_auto - rec["grad"][i]).abs().max()), tol)
        assert float((g - rec["adam_grad"][i]).abs().max()) <= tol, (i, "grad_xt_lik")
        x = R.step(vel, op.H, x, x_init, y, [None], i, N, R.LMBDA, R.ETA, zero_trace=True)[0]
        print(f"pin iteration {i}: loss {loss:.6g} vs {rec['loss'][i]:.6g}, max|g - ref| {float((g - rec['adam_grad'][i]).abs().max()):.2e} (tol {tol:.2e})")
    err = float((x - rec["final"]).abs().max())
    print(f"pin final image: max|restatement - reference| {err:.2e}")
    assert err <= 2 * N * R.ETA * 1e-3 + 1e-5, err          # the sign steps agree but for isolated near-zero gradients


def single_step(name, case, vel32, vel64, prefix, S, half):
    op, noise_type, it, inp = R.case_inputs(case, S=S, half=half)
    i64 = to64(inp)
    lap = noise_type == "laplace"
    g32 = R.grad(vel32, op.H, inp["x"], inp["x_init"], inp["y"], inp["eps"], it, R.N_STEP, R.LMBDA, noise_type)
    g64 = R.grad(vel64, op.H, i64["x"], i64["x_init"], i64["y"], i64["eps"], it, R.N_STEP, R.LMBDA, noise_type)
    g, g_data, g_trace, g_extra, pred, info = g64
    num_t, dt = info["num_t"], info["dt"]
    x_new = R.step(vel64, op.H, i64["x"], i64["x_init"], i64["y"], [i64["eps"]], it, R.N_STEP, R.LMBDA, R.ETA, noise_type)[0]
    c = R.LMBDA if lap else 2 * R.LMBDA
    w = op.H_adj(c * (torch.sign(info["r"]) if lap else info["r"]))
    jtw = R.vjp(vel64, i64["x"], num_t, w)
    assert float((w + dt * jtw - g_data).abs().max()) <= 1e-9 * float(g_data.abs().max()), "g_data is not w + dt J^T w"
    jte = R.vjp(vel64, i64["x"], num_t, i64["eps"])
    trunc = [float((R.fd_grad_trace(vel64, i64["x"], i64["eps"], it, R.N_STEP, h) - g_trace).abs().max()) for h in R.FD_STEPS]
    out = dict(g64=g.float().numpy(), g_data64=g_data.float().numpy(), g_trace64=g_trace.float().numpy(), x_new64=x_new.float().numpy(),
               pred_max=np.array(float(pred.abs().max())), jtw_max=np.array(float(jtw.abs().max())), jteps_max=np.array(float(jte.abs().max())),
               g_extra_max=np.array(float(g_extra.abs().max())), g32_err=np.array(float((g32[0].double() - g).abs().max())), trunc64=np.array(trunc),
               iteration=np.array(it), seed=np.array(case[4]))
    if lap:
        small = (info["r"].abs() <= dt * 2e-5 * float(pred.abs().max())).reshape(-1).nonzero().reshape(-1).numpy().astype(np.int64)
        assert small.size <= GATE_SHARE * info["r"].numel(), (name, small.size)
        out["r_small"] = small
    for h in R.FD_STEPS:
        tol_g = R.tolerances(out, h, laplace=lap)[3]
        share = float((g.abs() <= 4 * tol_g).double().mean())
        print(f"  {name} h {h:g}: TOL_g {tol_g:.3e}, share of |g64| <= 4 TOL_g {100 * share:.3f} %")
        assert share <= GATE_SHARE or h not in GATE_STEPS, (name, h, share, "change the case's seed")
    assert all(np.isfinite(v).all() for v in out.values()), name
    path = os.path.join(OUT, f"{prefix}_{name}.npz")
    np.savez_compressed(path, **out)
    print(name, "max|g|", float(g.abs().max()), "max|g_trace|", float(g_trace.abs().max()), "g32_err", float(out["g32_err"]), "trunc64", trunc,
          os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 458 * 1024, path


def tiny4_vels():
    cfg = O.unet_config(**TINY4)
    sd = O.synthetic_state_dict(cfg, 0)
    return R.oracle_vel(sd, cfg, torch.float32), R.oracle_vel(sd, cfg, D)


def gen_steps():
    v32, v64 = tiny4_vels()
    for name, case in R.CASES.items():
        single_step(name, case, v32, v64, "flow_priors_tiny4", 64, 10)


def gen_ncsnpp():
    from oracle import ncsnpp_oracle as NO
    cfg = NO.ncsnpp_config(**NCSNPP_TINY)
    sd = NO.synthetic_state_dict(cfg, 0)
    single_step("inpainting_it50", R.NCSNPP_CASE, R.ncsnpp_vel(sd, cfg, torch.float32), R.ncsnpp_vel(sd, cfg, D), "flow_priors_ncsnpp_tiny", 32, 5)


def gen_free():
    v32, v64 = tiny4_vels()
    op, noise_type, _, inp = R.case_inputs(R.FREE_CASE)
    seed = R.FREE_CASE[4]
    shape = tuple(inp["x_init"].shape)
    pmax = [0.0]

    def run(vel, dtype):
        def vel_rec(x, t):
            out = vel(x, t)
            pmax[0] = max(pmax[0], float(out.detach().abs().max()))
            return out
        vel_rec.vjp, vel_rec.dtype = vel.vjp, vel.dtype
        return R.solve(vel_rec, op.H, inp["x_init"].to(dtype), inp["y"].to(dtype), lambda i, k: R.probe(shape, seed, 100 + i, dtype), R.FREE_N, 1, R.LMBDA, R.ETA)
    x64 = run(v64, D)
    x32 = run(v32, torch.float32)
    first = lambda vel, dtype: R.step(vel, op.H, inp["x_init"].to(dtype), inp["x_init"].to(dtype), inp["y"].to(dtype), [R.probe(shape, seed, 100, dtype)], 0,
                                      R.FREE_N, R.LMBDA, R.ETA)[0].float().numpy()
    dist = (x32.double() - x64).abs()
    far = dist > R.ETA / 2
    d32, m32 = float(far.double().mean()), float(dist[~far].max())
    psnr = lambda x: O.psnr_per_image(x.float(), inp["clean"]).numpy()
    # the fp32 reference's own forward error, relative to max|v|, at the first and at the last point of the run: what the free-run test scales m32 by
    fwd32 = 0.0
    for xq, i in ((inp["x_init"], 0), (x64.float(), R.FREE_N - 1)):
        tq = torch.ones(len(xq)) * R.schedule(R.FREE_N, 0.0, i)[0]
        with torch.no_grad():
            p64, p32 = v64(xq.double(), tq.double()), v32(xq, tq)
        fwd32 = max(fwd32, float((p32.double() - p64).abs().max() / p64.abs().max()))
    out = dict(x32=x32.numpy(), x64=x64.float().numpy(), psnr32=psnr(x32), psnr64=psnr(x64), d32=np.array(d32), m32=np.array(m32), fwd32_rel=np.array(fwd32), pred_max=np.array(pmax[0]),
               seed=np.array(seed), x32_first=first(v32, torch.float32), x64_first=first(v64, D))
    path = os.path.join(OUT, "flow_priors_tiny4_free_run.npz")
    np.savez_compressed(path, **out)
    print("free run: d32", d32, "m32", m32, "fwd32_rel", fwd32, "psnr32", out["psnr32"], "psnr64", out["psnr64"], "pred_max", pmax[0], os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 458 * 1024, path


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    which = sys.argv[1:] or ["pin", "steps", "free", "ncsnpp"]
    if "pin" in which:
        pin_to_reference()
    if "steps" in which:
        gen_steps()
    if "free" in which:
        gen_free()
    if "ncsnpp" in which:
        gen_ncsnpp()
