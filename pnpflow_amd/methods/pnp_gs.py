"""PROX_PNP solver with the API of pnpflow/methods/pnp_gs.py (reference :11-264; Prox-PnP with the gradient-step denoiser, Hurault et
al., 2022).

`model` is a GRADIENT_STEP_DENOISER (pnpflow_amd/train_denoiser.py).  Every iteration needs Dg = (z - N) - J_N(z)^T (z - N) at some
point z and denoiser level, then one of four closed forms:

    algo pgd                             z = x - lr grad_datafit(x) (not for gaussian denoising);  x = z - alpha Dg(z)
    algo hqs, random_inpainting          Dx = x - Dg(x);  x = H(y) - H(Dx) + Dx  (the last iteration leaves x as it is)
    algo hqs, gaussian_deblurring_FFT    Fourier-domain prox of 0.1 alpha Dx + alpha (1 - 0.1 alpha) x, then alpha *= 0.9 when the
                                         objective gap falls below 0.1 / alpha |x_new - x|^2
    algo hqs, superresolution_blur /     z = 0.065 alpha Dx + alpha (1 - 0.065 alpha) x, then the exact prox of alpha/2 |H x - y|^2 at z; the denoiser
              superresolution_bicubic    level is 2 sigma_noise, alpha never decays (the schedule of the reference's branch, pnp_gs.py:180-200)

The reference's own prox_datafit for superresolution_bicubic (pnp_gs.py:45-76; main.py cannot reach it) is not a proximal map: its `below` multiplies
the aliased power spectrum by the data spectrum (:71-72).  What is built instead is exact.  For circular H = S K (blur, keep every sf-th sample)
H H^T is circulant on the low-resolution grid with the eigenvalues lam[u, v] = 1/sf^2 sum_{a, b < sf} |fft2 k|^2 [u + a H/sf, v + b W/sf], so by the
Woodbury identity  prox(z) = r - alpha H_adj( ifft2_l( fft2_l(H r) / (alpha lam + 1) ) ),  r = z + alpha H_adj(y):  one Fourier solve on the
low-resolution grid between one H and one H_adj (pf_sr_prox).

The whole loop of a batch is one engine call (pf_pnp_gs_restore): retained forward, seed, hand-written backward and the fused combine
per iteration, replayed as one hipGraph; alpha lives on the device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from . import _harness
from ._harness import IterCallback, Solver

SUPPORTED = ("algo pgd (any problem, gaussian or laplace noise), algo hqs with problem random_inpainting, algo hqs with problem gaussian_deblurring_FFT "
             "or psf_deblurring_FFT, algo hqs with problem superresolution_blur or superresolution_bicubic")
FFT_BLURS = ("gaussian_deblurring_FFT", "psf_deblurring_FFT")      # the circular blurs: hqs has a Fourier-domain prox for them
SR_BLURS = ("superresolution_blur", "superresolution_bicubic")     # circular blur, then decimation: the same on the low-resolution grid


class PROX_PNP(Solver):

    def __init__(self, model, device, args):
        super().__init__(model, device, args)       # the library is loaded on the first engine call
        self.use_graph = True               # one hipGraph per iteration
        self.last_alpha = None              # alpha after the last restore_batch (hqs deblurring decays it)
        self.last_gap_log = None            # hqs deblurring: [max_iter, 2] (gap, threshold) of the iterations the last restore_batch ran

    # ---- the reference's method surface (grad_datafit, pnp_gs.py:23-30, is Solver's) -------------------------------------------
    def model_forward(self, x):
        sigma = torch.ones(len(x), device=self.device) * self.args.sigma_noise
        if self.args.model == "gradient_step":
            return self.model(x, sigma)

    def prox_datafit(self, x, y, H, H_adj, degradation=None, alpha=None):
        """pnp_gs.py:32-44; for the blur-then-decimate problems the exact prox (module docstring) in place of the reference's :45-76."""
        if self.args.noise_type == 'gaussian' and self.args.problem == "random_inpainting":
            return H(y) - H(x) + x
        if self.args.noise_type == 'gaussian' and self.args.problem in FFT_BLURS:
            fft_d = torch.fft.fft2(alpha * H_adj(y) + x)
            fft_kernel = torch.fft.fft2(degradation.filter.to(x.device))
            inv = alpha * torch.conj(fft_kernel) * fft_kernel + 1.
            return torch.real(torch.fft.ifft2(fft_d / inv))
        if self.args.noise_type == 'gaussian' and self.args.problem in SR_BLURS:
            r = x + alpha * H_adj(y)
            k2 = torch.fft.fft2(degradation.filter.to(x.device)).abs() ** 2
            sf, Hl, Wl = degradation.sf, x.shape[-2] // degradation.sf, x.shape[-1] // degradation.sf
            lam = k2.reshape(*k2.shape[:2], sf, Hl, sf, Wl).sum(dim=(2, 4)) / sf ** 2
            sol = torch.real(torch.fft.ifft2(torch.fft.fft2(H(r)) / (alpha * lam + 1.)))
            return r - alpha * H_adj(sol)
        raise NotImplementedError(f"prox_datafit: no closed form for problem {self.args.problem!r} with {self.args.noise_type} noise")

    def objective(self, x, y, H, H_adj, lmbda, g):
        if self.args.noise_type == 'gaussian':
            return 0.5 * torch.linalg.norm(H(x) - y) ** 2 + lmbda * g
        elif self.args.noise_type == 'laplace':
            return torch.mean(torch.abs(H(x) - y)) + lmbda * g
        raise ValueError('Noise type not supported')

    # ---- host schedule ---------------------------------------------------------------------------------------------------------
    def algo_code(self):
        """0 pgd | 1 hqs random_inpainting | 2 hqs gaussian_deblurring_FFT / psf_deblurring_FFT | 3 hqs superresolution_blur / superresolution_bicubic.  The reference's loop matches no branch for any other
        pair and silently returns the initialisation; here that is an error."""
        algo, problem = self.args.algo, self.args.problem
        if algo == "pgd":
            return 0
        if algo == "hqs" and problem == "random_inpainting":
            return 1
        if algo == "hqs" and problem in FFT_BLURS:
            return 2
        if algo == "hqs" and problem in SR_BLURS:
            return 3
        if algo == "hqs" and problem in ("gaussian_deblurring", "psf_deblurring"):
            raise ValueError(f"pnp_gs: algo 'hqs' has no form for problem {problem!r} (the zero-boundary blur): its prox is a Fourier solve of the "
                             f"circular operator (problem '{problem}_FFT'); use algo 'pgd'")
        raise ValueError(f"pnp_gs: algo {algo!r} with problem {problem!r} is not supported; supported: {SUPPORTED}")

    def level_table(self, sigma_noise):
        """Denoiser level of every iteration, fp32 as the reference's `c * torch.ones(B)` makes it (pnp_gs.py:141-145, 159-160, 213-214)."""
        code, n = self.algo_code(), int(self.args.max_iter)
        if code == 1:
            tab = [0.2 if it < 20 else sigma_noise for it in range(n)]
        elif code == 2:
            tab = [1.8 * sigma_noise] * n
        elif code == 3:
            tab = [2.0 * sigma_noise] * n          # pnp_gs.py:182-183
        else:
            tab = [self.args.sigma_factor * sigma_noise] * n
        return np.asarray(tab, dtype=np.float32)

    def initialise(self, noisy_img, degradation):
        """pnp_gs.py:119-130."""
        problem = self.args.problem
        if problem == "random_inpainting":
            return 1.5 * noisy_img.clone() - degradation.H(noisy_img)
        if problem == "superresolution":
            from ..degradations import Superresolution
            S = self.model.input_height
            sf = 2 if S == 128 else 4
            return Superresolution(sf, S, mode="bicubic", device=self.device).H_adj(noisy_img.clone())
        return degradation.H_adj(noisy_img.clone())

    # ---- engine loop -----------------------------------------------------------------------------------------------------------
    def restore_batch(self, noisy_img, degradation, sigma_noise, first=0, stop=None, x0=None, lr=None, alpha=None, iter_cb=None, cb_iterations=None):
        """Iterations [first, stop) of the loop of solve_ip for one batch (pnp_gs.py:132-222) on the engine.  x0: the iterate entering
        iteration `first` (None: the reference's initialisation); lr: the step of the data-term gradient (None: sigma_noise^2 * lr_pnp);
        alpha: the entering alpha (None: args.alpha).  Returns x; alpha afterwards is in last_alpha."""
        args = self.args
        code = self.algo_code()
        if args.noise_type not in ("gaussian", "laplace"):
            raise ValueError('Noise type not supported')
        if args.noise_type == "laplace" and code != 0:
            raise ValueError(f"pnp_gs: laplace noise is supported by algo pgd only; supported: {SUPPORTED}")
        max_iter = int(args.max_iter)
        stop = max_iter if stop is None else int(stop)
        if not noisy_img.is_cuda:
            raise _lib.PnpFlowHipError("PROX_PNP needs GPU tensors (there is no CPU path)")
        B, Hh = noisy_img.shape[0], self.model.input_height
        y = noisy_img.detach().contiguous().float()
        x = _harness.check_image((self.initialise(y, degradation) if x0 is None else x0.detach().clone()).to(y.device), "iterate", self.model, "PROX_PNP")
        if x.shape[0] != B:
            raise ValueError(f"iterate of shape {tuple(x.shape)} does not match the measurement's batch of {B}")
        d = degradation.descriptor(B, Hh, Hh, y.device)
        lr = sigma_noise ** 2 * args.lr_pnp if lr is None else lr
        tab = self.level_table(sigma_noise)
        prm = _lib.PfPnpGsParams()
        prm.algo, prm.noise_model = code, 1 if args.noise_type == "laplace" else 0
        prm.max_iter, prm.first, prm.stop = max_iter, int(first), stop
        prm.skip_grad_step = 1 if (args.problem == "denoising" and args.noise_type != "laplace") else 0      # pnp_gs.py:204-210
        prm.host_sigma_den = tab.ctypes.data_as(C.POINTER(C.c_float))
        prm.grad_coef = float(lr) / (sigma_noise ** 2 if args.noise_type == "gaussian" else sigma_noise)
        prm.alpha = float(args.alpha if alpha is None else alpha)
        prm.use_graph = 1 if self.use_graph else 0
        call = IterCallback(iter_cb, max_iter, cb_iterations)
        call.attach(prm); call.bind(x)
        alpha_out = C.c_double(prm.alpha)
        log = np.zeros((max_iter, 2), dtype=np.float64)
        with _lib.solver_stream():       # engine launches and metric callbacks on ONE stream (a real one: graph capture)
            _lib.check(self.lib.pf_pnp_gs_restore(self.model.handle, C.byref(d), C.byref(prm), y.data_ptr(), x.data_ptr(), C.byref(alpha_out),
                                                  log.ctypes.data_as(C.POINTER(C.c_double)), B, _lib.current_stream_ptr(), call.cb, None),
                       self.model.handle, "pf_pnp_gs_restore")
        self.last_callback_seconds = call.seconds
        call.reraise()
        self.last_alpha = float(alpha_out.value)
        self.last_gap_log = log if code == 2 else None
        return x

    def solve_ip(self, test_loader, degradation, sigma_noise):
        # the hqs deblurring rule compares norms over the whole batch tensor: a split batch would take other alpha decisions
        _harness.single_gpu_only(_harness.env_world(), "pnp_gs runs on one GPU only: its hqs deblurring branch decays alpha on norms over the whole batch")
        self.algo_code()                    # an unsupported (algo, problem) pair fails before anything is drawn
        H, H_adj = degradation.H, degradation.H_adj
        self.args.sigma_noise = sigma_noise
        self.args.lr_pnp = sigma_noise ** 2 * self.args.lr_pnp      # in place on every call, as the reference (pnp_gs.py:90)
        lr = self.args.lr_pnp
        max_iter = int(self.args.max_iter)
        alpha = self.args.alpha             # read once before the batch loop: a decay carries over to later batches (pnp_gs.py:96)
        loader = iter(test_loader)
        for batch in range(self.args.max_batch):
            (clean_img, labels) = next(loader)
            self.args.batch = batch
            noisy_img = H(clean_img.clone().to(self.device))
            G = noisy_img.shape[0]
            gshape = tuple(noisy_img.shape)
            # pnp_gs.py:105-110: gaussian after torch.manual_seed(batch); the Laplace sample (unit scale here, scaled below) is not re-seeded
            noise = _harness.measurement_noise(self, batch, noisy_img, gshape, 0, G, self.args.noise_type)
            noisy_img = noisy_img + noise.to(self.device) * sigma_noise
            clean_img = clean_img.to('cpu')

            def on_iter(iteration, x):
                self.write_metrics(clean_img, noisy_img, x, H_adj, iteration)

            log_its = [it for it in range(max_iter) if it % 10 == 0] if self.args.save_results else []      # pnp_gs.py:224
            with _harness.batch_stats(self, batch):
                x = self.restore_batch(noisy_img, degradation, sigma_noise, lr=lr, alpha=alpha,
                                       iter_cb=on_iter if self.args.save_results else None, cb_iterations=log_its)
                alpha = self.last_alpha
                self.last_restored = x
            self.write_final(clean_img, noisy_img, x, H_adj, max_iter - 1)         # pnp_gs.py:239-244
        self.write_averages()

    def should_save_image(self, iteration, steps):
        return iteration % (steps // 5) == 0
