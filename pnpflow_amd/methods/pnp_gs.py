"""PROX_PNP solver with the API of pnpflow/methods/pnp_gs.py (reference :11-264; Prox-PnP with the gradient-step denoiser, Hurault et
al., 2022).

`model` is a GRADIENT_STEP_DENOISER (pnpflow_amd/train_denoiser.py).  Every iteration needs Dg = (z - N) - J_N(z)^T (z - N) at some
point z and denoiser level, then one of three closed forms:

    algo pgd                             z = x - lr grad_datafit(x) (not for gaussian denoising);  x = z - alpha Dg(z)
    algo hqs, random_inpainting          Dx = x - Dg(x);  x = H(y) - H(Dx) + Dx  (the last iteration leaves x as it is)
    algo hqs, gaussian_deblurring_FFT    Fourier-domain prox of 0.1 alpha Dx + alpha (1 - 0.1 alpha) x, then alpha *= 0.9 when the
                                         objective gap falls below 0.1 / alpha |x_new - x|^2

The whole loop of a batch is one engine call (pf_pnp_gs_restore): retained forward, seed, hand-written backward and the fused combine
per iteration, replayed as one hipGraph; alpha lives on the device.
"""
from __future__ import annotations

import ctypes as C
import os
from time import perf_counter

import numpy as np
import torch

from .. import _lib
from .. import parallel
from .. import utils

SUPPORTED = "algo pgd (any problem, gaussian or laplace noise), algo hqs with problem random_inpainting, algo hqs with problem gaussian_deblurring_FFT"


class PROX_PNP(object):

    def __init__(self, model, device, args):
        self.device = device
        self.args = args
        self.model = model
        self.method = args.method
        self._lib = None
        self.use_graph = True               # one hipGraph per iteration
        self.measurement_noise = None       # optional measurement_noise(batch, noisy) replacing the seeded draw (unit scale)
        self.measurement_noise_source = getattr(args, "measurement_noise", "cpu")      # "cpu" | "device" (the reference's: pnp_gs.py:105-106)
        self.last_restored = None
        self.last_alpha = None              # alpha after the last restore_batch (hqs deblurring decays it)
        self.last_gap_log = None            # hqs deblurring: [max_iter, 2] (gap, threshold) of the iterations the last restore_batch ran
        self.last_callback_seconds = 0.0

    @property
    def lib(self):
        if self._lib is None:
            self._lib = _lib.load()
        return self._lib

    # ---- the reference's method surface ----------------------------------------------------------------------------------------
    def model_forward(self, x):
        sigma = torch.ones(len(x), device=self.device) * self.args.sigma_noise
        if self.args.model == "gradient_step":
            return self.model(x, sigma)

    def grad_datafit(self, x, y, H, H_adj):
        if self.args.noise_type == 'gaussian':
            return H_adj(H(x) - y) / (self.args.sigma_noise ** 2)
        elif self.args.noise_type == 'laplace':
            r = H(x) - y
            return H_adj(2 * torch.heaviside(r, torch.zeros_like(r)) - 1) / self.args.sigma_noise
        raise ValueError('Noise type not supported')

    def prox_datafit(self, x, y, H, H_adj, degradation=None, alpha=None):
        """pnp_gs.py:32-44 (the unreachable superresolution_bicubic branch is not implemented)."""
        if self.args.noise_type == 'gaussian' and self.args.problem == "random_inpainting":
            return H(y) - H(x) + x
        if self.args.noise_type == 'gaussian' and self.args.problem == "gaussian_deblurring_FFT":
            fft_d = torch.fft.fft2(alpha * H_adj(y) + x)
            fft_kernel = torch.fft.fft2(degradation.filter.to(x.device))
            inv = alpha * torch.conj(fft_kernel) * fft_kernel + 1.
            return torch.real(torch.fft.ifft2(fft_d / inv))
        raise NotImplementedError(f"prox_datafit: no closed form for problem {self.args.problem!r} with {self.args.noise_type} noise")

    def objective(self, x, y, H, H_adj, lmbda, g):
        if self.args.noise_type == 'gaussian':
            return 0.5 * torch.linalg.norm(H(x) - y) ** 2 + lmbda * g
        elif self.args.noise_type == 'laplace':
            return torch.mean(torch.abs(H(x) - y)) + lmbda * g
        raise ValueError('Noise type not supported')

    # ---- host schedule ---------------------------------------------------------------------------------------------------------
    def algo_code(self):
        """0 pgd | 1 hqs random_inpainting | 2 hqs gaussian_deblurring_FFT.  The reference's loop matches no branch for any other
        pair and silently returns the initialisation; here that is an error."""
        algo, problem = self.args.algo, self.args.problem
        if algo == "pgd":
            return 0
        if algo == "hqs" and problem == "random_inpainting":
            return 1
        if algo == "hqs" and problem == "gaussian_deblurring_FFT":
            return 2
        if algo == "hqs" and problem == "gaussian_deblurring":
            raise ValueError("pnp_gs: algo 'hqs' has no form for problem 'gaussian_deblurring' (the zero-boundary blur): its prox is a Fourier solve of the "
                             "circular operator (problem 'gaussian_deblurring_FFT'); use algo 'pgd'")
        raise ValueError(f"pnp_gs: algo {algo!r} with problem {problem!r} is not supported; supported: {SUPPORTED}")

    def level_table(self, sigma_noise):
        """Denoiser level of every iteration, fp32 as the reference's `c * torch.ones(B)` makes it (pnp_gs.py:141-145, 159-160, 213-214)."""
        code, n = self.algo_code(), int(self.args.max_iter)
        if code == 1:
            tab = [0.2 if it < 20 else sigma_noise for it in range(n)]
        elif code == 2:
            tab = [1.8 * sigma_noise] * n
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
        x = (self.initialise(y, degradation) if x0 is None else x0.detach().clone()).to(y.device).contiguous().float()
        if tuple(x.shape) != (B, self.model.input_channels, Hh, Hh):
            raise ValueError(f"iterate of shape {tuple(x.shape)} does not match the net's (B, {self.model.input_channels}, {Hh}, {Hh})")
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
        holder = {"err": None}
        self.last_callback_seconds = 0.0
        if iter_cb is not None:
            def _cb(it, user):
                t_cb = perf_counter()
                try:
                    if holder["err"] is None:
                        iter_cb(it, x)
                except BaseException as exc:      # must not unwind through the C frames: re-raised below
                    holder["err"] = exc
                self.last_callback_seconds += perf_counter() - t_cb
            cb = _lib.ITER_CB(_cb)
            if cb_iterations is not None:
                mask = np.zeros(max_iter, dtype=np.uint8)
                mask[[i for i in cb_iterations if 0 <= i < max_iter]] = 1
                holder["mask"] = mask
                prm.host_cb_mask = mask.ctypes.data
        else:
            cb = C.cast(None, _lib.ITER_CB)
        alpha_out = C.c_double(prm.alpha)
        log = np.zeros((max_iter, 2), dtype=np.float64)
        with _lib.solver_stream():       # engine launches and metric callbacks on ONE stream (a real one: graph capture)
            _lib.check(self.lib.pf_pnp_gs_restore(self.model.handle, C.byref(d), C.byref(prm), y.data_ptr(), x.data_ptr(), C.byref(alpha_out),
                                                  log.ctypes.data_as(C.POINTER(C.c_double)), B, _lib.current_stream_ptr(), cb, None),
                       self.model.handle, "pf_pnp_gs_restore")
        if holder["err"] is not None:
            raise holder["err"]
        self.last_alpha = float(alpha_out.value)
        self.last_gap_log = log if code == 2 else None
        return x

    def solve_ip(self, test_loader, degradation, sigma_noise):
        world = max(parallel.rank_world()[1], int(os.environ.get("WORLD_SIZE", "1")))
        if world > 1:
            # the hqs deblurring rule compares norms over the whole batch tensor: a split batch would take other alpha decisions
            raise RuntimeError("pnp_gs runs on one GPU only: its hqs deblurring branch decays alpha on norms over the whole batch, "
                               f"so a batch split over {world} ranks would change the result. Run it without torchrun.")
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
            if self.measurement_noise is not None:
                noise = self.measurement_noise(batch, noisy_img)
            elif self.args.noise_type == 'laplace':
                # pnp_gs.py:107-110: a Laplace sample of scale sigma_noise (unit scale here, scaled below), drawn on the CPU generator
                noise = torch.distributions.laplace.Laplace(torch.zeros(gshape), torch.ones(gshape)).sample().to(self.device)
            elif self.args.noise_type == 'gaussian':
                noise = utils.draw_measurement_noise(batch, gshape, 0, G, self.device, self.measurement_noise_source)      # pnp_gs.py:105-106
            else:
                raise ValueError('Noise type not supported')
            noisy_img = noisy_img + noise.to(self.device) * sigma_noise
            clean_img = clean_img.to('cpu')
            if self.args.compute_time:
                torch.cuda.synchronize(); t0 = perf_counter()
            if self.args.compute_memory:
                torch.cuda.reset_peak_memory_stats(self.device)

            def on_iter(iteration, x):
                utils.compute_psnr(clean_img, noisy_img, x.detach().clone(), self.args, H_adj, iter=iteration)
                utils.compute_ssim(clean_img, noisy_img, x.detach().clone(), self.args, H_adj, iter=iteration)
                utils.compute_lpips(clean_img, noisy_img, x.detach().clone(), self.args, H_adj, iter=iteration)

            log_its = [it for it in range(max_iter) if it % 10 == 0] if self.args.save_results else []      # pnp_gs.py:224
            x = self.restore_batch(noisy_img, degradation, sigma_noise, lr=lr, alpha=alpha,
                                   iter_cb=on_iter if self.args.save_results else None, cb_iterations=log_its)
            alpha = self.last_alpha
            self.last_restored = x
            if self.args.compute_memory:
                utils.save_memory_use({"batch": batch, "max_allocated": torch.cuda.max_memory_allocated(self.device) + self.model.memory_bytes()},
                                      self.args)
            if self.args.compute_time:
                torch.cuda.synchronize()
                utils.save_time_use({"batch": batch, "time_per_batch": perf_counter() - t0 - self.last_callback_seconds}, self.args)
            if self.args.save_results:
                last = max_iter - 1         # the final metrics carry the last loop index as `iter` (pnp_gs.py:239-244)
                utils.save_images(clean_img, noisy_img, x.detach().clone(), self.args, H_adj, iter='final')
                utils.compute_psnr(clean_img, noisy_img, x.detach().clone(), self.args, H_adj, iter=last)
                utils.compute_ssim(clean_img, noisy_img, x.detach().clone(), self.args, H_adj, iter=last)
                utils.compute_lpips(clean_img, noisy_img, x.detach().clone(), self.args, H_adj, iter=last)
        if self.args.save_results:
            utils.compute_average_psnr(self.args)
            utils.compute_average_ssim(self.args)
            utils.compute_average_lpips(self.args)
        if self.args.compute_memory:
            utils.compute_average_memory(self.args)
        if self.args.compute_time:
            utils.compute_average_time(self.args)

    def should_save_image(self, iteration, steps):
        return iteration % (steps // 5) == 0

    def run_method(self, data_loaders, degradation, sigma_noise):
        folder = utils.get_save_path_ip(self.args.dict_cfg_method)
        self.args.save_path_ip = os.path.join(self.args.save_path, folder)
        os.makedirs(self.args.save_path_ip, exist_ok=True)
        self.solve_ip(data_loaders[self.args.eval_split], degradation, sigma_noise)
