"""FLOW_PRIORS solver with the API of pnpflow/methods/flow_priors.py (reference :9-208; Zhang et al., "Flow Priors for Linear Inverse
Problems via Iterative Corrupted Trajectory Matching", 2024).

Per outer iteration i of N (t = i/N (1 - eps0) + eps0) a fresh Adam takes K steps on

    lmbda |H(x + v(x, t) dt) - y_next|^2  (|.|_1 for laplace noise)  +  dt eps . J_v(x, t) eps   (+ 0.5 |x|^2 on iteration 0)

with y_next = (t + dt) y + (1 - (t + dt)) H(x_init), adds the detached grad_xt_lik = -1/(1 - t) (-x + t v) to the gradient on later
iterations, and then moves x += v(x, t) dt.  The reference differentiates the Hutchinson trace term with a second-order autograd pass;
here its gradient is the central difference of two first-order VJPs of the engine,

    grad_x (eps . J(x) eps) = d/ds [J(x + s eps)^T eps] at s = 0  ~  (J(x + h eps)^T eps - J(x - h eps)^T eps) / (2 h),   h = fd_step,

and the whole N x K loop runs on the device (pf_flow_priors_restore).  The probes are the engine's Rademacher fill (seeded by the batch number),
not torch.rand on the device: DESIGN.md section 11.
"""
from __future__ import annotations

import ctypes as C
import os
from time import perf_counter

import torch

from .. import _lib
from .. import parallel
from .. import utils

DEFAULT_FD_STEP = 3e-3          # the step with the smallest measured error of the engine's trace gradient
NOISE_MODELS = {"gaussian": 0, "laplace": 1}


class FLOW_PRIORS(object):

    def __init__(self, model, device, args):
        self.device = device
        self.args = args
        self.model = model.to(device)
        self.method = args.method
        self.N = args.N
        self.lib = None                     # loaded on the first engine call
        self.fd_step = float(getattr(args, "fd_step", DEFAULT_FD_STEP))
        self.probes = None                  # optional probes(batch, first, stop, K, shape) -> (stop - first) * K injected probes (parity runs)
        self.measurement_noise = None       # optional measurement_noise(batch, noisy) replacing the seeded draw (unit scale)
        self.init_noise = None              # optional init_noise(batch, shape) replacing the torch.randn of x_init
        self.measurement_noise_source = getattr(args, "measurement_noise", "cpu")
        self.last_restored = None

    def model_forward(self, x, t):
        if self.args.model == "ot":
            return self.model(x, t)
        if self.args.model == "rectified":        # flow_priors.py:22-25: model_fn(x, t * 999)
            return self.model(x.type(torch.float), t * 999)
        raise NotImplementedError("only the 'ot' U-Net and the 'rectified' NCSN++ net are implemented")

    # ---- engine calls ------------------------------------------------------------------------------------------------------------
    def _time_scale(self):
        if self.args.model not in ("ot", "rectified"):
            raise NotImplementedError("only the 'ot' U-Net and the 'rectified' NCSN++ net are implemented")
        return 999.0 if self.args.model == "rectified" else 1.0

    def _params(self, batch=0, first=0, stop=0):
        if self.args.noise_type not in NOISE_MODELS:
            raise ValueError('Noise type not supported')
        prm = _lib.PfFlowPriorsParams()
        prm.N, prm.K, prm.first, prm.stop = int(self.args.N), int(self.args.K), int(first), int(stop)
        prm.lmbda, prm.eta, prm.start_time, prm.fd_step = float(self.args.lmbda), float(self.args.eta), float(self.args.start_time), float(self.fd_step)
        prm.noise_model = NOISE_MODELS[self.args.noise_type]
        prm.seed, prm.stream_base = int(batch) & 0xFFFFFFFFFFFFFFFF, 0          # one probe stream per inner step: stream id i * K + k under key `batch`
        prm.time_scale = self._time_scale()
        return prm

    def _check(self, x, what):
        Hh = self.model.input_height
        if x.ndim != 4 or tuple(x.shape[1:]) != (self.model.input_channels, Hh, Hh):
            raise ValueError(f"{what} of shape {tuple(x.shape)} does not match the net's (B, {self.model.input_channels}, {Hh}, {Hh})")
        if not x.is_cuda:
            raise _lib.PnpFlowHipError("FLOW_PRIORS needs GPU tensors (there is no CPU path)")
        return x.detach().contiguous().float()

    def _check_measurement(self, y, degradation, B):
        Hh = self.model.input_height
        sf = getattr(degradation, "sf", 1) if degradation.kind in (_lib.PF_DEG_SUPERRESOLUTION, _lib.PF_DEG_SR_FILTERED) else 1
        if tuple(y.shape) != (B, self.model.input_channels, Hh // sf, Hh // sf):
            raise ValueError(f"measurement of shape {tuple(y.shape)} does not match the operator's output ({B}, {self.model.input_channels}, "
                             f"{Hh // sf}, {Hh // sf})")
        return y.detach().contiguous().float()

    def gradient(self, x, x_init, noisy_img, degradation, eps, iteration):
        """(g, g_data, g_trace, pred) of one inner step of outer iteration `iteration` at x with the probe eps (pf_flow_priors_grad)."""
        x, x_init, eps = self._check(x, "x"), self._check(x_init, "x_init"), self._check(eps, "eps")
        B, Hh = x.shape[0], self.model.input_height
        y = self._check_measurement(noisy_img, degradation, B)
        d = degradation.descriptor(B, Hh, Hh, x.device)
        prm = self._params()
        self.lib = self.lib or _lib.load()
        outs = [torch.empty_like(x) for _ in range(4)]
        _lib.check(self.lib.pf_flow_priors_grad(self.model.handle, C.byref(d), C.byref(prm), x.data_ptr(), x_init.data_ptr(), y.data_ptr(), eps.data_ptr(),
                                                int(iteration), *[o.data_ptr() for o in outs], B, _lib.current_stream_ptr()),
                   self.model.handle, "pf_flow_priors_grad")
        return tuple(outs)

    def restore_batch(self, noisy_img, x_init, degradation, batch=0, first=0, stop=0, x0=None, probes=None):
        """Outer iterations [first, stop) (stop 0: N) of the loop for one batch (pf_flow_priors_restore); x0: the iterate entering `first` > 0."""
        x_init = self._check(x_init, "x_init")
        B, Hh = x_init.shape[0], self.model.input_height
        y = self._check_measurement(noisy_img, degradation, B)
        d = degradation.descriptor(B, Hh, Hh, x_init.device)
        prm = self._params(batch, first, stop)
        if first > 0 and x0 is None:
            raise ValueError("restore_batch: entering the loop at iteration first > 0 needs the iterate x0")
        x = self._check(x0, "x0").clone() if first > 0 else torch.empty_like(x_init)
        if probes is not None:
            probes = probes.detach().contiguous().float()
            n_steps = ((stop or int(self.args.N)) - first) * int(self.args.K)
            if probes.numel() != n_steps * x_init.numel() or not probes.is_cuda:
                raise ValueError(f"probes must hold {n_steps} device tensors of shape {tuple(x_init.shape)}")
        self.lib = self.lib or _lib.load()
        with _lib.solver_stream():
            _lib.check(self.lib.pf_flow_priors_restore(self.model.handle, C.byref(d), C.byref(prm), y.data_ptr(), x_init.data_ptr(),
                                                       probes.data_ptr() if probes is not None else None, x.data_ptr(), B, _lib.current_stream_ptr()),
                       self.model.handle, "pf_flow_priors_restore")
        return x

    # ---- solver ------------------------------------------------------------------------------------------------------------------
    def solve_ip(self, test_loader, degradation, sigma_noise):
        world = max(parallel.rank_world()[1], int(os.environ.get("WORLD_SIZE", "1")))
        if world > 1:
            raise RuntimeError("flow_priors runs on one GPU only: multi-GPU sharding of this solver is not built, "
                               f"so a batch split over {world} ranks would change the result. Run it without torchrun.")
        if self.args.noise_type not in NOISE_MODELS:
            raise ValueError('Noise type not supported')
        self._time_scale()
        H, H_adj = degradation.H, degradation.H_adj
        self.args.sigma_noise = sigma_noise
        loader = iter(test_loader)
        for batch in range(self.args.max_batch):
            (clean_img, labels) = next(loader)
            self.args.batch = batch
            noisy_img = H(clean_img.clone().to(self.device))
            G = noisy_img.shape[0]
            if self.measurement_noise is not None:
                noise = self.measurement_noise(batch, noisy_img)
            elif self.args.noise_type == 'gaussian':
                noise = utils.draw_measurement_noise(batch, tuple(noisy_img.shape), 0, G, self.device, self.measurement_noise_source)   # flow_priors.py:44-45
            else:
                # flow_priors.py:48-50: the laplace draw is not re-seeded by the reference
                noise = torch.distributions.laplace.Laplace(torch.zeros(tuple(noisy_img.shape)), torch.ones(tuple(noisy_img.shape))).sample().to(self.device)
            noisy_img = noisy_img + noise * sigma_noise
            clean_img = clean_img.to('cpu')
            shape = (G, self.model.input_channels, self.model.input_height, self.model.input_height)
            # flow_priors.py:57-58: x_init ~ N(0, I), the draw after the measurement noise on the CPU generator
            x_init = (self.init_noise(batch, shape) if self.init_noise is not None else torch.randn(shape)).to(self.device).float()

            if self.args.compute_time:
                torch.cuda.synchronize()
                t0 = perf_counter()
            if self.args.compute_memory:
                torch.cuda.reset_peak_memory_stats(self.device)
            probes = self.probes(batch, 0, int(self.args.N), int(self.args.K), shape) if self.probes is not None else None
            restored_img = self.restore_batch(noisy_img, x_init, degradation, batch=batch, probes=probes)
            self.last_restored = restored_img
            iteration = int(self.args.N) - 1

            if self.args.compute_memory:
                utils.save_memory_use({"batch": batch, "max_allocated": torch.cuda.max_memory_allocated(self.device) + self.model.memory_bytes()},
                                      self.args)
            if self.args.compute_time:
                torch.cuda.synchronize()
                utils.save_time_use({"batch": batch, "time_per_batch": perf_counter() - t0}, self.args)
            if self.args.save_results:
                utils.save_images(clean_img, noisy_img, restored_img, self.args, H_adj, iter='final')
                utils.compute_psnr(clean_img, noisy_img, restored_img, self.args, H_adj, iter=iteration)
                utils.compute_ssim(clean_img, noisy_img, restored_img, self.args, H_adj, iter=iteration)
                utils.compute_lpips(clean_img, noisy_img, restored_img, self.args, H_adj, iter=iteration)
        if self.args.save_results:
            utils.compute_average_psnr(self.args)
            utils.compute_average_ssim(self.args)
            utils.compute_average_lpips(self.args)
        if self.args.compute_memory:
            utils.compute_average_memory(self.args)
        if self.args.compute_time:
            utils.compute_average_time(self.args)

    def run_method(self, data_loaders, degradation, sigma_noise):
        folder = utils.get_save_path_ip(self.args.dict_cfg_method)
        self.args.save_path_ip = os.path.join(self.args.save_path, folder)
        os.makedirs(self.args.save_path_ip, exist_ok=True)
        self.solve_ip(data_loaders[self.args.eval_split], degradation, sigma_noise)
