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

import torch

from .. import _lib
from . import _harness
from ._harness import Solver

DEFAULT_FD_STEP = 3e-3          # the step with the smallest measured error of the engine's trace gradient
NOISE_MODELS = {"gaussian": 0, "laplace": 1}


class FLOW_PRIORS(Solver):

    def __init__(self, model, device, args):
        super().__init__(model.to(device), device, args)       # the library is loaded on the first engine call
        self.N = args.N
        self.fd_step = float(getattr(args, "fd_step", DEFAULT_FD_STEP))
        self.probes = None                  # optional probes(batch, first, stop, K, shape) -> (stop - first) * K injected probes (parity runs)
        self.init_noise = None              # optional init_noise(batch, shape) replacing the torch.randn of x_init

    # model_forward (flow_priors.py:22-25) is Solver's

    # ---- engine calls ------------------------------------------------------------------------------------------------------------
    def _time_scale(self):
        if self.args.model not in ("ot", "rectified"):
            raise self._coupling_error()
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
        return _harness.check_image(x, what, self.model, "FLOW_PRIORS")

    def gradient(self, x, x_init, noisy_img, degradation, eps, iteration):
        """(g, g_data, g_trace, pred) of one inner step of outer iteration `iteration` at x with the probe eps (pf_flow_priors_grad)."""
        x, x_init, eps = self._check(x, "x"), self._check(x_init, "x_init"), self._check(eps, "eps")
        B, Hh = x.shape[0], self.model.input_height
        y = _harness.check_measurement(noisy_img, degradation, B, self.model)
        d = degradation.descriptor(B, Hh, Hh, x.device)
        prm = self._params()
        outs = [torch.empty_like(x) for _ in range(4)]
        _lib.check(self.lib.pf_flow_priors_grad(self.model.handle, C.byref(d), C.byref(prm), x.data_ptr(), x_init.data_ptr(), y.data_ptr(), eps.data_ptr(),
                                                int(iteration), *[o.data_ptr() for o in outs], B, _lib.current_stream_ptr()),
                   self.model.handle, "pf_flow_priors_grad")
        return tuple(outs)

    def restore_batch(self, noisy_img, x_init, degradation, batch=0, first=0, stop=0, x0=None, probes=None):
        """Outer iterations [first, stop) (stop 0: N) of the loop for one batch (pf_flow_priors_restore); x0: the iterate entering `first` > 0."""
        x_init = self._check(x_init, "x_init")
        B, Hh = x_init.shape[0], self.model.input_height
        y = _harness.check_measurement(noisy_img, degradation, B, self.model)
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
        with _lib.solver_stream():
            _lib.check(self.lib.pf_flow_priors_restore(self.model.handle, C.byref(d), C.byref(prm), y.data_ptr(), x_init.data_ptr(),
                                                       probes.data_ptr() if probes is not None else None, x.data_ptr(), B, _lib.current_stream_ptr()),
                       self.model.handle, "pf_flow_priors_restore")
        return x

    # ---- solver ------------------------------------------------------------------------------------------------------------------
    def solve_ip(self, test_loader, degradation, sigma_noise):
        _harness.single_gpu_only(_harness.env_world(), "flow_priors runs on one GPU only: multi-GPU sharding of this solver is not built")
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
            # flow_priors.py:44-50: the laplace draw is not re-seeded by the reference
            noise = _harness.measurement_noise(self, batch, noisy_img, tuple(noisy_img.shape), 0, G, self.args.noise_type)
            noisy_img = noisy_img + noise * sigma_noise
            clean_img = clean_img.to('cpu')
            shape = (G, self.model.input_channels, self.model.input_height, self.model.input_height)
            # flow_priors.py:57-58: x_init ~ N(0, I), the draw after the measurement noise on the CPU generator
            x_init = (self.init_noise(batch, shape) if self.init_noise is not None else torch.randn(shape)).to(self.device).float()

            with _harness.batch_stats(self, batch):
                probes = self.probes(batch, 0, int(self.args.N), int(self.args.K), shape) if self.probes is not None else None
                restored_img = self.restore_batch(noisy_img, x_init, degradation, batch=batch, probes=probes)
                self.last_restored = restored_img
            self.write_final(clean_img, noisy_img, restored_img, H_adj, int(self.args.N) - 1)
        self.write_averages()
