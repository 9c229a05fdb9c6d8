"""D_FLOW solver with the API of pnpflow/methods/d_flow.py (reference :13-176; Ben-Hamu et al., "D-Flow: Differentiating through
flows for controlled generation", 2024).

The latent z is initialised by integrating the flow ODE backwards from the back-projected measurement (dopri5, rtol = atol = 1e-5),
blended with noise, then refined by torch.optim.LBFGS on

    loss(z) = sum_b |H(T(z_b)) - y_b|^2 + lmbda (0.5 clamp(|z_b|^2, +-1e6) - (d-1) log(|z_b| + 1e-5))

with T = steps_euler - 1 explicit midpoint steps of the velocity net.  The reference differentiates T with autograd; here one engine
call (pf_d_flow_value_and_grad) returns the per-image loss and its gradient from the hand-written adjoint of T on the net's VJP,
replayed as one hipGraph per closure.  The dopri5 solve is pf_flow_ode_dopri5.  LBFGS itself is PyTorch's, with the reference's
arguments, over the device tensor z.
"""
from __future__ import annotations

import ctypes as C
from time import perf_counter

import numpy as np
import torch

from .. import _lib
from .. import parallel
from . import _harness
from ._harness import Solver


class D_FLOW(Solver):

    def __init__(self, model, device, args):
        super().__init__(model.to(device), device, args)
        self.lib = _lib.load()              # here, not on first use: a missing library fails the constructor
        self.use_graph = True               # one hipGraph per T(z) and per closure
        self.init_latent = None             # optional init_latent(batch, x) replacing the dopri5 solve (parity runs)
        self.blend_noise = None             # optional blend_noise(batch, shape) replacing the randn_like(z) of the blend
        self.dopri5_max_steps = 1000        # attempts (accepted + rejected) before the latent initialisation fails loudly
        self.last_dopri5_stats = None
        self.closure_calls = 0

    # model_forward (d_flow.py:29-34) is Solver's
    def gaussian(self, img):
        if img.ndim != 4:
            raise RuntimeError(f"Expected input `img` to be an 4D tensor, but got {img.shape}")
        return (img ** 2).sum([1, 2, 3]) * 0.5

    def compute_norm(self, img):
        if img.ndim != 4:
            raise RuntimeError(f"Expected input `img` to be an 4D tensor, but got {img.shape}")
        return torch.sqrt((img ** 2).sum([1, 2, 3]))

    # ---- engine calls ------------------------------------------------------------------------------------------------------------
    def _params(self):
        """Schedule of forward_flow_matching (d_flow.py:41-49) with the reference's own fp32 expressions."""
        steps, start = int(self.args.steps_euler), self.args.start_time
        if steps < 2:
            raise ValueError(f"steps_euler must be >= 2, not {steps}")
        delta = (1 - start) / (steps - 1)
        t = np.zeros(steps - 1, dtype=np.float32)
        tm = np.zeros(steps - 1, dtype=np.float32)
        for i in range(steps - 1):
            t1 = torch.ones(1) * delta * i + start
            t[i], tm[i] = float(t1[0]), float((t1 + delta / 2)[0])
        prm = _lib.PfDFlowParams()
        prm.steps_euler = steps
        prm.use_graph = 1 if self.use_graph else 0
        prm.host_t, prm.host_t_mid = t.ctypes.data_as(C.POINTER(C.c_float)), tm.ctypes.data_as(C.POINTER(C.c_float))
        prm.delta, prm.half_delta = float(np.float32(delta)), float(np.float32(delta / 2))
        prm._keep = (t, tm)                # the host tables live as long as the struct
        return prm

    def _latent(self, z):
        return _harness.check_image(z, "latent", self.model, "D_FLOW")

    def forward_flow_matching(self, z):
        """T(z) (d_flow.py:41-49) on the engine."""
        z = self._latent(z)
        self._set_time_scale()
        out = torch.empty_like(z)
        prm = self._params()
        with _lib.solver_stream():
            _lib.check(self.lib.pf_d_flow_forward(self.model.handle, C.byref(prm), z.data_ptr(), out.data_ptr(), z.shape[0], _lib.current_stream_ptr()),
                       self.model.handle, "pf_d_flow_forward")
        return out

    def value_and_grad(self, z, noisy_img, degradation, lmbda):
        """(loss per image [B], d sum(loss) / dz) of the closure (d_flow.py:110-121) at z."""
        z = self._latent(z)
        self._set_time_scale()
        B, Hh = z.shape[0], self.model.input_height
        if noisy_img.shape[0] != B:
            raise ValueError(f"measurement batch {noisy_img.shape[0]} != latent batch {B}")
        y = _harness.check_measurement(noisy_img, degradation, B, self.model)
        d = degradation.descriptor(B, Hh, Hh, z.device)
        loss = torch.empty(B, dtype=torch.float32, device=z.device)
        grad = torch.empty_like(z)
        prm = self._params()
        with _lib.solver_stream():
            _lib.check(self.lib.pf_d_flow_value_and_grad(self.model.handle, C.byref(d), C.byref(prm), z.data_ptr(), y.data_ptr(), float(lmbda),
                                                         loss.data_ptr(), grad.data_ptr(), B, _lib.current_stream_ptr()),
                       self.model.handle, "pf_d_flow_value_and_grad")
        return loss, grad

    def inverse_flow_matching(self, z):
        """odeint(cnf, z, [1, 0], rtol = atol = 1e-5, method='dopri5')[-1] (d_flow.py:51-60) on the engine; counts in last_dopri5_stats."""
        z = self._latent(z)
        self._set_time_scale()
        out = torch.empty_like(z)
        prm = _lib.PfDopri5Params()
        prm.t0, prm.t1, prm.rtol, prm.atol, prm.max_steps = 1.0, 0.0, 1e-5, 1e-5, int(self.dopri5_max_steps)
        stats = (C.c_int64 * 3)()
        with _lib.solver_stream():
            _lib.check(self.lib.pf_flow_ode_dopri5(self.model.handle, C.byref(prm), z.data_ptr(), out.data_ptr(), z.shape[0], stats,
                                                   _lib.current_stream_ptr()), self.model.handle, "pf_flow_ode_dopri5")
        self.last_dopri5_stats = dict(accepted=int(stats[0]), rejected=int(stats[1]), nfev=int(stats[2]))
        return out

    # ---- solver ------------------------------------------------------------------------------------------------------------------
    def solve_ip(self, test_loader, degradation, sigma_noise):
        # LBFGS (one line search over the whole batch) and the dopri5 error norm (one step sequence for the whole batch) couple the
        # images: a split batch would compute something else
        _harness.single_gpu_only(parallel.rank_world()[1], "d_flow runs on one GPU only: its LBFGS line search and its dopri5 step control couple the whole batch")
        H, H_adj = degradation.H, degradation.H_adj
        self.args.sigma_noise = sigma_noise
        loader = iter(test_loader)
        for batch in range(self.args.max_batch):
            (clean_img, labels) = next(loader)
            self.args.batch = batch
            noisy_img = H(clean_img.clone().to(self.device))
            G = noisy_img.shape[0]
            noise = _harness.measurement_noise(self, batch, noisy_img, tuple(noisy_img.shape), 0, G)   # d_flow.py:78-80: gaussian whatever noise_type says
            noisy_img = noisy_img + noise * sigma_noise
            clean_img = clean_img.to('cpu')
            zshape = (G, self.model.input_channels, self.model.input_height, self.model.input_height)
            # the blend's randn_like(z) (d_flow.py:89-91): the draw after the measurement noise on the generator it came from (the dopri5
            # solve in between draws nothing)
            if self.blend_noise is not None:
                eps = self.blend_noise(batch, zshape)
            elif self.measurement_noise_source == "device":
                eps = torch.randn(zshape, dtype=torch.float32, device=self.device)
            else:
                eps = torch.randn(zshape, dtype=torch.float32).to(self.device)

            x = H_adj(noisy_img.clone()).to(self.device)
            z = self.init_latent(batch, x) if self.init_latent is not None else self.inverse_flow_matching(x)
            z = z.to(self.device).float()
            z = np.sqrt(self.args.alpha) * z + np.sqrt(1 - self.args.alpha) * eps.to(self.device)
            z = z.detach().contiguous().requires_grad_(True)

            optim_img = torch.optim.LBFGS([z], max_iter=self.args.LBFGS_iter, history_size=100, line_search_fn='strong_wolfe')
            _harness.begin_batch_stats(self)
            time_per_batch = 0

            def closure():
                optim_img.zero_grad()
                loss, grad = self.value_and_grad(z, noisy_img, degradation, self.args.lmbda)
                z.grad = grad
                self.closure_calls += 1
                return loss.sum()

            restored_img = None
            iteration = 0
            for iteration in range(self.args.max_iter):
                if self.args.compute_time:
                    t0 = perf_counter()
                optim_img.step(closure)
                restored_img = self.forward_flow_matching(z.detach())       # d_flow.py:125 (timed, as in the reference)
                if self.args.compute_time:
                    torch.cuda.synchronize()
                    time_per_batch += perf_counter() - t0
            self.model.check_numerics()
            self.last_restored = restored_img
            self.last_latent = z.detach().clone()

            # the reference times step + forward only (d_flow.py:104-127), so the sum is kept here and not by _harness.batch_stats
            _harness.write_batch_stats(self, batch, time_per_batch)
            if self.args.save_results:
                restored_img = self.forward_flow_matching(z.detach())
                self.write_final(clean_img, noisy_img, restored_img, H_adj, iteration)
        self.write_averages()
