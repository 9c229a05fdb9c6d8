"""GRADIENT_STEP_DENOISER with the inference API of pnpflow/train_denoiser.py (reference :16-76; Hurault et al., "Gradient step
denoiser for convergent plug-and-play", 2022).

The regulariser is g(x) = 0.5 |x - N(x, sigma)|^2 with N the U-Net; its gradient

    Dg(x) = (x - N) - J_N(x)^T (x - N)

is what the reference obtains from torch.autograd.grad.  Here it is one engine call (pf_gs_denoiser_grad): a retained forward, the seed
x - N, the hand-written backward and the combine, all on the device.  Training the denoiser is out of scope.
"""
from __future__ import annotations

import torch

from . import _lib


class GRADIENT_STEP_DENOISER(object):

    def __init__(self, model, device, args):
        self.d = getattr(args, "dim_image", None)
        self.num_channels = getattr(args, "num_channels", None)
        self.device = device
        self.args = args
        self.lr = getattr(args, "lr", None)
        self.model = model.to(device)
        self.lib = _lib.load()
        self.sigma_step = False
        self.weight_Ds = 1.
        self.grad_matching = True

    # the engine net underneath (what PROX_PNP hands to pf_pnp_gs_restore)
    @property
    def handle(self):
        return self.model.handle

    @property
    def input_channels(self):
        return self.model.input_channels

    @property
    def input_height(self):
        return self.model.input_height

    def to(self, device=None):
        self.model.to(device)
        return self

    def eval(self):
        self.model.eval()
        return self

    def load_state_dict(self, *a, **k):
        return self.model.load_state_dict(*a, **k)

    def set_precision(self, mode):
        return self.model.set_precision(mode)

    def check_numerics(self):
        return self.model.check_numerics()

    def memory_bytes(self):
        return self.model.memory_bytes()

    def calculate_grad(self, x, sigma, compute_g=False):
        """(Dg(x), N(x)[, g]) of train_denoiser.py:39-57; sigma: [B] denoiser levels (a 0-d tensor or a number is broadcast)."""
        if not x.is_cuda:
            raise _lib.PnpFlowHipError("GRADIENT_STEP_DENOISER needs GPU tensors (there is no CPU path)")
        Hh = self.model.input_height
        if x.ndim != 4 or tuple(x.shape[1:]) != (self.model.input_channels, Hh, Hh):
            raise ValueError(f"input of shape {tuple(x.shape)} does not match the net's (B, {self.model.input_channels}, {Hh}, {Hh})")
        x = x.detach().contiguous().float()
        B = x.shape[0]
        sigma = torch.as_tensor(sigma, dtype=torch.float32, device=x.device).reshape(-1)
        if sigma.numel() == 1:
            sigma = sigma.expand(B)
        if sigma.numel() != B:
            raise ValueError(f"sigma has {sigma.numel()} entries for a batch of {B}")
        sigma = sigma.contiguous()
        Dg, N = torch.empty_like(x), torch.empty_like(x)
        g = torch.empty(1, dtype=torch.float64, device=x.device) if compute_g else None
        _lib.check(self.lib.pf_gs_denoiser_grad(self.model.handle, x.data_ptr(), sigma.data_ptr(), Dg.data_ptr(), N.data_ptr(),
                                                g.data_ptr() if compute_g else None, B, _lib.current_stream_ptr()),
                   self.model.handle, "pf_gs_denoiser_grad")
        if compute_g:
            return Dg, N, g[0].float()
        return Dg, N

    def forward(self, x, sigma):
        """(x_hat, Dg) of train_denoiser.py:59-76 (gradient-step form, weight 1)."""
        Dg, _ = self.calculate_grad(x, sigma)
        if self.sigma_step:
            x_hat = x - self.weight_Ds * torch.as_tensor(sigma, device=x.device).reshape(-1, 1, 1, 1) * Dg
        else:
            x_hat = x - self.weight_Ds * Dg
        return x_hat, Dg

    __call__ = forward

    # ---- training: out of scope of this engine ---------------------------------------------------------------------------------
    def configure_optimizers(self):
        raise NotImplementedError("training the gradient-step denoiser is not implemented by this engine (inference only)")

    def train_denoiser(self, train_loader, opt, num_epoch):
        raise NotImplementedError("training the gradient-step denoiser is not implemented by this engine (inference only)")

    def train(self, data_loaders):
        raise NotImplementedError("training the gradient-step denoiser is not implemented by this engine (inference only)")
