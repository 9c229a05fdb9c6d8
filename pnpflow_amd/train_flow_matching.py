"""FLOW_MATCHING with the sampling API of pnpflow/train_flow_matching.py (reference :40-262): samples from the flow prior.

    fm = FLOW_MATCHING(model, device, args)
    x = fm.apply_flow_matching(16)                                       # dopri5, t 0 -> 1, rtol = atol = 1e-5
    imgs = fm.generate_samples("euler", n_samples=64, batch_size=16, integration_steps=10)

The reference hands `cnf(model)` to torchdiffeq; here the adaptive solve is pf_flow_ode_dopri5 (torchdiffeq's dopri5 rules) and the
fixed-grid one pf_flow_ode_euler, both on the device.  The latents are torch.randn draws on the device, as in the reference, or injected.
Training the flow is out of scope; compute_fid runs on the engine's Inception network (models.InceptionV3).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


class FLOW_MATCHING(object):

    def __init__(self, model, device, args):
        self.d = getattr(args, "dim_image", None) or model.input_height
        self.num_channels = getattr(args, "num_channels", None) or model.input_channels
        self.device = device
        self.args = args
        self.lr = getattr(args, "lr", None)
        self.model = model.to(device)
        self.coupling = getattr(args, "model", None)
        self.lib = _lib.load()
        self.dopri5_max_steps = 1000        # attempts (accepted + rejected) before a solve fails loudly
        self.last_dopri5_stats = None

    # ---- engine calls ------------------------------------------------------------------------------------------------------------
    def _prepare(self, latent):
        Hh = self.model.input_height
        if latent.ndim != 4 or tuple(latent.shape[1:]) != (self.model.input_channels, Hh, Hh):
            raise ValueError(f"latent of shape {tuple(latent.shape)} does not match the net's (B, {self.model.input_channels}, {Hh}, {Hh})")
        if not latent.is_cuda:
            raise _lib.PnpFlowHipError("FLOW_MATCHING needs GPU tensors (there is no CPU path)")
        if hasattr(self.model, "set_solver_time_scale"):
            self.model.set_solver_time_scale(1.0)          # cnf.forward (train_flow_matching.py:258-262): model(x, t) with t as it is
        return latent.detach().contiguous().float()

    def _dopri5(self, latent, t0, t1, tol):
        z = self._prepare(latent)
        out = torch.empty_like(z)
        prm = _lib.PfDopri5Params()
        prm.t0, prm.t1, prm.rtol, prm.atol, prm.max_steps = float(t0), float(t1), float(tol), float(tol), int(self.dopri5_max_steps)
        stats = (C.c_int64 * 3)()
        with _lib.solver_stream():
            _lib.check(self.lib.pf_flow_ode_dopri5(self.model.handle, C.byref(prm), z.data_ptr(), out.data_ptr(), z.shape[0], stats,
                                                   _lib.current_stream_ptr()), self.model.handle, "pf_flow_ode_dopri5")
        self.last_dopri5_stats = dict(accepted=int(stats[0]), rejected=int(stats[1]), nfev=int(stats[2]))
        return out

    def _latent(self, count, num_channels, latent, first=0):
        if latent is not None:
            return latent[first:first + count].to(self.device)
        return torch.randn(count, num_channels, self.d, self.d, device=self.device)

    @staticmethod
    def sample_schedule(n_samples, batch_size, integration_steps, tmax):
        """(batch sizes, fp32 time grid) of generate_samples (train_flow_matching.py:177-188)."""
        if batch_size is None:
            batch_size = n_samples
        batches = [batch_size] * (n_samples // batch_size)
        if n_samples % batch_size:
            batches += [n_samples % batch_size]
        return batches, torch.linspace(0, tmax, int(tmax * integration_steps))

    # ---- the reference's sampling surface ------------------------------------------------------------------------------------------
    def apply_flow_matching(self, NO_samples, latent=None):
        """odeint(cnf(model), latent, [0, 1], atol = rtol = 1e-5, method='dopri5')[-1] (train_flow_matching.py:131-150)."""
        if latent is not None and latent.shape[0] != NO_samples:
            raise ValueError(f"latent holds {latent.shape[0]} samples, NO_samples is {NO_samples}")
        return self._dopri5(self._latent(NO_samples, self.num_channels, latent), 0.0, 1.0, 1e-5)

    def generate_samples(self, integration_method="dopri5", tol=1e-5, n_samples=1028, batch_size=None, num_channels=3, integration_steps=100, tmax=1,
                         latent=None):
        """(n_samples, num_channels, d, d) samples (train_flow_matching.py:170-198): per batch, x0 ~ N(0, I) integrated over
        torch.linspace(0, tmax, int(tmax * integration_steps)) by 'euler' (the fixed grid) or 'dopri5' (first to last grid point)."""
        if integration_method not in ("euler", "dopri5"):
            raise NotImplementedError(f"integration method {integration_method!r} is not implemented by this engine ('euler' and 'dopri5' are)")
        if latent is not None and latent.shape[0] != n_samples:
            raise ValueError(f"latent holds {latent.shape[0]} samples, n_samples is {n_samples}")
        batches, time_points = self.sample_schedule(n_samples, batch_size, integration_steps, tmax)
        if time_points.numel() < 2:
            raise ValueError(f"int(tmax * integration_steps) = {time_points.numel()} grid points: at least 2 are needed")
        images_list, first = [], 0
        for batch in batches:
            x0 = self._prepare(self._latent(batch, num_channels, latent, first))
            first += batch
            if integration_method == "euler":
                images_list.append(self.model.euler(x0, time_points))
            else:
                images_list.append(self._dopri5(x0, float(time_points[0]), float(time_points[-1]), tol))
        return torch.cat(images_list, dim=0)

    # ---- training: out of scope of this engine; FID -------------------------------------------------------------------------------
    def train_FM_model(self, train_loader, opt, num_epoch):
        raise NotImplementedError("training the flow-matching model is not implemented by this engine (inference only)")

    def train(self, data_loaders):
        raise NotImplementedError("training the flow-matching model is not implemented by this engine (inference only)")

    def sample_plot(self, x, ep=None):
        raise NotImplementedError("sample_plot belongs to the training loop, which is not implemented by this engine; tools/prior_report.py writes a sample grid")

    def compute_fid(self, num_images_fid, train_feat, ft_extractor, batch_size=512, integration_method="dopri5", integration_steps=100, epoch='final'):
        """FID of num_images_fid samples (generate_samples at tol 1e-4, train_flow_matching.py:200-214) against `train_feat`, the (N, dims)
        features of the training images from the same `ft_extractor`, a pnpflow_amd.models.InceptionV3.  The reference's goes through the
        `fld` package (absent): its extractor takes uint8 images; here the PREPROCESSING IS PYTORCH-FID'S - samples mapped from [-1, 1] to
        [0, 1] and clipped, resized to 299 x 299 and normalised by the network - and the distance is fid_score.calculate_frechet_distance.
        The grid of the first 16 samples goes to training_images/<dataset>/gen_images_epoch<epoch>.png as in the reference."""
        import os

        import numpy as np

        from .models import InceptionV3
        if not isinstance(ft_extractor, InceptionV3) or train_feat is None:
            raise NotImplementedError("compute_fid takes a pnpflow_amd.models.InceptionV3 as ft_extractor and its (N, dims) features of the training images as "
                                      "train_feat; the reference's `fld` feature extractors are not implemented by this engine")

        from . import fid_score as fs
        from . import utils
        gen_images = self.generate_samples(integration_method=integration_method, tol=1e-4, n_samples=num_images_fid, batch_size=batch_size,
                                           num_channels=self.num_channels, integration_steps=integration_steps)
        imgs = (gen_images * 0.5 + 0.5).clip(0, 1)
        if imgs.shape[1] == 1:
            imgs = imgs.expand(-1, 3, -1, -1)
        train_feat = np.asarray(train_feat.cpu() if torch.is_tensor(train_feat) else train_feat, dtype=np.float64)
        gen_feat = fs.get_activations(imgs, ft_extractor, min(50, len(imgs)), train_feat.shape[1], self.device)
        fid_val = fs.calculate_frechet_distance(np.mean(train_feat, axis=0), np.cov(train_feat, rowvar=False), np.mean(gen_feat, axis=0), np.cov(gen_feat, rowvar=False))
        os.makedirs(f"training_images/{self.args.dataset}", exist_ok=True)
        grid = imgs[:16].permute(0, 2, 3, 1).cpu().numpy()
        utils._imshow_grid(f"training_images/{self.args.dataset}/gen_images_epoch{epoch}.png", grid, gray=self.num_channels == 1)
        return fid_val
