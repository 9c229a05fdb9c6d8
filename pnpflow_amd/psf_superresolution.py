"""PSFSuperresolution: superresolution through a blur kernel, y = (k (*) x) decimated by sf, with the API of the operators of degradations.py
(reached as `degradations.PSFSuperresolution`).  Kernels: psf.py; device code: csrc/psf.hip (one launch per application), csrc/fft2.hip (the
aliased spectrum and the Fourier solves on the low-resolution grid)."""
from __future__ import annotations

import torch

from . import _lib
from .degradations import Degradation
from .psf_deblurring import sanitise_kernel


class PSFSuperresolution(Degradation):
    """Blur with any real 2-D point-spread function, then keep every sf-th sample: what the reference's Superresolution(mode="bicubic") computes
    when its `.filter` holds the PSF (degradations.py:113-127).  H is the circular convolution of PSFDeblurring(mode='fft') sampled at
    (i sf, j sf), H_adj the zero-fill followed by the circular correlation (PF_DEG_PSF_SR).  The engine computes the K^2 multiply-adds of the
    low-resolution outputs only and the adjoint in its polyphase form; H H^T is circulant on the low-resolution grid, which gives OT-ODE and
    the hqs prox of pnp_gs one Fourier solve there.
    `kernel`: as PSFDeblurring (2-D, odd sides <= 63, padded to a square, zero rings cropped); `sf`: 1 .. 8, dividing dim_image."""
    kind = _lib.PF_DEG_PSF_SR

    def __init__(self, kernel, sf, num_channels=3, dim_image=128, device="cuda"):
        super().__init__()
        sq, K = sanitise_kernel(kernel, "PSFSuperresolution")
        if int(sf) != sf or not 1 <= sf <= _lib.PSF_SR_MAX_SF:
            raise ValueError(f"PSFSuperresolution: sf must be an integer in 1 .. {_lib.PSF_SR_MAX_SF}, got {sf}")
        if dim_image % sf:
            raise ValueError(f"PSFSuperresolution: sf = {sf} does not divide the image side {dim_image}")
        if K > dim_image:
            raise ValueError(f"PSFSuperresolution: the {K} x {K} kernel does not fit the {dim_image} x {dim_image} filter")
        self.sf, self.mode, self.kernel_size = int(sf), "psf", K
        self.taps_host = sq
        self.num_channels, self.dim_image, self._device = num_channels, dim_image, device
        self._taps, self._filter = {}, None

    @property
    def kernel(self):
        """The (K, K) fp32 taps."""
        return torch.from_numpy(self.taps_host)

    @property
    def filter(self):
        """The reference's attribute (degradations.py:103-109): the kernel zero-padded to (1, C, dim, dim) and rolled so that its centre sits
        at (0, 0)."""
        if self._filter is None:
            K, D = self.kernel_size, self.dim_image
            f = torch.zeros((1, self.num_channels, D, D), dtype=torch.float32)
            f[:, :, :K, :K] = torch.from_numpy(self.taps_host)
            f = torch.roll(f, shifts=(-(K - 1) // 2, -(K - 1) // 2), dims=(2, 3))
            self._filter = f.to(self._device if torch.cuda.is_available() else "cpu")
        return self._filter

    def descriptor(self, B, H, W, device):
        key = str(device)
        if key not in self._taps:
            self._taps[key] = torch.from_numpy(self.taps_host).to(device)
        d = _lib.PfDegradation(); d.kind = self.kind; d.sf = self.sf; d.ntaps = int(self.kernel_size)
        d.taps = self._taps[key].data_ptr()
        return d

    def H(self, x):
        return self._apply(x, False)

    def H_adj(self, x):
        return self._apply(x, True, out_hw=(x.shape[2] * self.sf, x.shape[3] * self.sf))
