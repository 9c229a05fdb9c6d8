"""PSFDeblurring: blur with any real 2-D point-spread function, with the API of the operators of degradations.py (reached as
`degradations.PSFDeblurring`).  Kernels: psf.py; device code: csrc/psf.hip, csrc/fft2.hip."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .degradations import Degradation


def sanitise_kernel(kernel, who):
    """A real, finite 2-D kernel with odd sides <= 63 -> (square fp32 taps, side): a rectangular kernel is zero-padded, centred, to a square, and
    all-zero border rings are cropped (no non-zero tap is dropped, the centre stays the centre).  `who` prefixes the error messages."""
    k = np.asarray(kernel.detach().cpu().numpy() if isinstance(kernel, torch.Tensor) else kernel)
    if k.ndim != 2 or k.size == 0 or np.iscomplexobj(k) or not np.issubdtype(k.dtype, np.number):
        raise ValueError(f"{who}: the kernel must be a real 2-D array, got shape {k.shape} dtype {k.dtype}")
    k = k.astype(np.float32)
    if not np.isfinite(k).all():
        raise ValueError(f"{who}: the kernel has non-finite taps")
    if k.shape[0] % 2 == 0 or k.shape[1] % 2 == 0:
        raise ValueError(f"{who}: both sides of the kernel must be odd (its centre is a tap), got {k.shape}")
    if max(k.shape) > _lib.PSF_MAX_SIDE:
        raise ValueError(f"{who}: kernel sides are limited to {_lib.PSF_MAX_SIDE}, got {k.shape}")
    K = max(k.shape)
    sq = np.zeros((K, K), dtype=np.float32)
    oy, ox = (K - k.shape[0]) // 2, (K - k.shape[1]) // 2
    sq[oy:oy + k.shape[0], ox:ox + k.shape[1]] = k
    while K > 1 and not (sq[0].any() or sq[-1].any() or sq[:, 0].any() or sq[:, -1].any()):
        sq, K = sq[1:-1, 1:-1], K - 2
    return np.ascontiguousarray(sq), K


class PSFDeblurring(Degradation):
    """Blur with any real 2-D point-spread function: what the reference computes when GaussianDeblurring's `.kernel` / `.filter` hold the
    PSF (degradations.py:55-89).  mode 'fft': the circular convolution, H_adj the circular correlation (PF_DEG_PSF_BLUR).  Any other
    mode: F.conv2d(padding='same'), i.e. the zero-boundary correlation, H_adj the zero-boundary convolution (PF_DEG_PSF_BLUR_ZERO) - the
    true adjoint, which the reference's own spatial H_adj (the same conv2d) is not for an asymmetric kernel.
    `kernel`: 2-D, odd sides <= 63; a rectangular kernel is zero-padded, centred, to a square, and all-zero border rings are cropped
    (no non-zero tap is dropped, the centre stays the centre)."""
    kind = _lib.PF_DEG_PSF_BLUR

    def __init__(self, kernel, mode="fft", num_channels=3, dim_image=128, device="cuda"):
        super().__init__()
        sq, K = sanitise_kernel(kernel, "PSFDeblurring")
        if mode == "fft" and K > dim_image:
            raise ValueError(f"PSFDeblurring(mode='fft'): the {K} x {K} kernel does not fit the {dim_image} x {dim_image} filter")
        self.kind = _lib.PF_DEG_PSF_BLUR if mode == "fft" else _lib.PF_DEG_PSF_BLUR_ZERO
        self.mode, self.kernel_size = mode, K
        self.taps_host = np.ascontiguousarray(sq)
        self.num_channels, self.dim_image, self._device = num_channels, dim_image, device
        self._taps, self._filter = {}, None

    @property
    def kernel(self):
        """The reference's attribute: the (K, K) fp32 taps."""
        return torch.from_numpy(self.taps_host)

    @property
    def filter(self):
        """The reference's attribute (degradations.py:59-69): the kernel zero-padded to (1, C, dim, dim) and rolled so that its centre
        sits at (0, 0)."""
        if self._filter is None:
            K, D = self.kernel_size, self.dim_image
            if K > D:
                raise ValueError(f"PSFDeblurring.filter: the {K} x {K} kernel does not fit a {D} x {D} filter")
            f = torch.zeros((1, self.num_channels, D, D), dtype=torch.float32)
            f[:, :, :K, :K] = torch.from_numpy(self.taps_host)
            f = torch.roll(f, shifts=(-(K - 1) // 2, -(K - 1) // 2), dims=(2, 3))
            self._filter = f.to(self._device if torch.cuda.is_available() else "cpu")
        return self._filter

    def descriptor(self, B, H, W, device):
        key = str(device)
        if key not in self._taps:
            self._taps[key] = torch.from_numpy(self.taps_host).to(device)
        d = _lib.PfDegradation(); d.kind = self.kind; d.ntaps = int(self.kernel_size)
        d.taps = self._taps[key].data_ptr()
        return d

    def H(self, x):
        return self._apply(x, False)

    def H_adj(self, x):
        return self._apply(x, True)
