"""Point-spread functions for degradations.PSFDeblurring: a seeded camera-shake trajectory, a defocus disk, or a kernel from a file.
Every kernel is a (size, size) float32 array, non-negative, of sum 1.  numpy only."""
from __future__ import annotations

import numpy as np


def _check_size(size):
    size = int(size)
    if size < 1 or size % 2 == 0:
        raise ValueError(f"a point-spread function needs an odd side >= 1, got {size}")
    return size


def motion_psf(size, seed=0):
    """Camera shake: a random walk with inertia (numpy's Philox generator, key [seed, size]), centred on its mean, scaled to the
    kernel's support and rasterised by bilinear splatting.  Splatting keeps the first moment, so the centroid of the kernel is its
    centre tap (to rounding); the walk is not point-symmetric, so H and H_adj differ."""
    size = _check_size(size)
    if size == 1:
        return np.ones((1, 1), dtype=np.float32)
    g = np.random.Generator(np.random.Philox(key=[int(seed), size]))
    n = 32 * size
    acc = g.standard_normal(size=(n, 2))
    vel = np.zeros(2)
    pos = np.zeros((n, 2))
    for i in range(1, n):
        vel = 0.95 * vel + acc[i]                 # inertia: long smooth strokes with a few sharp turns
        pos[i] = pos[i - 1] + vel
    pos -= pos.mean(axis=0)
    r = size // 2
    pos *= (r - 0.5) / np.abs(pos).max()          # every splat stays inside the support
    k = np.zeros((size, size), dtype=np.float64)
    fy, fx = np.floor(pos[:, 0]), np.floor(pos[:, 1])
    wy, wx = pos[:, 0] - fy, pos[:, 1] - fx
    iy, ix = fy.astype(int) + r, fx.astype(int) + r
    np.add.at(k, (iy, ix), (1 - wy) * (1 - wx)); np.add.at(k, (iy, ix + 1), (1 - wy) * wx)
    np.add.at(k, (iy + 1, ix), wy * (1 - wx)); np.add.at(k, (iy + 1, ix + 1), wy * wx)
    return (k / k.sum()).astype(np.float32)


def disk_psf(size, radius):
    """Defocus: the area of each tap's pixel that a disk of `radius` pixels around the centre covers (8 x 8 sub-samples), normalised."""
    size = _check_size(size)
    radius = float(radius)
    if not radius > 0:
        raise ValueError(f"disk_psf: the radius must be positive, got {radius}")
    sub = (np.arange(size * 8) + 0.5) / 8.0 - size / 2.0        # sub-sample centres, pixel units, 0 = the kernel's centre
    inside = (sub[:, None] ** 2 + sub[None, :] ** 2 <= radius ** 2).astype(np.float64)
    k = inside.reshape(size, 8, size, 8).sum(axis=(1, 3))
    if k.sum() == 0:
        k[size // 2, size // 2] = 1.0
    return (k / k.sum()).astype(np.float32)


def load_psf(path):
    """A kernel from a 2-D .npy file, as float32 (PSFDeblurring checks sides and pads / crops it)."""
    k = np.load(path, allow_pickle=False)
    if k.ndim != 2:
        raise ValueError(f"load_psf: {path} holds an array of shape {k.shape}, a 2-D kernel is needed")
    return np.ascontiguousarray(k, dtype=np.float32)
