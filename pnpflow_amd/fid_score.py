"""Frechet Inception Distance with the functions and signatures of the reference's pnpflow/fid_score.py (:21-197, adapted there from
pytorch-fid): Inception features on the HIP engine (csrc/inception.hip), statistics and distance in fp64 on the host.

    d^2 = |mu1 - mu2|^2 + Tr(C1 + C2 - 2 sqrt(C1 C2))

`model` is a pnpflow_amd.models.InceptionV3 (or anything whose call returns [(B, dims, h, w)]).  The Frechet distance is pinned against
the reference (tests/golden/fid_frechet.npz); the network is PARITY UNPINNED (see csrc/inception.hip).
"""
from __future__ import annotations

import numpy as np
import torch
from scipy import linalg


def get_activations(images, model, batch_size=50, dims=2048, device='cpu'):
    """(len(images), dims) fp64 array of the model's features (fid_score.py:21-71): images (N, 3, H, W) in [0, 1], numpy or tensor, walked in
    batches of batch_size (the last one may be smaller), every output that still has a spatial extent averaged over it."""
    model.eval()
    n = len(images)
    if batch_size > n:
        print('Warning: batch size is bigger than the data size. Setting batch size to data size')
        batch_size = n
    pred_arr = np.empty((n, dims))
    for start in range(0, n, max(batch_size, 1)):
        batch = torch.as_tensor(images[start:start + batch_size]).to(device)
        with torch.no_grad():
            pred = model(batch)[0]
        if pred.size(2) != 1 or pred.size(3) != 1:
            pred = pred.mean(dim=(2, 3), keepdim=True)
        pred_arr[start:start + pred.shape[0]] = pred.squeeze(3).squeeze(2).cpu().numpy()
    return pred_arr


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """Frechet distance of N(mu1, sigma1) and N(mu2, sigma2) (fid_score.py:74-128), with the reference's two stabilisation branches
    (:109-123): a non-finite sqrtm is retried with eps on both diagonals; an imaginary part of the root is dropped when its diagonal is
    below 1e-3 and is an error otherwise."""
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape, 'Training and test mean vectors have different lengths'
    assert sigma1.shape == sigma2.shape, 'Training and test covariances have different dimensions'
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        print('fid calculation produces singular product; adding %s to diagonal of cov estimates' % eps)
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError('Imaginary component {}'.format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def calculate_activation_statistics(images, model, batch_size=50, dims=2048, device='cpu'):
    """(mean, covariance) of the features over the images, fp64 (fid_score.py:131-156: np.mean, np.cov(rowvar=False))."""
    act = get_activations(images, model, batch_size, dims, device)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def evaluate_fid_score(images1, images2, batch_size=50, model=None):
    """FID of two image sets (N, H, W, C) in [0, 1] at 2048 dimensions (fid_score.py:159-197).  The reference builds its InceptionV3 here,
    downloading the weights; this engine loads them from disk (pnpflow_amd.models.load_fid_inception) unless `model` is given."""
    device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
    if model is None:
        from .models import InceptionV3, load_fid_inception
        model, _real = load_fid_inception([InceptionV3.BLOCK_INDEX_BY_DIM[2048]])
    if images1.shape[-1] == 1:
        images1 = np.concatenate([images1, images1, images1], axis=-1)
    if images2.shape[-1] == 1:
        images2 = np.concatenate([images2, images2, images2], axis=-1)
    if np.max(images1) > 1 or np.min(images1) < 0 or np.max(images2) > 1 or np.min(images2) < 0:
        import warnings
        warnings.warn('FID score: the values of images should be in range [0,1].')
    images1 = np.transpose(images1, axes=(0, 3, 1, 2))
    images2 = np.transpose(images2, axes=(0, 3, 1, 2))
    m1, s1 = calculate_activation_statistics(images1, model, batch_size, 2048, device)
    m2, s2 = calculate_activation_statistics(images2, model, batch_size, 2048, device)
    return calculate_frechet_distance(m1, s1, m2, s2)
