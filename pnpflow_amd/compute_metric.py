"""`ComputeMetric` of the reference (pnpflow/compute_metric.py:7-45): the FID of prior samples against test images, on the HIP engine.

    ComputeMetric(data_loaders, FLOW_MATCHING(model, device, args), device, args).compute_metrics(5000)

What the reference does, quirks included, is kept:
  * the real images are the FIRST `num_samples` of ONE test batch (next(iter(test loader))): a loader with a smaller batch gives fewer;
  * grayscale images are tiled to three channels;
  * the samples come from 50 rounds of apply_flow_matching(num_samples // 50): num_samples below 50 draws nothing, a remainder is dropped;
  * samples are clipped to [0, 1]; the test images are passed AS THE LOADER GIVES THEM (the reference's loaders give [-1, 1]; no rescale
    happens there and none happens here);
  * batches of 50 through the Inception network, `Epoch: final, FID: <value>` appended to <output_root>results/<dataset>/metrics.txt.
Added: args.fid_dims (64 / 192 / 768 / 2048, default 2048: the reference's) picks the output block; args.synthetic opts into synthetic
Inception weights when the published file is absent; `results_dir` names the folder under output_root ("results" unless the caller moves
synthetic runs to "results_synthetic"), and a PARITY_UNPINNED.txt beside metrics.txt says that the network is not pinned against torchvision.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import fid_score as fs
from .models import InceptionV3, load_fid_inception

N_ITER = 50          # sampling rounds (compute_metric.py:31)
BATCH_SIZE = 50      # images per Inception batch (compute_metric.py:26)


def three_channels(x):
    """(N, H, W, C) numpy -> (N, 3, H, W), a single channel tiled (compute_metric.py:22-25, 36-39)."""
    if x.shape[-1] == 1:
        x = np.concatenate([x, x, x], axis=-1)
    return np.transpose(x, axes=(0, 3, 1, 2))


class ComputeMetric:
    def __init__(self, full_data, generative_method, device, args, incep_model=None, results_dir="results"):
        self.test_set = full_data['test']
        self.device = device
        self.args = args
        self.generative_method = generative_method
        self.incep_model = incep_model
        self.save_path = args.output_root + '{}/{}/'.format(results_dir, args.dataset)
        self.last_fid = None

    def compute_metrics(self, num_samples):
        dims = int(getattr(self.args, "fid_dims", 2048) or 2048)
        if dims not in InceptionV3.BLOCK_INDEX_BY_DIM:
            raise ValueError(f"fid_dims must be one of {sorted(InceptionV3.BLOCK_INDEX_BY_DIM)}, not {dims}")
        incep_model = self.incep_model
        if incep_model is None:
            incep_model, _real = load_fid_inception([InceptionV3.BLOCK_INDEX_BY_DIM[dims]], output_root=self.args.output_root,
                                                    synthetic=bool(getattr(self.args, "synthetic", False)),
                                                    device_index=getattr(self.args, "device_index", 0) or 0)
        data_v = next(iter(self.test_set))
        gt = data_v[0].to(self.device)[:num_samples]
        gt = three_channels(gt.permute(0, 2, 3, 1).cpu().numpy())
        m1, s1 = fs.calculate_activation_statistics(gt, incep_model, BATCH_SIZE, dims, self.device)

        samples = torch.empty(0).to(self.device)
        for i in range(N_ITER):
            print('Iteration: ', i)
            samples = torch.cat([samples, self.generative_method.apply_flow_matching(num_samples // N_ITER)], dim=0)
        gen = three_channels(torch.clip(samples.permute(0, 2, 3, 1), 0, 1).cpu().numpy())
        m2, s2 = fs.calculate_activation_statistics(gen, incep_model, BATCH_SIZE, dims, self.device)
        fid_value = fs.calculate_frechet_distance(m1, s1, m2, s2)
        self.last_fid = float(fid_value)

        os.makedirs(self.save_path, exist_ok=True)
        with open(self.save_path + 'metrics.txt', 'a') as file:
            file.write(f'Epoch: final, FID: {fid_value}\n')
        note, line = self.save_path + 'PARITY_UNPINNED.txt', ("metrics.txt, FID: the Inception network is restated from pytorch-fid's published FID Inception "
                                                              "(torchvision is not installed in the build image); the Frechet distance is pinned against the reference\n")
        if not os.path.isfile(note) or line not in open(note).read():
            with open(note, 'a') as file:
                file.write(line)
        return fid_value
