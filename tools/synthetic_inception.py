"""Seed-fixed synthetic weights of the FID Inception network (pnpflow_amd.models.InceptionV3) for runs without the published weight
file: He-scaled conv weights, BatchNorm scale and running variance in [0.5, 1.5], small shifts and running means.  An FID on them is
a smoke figure, never comparable with a published one (product-side helper: does not import oracle/)."""
import math
import zlib

import numpy as np
import torch


def synthetic_inception_state_dict(shapes, seed=0):
    """shapes: {published key: shape} (InceptionV3.state_dict_shapes()) -> state_dict of fp32 tensors."""
    sd = {}
    for name, shape in shapes.items():
        rng = np.random.Generator(np.random.Philox(key=[seed, zlib.crc32(name.encode())]))
        if name.endswith(".conv.weight"):
            a = rng.standard_normal(size=shape) * math.sqrt(2.0 / int(np.prod(shape[1:])))
        elif name.endswith(".bn.weight") or name.endswith(".bn.running_var"):
            a = rng.uniform(0.5, 1.5, size=shape)
        else:
            a = rng.uniform(-0.1, 0.1, size=shape)
        sd[name] = torch.from_numpy(a.astype(np.float32))
    return sd
