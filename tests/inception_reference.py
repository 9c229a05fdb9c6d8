"""Plain-torch restatement of the FID Inception network (csrc/inception.hip, csrc/inception_plan.h), for the tests: the layer table as
data, synthetic weights under the published key names, and a forward that runs in fp64 or fp32 on the CPU.

A layer is BasicConv2d: conv without bias, BatchNorm on the running statistics with eps 1e-3, ReLU.  torchvision is not installed, so
nothing here is checked against it (PARITY UNPINNED); the table is the specification the kernels are held to.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3
BLOCK_DIMS = (64, 192, 768, 2048)


def _t(name, ci, co, k=1, s=1, p=0):
    kh, kw = (k, k) if isinstance(k, int) else k
    ph, pw = (p, p) if isinstance(p, int) else p
    return (name, ci, co, kh, kw, s, ph, pw)


def layer_table():
    """[(name, Cin, Cout, KH, KW, stride, PH, PW)] in network order: 94 convs."""
    L = [_t("Conv2d_1a_3x3", 3, 32, 3, 2), _t("Conv2d_2a_3x3", 32, 32, 3), _t("Conv2d_2b_3x3", 32, 64, 3, 1, 1), _t("Conv2d_3b_1x1", 64, 80),
         _t("Conv2d_4a_3x3", 80, 192, 3)]
    for n, ci, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        L += [_t(n + ".branch1x1", ci, 64), _t(n + ".branch5x5_1", ci, 48), _t(n + ".branch5x5_2", 48, 64, 5, 1, 2), _t(n + ".branch3x3dbl_1", ci, 64),
              _t(n + ".branch3x3dbl_2", 64, 96, 3, 1, 1), _t(n + ".branch3x3dbl_3", 96, 96, 3, 1, 1), _t(n + ".branch_pool", ci, pf)]
    L += [_t("Mixed_6a.branch3x3", 288, 384, 3, 2), _t("Mixed_6a.branch3x3dbl_1", 288, 64), _t("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1),
          _t("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)]
    for n, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        L += [_t(n + ".branch1x1", 768, 192), _t(n + ".branch7x7_1", 768, c7), _t(n + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3)),
              _t(n + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0)), _t(n + ".branch7x7dbl_1", 768, c7), _t(n + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)),
              _t(n + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3)), _t(n + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)),
              _t(n + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3)), _t(n + ".branch_pool", 768, 192)]
    L += [_t("Mixed_7a.branch3x3_1", 768, 192), _t("Mixed_7a.branch3x3_2", 192, 320, 3, 2), _t("Mixed_7a.branch7x7x3_1", 768, 192),
          _t("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)), _t("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0)),
          _t("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)]
    for n, ci in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        L += [_t(n + ".branch1x1", ci, 320), _t(n + ".branch3x3_1", ci, 384), _t(n + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)),
              _t(n + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0)), _t(n + ".branch3x3dbl_1", ci, 448), _t(n + ".branch3x3dbl_2", 448, 384, 3, 1, 1),
              _t(n + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)), _t(n + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0)), _t(n + ".branch_pool", ci, 192)]
    return L


LAYERS = {t[0]: t for t in layer_table()}


def synthetic_state_dict(seed=0):
    """He-scaled conv weights, BatchNorm scale and variance in [0.5, 1.5], small shifts and means, under the published key names (fp32)."""
    sd = {}
    for (name, ci, co, kh, kw, _s, _ph, _pw) in layer_table():
        g = np.random.Generator(np.random.Philox(key=[seed, zlib.crc32(name.encode())]))
        sd[name + ".conv.weight"] = torch.from_numpy((g.standard_normal((co, ci, kh, kw)) * np.sqrt(2.0 / (ci * kh * kw))).astype(np.float32))
        sd[name + ".bn.weight"] = torch.from_numpy(g.uniform(0.5, 1.5, co).astype(np.float32))
        sd[name + ".bn.bias"] = torch.from_numpy(g.uniform(-0.1, 0.1, co).astype(np.float32))
        sd[name + ".bn.running_mean"] = torch.from_numpy(g.uniform(-0.1, 0.1, co).astype(np.float32))
        sd[name + ".bn.running_var"] = torch.from_numpy(g.uniform(0.5, 1.5, co).astype(np.float32))
    return sd


def basic_conv(sd, name, x):
    (_n, _ci, _co, _kh, _kw, s, ph, pw) = LAYERS[name]
    d = x.dtype
    y = F.conv2d(x, sd[name + ".conv.weight"].to(d), None, stride=s, padding=(ph, pw))
    return F.relu(F.batch_norm(y, sd[name + ".bn.running_mean"].to(d), sd[name + ".bn.running_var"].to(d), sd[name + ".bn.weight"].to(d),
                               sd[name + ".bn.bias"].to(d), False, 0.0, BN_EPS))


def _avg(x):
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


def _block_a(sd, n, x):
    c = lambda b, v: basic_conv(sd, n + "." + b, v)
    return torch.cat([c("branch1x1", x), c("branch5x5_2", c("branch5x5_1", x)), c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x))),
                      c("branch_pool", _avg(x))], 1)


def _block_b(sd, n, x):
    c = lambda b, v: basic_conv(sd, n + "." + b, v)
    return torch.cat([c("branch3x3", x), c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x))), F.max_pool2d(x, 3, 2)], 1)


def _block_c(sd, n, x):
    c = lambda b, v: basic_conv(sd, n + "." + b, v)
    d = x
    for b in ("branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"):
        d = c(b, d)
    return torch.cat([c("branch1x1", x), c("branch7x7_3", c("branch7x7_2", c("branch7x7_1", x))), d, c("branch_pool", _avg(x))], 1)


def _block_d(sd, n, x):
    c = lambda b, v: basic_conv(sd, n + "." + b, v)
    d = x
    for b in ("branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"):
        d = c(b, d)
    return torch.cat([c("branch3x3_2", c("branch3x3_1", x)), d, F.max_pool2d(x, 3, 2)], 1)


def _block_e(sd, n, x, max_pool):
    c = lambda b, v: basic_conv(sd, n + "." + b, v)
    a = c("branch3x3_1", x)
    d = c("branch3x3dbl_2", c("branch3x3dbl_1", x))
    pooled = F.max_pool2d(x, 3, 1, 1) if max_pool else _avg(x)
    return torch.cat([c("branch1x1", x), c("branch3x3_2a", a), c("branch3x3_2b", a), c("branch3x3dbl_3a", d), c("branch3x3dbl_3b", d), c("branch_pool", pooled)], 1)


def forward(sd, x, resize_input=True, normalize_input=True, dtype=torch.float64, last_block=3):
    """[block 0, ..., block last_block] feature maps (B, C, H, W) of images x (B, 3, H, W) in (0, 1), computed in `dtype` on the CPU."""
    x = x.to(dtype)
    if resize_input:
        x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
    if normalize_input:
        x = 2 * x - 1
    out = []
    for n in ("Conv2d_1a_3x3", "Conv2d_2a_3x3", "Conv2d_2b_3x3"):
        x = basic_conv(sd, n, x)
    x = F.max_pool2d(x, 3, 2); out.append(x)
    if last_block == 0:
        return out
    x = basic_conv(sd, "Conv2d_4a_3x3", basic_conv(sd, "Conv2d_3b_1x1", x))
    x = F.max_pool2d(x, 3, 2); out.append(x)
    if last_block == 1:
        return out
    for n in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = _block_a(sd, n, x)
    x = _block_b(sd, "Mixed_6a", x)
    for n in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        x = _block_c(sd, n, x)
    out.append(x)
    if last_block == 2:
        return out
    x = _block_d(sd, "Mixed_7a", x)
    x = _block_e(sd, "Mixed_7b", x, False)
    x = _block_e(sd, "Mixed_7c", x, True)
    out.append(x.mean(dim=(2, 3), keepdim=True))
    return out


def features(sd, x, resize_input=True, normalize_input=True, dtype=torch.float64, last_block=3):
    """[(B, dims)] per block: the spatial average the FID takes of every block (the identity for block 3)."""
    return [f.mean(dim=(2, 3)) for f in forward(sd, x, resize_input, normalize_input, dtype, last_block)]


def images(B, H, W, seed):
    """(B, 3, H, W) fp32 images in (0, 1): smooth structure plus noise, so that resizing and pooling see gradients and edges."""
    g = np.random.Generator(np.random.Philox(key=[seed, B * 1000003 + H * 1009 + W]))
    x = g.uniform(0.0, 1.0, (B, 3, H, W))
    yy, xx = np.meshgrid(np.linspace(0, 3, H), np.linspace(0, 3, W), indexing="ij")
    x = 0.5 * x + 0.25 * (1 + np.sin(yy * (1 + g.uniform(0, 2, (B, 3, 1, 1))) + xx * g.uniform(0, 2, (B, 3, 1, 1))))
    return torch.from_numpy(np.clip(x, 0.0, 1.0).astype(np.float32))


def bound(hip, ref64, ref32, margin=4.0):
    """(error of hip, allowed): max |hip - fp64| against `margin` x the fp32 CPU run's error on the same input plus one fp32 ulp of the output maximum."""
    ref64 = ref64.double()
    err = float((hip.double() - ref64).abs().max())
    err32 = float((ref32.double() - ref64).abs().max())
    ulp = float(np.spacing(np.float32(ref64.abs().max())))
    return err, margin * err32 + ulp, err32
