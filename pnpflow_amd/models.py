"""`UNet` with the constructor / call / state_dict surface of pnpflow.models.UNet
(reference pnpflow/models.py:302-495), executed by the HIP engine.

    model = UNet(3, 128, 32, ch_mult=(1,2,4,8), num_res_blocks=6, attn_resolutions=(16,8))
    model.load_state_dict(torch.load(".../model_final.pt"))     # the reference's checkpoint format
    v = model(x, t)            # x: (B,C,H,W) fp32 on the GPU, t: (B,) -> (B,C,H,W)
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np
import torch

from . import _lib


class _EngineNet:
    """What UNet and NCSNpp share: the torch.nn.Module-like surface the reference's callers use, on a pf_engine handle."""

    # ---- torch.nn.Module-like surface used by the reference's callers -------------------
    def to(self, device=None):
        return self

    def eval(self):
        return self

    def parameters(self):
        return iter(())

    def state_dict_keys(self):
        n = self._lib.pf_engine_num_weights(self._h)
        return [self._lib.pf_engine_weight_name(self._h, i).decode() for i in range(n)]

    def state_dict_shapes(self):
        out = {}
        for i, k in enumerate(self.state_dict_keys()):
            shp = (C.c_int64 * 4)()
            nd = self._lib.pf_engine_weight_shape(self._h, i, shp)
            out[k] = tuple(int(shp[j]) for j in range(nd))
        return out

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        keys = self.state_dict_keys()
        missing = [k for k in keys if k not in state_dict]
        unexpected = [k for k in state_dict if k not in set(keys)]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:5]} unexpected {unexpected[:5]}")
        for k in keys:
            if k not in state_dict:
                continue
            a = np.ascontiguousarray(state_dict[k].detach().cpu().to(torch.float32).numpy())
            shp = (C.c_int64 * a.ndim)(*a.shape)
            _lib.check(self._lib.pf_engine_load_weight(self._h, k.encode(), a.ctypes.data_as(C.c_void_p), shp, a.ndim),
                       self._h, f"pf_engine_load_weight({k})")
        _lib.check(self._lib.pf_engine_finalize_weights(self._h), self._h, "pf_engine_finalize_weights")
        self._loaded = True
        return self

    @property
    def handle(self):
        return self._h

    def __call__(self, x: torch.Tensor, temp: torch.Tensor) -> torch.Tensor:
        return self.forward(x, temp)

    def forward(self, x: torch.Tensor, temp: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise _lib.PnpFlowHipError(f"{type(self).__name__}.forward needs tensors on the GPU (there is no CPU path)")
        x = x.contiguous().float()
        t = temp.contiguous().float().to(x.device)
        B, Cc, H, W = x.shape
        assert Cc == self.input_channels and H == self.input_height and W == H and t.shape == (B,)
        v = torch.empty((B, self.output_channels, H, W), dtype=torch.float32, device=x.device)
        _lib.check(self._lib.pf_unet_forward(self._h, x.data_ptr(), t.data_ptr(), v.data_ptr(), B, _lib.current_stream_ptr()),
                   self._h, "pf_unet_forward")
        return v

    def forward_retain(self, x: torch.Tensor, temp: torch.Tensor) -> torch.Tensor:
        """Forward that keeps every activation on the device, for a following `backward`."""
        x = x.contiguous().float(); t = temp.contiguous().float().to(x.device)
        B = x.shape[0]
        v = torch.empty((B, self.output_channels, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
        _lib.check(self._lib.pf_unet_forward_retain(self._h, x.data_ptr(), t.data_ptr(), v.data_ptr(), B, _lib.current_stream_ptr()),
                   self._h, "pf_unet_forward_retain")
        return v

    def backward(self, vec: torch.Tensor) -> torch.Tensor:
        """J^T vec (input gradient) at the last `forward_retain`."""
        vec = vec.contiguous().float()
        g = torch.empty((vec.shape[0], self.input_channels, vec.shape[2], vec.shape[3]), dtype=torch.float32, device=vec.device)
        _lib.check(self._lib.pf_unet_backward(self._h, vec.data_ptr(), g.data_ptr(), vec.shape[0], _lib.current_stream_ptr()),
                   self._h, "pf_unet_backward")
        return g

    def vjp(self, x: torch.Tensor, temp: torch.Tensor, vec: torch.Tensor):
        """(v_theta(x,t), J^T vec) - what torch.autograd.functional.vjp(lambda z: model(z,t), x, vec) returns
        (reference pnpflow/methods/ot_ode.py:137-138)."""
        v = self.forward_retain(x, temp)
        return v, self.backward(vec)

    # ---- the prior itself: divergence estimate, fixed-grid sampling, log-likelihood solve --------
    def _check_images(self, x: torch.Tensor, what: str):
        Hh = self.input_height
        if x.ndim != 4 or tuple(x.shape[1:]) != (self.input_channels, Hh, Hh):
            raise ValueError(f"{what} of shape {tuple(x.shape)} does not match the net's (B, {self.input_channels}, {Hh}, {Hh})")
        if not x.is_cuda:
            raise _lib.PnpFlowHipError(f"{type(self).__name__} needs GPU tensors (there is no CPU path)")
        return x.detach().contiguous().float()

    def divergence(self, x: torch.Tensor, temp: torch.Tensor, eps: torch.Tensor, return_velocity: bool = False):
        """Value of the Hutchinson estimator eps . (J_v(x, t) eps) per image, (B,) fp64 (pf_flow_divergence: one retained forward, one
        backward with vec = eps, a deterministic dot product).  The net sees t * the solver time scale.  No autograd graph."""
        x = self._check_images(x, "input"); eps = self._check_images(eps, "eps")
        B = x.shape[0]
        if eps.shape != x.shape:
            raise ValueError(f"eps of shape {tuple(eps.shape)} for an input of shape {tuple(x.shape)}")
        t = torch.as_tensor(temp, dtype=torch.float32, device=x.device).reshape(-1)
        t = (t.expand(B) if t.numel() == 1 else t).contiguous()
        if t.numel() != B:
            raise ValueError(f"t has {t.numel()} entries for a batch of {B}")
        div = torch.empty(B, dtype=torch.float64, device=x.device)
        v = torch.empty_like(x) if return_velocity else None
        _lib.check(self._lib.pf_flow_divergence(self._h, x.data_ptr(), t.data_ptr(), eps.data_ptr(), v.data_ptr() if return_velocity else None,
                                                div.data_ptr(), B, _lib.current_stream_ptr()), self._h, "pf_flow_divergence")
        return (div, v) if return_velocity else div

    def euler(self, x: torch.Tensor, time_points) -> torch.Tensor:
        """torchdiffeq's fixed-grid euler over `time_points` (fp32): x += (t[i+1] - t[i]) * v(x, t[i]) (pf_flow_ode_euler)."""
        x = self._check_images(x, "input")
        grid = np.ascontiguousarray(torch.as_tensor(time_points).detach().cpu().to(torch.float32).numpy().reshape(-1))
        if grid.size < 2:
            raise ValueError("the time grid needs at least 2 points")
        out = torch.empty_like(x)
        _lib.check(self._lib.pf_flow_ode_euler(self._h, grid.ctypes.data_as(C.POINTER(C.c_float)), int(grid.size), x.data_ptr(), out.data_ptr(),
                                               x.shape[0], _lib.current_stream_ptr()), self._h, "pf_flow_ode_euler")
        return out

    def likelihood_ode(self, x: torch.Tensor, eps: torch.Tensor, t0: float = 1.0, t1: float = 1e-5, rtol: float = 1e-5, atol: float = 1e-5,
                       offset: float = 7.0, max_attempts: int = 1000):
        """The augmented solve (x, logp) of get_likelihood_fn_rf under SciPy's RK45 rules (pf_flow_likelihood_rk45) ->
        (z (B,C,H,W), delta_logp (B,) fp64, bpd (B,) fp32, dict(accepted, rejected, nfev))."""
        x = self._check_images(x, "input"); eps = self._check_images(eps, "eps")
        if eps.shape != x.shape:
            raise ValueError(f"eps of shape {tuple(eps.shape)} for an input of shape {tuple(x.shape)}")
        B = x.shape[0]
        prm = _lib.PfLikelihoodParams()
        prm.t0, prm.t1, prm.rtol, prm.atol, prm.offset, prm.max_attempts = float(t0), float(t1), float(rtol), float(atol), float(offset), int(max_attempts)
        z = torch.empty_like(x)
        dlp = torch.empty(B, dtype=torch.float64, device=x.device)
        bpd = torch.empty(B, dtype=torch.float32, device=x.device)
        stats = (C.c_int64 * 3)()
        _lib.check(self._lib.pf_flow_likelihood_rk45(self._h, C.byref(prm), x.data_ptr(), eps.data_ptr(), z.data_ptr(), dlp.data_ptr(), bpd.data_ptr(),
                                                     stats, B, _lib.current_stream_ptr()), self._h, "pf_flow_likelihood_rk45")
        return z, dlp, bpd, dict(accepted=int(stats[0]), rejected=int(stats[1]), nfev=int(stats[2]))

    # ---- sampling the rectified-flow prior -----------------------------------------------------
    def rf_euler(self, x: torch.Tensor, n_steps: int, t_begin: float = 1e-3, t_end: float = 1.0, sigma_var: float = 0.0, noise_scale: float = 1.0,
                 noise: torch.Tensor = None, seed: int = 0, stream_id: int = 0) -> torch.Tensor:
        """euler_sampler of image_generation/sampling.py:69-109 from the latent `x` (pf_rf_euler_sampler): n_steps evaluations at
        num_t = i/N (t_end - t_begin) + t_begin with the reference's step dt = 1/N (not the grid spacing), the Euler-Maruyama form when
        sigma_var > 0.  `noise`: optional (n_steps, B, C, H, W) draws; otherwise the engine's Philox normals (seed, stream_id) are drawn
        inside the update kernel.  The net sees num_t * the solver time scale.  Nothing synchronises."""
        x = self._check_images(x, "input")
        n_steps = int(n_steps)
        if noise is not None:
            if tuple(noise.shape) != (n_steps,) + tuple(x.shape):
                raise ValueError(f"noise of shape {tuple(noise.shape)} does not match (n_steps, B, C, H, W) = {(n_steps,) + tuple(x.shape)}")
            if not noise.is_cuda:
                raise _lib.PnpFlowHipError(f"{type(self).__name__} needs GPU tensors (there is no CPU path)")
            noise = noise.detach().contiguous().float()
        prm = _lib.PfRfSamplerParams()
        prm.t_begin, prm.t_end, prm.n_steps, prm.sigma_var, prm.noise_scale = float(t_begin), float(t_end), n_steps, float(sigma_var), float(noise_scale)
        prm.seed, prm.stream_id = int(seed), int(stream_id)
        out = torch.empty_like(x)
        _lib.check(self._lib.pf_rf_euler_sampler(self._h, C.byref(prm), x.data_ptr(), noise.data_ptr() if noise is not None else None, out.data_ptr(),
                                                 x.shape[0], _lib.current_stream_ptr()), self._h, "pf_rf_euler_sampler")
        return out

    def ode_rk45(self, x: torch.Tensor, t0: float, t1: float, rtol: float, atol: float, max_attempts: int = 1000):
        """dx/dt = v(x, t) from t0 to t1 under SciPy's RK45 rules (pf_flow_ode_rk45) -> (x at t1, dict(accepted, rejected, nfev)).
        The error norm is the RMS over the WHOLE batch, as scipy.integrate.solve_ivp sees the flattened batch: the images of a batch share
        one step sequence, so a sample depends on its batch companions at the level of the tolerance."""
        x = self._check_images(x, "input")
        prm = _lib.PfRk45Params()
        prm.t0, prm.t1, prm.rtol, prm.atol, prm.max_attempts = float(t0), float(t1), float(rtol), float(atol), int(max_attempts)
        out = torch.empty_like(x)
        stats = (C.c_int64 * 3)()
        _lib.check(self._lib.pf_flow_ode_rk45(self._h, C.byref(prm), x.data_ptr(), out.data_ptr(), stats, x.shape[0], _lib.current_stream_ptr()),
                   self._h, "pf_flow_ode_rk45")
        return out, dict(accepted=int(stats[0]), rejected=int(stats[1]), nfev=int(stats[2]))

    # ---- debugging: named internal activations of the last forward (NCHW numpy) -----------
    def read_taps(self, B):
        """Internal activations of the last forward as {name: (B,C,H,W) numpy}.  Only
        meaningful when PNPFLOW_HIP_KEEP_ACTIVATIONS=1 was set before the first forward
        (otherwise activation buffers are recycled)."""
        out = {}
        big = np.empty(B * self.ch * max(self.ch_mult) * self.input_height * self.input_height, dtype=np.float32)
        for i in range(self._lib.pf_engine_num_taps(self._h)):
            name = self._lib.pf_engine_tap_name(self._h, i).decode()
            dims = (C.c_int32 * 3)()
            _lib.check(self._lib.pf_engine_read_tap(self._h, i, big.ctypes.data_as(C.c_void_p), big.size, dims, _lib.current_stream_ptr()),
                       self._h, "pf_engine_read_tap")
            c, h, w = dims[0], dims[1], dims[2]
            out[name] = big[: B * c * h * w].reshape(B, c, h, w).copy()
        return out

    def set_precision(self, mode: int):
        """1 (default): split-fp16 MFMA (fp32-equivalent, 3 x f16 MFMA per product); 0: exact fp32 MFMA; 2: single fp16 MFMA per
        product (fp16 operands, fp32 accumulate: TF32-class, ~1e-3 relative on the U-Net output)."""
        _lib.check(self._lib.pf_engine_set_precision(self._h, int(mode)), self._h, "pf_engine_set_precision")
        return self

    def check_numerics(self):
        """Synchronises the current stream and raises if any forward since the last check saw a non-finite activation."""
        _lib.check(self._lib.pf_engine_check_numerics(self._h, _lib.current_stream_ptr()), self._h, "pf_engine_check_numerics")

    def memory_bytes(self) -> int:
        """Device bytes the engine currently holds (weights, activation plans, solver buffers)."""
        return int(self._lib.pf_engine_memory_bytes(self._h))

    def profile(self, enable: bool):
        _lib.check(self._lib.pf_engine_profile(self._h, 1 if enable else 0), self._h, "pf_engine_profile")

    def profile_read(self):
        n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
        _lib.check(self._lib.pf_engine_profile_read(self._h, C.byref(n), C.byref(ms), C.byref(fl)), self._h, "pf_engine_profile_read")
        return n.value, ms.value, fl.value

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.pf_engine_destroy(self._h)
                self._h = None
        except Exception:
            pass


class UNet(_EngineNet):
    def __init__(self, input_channels, input_height, ch, output_channels=None, ch_mult=(1, 2, 4, 8),
                 num_res_blocks=2, attn_resolutions=(16,), dropout=0., resamp_with_conv=True, act=None,
                 normalize=None, device_index: int = 0):
        if dropout != 0. or not resamp_with_conv:
            raise NotImplementedError("engine implements the configuration define_model uses: dropout=0, resamp_with_conv=True")
        self.input_channels = input_channels
        self.input_height = input_height
        self.ch = ch
        self.output_channels = input_channels if output_channels is None else output_channels
        self.ch_mult = tuple(ch_mult)
        self.num_res_blocks = num_res_blocks
        self.attn_resolutions = tuple(attn_resolutions)
        self.num_resolutions = len(self.ch_mult)
        self._lib = _lib.load()
        cfg = _lib.PfUnetCfg()
        cfg.input_channels, cfg.output_channels, cfg.input_height, cfg.ch = input_channels, self.output_channels, input_height, ch
        cfg.num_levels, cfg.num_res_blocks = len(self.ch_mult), num_res_blocks
        for i, m in enumerate(self.ch_mult):
            cfg.ch_mult[i] = m
        cfg.num_attn_resolutions = len(self.attn_resolutions)
        for i, r in enumerate(self.attn_resolutions):
            cfg.attn_resolutions[i] = r
        self._device_index = device_index
        h = C.c_void_p()
        _lib.check(self._lib.pf_engine_create(device_index, C.byref(cfg), C.byref(h)), None, "pf_engine_create")
        self._h = h
        self._loaded = False
        self.training = False


FID_WEIGHTS_FILE = "pt_inception-2015-12-05-6726825d.pth"      # pytorch-fid's port of the TensorFlow FID Inception weights (reference models.py:501)


def find_fid_weights(output_root=None):
    """Path of the FID Inception weight file, or None: $PNPFLOW_FID_WEIGHTS (the file, or a folder holding it), <output_root>model/, then
    torch.hub's checkpoint folder, where the reference's load_state_dict_from_url leaves it (models.py:694)."""
    import os
    cands = []
    env = os.environ.get("PNPFLOW_FID_WEIGHTS")
    if env:
        cands += [env, os.path.join(env, FID_WEIGHTS_FILE)]
    if output_root is not None:
        cands.append(os.path.join(str(output_root) + "model", FID_WEIGHTS_FILE))
    cands.append(os.path.join(os.path.expanduser("~/.cache/torch/hub/checkpoints"), FID_WEIGHTS_FILE))
    return next((p for p in cands if os.path.isfile(p)), None)


class InceptionV3:
    """The FID feature network with the surface of the reference's InceptionV3 (pnpflow/models.py:504-651, use_fid_inception=True, eval mode)
    on csrc/inception.hip.

        net = InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[2048]]); net.load_state_dict(torch.load(find_fid_weights()))
        pred = net(batch)[0]          # batch: (B, 3, H, W) on the GPU, values in (0, 1)

    `forward` returns one tensor per requested block, ascending, like the reference's - but every block arrives spatially averaged,
    (B, dims, 1, 1): what fid_score.get_activations takes of it next (fid_score.py:60-65) and what block 3 is anyway.  One engine pass
    per requested block.  The constructor loads no weights (the reference downloads them there): load_state_dict takes pytorch-fid's
    key names `<layer>.conv.weight`, `<layer>.bn.{weight,bias,running_mean,running_var}`, ignores `fc.*`, `AuxLogits.*` and
    `num_batches_tracked`, and raises KeyError naming what is missing.  PARITY UNPINNED: torchvision is absent from the build image.
    """
    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input=True, normalize_input=True, requires_grad=False, use_fid_inception=True,
                 device_index: int = 0):
        if requires_grad or not use_fid_inception:
            raise NotImplementedError("the engine runs the FID Inception network in inference (use_fid_inception=True, requires_grad=False)")
        self.output_blocks = sorted(int(b) for b in output_blocks)
        if not self.output_blocks or self.output_blocks[0] < 0 or self.output_blocks[-1] > 3:
            raise ValueError("output blocks are 0..3 (the last possible output block index is 3)")
        self.last_needed_block = self.output_blocks[-1]
        self.resize_input, self.normalize_input = bool(resize_input), bool(normalize_input)
        self._lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self._lib.pf_inception_create(device_index, C.byref(h)), None, "pf_inception_create")
        self._h = h
        self._loaded = False
        self.training = False

    @staticmethod
    def layer_table():
        """[(name, Cin, Cout, KH, KW, stride, pad_h, pad_w)] of the 94 convs, as the engine's planner holds them (csrc/inception_plan.h)."""
        lib = _lib.load()
        out = []
        for i in range(lib.pf_inception_num_layers()):
            name, dims = C.create_string_buffer(96), (C.c_int32 * 7)()
            _lib.check(lib.pf_inception_layer(i, name, 96, dims), None, "pf_inception_layer")
            out.append((name.value.decode(),) + tuple(int(d) for d in dims))
        return out

    @classmethod
    def state_dict_shapes(cls):
        """{published key: shape} of everything load_state_dict needs."""
        out = {}
        for (n, ci, co, kh, kw, _s, _ph, _pw) in cls.layer_table():
            out[n + ".conv.weight"] = (co, ci, kh, kw)
            for s in ("weight", "bias", "running_mean", "running_var"):
                out[f"{n}.bn.{s}"] = (co,)
        return out

    def _err(self):
        return (self._lib.pf_inception_last_error(self._h) or b"").decode()

    @classmethod
    def select_weights(cls, state_dict, strict: bool = True):
        """{published key: tensor} of exactly what the network needs, out of a pytorch-fid state_dict: `fc.*`, `AuxLogits.*` and
        `*.num_batches_tracked` are ignored, a missing key is a KeyError that names it, any other extra key is one too when strict."""
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        need = cls.state_dict_shapes()
        missing = [k for k in need if k not in sd]
        if missing:
            raise KeyError(f"FID Inception weights missing: {missing[:8]}{' ...' if len(missing) > 8 else ''} ({len(missing)} of {len(need)} keys)")
        unexpected = [k for k in sd if k not in need and not k.startswith(("fc.", "AuxLogits.")) and not k.endswith("num_batches_tracked")]
        if strict and unexpected:
            raise KeyError(f"unexpected keys for the FID Inception network: {unexpected[:8]}")
        for k, shape in need.items():
            if tuple(sd[k].shape) != tuple(shape):
                raise ValueError(f"FID Inception weight {k} has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
        return {k: sd[k] for k in need}

    def load_state_dict(self, state_dict, strict: bool = True):
        sd = need = self.select_weights(state_dict, strict)
        for k in need:
            a = np.ascontiguousarray(sd[k].detach().cpu().to(torch.float32).numpy())
            shp = (C.c_int64 * a.ndim)(*a.shape)
            rc = self._lib.pf_inception_load_weight(self._h, k.encode(), a.ctypes.data_as(C.c_void_p), shp, a.ndim)
            if rc != 0:
                raise _lib.PnpFlowHipError(f"pf_inception_load_weight({k}) failed (status {rc}): {self._err()}")
        self._loaded = True
        return self

    def to(self, device=None):
        return self

    def eval(self):
        return self

    def parameters(self):
        return iter(())

    def profile(self, enable: bool):
        _lib.check(self._lib.pf_inception_profile(self._h, 1 if enable else 0), None, "pf_inception_profile")

    def profile_read(self):
        """[(launch name, milliseconds, floating-point operations)] of the last profiled forward."""
        out, i = [], 0
        name, ms, fl = C.create_string_buffer(96), C.c_float(), C.c_double()
        while self._lib.pf_inception_profile_read(self._h, i, name, 96, C.byref(ms), C.byref(fl)) == 0:
            out.append((name.value.decode(), float(ms.value), float(fl.value))); i += 1
        return out

    def features(self, inp: torch.Tensor, block: int) -> torch.Tensor:
        """(B, dims) spatially averaged output of one block."""
        if not inp.is_cuda:
            raise _lib.PnpFlowHipError("InceptionV3 needs GPU tensors (there is no CPU path)")
        if inp.ndim != 4 or inp.shape[1] != 3:
            raise ValueError(f"InceptionV3 expects (B, 3, H, W) images, got {tuple(inp.shape)}")
        x = inp.detach().contiguous().float()
        B, _c, H, W = x.shape
        dims = {v: k for k, v in self.BLOCK_INDEX_BY_DIM.items()}[int(block)]
        out = torch.empty((B, dims), dtype=torch.float32, device=x.device)
        if B == 0:
            return out
        rc = self._lib.pf_inception_forward(self._h, x.data_ptr(), out.data_ptr(), B, H, W, int(self.resize_input), int(self.normalize_input), int(block),
                                            _lib.current_stream_ptr())
        if rc != 0:
            raise _lib.PnpFlowHipError(f"pf_inception_forward failed (status {rc}): {self._err()}")
        return out

    def forward(self, inp: torch.Tensor):
        return [self.features(inp, b)[:, :, None, None] for b in self.output_blocks]

    __call__ = forward

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.pf_inception_destroy(self._h)
                self._h = None
        except Exception:
            pass


def load_fid_inception(output_blocks=(3,), output_root=None, synthetic=False, device_index=0, resize_input=True, normalize_input=True):
    """(InceptionV3 with weights, real) - the published weights when find_fid_weights has them; otherwise FileNotFoundError, unless
    `synthetic` opts into seed-fixed synthetic weights (tools/synthetic_inception.py; the FID is then not comparable with anything)."""
    net = InceptionV3(output_blocks, resize_input=resize_input, normalize_input=normalize_input, device_index=device_index)
    path = find_fid_weights(output_root)
    if path is not None:
        return net.load_state_dict(torch.load(path, map_location="cpu")), True
    if not synthetic:
        raise FileNotFoundError(f"{FID_WEIGHTS_FILE} not found in $PNPFLOW_FID_WEIGHTS, <output_root>model/ or ~/.cache/torch/hub/checkpoints/ (pytorch-fid's "
                                "release 'fid_weights'). Pass `--opts synthetic True` to run on seed-fixed synthetic weights instead.")
    print(f"[pnpflow_amd] synthetic=True: {FID_WEIGHTS_FILE} not found, using SYNTHETIC Inception weights (the FID is not meaningful)")
    from tools.synthetic_inception import synthetic_inception_state_dict
    return net.load_state_dict(synthetic_inception_state_dict(InceptionV3.state_dict_shapes())), False
