"""Host plumbing shared by the five solvers of this package: everything around a batch that is the same whichever loop restores it.

The loops themselves (solve_ip, restore_batch) stay in the solvers' own files, next to the reference lines they mirror; what they repeated
is here once: the iteration-callback trampoline of the engine loops, the measurement-noise draw, the shard prologue, the one-GPU
refusal, the time / memory bookkeeping, the metric files and the shape checks.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from time import perf_counter

import numpy as np
import torch

from .. import _lib
from .. import parallel
from .. import utils


class Solver(object):
    """What the five solver classes have in common: the constructor's fields, the lazily loaded library, the reference's model_forward
    and grad_datafit, and the result files."""
    unscaled_couplings = ("ot",)        # args.model values whose net takes t as it is ('rectified' takes t * 999)

    def __init__(self, model, device, args):
        self.device = device
        self.args = args
        self.model = model
        self.method = args.method
        self._lib = None
        self.measurement_noise = None       # optional measurement_noise(batch, noisy) replacing the seeded draw (unit scale; multi-GPU shards, parity runs)
        # where the torch.manual_seed(batch) measurement noise is drawn: "cpu" (default: the same values on any device and on every
        # rank) or "device" - the reference's own behaviour (torch.randn_like of a device tensor), drawn for the GLOBAL batch on this
        # rank's device generator and sliced, so that shards still reproduce the single-device run
        self.measurement_noise_source = getattr(args, "measurement_noise", "cpu")
        self.last_restored = None           # the final x of the last batch (the reference only writes it to disk)
        self.last_callback_seconds = 0.0

    @property
    def lib(self):
        if self._lib is None:
            self._lib = _lib.load()
        return self._lib

    @lib.setter
    def lib(self, value):
        self._lib = value

    # ---- the reference's small methods -----------------------------------------------------------------------------------------
    def _coupling_error(self):
        names = "/".join(repr(c) for c in self.unscaled_couplings)
        return NotImplementedError(f"only the {names} U-Net and the 'rectified' NCSN++ net are implemented")

    def model_forward(self, x, t):
        if self.args.model in self.unscaled_couplings:
            return self.model(x, t)
        if self.args.model == "rectified":        # model_fn(x, t * 999)
            return self.model(x.type(torch.float), t * 999)
        raise self._coupling_error()

    def _set_time_scale(self):
        """The engine's loops evaluate model(x, t * 999) for the rectified coupling (model_forward above)."""
        if hasattr(self.model, "set_solver_time_scale"):
            self.model.set_solver_time_scale(999.0 if self.args.model == "rectified" else 1.0)

    def grad_datafit(self, x, y, H, H_adj):
        if self.args.noise_type == 'gaussian':
            return H_adj(H(x) - y) / (self.args.sigma_noise ** 2)
        elif self.args.noise_type == 'laplace':
            r = H(x) - y
            return H_adj(2 * torch.heaviside(r, torch.zeros_like(r)) - 1) / self.args.sigma_noise
        raise ValueError('Noise type not supported')

    # ---- result files ----------------------------------------------------------------------------------------------------------
    def write_metrics(self, clean, noisy, x, H_adj, iteration):
        """One line per metric file of the batch; none of the three writes to its inputs, so x goes in as it is."""
        if self.args.save_results:
            x = x.detach()
            utils.compute_psnr(clean, noisy, x, self.args, H_adj, iter=iteration)
            utils.compute_ssim(clean, noisy, x, self.args, H_adj, iter=iteration)
            utils.compute_lpips(clean, noisy, x, self.args, H_adj, iter=iteration)

    def write_final(self, clean, noisy, x, H_adj, last):
        """The images of the batch and its final metric lines, which carry the last loop index as `iter`."""
        if self.args.save_results:
            utils.save_images(clean, noisy, x.detach(), self.args, H_adj, iter='final')
            self.write_metrics(clean, noisy, x, H_adj, last)

    def write_averages(self):
        if self.args.save_results:
            utils.compute_average_psnr(self.args)
            utils.compute_average_ssim(self.args)
            utils.compute_average_lpips(self.args)
        if self.args.compute_memory:
            utils.compute_average_memory(self.args)
        if self.args.compute_time:
            utils.compute_average_time(self.args)

    def run_method(self, data_loaders, degradation, sigma_noise, H_funcs=None):
        folder = utils.get_save_path_ip(self.args.dict_cfg_method)
        self.args.save_path_ip = os.path.join(self.args.save_path, folder)
        os.makedirs(self.args.save_path_ip, exist_ok=True)
        self.solve_ip(data_loaders[self.args.eval_split], degradation, sigma_noise)


class IterCallback:
    """Trampoline between an engine loop and iter_cb(iteration, x): `cb` is what the engine call takes (NULL when iter_cb is None).
    An exception of iter_cb must not unwind through the C frames: the first one is kept, later calls are dropped, and `reraise` raises
    it after the engine call.  `seconds` is the host time spent inside iter_cb.  The object owns the ctypes callback and the mask the
    engine reads, so it has to live until the engine call returns."""

    def __init__(self, iter_cb, n_iterations, cb_iterations=None):
        self.error, self.seconds, self.x, self.mask = None, 0.0, None, None
        if iter_cb is None:
            self.cb = C.cast(None, _lib.ITER_CB)
            return

        def _cb(it, user):
            t_cb = perf_counter()
            try:
                if self.error is None:
                    iter_cb(it, self.x)
            except BaseException as exc:
                self.error = exc
            self.seconds += perf_counter() - t_cb
        self.cb = _lib.ITER_CB(_cb)
        if cb_iterations is not None:       # None: every iteration
            self.mask = np.zeros(n_iterations, dtype=np.uint8)
            self.mask[[i for i in cb_iterations if 0 <= i < n_iterations]] = 1

    def attach(self, prm):
        if self.mask is not None:
            prm.host_cb_mask = self.mask.ctypes.data

    def bind(self, x):
        self.x = x

    def reraise(self):
        if self.error is not None:
            raise self.error


def measurement_noise(solver, batch, noisy_img, gshape, lo, hi, noise_type='gaussian'):
    """Unit-scale measurement noise of images [lo, hi) of the batch of global shape `gshape`.  The override hook wins; 'gaussian' is
    the reference's torch.manual_seed(batch); randn_like(noisy_img) (utils.draw_measurement_noise); 'laplace' is the reference's
    Laplace sample, which it does NOT re-seed, on the CPU generator.  Both draw the global batch and slice it."""
    if solver.measurement_noise is not None:
        return solver.measurement_noise(batch, noisy_img)
    if noise_type == 'laplace':
        return torch.distributions.laplace.Laplace(torch.zeros(gshape), torch.ones(gshape)).sample()[lo:hi].to(solver.device)
    if noise_type != 'gaussian':
        raise ValueError('Noise type not supported')
    return utils.draw_measurement_noise(batch, gshape, lo, hi, solver.device, solver.measurement_noise_source)


def shard_of_batch(clean_img, degradation):
    """(this rank's images, global batch size G, lo, hi).  Multi-GPU (torchrun, one process per GPU): every rank walks the same loader
    and restores its contiguous slice [lo, hi) of each batch; the batch-shaped random draws are taken for the whole batch and sliced,
    metrics are all_gathered per image and written by rank 0 - so the result files equal a single-device run's (parallel.py)."""
    rank, world = parallel.rank_world()
    G = clean_img.shape[0]
    lo, hi = parallel.shard_range(G, rank, world)
    if world > 1:
        clean_img = clean_img[lo:hi]
        if hasattr(degradation, "set_shard"):
            degradation.set_shard(G, lo)
    return clean_img, G, lo, hi


def env_world():
    """World size of the job, also before main.py has joined its process group (torchrun sets WORLD_SIZE)."""
    return max(parallel.rank_world()[1], int(os.environ.get("WORLD_SIZE", "1")))


def single_gpu_only(world, message):
    """Refusal of the solvers whose batch cannot be split: `message` is '<method> runs on one GPU only: <why>'."""
    if world > 1:
        raise RuntimeError(f"{message}, so a batch split over {world} ranks would change the result. Run it without torchrun.")


def write_batch_stats(solver, batch, seconds):
    """memory_stats.txt, then time_stats.txt (`seconds`: the batch's time, measured by the caller)."""
    if solver.args.compute_memory:
        # torch's caching allocator (measurement, noise, output tensors) + the engine's own device memory
        utils.save_memory_use({"batch": batch, "max_allocated": torch.cuda.max_memory_allocated(solver.device) + solver.model.memory_bytes()},
                              solver.args)
    if solver.args.compute_time:
        utils.save_time_use({"batch": batch, "time_per_batch": seconds}, solver.args)


def begin_batch_stats(solver):
    """Start of a batch's timed part: an idle device, a fresh peak-memory counter.  Returns the start time."""
    if solver.args.compute_time:
        torch.cuda.synchronize()
    t0 = perf_counter()
    if solver.args.compute_memory:
        torch.cuda.reset_peak_memory_stats(solver.device)
    return t0


@contextlib.contextmanager
def batch_stats(solver, batch):
    """Times the body and records its peak memory.  As the reference accumulates the iteration bodies only, the time the body spent
    in metric callbacks (solver.last_callback_seconds) is excluded."""
    t0 = begin_batch_stats(solver)
    solver.last_callback_seconds = 0.0
    yield
    if solver.args.compute_time:
        torch.cuda.synchronize()
    write_batch_stats(solver, batch, perf_counter() - t0 - solver.last_callback_seconds)


def check_image(x, what, model, who):
    """x as the contiguous fp32 tensor the engine reads; it must be a device tensor of the net's image shape."""
    Hh = model.input_height
    if x.ndim != 4 or tuple(x.shape[1:]) != (model.input_channels, Hh, Hh):
        raise ValueError(f"{what} of shape {tuple(x.shape)} does not match the net's (B, {model.input_channels}, {Hh}, {Hh})")
    if not x.is_cuda:
        raise _lib.PnpFlowHipError(f"{who} needs GPU tensors (there is no CPU path)")
    return x.detach().contiguous().float()


def check_measurement(y, degradation, B, model):
    side = degradation.out_side(model.input_height)
    if tuple(y.shape) != (B, model.input_channels, side, side):
        raise ValueError(f"measurement of shape {tuple(y.shape)} does not match the operator's output ({B}, {model.input_channels}, {side}, {side})")
    return y.detach().contiguous().float()
