"""The five run_method cases shared by tests/test_gpu_solver_files.py and tools/record_solver_files.py: the tiny4 net at 64^2, two batches
of two images, save_results / compute_time / compute_memory on, the smallest settings that still cross every logging rule of the
solver.  Only the public API of the package is used, so the recording tool runs unchanged on any commit that has the five solvers."""
import contextlib
import os

import torch

from conftest import CFGS, det_image
from oracle import pnpflow_oracle as O

SIGMA = 0.05
STAT_FILES = ("time_stats.txt", "memory_stats.txt", "time_average.txt", "max_memory_average.txt")

# name -> (module, class, problem, method hyper-parameters (they also name the result folder), further args)
CASES = {
    "pnp_flow": ("pnp_flow", "PNP_FLOW", "superresolution",
                 dict(steps_pnp=20, lr_pnp=1.0, gamma_style="alpha_1_minus_t", num_samples=1, alpha=0.3), dict(model="ot")),
    "ot_ode": ("ot_ode", "OT_ODE", "random_inpainting", dict(steps_ode=20, start_time=0.3, gamma="constant"), dict(model="ot")),
    "pnp_gs": ("pnp_gs", "PROX_PNP", "inpainting", dict(algo="pgd", max_iter=12, lr_pnp=1.0, alpha=0.5, sigma_factor=1.0),
               dict(model="gradient_step", dim_image=64, num_channels=3)),
    "d_flow": ("d_flow", "D_FLOW", "denoising", dict(steps_euler=3, LBFGS_iter=2, max_iter=1, lmbda=0.001, alpha=0.1, start_time=0.0),
               dict(model="ot")),
    "flow_priors": ("flow_priors", "FLOW_PRIORS", "inpainting", dict(N=3, K=1, lmbda=1000.0, eta=0.01, start_time=0.0), dict(model="ot")),
}


def logging_iterations(name):
    """The iteration column of every per-batch metric file: the solver's logging rule, then the final line with the last loop index."""
    cfg = CASES[name][3]
    if name == "pnp_flow":
        n = cfg["steps_pnp"]
        return [it for it in range(n) if it % 50 == 0 or it % (n // 10) == 0] + [n - 1]
    if name == "ot_ode":
        n = cfg["steps_ode"]
        return [it for it in range(int(n * cfg["start_time"]), n) if it % 10 == 0 or it % (n // 10) == 0] + [n - 1]
    if name == "pnp_gs":
        n = cfg["max_iter"]
        return [it for it in range(n) if it % 10 == 0] + [n - 1]
    return [(cfg["max_iter"] if name == "d_flow" else cfg["N"]) - 1]


def degradation(problem):
    import pnpflow_amd.degradations as D
    return {"superresolution": lambda: D.Superresolution(2, 64), "random_inpainting": lambda: D.RandomInpainting(0.7),
            "inpainting": lambda: D.BoxInpainting(10), "denoising": lambda: D.Denoising()}[problem]()


def new_model():
    from pnpflow_amd.models import UNet
    c = CFGS["tiny4"]
    m = UNet(c["input_channels"], c["input_height"], c["ch"], ch_mult=c["ch_mult"], num_res_blocks=c["num_res_blocks"],
             attn_resolutions=c["attn_resolutions"])
    m.load_state_dict(O.synthetic_state_dict(O.unet_config(**c), 0))
    return m


@contextlib.contextmanager
def synthetic_lpips():
    """LPIPS with synthetic weights under the published key names, so that the lpips_* files are written where the real weights are absent."""
    from pnpflow_amd import utils as U
    from pnpflow_amd.lpips import LPIPS
    U.set_lpips_model(LPIPS("alex").load_state_dict(O.synthetic_lpips_state_dict(1)))
    try:
        yield
    finally:
        U.set_lpips_model(None); U._LPIPS["resolved"] = False


def run_case(name, net, save_path):
    """run_method of case `name` on the UNet `net` into `save_path`; returns (args, the model the solver holds)."""
    import importlib
    from pnpflow_amd.utils import CfgNode
    module, cls, problem, cfg, extra = CASES[name]
    args = CfgNode(dict(method=name, dataset="celeba", problem=problem, noise_type="gaussian", max_batch=2, compute_time=True, compute_memory=True,
                        save_results=True, eval_split="test", save_path=str(save_path), dict_cfg_method=dict(cfg), **cfg, **extra))
    dev = torch.device("cuda")
    model = net
    if name == "pnp_gs":
        from pnpflow_amd.train_denoiser import GRADIENT_STEP_DENOISER
        model = GRADIENT_STEP_DENOISER(net, dev, args)
    solver = getattr(importlib.import_module("pnpflow_amd.methods." + module), cls)(model, dev, args)
    clean = det_image((2, 3, 64, 64), 31)
    with synthetic_lpips():
        solver.run_method({"test": [(clean, torch.zeros(2)), (clean.flip(0), torch.zeros(2))]}, degradation(problem), SIGMA)
    return args, solver.model


def collect(save_path):
    """{relative path: text, or None for a file that is not a metric text file} of everything run_case wrote."""
    out = {}
    for root, _, files in os.walk(str(save_path)):
        for f in files:
            rel = os.path.relpath(os.path.join(root, f), str(save_path)).replace(os.sep, "/")
            metric = f.endswith(".txt") and f not in STAT_FILES
            out[rel] = open(os.path.join(root, f)).read() if metric else None
    return out
