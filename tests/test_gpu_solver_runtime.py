"""What the solvers share on the engine (pnpflow_amd/csrc/solver_rt.inc): the cached hipGraphs and the device buffers of every solver family,
on the tiny4 net at 64 x 64, B = 2.  Needs a real MI355X:  python -m pytest tests/test_gpu_solver_runtime.py -m gpu

1. every cached graph is dropped when the precision mode or the solver time scale changes (a captured graph bakes both in);
2. a plan a cached graph replays survives the plan cache's eviction;
3. the device bytes of the solver families that had no such test are counted, stay put on a second call, and come back on destroy.

Graph runs are compared with direct launches (and with earlier graph runs) by the rule of each solver's own graph test:
  PnP-Flow   atol 1e-5 (test_philox_path_is_deterministic_and_graph_equals_eager: the statistics atomics reorder the last bits)
  OT-ODE     1e-3 max|x| (test_ot_ode_graph_replays_are_reproducible_at_size: the recursion amplifies that reordering)
  D-Flow     relative 1e-6 (test_graph_replay_matches_eager_and_rebuilds_on_change)
  Prox-PnP   bitwise (test_replays_are_bit_identical_and_graphs_rebuild)
On this net (the OT U-Net) the solver time scale does not enter any launch - only NCSN++ reads it - so that step holds the drop and the
re-capture to a consistent graph, not to changed numbers.
"""
import gc

import numpy as np
import pytest
import torch

from conftest import CFGS, det_image, det_normal
from oracle import pnpflow_oracle as O

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 64, 64)


@pytest.fixture(scope="module")
def hip():
    import pnpflow_amd._lib as L
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return L.load()


def new_model():
    from pnpflow_amd.models import UNet
    c = CFGS["tiny4"]
    m = UNet(c["input_channels"], c["input_height"], c["ch"], ch_mult=c["ch_mult"], num_res_blocks=c["num_res_blocks"], attn_resolutions=c["attn_resolutions"])
    m.load_state_dict(O.synthetic_state_dict(O.unet_config(**c), 0))
    return m


_MODEL = []


def shared_model():
    if not _MODEL:
        _MODEL.append(new_model())
    return _MODEL[0]


def cfg(**kw):
    from pnpflow_amd.utils import CfgNode
    a = dict(model="ot", max_batch=1, compute_time=False, compute_memory=False, save_results=False, batch=0)
    a.update(kw)
    return CfgNode(a)


def measurement(seed):
    return (det_image(SHAPE, seed) + 0.05 * det_normal(SHAPE, seed + 1)).cuda()


# ---- the six graph users: case(m) -> (run(use_graph, B=2) -> tuple of tensors, same(a, b) -> None or raises) --------------------------------------
def close(atol=0.0, rel=0.0):
    def same(a, b):
        for p, q in zip(a, b):
            np.testing.assert_allclose(p.cpu().numpy(), q.cpu().numpy(), rtol=0, atol=atol + rel * float(q.abs().max()))
    return same


def bitwise(a, b):
    for p, q in zip(a, b):
        assert torch.equal(p, q), f"max difference {float((p - q).abs().max()):.3e}"


def pnp_flow_case(m):
    from pnpflow_amd.methods.pnp_flow import PNP_FLOW
    import pnpflow_amd.degradations as D
    s = PNP_FLOW(m, torch.device("cuda"), cfg(method="pnp_flow", problem="inpainting", noise_type="gaussian", num_samples=2, steps_pnp=4, lr_pnp=1.0,
                                               gamma_style="alpha_1_minus_t", alpha=0.3, sigma_noise=0.05))
    s.noise_seed = 4242
    y, dg = measurement(11), D.BoxInpainting(10)

    def run(use_graph, B=2):
        s.use_graph = use_graph
        return (s.restore_batch(y[:B], dg, 0.05, lr=0.05 ** 2).clone(),)
    return run, close(atol=1e-5)


def ot_ode_case(m, zero_blur):
    from pnpflow_amd.methods.ot_ode import OT_ODE
    import pnpflow_amd.degradations as D
    s = OT_ODE(m, torch.device("cuda"), cfg(method="ot_ode", problem="gaussian_deblurring" if zero_blur else "inpainting", steps_ode=10, start_time=0.6,
                                            gamma="constant"))
    y = measurement(13)
    dg = D.GaussianDeblurring(1.0, 61, "spatial", 3, 64) if zero_blur else D.BoxInpainting(10)
    noise = det_normal(SHAPE, 15).cuda()

    def run(use_graph, B=2):
        s.use_graph = use_graph
        s.init_noise = noise[:B]
        return (s.restore_batch(y[:B], dg, 0.05).clone(),)
    return run, close(rel=1e-3)


def d_flow_case(m, closure):
    from pnpflow_amd.methods.d_flow import D_FLOW
    import pnpflow_amd.degradations as D
    s = D_FLOW(m, torch.device("cuda"), cfg(method="d_flow", problem="denoising", steps_euler=6, lmbda=0.001, alpha=0.1, max_iter=1, LBFGS_iter=3,
                                            start_time=0.0))
    z, y, dg = det_normal(SHAPE, 17).cuda(), det_normal(SHAPE, 18).cuda(), D.Denoising()

    def run(use_graph, B=2):
        s.use_graph = use_graph
        if closure:
            loss, grad = s.value_and_grad(z[:B], y[:B], dg, 0.001)
            return loss.clone(), grad.clone()
        return (s.forward_flow_matching(z[:B]).clone(),)

    def same(a, b):
        if closure:
            np.testing.assert_allclose(a[0].cpu().numpy(), b[0].cpu().numpy(), rtol=1e-6)
        close(rel=1e-6)(a[-1:], b[-1:])
    return run, same


def pnp_gs_case(m):
    from pnpflow_amd.methods.pnp_gs import PROX_PNP
    from pnpflow_amd.train_denoiser import GRADIENT_STEP_DENOISER
    import pnpflow_amd.degradations as D
    args = cfg(method="pnp_gs", model="gradient_step", problem="inpainting", noise_type="gaussian", algo="pgd", max_iter=3, lr_pnp=1.0, alpha=0.5,
               sigma_factor=1.0, dim_image=64, num_channels=3)
    s = PROX_PNP(GRADIENT_STEP_DENOISER(m, torch.device("cuda"), args), torch.device("cuda"), args)
    y, dg = measurement(19), D.BoxInpainting(10)

    def run(use_graph, B=2):
        s.use_graph = use_graph
        return (s.restore_batch(y[:B], dg, 0.05).clone(),)
    return run, bitwise


CASES = {"pnp_flow": pnp_flow_case,
         "ot_ode_closed_form": lambda m: ot_ode_case(m, False),
         "ot_ode_zero_blur": lambda m: ot_ode_case(m, True),
         "d_flow_value_and_grad": lambda m: d_flow_case(m, True),
         "d_flow_forward": lambda m: d_flow_case(m, False),
         "pnp_gs_pgd": pnp_gs_case}


@pytest.mark.parametrize("name", list(CASES))
def test_cached_graphs_are_dropped_when_precision_or_time_scale_change(hip, name):
    m = shared_model()
    run, same = CASES[name](m)
    try:
        g1 = run(True)
        g1b = run(True)                           # a graph is cached now: this call replayed it from the first iteration on
        same(g1b, g1)
        m.set_precision(2)
        g2, e2 = run(True), run(False)
        same(g2, e2)
        m.set_precision(1)
        assert hip.pf_engine_set_solver_time_scale(m.handle, 0.5) == 0
        g3, e3 = run(True), run(False)
        same(g3, e3)
        assert hip.pf_engine_set_solver_time_scale(m.handle, 1.0) == 0
        g4, e4 = run(True), run(False)
        same(g4, e4)
        same(g4, g1)
    finally:
        m.set_precision(1)
        hip.pf_engine_set_solver_time_scale(m.handle, 1.0)


@pytest.mark.parametrize("name", list(CASES))
def test_plan_of_a_cached_graph_survives_eviction(hip, name):
    m = shared_model()
    run, same = CASES[name](m)
    g1 = run(True)
    for B in (1, 3, 4, 5, 6, 7, 8, 9, 10):        # nine more plans than the one the graph replays: the cache keeps eight
        m(torch.zeros((B, 3, 64, 64), device="cuda"), torch.full((B,), 0.3, device="cuda"))
    g2 = run(True)
    same(g2, g1)
    v = m.forward_retain(det_normal(SHAPE, 21).cuda(), torch.full((2,), 0.3, device="cuda"))
    assert torch.isfinite(m.backward(torch.ones_like(v))).all()


# ---- device bytes ----------------------------------------------------------------------------------------------------------------------------------
def prior_eval_call(m, B):
    x, eps = det_image(SHAPE, 23).cuda()[:B], det_normal(SHAPE, 24).cuda()[:B]
    m.divergence(x, torch.full((B,), 0.5), eps)          # first stage: g, stage, t and the doubles
    m.likelihood_ode(x, eps, rtol=1e-2, atol=1e-2)       # second stage, added to the live state: y, y1 and the seven stage buffers


def byte_cases():
    graphed = lambda run: lambda B: run(True, B)
    return {"pnp_flow": lambda m: graphed(pnp_flow_case(m)[0]),
            "ot_ode_closed_form": lambda m: graphed(ot_ode_case(m, False)[0]),
            "ot_ode_fourier": lambda m: graphed(ot_ode_fourier_run(m)),
            "ot_ode_krylov": lambda m: graphed(ot_ode_case(m, True)[0]),
            "d_flow_closure": lambda m: graphed(d_flow_case(m, True)[0]),
            "dopri5": dopri5_run,
            "prior_eval": lambda m: lambda B: prior_eval_call(m, B)}


def ot_ode_fourier_run(m):
    from pnpflow_amd.methods.ot_ode import OT_ODE
    import pnpflow_amd.degradations as D
    s = OT_ODE(m, torch.device("cuda"), cfg(method="ot_ode", problem="gaussian_deblurring_FFT", steps_ode=10, start_time=0.6, gamma="constant"))
    y, dg, noise = measurement(13), D.GaussianDeblurring(1.0, 61, "fft", 3, 64), det_normal(SHAPE, 15).cuda()

    def run(use_graph, B=2):
        s.use_graph = use_graph
        s.init_noise = noise[:B]
        return s.restore_batch(y[:B], dg, 0.05)
    return run


def dopri5_run(m):
    from pnpflow_amd.methods.d_flow import D_FLOW
    s = D_FLOW(m, torch.device("cuda"), cfg(method="d_flow", problem="denoising", steps_euler=6, lmbda=0.001, alpha=0.1, max_iter=1, LBFGS_iter=3, start_time=0.0))
    x0 = det_image(SHAPE, 41).cuda()
    return lambda B: s.inverse_flow_matching(x0[:B])


# memory_bytes() after the B = 2 call and after the B = 1 call, less the bytes of the weights (the fresh engine's count), measured on an MI355X on
# commit aa3c588 ("Add zero-boundary Gaussian deblurring and a batched GMRES on the device").  The sizes asked of hipMalloc are deterministic: no margin.
EXPECTED_BYTES = {"pnp_flow": (109472720, 120117952),
                  "ot_ode_closed_form": (217003680, 239952784),
                  "ot_ode_fourier": (217397408, 240149904),
                  "ot_ode_krylov": (227598496, 245250248),
                  "d_flow_closure": (230850976, 258556832),
                  "dopri5": (98484560, 103537232),
                  "prior_eval": (217595200, 240248824)}


@pytest.mark.parametrize("name", list(EXPECTED_BYTES))
def test_solver_buffers_are_counted_and_freed(hip, name):
    m = new_model()                               # an engine of its own
    call = byte_cases()[name](m)
    b0 = m.memory_bytes()
    call(2)
    b1 = m.memory_bytes()
    call(2)
    assert m.memory_bytes() == b1, "a second identical call changes the count"
    call(1)                                       # shape change: the B = 2 state is freed, a B = 1 one allocated
    b2 = m.memory_bytes()
    print(f"solver runtime bytes {name}: ({b1 - b0}, {b2 - b0})")
    assert (b1 - b0, b2 - b0) == EXPECTED_BYTES[name]
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    del call, m
    gc.collect()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] - free_before >= 0.9 * b2, "destroying the model does not give its device memory back"
