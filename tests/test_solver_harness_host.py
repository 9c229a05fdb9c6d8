"""pnpflow_amd/methods/_harness.py on the host (no GPU, no library): the callback trampoline, the measurement-noise draw and what it
consumes of the random stream, the one-GPU refusals, Degradation.out_side, and the result-file helpers with every flag off."""
import ctypes as C
import os
import time
import types

import numpy as np
import pytest
import torch

import pnpflow_amd._lib as L
import pnpflow_amd.degradations as D
from pnpflow_amd import utils as U
from pnpflow_amd.methods import _harness as H
from pnpflow_amd.utils import CfgNode


# ---- callback trampoline --------------------------------------------------------------------------------------------------------
def test_callback_keeps_the_first_exception_and_drops_later_calls():
    seen, boom = [], ValueError("second call")

    def iter_cb(it, x):
        seen.append((it, x))
        if len(seen) == 2:
            raise boom
    call = H.IterCallback(iter_cb, 8)
    x = torch.zeros(2)
    call.bind(x)
    for it in range(5):
        call.cb(it, None)            # a CFUNCTYPE object is callable from Python; the exception does not leave it
    assert [s[0] for s in seen] == [0, 1] and all(s[1] is x for s in seen)
    with pytest.raises(ValueError) as info:
        call.reraise()
    assert info.value is boom
    ok = H.IterCallback(lambda it, x: None, 8)
    ok.cb(0, None)
    ok.reraise()                     # nothing kept: nothing raised


def test_callback_seconds_counts_the_time_inside_iter_cb():
    call = H.IterCallback(lambda it, x: time.sleep(0.01), 4)
    assert call.seconds == 0.0
    call.cb(0, None)
    assert call.seconds > 0


def test_callback_mask_and_null_callback():
    call = H.IterCallback(lambda it, x: None, 8, cb_iterations=[-1, 0, 3, 3, 7, 99])
    prm = L.PfPnpParams()
    call.attach(prm)
    assert call.mask.tolist() == [1, 0, 0, 1, 0, 0, 0, 1] and call.mask.dtype == np.uint8
    assert prm.host_cb_mask == call.mask.ctypes.data and bool(call.cb)
    # no iter_cb: a NULL callback and no mask, whatever cb_iterations says
    null = H.IterCallback(None, 8, cb_iterations=[0, 1])
    prm = L.PfPnpParams()
    null.attach(prm)
    assert not bool(null.cb) and not prm.host_cb_mask and isinstance(null.cb, L.ITER_CB)
    # cb_iterations None = every iteration: no mask
    every = H.IterCallback(lambda it, x: None, 8)
    prm = L.PfPnpParams()
    every.attach(prm)
    assert bool(every.cb) and not prm.host_cb_mask and every.mask is None


# ---- measurement noise ----------------------------------------------------------------------------------------------------------
GSHAPE, LO, HI, BATCH = (4, 3, 8, 8), 1, 3, 5


def _solver(source="cpu", hook=None):
    return types.SimpleNamespace(measurement_noise=hook, measurement_noise_source=source, device=torch.device("cpu"))


def test_gaussian_draw_and_the_stream_after_it():
    """The draw order d_flow (eps), ot_ode (init) and flow_priors (x_init) rely on: one randn of the GLOBAL shape after
    torch.manual_seed(batch), then the caller's own draws continue that stream."""
    torch.manual_seed(123)
    got = H.measurement_noise(_solver(), BATCH, torch.zeros(2, 3, 8, 8), GSHAPE, LO, HI)
    after = torch.randn(3)
    torch.manual_seed(BATCH)
    want = torch.randn(GSHAPE)[LO:HI]
    assert torch.equal(got, want) and torch.equal(after, torch.randn(3))
    assert torch.equal(H.measurement_noise(_solver(), BATCH, None, GSHAPE, LO, HI, 'gaussian'), want)


def test_laplace_draw_is_not_reseeded_by_the_batch():
    torch.manual_seed(7)
    got = H.measurement_noise(_solver(), BATCH, torch.zeros(2, 3, 8, 8), GSHAPE, LO, HI, 'laplace')
    after = torch.randn(3)
    torch.manual_seed(7)
    want = torch.distributions.laplace.Laplace(torch.zeros(GSHAPE), torch.ones(GSHAPE)).sample()[LO:HI]
    assert torch.equal(got, want) and torch.equal(after, torch.randn(3))
    torch.manual_seed(BATCH)
    assert not torch.equal(got, torch.distributions.laplace.Laplace(torch.zeros(GSHAPE), torch.ones(GSHAPE)).sample()[LO:HI])


def test_override_hook_wins_and_consumes_nothing():
    fixed, noisy = torch.full((2, 3, 8, 8), 0.5), torch.zeros(2, 3, 8, 8)
    calls = []
    hook = lambda batch, y: calls.append((batch, y)) or fixed
    torch.manual_seed(11)
    state = torch.random.get_rng_state()
    for noise_type in ('gaussian', 'laplace', 'poisson'):
        assert H.measurement_noise(_solver(hook=hook), BATCH, noisy, GSHAPE, LO, HI, noise_type) is fixed
    assert torch.equal(torch.random.get_rng_state(), state)
    assert [c[0] for c in calls] == [BATCH] * 3 and all(c[1] is noisy for c in calls)


def test_unknown_noise_type_and_device_source():
    with pytest.raises(ValueError, match="^Noise type not supported$"):
        H.measurement_noise(_solver(), BATCH, None, GSHAPE, LO, HI, 'poisson')
    got = H.measurement_noise(_solver("device"), BATCH, None, GSHAPE, LO, HI)
    want = U.draw_measurement_noise(BATCH, GSHAPE, LO, HI, torch.device("cpu"), "device")
    assert torch.equal(got, want) and got.is_contiguous()
    with pytest.raises(ValueError, match="must be 'cpu' or 'device'"):
        H.measurement_noise(_solver("host"), BATCH, None, GSHAPE, LO, HI)


# ---- one-GPU refusals -----------------------------------------------------------------------------------------------------------
TAIL = ", so a batch split over 2 ranks would change the result. Run it without torchrun."
REFUSALS = {
    "pnp_gs": "pnp_gs runs on one GPU only: its hqs deblurring branch decays alpha on norms over the whole batch" + TAIL,
    "d_flow": "d_flow runs on one GPU only: its LBFGS line search and its dopri5 step control couple the whole batch" + TAIL,
    "flow_priors": "flow_priors runs on one GPU only: multi-GPU sharding of this solver is not built" + TAIL,
}


class _NoNet:
    input_channels, input_height = 3, 64

    def to(self, device):
        return self


class _Loader:
    taken = 0

    def __iter__(self):
        return self

    def __next__(self):
        self.taken += 1
        raise AssertionError("no batch may be taken")


def _host_solver(name, monkeypatch):
    import importlib
    cls = {"pnp_gs": "PROX_PNP", "d_flow": "D_FLOW", "flow_priors": "FLOW_PRIORS"}[name]
    args = CfgNode(dict(method=name, model="gradient_step" if name == "pnp_gs" else "ot", problem="inpainting", noise_type="gaussian", algo="pgd",
                        max_iter=3, lr_pnp=1.0, alpha=0.5, sigma_factor=1.0, N=3, K=1, lmbda=1.0, eta=0.01, start_time=0.0, steps_euler=3,
                        LBFGS_iter=2, max_batch=0, compute_time=False, compute_memory=False, save_results=False, batch=0))
    monkeypatch.setattr(L, "load", lambda: object())        # D_FLOW loads the library in its constructor; none is needed here
    return getattr(importlib.import_module("pnpflow_amd.methods." + name), cls)(_NoNet(), torch.device("cpu"), args)


@pytest.mark.parametrize("name", list(REFUSALS))
def test_single_gpu_refusal_messages(name, monkeypatch):
    import pnpflow_amd.parallel as P
    s = _host_solver(name, monkeypatch)
    ld = _Loader()
    s.solve_ip(ld, D.BoxInpainting(10), 0.05)                # one rank, max_batch 0: nothing raised, nothing taken
    if name == "d_flow":                                      # looks at the joined process group only
        monkeypatch.setattr(P, "rank_world", lambda group=None: (0, 2))
    else:                                                     # also refuses before main.py has joined the group
        monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError) as info:
        s.solve_ip(ld, D.BoxInpainting(10), 0.05)
    assert str(info.value) == REFUSALS[name] and ld.taken == 0


def test_single_gpu_only_helper():
    H.single_gpu_only(1, "x runs on one GPU only: why")
    with pytest.raises(RuntimeError) as info:
        H.single_gpu_only(2, "x runs on one GPU only: why")
    assert str(info.value) == "x runs on one GPU only: why" + TAIL


# ---- Degradation.out_side -------------------------------------------------------------------------------------------------------
def test_out_side_equals_the_expression_it_replaces():
    ops = [D.Denoising(), D.BoxInpainting(10), D.RandomInpainting(0.7), D.PaintbrushInpainting(), D.GaussianDeblurring(1.0, 61, "fft", 3, 64, device="cpu"),
           D.GaussianDeblurring(1.0, 61, "zero", 3, 64, device="cpu"), D.Superresolution(2, 64), D.Superresolution(4, 64),
           D.Superresolution(2, 64, mode="bicubic"), D.Superresolution(4, 64, mode="bicubic")]
    assert {type(o) for o in ops} == {c for c in vars(D).values() if isinstance(c, type) and issubclass(c, D.Degradation) and c is not D.Degradation}
    for op in ops:
        sf = getattr(op, "sf", 1) if op.kind in (L.PF_DEG_SUPERRESOLUTION, L.PF_DEG_SR_FILTERED) else 1
        for side in (64, 128, 50):
            assert op.out_side(side) == side // sf, (type(op).__name__, side)
    assert D.Superresolution(4, 64).out_side(64) == 16 and D.Superresolution(2, 64, mode="bicubic").out_side(64) == 32 and D.Denoising().out_side(64) == 64


# ---- result files with every flag off -------------------------------------------------------------------------------------------
def test_result_file_helpers_do_nothing_with_every_flag_off(tmp_path, monkeypatch):
    called = []
    for fn in ("compute_psnr", "compute_ssim", "compute_lpips", "save_images", "compute_average_psnr", "compute_average_ssim", "compute_average_lpips",
               "compute_average_memory", "compute_average_time", "save_time_use", "save_memory_use"):
        monkeypatch.setattr(U, fn, lambda *a, _fn=fn, **k: called.append(_fn))
    args = CfgNode(dict(method="pnp_flow", model="ot", problem="inpainting", save_results=False, compute_time=False, compute_memory=False, batch=0,
                        max_batch=1, save_path=str(tmp_path), save_path_ip=str(tmp_path)))
    s = H.Solver(_NoNet(), torch.device("cpu"), args)
    x = torch.zeros(1, 3, 64, 64)
    s.write_metrics(x, x, x, lambda t: t, 0)
    s.write_final(x, x, x, lambda t: t, 0)
    H.write_batch_stats(s, 0, 1.0)
    s.write_averages()
    assert called == [] and os.listdir(str(tmp_path)) == []
    # each flag switches on its own calls only
    args.compute_time = True
    H.write_batch_stats(s, 0, 1.0); s.write_averages()
    assert called == ["save_time_use", "compute_average_time"]
    del called[:]
    args.compute_time, args.save_results = False, True
    s.write_final(x, x, x, lambda t: t, 4); s.write_averages()
    assert called == ["save_images", "compute_psnr", "compute_ssim", "compute_lpips", "compute_average_psnr", "compute_average_ssim", "compute_average_lpips"]
