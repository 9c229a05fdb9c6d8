"""PnP-Flow and OT-ODE refuse a bad pf_degradation the way the other three solvers do: PF_ERR_INVALID with a text under the solver's prefix, before
anything is allocated, copied or launched (check_operator, pnpflow_amd/csrc/solver_rt.inc, on the rules of csrc/deg_rules.h).  The tiny4 net at
64 x 64, B = 2.  Needs a real MI355X:  python -m pytest tests/test_gpu_operator_refusals.py -m gpu

Every descriptor here is one the launchers' host code stops as well (hipErrorInvalidValue before a kernel of the operator is enqueued): none can reach a
device dereference.  PF_DEG_MASK_INPAINTING without a mask and PF_DEG_SR_FILTERED without taps are pinned on the CPU (tests/test_deg_rules_host.py) and are
not sent to the GPU.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import CFGS, det_image, det_normal
from oracle import pnpflow_oracle as O

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 64, 64)
PF_ERR_INVALID = -1


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


def bad_descriptors(taps):
    """(name, descriptor); `taps`: a device buffer of at least 129 floats"""
    import pnpflow_amd._lib as L

    def d(kind, sf=0, ntaps=0, with_taps=False):
        v = L.PfDegradation()
        v.kind, v.sf, v.ntaps, v.taps = kind, sf, ntaps, (taps.data_ptr() if with_taps else None)
        return v
    return [("kind 10", d(10)), ("kind 3, sf 0", d(L.PF_DEG_SUPERRESOLUTION, sf=0)), ("kind 3, sf 3", d(L.PF_DEG_SUPERRESOLUTION, sf=3)),
            ("kind 4, 129 taps", d(L.PF_DEG_GAUSSIAN_BLUR, ntaps=129, with_taps=True)), ("kind 4, 9 taps, NULL", d(L.PF_DEG_GAUSSIAN_BLUR, ntaps=9)),
            ("kind 7, 4 x 4 PSF", d(L.PF_DEG_PSF_BLUR, ntaps=4, with_taps=True))]


def test_pnp_flow_and_ot_ode_refuse_bad_operators_and_stay_usable(hip):
    import pnpflow_amd._lib as L
    import pnpflow_amd.degradations as D
    from pnpflow_amd.methods.pnp_flow import PNP_FLOW
    from pnpflow_amd.utils import CfgNode
    m = new_model()
    y = (det_image(SHAPE, 11) + 0.05 * det_normal(SHAPE, 12)).cuda()
    solver = PNP_FLOW(m, torch.device("cuda"), CfgNode(dict(method="pnp_flow", model="ot", problem="inpainting", noise_type="gaussian", num_samples=1, steps_pnp=2,
                                                            lr_pnp=1.0, gamma_style="alpha_1_minus_t", alpha=0.3, sigma_noise=0.05, max_batch=1, compute_time=False,
                                                            compute_memory=False, save_results=False, batch=0)))
    solver.noise_seed, solver.use_graph = 4242, False

    def valid():
        return solver.restore_batch(y, D.BoxInpainting(10), 0.05, lr=0.05 ** 2).clone()
    before = valid()
    assert torch.isfinite(before).all()

    tab = np.linspace(0.1, 0.9, 4).astype(np.float32)
    fp = tab.ctypes.data_as(C.POINTER(C.c_float))
    pnp = L.PfPnpParams()
    pnp.steps, pnp.num_samples, pnp.host_t, pnp.host_coef, pnp.seed, pnp.stream_base, pnp.use_graph = 2, 1, fp, fp, 4242, 1, 1
    ode = L.PfOtOdeParams()
    ode.steps, ode.first, ode.host_t, ode.host_one_minus_t, ode.host_rt2, ode.host_coef, ode.sigma2, ode.delta, ode.use_graph = 4, 2, fp, fp, fp, fp, 0.0025, 0.25, 1
    calls = (("pnp_flow: ", hip.pf_pnp_flow_restore, pnp), ("ot_ode: ", hip.pf_ot_ode_restore, ode))
    taps = torch.full((129,), 1.0 / 129, device="cuda")
    x = torch.full(SHAPE, float("nan"), device="cuda")
    for name, d in bad_descriptors(taps):
        for prefix, restore, prm in calls:
            held = hip.pf_engine_memory_bytes(m.handle)
            with L.solver_stream():
                rc = restore(m.handle, C.byref(d), C.byref(prm), y.data_ptr(), x.data_ptr(), 2, L.current_stream_ptr(), C.cast(None, L.ITER_CB), None)
            msg = (hip.pf_last_error(m.handle) or b"").decode()
            print(f"{prefix}{name}: rc {rc}, '{msg}'")
            assert rc == PF_ERR_INVALID, (name, prefix, rc, msg)
            assert msg.startswith(prefix) and len(msg) > len(prefix), (name, prefix, msg)
            assert hip.pf_engine_memory_bytes(m.handle) == held, (name, prefix)
    torch.cuda.synchronize()
    assert torch.isnan(x).all()                      # nothing ran
    after = valid()
    assert torch.equal(after, before), f"the engine no longer reproduces its result after the refusals: max difference {float((after - before).abs().max()):.3e}"
