"""CPU checks of the rectified-flow samplers: the restatement (tests/rf_sampler_restatement.py) on the NCSN++ oracle against the outputs of the
REAL reference samplers on the REAL module (tests/golden/rf_sampler_tiny.npz, tools/make_golden_rf_sampler.py), the C ABI surface, and the Python
surface (sampling.py, sde_lib.py, PriorSampler) on a fake net that records what it is handed.  No GPU needed.

Tolerance of the restatement: the oracle is held to the real module at 1e-6 of max|output| (test_oracle_golden.py
test_ncsnpp_oracle_matches_reference_module: the same ops in the same order, observed 0), so the samplers' outputs are held to 1e-6 of max|x|
and the adaptive solves to the same evaluation count.
"""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import rf_sampler_restatement as R
from conftest import det_image, det_normal
from oracle import ncsnpp_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(image_size=32, nf=32, ch_mult=(1, 1, 2), num_res_blocks=2, attn_resolutions=(16,))
SHAPE = (2, 3, 32, 32)
PF_ERR_INVALID = -1


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "rf_sampler_tiny.npz"))


@pytest.fixture(scope="module")
def net():
    cfg = NO.ncsnpp_config(**TINY)
    sd = NO.synthetic_state_dict(cfg, 0)
    return lambda x, lab: NO.ncsnpp_forward(sd, cfg, x, lab)


# ---- 1. the restatement against the real samplers ---------------------------------------------------------------------------------------
def test_restatement_euler_matches_the_real_sampler(gold, net):
    z = det_normal(SHAPE, int(gold["z_seed"]))
    x, nfe = R.euler_sampler(net, z, 4)
    assert nfe == int(gold["a_nfe"]) == 4
    np.testing.assert_allclose(x.numpy(), gold["a_x"], rtol=0, atol=1e-6 * float(np.abs(gold["a_x"]).max()))
    noise = torch.from_numpy(gold["b_noise"])
    xs, _ = R.euler_sampler(net, z, 4, sigma_var=float(gold["b_sigma_var"]), noise=noise)
    np.testing.assert_allclose(xs.numpy(), gold["b_x"], rtol=0, atol=1e-6 * float(np.abs(gold["b_x"]).max()))
    assert float((xs - x).abs().max()) > 0.1          # the noise term is there
    e = R.euler_ode(net, z, N=3)
    np.testing.assert_allclose(e.numpy(), gold["e_x"], rtol=0, atol=1e-6 * float(np.abs(gold["e_x"]).max()))
    assert torch.equal(e, R.euler_ode(net, z, reverse=True, N=3))          # `reverse` is ignored, as in the reference
    with pytest.raises(ValueError, match="normal draws"):
        R.euler_sampler(net, z, 2, sigma_var=0.1)


def test_restatement_rk45_matches_the_real_sampler(gold, net):
    z = det_normal(SHAPE, int(gold["z_seed"]))
    y, nfev, accepted = R.rk45_sampler(net, z, 1e-5)
    assert nfev == int(gold["c_ref32_nfev"]) and (nfev - 2) % 6 == 0 and 1 <= accepted <= (nfev - 2) // 6
    np.testing.assert_allclose(y.astype(np.float32), gold["c_ref32_x"], rtol=0, atol=1e-6 * float(np.abs(gold["c_ref32_x"]).max()))


def test_restatement_reverse_ode_matches_the_real_sde(gold, net):
    x0 = det_image(SHAPE, int(gold["x_seed"]))
    y, nfev, _ = R.ode(net, x0, reverse=True)
    assert nfev == int(gold["d_ref32_nfev"])
    np.testing.assert_allclose(y.astype(np.float32), gold["d_ref32_x"], rtol=0, atol=1e-6 * float(np.abs(gold["d_ref32_x"]).max()))
    # the fixture's yardsticks are consistent: the fp64 run at the same tolerance sits where the stored gap says
    for c in "cd":
        assert float(np.abs(gold[c + "_ref32_x"].astype(np.float64) - gold[c + "_ref64_x"]).max()) == pytest.approx(float(gold[c + "_gap"]), rel=1e-3, abs=1e-7)
        assert int(gold[c + "_tight_nfev"]) > 10 * int(gold[c + "_ref64_nfev"])


# ---- 2. ABI surface -----------------------------------------------------------------------------------------------------------------------
def _fields(header, name):
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(ty, f) for ty, decl in re.findall(r"(double|int32_t|uint64_t)\s+([^;]+);", body) for f in re.split(r"\s*,\s*", decl.strip())]


def test_symbols_declared_exported_and_typed():
    import pnpflow_amd._lib as L
    header = open(os.path.join(ROOT, "include", "pnpflow_hip.h")).read()
    lib = L.load()
    for name in ("pf_rf_euler_sampler", "pf_flow_ode_rk45"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in include/pnpflow_hip.h"
        assert name in L.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1] and getattr(lib, name).restype is C.c_int
    m = re.search(r"#define PF_ABI_VERSION (\d+)", header)
    assert int(m.group(1)) == L.PF_ABI_VERSION == lib.pf_abi_version() == 6
    size = dict(double=8, int32_t=4, uint64_t=8)
    ctype = dict(double=C.c_double, int32_t=C.c_int32, uint64_t=C.c_uint64)
    for cname, struct in (("pf_rf_sampler_params", L.PfRfSamplerParams), ("pf_rk45_params", L.PfRk45Params)):
        fields = _fields(header, cname)
        assert [f for _, f in fields] == [f[0] for f in struct._fields_], fields
        assert [ctype[t] for t, _ in fields] == [f[1] for f in struct._fields_]
        assert C.sizeof(struct) == sum(size[t] for t, _ in fields)          # naturally aligned as declared: no padding
    assert C.sizeof(L.PfRfSamplerParams) == 56 and C.sizeof(L.PfRk45Params) == 40


def test_null_engine_and_null_arguments_are_invalid():
    import pnpflow_amd._lib as L
    lib = L.load()
    sp, rp = L.PfRfSamplerParams(), L.PfRk45Params()
    sp.t_begin, sp.t_end, sp.n_steps, sp.sigma_var, sp.noise_scale = 1e-3, 1.0, 4, 0.0, 1.0
    rp.t0, rp.t1, rp.rtol, rp.atol, rp.max_attempts = 1e-3, 1.0, 1e-5, 1e-5, 10
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    stats = (C.c_int64 * 3)(7, 7, 7)
    assert lib.pf_rf_euler_sampler(None, C.byref(sp), p, None, p, 1, None) == PF_ERR_INVALID
    assert lib.pf_rf_euler_sampler(None, None, p, None, p, 1, None) == PF_ERR_INVALID
    assert lib.pf_rf_euler_sampler(None, C.byref(sp), None, None, None, 0, None) == PF_ERR_INVALID
    assert lib.pf_flow_ode_rk45(None, C.byref(rp), p, p, stats, 1, None) == PF_ERR_INVALID
    assert lib.pf_flow_ode_rk45(None, None, None, None, None, -1, None) == PF_ERR_INVALID
    for bad in (dict(n_steps=0), dict(sigma_var=-1.0), dict(noise_scale=0.0), dict(t_end=1e-3), dict(t_begin=float("nan"))):
        q = L.PfRfSamplerParams()
        C.memmove(C.byref(q), C.byref(sp), C.sizeof(sp))
        for k, v in bad.items():
            setattr(q, k, v)
        assert lib.pf_rf_euler_sampler(None, C.byref(q), p, None, p, 1, None) == PF_ERR_INVALID
    for bad in (dict(rtol=0.0), dict(atol=-1.0), dict(t1=1e-3), dict(t0=float("inf")), dict(max_attempts=0)):
        q = L.PfRk45Params()
        C.memmove(C.byref(q), C.byref(rp), C.sizeof(rp))
        for k, v in bad.items():
            setattr(q, k, v)
        assert lib.pf_flow_ode_rk45(None, C.byref(q), p, p, stats, 1, None) == PF_ERR_INVALID
    assert list(stats) == [7, 7, 7] and not any(buf)


# ---- 3. Python surface ----------------------------------------------------------------------------------------------------------------------
class FakeNet:
    """Records what sampling.py / sde_lib.py hand to the engine net; `scaled`: it takes a scaled label, like NCSNpp."""
    input_channels, input_height, handle = 3, 8, 1

    def __init__(self, scaled=True):
        self.calls, self.scale = [], None
        if scaled:
            self.set_solver_time_scale = lambda s: setattr(self, "scale", s)

    def rf_euler(self, x, n_steps, t_begin=1e-3, t_end=1.0, sigma_var=0.0, noise_scale=1.0, noise=None, seed=0, stream_id=0):
        self.calls.append(("euler", n_steps, t_begin, t_end, sigma_var, noise_scale, self.scale, noise, seed, stream_id, x.clone()))
        return x + 1

    def ode_rk45(self, x, t0, t1, rtol, atol, max_attempts=1000):
        self.calls.append(("rk45", t0, t1, rtol, atol, self.scale, x.clone()))
        return x + 2, dict(accepted=3, rejected=1, nfev=26)


def sampling_config(**kw):
    from pnpflow_amd.image_generation.configs.rectified_flow.celeba_hq_pytorch_rf_gaussian import get_config
    cfg = get_config()
    cfg.sampling.update(kw)
    cfg.device = "cpu"
    return cfg


def test_get_sampling_fn_surface_and_refusals():
    from pnpflow_amd.image_generation import sampling as S, sde_lib as D
    cfg = sampling_config()
    assert (cfg.sampling.init_type, cfg.sampling.use_ode_sampler, cfg.sampling.ode_tol, cfg.sampling.sigma_variance) == ("gaussian", "rk45", 1e-5, 0.0)
    scaler = lambda x: (x + 1.) / 2.
    z = torch.arange(2 * 3 * 8 * 8, dtype=torch.float32).view(2, 3, 8, 8)
    # rk45: (eps, T) at ode_tol, label scale 999 on a net that has one, the count of evaluations back
    sde = S.rectified_flow_from_config(cfg, ode_tol=1e-4)
    assert (sde.T, sde.noise_scale, sde.use_ode_sampler, sde.ode_tol, sde.sample_N, sde.sigma_t(0.25)) == (1., 1.0, "rk45", 1e-4, 1000, 0.0)
    fn = S.get_sampling_fn(cfg, sde, (2, 3, 8, 8), scaler, 1e-3)
    net = FakeNet()
    x, nfe = fn(net, z=z)
    assert nfe == 26 and torch.equal(x, scaler(z + 2)) and fn.last_stats["accepted"] == 3
    assert net.calls[0][:6] == ("rk45", 1e-3, 1., 1e-4, 1e-4, 999.0)
    # euler: sample_N steps from 1e-3 to T; sigma_var and the initial noise scale go through; a U-Net-like net keeps t as it is
    sde = D.RectifiedFlow(init_type="gaussian", noise_scale=2.0, use_ode_sampler="euler", sigma_var=0.5, sample_N=7)
    assert sde.sigma_t(0.5) == 0.25
    fn = S.get_rectified_flow_sampler(sde, (2, 3, 8, 8), scaler, device="cpu")
    for scaled, want in ((True, 999.0), (False, None)):
        net = FakeNet(scaled)
        noise = torch.zeros(7, 2, 3, 8, 8)
        x, nfe = fn(net, z=z, noise=noise)
        assert nfe == 7 and torch.equal(x, scaler(z + 1))
        assert net.calls[0][:7] == ("euler", 7, 1e-3, 1., 0.5, 2.0, want) and net.calls[0][7] is noise
    # no latent: get_z0, a CPU torch.randn draw times noise_scale that torch.manual_seed reproduces; no noise: a Philox key per call
    net = FakeNet()
    torch.manual_seed(5)
    fn(net)
    fn(net)
    torch.manual_seed(5)
    want = torch.randn(2, 3, 8, 8) * 2.0
    assert torch.equal(net.calls[0][-1], want) and not torch.equal(net.calls[1][-1], want)
    assert net.calls[0][8] == net.calls[1][8] == 5 and net.calls[1][9] == net.calls[0][9] + 1
    assert sde.get_z0(torch.zeros(4, 1, 2, 2)).shape == (4, 1, 2, 2) and not sde.get_z0(torch.zeros(4, 1, 2, 2)).is_cuda
    # refusals, with the reference's texts
    with pytest.raises(ValueError, match="Sampler name pc unknown."):
        S.get_sampling_fn(sampling_config(method="pc"), sde, (2, 3, 8, 8), scaler, 1e-3)
    with pytest.raises(AssertionError, match="Not Implemented!"):
        S.get_rectified_flow_sampler(D.RectifiedFlow(use_ode_sampler="heun"), (2, 3, 8, 8), scaler)
    with pytest.raises(NotImplementedError, match="INITIALIZATION TYPE NOT IMPLEMENTED"):
        D.RectifiedFlow(init_type="uniform").get_z0(torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="reflow"):
        D.RectifiedFlow(reflow_flag=True)
    with pytest.raises(TypeError, match="engine net"):
        fn(object(), z=z)
    with pytest.raises(ValueError, match="unknown sampling overrides"):
        S.rectified_flow_from_config(cfg, steps=3)


def test_sde_ode_and_euler_ode():
    from pnpflow_amd.image_generation import sde_lib as D
    sde = D.RectifiedFlow()
    z = torch.ones(1, 3, 8, 8)
    net = FakeNet()
    assert torch.equal(sde.ode(z, net), z + 2) and torch.equal(sde.ode(z, net, reverse=True), z + 2)
    assert net.calls[0][:6] == ("rk45", 1e-3, 1., 1e-5, 1e-5, 999.0) and net.calls[1][:6] == ("rk45", 1., 1e-3, 1e-5, 1e-5, 999.0)
    assert sde.last_ode_stats["nfev"] == 26
    net = FakeNet()
    sde.euler_ode(z, net, N=5); sde.euler_ode(z, net, reverse=True, N=5); sde.euler_ode(z, net)
    assert net.calls[0][:7] == net.calls[1][:7] == ("euler", 5, 1e-3, 1., 0.0, 1.0, 999.0) and net.calls[2][1] == 100
    assert "IGNORED" in D.RectifiedFlow.euler_ode.__doc__ and "share one step sequence" in D.RectifiedFlow.ode.__doc__


def test_reference_import_paths():
    import pnpflow.image_generation.sampling as RS
    import pnpflow.image_generation.sde_lib as RD
    from pnpflow_amd.image_generation import sampling as S, sde_lib as D
    assert RS.get_sampling_fn is S.get_sampling_fn and RS.get_rectified_flow_sampler is S.get_rectified_flow_sampler and RS.PriorSampler is S.PriorSampler
    assert RD.RectifiedFlow is D.RectifiedFlow


def test_prior_sampler_rounds_and_batches():
    from pnpflow_amd.image_generation import sampling as S, sde_lib as D
    P = S.PriorSampler
    assert P.batch_sizes(10, 4) == [4, 4, 2] and P.batch_sizes(8, 4) == [4, 4] and P.batch_sizes(3, 4) == [3] and P.batch_sizes(5, None) == [5]
    assert P.batch_sizes(0, 4) == []
    net = FakeNet()
    sde = D.RectifiedFlow(use_ode_sampler="euler", sample_N=2)
    ps = P(net, sde, (4, 3, 8, 8), device="cpu")
    latent = torch.arange(10 * 3 * 8 * 8, dtype=torch.float32).view(10, 3, 8, 8)
    out = ps.generate_samples(10, latent=latent)          # batch size: shape[0]
    assert torch.equal(out, latent + 1) and [c[-1].shape[0] for c in net.calls] == [4, 4, 2] and ps.last_nfe == 2
    assert torch.equal(torch.cat([c[-1] for c in net.calls]), latent)          # the data range is the net's own: the inverse scaler is the identity
    net.calls.clear()
    assert ps.generate_samples(5, batch_size=5).shape == (5, 3, 8, 8) and ps.apply_flow_matching(3).shape == (3, 3, 8, 8)
    assert [c[-1].shape[0] for c in net.calls] == [5, 3]
    assert ps.apply_flow_matching(0).shape == (0, 3, 8, 8) and len(net.calls) == 2
    with pytest.raises(ValueError, match="latent holds"):
        ps.apply_flow_matching(2, latent=latent)
    assert "999" in P.__doc__


def test_entry_points_name_the_rectified_model():
    import main
    src = open(os.path.join(ROOT, "main.py")).read()
    assert "'ot' or 'indep'" in src and "'rectified'" in src
    args = types.SimpleNamespace(model="rectified", batch_size_ip=4, num_channels=3, dim_image=8, use_ode_sampler="euler", sample_N=3, sigma_variance=0.25)
    net = FakeNet(); net.config = sampling_config()
    ps = main.prior_sampler(args, net, "cpu")
    assert (ps.sde.use_ode_sampler, ps.sde.sample_N, ps.sde.sigma_t(0.0), ps.sde.ode_tol, ps.shape) == ("euler", 3, 0.25, 1e-5, (4, 3, 8, 8))
    report = open(os.path.join(ROOT, "tools", "prior_report.py")).read()
    assert "does not implement" not in report and "prior_sampler" in report
