"""The rectified-flow samplers on the engine - pf_rf_euler_sampler (Euler / Euler-Maruyama, injected and in-kernel noise), pf_flow_ode_rk45 (both
directions) and the Python surface on top of them - against the CPU restatement (tests/rf_sampler_restatement.py) on the oracles and against
the outputs of the REAL reference samplers (tests/golden/rf_sampler_tiny.npz, tools/make_golden_rf_sampler.py).
Needs a real MI355X:  python -m pytest tests -m gpu

Tolerances:
  Euler, N <= 4 chained evaluations      5 x NX_RTOL x max|v| on the NCSN++ net (NX_RTOL = 1e-5 of test_gpu_ncsnpp.py, relative to the largest velocity
                                         of the trajectory; the chained-evaluation factor 5 of test_euler_sampling_matches_oracle_loop), 5 x FWD_ATOL on
                                         the U-Net
  in-kernel Philox draw                  1e-6 x max|x| against the run fed O.engine_normal's restatement of the same numbers (the device's logf /
                                         sincosf differ from numpy's in the last bits: test_gpu_prior_eval.py holds the fill itself to 2e-5)
  RK45                                   distance to the fp64 rtol = atol = 1e-9 solution at most 1.5 x the real fp32 SciPy run's, plus twice the stored
                                         |ref32 - ref64| gap (the criterion of test_likelihood_matches_scipy_fixture)
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rf_sampler_restatement as R
from conftest import CFGS, det_image, det_normal
from oracle import ncsnpp_oracle as NO
from oracle import pnpflow_oracle as O

pytestmark = pytest.mark.gpu

NX_RTOL = 1e-5          # test_gpu_ncsnpp.py
FWD_ATOL = 2e-5         # test_gpu_prior_eval.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(image_size=32, nf=32, ch_mult=(1, 1, 2), num_res_blocks=2, attn_resolutions=(16,))
SHAPE = (2, 3, 32, 32)

_CACHE = {}


@pytest.fixture(scope="module")
def hip():
    import pnpflow_amd._lib as L
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return L.load()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "rf_sampler_tiny.npz"))


def ncsnpp():
    """(engine net of its own - the solver time scale stays out of other tests -, oracle forward)"""
    if "ncsnpp" not in _CACHE:
        from pnpflow_amd.image_generation.models.ncsnpp import NCSNpp
        from test_gpu_ncsnpp import ref_config
        cfg = NO.ncsnpp_config(**TINY); sd = NO.synthetic_state_dict(cfg, 0)
        m = NCSNpp(ref_config(TINY)); m.load_state_dict(sd)
        m.set_solver_time_scale(999.0)
        _CACHE["ncsnpp"] = (m, lambda x, lab: NO.ncsnpp_forward(sd, cfg, x, lab))
    return _CACHE["ncsnpp"]


def euler_reference(N, z):
    """(restatement's x, max|v| over its trajectory) at sigma_var = 0, computed once per N"""
    if ("euler", N) not in _CACHE:
        _m, f = ncsnpp()
        vmax = [0.0]

        def fn(x, lab):
            v = f(x, lab)
            vmax[0] = max(vmax[0], float(v.abs().max()))
            return v
        x, _ = R.euler_sampler(fn, z, N)
        _CACHE[("euler", N)] = (x, vmax[0])
    return _CACHE[("euler", N)]


# ---- 1. Euler ODE -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("N", [4, 1])
def test_euler_ode_matches_restatement_and_real_sampler(hip, gold, N, mode):
    m, _f = ncsnpp()
    z = det_normal(SHAPE, int(gold["z_seed"]))
    ref, vmax = euler_reference(N, z)
    m.set_precision(mode)
    try:
        x = m.rf_euler(z.cuda(), N).cpu()
        m.check_numerics()
    finally:
        m.set_precision(1)
    bound = 5 * NX_RTOL * vmax
    err = float((x - ref).abs().max())
    print(f"rf_euler tiny N={N} mode={mode}: max|hip - restatement| {err:.3g}, bound {bound:.3g} (max|v| {vmax:.4g})")
    assert err <= bound
    if N == 4:
        eg = float(np.abs(x.numpy() - gold["a_x"]).max())
        print(f"  max|hip - real sampler| {eg:.3g}")
        assert eg <= bound
    assert float((x - z).abs().max()) > 0.1          # the sampler moved the latent


# ---- 2. SDE step with injected noise --------------------------------------------------------------------------------------------------------
def test_sde_step_with_injected_noise_matches_real_sampler(hip, gold):
    m, _f = ncsnpp()
    z = det_normal(SHAPE, int(gold["z_seed"]))
    _ref, vmax = euler_reference(4, z)
    noise = torch.from_numpy(gold["b_noise"]).cuda()
    x = m.rf_euler(z.cuda(), 4, sigma_var=float(gold["b_sigma_var"]), noise=noise).cpu()
    m.check_numerics()
    err = float(np.abs(x.numpy() - gold["b_x"]).max())
    print(f"rf_euler tiny sigma_var=0.5 injected: max|hip - real sampler| {err:.3g}, bound {5 * NX_RTOL * vmax:.3g}")
    assert err <= 5 * NX_RTOL * vmax
    assert float(np.abs(gold["b_x"] - gold["a_x"]).max()) > 0.1          # the fixture's noise term is there


# ---- 3. Philox path ------------------------------------------------------------------------------------------------------------------------
def test_in_kernel_philox_draw_is_the_engine_stream(hip, gold):
    m, _f = ncsnpp()
    z = det_normal(SHAPE, int(gold["z_seed"])).cuda()
    N, tot = 4, int(np.prod(SHAPE))
    drawn = m.rf_euler(z, N, sigma_var=0.5, seed=3, stream_id=4)
    noise = torch.from_numpy(np.stack([O.engine_normal(tot, 3, 4, offset=i * tot) for i in range(N)])).view((N,) + SHAPE).float().cuda()
    fed = m.rf_euler(z, N, sigma_var=0.5, noise=noise)
    plain = m.rf_euler(z, N)
    m.check_numerics()
    err, scale = float((drawn - fed).abs().max()), float(fed.abs().max())
    print(f"rf_euler tiny philox: max|drawn - fed| {err:.3g} of max|x| {scale:.4g}")
    assert err <= 1e-6 * scale
    assert float((drawn - plain).abs().max()) > 0.1
    assert torch.equal(drawn, m.rf_euler(z, N, sigma_var=0.5, seed=3, stream_id=4))          # the draw is a function of (seed, stream, offset)
    assert not torch.equal(drawn, m.rf_euler(z, N, sigma_var=0.5, seed=3, stream_id=5))


# ---- 4. tail and second net -------------------------------------------------------------------------------------------------------------------
def test_unet_with_a_ragged_tail(hip):
    """gray40: 1 x 40 x 40 = 400 float4 lanes per image, 1200 in the batch of 3: not a multiple of the 256-thread block; time scale 1."""
    from pnpflow_amd.models import UNet
    c = CFGS["gray40"]
    cfg = O.unet_config(**c); sd = O.synthetic_state_dict(cfg, 0)
    m = UNet(c["input_channels"], c["input_height"], c["ch"], ch_mult=c["ch_mult"], num_res_blocks=c["num_res_blocks"], attn_resolutions=c["attn_resolutions"])
    m.load_state_dict(sd)
    shape = (3, 1, 40, 40)
    z = det_normal(shape, 71)
    noise = torch.stack([det_normal(shape, 72, i) for i in range(2)])
    ref, _ = R.euler_sampler(lambda x, lab: O.unet_forward(sd, cfg, x, lab), z, 2, sigma_var=0.3, noise=noise, label_scale=1)
    # in place through the C call, inside a padded buffer: the update must stay inside [0, B n)
    import pnpflow_amd._lib as L
    pad = torch.full((z.numel() + 64,), 7.0, device="cuda")
    buf = pad[32:32 + z.numel()].view(shape)
    buf.copy_(z)
    nz = noise.cuda()
    prm = L.PfRfSamplerParams()
    prm.t_begin, prm.t_end, prm.n_steps, prm.sigma_var, prm.noise_scale = 1e-3, 1.0, 2, 0.3, 1.0
    L.check(hip.pf_rf_euler_sampler(m.handle, C.byref(prm), buf.data_ptr(), nz.data_ptr(), buf.data_ptr(), 3, L.current_stream_ptr()), m.handle, "pf_rf_euler_sampler")
    m.check_numerics()
    x = buf.cpu()
    err = float((x - ref).abs().max())
    print(f"rf_euler gray40 B=3 N=2 sigma_var=0.3: max|hip - restatement| {err:.3g}, bound {5 * FWD_ATOL:.3g}")
    assert err <= 5 * FWD_ATOL
    assert bool((pad[:32] == 7.0).all()) and bool((pad[32 + z.numel():] == 7.0).all())
    assert torch.equal(m.rf_euler(z.cuda(), 2, sigma_var=0.3, noise=nz).cpu(), x)          # the Python call, out of place: the same values
    # through the sampler: a U-Net has no scaled label, its engine's time scale is put to 1
    from pnpflow_amd.image_generation import sampling as S, sde_lib as D
    assert hip.pf_engine_set_solver_time_scale(m.handle, 999.0) == 0
    fn = S.get_rectified_flow_sampler(D.RectifiedFlow(use_ode_sampler="euler", sigma_var=0.3, sample_N=2), shape, lambda v: v)
    xs, nfe = fn(m, z=z.cuda(), noise=nz)
    assert nfe == 2 and torch.equal(xs.cpu(), x)


# ---- 5. RK45 -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["c", "d"])
def test_rk45_matches_scipy_fixture(hip, gold, case):
    """c: z -> data, t 1e-3 -> 1 (rk45_sampler); d: data -> latent, t 1 -> 1e-3 (sde.ode(reverse=True)); rtol = atol = 1e-5, B = 2.
    The real fp32 SciPy runs: c 43 attempts, 260 evaluations, distance to the fp64 1e-9 solution 1.60e-3, |ref32 - ref64| 2.31e-3 (bound 7.03e-3);
    d 57 attempts, 344 evaluations, 2.70e-3, 2.73e-3 (bound 9.51e-3).
    Measured on an MI355X (precision mode 1 / 0): c 33 accepted + 15 rejected, 290 evaluations / 32 + 11, 260; distance to the 1e-9 solution
    1.73e-3 / 1.69e-3; |hip - ref32| 1.9e-3 / 1.1e-4.  d 24 + 28, 314 / 24 + 26, 302; 2.43e-3 / 2.52e-3; |hip - ref32| 2.3e-3 / 2.6e-3.
    (This velocity field - synthetic weights, the output divided by the label - makes SciPy itself reject a quarter to a half of its attempts;
    the accepted / rejected split moves with the last bits of the velocity, the distance to the tight solution does not.)"""
    m, _f = ncsnpp()
    x0 = det_normal(SHAPE, int(gold["z_seed"])) if case == "c" else det_image(SHAPE, int(gold["x_seed"]))
    t0, t1 = (1e-3, 1.0) if case == "c" else (1.0, 1e-3)
    tight = gold[case + "_tight_x"]
    d_ref = float(np.abs(gold[case + "_ref32_x"].astype(np.float64) - tight).max())
    bound = 1.5 * d_ref + 2 * float(gold[case + "_gap"])
    for mode in (1, 0):
        m.set_precision(mode)
        try:
            x, st = m.ode_rk45(x0.cuda(), t0, t1, 1e-5, 1e-5)
            m.check_numerics()
        finally:
            m.set_precision(1)
        d_hip = float(np.abs(x.cpu().double().numpy() - tight).max())
        print(f"ode_rk45 tiny case {case} mode={mode}: {st}, d_hip {d_hip:.4g}, d_ref32 {d_ref:.4g}, bound {bound:.4g}, "
              f"|hip - ref32| {float(np.abs(x.cpu().numpy() - gold[case + '_ref32_x']).max()):.4g} (real SciPy run: {int(gold[case + '_ref32_nfev'])} evaluations)")
        assert st["nfev"] == 2 + 6 * (st["accepted"] + st["rejected"]) and st["accepted"] >= 1
        assert d_hip <= bound, (d_hip, bound)


# ---- 6. device-side refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hip):
    import pnpflow_amd._lib as L
    m, _f = ncsnpp()
    z = det_normal(SHAPE, 61).cuda()
    out = torch.full(SHAPE, 7.0, device="cuda")
    stats = (C.c_int64 * 3)(7, 7, 7)

    def euler(**kw):
        p = L.PfRfSamplerParams()
        p.t_begin, p.t_end, p.n_steps, p.sigma_var, p.noise_scale = 1e-3, 1.0, 2, 0.0, 1.0
        for k, v in kw.items():
            setattr(p, k, v)
        return hip.pf_rf_euler_sampler(m.handle, C.byref(p), z.data_ptr(), None, out.data_ptr(), 2, L.current_stream_ptr())

    def rk45(**kw):
        p = L.PfRk45Params()
        p.t0, p.t1, p.rtol, p.atol, p.max_attempts = 1e-3, 1.0, 1e-5, 1e-5, 1000
        for k, v in kw.items():
            setattr(p, k, v)
        return hip.pf_flow_ode_rk45(m.handle, C.byref(p), z.data_ptr(), out.data_ptr(), stats, 2, L.current_stream_ptr())

    for bad in (dict(n_steps=0), dict(sigma_var=-0.5), dict(noise_scale=0.0), dict(noise_scale=-1.0), dict(t_end=1e-3), dict(t_begin=float("inf")),
                dict(t_end=float("nan")), dict(sigma_var=0.5, t_begin=1.0, t_end=0.5)):
        assert euler(**bad) == -1, bad
        assert b"rf_euler_sampler" in hip.pf_last_error(m.handle)
    for bad in (dict(rtol=0.0), dict(atol=0.0), dict(rtol=-1.0), dict(t1=1e-3), dict(t0=float("nan")), dict(max_attempts=0)):
        assert rk45(**bad) == -1, bad
        assert b"flow_ode_rk45" in hip.pf_last_error(m.handle)
    p = L.PfRfSamplerParams(); p.t_begin, p.t_end, p.n_steps, p.noise_scale = 1e-3, 1.0, 2, 1.0
    assert hip.pf_rf_euler_sampler(m.handle, C.byref(p), z.data_ptr(), None, None, 2, L.current_stream_ptr()) == -1
    assert hip.pf_rf_euler_sampler(m.handle, C.byref(p), z.data_ptr(), None, out.data_ptr(), 0, L.current_stream_ptr()) == -1
    assert hip.pf_rf_euler_sampler(m.handle, None, z.data_ptr(), None, out.data_ptr(), 2, L.current_stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and list(stats) == [7, 7, 7]
    # the Python layer refuses what it can see; an attempt cap fails loudly and leaves the engine usable
    with pytest.raises(ValueError, match="noise of shape"):
        m.rf_euler(z, 2, sigma_var=0.5, noise=torch.zeros((3,) + SHAPE, device="cuda"))
    with pytest.raises(L.PnpFlowHipError, match="n_steps"):
        m.rf_euler(z, 0)
    with pytest.raises(L.PnpFlowHipError, match="max_attempts attempts"):
        m.ode_rk45(z, 1e-3, 1.0, 1e-5, 1e-5, max_attempts=2)
    assert torch.isfinite(m.rf_euler(z, 1)).all()


# ---- 7. through the top -----------------------------------------------------------------------------------------------------------------------------
def test_samplers_through_the_reference_surface(hip, gold):
    from pnpflow_amd.image_generation import sampling as S, sde_lib as D
    m, _f = ncsnpp()
    z = det_normal(SHAPE, int(gold["z_seed"])).cuda()
    scaler = lambda x: (x + 1.) / 2.
    sde = D.RectifiedFlow(use_ode_sampler="euler", sample_N=4)
    x, nfe = S.get_rectified_flow_sampler(sde, SHAPE, scaler)(m, z=z)
    assert nfe == 4 and torch.equal(x, scaler(m.rf_euler(z, 4)))
    np.testing.assert_allclose(x.cpu().numpy(), (gold["a_x"] + 1) / 2, rtol=0, atol=5 * NX_RTOL * euler_reference(4, z.cpu())[1])
    sde = D.RectifiedFlow(use_ode_sampler="rk45", ode_tol=1e-3)
    fn = S.get_rectified_flow_sampler(sde, SHAPE, scaler)
    x, nfe = fn(m, z=z)
    ref, st = m.ode_rk45(z, 1e-3, 1.0, 1e-3, 1e-3)
    assert nfe == st["nfev"] == fn.last_stats["nfev"] and torch.equal(x, scaler(ref))
    drawn, _ = fn(m)          # get_z0's latent
    assert drawn.shape == SHAPE and torch.isfinite(drawn).all() and drawn.is_cuda
    assert torch.equal(D.RectifiedFlow().euler_ode(z, m, N=3), m.rf_euler(z, 3))
    np.testing.assert_allclose(D.RectifiedFlow().euler_ode(z, m, N=3).cpu().numpy(), gold["e_x"], rtol=0, atol=5 * NX_RTOL * euler_reference(4, z.cpu())[1])


def test_compute_metric_with_a_prior_sampler(hip, tmp_path):
    """ComputeMetric on the tiny NCSN++ net: 50 Euler samples (N = 2) against 50 synthetic images at 64 Inception features, synthetic Inception
    weights unless the published file is installed.  The FID it writes is the FID of the same samples computed directly."""
    import types
    from main import SyntheticLoader
    from pnpflow_amd import compute_metric as CM, fid_score as fs
    from pnpflow_amd.image_generation import sampling as S, sde_lib as D
    from pnpflow_amd.models import InceptionV3, load_fid_inception
    m, _f = ncsnpp()
    incep, _real = load_fid_inception([InceptionV3.BLOCK_INDEX_BY_DIM[64]], synthetic=True)
    sde = D.RectifiedFlow(use_ode_sampler="euler", sample_N=2)
    ps = S.PriorSampler(m, sde, (1, 3, 32, 32))
    args = types.SimpleNamespace(output_root=str(tmp_path) + "/", dataset="celebahq", fid_dims=64, synthetic=True, device_index=0)
    loaders = {"test": SyntheticLoader(50, 3, 32, 1)}
    torch.manual_seed(17)
    fid = CM.ComputeMetric(loaders, ps, torch.device("cuda"), args, incep_model=incep, results_dir="results_synthetic").compute_metrics(50)
    line = (tmp_path / "results_synthetic" / "celebahq" / "metrics.txt").read_text().strip()
    assert np.isfinite(fid) and line == f"Epoch: final, FID: {fid}"
    # the same samples, drawn here: 50 rounds of one get_z0 draw each, injected as z
    torch.manual_seed(17)
    zs = torch.cat([sde.get_z0(torch.zeros(1, 3, 32, 32)) for _ in range(CM.N_ITER)]).cuda()
    samples = ps.generate_samples(50, batch_size=1, latent=zs)
    gt = next(iter(loaders["test"]))[0]
    m1, s1 = fs.calculate_activation_statistics(CM.three_channels(gt.permute(0, 2, 3, 1).numpy()), incep, 50, 64, "cuda")
    m2, s2 = fs.calculate_activation_statistics(CM.three_channels(torch.clip(samples.permute(0, 2, 3, 1), 0, 1).cpu().numpy()), incep, 50, 64, "cuda")
    direct = fs.calculate_frechet_distance(m1, s1, m2, s2)
    print(f"FID of 50 tiny-net Euler samples at 64 features: {fid} (direct {direct})")
    assert fid == direct
