"""The prior's evaluation on the engine - Rademacher fill, Hutchinson divergence, fixed-grid Euler sampling, the RK45 likelihood solve -
against the oracle (fp32 and fp64) and the SciPy-integrated fixture tests/golden/prior_eval_tiny4.npz (tools/make_golden_prior_eval.py).
Needs a real MI355X:  python -m pytest tests -m gpu

Tolerances:
  Rademacher fill      bit-exact
  divergence           VJP_RTOL sqrt(n) max|g64| per image sum of n products, each factor within the project's VJP tolerance (5e-5 of
                       max|J^T eps|) under independent per-element errors; reference: eps . unet_vjp in fp64
  velocity             FWD_ATOL
  Euler, 10 points     5 x FWD_ATOL (the bound test_forward_map_matches_oracle uses for ten chained evaluations)
  likelihood           distance to the fp64 rtol = atol = 1e-9 solution at most 1.5 x the fp32-oracle SciPy run's, plus twice the stored
                       |ref32 - ref64| gap (fp32-equivalent arithmetic in another summation order)
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import CFGS, det_image, det_normal
from oracle import pnpflow_oracle as O

pytestmark = pytest.mark.gpu

FWD_ATOL = 2e-5
VJP_RTOL = 5e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EPS_SEED, EPS_STREAM, IMAGE_SEED = 5, 7, 41          # tools/make_golden_prior_eval.py

_MODELS, _REFS = {}, {}


def model_for(name):
    from pnpflow_amd.models import UNet
    if name not in _MODELS:
        c = CFGS[name]
        cfg = O.unet_config(**c)
        sd = O.synthetic_state_dict(cfg, 0)
        m = UNet(c["input_channels"], c["input_height"], c["ch"], ch_mult=c["ch_mult"], num_res_blocks=c["num_res_blocks"],
                 attn_resolutions=c["attn_resolutions"])
        m.load_state_dict(sd)
        _MODELS[name] = (m, cfg, sd)
    return _MODELS[name]


def rademacher(n, seed, stream, offset=0):
    """numpy restatement of pf_fill_rademacher: element e is word e % 4 of Philox counter (e/4 lo, e/4 hi, stream lo, stream hi) under key
    (seed lo, seed hi); +1 when the word's top bit is set, else -1."""
    q_lo = offset // 4
    qs = np.arange(q_lo, (offset + n + 3) // 4, dtype=np.uint64)
    ctr = np.zeros((qs.size, 4), dtype=np.uint32)
    ctr[:, 0] = (qs & np.uint64(0xFFFFFFFF)).astype(np.uint32); ctr[:, 1] = (qs >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = np.uint32(stream & 0xFFFFFFFF); ctr[:, 3] = np.uint32((stream >> 32) & 0xFFFFFFFF)
    r = O.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32))
    return np.where(r.reshape(-1)[offset - 4 * q_lo:offset - 4 * q_lo + n] >> np.uint32(31), 1.0, -1.0).astype(np.float32)


def probe(shape, seed=EPS_SEED, stream=EPS_STREAM):
    return torch.from_numpy(rademacher(int(np.prod(shape)), seed, stream)).view(shape)


@pytest.fixture(scope="module")
def hip():
    import pnpflow_amd._lib as L
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return L.load()


# ---- 1. Rademacher fill ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,offset", [(1, 0), (5, 0), (4096, 0), (70001, 0), (1000, 3), (777, 4 * 1234 + 2), (2, 1), (1031, 2 ** 34 + 5)])
def test_rademacher_fill_is_bit_exact(hip, n, offset):
    import pnpflow_amd._lib as L
    seed, stream = 0x1234567890ABCDEF, 0xFEDCBA9876543210
    buf = torch.full((n + 16,), 7.0, device="cuda")
    L.check(hip.pf_fill_rademacher(buf.data_ptr() + 32, n, seed, stream, offset, L.current_stream_ptr()), None, "pf_fill_rademacher")
    got = buf.cpu().numpy()
    assert (got[:8] == 7.0).all() and (got[8 + n:] == 7.0).all(), "the fill wrote outside [0, n)"
    want = rademacher(n, seed, stream, offset)
    assert np.array_equal(got[8:8 + n].view(np.uint32), want.view(np.uint32))
    if n >= 4096:
        assert abs(float(want.mean())) < 0.05          # the restatement itself draws both signs


def test_device_draw_and_hut_estimator_draws(hip):
    from pnpflow_amd import utils
    m, cfg, sd = model_for("tiny4")
    x = det_image((2, 3, 64, 64), 43).cuda()
    e = utils.device_draw("rademacher", (2, 3, 64, 64), "cuda", seed=EPS_SEED, stream_id=EPS_STREAM)
    assert torch.equal(e.cpu(), probe((2, 3, 64, 64)))
    gn = utils.device_draw("gaussian", (1000,), "cuda", seed=3, stream_id=4).cpu().numpy()
    np.testing.assert_allclose(gn, O.engine_normal(1000, 3, 4), rtol=0, atol=2e-5)
    torch.manual_seed(11)
    utils._device_draws = 0
    got = utils.hut_estimator(2, m, x, 0.5)
    draws = [utils.device_draw("rademacher", x.shape, "cuda", seed=11, stream_id=i) for i in range(2)]
    want = sum(m.divergence(x, torch.full((2,), 0.5), d) for d in draws) / 2
    assert got.shape == (2,) and got.dtype == torch.float32 and torch.equal(got, want.float())
    assert utils._device_draws == 2


# ---- 2. divergence -----------------------------------------------------------------------------------------------------------------------
def divergence_reference(net, B):
    """(x, t, eps, v64, g64, div64) with the oracle in fp64, computed once per (net, B)."""
    if (net, B) not in _REFS:
        m, cfg, sd = model_for(net)
        c = CFGS[net]
        shape = (B, c["input_channels"], c["input_height"], c["input_height"])
        x = det_image(shape, IMAGE_SEED + B)
        t = torch.tensor([1.0, 0.5, 1e-5][:B])
        eps = probe(shape)
        sd64 = {k: v.double() for k, v in sd.items()}
        emb = O.sinusoidal_embedding
        O.sinusoidal_embedding = lambda tt, dim: emb(tt, dim).double()
        try:
            xx = x.double().requires_grad_(True)
            with torch.enable_grad():
                v64 = O.unet_forward(sd64, cfg, xx, t.double())
                (g64,) = torch.autograd.grad(v64, xx, grad_outputs=eps.double())
        finally:
            O.sinusoidal_embedding = emb
        _REFS[(net, B)] = (x, t, eps, v64.detach(), g64, (g64 * eps.double()).sum(dim=(1, 2, 3)))
    return _REFS[(net, B)]


@pytest.mark.parametrize("net,B", [("tiny4", 2), ("tiny4", 3), ("gray40", 1)])
@pytest.mark.parametrize("mode", [0, 1])
def test_divergence_matches_fp64_oracle(hip, net, B, mode):
    """Measured on an MI355X, max over the images of |div - div64| against the bound, precision mode 0 / 1:
    tiny4 B = 2: 1.5e-3 / 6.3e-4 of 0.146 (div64 -1216.7, -193.6); tiny4 B = 3: 3.4e-3 / 3.5e-3 of 0.213; gray40 B = 1: 2.4e-3 / 4.3e-4 of
    0.104.  max|v - v64| <= 1.1e-5."""
    m, cfg, sd = model_for(net)
    x, t, eps, v64, g64, div64 = divergence_reference(net, B)
    m.set_precision(mode)
    try:
        div, v = m.divergence(x.cuda(), t.cuda(), eps.cuda(), return_velocity=True)
        div2 = m.divergence(x.cuda(), t.cuda(), eps.cuda())
        gb = m.backward(eps.cuda()).cpu()          # afterwards the retained forward is that of (x, t)
        m.check_numerics()
    finally:
        m.set_precision(1)
    n = x[0].numel()
    bound = VJP_RTOL * np.sqrt(n) * float(g64.abs().max())
    err = (div.cpu() - div64).abs()
    print(f"divergence {net} B={B} mode={mode}: div64 {div64.numpy()}, |div - div64| {err.numpy()}, bound {bound:.4g}, "
          f"max|v - v64| {float((v.cpu().double() - v64).abs().max()):.3g}")
    assert div.dtype == torch.float64 and div.shape == (B,)
    assert torch.equal(div, div2), "two evaluations of one input differ: the reduction is not deterministic"
    assert float(err.max()) <= bound, (err, bound)
    np.testing.assert_allclose(v.cpu().numpy(), v64.float().numpy(), atol=FWD_ATOL)
    np.testing.assert_allclose(gb.numpy(), g64.float().numpy(), atol=VJP_RTOL * float(g64.abs().max()))


def test_divergence_ncsnpp_matches_oracle(hip):
    """The NCSN++ net at t = 0.5 under the solver time scale 999: the net sees 499.5.  Measured on an MI355X: |div - ref| <= 9.6e-7 on
    (0.470, 0.730), bound 1.2e-4; the likelihood solve to eps = 0.1 takes 22 accepted + 9 rejected steps, 188 evaluations, bpd (8.395, 8.374)."""
    from oracle import ncsnpp_oracle as NO
    from pnpflow_amd.image_generation.models.ncsnpp import NCSNpp
    from test_gpu_ncsnpp import CFGS as NCFGS, ref_config
    c = NCFGS["tiny"]; cfg = NO.ncsnpp_config(**c); sd = NO.synthetic_state_dict(cfg, 0)
    m = NCSNpp(ref_config(c)); m.load_state_dict(sd)         # an engine of its own: the solver time scale stays out of other tests
    m.set_solver_time_scale(999.0)
    S = c["image_size"]
    x = det_image((2, 3, S, S), IMAGE_SEED); eps = probe((2, 3, S, S)); t = torch.full((2,), 0.5)
    div, v = m.divergence(x.cuda(), t.cuda(), eps.cuda(), return_velocity=True)
    m.check_numerics()
    g = NO.ncsnpp_vjp(sd, cfg, x, t * 999, eps)
    ref = (g.double() * eps.double()).sum(dim=(1, 2, 3))
    bound = VJP_RTOL * np.sqrt(x[0].numel()) * float(g.abs().max())
    print(f"divergence ncsnpp tiny: ref {ref.numpy()}, |div - ref| {(div.cpu() - ref).abs().numpy()}, bound {bound:.4g}")
    assert float((div.cpu() - ref).abs().max()) <= bound
    vref = NO.ncsnpp_forward(sd, cfg, x, t * 999)
    assert float((v.cpu() - vref).abs().max()) <= 5e-5 * float(vref.abs().max())
    # the likelihood solve on this net: it divides by its label, so the solve ends at eps = 0.1; finite, and the evaluation count identity
    from pnpflow_amd.image_generation.likelihood import get_likelihood_fn_rf
    fn = get_likelihood_fn_rf(eps=0.1)
    bpd, z, nfe = fn(m, x.cuda(), epsilon=eps.cuda())
    st = fn.last_stats
    print(f"likelihood ncsnpp tiny: bpd {bpd.cpu().numpy()}, {st}")
    assert torch.isfinite(bpd).all() and torch.isfinite(z).all() and torch.isfinite(fn.last_delta_logp).all()
    assert nfe == st["nfev"] == 2 + 6 * (st["accepted"] + st["rejected"]) and st["accepted"] >= 1


# ---- 3. sampling -------------------------------------------------------------------------------------------------------------------------
def flow_matching(m):
    from pnpflow_amd.train_flow_matching import FLOW_MATCHING
    from pnpflow_amd.utils import CfgNode
    return FLOW_MATCHING(m, torch.device("cuda"), CfgNode(dict(dim_image=m.input_height, num_channels=m.input_channels, model="ot")))


def test_euler_sampling_matches_oracle_loop(hip):
    m, cfg, sd = model_for("tiny4")
    z = det_normal((3, 3, 64, 64), 91)
    out = flow_matching(m).generate_samples("euler", n_samples=3, batch_size=2, integration_steps=10, latent=z.cuda()).cpu()
    m.check_numerics()
    grid = torch.linspace(0, 1, 10)
    x = z.clone()
    for i in range(9):
        x = x + (grid[i + 1] - grid[i]) * O.unet_forward(sd, cfg, x, grid[i].repeat(3))
    print(f"euler tiny4: max|hip - oracle| {float((out - x).abs().max()):.3g}")
    np.testing.assert_allclose(out.numpy(), x.numpy(), atol=5 * FWD_ATOL)
    assert float((out - z).abs().max()) > 0.1          # the sampler moved the latent
    # drawn latents: finite samples of the right shape
    drawn = flow_matching(m).generate_samples("euler", n_samples=2, integration_steps=3)
    assert drawn.shape == (2, 3, 64, 64) and torch.isfinite(drawn).all()


def test_apply_flow_matching_is_the_dopri5_solve(hip):
    import pnpflow_amd._lib as L
    m, cfg, sd = model_for("tiny4")
    z = det_normal((2, 3, 64, 64), 92).cuda()
    fm = flow_matching(m)
    out = fm.apply_flow_matching(2, latent=z)
    prm = L.PfDopri5Params()
    prm.t0, prm.t1, prm.rtol, prm.atol, prm.max_steps = 0.0, 1.0, 1e-5, 1e-5, 1000
    ref = torch.empty_like(z); stats = (C.c_int64 * 3)()
    with L.solver_stream():
        L.check(hip.pf_flow_ode_dopri5(m.handle, C.byref(prm), z.data_ptr(), ref.data_ptr(), 2, stats, L.current_stream_ptr()), m.handle, "pf_flow_ode_dopri5")
    assert torch.equal(out, ref) and torch.isfinite(out).all()
    assert fm.last_dopri5_stats == dict(accepted=int(stats[0]), rejected=int(stats[1]), nfev=int(stats[2])) and stats[0] >= 1
    g = fm.generate_samples("dopri5", tol=1e-5, n_samples=2, integration_steps=100, latent=z)
    assert torch.equal(g, ref)


# ---- 4. likelihood -----------------------------------------------------------------------------------------------------------------------
def test_likelihood_matches_scipy_fixture(hip):
    """State (x, logp) from t = 1 to 1e-5 at rtol = atol = 1e-5 on det_image((2, 3, 64, 64), 41), eps by recipe (seed 5, stream 7).
    SciPy on the fp32 oracle: 9 attempts, 56 evaluations, delta_logp (580.1225, 455.6756), bpd (8.551884, 8.548475); its distance to the
    fp64 1e-9 solution: 1.06e-3 in z, 1.75e-2 in delta_logp, 1.52e-5 in bpd; |ref32 - ref64|: 5.5e-5, 2.2e-3, 2.9e-7.
    Measured on an MI355X (precision mode 1 / 0): 9 accepted, 0 rejected, 56 evaluations in both; delta_logp (580.1260, 455.6740) /
    (580.1231, 455.6791); bpd (8.551883, 8.548475) / (8.551884, 8.548474); distance to the 1e-9 solution 1.10e-3 / 1.17e-3 in z (bound
    1.70e-3), 1.40e-2 / 1.69e-2 in delta_logp (bound 3.08e-2), 1.44e-5 / 1.53e-5 in bpd (bound 2.34e-5); |hip - ref32| 1.1e-4 / 3.2e-4 in z,
    3.5e-3 in delta_logp, 8.3e-7 / 1.0e-6 in bpd."""
    g = np.load(os.path.join(GOLD, "prior_eval_tiny4.npz"))
    m, cfg, sd = model_for("tiny4")
    x = det_image((2, 3, 64, 64), IMAGE_SEED).cuda()
    eps = probe((2, 3, 64, 64)).cuda()
    for mode in (1, 0):
        m.set_precision(mode)
        try:
            z, dlp, bpd, st = m.likelihood_ode(x, eps, t0=float(g["t0"]), t1=float(g["t1"]), rtol=float(g["rtol"]), atol=float(g["atol"]),
                                               offset=float(g["offset"]))
        finally:
            m.set_precision(1)
        got = {"z": z.cpu().double().numpy(), "delta_logp": dlp.cpu().numpy(), "bpd": bpd.cpu().double().numpy()}
        attempts = st["accepted"] + st["rejected"]
        lines = [f"likelihood tiny4 mode={mode}: {st}, delta_logp {got['delta_logp']}, bpd {got['bpd']}"]
        checks = []
        for q in ("z", "delta_logp", "bpd"):
            tight = g["tight_" + q].astype(np.float64)
            d_hip = float(np.abs(got[q] - tight).max()); d_ref = float(np.abs(g["ref32_" + q].astype(np.float64) - tight).max())
            floor = 2 * float(g["gap_" + q])
            lines.append(f"  {q}: d_hip {d_hip:.4g}, d_ref32 {d_ref:.4g}, floor {floor:.3g}, |hip - ref32| {float(np.abs(got[q] - g['ref32_' + q]).max()):.4g}")
            checks.append((q, d_hip, 1.5 * d_ref + floor))
        print("\n".join(lines))
        assert st["nfev"] == 2 + 6 * attempts
        assert abs(attempts - int(g["ref32_attempts"])) <= 1, (st, int(g["ref32_attempts"]))
        for q, d_hip, bound in checks:
            assert d_hip <= bound, (q, d_hip, bound)


def test_likelihood_fn_matches_the_c_call(hip):
    from pnpflow_amd.image_generation.likelihood import get_likelihood_fn_rf
    m, cfg, sd = model_for("tiny4")
    x = det_image((3, 3, 64, 64), IMAGE_SEED + 1).cuda()
    eps = probe((3, 3, 64, 64), stream=9).cuda()
    fn = get_likelihood_fn_rf()
    bpd, z, nfe = fn(m, x, epsilon=eps)
    z2, dlp2, bpd2, st2 = m.likelihood_ode(x, eps, t0=1.0, t1=1e-5, rtol=1e-5, atol=1e-5, offset=7.0)
    assert torch.equal(bpd, bpd2) and torch.equal(z, z2) and torch.equal(fn.last_delta_logp, dlp2) and nfe == st2["nfev"] == fn.last_stats["nfev"]
    assert bpd.shape == (3,) and torch.isfinite(bpd).all() and z.shape == x.shape
    # bits/dim is the documented function of (z, delta_logp)
    N = x[0].numel()
    prior = -N / 2.0 * np.log(2 * np.pi) - 0.5 * (z.double() ** 2).sum(dim=(1, 2, 3))
    want = -(prior + dlp2) / (N * np.log(2.0)) + 7.0
    np.testing.assert_allclose(bpd.cpu().double().numpy(), want.cpu().numpy(), rtol=0, atol=1e-6)
    # offset follows the inverse scaler; the probe is drawn on the device when none is given
    fn8 = get_likelihood_fn_rf(inverse_scaler=lambda v: v)
    bpd8, _, _ = fn8(m, x, epsilon=eps)
    np.testing.assert_allclose((bpd8 - bpd).cpu().numpy(), 1.0, atol=1e-6)
    bpd_drawn, _, nfe_drawn = get_likelihood_fn_rf(hutchinson_type="Gaussian")(m, x)
    assert torch.isfinite(bpd_drawn).all() and (nfe_drawn - 2) % 6 == 0
    m.check_numerics()


def test_loud_errors(hip):
    import pnpflow_amd._lib as L
    from pnpflow_amd.models import UNet
    m, cfg, sd = model_for("tiny4")
    x = det_image((2, 3, 64, 64), IMAGE_SEED).cuda(); eps = probe((2, 3, 64, 64)).cuda()
    with pytest.raises(L.PnpFlowHipError, match="max_attempts"):
        m.likelihood_ode(x, eps, max_attempts=1)
    with pytest.raises(L.PnpFlowHipError, match="rtol"):
        m.likelihood_ode(x, eps, rtol=0.0)
    with pytest.raises(L.PnpFlowHipError, match="t0 != t1"):
        m.likelihood_ode(x, eps, t0=0.5, t1=0.5)
    with pytest.raises(ValueError, match="eps of shape"):
        m.divergence(x, torch.full((2,), 0.5), eps[:1])
    with pytest.raises(ValueError, match="entries for a batch"):
        m.divergence(x, torch.full((3,), 0.5), eps)
    with pytest.raises(L.PnpFlowHipError, match="GPU tensors"):
        m.divergence(x.cpu(), torch.full((2,), 0.5), eps.cpu())
    with pytest.raises(ValueError, match="at least 2"):
        m.euler(x, torch.tensor([0.0]))
    c = CFGS["tiny4"]
    raw = UNet(c["input_channels"], c["input_height"], c["ch"], ch_mult=c["ch_mult"], num_res_blocks=c["num_res_blocks"],
               attn_resolutions=c["attn_resolutions"])          # weights never loaded / finalised
    for call in (lambda: raw.divergence(x, torch.full((2,), 0.5), eps), lambda: raw.euler(x, torch.linspace(0, 1, 3)), lambda: raw.likelihood_ode(x, eps)):
        with pytest.raises(L.PnpFlowHipError, match="not finalized"):
            call()
    # a failed solve leaves the engine usable
    assert torch.isfinite(m.divergence(x, torch.full((2,), 0.5), eps)).all()


def test_prior_report_tool(hip, tmp_path):
    """`python tools/prior_report.py --opts ... synthetic True` in a child process writes the sample grid and the bits/dim table."""
    cmd = [sys.executable, os.path.join(ROOT, "tools", "prior_report.py"), "--opts", "dataset", "celeba", "model", "ot", "synthetic", "True",
           "n_samples", "2", "integration_method", "euler", "integration_steps", "3", "n_images", "1", "batch_size_ip", "2", "output_root", str(tmp_path) + "/"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    base = tmp_path / "results_synthetic" / "celeba" / "ot" / "prior_report"
    assert (base / "samples.png").stat().st_size > 1000
    rows = [l.split() for l in (base / "bits_per_dim.txt").read_text().splitlines() if not l.startswith("#")]
    assert len(rows) == 1 and np.isfinite(float(rows[0][1])) and np.isfinite(float(rows[0][2])), rows
