"""Prox-PnP with the gradient-step denoiser (pnpflow/methods/pnp_gs.py, pnpflow/train_denoiser.py) on the engine, against the oracle, the
CPU restatement (tests/pnp_gs_restatement.py) and goldens of the REAL reference (tests/golden/pnp_gs_tiny4_*.npz,
tools/make_golden_pnp_gs.py).  Needs a real MI355X:  python -m pytest tests -m gpu

Tolerance, from the project's own constants (tests/test_gpu_parity.py): FWD_ATOL = 2e-5 on a forward, VJP_RTOL = 5e-5 of max|J^T v| on a VJP.
    TOL(ref) = FWD_ATOL + 2 * VJP_RTOL * max|J^T (x - N)|_ref
one forward error plus one VJP error, doubled because the VJP's seed x - N carries the forward's error.  Every iteration form maps
(z, N, J^T r) to its output with factors of at most 1 (alpha <= 1, both proxes are non-expansive), so one iteration is held to TOL;
a free-running solve to TOL * growth^(k-1) after iteration k, `growth` being the reference's own fp32-vs-fp64 amplification per iteration
stored in the golden.  g = 0.5 sum (x - N)^2: 1e-5 relative.
The teacher-forced tests print `PNP_GS_RATIO <case> <k> <mode> <max|err| / TOL>` (tools/gpu_pnp_gs_time.py collects the largest).
"""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import CFGS, det_image, det_normal
from oracle import pnpflow_oracle as O
import pnp_gs_restatement as R

pytestmark = pytest.mark.gpu

FWD_ATOL = 2e-5
VJP_RTOL = 5e-5
G_RTOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLEAN_SEED, GRAD_SEED = 33, 77          # tools/make_golden_pnp_gs.py
MAX_ITER, ALPHA = 3, 0.5
CASES = {"pgd_denoising": ("pgd", "denoising", "gaussian"),
         "pgd_inpainting": ("pgd", "inpainting", "gaussian"),
         "pgd_superresolution": ("pgd", "superresolution", "gaussian"),
         "pgd_gaussian_deblurring_FFT": ("pgd", "gaussian_deblurring_FFT", "gaussian"),
         "pgd_laplace_denoising": ("pgd", "denoising", "laplace"),
         "pgd_laplace_inpainting": ("pgd", "inpainting", "laplace"),
         "hqs_random_inpainting": ("hqs", "random_inpainting", "gaussian"),
         "hqs_gaussian_deblurring_FFT": ("hqs", "gaussian_deblurring_FFT", "gaussian")}


def TOL(jn_max):
    return FWD_ATOL + 2 * VJP_RTOL * float(jn_max)


_MODELS = {}


def new_model(name):
    from pnpflow_amd.models import UNet
    c = CFGS[name]
    cfg = O.unet_config(**c)
    sd = O.synthetic_state_dict(cfg, 0)
    m = UNet(c["input_channels"], c["input_height"], c["ch"], ch_mult=c["ch_mult"], num_res_blocks=c["num_res_blocks"],
             attn_resolutions=c["attn_resolutions"])
    m.load_state_dict(sd)
    return m, cfg, sd


def model_for(name):
    if name not in _MODELS:
        _MODELS[name] = new_model(name)
    return _MODELS[name]


def oracle_net(name):
    _, cfg, sd = model_for(name)
    return lambda x, s: O.unet_forward(sd, cfg, x, s)


def solver_for(m, **kw):
    from pnpflow_amd.methods.pnp_gs import PROX_PNP
    from pnpflow_amd.train_denoiser import GRADIENT_STEP_DENOISER
    from pnpflow_amd.utils import CfgNode
    a = dict(method="pnp_gs", model="gradient_step", problem="denoising", noise_type="gaussian", algo="pgd", max_iter=MAX_ITER, lr_pnp=1.0, alpha=ALPHA,
             sigma_factor=1.0, max_batch=1, compute_time=False, compute_memory=False, save_results=False, batch=0, dim_image=m.input_height,
             num_channels=m.input_channels)
    a.update(kw)
    args = CfgNode(a)
    return PROX_PNP(GRADIENT_STEP_DENOISER(m, torch.device("cuda"), args), torch.device("cuda"), args)


def degradations(problem, S, C_=3, ksize=61):
    import pnpflow_amd.degradations as D
    return {"denoising": lambda: (D.Denoising(), O.Denoising()),
            "inpainting": lambda: (D.BoxInpainting(10), O.BoxInpainting(10)),
            "superresolution": lambda: (D.Superresolution(4, S), O.Superresolution(4, S)),
            "gaussian_deblurring_FFT": lambda: (D.GaussianDeblurring(1.0, ksize, "fft", C_, S), O.GaussianDeblurring(1.0, ksize, "fft", C_, S)),
            "random_inpainting": lambda: (D.RandomInpainting(0.7), O.RandomInpainting(0.7))}[problem]()


@pytest.fixture(scope="module")
def hip():
    import pnpflow_amd._lib as L
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return L.load()


_GOLD = {}


def golden(name):
    if name not in _GOLD:
        _GOLD[name] = dict(np.load(os.path.join(GOLD, f"pnp_gs_tiny4_{name}.npz")))
    return _GOLD[name]


class precision:
    def __init__(self, m, mode):
        self.m, self.mode = m, mode

    def __enter__(self):
        self.m.set_precision(self.mode)

    def __exit__(self, *exc):
        self.m.set_precision(1)
        return False


# ---- 5 / 6. calculate_grad ----------------------------------------------------------------------------------------------------
_GRAD_REF = {}


def grad_reference(net_name, B):
    """(x, sigma, Dg, N, g, JN) of the oracle, computed once per net."""
    if net_name not in _GRAD_REF:
        c = CFGS[net_name]
        shape = (B, c["input_channels"], c["input_height"], c["input_height"])
        x = det_image(shape, 91) + 0.1 * det_normal(shape, 92)
        sigma = torch.tensor([0.02, 0.6, 0.3][:B])
        Dg, N, g, JN = R.calculate_grad(oracle_net(net_name), x, sigma)
        # a kernel that broadcasts sigma[0] is far outside the bound (CPU oracle: 34 x, 34 x, 63 x TOL on the three nets)
        N0 = oracle_net(net_name)(x, sigma[:1].expand(B))
        assert float((N0 - N).abs().max()) > 10 * TOL(JN.abs().max())
        _GRAD_REF[net_name] = (x, sigma, Dg, N, g, JN)
    return _GRAD_REF[net_name]


@pytest.mark.parametrize("net,B", [("tiny4", 2), ("odd48", 2), ("mnist", 3)])
@pytest.mark.parametrize("mode", [0, 1])
def test_calculate_grad_matches_oracle(hip, net, B, mode):
    m, _, _ = model_for(net)
    x, sigma, Dg, N, g, JN = grad_reference(net, B)
    den = solver_for(m).model
    with precision(m, mode):
        dg, n, gg = den.calculate_grad(x.cuda(), sigma.cuda(), compute_g=True)
        dg2, n2 = den.calculate_grad(x.cuda(), sigma.cuda())
        xh, dgf = den.forward(x.cuda(), sigma.cuda())
    tol = TOL(JN.abs().max())
    print(f"calculate_grad {net} mode {mode}: Dg err/TOL {float((dg.cpu() - Dg).abs().max()) / tol:.3f}  N err/TOL {float((n.cpu() - N).abs().max()) / tol:.3f}"
          f"  g rel {abs(float(gg) - float(g)) / float(g):.2e}")
    np.testing.assert_allclose(dg.cpu().numpy(), Dg.numpy(), atol=tol)
    np.testing.assert_allclose(n.cpu().numpy(), N.numpy(), atol=tol)
    assert abs(float(gg) - float(g)) <= G_RTOL * abs(float(g))
    assert torch.equal(dg, dg2) and torch.equal(n, n2)
    assert torch.equal(dgf, dg) and torch.equal(xh, x.cuda() - dg)


@pytest.mark.parametrize("mode", [0, 1])
def test_calculate_grad_matches_reference_golden(hip, mode):
    g = np.load(os.path.join(GOLD, "pnp_gs_tiny4_calculate_grad.npz"))
    m, _, _ = model_for("tiny4")
    shape = (2, 3, 64, 64)
    x = det_image(shape, GRAD_SEED) + 0.1 * det_normal(shape, GRAD_SEED, 1)
    with precision(m, mode):
        dg, n, gg = solver_for(m).model.calculate_grad(x.cuda(), torch.from_numpy(g["sigma"]).cuda(), compute_g=True)
    jn = x.numpy() - g["N"] - g["Dg"]
    tol = TOL(np.abs(jn).max())
    np.testing.assert_allclose(dg.cpu().numpy(), g["Dg"], atol=tol)
    np.testing.assert_allclose(n.cpu().numpy(), g["N"], atol=tol)
    assert abs(float(gg) - float(g["g"])) <= G_RTOL * abs(float(g["g"]))


# ---- 7. teacher-forced single iterations against the real reference --------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("mode", [0, 1])
def test_teacher_forced_iteration_matches_reference_golden(hip, name, k, mode):
    g = golden(name)
    algo, problem, noise_type = CASES[name]
    m, _, _ = model_for("tiny4")
    dg, _ = degradations(problem, 64)
    sigma = float(g["sigma"])
    s = solver_for(m, algo=algo, problem=problem, noise_type=noise_type)
    if "mask" in g:
        assert np.array_equal(dg.mask(2, 64, 64, "cpu").numpy(), g["mask"])
    x_in = torch.from_numpy(g["iterates"][k]).cuda()
    with precision(m, mode):
        x = s.restore_batch(torch.from_numpy(g["noisy"]).cuda(), dg, sigma, first=k, stop=k + 1, x0=x_in, alpha=float(g["alpha"][k]))
    tol = TOL(g["jn_max"][k])
    err = float(np.abs(x.cpu().numpy() - g["iterates"][k + 1]).max())
    print(f"PNP_GS_RATIO {name} {k} {mode} {err / tol:.4f}")
    assert s.last_alpha == float(g["alpha"][k + 1]), (s.last_alpha, g["alpha"])
    if name == "hqs_gaussian_deblurring_FFT":
        np.testing.assert_allclose(s.last_gap_log[k], g["gap"][k], rtol=1e-2)
    if name == "hqs_random_inpainting" and k == MAX_ITER - 1:
        assert torch.equal(x, x_in)          # the last iteration returns x unchanged
    np.testing.assert_allclose(x.cpu().numpy(), g["iterates"][k + 1], atol=tol)


# ---- 8. free-running solve through the public class ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_solve_ip_matches_reference_golden(hip, name):
    g = golden(name)
    algo, problem, noise_type = CASES[name]
    m, _, _ = model_for("tiny4")
    dg, _ = degradations(problem, 64)
    sigma, growth = float(g["sigma"]), float(g["growth"])
    clean = det_image((2, 3, 64, 64), CLEAN_SEED)
    noisy = torch.from_numpy(g["noisy"]).cuda()
    # the bound of iteration k: one iteration's TOL (the largest of the iterations so far) amplified by the reference's own growth
    bound = lambda k: max(TOL(j) for j in g["jn_max"][:k]) * growth ** (k - 1)
    with precision(m, 0):
        s = solver_for(m, algo=algo, problem=problem, noise_type=noise_type)
        s.measurement_noise = lambda batch, hx: (noisy - hx) / sigma          # reproduces the golden's measurement
        s.solve_ip([(clean, torch.zeros(2))], dg, sigma)
        assert s.args.lr_pnp == sigma ** 2 * 1.0                              # multiplied in place
        final, alpha_final = s.last_restored.cpu().numpy(), s.last_alpha
        mid = []
        for k in (1, 2):
            x = s.restore_batch(noisy, dg, sigma, first=0, stop=k, lr=sigma ** 2, alpha=ALPHA)
            mid.append((x.cpu().numpy(), s.last_alpha))
    for k, (x, a) in zip((1, 2), mid):
        print(f"solve_ip {name} after iteration {k}: err/bound {float(np.abs(x - g['iterates'][k]).max()) / bound(k):.4f}")
        assert a == float(g["alpha"][k]), (k, a, g["alpha"])
        np.testing.assert_allclose(x, g["iterates"][k], atol=bound(k), err_msg=f"after iteration {k}")
    print(f"solve_ip {name} after iteration 3: err/bound {float(np.abs(final - g['iterates'][3]).max()) / bound(3):.4f}")
    assert alpha_final == float(g["alpha"][3]), (alpha_final, g["alpha"])
    np.testing.assert_allclose(final, g["iterates"][3], atol=bound(3), err_msg="final")


# ---- 9. other shapes against the restatement --------------------------------------------------------------------------------------
_SHAPE_REF = {}


def shape_reference(which):
    """Two restatement iterations, computed once: hqs deblurring on odd48 (48 px: the direct-DFT path), pgd inpainting on gray40."""
    if which not in _SHAPE_REF:
        if which == "odd48":
            net, S, Cc, algo, problem, sigma, ks = "odd48", 48, 3, "hqs", "gaussian_deblurring_FFT", 0.05, 25
        else:
            net, S, Cc, algo, problem, sigma, ks = "gray40", 40, 1, "pgd", "inpainting", 0.05, 25
        dg, do = degradations(problem, S, Cc, ks)
        shape = (2, Cc, S, S)
        noisy = do.H(det_image(shape, 93)) + sigma * det_normal(shape, 94)
        kw = dict(algo=algo, problem=problem, max_iter=2, sigma_noise=sigma)
        xs, alphas, infos = R.solve(oracle_net(net), do, noisy, alpha=ALPHA, **kw)
        if which == "odd48":      # the decisions of the comparison must not hang on rounding
            assert all(abs(i["gap"] - i["thr"]) >= 0.01 * max(abs(i["gap"]), abs(i["thr"])) for i in infos)
        _SHAPE_REF[which] = (net, dg, do, noisy, sigma, kw, xs, alphas, infos)
    return _SHAPE_REF[which]


@pytest.mark.parametrize("which", ["odd48", "gray40"])
@pytest.mark.parametrize("mode", [0, 1])
def test_other_shapes_match_restatement(hip, which, mode):
    net, dg, do, noisy, sigma, kw, xs, alphas, infos = shape_reference(which)
    m, _, _ = model_for(net)
    s = solver_for(m, algo=kw["algo"], problem=kw["problem"], max_iter=2)
    for k in range(2):
        with precision(m, mode):
            x = s.restore_batch(noisy.cuda(), dg, sigma, first=k, stop=k + 1, x0=xs[k].cuda(), alpha=alphas[k])
        tol = TOL(infos[k]["JN"].abs().max())
        print(f"{which} mode {mode} iteration {k}: err/TOL {float((x.cpu() - xs[k + 1]).abs().max()) / tol:.4f}")
        assert s.last_alpha == alphas[k + 1]
        np.testing.assert_allclose(x.cpu().numpy(), xs[k + 1].numpy(), atol=tol)


def test_alpha_carries_over_to_the_next_batch(hip):
    """Two consecutive batches in one solve_ip: the second starts from the alpha the first one's backtracking left (pnp_gs.py:96)."""
    net, dg, do, noisy, sigma, kw, xs, alphas, infos = shape_reference("odd48")
    assert alphas[-1] < ALPHA, "the comparison run never decays alpha"
    m, _, _ = model_for(net)
    s = solver_for(m, algo=kw["algo"], problem=kw["problem"], max_iter=2, max_batch=2)
    shape = (2, 3, 48, 48)
    cleans = [det_image(shape, 93), det_image(shape, 95)]
    n2 = do.H(cleans[1]) + sigma * det_normal(shape, 96)
    target = [noisy, n2]
    s.measurement_noise = lambda batch, hx: (target[batch].cuda() - hx) / sigma
    entering = []
    rb = s.restore_batch
    s.restore_batch = lambda *a, **k: (entering.append(k["alpha"]), rb(*a, **k))[1]
    s.solve_ip([(c, torch.zeros(2)) for c in cleans], dg, sigma)
    _, alphas2, infos2 = R.solve(oracle_net(net), do, n2, alpha=alphas[-1], **kw)
    assert all(abs(i["gap"] - i["thr"]) >= 0.01 * max(abs(i["gap"]), abs(i["thr"])) for i in infos2)
    assert entering == [ALPHA, alphas[-1]], entering
    assert s.last_alpha == alphas2[-1], (s.last_alpha, alphas2)
    assert torch.isfinite(s.last_restored).all()


# ---- 10. determinism, graphs, memory ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pgd_inpainting", "hqs_gaussian_deblurring_FFT"])
def test_replays_are_bit_identical_and_graphs_rebuild(hip, name):
    g = golden(name)
    algo, problem, noise_type = CASES[name]
    m, _, _ = model_for("tiny4")
    dg, do = degradations(problem, 64)
    sigma = float(g["sigma"])
    noisy = torch.from_numpy(g["noisy"]).cuda()
    s = solver_for(m, algo=algo, problem=problem)
    x1 = s.restore_batch(noisy, dg, sigma); a1 = s.last_alpha          # iteration 0 launched directly, then capture + replay
    x2 = s.restore_batch(noisy, dg, sigma); a2 = s.last_alpha          # every iteration replayed
    assert torch.equal(x1, x2) and a1 == a2, "the same restore_batch twice differs"
    s.use_graph = False
    x3 = s.restore_batch(noisy, dg, sigma); a3 = s.last_alpha
    s.use_graph = True
    assert torch.equal(x1, x3) and a1 == a3, "graph replay and direct launches differ"
    # another batch size, then another operator: the cached graph must not be replayed
    clean3 = det_image((3, 3, 64, 64), 97)
    noisy3 = do.H(clean3) + sigma * det_normal(tuple(do.H(clean3).shape), 98)
    kw = dict(algo=algo, problem=problem, max_iter=MAX_ITER, sigma_noise=sigma)
    x0 = R.initialise(problem, noisy3, do)
    ref, aref, info = R.iterate(oracle_net("tiny4"), do, x0, noisy3, 0, alpha=ALPHA, **kw)
    xb = s.restore_batch(noisy3.cuda(), dg, sigma, first=0, stop=1)
    np.testing.assert_allclose(xb.cpu().numpy(), ref.numpy(), atol=TOL(info["JN"].abs().max()))
    assert s.last_alpha == aref
    dn, don = degradations("denoising", 64)
    sd = solver_for(m, algo="pgd", problem="denoising")
    xs_ref, _, infos = R.solve(oracle_net("tiny4"), don, noisy3, alpha=ALPHA, algo="pgd", problem="denoising", max_iter=MAX_ITER, sigma_noise=0.2, stop=1)
    xd = sd.restore_batch(noisy3.cuda(), dn, 0.2, first=0, stop=1)
    np.testing.assert_allclose(xd.cpu().numpy(), xs_ref[1].numpy(), atol=TOL(infos[0]["JN"].abs().max()))
    x4 = s.restore_batch(noisy, dg, sigma)
    assert torch.equal(x1, x4), "after the rebuilds the first configuration no longer reproduces its bits"
    # the retained forward left behind is usable
    v = m.forward_retain(noisy, torch.full((2,), 0.3, device="cuda"))
    assert torch.isfinite(m.backward(torch.ones_like(v))).all()


def test_solver_buffers_are_counted_and_freed(hip):
    import pnpflow_amd.degradations as D
    m, _, _ = new_model("tiny4")              # an engine of its own
    b0 = m.memory_bytes()
    y = det_image((2, 3, 64, 64), 99).cuda()
    m.forward_retain(y, torch.full((2,), 0.1, device="cuda"))
    plan = m.memory_bytes() - b0                # the retained plan alone
    s = solver_for(m, algo="hqs", problem="gaussian_deblurring_FFT")
    s.restore_batch(y, D.GaussianDeblurring(1.0, 61, "fft", 3, 64), 0.05)
    b1 = m.memory_bytes()
    state = b1 - b0 - plan
    assert state >= 11 * y.numel() * 4, (state, y.numel())       # 7 image buffers, 2 measurement buffers, 2 images of scratch
    s.restore_batch(y, D.GaussianDeblurring(1.0, 61, "fft", 3, 64), 0.05)
    assert m.memory_bytes() == b1               # nothing grows on a second call
    s.restore_batch(y[:1], D.GaussianDeblurring(1.0, 61, "fft", 3, 64), 0.05)      # shape change: the B = 2 state is freed, a B = 1 one allocated
    b2 = m.memory_bytes()
    m.forward_retain(y[:1], torch.full((1,), 0.1, device="cuda"))
    assert m.memory_bytes() == b2
    assert b2 - b1 < plan, (b0, b1, b2, plan)   # a B = 1 plan and a smaller state: less than a second B = 2 plan
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    del s, m
    gc.collect()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] - free_before >= 0.9 * b2, "destroying the model does not give its device memory back"


# ---- 11. ABI error paths ------------------------------------------------------------------------------------------------------------
def test_abi_error_paths(hip):
    import pnpflow_amd._lib as L
    import pnpflow_amd.degradations as D
    m, _, _ = model_for("tiny4")
    y = det_image((2, 3, 64, 64), 99).cuda()
    x = y.clone()
    tab = np.full(3, 0.05, dtype=np.float32)

    def call(d, **kw):
        prm = L.PfPnpGsParams()
        prm.algo, prm.noise_model, prm.max_iter, prm.first, prm.stop, prm.skip_grad_step = 0, 0, 3, 0, 3, 0
        prm.host_sigma_den = tab.ctypes.data_as(C.POINTER(C.c_float))
        prm.grad_coef, prm.alpha, prm.use_graph = 1.0, 0.5, 1
        for k, v in kw.items():
            setattr(prm, k, v)
        rc = hip.pf_pnp_gs_restore(m.handle, C.byref(d), C.byref(prm), y.data_ptr(), x.data_ptr(), None, None, 2, L.current_stream_ptr(),
                                   C.cast(None, L.ITER_CB), None)
        return rc, (hip.pf_last_error(m.handle) or b"").decode()
    box = D.BoxInpainting(10).descriptor(2, 64, 64, y.device)
    blur = D.GaussianDeblurring(1.0, 61, "fft", 3, 64).descriptor(2, 64, 64, y.device)
    rmask = D.RandomInpainting(0.7)
    rnd = rmask.descriptor(2, 64, 64, y.device)
    nomask = L.PfDegradation(); nomask.kind = L.PF_DEG_MASK_INPAINTING
    for d, kw, word in ((box, dict(algo=1), "MASK_INPAINTING"), (nomask, dict(algo=1), "mask"), (box, dict(algo=2), "GAUSSIAN_BLUR"),
                        (rnd, dict(algo=1, noise_model=1), "laplace"), (blur, dict(algo=2, noise_model=1), "laplace"),
                        (box, dict(first=2, stop=1), "first"), (box, dict(stop=4), "max_iter"), (box, dict(algo=3), "algo")):
        rc, msg = call(d, **kw)
        assert rc == -1 and word in msg, (kw, rc, msg)           # PF_ERR_INVALID with a message
    torch.cuda.synchronize()
    assert torch.equal(x, y)                                       # nothing ran
    with pytest.raises(ValueError, match="laplace"):
        solver_for(m, algo="hqs", problem="random_inpainting", noise_type="laplace").restore_batch(y, rmask, 0.3)


# ---- 12. CLI ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,problem", [((), "inpainting"), (("algo", "hqs"), "gaussian_deblurring_FFT")])
def test_main_end_to_end(hip, tmp_path, extra, problem):
    """`python main.py --opts ... model gradient_step method pnp_gs ...` in a fresh child process writes the reference's result files."""
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--opts", "dataset", "celeba", "problem", problem, "model", "gradient_step", "method", "pnp_gs",
           "max_iter", "3", "max_batch", "1", "batch_size_ip", "2", "synthetic", "True", "output_root", str(tmp_path) + "/"] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    base = tmp_path / "results_synthetic" / "celeba" / "gradient_step" / problem / "pnp_gs"
    found = {p.name for p in base.rglob("*") if p.is_file()}
    assert "psnr_rec_batch0.txt" in found, found
    d = [p for p in base.rglob("psnr_rec_batch0.txt")][0].parent
    assert "max_iter=3" in str(d) and ("algo=hqs" if extra else "algo=pgd") in str(d), str(d)
