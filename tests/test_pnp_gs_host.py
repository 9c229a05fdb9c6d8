"""CPU checks of Prox-PnP with the gradient-step denoiser (pnpflow/methods/pnp_gs.py, pnpflow/train_denoiser.py): the restatement
(tests/pnp_gs_restatement.py) against goldens of the REAL reference (tests/golden/pnp_gs_tiny4_*.npz, tools/make_golden_pnp_gs.py), the
C ABI surface, the config / CLI wiring, the host schedule and the error paths.  No GPU needed.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import CFGS, det_image, det_normal
from oracle import pnpflow_oracle as O
import pnp_gs_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("pf_gs_denoiser_grad", "pf_pnp_gs_restore")
CLEAN_SEED, GRAD_SEED = 33, 77          # tools/make_golden_pnp_gs.py
MAX_ITER, ALPHA = 3, 0.5
# name -> (algo, problem, noise_type)
CASES = {"pgd_denoising": ("pgd", "denoising", "gaussian"),
         "pgd_inpainting": ("pgd", "inpainting", "gaussian"),
         "pgd_superresolution": ("pgd", "superresolution", "gaussian"),
         "pgd_gaussian_deblurring_FFT": ("pgd", "gaussian_deblurring_FFT", "gaussian"),
         "pgd_laplace_denoising": ("pgd", "denoising", "laplace"),
         "pgd_laplace_inpainting": ("pgd", "inpainting", "laplace"),
         "hqs_random_inpainting": ("hqs", "random_inpainting", "gaussian"),
         "hqs_gaussian_deblurring_FFT": ("hqs", "gaussian_deblurring_FFT", "gaussian")}


def oracle_degradation(problem, S):
    return {"denoising": lambda: O.Denoising(), "inpainting": lambda: O.BoxInpainting(10), "superresolution": lambda: O.Superresolution(4, S),
            "gaussian_deblurring_FFT": lambda: O.GaussianDeblurring(1.0, 61, "fft", 3, S), "random_inpainting": lambda: O.RandomInpainting(0.7)}[problem]()


_NET = {}


def tiny4_net():
    if not _NET:
        c = CFGS["tiny4"]; cfg = O.unet_config(**c); sd = O.synthetic_state_dict(cfg, 0)
        _NET["f"] = lambda x, s: O.unet_forward(sd, cfg, x, s)
    return _NET["f"]


def kwargs_of(name, g):
    algo, problem, noise_type = CASES[name]
    return dict(algo=algo, problem=problem, noise_type=noise_type, max_iter=MAX_ITER, sigma_noise=float(g["sigma"]))


# ---- 1. the restatement against the real reference ----------------------------------------------------------------------------
def test_restatement_calculate_grad_matches_reference_golden():
    g = np.load(os.path.join(GOLD, "pnp_gs_tiny4_calculate_grad.npz"))
    shape = (2, 3, 64, 64)
    x = det_image(shape, GRAD_SEED) + 0.1 * det_normal(shape, GRAD_SEED, 1)
    assert g["sigma"][0] != g["sigma"][1]
    Dg, N, gg, _ = R.calculate_grad(tiny4_net(), x, torch.from_numpy(g["sigma"]))
    np.testing.assert_allclose(Dg.numpy(), g["Dg"], atol=1e-5 * float(np.abs(g["Dg"]).max()))
    np.testing.assert_allclose(N.numpy(), g["N"], atol=1e-5 * float(np.abs(g["N"]).max()))
    assert abs(float(gg) - float(g["g"])) <= 1e-5 * abs(float(g["g"]))


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_reference_goldens(name):
    g = np.load(os.path.join(GOLD, f"pnp_gs_tiny4_{name}.npz"))
    algo, problem, noise_type = CASES[name]
    net, d = tiny4_net(), oracle_degradation(problem, 64)
    shape = (2, 3, 64, 64)
    sigma, seed = float(g["sigma"]), int(g["noise_seed"])
    its = [torch.from_numpy(a) for a in g["iterates"]]
    assert len(its) == MAX_ITER + 1 and len(g["alpha"]) == MAX_ITER + 1
    # the measurement by recipe: distinct clean images, the tool's deterministic draw
    clean = det_image(shape, CLEAN_SEED)
    hc = d.H(clean)
    unit = R.det_laplace(tuple(hc.shape), seed, 0) if noise_type == "laplace" else det_normal(tuple(hc.shape), seed, 0)
    np.testing.assert_allclose((hc + unit * sigma).numpy(), g["noisy"], atol=1e-6)
    if "mask" in g.files:
        assert np.array_equal(g["mask"], O.random_mask_array(2, 64, 64, 0.7).astype(np.uint8))
    noisy = torch.from_numpy(g["noisy"])
    kw = kwargs_of(name, g)
    scale = lambda a: float(a.abs().max())
    # initialisation and teacher-forced single iterations (1-step comparisons)
    np.testing.assert_allclose(R.initialise(problem, noisy, d).numpy(), its[0].numpy(), atol=1e-4 * scale(its[0]))
    for k in range(MAX_ITER):
        xn, an, info = R.iterate(net, d, its[k], noisy, k, alpha=float(g["alpha"][k]), **kw)
        np.testing.assert_allclose(xn.numpy(), its[k + 1].numpy(), atol=1e-4 * scale(its[k + 1]), err_msg=f"iteration {k}")
        assert an == float(g["alpha"][k + 1]), (k, an, g["alpha"])
        if name == "hqs_gaussian_deblurring_FFT":
            np.testing.assert_allclose([info["gap"], info["thr"]], g["gap"][k], rtol=1e-3)
    # free-running from the restatement's own initialisation
    xs, alphas, _ = R.solve(net, d, noisy, alpha=ALPHA, **kw)
    assert alphas == [float(a) for a in g["alpha"]]
    growth = float(g["growth"])
    assert growth >= 1.0 and growth ** 2 * 2e-4 <= 0.05
    for k in range(1, MAX_ITER + 1):
        np.testing.assert_allclose(xs[k].numpy(), its[k].numpy(), atol=2e-4 * growth ** (k - 1) * scale(its[k]), err_msg=f"after iteration {k}")
    if name == "hqs_random_inpainting":
        assert np.array_equal(g["iterates"][MAX_ITER], g["iterates"][MAX_ITER - 1])      # the last iteration leaves x as it is
    if name == "hqs_gaussian_deblurring_FFT":
        gap, thr = g["gap"][:, 0], g["gap"][:, 1]
        assert (np.abs(gap - thr) >= 0.01 * np.maximum(np.abs(gap), np.abs(thr))).all()       # no decision can flip on rounding
        assert g["alpha"][-1] < ALPHA                                                           # the golden exercises the decay


# ---- 2. ABI surface, config, CLI wiring -------------------------------------------------------------------------------------------
def test_new_symbols_declared_exported_and_typed():
    import pnpflow_amd._lib as L
    header = open(os.path.join(ROOT, "include", "pnpflow_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in include/pnpflow_hip.h"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
    declared = set(re.findall(r"\b(pf_[a-z_A-Z0-9]+)\s*\(", header)) - {"pf_iter_callback"}
    assert set(L.SIGNATURES) <= declared
    m = re.search(r"#define PF_ABI_VERSION (\d+)", header)
    assert int(m.group(1)) == L.PF_ABI_VERSION >= 5
    # the params struct mirrors the header field for field
    body = re.search(r"typedef struct pf_pnp_gs_params \{(.*?)\} pf_pnp_gs_params;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip().replace("*", " "))]
    assert fields == [f[0] for f in L.PfPnpGsParams._fields_], fields
    if os.path.isfile(L.LIB_PATH):
        lib = L.load()
        for name in NEW_SYMBOLS:
            assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    import __graft_entry__ as G
    assert "prox_pnp.hip" in G.SOURCES


def test_config_loads_through_parse_args(monkeypatch):
    import main as M
    monkeypatch.chdir(ROOT)
    monkeypatch.setattr(sys, "argv", ["main.py", "--opts", "method", "pnp_gs", "model", "gradient_step", "dataset", "celeba"])
    cfg = M.parse_args()
    assert list(cfg.dict_cfg_method.keys()) == ["max_iter", "lr_pnp", "alpha", "algo", "sigma_factor"]
    assert dict(cfg.dict_cfg_method) == dict(max_iter=30, lr_pnp=1.0, alpha=0.5, algo="pgd", sigma_factor=1.0)
    assert cfg.method == "pnp_gs" and cfg.model == "gradient_step"
    monkeypatch.setattr(sys, "argv", ["main.py", "--opts", "method", "pnp_gs", "model", "gradient_step", "algo", "hqs", "max_iter", "7"])
    cfg = M.parse_args()
    assert cfg.algo == "hqs" and cfg.max_iter == 7 and cfg.dict_cfg_method["algo"] == "hqs"
    src = open(os.path.join(ROOT, "main.py")).read()
    assert "args.method == 'pnp_gs'" in src and "PROX_PNP(GRADIENT_STEP_DENOISER(model, device, args), device, args)" in src
    from pnpflow.methods.pnp_gs import PROX_PNP
    from pnpflow_amd.methods.pnp_gs import PROX_PNP as P2
    from pnpflow.train_denoiser import GRADIENT_STEP_DENOISER
    from pnpflow_amd.train_denoiser import GRADIENT_STEP_DENOISER as G2
    assert PROX_PNP is P2 and GRADIENT_STEP_DENOISER is G2
    for m in ("model_forward", "grad_datafit", "prox_datafit", "objective", "solve_ip", "run_method", "should_save_image", "restore_batch"):
        assert callable(getattr(PROX_PNP, m))
    for m in ("calculate_grad", "forward", "train", "configure_optimizers"):
        assert callable(getattr(GRADIENT_STEP_DENOISER, m))
    for m in ("train", "configure_optimizers"):
        with pytest.raises(NotImplementedError):
            getattr(GRADIENT_STEP_DENOISER, m)(object.__new__(GRADIENT_STEP_DENOISER), *([None] if m == "train" else []))


# ---- 3. host schedule -----------------------------------------------------------------------------------------------------------
class _NoNet:
    input_channels, input_height = 3, 64


def solver_for(**kw):
    from pnpflow_amd.methods.pnp_gs import PROX_PNP
    from pnpflow_amd.utils import CfgNode
    a = dict(method="pnp_gs", model="gradient_step", problem="inpainting", noise_type="gaussian", algo="pgd", max_iter=30, lr_pnp=1.0, alpha=0.5,
             sigma_factor=1.0, max_batch=0, compute_time=False, compute_memory=False, save_results=False, batch=0)
    a.update(kw)
    return PROX_PNP(_NoNet(), torch.device("cpu"), CfgNode(a))


def test_level_tables_follow_the_reference():
    f32 = np.float32
    t = solver_for(algo="hqs", problem="random_inpainting", max_iter=25).level_table(0.01)
    assert t.dtype == f32 and t.shape == (25,)
    assert (t[:20] == f32(0.2)).all() and (t[20:] == f32(0.01)).all()
    t = solver_for(algo="hqs", problem="gaussian_deblurring_FFT", max_iter=4).level_table(0.05)
    assert (t == f32(1.8 * 0.05)).all() and t.shape == (4,)
    t = solver_for(algo="pgd", sigma_factor=1.5, max_iter=3).level_table(0.2)
    assert (t == f32(1.5 * 0.2)).all()
    # the restatement's schedule is the same one
    for code, s in ((solver_for(algo="hqs", problem="random_inpainting", max_iter=25), 0.01), (solver_for(algo="pgd", sigma_factor=1.5), 0.2)):
        tab = code.level_table(s)
        assert [f32(R.level(code.algo_code(), it, s, code.args.sigma_factor)) for it in range(len(tab))] == list(tab)
    assert [solver_for(algo=a, problem=p).algo_code() for a, p in (("pgd", "denoising"), ("hqs", "random_inpainting"), ("hqs", "gaussian_deblurring_FFT"))] == [0, 1, 2]


def test_lr_pnp_is_multiplied_in_place_on_every_solve_ip_call():
    import pnpflow_amd.degradations as D
    s = solver_for(lr_pnp=2.0)
    s.solve_ip(iter([]), D.BoxInpainting(10), 0.05)          # max_batch 0: the schedule runs, no batch does
    assert s.args.lr_pnp == 0.05 ** 2 * 2.0 and s.args.sigma_noise == 0.05
    s.solve_ip(iter([]), D.BoxInpainting(10), 0.05)
    assert s.args.lr_pnp == 0.05 ** 2 * (0.05 ** 2 * 2.0)


# ---- 4. error paths without a GPU -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", ["denoising", "inpainting", "superresolution", "paintbrush_inpainting"])
def test_hqs_with_an_unsupported_problem_is_an_error(problem):
    import pnpflow_amd.degradations as D
    s = solver_for(algo="hqs", problem=problem)
    with pytest.raises(ValueError, match="random_inpainting.*gaussian_deblurring_FFT"):
        s.solve_ip(iter([]), D.Denoising(), 0.05)
    with pytest.raises(ValueError, match="supported"):
        s.level_table(0.05)
    with pytest.raises(ValueError, match="supported"):
        solver_for(algo="admm").algo_code()


def test_pnp_gs_needs_the_gradient_step_model(monkeypatch):
    import main as M
    monkeypatch.chdir(ROOT)
    monkeypatch.setattr(sys, "argv", ["main.py", "--opts", "method", "pnp_gs", "model", "ot", "synthetic", "True"])
    with pytest.raises(SystemExit, match="model gradient_step"):
        M.main()


def test_multi_rank_runs_are_refused(monkeypatch):
    import pnpflow_amd.degradations as D
    monkeypatch.setenv("WORLD_SIZE", "2")
    s = solver_for()
    with pytest.raises(RuntimeError, match="one GPU only"):
        s.solve_ip(iter([]), D.BoxInpainting(10), 0.05)
    assert s.args.lr_pnp == 1.0          # refused before anything is touched


def test_define_and_load_gradient_step_model_accepts_both_checkpoint_forms(tmp_path, monkeypatch):
    """load_model('gradient_step') takes a plain state dict or a dict holding model_state_dict (the per-epoch training checkpoints)."""
    from pnpflow_amd import utils as U

    class Rec:
        def load_state_dict(self, sd):
            self.sd = sd

        def to(self, d):
            return self
    sd = {"w": torch.ones(2)}
    for i, obj in enumerate((sd, {"model_state_dict": sd, "optimizer_state_dict": {}})):
        p = tmp_path / f"c{i}.pt"
        torch.save(obj, p)
        m = Rec()
        U.load_model("gradient_step", m, None, checkpoint_path=str(p), device="cpu")
        assert list(m.sd.keys()) == ["w"]
    src = open(os.path.join(ROOT, "pnpflow_amd", "utils.py")).read()
    assert '"gradient_step"' in src
