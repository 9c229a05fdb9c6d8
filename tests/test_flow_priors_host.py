"""CPU checks of Flow-Priors (pnpflow/methods/flow_priors.py): the C ABI surface, the one-element Adam update of csrc/adam_step.h against
torch.optim.Adam, the CPU restatement (tests/flow_priors_restatement.py) against its fixtures (tests/golden/flow_priors_*.npz,
tools/make_golden_flow_priors.py), the finite-difference identity the engine's trace gradient rests on, and the config / class wiring.
No GPU needed.

tests/adam_step_shim.cpp is compiled with ROCm's host clang++ into a temporary directory and loaded with ctypes; a missing compiler is a failure.

The Adam bound (also the GPU test's): each updated x lies within 2 ulp(|x|) + 1e-6 lr of torch's, m and v within 2 ulp.  Derived, not measured:
the update is six fp32 roundings (lerp, two products and a sum for v, sqrt, the quotient by sqrt(bc2), the sum with eps, the step product, the
quotient, the sum with x) of which those behind m / denom scale the step, at most a few lr, by a few 2^-24 < 1e-6.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import pnpflow_oracle as O
import flow_priors_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "pnpflow_amd", "csrc")
NEW_SYMBOLS = ("pf_adam_step", "pf_flow_priors_grad", "pf_flow_priors_restore")
TINY4 = dict(input_channels=3, input_height=64, ch=32, ch_mult=(1, 2, 4, 8), num_res_blocks=1, attn_resolutions=(16, 8))
D = torch.float64


# ---- 1. ABI surface -----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_declared_exported_and_typed():
    import pnpflow_amd._lib as L
    header = open(os.path.join(ROOT, "include", "pnpflow_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} not declared in include/pnpflow_hip.h"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
    body = re.search(r"typedef struct pf_flow_priors_params \{(.*?)\} pf_flow_priors_params;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(m.group(1), m.group(2)) for m in re.finditer(r"(int32_t|uint64_t|double|float)\s+(\w+)\s*;", body)]
    ctype = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(L.PfFlowPriorsParams._fields_), "PfFlowPriorsParams does not mirror the header's struct"
    assert "#define PF_ABI_VERSION 6" in header and L.PF_ABI_VERSION == 6          # the calls are additive
    if os.path.isfile(L.LIB_PATH):
        lib = L.load()
        for name in NEW_SYMBOLS:
            assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    import __graft_entry__ as G
    assert "flow_priors.hip" in G.SOURCES
    assert '#include "engine_flow_priors.inc"' in open(os.path.join(CSRC, "engine.hip")).read()


# ---- 2. adam_step.h against torch.optim.Adam ------------------------------------------------------------------------------------------------
def _host_clang():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for cand in (os.path.join(os.path.dirname(hipcc), "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.isfile(cand):
            return cand
    pytest.fail("no host clang++ next to HIPCC or under /opt/rocm/llvm/bin: the Adam test cannot run")


@pytest.fixture(scope="module")
def adam(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("adam_step") / "libadam_step_shim.so")
    cmd = [_host_clang(), "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so, os.path.join(ROOT, "tests", "adam_step_shim.cpp")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, "adam_step.h must compile as plain host C++17:\n" + res.stderr
    lib = C.CDLL(so)
    lib.adam_step_array.restype = None
    lib.adam_step_array.argtypes = [C.c_void_p] * 4 + [C.c_int64] + [C.c_double] * 4 + [C.c_int]
    return lib


@pytest.mark.parametrize("lr", [0.01, 0.3])
def test_adam_step_header_matches_torch(adam, lr):
    x, gs = R.adam_inputs(4099, 3)
    ref = R.torch_adam_reference(x, gs, lr)
    m, v = np.zeros_like(x), np.zeros_like(x)
    for k, g in enumerate(gs):
        adam.adam_step_array(x.ctypes.data, m.ctypes.data, v.ctypes.data, g.ctypes.data, x.size, lr, 0.9, 0.999, 1e-8, k + 1)
        R.check_adam_bound(x, m, v, *ref[k], lr, f"step {k + 1}")
    # a fresh Adam's first step is eta sign(g) to rounding, 0 where g is 0 (what the solver's tests are built around)
    x0, gs0 = R.adam_inputs(4099, 3)
    g0 = gs0[0]
    big = (np.abs(g0) > 1e-3) & (np.abs(g0) < 1e15)
    np.testing.assert_allclose((ref[0][0] - x0)[big], (-lr * np.sign(g0))[big], rtol=1e-4)
    assert np.all((ref[0][0] - x0)[g0 == 0] == 0)


# ---- 3. the restatement reproduces every fixture ---------------------------------------------------------------------------------------------
_VELS = {}


def vels(which="tiny4"):
    if which not in _VELS:
        if which == "tiny4":
            cfg = O.unet_config(**TINY4)
            sd = O.synthetic_state_dict(cfg, 0)
            _VELS[which] = (R.oracle_vel(sd, cfg, torch.float32), R.oracle_vel(sd, cfg, D))
        else:
            from oracle import ncsnpp_oracle as NO
            cfg = NO.ncsnpp_config(image_size=32, nf=32, ch_mult=(1, 1, 2), num_res_blocks=2, attn_resolutions=(16,))
            sd = NO.synthetic_state_dict(cfg, 0)
            _VELS[which] = (R.ncsnpp_vel(sd, cfg, torch.float32), R.ncsnpp_vel(sd, cfg, D))
    return _VELS[which]


def check_single_step(g, case, v32, v64, S, half):
    op, noise_type, it, inp = R.case_inputs(case, S=S, half=half)
    i64 = {k: v.double() for k, v in inp.items()}
    assert int(g["iteration"]) == it and int(g["seed"]) == case[4]
    out = R.grad(v64, op.H, i64["x"], i64["x_init"], i64["y"], i64["eps"], it, R.N_STEP, R.LMBDA, noise_type)
    scale = float(np.abs(g["g64"]).max())
    for key, val in (("g64", out[0]), ("g_data64", out[1]), ("g_trace64", out[2])):
        # stored as fp32: 2^-24 relative per value, plus the thread-count dependence of the CPU convolutions' summation order
        np.testing.assert_allclose(val.numpy(), g[key].astype(np.float64), atol=2e-7 * max(scale if key != "g_trace64" else 0.0, float(np.abs(g[key]).max())), err_msg=key)
    assert abs(float(out[4].abs().max()) - float(g["pred_max"])) <= 1e-9 * float(g["pred_max"])
    assert abs(float(out[3].abs().max()) - float(g["g_extra_max"])) <= 1e-9 * float(g["g_extra_max"])
    g32 = R.grad(v32, op.H, inp["x"], inp["x_init"], inp["y"], inp["eps"], it, R.N_STEP, R.LMBDA, noise_type)[0]
    err32 = float((g32.double() - out[0]).abs().max())
    assert 0.25 * float(g["g32_err"]) <= err32 <= 4 * float(g["g32_err"]), (err32, float(g["g32_err"]))          # fp32 rounding: the same size, not the same bits
    x_new = R.step(v64, op.H, i64["x"], i64["x_init"], i64["y"], [i64["eps"]], it, R.N_STEP, R.LMBDA, R.ETA, noise_type)[0]
    np.testing.assert_allclose(x_new.numpy(), g["x_new64"].astype(np.float64), atol=2e-7 * float(np.abs(g["x_new64"]).max()))


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_reproduces_single_step_fixture(name):
    g = np.load(os.path.join(GOLD, f"flow_priors_tiny4_{name}.npz"))
    check_single_step(g, R.CASES[name], *vels("tiny4"), 64, 10)


def test_restatement_reproduces_ncsnpp_fixture():
    g = np.load(os.path.join(GOLD, "flow_priors_ncsnpp_tiny_inpainting_it50.npz"))
    check_single_step(g, R.NCSNPP_CASE, *vels("ncsnpp"), 32, 5)


def test_free_run_fixture_is_consistent_and_starts_as_the_restatement_does():
    """The N = 24 run takes minutes on the CPU: the test repeats its first outer iteration in fp32 and fp64 and re-derives the statistics
    (d32, m32, PSNR) from the stored final iterates."""
    g = np.load(os.path.join(GOLD, "flow_priors_tiny4_free_run.npz"))
    v32, v64 = vels("tiny4")
    op, noise_type, _, inp = R.case_inputs(R.FREE_CASE)
    seed = R.FREE_CASE[4]
    shape = tuple(inp["x_init"].shape)
    for vel, dtype, key in ((v32, torch.float32, "x32_first"), (v64, D, "x64_first")):
        x1 = R.step(vel, op.H, inp["x_init"].to(dtype), inp["x_init"].to(dtype), inp["y"].to(dtype), [R.probe(shape, seed, 100, dtype)], 0, R.FREE_N, R.LMBDA, R.ETA)[0]
        # identical but for pixels whose gradient sign hangs on rounding (fp32 thread-count dependence): at most 2 eta there, 0.1 % of them
        diff = (x1.double() - torch.from_numpy(g[key]).double()).abs()
        assert float((diff > 1e-5).double().mean()) <= 1e-3 and float(diff.max()) <= 2 * R.ETA + 1e-5, key
    dist = np.abs(g["x32"].astype(np.float64) - g["x64"])
    far = dist > R.ETA / 2
    assert abs(far.mean() - float(g["d32"])) <= 1e-4 and abs(dist[~far].max() - float(g["m32"])) <= 1e-6
    for key, x in (("psnr32", g["x32"]), ("psnr64", g["x64"])):
        np.testing.assert_allclose(O.psnr_per_image(torch.from_numpy(x), inp["clean"]).numpy(), g[key], atol=1e-3)


# ---- 4. the identity: the central difference of two VJPs converges to the autograd trace gradient at second order ------------------------------
def test_fd_trace_gradient_converges_at_second_order_fp64():
    g = np.load(os.path.join(GOLD, "flow_priors_tiny4_inpainting_it0.npz"))
    _, v64 = vels("tiny4")
    op, noise_type, it, inp = R.case_inputs(R.CASES["inpainting_it0"])
    x, eps = inp["x"].double(), inp["eps"].double()
    with torch.enable_grad():
        xx = x.clone().requires_grad_(True)
        tr = R.trace_value(v64, xx, R.schedule(R.N_STEP, 0.0, it)[0], eps, create_graph=True) * R.schedule(R.N_STEP, 0.0, it)[1]
        (exact,) = torch.autograd.grad(tr.sum(), xx)
    np.testing.assert_allclose(exact.numpy(), g["g_trace64"].astype(np.float64), atol=2e-7 * float(np.abs(g["g_trace64"]).max()))
    errs = [float((R.fd_grad_trace(v64, x, eps, it, R.N_STEP, h) - exact).abs().max()) for h in R.FD_STEPS]
    np.testing.assert_allclose(errs, g["trunc64"], rtol=0.02)
    for (h0, e0), (h1, e1) in zip(zip(R.FD_STEPS, errs), list(zip(R.FD_STEPS, errs))[1:]):
        order = np.log(e1 / e0) / np.log(h1 / h0)
        assert 1.9 <= order <= 2.1, (h0, h1, order, errs)
    assert errs[0] <= 1e-4 * float(exact.abs().max())          # and it converges to the autograd value, not to something else


# ---- 5 / 6. config, class wiring, refusals --------------------------------------------------------------------------------------------------
def test_config_names_the_result_folder_from_five_keys():
    from pnpflow_amd.utils import get_save_path_ip, load_cfg_from_cfg_file
    cfg = load_cfg_from_cfg_file(os.path.join(ROOT, "config", "method_config", "flow_priors.yaml"))
    assert list(cfg.keys()) == ["start_time", "K", "N", "lmbda", "eta"]
    assert dict(cfg) == dict(start_time=0.0, K=1, N=100, lmbda=1000, eta=0.01)
    assert get_save_path_ip(dict(cfg)) == "start_time=0.0/K=1/N=100/lmbda=1000/eta=0.01"
    src = open(os.path.join(ROOT, "main.py")).read()
    assert "args.method == 'flow_priors'" in src and "FLOW_PRIORS(model, device, args)" in src
    from pnpflow.methods.flow_priors import FLOW_PRIORS
    from pnpflow_amd.methods.flow_priors import FLOW_PRIORS as F2
    assert FLOW_PRIORS is F2
    for m in ("model_forward", "solve_ip", "run_method"):
        assert callable(getattr(FLOW_PRIORS, m))


class _NoNet:
    input_channels, input_height = 3, 64

    def to(self, device):
        return self


class _Loader:
    """Counts what solve_ip takes from it: a refusal must come before the first batch is drawn."""
    def __init__(self):
        self.taken = 0

    def __iter__(self):
        return self

    def __next__(self):
        self.taken += 1
        return torch.zeros(2, 3, 64, 64), torch.zeros(2)


def solver_for(**kw):
    from pnpflow_amd.methods.flow_priors import FLOW_PRIORS
    from pnpflow_amd.utils import CfgNode
    a = dict(method="flow_priors", model="ot", problem="inpainting", noise_type="gaussian", N=100, K=1, lmbda=1000, eta=0.01, start_time=0.0, max_batch=1,
             compute_time=False, compute_memory=False, save_results=False, batch=0)
    a.update(kw)
    return FLOW_PRIORS(_NoNet(), torch.device("cpu"), CfgNode(a))


def test_refuses_multi_rank_and_unknown_noise_before_drawing(monkeypatch):
    import pnpflow_amd.degradations as Dg
    from pnpflow_amd.methods.flow_priors import DEFAULT_FD_STEP
    s = solver_for(noise_type="poisson")
    ld = _Loader()
    state = torch.random.get_rng_state()
    with pytest.raises(ValueError, match="Noise type not supported"):
        s.solve_ip(ld, Dg.BoxInpainting(10), 0.05)
    assert ld.taken == 0 and torch.equal(torch.random.get_rng_state(), state)
    monkeypatch.setenv("WORLD_SIZE", "2")
    s = solver_for()
    with pytest.raises(RuntimeError, match="one GPU only"):
        s.solve_ip(ld, Dg.BoxInpainting(10), 0.05)
    assert ld.taken == 0 and torch.equal(torch.random.get_rng_state(), state)
    assert s.fd_step == DEFAULT_FD_STEP and solver_for(fd_step=1e-2).fd_step == 1e-2          # --opts fd_step ...
