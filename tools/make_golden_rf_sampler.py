"""Generate tests/golden/rf_sampler_tiny.npz: the REAL rectified-flow samplers of the reference (pnpflow/image_generation/sampling.py,
sde_lib.py) on the REAL NCSN++ module with the oracle's synthetic weights.  Run in the build container:   python tools/make_golden_rf_sampler.py

Imports go through tools/ref_import.install_stubs and the torch.utils.cpp_extension.load stub of make_golden.py::gen_ncsnpp (on CPU tensors the
reference takes its pure-torch FIR branch); sde_lib.RectifiedFlow.ode imports `models.utils`, which is aliased to the reference's
pnpflow.image_generation.models.utils.  The file holds data only: inputs, the recorded noise, outputs, evaluation counts.

Net: NCSN++ `tiny` (32^2, nf 32, ch_mult (1, 1, 2), 2 blocks, attention at 16) with ncsnpp_oracle.synthetic_state_dict(cfg, 0); B = 2;
z = det_normal((2, 3, 32, 32), 61); x0 = det_image((2, 3, 32, 32), 62) for the reverse solve.

  a_x                 euler_sampler, sample_N = 4, sigma_var = 0
  b_x, b_noise        euler_sampler, sample_N = 4, sigma_var = 0.5, torch.randn_like patched to the recorded draws b_noise[i]
  c_ref32_*           rk45_sampler at ode_tol = 1e-5 on the fp32 module;  c_ref64_*: tests/rf_sampler_restatement.py on the fp64 oracle at 1e-5;
  c_tight_*           the same at 1e-9 (the yardstick the GPU test measures distances to);  c_gap = max|ref32 - ref64|
  d_*                 sde.ode(x0, reverse=True) likewise (ref32 from the real sde_lib; its evaluation count by counting the module's calls)
  e_x                 sde.euler_ode(z, N = 3)
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ncsnpp_oracle as NO  # noqa: E402
from oracle import pnpflow_oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CFG = dict(image_size=32, nf=32, ch_mult=(1, 1, 2), num_res_blocks=2, attn_resolutions=(16,))      # make_golden.py NCSNPP_CFGS["tiny"]
SHAPE = (2, 3, 32, 32)
Z_SEED, X_SEED, NOISE_SEED = 61, 62, 63

torch.set_num_threads(8)


def det_normal(shape, seed, idx=0):
    g = np.random.Generator(np.random.Philox(key=[seed, idx]))
    return torch.from_numpy(g.standard_normal(size=shape, dtype=np.float32))


def det_image(shape, seed):
    """tests/conftest.py det_image."""
    x = det_normal(shape, seed, 7)
    k = torch.ones(shape[1], 1, 3, 3) / 9.0
    for _ in range(5):
        x = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), k, groups=shape[1])
    lo = x.amin(dim=(1, 2, 3), keepdim=True); hi = x.amax(dim=(1, 2, 3), keepdim=True)
    return ((x - lo) / (hi - lo) * 2 - 1).contiguous()


def import_reference():
    import torch.utils.cpp_extension as ce
    saved = ce.load
    ce.load = lambda *a, **k: types.SimpleNamespace()
    try:
        from ref_import import REF, install_stubs
        install_stubs()
        for name in ("tqdm", "matplotlib", "matplotlib.pyplot"):
            try:
                importlib.import_module(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
                if name == "tqdm":
                    sys.modules[name].tqdm = lambda it, *a, **k: it
        if REF not in sys.path:
            sys.path.insert(0, REF)
        nc = importlib.import_module("pnpflow.image_generation.models.ncsnpp")
        mutils = importlib.import_module("pnpflow.image_generation.models.utils")
        sys.modules.setdefault("models", importlib.import_module("pnpflow.image_generation.models"))
        sys.modules.setdefault("models.utils", mutils)
        sampling = importlib.import_module("pnpflow.image_generation.sampling")
        sde_lib = importlib.import_module("pnpflow.image_generation.sde_lib")
    finally:
        ce.load = saved
    return nc, sampling, sde_lib


def ref_config(c):      # make_golden.py gen_ncsnpp
    NS = types.SimpleNamespace
    return NS(model=NS(nf=c["nf"], ch_mult=c["ch_mult"], num_res_blocks=c["num_res_blocks"], attn_resolutions=c["attn_resolutions"],
                       dropout=0., resamp_with_conv=True, conditional=True, fir=True, fir_kernel=[1, 3, 3, 1], skip_rescale=True,
                       resblock_type='biggan', progressive='output_skip', progressive_input='input_skip', progressive_combine='sum',
                       attention_type='ddpm', embedding_type='fourier', init_scale=0., fourier_scale=16, conv_size=3,
                       nonlinearity='swish', scale_by_sigma=True, sigma_max=378, sigma_min=0.01, num_scales=2000, name='ncsnpp'),
              data=NS(image_size=c["image_size"], num_channels=3, centered=True),
              training=NS(continuous=False, sde='rectified_flow'))


def main():
    import rf_sampler_restatement as R
    nc, sampling, sde_lib = import_reference()
    cfg = NO.ncsnpp_config(**CFG)
    sd = NO.synthetic_state_dict(cfg, 0)
    m = nc.NCSNpp(ref_config(CFG)).eval()
    m.load_state_dict(sd, strict=False)
    calls = [0]
    m.register_forward_hook(lambda *a: calls.__setitem__(0, calls[0] + 1))
    sd64 = {k: v.double() for k, v in sd.items()}
    fir = O.fir_kernel_2d
    O.fir_kernel_2d = lambda k, gain=1.0: fir(k, gain).double()          # the FIR taps ([1, 3, 3, 1] / 8 per axis) are exact in either format
    f64 = lambda x, lab: NO.ncsnpp_forward(sd64, cfg, x, lab)
    ident = lambda x: x
    z, x0 = det_normal(SHAPE, Z_SEED), det_image(SHAPE, X_SEED)
    out = dict(z_seed=np.array(Z_SEED), x_seed=np.array(X_SEED))

    def sde(**kw):
        return sde_lib.RectifiedFlow(init_type='gaussian', noise_scale=1.0, **kw)

    # (a) Euler ODE
    x, nfe = sampling.get_rectified_flow_sampler(sde(use_ode_sampler='euler', sigma_var=0.0, sample_N=4), SHAPE, ident, device='cpu')(m, z=z.clone())
    out["a_x"], out["a_nfe"] = x.numpy(), np.array(nfe)
    # (b) the SDE form with recorded draws
    noise = torch.stack([det_normal(SHAPE, NOISE_SEED, i) for i in range(4)])
    draws = iter(noise)
    saved = torch.randn_like
    torch.randn_like = lambda t, *a, **k: next(draws).clone()
    try:
        x, nfe = sampling.get_rectified_flow_sampler(sde(use_ode_sampler='euler', sigma_var=0.5, sample_N=4), SHAPE, ident, device='cpu')(m, z=z.clone())
    finally:
        torch.randn_like = saved
    assert next(draws, None) is None
    out["b_x"], out["b_noise"], out["b_sigma_var"] = x.numpy(), noise.numpy(), np.array(0.5)
    # (c) RK45 sampler
    x, nfe = sampling.get_rectified_flow_sampler(sde(use_ode_sampler='rk45', ode_tol=1e-5), SHAPE, ident, device='cpu')(m, z=z.clone())
    runs = {"c_ref32": (x.double().numpy(), nfe), "c_ref64": R.rk45_sampler(f64, z, 1e-5, dtype=torch.float64)[:2],
            "c_tight": R.rk45_sampler(f64, z, 1e-9, dtype=torch.float64)[:2]}
    # (d) the reverse solve of sde_lib
    calls[0] = 0
    x = sde().ode(x0.clone(), m, reverse=True)
    runs.update({"d_ref32": (x.double().numpy(), calls[0]), "d_ref64": R.ode(f64, x0, True, dtype=torch.float64)[:2],
                 "d_tight": R.ode(f64, x0, True, dtype=torch.float64, rtol=1e-9, atol=1e-9)[:2]})
    for k, (y, nfev) in runs.items():
        assert (nfev - 2) % 6 == 0
        out[k + "_x"] = y.astype(np.float32) if "ref32" in k else y
        out[k + "_nfev"] = np.array(nfev)
        print(k, "nfev", nfev, "attempts", (nfev - 2) // 6, "max|x|", float(np.abs(y).max()))
    for c in "cd":
        out[c + "_gap"] = np.array(np.abs(runs[c + "_ref32"][0] - runs[c + "_ref64"][0]).max())
        print(c, "ref32-ref64", float(out[c + "_gap"]), "ref32-tight", float(np.abs(runs[c + "_ref32"][0] - runs[c + "_tight"][0]).max()))
    # (e) euler_ode
    out["e_x"] = sde().euler_ode(z.clone(), m, N=3).numpy()
    path = os.path.join(OUT, "rf_sampler_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
