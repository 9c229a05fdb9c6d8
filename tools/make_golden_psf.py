"""Fixtures of the point-spread-function blur (PF_DEG_PSF_BLUR / PF_DEG_PSF_BLUR_ZERO) from the REAL reference on the CPU.

Run in the build container only:   python tools/make_golden_psf.py [op] [pnp] [ot_ode] [pnp_gs]
Writes data only, under tests/golden/.  The operator is the reference's own GaussianDeblurring object with `.kernel` and `.filter` overwritten by the
PSF (its H / H_adj and every solver loop read nothing else).  In the zero mode the reference's H_adj is F.conv2d with the kernel again, which is not
the adjoint of H for an asymmetric kernel; the object's H_adj is replaced by the zero-boundary convolution (conv2d with the kernel turned by 180
degrees) before the reference's loops run.  The loops themselves are the generators of tools/make_golden.py, tools/make_golden_spatial.py and
tools/make_golden_pnp_gs.py, handed a degradations module whose GaussianDeblurring builds that object; every fixture also stores the PSF.

  psf_op.npz                       H and H_adj of image 0 of det_image at 2 x 3 x 64 x 64, both modes, psf_restatement.psf_kernel(K) for K = 9 and 21
  pnp_traj_psf_fft.npz             PNP_FLOW.solve_ip, tiny4, 10 x 2, Gaussian noise, circular; iterates 0 / 1 / 4 / 9
  pnp_traj_laplace_psf_zero.npz    the same with Laplace noise, zero boundary
  ot_ode_traj_psf_fft.npz          OT_ODE.solve_ip, tiny4, B = 2, 10 steps: the Fourier branch (problem gaussian_deblurring_FFT)
  ot_ode_traj_psf_zero.npz         the generic GMRES branch, with the Krylov vectors of every solve (below the cap of 100: asserted)
  pnp_gs_tiny4_hqs_psf_fft.npz     PROX_PNP.solve_ip, hqs, circular, in the format of pnp_gs_tiny4_hqs_gaussian_deblurring_FFT.npz (with `growth`)
The solver fixtures use the camera-shake kernel pnpflow_amd.psf.motion_psf(21, 0); ot_ode_traj_psf_zero.npz uses motion_psf(21, 1) (see KRYLOV_PSF).
"""
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden as MG  # noqa: E402
import make_golden_spatial as MS  # noqa: E402
from make_golden import OUT, det_image  # noqa: E402
import psf_restatement as P  # noqa: E402
from pnpflow_amd.psf import motion_psf  # noqa: E402

SOLVER_PSF = motion_psf(21, 0)
# the GMRES fixture alone uses seed 1: with the seed-0 kernel one of the reference's fp32 solves (step 2, image 0) runs into the cap of 100 vectors
# while its neighbours stop at about 30, and a capped solve is not a result the engine can be held to
KRYLOV_PSF = motion_psf(21, 1)


def psf_object(degr, kernel, mode, num_channels, dim_image):
    """the reference's GaussianDeblurring carrying `kernel`; mode "fft" or anything else (zero boundary, true adjoint)"""
    K = kernel.shape[0]
    d = degr.GaussianDeblurring(1.0, K, mode, num_channels, dim_image, "cpu")
    k = torch.from_numpy(np.ascontiguousarray(kernel, dtype=np.float32)).view(1, 1, K, K)
    f = torch.zeros((1, num_channels, dim_image, dim_image))
    f[..., :K, :K] = k
    d.kernel, d.filter = k, torch.roll(f, shifts=(-(K - 1) // 2, -(K - 1) // 2), dims=(2, 3))      # degradations.py:61-68
    if mode != "fft":
        def conv_adjoint(x, d=d):
            kk = torch.flip(d.kernel, dims=(2, 3)).to(x.dtype).repeat(x.shape[1], 1, 1, 1)
            return F.conv2d(x, kk, stride=1, padding="same", groups=x.shape[1])
        d.H_adj = conv_adjoint
    return d


def degr_with(degr, kernel, mode):
    """a stand-in for the reference's degradations module: GaussianDeblurring(...) builds the PSF object in `mode`, whatever the generator asks for"""
    ns = types.SimpleNamespace(**{n: getattr(degr, n) for n in dir(degr) if not n.startswith("_")})
    ns.GaussianDeblurring = lambda sigma, K, m="fft", num_channels=3, dim_image=128, device="cpu": psf_object(degr, kernel, mode, num_channels, dim_image)
    return ns


def rehome(tmp, name, new, extra):
    """tmp/name -> OUT/new with `extra` arrays added"""
    g = np.load(os.path.join(tmp, name))
    rec = {k: g[k] for k in g.files}
    rec.update(extra)
    path = os.path.join(OUT, new)
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) <= 460 * 1024, (new, os.path.getsize(path))
    print(new, os.path.getsize(path), "bytes")


def with_out(modules, fn):
    """run fn() with the generators' output folder pointed at a scratch folder; returns that folder"""
    tmp = tempfile.mkdtemp()
    saved = [m.OUT for m in modules]
    for m in modules:
        m.OUT = tmp
    try:
        fn()
    finally:
        for m, o in zip(modules, saved):
            m.OUT = o
    return tmp


def gen_op(degr):
    x = det_image((2, 3, 64, 64), 31)[:1]            # one image: eight outputs stay below the size of the other fixtures
    rec = {}
    for K in (9, 21):
        k = P.psf_kernel(K)
        rec[f"psf{K}"] = k
        for mode in ("fft", "zero"):
            d = psf_object(degr, k, "fft" if mode == "fft" else "spatial", 3, 64)
            rec[f"k{K}_{mode}_H"] = d.H(x).numpy(); rec[f"k{K}_{mode}_Hadj"] = d.H_adj(x).numpy()
            # the pair is adjoint, and is what the fp64 direct sums say
            w = x.flip(0)
            lhs, rhs = float((d.H(x).double() * w.double()).sum()), float((x.double() * d.H_adj(w).double()).sum())
            assert abs(lhs - rhs) <= 1e-5 * float((d.H(x) * w).abs().sum()), (K, mode, lhs, rhs)
            for adj, key in ((False, "H"), (True, "Hadj")):
                err = float(np.abs(rec[f"k{K}_{mode}_{key}"] - P.apply64(x.numpy(), k, mode == "zero", adj)).max())
                assert err < 5e-6, (K, mode, key, err)
    rehome_path = os.path.join(OUT, "psf_op.npz")
    np.savez_compressed(rehome_path, **rec)
    assert os.path.getsize(rehome_path) <= 460 * 1024
    print("psf_op.npz", os.path.getsize(rehome_path), "bytes")


def gen_pnp(models, degr, utils, pnp):
    extra = dict(psf=SOLVER_PSF)
    tmp = with_out([MS], lambda: MS.gen_pnp(models, degr_with(degr, SOLVER_PSF, "fft"), utils, pnp))
    rehome(tmp, "pnp_traj_zero_blur.npz", "pnp_traj_psf_fft.npz", extra)                      # the generator's Gaussian-noise case, circular operator
    shutil.rmtree(tmp)
    tmp = with_out([MS], lambda: MS.gen_pnp(models, degr_with(degr, SOLVER_PSF, "spatial"), utils, pnp))
    rehome(tmp, "pnp_traj_laplace_zero_blur.npz", "pnp_traj_laplace_psf_zero.npz", extra)      # its Laplace case, zero boundary
    shutil.rmtree(tmp)


def gen_ot_ode(models, degr, utils):
    extra = dict(psf=SOLVER_PSF)
    tmp = with_out([MG], lambda: MG.gen_ot_ode(models, degr_with(degr, SOLVER_PSF, "fft"), utils, only=["tiny4_gaussian_deblurring_FFT"]))
    rehome(tmp, "ot_ode_traj_tiny4_gaussian_deblurring_FFT.npz", "ot_ode_traj_psf_fft.npz", extra)
    shutil.rmtree(tmp)
    tmp = with_out([MS], lambda: MS.gen_ot_ode(models, degr_with(degr, KRYLOV_PSF, "spatial"), utils))      # asserts 0 < Krylov vectors < 100
    rehome(tmp, "ot_ode_traj_zero_blur.npz", "ot_ode_traj_psf_zero.npz", dict(psf=KRYLOV_PSF))
    shutil.rmtree(tmp)


def gen_pnp_gs(models, degr, utils):
    import make_golden_pnp_gs as PG
    all_cases = PG.cases
    proxy = degr_with(degr, SOLVER_PSF, "fft")
    PG.cases = lambda _degr, S: [c for c in all_cases(proxy, S) if c[0] == "hqs_gaussian_deblurring_FFT"]
    try:
        tmp = with_out([PG], lambda: PG.gen(models, proxy, utils))
    finally:
        PG.cases = all_cases
    rehome(tmp, "pnp_gs_tiny4_hqs_gaussian_deblurring_FFT.npz", "pnp_gs_tiny4_hqs_psf_fft.npz", dict(psf=SOLVER_PSF))
    shutil.rmtree(tmp)


if __name__ == "__main__":
    which = sys.argv[1:] or ["op", "pnp", "ot_ode", "pnp_gs"]
    os.makedirs(OUT, exist_ok=True)
    models, degr, utils, pnp = MG.import_reference()
    if "op" in which:
        gen_op(degr)
    if "pnp" in which:
        gen_pnp(models, degr, utils, pnp)
    if "ot_ode" in which:
        gen_ot_ode(models, degr, utils)
    if "pnp_gs" in which:
        gen_pnp_gs(models, degr, utils)
