"""Timing of the point-spread-function blur on the GPU; writes profiles/psf_timing.md with --out.  Not gated by any test.

At 256 x 256, B = 32, C = 3, by device events after warm-up (median of REPS calls through the C ABI):
  * pf_grad_step (two applications of psf2d_kernel) with a K x K PSF for K = 9 / 31 / 61: ms, GFLOP/s and GB/s from the shapes (2 x 2 K^2 flops per
    pixel; six tensors of algorithmic traffic: x, y in and r out, then r, x in and z out), and which of the two lower bounds - fp32 vector
    peak 157.3 TFLOP/s, HBM peak 8 TB/s (datasheet values) - is the larger one;
  * beside it the separable Gaussian kind on the 61 taps g, and the PSF kind on outer(g, g): the same operator both ways;
  * the linear solve of one OT-ODE Euler step (pf_ot_ode_vec: x1_hat, H, three FFT launches, H_adj) with the PSF's 2-D spectrum table beside the
    Gaussian's separable one, K = 61 both, and pf_psf_power_spectrum alone (the engine's loop computes the table once per call, pf_ot_ode_vec on
    every call).
Seed-fixed inputs: times, not restoration quality.
Usage:  python tools/gpu_psf_time.py [--out profiles/psf_timing.md]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, CH, S = 32, 3, 256
WARM, REPS = 3, 11
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12


def det_normal(shape, seed, idx=0):
    g = np.random.Generator(np.random.Philox(key=[seed, idx]))
    return torch.from_numpy(g.standard_normal(size=shape, dtype=np.float32))


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pnpflow_amd._lib as L
    import pnpflow_amd.degradations as D
    from pnpflow_amd.psf import motion_psf
    lib = L.load()
    shape = (B, CH, S, S)
    n = int(np.prod(shape))
    x, y = det_normal(shape, 1).cuda(), det_normal(shape, 2).cuda()
    vt = det_normal(shape, 3).cuda()
    z = torch.empty_like(x)
    coef = torch.full((B,), 0.5, device="cuda")
    omt, rt2 = torch.full((B,), 0.6, device="cuda"), torch.full((B,), 0.4, device="cuda")
    scr = torch.empty(4 * n + S * S, device="cuda")
    st = L.current_stream_ptr()

    def desc(kind, taps):
        t = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float32)).cuda()
        d = L.PfDegradation(); d.kind = kind; d.ntaps = int(taps.shape[0]); d.taps = t.data_ptr()
        return d, t

    def grad_step(d):
        def call():
            rc = lib.pf_grad_step(C.byref(d), x.data_ptr(), y.data_ptr(), coef.data_ptr(), z.data_ptr(), B, CH, S, S, scr.data_ptr(), st)
            assert rc == 0, rc
        return call

    def vec(d):
        def call():
            rc = lib.pf_ot_ode_vec(C.byref(d), x.data_ptr(), vt.data_ptr(), y.data_ptr(), omt.data_ptr(), rt2.data_ptr(), 0.0025, z.data_ptr(), B, CH, S, S, scr.data_ptr(), st)
            assert rc == 0, rc
        return call

    rows = []

    def row(label, K, ms, taps_per_pixel):
        flops = 2.0 * 2.0 * taps_per_pixel * n            # two applications, one multiply-add per tap
        byts = 6.0 * n * 4
        t_f, t_b = flops / PEAK_FLOPS * 1e3, byts / PEAK_BYTES * 1e3
        rows.append(f"| {label} | {K} | {ms:.3f} | {flops / ms / 1e6:.0f} | {byts / ms / 1e6:.0f} | {'VALU' if t_f > t_b else 'HBM'} ({max(t_f, t_b):.3f} ms) |")

    for K in (9, 31, 61):
        d, keep = desc(L.PF_DEG_PSF_BLUR, motion_psf(K, 0))
        row("PSF, camera shake", K, timed(grad_step(d)), K * K)
    g = D.GaussianDeblurring(3.0, 61, "fft").taps_host
    d, keep = desc(L.PF_DEG_PSF_BLUR, np.outer(g, g))
    row("PSF, outer(g, g) of the sigma-3 Gaussian", 61, timed(grad_step(d)), 61 * 61)
    d4, keep4 = desc(L.PF_DEG_GAUSSIAN_BLUR, g)
    row("separable Gaussian kind, the same g", 61, timed(grad_step(d4)), 2 * 61)

    solve = []
    d7, keep7 = desc(L.PF_DEG_PSF_BLUR, motion_psf(61, 0))
    solve.append(f"| pf_ot_ode_vec, PSF (2-D spectrum table, computed in the call) | {timed(vec(d7)):.3f} |")
    solve.append(f"| pf_ot_ode_vec, separable Gaussian, 61 taps | {timed(vec(d4)):.3f} |")
    pw = torch.empty(S * S, device="cuda")

    def spectrum():
        assert lib.pf_psf_power_spectrum(C.byref(d7), S, S, pw.data_ptr(), st) == 0
    solve.append(f"| pf_psf_power_spectrum alone (once per engine-loop call) | {timed(spectrum):.3f} |")

    text = "\n".join([
        "# Point-spread-function blur: timing", "",
        f"`python tools/gpu_psf_time.py --out profiles/psf_timing.md` on {torch.cuda.get_device_name(0)}; {B} x {CH} x {S} x {S}, device events, median of {REPS} calls after"
        f" {WARM} warm-up calls.  GFLOP/s and GB/s are computed from the shapes (see the tool's header), the bound is the larger of the two lower bounds at the"
        " datasheet peaks.", "",
        "## pf_grad_step (two operator applications)", "",
        "| operator | K | ms | GFLOP/s | GB/s | larger lower bound |", "|---|---|---|---|---|---|", *rows, "",
        "## The solve of one OT-ODE Euler step", "",
        "| call | ms |", "|---|---|", *solve, ""])
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
