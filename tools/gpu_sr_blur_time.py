"""Timing of superresolution through a blur kernel (PF_DEG_PSF_SR) on the GPU; writes profiles/sr_blur_timing.md with --out.  Not gated by any test.

At 256 x 256, B = 32, C = 3, K in {9, 31, 61}, sf in {2, 4}, by device events after warm-up.  One sample is CALLS back-to-back calls through the C ABI
between one pair of events, divided by CALLS - the queue stays full, so a sample is kernel time, not the launch latency of a call that finds the GPU idle
(which would weigh differently on the one-launch and the two-launch forms) - and a figure is the median of REPS samples; the largest spread (max - min) / median
over any figure's samples is written into the file.  Timed:
  * pf_grad_step of kind 9 (psf_sr_fwd_kernel with the residual epilogue, then psf_sr_adj_kernel with the update epilogue),
  * one pf_ot_ode_vec of kind 9 (x1_hat, H, the aliased spectrum, three FFT launches on the low-resolution grid, H_adj),
  * the aliased spectrum alone (pf_sr_aliased_spectrum: the full-resolution table, then the fold; the engine's loops compute it once per call),
each beside what the library could already do for the same result before the kind existed: the PF_DEG_PSF_BLUR kernel at full resolution, then the
decimation kernel (PF_DEG_SUPERRESOLUTION's H), and for the adjoint the zero-fill kernel, then PF_DEG_PSF_BLUR's H_adj - four launches per gradient
step without its residual / update passes, so the comparison favours the old form.  The fused kernels do 1 / sf^2 of its multiply-adds.
Seed-fixed inputs: times, not restoration quality.
Usage:  python tools/gpu_sr_blur_time.py [--out profiles/sr_blur_timing.md]
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
WARM, REPS, CALLS = 3, 11, 50


def det_normal(shape, seed, idx=0):
    g = np.random.Generator(np.random.Philox(key=[seed, idx]))
    return torch.from_numpy(g.standard_normal(size=shape, dtype=np.float32))


SPREAD = []      # (max - min) / median of every figure's samples


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / CALLS)
    med = float(np.median(ms))
    SPREAD.append((max(ms) - min(ms)) / med)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pnpflow_amd._lib as L
    from pnpflow_amd.psf import motion_psf
    lib = L.load()
    shape = (B, CH, S, S)
    n = int(np.prod(shape))
    x, vt = det_normal(shape, 1).cuda(), det_normal(shape, 3).cuda()
    z, full = torch.empty_like(x), torch.empty_like(x)
    coef = torch.full((B,), 0.5, device="cuda")
    omt, rt2 = torch.full((B,), 0.6, device="cuda"), torch.full((B,), 0.4, device="cuda")
    st = L.current_stream_ptr()
    rows, wins = [], True
    for sf in (2, 4):
        low = (B, CH, S // sf, S // sf)
        y, r = det_normal(low, 2).cuda(), torch.empty(low, device="cuda")
        scr = torch.empty(int(lib.pf_sr_solve_scratch_floats(B, CH, S, S, sf)), device="cuda")
        lam = torch.empty((S // sf) * (S // sf), device="cuda")
        for K in (9, 31, 61):
            taps = torch.from_numpy(motion_psf(K, 0)).cuda()

            def desc(kind):
                d = L.PfDegradation(); d.kind = kind; d.sf = sf; d.ntaps = K; d.taps = taps.data_ptr()
                return d
            d9, d7, d3 = desc(L.PF_DEG_PSF_SR), desc(L.PF_DEG_PSF_BLUR), desc(L.PF_DEG_SUPERRESOLUTION)

            def grad():
                assert lib.pf_grad_step(C.byref(d9), x.data_ptr(), y.data_ptr(), coef.data_ptr(), z.data_ptr(), B, CH, S, S, scr.data_ptr(), st) == 0

            def fwd():
                assert lib.pf_degradation_H(C.byref(d9), x.data_ptr(), r.data_ptr(), B, CH, S, S, None, st) == 0

            def adj():
                assert lib.pf_degradation_H_adj(C.byref(d9), y.data_ptr(), z.data_ptr(), B, CH, S, S, None, st) == 0

            def old_fwd():       # blur at full resolution, then decimate
                assert lib.pf_degradation_H(C.byref(d7), x.data_ptr(), full.data_ptr(), B, CH, S, S, None, st) == 0
                assert lib.pf_degradation_H(C.byref(d3), full.data_ptr(), r.data_ptr(), B, CH, S, S, None, st) == 0

            def old_adj():       # zero-fill, then the correlation at full resolution
                assert lib.pf_degradation_H_adj(C.byref(d3), y.data_ptr(), full.data_ptr(), B, CH, S, S, None, st) == 0
                assert lib.pf_degradation_H_adj(C.byref(d7), full.data_ptr(), z.data_ptr(), B, CH, S, S, None, st) == 0

            def vec():
                assert lib.pf_ot_ode_vec(C.byref(d9), x.data_ptr(), vt.data_ptr(), y.data_ptr(), omt.data_ptr(), rt2.data_ptr(), 0.0025, z.data_ptr(), B, CH, S, S,
                                         scr.data_ptr(), st) == 0

            def spectrum():
                assert lib.pf_sr_aliased_spectrum(C.byref(d9), S, S, lam.data_ptr(), scr.data_ptr(), st) == 0
            t = {name: timed(fn) for name, fn in (("grad", grad), ("fwd", fwd), ("adj", adj), ("old_fwd", old_fwd), ("old_adj", old_adj), ("vec", vec),
                                                  ("spectrum", spectrum))}
            wins = wins and t["fwd"] < t["old_fwd"] and t["adj"] < t["old_adj"] and t["grad"] < t["old_fwd"] + t["old_adj"]
            gflops = 2.0 * 2.0 * K * K * n / (sf * sf) / t["grad"] / 1e6        # both kernels: K^2 / sf^2 multiply-adds per full-resolution pixel
            rows.append(f"| {sf} | {K} | {t['grad']:.3f} | {gflops:.0f} | {t['fwd']:.3f} | {t['old_fwd']:.3f} | {t['adj']:.3f} | {t['old_adj']:.3f} | {t['vec']:.3f} |"
                        f" {t['spectrum']:.3f} |")
    verdict = ("The fused forward, the polyphase adjoint and the gradient step are faster than blur-at-full-resolution + decimation / zero-fill + correlation at "
               "every point of the table." if wins else
               "NOT every point of the table is a win for the fused kernels over blur-at-full-resolution + decimation / zero-fill + correlation: see the rows "
               "where a fused time is not below its neighbour.")
    text = "\n".join([
        "# Superresolution through a blur kernel: timing", "",
        f"`python tools/gpu_sr_blur_time.py --out profiles/sr_blur_timing.md` on {torch.cuda.get_device_name(0)}; {B} x {CH} x {S} x {S}, camera-shake PSF, device events,"
        f" median of {REPS} samples of {CALLS} back-to-back calls each (ms per call) after {WARM} warm-up calls; the largest (max - min) / median over the samples of any figure"
        f" below is {max(SPREAD) * 100:.1f} %.  `H` / `H_adj`: one launch of kind 9; `old`: PF_DEG_PSF_BLUR at full resolution followed by the decimation"
        " kernel, resp. the zero-fill kernel followed by PF_DEG_PSF_BLUR's adjoint (two launches, a full-resolution tensor in between).  GFLOP/s of pf_grad_step from the"
        " shapes: 2 x 2 K^2 / sf^2 flops per full-resolution pixel.", "",
        "| sf | K | pf_grad_step ms | GFLOP/s | H ms | old H ms | H_adj ms | old H_adj ms | pf_ot_ode_vec ms | aliased spectrum ms |",
        "|---|---|---|---|---|---|---|---|---|---|", *rows, "", verdict, ""])
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
