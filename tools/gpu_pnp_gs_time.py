"""Prox-PnP (method pnp_gs) timing on the GPU; writes profiles/pnp_gs_timing.md with --out:

  * ms per iteration of pf_pnp_gs_restore (graph-replayed and with direct launches) at the celeba 128^2 net, B = 16, for pgd box
    inpainting and hqs gaussian_deblurring_FFT, beside the bare pf_unet_vjp (retained forward + backward) at the same shape measured
    in the same process;
  * the glue kernels' share of kernel time from one `rocprofv3 --kernel-trace --stats` run of this script with --iterations-only
    (started here as a child process; the program goes after `--`);
  * the largest error / TOL ratio of the teacher-forced parity tests (tests/test_gpu_pnp_gs.py prints one line per case), from a
    child pytest run.

Synthetic seed-fixed weights (the oracle's recipe) and inputs: times, not restoration quality.
Usage:  python tools/gpu_pnp_gs_time.py [--out profiles/pnp_gs_timing.md] [--no-trace] [--no-parity] [--iterations-only]
"""
import argparse
import csv
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile
from time import perf_counter

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, S, ITERS = 16, 128, 12
GLUE = ("pnpgs_", "fft_rows", "fft_cols", "blur_power_spectrum", "grad_step", "bump_iter", "blur2d", "blur_rows", "blur_cols", "mask_apply", "::fill_kernel")       # kernels that are not the U-Net's


def det_normal(shape, seed, idx=0):
    g = np.random.Generator(np.random.Philox(key=[seed, idx]))
    return torch.from_numpy(g.standard_normal(size=shape, dtype=np.float32))


def build_celeba128():
    from oracle import pnpflow_oracle as O
    from pnpflow_amd.models import UNet
    c = dict(input_channels=3, input_height=S, ch=32, ch_mult=(1, 2, 4, 8), num_res_blocks=6, attn_resolutions=(16, 8))
    m = UNet(3, S, 32, ch_mult=c["ch_mult"], num_res_blocks=6, attn_resolutions=c["attn_resolutions"])
    m.load_state_dict(O.synthetic_state_dict(O.unet_config(**c), 0))
    return m


def solver(m, algo, problem):
    from pnpflow_amd.methods.pnp_gs import PROX_PNP
    from pnpflow_amd.train_denoiser import GRADIENT_STEP_DENOISER
    from pnpflow_amd.utils import CfgNode
    args = CfgNode(dict(method="pnp_gs", model="gradient_step", problem=problem, noise_type="gaussian", algo=algo, max_iter=ITERS, lr_pnp=1.0, alpha=0.5,
                        sigma_factor=1.0, max_batch=1, compute_time=False, compute_memory=False, save_results=False, batch=0, dim_image=S, num_channels=3))
    return PROX_PNP(GRADIENT_STEP_DENOISER(m, torch.device("cuda"), args), torch.device("cuda"), args)


def configs():
    import pnpflow_amd.degradations as D
    return [("pgd, box inpainting", "pgd", "inpainting", D.BoxInpainting(20), 0.05),
            ("hqs, gaussian_deblurring_FFT", "hqs", "gaussian_deblurring_FFT", D.GaussianDeblurring(1.0, 61, "fft", 3, S), 0.05)]


def ms_per_iteration(s, y, dg, sigma, x0):
    """One warm-up call (captures the graph), then `reps` calls of ITERS iterations, each restarted from x0."""
    run = lambda: s.restore_batch(y, dg, sigma, x0=x0)
    run(); torch.cuda.synchronize()
    reps = 3
    t0 = perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    return (perf_counter() - t0) / (reps * ITERS) * 1e3


def damped(m):
    """The synthetic net is no contraction: ITERS free iterations overflow.  alpha tiny keeps every iterate near x0 (pgd: x = z - alpha Dg;
    hqs deblurring: the prox input scales with alpha) without changing a single launch."""
    return 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iterations-only", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-parity", action="store_true")
    a = ap.parse_args()
    m = build_celeba128()
    y = (det_normal((B, 3, S, S), 1).clamp(-3, 3) * 0.3).cuda()
    if a.iterations_only:
        for label, algo, problem, dg, sigma in configs():
            s = solver(m, algo, problem); s.args.alpha = damped(m)
            for _ in range(2):
                s.restore_batch(y, dg, sigma, x0=y)
        torch.cuda.synchronize()
        print("iterations done")
        return
    t = torch.full((B,), 0.05, device="cuda")
    vec = det_normal((B, 3, S, S), 2).cuda()
    m.vjp(y, t, vec); torch.cuda.synchronize()
    t0 = perf_counter()
    for _ in range(10):
        m.vjp(y, t, vec)
    torch.cuda.synchronize()
    ms_vjp = (perf_counter() - t0) / 10 * 1e3
    rows = []
    for label, algo, problem, dg, sigma in configs():
        s = solver(m, algo, problem); s.args.alpha = damped(m)
        ms_g = ms_per_iteration(s, y, dg, sigma, y)
        s.use_graph = False
        ms_e = ms_per_iteration(s, y, dg, sigma, y)
        rows.append((label, ms_g, ms_e))
    m.check_numerics()
    out = [f"# Prox-PnP (method pnp_gs) timing", "",
           f"Device: {torch.cuda.get_device_name(0)} ({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')}).  Net: celeba 128^2 U-Net (ch 32, ch_mult 1 2 4 8, 6 residual blocks per level), synthetic seed-fixed weights,",
           f"precision mode 1 (default), B = {B}, {ITERS} iterations per call, alpha 1e-6 (the synthetic net is no contraction; the launches are the same).",
           "`python tools/gpu_pnp_gs_time.py` (host clock around calls that end in a device synchronise; one capture / warm-up call, then 3 calls).", "",
           f"Bare `pf_unet_vjp` (retained forward + backward) at the same shape, same process: **{ms_vjp:.2f} ms**.", "",
           "| configuration | ms / iteration (graph replay) | ms / iteration (direct launches) | graph / bare VJP |", "|---|---|---|---|"]
    for label, ms_g, ms_e in rows:
        out.append(f"| {label} | {ms_g:.2f} | {ms_e:.2f} | {ms_g / ms_vjp:.3f} |")
    out.append("")
    if not a.no_trace:
        out += trace_section()
    if not a.no_parity:
        out += parity_section()
    txt = "\n".join(out) + "\n"
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt)


def trace_section():
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.isfile(exe):
        return ["Kernel trace: rocprofv3 not found on this box; no share recorded.", ""]
    tmp = tempfile.mkdtemp(prefix="pnp_gs_trace_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
                            "--iterations-only"], cwd=ROOT, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return [f"Kernel trace: the rocprofv3 run did not produce kernel statistics (exit {r.returncode}); no share recorded.", ""]
        total, glue, names = 0.0, 0.0, {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                ns = float(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
                name = row.get("Kernel_Name", "")
                total += ns
                if any(k in name for k in GLUE):
                    glue += ns
                    key = re.sub(r"<.*|\(.*", "", name.replace("(anonymous namespace)::", "").replace("void ", "")).replace("pf::", "")
                    names[key] = names.get(key, 0.0) + ns
        lines = ["**Kernel trace** (`rocprofv3 --kernel-trace --stats -- python tools/gpu_pnp_gs_time.py --iterations-only`: both configurations, "
                 f"2 calls of {ITERS} iterations each; no counters in that run):", "",
                 "| | ms | share of kernel time |", "|---|---|---|", f"| all kernels | {total / 1e6:.1f} | 100 % |",
                 f"| glue (everything that is not the U-Net's forward / backward) | {glue / 1e6:.2f} | **{100 * glue / max(total, 1):.2f} %** |"]
        for k, v in sorted(names.items(), key=lambda kv: -kv[1]):
            lines.append(f"| `{k}` | {v / 1e6:.3f} | {100 * v / max(total, 1):.3f} % |")
        return lines + [""]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def parity_section():
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_pnp_gs.py"), "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider",
                        "-k", "teacher_forced"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    ratios = [(float(mm.group(4)), mm.group(1), int(mm.group(2)), int(mm.group(3))) for mm in re.finditer(r"PNP_GS_RATIO (\S+) (\d) (\d) ([0-9.eE+-]+)", r.stdout)]
    if not ratios:
        return [f"Teacher-forced parity: the pytest run printed no ratio (exit {r.returncode}); nothing recorded.", ""]
    worst = max(ratios)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    return [f"**Teacher-forced parity** (tests/test_gpu_pnp_gs.py, {len(ratios)} single iterations against the real reference's goldens, precision modes 0 and 1): "
            f"largest max|err| / TOL = **{worst[0]:.3f}** ({worst[1]}, iteration {worst[2]}, mode {worst[3]}); pytest: `{tail}`.", ""]


if __name__ == "__main__":
    main()
