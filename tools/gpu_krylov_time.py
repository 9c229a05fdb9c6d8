"""Cost of the device GMRES inside OT-ODE's zero-boundary deblurring step, on the GPU (markdown to stdout and, with --out, to a file):

  * one OT-ODE Euler step (t = 0.5) of the 256^2 net at B = 32 from a device-event timing of one warm run: with the Krylov solve
    (problem gaussian_deblurring) and, beside it, the same step with the circular blur's Fourier solve (gaussian_deblurring_FFT), i.e.
    the step without a Krylov solve;
  * pf_krylov_solve alone on a right-hand side of that size (device events), its Krylov vector counts;
  * the multi-dot kernel's achieved bytes/s from a child `rocprofv3 --kernel-trace --stats` run of `--krylov-only` (bytes from the shapes
    and the per-image iteration counts: each launch of iteration j reads w and j + 1 basis vectors of every unfinished image), against
    the 6.3 TB/s streaming figure of the MI355X.

Synthetic seed-fixed weights and inputs: times, not restoration quality.  Nothing here is a pass mark.
Usage:  python tools/gpu_krylov_time.py [--out profiles/krylov_timing.md] [--batch 32] [--krylov-only]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
S, SIGMA, T_STEP = 256, 0.05, 0.5
PEAK_TBS = 6.3


def det_normal(shape, seed, idx=0):
    g = np.random.Generator(np.random.Philox(key=[seed, idx]))
    return torch.from_numpy(g.standard_normal(size=shape, dtype=np.float32))


def smooth(shape, seed):
    x = det_normal(shape, seed)
    k = torch.ones(shape[1], 1, 3, 3) / 9.0
    for _ in range(5):
        x = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), k, groups=shape[1])
    return (x / x.abs().amax(dim=(1, 2, 3), keepdim=True)).contiguous()


def build_afhq256():
    from oracle import pnpflow_oracle as O
    from pnpflow_amd.models import UNet
    c = dict(input_channels=3, input_height=S, ch=32, ch_mult=(1, 2, 4, 8), num_res_blocks=6, attn_resolutions=(16, 8))
    m = UNet(3, S, 32, ch_mult=c["ch_mult"], num_res_blocks=6, attn_resolutions=c["attn_resolutions"])
    m.load_state_dict(O.synthetic_state_dict(O.unet_config(**c), 0))
    return m


def event_ms(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream); out = fn(); b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), out


def krylov_alone(B, stream, timed=True):
    """pf_krylov_solve on a d-like right-hand side -> (ms of the second call, Krylov vectors per image)"""
    import pnpflow_amd._lib as L
    import pnpflow_amd.degradations as D
    lib = L.load()
    dg = D.GaussianDeblurring(3.0, 61, "spatial", 3, S)
    d = dg.descriptor(B, S, S, torch.device("cuda"))
    rhs = (0.3 * smooth((B, 3, S, S), 5) + SIGMA * det_normal((B, 3, S, S), 6)).cuda()
    rt2 = torch.full((B,), (1 - T_STEP) ** 2 / ((1 - T_STEP) ** 2 + T_STEP ** 2), device="cuda")
    nws = int(lib.pf_krylov_workspace_floats(B, 3, S, S, 100))
    ws = torch.empty(nws, device="cuda"); sol = torch.empty_like(rhs); iters = torch.zeros(B, dtype=torch.int32, device="cuda")

    def call():
        rc = lib.pf_krylov_solve(C.byref(d), rt2.data_ptr(), SIGMA ** 2, rhs.data_ptr(), sol.data_ptr(), B, 3, S, S, 100, 1e-6, 1e-6, ws.data_ptr(), nws,
                                 iters.data_ptr(), C.c_void_p(stream.cuda_stream))
        assert rc == 0, rc
    call(); stream.synchronize()
    ms = event_ms(call, stream)[0] if timed else float("nan")
    return ms, iters.cpu().numpy().tolist()


def ode_step(m, B, problem, stream):
    """ms of the single Euler step at t = 0.5 (steps_ode 2, start_time 0.5), second call (buffers, plans and lazy attributes in place)"""
    import pnpflow_amd.degradations as D
    from pnpflow_amd.methods.ot_ode import OT_ODE
    from pnpflow_amd.utils import CfgNode
    args = CfgNode(dict(method="ot_ode", model="ot", problem=problem, steps_ode=2, start_time=T_STEP, gamma="constant", max_batch=1, compute_time=False,
                        compute_memory=False, save_results=False, batch=0))
    s = OT_ODE(m, torch.device("cuda"), args)
    dg = D.GaussianDeblurring(3.0, 61, "spatial" if problem == "gaussian_deblurring" else "fft", 3, S)
    clean = smooth((B, 3, S, S), 7).cuda()
    y = dg.H(clean) + SIGMA * det_normal((B, 3, S, S), 8).cuda()
    s.init_noise = det_normal((B, 3, S, S), 9).cuda()
    s.restore_batch(y, dg, SIGMA); stream.synchronize()
    ms, _ = event_ms(lambda: s.restore_batch(y, dg, SIGMA), stream)
    return ms, s.last_krylov_iterations


def multidot_rate(B):
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.isfile(exe):
        return ["Multi-dot kernel: rocprofv3 not found on this box; not measured.", ""]
    tmp = tempfile.mkdtemp(prefix="krylov_trace_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--krylov-only",
                            "--batch", str(B)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("KRYLOV_ITERS ")]
        if r.returncode != 0 or not files or not line:
            return [f"Multi-dot kernel: the rocprofv3 run gave no kernel trace (exit {r.returncode}); not measured.", ""]
        iters = json.loads(line[0].split(" ", 1)[1])
        ns, calls = {}, {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                for key in ("krylov_multidot", "krylov_update", "blur2d_fused", "krylov_"):
                    if key in name:
                        ns[key] = ns.get(key, 0.0) + float(int(row["End_Timestamp"]) - int(row["Start_Timestamp"])); calls[key] = calls.get(key, 0) + 1
                        break
        n = 3 * S * S
        # the child runs the solve twice (warm-up + one more): both are in the trace
        byt = 2 * sum(2 * (j + 2) * n * 4 for k in iters for j in range(k))
        t = ns.get("krylov_multidot", 0.0) * 1e-9
        if t <= 0:
            return ["Multi-dot kernel: no krylov_multidot_kernel row in the trace; not measured.", ""]
        upd = ns.get("krylov_update", 0.0) * 1e-9
        return [f"**Multi-dot kernel** (`rocprofv3 --kernel-trace --stats -- python tools/gpu_krylov_time.py --krylov-only --batch {B}`, two solves, Krylov vectors per "
                f"image {min(iters)} ... {max(iters)}): {calls['krylov_multidot']} launches, {t * 1e3:.2f} ms, {byt / 1e9:.1f} GB read (w + the basis, from the shapes) = "
                f"**{byt / t / 1e12:.2f} TB/s, {100 * byt / t / 1e12 / PEAK_TBS:.0f} % of the {PEAK_TBS} TB/s streaming figure**.  Fused update (same reads + one write of "
                f"w): {upd * 1e3:.2f} ms; the blur passes of the operator: {ns.get('blur2d_fused', 0.0) / 1e6:.2f} ms; the other Krylov kernels: {ns.get('krylov_', 0.0) / 1e6:.2f} ms.", ""]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--krylov-only", action="store_true")
    a = ap.parse_args()
    B = a.batch
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        if a.krylov_only:
            _, iters = krylov_alone(B, stream)
            print("KRYLOV_ITERS " + json.dumps(iters))
            return
        ms_k, iters = krylov_alone(B, stream)
        m = build_afhq256()
        ms_fft, _ = ode_step(m, B, "gaussian_deblurring_FFT", stream)
        ms_zero, kr = ode_step(m, B, "gaussian_deblurring", stream)
    n = 3 * S * S
    out = [f"# Device GMRES in OT-ODE's zero-boundary deblurring step: 256^2 net, B = {B}, blur sigma 3 (43 visible taps), noise sigma {SIGMA}, t = {T_STEP}", "",
           "Device-event timings of one warm run each (not gated; synthetic weights and images).", "",
           "| | ms |", "|---|---|",
           f"| one Euler step, zero-boundary blur: forward + d + GMRES(100, 1e-6) + H_adj + backward + update ({kr} Krylov iterations enqueued) | {ms_zero:.1f} |",
           f"| one Euler step, circular blur (Fourier solve in place of the Krylov solve) | {ms_fft:.1f} |",
           f"| difference | {ms_zero - ms_fft:.1f} |",
           f"| pf_krylov_solve alone on a right-hand side of that size (Krylov vectors per image {min(iters)} ... {max(iters)}) | {ms_k:.1f} |", "",
           f"Basis of the solve: 101 x {B} x 3 x 256 x 256 floats = {101 * B * n * 4 / 1e9:.2f} GB.", ""]
    out += multidot_rate(B)
    txt = "\n".join(out) + "\n"
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
