"""Timing of the FID Inception network on the GPU; writes profiles/fid_timing.md with --out.  Not gated by any test.

The work of one half of a `compute_metrics` run: N images (default 5 000) at 299 x 299 in batches of 50 through output block 3 (2048
features), by device events after a warm-up batch:
  * total time, images per second and the achieved fp32 TFLOP/s (2 M K Cout of every conv launch over the time of the whole forward;
    the datasheet's fp32 matrix peak is 157.3 TFLOP/s);
  * one profiled batch: the share of time per launch group (the stem layers, every Mixed block, the pools) and the ten slowest convs with
    their own TFLOP/s.
Seed-fixed synthetic weights and images: times, not a FID.
Usage:  python tools/gpu_fid_time.py [--images 5000] [--batch 50] [--side 299] [--out profiles/fid_timing.md]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--side", type=int, default=299)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from pnpflow_amd.models import InceptionV3
    from tools.synthetic_inception import synthetic_inception_state_dict
    net = InceptionV3([3], resize_input=a.side != 299).load_state_dict(synthetic_inception_state_dict(InceptionV3.state_dict_shapes()))
    g = np.random.Generator(np.random.Philox(key=[3, 0]))
    x = torch.from_numpy(g.uniform(0, 1, (a.batch, 3, a.side, a.side)).astype(np.float32)).cuda()

    net.profile(True)
    net.features(x, 3)                                  # warm-up, and the per-launch times of one batch
    net.features(x, 3)
    prof = net.profile_read()
    net.profile(False)
    flops_batch = sum(f for _n, _ms, f in prof)
    nb = a.images // a.batch
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(nb):
        net.features(x, 3)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1)
    tf = flops_batch * nb / (ms * 1e-3) / 1e12

    lines = ["# FID Inception network: time of one image set", "",
             f"{nb * a.batch} images at {a.side} x {a.side}, batches of {a.batch}, output block 3 (2048 features), synthetic weights; `python tools/gpu_fid_time.py`.", "",
             f"* total {ms / 1e3:.2f} s, {nb * a.batch / (ms * 1e-3):.0f} images/s, {ms / nb:.1f} ms per batch",
             f"* {flops_batch / a.batch / 1e9:.2f} GFLOP per image in the convs ({flops_batch * nb / 1e12:.1f} TFLOP in all): {tf:.1f} TFLOP/s fp32 achieved over the whole forward, "
             f"{100 * tf * 1e12 / PEAK_FLOPS:.0f} % of the {PEAK_FLOPS / 1e12:.1f} TFLOP/s fp32 matrix peak", ""]
    total = sum(m for _n, m, _f in prof)
    groups = {}
    for n, m, f in prof:
        key = n.split(".")[0] if "." in n else ("stem" if n.startswith("Conv2d") else n)
        gm, gf = groups.get(key, (0.0, 0.0))
        groups[key] = (gm + m, gf + f)
    lines += ["One profiled batch (device events around every launch; the sum of the launches is " + f"{total:.1f} ms):", "", "| group | ms | share | TFLOP/s |", "|---|---|---|---|"]
    for k, (m, f) in groups.items():
        lines.append(f"| {k} | {m:.2f} | {100 * m / total:.1f} % | {f / (m * 1e-3) / 1e12 if f else 0:.1f} |")
    lines += ["", "The ten slowest launches:", "", "| launch | ms | share | TFLOP/s |", "|---|---|---|---|"]
    for n, m, f in sorted(prof, key=lambda r: -r[1])[:10]:
        lines.append(f"| {n} | {m:.3f} | {100 * m / total:.1f} % | {f / (m * 1e-3) / 1e12 if f else 0:.1f} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
