"""D-Flow timing on the GPU (writes a markdown table to stdout and, with --out, to a file):

  * ms per LBFGS closure (pf_d_flow_value_and_grad, graph-replayed) at the timing config of the reference's
    scripts/script_compute_time.sh (celeba 128^2 net, gaussian_deblurring_FFT, batch_size_ip 2) and at B = 32;
  * ms per T(z) (pf_d_flow_forward, graph-replayed);
  * the dopri5 latent initialisation: accepted / rejected steps, velocity evaluations, ms;
  * optionally (--closures-only) just a few closures, for a `rocprofv3 --kernel-trace --stats` pass.

Synthetic seed-fixed weights (tools/synthetic_weights.py recipe via the oracle) and inputs: times, not restoration quality.
Usage:  python tools/gpu_dflow_time.py [--out profiles/dflow_timing.md] [--closures-only]
"""
import argparse
import os
import sys
from time import perf_counter

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def det_normal(shape, seed, idx=0):
    g = np.random.Generator(np.random.Philox(key=[seed, idx]))
    return torch.from_numpy(g.standard_normal(size=shape, dtype=np.float32))


def build_celeba128():
    from oracle import pnpflow_oracle as O
    from pnpflow_amd.models import UNet
    c = dict(input_channels=3, input_height=128, ch=32, ch_mult=(1, 2, 4, 8), num_res_blocks=6, attn_resolutions=(16, 8))
    m = UNet(3, 128, 32, ch_mult=c["ch_mult"], num_res_blocks=6, attn_resolutions=c["attn_resolutions"])
    m.load_state_dict(O.synthetic_state_dict(O.unet_config(**c), 0))
    return m


def solver(m):
    from pnpflow_amd.methods.d_flow import D_FLOW
    from pnpflow_amd.utils import CfgNode
    return D_FLOW(m, torch.device("cuda"), CfgNode(dict(method="d_flow", model="ot", problem="gaussian_deblurring_FFT", steps_euler=6, lmbda=0.001,
                                                        alpha=0.1, max_iter=7, LBFGS_iter=20, start_time=0.0, max_batch=1, compute_time=False,
                                                        compute_memory=False, save_results=False, batch=0)))


def timed(fn, reps):
    fn(); torch.cuda.synchronize()          # capture / warm-up
    t0 = perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--closures-only", action="store_true")
    a = ap.parse_args()
    import pnpflow_amd.degradations as D
    m = build_celeba128()
    s = solver(m)
    dg = D.GaussianDeblurring(1.0, 61, "fft", 3, 128)
    if a.closures_only:
        z = det_normal((2, 3, 128, 128), 1).cuda(); y = det_normal((2, 3, 128, 128), 2).cuda()
        for _ in range(5):
            s.value_and_grad(z, y, dg, 0.001)
        torch.cuda.synchronize()
        print("5 closures done")
        return
    rows = []
    for B in (2, 32):
        z = det_normal((B, 3, 128, 128), 1).cuda(); y = det_normal((B, 3, 128, 128), 2).cuda()
        reps = 20 if B == 2 else 5
        ms_c = timed(lambda: s.value_and_grad(z, y, dg, 0.001), reps)
        ms_t = timed(lambda: s.forward_flow_matching(z), reps)
        s.use_graph = False
        ms_ce = timed(lambda: s.value_and_grad(z, y, dg, 0.001), reps)
        s.use_graph = True
        x = dg.H_adj(dg.H(det_normal((B, 3, 128, 128), 3).clamp(-1, 1).cuda()))
        torch.cuda.synchronize(); t0 = perf_counter()
        s.inverse_flow_matching(x)
        torch.cuda.synchronize(); ms_o = (perf_counter() - t0) * 1e3
        st = s.last_dopri5_stats
        rows.append((B, ms_c, ms_ce, ms_t, st["accepted"], st["rejected"], st["nfev"], ms_o))
    lines = ["| B | closure ms (graph) | closure ms (eager launches) | T(z) ms (graph) | dopri5 accepted | rejected | evaluations | dopri5 ms |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r[0]} | {r[1]:.2f} | {r[2]:.2f} | {r[3]:.2f} | {r[4]} | {r[5]} | {r[6]} | {r[7]:.1f} |")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
