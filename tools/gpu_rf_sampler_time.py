"""Rectified-flow sampler timing on the GPU (a markdown table to stdout and, with --out, to a file): samples/s of euler_sampler and rk45_sampler
(pnpflow_amd/image_generation/sampling.py) on the reference's NCSN++ configuration (256^2, nf 128, ch_mult (1, 1, 2, 2, 2, 2, 2)), with the
accepted / rejected step counts of the RK45 solve.

Synthetic seed-fixed weights (oracle/ncsnpp_oracle.py) and a det_normal latent: times and step counts of THIS velocity field, not of a trained one.
Usage:  python tools/gpu_rf_sampler_time.py [--batch 16] [--steps 100] [--tol 1e-5] [--skip-rk45] [--out profiles/rf_sampler_timing.md]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--skip-rk45", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from oracle import ncsnpp_oracle as NO
    from pnpflow_amd.image_generation import sampling as S
    from pnpflow_amd.image_generation.configs.rectified_flow.celeba_hq_pytorch_rf_gaussian import get_config
    from pnpflow_amd.image_generation.models.ncsnpp import NCSNpp
    config = get_config()
    m = NCSNpp(config)
    m.load_state_dict(NO.synthetic_state_dict(NO.ncsnpp_config(), 0))
    shape = (a.batch, 3, 256, 256)
    z = det_normal(shape, 1).cuda()
    ident = lambda x: x
    rows = []
    for sigma_var in (0.0, 0.5):
        fn = S.get_rectified_flow_sampler(S.rectified_flow_from_config(config, use_ode_sampler="euler", sample_N=a.steps, sigma_variance=sigma_var), shape, ident)
        fn(m, z=z); torch.cuda.synchronize()          # plans and buffers
        t0 = perf_counter()
        x, nfe = fn(m, z=z)
        torch.cuda.synchronize(); sec = perf_counter() - t0
        m.check_numerics()
        rows.append((f"euler N = {a.steps}, sigma_var = {sigma_var:g}", nfe, "-", "-", sec, a.batch / sec, bool(torch.isfinite(x).all())))
    if not a.skip_rk45:
        fn = S.get_rectified_flow_sampler(S.rectified_flow_from_config(config, use_ode_sampler="rk45", ode_tol=a.tol), shape, ident)
        m.ode_rk45(z, 1e-3, 2e-3, 1e-2, 1e-2)          # plans and buffers: a short solve
        torch.cuda.synchronize(); t0 = perf_counter()
        x, nfe = fn(m, z=z)
        torch.cuda.synchronize(); sec = perf_counter() - t0
        st = fn.last_stats
        rows.append((f"rk45 rtol = atol = {a.tol:g}", nfe, st["accepted"], st["rejected"], sec, a.batch / sec, bool(torch.isfinite(x).all())))
    lines = [f"| sampler (256^2, B = {a.batch}) | evaluations | accepted | rejected | seconds | samples/s | finite |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]:.2f} | {r[5]:.3f} | {r[6]} |")
    txt = "\n".join(lines) + "\n"
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
