"""Generate tests/golden/prior_eval_tiny4.npz: the likelihood solve of pnpflow/image_generation/likelihood.py:172-193 restated on the
oracle, integrated by SciPy itself.  Oracle + SciPy only (no reference code):   python tools/make_golden_prior_eval.py

State (x, logp), d x/dt = v(x, t), d logp/dt = eps . (J_v(x, t)^T eps), from t = 1 to t = 1e-5 with
scipy.integrate.solve_ivp(method='RK45', rtol = atol = 1e-5) - the call the reference makes.  Net: the 4-level test U-Net `tiny4`
(synthetic weights of oracle/pnpflow_oracle.py), input det_image((2, 3, 64, 64), 41), eps the engine's Rademacher draw (seed 5, stream 7):
element e is word e % 4 of Philox4x32-10 at counter (e/4 lo, e/4 hi, stream lo, stream hi), key (seed lo, seed hi); +1 when the word's top
bit is set, else -1.

  ref32   the net and its VJP evaluated in fp32 (as the reference evaluates them), the state in SciPy's fp64
  ref64   the same with the net in fp64
  tight   fp64 at rtol = atol = 1e-9: the yardstick the GPU test measures distances to

Each holds z, delta_logp, bpd (offset 7, the reference's default inverse_scaler), nfev and the attempt count (nfev - 2) / 6; gap_* is
max|ref32 - ref64| of each quantity in fp64.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pnpflow_oracle as O  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CFG = dict(input_channels=3, input_height=64, ch=32, ch_mult=(1, 2, 4, 8), num_res_blocks=1, attn_resolutions=(16, 8))      # tests/conftest.py CFGS["tiny4"]
SHAPE = (2, 3, 64, 64)
IMAGE_SEED, EPS_SEED, EPS_STREAM = 41, 5, 7
T0, T1, OFFSET = 1.0, 1e-5, 7.0

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


def rademacher(n, seed, stream, offset=0):
    q_lo = offset // 4
    qs = np.arange(q_lo, (offset + n + 3) // 4, dtype=np.uint64)
    ctr = np.zeros((qs.size, 4), dtype=np.uint32)
    ctr[:, 0] = (qs & np.uint64(0xFFFFFFFF)).astype(np.uint32); ctr[:, 1] = (qs >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = np.uint32(stream & 0xFFFFFFFF); ctr[:, 3] = np.uint32((stream >> 32) & 0xFFFFFFFF)
    r = O.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32))
    return np.where(r.reshape(-1)[offset - 4 * q_lo:offset - 4 * q_lo + n] >> np.uint32(31), 1.0, -1.0).astype(np.float32)


def solve(dtype, rtol, atol):
    from scipy.integrate import solve_ivp
    B = SHAPE[0]
    cfg = O.unet_config(**CFG)
    sd = {k: v.to(dtype) for k, v in O.synthetic_state_dict(cfg, seed=0).items()}
    eps = torch.from_numpy(rademacher(int(np.prod(SHAPE)), EPS_SEED, EPS_STREAM)).view(SHAPE).to(dtype)
    emb = O.sinusoidal_embedding
    O.sinusoidal_embedding = lambda t, dim: emb(t, dim).to(dtype)

    def f(t, y):
        x = torch.from_numpy(y[:-B]).view(SHAPE).to(dtype).requires_grad_(True)
        with torch.enable_grad():
            v = O.unet_forward(sd, cfg, x, torch.full((B,), t, dtype=dtype))
            (g,) = torch.autograd.grad(v, x, grad_outputs=eps)
        div = (g.detach() * eps).sum(dim=(1, 2, 3))
        return np.concatenate([v.detach().reshape(-1).double().numpy(), div.double().numpy()])
    try:
        y0 = np.concatenate([det_image(SHAPE, IMAGE_SEED).double().reshape(-1).numpy(), np.zeros(B)])
        sol = solve_ivp(f, (T0, T1), y0, method="RK45", rtol=rtol, atol=atol)
    finally:
        O.sinusoidal_embedding = emb
    assert sol.success, sol.message
    z, dlp = sol.y[:-B, -1].reshape(SHAPE), sol.y[-B:, -1]
    N = int(np.prod(SHAPE[1:]))
    prior = -N / 2.0 * np.log(2 * np.pi) - 0.5 * (z ** 2).sum(axis=(1, 2, 3))
    bpd = -(prior + dlp) / (N * np.log(2.0)) + OFFSET
    assert (sol.nfev - 2) % 6 == 0
    return dict(z=z, delta_logp=dlp, bpd=bpd, nfev=sol.nfev, attempts=(sol.nfev - 2) // 6, accepted=sol.t.size - 1)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    runs = {"ref32": solve(torch.float32, 1e-5, 1e-5), "ref64": solve(torch.float64, 1e-5, 1e-5), "tight": solve(torch.float64, 1e-9, 1e-9)}
    out = dict(offset=np.array(OFFSET), rtol=np.array(1e-5), atol=np.array(1e-5), t0=np.array(T0), t1=np.array(T1))
    for name, r in runs.items():
        out[name + "_z"] = r["z"].astype(np.float32)
        out[name + "_delta_logp"] = r["delta_logp"]
        out[name + "_bpd"] = r["bpd"]
        out[name + "_nfev"] = np.array(r["nfev"]); out[name + "_attempts"] = np.array(r["attempts"]); out[name + "_accepted"] = np.array(r["accepted"])
        print(name, "attempts", r["attempts"], "accepted", r["accepted"], "nfev", r["nfev"], "delta_logp", r["delta_logp"], "bpd", r["bpd"])
    for q in ("z", "delta_logp", "bpd"):
        out["gap_" + q] = np.array(np.abs(runs["ref32"][q] - runs["ref64"][q]).max())
        print(q, "ref32-ref64", float(out["gap_" + q]), "ref32-tight", float(np.abs(runs["ref32"][q] - runs["tight"][q]).max()))
    path = os.path.join(OUT, "prior_eval_tiny4.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
