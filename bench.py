"""Benchmark of the PnP-Flow restoration hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload c2_256|c2|c3|c4|c5|tiny] [--dump-outputs DIR] [--full]

A "step" = one full PnP-Flow restoration (steps_pnp=100 outer iterations x num_samples=5
U-Net evaluations + data-fidelity / interpolation / averaging kernels) of ONE batch of
synthetic degraded images that already resides in HBM.  Default workload = the configuration
BASELINE.json's `metric` is quoted on: CelebA-shaped 256x256 box inpainting (half-size 40,
sigma 0.05, alpha 0.5 - the reference's main.py:132-136 at 256^2), pnp_flow, batch 32 per GPU,
100 x 5.  Each rank restores its own batch (independent units, weak scaling).  Rank 0 prints
ONE JSON line.

A plain run sets up, runs W warm-up steps, times K steps and prints the headline (`value`,
`ms_per_step`).  `--full` adds everything else the line can carry, each with runs of its own:
per-image PSNR (all_gathered in global image order), board power over the timed steps, the conv
roofline with the box's streaming / MFMA ceilings, the CPU baseline, BASELINE configs[1..4]
beside the headline in `configs`, precision mode 2, the NCSN++ forward and the pointwise block.

`--dump-outputs DIR` writes what the last timed step returned - the restored images of the global
batch, in global image order - as DIR/restored.npy (float32; a fixed, seeded sample of whole
images when the batch exceeds 64 MB).  The inputs depend only on the arguments, so two builds
can be compared output for output.

`--gpus N` IS the job size: with N > 1 and no torchrun environment the script re-executes itself
under `python -m torch.distributed.run --nproc-per-node N` (one process per GPU, backend "nccl" =
RCCL); launched under torchrun (as the driver does) it requires WORLD_SIZE == N and aborts otherwise.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (dim, batch per GPU, problem, alpha, steps_pnp, num_samples, net config, GFLOP per image per forward)
    "c2_256": dict(dim=256, B=32, problem="inpainting", alpha=0.5, steps=100, ns=5, nres=6,
                   label="CelebA-shaped 256x256 box-inpainting (half-size 40, sigma 0.05) pnp_flow B=32/GPU 100x5 (the configuration BASELINE.json's metric is quoted on; main.py:132-136 at 256^2)"),
    "c2": dict(dim=128, B=32, problem="inpainting", alpha=0.5, steps=100, ns=5, nres=6, label="CelebA-128 box-inpainting pnp_flow B=32/GPU 100x5 (BASELINE configs[1])"),
    "c3": dict(dim=128, B=64, problem="gaussian_deblurring_FFT", alpha=0.01, steps=100, ns=5, nres=6, label="CelebA-128 Gaussian deblurring pnp_flow B=64/GPU 100x5 (BASELINE configs[2])"),
    "c4": dict(dim=256, B=16, problem="superresolution", alpha=0.3, steps=100, ns=5, nres=6, label="AFHQ-256 superresolution x4 pnp_flow B=16/GPU 100x5 (BASELINE configs[3])"),
    "c5": dict(dim=256, B=32, problem="random_inpainting", method="ot_ode", start_time=0.1, gamma="constant", alpha=0.0, steps=100, ns=1, nres=6,
               label="AFHQ-256 random-inpainting ot_ode B=32/GPU steps_ode=100 start_time=0.1 (BASELINE configs[4])"),
    "tiny": dict(dim=64, B=4, problem="inpainting", alpha=0.5, steps=10, ns=2, nres=1, label="4-level test net 64x64 (smoke)"),
}


def det_image(shape, seed):
    g = np.random.Generator(np.random.Philox(key=[seed, 7]))
    x = torch.from_numpy(g.standard_normal(size=shape, dtype=np.float32))
    k = torch.ones(shape[1], 1, 3, 3) / 9.0
    for _ in range(5):
        x = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (1, 1, 1, 1), mode="replicate"), k, groups=shape[1])
    lo = x.amin(dim=(1, 2, 3), keepdim=True); hi = x.amax(dim=(1, 2, 3), keepdim=True)
    return ((x - lo) / (hi - lo) * 2 - 1).contiguous()


def global_clean(dim, lo, hi, seed=1234):
    """Images [lo, hi) of the synthetic test set: image i is det_image(seed + i) whatever the sharding, so N ranks restore
    exactly the images a single-device run at the global batch size restores."""
    return torch.cat([det_image((1, 3, dim, dim), seed + i) for i in range(lo, hi)])


def shard_inputs(wl, rank, world, step=0):
    """(lo, hi, clean, measurement noise, OT-ODE initialisation noise) of this rank's slice of the global batch world*B:
    every batch-shaped random draw is made for the GLOBAL batch and sliced (pnpflow_amd/parallel.py)."""
    from pnpflow_amd.parallel import global_measurement_noise, global_normal, shard_range
    dim, B = wl["dim"], wl["B"]
    G = world * B
    lo, hi = shard_range(G, rank, world)
    clean = global_clean(dim, lo, hi)
    sf = {128: 2, 256: 4}.get(dim, 2) if wl["problem"] == "superresolution" else 1
    meas = global_measurement_noise(step, (G, 3, dim // sf, dim // sf), lo, hi)
    init = global_normal((98, step), (G, 3, dim, dim), lo, hi) if wl.get("method") == "ot_ode" else None
    return lo, hi, clean, meas, init


def make_problem(D, problem, dim, global_batch=None, batch_offset=0):
    if problem == "inpainting":
        return D.BoxInpainting({64: 10, 128: 20, 256: 40}[dim]), 0.05
    if problem == "gaussian_deblurring_FFT":
        return D.GaussianDeblurring({128: 1.0, 256: 3.0}[dim], 61, "fft", 3, dim), 0.05
    if problem == "superresolution":
        return D.Superresolution({128: 2, 256: 4}[dim], dim), 0.05
    if problem == "random_inpainting":
        return D.RandomInpainting(0.7, global_batch=global_batch, batch_offset=batch_offset), 0.01
    raise ValueError(problem)


def usable_cores():
    """Host threads this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(float(q) / float(per))))
    except Exception:
        pass
    return n


def cpu_baseline(wl, budget_s=20.0):
    """The oracle (CPU restatement of the reference path, torch fp32, all usable host cores) timed on
    a bounded sample of the same workload: B=2 images and as many U-Net evaluations of the first
    outer iterations as fit in ~budget_s seconds.  Cost is linear in (evaluations x images); the
    extrapolation to steps_pnp x num_samples evaluations is stated in `sample`."""
    from oracle import pnpflow_oracle as O          # the ONLY use of oracle/ in this file: the thing timed as the CPU baseline
    cores = usable_cores()
    torch.set_num_threads(cores)
    Bc, dim = 2, wl["dim"]
    cfg = O.unet_config(3, dim, 32, (1, 2, 4, 8), wl["nres"], (16, 8))
    sd = O.synthetic_state_dict(cfg, 0)             # same seed-fixed recipe as tools/synthetic_weights.py
    deg, sigma = O.make_degradation(wl["problem"], dim) if dim in (128, 256) else (O.BoxInpainting(10), 0.05)
    clean = det_image((Bc, 3, dim, dim), 31)
    y = O.make_measurement(clean, deg, sigma, 0)
    model = lambda a, t: O.unet_forward(sd, cfg, a, t)
    with torch.no_grad():
        model(clean, torch.zeros(Bc))                      # warm the thread pool / allocator
        t0 = time.perf_counter(); model(clean, torch.zeros(Bc)); tf = time.perf_counter() - t0
    total_fw = wl["steps"] * wl["ns"]
    n_fw = int(max(1, min(total_fw, budget_s / max(tf, 1e-6))))
    H, H_adj = deg.H, deg.H_adj
    lr, delta = sigma ** 2, 1.0 / wl["steps"]
    done = 0
    t0 = time.perf_counter()
    x = H_adj(torch.ones_like(y))
    with torch.no_grad():
        for it in range(wl["steps"]):
            t1 = torch.ones(len(x)) * delta * it
            lr_t = O.learning_rate_strat(lr, t1, "alpha_1_minus_t", wl["alpha"])
            z = x - lr_t * (H_adj(H(x) - y) / sigma ** 2)
            x_new = torch.zeros_like(x)
            tv = t1.view(-1, 1, 1, 1)
            for _ in range(wl["ns"]):
                zt = tv * z + torch.randn_like(z) * (1 - tv)
                x_new += zt + (1 - tv) * model(zt, t1)
                done += 1
                if done >= n_fw:
                    break
            x = x_new / wl["ns"]
            if done >= n_fw:
                break
    dt = time.perf_counter() - t0
    per_image_full = dt / done * total_fw / Bc
    return dict(value=1.0 / per_image_full, unit="images/s", cores=cores, kind="port",
                sample=f"oracle PnP-Flow loop, B={Bc}, first {done} of {total_fw} U-Net evaluations (+ their pointwise steps) "
                       f"in {dt:.1f}s on {cores} threads, scaled linearly to {total_fw} evaluations")


FWD_FLOPS = {128: 49.78e9, 256: 189.44e9}      # algorithmic FLOP per image per U-Net forward

def measured_traffic(workload, kernel_class=None):
    """HBM bytes per launch of the dominant conv kernel of `workload`, measured with rocprofv3 --pmc in separate FETCH_SIZE / WRITE_SIZE
    passes (FETCH doubled as MI355X_MICROARCH.md prescribes for gfx950) by tools/pmc_traffic.sh, which writes profiles/traffic.json:
    {workload: {"bytes_per_launch": <conv family average>, "kernels": [{kernel, launches, read_mb_per_launch, write_mb_per_launch}], ...}}.
    The bench line carries what that committed file holds (null when the workload has no entry) - never a constant of this script."""
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as fh:
            rec = json.load(fh).get(workload)
        if not rec:
            return None, None
        if kernel_class:
            pat = kernel_class.split(" ")[0].replace("<", "<").split("<")
            name, tile = pat[0], (pat[1].rstrip(">").split(",") if len(pat) > 1 else None)
            tot_b, tot_n = 0.0, 0
            for k in rec.get("kernels", []):
                kn = k["kernel"].replace(" ", "")
                if name in kn and (tile is None or ("<" + ",".join(tile) + ",") in kn):
                    if tile is not None:
                        return (k["read_mb_per_launch"] + k["write_mb_per_launch"]) * 1e6, rec.get("source")
                    tot_b += (k["read_mb_per_launch"] + k["write_mb_per_launch"]) * 1e6 * k["launches"]; tot_n += k["launches"]
            if tot_n:          # a class made of several instantiations (conv_pp_kernel<chunk structure>): launch-weighted mean
                return tot_b / tot_n, rec.get("source")
        return float(rec["bytes_per_launch"]), rec.get("source")
    except Exception:           # noqa: BLE001
        return None, None


def live_traffic(dim, unet_batch, kernel_class):
    """HBM bytes per launch of `kernel_class`, measured IN THIS RUN when rocprofv3 is on the box: two child processes (separate
    `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes with the kernel trace only, as MI355X_MICROARCH.md prescribes; FETCH doubled for
    gfx950, KiB units) over two forwards of the same net at the same U-Net batch (tools/gpu_forward_only.py).  -> (bytes, source) or
    (None, None) - the caller then falls back to the committed profiles/traffic.json, labelled as not measured in this run."""
    import shutil, sqlite3, subprocess, tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.isfile("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, None
    name = kernel_class.split(" ")[0].split("<")[0]
    tile = kernel_class.split(" ")[0].split("<")[1].rstrip(">") if "<" in kernel_class.split(" ")[0] else None
    tot = {}
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = tempfile.mkdtemp(prefix="pf_pmc_", dir="/tmp")
            env = dict(os.environ, TMPDIR="/tmp")
            env.pop("PNPFLOW_HIP_PROFILE_CSV", None)
            subprocess.run([exe, "--kernel-trace", "--pmc", counter, "-d", d, "-o", "r", "--", sys.executable,
                            os.path.join(ROOT, "tools", "gpu_forward_only.py"), str(dim), str(unet_batch), "2"],
                           cwd="/tmp", env=env, capture_output=True, text=True, timeout=240)
            dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith(".db")]
            if not dbs:
                return None, None
            cur = sqlite3.connect(dbs[0]).cursor()
            s_, n_ = 0.0, 0
            for kn, val, cnt in cur.execute("select kernel_name, sum(value), count(*) from counters_collection where counter_name = ? group by kernel_name", (counter,)):
                k0 = str(kn).replace(" ", "")
                if name in k0 and (tile is None or ("<" + tile + ",") in k0):
                    s_ += float(val); n_ += int(cnt)
            shutil.rmtree(d, ignore_errors=True)
            if n_ == 0:
                return None, None
            tot[counter] = s_ * 1024.0 / n_
        return 2.0 * tot["FETCH_SIZE"] + tot["WRITE_SIZE"], ("rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes in this bench run (2 forwards of "
                f"tools/gpu_forward_only.py {dim} {unet_batch}); 2 x FETCH_SIZE + WRITE_SIZE, KiB units; launch-weighted mean over the instantiations of the class")
    except Exception:          # noqa: BLE001   (a profiler hiccup must not take the measured line with it)
        return None, None


class Runner:
    """One BASELINE workload on this rank: model, solver, resident synthetic batch, `step(i)` = one full restoration."""

    def __init__(self, name, rank, world, dev, precision=1, use_graph=True, models=None):
        import pnpflow_amd.degradations as D
        from pnpflow_amd.methods.pnp_flow import PNP_FLOW
        from pnpflow_amd.models import UNet
        from pnpflow_amd.utils import CfgNode
        from tools.synthetic_weights import synthetic_state_dict      # product-side recipe (no checkpoint is reachable offline)
        self.name, self.wl, self.rank, self.world, self.dev = name, WORKLOADS[name], rank, world, dev
        wl = self.wl
        dim, B = wl["dim"], wl["B"]
        key = (dim, wl["nres"])
        if models is not None and key in models:
            self.model = models[key]
        else:
            self.model = UNet(3, dim, 32, ch_mult=(1, 2, 4, 8), num_res_blocks=wl["nres"], attn_resolutions=(16, 8), device_index=dev.index or 0)
            self.model.load_state_dict(synthetic_state_dict(self.model, 0))
            if models is not None:
                models[key] = self.model
        self.model.set_precision(precision)
        lo, hi, clean, meas_noise, init_noise = shard_inputs(wl, rank, world)
        self.degradation, self.sigma = make_problem(D, wl["problem"], dim, global_batch=world * B, batch_offset=lo)
        self.is_ode = wl.get("method") == "ot_ode"
        self.args = CfgNode(dict(method=wl.get("method", "pnp_flow"), model="ot", problem=wl["problem"], noise_type="gaussian", num_samples=wl["ns"],
                                 steps_pnp=wl["steps"], lr_pnp=1.0, gamma_style="alpha_1_minus_t", alpha=wl["alpha"], max_batch=1,
                                 steps_ode=wl["steps"], start_time=wl.get("start_time", 0.1), gamma=wl.get("gamma", "constant"),
                                 compute_time=False, compute_memory=False, save_results=False, batch=0, sigma_noise=self.sigma))
        if self.is_ode:
            from pnpflow_amd.methods.ot_ode import OT_ODE
            self.solver = OT_ODE(self.model, dev, self.args)
            self.solver.use_graph = use_graph
            self.solver.init_noise = init_noise.to(dev)
        else:
            self.solver = PNP_FLOW(self.model, dev, self.args)
            self.solver.use_graph = use_graph
            self.solver.noise_seed = 2024          # one Philox key for the job; the shard draws ITS slice of every global noise tensor:
            self.solver.image_offset = lo          # pf_pnp_params.elem_offset = lo*C*H*W
        # synthetic batch of this rank (global batch = world*B, rank r owns images [lo, hi)), resident in HBM
        self.clean = clean.to(dev)
        self.y = self.degradation.H(self.clean) + self.sigma * meas_noise.to(dev)
        self.lr = self.sigma ** 2 * 1.0

    def step(self, i, steps=None):
        self.args.batch = i            # selects the Philox noise stream block
        if steps is not None:          # short warm-up: same kernels / plans / graph, fewer outer iterations
            self.args.steps_pnp = steps; self.args.steps_ode = steps
        try:
            if self.is_ode:
                return self.solver.restore_batch(self.y, self.degradation, self.sigma)
            return self.solver.restore_batch(self.y, self.degradation, self.sigma, self.lr)
        finally:
            self.args.steps_pnp = self.wl["steps"]; self.args.steps_ode = self.wl["steps"]

    def flops_per_image(self):
        f = FWD_FLOPS.get(self.wl["dim"])
        if f is None:
            return None
        if self.is_ode:   # algorithmic: 1 forward + 1 input-gradient backward (= 2 forward-equivalents) per Euler step
            return (self.wl["steps"] - int(self.wl["steps"] * self.wl["start_time"])) * 2 * f
        return self.wl["steps"] * self.wl["ns"] * f

    def unet_batch(self):
        return self.wl["B"] * (self.wl["ns"] if getattr(self.solver, "batch_samples", False) else 1)


STREAM_CEILING_GBS = 5500.0      # fallback when the probe binary is absent (profiles/r03_level0_bound_ab.md section 1); normally measured in this run
GUIDE_COPY_GBS = 6300.0          # MI355X_MICROARCH.md: what a float4 copy reaches (79 % of the 8 TB/s spec peak)


def streaming_ceiling(tensor_bytes, passes):
    """The HBM rate a pure float4 streaming kernel reaches ON THIS BOX, NOW, on tensors of the dominant kernel's size with its read /
    write mix (tools/ubench/stream_mix.hip `quick`: the best of two grid-stride grids and a 16 KB-per-workgroup split).  Run as a child
    process while this process's GPU queue is idle.  -> (GB/s, measured_this_run, detail)"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "ubench", "stream_mix")
    try:
        res = subprocess.run([exe, "quick", str(int(tensor_bytes))], capture_output=True, text=True, timeout=120)
        d = json.loads(res.stdout.strip().splitlines()[-1])
        key = {2: "1R+1W", 3: "2R+1W"}.get(int(round(passes)), "3R+1W")
        return float(d[key]), True, d
    except Exception as exc:          # noqa: BLE001   (a missing probe must not take the measured line with it)
        return STREAM_CEILING_GBS, False, {"error": f"{type(exc).__name__}: {exc}"[:200]}


class PowerSampler:
    """Board power and shader clock of THIS rank's GPU during the timed region, read from the amdgpu hwmon files (power1_input in uW,
    freq1_input in Hz; the card is matched by PCI address) every 100 ms on a host thread - no GPU work, no effect on the timed steps.
    Round 6 (profiles/r06_power_bound.md): the conv kernels run against the board's power management (1.6-2.1 GHz shader clock against the
    2.4 GHz of the datasheet peaks); the line carries the evidence.  Best effort: `available: false` when the files are not readable."""

    def __init__(self, dev_index):
        import glob, threading
        self.samples, self._stop, self._thread, self.hw, self.cap_w = [], threading.Event(), None, None, None
        try:
            prop = torch.cuda.get_device_properties(dev_index)
            bdf = f"{getattr(prop, 'pci_domain_id', 0):04x}:{prop.pci_bus_id:02x}:{prop.pci_device_id:02x}"
            for h in glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*"):
                if bdf in os.path.realpath(os.path.join(h, "device")) and os.path.isfile(os.path.join(h, "power1_input")):
                    self.hw = h
                    break
            if self.hw:
                try:
                    self.cap_w = int(open(os.path.join(self.hw, "power1_cap")).read()) / 1e6
                except Exception:      # noqa: BLE001
                    self.cap_w = None
                self._thread = threading.Thread(target=self._run, daemon=True)
        except Exception:              # noqa: BLE001
            self.hw = None

    def _run(self):
        while not self._stop.is_set():
            try:
                pw = int(open(os.path.join(self.hw, "power1_input")).read()) / 1e6
                fq = int(open(os.path.join(self.hw, "freq1_input")).read()) / 1e9
                self.samples.append((pw, fq))
            except Exception:          # noqa: BLE001
                pass
            self._stop.wait(0.1)

    def start(self):
        if self._thread:
            self._thread.start()
        return self

    def stop(self):
        if not self._thread:
            return {"available": False}
        self._stop.set(); self._thread.join(timeout=2)
        if not self.samples:
            return {"available": False}
        pw = sorted(s[0] for s in self.samples); fq = sorted(s[1] for s in self.samples)
        return {"available": True, "source": "amdgpu hwmon power1_input / freq1_input, 100 ms samples over the timed steps", "samples": len(pw),
                "board_power_w_mean": round(sum(pw) / len(pw), 1), "board_power_w_p95": round(pw[int(0.95 * (len(pw) - 1))], 1), "board_power_cap_w": self.cap_w,
                "sclk_ghz_mean": round(sum(fq) / len(fq), 3), "sclk_ghz_min": round(fq[0], 3), "sclk_ghz_max": round(fq[-1], 3), "sclk_ghz_datasheet": 2.4}


def mfma_ceiling():
    """The dense f16 MFMA rate THIS BOX delivers NOW under a pure v_mfma_f32_32x32x16_f16 load (tools/ubench/mfma_f16_chain.hip `quick`: one
    wave per SIMD, four independent accumulator chains, ~0.6 s warm-up + ~1.2 s measured) - the matrix-pipe counterpart of
    streaming_ceiling.  The clock under a matrix load is power-managed and differs between boxes by a few percent; a class's executed-MFMA
    rate as a fraction of this number is comparable across boxes.  -> (TFLOP/s, measured_this_run, detail)"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "ubench", "mfma_f16_chain")
    try:
        res = subprocess.run([exe, "quick"], capture_output=True, text=True, timeout=120)
        d = json.loads(res.stdout.strip().splitlines()[-1])
        return float(d["tflops_f16_dense"]), True, d
    except Exception as exc:          # noqa: BLE001
        return None, False, {"error": f"{type(exc).__name__}: {exc}"[:200]}


def conv_roofline(r, precision, workload, measure_traffic=False):
    """Roofline of the conv family (every 3x3 / 1x1 conv of the U-Net), from HIP-event timing of every conv launch over a profiled
    slice of the SAME workload at the SAME U-Net batch (eager launches; graph replay hides the per-kernel boundaries; a conv_dma
    launch is timed together with its prep pass).  Two views:
      * the DOMINANT kernel class by time decides `bound`: at 256^2 that is the 32-channel full-resolution level
        (conv_mfma16_kernel<2,1,4,1,...>, ~1/3 of the step), whose floor is HBM - every operand tensor read once, the result written
        once, the residual read once (`alg_mb` of the engine's per-launch CSV) against the 8 TB/s HBM3E peak;
      * `mfma_family`: algorithmic FLOPs of ALL conv launches against the dense f16 MFMA peak (the round-1/2 figure)."""
    import csv, tempfile
    model = r.model
    rep = r.unet_batch() // r.wl["B"]
    n_fw = 2 if rep > 1 else 4
    t_dev = torch.full((r.wl["B"] * rep,), 0.37, device=r.dev)
    zt = (r.clean + 0.1).repeat(rep, 1, 1, 1)
    model(zt, t_dev)                     # builds the plan outside the profiled slice
    tmp = tempfile.NamedTemporaryFile(prefix="pf_layers_", suffix=".csv", delete=False); tmp.close()
    os.environ["PNPFLOW_HIP_PROFILE_CSV"] = tmp.name
    model.profile(True)
    for _ in range(n_fw):
        model(zt, t_dev)
    launches, ms, flops = model.profile_read()
    model.profile(False)
    os.environ.pop("PNPFLOW_HIP_PROFILE_CSV", None)
    rows = list(csv.DictReader(open(tmp.name))); os.unlink(tmp.name)
    ach = flops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0      # ALGORITHMIC (fp32-equivalent) TFLOP/s of the conv-GEMM launches
    # kernel classes: the engine's per-launch CSV says which kernel a launch took ("dma" column); conv_mfma16's tile follows Cout
    PERSISTENT = {2: "conv_pp_kernel (Cout 32, persistent two-team)", 5: "conv_sp_kernel (Cout 64 / 128, persistent, one wave per SIMD)"}
    cls = {}
    for w in rows:
        k = int(w["dma"])
        key = PERSISTENT[k] if k in PERSISTENT else "conv_dma_kernel (+ prep_split)" if k == 1 else (
            "conv_mfma16_kernel<2,1,4,1> (Cout 32)" if int(w["Cout"]) <= 32 else
            "conv_mfma16_kernel<4,1,2,2> (Cout 64)" if int(w["Cout"]) <= 64 else "conv_mfma16_kernel<4,1,1,4> (Cout >= 128)")
        c = cls.setdefault(key, dict(us=0.0, mb=0.0, n=0, gflop=0.0))
        c["us"] += float(w["us"]); c["mb"] += float(w["alg_mb"]); c["n"] += 1; c["gflop"] += float(w["gflop"])
    tot_us = sum(c["us"] for c in cls.values()) or 1.0
    dtype_peak = 157.3 if precision == 0 else 2500.0
    terms = 3 if precision == 1 else 1
    # every class against ITS OWN roof: the higher of its HBM floor (algorithmic bytes at 8 TB/s) and its MFMA floor (executed flops
    # at the dense peak of the dtype) decides the bound; frac = achieved / peak of that bound
    for c in cls.values():
        c["hbm_floor_us"] = c["mb"] * 1e6 / 8e12 * 1e6 / c["n"]
        c["mfma_floor_us"] = terms * c["gflop"] * 1e9 / (dtype_peak * 1e12) * 1e6 / c["n"]
        c["bound"] = "hbm" if c["hbm_floor_us"] >= c["mfma_floor_us"] else "mfma"
        c["gbs"] = c["mb"] * 1e6 / (c["us"] * 1e-6) / 1e9
        c["tfl"] = c["gflop"] * 1e9 / (c["us"] * 1e-6) / 1e12
        c["frac"] = c["gbs"] / 8000.0 if c["bound"] == "hbm" else c["tfl"] / dtype_peak
    # the dominant class, deterministically: the largest share of the conv time; classes within one percentage point of it tie, and a
    # tie goes to the HBM-bound class, then to the name (round 4: at 128^2 two classes tie and `bound` flipped from run to run)
    top = max(c["us"] for c in cls.values())
    tied = [k for k in cls if cls[k]["us"] >= top - 0.01 * tot_us]
    dom = sorted(tied, key=lambda k: (cls[k]["bound"] != "hbm", k))[0]
    d = cls[dom]
    traffic, src, traffic_live = (None, None, False)
    if precision == 1 and rep == 5:
        traffic, src = live_traffic(r.wl["dim"], r.wl["B"] * rep, dom) if measure_traffic else (None, None)
        traffic_live = traffic is not None
        if traffic is None:
            traffic, src = measured_traffic(workload, dom)
    fam = dict(bound="mfma", achieved=round(ach, 2), peak=dtype_peak, unit="TFLOP/s", frac=round(ach / dtype_peak, 4),
               launches=int(launches // n_fw), avg_launch_us=round(ms * 1e3 / max(1, launches), 2),
               algorithmic_gflop_per_launch=round(flops / max(1, launches) / 1e9, 4),
               kernel="conv family: conv_pp_kernel (persistent, LDS-resident weights: the 32-channel level) + conv_dma_kernel (LDS-DMA A operand from the prep_split pass; selected where a prepped element feeds >= 2000 MACs) + conv_mfma16_kernel "
                      "(register-staged) - f16 32x32x16 MFMA implicit GEMM, " + {0: "exact fp32 MFMA (conv_mfma_kernel)", 1: "3 MFMAs per product (fp32-equivalent split)", 2: "1 MFMA per product (hi-only operands)"}[precision])
    if precision == 1:
        fam.update(mfma_tflops_executed=round(3 * ach, 2), frac_executed=round(3 * ach / dtype_peak, 4))
    gbs, tfl, hbm_floor_us, mfma_floor_us = d["gbs"], d["tfl"], d["hbm_floor_us"], d["mfma_floor_us"]
    hbm_bound = d["bound"] == "hbm"
    tensor_bytes = r.wl["B"] * rep * r.wl["dim"] ** 2 * 32 * 4          # one full-resolution 32-channel activation at the U-Net batch
    passes = d["mb"] * 1e6 / d["n"] / tensor_bytes if "Cout 32" in dom else 3.0
    torch.cuda.synchronize()
    ceil_gbs, ceil_measured, ceil_detail = streaming_ceiling(tensor_bytes, passes)
    mf_tfl, mf_measured, mf_detail = mfma_ceiling() if precision != 0 else (None, False, {"note": "precision mode 0 multiplies on the f32 MFMA"})
    # every class against what THIS box delivered in THIS run: an HBM-bound class against the streaming probe with its own read / write
    # mix, a matrix-bound class's EXECUTED MFMA rate against the pure-MFMA probe
    mix = ceil_detail if ceil_measured else {}
    for c in cls.values():
        if c["bound"] == "hbm":
            pc = c["mb"] * 1e6 / c["n"] / tensor_bytes
            roof_gbs = float(mix.get({2: "1R+1W", 3: "2R+1W"}.get(int(round(pc)), "3R+1W"), ceil_gbs))
            c["box_frac"] = c["gbs"] / roof_gbs
        else:
            c["box_frac"] = terms * c["tfl"] / mf_tfl if mf_tfl else None
    roof = dict(bound="hbm" if hbm_bound else "mfma",
                achieved=round(gbs, 1) if hbm_bound else round(tfl, 2), peak=8000.0 if hbm_bound else dtype_peak,
                unit="GB/s" if hbm_bound else "TFLOP/s", frac=round(gbs / 8000.0, 4) if hbm_bound else round(tfl / dtype_peak, 4),
                traffic=traffic, traffic_source=src, traffic_measured_this_run=traffic_live if traffic is not None else None, kernel=dom, share_of_conv_time=round(d["us"] / tot_us, 4),
                launches=d["n"] // n_fw, avg_launch_us=round(d["us"] / d["n"], 2), algorithmic_mb_per_launch=round(d["mb"] / d["n"], 2),
                hbm_floor_us_at_8tbs=round(hbm_floor_us, 1), mfma_floor_us=round(mfma_floor_us, 1), unet_batch=r.wl["B"] * rep,
                # what a pure streaming kernel reaches on tensors of this size with the same read / write mix, measured in THIS run
                streaming_ceiling_gbs=round(ceil_gbs, 1), frac_of_streaming_ceiling=round(gbs / ceil_gbs, 4) if hbm_bound else None,
                streaming_ceiling={"measured_this_run": ceil_measured, "probe": "tools/ubench/stream_mix quick", "tensor_bytes": tensor_bytes,
                                   "tensor_passes_per_launch": round(passes, 2), "detail": ceil_detail, "guide_float4_copy_gbs": GUIDE_COPY_GBS,
                                   "frac_of_guide_copy": round(gbs / GUIDE_COPY_GBS, 4) if hbm_bound else None},
                # the matrix pipe of this box in this run (pure v_mfma_f32_32x32x16_f16 load): the counterpart of streaming_ceiling
                mfma_ceiling={"measured_this_run": mf_measured, "probe": "tools/ubench/mfma_f16_chain quick", "tflops_f16_dense": mf_tfl,
                              "frac_of_datasheet_2500": round(mf_tfl / 2500.0, 4) if mf_tfl else None, "detail": mf_detail,
                              "family_executed_frac_of_box_ceiling": round(terms * ach / mf_tfl, 4) if mf_tfl else None},
                frac_of_box_ceiling=round(d["box_frac"], 4) if d.get("box_frac") is not None else None,
                classes={k: dict(share=round(v["us"] / tot_us, 4), avg_us=round(v["us"] / v["n"], 1), bound=v["bound"], frac=round(v["frac"], 4),
                                 algorithmic_gbs=round(v["gbs"], 1), algorithmic_tflops=round(v["tfl"], 1),
                                 executed_mfma_frac=round(terms * v["tfl"] / dtype_peak, 4),
                                 # against the ceilings measured on this box in this run (HBM-bound: streaming probe with the class's mix;
                                 # matrix-bound: executed MFMA rate over the pure-MFMA probe)
                                 frac_of_box_ceiling=round(v["box_frac"], 4) if v.get("box_frac") is not None else None,
                                 executed_mfma_frac_of_box_ceiling=round(terms * v["tfl"] / mf_tfl, 4) if mf_tfl else None)
                         for k, v in sorted(cls.items(), key=lambda kv: -kv[1]["us"])},
                mfma_family=fam)
    return roof


def pointwise_block(dev, D):
    """HBM-side evidence for the per-pixel prox / data-fidelity kernels (north_star): each kernel timed with HIP events on the
    launch stream over `reps` back-to-back launches at the BASELINE configs' sizes; achieved = ALGORITHMIC bytes / time against
    the 8 TB/s HBM3E peak (6.3 TB/s is what a float4 copy reaches, MI355X_MICROARCH.md).  The working sets (6-50 MB) fit the
    256 MiB Infinity Cache, so 'achieved' is an on-die streaming rate, and at 5-15 us per launch these kernels are launch-latency-
    sized: they sit inside the per-iteration hipGraph for that reason."""
    import ctypes as C
    from pnpflow_amd import _lib
    lib = _lib.load()
    st = _lib.current_stream_ptr

    def timed(fn, reps=20):
        fn(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    out = {}

    def add(name, secs, nbytes, shape):
        # working sets below the 256 MiB Infinity Cache are served on-die and the launches are latency-sized (5-15 us): the rate is labelled
        # cache-resident and NOT quoted as a fraction of the HBM peak; only tensors the cache cannot hold get frac_of_8tbs
        resident = nbytes < 256 * 2 ** 20
        out[name] = dict(us=round(secs * 1e6, 2), algorithmic_mb=round(nbytes / 1e6, 2), achieved_gbs=round(nbytes / secs / 1e9, 1),
                         regime="cache-resident, launch-latency-sized (not an HBM figure)" if resident else "hbm",
                         frac_of_8tbs=None if resident else round(nbytes / secs / 8e12, 4),
                         frac_of_6p3tbs=None if resident else round(nbytes / secs / 6.3e12, 4), shape=shape)

    cases = [("c2 box mask 32x3x128^2", D.BoxInpainting(20), 32, 128, 1), ("c3 gaussian blur 64x3x128^2", D.GaussianDeblurring(1.0, 61, "fft", 3, 128), 64, 128, 1),
             ("c4 decimation x4 16x3x256^2", D.Superresolution(4, 256), 16, 256, 4), ("c5 random mask 32x3x256^2", D.RandomInpainting(0.7), 32, 256, 1)]
    for label, deg, B, dim, sf in cases:
        x = torch.randn(B, 3, dim, dim, device=dev); y = torch.randn(B, 3, dim // sf, dim // sf, device=dev); z = torch.empty_like(x)
        coef = torch.full((B,), 0.5, device=dev); scratch = torch.empty((2,) + tuple(x.shape), device=dev)
        d = deg.descriptor(B, dim, dim, dev)
        n = x.numel() * 4
        blur = "blur" in label
        # grad step: read x, read y, write z (+ 4 separable passes of read+write and the aux reads for the blur)
        nb = n * (2 + 1.0 / (sf * sf)) if not blur else n * (2 * 4 + 2)
        secs = timed(lambda: lib.pf_grad_step(C.byref(d), x.data_ptr(), y.data_ptr(), coef.data_ptr(), z.data_ptr(), B, 3, dim, dim, scratch.data_ptr(), st()))
        add("grad_step " + label, secs, nb, [B, 3, dim, dim])
    for label, B, dim in (("c2/c3 128^2", 32, 128), ("c4 256^2", 16, 256)):
        x = torch.randn(B, 3, dim, dim, device=dev); zt = torch.empty_like(x); v = torch.randn_like(x); acc = torch.zeros_like(x)
        t = torch.full((B,), 0.3, device=dev); n = x.numel() * 4; npi = 3 * dim * dim
        secs = timed(lambda: lib.pf_interpolate(x.data_ptr(), t.data_ptr(), None, 2024, 5, zt.data_ptr(), B, npi, st()))
        add(f"interpolate+philox {label} B={B}", secs, 2 * n, [B, 3, dim, dim])
        secs = timed(lambda: lib.pf_denoise_accumulate(acc.data_ptr(), zt.data_ptr(), v.data_ptr(), t.data_ptr(), 0, 5.0, B, npi, st()))
        add(f"denoise_accumulate {label} B={B}", secs, 4 * n, [B, 3, dim, dim])
    return out


def cpu_baseline_ot_ode(wl, budget_s=15.0):
    """The oracle's OT-ODE loop (forward + autograd input-gradient per Euler step) on the usable host cores, B=1, as many of the
    first steps as fit in ~budget_s; scaled linearly to all steps (cost is linear in steps x images)."""
    from oracle import pnpflow_oracle as O
    cores = usable_cores()
    torch.set_num_threads(cores)
    dim = wl["dim"]
    cfg = O.unet_config(3, dim, 32, (1, 2, 4, 8), wl["nres"], (16, 8))
    sd = O.synthetic_state_dict(cfg, 0)
    deg, sigma = O.make_degradation(wl["problem"], dim)
    clean = det_image((1, 3, dim, dim), 31)
    y = O.make_measurement(clean, deg, sigma, 0)
    total = wl["steps"] - int(wl["steps"] * wl["start_time"])
    done = {"n": 0}
    t0 = time.perf_counter()

    class _Stop(Exception):
        pass

    def rec(it, xx):
        done["n"] += 1
        if time.perf_counter() - t0 > budget_s:
            raise _Stop()
    try:
        O.ot_ode_restore(lambda a, t: O.unet_forward(sd, cfg, a, t), lambda a, t, v: O.unet_vjp(sd, cfg, a, t, v), deg, wl["problem"], y, sigma,
                         steps=wl["steps"], start_time=wl["start_time"], gamma=wl.get("gamma", "constant"), record=rec)
    except _Stop:
        pass
    dt = time.perf_counter() - t0
    per_image = dt / max(1, done["n"]) * total
    return dict(value=1.0 / per_image, unit="images/s", cores=cores, kind="port",
                sample=f"oracle OT-ODE loop, B=1, first {done['n']} of {total} Euler steps (forward + input-gradient backward each) in {dt:.1f}s "
                       f"on {cores} threads, scaled linearly to {total} steps")


def ncsnpp_forward_block(dev, B=32, reps=3):
    """Velocity evaluations of the NCSN++ ("rectified") net at the reference's 256^2 config, synthetic weights.
    The measured unit is the velocity evaluation model(x, t * 999) itself: the reference's PnP-Flow schedule starts at t = 0 where
    this net's log-sigma conditioning is singular (its own output is NaN from the first iteration on); OT_ODE (start_time > 0)
    is the solver that runs with it, on the forward + the hand-written VJP (tests/test_gpu_ncsnpp.py)."""
    from pnpflow_amd.image_generation.configs.rectified_flow.afhq_cat_pytorch_rf_gaussian import get_config
    from pnpflow_amd.image_generation.models.ncsnpp import NCSNpp
    from tools.synthetic_weights import synthetic_state_dict
    m = NCSNpp(get_config(), device_index=dev.index or 0)
    m.load_state_dict(synthetic_state_dict(m))
    g = torch.Generator(device="cpu"); g.manual_seed(0)
    x = torch.randn(B, 3, 256, 256, generator=g).to(dev); lab = torch.full((B,), 0.5 * 999, device=dev)
    m(x, lab); torch.cuda.synchronize(); m.check_numerics()
    t0 = time.perf_counter()
    for _ in range(reps):
        m(x, lab)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    flop = 0.5318e12          # convs + attention matmuls per 256^2 image, from the module list
    rec = {"workload": f"NCSN++ rectified-flow net (nf 128, 7 levels, 65.6 M parameters) forward at 256x256, B={B}",
           "images_per_s": round(B / dt, 2), "ms_per_forward": round(dt * 1e3, 1), "algorithmic_tflops": round(B * flop / dt / 1e12, 1),
           "frac_of_2p5pf": round(B * flop / dt / 2.5e15, 4)}
    del m
    return rec


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def resolve_job(gpus):
    """Makes `--gpus N` the job size.  No torchrun environment and N > 1: re-execute under torch.distributed.run with N ranks on
    127.0.0.1 (never returns).  Torchrun environment present: WORLD_SIZE must equal N."""
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None:
        if gpus > 1:
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}", "--master-addr", "127.0.0.1",
                   "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
            sys.stdout.flush(); sys.stderr.flush()
            os.execv(sys.executable, cmd)
        return 0, 1
    world = int(env_world)
    if world != gpus:
        sys.exit(f"bench.py: --gpus {gpus} but the launcher started WORLD_SIZE={world} ranks: refusing to report a mislabelled line "
                 f"(launch with --nproc-per-node {gpus}, or pass --gpus {world})")
    return int(os.environ.get("RANK", "0")), world


DUMP_BYTES = 64 * 10 ** 6      # --dump-outputs writes at most this much


def dump_outputs(path, x, seed=0):
    """DIR/restored.npy: the restored images `x` (global batch, global image order) as float32.  Above DUMP_BYTES, a fixed
    sample of whole images (numpy Philox keyed by `seed`, kept in image order) that fits."""
    arr = x.detach().float().cpu().numpy()
    if arr.nbytes > DUMP_BYTES - 4096:       # room for the .npy header
        k = max(1, (DUMP_BYTES - 4096) // arr[0].nbytes)
        idx = np.sort(np.random.Generator(np.random.Philox(key=[seed, 0])).choice(len(arr), size=k, replace=False))
        arr = arr[idx]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "restored.npy"), np.ascontiguousarray(arr, dtype=np.float32))


def dry_run(a, rank, world, backend):
    """PNPFLOW_BENCH_DRY=1: the launch / rendezvous / reduction path of the bench without any GPU work (CPU containers: the
    `--gpus N` contract is testable where there is no device).  Prints the same line shape with "dry_run": true."""
    import torch.distributed as dist
    dt = 0.001 * (rank + 1)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo" if backend != "nccl" or not torch.cuda.is_available() else "nccl", rank=rank, world_size=world)
        tt = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX); dt = float(tt.item())
        ranks = dist.get_world_size()
    else:
        ranks = 1
    if rank == 0:
        wl = WORKLOADS[a.workload]
        print(json.dumps({"metric": "restored images/sec", "value": 0.0, "unit": "images/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                          "ms_per_step": round(dt * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dry_run": True,
                          "data": "none (dry run)", "ranks_in_job": ranks, "config": {"workload": wl["label"], "global_batch": world * wl["B"]}}), flush=True)
    if world > 1:
        dist.barrier(); dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="c2_256", choices=list(WORKLOADS))
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need: PSNR, board power, conv roofline, CPU baseline, the other "
                         "BASELINE configs, precision mode 2, NCSN++ forward, pointwise block (each narrowed by the --no-* options)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the restored images of the last timed step to DIR/restored.npy (float32, at most 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the secondary BASELINE configs, the pointwise block and the live traffic passes")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--batch", type=int, default=0, help="override the workload's batch per GPU (tests)")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise torch.distributed (backend 'nccl' = RCCL) even for a one-rank job and execute the job's collectives "
                         "(barrier, all_reduce(MAX) of the step time; with --full the all_gather of the per-image PSNR) on device tensors: the RCCL "
                         "path on a 1-GPU box")
    ap.add_argument("--precision", type=int, default=1, choices=[0, 1, 2],
                    help="1 (default): fp32-equivalent split-fp16 MFMA (3 x f16 MFMA per product); 0: exact fp32 MFMA; 2: one f16 MFMA per product")
    a = ap.parse_args()
    if a.gpus < 1:
        sys.exit("bench.py: --gpus must be >= 1")
    if a.steps < 1:
        sys.exit("bench.py: --steps must be >= 1")
    rank, world = resolve_job(a.gpus)
    if a.batch > 0:
        WORKLOADS[a.workload] = dict(WORKLOADS[a.workload], B=a.batch)
    wl = WORKLOADS[a.workload]

    # one process per GPU over RCCL ("nccl" on ROCm).  Functional tests on a 1-GPU box run the SAME rank logic with every rank
    # on device PNPFLOW_FORCE_DEVICE and the collectives on gloo (PNPFLOW_DIST_BACKEND=gloo; tensors staged through the host)
    backend = os.environ.get("PNPFLOW_DIST_BACKEND", "nccl")
    if os.environ.get("PNPFLOW_BENCH_DRY") == "1":
        return dry_run(a, rank, world, backend)
    local = int(os.environ.get("PNPFLOW_FORCE_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist_on = world > 1 or a.force_dist
    if dist_on:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            os.environ.setdefault("MASTER_PORT", str(_free_port()))
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        if dist.get_world_size() != a.gpus:
            sys.exit(f"bench.py: process group has {dist.get_world_size()} ranks, --gpus {a.gpus}")
    comm = (lambda t: t) if backend == "nccl" else (lambda t: t.cpu())

    import pnpflow_amd.degradations as D
    from pnpflow_amd.utils import psnr_per_image

    models = {}
    r = Runner(a.workload, rank, world, dev, a.precision, not a.no_graph, models)
    dim, B = wl["dim"], wl["B"]
    for i in range(a.warmup):
        r.step(i)

    def sync():
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
            torch.cuda.synchronize()

    sync()
    sampler = PowerSampler(local).start() if rank == 0 and a.full else None
    t0 = time.perf_counter()
    x = None
    for i in range(a.steps):
        x = r.step(a.warmup + i)
    sync()
    dt = time.perf_counter() - t0
    power = sampler.stop() if sampler else None
    if dist_on:
        tt = comm(torch.tensor([dt], device=dev, dtype=torch.float64))
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())

    if a.dump_outputs:
        xs = x
        if dist_on:
            from pnpflow_amd.parallel import gather_in_image_order
            xs = gather_in_image_order(x.reshape(-1)).view(-1, *x.shape[1:])
        if rank == 0:
            dump_outputs(a.dump_outputs, xs)

    if a.full:
        # the ONE data-path collective: per-image PSNR gathered in global image order
        psnr = psnr_per_image(x, r.clean)
        if dist_on:
            psnr = comm(psnr)
            allp = [torch.empty_like(psnr) for _ in range(world)]
            dist.all_gather(allp, psnr)
            psnr = torch.cat(allp)
        psnr_mean = float(psnr.mean())

    if rank == 0:
        total_images = world * B * a.steps
        out = {
            "metric": "restored images/sec", "value": round(total_images / dt, 4), "unit": "images/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 2),
            "collective_backend": (("rccl (torch.distributed 'nccl')" if backend == "nccl" else backend) if dist_on else None),
            "rccl_version": (".".join(str(v) for v in torch.cuda.nccl.version()) if dist_on and backend == "nccl" else None),
            "ranks_in_job": (dist.get_world_size() if dist_on else 1),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {0: "f32", 1: "f32-equivalent (f16 hi+lo split operands, 3 x f16 MFMA per product, f32 accumulate)",
                      2: "f16 operands (power-of-two scaled), f32 accumulate - TF32-class, not fp32-equivalent"}[a.precision],
            "data": "synthetic",
            "config": {"workload": wl["label"], "image": f"{dim}x{dim}x3", "batch_per_gpu": B, "global_batch": world * B,
                       "steps_pnp": wl["steps"], "num_samples": wl["ns"], "weights": "synthetic seed 0 (no checkpoint offline)",
                       "noise": "on-device Philox4x32-10 (one global stream per (iteration, sample), sliced per shard)",
                       "hipgraph": bool(getattr(r.solver, "use_graph", False)), "unet_batch": r.unet_batch(),
                       "parallelism": f"dp{world} (contiguous shards of the global batch, no data-path collective)"},
        }
        if a.full:
            out.update(psnr_db=round(psnr_mean, 4), power=power,
                       roofline=conv_roofline(r, a.precision, a.workload, measure_traffic=(world == 1 and not a.no_extra)))
        fpi = r.flops_per_image()
        if fpi:
            out["unet_tflops_end_to_end"] = round(total_images * fpi / dt / 1e12, 2)
        # the boxes of the pool differ by up to 7 % in what their matrix pipe delivers under the power cap, and `value` follows that figure to within 1 % (round 6:
        # 3.17 / 3.30 / 3.40 images/s at probes of 1 703 / 1 759 / 1 825 TFLOP/s): the headline per PFLOP/s of THIS box's measured MFMA ceiling is the
        # number that compares runs on different boxes (not a throughput: `value` is)
        mc = (out.get("roofline") or {}).get("mfma_ceiling") or {}
        if world == 1 and mc.get("measured_this_run") and mc.get("tflops_f16_dense"):
            out["roofline"]["mfma_ceiling"]["value_per_box_pflops"] = round(out["value"] / (mc["tflops_f16_dense"] / 1000.0), 4)
        if a.full and not a.no_cpu_baseline and world == 1:
            try:
                out["cpu_baseline"] = cpu_baseline_ot_ode(wl) if r.is_ode else cpu_baseline(wl)
            except Exception as exc:          # noqa: BLE001   (the reported baseline must not take the measured line with it)
                out["cpu_baseline"] = {"error": f"{type(exc).__name__}: {exc}"[:400]}
        if a.full and world == 1 and not a.no_extra and a.workload in ("c2_256", "c2"):
            # the other BASELINE configs under the same clock (EXTRA_STEPS full restorations each after a short warm-up that
            # builds the plans / graph), the headline workload in precision mode 2, and the HBM-side numbers of the pointwise
            # prox kernels
            extra = {}
            EXTRA_STEPS = 3

            def guarded(key, fn):
                # a failure of a secondary measurement must not take the headline line with it: it is recorded in place
                try:
                    extra[key] = fn()
                except Exception as exc:      # noqa: BLE001
                    extra[key] = {"error": f"{type(exc).__name__}: {exc}"[:400]}
                    try:
                        torch.cuda.synchronize()
                    except Exception:          # noqa: BLE001
                        pass

            def timed_steps(rr, n):
                rr.step(0, steps=12 if rr.is_ode else 2)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                xx = None
                for k in range(n):
                    xx = rr.step(1 + k)
                torch.cuda.synchronize()
                return (time.perf_counter() - t1) / n, xx

            def run_config(name):
                rr = Runner(name, 0, 1, dev, a.precision, not a.no_graph, models)
                d1, xx = timed_steps(rr, EXTRA_STEPS)
                w2 = rr.wl
                rec = {"workload": w2["label"], "images_per_s": round(w2["B"] / d1, 4), "ms_per_step": round(d1 * 1e3, 1), "steps": EXTRA_STEPS,
                       "unet_batch": rr.unet_batch(), "psnr_db": round(float(psnr_per_image(xx, rr.clean).mean()), 4),
                       "unet_tflops_end_to_end": round(w2["B"] * rr.flops_per_image() / d1 / 1e12, 2)}
                if not rr.is_ode:
                    rec["roofline"] = conv_roofline(rr, a.precision, name)
                elif not a.no_cpu_baseline:
                    rec["cpu_baseline"] = cpu_baseline_ot_ode(w2, budget_s=12.0)
                return rec

            def run_mode2():
                # the headline workload in precision mode 2 (one fp16 MFMA per product: NOT fp32-equivalent, ~7e-4 relative on the U-Net
                # output; within the BASELINE tolerance of +-0.05 dB PSNR, tests/test_gpu_parity.py::test_fp16_mode_*).  Reported
                # beside the headline, never as `value`.
                rr = Runner(a.workload, 0, 1, dev, 2, not a.no_graph, models)
                try:
                    d1, xx = timed_steps(rr, EXTRA_STEPS)
                    return {"workload": rr.wl["label"] + ", precision mode 2", "dtype": "f16 operands, f32 accumulate (TF32-class)",
                            "images_per_s": round(rr.wl["B"] / d1, 4), "ms_per_step": round(d1 * 1e3, 1), "steps": EXTRA_STEPS,
                            "psnr_db": round(float(psnr_per_image(xx, rr.clean).mean()), 4), "psnr_db_headline_mode": out["psnr_db"],
                            "roofline": conv_roofline(rr, 2, a.workload)}
                finally:
                    rr.model.set_precision(1)

            for name in ("c2", "c3", "c4", "c5"):
                if name != a.workload:
                    guarded(name, lambda name=name: run_config(name))
            if a.precision == 1:
                guarded("headline_fp16_mode", run_mode2)
            guarded("n4_ncsnpp_forward", lambda: ncsnpp_forward_block(dev))
            out["configs"] = extra
            try:
                out["pointwise"] = pointwise_block(dev, D)
            except Exception as exc:          # noqa: BLE001
                out["pointwise"] = {"error": f"{type(exc).__name__}: {exc}"[:400]}
        print(json.dumps(out), flush=True)
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
