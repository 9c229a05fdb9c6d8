"""Look at a flow-prior checkpoint: a grid of samples drawn from it and a bits/dim table of images under it.

    python tools/prior_report.py --opts dataset celeba model ot [n_samples 16] [integration_method dopri5] [integration_steps 100] [seed 0] [fid N] [fid_dims 2048]
    python tools/prior_report.py --opts dataset celebahq model rectified [n_samples 16] [use_ode_sampler rk45|euler] [sample_N 100] [sigma_variance 0] [ode_tol 1e-5]

Uses main.py's config surface (config/main_config.yaml, the dataset YAML, then --opts) to build the net and to find the checkpoint
`<output_root>model/<dataset>/<model>/model_final.pt` and the test images.  Like main.py it FAILS when either is missing, unless
`--opts synthetic True` opts into seed-fixed synthetic weights / images; the report then goes under `results_synthetic/`.

Writes `<output_root>results[_synthetic]/<dataset>/<model>/prior_report/`:
    samples.png      n_samples draws (FLOW_MATCHING.generate_samples; `model rectified`: the rectified-flow sampler of image_generation/sampling.py
                     on the config's sampling fields, which the four sampler options override), postprocessed to [0, 1]
    bits_per_dim.txt one row per image: bits/dim, delta_logp, accepted / rejected steps and evaluations of its batch (get_likelihood_fn_rf)
    fid.txt          with `fid N`: the FID of N prior samples against N test images (compute_metric.ComputeMetric at fid_dims features; its own
                     `Epoch: final, FID:` line goes to results[_synthetic]/<dataset>/metrics.txt as main.py's does)
"""
import argparse
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args():
    from pnpflow_amd.utils import load_cfg_from_cfg_file, merge_cfg_from_list
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--opts', default=None, nargs=argparse.REMAINDER)
    a = parser.parse_args()
    cfg = load_cfg_from_cfg_file(os.path.join(ROOT, 'config', 'main_config.yaml'))
    extra = dict(n_samples=16, integration_method="dopri5", integration_steps=100, tol=1e-5, n_images=None, fid=0, fid_dims=2048,
                 use_ode_sampler=None, sample_N=None, sigma_variance=None, ode_tol=None)
    kinds = dict(n_images=int, use_ode_sampler=str, sample_N=int, sigma_variance=float, ode_tol=float)      # of the options whose default is None
    opts = list(a.opts or [])
    for k in list(extra):          # report-only options: taken out of --opts before the config merge (which knows main.py's keys only)
        if k in opts:
            i = opts.index(k)
            extra[k] = type(extra[k])(opts[i + 1]) if extra[k] is not None else kinds[k](opts[i + 1])
            del opts[i:i + 2]
    cfg = merge_cfg_from_list(cfg, opts)
    cfg.update(load_cfg_from_cfg_file(os.path.join(ROOT, 'config', 'dataset_config', f'{cfg.dataset}.yaml')))
    cfg = merge_cfg_from_list(cfg, opts)
    cfg.update(extra)
    return cfg


def main():
    args = parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pnpflow_amd needs an MI355X (there is no CPU path)")
    device = torch.device("cuda", 0)
    if args.seed is not None:
        random.seed(args.seed); torch.manual_seed(args.seed); np.random.seed(args.seed)
    from main import SyntheticLoader, prior_sampler
    from pnpflow_amd import utils
    from pnpflow_amd.dataloaders import DataLoaders
    from pnpflow_amd.image_generation.likelihood import get_likelihood_fn_rf

    synthetic = bool(getattr(args, "synthetic", False))
    args.device_index = 0
    (model, state) = utils.define_model(args)
    model_path = args.output_root + 'model/{}/{}/model_final.{}'.format(args.dataset, args.model, 'pth' if args.model == 'rectified' else 'pt')
    real = os.path.isfile(model_path)
    if real:
        utils.load_model(args.model, model, state, download=False, checkpoint_path=model_path, dataset=None, device=device)
    elif synthetic:
        print(f"[prior_report] synthetic=True: checkpoint {model_path} not found, using SYNTHETIC weights (the figures are not meaningful)")
        from tools.synthetic_weights import synthetic_state_dict
        model.load_state_dict(synthetic_state_dict(model))
    else:
        raise FileNotFoundError(f"{model_path} not found. Pass `--opts synthetic True` to run on seed-fixed synthetic weights instead.")
    n_images = args.n_images or args.batch_size_ip
    dl = DataLoaders(args.dataset, n_images, n_images, root=args.root)
    if dl.available(args.eval_split):
        loader = dl.load_data()[args.eval_split]
    elif synthetic:
        print(f"[prior_report] synthetic=True: dataset files {dl.paths()} not found, using SYNTHETIC images")
        loader, real = SyntheticLoader(n_images, args.num_channels, args.dim_image, 1), False
    else:
        raise FileNotFoundError(f"dataset files {dl.paths()} not found. Pass `--opts synthetic True` to run on synthetic images instead.")
    out = os.path.join(args.output_root, 'results' if real else 'results_synthetic', args.dataset, args.model, 'prior_report')
    os.makedirs(out, exist_ok=True)

    # samples
    fm = prior_sampler(args, model, device)
    if args.model == "rectified":
        imgs = fm.generate_samples(args.n_samples, batch_size=args.batch_size_ip)
    else:
        imgs = fm.generate_samples(args.integration_method, tol=args.tol, n_samples=args.n_samples, batch_size=args.batch_size_ip,
                                   num_channels=args.num_channels, integration_steps=args.integration_steps)
    model.check_numerics()
    grid = utils.postprocess(imgs, args).clamp(0, 1).permute(0, 2, 3, 1).cpu().numpy()          # (B, H, W, C), as save_images hands it over
    utils._imshow_grid(os.path.join(out, "samples.png"), grid, gray=args.num_channels == 1)

    # bits/dim
    likelihood_fn = get_likelihood_fn_rf()
    (clean, _labels) = next(iter(loader))
    bpd, z, nfe = likelihood_fn(model, clean.to(device))
    st, dlp = likelihood_fn.last_stats, likelihood_fn.last_delta_logp.cpu().numpy()
    with open(os.path.join(out, "bits_per_dim.txt"), "w") as f:
        f.write(f"# checkpoint {model_path if os.path.isfile(model_path) else 'SYNTHETIC'}; RK45 rtol = atol = 1e-5, t 1 -> 1e-5; "
                f"{st['accepted']} accepted + {st['rejected']} rejected steps, {nfe} evaluations\n# image bits/dim delta_logp\n")
        for i, (b, d) in enumerate(zip(bpd.cpu().numpy(), dlp)):
            f.write(f"{i} {b:.6f} {d:.4f}\n")
        f.write(f"# mean {float(bpd.mean()):.6f}\n")
    if args.fid:
        from pnpflow_amd.compute_metric import ComputeMetric
        from pnpflow_amd.models import find_fid_weights
        fdl = DataLoaders(args.dataset, args.fid, args.fid, root=args.root)
        if fdl.available('test'):
            fid_loaders, fid_real = fdl.load_data(), real
        elif synthetic:
            fid_loaders, fid_real = {'test': SyntheticLoader(args.fid, args.num_channels, args.dim_image, 1)}, False
        else:
            raise FileNotFoundError(f"dataset files {fdl.paths()} not found. Pass `--opts synthetic True` to run on synthetic images instead.")
        fid_real = fid_real and find_fid_weights(args.output_root) is not None
        metric = ComputeMetric(fid_loaders, fm, device, args, results_dir='results' if fid_real else 'results_synthetic')
        fid = metric.compute_metrics(args.fid)
        with open(os.path.join(out, "fid.txt"), "w") as f:
            f.write(f"# FID of {args.fid // 50 * 50} prior samples against {args.fid} test images, {args.fid_dims} Inception features"
                    f"{'' if fid_real else ' (SYNTHETIC weights or images: not comparable with anything)'}\n{fid}\n")
        print(f"[prior_report] FID ({args.fid} samples, {args.fid_dims} features): {fid} -> {out}/fid.txt")
    print(f"[prior_report] {args.n_samples} samples -> {out}/samples.png; mean bits/dim {float(bpd.mean()):.4f} over {bpd.numel()} images "
          f"({nfe} evaluations) -> {out}/bits_per_dim.txt")


if __name__ == "__main__":
    main()
