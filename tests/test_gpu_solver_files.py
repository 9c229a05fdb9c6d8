"""The result files of run_method for each of the five solvers (tests/solver_file_cases.py: tiny4 net at 64^2, B = 2, two batches, every
bookkeeping flag on) against tests/golden/solver_files_parent.json, which tools/record_solver_files.py recorded on the commit BEFORE the
solvers' host code moved into pnpflow_amd/methods/_harness.py.  Needs a real MI355X.

The recording was made twice on that commit.  Every PSNR and LPIPS file, every average and every final_*.txt was byte-identical between
the two; they are compared as text.  The per-batch SSIM files were not (pf_ssim accumulates in fp64 atomics, so the last digits depend on
the order the blocks arrive in): the largest difference between the two recordings was 5.6e-17 (pnp_flow), 1.1e-16 (pnp_gs, d_flow,
flow_priors) and 1.7e-16 (ot_ode), on values of 0.003 ... 0.94.  Their value column is compared with 4 x the largest of these,
SSIM_ATOL = 4 x 1.6653345369377348e-16; iteration columns and file names are exact everywhere.
"""
import json
import os

import pytest
import torch

import solver_file_cases as S
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SSIM_ATOL = 4 * 1.6653345369377348e-16

_NET = []


@pytest.fixture(scope="module")
def net():
    import pnpflow_amd._lib as L
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    L.load()
    if not _NET:
        _NET.append(S.new_model())
    return _NET[0]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "solver_files_parent.json")) as f:
        return json.load(f)


def _columns(text):
    rows = [line.split() for line in text.strip().splitlines()]
    assert all(len(r) == 2 for r in rows), text
    return [int(r[0]) for r in rows], [float(r[1]) for r in rows]


@pytest.mark.parametrize("name", list(S.CASES))
def test_run_method_files_match_the_parent_recording(net, recorded, tmp_path, name):
    args, model = S.run_case(name, net, tmp_path)
    got, want = S.collect(tmp_path), recorded[name]
    folder = os.path.relpath(args.save_path_ip, str(tmp_path)).replace(os.sep, "/")
    assert folder == "/".join(f"{k}={v}" for k, v in S.CASES[name][3].items())

    # file names: next to the result folder, and inside it (the image files carry PSNR values in their names: from the recording)
    assert {f for f in got if "/" not in f} == {"final_psnr.txt", "final_ssim.txt", "final_lpips.txt", "PARITY_UNPINNED.txt"}
    texts = {f"{m}_{w}_{k}.txt" for m in ("psnr", "ssim", "lpips") for w in ("rec", "noisy") for k in ("batch0", "batch1", "average")}
    texts |= set(S.STAT_FILES)
    inside = {f[len(folder) + 1:] for f in got if f.startswith(folder + "/")}
    assert {f for f in inside if f.endswith(".txt")} == texts
    assert len(inside) + 4 == len(got) and set(got) == set(want)

    # iteration column of every per-batch metric file: the solver's logging rule, then the final line
    its = S.logging_iterations(name)
    for f in sorted(texts):
        if "_batch" in f:
            assert _columns(got[f"{folder}/{f}"])[0] == its, (f, its)

    # metric values: the parent's
    for f, text in sorted(want.items()):
        if text is None:
            continue
        base = f.rsplit("/", 1)[-1]
        if base.startswith("ssim_") and "_batch" in base:
            (it_g, v_g), (it_w, v_w) = _columns(got[f]), _columns(text)
            worst = max(abs(a - b) for a, b in zip(v_g, v_w))
            print(f"{name} {base}: max |ssim - recorded| = {worst:.3e} (bound {SSIM_ATOL:.3e})")
            assert it_g == it_w and worst <= SSIM_ATOL, (f, worst)
        else:
            assert got[f] == text, f

    # time and memory files
    ip = args.save_path_ip
    t = [eval(l) for l in open(os.path.join(ip, "time_stats.txt")).read().strip().splitlines()]
    assert [r["batch"] for r in t] == [0, 1] and all(r["time_per_batch"] > 0 for r in t)
    mem = [eval(l) for l in open(os.path.join(ip, "memory_stats.txt")).read().strip().splitlines()]
    assert [r["batch"] for r in mem] == [0, 1] and all(r["max_allocated"] >= model.memory_bytes() > 0 for r in mem)
    assert open(os.path.join(ip, "time_average.txt")).read().startswith("average time: ")
    assert open(os.path.join(ip, "max_memory_average.txt")).read().startswith("average mem: ")
