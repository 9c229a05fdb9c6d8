"""CPU tests of the FID path: the Inception planner (pnpflow_amd/csrc/inception_plan.h through tests/inception_plan_shim.cpp, compiled with
ROCm's host clang++; a missing compiler is a failure), the Frechet distance against the reference's (tests/golden/fid_frechet.npz, written by
tools/make_golden_fid.py), the weight-name loader, ComputeMetric on a fake extractor and a fake sampler, and the C ABI.  No GPU is touched.
"""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import inception_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pnpflow_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "inception_plan_shim.cpp")
OP_CONV, OP_MAXPOOL_S2, OP_AVGPOOL_S1, OP_MAXPOOL_S1 = range(4)


def _host_clang():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for cand in (os.path.join(os.path.dirname(hipcc), "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.isfile(cand):
            return cand
    pytest.fail("no host clang++ next to HIPCC or under /opt/rocm/llvm/bin: the planner test cannot run")


@pytest.fixture(scope="module")
def ip(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("inception_plan") / "libinception_plan_shim.so")
    res = subprocess.run([_host_clang(), "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so, SHIM], capture_output=True, text=True)
    assert res.returncode == 0, "inception_plan.h must compile as plain host C++17:\n" + res.stderr
    lib = C.CDLL(so)
    lib.ip_choose_tile.argtypes = [C.c_longlong, C.c_int]
    return lib


def plan(ip, B, H, W, resize, block):
    head, bufs, err = (C.c_longlong * 10)(), (C.c_longlong * 6)(), C.create_string_buffer(256)
    rc = ip.ip_plan(B, H, W, int(resize), block, head, bufs, err, 256)
    h = dict(zip(("ok", "nops", "nblocks", "nsides", "out_buf", "out_C", "out_H", "out_W", "H0", "W0"), list(head)))
    assert (rc == 0) == bool(h["ok"])
    h["bufs"], h["err"] = list(bufs), err.value.decode()
    a = (B, H, W, int(resize), block)
    h["ops"], h["blocks"], h["sides"] = [], [], []
    for i in range(h["nops"] if h["ok"] else 0):
        v = (C.c_int * 14)()
        assert ip.ip_op(*a, i, v) == 0
        h["ops"].append(dict(zip(("kind", "layer", "src", "src_off", "src_cs", "dst", "dst_off", "dst_cs", "C", "Hi", "Wi", "Ho", "Wo", "tile"), list(v))))
    for i in range(h["nblocks"] if h["ok"] else 0):
        name, head4, sl = C.create_string_buffer(64), (C.c_int * 4)(), (C.c_int * 16)()
        assert ip.ip_block(*a, i, name, 64, head4, sl) == 0
        h["blocks"].append(dict(name=name.value.decode(), width=head4[0], H=head4[1], W=head4[2], slices=[(sl[2 * k], sl[2 * k + 1]) for k in range(head4[3])]))
    for i in range(h["nsides"] if h["ok"] else 0):
        hw = (C.c_int * 2)()
        assert ip.ip_side(*a, i, hw) == 0
        h["sides"].append((hw[0], hw[1]))
    return h


def shim_layers(ip):
    out = []
    for i in range(ip.ip_num_layers()):
        name, dims = C.create_string_buffer(96), (C.c_int * 7)()
        assert ip.ip_layer(i, name, 96, dims) == 0
        out.append((name.value.decode(),) + tuple(dims))
    return out


# ---- 1. the planner ----------------------------------------------------------------------------------------------------------------------
def test_layer_table(ip):
    L = shim_layers(ip)
    assert len(L) == 94
    assert L == R.layer_table()                       # the header and the torch restatement state one table, written twice
    assert len({l[0] for l in L}) == 94
    assert sum(1 for l in L if (l[3], l[4]) == (1, 7)) == sum(1 for l in L if (l[3], l[4]) == (7, 1)) == 4 * 3 + 1      # per C block 3 + 3 and Mixed_7a's pair: 13 each
    assert {l[2] for l in L} >= {48, 80, 320, 448}


def test_block_widths_and_sides(ip):
    p = plan(ip, 2, 75, 75, False, 3)
    assert p["ok"] and sum(o["kind"] == OP_CONV for o in p["ops"]) == 94
    assert [b["name"] for b in p["blocks"]] == ["Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b", "Mixed_7c"]
    assert [b["width"] for b in p["blocks"]] == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
    assert [s[0] for s in p["sides"]] == [37, 35, 35, 17, 17, 15, 7, 3, 1] and all(s[0] == s[1] for s in p["sides"])
    assert (p["out_C"], p["out_H"], p["out_W"]) == (2048, 1, 1)
    q = plan(ip, 1, 299, 299, False, 3)
    assert [s[0] for s in q["sides"]] == [149, 147, 147, 73, 73, 71, 35, 17, 8]
    r = plan(ip, 1, 64, 40, True, 3)                  # resize: the network sees 299 x 299 whatever comes in
    assert r["sides"] == q["sides"] and (r["H0"], r["W0"]) == (299, 299)
    rect = plan(ip, 1, 139, 151, False, 3)            # the two axes propagate on their own
    assert rect["sides"] == [(69, 75), (67, 73), (67, 73), (33, 36), (33, 36), (31, 34), (15, 16), (7, 7), (3, 3)]
    assert [(b["H"], b["W"]) for b in p["blocks"]] == [(7, 7)] * 3 + [(3, 3)] * 5 + [(1, 1)] * 3
    # output blocks: dims and the pixels the average runs over
    for blk, (c, side75) in enumerate(((64, 17), (192, 7), (768, 3), (2048, 1))):
        o = plan(ip, 2, 75, 75, False, blk)
        assert (o["out_C"], o["out_H"]) == (c, side75)
    assert plan(ip, 2, 75, 75, False, 0)["nops"] == 4 and plan(ip, 2, 75, 75, False, 1)["nops"] == 7


def test_slices_tile_each_block_and_buffers_hold_every_tensor(ip):
    for (B, H, W, resize) in ((2, 75, 75, False), (3, 139, 151, False), (1, 64, 64, True)):
        p = plan(ip, B, H, W, resize, 3)
        for b in p["blocks"]:
            cover = np.zeros(b["width"], dtype=int)
            for off, ln in b["slices"]:
                assert 0 <= off and off + ln <= b["width"]
                cover[off:off + ln] += 1
            assert (cover == 1).all(), b["name"]       # no gap, no overlap
        L = shim_layers(ip)
        for o in p["ops"]:
            width = L[o["layer"]][2] if o["kind"] == OP_CONV else o["C"]
            assert 0 <= o["dst_off"] and o["dst_off"] + width <= o["dst_cs"] and o["src_off"] + o["C"] <= o["src_cs"]
            assert B * o["Ho"] * o["Wo"] * o["dst_cs"] <= p["bufs"][o["dst"]] and B * o["Hi"] * o["Wi"] * o["src_cs"] <= p["bufs"][o["src"]]
            assert o["src"] != o["dst"]
            if o["kind"] == OP_CONV:
                (_n, ci, _co, kh, kw, s, ph, pw) = L[o["layer"]]
                assert o["C"] == ci and o["src_cs"] == ci
                assert o["Ho"] == (o["Hi"] + 2 * ph - kh) // s + 1 and o["Wo"] == (o["Wi"] + 2 * pw - kw) // s + 1
                assert o["tile"] == ip.ip_choose_tile(B * o["Ho"] * o["Wo"], L[o["layer"]][2])
        # the pools: two stem max pools, 6a's and 7a's, 3 + 4 + 1 average pools, 7c's stride-1 max pool
        kinds = [o["kind"] for o in p["ops"]]
        assert kinds.count(OP_MAXPOOL_S2) == 4 and kinds.count(OP_AVGPOOL_S1) == 8 and kinds.count(OP_MAXPOOL_S1) == 1
        assert p["ops"][-2]["kind"] == OP_MAXPOOL_S1


def test_tile_rule(ip):
    t = lambda M, N: (ip.ip_tile_mt(ip.ip_choose_tile(M, N)), ip.ip_tile_nt(ip.ip_choose_tile(M, N)))
    # NT = 128 only where it pads Cout no further than 64 does
    assert [t(10 ** 6, n)[1] for n in (32, 48, 64, 80, 96, 128, 192, 320, 384, 448)] == [64, 64, 64, 128, 128, 128, 64, 64, 128, 64]
    # MT = 128 from 256 workgroups on: Cout 384 is 3 column blocks, so 86 row blocks of 128 (M > 85 * 128) are needed
    assert t(85 * 128, 384) == (64, 128) and t(85 * 128 + 1, 384) == (128, 128)
    assert t(2, 192) == (64, 64) and t(1, 2048)[0] == 64


def test_refusals(ip):
    for side in (1, 64, 74):
        for blk in range(4):
            p = plan(ip, 2, side, side, False, blk)
            assert not p["ok"] and "75" in p["err"] and "Mixed_7a" in p["err"]
    assert not plan(ip, 2, 299, 74, False, 3)["ok"]
    assert plan(ip, 2, 75, 75, False, 3)["ok"] and plan(ip, 2, 20, 20, True, 3)["ok"]
    for bad in ((0, 75, 75, False, 3), (2, 75, 75, False, 4), (2, 75, 75, False, -1), (2, 0, 75, True, 3), (100000, 299, 299, False, 3)):
        p = plan(ip, *bad)
        assert not p["ok"] and p["err"]


def test_planner_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "inception_plan_main")
    res = subprocess.run([_host_clang(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DINC_PLAN_MAIN",
                          "-I" + CSRC, "-o", exe, SHIM], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "94 layers: ok" in run.stdout, run.stdout + run.stderr


# ---- 2. the Frechet distance against the reference's --------------------------------------------------------------------------------
def test_frechet_distance_matches_reference(golden):
    from pnpflow_amd import fid_score as fs
    g = golden("fid_frechet")
    n = int(g["n_cases"])
    assert n >= 4
    for i in range(n):
        ours = fs.calculate_frechet_distance(g[f"mu1_{i}"], g[f"s1_{i}"], g[f"mu2_{i}"], g[f"s2_{i}"])
        ref, gap = float(g[f"ref{i}"]), float(g[f"gap{i}"])
        assert gap < 1e-9 * abs(ref)                  # the recorded cases are well conditioned: two fp64 routes agree
        print(f"case {i}: ours {ours:.12f} reference {ref:.12f} |diff| {abs(ours - ref):.3e} (100 x gap = {100 * gap:.3e})")
        assert abs(ours - ref) <= 100 * gap
    # statistics as calculate_activation_statistics forms them, through a feature "model" that returns the stored rows
    a, b = g["a0"], g["b0"]

    class Rows:
        def eval(self):
            return self

        def __call__(self, batch):
            return [batch.double()[:, :, None, None]]
    m1, s1 = fs.calculate_activation_statistics(a, Rows(), 50, a.shape[1], "cpu")
    m2, s2 = fs.calculate_activation_statistics(b, Rows(), 50, b.shape[1], "cpu")
    assert np.array_equal(m1, g["mu1_0"]) and np.array_equal(s1, g["s1_0"]) and np.array_equal(s2, g["s2_0"])
    assert abs(fs.calculate_frechet_distance(m1, s1, m2, s2) - float(g["ref0"])) <= 100 * float(g["gap0"])


def test_frechet_stabilisation_branches(capsys):
    from pnpflow_amd import fid_score as fs
    # identical Gaussians: 0; a rank-deficient product is still finite through sqrtm or its eps retry
    s = np.diag(np.arange(1.0, 9.0))
    assert abs(fs.calculate_frechet_distance(np.zeros(8), s, np.zeros(8), s)) < 1e-9
    assert abs(fs.calculate_frechet_distance(np.ones(8), s, np.zeros(8), s) - 8.0) < 1e-9
    z = np.zeros((4, 4))
    assert np.isfinite(fs.calculate_frechet_distance(np.zeros(4), z, np.zeros(4), z))
    with pytest.raises(AssertionError, match="mean vectors"):
        fs.calculate_frechet_distance(np.zeros(3), np.eye(3), np.zeros(4), np.eye(4))
    # a root with a large imaginary diagonal is refused: C1 C2 with a negative eigenvalue
    with pytest.raises(ValueError, match="Imaginary component"):
        fs.calculate_frechet_distance(np.zeros(2), np.diag([1.0, -1.0]), np.zeros(2), np.eye(2))


def test_get_activations_batching():
    from pnpflow_amd import fid_score as fs
    seen = []

    class Net:
        def eval(self):
            return self

        def __call__(self, batch):
            seen.append(tuple(batch.shape))
            return [batch.mean(dim=1, keepdim=True).repeat(1, 5, 1, 1)]       # (B, 5, H, W): still spatial, get_activations averages it
    x = np.random.default_rng(0).uniform(size=(23, 3, 4, 6)).astype(np.float32)
    act = fs.get_activations(x, Net(), 10, 5, "cpu")
    assert seen == [(10, 3, 4, 6), (10, 3, 4, 6), (3, 3, 4, 6)] and act.shape == (23, 5) and act.dtype == np.float64
    np.testing.assert_allclose(act[:, 0], x.mean(axis=(1, 2, 3)), rtol=1e-6)
    seen.clear()
    fs.get_activations(x[:4], Net(), 50, 5, "cpu")    # batch larger than the data: one batch of all of it
    assert seen == [(4, 3, 4, 6)]


# ---- 3. the weight-name loader ---------------------------------------------------------------------------------------------------------
def test_loader_takes_published_names():
    from pnpflow_amd.models import InceptionV3, find_fid_weights, FID_WEIGHTS_FILE
    assert InceptionV3.BLOCK_INDEX_BY_DIM == {64: 0, 192: 1, 768: 2, 2048: 3} and InceptionV3.DEFAULT_BLOCK_INDEX == 3
    assert InceptionV3.layer_table() == R.layer_table()
    sd = R.synthetic_state_dict(0)
    assert set(InceptionV3.state_dict_shapes()) == set(sd) and len(sd) == 94 * 5
    extra = dict(sd)
    extra.update({"fc.weight": torch.zeros(1008, 2048), "fc.bias": torch.zeros(1008), "AuxLogits.conv0.conv.weight": torch.zeros(128, 768, 1, 1),
                  "Mixed_5b.branch1x1.bn.num_batches_tracked": torch.tensor(0), "module.Conv2d_1a_3x3.conv.weight": sd["Conv2d_1a_3x3.conv.weight"]})
    del extra["Conv2d_1a_3x3.conv.weight"]            # reached through its DataParallel name
    got = InceptionV3.select_weights(extra)
    assert list(got) == list(InceptionV3.state_dict_shapes()) and all(got[k] is sd[k] for k in got)
    missing = dict(sd); del missing["Mixed_6c.branch7x7dbl_3.bn.running_var"]
    with pytest.raises(KeyError, match=r"Mixed_6c\.branch7x7dbl_3\.bn\.running_var"):
        InceptionV3.select_weights(missing)
    with pytest.raises(KeyError, match="unexpected"):
        InceptionV3.select_weights(dict(sd, **{"Mixed_9z.conv.weight": torch.zeros(1)}))
    bad = dict(sd); bad["Mixed_7a.branch3x3_2.conv.weight"] = torch.zeros(320, 192, 3, 1)
    with pytest.raises(ValueError, match="Mixed_7a.branch3x3_2.conv.weight"):
        InceptionV3.select_weights(bad)
    with pytest.raises(ValueError):
        InceptionV3([4])
    with pytest.raises(NotImplementedError):
        InceptionV3([3], use_fid_inception=False)
    assert FID_WEIGHTS_FILE == "pt_inception-2015-12-05-6726825d.pth"


def test_weight_file_search_order_and_synthetic_opt_in(tmp_path, monkeypatch):
    from pnpflow_amd import models as M
    monkeypatch.setenv("HOME", str(tmp_path / "home"))
    monkeypatch.delenv("PNPFLOW_FID_WEIGHTS", raising=False)
    root = str(tmp_path / "out") + "/"
    assert M.find_fid_weights(root) is None
    with pytest.raises(FileNotFoundError, match="synthetic True"):
        M.load_fid_inception([3], output_root=root, synthetic=False)
    hub = tmp_path / "home" / ".cache" / "torch" / "hub" / "checkpoints"; hub.mkdir(parents=True); (hub / M.FID_WEIGHTS_FILE).write_bytes(b"x")
    assert M.find_fid_weights(root) == str(hub / M.FID_WEIGHTS_FILE)
    (tmp_path / "out" / "model").mkdir(parents=True); (tmp_path / "out" / "model" / M.FID_WEIGHTS_FILE).write_bytes(b"x")
    assert M.find_fid_weights(root) == str(tmp_path / "out" / "model" / M.FID_WEIGHTS_FILE)
    env = tmp_path / "env"; env.mkdir(); (env / M.FID_WEIGHTS_FILE).write_bytes(b"x")
    monkeypatch.setenv("PNPFLOW_FID_WEIGHTS", str(env))
    assert M.find_fid_weights(root) == str(env / M.FID_WEIGHTS_FILE)
    monkeypatch.setenv("PNPFLOW_FID_WEIGHTS", str(env / M.FID_WEIGHTS_FILE))
    assert M.find_fid_weights(root) == str(env / M.FID_WEIGHTS_FILE)
    from tools.synthetic_inception import synthetic_inception_state_dict
    sd = synthetic_inception_state_dict(M.InceptionV3.state_dict_shapes())
    again = synthetic_inception_state_dict(M.InceptionV3.state_dict_shapes())
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    for k, v in sd.items():
        if k.endswith(".bn.weight") or k.endswith(".bn.running_var"):
            assert 0.5 <= float(v.min()) and float(v.max()) <= 1.5
    w = sd["Mixed_7b.branch3x3dbl_2.conv.weight"]
    assert abs(float(w.std()) / np.sqrt(2.0 / (448 * 9)) - 1) < 0.02      # He scale


# ---- 4. ComputeMetric on a fake extractor and a fake sampler -------------------------------------------------------------------------
class FakeExtractor:
    """features = (mean, mean of squares, max, min) of the image plus the three channel means: 7 dims"""
    def __init__(self):
        self.batches = []

    def eval(self):
        return self

    def __call__(self, batch):
        self.batches.append(batch.clone())
        f = torch.stack([batch.mean(dim=(1, 2, 3)), (batch ** 2).mean(dim=(1, 2, 3)), batch.amax(dim=(1, 2, 3)), batch.amin(dim=(1, 2, 3))]
                        + [batch[:, c].mean(dim=(1, 2)) for c in range(3)], dim=1)
        return [f[:, :, None, None]]


class FakeSampler:
    def __init__(self, channels):
        self.calls, self.channels = [], channels

    def apply_flow_matching(self, n):
        self.calls.append(n)
        g = torch.Generator().manual_seed(len(self.calls))
        return torch.randn(n, self.channels, 6, 6, generator=g) * 1.5 + 0.5      # well outside [0, 1] on both sides


@pytest.mark.parametrize("channels", [3, 1])
def test_compute_metric_protocol(tmp_path, channels, monkeypatch):
    from pnpflow_amd import compute_metric as CM
    monkeypatch.setattr(CM.InceptionV3, "BLOCK_INDEX_BY_DIM", {7: 0, 64: 0, 192: 1, 768: 2, 2048: 3})      # the fake extractor's 7 dims
    g = torch.Generator().manual_seed(0)
    test_batch = torch.rand(130, channels, 6, 6, generator=g) * 2 - 1              # a loader's [-1, 1] images
    loaders = {"test": [(test_batch, torch.zeros(130)), (torch.zeros(130, channels, 6, 6), torch.zeros(130))]}
    args = types.SimpleNamespace(output_root=str(tmp_path) + "/", dataset="celeba", fid_dims=7)
    ext, smp = FakeExtractor(), FakeSampler(channels)
    cm = CM.ComputeMetric(loaders, smp, "cpu", args, incep_model=ext)
    fid = cm.compute_metrics(120)
    # 50 rounds of 120 // 50 = 2 samples (the remainder of 20 is dropped, as in the reference)
    assert smp.calls == [2] * 50
    # the first 120 images of ONE test batch in batches of 50, then the 100 samples in batches of 50
    assert [b.shape[0] for b in ext.batches] == [50, 50, 20, 50, 50]
    assert all(b.shape[1] == 3 for b in ext.batches)
    real = torch.cat(ext.batches[:3]); gen = torch.cat(ext.batches[3:])
    want = test_batch[:120].expand(-1, 3, -1, -1) if channels == 1 else test_batch[:120]
    assert torch.equal(real, want)                    # as the loader gives them: no rescale, no clip ([-1, 1] values pass through)
    assert float(real.min()) < -0.5
    if channels == 1:
        assert torch.equal(gen[:, 0], gen[:, 1]) and torch.equal(gen[:, 0], gen[:, 2])
    assert float(gen.min()) == 0.0 and float(gen.max()) == 1.0      # clipped to [0, 1]
    # the value: the same statistics by hand
    from pnpflow_amd import fid_score as fs
    f = lambda x: ext(x)[0][:, :, 0, 0].double().numpy()
    fr, fg = f(real), f(gen)
    want_fid = fs.calculate_frechet_distance(fr.mean(0), np.cov(fr, rowvar=False), fg.mean(0), np.cov(fg, rowvar=False))
    assert abs(fid - want_fid) <= 1e-9 * max(1.0, abs(want_fid))
    lines = open(tmp_path / "results" / "celeba" / "metrics.txt").read().splitlines()
    assert lines == [f"Epoch: final, FID: {fid}"] and re.fullmatch(r"Epoch: final, FID: -?\d+(\.\d+)?(e[-+]?\d+)?", lines[0])
    assert "Inception" in open(tmp_path / "results" / "celeba" / "PARITY_UNPINNED.txt").read()
    cm.compute_metrics(100)                           # appended, never overwritten
    assert len(open(tmp_path / "results" / "celeba" / "metrics.txt").read().splitlines()) == 2
    assert len(open(tmp_path / "results" / "celeba" / "PARITY_UNPINNED.txt").read().splitlines()) == 1
    with pytest.raises(ValueError, match="fid_dims"):
        CM.ComputeMetric(loaders, smp, "cpu", types.SimpleNamespace(output_root=str(tmp_path) + "/", dataset="celeba", fid_dims=100), incep_model=ext).compute_metrics(100)
    synth = CM.ComputeMetric(loaders, smp, "cpu", args, incep_model=ext, results_dir="results_synthetic")
    assert synth.save_path == str(tmp_path) + "/results_synthetic/celeba/"


def test_config_and_import_shims():
    from pnpflow_amd.utils import load_cfg_from_cfg_file
    cfg = load_cfg_from_cfg_file(os.path.join(ROOT, "config", "main_config.yaml"))
    assert cfg.compute_metrics is False
    from pnpflow.compute_metric import ComputeMetric
    import pnpflow.fid_score as shim
    from pnpflow.models import InceptionV3
    from pnpflow_amd import compute_metric as CM, fid_score as fs, models as M
    assert ComputeMetric is CM.ComputeMetric and InceptionV3 is M.InceptionV3
    for name in ("get_activations", "calculate_activation_statistics", "calculate_frechet_distance", "evaluate_fid_score"):
        assert getattr(shim, name) is getattr(fs, name)
    src = open(os.path.join(ROOT, "main.py")).read()
    assert "compute_metrics" in src and "fid_samples" in src and "fid_dims" in src


def test_compute_fid_needs_the_engine_extractor():
    from pnpflow_amd.train_flow_matching import FLOW_MATCHING
    fm = FLOW_MATCHING.__new__(FLOW_MATCHING)
    with pytest.raises(NotImplementedError, match="InceptionV3"):
        fm.compute_fid(10, np.zeros((4, 64)), object())


# ---- 5. the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_header_signatures_and_library_agree():
    import pnpflow_amd._lib as L
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "pnpflow_hip.h")).read()
    assert re.search(r"#define PF_ABI_VERSION 6\b", hdr) and L.PF_ABI_VERSION == 6 and lib.pf_abi_version() == 6
    decl = dict(re.findall(r"\b(pf_inception_[a-z_]+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S))
    want = {"pf_inception_create", "pf_inception_destroy", "pf_inception_last_error", "pf_inception_load_weight", "pf_inception_forward", "pf_inception_conv",
            "pf_inception_pool", "pf_inception_front", "pf_inception_profile", "pf_inception_profile_read", "pf_inception_num_layers", "pf_inception_layer"}
    assert set(decl) == want == {k for k in L.SIGNATURES if k.startswith("pf_inception_")}
    for name, params in decl.items():
        n = 0 if params.strip() == "void" else len(params.split(","))
        assert len(L.SIGNATURES[name][1]) == n, name
        assert hasattr(lib, name)
    assert lib.pf_inception_num_layers() == 94
    import __graft_entry__ as G
    assert "inception.hip" in G.SOURCES and set(G.AUDITED) == {"conv_dma.hip", "conv_sp.hip"}
    src = open(os.path.join(CSRC, "inception.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", src)       # builtins only
    # a forward on a handle without weights or with a refused size says why, without a device
    h = C.c_void_p()
    assert lib.pf_inception_create(0, C.byref(h)) == 0
    try:
        assert lib.pf_inception_forward(h, C.c_void_p(16), C.c_void_p(16), 2, 64, 64, 0, 1, 3, None) == -1
        assert b"below 75" in lib.pf_inception_last_error(h)
        assert lib.pf_inception_load_weight(h, b"Mixed_9z.conv.weight", (C.c_float * 1)(), (C.c_int64 * 1)(1), 1) == -3
    finally:
        lib.pf_inception_destroy(h)
