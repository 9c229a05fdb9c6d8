"""GPU tests of the FID Inception network (csrc/inception.hip) and of the FID on top of it.

Reference: tests/inception_reference.py, a plain-torch restatement of the layer table, run on the CPU in fp64 and in fp32 for the same input.
Tolerance, everywhere a number is compared: the HIP result's maximum error against fp64 may be at most 4 x the fp32 CPU run's error against
fp64 plus one fp32 ulp of the output maximum (R.bound; 4 x is the project's margin over a measured fp32 error - the kernel's fp32-input MFMA
sums products in plain fp32, so it should sit at the error of an fp32 run).  Every comparison prints its figures before it asserts.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.25


@pytest.fixture(scope="module")
def hip():
    import pnpflow_amd._lib as L
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return L.load()


@functools.lru_cache(maxsize=None)
def weights():
    return R.synthetic_state_dict(0)


@functools.lru_cache(maxsize=None)
def net(block, resize):
    from pnpflow_amd.models import InceptionV3
    return InceptionV3([block], resize_input=resize, normalize_input=True).load_state_dict(weights())


@functools.lru_cache(maxsize=None)
def reference(B, H, W, resize, seed):
    """(images, fp64 features per block, fp32 features per block): computed once per case, shared by every test of it, never modified"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    x = R.images(B, H, W, seed)
    return x, R.features(weights(), x, resize, True, torch.float64), R.features(weights(), x, resize, True, torch.float32)


def check(what, hip_out, ref64, ref32):
    err, allowed, err32 = R.bound(hip_out.cpu(), ref64, ref32)
    print(f"{what}: max|hip - fp64| {err:.3e}  fp32 CPU error {err32:.3e}  ratio {err / err32 if err32 else float('nan'):.2f}  allowed {allowed:.3e}  "
          f"max|out| {float(ref64.abs().max()):.3e}")
    assert torch.isfinite(hip_out).all()
    assert err <= allowed, f"{what}: {err:.3e} > {allowed:.3e} (fp32 CPU error {err32:.3e})"


# ---- 1. one conv launch, every branch ------------------------------------------------------------------------------------------------
#        (Cin, Cout, KH, KW, stride, PH, PW, B, H, W)
CONVS = {
    "stem_3to32_s2": (3, 32, 3, 3, 2, 0, 0, 2, 19, 19),           # K = 27: not a multiple of the chunk, scalar staging
    "80to192_3x3": (80, 192, 3, 3, 1, 0, 0, 1, 9, 9),
    "48to64_5x5": (48, 64, 5, 5, 1, 2, 2, 1, 7, 7),               # Cout below one N-tile
    "128_1x7": (128, 128, 1, 7, 1, 0, 3, 3, 5, 5),                # zero padding on the x axis only
    "160to192_7x1": (160, 192, 7, 1, 1, 3, 0, 1, 3, 3),           # ... on the y axis only, taller than the image
    "768to192_1x1_M2": (768, 192, 1, 1, 1, 0, 0, 2, 1, 1),        # M = 2
    "448to384_3x3": (448, 384, 3, 3, 1, 1, 1, 1, 2, 2),           # K = 4032, Cin and Cout no multiple of 128
    "288to384_s2": (288, 384, 3, 3, 2, 0, 0, 1, 7, 7),
    "2048to320_1x1": (2048, 320, 1, 1, 1, 0, 0, 1, 8, 8),         # Cout = 5 x 64
}


def conv_case(name):
    (ci, co, kh, kw, s, ph, pw, B, H, W) = CONVS[name]
    g = np.random.Generator(np.random.Philox(key=[11, sum(map(ord, name))]))
    x = torch.from_numpy(np.maximum(g.standard_normal((B, ci, H, W)), -0.2).astype(np.float32))       # mostly-positive activations, like a ReLU's output
    w = torch.from_numpy((g.standard_normal((co, ci, kh, kw)) * np.sqrt(2.0 / (ci * kh * kw))).astype(np.float32))
    bn = [torch.from_numpy(g.uniform(lo, hi, co).astype(np.float32)) for lo, hi in ((0.5, 1.5), (-0.1, 0.1), (-0.1, 0.1), (0.5, 1.5))]      # weight, bias, mean, var
    return x, w, bn, (s, ph, pw)


def conv_ref(x, w, bn, geo, dtype):
    s, ph, pw = geo
    y = F.conv2d(x.to(dtype), w.to(dtype), None, stride=s, padding=(ph, pw))
    return F.relu(F.batch_norm(y, bn[2].to(dtype), bn[3].to(dtype), bn[0].to(dtype), bn[1].to(dtype), False, 0.0, R.BN_EPS))


def fold(bn):
    sc = bn[0].double() / torch.sqrt(bn[3].double() + R.BN_EPS)
    return sc.float().cuda(), (bn[1].double() - bn[2].double() * sc).float().cuda()


def hip_conv(hip, x, w, bn, geo, out=None, out_off=0, tile=-1):
    """x NCHW on the CPU -> NCHW result of pf_inception_conv on the slice [out_off, out_off + Cout) of `out` (NHWC on the GPU; made when None)"""
    s, ph, pw = geo
    B, ci, H, W = x.shape
    co, _, kh, kw = w.shape
    Ho, Wo = (H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw) // s + 1
    xin = x.permute(0, 2, 3, 1).contiguous().cuda()
    if out is None:
        out = torch.full((B, Ho, Wo, co), SENTINEL, dtype=torch.float32, device="cuda")
    sc, sh = fold(bn)
    wh = np.ascontiguousarray(w.numpy())
    rc = hip.pf_inception_conv(xin.data_ptr(), wh.ctypes.data, sc.data_ptr(), sh.data_ptr(), out.data_ptr(), B, H, W, ci, co, kh, kw, s, ph, pw, out_off, out.shape[3],
                               tile, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out[..., out_off:out_off + co].permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("name", list(CONVS))
def test_conv_branches(hip, name):
    x, w, bn, geo = conv_case(name)
    ref64, ref32 = conv_ref(x, w, bn, geo, torch.float64), conv_ref(x, w, bn, geo, torch.float32)
    got = hip_conv(hip, x, w, bn, geo)
    assert got.shape == ref64.shape
    check(f"conv {name}", got, ref64, ref32)
    for tile in range(4):                              # every tile instantiation: the same bits (a pixel's sum does not depend on the tile)
        assert torch.equal(hip_conv(hip, x, w, bn, geo, tile=tile), got), f"tile {tile} differs from the planner's choice"


def test_conv_writes_its_channel_slice_only(hip):
    """384 -> 384 (1,3) and (3,1) at offsets 0 and 384 of a 768-wide tensor (Mixed_7b / 7c's inner concatenation), and at 192 of a 1024-wide
    one: the sentinel survives everywhere else"""
    g = np.random.Generator(np.random.Philox(key=[12, 0]))
    B, H, W = 2, 3, 2
    x = torch.from_numpy(np.maximum(g.standard_normal((B, 384, H, W)), -0.2).astype(np.float32))
    out = torch.full((B, H, W, 768), SENTINEL, dtype=torch.float32, device="cuda")
    for off, (kh, kw, ph, pw) in ((0, (1, 3, 0, 1)), (384, (3, 1, 1, 0))):
        w = torch.from_numpy((g.standard_normal((384, 384, kh, kw)) * np.sqrt(2.0 / (384 * 3))).astype(np.float32))
        bn = [torch.from_numpy(g.uniform(lo, hi, 384).astype(np.float32)) for lo, hi in ((0.5, 1.5), (-0.1, 0.1), (-0.1, 0.1), (0.5, 1.5))]
        geo = (1, ph, pw)
        before = out.clone()
        got = hip_conv(hip, x, w, bn, geo, out=out, out_off=off)
        check(f"conv 384->384 ({kh},{kw}) at offset {off}", got, conv_ref(x, w, bn, geo, torch.float64), conv_ref(x, w, bn, geo, torch.float32))
        keep = torch.ones(768, dtype=torch.bool, device="cuda"); keep[off:off + 384] = False
        assert torch.equal(out[..., keep], before[..., keep])
    assert not (out == SENTINEL).any()
    wide = torch.full((B, H, W, 1024), SENTINEL, dtype=torch.float32, device="cuda")
    hip_conv(hip, x, w, bn, geo, out=wide, out_off=192)
    assert (wide[..., :192] == SENTINEL).all() and (wide[..., 576:] == SENTINEL).all() and torch.equal(wide[..., 192:576], out[..., 384:])
    # refusals: nothing is launched
    sc, sh = fold(bn)
    xin = x.permute(0, 2, 3, 1).contiguous().cuda()
    wh = np.ascontiguousarray(w.numpy())
    bad = lambda **k: hip.pf_inception_conv(xin.data_ptr(), wh.ctypes.data, sc.data_ptr(), sh.data_ptr(), wide.data_ptr(), B, H, W, 384, 384, 3, 1, 1, 1, 0,
                                            k.get("off", 0), k.get("cs", 1024), k.get("tile", -1), None)
    assert bad(off=700) == -1 and bad(cs=100) == -1 and bad(tile=4) == -1


# ---- 2. pools and the front end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [3, 8])
def test_pools(hip, side):
    g = np.random.Generator(np.random.Philox(key=[13, side]))
    B, Cc = 2, 40
    x = torch.from_numpy(g.standard_normal((B, Cc, side, side)).astype(np.float32))
    total = torch.from_numpy(g.standard_normal((B, side, side, 64)).astype(np.float32)).cuda()        # the slice [8, 48) of a 64-wide tensor is read
    total[..., 8:48] = x.permute(0, 2, 3, 1).cuda()
    refs = {2: lambda t: F.avg_pool2d(t, 3, 1, 1, count_include_pad=False), 3: lambda t: F.max_pool2d(t, 3, 1, 1), 1: lambda t: F.max_pool2d(t, 3, 2)}
    for kind, fn in refs.items():
        So = (side - 3) // 2 + 1 if kind == 1 else side
        out = torch.full((B, So, So, 50), SENTINEL, dtype=torch.float32, device="cuda")
        assert hip.pf_inception_pool(total.data_ptr(), out.data_ptr(), B, Cc, side, side, kind, 8, 64, 5, 50, None) == 0
        torch.cuda.synchronize()
        got = out[..., 5:45].permute(0, 3, 1, 2).contiguous().cpu()
        assert (out[..., :5] == SENTINEL).all() and (out[..., 45:] == SENTINEL).all()
        if kind == 2:
            check(f"avgpool {side}x{side} (count_include_pad=False)", got, fn(x.double()), fn(x))
        else:
            assert torch.equal(got, fn(x)), f"maxpool kind {kind} at {side}"
    assert hip.pf_inception_pool(total.data_ptr(), total.data_ptr(), B, Cc, 2, 2, 1, 0, 64, 0, 64, None) == -1       # no 3 x 3 window in a 2 x 2 image


@pytest.mark.parametrize("H,W", [(64, 64), (300, 300), (299, 299), (75, 139)])
def test_front_end(hip, H, W):
    x = R.images(2, H, W, 5)
    out = torch.empty((2, 299, 299, 3), dtype=torch.float32, device="cuda")
    assert hip.pf_inception_front(x.cuda().data_ptr(), out.data_ptr(), 2, H, W, 1, 1, None) == 0
    torch.cuda.synchronize()
    ref = lambda t: 2 * F.interpolate(t, size=(299, 299), mode="bilinear", align_corners=False) - 1
    check(f"resize {H}x{W} -> 299", out.permute(0, 3, 1, 2).cpu(), ref(x.double()), ref(x))
    plain = torch.empty((2, H, W, 3), dtype=torch.float32, device="cuda")
    assert hip.pf_inception_front(x.cuda().data_ptr(), plain.data_ptr(), 2, H, W, 0, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(plain.permute(0, 3, 1, 2).cpu(), x)       # layout change alone: the same bits


# ---- 3. the whole network ----------------------------------------------------------------------------------------------------------------
NETS = {"75": (2, 75, 75, False), "139": (3, 139, 139, False), "64_resized": (2, 64, 64, True)}


@pytest.mark.parametrize("block", [0, 1, 2, 3])
@pytest.mark.parametrize("case", list(NETS))
def test_whole_network(hip, case, block):
    B, H, W, resize = NETS[case]
    x, f64, f32 = reference(B, H, W, resize, 21)
    got = net(block, resize).features(x.cuda(), block)
    assert got.shape == (B, R.BLOCK_DIMS[block])
    check(f"network {case} block {block}", got, f64[block], f32[block])
    out = net(block, resize)(x.cuda())                 # the reference's call: a list with one (B, dims, 1, 1) tensor per requested block
    assert len(out) == 1 and out[0].shape == (B, R.BLOCK_DIMS[block], 1, 1) and torch.equal(out[0][:, :, 0, 0], got)


def test_refusals_and_missing_weights(hip):
    import pnpflow_amd._lib as L
    from pnpflow_amd.models import InceptionV3
    with pytest.raises(L.PnpFlowHipError, match="below 75"):
        net(3, False).features(torch.zeros(2, 3, 74, 74, device="cuda"), 3)
    with pytest.raises(L.PnpFlowHipError, match="no CPU path"):
        net(3, False).features(torch.zeros(2, 3, 75, 75), 3)
    empty = InceptionV3([3])
    with pytest.raises(L.PnpFlowHipError, match="not loaded: Conv2d_1a_3x3"):
        empty.features(torch.zeros(1, 3, 75, 75, device="cuda"), 3)


# ---- 4. / 5. batch invariance and regrow ---------------------------------------------------------------------------------------------
def test_batch_invariance(hip):
    x = R.images(5, 75, 75, 31).cuda()
    for block in (0, 3):
        n = net(block, False)
        together = n.features(x, block)
        for i in range(5):
            assert torch.equal(n.features(x[i:i + 1], block)[0], together[i]), f"image {i} of the batch differs from the same image alone (block {block})"


def test_regrow(hip):
    from pnpflow_amd.models import InceptionV3
    n = InceptionV3([3], resize_input=False).load_state_dict(weights())        # a handle of its own: its buffers start empty
    small, big = R.images(2, 75, 75, 41).cuda(), R.images(3, 139, 139, 42).cuda()
    first = n.features(small, 3).clone()
    middle = n.features(big, 3).clone()
    last = n.features(small, 3).clone()
    assert torch.equal(first, last)
    _x, f64, f32 = reference(3, 139, 139, False, 42)
    check("regrown 139", middle, f64[3], f32[3])


# ---- 6. the FID end to end at 64 dimensions ---------------------------------------------------------------------------------------------
def test_fid_end_to_end_dims64(hip):
    from pnpflow_amd import fid_score as fs
    a, b = R.images(128, 75, 75, 51), (R.images(128, 75, 75, 52) * 0.8 + 0.1)
    n = net(0, False)
    stats = lambda feats: (feats.mean(axis=0), np.cov(feats, rowvar=False))
    fid = {}
    for dtype in (torch.float64, torch.float32):
        fa = R.features(weights(), a, False, True, dtype, last_block=0)[0].double().numpy()
        fb = R.features(weights(), b, False, True, dtype, last_block=0)[0].double().numpy()
        fid[dtype] = float(fs.calculate_frechet_distance(*stats(fa), *stats(fb)))
    m1, s1 = fs.calculate_activation_statistics(a, n, 50, 64, "cuda")
    m2, s2 = fs.calculate_activation_statistics(b, n, 50, 64, "cuda")
    got = float(fs.calculate_frechet_distance(m1, s1, m2, s2))
    err, err32 = abs(got - fid[torch.float64]), abs(fid[torch.float32] - fid[torch.float64])
    allowed = 4 * err32 + float(np.spacing(np.float32(fid[torch.float64])))
    print(f"FID dims 64: hip {got:.9f} fp64 {fid[torch.float64]:.9f} fp32 {fid[torch.float32]:.9f}  error {err:.3e}  fp32 pipeline error {err32:.3e}  allowed {allowed:.3e}")
    assert np.isfinite(got) and err <= allowed


# ---- 7. main.py ---------------------------------------------------------------------------------------------------------------------------
def test_main_compute_metrics(hip, tmp_path):
    """`python main.py --opts ... compute_metrics True fid_samples 100 fid_dims 64 synthetic True ...` in a fresh process (output_root moved to a temporary
    folder, as the other main.py tests do): one FID line under results_synthetic/, then the restoration as before."""
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--opts", "dataset", "celeba", "model", "ot", "compute_metrics", "True", "fid_samples", "100", "fid_dims", "64",
           "synthetic", "True", "max_batch", "1", "batch_size_ip", "2", "output_root", str(tmp_path) + "/"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = open(tmp_path / "results_synthetic" / "celeba" / "metrics.txt").read().splitlines()
    assert len(lines) == 1 and lines[0].startswith("Epoch: final, FID: ")
    assert np.isfinite(float(lines[0].split("FID: ")[1]))
    assert (tmp_path / "results_synthetic" / "celeba" / "PARITY_UNPINNED.txt").is_file()
    assert not (tmp_path / "results").exists()
    base = tmp_path / "results_synthetic" / "celeba" / "ot" / "superresolution" / "pnp_flow"
    found = {p.name for p in base.rglob("*") if p.is_file()}
    assert "psnr_rec_batch0.txt" in found, found         # the restoration ran after the metric
    assert r.stdout.index("Computing metrics done") < r.stdout.index("Solving the superresolution inverse problem")
