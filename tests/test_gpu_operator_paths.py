"""Every dispatch branch of the operator and per-pixel kernels (csrc/pointwise.hip, csrc/fft2.hip), through the C ABI, against the
fp64 restatement of tests/operator_reference.py: non-square images, asymmetric taps (convolution and correlation differ by
0.06 ... 0.9 with them), misaligned pointers.  Needs a real MI355X:  python -m pytest tests/test_gpu_operator_paths.py -m gpu

B = 3 images, C = 2 channels unless a case says otherwise, per-image coefficients (0.7, 0.0, 0.25).  Tolerances are the project's own
(tests/test_gpu_parity.py): H / H_adj of the mask and SR family bit exact; filtered operators 1e-5 absolute; gradient steps 2e-5;
pf_ot_ode_vec closed forms rtol 2e-5 + 2e-5 max|ref|; the Fourier solve 5e-5 max|ref|.

The branch each case is meant to take (tests/test_operator_reference_host.py proves the mapping from the restated predicates):

  blur (PF_DEG_GAUSSIAN_BLUR; H, H_adj, pf_grad_step = modes 1 + 2, pf_grad_step_laplace = modes 3 + 2), (H, W, K):
    (37, 50, 15)   blur2d_fused_kernel<32>   ragged tiles on both axes, W % 4 = 2
    (33, 35, 15)   blur2d_fused_kernel<32>   the last tile wraps twice on both axes while staging
    (16, 20, 1)    blur2d_fused_kernel<32>   the smallest sizes the predicate admits
    (20, 23, 3)    blur2d_fused_kernel<32>
    (70, 45, 43)   blur2d_fused_kernel<64>   double wrap at y0 = 64
    (40, 72, 19)   blur2d_fused_kernel<64>   r = 9, the smallest
    (52, 60, 49)   blur2d_fused_kernel<64>   r = 24, the largest, on the opt-in LDS size
    (24, 36, 8)    blur_rows + blur_cols     even taps
    (66, 130, 61)  blur_rows + blur_cols     r > 24
    (33, 21, 127)  blur_rows + blur_cols     K > N: the staged line wraps several times
    (16, 40, 15)   blur_rows + blur_cols     TS + r > 2 min(H, W)
    (15, 20, 15)   blur_rows + blur_cols     K == H
    the seven fused cases once more in a child process with PNPFLOW_HIP_BLUR_FUSED=0: blur_rows + blur_cols, modes 0 - 3
  SR-filtered (PF_DEG_SR_FILTERED; sr_residual_kernel in both gradient steps), (H, W, sf, K):
    (24, 36, 2, 8), (36, 48, 3, 12)   two-pass filter;   (40, 24, 4, 15)   fused filter feeds the decimation
  mask family (denoising, box, byte mask; H, H_adj, both gradient steps, pf_ot_ode_vec):
    (18, 24)                          mask_apply4_kernel / grad_step_mask4_kernel
    (18, 23), (7, 5) with C = 1       mask_apply_kernel / grad_step_mask_kernel (W % 4 != 0)
    (18, 24), every tensor + 4 bytes  the scalar kernels (misaligned tensors)
    (18, 24), mask pointer + 1 byte   the scalar kernels (misaligned byte mask)
    box 5 at (24, 18), box 4 at (24, 14) (hole clipped at W), box 0 at (18, 24)
  plain super-resolution (H, H_adj, both gradient steps, pf_ot_ode_vec), (sf, H, W):
    (3, 24, 24), (4, 24, 36), (8, 16, 24)    grad_step_sr4_kernel (a quad holds two, one or no sample)
    (3, 9, 15), (2, 10, 6) with C = 1        grad_step_sr_kernel
  Fourier solve (pf_ot_ode_vec of the blur), (H, W, K): columns / rows
    (32, 24, 15) radix-2 / DFT;  (24, 32, 9) DFT / radix-2;  (20, 28, 15), C = 1: DFT / DFT, ragged line batches;
    (64, 32, 19) radix-2 / radix-2;  (16, 15, 15) radix-2 / DFT, K == W
  per-pixel: pf_denoise_accumulate's scalar branch (B == 1; n % 4 != 0; acc misaligned), pf_interpolate and pf_ot_ode_update at
    n % 4 != 0, normals_at's r != 0 branch and the high words of the Philox counter / stream / seed, pf_psnr at n < 1024 and n % 1024 != 0
"""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import operator_reference as R
from conftest import det_normal
from oracle import pnpflow_oracle as O

pytestmark = pytest.mark.gpu

KINDS = {"denoise": 0, "box": 1, "mask": 2, "sr": 3, "blur": 4, "sr_filter": 5}
SENTINEL = 123.0


@pytest.fixture(scope="module")
def hip():
    import pnpflow_amd._lib as L
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    L.load()                      # raises if libpnpflow_hip.so is missing - no fallback
    return L


# ---------------------------------------------------------------------------------------------
# device buffers and the ABI
# ---------------------------------------------------------------------------------------------
def dev(a, offset=False):
    """fp32 device copy; offset: the data start one float past a 16-byte boundary (a view [1:] of a buffer one element longer)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not offset:
        return torch.from_numpy(a).cuda()
    v = torch.empty(a.size + 1, device="cuda")[1:]
    v.copy_(torch.from_numpy(a).reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v.view(a.shape)


def out_buf(shape, offset=False):
    return dev(np.full(shape, np.nan, dtype=np.float32), offset)


def scratch_buf(n):
    return torch.full((max(int(n), 1),), float("nan"), device="cuda")


def descriptor(L, op, shape, mask_offset=False):
    """(pf_degradation, the device tensors it points into)"""
    d = L.PfDegradation(); keep = []
    d.kind = KINDS[op.kind]; d.half_size_mask = int(op.half); d.sf = int(op.sf) if op.kind in ("sr", "sr_filter") else 0
    if op.taps is not None:
        t = torch.from_numpy(np.asarray(op.taps, dtype=np.float32)).cuda()
        d.ntaps = int(t.numel()); d.taps = t.data_ptr(); keep.append(t)
    if op.kind == "mask":
        m = torch.from_numpy(np.ascontiguousarray(op.mask, dtype=np.uint8))
        if mask_offset:
            v = torch.empty(m.numel() + 1, dtype=torch.uint8, device="cuda")[1:]
            v.copy_(m.reshape(-1))
            assert v.data_ptr() % 4 == 1
        else:
            v = m.cuda()
        d.mask = v.data_ptr(); keep.append(v)
    return d, keep


def scratch_floats(op, shape, what):
    S = int(np.prod(shape))
    if what == "vec":
        return 4 * S + shape[2] + shape[3] if op.kind == "blur" else 0
    if op.kind not in ("blur", "sr_filter"):
        return 0
    if what in ("grad", "laplace") or op.kind == "sr_filter":
        return 2 * S
    return S


def run(L, op, shape, what, data, offset=None):
    """one ABI call -> (status, output as numpy)"""
    lib = L.load()
    B, Cc, H, W = shape
    off = offset == "all"
    d, keep = descriptor(L, op, shape, mask_offset=offset == "mask")
    n_scr = scratch_floats(op, shape, what)
    scr = scratch_buf(n_scr) if n_scr else None
    sp = scr.data_ptr() if scr is not None else None
    st = L.current_stream_ptr()
    if what == "H":
        x, out = dev(data["x"], off), out_buf(op.out_shape(shape), off)
        rc = lib.pf_degradation_H(C.byref(d), x.data_ptr(), out.data_ptr(), B, Cc, H, W, sp, st)
    elif what == "H_adj":
        w, out = dev(data["w"], off), out_buf(shape, off)
        rc = lib.pf_degradation_H_adj(C.byref(d), w.data_ptr(), out.data_ptr(), B, Cc, H, W, sp, st)
    elif what in ("grad", "laplace"):
        x, y, cf, out = dev(data["x"], off), dev(data["y_g" if what == "grad" else "y_l"], off), dev(data["coef"]), out_buf(shape, off)
        fn = lib.pf_grad_step if what == "grad" else lib.pf_grad_step_laplace
        rc = fn(C.byref(d), x.data_ptr(), y.data_ptr(), cf.data_ptr(), out.data_ptr(), B, Cc, H, W, sp, st)
    elif what == "vec":
        x, vt, y, out = dev(data["x"], off), dev(data["vt"], off), dev(data["y_g"], off), out_buf(shape, off)
        om, r2 = dev(data["omt"]), dev(data["rt2"])
        rc = lib.pf_ot_ode_vec(C.byref(d), x.data_ptr(), vt.data_ptr(), y.data_ptr(), om.data_ptr(), r2.data_ptr(), data["sigma2"],
                               out.data_ptr(), B, Cc, H, W, sp, st)
    else:
        raise ValueError(what)
    torch.cuda.synchronize()
    del keep
    return rc, out.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# inputs and fp64 references, computed once per case
# ---------------------------------------------------------------------------------------------
T1 = np.array([0.3, 0.65, 0.9])
_DATA = {}


def case_data(key, op, shape, ties):
    """ties False: the Laplace measurement is H_ref(x) + delta, |delta| >= 0.05, so no residual is near a tie and the comparison is
    complete.  ties True (operators whose H is exact in fp32): the measurement is bit-equal to H(x) on a checkerboard half of the
    samples - those must take sign -1 - and H(x) + delta on the rest."""
    if key in _DATA:
        return _DATA[key]
    seed = 100 + zlib.crc32(key.encode()) % 100000
    x = det_normal(shape, seed, 0).numpy()
    hx = op.H(x)
    yshape = hx.shape
    n = det_normal(yshape, seed, 3).numpy().astype(np.float64)
    delta = np.where(n >= 0, 1.0, -1.0) * (0.05 + np.abs(n))
    if ties:
        assert np.array_equal(hx.astype(np.float32).astype(np.float64), hx)
        idx = np.indices(yshape)
        delta = np.where((idx[1] + idx[2] + idx[3]) % 2 == 0, 0.0, delta)
    omt = (1.0 - T1).astype(np.float32)
    d = dict(x=x, w=det_normal(yshape, seed, 1).numpy(), y_g=det_normal(yshape, seed, 2).numpy(), y_l=(hx + delta).astype(np.float32),
             vt=det_normal(shape, seed, 4).numpy(), coef=np.array(R.COEF, dtype=np.float32), omt=omt,
             rt2=((1 - T1) ** 2 / ((1 - T1) ** 2 + T1 ** 2)).astype(np.float32), sigma2=0.05 ** 2)
    r = np.abs(hx - d["y_l"].astype(np.float64))
    assert (r[delta != 0] >= 0.049).all() and (r[delta == 0] == 0).all() and (not ties or (delta == 0).sum() >= delta.size // 2)
    d["ref"] = {"H": hx}
    _DATA[key] = d
    return d


def reference(data, op, what):
    ref = data["ref"]
    if what not in ref:
        if what == "H_adj":
            ref[what] = op.H_adj(data["w"])
        elif what == "grad":
            ref[what] = R.grad_step(op, data["x"], data["y_g"], data["coef"])
        elif what == "laplace":
            ref[what] = R.grad_step_laplace(op, data["x"], data["y_l"], data["coef"])
        else:
            ref[what] = R.ot_ode_vec(op, data["x"], data["vt"], data["y_g"], data["omt"], data["rt2"], float(np.float32(data["sigma2"])))
    return ref[what]


def check(L, key, op, shape, what, ties=False, offset=None):
    data = case_data(key, op, shape, ties)
    rc, got = run(L, op, shape, what, data, offset)
    assert rc == 0, (key, what, rc)
    ref = reference(data, op, what)
    assert got.shape == ref.shape
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{key} {what}: max|hip - fp64| = {err:.3e}")
    filtered = op.taps is not None
    if what in ("H", "H_adj"):
        if filtered:
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-5, err_msg=f"{key} {what}")
        else:
            assert np.array_equal(got, ref.astype(np.float32)), f"{key} {what}: not bit exact (max error {err:.3e})"
    elif what in ("grad", "laplace"):
        np.testing.assert_allclose(got, ref, rtol=0, atol=2e-5, err_msg=f"{key} {what}")
    elif filtered:
        np.testing.assert_allclose(got, ref, rtol=0, atol=5e-5 * float(np.abs(ref).max()), err_msg=f"{key} {what}")
    else:
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5 * float(np.abs(ref).max()), err_msg=f"{key} {what}")
    return got, data


def blur_case(case):
    H, W, K = case
    return f"blur-{H}x{W}-k{K}", R.Op("blur", taps=R.asym_taps(K)), (R.BATCH, R.CHANNELS, H, W)


FOUR = ["H", "H_adj", "grad", "laplace"]


# ---------------------------------------------------------------------------------------------
# blur path matrix
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", FOUR)
@pytest.mark.parametrize("case,path", R.BLUR_CASES, ids=[f"{p}-{c[0]}x{c[1]}-k{c[2]}" for c, p in R.BLUR_CASES])
def test_blur_paths(hip, case, path, what):
    assert R.blur_path(*case) == path
    check(hip, *blur_case(case), what)


def test_blur_two_pass_switch_in_a_fresh_process(hip):
    """PNPFLOW_HIP_BLUR_FUSED=0 (the test-only switch of INTEGRATION.md) sends the fused-eligible cases through blur_rows_kernel +
    blur_cols_kernel - odd taps, and modes 1 and 3, which the even-tap filters never give that path.  The switch is read once per
    process, hence the child."""
    env = dict(os.environ, PNPFLOW_HIP_BLUR_FUSED="0")
    res = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    n = sum(1 for _, p in R.BLUR_CASES if p != "two_pass")
    assert n >= 6 and f"two-pass switch ok: {4 * n} checks" in res.stdout, res.stdout[-3000:]


def _child_main():
    import pnpflow_amd._lib as L
    assert os.environ.get("PNPFLOW_HIP_BLUR_FUSED") == "0" and torch.cuda.is_available()
    L.load()
    done = 0
    for case, path in R.BLUR_CASES:
        if path == "two_pass":
            continue
        assert R.blur_path(*case, fused_enabled=False) == "two_pass"
        for what in FOUR:
            check(L, *blur_case(case), what)
            done += 1
    print(f"two-pass switch ok: {done} checks")


# ---------------------------------------------------------------------------------------------
# SR-filtered
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", FOUR)
@pytest.mark.parametrize("case,path", R.SR_FILTER_CASES, ids=[f"{p}-{c[0]}x{c[1]}-sf{c[2]}-k{c[3]}" for c, p in R.SR_FILTER_CASES])
def test_sr_filtered(hip, case, path, what):
    H, W, sf, K = case
    assert R.blur_path(H, W, K) == path
    check(hip, f"srf-{H}x{W}-sf{sf}-k{K}", R.Op("sr_filter", sf=sf, taps=R.asym_taps(K)), (R.BATCH, R.CHANNELS, H, W), what)


# ---------------------------------------------------------------------------------------------
# mask family
# ---------------------------------------------------------------------------------------------
def byte_mask(B, H, W):
    return (np.random.Generator(np.random.Philox(key=[7, H * W])).random((B, H, W)) < 0.7).astype(np.uint8)


@pytest.mark.parametrize("what", FOUR + ["vec"])
@pytest.mark.parametrize("case,path", R.MASK_CASES, ids=[f"{c[0]}{c[1]}-{c[2]}x{c[3]}-c{c[4]}-{c[5]}-{p}" for c, p in R.MASK_CASES])
def test_mask_family(hip, case, path, what):
    kind, half, H, W, Cc, offset = case
    assert R.mask_case_path(H, W, offset) == path and half <= H // 2
    op = R.Op(kind, half=half, mask=byte_mask(R.BATCH, H, W) if kind == "mask" else None)
    got, data = check(hip, f"{kind}{half}-{H}x{W}-c{Cc}", op, (R.BATCH, Cc, H, W), what, ties=True, offset=offset)
    if what == "laplace":
        # the ties themselves: where the sample is kept and y == m x bit for bit, the step is exactly x + coef
        m = np.broadcast_to(op.weights(H, W), got.shape)
        tie = (data["y_l"] == (m * data["x"]).astype(np.float32)) & (m == 1)
        assert tie.sum() >= got.size // 8
        cf = np.broadcast_to(data["coef"].reshape(-1, 1, 1, 1), got.shape)
        assert np.array_equal(got[tie], (data["x"] + cf)[tie].astype(np.float32))


# ---------------------------------------------------------------------------------------------
# plain super-resolution
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", FOUR + ["vec"])
@pytest.mark.parametrize("case,path", R.SR_CASES, ids=[f"sf{c[0]}-{c[1]}x{c[2]}-c{c[3]}-{p}" for c, p in R.SR_CASES])
def test_plain_superresolution(hip, case, path, what):
    sf, H, W, Cc = case
    got, data = check(hip, f"sr{sf}-{H}x{W}-c{Cc}", R.Op("sr", sf=sf), (R.BATCH, Cc, H, W), what, ties=True)
    if what == "laplace":
        tie = R.zerofill((data["y_l"] == data["x"][..., ::sf, ::sf]).astype(np.float64), sf) == 1
        assert tie.sum() >= data["y_l"].size // 2
        cf = np.broadcast_to(data["coef"].reshape(-1, 1, 1, 1), got.shape)
        assert np.array_equal(got[tie], (data["x"] + cf)[tie].astype(np.float32))


@pytest.mark.parametrize("H,W", [(10, 12), (9, 10)])
def test_superresolution_refuses_sizes_the_factor_does_not_divide(hip, H, W):
    lib = hip.load()
    B, Cc, sf = R.BATCH, R.CHANNELS, 3
    assert H % sf or W % sf
    d = hip.PfDegradation(); d.kind = KINDS["sr"]; d.sf = sf
    x = det_normal((B, Cc, H, W), 61).cuda(); y = det_normal((B, Cc, H // sf + 1, W // sf + 1), 62).cuda()
    cf, om, r2 = dev(np.array(R.COEF)), dev(1 - T1), dev(T1)
    st = hip.current_stream_ptr()
    big = torch.full((B, Cc, H, W), SENTINEL, device="cuda"); small = torch.full_like(y, SENTINEL)
    assert lib.pf_degradation_H(C.byref(d), x.data_ptr(), small.data_ptr(), B, Cc, H, W, None, st) != 0
    assert lib.pf_degradation_H_adj(C.byref(d), y.data_ptr(), big.data_ptr(), B, Cc, H, W, None, st) != 0
    assert lib.pf_grad_step(C.byref(d), x.data_ptr(), y.data_ptr(), cf.data_ptr(), big.data_ptr(), B, Cc, H, W, None, st) != 0
    assert lib.pf_grad_step_laplace(C.byref(d), x.data_ptr(), y.data_ptr(), cf.data_ptr(), big.data_ptr(), B, Cc, H, W, None, st) != 0
    assert lib.pf_ot_ode_vec(C.byref(d), x.data_ptr(), x.data_ptr(), y.data_ptr(), om.data_ptr(), r2.data_ptr(), 0.0025, big.data_ptr(),
                             B, Cc, H, W, None, st) != 0
    torch.cuda.synchronize()
    assert bool((big == SENTINEL).all()) and bool((small == SENTINEL).all())


# ---------------------------------------------------------------------------------------------
# Fourier solve, non-square
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,paths", R.FOURIER_CASES, ids=[f"{c[0]}x{c[1]}-k{c[2]}-cols_{p[0]}-rows_{p[1]}" for c, p in R.FOURIER_CASES])
def test_fourier_solve_non_square(hip, case, paths):
    H, W, K, Cc = case
    assert (R.fft_path(H), R.fft_path(W)) == paths
    op = R.Op("blur", taps=R.asym_taps(K))
    got, data = check(hip, f"fourier-{H}x{W}-k{K}", op, (R.BATCH, Cc, H, W), "vec")
    # the size-independent identity of test_ot_ode_fourier_solve_sizes, evaluated in fp64 on the kernel's result:
    # rt2 H(H_adj(vec)) + sigma2 vec == H_adj(d),  d = y - H(x + (1 - t) vt)
    vec = got.astype(np.float64)
    r2 = data["rt2"].astype(np.float64).reshape(-1, 1, 1, 1)
    x1 = data["x"].astype(np.float64) + data["omt"].astype(np.float64).reshape(-1, 1, 1, 1) * data["vt"]
    rhs = op.H_adj(data["y_g"] - op.H(x1))
    lhs = r2 * op.H(op.H_adj(vec)) + float(np.float32(data["sigma2"])) * vec
    np.testing.assert_allclose(lhs, rhs, rtol=0, atol=2e-4 * float(np.abs(rhs).max()))


def test_fourier_solve_refusals(hip):
    lib = hip.load()
    B, Cc, H, W, K = R.BATCH, R.CHANNELS, 32, 12, 15
    op = R.Op("blur", taps=R.asym_taps(K))
    d, keep = descriptor(hip, op, (B, Cc, H, W))
    x = det_normal((B, Cc, H, W), 71).cuda()
    om, r2 = dev(1 - T1), dev(T1)
    vec = torch.full((B, Cc, H, W), SENTINEL, device="cuda")
    scr = scratch_buf(4 * x.numel() + H + W)
    st = hip.current_stream_ptr()
    assert K > W
    assert lib.pf_ot_ode_vec(C.byref(d), x.data_ptr(), x.data_ptr(), x.data_ptr(), om.data_ptr(), r2.data_ptr(), 0.0025, vec.data_ptr(),
                             B, Cc, H, W, scr.data_ptr(), st) != 0                       # K > W
    assert lib.pf_ot_ode_vec(C.byref(d), x.data_ptr(), x.data_ptr(), x.data_ptr(), om.data_ptr(), r2.data_ptr(), 0.0025, vec.data_ptr(),
                             B, Cc, W, H, scr.data_ptr(), st) != 0                       # K > H
    d2, keep2 = descriptor(hip, R.Op("blur", taps=R.asym_taps(9)), (B, Cc, H, W))
    assert lib.pf_ot_ode_vec(C.byref(d2), x.data_ptr(), x.data_ptr(), x.data_ptr(), om.data_ptr(), r2.data_ptr(), 0.0025, vec.data_ptr(),
                             B, Cc, H, W, None, st) != 0                                 # no workspace
    torch.cuda.synchronize()
    assert bool((vec == SENTINEL).all())


# ---------------------------------------------------------------------------------------------
# per-pixel kernels
# ---------------------------------------------------------------------------------------------
def _t(B):
    return np.array([0.31, 0.0, 0.99][:B], dtype=np.float32)


@pytest.mark.parametrize("B,n,offset", [(1, 3072, False), (3, 105, False), (2, 8, True)], ids=["B1", "n105", "acc_misaligned"])
def test_denoise_accumulate_scalar_branches(hip, B, n, offset):
    """first / middle / last over three distinct samples; 2e-6 as tests/test_gpu_parity.py::test_interpolate_and_accumulate"""
    lib = hip.load()
    t = _t(B); td = dev(t)
    acc = dev(np.full((B, n), SENTINEL), offset)
    ref = np.full((B, n), SENTINEL, dtype=np.float64)
    for s, mode in enumerate((1, 0, 2)):
        zt, v = det_normal((B, n), 41, s).numpy(), det_normal((B, n), 43, s).numpy()
        ztd, vd = dev(zt), dev(v)
        assert lib.pf_denoise_accumulate(acc.data_ptr(), ztd.data_ptr(), vd.data_ptr(), td.data_ptr(), mode, 3.0, B, n, hip.current_stream_ptr()) == 0
        ref = R.accumulate(ref, zt, v, t, first=bool(mode & 1), last=bool(mode & 2), num_samples=3.0)
        torch.cuda.synchronize()
        np.testing.assert_allclose(acc.cpu().numpy(), ref, rtol=0, atol=2e-6, err_msg=f"mode {mode}")


@pytest.mark.parametrize("B,n", [(3, 105), (1, 5)])
def test_interpolate_ragged_sizes(hip, B, n):
    """1e-6 with injected noise, 2e-5 with the engine's normals, as tests/test_gpu_parity.py::test_interpolate_and_accumulate"""
    lib = hip.load()
    z, eps, t = det_normal((B, n), 44).numpy(), det_normal((B, n), 45).numpy(), _t(B)
    zd, ed, td = dev(z), dev(eps), dev(t)
    zt = out_buf((B, n))
    assert lib.pf_interpolate(zd.data_ptr(), td.data_ptr(), ed.data_ptr(), 0, 0, zt.data_ptr(), B, n, hip.current_stream_ptr()) == 0
    np.testing.assert_allclose(zt.cpu().numpy(), R.interpolate(z, t, eps), rtol=0, atol=1e-6)
    zt = out_buf((B, n))
    assert lib.pf_interpolate(zd.data_ptr(), td.data_ptr(), None, 1234, 77, zt.data_ptr(), B, n, hip.current_stream_ptr()) == 0
    e = O.engine_normal(B * n, 1234, 77).reshape(B, n)
    np.testing.assert_allclose(zt.cpu().numpy(), R.interpolate(z, t, e), rtol=0, atol=2e-5)


def test_ot_ode_update_ragged_size(hip):
    lib = hip.load()
    B, n, delta = 3, 105, 0.01
    x, vt, vec, g = (det_normal((B, n), 46, i).numpy() for i in range(4))
    omt, coef = (1 - T1).astype(np.float32), np.array([1.7, 0.0, 0.4], dtype=np.float32)
    xd, vtd, vecd, gd, od, cd = dev(x), dev(vt), dev(vec), dev(g), dev(omt), dev(coef)
    assert lib.pf_ot_ode_update(xd.data_ptr(), vtd.data_ptr(), vecd.data_ptr(), gd.data_ptr(), od.data_ptr(), cd.data_ptr(), delta, B, n,
                                hip.current_stream_ptr()) == 0
    ref = R.ot_ode_update(x, vt, vec, g, omt, coef, float(np.float32(delta)))
    np.testing.assert_allclose(xd.cpu().numpy(), ref, rtol=0, atol=1e-6)


NORMAL_SEED, NORMAL_STREAM = 99, 5
NORMAL_OFFSETS = {1: 1, 2: 4 * 37 + 2, 3: 4 * 1000 + 3}


@pytest.fixture(scope="module")
def whole_stream(hip):
    n = max(NORMAL_OFFSETS.values()) + 1001
    out = torch.empty(n, device="cuda")
    assert hip.load().pf_fill_normal(out.data_ptr(), n, NORMAL_SEED, NORMAL_STREAM, hip.current_stream_ptr()) == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 1001])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_fill_normal_at_unaligned_offsets(hip, whole_stream, r, n):
    off = NORMAL_OFFSETS[r]
    assert off % 4 == r
    out = out_buf((n + 2,))
    assert hip.load().pf_fill_normal_at(out.data_ptr(), n, NORMAL_SEED, NORMAL_STREAM, off, hip.current_stream_ptr()) == 0
    got = out.cpu().numpy()
    assert np.isnan(got[n:]).all()                   # nothing past n is written
    np.testing.assert_allclose(got[:n], O.engine_normal(n, NORMAL_SEED, NORMAL_STREAM, off), rtol=0, atol=2e-5)
    assert np.array_equal(got[:n], whole_stream[off:off + n])


def test_fill_normal_at_uses_the_high_words(hip):
    seed, stream, off, n = (7 << 32) | 99, (3 << 32) | 5, (1 << 34) + 4 * 5 + 3, 1001
    out = out_buf((n,))
    assert hip.load().pf_fill_normal_at(out.data_ptr(), n, seed, stream, off, hip.current_stream_ptr()) == 0
    got = out.cpu().numpy()
    np.testing.assert_allclose(got, O.engine_normal(n, seed, stream, off), rtol=0, atol=2e-5)
    # each high word changes the draw, so the comparison above sees all three
    lo = 0xFFFFFFFF
    for other in (O.engine_normal(n, seed & lo, stream, off), O.engine_normal(n, seed, stream & lo, off), O.engine_normal(n, seed, stream, off & (4 * lo + 3))):
        assert np.abs(other - got).max() > 1.0


@pytest.mark.parametrize("n", [5, 1000, 3 * 50 * 70])
@pytest.mark.parametrize("B", [1, 3])
def test_psnr_sizes(hip, B, n):
    a = np.clip(0.5 * det_normal((B, n), 51).numpy(), -1, 1); b = (a + 0.05 * det_normal((B, n), 52).numpy()).astype(np.float32)
    ad, bd = dev(a), dev(b)
    out = out_buf((B,))
    assert hip.load().pf_psnr(bd.data_ptr(), ad.data_ptr(), out.data_ptr(), B, n, hip.current_stream_ptr()) == 0
    np.testing.assert_allclose(out.cpu().numpy(), R.psnr(b, a), rtol=0, atol=1e-4)


if __name__ == "__main__":
    _child_main()
