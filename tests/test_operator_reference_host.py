"""Pins tests/operator_reference.py, the fp64 restatement the GPU operator-path tests (tests/test_gpu_operator_paths.py) compare
the kernels with: against the oracle and the reference's golden vectors where those exist (square images, symmetric taps), by
the adjoint identity everywhere else, and proves two things about the GPU cases themselves - that their taps tell convolution
from correlation, and that each case lands on the dispatch branch its table row names.  CPU only."""
import numpy as np
import pytest
import torch

import operator_reference as R
from conftest import det_normal
from oracle import pnpflow_oracle as O


def _np(t):
    return t.numpy().astype(np.float64)


def _normal(shape, seed, idx=0):
    return det_normal(shape, seed, idx).numpy()


def bicubic_taps_1d(sf):
    """1-D factor of the oracle's normalised bicubic filter (outer(w, w) == filter, tests/test_oracle_golden.py)"""
    return O.bicubic_filter(sf)[0, 0].numpy().astype(np.float64).sum(0)


@pytest.mark.parametrize("S", [64, 40])
@pytest.mark.parametrize("sigma", [1.0, 3.0])
def test_blur_matches_oracle(S, sigma):
    if S == 40 and sigma == 3.0:
        K = 31           # the oracle pads the K x K filter into the S x S image
    else:
        K = 61 if S == 64 else 21
    g = O.gaussian_1d_taps(sigma, K)
    do = O.GaussianDeblurring(sigma, K, "fft", 3, S)
    x = det_normal((2, 3, S, S), 21)
    np.testing.assert_allclose(R.blur_H(x.numpy(), g), _np(do.H(x)), rtol=0, atol=1e-6)
    np.testing.assert_allclose(R.blur_H_adj(x.numpy(), g), _np(do.H_adj(x)), rtol=0, atol=1e-6)


@pytest.mark.parametrize("sf", [2, 4])
def test_sr_filtered_matches_oracle(sf):
    S = 64
    op = R.Op("sr_filter", sf=sf, taps=bicubic_taps_1d(sf))
    do = O.Superresolution(sf, S, mode="bicubic")
    x = det_normal((2, 3, S, S), 21); w = det_normal((2, 3, S // sf, S // sf), 24)
    np.testing.assert_allclose(op.H(x.numpy()), _np(do.H(x)), rtol=0, atol=1e-6)
    np.testing.assert_allclose(op.H_adj(w.numpy()), _np(do.H_adj(w)), rtol=0, atol=1e-6)


def test_filtered_operators_match_the_reference_golden(golden):
    g = golden("degradations")
    x64 = _normal((2, 3, 64, 64), 21)
    for sig in (1.0, 3.0):
        taps = O.gaussian_1d_taps(sig, 61)
        np.testing.assert_allclose(R.blur_H(x64, taps), g[f"blur{sig}_H"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(R.blur_H_adj(x64, taps), g[f"blur{sig}_Hadj"], rtol=0, atol=1e-6)
    for sf in (2, 4):
        op = R.Op("sr_filter", sf=sf, taps=bicubic_taps_1d(sf))
        np.testing.assert_allclose(op.H(x64), g[f"srbic{sf}_H"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(op.H_adj(_normal((2, 3, 64 // sf, 64 // sf), 24)), g[f"srbic{sf}_Hadj"], rtol=0, atol=1e-6)
    for half in (10, 20):
        np.testing.assert_array_equal(R.Op("box", half=half).H(x64).astype(np.float32), g[f"box{half}_H"])
    for sf in (2, 4):
        op = R.Op("sr", sf=sf)
        np.testing.assert_array_equal(op.H(x64).astype(np.float32), g[f"sr{sf}_H"])
        np.testing.assert_array_equal(op.H_adj(g[f"sr{sf}_H"]).astype(np.float32), g[f"sr{sf}_Hadj"])


def test_mask_and_decimation_match_oracle_at_non_square_sizes():
    """the oracle's square_mask and slicing take any (H, W): the restated box (centre H // 2 on both axes, clipped at W) and the
    decimation / zero-fill for every sf of the GPU cases"""
    for (kind, half, H, W, Cc, _), _path in R.MASK_CASES:
        if kind != "box":
            continue
        x = det_normal((2, Cc, H, W), 3)
        np.testing.assert_array_equal(R.Op("box", half=half).H(x.numpy()), _np(O.BoxInpainting(half).H(x)))
    for (sf, H, W, Cc), _path in R.SR_CASES:
        x = det_normal((2, Cc, H, W), 4)
        do = O.Superresolution(sf, H)
        np.testing.assert_array_equal(R.decimate(x.numpy(), sf), _np(do.H(x)))
        np.testing.assert_array_equal(R.zerofill(_np(do.H(x)), sf), _np(do.H_adj(do.H(x))))


def test_ot_ode_vec_matches_oracle():
    B, S = 2, 32
    x = det_normal((B, 3, S, S), 81); vt = det_normal((B, 3, S, S), 82)
    t1 = torch.tensor([0.3, 0.65]); omt = 1 - t1
    rt2 = (1 - t1) ** 2 / ((1 - t1) ** 2 + t1 ** 2)
    mask = O.random_mask_array(B, S, S, 0.7)
    for problem, do, op, sigma in (("denoising", O.Denoising(), R.Op("denoise"), 0.2), ("inpainting", O.BoxInpainting(6), R.Op("box", half=6), 0.05),
                                   ("random_inpainting", O.RandomInpainting(0.7), R.Op("mask", mask=mask), 0.01),
                                   ("gaussian_deblurring_FFT", O.GaussianDeblurring(1.0, 9, "fft", 3, S), R.Op("blur", taps=O.gaussian_1d_taps(1.0, 9)), 0.05)):
        y = det_normal(tuple(do.H(x).shape), 84)
        dd = y - do.H(x + omt.view(-1, 1, 1, 1) * vt)
        ref = _np(do.H_adj(O.ot_ode_solution(problem, dd, do, x, t1, sigma, 0.01, 30)))
        got = R.ot_ode_vec(op, x.numpy(), vt.numpy(), y.numpy(), omt.numpy(), rt2.numpy(), sigma ** 2)
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max(), err_msg=problem)
    # decimation: diag(D D^T) = 1
    do, op = O.Superresolution(2, S), R.Op("sr", sf=2)
    y = det_normal((B, 3, S // 2, S // 2), 84)
    dd = y - do.H(x + omt.view(-1, 1, 1, 1) * vt)
    ref = _np(do.H_adj((1 / (rt2.view(-1, 1, 1, 1) + 0.05 ** 2)) * dd))
    got = R.ot_ode_vec(op, x.numpy(), vt.numpy(), y.numpy(), omt.numpy(), rt2.numpy(), 0.05 ** 2)
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max())


def test_psnr_matches_oracle():
    a = det_normal((3, 2, 9, 7), 51).clamp(-1, 1); b = a + 0.05 * det_normal((3, 2, 9, 7), 52)
    np.testing.assert_allclose(R.psnr(b.numpy(), a.numpy()), O.psnr_per_image(b, a).numpy(), atol=1e-4)


# ---------------------------------------------------------------------------------------------
# every case of the GPU tables
# ---------------------------------------------------------------------------------------------
def table_ops():
    """(id, operator, full-resolution shape) of every case the GPU tests run"""
    out = []
    B = R.BATCH
    for (H, W, K), _ in R.BLUR_CASES:
        out.append((f"blur-{H}x{W}-k{K}", R.Op("blur", taps=R.asym_taps(K)), (B, R.CHANNELS, H, W)))
    for (H, W, sf, K), _ in R.SR_FILTER_CASES:
        out.append((f"srf-{H}x{W}-sf{sf}-k{K}", R.Op("sr_filter", sf=sf, taps=R.asym_taps(K)), (B, R.CHANNELS, H, W)))
    for (kind, half, H, W, Cc, off), _ in R.MASK_CASES:
        mask = (np.random.Generator(np.random.Philox(key=[7, H * W])).random((B, H, W)) < 0.7) if kind == "mask" else None
        out.append((f"{kind}{half}-{H}x{W}-c{Cc}-{off}", R.Op(kind, half=half, mask=mask), (B, Cc, H, W)))
    for (sf, H, W, Cc), _ in R.SR_CASES:
        out.append((f"sr{sf}-{H}x{W}-c{Cc}", R.Op("sr", sf=sf), (B, Cc, H, W)))
    for (H, W, K, Cc), _ in R.FOURIER_CASES:
        out.append((f"fourier-{H}x{W}-k{K}", R.Op("blur", taps=R.asym_taps(K)), (B, Cc, H, W)))
    return out


TABLE = table_ops()


@pytest.mark.parametrize("name,op,shape", TABLE, ids=[t[0] for t in TABLE])
def test_adjoint_identity_fp64(name, op, shape):
    x = _normal(shape, 5).astype(np.float64)
    hx = op.H(x)
    w = _normal(hx.shape, 6).astype(np.float64)
    a, b = float((hx * w).sum()), float((x * op.H_adj(w)).sum())
    assert abs(a - b) <= 1e-12 * max(1.0, abs(a)), (name, a, b)


ASYM = [t for t in TABLE if t[1].taps is not None]


@pytest.mark.parametrize("name,op,shape", ASYM, ids=[t[0] for t in ASYM])
def test_taps_tell_convolution_from_correlation(name, op, shape):
    """with the case's own taps and inputs, H and H_adj of the filter differ by far more than any tolerance of the GPU tests"""
    x = _normal(shape, 5)
    moved = float(np.abs(R.blur_H(x, op.taps) - R.blur_H_adj(x, op.taps)).max())
    if len(op.taps) == 1:
        assert moved == 0.0          # a single tap has no direction: the case is there for the predicate's smallest size
        return
    assert moved > 1e-2, (name, moved)
    assert not np.allclose(op.taps, op.taps[::-1], atol=1e-3)
    assert abs(float(op.taps.astype(np.float64).sum()) - 1.0) < 1e-6 and (op.taps > 0).all()


def test_filters_alias_when_the_taps_outnumber_the_pixels():
    """K > N: the roll-sum equals the filter folded onto N taps first"""
    g = R.asym_taps(127).astype(np.float64)
    N = 21
    folded = np.zeros(N)
    for k in range(127):
        folded[(k - 63) % N] += g[k]
    x = _normal((1, 1, 1, N), 9).astype(np.float64)
    want = np.array([sum(folded[m] * x[0, 0, 0, (i - m) % N] for m in range(N)) for i in range(N)])
    np.testing.assert_allclose(R._filter_axis(x, g, -1, +1)[0, 0, 0], want, rtol=0, atol=1e-13)


def test_every_case_lands_on_the_path_its_row_names():
    seen = set()
    for (H, W, K), path in R.BLUR_CASES:
        assert R.blur_path(H, W, K) == path, (H, W, K)
        assert R.blur_path(H, W, K, fused_enabled=False) == "two_pass"
        seen.add(path)
    assert seen == {"fused32", "fused64", "two_pass"}
    for (H, W, sf, K), path in R.SR_FILTER_CASES:
        assert R.blur_path(H, W, K) == path and H % sf == 0 and W % sf == 0, (H, W, sf, K)
    # what the rows say about their cases
    assert R.blur_path(33, 35, 15) == "fused32" and 32 - 7 + 32 + 2 * 7 - 1 >= 2 * 33      # the tile at y0 = 32 stages row 70 >= 2 H
    assert 64 - 21 + 64 + 2 * 21 - 1 >= 2 * 70                                             # (70, 45, 43): the tile at y0 = 64 stages row 148
    assert R.blur_path(16, 20, 1) == "fused32" and R.blur_path(15, 20, 1) == "two_pass"    # the smallest sizes the predicate admits
    assert R.blur_path(20, 23, 3) == "fused32" and R.blur_path(16, 23, 3) == "two_pass"
    assert R.blur_path(40, 72, 17) == "fused32" and R.blur_path(40, 72, 19) == "fused64"   # r = 9 is the first on TS = 64
    assert R.blur_path(52, 60, 49) == "fused64" and R.blur_path(52, 60, 51) == "two_pass"  # r = 24 is the last
    for (kind, half, H, W, Cc, off), path in R.MASK_CASES:
        assert R.mask_case_path(H, W, off) == path, (kind, H, W, off)
        assert half <= H // 2
    assert {p for _, p in R.MASK_CASES} == {"vec4", "scalar"}
    for (sf, H, W, Cc), path in R.SR_CASES:
        assert ("vec4" if W % 4 == 0 else "scalar") == path and H % sf == 0 and W % sf == 0
    for (H, W, K, Cc), (cols, rows) in R.FOURIER_CASES:
        assert (R.fft_path(H), R.fft_path(W)) == (cols, rows) and K <= H and K <= W and H != W
    assert {c for _, c in R.FOURIER_CASES} == {("radix2", "dft"), ("dft", "radix2"), ("dft", "dft"), ("radix2", "radix2")}
