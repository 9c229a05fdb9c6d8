"""CPU test of the weight images (pnpflow_amd/csrc/weight_pack.h): every packer and both host transforms, byte for byte.

tests/weight_pack_shim.cpp (extern "C" wrappers around the header) is compiled with ROCm's host clang++ into a temporary directory
and loaded with ctypes; a missing compiler is a failure.  The expected images are NOT a transliteration of the C++ loops: each one is
built in numpy straight from the index formula documented above its packer - pad / permute the OIHW tensor, name its axes with a
reshape, and transpose them into the order the formula lists - so a wrong index on either side shows up as a mismatch here instead
of as a parity failure deep inside a GPU run.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pnpflow_amd", "csrc")


def _host_clang():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for cand in (os.path.join(os.path.dirname(hipcc), "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.isfile(cand):
            return cand
    pytest.fail("no host clang++ next to HIPCC or under /opt/rocm/llvm/bin: the weight-image test cannot run")


@pytest.fixture(scope="module")
def wp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("weight_pack") / "libweight_pack_shim.so")
    cmd = [_host_clang(), "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so, os.path.join(ROOT, "tests", "weight_pack_shim.cpp")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, "weight_pack.h must compile as plain host C++17:\n" + res.stderr
    lib = C.CDLL(so)
    for name in ("wp_frag32", "wp_slice16", "wp_chunk_pp", "wp_chunk_sp", "wp_edge_frag", "wp_adjoint", "wp_phase_sums"):
        getattr(lib, name).restype = C.c_size_t
    return lib


def call(fn, w, *args, dtype):
    """Runs one shim packer on the OIHW array w [O][I][kk]; returns its image as a flat array of dtype."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    head = [w.ctypes.data_as(C.c_void_p)] + [C.c_int(int(v)) for v in w.shape + tuple(args)]
    size = fn(*head, None, C.c_size_t(0))
    buf = np.full(size, 0xAB, dtype=np.uint8)
    assert fn(*head, buf.ctypes.data_as(C.c_void_p), C.c_size_t(size)) == size
    return buf.view(dtype)


def same_bytes(got, want):
    want = np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    bad = np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))
    assert bad.size == 0, f"{bad.size} differing bytes, first at byte {bad[0]}"


def zero_bytes(a):
    return not np.ascontiguousarray(a).view(np.uint8).any()


def weight(O, I, kk, seed):
    """Seeded normal(0, 0.1) OIHW weight [O][I][kk] with planted zeros, exact powers of two and values that are subnormal (or round
    to zero, or tie) in fp16 after the 2^8 pre-scale."""
    g = np.random.default_rng(seed)
    w = g.normal(0.0, 0.1, size=(O, I, kk)).astype(np.float32)
    special = np.array([0.0, -0.0, 0.5, -1.0, 2.0 ** -10, 2.0 ** -20, 1e-7, -3e-8, 2.3e-9, 2.0 ** -32, 2.0 ** -33, -(2.0 ** -33) * 1.5, 6.1e-5 / 256], dtype=np.float32)
    flat = w.reshape(-1)
    pos = g.choice(flat.size, size=max(flat.size // 8, min(flat.size, special.size)), replace=False)
    flat[pos] = special[np.arange(pos.size) % special.size]
    return w


def split(w):
    w256 = w * np.float32(256)
    hi = w256.astype(np.float16)
    lo = (w256 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def parts(w, terms):
    """[part][...]: the hi image alone at terms 1, hi then lo at terms 3."""
    hi, lo = split(w)
    return np.stack([hi] if terms == 1 else [hi, lo])


# MFMA column n of the persistent kernels carries output channel 4 (n mod 8) + n div 8 of its 32-channel N-tile
COL_CHANNEL = np.array([4 * (n % 8) + n // 8 for n in range(32)])


def padded_slice(w, lo, hi):
    """Input channels [lo, hi) of w, zero-extended to whole 16-channel slices: [O][nchunk * 16][kk]."""
    O, _, kk = w.shape
    nchunk = -(-(hi - lo) // 16)
    pad = np.zeros((O, nchunk * 16, kk), dtype=np.float32)
    pad[:, :hi - lo] = w[:, lo:hi]
    return pad, nchunk


def test_split16_is_the_documented_split(wp):
    vals = np.array([0.0, 0.1, -0.1, 0.5, 1e-7, -3e-8, 2.0 ** -33, 0.3333333, 100.0, 6.1e-5 / 256], dtype=np.float32)
    hi, lo = split(vals)
    for v, h, l in zip(vals, hi, lo):
        out = (C.c_ushort * 2)()
        wp.wp_split16(C.c_float(float(v)), out)
        assert (out[0], out[1]) == (int(h.view(np.uint16)), int(l.view(np.uint16))), float(v)
    # what the split is for: hi + lo carries 256 w to ~2^-22 relative (two 11-bit significands), far inside fp32's rounding of the products
    big = np.abs(vals) > 1e-3
    assert np.all(np.abs(hi[big].astype(np.float64) + lo[big].astype(np.float64) - 256.0 * vals[big]) <= 2.0 ** -21 * np.abs(256.0 * vals[big]))


# (O, I, kk, lo, hi): 3x3 and 1x1 taps, whole and ragged K (hi - lo not a multiple of 16), sub-ranges with lo > 0
SLICES = [(32, 32, 9, 0, 32), (64, 32, 1, 0, 32), (32, 40, 9, 8, 27), (48, 40, 1, 5, 40), (32, 96, 9, 64, 96), (8, 3, 9, 0, 3), (32, 20, 4, 3, 20)]


@pytest.mark.parametrize("O,I,kk,lo,hi", SLICES)
def test_frag32(wp, O, I, kk, lo, hi):
    w = weight(O, I, kk, seed=O + I + kk)
    pad, nchunk = padded_slice(w, lo, hi)
    # img[chunk][tap][kstep][n][j] = w(n, lo + 16 chunk + 8 kstep + j, tap)
    want = pad.reshape(O, nchunk, 2, 8, kk).transpose(1, 4, 2, 0, 3)
    got = call(wp.wp_frag32, w, lo, hi, dtype=np.float32)
    same_bytes(got, want)
    tail = got.reshape(nchunk, kk, 2, O, 8).transpose(0, 2, 4, 1, 3).reshape(nchunk * 16, kk, O)[hi - lo:]
    assert zero_bytes(tail), "the K tail beyond hi must be zero"


@pytest.mark.parametrize("terms", [1, 3])
@pytest.mark.parametrize("O,I,kk,lo,hi", SLICES)
def test_slice16(wp, O, I, kk, lo, hi, terms):
    w = weight(O, I, kk, seed=2 * (O + I + kk))
    pad, nchunk = padded_slice(w, lo, hi)
    P = 1 if terms == 1 else 2
    # img[chunk][tap][part][n][k] = split16(w(n, lo + 16 chunk + k, tap)).part
    want = parts(pad, terms).reshape(P, O, nchunk, 16, kk).transpose(2, 4, 0, 1, 3)
    got = call(wp.wp_slice16, w, lo, hi, terms, dtype=np.float16)
    same_bytes(got, want)
    tail = got.reshape(nchunk, kk, P, O, 16).transpose(0, 4, 1, 2, 3).reshape(nchunk * 16, -1)[hi - lo:]
    assert zero_bytes(tail), "the K tail beyond hi must be zero"


@pytest.mark.parametrize("kk", [9, 1])
@pytest.mark.parametrize("I,lo", [(32, 0), (96, 32), (96, 64)])
def test_chunk_pp(wp, I, lo, kk):
    w = weight(32, I, kk, seed=I + lo + kk)
    # img[tap][j][part][khalf][n][i] = split16(w(col_channel(n), lo + 16 j + 8 khalf + i, tap)).part
    sub = w[COL_CHANNEL][:, lo:lo + 32]                                          # [n][c = 16 j + 8 khalf + i][tap]
    want = parts(sub, 3).reshape(2, 32, 2, 2, 8, kk).transpose(5, 2, 0, 3, 1, 4)     # (part, n, j, khalf, i, tap) -> formula order
    same_bytes(call(wp.wp_chunk_pp, w, lo, dtype=np.float16), want)


@pytest.mark.parametrize("terms", [1, 3])
@pytest.mark.parametrize("kk", [9, 1])
@pytest.mark.parametrize("O,I,lo", [(32, 16, 0), (64, 48, 16), (128, 48, 32), (128, 16, 0)])
def test_chunk_sp(wp, O, I, lo, kk, terms):
    w = weight(O, I, kk, seed=O + I + lo + kk)
    NT, P = O // 32, 1 if terms == 1 else 2
    # img[tap][part][ntile][khalf][n][i] = split16(w(32 ntile + col_channel(n), lo + 8 khalf + i, tap)).part
    sub = w[:, lo:lo + 16].reshape(NT, 32, 16, kk)[:, COL_CHANNEL]                # [ntile][n][c = 8 khalf + i][tap]
    want = parts(sub, terms).reshape(P, NT, 32, 2, 8, kk).transpose(5, 0, 1, 3, 2, 4)
    got = call(wp.wp_chunk_sp, w, lo, NT, terms, dtype=np.float16)
    assert got.size == kk * P * NT * 512
    same_bytes(got, want)


@pytest.mark.parametrize("cimg", [1, 3])
def test_begin_conv_fragments(wp, cimg):
    w = weight(32, cimg, 9, seed=10 + cimg)
    # B[k][n] = w(n, ci, tap) at MFMA k = 9 ci + tap (zero for k >= 9 Cimg), k = 16 kstep + 8 half + j; img[kstep][part][half][n][j]
    B = np.zeros((32, 32), dtype=np.float32)
    B[:9 * cimg] = w.reshape(32, 9 * cimg).T
    want = parts(B, 3).reshape(2, 2, 2, 8, 32).transpose(1, 0, 2, 4, 3)            # (part, kstep, half, j, n) -> formula order
    got = call(wp.wp_edge_frag, w, 1, dtype=np.float16)
    same_bytes(got, want)
    unused = got.reshape(2, 2, 2, 32, 8).transpose(0, 2, 4, 1, 3).reshape(32, -1)[9 * cimg:]
    assert zero_bytes(unused), "MFMA rows beyond 9 Cimg must be zero"


@pytest.mark.parametrize("cimg", [1, 3])
def test_end_conv_fragments(wp, cimg):
    w = weight(cimg, 32, 9, seed=20 + cimg)
    # M[c][n] = w(co, c, tap) at column n = Cimg tap + co (zero for n >= 9 Cimg), channel c = 16 half + 8 kstep + j; img[kstep][part][half][n][j]
    M = np.zeros((32, 32), dtype=np.float32)
    M[:, :9 * cimg] = w.transpose(1, 2, 0).reshape(32, 9 * cimg)
    want = parts(M, 3).reshape(2, 2, 2, 8, 32).transpose(2, 0, 1, 4, 3)            # (part, half, kstep, j, n) -> formula order
    got = call(wp.wp_edge_frag, w, 0, dtype=np.float16)
    same_bytes(got, want)
    unused = got.reshape(2, 2, 2, 32, 8)[:, :, :, 9 * cimg:]
    assert zero_bytes(unused), "MFMA columns beyond 9 Cimg must be zero"


@pytest.mark.parametrize("O,I,kk,lo,hi", [(32, 64, 9, 0, 64), (64, 96, 9, 32, 96), (48, 40, 1, 5, 40), (16, 8, 4, 0, 8)])
def test_adjoint_weight(wp, O, I, kk, lo, hi):
    w = weight(O, I, kk, seed=3 * (O + I + kk))
    # t(ci, co, tap) = w(co, lo + ci, kk - 1 - tap)
    want = w[:, lo:hi].transpose(1, 0, 2)[:, :, ::-1]
    same_bytes(call(wp.wp_adjoint, w, lo, hi, dtype=np.float32), want)


@pytest.mark.parametrize("O,I", [(32, 32), (64, 64), (8, 5)])
def test_phase_sums(wp, O, I):
    w = weight(O, I, 9, seed=5 * O + I)
    w4 = w.reshape(O, I, 3, 3).astype(np.float64)
    R = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}      # (output phase d, window tap t) -> 3x3 indices that read the same source pixel
    want = np.zeros((2, 2, O, I, 2, 2), dtype=np.float32)                # t((2 dy + dx) O + o, i, 2 ty + tx)
    for dy, dx, ty, tx in np.ndindex(2, 2, 2, 2):
        acc = np.zeros((O, I), dtype=np.float64)
        for ky in R[dy, ty]:
            for kx in R[dx, tx]:
                acc = acc + w4[:, :, ky, kx]
        want[dy, dx, :, :, ty, tx] = acc.astype(np.float32)
    same_bytes(call(wp.wp_phase_sums, w, dtype=np.float32), want)
    # the four phases together spend every 3x3 weight exactly once per output phase
    np.testing.assert_allclose(want.astype(np.float64).sum(axis=(4, 5)), np.broadcast_to(w4.sum(axis=(2, 3)), (2, 2, O, I)), rtol=0, atol=1e-6)
