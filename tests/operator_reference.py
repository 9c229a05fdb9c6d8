"""Plain fp64 numpy restatement of the degradation operators, the data-fit gradient steps, the OT-ODE solves and the
per-pixel iteration kernels of csrc/pointwise.hip and csrc/fft2.hip, for general (B, C, H, W) with H != W and general
taps g[0..K-1] (tap c = K // 2 sits at offset 0).  The filters are written as sums over np.roll, not as FFT products, so
that they share nothing with the oracle's formulation; they stay valid for K > N, where the filter aliases.

Also the case tables the host and the GPU tests share, and a restatement of the predicate by which `blur2`
(csrc/pointwise.hip) picks one of its three paths.  Imports numpy only.
"""
import numpy as np


# ---------------------------------------------------------------------------------------------
# taps
# ---------------------------------------------------------------------------------------------
def asym_taps(K, seed=0):
    """K positive fp32 taps of sum 1 with no symmetry: convolution and correlation with them differ."""
    g = np.random.Generator(np.random.Philox(key=[seed, K])).random(K) + 0.05
    g = g * np.linspace(0.2, 1.8, K)
    return (g / g.sum()).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------
def _filter_axis(x, g, axis, sign):
    """sign +1: out[i] = sum_k g[k] x[(i - (k - c)) mod N];  sign -1: out[i] = sum_k g[k] x[(i + (k - c)) mod N]"""
    g = np.asarray(g, dtype=np.float64)
    c = len(g) // 2
    out = np.zeros_like(x, dtype=np.float64)
    for k in range(len(g)):
        out += g[k] * np.roll(x, sign * (k - c), axis=axis)      # np.roll(x, s)[i] = x[i - s]
    return out


def blur_H(x, g):
    """circular convolution with outer(g, g): along x, then along y"""
    x = np.asarray(x, dtype=np.float64)
    return _filter_axis(_filter_axis(x, g, -1, +1), g, -2, +1)


def blur_H_adj(w, g):
    """circular correlation with outer(g, g)"""
    w = np.asarray(w, dtype=np.float64)
    return _filter_axis(_filter_axis(w, g, -1, -1), g, -2, -1)


def box_mask(H, W, half):
    """the reference's square mask: the centre H // 2 serves both axes; the hole is clipped at W as slicing clips it"""
    c = H // 2
    m = np.ones((H, W), dtype=np.float64)
    m[c - half:c + half, c - half:c + half] = 0.0
    return m


def decimate(x, sf):
    return np.asarray(x, dtype=np.float64)[..., ::sf, ::sf]


def zerofill(y, sf):
    y = np.asarray(y, dtype=np.float64)
    z = np.zeros(y.shape[:-2] + (y.shape[-2] * sf, y.shape[-1] * sf), dtype=np.float64)
    z[..., ::sf, ::sf] = y
    return z


class Op:
    """kind: 'denoise' | 'box' (half) | 'mask' (mask: (B, H, W) of 0/1) | 'sr' (sf) | 'blur' (taps) | 'sr_filter' (sf, taps)"""

    def __init__(self, kind, half=0, mask=None, sf=1, taps=None):
        self.kind, self.half, self.mask, self.sf, self.taps = kind, half, mask, sf, taps

    def weights(self, H, W):
        """the multiplier of the mask family, broadcastable against (B, C, H, W)"""
        if self.kind == "denoise":
            return np.ones((1, 1, H, W))
        if self.kind == "box":
            return box_mask(H, W, self.half)[None, None]
        if self.kind == "mask":
            return np.asarray(self.mask, dtype=np.float64)[:, None]
        raise ValueError(self.kind)

    def out_shape(self, shape):
        if self.kind in ("sr", "sr_filter"):
            return tuple(shape[:-2]) + (shape[-2] // self.sf, shape[-1] // self.sf)
        return tuple(shape)

    def H(self, x):
        x = np.asarray(x, dtype=np.float64)
        if self.kind in ("denoise", "box", "mask"):
            return self.weights(*x.shape[-2:]) * x
        if self.kind == "sr":
            return decimate(x, self.sf)
        if self.kind == "blur":
            return blur_H(x, self.taps)
        if self.kind == "sr_filter":
            return decimate(blur_H(x, self.taps), self.sf)
        raise ValueError(self.kind)

    def H_adj(self, y):
        y = np.asarray(y, dtype=np.float64)
        if self.kind in ("denoise", "box", "mask"):
            return self.weights(*y.shape[-2:]) * y
        if self.kind == "sr":
            return zerofill(y, self.sf)
        if self.kind == "blur":
            return blur_H_adj(y, self.taps)
        if self.kind == "sr_filter":
            return blur_H_adj(zerofill(y, self.sf), self.taps)
        raise ValueError(self.kind)


def _per_image(v):
    return np.asarray(v, dtype=np.float64).reshape(-1, 1, 1, 1)


def grad_step(op, x, y, coef):
    """z = x - coef[b] H_adj(H x - y)"""
    x = np.asarray(x, dtype=np.float64)
    return x - _per_image(coef) * op.H_adj(op.H(x) - np.asarray(y, dtype=np.float64))


def laplace_sign(r):
    """2 heaviside(r, 0) - 1: an exact zero gives -1"""
    return np.where(r > 0, 1.0, -1.0)


def grad_step_laplace(op, x, y, coef):
    x = np.asarray(x, dtype=np.float64)
    return x - _per_image(coef) * op.H_adj(laplace_sign(op.H(x) - np.asarray(y, dtype=np.float64)))


def blur_filter_2d(g, H, W):
    """outer(g, g) zero-padded to (H, W), tap c rolled to index 0 on both axes (K <= H, W)"""
    g = np.asarray(g, dtype=np.float64)
    K, c = len(g), len(g) // 2
    f = np.zeros((H, W), dtype=np.float64)
    f[:K, :K] = np.outer(g, g)
    return np.roll(f, (-c, -c), axis=(0, 1))


def ot_ode_vec(op, x, vt, y, one_minus_t, rt2, sigma2):
    """H_adj((rt2 H H^T + sigma2)^-1 (y - H(x + (1 - t) vt)))"""
    x1 = np.asarray(x, dtype=np.float64) + _per_image(one_minus_t) * np.asarray(vt, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    r2 = _per_image(rt2)
    if op.kind == "denoise":
        return (y - x1) / (r2 + sigma2)
    if op.kind in ("box", "mask"):
        m = op.weights(*x1.shape[-2:])
        return m * ((y - m * x1) / (m * r2 + sigma2))
    if op.kind == "sr":
        return zerofill((y - decimate(x1, op.sf)) / (r2 + sigma2), op.sf)
    if op.kind == "blur":
        d = y - blur_H(x1, op.taps)
        p = np.abs(np.fft.fft2(blur_filter_2d(op.taps, *x1.shape[-2:]))) ** 2
        sol = np.real(np.fft.ifft2(np.fft.fft2(d) / (r2 * p + sigma2)))
        return blur_H_adj(sol, op.taps)
    raise ValueError(op.kind)


# ---------------------------------------------------------------------------------------------
# per-pixel iteration kernels ((B, n) arrays)
# ---------------------------------------------------------------------------------------------
def interpolate(z, t, eps):
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    return t * np.asarray(z, dtype=np.float64) + (1.0 - t) * np.asarray(eps, dtype=np.float64)


def accumulate(acc, zt, v, t, first, last, num_samples):
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    val = np.asarray(zt, dtype=np.float64) + (1.0 - t) * np.asarray(v, dtype=np.float64)
    if not first:
        val = np.asarray(acc, dtype=np.float64) + val
    return val / num_samples if last else val


def ot_ode_update(x, vt, vec, g, one_minus_t, coef, delta):
    o = np.asarray(one_minus_t, dtype=np.float64).reshape(-1, 1)
    c = np.asarray(coef, dtype=np.float64).reshape(-1, 1)
    x, vt, vec, g = (np.asarray(a, dtype=np.float64) for a in (x, vt, vec, g))
    return x + delta * (vt + c * (vec + o * g))


def psnr(rec, clean):
    """per image, data range 1, after (x + 1) / 2"""
    a = (np.asarray(rec, dtype=np.float64) + 1.0) / 2.0
    b = (np.asarray(clean, dtype=np.float64) + 1.0) / 2.0
    mse = ((a - b) ** 2).reshape(a.shape[0], -1).mean(axis=1)
    return 10.0 * np.log10(1.0 / mse)


# ---------------------------------------------------------------------------------------------
# blur2's path predicate (csrc/pointwise.hip), restated
# ---------------------------------------------------------------------------------------------
def blur_path(H, W, K, fused_enabled=True):
    """'fused32' | 'fused64' | 'two_pass' for an out-of-place application"""
    r = K // 2
    ts = 32 if r <= 8 else 64
    if fused_enabled and K % 2 == 1 and r <= 24 and K < H and K < W and ts + r <= 2 * min(H, W):
        return "fused32" if r <= 8 else "fused64"
    return "two_pass"


# ---------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------
BATCH, CHANNELS = 3, 2
COEF = (0.7, 0.0, 0.25)          # distinct per image, so that a wrong image index shows

# (H, W, K) -> the path of blur2 the case is meant to take
BLUR_CASES = [
    ((37, 50, 15), "fused32"),     # ragged tiles on both axes, W % 4 = 2
    ((33, 35, 15), "fused32"),     # the last tile wraps twice on both axes
    ((16, 20, 1), "fused32"),      # the smallest sizes the predicate admits
    ((20, 23, 3), "fused32"),
    ((70, 45, 43), "fused64"),     # double wrap at y0 = 64
    ((40, 72, 19), "fused64"),     # r = 9, the smallest
    ((52, 60, 49), "fused64"),     # r = 24, the largest, on the opt-in LDS size
    ((24, 36, 8), "two_pass"),     # even taps
    ((66, 130, 61), "two_pass"),   # r > 24
    ((33, 21, 127), "two_pass"),   # K > N, several wraps
    ((16, 40, 15), "two_pass"),    # fails the wrap condition
    ((15, 20, 15), "two_pass"),    # K == H
]

# (H, W, sf, K) -> path of the filter that feeds the decimation
SR_FILTER_CASES = [
    ((24, 36, 2, 8), "two_pass"),
    ((36, 48, 3, 12), "two_pass"),
    ((40, 24, 4, 15), "fused32"),
]

# (kind, half, H, W, C, offset): offset None | "all" (every tensor starts one float past a 16-byte boundary) | "mask" (only the
# byte mask starts one byte past a 4-byte boundary).  `vec4` names the kernels the case is meant to take.
MASK_CASES = []
for _kind, _halves in (("denoise", (0, 0, 0)), ("box", (5, 5, 2)), ("mask", (0, 0, 0))):
    MASK_CASES += [((_kind, _halves[0], 18, 24, 2, None), "vec4"),
                   ((_kind, _halves[1], 18, 23, 2, None), "scalar"),
                   ((_kind, _halves[2], 7, 5, 1, None), "scalar"),
                   ((_kind, _halves[0], 18, 24, 2, "all"), "scalar")]
MASK_CASES += [(("mask", 0, 18, 24, 2, "mask"), "scalar"),
               (("box", 5, 24, 18, 2, None), "scalar"),      # H > W: the column centre is H // 2 = 12, not W // 2 = 9
               (("box", 4, 24, 14, 2, None), "scalar"),      # the hole [8, 16) is clipped at W = 14
               (("box", 0, 18, 24, 2, None), "vec4")]        # an empty hole


def mask_case_path(H, W, offset):
    return "vec4" if W % 4 == 0 and offset is None else "scalar"


# (sf, H, W, C)
SR_CASES = [
    ((3, 24, 24, 2), "vec4"),      # a quad holds one or two samples
    ((4, 24, 36, 2), "vec4"),
    ((8, 16, 24, 2), "vec4"),      # every other quad holds no sample
    ((3, 9, 15, 2), "scalar"),
    ((2, 10, 6, 1), "scalar"),
]

# (H, W, K, C) -> (column transform, row transform) of the Fourier solve
FOURIER_CASES = [
    ((32, 24, 15, 2), ("radix2", "dft")),
    ((24, 32, 9, 2), ("dft", "radix2")),
    ((20, 28, 15, 1), ("dft", "dft")),       # ragged line batches: 20 = 8 + 8 + 4 rows, 28 = 3 * 8 + 4 columns
    ((64, 32, 19, 2), ("radix2", "radix2")),
    ((16, 15, 15, 2), ("radix2", "dft")),    # K == W
]


def fft_path(N):
    return "radix2" if N & (N - 1) == 0 else "dft"
