"""References of the batched GMRES (pf_krylov_solve, csrc/krylov.hip) for every kind it is documented for: the case table the GPU tests
(tests/test_gpu_krylov_paths.py) and the fixture tool (tools/make_golden_spatial.py gmres_paths) share, the right-hand sides, fp64 forms of
A = rt2[b] H H^T + sigma2 and the EXACT fp64 solutions of A sol = rhs.  No exact solution needs a dense n x n matrix but the smallest case:

  kinds 0, 1, 2   H H^T is the 0/1 mask:                      sol = rhs / (rt2 m + sigma2)
  kinds 4, 7      H H^T is circulant with eigenvalues |K^|^2:   sol = ifft2(fft2(rhs) / (rt2 |K^|^2 + sigma2))
  kind 6          H H^T = (Th Th^T) (x) (Tw Tw^T), Th / Tw the 1-D zero-boundary correlation matrices: two small eigh,
                  sol = Uh [(Uh^T R Uw) / (rt2 lh lw^T + sigma2)] Uw^T
  kind 8          not separable: the dense per-channel matrix of H from fp64 direct sums, numpy.linalg.solve (H W <= 200 only)

The capped cases (cap5, zvcap5, dzcap5, cap256) are compared with the iterate of zero_blur_restatement.gmres64 after exactly max_iter vectors.
numpy only (torch through conftest's det_normal)."""
import numpy as np

import psf_restatement as P
import zero_blur_restatement as Z

KR_CHUNK = 4096            # elements of an image per workgroup of the multi-dot / update kernels (csrc/krylov.hip)
KR_MAXM = 256              # the largest max_iter
TOL = ATOL = 1e-6          # the reference's defaults (pnpflow/utils.py:976-977)
RT2 = (0.9, 0.15, 0.5, 0.35, 0.7)      # per image: different conditioning, different Krylov vector counts


def gauss_taps(sigma, K=61):
    """the K fp32 taps of the normalised 1-D Gaussian, as the descriptors carry them"""
    ax = np.arange(-K // 2 + 1.0, K // 2 + 1.0)
    g = np.exp(-(ax ** 2) / (2 * sigma ** 2))
    return (g / g.sum()).astype(np.float32)


def visible_taps(taps):
    """the taps above 2^-36 of the peak, symmetric about the centre (GaussianDeblurring.taps_eff)"""
    K = len(taps)
    keep = np.nonzero(taps >= taps.max() * 2.0 ** -36)[0]
    re = int(max(K // 2 - keep[0], keep[-1] - K // 2))
    return np.ascontiguousarray(taps[K // 2 - re: K // 2 + re + 1])


def motion_psf(size, seed):
    from pnpflow_amd.psf import motion_psf as mp       # numpy only
    return mp(size, seed)


def _case(kind, shape, seed, what, **kw):
    c = dict(kind=kind, shape=shape, seed=seed, what=what, sigma2=0.04, max_iter=100, capped=False, blur=None, visible=True, psf=None, half=0, keep=None,
             counts=True, rt2=RT2[:shape[0]])
    c.update(kw)
    return c


# id -> case.  `what`: (path of the templated kernels, workgroups per image).  `counts`: the GPU test compares the Krylov vector counts with the
# reference's (the tool asserts that the fp32 and fp64 references agree within 1 there).
CASES = {
    "zs": _case(6, (3, 3, 37, 41), 7401, ("scalar", 2), blur=1.0),                      # n % 4 = 3, image bases unaligned, ragged tail
    "zv": _case(6, (2, 1, 64, 65), 7402, ("vector", 2), blur=1.0),                      # 64 elements in the second workgroup
    "z3k43": _case(6, (2, 3, 20, 24), 7403, ("vector", 1), blur=3.0, counts=False),     # blur2d_fused_kernel<64, zero> under the solve
    "z3k61": _case(6, (2, 3, 20, 24), 7403, ("vector", 1), blur=3.0, visible=False, counts=False),    # the row / column passes on the workspace's scratch
    "pc": _case(7, (2, 3, 64, 64), 7404, ("vector", 3), psf=(21, 1)),                   # 3 full workgroups, the engine's tiny4 size
    "pc128": _case(7, (1, 3, 128, 128), 7405, ("vector", 12), psf=(21, 1), counts=False),
    "gc": _case(4, (2, 3, 96, 70), 7406, ("vector", 5), blur=1.0, counts=False),                      # non-square
    "pz": _case(8, (3, 1, 13, 15), 7407, ("scalar", 1), psf=(9, 1)),                    # below one quad row; asymmetric: H_adj must be the adjoint
    "dn": _case(0, (3, 1, 17, 241), 7408, ("scalar", 2)),                               # one element in the second workgroup; exact in 1 vector
    "bx": _case(1, (3, 3, 20, 24), 7409, ("vector", 1), half=5),                        # mask_apply4 under the solve; exact in 2 vectors
    "mk": _case(2, (3, 3, 21, 23), 7410, ("scalar", 1), keep=0.7),                      # mask_apply under the solve
    "cap5": _case(6, (3, 3, 37, 41), 7401, ("scalar", 2), blur=1.0, max_iter=5, capped=True),
    # a converged solve corrects a small consistent error of a reduction by itself (the Arnoldi relation holds for whatever coefficients were used), so
    # the small tails of zv and dn are also held to the iterate at a cap, where nothing is corrected yet
    "zvcap5": _case(6, (2, 1, 64, 65), 7402, ("vector", 2), blur=1.0, max_iter=5, capped=True),
    "dzcap5": _case(6, (3, 1, 17, 241), 7408, ("scalar", 2), blur=1.0, max_iter=5, capped=True),      # dn's shape under the blur: a 1-element tail
    "cap256": _case(6, (2, 3, 37, 41), 7411, ("scalar", 2), blur=1.0, sigma2=0.0004, max_iter=256, capped=True, rt2=(0.9, 0.7)),    # both images run to the cap in fp32 and in fp64
    "mix": _case(6, (5, 3, 20, 24), 7412, ("vector", 1), blur=1.0, rt2=RT2[:4] + (0.0,)),                     # per-image flags: rhs()
}
# mix: image 1 is zero, images 2 and 3 have these norms (below 1e-8: the right-hand side is returned; 1e-5: leaves by atol), image 4 has rt2 = 0 (A = sigma2 I)
MIX_NORMS = {2: 5e-9, 3: 1e-5}


def n_of(case):
    return int(np.prod(case["shape"][1:]))


def nparts_of(case):
    return (n_of(case) + KR_CHUNK - 1) // KR_CHUNK


def path_of(case):
    """'vector' when n % 4 == 0 (and the caller's pointers are 16-byte aligned, as a fresh allocation is), else 'scalar'"""
    return "vector" if n_of(case) % 4 == 0 else "scalar"


def rt2_of(name):
    return np.array(CASES[name]["rt2"], dtype=np.float32)


def taps_of(case):
    """what the descriptor's taps hold: [ntaps] for kinds 4 and 6, [K][K] for kinds 7 and 8, None for the mask family"""
    if case["kind"] in (4, 6):
        t = gauss_taps(case["blur"])
        return visible_taps(t) if case["visible"] else t
    if case["kind"] in (7, 8):
        return motion_psf(*case["psf"])
    return None


def mask_of(case):
    """(B, H, W) uint8 keep-mask of kind 2, a different one per image"""
    B, _, H, W = case["shape"]
    g = np.random.Generator(np.random.Philox(key=[case["seed"], 99]))
    return (g.random((B, H, W)) < case["keep"]).astype(np.uint8)


def weights_of(case):
    """the 0/1 multiplier of the mask family, broadcastable against (B, C, H, W), fp64"""
    B, _, H, W = case["shape"]
    if case["kind"] == 0:
        return np.ones((1, 1, H, W))
    if case["kind"] == 1:
        c, h = H // 2, case["half"]            # the reference's square mask: H // 2 serves both axes
        m = np.ones((H, W)); m[c - h:c + h, c - h:c + h] = 0.0
        return m[None, None]
    return mask_of(case).astype(np.float64)[:, None]


_RHS = {}


def rhs(name):
    """fp32 right-hand sides from the numpy Philox recipe (conftest.det_normal); read-only, made once"""
    if name not in _RHS:
        c = CASES[name]
        g = np.random.Generator(np.random.Philox(key=[c["seed"], 0]))
        r = g.standard_normal(size=c["shape"], dtype=np.float32)
        if name == "mix":
            r[1] = 0.0
            for b, nrm in MIX_NORMS.items():
                r[b] = (r[b].astype(np.float64) * (nrm / np.linalg.norm(r[b].astype(np.float64)))).astype(np.float32)
        r.setflags(write=False)
        _RHS[name] = r
    return _RHS[name]


def returns_rhs(name):
    """per image: the solve returns the right-hand side itself (|rhs_b| < 1e-8, utils.py:995-996)"""
    r = rhs(name).astype(np.float64)
    return np.sqrt((r * r).reshape(r.shape[0], -1).sum(axis=1)) < 1e-8


# ---- A = rt2 H H^T + sigma2 in fp64 -----------------------------------------------------------------------------------------------------------
def _kernel2d(case):
    t = taps_of(case).astype(np.float64)
    return np.outer(t, t) if t.ndim == 1 else t


def hht_fast(case, v):
    """H(H_adj(v)) on (..., C, H, W) fp64 by the form the exact solution is built on (matrix products, FFT, masks)"""
    k = case["kind"]
    if k in (0, 1, 2):
        w = weights_of(case)
        return w * (w * v)             # (the whole batch only: kind 2's multiplier differs per image)
    if k == 6:
        t = taps_of(case)
        return Z.blur64(Z.blur64(v, t, adjoint=True), t)
    if k in (4, 7):
        pw = P.power_spectrum64(_kernel2d(case), *case["shape"][2:])
        return np.real(np.fft.ifft2(np.fft.fft2(v) * pw))
    if k == 8:
        kk = _kernel2d(case)
        return P.apply64(P.apply64(v, kk, zero=True, adjoint=True), kk, zero=True)
    raise ValueError(k)


def hht_direct(case, v):
    """The same product by an independent form: direct sums over the taps (kinds 4, 6, 7), torch's fp64 conv2d (kind 8), the multiplier twice"""
    k = case["kind"]
    if k in (0, 1, 2):
        w = weights_of(case)
        return w * w * v
    kk = _kernel2d(case)
    if k == 8:
        import torch
        import torch.nn.functional as F
        x = torch.from_numpy(np.array(v)).reshape(-1, 1, *v.shape[-2:])
        kt = torch.from_numpy(np.ascontiguousarray(kk))[None, None]
        ha = F.conv2d(x, torch.flip(kt, dims=(2, 3)), padding="same")        # H_adj: the convolution
        return F.conv2d(ha, kt, padding="same").reshape(v.shape).numpy()     # H: the correlation
    zero = k == 6
    return P.apply64(P.apply64(v, kk, zero=zero, adjoint=True), kk, zero=zero)


def apply_A(name, v, direct=False):
    """A v on the whole batch (B, C, H, W), fp64"""
    c = CASES[name]
    v = np.asarray(v, dtype=np.float64)
    r2 = rt2_of(name).astype(np.float64).reshape(-1, 1, 1, 1)
    return r2 * (hht_direct if direct else hht_fast)(c, v) + float(np.float32(c["sigma2"])) * v


def avp_image(name, b):
    """z -> A_b z on a flat image, for gmres64"""
    c = CASES[name]
    shp = c["shape"][1:]
    r2, s2 = float(rt2_of(name)[b]), float(np.float32(c["sigma2"]))
    if c["kind"] in (0, 1, 2):
        w = weights_of(c)
        w = w[b if w.shape[0] > 1 else 0]          # (1, H, W)
        return lambda z: ((r2 * w * w + s2) * z.reshape(shp)).reshape(-1)
    if c["kind"] == 8:
        M = _dense_A(name, b)
        return lambda z: np.einsum("ij,cj->ci", M, z.reshape(shp[0], -1)).reshape(-1)
    return lambda z: (r2 * hht_fast(c, z.reshape(shp)) + s2 * z.reshape(shp)).reshape(-1)


_DENSE = {}


def _dense_H(case):
    """(H W, H W) fp64 matrix of kind 8's H on one channel, from the direct sums of psf_restatement.apply64"""
    key = (case["kind"], case["psf"], case["shape"][2:])
    if key not in _DENSE:
        Hh, Ww = case["shape"][2:]
        assert case["kind"] == 8 and Hh * Ww <= 200
        e = np.eye(Hh * Ww).reshape(Hh * Ww, Hh, Ww)
        _DENSE[key] = P.apply64(e, _kernel2d(case), zero=True).reshape(Hh * Ww, Hh * Ww).T.copy()      # column j = H e_j
    return _DENSE[key]


def _dense_A(name, b):
    c = CASES[name]
    Hm = _dense_H(c)
    return float(rt2_of(name)[b]) * (Hm @ Hm.T) + float(np.float32(c["sigma2"])) * np.eye(Hm.shape[0])


# ---- exact solutions ------------------------------------------------------------------------------------------------------------------------
_EXACT = {}


def exact(name):
    """(B, C, H, W) fp64 solution of A sol = rhs; read-only, made once"""
    if name in _EXACT:
        return _EXACT[name]
    c = CASES[name]
    B, Cc, Hh, Ww = c["shape"]
    R = rhs(name).astype(np.float64)
    r2 = rt2_of(name).astype(np.float64).reshape(-1, 1, 1, 1)
    s2 = float(np.float32(c["sigma2"]))
    k = c["kind"]
    if k in (0, 1, 2):
        sol = R / (r2 * weights_of(c) + s2)
    elif k in (4, 7):
        pw = P.power_spectrum64(_kernel2d(c), Hh, Ww)
        sol = np.real(np.fft.ifft2(np.fft.fft2(R) / (r2 * pw + s2)))
    elif k == 6:
        t = taps_of(c)
        Th, Tw = Z.corr_matrix(t, Hh), Z.corr_matrix(t, Ww)
        lh, Uh = np.linalg.eigh(Th @ Th.T)
        lw, Uw = np.linalg.eigh(Tw @ Tw.T)
        sol = Uh @ ((Uh.T @ R @ Uw) / (r2 * np.outer(lh, lw) + s2)) @ Uw.T
    elif k == 8:
        sol = np.stack([np.linalg.solve(_dense_A(name, b), R[b].reshape(Cc, -1).T).T.reshape(Cc, Hh, Ww) for b in range(B)])
    else:
        raise ValueError(k)
    sol.setflags(write=False)
    _EXACT[name] = sol
    return sol


_G64 = {}


def gmres64(name):
    """Z.gmres64 per image -> (sol (B, C, H, W) fp64, Krylov vectors (B,)); for a capped case its iterate after exactly max_iter vectors"""
    if name not in _G64:
        c = CASES[name]
        sols, its = [], []
        for b in range(c["shape"][0]):
            s, k = Z.gmres64(avp_image(name, b), rhs(name)[b].reshape(-1), c["max_iter"], TOL, ATOL)
            sols.append(s.reshape(c["shape"][1:])); its.append(k)
        sol, its = np.stack(sols), np.array(its)
        sol.setflags(write=False)
        _G64[name] = (sol, its)
    return _G64[name]


def fixture_keys():
    """the arrays of tests/golden/krylov_paths.npz: per case the reference's and gmres64's Krylov vector counts, per image d_ref = max|ref32 - exact|
    (capped cases: max|ref32 - gmres64's iterate at the cap|) and max|exact| (capped: max|iterate|)"""
    return sorted(f"{name}_{what}" for name in CASES for what in ("iters32", "iters64", "dref", "solmax"))
