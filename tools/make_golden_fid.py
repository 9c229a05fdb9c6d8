"""Generate tests/golden/fid_frechet.npz FROM the reference: pnpflow.fid_score.calculate_frechet_distance (fid_score.py:74-128), imported
through tools/ref_import.py (its torchvision stubs are enough: no Inception network is built).   python tools/make_golden_fid.py

Cases: pairs of 64-dimensional feature sets with N = 256 rows each (well-conditioned covariances: N > 4 x dims), drawn from Gaussians with
different means, scales and mixing matrices.  For each case the file holds the fp64 mean and np.cov of the two sets (as
fid_score.py:154-155 forms them; case 0 also the feature sets themselves), the reference's distance, and the same distance by the symmetric eigenvalue route in fp64:
    Tr sqrt(C1 C2) = sum sqrt(eig(C1^1/2 C2 C1^1/2)),  C1^1/2 from eigh
`gap` = |reference - eigenvalue route|: what two fp64 routes to the same number disagree by, the unit of the test's tolerance.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "fid_frechet.npz")
DIMS, N = 64, 256
CASES = (dict(seed=1, shift=0.0, scale=1.0), dict(seed=2, shift=0.3, scale=1.0), dict(seed=3, shift=1.0, scale=2.5), dict(seed=4, shift=0.05, scale=0.2))


def feature_sets(seed, shift, scale):
    g = np.random.Generator(np.random.Philox(key=[77, seed]))
    mix1 = np.eye(DIMS) + 0.2 * g.standard_normal((DIMS, DIMS)) / np.sqrt(DIMS)
    mix2 = np.eye(DIMS) + 0.2 * g.standard_normal((DIMS, DIMS)) / np.sqrt(DIMS)
    a = np.abs(g.standard_normal((N, DIMS))) @ mix1                      # non-negative before mixing, like averaged ReLU features
    b = (scale * np.abs(g.standard_normal((N, DIMS))) + shift) @ mix2
    return a, b


def eig_route(mu1, s1, mu2, s2):
    w, v = np.linalg.eigh(s1)
    r1 = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
    ev = np.linalg.eigvalsh(r1 @ s2 @ r1)
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(np.clip(ev, 0, None)).sum())


def main():
    from tools import ref_import
    ref_import.install_stubs()
    if ref_import.REF not in sys.path:
        sys.path.insert(0, ref_import.REF)
    for m in [k for k in sys.modules if k == "pnpflow" or k.startswith("pnpflow.")]:      # the repo's own shim package must not shadow the reference
        del sys.modules[m]
    import pnpflow.fid_score as ref_fs
    assert os.path.realpath(ref_fs.__file__).startswith(os.path.realpath(ref_import.REF)), ref_fs.__file__
    out = {"n_cases": np.int64(len(CASES))}
    for i, c in enumerate(CASES):
        a, b = feature_sets(**c)
        mu1, s1, mu2, s2 = a.mean(axis=0), np.cov(a, rowvar=False), b.mean(axis=0), np.cov(b, rowvar=False)
        ref = float(ref_fs.calculate_frechet_distance(mu1, s1, mu2, s2))
        eig = eig_route(mu1, s1, mu2, s2)
        if i == 0:          # one case keeps its feature sets too (the mean / np.cov step); all of them would pass the size limit of a committed file
            out.update(a0=a, b0=b)
        out.update({f"mu1_{i}": mu1, f"s1_{i}": s1, f"mu2_{i}": mu2, f"s2_{i}": s2, f"ref{i}": np.float64(ref), f"eig{i}": np.float64(eig),
                    f"gap{i}": np.float64(abs(ref - eig))})
        print(f"case {i}: reference {ref:.12f}  eigenvalue route {eig:.12f}  gap {abs(ref - eig):.3e}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
