"""tests/krylov_reference.py on the CPU: the exact solutions solve their systems under an independent form of the operator, gmres64 converges to
them, the case table's n / workgroup / path columns are what csrc/krylov.hip's rules give, and tests/golden/krylov_paths.npz holds the table's keys
and what tests/test_gpu_krylov_paths.py relies on."""
import os
import re

import numpy as np
import pytest

import krylov_reference as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONVERGED = [name for name, c in K.CASES.items() if not c["capped"]]


def norms(a):
    return np.sqrt((np.asarray(a, dtype=np.float64) ** 2).reshape(a.shape[0], -1).sum(axis=1))


@pytest.mark.parametrize("name", list(K.CASES))
def test_exact_solution_solves_the_system(name):
    """|A sol - rhs| <= 1e-10 |rhs| per image, A applied by direct sums over the taps / torch's fp64 conv2d / the multiplier - none of which the
    exact solution is built on (matrix eigendecompositions, FFT, division, a dense solve)"""
    sol, rhs = K.exact(name), K.rhs(name).astype(np.float64)
    res = norms(K.apply_A(name, sol, direct=True) - rhs)
    assert np.isfinite(sol).all()
    assert (res <= 1e-10 * norms(rhs)).all(), (res, norms(rhs))
    # and the two operator forms agree on a vector that is not a solution
    v = rhs[:, ::-1].copy()
    a, b = K.apply_A(name, v), K.apply_A(name, v, direct=True)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("name", CONVERGED)
def test_gmres64_converges_to_the_exact_solution(name):
    """GMRES leaves with |rhs - A x| < max(tol |rhs|, atol); sigma2 is a lower bound of A's spectrum, so |x - exact| <= that / sigma2"""
    c = K.CASES[name]
    sol, its = K.gmres64(name)
    ret = K.returns_rhs(name)
    bn = norms(K.rhs(name))
    err = norms(sol - K.exact(name))
    bound = np.maximum(K.TOL * bn, K.ATOL) / float(np.float32(c["sigma2"]))
    assert (its < c["max_iter"]).all()
    assert np.array_equal(its == 0, ret)
    assert (err[~ret] <= bound[~ret]).all(), (err, bound)
    for b in np.nonzero(ret)[0]:
        assert np.array_equal(sol[b], K.rhs(name)[b].astype(np.float64))


def test_table_matches_the_kernels_rules():
    src = open(os.path.join(ROOT, "pnpflow_amd", "csrc", "krylov.hip")).read()
    ept = int(re.search(r"constexpr int KR_EPT = (\d+);", src).group(1))
    assert re.search(r"constexpr int KR_CHUNK = 256 \* KR_EPT;", src) and 256 * ept == K.KR_CHUNK
    assert int(re.search(r"constexpr int KR_MAXM = (\d+);", src).group(1)) == K.KR_MAXM
    assert "const bool vec = (n % 4 == 0)" in src
    expect = {"zs": 4551, "zv": 4160, "z3k43": 1440, "z3k61": 1440, "pc": 12288, "pc128": 49152, "gc": 20160, "pz": 195, "dn": 4097, "bx": 1440, "mk": 1449,
              "cap5": 4551, "zvcap5": 4160, "dzcap5": 4097, "cap256": 4551, "mix": 1440}
    assert set(expect) == set(K.CASES)
    for name, c in K.CASES.items():
        assert K.n_of(c) == expect[name], name
        assert c["what"] == (K.path_of(c), K.nparts_of(c)), name
        assert 0 <= c["max_iter"] <= K.KR_MAXM
        assert len(c["rt2"]) == c["shape"][0] and len(set(c["rt2"])) == c["shape"][0], name      # rt2 differs per image
    assert K.n_of(K.CASES["zv"]) - K.KR_CHUNK == 64 and K.n_of(K.CASES["dn"]) - K.KR_CHUNK == 1       # the ragged tails the table names
    assert K.n_of(K.CASES["pc"]) == 3 * K.KR_CHUNK
    assert K.CASES["cap256"]["max_iter"] == K.KR_MAXM
    # the sigma-3 pair takes both blur paths: 43 visible taps (radius 21 <= 24: fused) and the 61 raw ones (radius 30: row and column passes)
    assert len(K.taps_of(K.CASES["z3k43"])) == 43 and len(K.taps_of(K.CASES["z3k61"])) == 61 and len(K.taps_of(K.CASES["zs"])) == 15
    # kind 8's kernel is not point-symmetric: the correlation is not its own adjoint
    k = K.taps_of(K.CASES["pz"])
    assert k.shape == (9, 9) and not np.array_equal(k, k[::-1, ::-1])
    # mix: one zero image, one below the 1e-8 rule, one of norm 1e-5
    n = norms(K.rhs("mix"))
    assert n[1] == 0 and n[2] < 1e-8 and abs(n[3] - 1e-5) < 1e-9 and K.rt2_of("mix")[4] == 0
    assert K.returns_rhs("mix").tolist() == [False, True, True, False, False]


def test_fixture_matches_the_table(golden):
    g = golden("krylov_paths")
    assert sorted(g.files) == K.fixture_keys()
    for name, c in K.CASES.items():
        B = c["shape"][0]
        i32, i64, dref, solmax = (g[f"{name}_{k}"] for k in ("iters32", "iters64", "dref", "solmax"))
        assert i32.shape == i64.shape == dref.shape == solmax.shape == (B,)
        assert np.isfinite(dref).all() and (dref >= 0).all()
        assert np.array_equal(i32 == 0, K.returns_rhs(name))
        if c["capped"]:
            assert (i32 == c["max_iter"]).all() and (i64 == c["max_iter"]).all()
        else:
            assert i32.max() < c["max_iter"]
            if c["counts"]:
                assert np.abs(i32 - i64).max() <= 1
    # the cases with a known Krylov dimension: one eigenvalue (identity; rt2 = 0), two (the masks)
    assert g["dn_iters32"].tolist() == [1, 1, 1] and g["bx_iters32"].tolist() == [2, 2, 2] and g["mk_iters32"].tolist() == [2, 2, 2]
    assert g["mix_iters32"][4] == 1
    # mix's image 3 leaves by atol several vectors before tol alone would stop it
    import zero_blur_restatement as Z
    _, k_tol = Z.gmres64(K.avp_image("mix", 3), K.rhs("mix")[3].reshape(-1), 100, K.TOL, 0.0)
    assert 0 < g["mix_iters32"][3] <= k_tol - 4, (g["mix_iters32"][3], k_tol)
