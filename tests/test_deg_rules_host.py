"""CPU test of the operator rules (pnpflow_amd/csrc/deg_rules.h): when a pf_degradation may be applied, the side of its measurement, the linear solve
OT-ODE takes for it and the scratch that solve needs.

tests/deg_rules_shim.cpp (extern "C" wrappers around the header) is compiled with ROCm's host clang++ into a temporary directory and loaded with ctypes;
a missing compiler is a failure.  The expected answers are a restatement written here from the rule table of include/pnpflow_hip.h - not generated from the
header - and compared on every point of a grid that crosses each bound of each rule.  The same shim with its own main is built once with
-fsanitize=address,undefined and walks the grid as a stand-alone program.
"""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pnpflow_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "deg_rules_shim.cpp")

KINDS = range(-1, 11)
SFS = (0, 1, 2, 3, 8, 9, 16)
NTAPS = (0, 1, 3, 4, 9, 63, 65, 127, 128)
SHAPES = ((8, 8), (64, 64), (80, 90), (2048, 2048), (2049, 64))
GRID = [(k, sf, nt, taps, mask, H, W) for k, sf, nt, taps, mask, (H, W) in itertools.product(KINDS, SFS, NTAPS, (0, 1), (0, 1), SHAPES)]

CLOSED_FORM, FOURIER_SEPARABLE, KRYLOV, FOURIER_PSF, FOURIER_LOW_RES = range(5)      # enum class DegSolve, in its order


def _host_clang():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for cand in (os.path.join(os.path.dirname(hipcc), "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.isfile(cand):
            return cand
    pytest.fail("no host clang++ next to HIPCC or under /opt/rocm/llvm/bin: the operator-rules test cannot run")


def _compile(out, *extra):
    cmd = [_host_clang(), "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), *extra, "-o", out, SHIM]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, "deg_rules.h must compile as plain host C++17:\n" + res.stderr


@pytest.fixture(scope="module")
def dr(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("deg_rules") / "libdeg_rules_shim.so")
    _compile(so, "-shared")       # (the header's static_asserts - DEG_x == PF_DEG_x, sizeof(DegView) == 32 - are checked by this compile)
    lib = C.CDLL(so)
    lib.dr_rule.restype = C.c_char_p
    lib.dr_sr_scratch.restype = lib.dr_ode_scratch.restype = C.c_size_t
    return lib


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------
def rule_ok(kind, sf, ntaps, taps, mask, H, W):
    if not 0 <= kind <= 9:
        return False
    if kind == 2 and not mask:
        return False
    if kind in (3, 5, 9) and not (sf >= 1 and H % sf == 0 and W % sf == 0):
        return False
    if kind in (4, 5, 6) and not (taps and 1 <= ntaps <= 127):
        return False
    if kind in (7, 8, 9):
        if not (taps and ntaps % 2 == 1 and 1 <= ntaps <= 63):
            return False
        if kind in (7, 9) and ntaps > min(H, W):
            return False
        if kind == 9 and not 1 <= sf <= 8:
            return False
    return True


def out_side(kind, sf, side):
    return side // sf if kind in (3, 5, 9) else side


def solve_of(kind):
    return {4: FOURIER_SEPARABLE, 6: KRYLOV, 8: KRYLOV, 7: FOURIER_PSF, 5: FOURIER_LOW_RES, 9: FOURIER_LOW_RES}.get(kind, CLOSED_FORM)


def fourier_separable_ok(kind, sf, ntaps, taps, mask, H, W):
    return kind == 4 and rule_ok(kind, sf, ntaps, taps, mask, H, W) and ntaps <= min(H, W) and H <= 2048 and W <= 2048


def fourier_psf_ok(kind, sf, ntaps, taps, mask, H, W):
    return kind == 7 and rule_ok(kind, sf, ntaps, taps, mask, H, W) and H <= 2048 and W <= 2048


def fourier_low_res_ok(kind, sf, ntaps, taps, mask, H, W):      # (sr_solve_shape_ok)
    return kind in (5, 9) and rule_ok(kind, sf, ntaps, taps, mask, H, W) and ntaps <= min(H, W) and H <= 2048 and W <= 2048


def solve_ok(*p):
    """The operator rules plus the shape rule of the kind's solve family (none for the closed forms and the Krylov solve)."""
    fam = solve_of(p[0])
    if fam == FOURIER_SEPARABLE:
        return fourier_separable_ok(*p)
    if fam == FOURIER_PSF:
        return fourier_psf_ok(*p)
    if fam == FOURIER_LOW_RES:
        return fourier_low_res_ok(*p)
    return rule_ok(*p)


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------------
def test_rules_match_the_restatement_on_the_grid(dr):
    assert dr.dr_sizeof_view() == 32
    for kind in KINDS:
        assert dr.dr_solve(kind) == solve_of(kind), kind
    seen = {True: 0, False: 0}
    for p in GRID:
        kind, sf, ntaps, taps, mask, H, W = p
        want = rule_ok(*p)
        text = dr.dr_rule(*p)
        assert (text is None) == want, (p, text)
        seen[want] += 1
        for side in (H, W):
            assert dr.dr_out_side(*p, side) == (out_side(kind, sf, side) if want else -1), (p, side)
        assert bool(dr.dr_solve_ok(*p)) == solve_ok(*p), p
        assert bool(dr.dr_sr_solve_shape_ok(*p)) == fourier_low_res_ok(*p), p
        if kind in (7, 8, 9):
            assert bool(dr.dr_psf_taps_ok(kind, sf, ntaps, taps, H, W)) == want, p
    assert min(seen.values()) > 1000, seen           # the grid exercises both answers


def test_the_two_holes_are_closed(dr):
    """PF_DEG_MASK_INPAINTING without a mask and PF_DEG_SR_FILTERED without taps used to reach the device through the direct entry points."""
    assert b"mask" in dr.dr_rule(2, 0, 0, 0, 0, 64, 64) and dr.dr_rule(2, 0, 0, 0, 1, 64, 64) is None
    assert b"taps" in dr.dr_rule(5, 2, 8, 0, 0, 64, 64) and dr.dr_rule(5, 2, 8, 1, 0, 64, 64) is None


def test_texts_name_the_rule(dr):
    assert b"unknown" in dr.dr_rule(10, 1, 1, 1, 1, 64, 64) and b"unknown" in dr.dr_rule(-1, 1, 1, 1, 1, 64, 64)
    assert b"divide" in dr.dr_rule(3, 0, 0, 0, 0, 64, 64) and b"divide" in dr.dr_rule(3, 3, 0, 0, 0, 64, 64) and b"divide" in dr.dr_rule(9, 3, 3, 1, 0, 64, 64)
    assert b"127" in dr.dr_rule(4, 0, 128, 1, 0, 64, 64) and b"taps" in dr.dr_rule(6, 0, 9, 0, 0, 64, 64)
    assert b"odd" in dr.dr_rule(7, 0, 4, 1, 0, 64, 64) and b"odd" in dr.dr_rule(8, 0, 65, 1, 0, 64, 64)


def test_scratch_sizes_are_the_parents(dr):
    for B, Cc, H, sf in itertools.product((1, 2, 32), (1, 3), (8, 64, 256), (1, 2, 4, 8)):
        n, ny, tot = Cc * H * H, Cc * (H // sf) ** 2, B * Cc * H * H
        parent = 3 * tot + 3 * B * ny + 1 + ny // (n // (H * H)) + max(H * H, 4 * H + 2) + B      # ensure_ode's written-out expression before deg_rules.h
        assert dr.dr_sr_scratch(B, Cc, H, H, sf) == parent, (B, Cc, H, sf)
        assert dr.dr_ode_scratch(FOURIER_LOW_RES, B, Cc, H, H, sf) == parent
        assert dr.dr_sr_scratch(B, Cc, H, H, sf) - (H // sf) ** 2 == 3 * tot + 3 * B * ny + 1 + B + max(H * H, 4 * H + 2)      # Prox-PnP's: lam is a buffer of its own
        assert dr.dr_ode_scratch(FOURIER_SEPARABLE, B, Cc, H, H, sf) == 4 * tot + 2 * H
        assert dr.dr_ode_scratch(FOURIER_PSF, B, Cc, H, H, sf) == 4 * tot + H * H
        assert dr.dr_ode_scratch(KRYLOV, B, Cc, H, H, sf) == tot
        assert dr.dr_ode_scratch(CLOSED_FORM, B, Cc, H, H, sf) == 0


def test_grid_walk_is_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "deg_rules_walk")
    _compile(exe, "-DDEG_RULES_MAIN", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stderr == "", res.stderr
    points, ok, s_ok, sr_ok = (int(v) for v in res.stdout.split()[:4])
    assert points == len(GRID)
    assert ok == sum(rule_ok(*p) for p in GRID) and s_ok == sum(solve_ok(*p) for p in GRID) and sr_ok == sum(fourier_low_res_ok(*p) for p in GRID)
