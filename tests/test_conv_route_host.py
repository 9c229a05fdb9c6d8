"""CPU test of the kernel router (pnpflow_amd/csrc/conv_route.h): which kernel, instantiation and launch geometry every conv launch gets.

tests/conv_route_shim.cpp (extern "C" wrappers around the header) is compiled with ROCm's host clang++ into a temporary directory and
loaded with ctypes; a missing compiler is a failure.  No GPU is touched.  Every expected value is a known answer worked out by hand from
the predicates and launcher ladders the router replaced (the derivation stands next to each case); none is produced by calling the router.
Unless a case says otherwise: cu_grid = 256 (the persistent grid of an MI355X), terms = 3, stride 1, the shipped switch values.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pnpflow_amd", "csrc")
LDS_MAX = 160 * 1024
FIELDS = ("family", "terms", "MT", "NT", "WM", "WN", "S", "UP", "BM", "KC", "n9", "n1", "teams", "nsplit", "res", "gnb",
          "grid_x", "grid_y", "xcd_map", "lds_bytes", "csv_code", "refused")


def _host_clang():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for cand in (os.path.join(os.path.dirname(hipcc), "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.isfile(cand):
            return cand
    pytest.fail("no host clang++ next to HIPCC or under /opt/rocm/llvm/bin: the router test cannot run")


@pytest.fixture(scope="module")
def cr(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("conv_route") / "libconv_route_shim.so")
    cmd = [_host_clang(), "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so, os.path.join(ROOT, "tests", "conv_route_shim.cpp")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, "conv_route.h must compile as plain host C++17:\n" + res.stderr
    lib = C.CDLL(so)
    lib.cr_route.restype = None
    return lib


def seg(C_, taps=9, xform=2, w_mode=0, has_w16=True, has_src=True, src=None, src_O=None, src_kk=None, cstride=None):
    """One K-segment; by default a packed segment whose 16-bit image was packed from input channels [0, C) of a tensor with the launch's
    Cout output channels and `taps` taps (src_O is filled in by shape())."""
    lo, hi = src if src is not None else (0, C_)
    return dict(C=C_, cstride=cstride or C_, taps=taps, xform=xform, w_mode=w_mode, has_w16=has_w16 and w_mode == 0, has_src=has_src and has_w16 and w_mode == 0,
                lo=lo, hi=hi, O=src_O, kk=src_kk if src_kk is not None else taps)


def shape(Cout, H, W, B, segs, *, Hs=None, Ws=None, residual=False, addvec=True, gnb=False, coef=None, scale=None, out_cstride=None, res_cstride=None):
    gn_C = sum(s["C"] for s in segs if s["xform"] != 0)
    v = [len(segs), B, H, W, H if Hs is None else Hs, W if Ws is None else Ws, Cout, Cout if out_cstride is None else out_cstride,
         (Cout if res_cstride is None else res_cstride) if residual else 0, gn_C, int(residual), int(addvec),
         int(gn_C > 0 if coef is None else coef), int(gn_C > 0 if scale is None else scale), int(gnb)]
    for i in range(3):
        s = segs[i] if i < len(segs) else None
        v += [0] * 11 if s is None else [s["C"], s["cstride"], s["taps"], s["xform"], s["w_mode"], int(s["has_w16"]), int(s["has_src"]), s["lo"], s["hi"],
                                         Cout if s["O"] is None else s["O"], s["kk"]]
    return v


def env(cu_grid=256, pp=1, sp=1, dma=1, upphase=1):
    return [cu_grid, pp, sp, dma, upphase]


def route(cr, shp, stride=1, up=0, terms=3, e=None):
    out = (C.c_longlong * 22)(*([-0x5A5A5A5A] * 22))
    cr.cr_route((C.c_int * len(shp))(*shp), stride, up, terms, (C.c_int * 5)(*(e or env())), out)
    r = dict(zip(FIELDS, list(out)))
    assert all(v != -0x5A5A5A5A for v in r.values()), r
    fam = {cr.cr_family(i): n for i, n in enumerate(("MFMA32", "MFMA16", "DMA", "PP", "SP"))}
    r["family"] = fam[r["family"]]
    assert not (r["family"] == "DMA" and r["gnb"]), "conv_dma has no GroupNorm-backward form"     # holds for every route this file asks for
    assert r["csv_code"] == {"MFMA32": 0, "MFMA16": 0, "DMA": 1, "PP": 2, "SP": 5}[r["family"]]
    return r


def tile(r):
    return (r["MT"], r["NT"], r["WM"], r["WN"])


def form(r):
    return tile(r) + (r["S"], r["UP"], r["KC"])


def phase_ok(cr, shp, terms=3, e=None):
    return bool(cr.cr_phase_ok((C.c_int * len(shp))(*shp), terms, (C.c_int * 5)(*(e or env()))))


# ---- persistent-grid edges ------------------------------------------------------------------------------------------------------------

def pp_shape(B, n9=1, n1=0, residual=True, H=128, W=128):
    segs = [seg(32 * n9)] + ([seg(32 * n1, taps=1, xform=0)] if n1 else [])
    return shape(32, H, W, B, segs, residual=residual)


def test_conv_pp_needs_32_tiles_per_team(cr):
    # 8 x 16-pixel tiles: 16 x 8 = 128 per 128^2 image; 2 teams per CU x 256 CUs x 32 tiles = 16384 = 128 images
    r = route(cr, pp_shape(128))
    assert (r["family"], r["n9"], r["n1"], r["res"], r["terms"]) == ("PP", 1, 0, 1, 3)
    # one 9-tap chunk image 36864 B + one 8 x 16 halo patch 10 x 18 x 128 = 23040 B: 59904 B fit twice -> two 4-wave workgroups per CU
    assert (r["teams"], r["grid_x"], r["grid_y"], r["lds_bytes"]) == (1, 512, 1, 59904)
    r = route(cr, pp_shape(127))
    assert r["family"] == "MFMA16" and form(r) == (2, 1, 4, 1, 1, 0, 32)      # Cout <= 32: the 16x16 px x 32 tile; 32-channel chunks


def sp_shape(Cout, H, W, B, Cin=None, **kw):
    return shape(Cout, H, W, B, [seg(Cin or Cout)], **kw)


def test_conv_sp_needs_4_tiles_per_workgroup(cr):
    # Cout 128: 16 x 16-pixel tiles, 4 per 32^2 image; 4 x 256 = 1024 tiles = 256 images
    r = route(cr, sp_shape(128, 32, 32, 256))
    assert (r["family"], r["MT"], r["NT"], r["nsplit"], r["res"], r["n9"], r["grid_x"]) == ("SP", 2, 4, 1, 0, 8, 256)
    # slot X 5 taps x 8 KiB = 40960, slot Y 4 x 8 KiB = 32768, two patches 18 x 20 x 64 = 23040, chunk table 1024
    assert r["lds_bytes"] == 40960 + 32768 + 2 * 23040 + 1024
    # 255 images: 1020 tiles.  conv_dma: 9 x 128 x 128 / 128 = 1152 MACs per element < 2000 -> conv_mfma16, 8x16 px x 128 (2040 workgroups)
    r = route(cr, sp_shape(128, 32, 32, 255))
    assert r["family"] == "MFMA16" and form(r) == (4, 1, 1, 4, 1, 0, 32)
    # Cout 64: 32 x 16-pixel tiles, 2 x 4 = 8 per 64^2 image: 128 images
    r = route(cr, sp_shape(64, 64, 64, 128))
    assert (r["family"], r["MT"], r["NT"], r["nsplit"]) == ("SP", 4, 2, 1)
    assert r["lds_bytes"] == 20480 + 16384 + 2 * (34 * 20 * 64) + 1024
    assert route(cr, sp_shape(64, 64, 64, 127))["family"] == "MFMA16"


def test_conv_sp_256_channels_as_two_halves(cr):
    # an item is a (tile, N-half): 2 x 4 per 32^2 image, 1024 items = 128 images
    r = route(cr, sp_shape(256, 32, 32, 128))
    assert (r["family"], r["MT"], r["NT"], r["nsplit"], r["n9"]) == ("SP", 2, 4, 2, 16)
    # the shapes that miss conv_sp land on conv_dma: 9 x 256 x 256 / 256 = 2304 MACs per element, >= 512 workgroups of 8 x 16 px x 128
    assert route(cr, sp_shape(256, 32, 32, 127))["family"] == "DMA"
    assert route(cr, sp_shape(256, 32, 32, 128), e=env(cu_grid=248))["family"] == "DMA"      # 31 workgroups per XCD do not pair up
    assert route(cr, sp_shape(256, 32, 32, 128), terms=1)["family"] == "DMA"                 # the two-half form is built for terms 3 only


# ---- hard limits ----------------------------------------------------------------------------------------------------------------------

def test_packed_pixel_offsets(cr):
    # conv_sp: (TH + 1) W + 17 <= 65535.  Cout 64 (TH 32): 33 x 1024 + 17 = 33809 fits, 33 x 2048 + 17 = 67601 does not
    assert route(cr, sp_shape(64, 32, 1024, 16))["family"] == "SP"          # 64 tiles per image x 16 = 1024
    assert route(cr, sp_shape(64, 32, 2048, 16))["family"] == "MFMA16"
    # Cout 128 (TH 16): 17 x 2048 + 17 = 34833 fits, 17 x 4096 + 17 = 69649 does not
    assert route(cr, sp_shape(128, 16, 2048, 8))["family"] == "SP"          # 128 tiles per image x 8 = 1024
    assert route(cr, sp_shape(128, 16, 4096, 8))["family"] == "MFMA16"
    # conv_pp: W <= 2048
    assert route(cr, pp_shape(128, H=8, W=2048))["family"] == "PP"          # 128 tiles per image x 128 = 16384
    assert route(cr, pp_shape(128, H=8, W=4096))["family"] == "MFMA16"


def test_conv_sp_refusals_go_to_mfma16(cr):
    ok = dict(Cout=128, H=32, W=32, B=256)
    assert route(cr, sp_shape(**ok, addvec=False))["family"] == "MFMA16"      # the hand-counted vmcnt counts the bias loads
    assert route(cr, shape(128, 32, 32, 256, [seg(128, xform=0)]))["family"] == "MFMA16"      # raw segment
    r = route(cr, shape(128, 32, 32, 256, [seg(128), seg(64, taps=1, xform=0)]))              # 1-tap segment: (147456 + 8192) / 192 = 810 MACs per element
    assert r["family"] == "MFMA16" and r["KC"] == 32
    r = route(cr, shape(128, 32, 32, 256, [seg(48)]))                                          # three 16-channel chunks
    assert r["family"] == "MFMA16" and r["KC"] == 16
    # the chunk images are packed from the host slice behind the 16-bit image: no record, other output channels or a 1x1 source -> no conv_sp
    assert route(cr, shape(128, 32, 32, 256, [seg(128, has_src=False)]))["family"] == "MFMA16"
    assert route(cr, shape(128, 32, 32, 256, [seg(128, src_O=256)]))["family"] == "MFMA16"
    assert route(cr, shape(128, 32, 32, 256, [seg(128, src_kk=1)]))["family"] == "MFMA16"


PP_STRUCTURES = [(1, 0, True), (1, 0, False), (2, 0, False), (3, 0, False), (1, 2, False), (1, 3, False)]
# weights + one patch, by hand (terms 3): 36864 n9 + 4096 n1 + 23040 -> 59904, 59904, 96768, 133632, 68096, 72192; twice that <= 163840 for all but (2, 0) and (3, 0)
PP_TEAMS_3 = {(1, 0, True): 1, (1, 0, False): 1, (2, 0, False): 2, (3, 0, False): 2, (1, 2, False): 1, (1, 3, False): 1}


@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("n9,n1,res", PP_STRUCTURES)
def test_conv_pp_structures_and_teams(cr, n9, n1, res, terms):
    r = route(cr, pp_shape(128, n9, n1, res), terms=terms)
    assert (r["family"], r["n9"], r["n1"], r["res"], r["terms"]) == ("PP", n9, n1, int(res), terms)
    one = n9 * cr.cr_pp_w9(terms) + n1 * cr.cr_pp_w1(terms) + cr.cr_pp_patch()      # the byte counts the kernel itself uses
    teams = 1 if 2 * one <= LDS_MAX else 2
    assert teams == (PP_TEAMS_3[n9, n1, res] if terms == 3 else 1)       # hi-only images are half the size: 3 x 18432 + 23040 = 78336 still fits twice
    assert (cr.cr_pp_w9(3), cr.cr_pp_w1(3), cr.cr_pp_w9(1), cr.cr_pp_w1(1), cr.cr_pp_patch()) == (36864, 4096, 18432, 2048, 23040)
    assert r["teams"] == teams and r["grid_x"] == 256 * (2 if teams == 1 else 1)
    assert r["lds_bytes"] == one + (teams - 1) * cr.cr_pp_patch() <= LDS_MAX


@pytest.mark.parametrize("n9,n1,res", [(2, 0, True), (2, 1, False), (1, 1, False), (4, 0, False), (1, 4, False)])
def test_conv_pp_refuses_other_structures(cr, n9, n1, res):
    assert route(cr, pp_shape(128, n9, n1, res))["family"] == "MFMA16"


# ---- conv_dma -------------------------------------------------------------------------------------------------------------------------

def test_conv_dma_thresholds(cr):
    # workgroups of 8 x 16 px x 128 channels.  Upsampling conv 128 -> 128 onto 8 x 16 pixels: one workgroup per image; the operand is at quarter
    # resolution, 9 x 128 x 128 / (128 / 4) = 4608 MACs per element
    up = dict(Cout=128, H=8, W=16, Hs=4, Ws=8, segs=[seg(128, xform=0)])
    r = route(cr, shape(B=512, **up), up=1)
    assert (r["family"], tile(r), r["UP"], r["grid_x"], r["grid_y"], r["xcd_map"]) == ("DMA", (4, 1, 1, 4), 1, 512, 1, 1)
    assert r["lds_bytes"] == 2 * 24 * 1024      # 10 x 18 pixels x 8 pieces = 1440 lanes -> 23 instructions of 64 -> 6 rounds of four 1 KiB instructions per buffer
    r = route(cr, shape(B=511, **up), up=1)
    assert r["family"] == "MFMA16" and (r["S"], r["UP"], r["KC"]) == (1, 1, 32)
    # 256 -> 256 3x3: 2304 taken (16^2 x 128 images: 2 x 1 x 2 = 4 workgroups per image -> 512; conv_sp would want 1024 items, has 256)
    r = route(cr, sp_shape(256, 16, 16, 128))
    assert (r["family"], r["UP"], r["KC"], r["grid_x"], r["grid_y"]) == ("DMA", 0, 32, 512, 1)
    # 128 -> 128 3x3: 1152 is not (1024 workgroups; conv_sp has 512 of 1024 tiles)
    assert route(cr, sp_shape(128, 16, 16, 512))["family"] == "MFMA16"
    # pure 1x1 from 256 channels: taken at Cout 768 >= 3 x 256 (q, k, v stacked), not at Cout 256 (-> 64-channel chunks of conv_mfma16)
    assert route(cr, shape(768, 16, 16, 128, [seg(256, taps=1, xform=1)]))["family"] == "DMA"
    r = route(cr, shape(256, 16, 16, 128, [seg(256, taps=1, xform=1)]))
    assert r["family"] == "MFMA16" and r["KC"] == 64


def test_conv_dma_segment_order_and_switch(cr):
    nine, one = seg(256), seg(256, taps=1, xform=0)
    assert route(cr, shape(256, 16, 16, 128, [one, nine]), e=env(dma=2))["family"] == "MFMA16"      # ring phase: 9-tap chunks run first
    assert route(cr, shape(256, 16, 16, 128, [nine, one]), e=env(dma=2))["family"] == "DMA"
    # dma = 2 ignores the workgroup count and the ratio (one image, one workgroup, 1152); dma = 0 refuses what dma = 1 takes
    assert route(cr, sp_shape(128, 8, 16, 1), e=env(dma=2))["family"] == "DMA"
    assert route(cr, sp_shape(128, 8, 16, 1))["family"] == "MFMA16"
    assert route(cr, sp_shape(256, 16, 16, 128), e=env(dma=0))["family"] == "MFMA16"
    # shape limits hold under dma = 2 as well: whole 128-channel N-blocks, whole 8 x 16 tiles, whole 32-channel chunks
    assert route(cr, sp_shape(192, 8, 16, 1, Cin=128), e=env(dma=2))["family"] == "MFMA16"
    assert route(cr, sp_shape(128, 12, 16, 1), e=env(dma=2))["family"] == "MFMA16"
    assert route(cr, sp_shape(128, 8, 16, 1, Cin=48), e=env(dma=2))["family"] == "MFMA16"


def phase_shape(B=64, Cout=128, Cin=128, Hs=16, Ws=16, H=None, W=None, taps=4, **kw):
    has_w16 = kw.pop("has_w16", True)
    return shape(Cout, 2 * Hs if H is None else H, 2 * Ws if W is None else W, B, [seg(Cin, taps=taps, xform=0, has_w16=has_w16, src_O=4 * Cout)], Hs=Hs, Ws=Ws, **kw)


def test_conv_dma_phase_form(cr):
    # tiles over the SOURCE image, the four phases as 4 Cout output channels: 64 x (16 / 8) x (16 / 16) x (512 / 128) = 512 workgroups
    assert phase_ok(cr, phase_shape())
    r = route(cr, phase_shape(), up=2)
    assert (r["family"], r["UP"], r["grid_x"], r["grid_y"], r["xcd_map"]) == ("DMA", 2, 512, 1, 1)
    refused = [phase_shape(B=63),                    # 504 workgroups
               phase_shape(residual=True), phase_shape(Hs=12), phase_shape(Ws=8), phase_shape(Cout=48), phase_shape(Cin=48),
               phase_shape(H=48), phase_shape(W=48)]       # not twice the source
    for shp in refused:
        assert not phase_ok(cr, shp), shp
        r = route(cr, shp, up=2)
        assert r["family"] == "MFMA16" and (r["S"], r["UP"], r["KC"]) == (1, 2, 16)
    for e in (env(upphase=0), env(dma=0)):
        assert not phase_ok(cr, phase_shape(), e=e) and route(cr, phase_shape(), up=2, e=e)["family"] == "MFMA16"
    assert phase_ok(cr, phase_shape(B=1), e=env(dma=2))      # dma = 2 drops the workgroup count only
    # whole 32-channel chunks at terms 3, whole 64-channel chunks at terms 1
    assert phase_ok(cr, phase_shape(Cin=96)) and not phase_ok(cr, phase_shape(Cin=96), terms=1) and phase_ok(cr, phase_shape(Cin=64), terms=1)
    # the launch test on top of the shape test: the one segment carries the packed 2 x 2 phase image
    assert phase_ok(cr, phase_shape(taps=9)) and route(cr, phase_shape(taps=9), up=2)["family"] != "DMA"
    assert phase_ok(cr, phase_shape(has_w16=False)) and route(cr, phase_shape(has_w16=False), up=2)["family"] != "DMA"


def test_no_gnb_on_conv_dma(cr):
    # the adjoint conv with the fused GroupNorm-backward epilogue: conv_mfma16 only, whatever the switches say
    for e in (env(), env(dma=2)):
        r = route(cr, sp_shape(256, 16, 16, 128, gnb=True), e=e)
        assert (r["family"], r["gnb"]) == ("MFMA16", 1)
    assert not phase_ok(cr, phase_shape(gnb=True))
    assert route(cr, phase_shape(gnb=True), up=2)["refused"] == 1      # the epilogue exists at stride 1 without upsampling only
    assert route(cr, sp_shape(64, 16, 16, 8, gnb=True), terms=0)["refused"] == 1


# ---- the tile ladders of conv_mfma16 and conv_mfma ------------------------------------------------------------------------------------

def raw(Cout, B, stride=1, H=16, W=16, Cin=16, taps=9):
    """A raw 16-channel segment keeps every other kernel away: no GroupNorm (conv_pp / conv_sp), no whole 32-channel chunk (conv_dma)."""
    return shape(Cout, H, W, B, [seg(Cin, taps=taps, xform=0)], Hs=H * stride, Ws=W * stride)


# 16 x 16 pixels per image, so a tile of TH rows x 16 pixels x BN channels gives B x (16 / TH) x ceil(Cout / BN) workgroups; first tile with >= 512
LADDER16 = [  # (Cout, B) -> <MT, NT, WM, WN>
    (32, 1, (2, 1, 4, 1)), (32, 4096, (2, 1, 4, 1)),                                                     # 16x16 px x 32, always
    (64, 512, (4, 1, 2, 2)), (64, 511, (2, 1, 2, 2)), (64, 256, (2, 1, 2, 2)), (64, 255, (1, 1, 2, 2)),  # 16x16 x 64: B; 8x16 x 64: 2 B; else 4x16 x 64
    (128, 256, (4, 1, 1, 4)), (128, 255, (2, 1, 1, 4)), (128, 128, (2, 1, 1, 4)), (128, 127, (1, 1, 2, 2)),      # 8x16 x 128: 2 B; 4x16 x 128: 4 B; else 4x16 x 64
    (256, 128, (4, 1, 1, 4)), (256, 127, (2, 1, 1, 4)), (256, 64, (2, 1, 1, 4)), (256, 63, (1, 1, 2, 2)),        # two N-blocks: 4 B; 8 B
]
LADDER16_S2 = {32: (1, 1, 4, 1), 64: (2, 1, 2, 2), 128: (1, 1, 2, 2), 256: (1, 1, 2, 2)}
LADDER32 = [
    (32, 1, (2, 1, 4, 1)), (32, 4096, (2, 1, 4, 1)),
    (64, 512, (2, 2, 4, 1)), (64, 511, (1, 2, 4, 1)), (64, 256, (1, 2, 4, 1)), (64, 255, (1, 1, 2, 2)),          # 16x16 x 64: B; 8x16 x 64: 2 B; else 4x16 x 64
    (128, 256, (2, 2, 2, 2)), (128, 255, (1, 2, 2, 2)), (128, 128, (1, 2, 2, 2)), (128, 127, (1, 1, 2, 2)),      # 8x16 x 128: 2 B; 4x16 x 128: 4 B; 8x16 x 64: 4 B as well
    (256, 128, (2, 2, 2, 2)), (256, 127, (1, 2, 2, 2)), (256, 64, (1, 2, 2, 2)), (256, 63, (1, 1, 2, 2)),        # 4 B; 8 B; 8x16 x 64: 8 B as well
]
LADDER32_S2 = {32: (1, 1, 4, 1), 64: (1, 2, 4, 1), 128: (1, 1, 2, 2), 256: (1, 1, 2, 2)}


@pytest.mark.parametrize("Cout,B,want", LADDER16)
def test_mfma16_ladder_stride1(cr, Cout, B, want):
    r = route(cr, raw(Cout, B))
    assert r["family"] == "MFMA16" and form(r) == want + (1, 0, 16), r


@pytest.mark.parametrize("Cout,B,want", LADDER32)
def test_mfma32_ladder_stride1(cr, Cout, B, want):
    r = route(cr, raw(Cout, B), terms=0)
    assert r["family"] == "MFMA32" and form(r) == want + (1, 0, 16) and (r["BM"], r["xcd_map"]) == (0, 0), r


@pytest.mark.parametrize("B", [1, 511, 512, 4096])
@pytest.mark.parametrize("Cout", [32, 64, 128, 256])
def test_stride2_tiles_do_not_depend_on_the_grid(cr, Cout, B):
    r = route(cr, raw(Cout, B, stride=2), stride=2)
    assert r["family"] == "MFMA16" and form(r) == LADDER16_S2[Cout] + (2, 0, 16)
    r = route(cr, raw(Cout, B, stride=2), stride=2, terms=0)
    assert r["family"] == "MFMA32" and form(r) == LADDER32_S2[Cout] + (2, 0, 16)


def test_mfma32_8x16x64_tile_above_64_channels(cr):
    # four rows: 4x16 px x 128 gives B workgroups, 8x16 px x 64 two N-blocks -> 2 B: the only way onto <1, 2, 4, 1> at Cout > 64
    assert tile(route(cr, raw(128, 256, H=4), terms=0)) == (1, 2, 4, 1)
    assert tile(route(cr, raw(128, 255, H=4), terms=0)) == (1, 1, 2, 2)
    assert tile(route(cr, raw(128, 512, H=4), terms=0)) == (2, 2, 2, 2)      # (8 rows or 4: one tile row either way, so 8x16 px x 128 has its 512 first)


def test_pure_1x1_launches_want_1024_workgroups(cr):
    one = lambda Cout, B: raw(Cout, B, Cin=64, taps=1)      # 64-channel chunks (KC = 64); Cout < 3 x 64 keeps conv_dma away
    for B, want in ((1024, (4, 1, 2, 2)), (1023, (2, 1, 2, 2)), (512, (2, 1, 2, 2)), (511, (1, 1, 2, 2))):
        r = route(cr, one(64, B))
        assert r["family"] == "MFMA16" and form(r) == want + (1, 0, 64), (B, r)
    for B, want in ((512, (4, 1, 1, 4)), (511, (2, 1, 1, 4)), (256, (2, 1, 1, 4)), (255, (1, 1, 2, 2))):
        r = route(cr, one(128, B))
        assert r["family"] == "MFMA16" and form(r) == want + (1, 0, 64), (B, r)
    # conv_mfma keeps 512 for its 64-channel chunks
    assert form(route(cr, one(64, 512), terms=0)) == (2, 2, 4, 1, 1, 0, 64)
    assert form(route(cr, one(64, 511), terms=0)) == (1, 2, 4, 1, 1, 0, 64)


def test_grid_and_lds_of_the_mfma_kernels(cr):
    # conv_mfma16 <4,1,2,2> KC 16 terms 3: patch 18 rows of ceil(18 x 20 / 64) x 64 = 384 floats = 6912 > epilogue 4608 + 2 x 64 x 2 = 4864 floats
    r = route(cr, raw(64, 512))
    assert (r["grid_x"], r["grid_y"], r["xcd_map"], r["lds_bytes"]) == (512, 1, 1, 6912 * 4)
    # 255 images on the 4x16 px tile: 1020 workgroups, not a multiple of the 8 XCDs -> the plain 2-D grid
    r = route(cr, raw(64, 255))
    assert (r["grid_x"], r["grid_y"], r["xcd_map"]) == (1020, 1, 0)
    # two N-blocks fold into the flat grid when the product is a multiple of 8
    r = route(cr, raw(256, 128))
    assert (r["grid_x"], r["grid_y"], r["xcd_map"]) == (512, 1, 1)
    # conv_mfma <2,2,4,1> KC 16: patch 18 x 18 pixels x 20 floats = 6480 > epilogue 4608 + 4 x 64 x 2 = 5120; N-blocks in grid.y
    r = route(cr, raw(64, 512), terms=0)
    assert (r["grid_x"], r["grid_y"], r["lds_bytes"]) == (512, 1, 6480 * 4)
    r = route(cr, raw(256, 128), terms=0)
    assert (r["grid_x"], r["grid_y"]) == (256, 2)
    # GroupNorm coefficients park behind the patch: 2 x gn_C floats
    r = route(cr, shape(64, 16, 16, 512, [seg(48, xform=1)]))
    assert r["family"] == "MFMA16" and r["lds_bytes"] == (6912 + 2 * 48) * 4


def test_chunk_width(cr):
    kc = lambda segs, **kw: route(cr, shape(64, 16, 16, 8, segs, **{k: v for k, v in kw.items() if k in ("Hs", "Ws")}), **{k: v for k, v in kw.items() if k in ("stride", "up")})
    assert form(kc([seg(64, taps=1, xform=0)]))[4:] == (1, 0, 64)
    assert form(kc([seg(64, taps=1, xform=0), seg(128, taps=1, xform=0)]))[4:] == (1, 0, 64)
    assert form(kc([seg(64, taps=1, xform=0)], stride=2, Hs=32, Ws=32))[4:] == (2, 0, 16)
    assert form(kc([seg(64, taps=1, xform=0)], up=1, Hs=8, Ws=8))[4:] == (1, 1, 32)
    assert form(kc([seg(96, taps=1, xform=0)]))[4:] == (1, 0, 32)
    assert form(kc([seg(32, xform=0)]))[4:] == (1, 0, 32)
    assert form(kc([seg(64, xform=0), seg(64, taps=1, xform=0)]))[4:] == (1, 0, 32)
    assert form(kc([seg(32, xform=0), seg(16, taps=1, xform=0)]))[4:] == (1, 0, 16)
    assert form(kc([seg(32, xform=0)], up=1, Hs=8, Ws=8))[4:] == (1, 1, 32)
    assert form(kc([seg(16, xform=0)], up=1, Hs=8, Ws=8))[4:] == (1, 1, 16)
    assert form(kc([seg(32, taps=4, xform=0)], up=2, Hs=8, Ws=8))[4:] == (1, 2, 16)


def test_generic_operands(cr):
    gen = lambda C_: seg(C_, taps=1, xform=0, w_mode=1)
    for terms in (0, 1, 3):
        r = route(cr, shape(64, 16, 16, 8, [gen(64)]), terms=terms)
        assert (r["family"], r["BM"], r["KC"], r["refused"]) == ("MFMA32", 1, 64, 0)
        r = route(cr, shape(64, 16, 16, 8, [gen(48)]), terms=terms)       # the generic operand clamps its k index: 64-channel chunks from 64 channels on
        assert (r["family"], r["BM"], r["KC"]) == ("MFMA32", 1, 16)
        assert route(cr, shape(64, 16, 16, 8, [gen(64), seg(64, taps=1, xform=0)]), terms=terms)["refused"] == 1
        assert route(cr, shape(64, 8, 8, 8, [gen(64)], Hs=16, Ws=16), stride=2, terms=terms)["refused"] == 1
    # a packed segment without a 16-bit image keeps the whole launch on the fp32 kernel
    r = route(cr, shape(64, 16, 16, 8, [seg(32, xform=0), seg(32, xform=0, has_w16=False)]))
    assert (r["family"], r["BM"], r["refused"]) == ("MFMA32", 0, 0)
    # conv_mfma16 parks at most 1024 GroupNorm channels and needs their coefficients
    assert route(cr, shape(64, 16, 16, 8, [seg(32)], coef=False))["refused"] == 1


# ---- precision modes and switches -----------------------------------------------------------------------------------------------------

def test_exact_mode_is_always_conv_mfma(cr):
    for shp, kw in ((pp_shape(128), {}), (sp_shape(128, 32, 32, 256), {}), (sp_shape(256, 32, 32, 128), {}), (sp_shape(256, 16, 16, 128), {}),
                    (phase_shape(), dict(up=2))):
        r = route(cr, shp, terms=0, **kw)
        assert (r["family"], r["terms"], r["refused"]) == ("MFMA32", 0, 0)
    assert not phase_ok(cr, phase_shape(), terms=0)


def test_single_term_mode(cr):
    r = route(cr, pp_shape(128), terms=1)
    assert (r["family"], r["terms"], r["teams"], r["lds_bytes"]) == ("PP", 1, 1, 18432 + 23040)
    r = route(cr, sp_shape(128, 32, 32, 256), terms=1)
    assert (r["family"], r["terms"], r["MT"], r["NT"], r["lds_bytes"]) == ("SP", 1, 2, 4, 20480 + 16384 + 2 * 23040 + 1024)
    assert r["lds_bytes"] == cr.cr_sp_lds(2, 4, 1)
    assert route(cr, sp_shape(64, 64, 64, 128), terms=1)["family"] == "SP"
    # switch value 3: the persistent kernels in the default mode only
    r = route(cr, pp_shape(128), terms=1, e=env(pp=3))
    assert (r["family"], r["terms"]) == ("MFMA16", 1)
    assert route(cr, pp_shape(128), terms=3, e=env(pp=3))["family"] == "PP"
    assert route(cr, sp_shape(128, 32, 32, 256), terms=1, e=env(sp=3))["family"] == "MFMA16"
    assert route(cr, sp_shape(128, 32, 32, 256), terms=3, e=env(sp=3))["family"] == "SP"
    # conv_dma's hi-only images are packed in whole 64-channel chunks from a recorded host slice
    r = route(cr, sp_shape(256, 16, 16, 128), terms=1)
    assert (r["family"], r["terms"], r["KC"]) == ("DMA", 1, 64)
    assert route(cr, shape(256, 16, 16, 128, [seg(256, src=(0, 224))]), terms=1)["family"] == "MFMA16"
    assert route(cr, shape(256, 16, 16, 128, [seg(256, has_src=False)]), terms=1)["family"] == "MFMA16"
    assert route(cr, shape(256, 16, 16, 128, [seg(256, has_src=False)]), terms=3)["family"] == "DMA"      # the split images are the segments' own


def test_conv_sp_switch(cr):
    s64, s128, s256 = sp_shape(64, 64, 64, 128), sp_shape(128, 32, 32, 256), sp_shape(256, 32, 32, 128)
    assert [route(cr, s, e=env(sp=2))["family"] for s in (s64, s128, s256)] == ["MFMA16", "SP", "DMA"]      # the 128-channel level only
    assert [route(cr, s, e=env(sp=4))["family"] for s in (s64, s128, s256)] == ["SP", "SP", "DMA"]          # the 256-channel level stays on conv_dma
    assert [route(cr, s, e=env(sp=0))["family"] for s in (s64, s128, s256)] == ["MFMA16", "MFMA16", "DMA"]
    assert route(cr, pp_shape(128), e=env(pp=0))["family"] == "MFMA16"


# ---- self-consistency over a seeded sweep ---------------------------------------------------------------------------------------------

def instantiated(r):
    """The template instantiations the five kernel files build (their launchers' switches): a route outside them would be hipErrorInvalidValue at launch."""
    f = r["family"]
    if f == "MFMA16":
        tiles = {(2, 1, 4, 1), (4, 1, 2, 2), (2, 1, 2, 2), (1, 1, 2, 2), (4, 1, 1, 4), (2, 1, 1, 4)} if r["S"] == 1 else {(1, 1, 4, 1), (2, 1, 2, 2), (1, 1, 2, 2)}
        forms = {(1, 0, 64), (2, 0, 16), (1, 2, 16), (1, 1, 32), (1, 1, 16), (1, 0, 32), (1, 0, 16)}
        return tile(r) in tiles and (r["S"], r["UP"], r["KC"]) in forms and r["terms"] in (1, 3) and (not r["gnb"] or (r["S"], r["UP"]) == (1, 0))
    if f == "MFMA32":
        tiles = {(2, 1, 4, 1), (2, 2, 4, 1), (2, 2, 2, 2), (1, 2, 2, 2), (1, 2, 4, 1), (1, 1, 2, 2), (1, 1, 4, 1)}
        forms = {(1, 0, 1, 64), (1, 0, 0, 64), (1, 0, 1, 16), (2, 0, 0, 16), (1, 2, 0, 16), (1, 1, 0, 16), (1, 0, 0, 16)}
        return tile(r) in tiles and (r["S"], r["UP"], r["BM"], r["KC"]) in forms and not r["gnb"]
    if f == "DMA":
        return tile(r) == (4, 1, 1, 4) and r["UP"] in (0, 1, 2) and r["terms"] in (1, 3) and not r["gnb"]
    if f == "PP":
        return (r["n9"], r["n1"], bool(r["res"])) in PP_STRUCTURES and r["terms"] in (1, 3) and r["MT"] == 1
    return (r["MT"], r["NT"], r["nsplit"], r["terms"]) in {(2, 4, 2, 3), (2, 4, 1, 3), (2, 4, 1, 1), (4, 2, 1, 3), (4, 2, 1, 1)} and 2 <= r["n9"] <= 32 and r["n9"] % 2 == 0

def test_sweep_is_total_and_covers_the_output(cr):
    g = np.random.default_rng(20240611)
    couts, sides, batches, cins = [3, 32, 64, 96, 128, 256, 768], [8, 16, 32, 64, 128, 256], [1, 2, 3, 8, 31, 32, 127, 128, 160, 255, 256, 512], [16, 32, 48, 64, 128, 256]
    seen = set()
    for _ in range(4000):
        Cout, H, B, Cin = (int(g.choice(v)) for v in (couts, sides, batches, cins))
        stride, up, terms = int(g.choice([1, 1, 2])), int(g.choice([0, 0, 1, 2])), int(g.choice([0, 1, 3]))
        if stride == 2:
            up = 0
        mix = int(g.integers(0, 7))
        segs = [[seg(Cin)], [seg(Cin), seg(Cin)], [seg(Cin), seg(Cin, taps=1, xform=0)], [seg(Cin, xform=0)], [seg(Cin, taps=1, xform=0)],
                [seg(Cin, taps=1, xform=0, w_mode=1)], [seg(Cin, taps=4, xform=0, src_O=4 * Cout)]][mix]
        Hs = H * 2 if stride == 2 else max(H // 2, 1) if up else H
        shp = shape(Cout, H, H, B, segs, Hs=Hs, Ws=Hs, residual=bool(g.integers(0, 2)), addvec=bool(g.integers(0, 4)), gnb=bool(g.integers(0, 8) == 0))
        e = env(cu_grid=int(g.choice([256, 256, 248, 64, 0])), pp=int(g.integers(0, 5)), sp=int(g.integers(0, 5)), dma=int(g.integers(0, 3)), upphase=int(g.integers(0, 2)))
        r = route(cr, shp, stride=stride, up=up, terms=terms, e=e)      # (route() checks: every field written, csv_code matches the family, no conv_dma with gnb)
        seen.add(r["family"])
        if r["refused"]:
            continue
        assert 0 < r["lds_bytes"] <= LDS_MAX and r["grid_x"] > 0 and r["grid_y"] > 0 and r["xcd_map"] in (0, 1), r
        assert r["terms"] == (0 if r["family"] == "MFMA32" and terms == 0 else terms) and r["gnb"] in (0, 1)
        assert instantiated(r), r
        if r["family"] in ("MFMA32", "MFMA16", "DMA"):
            TH, BN = 2 * r["MT"] * r["WM"], 32 * r["NT"] * r["WN"]
            need = B * -(-Hs // TH) * -(-Hs // 16) * -(-4 * Cout // BN) if r["UP"] == 2 and r["family"] == "DMA" else B * -(-H // TH) * -(-H // 16) * -(-Cout // BN)
            assert r["grid_x"] * r["grid_y"] >= need and (r["S"], r["UP"]) == (stride, up) and r["KC"] in (16, 32, 64), (r, need)
            assert r["xcd_map"] == 0 or (r["grid_y"] == 1 and r["grid_x"] % 8 == 0)
        else:
            assert r["grid_x"] == e[0] * (2 if r["teams"] == 1 else 1) and e[0] >= 8 and (stride, up) == (1, 0)
            assert r["nsplit"] in ((1, 2) if r["family"] == "SP" else (0,)) and r["teams"] in ((1, 2) if r["family"] == "PP" else (0,))
    assert seen == {"MFMA32", "MFMA16", "DMA", "PP", "SP"}
