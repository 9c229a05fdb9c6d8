"""Host-side pins of tests/attention_reference.py, the reference side of tests/test_gpu_attention_paths.py: the packed fp16 pair is bit exact, every
input recipe has the property it is named for, the restated kernel arithmetic stays inside the derived bound on every case of the table (so a GPU
failure is the kernel's, not the case's), and the refusal list agrees with the sources.  No GPU."""
import os
import re

import numpy as np
import pytest

import attention_reference as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- pack / unpack ------------------------------------------------------------------------------------------------------------------------------
def rne16_bits(x):
    """fp32 -> fp16 bit pattern by integer arithmetic (round to nearest even, subnormals kept, overflow to infinity): independent of numpy's cast"""
    u = int(np.float32(x).view(np.uint32))
    sign, e, m = (u >> 16) & 0x8000, (u >> 23) & 0xFF, u & 0x7FFFFF
    if e == 0xFF:
        return sign | 0x7C00 | (0x200 if m else 0)
    if e == 0:
        return sign                                        # fp32 subnormals are below half of fp16's smallest subnormal
    m |= 0x800000
    shift = 13 if e - 127 >= -14 else 13 + (-14 - (e - 127))
    if shift > 25:
        return sign
    q, r = m >> shift, m & ((1 << shift) - 1)
    half = 1 << (shift - 1)
    if r > half or (r == half and (q & 1)):
        q += 1
    if e - 127 >= -14:
        h = ((e - 127 + 15 - 1) << 10) + q                 # q carries the implicit bit: a mantissa overflow carries into the exponent
    else:
        h = q
    return sign | min(h, 0x7C00)


def test_pack_hilo_is_the_bit_exact_split_and_unpack_inverts_it():
    g = np.random.Generator(np.random.Philox(key=[7530, 0]))
    x = g.standard_normal(4000, dtype=np.float32) * np.float32(10.0) ** g.integers(-9, 5, 4000).astype(np.float32)
    special = np.array([0.0, -0.0, 65504.0, -65504.0, 65519.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -24,
                        1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -12, 0.1, 1e-4, 1e-6, 6.0e4, 2049.0, 1.0 + 2.0 ** -11 + 2.0 ** -23], dtype=np.float32)
    x = np.concatenate([x, special])
    w = A.pack_hilo(x)
    assert w.dtype == np.int32 and w.shape == x.shape
    for xi, wi in zip(x, w.view(np.uint32)):
        hb = rne16_bits(xi)
        hi = np.array([hb], dtype=np.uint16).view(np.float16)[0]
        lb = rne16_bits(np.float32(xi) - np.float32(hi))
        assert int(wi) == hb | (lb << 16), (float(xi), hex(int(wi)), hex(hb | (lb << 16)))
    hi, lo = A.unpack_hilo(w)
    assert hi.dtype == lo.dtype == np.float16
    assert np.array_equal(hi.view(np.uint16).astype(np.uint32) | (lo.view(np.uint16).astype(np.uint32) << 16), w.view(np.uint32))
    # named patterns: -0 keeps its sign in hi and has lo = +0; the largest finite fp16; a lo in fp16's subnormal range; the smallest subnormal alone
    u = lambda v: int(A.pack_hilo(np.array([v], dtype=np.float32)).view(np.uint32)[0])
    assert u(0.0) == 0x00000000 and u(-0.0) == 0x00008000
    assert u(65504.0) == 0x00007BFF and u(-65504.0) == 0x0000FBFF
    assert u(2.0 ** -24) == 0x00000001 and u(2.0 ** -25) == 0x00000000 and u(3 * 2.0 ** -25) == 0x80000002     # the last: hi ties up to 2^-23, lo = -2^-25 ties to -0
    assert u(1.0 + 2.0 ** -11) == 0x3C00 | (0x1000 << 16)                    # hi ties to even (1.0), lo = 2^-11
    assert u(0.1) == 0x2E66 | (0x019A << 16)                                 # 0.1f - 0x2E66 = 409.6 * 2^-24: a subnormal lo, 410, and 0.4 * 2^-24 is lost
    # |x| <= 0.25: every lo is subnormal (|lo| <= 2^-14) and hi + lo is x to 2^-25 absolute
    small = g.uniform(-0.25, 0.25, 2000).astype(np.float32)
    hs, ls = A.unpack_hilo(A.pack_hilo(small))
    assert np.all(np.abs(ls.astype(np.float64)) <= 2.0 ** -14)
    assert np.all(np.abs(hs.astype(np.float64) + ls.astype(np.float64) - small) <= 2.0 ** -25)
    # above 0.25 the pair carries 22 bits
    big = g.uniform(1.0, 6.0e4, 2000).astype(np.float32)
    hb_, lb_ = A.unpack_hilo(A.pack_hilo(big))
    assert np.all(np.abs(hb_.astype(np.float64) + lb_.astype(np.float64) - big) <= 2.0 ** -22 * big)


def test_packed_qkv_leaves_q_and_packs_k_and_v():
    qkv = A.inputs(128, 128, 2, "peaked")
    w = A.packed_qkv(qkv)
    assert w.dtype == np.int32 and w.shape == qkv.shape
    assert np.array_equal(w[..., :128], qkv[..., :128].view(np.int32))
    assert np.array_equal(w[..., 128:], A.pack_hilo(qkv[..., 128:]))
    over = np.array([7.0e4, -7.0e4], dtype=np.float32)          # above fp16: hi = +-inf, lo = -+inf - the kernel's product is then NaN, never finite
    assert [hex(v) for v in A.pack_hilo(over).view(np.uint32)] == ["0xfc007c00", "0x7c00fc00"]


# ---- the table ----------------------------------------------------------------------------------------------------------------------------------
def test_the_table_names_all_twelve_instantiations_with_both_epilogues():
    want = {f"attn_fused_kernel<{tk},{tc},{kv}>" for tk in (1, 2) for tc in (1, 2) for kv in ("true", "false")}
    want |= {f"attn_fused_long_kernel<{tc},{kv}>" for tc in (1, 2) for kv in ("true", "false")}
    assert len(want) == 12
    for epi in ("plain", "folded"):
        for recipe in ("peaked", "flat"):
            got = {A.instantiation(c["T"], c["C"], c["packed"]) for n, c in A.CASES.items()
                   if n.startswith("variant-") and c["epilogue"] == epi and c["recipe"] == recipe and c["B"] == 9}
            assert got == want
    src = open(os.path.join(ROOT, "pnpflow_amd", "csrc", "attention.hip")).read()
    launched = set(re.findall(r"launch_attn_cfg<(\d), (\d), (true|false)>", src)) | {("L",) + m for m in re.findall(r"launch_attn_long_cfg<(\d), (true|false)>", src)}
    assert len(launched) == 12                                  # what launch_attn_fused can pick
    longs = [c for n, c in A.CASES.items() if n.startswith("long-")]
    assert {c["T"] for c in longs} == {512, 768, 2048, 4096} and {c["recipe"] for c in longs} == {"rising", "falling", "last", "wide"}
    assert {(c["C"], c["B"]) for c in longs} == {(128, 2), (256, 1)}
    assert any(c["T"] == 4096 and c["C"] == 256 and c["packed"] for c in longs)
    assert all(A.supported(c["T"], c["C"]) for c in A.CASES.values())


def test_refusal_list_agrees_with_the_sources():
    ok_T = [T for T in range(0, 5000) if A.supported(T, 128)]
    assert ok_T == [128] + list(range(256, 4097, 256))
    assert [C for C in range(0, 1025) if A.supported(128, C)] == [128, 256]
    for T in (64, 196, 384, 4352):
        assert not A.supported(T, 128) and not A.supported(T, 256)
    for C in (64, 512):
        assert not A.supported(128, C) and not A.supported(1024, C)
    hdr = open(os.path.join(ROOT, "include", "pnpflow_hip.h")).read()
    assert "Shapes: T in {128, 256, 512, 768, ... 4096}, C in {128, 256}; anything else returns PF_ERR_INVALID" in hdr
    src = open(os.path.join(ROOT, "pnpflow_amd", "csrc", "attention.hip")).read()
    assert ("bool attn_fused_supported(int T, int C) { return (T == 128 || (T >= 256 && T % 256 == 0 && T <= 4096)) && (C == 128 || C == 256); }") in src
    assert "constexpr int TB = 256" in src and A.TB == 256
    # the additive entry point: declared, bound, and the ABI version is what it was
    import pnpflow_amd._lib as L
    assert "int pf_attention_core_ex(const float* qkv, float* out, int B, int T, int C, const float* bias, const float* residual, float* stats_part, double* stats," in hdr
    assert len(L.SIGNATURES["pf_attention_core_ex"][1]) == 11 and len(L.SIGNATURES["pf_attention_core"][1]) == 6
    assert re.search(r"#define\s+PF_ABI_VERSION\s+6\b", hdr) and L.PF_ABI_VERSION == 6


# ---- recipes ------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(128, 128, 2), (256, 256, 1), (512, 128, 2), (768, 256, 1), (2048, 128, 2), (4096, 256, 1)]


def rows(T, C, B, recipe):
    """per image: fp64 logits [T][T]"""
    qkv = A.inputs(T, C, B, recipe)
    for b in range(B):
        yield A.logits64(qkv[b:b + 1])[0].numpy()


def block_max(s):
    T = s.shape[1]
    return s.reshape(s.shape[0], max(T // A.TB, 1), -1).max(axis=2)


@pytest.mark.parametrize("T,C,B", [(128, 128, 9), (256, 256, 9), (768, 128, 9)])
def test_peaked_and_flat(T, C, B):
    for s in rows(T, C, B, "peaked"):
        assert (s.max(axis=1) - s.min(axis=1)).min() >= 8.0             # a peaked softmax: e^8 between the ends of every row
    for s in rows(T, C, B, "flat"):
        p = np.exp(s - s.max(axis=1, keepdims=True)); p /= p.sum(axis=1, keepdims=True)
        assert p.min() * T >= 0.5 and p.max() * T <= 2.0                # all p ~ 1/T
        if not A.is_long(T):                                            # the short kernel splits the normalised P: its lo half is subnormal throughout
            _, lo = A.unpack_hilo(A.pack_hilo(p.astype(np.float32)))
            assert np.abs(lo.astype(np.float64)).max() < 2.0 ** -14


@pytest.mark.parametrize("T,C,B", [s for s in SHAPES if s[0] >= 512])
def test_rising_falling_last_wide(T, C, B):
    for s in rows(T, C, B, "rising"):
        assert np.diff(block_max(s), axis=1).min() >= 5.0               # every block raises the maximum of EVERY row: every block rescales acc_o
    for s in rows(T, C, B, "falling"):
        bm = block_max(s)
        assert np.diff(bm, axis=1).max() <= -5.0
        assert np.all(s.argmax(axis=1) < A.TB)
        e = np.exp((s - s.max(axis=1, keepdims=True)).astype(np.float32))
        assert e.dtype == np.float32 and np.all(e[:, A.TB:] == 0.0) and np.all(e[:, :A.TB] > 0.0)     # everything past the first block underflows to 0, in every row
    for s in rows(T, C, B, "last"):
        assert np.all(s.argmax(axis=1) >= T - 32)
        assert np.all(s[:, T - 32:].max(axis=1) - s[:, :T - 32].max(axis=1) >= 2.0)
    for s in rows(T, C, B, "wide"):
        assert s.max(axis=1).min() >= 75.0 and s.min(axis=1).max() <= -75.0 and np.abs(s).max() <= 85.0
        with np.errstate(over="raise"):
            tot = np.exp(s.astype(np.float32)).sum(axis=1, dtype=np.float32)  # no overflow even without the subtraction of the maximum
        assert np.all(np.isfinite(tot)) and tot.max() < 1e37


@pytest.mark.parametrize("T,C,B", [(128, 128, 2), (512, 256, 1)])
def test_operand_range_recipes(T, C, B):
    for recipe, top in (("small_v4", 1e-3), ("small_v6", 1e-5)):
        qkv = A.inputs(T, C, B, recipe)
        assert np.abs(qkv[..., 2 * C:]).max() < top
        ref, pv = A.reference(qkv)
        assert np.all(A.ATTN_RTOL * np.abs(pv).reshape(B, -1).max(axis=1) < 0.25 * A.ABS_TERM)        # the absolute term is what holds
        _, lo = A.unpack_hilo(A.pack_hilo(qkv[..., 2 * C:]))
        assert np.abs(lo.astype(np.float64)).max() < 2.0 ** -14                                       # v's lo half is subnormal (or zero) throughout
    qkv = A.inputs(T, C, B, "small_k")
    assert np.abs(qkv[..., C:2 * C]).max() < 6e-3 and np.abs(qkv[..., :C]).max() > 90.0
    _, lo = A.unpack_hilo(A.pack_hilo(qkv[..., C:2 * C]))
    assert np.abs(lo.astype(np.float64)).max() < 2.0 ** -14
    s = A.logits64(qkv).numpy()
    assert 0.05 < (s.max(axis=2) - s.min(axis=2)).min() and np.abs(s).max() < 1.0                     # the keys still decide the weights
    qkv = A.inputs(T, C, B, "big")
    for part in (qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]):
        assert 5.99e4 <= np.abs(part).max() <= 6.0e4 < A.FP16_MAX
    hi, lo = A.unpack_hilo(A.pack_hilo(qkv))
    assert np.all(np.isfinite(hi.astype(np.float32))) and np.all(np.isfinite(lo.astype(np.float32)))


# ---- the design passes every case -------------------------------------------------------------------------------------------------------------------
_EMU = {}


@pytest.mark.parametrize("name", list(A.CASES))
def test_emulated_kernel_arithmetic_stays_within_bound(name):
    """packed and plain share their arithmetic (the same split, made earlier), so they share the emulation"""
    c = A.CASES[name]
    key = (c["T"], c["C"], c["B"], c["recipe"], c["epilogue"])
    if key not in _EMU:
        qkv, bias, res = A.case_inputs(name)
        ref, pv = A.case_reference(name)
        bd = A.bound(ref, pv, c["epilogue"] == "folded")
        _EMU[key] = (A.max_err(A.emulate(qkv, bias, res), ref), bd)
    err, bd = _EMU[key]
    assert bd.shape == (c["B"],) and np.all(err <= bd), (name, err, bd)


def test_bound_terms():
    pv = np.zeros((2, 4, 3)); pv[1, 2, 1] = -3.0
    ref = pv + 1.0
    assert np.allclose(A.bound(pv, pv), [2.0 ** -24, 6e-5 + 2.0 ** -24], rtol=1e-12)
    assert np.allclose(A.bound(ref, pv), [2.0 ** -24 + 2.0 ** -23, 6e-5 + 2.0 ** -24 + 2.0 ** -22], rtol=1e-12)
    assert np.array_equal(A.bound(ref, pv, folded=False), A.bound(pv, pv))
    assert A.max_err(np.array([[1.0, np.nan]]), np.zeros((1, 2)))[0] == np.inf
    assert (A.ATTN_RTOL, A.ABS_TERM, A.FOLD_TERM, A.S1_RTOL, A.S2_RTOL) == (2e-5, 2.0 ** -24, 2.0 ** -23, 2.0 ** -19, 2.0 ** -18)


def test_emulation_would_notice_a_dropped_term_or_a_missing_rescale():
    """the bound is tight enough for what it is meant to catch: one of the three MFMA terms dropped, the rescale of the accumulated output left out"""
    import torch
    qkv = A.inputs(768, 128, 9, "peaked")[:1]
    ref, pv = A.reference(qkv)
    bd = A.bound(ref, pv, False)
    q, k, v = (torch.from_numpy(np.array(qkv[0, :, i * 128:(i + 1) * 128])) for i in range(3))
    p = torch.softmax(A.logits64(qkv)[0], dim=-1)
    no_lo = (p @ v.half().double()).numpy()[None]                       # P (v hi) only
    assert A.max_err(no_lo, ref)[0] > 4 * bd[0]
    s = A.logits64(qkv)[0]
    acc, m, l = torch.zeros(768, 128, dtype=torch.float64), torch.full((768, 1), -np.inf, dtype=torch.float64), torch.zeros(768, 1, dtype=torch.float64)
    for k0 in range(0, 768, A.TB):
        m_new = torch.maximum(m, s[:, k0:k0 + A.TB].max(dim=1, keepdim=True).values)
        e = torch.exp(s[:, k0:k0 + A.TB] - m_new)
        l = l * torch.exp(m - m_new) + e.sum(dim=1, keepdim=True); m = m_new
        acc = acc + e @ v[k0:k0 + A.TB].double()                        # no rescale
    assert A.max_err((acc / l).numpy()[None], ref)[0] > 100 * bd[0]
