"""References of the fused attention core (pf_attention_core / pf_attention_core_ex, csrc/attention.hip): the case table the GPU tests
(tests/test_gpu_attention_paths.py) and the host tests (tests/test_attention_reference_host.py) share, the input recipes, the packed fp16 pair
of the keys and values, the fp64 reference, the fp32 formulation of the unfused path, a restatement of the kernel's documented arithmetic and
the derived error bound.  numpy and torch on the CPU only (the numbers come from conftest.det_normal's numpy Philox recipe).

  out[b] = softmax(q k^T * C^-1/2, dim=-1) v   (+ bias[c] + residual[b][t][c] with the folded output projection),   qkv = [B][T][q | k | v]

The kernel's arithmetic (attention.hip): every operand of the two contractions is split into an fp16 pair hi = RNE16(x), lo = RNE16(x - hi), a
product is lo*hi + hi*lo + hi*hi accumulated in fp32 (lo*lo is dropped).  T <= 256: the normalised probabilities are split.  T >= 512: the keys
are walked in blocks of 256 with a running row maximum m and row sum l, P = exp(S - m) is split UNNORMALISED, the accumulated output is
rescaled by exp(m_old - m_new) per block and divided by l once at the end."""
import functools
import math

import numpy as np
import torch

TB = 256                    # keys per block of the long kernel
FP16_MAX = 65504.0
RECIPES = ("peaked", "flat", "rising", "falling", "last", "wide", "small_v4", "small_v6", "small_k", "big")
RISE = 6.0                  # rising: logit step between the key blocks' common offsets (the noise spread leaves >= 5 between their row maxima)
FALL = 110.0                # falling: ... so that exp(later block - maximum) is below half of fp32's smallest subnormal (e^-103.98)
NOISE = 0.3                 # scale of q and k under the structured recipes: logit noise of standard deviation ~0.09


def supported(T, C):
    """the shapes attn_fused_supported (attention.hip) takes; everything else is refused"""
    return (T == 128 or (T >= 256 and T % 256 == 0 and T <= 4096)) and C in (128, 256)


def is_long(T):
    return T > 256


def instantiation(T, C, packed):
    """the kernel template launch_attn_fused picks"""
    kv = "true" if packed else "false"
    return f"attn_fused_long_kernel<{C // 128},{kv}>" if is_long(T) else f"attn_fused_kernel<{T // 128},{C // 128},{kv}>"


# ---- case table -------------------------------------------------------------------------------------------------------------------------------
def _case(T, C, B, recipe, packed, epilogue):
    assert supported(T, C) and recipe in RECIPES and epilogue in ("plain", "folded")
    return dict(T=T, C=C, B=B, recipe=recipe, packed=bool(packed), epilogue=epilogue)


def _name(group, c):
    return f"{group}-T{c['T']}-C{c['C']}-B{c['B']}-{c['recipe']}-{'packed' if c['packed'] else 'plain'}-{c['epilogue']}"


VARIANT_SHAPES = ((128, 128), (128, 256), (256, 128), (256, 256), (768, 128), (768, 256))     # x packed / plain = the 12 instantiations; 768 = 3 key blocks
LONG_T = (512, 768, 2048, 4096)
CASES = {}
# every instantiation x both epilogues; B = 9: two groups of 8 images (one per XCD), the workgroups of images 9..15 exit
for _T, _C in VARIANT_SHAPES:
    for _packed in (False, True):
        for _epi in ("plain", "folded"):
            for _r in ("peaked", "flat"):
                _c = _case(_T, _C, 9, _r, _packed, _epi); CASES[_name("variant", _c)] = _c
# the online softmax of the long kernel: C = 128 at B = 2 (plain), C = 256 at B = 1 (packed; T = 4096 is the largest launch: 12.6 MB of qkv)
for _T in LONG_T:
    for _r in ("rising", "falling", "last", "wide"):
        for _C, _B, _packed in ((128, 2, False), (256, 1, True)):
            _c = _case(_T, _C, _B, _r, _packed, "plain"); CASES[_name("long", _c)] = _c
# operand range: one short and one long shape
for _T, _C, _B in ((128, 128, 2), (512, 256, 1)):
    for _r in ("small_v4", "small_v6", "small_k", "big"):
        for _packed in (False, True):
            _c = _case(_T, _C, _B, _r, _packed, "plain"); CASES[_name("range", _c)] = _c


def names(group):
    return [n for n in CASES if n.startswith(group + "-")]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def _det_normal(shape, seed, idx):
    from conftest import det_normal
    return det_normal(shape, seed, idx).numpy()


def block_offsets(T, recipe):
    """the last channel of the keys under the structured recipes, as logit offsets per key (q's last channel is C^1/2, so the offset arrives unscaled).
    The LAST channel: the fp32 accumulation of q k^T then carries the large term through its final steps only.  A logit of magnitude 80 has an fp32
    spacing of 7.6e-6 however it is computed; every rounding of a partial sum at the unscaled magnitude (80 C^1/2) adds as much to it: with the
    large term in channel 0 the fp32 formulation itself was at 1.9 x `bound` on the wide recipe."""
    j = np.arange(T)
    nblk = max(T // TB, 1)
    blk = np.minimum(j // TB, nblk - 1)
    if recipe == "rising":
        return -RISE * (nblk - 1 - blk)                    # the last block sits at 0: the logits are small where the probabilities are not
    if recipe == "falling":
        return -FALL * blk
    if recipe == "last":
        return np.where(j >= T - 32, 4.0, 0.0)
    if recipe == "wide":
        perm = np.random.Generator(np.random.Philox(key=[7599, T])).permutation(T)
        return 80.0 - 160.0 * perm / (T - 1)
    raise ValueError(recipe)


@functools.lru_cache(maxsize=6)
def inputs(T, C, B, recipe):
    """qkv [B][T][3C] fp32, read-only"""
    x = _det_normal((B, T, 3 * C), 7500 + RECIPES.index(recipe), T * 4 + C // 128).copy()
    q, k, v = x[..., :C], x[..., C:2 * C], x[..., 2 * C:]
    if recipe in ("peaked", "small_v4", "small_v6"):
        q *= 3.0
        if recipe != "peaked":
            v *= np.float32(1e-4 if recipe == "small_v4" else 1e-6)
    elif recipe == "flat":
        q *= np.float32(0.05)
    elif recipe == "small_k":
        q *= 30.0; k *= np.float32(1e-3)
    elif recipe == "big":
        for part in (q, k, v):
            part *= np.float32(6.0e4) / np.abs(part).max()
            np.clip(part, -6.0e4, 6.0e4, out=part)
    else:
        q *= np.float32(NOISE); k *= np.float32(NOISE)
        q[..., C - 1] = np.float32(math.sqrt(C))
        k[..., C - 1] = block_offsets(T, recipe).astype(np.float32)[None, :]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=6)
def epilogue_inputs(T, C, B):
    """(bias [C], residual [B][T][C]) of the folded output projection, fp32, read-only"""
    bias = _det_normal((C,), 7520, T * 4 + C // 128)
    res = _det_normal((B, T, C), 7521, T * 4 + C // 128)
    bias.setflags(write=False); res.setflags(write=False)
    return bias, res


def case_inputs(name):
    """(qkv, bias or None, residual or None) of a table case"""
    c = CASES[name]
    qkv = inputs(c["T"], c["C"], c["B"], c["recipe"])
    if c["epilogue"] == "plain":
        return qkv, None, None
    return (qkv,) + epilogue_inputs(c["T"], c["C"], c["B"])


# ---- the packed fp16 pair -----------------------------------------------------------------------------------------------------------------------
def pack_hilo(x):
    """fp32 -> int32 words hi | lo << 16, hi = RNE16(x), lo = RNE16(x - hi): pf_common.h pack_hilo / ConvParams::pack_from_p1.  Integers, so that no
    word that happens to be a NaN pattern is ever copied as a float."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)                          # numpy rounds to nearest even and keeps subnormals
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    w = hi.view(np.uint16).astype(np.uint32) | (lo.view(np.uint16).astype(np.uint32) << np.uint32(16))
    return w.view(np.int32)


def unpack_hilo(w):
    """int32 words -> (hi, lo) as float16 arrays"""
    u = np.ascontiguousarray(w, dtype=np.int32).view(np.uint32)
    return (u & np.uint32(0xFFFF)).astype(np.uint16).view(np.float16), (u >> np.uint32(16)).astype(np.uint16).view(np.float16)


def packed_qkv(qkv):
    """the int32 image of qkv with the k and v thirds packed (q stays fp32), as the stacked q,k,v conv leaves it"""
    C = qkv.shape[-1] // 3
    w = np.ascontiguousarray(qkv, dtype=np.float32).view(np.int32).copy()
    w[..., C:] = pack_hilo(qkv[..., C:])
    return w


# ---- fp64 reference, fp32 formulation ---------------------------------------------------------------------------------------------------------------
def _qkv_t(qkv, dtype):
    C = qkv.shape[-1] // 3
    t = torch.from_numpy(np.array(qkv)).to(dtype)
    return t[..., :C], t[..., C:2 * C], t[..., 2 * C:]


def logits64(qkv):
    """[B][T][T] fp64 scaled scores"""
    q, k, _ = _qkv_t(qkv, torch.float64)
    return torch.bmm(q, k.transpose(1, 2)) * (q.shape[-1] ** -0.5)


def reference(qkv, bias=None, residual=None):
    """(ref, pv) fp64 numpy [B][T][C]: pv = softmax(q k^T C^-1/2) v, ref = pv (+ bias + residual)"""
    _, _, v = _qkv_t(qkv, torch.float64)
    pv = torch.bmm(torch.softmax(logits64(qkv), dim=-1), v).numpy()
    ref = pv
    if residual is not None:
        ref = pv + (0.0 if bias is None else np.asarray(bias, dtype=np.float64)) + np.asarray(residual, dtype=np.float64)
    return ref, pv


@functools.lru_cache(maxsize=8)
def _reference_of(T, C, B, recipe, epilogue):
    qkv = inputs(T, C, B, recipe)
    bias, res = epilogue_inputs(T, C, B) if epilogue == "folded" else (None, None)
    ref, pv = reference(qkv, bias, res)
    ref.setflags(write=False); pv.setflags(write=False)
    return ref, pv


def case_reference(name):
    """(ref, pv) of a table case, made once per (shape, recipe, epilogue) and read-only"""
    c = CASES[name]
    return _reference_of(c["T"], c["C"], c["B"], c["recipe"], c["epilogue"])


def stats64(out):
    """fp64 per image and channel (sum o, sum o^2, sum |o|) over the tokens of out [B][T][C] -> three [B][C] arrays"""
    o = np.asarray(out, dtype=np.float64)
    return o.sum(axis=1), (o * o).sum(axis=1), np.abs(o).sum(axis=1)


def fp32_formulation(qkv, bias=None, residual=None):
    """the unfused path's arithmetic in torch fp32: bmm, * C^-1/2, softmax, bmm (+ bias, + residual)"""
    q, k, v = _qkv_t(qkv, torch.float32)
    o = torch.bmm(torch.softmax(torch.bmm(q, k.transpose(1, 2)) * (q.shape[-1] ** -0.5), dim=-1), v)
    if residual is not None:
        if bias is not None:
            o = o + torch.from_numpy(np.array(bias))
        o = o + torch.from_numpy(np.array(residual))
    return o.numpy()


# ---- the kernel's documented arithmetic -------------------------------------------------------------------------------------------------------------
def _split(x):
    """fp32 tensor -> (hi, lo) of split4, as fp64 (torch's half conversion rounds to nearest even and keeps subnormals)"""
    hi = x.half().float()
    lo = (x - hi).half().float()
    return hi.double(), lo.double()


def _prod3(a, b):
    """lo*hi + hi*lo + hi*hi of two split operands, exact sums (the fp32 accumulation noise of the MFMA is left out), rounded to fp32 once"""
    (ah, al), (bh, bl) = a, b
    return (al @ bh + ah @ bl + ah @ bh).float()


def emulate(qkv, bias=None, residual=None):
    """The kernel's arithmetic restated on the CPU -> fp32 numpy [B][T][C]; the short form for T <= 256, the key-blocked form above"""
    q, k, v = _qkv_t(qkv, torch.float32)
    B, T, C = q.shape
    scale = torch.tensor(1.0 / math.sqrt(C), dtype=torch.float32)
    out = torch.empty((B, T, C), dtype=torch.float32)
    for b in range(B):
        qs = _split(q[b])
        if not is_long(T):
            kh, kl = _split(k[b])
            s = _prod3(qs, (kh.T, kl.T)) * scale
            e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
            p = e * (1.0 / e.sum(dim=-1, keepdim=True))
            o = _prod3(_split(p), _split(v[b]))
        else:
            m = torch.full((T, 1), -math.inf, dtype=torch.float32)
            l = torch.zeros((T, 1), dtype=torch.float32)
            acc = torch.zeros((T, C), dtype=torch.float32)
            for k0 in range(0, T, TB):
                kh, kl = _split(k[b, k0:k0 + TB])
                s = _prod3(qs, (kh.T, kl.T)) * scale
                m_new = torch.maximum(m, s.max(dim=-1, keepdim=True).values)
                sc = torch.exp(m - m_new)                          # 0 on the first block
                e = torch.exp(s - m_new)
                l = l * sc + e.sum(dim=-1, keepdim=True)
                m = m_new
                acc = (acc * sc + _prod3(_split(e), _split(v[b, k0:k0 + TB]))).float()
            o = acc * (1.0 / l)
        out[b] = o
    if residual is not None:
        if bias is not None:
            out = out + torch.from_numpy(np.array(bias))
        out = out + torch.from_numpy(np.array(residual))
    return out.numpy()


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------------
ATTN_RTOL = 2e-5            # of max|P v| per image: the project's attention tolerance (tests/test_gpu_parity.py)
ABS_TERM = 2.0 ** -24       # two half-spacings of fp16's smallest subnormal (2^-24): the rounding of the lo half of v and of P
FOLD_TERM = 2.0 ** -23      # x max|ref|: the two rounded fp32 additions of the folded epilogue
S1_RTOL = 2.0 ** -19        # of sum|o|: 31 roundings of a 32-term fp32 sum (the tiles are added in fp64)
S2_RTOL = 2.0 ** -18        # of sum o^2: ... plus one rounding per square


def bound(ref, pv, folded=None):
    """per image [B]: the largest |out - ref| the design allows.  folded: whether ref carries the epilogue (default: ref is not pv itself)"""
    ref, pv = np.asarray(ref), np.asarray(pv)
    if folded is None:
        folded = ref is not pv and not np.array_equal(ref, pv)
    B = pv.shape[0]
    bd = ATTN_RTOL * np.abs(pv).reshape(B, -1).max(axis=1) + ABS_TERM
    if folded:
        bd = bd + FOLD_TERM * np.abs(ref).reshape(B, -1).max(axis=1)
    return bd


def max_err(out, ref):
    """per image [B]: max|out - ref| in fp64 (inf where out is not finite)"""
    o = np.asarray(out, dtype=np.float64)
    d = np.abs(o - ref).reshape(o.shape[0], -1)
    d[~np.isfinite(d)] = np.inf
    return d.max(axis=1)
