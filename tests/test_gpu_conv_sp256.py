"""conv_sp's 256-channel form (round 7): the GroupNorm + SiLU 3x3 convs of the 256-channel level (ResidualBlock conv1 / conv2, models.py:58-113 at level
width 256) as two 128-channel N-halves of conv_sp_kernel<2, 4> (NSPLIT = 2) instead of conv_dma behind a prep pass.

Three views: the kernel alone against its reference kernel (tools/ubench/conv_sp_probe), whole forwards against the conv_dma path (test-only switch
PNPFLOW_HIP_SP=4), and which launches the engine hands to it (per-launch CSV).  The packer's half images are checked on the CPU in
test_weight_pack_halves.py.
"""
import os

import pytest

from test_gpu_parity import _ab_forwards, _profile_rows, _run_probe, hip, model_for  # noqa: F401  (hip: the module-scoped library fixture)

pytestmark = pytest.mark.gpu


# (H, W, B, chunks, residual): the smallest launches at which the N-half mapping can go wrong, on the probe's grid of 256 workgroups = 128 pairs
#   16 x 16 x 520, 16 chunks: one tile per image that touches all four borders (lx = ly = 0); 520 tiles over 128 pairs - ragged ranges
#   32 x 32 x 131, 16 chunks: corner tiles, the identity residual at pixel stride 256, ragged
#   16 x 32 x 260, 24 chunks: the cat[256, 128] launch
#   32 x 32 x 128, 32 chunks: the cat[256, 256] launch - the whole chunk table (PP_MAXCH)
@pytest.mark.parametrize("shape", [(16, 16, 520, 16, 0), (32, 32, 131, 16, 1), (16, 32, 260, 24, 1), (32, 32, 128, 32, 0)])
def test_conv_sp_n_halves_match_the_reference_kernel(hip, shape):
    """conv_sp_kernel<2, 4, *, 3, 2> ALONE against the probe's reference kernel over all 256 output channels (each half's weights read from that half's
    image; a bias that differs per image and channel) on every 7th pixel: 2e-5 of max|reference|; and stats_out of one launch, per image and channel of
    both halves, against fp64 sums of the kernel's own output within n 2^-24 of sum|v| (sum v^2), n = 256 fp32 addends per lane between two flushes
    (derivation next to the check in the probe).  The probe prints PARITY OK only when both hold."""
    H, W, B, nch, res = shape
    out = _run_probe("conv_sp_probe", (H, W, B, nch, res, 8, 0, 256, 3))
    assert "PARITY OK" in out and "FAIL" not in out, out[-1500:]


def test_conv_sp_n_halves_forward_matches_conv_dma(hip, tmp_path):
    """Whole forwards of the 256^2 net at U-Net batch 161 (ragged: 644 pixel tiles = 1 288 items, above the threshold of 4 per workgroup): with
    PNPFLOW_HIP_SP=4 the 256-channel level stays on conv_dma, with =1 its 22 GroupNorm-ed 3x3 launches run as N-halves on conv_sp.  The same products in
    another summation order: 2e-6 of max|v|.  Swapped halves, a wrong weight-row offset or wrong statistics (they feed the next GroupNorm) are O(1)."""
    _ab_forwards(tmp_path, (("afhq256", 161),), dict(PNPFLOW_HIP_SP="4"), dict(PNPFLOW_HIP_SP="1"), "sp256")


def test_conv_sp_takes_the_256_channel_level_at_the_headline_batch_only(hip, tmp_path):
    """Per-launch CSV of the 256^2 net.  At U-Net batch 160 (1 280 items over 256 workgroups) the Cout 256 launches on conv_sp (dma = 5) are conv1 / conv2 of
    the 256-channel ResidualBlocks: K = 2304 x 14, 4608 x 6 (cat[256, 256]), 3456 (cat[256, 128]) and 1152 (128 -> 256); the launches with a folded 1x1
    shortcut (K = 2816 / 2688 / 2432) stay on conv_mfma16 (dma = 0), the upsampling convs and the stacked q,k,v conv (Cout 768) on conv_dma (dma = 1).  At
    batch 80 (640 items) no Cout 256 launch is on conv_sp."""
    if os.environ.get("PNPFLOW_HIP_SP") not in (None, "1") or os.environ.get("PNPFLOW_HIP_DMA") not in (None, "1"):
        return
    m, cfg, sd = model_for("afhq256")
    rows = _profile_rows(m, 160, 256, tmp_path, "layers_sp256_160.csv")
    c256 = [r for r in rows if int(r["Cout"]) == 256]
    assert sorted(int(r["K"]) for r in c256 if int(r["dma"]) == 5) == sorted([2304] * 14 + [4608] * 6 + [3456, 1152])
    assert all(int(r["stride"]) == 1 and int(r["up"]) == 0 and int(r["H"]) == 32 for r in c256 if int(r["dma"]) == 5)
    folded = [r for r in c256 if int(r["K"]) in (2816, 2688, 2432)]
    assert folded and all(int(r["dma"]) == 0 for r in folded), [(r["K"], r["dma"]) for r in folded]
    up = [r for r in rows if int(r["up"]) == 2]
    assert up and all(int(r["dma"]) == 1 for r in up)
    qkv = [r for r in rows if int(r["Cout"]) == 768]
    assert len(qkv) == 1 and int(qkv[0]["dma"]) == 1
    rows80 = _profile_rows(m, 80, 256, tmp_path, "layers_sp256_80.csv")
    assert not any(int(r["Cout"]) == 256 and int(r["dma"]) == 5 for r in rows80)
