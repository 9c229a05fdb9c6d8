// Kernel routing: the one place that decides which kernel, which template instantiation and which launch geometry a convolution gets.
// Host-only and free of HIP, of pointers and of the environment (plain C++17: tests/test_conv_route_host.py compiles it with the host compiler),
// so that every launch a plan can contain is enumerable without a GPU.  The engine describes a launch as a RouteShape (pf_common.h:
// route_shape) plus the process' RouteEnv, asks conv_route() ONCE at plan build and stores the answer in the op; the launchers of the five
// kernel files switch on the answer's instantiation fields and select nothing themselves.
//
// Decision order:   terms 0 -> MFMA32;   conv_sp (Cout 64 / 128 / 256);   conv_pp (Cout 32);   conv_dma;
//                                    conv_mfma16 when every segment has a 16-bit weight image;   conv_mfma.
// The tile / LDS arithmetic below that a kernel file needs as well is defined here only and included from there.
#pragma once
#include <cstddef>

namespace pf {

constexpr int ROUTE_LDS_MAX = 160 * 1024;      // LDS of a gfx950 CU: every kernel's dynamic-LDS attribute is raised to it

// ---- conv_pp.hip: tile and LDS arithmetic shared with the kernel ------------------------------------------------------------------------
constexpr int PP_MAXCH = 32;     // conv_pp: <= 4 chunks of 32 channels; conv_sp: <= 32 chunks of 16 channels (cat[256, 256] -> 256)
// MT = M-tiles (2 rows x 16 pixels) per wave: a team's tile is 8 MT rows x 16 columns, its halo patch (8 MT + 2) x 18 pixels x 128 B
constexpr int PP_PW = 18;
constexpr int pp_w9(int TERMS) { return TERMS == 3 ? 36864 : 18432; }      // LDS bytes of a 9-tap / 1-tap 32-channel chunk image ([k16-step][hi | lo] or [k16-step][hi])
constexpr int pp_w1(int TERMS) { return TERMS == 3 ? 4096 : 2048; }
constexpr int pp_npix(int MT) { return (8 * MT + 2) * PP_PW; }
constexpr int pp_patch_bytes(int MT) { return pp_npix(MT) * 128; }                         // MT 1: 23 040 B, MT 2: 41 472 B per team
constexpr int PP_MT = 1;      // 8 x 16-pixel team tiles: at 2 waves per SIMD two register sets of raw patch + the residual + accumulators fit 256 registers.
                              // (16 x 16 tiles - MT = 2, 11 float4 per prefetch set - spill 57-156 registers with the two-step prefetch and measured
                              // +30 ... +70 % per launch, r4; they would need conv_pp64's one-step re-request scheme)
constexpr size_t pp_weight_bytes(int n9, int n1, int TERMS) { return (size_t)n9 * pp_w9(TERMS) + (size_t)n1 * pp_w1(TERMS); }
// TEAMS = 1: two independent 4-wave workgroups per CU (each with its own copy of the weights) where LDS allows - the teams of one
// 8-wave workgroup wait for each other at every phase boundary, independent workgroups only for their own data (r4: 192 vs 214 us on the
// one-chunk conv); TEAMS = 2 (one workgroup per CU, weights shared) for the structures whose weights do not fit twice
constexpr int pp_teams(int n9, int n1, int TERMS) { return 2 * (pp_weight_bytes(n9, n1, TERMS) + pp_patch_bytes(PP_MT)) <= (size_t)ROUTE_LDS_MAX ? 1 : 2; }
constexpr size_t pp_lds(int n9, int n1, int TEAMS, int TERMS) { return pp_weight_bytes(n9, n1, TERMS) + (size_t)TEAMS * pp_patch_bytes(PP_MT); }
// chunk structures instantiated: ResidualBlock conv1 / conv2 of the down path (one 3x3 chunk, with / without the identity residual), conv1 of
// the up path over cat[h, skip] (two / three 3x3 chunks), conv2 of the up path with the folded 1x1 shortcut (one 3x3 + two / three 1x1 chunks)
constexpr bool pp_structure(int n9, int n1, bool res) {
    if (res) return n9 == 1 && n1 == 0;
    return (n1 == 0 && n9 >= 1 && n9 <= 3) || (n9 == 1 && (n1 == 2 || n1 == 3));
}

// ---- conv_sp.hip ------------------------------------------------------------------------------------------------------------------------
constexpr int SP_PITCH = 20, SP_PW = 18;
constexpr int sp_rows(int MT) { return 8 * MT; }                                   // tile rows
constexpr int sp_npix(int MT) { return (sp_rows(MT) + 2) * SP_PW; }
constexpr int sp_patch(int MT) { return (sp_rows(MT) + 2) * SP_PITCH * 64; }      // MT 2: 23 040 B
// TERMS = 3: the fp32-equivalent split; TERMS = 1 (round 6): precision mode 2 - hi-only operands, one MFMA per (M-tile, N-tile) and tap, hi-only weight
// images (a tap is NT KiB; slot X is rounded up to whole 4 KiB refill rounds: at NT = 2 its five taps are 10 KiB and the refill fetches 12 - the two
// extra KiB are the head of tap 5 in the chunk image, never read from X)
constexpr int sp_tap(int NT, int TERMS = 3) { return (TERMS == 3 ? 2 : 1) * NT * 1024; }      // bytes of one tap: (hi | lo) x NT x 1 KiB
constexpr int sp_x(int NT, int TERMS = 3) { return (5 * sp_tap(NT, TERMS) + 4095) / 4096 * 4096; }      // slot X: taps 0..4
constexpr int sp_y(int NT, int TERMS = 3) { return 4 * sp_tap(NT, TERMS); }                  // slot Y: taps 5..8
constexpr int SP_TAB = PP_MAXCH * 32;                                               // chunk table: 32 B per chunk (see the kernel's prologue)
constexpr int sp_lds(int MT, int NT, int TERMS = 3) { return sp_x(NT, TERMS) + sp_y(NT, TERMS) + 2 * sp_patch(MT) + SP_TAB; }

// ---- conv_dma.hip -----------------------------------------------------------------------------------------------------------------------
// tile of the only instantiated shape: 8 x 16 pixels x 128 output channels (4 M-tiles per weight fragment, one N-tile per wave)
constexpr int DMA_TH = 8, DMA_BN = 128;
constexpr size_t dma_lds() {      // two buffers of the (TH + 2) x 18-pixel patch, in whole rounds of four 1 KiB LDS-DMA instructions
    constexpr int PH = DMA_TH + 2, PW = 18, NINST = (PH * PW * 8 + 63) / 64, IPW = (NINST + 3) / 4, BUF = IPW * 4 * 1024;
    return 2 * (size_t)BUF;
}

// ---- the interface ----------------------------------------------------------------------------------------------------------------------
struct RouteSeg {
    int C = 0, cstride = 0, taps = 0, xform = 0, w_mode = 0;      // ConvSeg's
    bool has_w16 = false;                      // the segment carries a split-fp16 weight image (ConvSeg::w16)
    // ... and the engine knows the host tensor slice that image was packed from (the further images - hi-only, LDS chunks - are packed from it):
    // input channels [src_lo, src_hi) of an OIHW tensor of src_O output channels and src_kk taps.  has_w16_src implies has_w16.
    bool has_w16_src = false;
    int src_lo = 0, src_hi = 0, src_O = 0, src_kk = 0;
};
struct RouteShape {      // the facts of ConvParams a decision may depend on - no pointers
    RouteSeg seg[3];
    int nseg = 0, B = 0, H = 0, W = 0, Hs = 0, Ws = 0, Cout = 0, out_cstride = 0, res_cstride = 0, gn_C = 0;
    bool residual = false, addvec = false, coef = false, scale = false, gnb = false;      // ConvParams::residual / addvec / coef / scale / gnb_x != nullptr
};
struct RouteEnv {
    int cu_grid = 0;      // persistent_grid() of the device: one workgroup per CU, a multiple of the 8 XCDs; 0 = unknown (the persistent kernels are refused)
    // the four test-only A/B switches, defaults = shipped:
    int pp = 1;           // PNPFLOW_HIP_PP: 0 off, 1 on, 3 on in the default mode only (mode 2 on conv_mfma16)
    int sp = 1;           // PNPFLOW_HIP_SP: 0 off, 1 on, 2 the 128-channel level only, 3 on in the default mode only, 4 as 1 but the 256-channel level stays on conv_dma
    int dma = 1;          // PNPFLOW_HIP_DMA: 0 off, 1 where the grid fills the chip, 2 wherever the shape is supported (tests)
    int upphase = 1;      // PNPFLOW_HIP_UPPHASE: 0 = the upsampling conv keeps its 9-tap form on the upsampled view
};
// the launches of the backward have no prep pass and no chunk list in front of them: they are routed with the three forward-only kernels off
inline RouteEnv mfma_only(RouteEnv env) { env.pp = env.sp = env.dma = 0; return env; }

enum class ConvFamily { MFMA32, MFMA16, DMA, PP, SP };      // conv_mfma.hip, conv_mfma16.hip, conv_dma.hip, conv_pp.hip, conv_sp.hip
struct ConvRoute {
    ConvFamily family = ConvFamily::MFMA32;
    int terms = 0;                                                    // the kernels' TERMS: 3 split-fp16, 1 single fp16 product, 0 exact fp32 (MFMA32 only)
    int MT = 0, NT = 0, WM = 0, WN = 0, S = 1, UP = 0, BM = 0, KC = 0;      // MFMA32 / MFMA16 / DMA instantiation (SP: MT, NT)
    int n9 = 0, n1 = 0, teams = 0, nsplit = 0; bool res = false, gnb = false;      // PP / SP instantiation; gnb: MFMA16's GroupNorm-backward epilogue
    int grid_x = 0, grid_y = 1, xcd_map = 0; size_t lds_bytes = 0;    // what the launcher passes to hipLaunchKernelGGL (xcd_map: ConvParams::xcd_map)
    int csv_code = 0;                                                 // the per-launch CSV's "dma" column: 0 conv_mfma / conv_mfma16, 1 conv_dma, 2 conv_pp, 5 conv_sp
    const char* refused = nullptr;                                    // non-null: no kernel runs this launch (the reason); the plan build fails with it
};

inline int ilog2_exact(int v) { int l = 0; while (l < 30 && (1 << l) < v) ++l; return (1 << l) == v ? l : -1; }

namespace route_detail {

inline bool packed16(const RouteShape& p) {
    for (int i = 0; i < p.nseg; ++i) if (p.seg[i].w_mode != 0 || !p.seg[i].has_w16) return false;
    return true;
}
// the LDS chunk images of conv_pp / conv_sp are packed from the host slice behind each segment's 16-bit image: all output channels of the tensor
inline bool chunk_sources(const RouteShape& p, bool nine_taps) {
    for (int i = 0; i < p.nseg; ++i) {
        const RouteSeg& s = p.seg[i];
        if (!s.has_w16_src || s.src_O != p.Cout || (nine_taps && s.src_kk != 9)) return false;
    }
    return true;
}

inline bool pp_ok(const RouteShape& p, int stride, int up, int terms, const RouteEnv& env, int& n9, int& n1) {
    constexpr int TH = 8 * PP_MT;
    if (env.pp == 0 || (terms != 3 && !(terms == 1 && env.pp != 3)) || stride != 1 || up != 0 || p.gnb) return false;
    if (p.Cout != 32 || p.out_cstride != 32 || (p.residual && p.res_cstride != 32)) return false;
    if (p.H % TH || p.W % 16 || p.Hs != p.H || p.Ws != p.W) return false;
    if (ilog2_exact(p.H / TH) < 0 || ilog2_exact(p.W / 16) < 0) return false;
    // a persistent grid pays its prologue (weights -> LDS per workgroup, two-step pipeline fill) over >= 32 tiles per team: measured at 256^2,
    // B = 8 / 16 / 32 / 80 -> +11 % / +1.5 % / -1.4 % / -3 % on the whole forward; smaller launches stay on conv_mfma16
    // (teams of the launch = 2 per CU; 32 x 512 tiles on the 256 CUs of an MI355X)
    if (env.cu_grid < 8 || (long long)p.B * (p.H / TH) * (p.W / 16) < 32LL * 2 * env.cu_grid) return false;
    if (p.W > 2048) return false;      // patch pixel offsets py * W + px are packed into 16 bits (pk9[])
    n9 = 0; n1 = 0;
    for (int i = 0; i < p.nseg; ++i) {
        const RouteSeg& s = p.seg[i];
        if (s.w_mode != 0 || !s.has_w16 || s.C % 32) return false;
        if (s.taps == 9) { if (n1 > 0 || s.xform == 0) return false; n9 += s.C / 32; }     // 9-tap chunks are GroupNorm-ed (their coefficient loads are unconditional)
        else if (s.taps == 1) { if (s.xform != 0) return false; n1 += s.C / 32; }
        else return false;
    }
    if (!pp_structure(n9, n1, p.residual)) return false;
    if (p.gn_C > 0 && !p.coef) return false;
    if (pp_weight_bytes(n9, n1, terms) + 2 * (size_t)pp_patch_bytes(PP_MT) > (size_t)ROUTE_LDS_MAX) return false;
    return chunk_sources(p, false);
}

inline bool sp_ok(const RouteShape& p, int stride, int up, int terms, const RouteEnv& env) {
    const int mode = env.sp;
    if (mode == 0 || (terms != 3 && !(terms == 1 && mode != 3)) || stride != 1 || up != 0 || p.gnb) return false;
    // Cout 256 (round 7): two N-halves of 128 channels (NSPLIT = 2), built for the default mode (terms 3) only
    const int nsplit = p.Cout == 256 ? 2 : 1;
    if (p.Cout != 128 && !(p.Cout == 64 && (mode == 1 || mode == 4)) && !(p.Cout == 256 && mode == 1 && terms == 3)) return false;
    if (p.out_cstride != p.Cout || (p.residual && p.res_cstride != p.Cout)) return false;
    // the hand-counted vmcnt in front of the first barrier of a tile's chunk 0 counts the NT bias loads of tile_inputs: a launch without a
    // bias vector would wait NT operations too loosely - such launches stay on conv_mfma16
    if (!p.addvec) return false;
    const int TH = p.Cout == 64 ? sp_rows(4) : sp_rows(2);      // 16 x 16-pixel workgroup tiles at 128 (and 2 x 128) channels, 32 x 16 at 64
    if (p.H % TH || p.W % 16 || p.Hs != p.H || p.Ws != p.W) return false;
    // the staging packs the patch-pixel offset py * W + px (py <= TH + 1, px <= 17) into 16 bits (pk[], issue_one): ADVICE r5 - the bound
    // depends on the tile height, W <= 1024 at Cout 64 / W <= 2048 at Cout 128
    if ((long long)(TH + 1) * p.W + SP_PW - 1 > 65535) return false;
    if (ilog2_exact(p.H / TH) < 0 || ilog2_exact(p.W / 16) < 0) return false;
    // the persistent grid pays its prologue and pipeline fill over >= 4 tiles per workgroup
    // (NSPLIT = 2: an item is a (tile, N-half); the workgroups pair up inside an XCD, so a grid of an even number of workgroups per XCD)
    const int grid = env.cu_grid;
    if (grid < 8 || (long long)nsplit * p.B * (p.H / TH) * (p.W / 16) < 4LL * grid || (nsplit == 2 && grid % 16 != 0)) return false;
    int nch = 0;
    for (int i = 0; i < p.nseg; ++i) {
        const RouteSeg& s = p.seg[i];
        if ((double)p.B * p.H * p.W * s.cstride >= 2147483648.0) return false;      // 32-bit element offsets (describe)
        if (s.w_mode != 0 || !s.has_w16 || s.C % 32 || s.taps != 9 || s.xform != 2) return false;      // GroupNorm + SiLU 3x3 segments of an even number of 16-channel chunks
        nch += s.C / 16;
    }
    if (nch < 2 || nch > PP_MAXCH || (nch & 1)) return false;
    if (!(p.gn_C > 0 && p.coef && p.scale)) return false;      // (with_coef: every GroupNorm-ed split-fp16 launch carries operand scales)
    return chunk_sources(p, true);
}

// the phase form of the nearest-x2 upsampling conv (conv_dma's UP = 2): one raw segment whose 2 x 2 taps carry the four phase images
inline bool dma_phase_shape_ok(const RouteShape& p, int terms, const RouteEnv& env) {
    if (env.upphase == 0 || env.dma == 0 || (terms != 3 && terms != 1) || p.nseg != 1 || p.residual || p.gnb) return false;
    if (p.H != 2 * p.Hs || p.W != 2 * p.Ws || p.Hs % DMA_TH != 0 || p.Ws % 16 != 0 || p.Cout % 32 != 0 || (4 * p.Cout) % DMA_BN != 0) return false;
    if (p.seg[0].w_mode != 0 || p.seg[0].C % (terms == 3 ? 32 : 64) != 0) return false;
    if ((size_t)(p.Hs + 2) * (p.Ws + 2) * 128 >= (1ull << 31)) return false;
    if (env.dma >= 2) return true;
    return (long long)p.B * (p.Hs / DMA_TH) * (p.Ws / 16) * (4 * p.Cout / DMA_BN) >= 512;
}

inline bool dma_ok(const RouteShape& p, int stride, int up, int terms, const RouteEnv& env) {
    if (terms != 3 && terms != 1) return false;
    // the single-term mode reads hi-only images, packed from the host slice behind the split image in whole 64-channel chunks
    if (terms == 1)
        for (int i = 0; i < p.nseg; ++i)
            if (p.seg[i].w_mode != 0 || !p.seg[i].has_w16_src || (p.seg[i].src_hi - p.seg[i].src_lo) % 64 != 0) return false;
    if (env.dma == 0 || stride != 1 || (up != 0 && up != 1 && up != 2)) return false;
    if (p.gnb) return false;      // the GroupNorm-backward epilogue exists on conv_mfma16 only
    if (up == 2) return dma_phase_shape_ok(p, terms, env) && p.seg[0].taps == 4 && p.seg[0].has_w16;
    if (p.Cout % DMA_BN != 0 || p.H % DMA_TH != 0 || p.W % 16 != 0) return false;
    if (up == 1 && (p.H != 2 * p.Hs || p.W != 2 * p.Ws)) return false;
    if (up == 0 && (p.H != p.Hs || p.W != p.Ws)) return false;
    const int kc = terms == 3 ? 32 : 64;
    for (int i = 1; i < p.nseg; ++i) if (p.seg[i].taps == 9 && p.seg[i - 1].taps == 1) return false;     // ring phase: 9-tap chunks run at phase 0
    for (int i = 0; i < p.nseg; ++i) {
        const RouteSeg& s = p.seg[i];
        if (s.w_mode != 0 || !s.has_w16) return false;
        if (s.C % kc != 0 || (s.taps != 9 && s.taps != 1)) return false;
    }
    if ((size_t)(p.Hs + 2) * (p.Ws + 2) * 128 >= (1ull << 31)) return false;     // 32-bit piece offsets inside a plane
    if (env.dma >= 2) return true;
    const long long wgs = (long long)p.B * (p.H / DMA_TH) * (p.W / 16) * (p.Cout / DMA_BN);
    if (wgs < 512) return false;
    // The prep pass costs one read + one write of every operand element (measured: 30 us on average, 8 % of a forward when every
    // qualifying launch took this path - profiles/r03_ab_dma_variants.md), the conv it feeds is ~15 % faster than the register-staged
    // kernel.  It pays where a prepped element feeds enough multiply-adds: MACs per operand element = K_total * Cout / (channels
    // prepped per output pixel).  Same-box layer table: 2304 (16^2 x 256, one or two 3x3 segments) and the upsampling convs (operand
    // at quarter resolution) win, 1152 (32^2 x 128) and the launches that drag 1-tap shortcut segments along lose; the pure 1x1
    // launches win when Cout >= 3 C (q,k,v stacked), not at Cout = C.
    constexpr double min_ratio = 2000.0;      // (frozen in round 5: it was an environment knob while the layer table was measured)
    double macs = 0.0, elts = 0.0; bool all1 = true;
    for (int i = 0; i < p.nseg; ++i) { macs += (double)p.seg[i].taps * p.seg[i].C * p.Cout; elts += p.seg[i].C; all1 &= p.seg[i].taps == 1; }
    if (up) elts *= 0.25;
    if (all1) return p.Cout >= 3 * (int)elts;
    return macs / elts >= min_ratio;
}

// ---- the two MFMA kernels' tile ladders -------------------------------------------------------------------------------------------------
struct Tile { int MT, NT, WM, WN; };      // workgroup tile: 2 MT WM rows x 16 pixels x 32 NT WN output channels
constexpr int tile_th(const Tile& t) { return 2 * t.MT * t.WM; }
constexpr int tile_bn(const Tile& t) { return t.WN * t.NT * 32; }
inline long long tile_wgs(const RouteShape& p, const Tile& t) {
    return (long long)p.B * ((p.H + tile_th(t) - 1) / tile_th(t)) * ((p.W + 15) / 16) * ((p.Cout + tile_bn(t) - 1) / tile_bn(t));
}
// the first tile of a ladder (largest first) that still gives min_wgs workgroups, else the last
inline Tile ladder(const RouteShape& p, const Tile* t, int n, long long min_wgs) {
    for (int i = 0; i + 1 < n; ++i) if (tile_wgs(p, t[i]) >= min_wgs) return t[i];
    return t[n - 1];
}
inline void set_tile(ConvRoute& r, const RouteShape& p, const Tile& t, bool xcd_fold) {
    r.MT = t.MT; r.NT = t.NT; r.WM = t.WM; r.WN = t.WN;
    const long long tiles = (long long)p.B * ((p.H + tile_th(t) - 1) / tile_th(t)) * ((p.W + 15) / 16), nblk = (p.Cout + tile_bn(t) - 1) / tile_bn(t);
    r.grid_x = (int)tiles; r.grid_y = (int)nblk; r.xcd_map = 0;
    // workgroup -> (tile, N-block) mapping that keeps neighbouring tiles and the N-blocks of a tile on one XCD: a flat grid of a multiple of 8 workgroups
    if (xcd_fold && (tiles * nblk) % 8 == 0) { r.xcd_map = 1; r.grid_x = (int)(tiles * nblk); r.grid_y = 1; }
}
inline size_t mfma_epilogue_floats(const Tile& t) { return 4 * 32 * 36 + (size_t)t.WM * tile_bn(t) * 2; }      // 4 per-wave transpose tiles + statistics scratch

inline ConvRoute mfma16(const RouteShape& p, int stride, int up, int terms) {
    ConvRoute r; r.family = ConvFamily::MFMA16; r.terms = terms == 1 ? 1 : 3; r.gnb = p.gnb; r.csv_code = 0;
    if (p.gn_C > 1024 || (p.gn_C > 0 && !p.coef)) { r.refused = "conv_mfma16 parks at most 4 x 256 GroupNorm channels and needs their coefficients"; return r; }
    bool all_1tap = true, all32 = true;
    for (int i = 0; i < p.nseg; ++i) {
        all_1tap &= p.seg[i].taps == 1 && p.seg[i].C % 64 == 0;    // 64-channel chunks need whole chunks: the packed weights end at C/16 slices
        all32 &= p.seg[i].C % 32 == 0;       // 32-channel chunks wherever every segment has whole ones (at the 32-channel level: whole 128-B pixel rows, -30 % HBM reads)
    }
    if (all_1tap && stride == 1 && !up) { r.S = 1; r.UP = 0; r.KC = 64; }
    else if (stride == 2) { r.S = 2; r.UP = 0; r.KC = 16; }
    else if (up == 2) { r.S = 1; r.UP = 2; r.KC = 16; }
    else { r.S = 1; r.UP = up ? 1 : 0; r.KC = all32 ? 32 : 16; }
    if (p.gnb && !(r.S == 1 && r.UP == 0)) { r.refused = "the GroupNorm-backward epilogue exists at stride 1 without upsampling only"; return r; }
    // >= 2 workgroups per CU; >= 4 for the pure 1x1 launches (KC = 64): four short chunks per workgroup are a latency chain (load - stage - barrier -
    // MFMA), which more, smaller workgroups overlap better - proj_out of the 128^2 nets' attention blocks at U-Net batch 160 (16^2 x 256 -> 256): 53.9 ->
    // 44.7 us on the 4 x 16-pixel tile (r6, same-box A/B with the threshold at 512 / 1024 / 2048 / 4096: C2 11.39 -> 11.46 images/s, C5 unchanged)
    const long long MIN_WGS = r.KC == 64 ? 1024 : 512;
    static constexpr Tile s1_32 = {2, 1, 4, 1};                                                  // 16x16 px x 32
    static constexpr Tile s1_64[] = {{4, 1, 2, 2}, {2, 1, 2, 2}, {1, 1, 2, 2}};                  // 16x16 px x 64, 8x16 px x 64, 4x16 px x 64
    static constexpr Tile s1_128[] = {{4, 1, 1, 4}, {2, 1, 1, 4}, {1, 1, 2, 2}};                 // 8x16 px x 128, 4x16 px x 128, 4x16 px x 64
    static constexpr Tile s2_32 = {1, 1, 4, 1}, s2_64 = {2, 1, 2, 2}, s2_128 = {1, 1, 2, 2};
    const Tile t = r.S == 1 ? (p.Cout <= 32 ? s1_32 : p.Cout <= 64 ? ladder(p, s1_64, 3, MIN_WGS) : ladder(p, s1_128, 3, MIN_WGS))
                            : (p.Cout <= 32 ? s2_32 : p.Cout <= 64 ? s2_64 : s2_128);
    set_tile(r, p, t, true);
    const int ROW = (r.terms == 3 ? r.KC : r.KC / 2) + 4, HALO = r.KC == 64 ? 0 : 1;
    const int PH = (tile_th(t) - 1) * r.S + 1 + 2 * HALO, PW = 15 * r.S + 1 + 2 * HALO, RS = ((PW * ROW + 63) / 64) * 64;
    const size_t patch = (size_t)PH * RS, epi = mfma_epilogue_floats(t);
    r.lds_bytes = ((patch > epi ? patch : epi) + 2 * (size_t)((p.gn_C + 3) & ~3)) * 4;
    return r;
}

inline ConvRoute mfma32(const RouteShape& p, int stride, int up, int terms) {
    ConvRoute r; r.family = ConvFamily::MFMA32; r.terms = terms; r.csv_code = 0;
    if (p.gnb) { r.refused = "the GroupNorm-backward epilogue exists on conv_mfma16 only"; return r; }
    bool generic = false;
    for (int i = 0; i < p.nseg; ++i) generic |= p.seg[i].w_mode != 0;
    if (generic) {
        for (int i = 0; i < p.nseg; ++i) if (p.seg[i].w_mode == 0) { r.refused = "packed and generic weight operands in one launch"; return r; }
        if (stride != 1 || up) { r.refused = "generic weight operands at stride 1 without upsampling only"; return r; }
    }
    bool all_1tap = true;
    // 64-channel chunks: the generic operand clamps its k index, the packed weights end at C/16 slices and need whole chunks
    for (int i = 0; i < p.nseg; ++i) all_1tap &= p.seg[i].taps == 1 && (generic ? p.seg[i].C >= 64 : p.seg[i].C % 64 == 0);
    r.BM = generic ? 1 : 0;
    if (all_1tap && stride == 1 && !up) { r.S = 1; r.UP = 0; r.KC = 64; }
    else if (generic) { r.S = 1; r.UP = 0; r.KC = 16; }
    else if (stride == 2) { r.S = 2; r.UP = 0; r.KC = 16; }
    else { r.S = 1; r.UP = up == 2 ? 2 : up ? 1 : 0; r.KC = 16; }
    constexpr long long MIN_WGS = 512;   // >= 2 workgroups per CU (a constant: finer tiles measured 12 % slower per unit of work, round 3)
    static constexpr Tile s1_32 = {2, 1, 4, 1};                                                  // 16x16 px x 32
    static constexpr Tile s1_64[] = {{2, 2, 4, 1}, {1, 2, 4, 1}, {1, 1, 2, 2}};                  // 16x16 px x 64, 8x16 px x 64, 4x16 px x 64
    static constexpr Tile s1_128[] = {{2, 2, 2, 2}, {1, 2, 2, 2}, {1, 2, 4, 1}, {1, 1, 2, 2}};   // 8x16 px x 128, 4x16 px x 128, 8x16 px x 64, 4x16 px x 64
    static constexpr Tile s2_32 = {1, 1, 4, 1}, s2_64 = {1, 2, 4, 1}, s2_128 = {1, 1, 2, 2};    // 8x16 px x 32, 8x16 px x 64, 4x16 px x 64
    const Tile t = r.S == 1 ? (p.Cout <= 32 ? s1_32 : p.Cout <= 64 ? ladder(p, s1_64, 3, MIN_WGS) : ladder(p, s1_128, 4, MIN_WGS))
                            : (p.Cout <= 32 ? s2_32 : p.Cout <= 64 ? s2_64 : s2_128);
    set_tile(r, p, t, false);
    const size_t patch = (size_t)((tile_th(t) - 1) * r.S + 3) * (15 * r.S + 3) * (r.KC + 4), epi = mfma_epilogue_floats(t);
    r.lds_bytes = ((patch > epi ? patch : epi) + 2 * (size_t)((p.gn_C + 3) & ~3)) * sizeof(float);
    return r;
}

}  // namespace route_detail

// what push_conv_up_phase asks before it builds the phase images: the nearest-x2 upsampling conv described by p (one raw segment) can run in
// conv_dma's phase form
inline bool conv_route_phase_ok(const RouteShape& p, int terms, const RouteEnv& env) { return route_detail::dma_phase_shape_ok(p, terms, env); }

// The decision.  terms: the kernels' TERMS of the plan's precision mode (0 exact fp32, 3 split-fp16, 1 single fp16 product); stride 1 / 2;
// up 0 / 1 (nearest x2 read through the source index) / 2 (phase form).  Total: every input gets a fully initialised answer.
inline ConvRoute conv_route(const RouteShape& p, int stride, int up, int terms, const RouteEnv& env) {
    namespace d = route_detail;
    if (terms != 1 && terms != 3) return d::mfma32(p, stride, up, 0);
    ConvRoute r; r.terms = terms;
    if (d::sp_ok(p, stride, up, terms, env)) {
        r.family = ConvFamily::SP; r.csv_code = 5;
        r.MT = p.Cout == 64 ? 4 : 2; r.NT = p.Cout == 64 ? 2 : 4; r.nsplit = p.Cout == 256 ? 2 : 1; r.res = p.residual;
        for (int i = 0; i < p.nseg; ++i) r.n9 += p.seg[i].C / 16;
        r.grid_x = env.cu_grid; r.lds_bytes = (size_t)sp_lds(r.MT, r.NT, terms);
        return r;
    }
    if (d::pp_ok(p, stride, up, terms, env, r.n9, r.n1)) {
        r.family = ConvFamily::PP; r.csv_code = 2;
        r.MT = PP_MT; r.res = p.residual; r.teams = pp_teams(r.n9, r.n1, terms);
        r.grid_x = env.cu_grid * (r.teams == 1 ? 2 : 1); r.lds_bytes = pp_lds(r.n9, r.n1, r.teams, terms);
        return r;
    }
    r.n9 = r.n1 = 0;
    if (d::dma_ok(p, stride, up, terms, env)) {
        r.family = ConvFamily::DMA; r.csv_code = 1;
        r.MT = 4; r.NT = 1; r.WM = 1; r.WN = 4; r.UP = up; r.KC = terms == 3 ? 32 : 64;
        const long long tiles = up == 2 ? (long long)p.B * (p.Hs / DMA_TH) * (p.Ws / 16) : (long long)p.B * (p.H / DMA_TH) * (p.W / 16);
        const long long nblk = (up == 2 ? 4 * p.Cout : p.Cout) / DMA_BN;
        r.grid_x = (int)tiles; r.grid_y = (int)nblk;
        if ((tiles * nblk) % 8 == 0) { r.xcd_map = 1; r.grid_x = (int)(tiles * nblk); r.grid_y = 1; }
        r.lds_bytes = dma_lds();
        return r;
    }
    return d::packed16(p) ? d::mfma16(p, stride, up, terms) : d::mfma32(p, stride, up, terms);
}

}  // namespace pf
