// Implicit-GEMM convolution on the gfx950 16-bit matrix cores with fp32-equivalent accuracy.
//
// Same GEMM view, fusion and epilogue as conv_mfma.hip, but the contraction runs on
// v_mfma_f32_32x32x16_f16 (16x the rate of the fp32 MFMA) with every operand carried as an
// unevaluated fp16 pair  a = a_hi + a_lo,  w = w_hi + w_lo  and the product expanded into three
// MFMAs  a_lo*w_hi + a_hi*w_lo + a_hi*w_hi  accumulated in fp32 (the dropped a_lo*w_lo term is
// 2^-22 relative).  fp16 products are exact in fp32, so the result matches the fp32-MFMA kernel to
// fp32-rounding level (same parity tolerances in tests/), at 3/16 of its matrix-pipe time.
//   * activations: split after GroupNorm/SiLU while staging; LDS row of a pixel =
//     [KC hi halfs | KC lo halfs | pad] = KC+4 dwords (the same conflict-free stride as the fp32 patch);
//   * weights: split on the host after an exact 2^8 pre-scale (keeps w_lo a normal fp16 number; the
//     epilogue multiplies by 2^-8), packed [k16-step][hi | lo][Cout][16] so that each B fragment load of a
//     wave (32 channels x 16 k, hi and lo) are one contiguous 2 KiB run, and read straight from L1/L2
//     into a register ring two steps ahead of their use (as in conv_mfma.hip).  At this MFMA rate the
//     weight stream is 16/3 x denser per matrix-pipe cycle than in the fp32 kernel, so the tile shapes
//     give every wave 4 (or 2) M-tiles per N-tile: one B fragment pair feeds 12 (6) MFMAs.
#include "pp_common.h"

namespace pf {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// v_exp_f32 / v_rcp_f32 (1 ulp each); __frcp_rn would be a correctly rounded division: 10 instructions per element
__device__ __forceinline__ float silu_fast16(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

// waves per SIMD the register allocation is bounded for: 3 on the tiles whose accumulators stay in VGPRs for the per-segment rescale
constexpr int conv16_lb(int MT, int WM, int KC) { return ((MT == 4 && WM == 2 && KC == 16) || (KC != 64 && ((MT == 4 && WM == 1) || (MT == 2 && WM == 4)))) ? 3 : 1; }

// TERMS = 3: every product as a_lo*w_hi + a_hi*w_lo + a_hi*w_hi (fp32-equivalent).  TERMS = 1: a_hi*w_hi only - operands rounded to
// fp16 (11-bit significands, the power-of-two operand scales keep them in range), fp32 accumulate: the precision class of the
// TF32 convolutions the reference's own CUDA runs use by PyTorch default; one third of the matrix-pipe work, no low halves staged.
template <int MT, int NT, int WM, int WN, int S, int UP, int KC, bool GNB = false, int TERMS = 3>
__global__ __launch_bounds__(256, conv16_lb(MT, WM, KC)) void conv_mfma16_kernel(const ConvParams p) {
    constexpr int ROW = (TERMS == 3 ? KC : KC / 2) + 4;   // dwords per LDS row: KC/2 (hi) + KC/2 (lo; not in the one-term mode) + 4 (pad); always 4 x odd
    constexpr int KQ = KC / 4, KH = KC / 2, KS = KC / 16;
    constexpr int TH = 2 * MT * WM, TW = 16;
    constexpr int HALO = KC == 64 ? 0 : 1;      // KC = 64 is instantiated for pure 1x1 launches only: their patch has no halo
    constexpr int PH = (TH - 1) * S + 1 + 2 * HALO, PW = (TW - 1) * S + 1 + 2 * HALO, PP = PH * PW;
    // dwords per patch row, padded to a multiple of 64: ds_read_b128 is serviced in the lane groups {0-3,12-15,20-27}, {4-11,16-19,
    // 28-31}, ... (MI355X_MICROARCH.md, LDS), i.e. 8 pixels of one tile row + 8 of the next per LDS cycle.  With the pixel pitch ROW
    // = 4 * odd the 16 pixels of ONE row land on 16 different 16-B bank slots; a row pitch that is not 0 mod 64 dwords shifts the
    // second row's slots onto the first's (PW * ROW = 648: 2-way conflicts on half of the A-fragment reads, SQ_LDS_BANK_CONFLICT =
    // 48 % of SQ_LDS_IDX_ACTIVE, profiles/r02_pmc_sq_*).
    constexpr int RS = ((PW * ROW + 63) / 64) * 64;
    constexpr int BN = WN * NT * 32;
    constexpr int A_F4 = PP * KQ, A_PER = (A_F4 + 255) / 256;
    static_assert(WM * WN == 4, "4 waves per workgroup");

    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    uint32_t* s_patch = reinterpret_cast<uint32_t*>(smem_raw);   // [PH][RS]: pixel (py, px) at py * RS + px * ROW
    constexpr int EPI = 4 * 32 * 36 + WM * BN * 2;           // floats needed by the epilogue (see below)
    float* s_sc = reinterpret_cast<float*>(s_patch + (PH * RS > EPI ? PH * RS : EPI));
    float* s_sh = s_sc + ((p.gn_C + 3) & ~3);

    const int tiles_x = (p.W + TW - 1) / TW, tiles_y = (p.H + TH - 1) / TH;
    // Workgroups are dispatched round-robin over the 8 XCDs (each with its own L2).  With the XCD-aware mapping workgroup L works on
    // item (L % 8) * (total / 8) + L / 8 of the (tile-major, N-block-minor) list: an XCD walks a contiguous band of tiles - halo
    // rows / columns and the second N-block of a tile are L2 hits instead of another trip to the memory side.
    int bid, nb;
    if (p.xcd_map) {
        const int NBk = gridDim.y == 1 ? (p.Cout + BN - 1) / BN : 1;
        const int total = gridDim.x;
        const int work = (blockIdx.x & 7) * (total >> 3) + (blockIdx.x >> 3);
        bid = work / NBk; nb = work % NBk;
    } else {
        bid = blockIdx.x; nb = blockIdx.y;
    }
    const int tx = bid % tiles_x; bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW, n0 = nb * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hi = lane >> 5, l31 = lane & 31;
    const int wm = wave % WM, wn = wave / WM;
    const int Hv = UP ? 2 * p.Hs : p.Hs, Wv = UP ? 2 * p.Ws : p.Ws;
    const int qi = tid % KQ, q4 = qi * 4;
    // power-of-two operand scales of this image, one per K-segment (1 unless the operands are far from O(1)): see ConvParams::scale
    float seg_scale[3], seg_inv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { seg_scale[i] = p.scale != nullptr ? p.scale[8 * b + i] : 1.0f; seg_inv[i] = p.scale != nullptr ? p.scale[8 * b + 4 + i] : 1.0f; }

    int a_pix[A_PER];                            // source pixel of staged float4 number tid + i*256 (-1: zero); its LDS slot is recomputed when used
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
        const int idx = tid + i * 256;
        a_pix[i] = -1;
        if (idx < A_F4) {
            const int pix = idx / KQ;
            const int py = pix / PW, px = pix % PW;
            const int gy = oy0 * S - HALO + py, gx = ox0 * S - HALO + px;
            if (gy >= 0 && gy < Hv && gx >= 0 && gx < Wv && !(UP == 2 && ((gy | gx) & 1))) {
                const int sy = UP ? (gy >> 1) : gy, sx = UP ? (gx >> 1) : gx;
                a_pix[i] = (b * p.Hs + sy) * (p.src_row_pitch > 0 ? p.src_row_pitch : p.Ws) + sx;
            }
        }
    }

    float4 ra[A_PER];
    auto prefetch = [&](int si, int ch) {
        const ConvSeg& sg = p.seg[si];
        const int c = min(ch * KC + q4, sg.C - 4);
        const float* base = sg.src + sg.coff + c;
#pragma unroll
        for (int i = 0; i < A_PER; ++i) ra[i] = *reinterpret_cast<const float4*>(base + (size_t)max(a_pix[i], 0) * sg.cstride);
    };
    auto store_lds = [&](int si, int ch) {
        const ConvSeg& sg = p.seg[si];
        const int c = ch * KC + q4;
        const bool cok = c < sg.C;
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (sg.xform != 0 && cok) {
            sc = *reinterpret_cast<const float4*>(s_sc + sg.gn_off + c);
            sh = *reinterpret_cast<const float4*>(s_sh + sg.gn_off + c);
        }
        const float a_scale = si == 0 ? seg_scale[0] : (si == 1 ? seg_scale[1] : seg_scale[2]);
#pragma unroll
        for (int i = 0; i < A_PER; ++i) {
            if (tid + i * 256 < A_F4) {
                const int a_p = (tid + i * 256) / KQ;
                const int a_lds = (a_p / PW) * RS + (a_p % PW) * ROW + qi * 2;      // dword offset of this thread's 4 hi halfs (lo at +KH)
                float4 v = ra[i];
                if (sg.xform != 0) {
                    v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y;
                    v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                    if (sg.xform == 2) {
                        v.x = silu_fast16(v.x); v.y = silu_fast16(v.y); v.z = silu_fast16(v.z); v.w = silu_fast16(v.w);
                    }
                }
                v.x *= a_scale; v.y *= a_scale; v.z *= a_scale; v.w *= a_scale;
                if (!(cok && a_pix[i] >= 0)) v = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (TERMS == 3) {
                    // hi = RNE16(v), lo = RNE16(v - hi) in six instructions (pp_common.h: hipcc's translation of the C++ expression takes 13;
                    // bit-identical, and no measurable difference on this kernel: 49.7 vs 49.6 ms per forward, r4); the asm also
                    // keeps the hi that is stored and the hi that is subtracted the SAME rounding of the SAME fp32 value
                    uint2 h, l;
                    split4_pp(v, h.x, h.y, l.x, l.y);
                    *reinterpret_cast<uint2*>(s_patch + a_lds) = h;
                    *reinterpret_cast<uint2*>(s_patch + a_lds + KH) = l;
                } else {
                    f16x4 h;
                    h[0] = (_Float16)v.x; h[1] = (_Float16)v.y; h[2] = (_Float16)v.z; h[3] = (_Float16)v.w;
                    *reinterpret_cast<f16x4*>(s_patch + a_lds) = h;
                }
            }
        }
    };

    // GroupNorm coefficients of image b: finalised once per launch by gn_coef_kernel (unet_misc.hip); requested BEFORE the
    // first patch chunk (loads return in order) and parked in LDS behind the patch, where the staging reads them.
    constexpr int GNP = 4;                       // passes of 256 channels: gn_C <= 1024 (checked by the launcher)
    float csc[GNP], csh[GNP];
    {
        const float* cb = p.coef + (size_t)b * 2 * p.coef_stride;
#pragma unroll
        for (int i = 0; i < GNP; ++i) {
            csc[i] = 0.f; csh[i] = 0.f;
            if (i * 256 < p.gn_C) {                                     // uniform: skips whole passes
                const int c = min(tid + i * 256, p.gn_C - 1);
                csc[i] = cb[c]; csh[i] = cb[p.coef_stride + c];
            }
        }
    }
    prefetch(0, 0);
#pragma unroll
    for (int i = 0; i < GNP; ++i) {
        const int c = tid + i * 256;
        if (c < p.gn_C) { s_sc[c] = csc[i]; s_sh[c] = csh[i]; }          // visible to store_lds after the chunk loop's first barrier
    }

    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    const int prow = l31 >> 4, pcol = l31 & 15;
    const int nbase = n0 + wn * NT * 32 + l31;
    int nclamp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) nclamp[nt] = min(nbase + nt * 32, p.Cout - 1);

    // B fragments of step s = tap * KS + j (tap of the 3x3 window, j-th 16-channel slice of the chunk):
    // 8 hi halfs + 8 lo halfs per lane, unconditional loads (clamped channel index)
    auto load_b = [&](const ConvSeg& sg, int ch, int s, uint4 (&dh)[NT], uint4 (&dl)[NT]) {
        const int tap = s / KS, j = s % KS;
        const size_t kidx = ((size_t)ch * KS + j) * sg.taps + tap;     // global 16-channel slice index x taps + tap
        const uint4* wp = reinterpret_cast<const uint4*>(sg.w16) + kidx * ((size_t)p.Cout * 4) + hi;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) { dh[nt] = wp[(size_t)nclamp[nt] * 2]; if constexpr (TERMS == 3) dl[nt] = wp[(size_t)p.Cout * 2 + (size_t)nclamp[nt] * 2]; else dl[nt] = dh[nt]; }
    };

    int si = 0, ch = 0;
    while (true) {
        const ConvSeg& sg = p.seg[si];
        if (ch == 0 && si > 0) {
            // the accumulator changes units: from segment si-1's operand scale to segment si's (both powers of two: exact)
            const float ratio = (si == 1 ? seg_scale[1] * seg_inv[0] : seg_scale[2] * seg_inv[1]);
            if (ratio != 1.0f)
            {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[mt][nt][r] *= ratio;
            }
        }
        __syncthreads();
        store_lds(si, ch);
        __syncthreads();
        int nsi = si, nch = ch + 1;
        if (nch * KC >= sg.C) { nsi = si + 1; nch = 0; }
        const bool more = nsi < p.nseg;

        const int nsteps = sg.taps * KS;      // k16-steps per chunk: 9 / 1 (KC 16), 18 / 2 (KC 32), 4 (KC 64, 1-tap launches)
        uint4 bh0[NT], bl0[NT], bh1[NT], bl1[NT], bh2[NT], bl2[NT];
        load_b(sg, ch, 0, bh0, bl0); load_b(sg, ch, min(1, nsteps - 1), bh1, bl1);
        if (more) prefetch(nsi, nch);

        auto k_step = [&](int s, uint4 (&ch_)[NT], uint4 (&cl_)[NT], uint4 (&nh_)[NT], uint4 (&nl_)[NT]) {
            load_b(sg, ch, min(s + 2, nsteps - 1), nh_, nl_);
            __builtin_amdgcn_sched_barrier(0);
            const int tap = s / KS, j = s % KS;
            // (taps == 4: a 2 x 2 window at (oy, ox) inside the 3 x 3 neighbourhood - the phase forms of the upsampling conv's adjoint)
            const int ky = sg.taps == 9 ? tap / 3 : (sg.taps == 4 ? (tap >> 1) + sg.oy : HALO), kx = sg.taps == 9 ? tap % 3 : (sg.taps == 4 ? (tap & 1) + sg.ox : HALO);
            f16x8 ah[MT], al[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int poff = (((wm * MT + mt) * 2 + prow) * S + ky) * RS + (pcol * S + kx) * ROW;
                ah[mt] = *reinterpret_cast<const f16x8*>(s_patch + poff + j * 8 + hi * 4);
                if constexpr (TERMS == 3) al[mt] = *reinterpret_cast<const f16x8*>(s_patch + poff + KH + j * 8 + hi * 4); else al[mt] = ah[mt];
            }
            // every A fragment of the k-step is requested before its first MFMA (the MFMAs then wait with counted lgkmcnt):
            // left alone hipcc recycles ONE register quad for the four low-half fragments and emits ds_read -> lgkmcnt(0) -> MFMA
            // four times per k-step.  Not on the 8x16x128 tile, where the extra live fragments spill at its 168-register bound.
            if constexpr (!(MT == 4 && WM == 1)) __builtin_amdgcn_sched_barrier(0);
            if constexpr (TERMS == 3) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mt], *reinterpret_cast<const f16x8*>(&ch_[nt]), acc[mt][nt], 0, 0, 0);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], *reinterpret_cast<const f16x8*>(&cl_[nt]), acc[mt][nt], 0, 0, 0);
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], *reinterpret_cast<const f16x8*>(&ch_[nt]), acc[mt][nt], 0, 0, 0);
        };
        __builtin_amdgcn_s_setprio(2);        // waves in their k-loop win instruction arbitration over waves that stage / store (-0.3 %)
        int s = 0;
        for (; s + 3 <= nsteps; s += 3) {
            k_step(s, bh0, bl0, bh2, bl2); k_step(s + 1, bh1, bl1, bh0, bl0); k_step(s + 2, bh2, bl2, bh1, bl1);
        }
        if (nsteps - s >= 1) k_step(s, bh0, bl0, bh2, bl2);
        if (nsteps - s == 2) k_step(s + 1, bh1, bl1, bh0, bl0);
        __builtin_amdgcn_s_setprio(0);
        if (!more) break;
        si = nsi; ch = nch;
    }

    // ---- epilogue ---------------------------------------------------------------------------------
    // The MFMA accumulator layout gives each lane 16 pixels of ONE channel (4-byte accesses, 128-byte
    // runs).  Each 32x32 tile is therefore transposed through a per-wave LDS scratch so that every lane
    // owns 4 consecutive channels of a pixel: residual loads and output stores are 16 B per lane and a
    // wave instruction covers 1 KiB of contiguous NHWC rows.
    __syncthreads();                                   // every wave is done reading the patch
    constexpr int TP = 36;                             // scratch row pitch in floats (32 + 4 pad)
    float* s_tr = reinterpret_cast<float*>(s_patch) + wave * (32 * TP);
    float* s_red = reinterpret_cast<float*>(s_patch) + 4 * 32 * TP;   // [WM][BN][2] behind the 4 scratch tiles
    const float oscale = p.out_scale * (1.0f / 256.0f) * (p.nseg == 1 ? seg_inv[0] : (p.nseg == 2 ? seg_inv[1] : seg_inv[2]));
    const int cq = lane & 7;                           // this lane's channel quad inside a 32-channel tile
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int ncol = n0 + (wn * NT + nt) * 32;     // first channel of this N-tile
        const int n = ncol + l31;
        const float add = (p.addvec != nullptr && n < p.Cout) ? p.addvec[(size_t)b * p.addvec_bs + n] : 0.f;
        const int n4 = ncol + cq * 4;
        const bool nok4 = n4 < p.Cout;
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
        // fused GroupNorm-backward first stage (GNB): per-channel forward coefficients of this lane's 4 channels
        float4 g_mu, g_rs, g_ga, g_be;
        if constexpr (GNB) {
            const int gc = p.gnb_coff + min(n4, p.Cout - 4);
            g_mu = *reinterpret_cast<const float4*>(p.gnb_mu + (size_t)b * p.gnb_Ct + gc);
            g_rs = *reinterpret_cast<const float4*>(p.gnb_rs + (size_t)b * p.gnb_Ct + gc);
            g_ga = *reinterpret_cast<const float4*>(p.gnb_gamma + gc);
            g_be = *reinterpret_cast<const float4*>(p.gnb_beta + gc);
        }
        // Residual values are requested for two M-tiles at a time, before any of their stores: a load issued while
        // stores are outstanding makes the wave wait for every store acknowledgement (one counter for loads and stores),
        // which the former load-add-store sequence per float4 paid 4 x MT times per workgroup.
        constexpr int RG = (MT >= 2 && WN != 4) ? 2 : 1;      // (one at a time where a second set of 16 registers would cost a wave per SIMD)
        float4 rv[RG][4];
        float4 xv[GNB ? RG : 1][4];                            // GNB: the GroupNorm's forward input at the same pixels, requested like the residual
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if constexpr (GNB) {
                if (mt % RG == 0) {
#pragma unroll
                    for (int g = 0; g < RG; ++g)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int px = (lane >> 3) + 8 * i;
                            const int oy = min(oy0 + (wm * MT + mt + g) * 2 + (px >> 4), p.H - 1), ox = min(ox0 + (px & 15), p.W - 1);
                            const size_t pix = ((size_t)b * p.H + oy) * p.W + ox;
                            xv[g][i] = *reinterpret_cast<const float4*>(p.gnb_x + pix * p.gnb_xstride + min(n4, p.Cout - 4));
                        }
                }
            }
            if (mt % RG == 0 && p.residual != nullptr) {
#pragma unroll
                for (int g = 0; g < RG; ++g)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int px = (lane >> 3) + 8 * i;
                        const int oy = min(oy0 + (wm * MT + mt + g) * 2 + (px >> 4), p.H - 1), ox = min(ox0 + (px & 15), p.W - 1);
                        const size_t pix = ((size_t)b * p.H + oy) * (p.dst_row_pitch > 0 ? p.dst_row_pitch : p.W) + ox;
                        rv[g][i] = *reinterpret_cast<const float4*>(p.residual + pix * p.res_cstride + min(n4, p.Cout - 4));
                    }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * hi;
                s_tr[row * TP + l31] = acc[mt][nt][r] * oscale + add;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int px = (lane >> 3) + 8 * i;    // pixel of the 32-pixel M-tile (2 rows x 16 cols)
                const int oy = oy0 + (wm * MT + mt) * 2 + (px >> 4), ox = ox0 + (px & 15);
                float4 v = *reinterpret_cast<const float4*>(s_tr + px * TP + cq * 4);
                if (nok4 && oy < p.H && ox < p.W) {
                    const size_t pix = ((size_t)b * p.H + oy) * (p.dst_row_pitch > 0 ? p.dst_row_pitch : p.W) + ox;
                    if (p.residual != nullptr) {
                        const float rsc = p.res_scale;
                        v.x = fmaf(rv[mt % RG][i].x, rsc, v.x); v.y = fmaf(rv[mt % RG][i].y, rsc, v.y); v.z = fmaf(rv[mt % RG][i].z, rsc, v.z); v.w = fmaf(rv[mt % RG][i].w, rsc, v.w);
                    }
                    if constexpr (GNB) {
                        // dyhat = da * act'(u) * gamma,  u = gamma*yhat + beta,  yhat = (x - mu)*rstd   (same expressions as gn_bwd_pre_kernel)
                        const float4 xx = xv[mt % RG][i];
                        float d[4] = {v.x, v.y, v.z, v.w};
                        const float xs[4] = {xx.x, xx.y, xx.z, xx.w}, mm[4] = {g_mu.x, g_mu.y, g_mu.z, g_mu.w}, rr[4] = {g_rs.x, g_rs.y, g_rs.z, g_rs.w};
                        const float gg[4] = {g_ga.x, g_ga.y, g_ga.z, g_ga.w}, bb[4] = {g_be.x, g_be.y, g_be.z, g_be.w};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float yh = (xs[j] - mm[j]) * rr[j];
                            if (p.gnb_silu) {
                                const float u = yh * gg[j] + bb[j];
                                const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-u));
                                d[j] *= sg * (1.0f + u * (1.0f - sg));
                            }
                            d[j] *= gg[j];
                            s1[j] += d[j]; s2[j] += d[j] * yh;
                        }
                        *reinterpret_cast<float4*>(p.out + pix * p.out_cstride + n4) = make_float4(d[0], d[1], d[2], d[3]);
                    } else {
                    *reinterpret_cast<float4*>(p.out + pix * p.out_cstride + n4) = (p.pack_from_p1 != 0 && n4 >= p.pack_from_p1 - 1) ? pack_hilo4(v) : v;
                    s1[0] += v.x; s1[1] += v.y; s1[2] += v.z; s1[3] += v.w;
                    s2[0] += v.x * v.x; s2[1] += v.y * v.y; s2[2] += v.z * v.z; s2[3] += v.w * v.w;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();            // scratch is rewritten by the next tile
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        if (GNB || p.stats_out != nullptr) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int o = 8; o < 64; o <<= 1) { s1[j] += __shfl_xor(s1[j], o); s2[j] += __shfl_xor(s2[j], o); }
            }
            if (lane < 8) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = (wn * NT + nt) * 32 + cq * 4 + j;
                    s_red[(wm * BN + col) * 2] = s1[j]; s_red[(wm * BN + col) * 2 + 1] = s2[j];
                }
            }
        }
    }
    if (GNB || p.stats_out != nullptr) {
        __syncthreads();
        for (int t = tid; t < BN * 2; t += 256) {
            const int col = t >> 1, which = t & 1;
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < WM; ++w) tot += s_red[(w * BN + col) * 2 + which];
            const int n = n0 + col;
            if (n < p.Cout) {
                if constexpr (GNB) unsafeAtomicAdd(p.gnb_sum + ((size_t)b * p.gnb_Ct + p.gnb_coff + n) * 2 + which, (double)tot);
                else unsafeAtomicAdd(p.stats_out + ((size_t)b * p.Cout + n) * 2 + which, (double)tot);
            }
        }
    }
}

// ---- host side: dispatch of a ConvRoute (conv_route.h decides tile, chunk width, grid and LDS) to its instantiation ---------------------

template <int MT, int NT, int WM, int WN, int S, int UP, int KC, int TERMS, bool GNB>
static hipError_t launch_kernel16(const ConvParams& p, const ConvRoute& r, hipStream_t stream) {
    static unsigned long long attr_set = 0ull;
    auto kern = conv_mfma16_kernel<MT, NT, WM, WN, S, UP, KC, GNB, TERMS>;
    { hipError_t e = set_max_dynamic_lds_once(reinterpret_cast<const void*>(kern), attr_set, ROUTE_LDS_MAX); if (e != hipSuccess) return e; }
    ConvParams pp = p; pp.xcd_map = r.xcd_map;
    hipLaunchKernelGGL(kern, dim3(r.grid_x, r.grid_y), dim3(256), r.lds_bytes, stream, pp);
    return hipGetLastError();
}
template <int MT, int NT, int WM, int WN, int S, int UP, int KC, int TERMS>
static hipError_t launch_cfg16(const ConvParams& p, const ConvRoute& r, hipStream_t stream) {
    if (!r.gnb) return launch_kernel16<MT, NT, WM, WN, S, UP, KC, TERMS, false>(p, r, stream);
    // adjoint conv with the fused GroupNorm-backward first stage: built at stride 1 without upsampling only
    if constexpr (S == 1 && UP == 0) return launch_kernel16<MT, NT, WM, WN, S, UP, KC, TERMS, true>(p, r, stream);
    return hipErrorInvalidValue;
}

// the tiles of conv_route.h's conv_mfma16 ladders, per stride
template <int S, int UP, int KC, int TERMS>
static hipError_t launch_tile16(const ConvParams& p, const ConvRoute& r, hipStream_t stream) {
#define PF_TILE16(mt, nt, wm, wn) if (r.MT == mt && r.NT == nt && r.WM == wm && r.WN == wn) return launch_cfg16<mt, nt, wm, wn, S, UP, KC, TERMS>(p, r, stream)
    if constexpr (S == 1) {
        PF_TILE16(2, 1, 4, 1); PF_TILE16(4, 1, 2, 2); PF_TILE16(2, 1, 2, 2); PF_TILE16(1, 1, 2, 2); PF_TILE16(4, 1, 1, 4); PF_TILE16(2, 1, 1, 4);
    } else {
        PF_TILE16(1, 1, 4, 1); PF_TILE16(2, 1, 2, 2); PF_TILE16(1, 1, 2, 2);
    }
#undef PF_TILE16
    return hipErrorInvalidValue;
}

template <int TERMS>
static hipError_t launch_conv16_t(const ConvParams& p, const ConvRoute& r, hipStream_t stream) {
    const int key = r.S * 1000 + r.UP * 100 + r.KC;
    switch (key) {
        case 1064: return launch_tile16<1, 0, 64, TERMS>(p, r, stream);
        case 2016: return launch_tile16<2, 0, 16, TERMS>(p, r, stream);
        case 1216: return launch_tile16<1, 2, 16, TERMS>(p, r, stream);
        case 1132: return launch_tile16<1, 1, 32, TERMS>(p, r, stream);
        case 1116: return launch_tile16<1, 1, 16, TERMS>(p, r, stream);
        case 1032: return launch_tile16<1, 0, 32, TERMS>(p, r, stream);
        case 1016: return launch_tile16<1, 0, 16, TERMS>(p, r, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_conv16(const ConvParams& p, const ConvRoute& r, hipStream_t stream) {
    if (r.family != ConvFamily::MFMA16) return hipErrorInvalidValue;
    return r.terms == 1 ? launch_conv16_t<1>(p, r, stream) : r.terms == 3 ? launch_conv16_t<3>(p, r, stream) : hipErrorInvalidValue;
}

}  // namespace pf
