// Host-only weight packers: pure functions from an OIHW fp32 conv weight to the byte image a kernel reads.  Plain C++17 (clang: _Float16),
// no HIP, no engine state - engine.hip uploads what these return, tests/test_weight_pack.py checks every image against its formula below.
//
// Notation: w(o, i, tap) = OIHW element, tap = ky * K + kx, kk = K * K taps.  Every image is zero where its formula names no element
// (ragged K tails, unused MFMA rows / columns).  "hi" / "lo" are the two halves of split16: the fp16 images carry w x 2^8 (the kernels'
// epilogues multiply by 2^-8), and the TERMS = 3 kernels multiply hi and lo, the TERMS = 1 kernels (precision mode 2) hi alone.
#pragma once
#include <cstddef>
#include <vector>

namespace wpack {

using half_t = _Float16;
constexpr int KC = 16;      // channels per K-chunk / 16-channel slice (pf_common.h: CONV_KC)

struct Oihw {
    const float* w; int O, I, kk;
    float operator()(int o, int i, int tap) const { return w[((size_t)o * I + i) * kk + tap]; }
};

// The one place the 2^8 pre-scale and the hi / lo split are written: hi = RNE16(256 w), lo = RNE16(256 w - hi).
struct Split { half_t hi, lo; half_t part(int p) const { return p ? lo : hi; } };
inline Split split16(float w) { w *= 256.0f; const half_t hi = (half_t)w; return {hi, (half_t)(w - (float)hi)}; }

// MFMA column n of the persistent kernels (conv_pp.hip, conv_sp.hip) carries output channel 4 (n mod 8) + n div 8 of its 32-channel N-tile
// (their epilogue transpose).
inline int col_channel(int n) { return 4 * (n & 7) + (n >> 3); }

// Fragment-major fp32 image of input channels [lo, hi) (conv_mfma.hip): floats
//   img[((((chunk * kk + tap) * 2 + kstep) * O + n) * 8 + j] = w(n, lo + 16 chunk + 8 kstep + j, tap),   chunk < ceil((hi - lo) / 16)
// - the B fragment of one wave (32 output channels x 8 k) is contiguous.
inline std::vector<float> frag32(const Oihw& w, int lo, int hi) {
    const int C = hi - lo, nchunk = (C + KC - 1) / KC;
    std::vector<float> img((size_t)nchunk * w.kk * w.O * KC, 0.f);
    for (int c = 0; c < C; ++c)
        for (int tap = 0; tap < w.kk; ++tap)
            for (int n = 0; n < w.O; ++n)
                img[((((size_t)(c / KC) * w.kk + tap) * 2 + c % KC / 8) * w.O + n) * 8 + c % 8] = w(n, lo + c, tap);
    return img;
}

// 16-channel-slice fp16 image of input channels [lo, hi) (conv_mfma16.hip, conv_dma.hip): halfs, P = 2 parts (hi, lo) at terms 3, P = 1 (hi) at terms 1
//   img[(((chunk * kk + tap) * P + part) * O + n) * 16 + k] = split16(w(n, lo + 16 chunk + k, tap)).part
// - per (slice, tap) all hi halves, then all lo halves: the hi (lo) fragment load of a wave (32 output channels x 32 B) is one contiguous 1 KiB run.
inline std::vector<half_t> slice16(const Oihw& w, int lo, int hi, int terms) {
    const int C = hi - lo, nchunk = (C + KC - 1) / KC, P = terms == 1 ? 1 : 2;
    std::vector<half_t> img((size_t)nchunk * w.kk * P * w.O * KC, (half_t)0.f);
    for (int c = 0; c < C; ++c)
        for (int tap = 0; tap < w.kk; ++tap)
            for (int n = 0; n < w.O; ++n) {
                const Split s = split16(w(n, lo + c, tap));
                for (int part = 0; part < P; ++part)
                    img[((((size_t)(c / KC) * w.kk + tap) * P + part) * w.O + n) * KC + c % KC] = s.part(part);
            }
    return img;
}

// LDS image of ONE 32-channel K-chunk [lo, lo + 32) for conv_pp.hip (O = 32): halfs
//   img[(((((tap * 2 + j) * 2 + part) * 2 + khalf) * 32 + n) * 8 + i] = split16(w(col_channel(n), lo + 16 j + 8 khalf + i, tap)).part
// - one k16-step (tap, j) = 2 KiB: its hi fragments, then its lo fragments.  Requires w.O == 32 and lo + 32 <= w.I (not checked).
inline std::vector<half_t> chunk_pp(const Oihw& w, int lo) {
    std::vector<half_t> img((size_t)w.kk * 2 * 2 * 2 * 32 * 8, (half_t)0.f);
    size_t at = 0;
    for (int tap = 0; tap < w.kk; ++tap)
        for (int j = 0; j < 2; ++j)
            for (int part = 0; part < 2; ++part)
                for (int kh = 0; kh < 2; ++kh)
                    for (int n = 0; n < 32; ++n)
                        for (int i = 0; i < 8; ++i) img[at++] = split16(w(col_channel(n), lo + 16 * j + 8 * kh + i, tap)).part(part);
    return img;
}

// LDS image of ONE 16-channel K-chunk [lo, lo + 16) for conv_sp.hip (O = 32 NT): halfs, P as in slice16
//   img[(((((tap * P + part) * NT + ntile) * 2 + khalf) * 32 + n) * 8 + i] = split16(w(32 ntile + col_channel(n), lo + 8 khalf + i, tap)).part
// - one tap slot = P NT KiB (8 KiB at 128 channels and terms 3).  `row0`: first output row of the image - the N-halves of a 256-channel conv are the
// images of rows [0, 128) and [128, 256), each what the 128-row slice alone would give (w(row0 + 32 ntile + col_channel(n), ...) in the formula).
// Requires row0 + 32 NT <= w.O and lo + 16 <= w.I (not checked).
inline std::vector<half_t> chunk_sp(const Oihw& w, int lo, int NT, int terms, int row0 = 0) {
    const int P = terms == 1 ? 1 : 2;
    std::vector<half_t> img((size_t)w.kk * P * NT * 512, (half_t)0.f);
    size_t at = 0;
    for (int tap = 0; tap < w.kk; ++tap)
        for (int part = 0; part < P; ++part)
            for (int nt = 0; nt < NT; ++nt)
                for (int kh = 0; kh < 2; ++kh)
                    for (int n = 0; n < 32; ++n)
                        for (int i = 0; i < 8; ++i) img[at++] = split16(w(row0 + 32 * nt + col_channel(n), lo + 8 * kh + i, tap)).part(part);
    return img;
}

// B fragments of the image-boundary MFMA kernels (unet_misc.hip; 32 feature channels, 3x3): halfs, lane = 32 half + n
//   img[(((kstep * 2 + part) * 2 + half) * 32 + n) * 8 + j] = split16(element).part
//   begin conv (w: [32][Cimg][3][3]): MFMA k = 16 kstep + 8 half + j = 9 ci + tap,  element = w(n, ci, tap)           for k < 9 Cimg
//   end conv   (w: [Cimg][32][3][3]): channel c = 16 half + 8 kstep + j, column n = Cimg tap + co, element = w(co, c, tap)   for n < 9 Cimg
inline std::vector<half_t> edge_frag(const Oihw& w, bool begin) {
    const int cimg = begin ? w.I : w.O;
    std::vector<half_t> img((size_t)2 * 2 * 64 * 8, (half_t)0.f);
    for (int ks = 0; ks < 2; ++ks) for (int hh = 0; hh < 2; ++hh) for (int n = 0; n < 32; ++n) for (int j = 0; j < 8; ++j) {
        const int k = begin ? 16 * ks + 8 * hh + j : n;
        if (k >= 9 * cimg) continue;
        const Split s = begin ? split16(w(n, k / 9, k % 9)) : split16(w(n % cimg, 16 * hh + 8 * ks + j, n / cimg));
        for (int part = 0; part < 2; ++part) img[((((size_t)ks * 2 + part) * 2 + hh) * 32 + n) * 8 + j] = s.part(part);
    }
    return img;
}

// Host transform: the adjoint conv's OIHW weight over input channels [lo, hi), transposed and spatially flipped: [hi - lo][O][K][K]
//   t(ci, co, tap) = w(co, lo + ci, kk - 1 - tap)
inline std::vector<float> adjoint(const Oihw& w, int lo, int hi) {
    const int C = hi - lo;
    std::vector<float> t((size_t)C * w.O * w.kk);
    for (int ci = 0; ci < C; ++ci) for (int co = 0; co < w.O; ++co) for (int tap = 0; tap < w.kk; ++tap)
        t[((size_t)ci * w.O + co) * w.kk + tap] = w(co, lo + ci, w.kk - 1 - tap);
    return t;
}

// Host transform: phase form of nearest-x2 upsampling followed by a 3x3 conv (w: kk = 9) - output pixel (2 i + dy, 2 j + dx) is a 2 x 2 conv of the
// SOURCE image whose tap (ty, tx) sums the 3x3 weights that read the same source pixel: OIHW [4 O][I][2][2]
//   t((2 dy + dx) O + o, i, 2 ty + tx) = sum of w(o, i, 3 ky + kx) over ky in R(dy, ty), kx in R(dx, tx),
//   R(0, 0) = {0}, R(0, 1) = {1, 2}, R(1, 0) = {0, 1}, R(1, 1) = {2}        (summed in double, rounded once to fp32)
inline std::vector<float> phase_sums(const Oihw& w) {
    static const int R0[2][2] = {{0, 1}, {0, 2}}, R1[2][2] = {{1, 3}, {2, 3}};      // [d][t] -> first / one-past-last 3x3 index
    std::vector<float> t((size_t)4 * w.O * w.I * 4, 0.f);
    for (int dy = 0; dy < 2; ++dy) for (int dx = 0; dx < 2; ++dx)
        for (int o = 0; o < w.O; ++o) for (int i = 0; i < w.I; ++i)
            for (int ty = 0; ty < 2; ++ty) for (int tx = 0; tx < 2; ++tx) {
                double sum = 0.0;
                for (int ky = R0[dy][ty]; ky < R1[dy][ty]; ++ky)
                    for (int kx = R0[dx][tx]; kx < R1[dx][tx]; ++kx) sum += (double)w(o, i, ky * 3 + kx);
                t[(((size_t)(dy * 2 + dx) * w.O + o) * w.I + i) * 4 + ty * 2 + tx] = (float)sum;
            }
    return t;
}

}  // namespace wpack
