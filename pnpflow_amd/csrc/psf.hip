// Blur with an arbitrary square K x K point-spread function (DEG_PSF_BLUR: circular, DEG_PSF_BLUR_ZERO: samples outside the image are 0).
// The reference reaches such an operator through GaussianDeblurring's `.kernel` / `.filter` attributes (pnpflow/degradations.py:55-89):
//   circular ("fft" mode):  H = convolution   y[i] = sum_j k[j] x[i - (j - r)],  H_adj = correlation  y[i] = sum_j k[j] x[i + (j - r)]
//   zero boundary:          H = correlation (F.conv2d, padding 'same'),          H_adj = convolution (the true adjoint)
// with r = K / 2 on both axes.  A PSF does not factor into two 1-D passes, so one launch is one application: K^2 multiply-adds per output.
#include <algorithm>
#include "pf_common.h"

namespace pf {

// A workgroup of 256 threads computes a tile of TS columns x 2 TS rows and stages its (TS + 2r) x (2 TS + 2r) neighbourhood once.  Wrap (true
// modulo: any tile size against any image size) or zero extension is resolved per staged row / column in two small index tables, so the staging
// loop itself is a lookup.  Every thread then owns PSF_NO = 8 consecutive outputs of one tile row and walks the taps in a fixed order (rows
// ascending, columns ascending) with a sliding window: one LDS read per tap feeds eight multiply-adds, one fp32 fmaf chain per output.  The
// correlation out[i] = sum_t g[t] in[i - r + t] slides the window up the staged rows, the convolution out[i] = sum_t g[t] in[i + r - t] (flip)
// down them; the taps are walked in the same ascending order either way.  The tap index does not depend on the lane: the taps are read through
// the scalar cache, not LDS.
//   mode 0: out = v;  1: out = v - aux;  2: out = aux - coef[b] v;  3: out = sgn(v - aux) in {-1, +1}     (as blur2d_fused_kernel)
// No atomics, no scratch tensor: two launches on the same input return the same bits.
constexpr int PSF_NO = 8;
template <int TS, bool ZERO>
__global__ __launch_bounds__(256) void psf2d_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ taps, int K, int H, int W,
                                                   int flip, int mode, const float* __restrict__ aux, const float* __restrict__ coef, int planes_per_image) {
    constexpr int TSY = 2 * TS, NO = PSF_NO;
    static_assert(TS % NO == 0 && TSY * (TS / NO) == 256, "one group of NO outputs per thread");
    extern __shared__ float s_p[];
    const int r = K / 2, PWX = TS + 2 * r, PWY = TSY + 2 * r, PWP = PWX + 1;      // +1: an odd pitch puts the 8 rows x 4 groups of a half-wave on 32 banks
    float* s_in = s_p;                                         // [PWY][PWP]
    int* s_iy = reinterpret_cast<int*>(s_in + PWY * PWP);      // [PWY] source row of staged row py, -1: outside the image (ZERO)
    int* s_ix = s_iy + PWY;                                    // [PWX] source column
    const int tid = threadIdx.x;
    const int plane = blockIdx.z, x0 = blockIdx.x * TS, y0 = blockIdx.y * TSY;
    for (int i = tid; i < PWY + PWX; i += 256) {
        const bool col = i >= PWY;
        const int N = col ? W : H;
        int g = (col ? x0 + i - PWY : y0 + i) - r;
        if (ZERO) g = (g >= 0 && g < N) ? g : -1;
        else { g %= N; g += g < 0 ? N : 0; }
        s_iy[i] = g;                                           // (s_ix follows s_iy)
    }
    __syncthreads();
    const float* src = in + (size_t)plane * H * W;
    for (int i = tid; i < PWY * PWX; i += 256) {
        const int py = i / PWX, px = i - py * PWX;
        const int gy = s_iy[py], gx = s_ix[px];
        s_in[py * PWP + px] = (!ZERO || (gy >= 0 && gx >= 0)) ? src[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    const int b = plane / planes_per_image;
    const int y = tid / (TS / NO), x = (tid - y * (TS / NO)) * NO;
    float a[NO], w[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) a[j] = 0.f;
    if (!flip) {
        // correlation: out[y][x + j] = sum g[ky][kx] in[y + ky][x + j + kx]; the window slides up the staged row
        for (int ky = 0; ky < K; ++ky) {
            const float* row = s_in + (y + ky) * PWP + x;
            const float* g = taps + ky * K;
#pragma unroll
            for (int j = 0; j < NO - 1; ++j) w[j] = row[j];
#pragma unroll 8
            for (int kx = 0; kx < K; ++kx) {
                w[NO - 1] = row[kx + NO - 1];                  // row[K + NO - 2] is the last staged sample of the row at x = TS - NO
                const float gk = g[kx];
#pragma unroll
                for (int j = 0; j < NO; ++j) a[j] = fmaf(gk, w[j], a[j]);
#pragma unroll
                for (int j = 0; j < NO - 1; ++j) w[j] = w[j + 1];
            }
        }
    } else {
        // convolution: out[y][x + j] = sum g[ky][kx] in[y + 2r - ky][x + j + 2r - kx]; the same tap order, the window slides down the row
        for (int ky = 0; ky < K; ++ky) {
            const float* row = s_in + (y + 2 * r - ky) * PWP + x + 2 * r;
            const float* g = taps + ky * K;
#pragma unroll
            for (int j = 1; j < NO; ++j) w[j] = row[j];
#pragma unroll 8
            for (int kx = 0; kx < K; ++kx) {
                w[0] = row[-kx];                               // row[-(K - 1)] is the first staged sample of the row at x = 0
                const float gk = g[kx];
#pragma unroll
                for (int j = 0; j < NO; ++j) a[j] = fmaf(gk, w[j], a[j]);
#pragma unroll
                for (int j = NO - 1; j > 0; --j) w[j] = w[j - 1];
            }
        }
    }
    if (y0 + y >= H) return;
#pragma unroll
    for (int j = 0; j < NO; ++j) {
        if (x0 + x + j >= W) break;
        float v = a[j];
        const size_t o = ((size_t)plane * H + y0 + y) * W + x0 + x + j;
        if (mode == 1) v = v - aux[o];
        else if (mode == 2) v = aux[o] - coef[b] * v;
        else if (mode == 3) v = (v - aux[o]) > 0.f ? 1.f : -1.f;
        out[o] = v;
    }
}

// ---- DEG_PSF_SR: blur with the PSF, then keep every sf-th sample:  H x [i][j] = (k (*) x)[i sf][j sf]  (circular) -------------------------------
// The forward kernel computes the K^2 multiply-adds of the LOW-resolution outputs only.  A workgroup owns a tile of SR_TLX x TLY low-resolution outputs and
// stages their high-resolution neighbourhood, ((TLY - 1) sf + K) rows x ((SR_TLX - 1) sf + K) columns, once, through the same true-modulo index tables as
// psf2d_kernel.  The staged columns are de-interleaved by their phase px % sf: output column x reads staged column x sf + c for the tap offset c = 2r - kx,
// i.e. element x + c / sf of phase plane c % sf - neighbouring outputs read neighbouring words, and the taps of one phase (c = p, p + sf, ...) slide a
// window of SR_NO consecutive outputs along the plane exactly as psf2d_kernel's window slides along a row: one LDS read per tap feeds eight multiply-adds.
// The tap order is fixed (rows ascending; phases ascending; offsets ascending), one fp32 fmaf chain per output, taps through the scalar cache.
constexpr int SR_TLX = 32, SR_NO = 8;
__global__ __launch_bounds__(256) void psf_sr_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ taps, int K, int sf, int H,
                                                        int W, int TLY, int mode, const float* __restrict__ aux, const float* __restrict__ coef,
                                                        int planes_per_image) {
    constexpr int NO = SR_NO, TLX = SR_TLX;
    extern __shared__ float s_p[];
    const int r = K / 2, Hl = H / sf, Wl = W / sf;
    const int PWX = (TLX - 1) * sf + K, PWY = (TLY - 1) * sf + K, QW = TLX + 2 * r / sf, PITCH = (sf * QW) | 1;
    float* s_in = s_p;                                         // [PWY][sf][QW], row pitch PITCH
    int* s_iy = reinterpret_cast<int*>(s_in + PWY * PITCH);    // [PWY] source row of staged row py
    int* s_ix = s_iy + PWY;                                    // [PWX] source column
    const int tid = threadIdx.x;
    const int plane = blockIdx.z, xl0 = blockIdx.x * TLX, yl0 = blockIdx.y * TLY;
    for (int i = tid; i < PWY + PWX; i += 256) {
        const bool col = i >= PWY;
        const int N = col ? W : H;
        int g = (col ? xl0 * sf + i - PWY : yl0 * sf + i) - r;
        g %= N; g += g < 0 ? N : 0;
        s_iy[i] = g;                                           // (s_ix follows s_iy)
    }
    __syncthreads();
    const float* src = in + (size_t)plane * H * W;
    for (int i = tid; i < PWY * PWX; i += 256) {
        const int py = i / PWX, px = i - py * PWX;
        const int q = px / sf;
        s_in[py * PITCH + (px - q * sf) * QW + q] = src[(size_t)s_iy[py] * W + s_ix[px]];
    }
    __syncthreads();
    const int y = tid / (TLX / NO), x = (tid - y * (TLX / NO)) * NO;
    if (y >= TLY || yl0 + y >= Hl) return;
    float a[NO], w[NO];
#pragma unroll
    for (int j = 0; j < NO; ++j) a[j] = 0.f;
    // convolution: out[y][x + j] = sum g[ky][kx] in[y sf + 2r - ky][(x + j) sf + 2r - kx]
    for (int ky = 0; ky < K; ++ky) {
        const float* row = s_in + (y * sf + 2 * r - ky) * PITCH + x;
        const float* g = taps + ky * K + 2 * r;
        for (int p = 0; p < sf && p <= 2 * r; ++p) {
            const float* pl = row + p * QW;
            const int nq = (2 * r - p) / sf + 1;               // offsets c = p + sf q <= 2r, tap column kx = 2r - c
#pragma unroll
            for (int j = 0; j < NO - 1; ++j) w[j] = pl[j];
            for (int q = 0; q < nq; ++q) {
                w[NO - 1] = pl[q + NO - 1];                    // <= element TLX - 1 + (2r - p) / sf of the plane: staged
                const float gk = g[-(p + sf * q)];
#pragma unroll
                for (int j = 0; j < NO; ++j) a[j] = fmaf(gk, w[j], a[j]);
#pragma unroll
                for (int j = 0; j < NO - 1; ++j) w[j] = w[j + 1];
            }
        }
    }
    const int b = plane / planes_per_image;
#pragma unroll
    for (int j = 0; j < NO; ++j) {
        if (xl0 + x + j >= Wl) break;
        float v = a[j];
        const size_t o = ((size_t)plane * Hl + yl0 + y) * Wl + xl0 + x + j;
        if (mode == 1) v = v - aux[o];
        else if (mode == 2) v = aux[o] - coef[b] * v;
        else if (mode == 3) v = (v - aux[o]) > 0.f ? 1.f : -1.f;
        out[o] = v;
    }
}

// The adjoint in its polyphase form: H_adj y [m][n] = sum over the taps (ky, kx) with m + ky - r = 0 and n + kx - r = 0 (mod sf) of
// g[ky][kx] y[(m + ky - r) / sf][(n + kx - r) / sf] - the zero-filled tensor is never formed, and an output sums only the <= ceil(K / sf)^2 taps of its phase
// (m mod sf, n mod sf).  A workgroup owns a high-resolution tile of 16 sf rows x 32 sf columns and stages the low-resolution patch under it (wrap through index
// tables, true modulo on the low-resolution grid).  The outputs of one phase form a 16 x 32 grid on which the phase's taps are a plain correlation of the patch:
// a wave takes one phase at a time (so its taps are uniform: scalar cache), a lane eight consecutive outputs of the phase with the sliding window.
constexpr int SRA_GX = 32, SRA_GY = 16;
__global__ __launch_bounds__(256) void psf_sr_adj_kernel(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ taps, int K, int sf, int H,
                                                        int W, int mode, const float* __restrict__ aux, const float* __restrict__ coef, int planes_per_image) {
    constexpr int NO = SR_NO, GX = SRA_GX, GY = SRA_GY;
    static_assert(GY * (GX / NO) == 64, "one wave per phase");
    extern __shared__ float s_p[];
    const int r = K / 2, Hl = H / sf, Wl = W / sf;
    const int RL = r / sf, RU = (r + sf - 1) / sf;             // low-resolution rows / columns needed before and after the tile's own
    const int PWX = GX + RL + RU, PWY = GY + RL + RU, PWP = PWX | 1;
    float* s_in = s_p;                                         // [PWY][PWP]
    int* s_iy = reinterpret_cast<int*>(s_in + PWY * PWP);
    int* s_ix = s_iy + PWY;
    const int tid = threadIdx.x;
    const int plane = blockIdx.z, xl0 = blockIdx.x * GX, yl0 = blockIdx.y * GY;
    for (int i = tid; i < PWY + PWX; i += 256) {
        const bool col = i >= PWY;
        const int N = col ? Wl : Hl;
        int g = (col ? xl0 + i - PWY : yl0 + i) - RL;
        g %= N; g += g < 0 ? N : 0;
        s_iy[i] = g;
    }
    __syncthreads();
    const float* src = in + (size_t)plane * Hl * Wl;
    for (int i = tid; i < PWY * PWX; i += 256) {
        const int py = i / PWX, px = i - py * PWX;
        s_in[py * PWP + px] = src[(size_t)s_iy[py] * Wl + s_ix[px]];
    }
    __syncthreads();
    const int b = plane / planes_per_image;
    const int wave = tid >> 6, lane = tid & 63;
    const int ay = lane / (GX / NO), ax = (lane - ay * (GX / NO)) * NO;
    for (int ph = wave; ph < sf * sf; ph += 4) {
        const int py = ph / sf, px = ph - py * sf;
        // first tap of the phase and the patch offset it reads: ky0 = (r - py) mod sf, rows ay + oy + a for the taps ky0 + sf a
        int ky0 = (r - py) % sf; ky0 += ky0 < 0 ? sf : 0;
        int kx0 = (r - px) % sf; kx0 += kx0 < 0 ? sf : 0;
        const int ny = ky0 < K ? (K - 1 - ky0) / sf + 1 : 0, nx = kx0 < K ? (K - 1 - kx0) / sf + 1 : 0;
        const int oy = (py + ky0 - r) / sf + RL, ox = (px + kx0 - r) / sf + RL;      // exact divisions; >= 0 after + RL
        float a[NO], w[NO];
#pragma unroll
        for (int j = 0; j < NO; ++j) a[j] = 0.f;
        for (int ta = 0; ta < ny; ++ta) {
            const float* row = s_in + (ay + oy + ta) * PWP + ax + ox;
            const float* g = taps + (ky0 + sf * ta) * K + kx0;
#pragma unroll
            for (int j = 0; j < NO - 1; ++j) w[j] = row[j];
            for (int tb = 0; tb < nx; ++tb) {
                w[NO - 1] = row[tb + NO - 1];                  // column ax + ox + tb + NO - 1 <= GX - 1 + RL + RU of the patch
                const float gk = g[sf * tb];
#pragma unroll
                for (int j = 0; j < NO; ++j) a[j] = fmaf(gk, w[j], a[j]);
#pragma unroll
                for (int j = 0; j < NO - 1; ++j) w[j] = w[j + 1];
            }
        }
        const int m = (yl0 + ay) * sf + py;
        if (m >= H) continue;
#pragma unroll
        for (int j = 0; j < NO; ++j) {
            const int n = (xl0 + ax + j) * sf + px;
            if (n >= W) break;
            float v = a[j];
            const size_t o = ((size_t)plane * H + m) * W + n;
            if (mode == 1) v = v - aux[o];
            else if (mode == 2) v = aux[o] - coef[b] * v;
            else if (mode == 3) v = (v - aux[o]) > 0.f ? 1.f : -1.f;
            out[o] = v;
        }
    }
}

// rows of low-resolution outputs per workgroup of psf_sr_fwd_kernel and the LDS they need: 64 rows (one per thread row) while the staged neighbourhood
// fits 64 KB; a large sf x K product takes up to 160 KB before the tile drops under 16 rows
static size_t psf_sr_fwd_lds(int K, int sf, int TLY) {
    const int PWX = (SR_TLX - 1) * sf + K, PWY = (TLY - 1) * sf + K, QW = SR_TLX + 2 * (K / 2) / sf, PITCH = (sf * QW) | 1;
    return ((size_t)PWY * PITCH + PWY + PWX) * sizeof(float);
}
static int psf_sr_fwd_rows(int K, int sf, int Hl) {
    auto fit = [&](size_t budget) { int t = std::min(256 / (SR_TLX / SR_NO), std::max(Hl, 1)); while (t > 1 && psf_sr_fwd_lds(K, sf, t) > budget) --t; return t; };
    const int t = fit(64 * 1024);
    return (t >= 16 || t >= Hl) ? t : fit(160 * 1024);
}

// one application of DEG_PSF_SR in one launch, no scratch: sign +1 = H ([H][W] -> [H / sf][W / sf]), -1 = H_adj; mode / aux / coef as launch_psf2d, on the
// OUTPUT's grid
hipError_t launch_psf_sr(const DegView& d, const float* in, float* out, int B, int C, int H, int W, int sign, int mode, const float* aux, const float* coef,
                         hipStream_t s) {
    if (!in || !out || in == out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || (int64_t)B * C > 65535 || d.kind != DEG_PSF_SR || !psf_taps_ok(d, H, W)) return hipErrorInvalidValue;
    if ((mode != 0 && !aux) || (mode == 2 && !coef)) return hipErrorInvalidValue;
    const int K = d.ntaps, sf = d.sf, Hl = H / sf, Wl = W / sf;
    if (sign > 0) {
        const int TLY = psf_sr_fwd_rows(K, sf, Hl);
        const size_t lds = psf_sr_fwd_lds(K, sf, TLY);
        if (lds > 160 * 1024) return hipErrorInvalidValue;
        static unsigned long long attr = 0ull;
        if (lds > 64 * 1024) { hipError_t e = set_max_dynamic_lds_once(reinterpret_cast<const void*>(psf_sr_fwd_kernel), attr, 160 * 1024); if (e != hipSuccess) return e; }
        hipLaunchKernelGGL(psf_sr_fwd_kernel, dim3((Wl + SR_TLX - 1) / SR_TLX, (Hl + TLY - 1) / TLY, B * C), dim3(256), lds, s, in, out, d.taps, K, sf, H, W, TLY, mode,
                           aux, coef, C);
    } else {
        const int r = K / 2, RL = r / sf, RU = (r + sf - 1) / sf, PWX = SRA_GX + RL + RU, PWY = SRA_GY + RL + RU;
        const size_t lds = ((size_t)PWY * (PWX | 1) + PWY + PWX) * sizeof(float);        // <= 31 KB at K = 63, sf = 1
        hipLaunchKernelGGL(psf_sr_adj_kernel, dim3((Wl + SRA_GX - 1) / SRA_GX, (Hl + SRA_GY - 1) / SRA_GY, B * C), dim3(256), lds, s, in, out, d.taps, K, sf, H, W, mode,
                           aux, coef, C);
    }
    return hipGetLastError();
}

// one application; sign +1 = H, -1 = H_adj (the zero-boundary kind turns it round, like blur2)
hipError_t launch_psf2d(const DegView& d, const float* in, float* out, int B, int C, int H, int W, int sign, int mode, const float* aux, const float* coef,
                        hipStream_t s) {
    constexpr int TS = 32;
    if (!in || !out || in == out || B <= 0 || C <= 0 || H <= 0 || W <= 0 || (int64_t)B * C > 65535 || !psf_taps_ok(d, H, W)) return hipErrorInvalidValue;
    if ((mode != 0 && !aux) || (mode == 2 && !coef)) return hipErrorInvalidValue;
    const bool zero = d.kind == DEG_PSF_BLUR_ZERO;
    const int flip = (zero ? -sign : sign) > 0;            // the convolution
    const int PWX = TS + 2 * (d.ntaps / 2), PWY = 2 * TS + 2 * (d.ntaps / 2);
    const size_t lds = ((size_t)PWY * (PWX + 1) + PWY + PWX) * sizeof(float);        // <= 48.8 KB at K = 63
    const dim3 grid((W + TS - 1) / TS, (H + 2 * TS - 1) / (2 * TS), B * C);
    if (zero) hipLaunchKernelGGL((psf2d_kernel<TS, true>), grid, dim3(256), lds, s, in, out, d.taps, d.ntaps, H, W, flip, mode, aux, coef, C);
    else hipLaunchKernelGGL((psf2d_kernel<TS, false>), grid, dim3(256), lds, s, in, out, d.taps, d.ntaps, H, W, flip, mode, aux, coef, C);
    return hipGetLastError();
}

}  // namespace pf
