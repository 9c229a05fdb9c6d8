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

bool psf_taps_ok(const DegView& d, int H, int W) {
    if (!d.taps || d.ntaps < 1 || d.ntaps > PSF_MAX_SIDE || !(d.ntaps & 1)) return false;
    return d.kind == DEG_PSF_BLUR_ZERO || (d.kind == DEG_PSF_BLUR && d.ntaps <= std::min(H, W));      // the circular filter must hold the kernel
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
