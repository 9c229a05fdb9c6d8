// Fourier-domain solve of OT-ODE's linear system for the circular Gaussian blur
// (pnpflow/methods/ot_ode.py:108-117):
//     sol = ifft2( fft2(d) / (r_t^2 |fft2(filter)|^2 + sigma^2) )
// Hand-written line-batched FFT in LDS (no hipFFT): one workgroup transforms LB lines of N complex points,
// radix-2 Stockham autosort when N is a power of two, a direct O(N^2) DFT otherwise (N <= 2048).
// The 2-D transform is rows -> columns; the column kernel applies the spectral division and goes straight
// back (forward FFT, scale, inverse FFT of the same LDS-resident columns), so the solve is 3 launches:
//     rows  forward  (real d = y - H(x1) in, complex spectrum out)
//     cols  forward + divide + inverse (in place)
//     rows  inverse  (complex in, real sol out, 1/(H W) folded in)
// The blur filter is separable (outer(g,g), utils.py:273-280) so |fft2(filter)|^2(u,v) = P_H[u] * P_W[v] with
// P_N[u] = |sum_j g[j] exp(-2 pi i u (j-r)/N)|^2, evaluated in fp64 by a tiny kernel.
#include <algorithm>
#include "pf_common.h"

namespace pf {
namespace {

__device__ inline float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// tw[m] = exp(-2 pi i m / N), m in [0, N)
__device__ inline void fill_twiddles(float2* tw, int N) {
    for (int m = threadIdx.x; m < N; m += blockDim.x) {
        float s, c;
        sincospif(2.0f * (float)m / (float)N, &s, &c);
        tw[m] = make_float2(c, -s);
    }
}

// Transforms LB lines (line l at a[l*N .. l*N+N)) in LDS; returns the buffer that holds the result.
// inverse: conjugated twiddles, no normalisation.
__device__ float2* fft_lines(float2* a, float2* b, const float2* tw, int N, int log2n, int LB, int inverse) {
    const float sgn = inverse ? -1.f : 1.f;
    if (log2n >= 0) {
        const int half = N >> 1;
        for (int s = 0; s < log2n; ++s) {
            const int p = 1 << s;
            const int tstep = half >> s;                         // exp(-i pi k / p) = tw[k * (N/2)/p]
            for (int idx = threadIdx.x; idx < LB * half; idx += blockDim.x) {
                const int l = idx / half, j = idx - l * half;
                const int k = j & (p - 1);
                float2 w = tw[k * tstep]; w.y *= sgn;
                const float2 u0 = a[l * N + j];
                const float2 u1 = cmul(w, a[l * N + j + half]);
                const int o = ((j - k) << 1) + k;
                b[l * N + o] = make_float2(u0.x + u1.x, u0.y + u1.y);
                b[l * N + o + p] = make_float2(u0.x - u1.x, u0.y - u1.y);
            }
            __syncthreads();
            float2* t = a; a = b; b = t;
        }
        return a;
    }
    for (int idx = threadIdx.x; idx < LB * N; idx += blockDim.x) {
        const int l = idx / N, k = idx - l * N;
        float2 acc = make_float2(0.f, 0.f);
        int m = 0;
        for (int n = 0; n < N; ++n) {
            float2 w = tw[m]; w.y *= sgn;
            const float2 v = cmul(w, a[l * N + n]);
            acc.x += v.x; acc.y += v.y;
            m += k; m -= m >= N ? N : 0;
        }
        b[l * N + k] = acc;
    }
    __syncthreads();
    return b;
}

// rows forward: z[plane][row][:] = FFT_W( y - hx )   (hx == nullptr: FFT_W( y ))
__global__ __launch_bounds__(256) void fft_rows_fwd_kernel(const float* y, const float* hx, float2* z, int H, int W, int log2w, int LB) {
    extern __shared__ float2 smem[];
    float2* a = smem; float2* b = a + LB * W; float2* tw = b + LB * W;
    fill_twiddles(tw, W);
    const size_t plane = (size_t)blockIdx.y * H * W;
    const int row0 = blockIdx.x * LB;
    for (int idx = threadIdx.x; idx < LB * W; idx += 256) {
        const int l = idx / W, k = idx - l * W;
        float v = 0.f;
        if (row0 + l < H) { const size_t o = plane + (size_t)(row0 + l) * W + k; v = hx ? y[o] - hx[o] : y[o]; }
        a[idx] = make_float2(v, 0.f);
    }
    __syncthreads();
    const float2* r = fft_lines(a, b, tw, W, log2w, LB, 0);
    for (int idx = threadIdx.x; idx < LB * W; idx += 256) {
        const int l = idx / W, k = idx - l * W;
        if (row0 + l < H) z[plane + (size_t)(row0 + l) * W + k] = r[idx];
    }
}

// columns: forward FFT_H, divide by (rt2 * P_H[u] * P_W[v] + sigma2), inverse FFT_H - in place
// alpha_dev != nullptr: the factor is the device scalar *alpha_dev for every image instead of rt2[image] (Prox-PnP's hqs deblurring prox,
// pnp_gs.py:42: alpha |fft2 filter|^2 + 1 with sigma2 = 1)
// pw2 != nullptr: a point-spread function's spectrum does not factor; it is the table pw2[H][W] (psf_power_spectrum_kernel)
__global__ __launch_bounds__(256) void fft_cols_solve_kernel(float2* z, const float* pw_h, const float* pw_w, const float* pw2, const float* rt2, const double* alpha_dev,
                                                             float sigma2, int C, int H, int W, int log2h, int LB) {
    extern __shared__ float2 smem[];
    float2* a = smem; float2* b = a + LB * H; float2* tw = b + LB * H;
    fill_twiddles(tw, H);
    const size_t plane = (size_t)blockIdx.y * H * W;
    const float r2 = alpha_dev ? (float)*alpha_dev : rt2[blockIdx.y / C];
    const int col0 = blockIdx.x * LB;
    for (int idx = threadIdx.x; idx < LB * H; idx += 256) {
        const int k = idx / LB, l = idx - k * LB;                 // adjacent lanes -> adjacent columns
        a[l * H + k] = col0 + l < W ? z[plane + (size_t)k * W + col0 + l] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    float2* r = fft_lines(a, b, tw, H, log2h, LB, 0);
    float2* o = r == a ? b : a;
    for (int idx = threadIdx.x; idx < LB * H; idx += 256) {
        const int l = idx / H, u = idx - l * H;
        float inv;
        if (pw2) {
            inv = r2 * (col0 + l < W ? pw2[(size_t)u * W + col0 + l] : 0.f) + sigma2;
        } else {
            const float pv = col0 + l < W ? pw_w[col0 + l] : 0.f;
            inv = r2 * (pw_h[u] * pv) + sigma2;                   // ot_ode.py:113-115
        }
        r[idx] = make_float2(r[idx].x / inv, r[idx].y / inv);     // :116
    }
    __syncthreads();
    const float2* q = fft_lines(r, o, tw, H, log2h, LB, 1);
    for (int idx = threadIdx.x; idx < LB * H; idx += 256) {
        const int k = idx / LB, l = idx - k * LB;
        if (col0 + l < W) z[plane + (size_t)k * W + col0 + l] = q[l * H + k];
    }
}

// rows inverse: sol[plane][row][:] = Re( IFFT_W( z ) ) / (H W)
__global__ __launch_bounds__(256) void fft_rows_inv_kernel(const float2* z, float* sol, int H, int W, int log2w, int LB) {
    extern __shared__ float2 smem[];
    float2* a = smem; float2* b = a + LB * W; float2* tw = b + LB * W;
    fill_twiddles(tw, W);
    const size_t plane = (size_t)blockIdx.y * H * W;
    const int row0 = blockIdx.x * LB;
    for (int idx = threadIdx.x; idx < LB * W; idx += 256) {
        const int l = idx / W, k = idx - l * W;
        a[idx] = row0 + l < H ? z[plane + (size_t)(row0 + l) * W + k] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const float2* r = fft_lines(a, b, tw, W, log2w, LB, 1);
    const float norm = 1.0f / ((float)H * (float)W);
    for (int idx = threadIdx.x; idx < LB * W; idx += 256) {
        const int l = idx / W, k = idx - l * W;
        if (row0 + l < H) sol[plane + (size_t)(row0 + l) * W + k] = r[idx].x * norm;
    }
}

// P_N[u] = |DFT_N of the rolled, zero-padded 1-D taps|^2  (degradations.py:62-68: peak rolled to index 0)
__global__ void blur_power_spectrum_kernel(const float* taps, int ntaps, int N, float* pw) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= N) return;
    const int r = ntaps / 2;
    double re = 0.0, im = 0.0;
    for (int j = 0; j < ntaps; ++j) {
        long long m = ((long long)u * (j - r)) % N;               // exp(-2 pi i u (j-r) / N)
        if (m < 0) m += N;
        double s, c;
        sincospi(2.0 * (double)m / (double)N, &s, &c);
        re += (double)taps[j] * c; im -= (double)taps[j] * s;
    }
    pw[u] = (float)(re * re + im * im);
}

// P[u][v] = |DFT_HxW of the rolled, zero-padded K x K taps|^2 for a 2-D point-spread function, in fp64, as two stages: along x into one
// complex value per tap row (the workgroup's column v of the K x W intermediate), then along y into the H values of column v.
// One workgroup per column v; LDS: the H twiddles exp(-2 pi i m / H), then the K intermediate values.
__global__ __launch_bounds__(256) void psf_power_spectrum_kernel(const float* taps, int K, int H, int W, float* pw2) {
    extern __shared__ double2 s_spec[];
    double2* tw = s_spec;
    double2* T = tw + H;
    const int v = blockIdx.x, r = K / 2;
    for (int m = threadIdx.x; m < H; m += 256) {
        double s, c;
        sincospi(2.0 * (double)m / (double)H, &s, &c);
        tw[m] = make_double2(c, -s);
    }
    for (int j = threadIdx.x; j < K; j += 256) {
        double re = 0.0, im = 0.0;
        for (int i = 0; i < K; ++i) {
            long long m = ((long long)v * (i - r)) % W;            // exp(-2 pi i v (i-r) / W)
            if (m < 0) m += W;
            double s, c;
            sincospi(2.0 * (double)m / (double)W, &s, &c);
            re += (double)taps[j * K + i] * c; im -= (double)taps[j * K + i] * s;
        }
        T[j] = make_double2(re, im);
    }
    __syncthreads();
    for (int u = threadIdx.x; u < H; u += 256) {
        long long m0 = (-(long long)u * r) % H;                    // exp(-2 pi i u (j-r) / H), j = 0, then + u per tap row
        int m = (int)(m0 < 0 ? m0 + H : m0);
        double re = 0.0, im = 0.0;
        for (int j = 0; j < K; ++j) {
            const double2 w = tw[m], t = T[j];
            re += t.x * w.x - t.y * w.y; im += t.x * w.y + t.y * w.x;
            m += u; m -= m >= H ? H : 0;
        }
        pw2[(size_t)u * W + v] = (float)(re * re + im * im);
    }
}

// The aliased spectrum of blur-then-decimate.  For circular H = S K (blur with the filter, keep every sf-th sample) the matrix H H^T is circulant on the
// low-resolution grid [Hl][Wl] = [H / sf][W / sf] with the eigenvalues
//     lam[u][v] = 1 / sf^2  sum_{a, b < sf} |fft2(filter)|^2 [u + a Hl][v + b Wl]
// summed in fp64 from the 2-D table of psf_power_spectrum_kernel (pw2 != nullptr: DEG_PSF_SR) or from the separable factors (DEG_SR_FILTER: the sum of the
// products is the product of the two folded factors fold_h[Hl], fold_w[Wl] of blur_fold_spectrum_kernel, kept in fp64 so that lam is rounded once).
__global__ void blur_fold_spectrum_kernel(const float* taps, int ntaps, int N, int sf, double* fold) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x, Nl = N / sf;
    if (u >= Nl) return;
    const int r = ntaps / 2;
    double acc = 0.0;
    for (int a = 0; a < sf; ++a) {                                 // P_N[u + a Nl], the expression of blur_power_spectrum_kernel
        const int uu = u + a * Nl;
        double re = 0.0, im = 0.0;
        for (int j = 0; j < ntaps; ++j) {
            long long m = ((long long)uu * (j - r)) % N;
            if (m < 0) m += N;
            double s, c;
            sincospi(2.0 * (double)m / (double)N, &s, &c);
            re += (double)taps[j] * c; im -= (double)taps[j] * s;
        }
        acc += re * re + im * im;
    }
    fold[u] = acc;
}

__global__ __launch_bounds__(256) void sr_fold_spectrum_kernel(const float* pw2, const double* fold_h, const double* fold_w, int sf, int Hl, int Wl, float* lam) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Hl * Wl) return;
    const int u = i / Wl, v = i - u * Wl, W = Wl * sf;
    double acc;
    if (pw2) {
        acc = 0.0;
        for (int a = 0; a < sf; ++a)
            for (int b = 0; b < sf; ++b) acc += (double)pw2[(size_t)(u + a * Hl) * W + v + b * Wl];
    } else {
        acc = fold_h[u] * fold_w[v];
    }
    lam[i] = (float)(acc / ((double)sf * (double)sf));
}

// coef[b] <- (float)*alpha_dev, b < B: the device scalar as the per-image coefficient of the operator kernels' mode-2 epilogue
__global__ void alpha_to_coef_kernel(const double* alpha_dev, float* coef, int B) {
    for (int b = threadIdx.x; b < B; b += blockDim.x) coef[b] = (float)*alpha_dev;
}

// out = a - (float)*alpha_dev * t
__global__ __launch_bounds__(256) void sub_scaled_kernel(const float* a, const float* t, const double* alpha_dev, float* out, int64_t total) {
    const float al = (float)*alpha_dev;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) out[i] = a[i] - al * t[i];
}

__global__ __launch_bounds__(256) void x1_hat_kernel(const float* x, const float* vt, const float* omt, float* out, int n, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
        out[i] = x[i] + omt[i / n] * vt[i];                       // ot_ode.py:74
}

inline int ilog2_exact(int n) { int l = 0; while ((1 << l) < n) ++l; return (1 << l) == n ? l : -1; }
inline int lines_per_wg(int N) { int lb = 2048 / N; return lb > 8 ? 8 : (lb < 1 ? 1 : lb); }

// sol = real( ifft2( fft2(y - hx) / (r2 P + sigma2) ) ) on an [Hh][Ww] grid, the three launches every Fourier solve here is made of (hx == nullptr: fft2(y));
// P = pw2[u][v] when the 2-D table is given, pw_h[u] pw_w[v] otherwise; r2 = *alpha_dev when given, rt2[image] otherwise
hipError_t fourier_solve(const float* y, const float* hx, float2* z, const float* pw_h, const float* pw_w, const float* pw2, const float* rt2,
                         const double* alpha_dev, float sigma2, float* sol, int B, int C, int Hh, int Ww, hipStream_t s) {
    const int lbw = lines_per_wg(Ww), lbh = lines_per_wg(Hh);
    const size_t lds_w = (size_t)(2 * lbw + 1) * Ww * sizeof(float2), lds_h = (size_t)(2 * lbh + 1) * Hh * sizeof(float2);
    hipLaunchKernelGGL(fft_rows_fwd_kernel, dim3((Hh + lbw - 1) / lbw, B * C), dim3(256), lds_w, s, y, hx, z, Hh, Ww, ilog2_exact(Ww), lbw);
    hipLaunchKernelGGL(fft_cols_solve_kernel, dim3((Ww + lbh - 1) / lbh, B * C), dim3(256), lds_h, s, z, pw_h, pw_w, pw2, rt2, alpha_dev, sigma2, C, Hh, Ww,
                       ilog2_exact(Hh), lbh);
    hipLaunchKernelGGL(fft_rows_inv_kernel, dim3((Hh + lbw - 1) / lbw, B * C), dim3(256), lds_w, s, (const float2*)z, sol, Hh, Ww, ilog2_exact(Ww), lbw);
    return hipGetLastError();
}

// The scratch of the blur-then-decimate solves (its size and layout: sr_solve_scratch_floats, deg_rules.h), S = B C H W, Sl = S / sf^2
struct SrScratch {
    float *buf0, *opscr, *hx, *lam; float2* z;
    SrScratch(float* scratch, size_t S, size_t Sl) {
        buf0 = scratch; opscr = scratch + S; hx = scratch + 3 * S;
        z = reinterpret_cast<float2*>(((uintptr_t)(hx + Sl) + 7) & ~(uintptr_t)7);      // (3 S + Sl floats is an odd count for an even sf and an odd Sl)
        lam = reinterpret_cast<float*>(z) + 2 * Sl;
    }
};

}  // namespace

float* sr_solve_lam(float* scratch, int B, int C, int H, int W, int sf) {
    const size_t S = (size_t)B * C * H * W;
    return SrScratch(scratch, S, S / ((size_t)sf * sf)).lam;
}

// lam[H / sf][W / sf] of DEG_PSF_SR / DEG_SR_FILTER (sr_fold_spectrum_kernel); tmp: H*W floats (DEG_PSF_SR: the full-resolution table) or 2 (H + W) + 2 floats
// (DEG_SR_FILTER: the two folded factors as doubles, at the first 8-byte boundary)
hipError_t launch_sr_aliased_spectrum(const DegView& d, int H, int W, float* lam, float* tmp, hipStream_t s) {
    if (!lam || !tmp || H < 1 || W < 1 || !sr_solve_shape_ok(d, H, W)) return hipErrorInvalidValue;
    const int Hl = H / d.sf, Wl = W / d.sf;
    if (d.kind == DEG_PSF_SR) {
        hipLaunchKernelGGL(psf_power_spectrum_kernel, dim3(W), dim3(256), (size_t)(H + d.ntaps) * sizeof(double2), s, d.taps, d.ntaps, H, W, tmp);
        hipLaunchKernelGGL(sr_fold_spectrum_kernel, dim3((Hl * Wl + 255) / 256), dim3(256), 0, s, (const float*)tmp, (const double*)nullptr, (const double*)nullptr, d.sf,
                           Hl, Wl, lam);
    } else {
        double* fold = reinterpret_cast<double*>(((uintptr_t)tmp + 7) & ~(uintptr_t)7);
        hipLaunchKernelGGL(blur_fold_spectrum_kernel, dim3((Hl + 63) / 64), dim3(64), 0, s, d.taps, d.ntaps, H, d.sf, fold);
        hipLaunchKernelGGL(blur_fold_spectrum_kernel, dim3((Wl + 63) / 64), dim3(64), 0, s, d.taps, d.ntaps, W, d.sf, fold + Hl);
        hipLaunchKernelGGL(sr_fold_spectrum_kernel, dim3((Hl * Wl + 255) / 256), dim3(256), 0, s, (const float*)nullptr, (const double*)fold, (const double*)(fold + Hl),
                           d.sf, Hl, Wl, lam);
    }
    return hipGetLastError();
}

// The blur-then-decimate kinds (DEG_PSF_SR, DEG_SR_FILTER): H H^T is circulant on the low-resolution grid with the eigenvalues lam, so
//     vec = H_adj( ifft2_l( fft2_l( y - H(x + (1-t) v_t) ) / (r_t^2 lam + sigma^2) ) )
// scratch: SrScratch
static hipError_t ot_ode_vec_sr(const DegView& d, const float* x, const float* vt, const float* y, const float* one_minus_t, const float* rt2, float sigma2, float* vec,
                                int B, int C, int H, int W, float* scratch, hipStream_t s, bool spectrum_ready) {
    if (!sr_solve_shape_ok(d, H, W)) return hipErrorInvalidValue;
    const int Hl = H / d.sf, Wl = W / d.sf;
    const size_t S = (size_t)B * C * H * W, Sl = (size_t)B * C * Hl * Wl;
    const SrScratch m(scratch, S, Sl);
    hipError_t r = spectrum_ready ? hipSuccess : launch_sr_aliased_spectrum(d, H, W, m.lam, m.lam + (size_t)Hl * Wl, s);
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(x1_hat_kernel, dim3((unsigned)std::min<size_t>((S + 255) / 256, 4096)), dim3(256), 0, s, x, vt, one_minus_t, m.buf0, C * H * W, (int64_t)S);
    r = launch_deg_H(d, m.buf0, m.hx, B, C, H, W, m.opscr, s);                                        // hx = H(x1_hat), low resolution
    if (r != hipSuccess) return r;
    r = fourier_solve(y, m.hx, m.z, nullptr, nullptr, m.lam, rt2, nullptr, sigma2, m.hx, B, C, Hl, Wl, s);      // hx <- sol (the rows-forward launch has consumed it)
    if (r != hipSuccess) return r;
    return launch_deg_Hadj(d, m.hx, vec, B, C, H, W, m.opscr, s);
}

// The exact proximal map of the Gaussian data term a/2 |H x - y|^2 for the blur-then-decimate kinds, by the Woodbury identity on the low-resolution grid:
//     prox(z) = r - alpha H_adj( ifft2_l( fft2_l(H r) / (alpha lam + 1) ) ),  r = z + alpha H_adj(y)        (r is the caller's `in`)
// lam: launch_sr_aliased_spectrum; scratch: 3 S + 3 Sl + 1 + B floats (SrScratch with the B coefficients in lam's place); in != out
hipError_t launch_fft_prox_sr(const DegView& d, const float* in, const double* alpha_dev, const float* lam, float* out, int B, int C, int H, int W, float* scratch,
                              hipStream_t s) {
    if (!in || !alpha_dev || !lam || !out || in == out || !scratch || !sr_solve_shape_ok(d, H, W)) return hipErrorInvalidValue;
    const int Hl = H / d.sf, Wl = W / d.sf;
    const size_t S = (size_t)B * C * H * W, Sl = (size_t)B * C * Hl * Wl;
    const SrScratch m(scratch, S, Sl);
    float* coef = m.lam;
    hipLaunchKernelGGL(alpha_to_coef_kernel, dim3(1), dim3(64), 0, s, alpha_dev, coef, B);
    hipError_t r = launch_deg_H(d, in, m.hx, B, C, H, W, m.opscr, s);
    if (r != hipSuccess) return r;
    r = fourier_solve(m.hx, nullptr, m.z, nullptr, nullptr, lam, nullptr, alpha_dev, 1.0f, m.hx, B, C, Hl, Wl, s);
    if (r != hipSuccess) return r;
    if (d.kind == DEG_PSF_SR) return launch_psf_sr(d, m.hx, out, B, C, H, W, -1, 2, in, coef, s);     // out = in - alpha H_adj(sol) in the adjoint's epilogue
    r = launch_deg_Hadj(d, m.hx, scratch, B, C, H, W, m.opscr, s);
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(sub_scaled_kernel, dim3((unsigned)std::min<size_t>((S + 255) / 256, 4096)), dim3(256), 0, s, in, (const float*)scratch, alpha_dev, out, (int64_t)S);
    return hipGetLastError();
}

// vec = H_adj( sol ),  sol = ifft2( fft2( y - H(x + (1-t) v_t) ) / (r_t^2 |fft2 filter|^2 + sigma^2) )
// scratch: 4*B*C*H*W + H + W floats; DEG_PSF_BLUR: 4*B*C*H*W + H*W (the 2-D spectrum table, filled here unless spectrum_ready)
hipError_t launch_ot_ode_vec_blur(const DegView& d, const float* x, const float* vt, const float* y, const float* one_minus_t,
                                  const float* rt2, float sigma2, float* vec, int B, int C, int H, int W, float* scratch, hipStream_t s, bool spectrum_ready) {
    const DegSolve solve = deg_solve(d.kind);
    if (!scratch || solve == DegSolve::ClosedForm || solve == DegSolve::Krylov || deg_solve_violation(d, H, W)) return hipErrorInvalidValue;
    if (solve == DegSolve::FourierLowRes) return ot_ode_vec_sr(d, x, vt, y, one_minus_t, rt2, sigma2, vec, B, C, H, W, scratch, s, spectrum_ready);
    const bool psf = solve == DegSolve::FourierPsf;
    const size_t S = (size_t)B * C * H * W;
    float* buf0 = scratch; float* buf1 = scratch + S; float2* z = reinterpret_cast<float2*>(scratch + 2 * S);
    float* pw_h = scratch + 4 * S; float* pw_w = pw_h + H;
    const float* pw2 = psf ? pw_h : nullptr;
    if (psf) {
        if (!spectrum_ready) { hipError_t e = launch_psf_power_spectrum(d, H, W, pw_h, s); if (e != hipSuccess) return e; }
    } else {
        hipLaunchKernelGGL(blur_power_spectrum_kernel, dim3((H + 63) / 64), dim3(64), 0, s, d.taps, d.ntaps, H, pw_h);
        hipLaunchKernelGGL(blur_power_spectrum_kernel, dim3((W + 63) / 64), dim3(64), 0, s, d.taps, d.ntaps, W, pw_w);
    }
    hipLaunchKernelGGL(x1_hat_kernel, dim3((unsigned)std::min<size_t>((S + 255) / 256, 4096)), dim3(256), 0, s, x, vt, one_minus_t, buf0,
                       C * H * W, (int64_t)S);
    hipError_t r = launch_deg_H(d, buf0, buf1, B, C, H, W, reinterpret_cast<float*>(z), s);          // buf1 = H(x1_hat)
    if (r != hipSuccess) return r;
    r = fourier_solve(y, buf1, z, pw_h, pw_w, pw2, rt2, nullptr, sigma2, buf0, B, C, H, W, s);
    if (r != hipSuccess) return r;
    return launch_deg_Hadj(d, buf0, vec, B, C, H, W, buf1, s);                                        // vec = H_adj(sol), ot_ode.py:130
}

hipError_t launch_psf_power_spectrum(const DegView& d, int H, int W, float* pw2, hipStream_t s) {
    if ((d.kind != DEG_PSF_BLUR && d.kind != DEG_PSF_SR) || !pw2 || H < 1 || W < 1 || H > 2048 || W > 2048 || !psf_taps_ok(d, H, W)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(psf_power_spectrum_kernel, dim3(W), dim3(256), (size_t)(H + d.ntaps) * sizeof(double2), s, d.taps, d.ntaps, H, W, pw2);
    return hipGetLastError();
}

hipError_t launch_blur_power_spectrum(const DegView& d, int H, int W, float* pw_h, float* pw_w, hipStream_t s) {
    if (deg_solve(d.kind) != DegSolve::FourierSeparable || deg_solve_violation(d, H, W)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(blur_power_spectrum_kernel, dim3((H + 63) / 64), dim3(64), 0, s, d.taps, d.ntaps, H, pw_h);
    hipLaunchKernelGGL(blur_power_spectrum_kernel, dim3((W + 63) / 64), dim3(64), 0, s, d.taps, d.ntaps, W, pw_w);
    return hipGetLastError();
}

// Prox-PnP's Fourier-domain prox of the Gaussian data term for the circular blur (pnp_gs.py:36-44):
//     out = real( ifft2( fft2(in) / (alpha |fft2 filter|^2 + 1) ) ),  in = alpha H_adj(y) + y'
// the same three launches as the OT-ODE solve; alpha is read on the device.  cplx: 2*B*C*H*W floats
hipError_t launch_fft_prox_blur(const float* in, const double* alpha_dev, const float* pw_h, const float* pw_w, float* out, int B, int C, int H, int W,
                                float* cplx, hipStream_t s, const float* pw2) {
    if (!in || !alpha_dev || (!pw2 && (!pw_h || !pw_w)) || !out || !cplx || H > 2048 || W > 2048) return hipErrorInvalidValue;
    return fourier_solve(in, nullptr, reinterpret_cast<float2*>(cplx), pw_h, pw_w, pw2, nullptr, alpha_dev, 1.0f, out, B, C, H, W, s);
}

}  // namespace pf
