// Glue kernels of Prox-PnP with the gradient-step denoiser (pnpflow/methods/pnp_gs.py, pnpflow/train_denoiser.py:39-57; Hurault et al.):
//   * seed       r = x - N (the VJP's vec), optionally with the partials of sum r^2 for g = 0.5 sum r^2;
//   * combine    one pass over z, N, J^T r that writes the iteration's output form (pgd step, hqs random-inpainting prox, the
//                right-hand side of the hqs deblurring prox) or the plain Dg = (z - N) - J^T r;
//   * backtracking of hqs deblurring: squared distances over the whole batch tensor and the one-thread alpha *= 0.9 decision.
// NCHW fp32 images; every per-image length is a multiple of 4 (float4 lanes).  alpha lives in a device double, so that a decay inside
// a replayed graph needs no host round-trip.  Reductions are deterministic: fp64 per-block partials (a fixed number of blocks per
// tensor, a fixed tree inside the block), summed in index order - no float atomics, so replays of one input give identical bits.
#include <algorithm>
#include "pf_common.h"

namespace pf {

namespace {

constexpr int kThreads = 256;

inline unsigned stream_blocks(int64_t n4) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n4 + kThreads - 1) / kThreads, 2048)); }

// fp64 sum over the 256 threads of a block in a fixed tree order; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    return sh[0];
}

__device__ __forceinline__ float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ double sumsq4(float4 a) { return (double)(a.x * a.x) + (double)(a.y * a.y) + (double)(a.z * a.z) + (double)(a.w * a.w); }

// r = x - N (train_denoiser.py:51: grad_outputs = x - N); partial (or nullptr): per-block sums of r^2 (:54)
__global__ __launch_bounds__(kThreads) void pnpgs_seed4_kernel(const float4* __restrict__ x, const float4* __restrict__ N, float4* __restrict__ r,
                                                               double* __restrict__ partial, int64_t n4) {
    __shared__ double sh[kThreads];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        const float4 d = sub4(x[i], N[i]);
        r[i] = d;
        acc += sumsq4(d);
    }
    if (partial) {
        const double s = block_sum(acc, sh);
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
    }
}

// Dg = (z - N) - JN (train_denoiser.py:52), then per MODE
//   PNPGS_DG          out = Dg
//   PNPGS_PGD         out = z - alpha Dg                                   (pnp_gs.py:220-222)
//   PNPGS_HQS_MASK    Dx = z - Dg;  out = M noisy - M Dx + Dx             (:150-156, prox_datafit :33-34 with H = the mask)
//   PNPGS_HQS_BLUR    Dx = z - Dg;  out = alpha H_adj(noisy) + (0.1 alpha Dx + alpha (1 - 0.1 alpha) z)      (:166-168, prox_datafit :36)
//   PNPGS_HQS_SR      the same with 0.065 for 0.1                                                           (:189-191; the input of launch_fft_prox_sr)
template <int MODE>
__global__ __launch_bounds__(kThreads) void pnpgs_combine4_kernel(const float4* z /* may be `out` */, const float4* __restrict__ N, const float4* __restrict__ JN,
                                                                  const float4* __restrict__ aux, const uchar4* __restrict__ mask,
                                                                  const double* __restrict__ alpha_dev, float4* out, int64_t n4, int64_t img4,
                                                                  int64_t hw4) {
    float a = 0.f, c1 = 0.f, c2 = 0.f;
    if (MODE == PNPGS_PGD || MODE == PNPGS_HQS_BLUR) {
        const double ad = *alpha_dev;
        a = (float)ad; c1 = (float)(0.1 * ad); c2 = (float)(ad * (1.0 - ad * 0.1));
    }
    if (MODE == PNPGS_HQS_SR) {
        const double ad = *alpha_dev;
        a = (float)ad; c1 = (float)(0.065 * ad); c2 = (float)(ad * (1.0 - ad * 0.065));
    }
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        const float4 zz = z[i];
        const float4 dg = sub4(sub4(zz, N[i]), JN[i]);
        float4 o;
        if (MODE == PNPGS_DG) {
            o = dg;
        } else if (MODE == PNPGS_PGD) {
            o = make_float4(zz.x - a * dg.x, zz.y - a * dg.y, zz.z - a * dg.z, zz.w - a * dg.w);
        } else if (MODE == PNPGS_HQS_MASK) {
            const float4 dx = sub4(zz, dg), y = aux[i];
            const uchar4 m = mask[(i / img4) * hw4 + (i % img4) % hw4];
            const float mx = m.x ? 1.f : 0.f, my = m.y ? 1.f : 0.f, mz = m.z ? 1.f : 0.f, mw = m.w ? 1.f : 0.f;
            o = make_float4((mx * y.x - mx * dx.x) + dx.x, (my * y.y - my * dx.y) + dx.y, (mz * y.z - mz * dx.z) + dx.z, (mw * y.w - mw * dx.w) + dx.w);
        } else {
            const float4 dx = sub4(zz, dg), h = aux[i];
            o = make_float4(a * h.x + (c1 * dx.x + c2 * zz.x), a * h.y + (c1 * dx.y + c2 * zz.y), a * h.z + (c1 * dx.z + c2 * zz.z),
                            a * h.w + (c1 * dx.w + c2 * zz.w));
        }
        out[i] = o;
    }
}

// per-block partials of sum (a - b)^2 over the whole tensor; copy_to (or nullptr) <- a in the same pass (the accepted iterate)
__global__ __launch_bounds__(kThreads) void pnpgs_sqdist4_kernel(const float4* __restrict__ a, const float4* b, float4* copy_to /* may be `b` */,
                                                                 double* __restrict__ partial, int64_t n4) {
    __shared__ double sh[kThreads];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        const float4 p = a[i];
        acc += sumsq4(sub4(p, b[i]));
        if (copy_to) copy_to[i] = p;
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// out[0] = scale * sum_j partial[j], j in index order
__global__ void pnpgs_sum_kernel(const double* __restrict__ partial, int nparts, double scale, double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int j = 0; j < nparts; ++j) s += partial[j];
    out[0] = scale * s;
}

// pnp_gs.py:174-178 on one thread: gap = 0.5 |H(x_new) - y|^2 - 0.5 |H(x) - y|^2 (the 0.1 g terms cancel);
// if gap < 0.1 / alpha |x_new - x|^2: alpha *= 0.9.  e_prev carries |H(x) - y|^2 to the next iteration.
__global__ void pnpgs_decide_kernel(const double* __restrict__ p_new, int np_new, const double* __restrict__ p_dx, int np_dx, double* __restrict__ e_prev,
                                    double* __restrict__ alpha_dev, const int* __restrict__ iter, double* __restrict__ log, int max_iter) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double e_new = 0.0, dx = 0.0;
    for (int j = 0; j < np_new; ++j) e_new += p_new[j];
    for (int j = 0; j < np_dx; ++j) dx += p_dx[j];
    const double alpha = *alpha_dev;
    const double gap = 0.5 * e_new - 0.5 * *e_prev, thr = 0.1 / alpha * dx;
    if (gap < thr) *alpha_dev = 0.9 * alpha;
    *e_prev = e_new;
    const int it = *iter;
    if (log && it >= 0 && it < max_iter) { log[2 * it] = gap; log[2 * it + 1] = thr; }
}

}  // namespace

int pnpgs_parts(int64_t n4) { return (int)std::max<int64_t>(1, std::min<int64_t>((n4 + kThreads - 1) / kThreads, PNPGS_MAX_PARTS)); }

hipError_t launch_pnpgs_seed(const float* x, const float* N, float* r, double* partial, int64_t n, hipStream_t s) {
    if (n % 4) return hipErrorInvalidValue;
    const unsigned grid = partial ? (unsigned)pnpgs_parts(n / 4) : stream_blocks(n / 4);
    hipLaunchKernelGGL(pnpgs_seed4_kernel, dim3(grid), dim3(kThreads), 0, s, (const float4*)x, (const float4*)N, (float4*)r, partial, n / 4);
    return hipGetLastError();
}

hipError_t launch_pnpgs_combine(int mode, const float* z, const float* N, const float* JN, const float* aux, const uint8_t* mask, const double* alpha_dev,
                                float* out, int B, int64_t n, int64_t hw, hipStream_t s) {
    if (n % 4 || B <= 0) return hipErrorInvalidValue;
    if (mode == PNPGS_HQS_MASK && (hw % 4 || n % hw || !mask || !aux)) return hipErrorInvalidValue;
    if ((mode == PNPGS_HQS_BLUR || mode == PNPGS_HQS_SR) && !aux) return hipErrorInvalidValue;
    if ((mode == PNPGS_PGD || mode == PNPGS_HQS_BLUR || mode == PNPGS_HQS_SR) && !alpha_dev) return hipErrorInvalidValue;
    const int64_t n4 = (int64_t)B * n / 4, img4 = n / 4, hw4 = std::max<int64_t>(hw / 4, 1);
    const dim3 grid(stream_blocks(n4)), block(kThreads);
#define PNPGS_COMBINE(M) hipLaunchKernelGGL(pnpgs_combine4_kernel<M>, grid, block, 0, s, (const float4*)z, (const float4*)N, (const float4*)JN, \
                                            (const float4*)aux, (const uchar4*)mask, alpha_dev, (float4*)out, n4, img4, hw4)
    switch (mode) {
        case PNPGS_DG: PNPGS_COMBINE(PNPGS_DG); break;
        case PNPGS_PGD: PNPGS_COMBINE(PNPGS_PGD); break;
        case PNPGS_HQS_MASK: PNPGS_COMBINE(PNPGS_HQS_MASK); break;
        case PNPGS_HQS_BLUR: PNPGS_COMBINE(PNPGS_HQS_BLUR); break;
        case PNPGS_HQS_SR: PNPGS_COMBINE(PNPGS_HQS_SR); break;
        default: return hipErrorInvalidValue;
    }
#undef PNPGS_COMBINE
    return hipGetLastError();
}

hipError_t launch_pnpgs_sqdist(const float* a, const float* b, float* copy_to, double* partial, int64_t n, hipStream_t s) {
    if (n % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pnpgs_sqdist4_kernel, dim3(pnpgs_parts(n / 4)), dim3(kThreads), 0, s, (const float4*)a, (const float4*)b, (float4*)copy_to, partial, n / 4);
    return hipGetLastError();
}

hipError_t launch_pnpgs_sum(const double* partial, int nparts, double scale, double* out, hipStream_t s) {
    hipLaunchKernelGGL(pnpgs_sum_kernel, dim3(1), dim3(64), 0, s, partial, nparts, scale, out);
    return hipGetLastError();
}

hipError_t launch_pnpgs_decide(const double* p_new, int np_new, const double* p_dx, int np_dx, double* e_prev, double* alpha_dev, const int* iter, double* log,
                               int max_iter, hipStream_t s) {
    hipLaunchKernelGGL(pnpgs_decide_kernel, dim3(1), dim3(64), 0, s, p_new, np_new, p_dx, np_dx, e_prev, alpha_dev, iter, log, max_iter);
    return hipGetLastError();
}

}  // namespace pf
