// Glue kernels of Flow-Priors (pnpflow/methods/flow_priors.py; Zhang et al., "Flow priors for linear inverse problems via iterative
// corrupted trajectory matching"): per inner step of the method
//   * residual / seed   x_next = x + pred dt (two roundings), y_next = (t + dt) y + (1 - (t + dt)) H(x_init), r = H(x_next) - y_next and the
//                       VJP's vec w = H_adj(2 lmbda r) (gaussian) or H_adj(lmbda sign r) (laplace): one pass for the per-pixel operators
//                       (identity, box / byte mask), the measurement-sized half between H and H_adj otherwise;
//   * probe shift       x + h eps and x - h eps in one pass;
//   * gradient + Adam   g = (w + dt J(x)^T w) + (dt / 2h) (J(x + h eps)^T eps - J(x - h eps)^T eps) + (x | grad_xt_lik), and the Adam update of
//                       x, m, v (adam_step.h) in the same pass; the three parts of g are written out when asked for.
// Flat fp32 tensors of any length and alignment: the body runs on float4 lanes when every pointer is 16-byte aligned (a scalar loop takes
// the n % 4 tail), on scalars otherwise.  The per-iteration scalars are kernel arguments; nothing reads back to the host.
#include <algorithm>
#include "pf_common.h"
#include "adam_step.h"

// Every sum and product below is rounded on its own, as torch evaluates the reference's expressions op by op.  HIP's default contracts a * b + c
// into an fma, and its __fmul_rn / __fadd_rn are plain operators that contract as well, so contraction is switched off for this file; the one
// fma of the method (Adam's lerp) is written as fmaf.
#pragma clang fp contract(off)

namespace pf {

namespace {

constexpr int kThreads = 256;

inline unsigned stream_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 2048)); }

inline bool aligned16(std::initializer_list<const void*> ps) {
    uintptr_t a = 0;
    for (const void* p : ps) a |= (uintptr_t)p;
    return (a & 15) == 0;
}

struct V4 { float v[4]; };
__device__ __forceinline__ V4 ld4(const float* p, int64_t q) { const float4 a = reinterpret_cast<const float4*>(p)[q]; return V4{{a.x, a.y, a.z, a.w}}; }
__device__ __forceinline__ void st4(float* p, int64_t q, const V4& a) { reinterpret_cast<float4*>(p)[q] = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]); }

// a + c*b with separate fp32 multiply and add (the reference's `x + pred * dt`: the product first, then the sum, never an fma)
__device__ __forceinline__ float axpy_rn(float a, float c, float b) { const float p = c * b; return a + p; }

// 1 = the pixel is kept by the operator (degradations.py:23-44; the box of utils.py:327-336 is centred on H/2 along both axes)
__device__ __forceinline__ float keep_at(const DegView& d, int64_t i, int64_t n, int H, int W) {
    if (d.kind == DEG_DENOISE) return 1.f;
    const int64_t b = i / n, r = i % n;
    const int px = (int)(r % W), py = (int)((r / W) % H);
    if (d.kind == DEG_BOX) {
        const int c = H / 2;
        return (py >= c - d.half && py < c + d.half && px >= c - d.half && px < c + d.half) ? 0.f : 1.f;
    }
    return d.mask[((size_t)b * H + py) * W + px] ? 1.f : 0.f;
}

// seed of the data term from the residual r: 2 lmbda r (gaussian: coef = 2 lmbda) or lmbda sign(r) (laplace: coef = lmbda; torch's abs has gradient 0 at 0)
__device__ __forceinline__ float data_seed(float r, float coef, int laplace) {
    if (laplace) return r > 0.f ? coef : (r < 0.f ? -coef : 0.f);
    return coef * r;
}
// y_next = tn y + omt H(x_init), the two products rounded before the sum (torch evaluates the expression op by op)
__device__ __forceinline__ float y_next(float y, float hxi, float tn, float omt) { const float p = tn * y, q = omt * hxi; return p + q; }

// second half for the operators that are not per-pixel: seed = data_seed(hx - y_next), over the measurement
__global__ __launch_bounds__(kThreads) void fp_seed_kernel(const float* __restrict__ hx, const float* __restrict__ y, const float* __restrict__ hxi,
                                                           float* __restrict__ seed, float tn, float omt, float coef, int laplace, int64_t n, int64_t n4) {
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t q = tid; q < n4; q += stride) {
        const V4 a = ld4(hx, q), b = ld4(y, q), c = ld4(hxi, q);
        V4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.v[j] = data_seed(a.v[j] - y_next(b.v[j], c.v[j], tn, omt), coef, laplace);
        st4(seed, q, o);
    }
    for (int64_t i = n4 * 4 + tid; i < n; i += stride) seed[i] = data_seed(hx[i] - y_next(y[i], hxi[i], tn, omt), coef, laplace);
}

// per-pixel operators in one pass: w = m data_seed(m (x + pred dt) - y_next)
__global__ __launch_bounds__(kThreads) void fp_residual_kernel(DegView d, const float* __restrict__ x, const float* __restrict__ pred, const float* __restrict__ y,
                                                               const float* __restrict__ hxi, float* __restrict__ w, float dt, float tn, float omt, float coef,
                                                               int laplace, int64_t n_img, int H, int W, int64_t n, int64_t n4) {
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t q = tid; q < n4; q += stride) {
        const V4 a = ld4(x, q), p = ld4(pred, q), b = ld4(y, q), c = ld4(hxi, q);
        V4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float m = keep_at(d, q * 4 + j, n_img, H, W);
            o.v[j] = m * data_seed(m * axpy_rn(a.v[j], dt, p.v[j]) - y_next(b.v[j], c.v[j], tn, omt), coef, laplace);
        }
        st4(w, q, o);
    }
    for (int64_t i = n4 * 4 + tid; i < n; i += stride) {
        const float m = keep_at(d, i, n_img, H, W);
        w[i] = m * data_seed(m * axpy_rn(x[i], dt, pred[i]) - y_next(y[i], hxi[i], tn, omt), coef, laplace);
    }
}

// out = a + c b, the product rounded before the sum: x_next of the two-halves path and the Euler update x + pred dt (out may be a)
__global__ __launch_bounds__(kThreads) void fp_axpy_kernel(const float* a, const float* __restrict__ b, float* out, float c, int64_t n, int64_t n4) {
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t q = tid; q < n4; q += stride) {
        const V4 x = ld4(a, q), y = ld4(b, q);
        V4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.v[j] = axpy_rn(x.v[j], c, y.v[j]);
        st4(out, q, o);
    }
    for (int64_t i = n4 * 4 + tid; i < n; i += stride) out[i] = axpy_rn(a[i], c, b[i]);
}

// xp = x + h eps, xm = x - h eps
__global__ __launch_bounds__(kThreads) void fp_shift_kernel(const float* __restrict__ x, const float* __restrict__ eps, float* __restrict__ xp,
                                                            float* __restrict__ xm, float h, int64_t n, int64_t n4) {
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t q = tid; q < n4; q += stride) {
        const V4 a = ld4(x, q), e = ld4(eps, q);
        V4 p, m;
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float s = h * e.v[j]; p.v[j] = a.v[j] + s; m.v[j] = a.v[j] - s; }
        st4(xp, q, p); st4(xm, q, m);
    }
    for (int64_t i = n4 * 4 + tid; i < n; i += stride) { const float s = h * eps[i]; xp[i] = x[i] + s; xm[i] = x[i] - s; }
}

struct GradOut { float* g; float* g_data; float* g_trace; float* g_extra; };

// one element of the gradient: (w + dt jw) + fd (jp - jm) + (first ? x : lik (num_t pred - x)),  fd = dt / (2 h), lik = -1 / (1 - num_t)
__device__ __forceinline__ float fp_grad_elem(const FlowPriorsCoef& c, float w, float jw, float jp, float jm, float x, float pred, float& gd, float& gt, float& ge) {
    gd = w + c.dt * jw;
    gt = c.fd * (jp - jm);
    ge = c.first ? x : c.lik * (-x + c.num_t * pred);
    return (gd + gt) + ge;
}

template <bool UPDATE>
__global__ __launch_bounds__(kThreads) void fp_grad_adam_kernel(FlowPriorsCoef c, AdamCoef ac, const float* __restrict__ w, const float* __restrict__ jw,
                                                                const float* __restrict__ jp, const float* __restrict__ jm, const float* __restrict__ pred,
                                                                float* x, float* __restrict__ m, float* __restrict__ v, GradOut out, int64_t n, int64_t n4) {
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t q = tid; q < n4; q += stride) {
        const V4 a = ld4(w, q), b = ld4(jw, q), p = ld4(jp, q), mm = ld4(jm, q), pr = ld4(pred, q);
        V4 xx = ld4(x, q), g, gd, gt, ge;
#pragma unroll
        for (int j = 0; j < 4; ++j) g.v[j] = fp_grad_elem(c, a.v[j], b.v[j], p.v[j], mm.v[j], xx.v[j], pr.v[j], gd.v[j], gt.v[j], ge.v[j]);
        if (out.g) st4(out.g, q, g);
        if (out.g_data) st4(out.g_data, q, gd);
        if (out.g_trace) st4(out.g_trace, q, gt);
        if (out.g_extra) st4(out.g_extra, q, ge);
        if (UPDATE) {
            V4 am = ld4(m, q), av = ld4(v, q);
#pragma unroll
            for (int j = 0; j < 4; ++j) adam_step(xx.v[j], am.v[j], av.v[j], g.v[j], ac);
            st4(x, q, xx); st4(m, q, am); st4(v, q, av);
        }
    }
    for (int64_t i = n4 * 4 + tid; i < n; i += stride) {
        float gd, gt, ge, xi = x[i];
        const float g = fp_grad_elem(c, w[i], jw[i], jp[i], jm[i], xi, pred[i], gd, gt, ge);
        if (out.g) out.g[i] = g;
        if (out.g_data) out.g_data[i] = gd;
        if (out.g_trace) out.g_trace[i] = gt;
        if (out.g_extra) out.g_extra[i] = ge;
        if (UPDATE) {
            float mi = m[i], vi = v[i];
            adam_step(xi, mi, vi, g, ac);
            x[i] = xi; m[i] = mi; v[i] = vi;
        }
    }
}

// the bare optimiser step on a given gradient (pf_adam_step)
__global__ __launch_bounds__(kThreads) void adam_kernel(AdamCoef ac, float* __restrict__ x, float* __restrict__ m, float* __restrict__ v,
                                                        const float* __restrict__ g, int64_t n, int64_t n4) {
    const int64_t tid = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t q = tid; q < n4; q += stride) {
        V4 xx = ld4(x, q), am = ld4(m, q), av = ld4(v, q);
        const V4 gg = ld4(g, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) adam_step(xx.v[j], am.v[j], av.v[j], gg.v[j], ac);
        st4(x, q, xx); st4(m, q, am); st4(v, q, av);
    }
    for (int64_t i = n4 * 4 + tid; i < n; i += stride) {
        float xi = x[i], mi = m[i], vi = v[i];
        adam_step(xi, mi, vi, g[i], ac);
        x[i] = xi; m[i] = mi; v[i] = vi;
    }
}

}  // namespace

hipError_t launch_fp_seed(const float* hx, const float* y, const float* hxi, float* seed, float tn, float omt, float coef, int laplace, int64_t n, hipStream_t s) {
    if (n <= 0) return hipErrorInvalidValue;
    const int64_t n4 = aligned16({hx, y, hxi, seed}) ? n / 4 : 0;
    hipLaunchKernelGGL(fp_seed_kernel, dim3(stream_blocks(std::max<int64_t>(n4, n - 4 * n4))), dim3(kThreads), 0, s, hx, y, hxi, seed, tn, omt, coef, laplace, n, n4);
    return hipGetLastError();
}

hipError_t launch_fp_residual(const DegView& d, const float* x, const float* pred, const float* y, const float* hxi, float* w, float dt, float tn, float omt,
                              float coef, int laplace, int B, int C, int H, int W, hipStream_t s) {
    if (d.kind != DEG_DENOISE && d.kind != DEG_BOX && d.kind != DEG_MASK) return hipErrorInvalidValue;
    if (d.kind == DEG_MASK && !d.mask) return hipErrorInvalidValue;
    const int64_t n_img = (int64_t)C * H * W, n = (int64_t)B * n_img;
    if (n <= 0) return hipErrorInvalidValue;
    const int64_t n4 = aligned16({x, pred, y, hxi, w}) ? n / 4 : 0;
    hipLaunchKernelGGL(fp_residual_kernel, dim3(stream_blocks(std::max<int64_t>(n4, n - 4 * n4))), dim3(kThreads), 0, s, d, x, pred, y, hxi, w, dt, tn, omt, coef,
                       laplace, n_img, H, W, n, n4);
    return hipGetLastError();
}

hipError_t launch_fp_axpy(const float* a, const float* b, float* out, float c, int64_t n, hipStream_t s) {
    if (n <= 0) return hipErrorInvalidValue;
    const int64_t n4 = aligned16({a, b, out}) ? n / 4 : 0;
    hipLaunchKernelGGL(fp_axpy_kernel, dim3(stream_blocks(std::max<int64_t>(n4, n - 4 * n4))), dim3(kThreads), 0, s, a, b, out, c, n, n4);
    return hipGetLastError();
}

hipError_t launch_fp_shift(const float* x, const float* eps, float* xp, float* xm, float h, int64_t n, hipStream_t s) {
    if (n <= 0) return hipErrorInvalidValue;
    const int64_t n4 = aligned16({x, eps, xp, xm}) ? n / 4 : 0;
    hipLaunchKernelGGL(fp_shift_kernel, dim3(stream_blocks(std::max<int64_t>(n4, n - 4 * n4))), dim3(kThreads), 0, s, x, eps, xp, xm, h, n, n4);
    return hipGetLastError();
}

hipError_t launch_fp_grad_adam(const FlowPriorsCoef& c, const AdamCoef* adam, const float* w, const float* jw, const float* jp, const float* jm, const float* pred,
                               float* x, float* m, float* v, float* out_g, float* out_g_data, float* out_g_trace, float* out_g_extra, int64_t n, hipStream_t s) {
    if (n <= 0 || (adam && (!m || !v))) return hipErrorInvalidValue;
    const int64_t n4 = aligned16({w, jw, jp, jm, pred, x, m, v, out_g, out_g_data, out_g_trace, out_g_extra}) ? n / 4 : 0;
    const dim3 grid(stream_blocks(std::max<int64_t>(n4, n - 4 * n4)));
    const GradOut out{out_g, out_g_data, out_g_trace, out_g_extra};
    if (adam) hipLaunchKernelGGL(fp_grad_adam_kernel<true>, grid, dim3(kThreads), 0, s, c, *adam, w, jw, jp, jm, pred, x, m, v, out, n, n4);
    else hipLaunchKernelGGL(fp_grad_adam_kernel<false>, grid, dim3(kThreads), 0, s, c, AdamCoef{}, w, jw, jp, jm, pred, x, m, v, out, n, n4);
    return hipGetLastError();
}

hipError_t launch_adam_step(const AdamCoef& c, float* x, float* m, float* v, const float* g, int64_t n, hipStream_t s) {
    if (n <= 0) return hipErrorInvalidValue;
    const int64_t n4 = aligned16({x, m, v, g}) ? n / 4 : 0;
    hipLaunchKernelGGL(adam_kernel, dim3(stream_blocks(std::max<int64_t>(n4, n - 4 * n4))), dim3(kThreads), 0, s, c, x, m, v, g, n, n4);
    return hipGetLastError();
}

}  // namespace pf
