// Glue kernels of the two flow solvers built on the velocity net's forward and input-gradient VJP:
//   * D-Flow (pnpflow/methods/d_flow.py): the explicit-midpoint map T(z) (forward_flow_matching, :41-49), its data term and latent
//     regulariser (closure, :110-121) and the reverse sweep of T's adjoint;
//   * the adaptive Dormand-Prince (dopri5) solve of dx/dt = v(x, t) that initialises the latent (inverse_flow_matching, :51-60);
//   * the prior's evaluation (pnpflow/utils.py:243-270 hut_estimator, pnpflow/image_generation/likelihood.py:116-195): the per-image dot
//     product eps . (J^T eps) of the Hutchinson estimator, the fp64 log-density entries of the augmented RK45 state and the bits/dim finish;
//   * the rectified-flow sampler (pnpflow/image_generation/sampling.py:69-109 euler_sampler): one fused Euler / Euler-Maruyama update per step.
// NCHW fp32 images; every per-image length is a multiple of 4 (float4 lanes: one thread = 4 consecutive values).
// Reductions are deterministic: per-block fp64 partial sums (a fixed number of blocks per image / tensor, a fixed tree inside the
// block) then a fixed-order finish - no float atomics, so replays of one input give bit-identical values (LBFGS's strong-Wolfe line
// search branches on them).
#include <algorithm>
#include "pf_common.h"
#include "philox_normal.h"

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

// a + c*b with the reference's separate fp32 multiply and add (no contraction into an fma): `z + delta * v`
__device__ __forceinline__ float axpy_rn(float a, float c, float b) { return __fadd_rn(a, __fmul_rn(c, b)); }

// ---- D-Flow -----------------------------------------------------------------------------------------------------------------------
// midpoint combine: out = z + c*v  (c = delta/2 for the evaluation point u_i, c = delta for the step z_{i+1})
__global__ __launch_bounds__(kThreads) void dflow_axpy4_kernel(const float4* __restrict__ z, const float4* __restrict__ v, float4* __restrict__ out,
                                                               float c, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        const float4 a = z[i], b = v[i];
        out[i] = make_float4(axpy_rn(a.x, c, b.x), axpy_rn(a.y, c, b.y), axpy_rn(a.z, c, b.z), axpy_rn(a.w, c, b.w));
    }
}

// per-image partials of sum(r^2), r = hx - y, and the seed numerator 2r (H_adj(2r) = 2 H_adj(r): the reverse sweep's seed)
__global__ __launch_bounds__(kThreads) void dflow_residual4_kernel(const float4* __restrict__ hx, const float4* __restrict__ y, float4* __restrict__ r2,
                                                                   double* __restrict__ partial, int64_t n4) {
    __shared__ double sh[kThreads];
    const int b = blockIdx.y;
    const float4* hb = hx + (size_t)b * n4; const float4* yb = y + (size_t)b * n4; float4* rb = r2 + (size_t)b * n4;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        const float4 a = hb[i], c = yb[i];
        const float rx = a.x - c.x, ry = a.y - c.y, rz = a.z - c.z, rw = a.w - c.w;
        acc += (double)(rx * rx) + (double)(ry * ry) + (double)(rz * rz) + (double)(rw * rw);
        rb[i] = make_float4(2.f * rx, 2.f * ry, 2.f * rz, 2.f * rw);
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// per-image partials of sum(z^2)
__global__ __launch_bounds__(kThreads) void sumsq4_kernel(const float4* __restrict__ z, double* __restrict__ partial, int64_t n4) {
    __shared__ double sh[kThreads];
    const int b = blockIdx.y;
    const float4* zb = z + (size_t)b * n4;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        const float4 a = zb[i];
        acc += (double)(a.x * a.x) + (double)(a.y * a.y) + (double)(a.z * a.z) + (double)(a.w * a.w);
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// per image b (one thread each, partials summed in index order):
//   loss[b] = |r_b|^2 + lmbda (0.5 clamp(|z_b|^2, -1e6, 1e6) - (d-1) log(|z_b| + 1e-5))
//   coef[b] = [-1e6 <= |z_b|^2 <= 1e6] - (d-1) / ((|z_b| + 1e-5) |z_b|)      (d reg / dz_b = coef[b] z_b)
__global__ void dflow_finish_kernel(const double* __restrict__ pdata, const double* __restrict__ pz, int nparts, int B, double dm1, float lmbda,
                                    float* __restrict__ loss, float* __restrict__ coef) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double data = 0.0, s = 0.0;
    for (int j = 0; j < nparts; ++j) { data += pdata[(size_t)b * nparts + j]; s += pz[(size_t)b * nparts + j]; }
    const double nrm = sqrt(s);
    const double reg = 0.5 * fmin(fmax(s, -1e6), 1e6) - dm1 * log(nrm + 1e-5);
    loss[b] = (float)(data + (double)lmbda * reg);
    coef[b] = (float)(((s >= -1e6 && s <= 1e6) ? 1.0 : 0.0) - dm1 / ((nrm + 1e-5) * nrm));
}

// grad = g + lmbda * coef[b] * z
__global__ __launch_bounds__(kThreads) void dflow_reg_grad4_kernel(const float4* __restrict__ g, const float4* __restrict__ z, const float* __restrict__ coef,
                                                                   float lmbda, float4* __restrict__ grad, int64_t n4) {
    const int b = blockIdx.y;
    const float c = lmbda * coef[b];
    const size_t o = (size_t)b * n4;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        const float4 a = g[o + i], w = z[o + i];
        grad[o + i] = make_float4(a.x + c * w.x, a.y + c * w.y, a.z + c * w.z, a.w + c * w.w);
    }
}

// reverse sweep of one midpoint step:  h = delta * J_v(u_i)^T g  (scale) ... g <- g + h + (delta/2) J_v(z_i)^T h  (accumulate)
__global__ __launch_bounds__(kThreads) void dflow_scale4_kernel(const float4* __restrict__ jg, float4* __restrict__ h, float delta, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        const float4 a = jg[i];
        h[i] = make_float4(delta * a.x, delta * a.y, delta * a.z, delta * a.w);
    }
}
__global__ __launch_bounds__(kThreads) void dflow_adjoint4_kernel(float4* __restrict__ g, const float4* __restrict__ h, const float4* __restrict__ jh,
                                                                  float half_delta, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        const float4 a = g[i], b = h[i], c = jh[i];
        g[i] = make_float4(a.x + b.x + half_delta * c.x, a.y + b.y + half_delta * c.y, a.z + b.z + half_delta * c.z, a.w + b.w + half_delta * c.w);
    }
}

// ---- dopri5 -----------------------------------------------------------------------------------------------------------------------
// out = y0 + sum_j c[j] k[j]   (torchdiffeq's y0 + k[..., :i+1] @ (beta_i * dt): the coefficients arrive already multiplied by dt)
__global__ __launch_bounds__(kThreads) void rk_combine4_kernel(const float4* __restrict__ y0, RkTerms t, float4* __restrict__ out, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < t.n; ++j) {
            const float4 k = reinterpret_cast<const float4*>(t.k[j])[i];
            const float c = t.c[j];
            acc.x = fmaf(c, k.x, acc.x); acc.y = fmaf(c, k.y, acc.y); acc.z = fmaf(c, k.z, acc.z); acc.w = fmaf(c, k.w, acc.w);
        }
        const float4 a = y0[i];
        out[i] = make_float4(a.x + acc.x, a.y + acc.y, a.z + acc.z, a.w + acc.w);
    }
}

// partials of sum((e / (atol + rtol * max(|y0|, |y1|)))^2) over the whole tensor, e = sum_j c[j] k[j] (the embedded error estimate,
// never materialised); y1 == nullptr: scale atol + rtol |y0| (the initial-step norms), e = a - b (b may be nullptr) when `err.n` is 0
__global__ __launch_bounds__(kThreads) void rk_norm4_kernel(const float4* __restrict__ a, const float4* __restrict__ b, const float4* __restrict__ y0,
                                                            const float4* __restrict__ y1, RkTerms err, float atol, float rtol,
                                                            double* __restrict__ partial, int64_t n4) {
    __shared__ double sh[kThreads];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        float4 e;
        if (err.n > 0) {
            e = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j = 0; j < err.n; ++j) {
                const float4 k = reinterpret_cast<const float4*>(err.k[j])[i];
                const float c = err.c[j];
                e.x = fmaf(c, k.x, e.x); e.y = fmaf(c, k.y, e.y); e.z = fmaf(c, k.z, e.z); e.w = fmaf(c, k.w, e.w);
            }
        } else {
            e = a[i];
            if (b) { const float4 q = b[i]; e = make_float4(e.x - q.x, e.y - q.y, e.z - q.z, e.w - q.w); }
        }
        const float4 p = y0[i];
        float4 m = make_float4(fabsf(p.x), fabsf(p.y), fabsf(p.z), fabsf(p.w));
        if (y1) { const float4 q = y1[i]; m = make_float4(fmaxf(m.x, fabsf(q.x)), fmaxf(m.y, fabsf(q.y)), fmaxf(m.z, fabsf(q.z)), fmaxf(m.w, fabsf(q.w))); }
        const float ex = e.x / (atol + rtol * m.x), ey = e.y / (atol + rtol * m.y), ez = e.z / (atol + rtol * m.z), ew = e.w / (atol + rtol * m.w);
        acc += (double)(ex * ex) + (double)(ey * ey) + (double)(ez * ez) + (double)(ew * ew);
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void sum_partials_kernel(const double* __restrict__ partial, int nparts, double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int j = 0; j < nparts; ++j) s += partial[j];
    out[0] = s;
}

// 4th-order dense output of the last accepted step at x = (t - t0) / (t1 - t0) (torchdiffeq interp.py _interp_fit/_interp_evaluate):
//   a = 2 dt (f1 - f0) - 8 (y1 + y0) + 16 ymid,  b = dt (5 f0 - 3 f1) + 18 y0 + 14 y1 - 32 ymid,  c = dt (f1 - 4 f0) - 11 y0 - 5 y1 + 16 ymid,
//   d = dt f0,  out = y0 + x d + x^2 c + x^3 b + x^4 a;   f = sign * k (k: the raw velocities, sign -1 for a reversed time axis)
__global__ __launch_bounds__(kThreads) void rk_interp4_kernel(const float* __restrict__ y0, const float* __restrict__ y1, const float* __restrict__ ymid,
                                                              const float* __restrict__ k0, const float* __restrict__ k6, float sign, float dt, float x,
                                                              float* __restrict__ out, int64_t n) {
    const float x2 = x * x, x3 = x2 * x, x4 = x3 * x;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const float f0 = sign * k0[i], f1 = sign * k6[i], a0 = y0[i], a1 = y1[i], am = ymid[i];
        const float ca = 2.f * dt * (f1 - f0) - 8.f * (a1 + a0) + 16.f * am;
        const float cb = dt * (5.f * f0 - 3.f * f1) + 18.f * a0 + 14.f * a1 - 32.f * am;
        const float cc = dt * (f1 - 4.f * f0) - 11.f * a0 - 5.f * a1 + 16.f * am;
        const float cd = dt * f0;
        out[i] = a0 + x * cd + x2 * cc + x3 * cb + x4 * ca;
    }
}

// ---- prior evaluation: Hutchinson divergence, augmented RK45 state, bits/dim ---------------------------------------------------------
// per-image partials of sum(a c)
__global__ __launch_bounds__(kThreads) void image_dot4_kernel(const float4* __restrict__ a, const float4* __restrict__ c, double* __restrict__ partial, int64_t n4) {
    __shared__ double sh[kThreads];
    const int b = blockIdx.y;
    const float4* ab = a + (size_t)b * n4; const float4* cb = c + (size_t)b * n4;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        const float4 p = ab[i], q = cb[i];
        acc += (double)(p.x * q.x) + (double)(p.y * q.y) + (double)(p.z * q.z) + (double)(p.w * q.w);
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = s;
}

// out[b] = sum of image b's partials, in index order (one thread per image)
__global__ void image_sum_kernel(const double* __restrict__ partial, int nparts, int B, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int j = 0; j < nparts; ++j) s += partial[(size_t)b * nparts + j];
    out[b] = s;
}

// The B log-density entries of the augmented state, in fp64 (one block; fixed strides and a fixed tree: deterministic):
//   new_b = logp_b + sum_j step[j] k[j][b],  err_b = sum_j err[j] k[j][b],  scale_b = atol + rtol max(|logp_b|, |new_b|)
//   sum_out[0] = (sum_x ? sum_x[0] : 0) + sum_b (err_b / scale_b)^2        logp_new (or nullptr) <- new
__global__ __launch_bounds__(kThreads) void rk_aug_kernel(RkAug c, const double* __restrict__ logp, double* __restrict__ logp_new, double atol, double rtol,
                                                          const double* __restrict__ sum_x, double* __restrict__ sum_out, int B) {
    __shared__ double sh[kThreads];
    double acc = 0.0;
    for (int b = threadIdx.x; b < B; b += kThreads) {
        double st = 0.0, er = 0.0;
        for (int j = 0; j < c.n; ++j) { const double k = c.k[j][b]; st += c.step[j] * k; er += c.err[j] * k; }
        const double y0 = logp[b], y1 = y0 + st;
        if (logp_new) logp_new[b] = y1;
        const double q = er / (atol + rtol * fmax(fabs(y0), fabs(y1)));
        acc += q * q;
    }
    const double s = block_sum(acc, sh);
    if (threadIdx.x == 0) sum_out[0] = (sum_x ? sum_x[0] : 0.0) + s;
}

// per image (one thread each, the partials of sum z^2 summed in index order), N = C*H*W:
//   prior = -N/2 ln(2 pi) - 1/2 sum z^2,   bpd = -(prior + delta_logp) / (N ln 2) + offset        (likelihood.py:144-148, 186-192)
__global__ void bpd_finish_kernel(const double* __restrict__ pz, int nparts, int B, double N, const double* __restrict__ delta_logp, double offset,
                                  float* __restrict__ bpd) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int j = 0; j < nparts; ++j) s += pz[(size_t)b * nparts + j];
    const double prior = -0.5 * N * 1.8378770664093453 - 0.5 * s;      // ln(2 pi)
    bpd[b] = (float)(-(prior + delta_logp[b]) / (N * 0.6931471805599453) + offset);
}


// ---- rectified-flow sampler: one step of euler_sampler (sampling.py:92-105) -------------------------------------------------------------
//   pred_sigma = pred + c0 (a1 pred - a2 x),   x <- x + pred_sigma dt + s n
// every product and sum rounded on its own, in the order torch evaluates the reference's expression (no contraction into an fma).
// kNoise 0: the deterministic step x + pred dt (c.s == 0: nothing is read or drawn); 1: n read from `noise`; 2: n drawn here - lane q of
// the tensor takes normals [first + 4q, first + 4q + 4) of the stream (first % 4 == 0: whole Philox counters), the values
// fill_normal_kernel writes for elem_offset = first.
template <int kNoise>
__global__ __launch_bounds__(kThreads) void rf_euler_step4_kernel(float4* __restrict__ x, const float4* __restrict__ pred, const float4* __restrict__ noise,
                                                                  RfStepCoef c, uint64_t seed, uint64_t stream, uint64_t first, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
        const float4 a = x[i], p = pred[i];
        if (kNoise == 0) {
            x[i] = make_float4(axpy_rn(a.x, c.dt, p.x), axpy_rn(a.y, c.dt, p.y), axpy_rn(a.z, c.dt, p.z), axpy_rn(a.w, c.dt, p.w));
            continue;
        }
        float4 z;
        if (kNoise == 1) z = noise[i]; else z = normal4((first >> 2) + (uint64_t)i, seed, stream);
        auto step = [&](float xv, float pv, float zv) {
            const float inner = __fsub_rn(__fmul_rn(c.a1, pv), __fmul_rn(c.a2, xv));
            const float ps = __fadd_rn(pv, __fmul_rn(c.c0, inner));
            return __fadd_rn(axpy_rn(xv, c.dt, ps), __fmul_rn(c.s, zv));
        };
        x[i] = make_float4(step(a.x, p.x, z.x), step(a.y, p.y, z.y), step(a.z, p.z, z.z), step(a.w, p.w, z.w));
    }
}

}  // namespace

int reduction_parts(int64_t n4) { return (int)std::max<int64_t>(1, std::min<int64_t>((n4 + kThreads - 1) / kThreads, 64)); }

hipError_t launch_dflow_axpy(const float* z, const float* v, float* out, float c, int64_t n, hipStream_t s) {
    if (n % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dflow_axpy4_kernel, dim3(stream_blocks(n / 4)), dim3(kThreads), 0, s, (const float4*)z, (const float4*)v, (float4*)out, c, n / 4);
    return hipGetLastError();
}

hipError_t launch_dflow_objective(const float* hx, const float* y, float* r2, const float* z, double* partial, float* loss, float* coef, float lmbda,
                                  int B, int64_t ny, int64_t n, hipStream_t s) {
    if (ny % 4 || n % 4) return hipErrorInvalidValue;
    const int pr = reduction_parts(ny / 4), pz = reduction_parts(n / 4), np = std::max(pr, pz);
    // both partial sets padded to `np` parts per image (unused parts written as 0 by blocks that find no work)
    hipLaunchKernelGGL(dflow_residual4_kernel, dim3(np, B), dim3(kThreads), 0, s, (const float4*)hx, (const float4*)y, (float4*)r2, partial, ny / 4);
    hipLaunchKernelGGL(sumsq4_kernel, dim3(np, B), dim3(kThreads), 0, s, (const float4*)z, partial + (size_t)B * np, n / 4);
    hipLaunchKernelGGL(dflow_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const double*)partial, (const double*)(partial + (size_t)B * np), np, B,
                       (double)(n - 1), lmbda, loss, coef);
    return hipGetLastError();
}

hipError_t launch_dflow_reg_grad(const float* g, const float* z, const float* coef, float lmbda, float* grad, int B, int64_t n, hipStream_t s) {
    if (n % 4) return hipErrorInvalidValue;
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n / 4 + kThreads - 1) / kThreads, std::max(1, 2048 / std::max(1, B))));
    hipLaunchKernelGGL(dflow_reg_grad4_kernel, dim3(gx, B), dim3(kThreads), 0, s, (const float4*)g, (const float4*)z, coef, lmbda, (float4*)grad, n / 4);
    return hipGetLastError();
}

hipError_t launch_dflow_scale(const float* jg, float* h, float delta, int64_t n, hipStream_t s) {
    if (n % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dflow_scale4_kernel, dim3(stream_blocks(n / 4)), dim3(kThreads), 0, s, (const float4*)jg, (float4*)h, delta, n / 4);
    return hipGetLastError();
}

hipError_t launch_dflow_adjoint(float* g, const float* h, const float* jh, float half_delta, int64_t n, hipStream_t s) {
    if (n % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dflow_adjoint4_kernel, dim3(stream_blocks(n / 4)), dim3(kThreads), 0, s, (float4*)g, (const float4*)h, (const float4*)jh, half_delta, n / 4);
    return hipGetLastError();
}

hipError_t launch_rk_combine(const float* y0, const RkTerms& t, float* out, int64_t n, hipStream_t s) {
    if (n % 4 || t.n < 0 || t.n > 7) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rk_combine4_kernel, dim3(stream_blocks(n / 4)), dim3(kThreads), 0, s, (const float4*)y0, t, (float4*)out, n / 4);
    return hipGetLastError();
}

hipError_t launch_rk_norm(const float* a, const float* b, const float* y0, const float* y1, const RkTerms& err, float atol, float rtol, double* partial,
                          double* out, int64_t n, hipStream_t s) {
    if (n % 4 || err.n < 0 || err.n > 7 || (err.n == 0 && !a)) return hipErrorInvalidValue;
    const int np = reduction_parts(n / 4);
    hipLaunchKernelGGL(rk_norm4_kernel, dim3(np), dim3(kThreads), 0, s, (const float4*)a, (const float4*)b, (const float4*)y0, (const float4*)y1, err,
                       atol, rtol, partial, n / 4);
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(64), 0, s, (const double*)partial, np, out);
    return hipGetLastError();
}

hipError_t launch_rk_interp(const float* y0, const float* y1, const float* ymid, const float* k0, const float* k6, float sign, float dt, float x, float* out,
                            int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(rk_interp4_kernel, dim3(stream_blocks(n)), dim3(kThreads), 0, s, y0, y1, ymid, k0, k6, sign, dt, x, out, n);
    return hipGetLastError();
}

hipError_t launch_image_dot(const float* a, const float* c, double* partial, double* out, int B, int64_t n, hipStream_t s) {
    if (n % 4 || B <= 0) return hipErrorInvalidValue;
    const int np = reduction_parts(n / 4);
    hipLaunchKernelGGL(image_dot4_kernel, dim3(np, B), dim3(kThreads), 0, s, (const float4*)a, (const float4*)c, partial, n / 4);
    hipLaunchKernelGGL(image_sum_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const double*)partial, np, B, out);
    return hipGetLastError();
}

hipError_t launch_rk_aug(const RkAug& c, const double* logp, double* logp_new, double atol, double rtol, const double* sum_x, double* sum_out, int B,
                         hipStream_t s) {
    if (c.n < 0 || c.n > 7 || B <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rk_aug_kernel, dim3(1), dim3(kThreads), 0, s, c, logp, logp_new, atol, rtol, sum_x, sum_out, B);
    return hipGetLastError();
}

hipError_t launch_bpd_finish(const float* z, const double* delta_logp, double* partial, float* bpd, double offset, int B, int64_t n, hipStream_t s) {
    if (n % 4 || B <= 0) return hipErrorInvalidValue;
    const int np = reduction_parts(n / 4);
    hipLaunchKernelGGL(sumsq4_kernel, dim3(np, B), dim3(kThreads), 0, s, (const float4*)z, partial, n / 4);
    hipLaunchKernelGGL(bpd_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const double*)partial, np, B, (double)n, delta_logp, offset, bpd);
    return hipGetLastError();
}

hipError_t launch_rf_euler_step(float* x, const float* pred, const float* noise, const RfStepCoef& c, uint64_t seed, uint64_t stream_id, uint64_t first,
                                int64_t n, hipStream_t s) {
    if (n % 4 || first % 4) return hipErrorInvalidValue;
    const dim3 grid(stream_blocks(n / 4)), block(kThreads);
    if (c.s == 0.f)
        hipLaunchKernelGGL(rf_euler_step4_kernel<0>, grid, block, 0, s, (float4*)x, (const float4*)pred, (const float4*)nullptr, c, seed, stream_id, first, n / 4);
    else if (noise)
        hipLaunchKernelGGL(rf_euler_step4_kernel<1>, grid, block, 0, s, (float4*)x, (const float4*)pred, (const float4*)noise, c, seed, stream_id, first, n / 4);
    else
        hipLaunchKernelGGL(rf_euler_step4_kernel<2>, grid, block, 0, s, (float4*)x, (const float4*)pred, (const float4*)nullptr, c, seed, stream_id, first, n / 4);
    return hipGetLastError();
}

}  // namespace pf
