// Batched GMRES on the device: (rt2[b] H H^T + sigma2 I) sol[b] = rhs[b] for every image of a batch at once, with the rules of the
// reference's utils.GMRES (pnpflow/utils.py:972-1109) as OT-ODE's generic branch calls it (ot_ode.py:119-128): zero initial guess, at
// most max_iter Krylov vectors and no restart, image b stops when |beta_{j+1}| < tol |rhs_b| or < atol, |rhs_b| < 1e-8 returns rhs_b
// itself (:995-996), _safe_normalize's eps rule (:1049-1054).
//
// Nothing of an iteration goes through the host.  Per Krylov iteration j the stream carries
//     H_adj, H on the whole batch  ->  w = rt2 H H^T v_j + sigma2 v_j  ->  [multi-dot, update] x 2  ->  one small kernel  ->  normalise
// - multi-dot: the j + 1 products <w, v_i> of every image in ONE launch; a workgroup holds its 4096-element piece of w in registers
//   and walks the basis once (classical Gram-Schmidt; modified Gram-Schmidt would be j + 1 dependent dot / axpy launch pairs);
// - update: w -= sum_i h_i v_i in one pass over the basis, with the squared norm of the result as a by-product of the second pass;
// - the second [multi-dot, update] pair is the re-orthogonalisation that gives classical Gram-Schmidt the accuracy of the modified one
//   (column = first coefficients + corrections);
// - the small kernel (one thread per image) owns the Hessenberg column, the Givens rotations, beta and the per-image done flag, in
//   fp64.  Every kernel returns at once for an image whose flag is set, so finished images cost nothing but the operator passes.
// Reductions: per-workgroup partial sums in fp64, wave butterflies and a fixed order over the workgroups - no float atomics, two runs
// agree bit for bit.  float4 accesses when n % 4 == 0 and every pointer is 16-byte aligned, scalar ones otherwise.
// The host polls the done flags every KR_POLL iterations only to leave the loop early; under stream capture it never polls (the
// loop then runs max_iter masked iterations).
#include <algorithm>
#include <cstdint>
#include <vector>
#include "pf_common.h"

namespace pf {

constexpr int KR_MAXM = 256;              // max_iter bound: the per-workgroup dot table lives in LDS
constexpr int KR_EPT = 16;                // elements of w per thread of the multi-dot / update kernels
constexpr int KR_CHUNK = 256 * KR_EPT;    // ... per workgroup
constexpr int KR_POLL = 8;

struct KrylovState {       // device pointers into the caller's workspace
    float* V;              // [m + 1][B][n] basis; slot j + 1 doubles as w of iteration j
    float* tmp;            // [B][n] H_adj(v_j)
    float* scratch;        // [B][n] scratch of the blur passes
    double* R;             // [B][m][m] rotated Hessenberg (column-major per image: R[i + j m])
    double* cs; double* sn;      // [B][m]
    double* beta;          // [B][m + 1]
    double* d1; double* d2;      // [B][m] Gram-Schmidt coefficients of the two passes
    double* ycoef;         // [B][m]
    double* pd;            // [B][nparts][m] partial dots
    double* pn;            // [B][nparts] partial squared norms
    double* bnorm;         // [B]
    float* wn;             // [B] norm of the vector to normalise
    int* done;             // [B]
    int* kfin;             // [B] Krylov vectors in the solution; 0: the right-hand side itself is returned
    size_t bn; int B, n, m, nparts;
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static int krylov_nparts(size_t n) { return (int)((n + KR_CHUNK - 1) / KR_CHUNK); }

size_t krylov_workspace_floats(int B, size_t n, int max_iter) {
    const size_t m = (size_t)std::max(max_iter, 1), bn = align_up((size_t)B * n, 4), np = (size_t)krylov_nparts(n);
    const size_t doubles = (size_t)B * (m * m + 6 * m + 2 + np * m + np);
    return (m + 3) * bn + 2 * doubles + align_up((size_t)B, 4) + 2 * align_up((size_t)B, 4) + 16;
}

static bool krylov_carve(KrylovState& k, float* ws, size_t ws_floats, int B, size_t n, int max_iter) {
    const size_t m = (size_t)max_iter, bn = align_up((size_t)B * n, 4), np = (size_t)krylov_nparts(n);
    if (((uintptr_t)ws & 15) != 0 || ws_floats < krylov_workspace_floats(B, n, max_iter)) return false;
    k.B = B; k.n = (int)n; k.m = max_iter; k.nparts = (int)np; k.bn = bn;
    float* p = ws;
    k.V = p; p += (m + 1) * bn;
    k.tmp = p; p += bn;
    k.scratch = p; p += bn;
    double* q = reinterpret_cast<double*>(p);      // (16-byte aligned: bn is a multiple of 4)
    k.R = q; q += (size_t)B * m * m;
    k.cs = q; q += (size_t)B * m; k.sn = q; q += (size_t)B * m;
    k.beta = q; q += (size_t)B * (m + 1);
    k.d1 = q; q += (size_t)B * m; k.d2 = q; q += (size_t)B * m;
    k.ycoef = q; q += (size_t)B * m;
    k.pd = q; q += (size_t)B * np * m;
    k.pn = q; q += (size_t)B * np;
    k.bnorm = q; q += B;
    p = reinterpret_cast<float*>(q);
    k.wn = p; p += align_up((size_t)B, 4);
    k.done = reinterpret_cast<int*>(p); p += align_up((size_t)B, 4);
    k.kfin = reinterpret_cast<int*>(p);
    return true;
}

// ---- element access: 4 consecutive elements per step, float4 or scalar --------------------------------------------------------
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ p, int e, int n, float v[4]) {
    if (VEC) {
        if (e < n) { const float4 t = *reinterpret_cast<const float4*>(p + e); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
        else { v[0] = v[1] = v[2] = v[3] = 0.f; }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = e + j < n ? p[e + j] : 0.f;
    }
}
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, int e, int n, const float v[4]) {
    if (VEC) {
        if (e < n) *reinterpret_cast<float4*>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e + j < n) p[e + j] = v[j];
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the four wave sums of a 256-thread workgroup, added in wave order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* s_red /* [4] */) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

// element index of quad q (0 .. KR_EPT / 4) of this thread inside the workgroup's piece: consecutive threads, consecutive quads
__device__ __forceinline__ int quad_elem(int part, int q) { return part * KR_CHUNK + (q * 256 + (int)threadIdx.x) * 4; }

// pd[b][part][i] = <w_b, v_i,b> over the workgroup's piece, i < k1
template <bool VEC>
__global__ __launch_bounds__(256) void krylov_multidot_kernel(const float* __restrict__ w, const float* __restrict__ V, size_t vstride, int k1, int n,
                                                             const int* __restrict__ done, double* __restrict__ pd, int m) {
    const int b = blockIdx.y, part = blockIdx.x;
    if (done[b]) return;
    __shared__ double s_dot[4][KR_MAXM];
    float wr[KR_EPT];
#pragma unroll
    for (int q = 0; q < KR_EPT / 4; ++q) load4<VEC>(w + (size_t)b * n, quad_elem(part, q), n, wr + 4 * q);
    for (int i = 0; i < k1; ++i) {
        const float* vi = V + (size_t)i * vstride + (size_t)b * n;
        double acc = 0.0;
#pragma unroll
        for (int q = 0; q < KR_EPT / 4; ++q) {
            float v[4];
            load4<VEC>(vi, quad_elem(part, q), n, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = fma((double)wr[4 * q + j], (double)v[j], acc);
        }
        acc = wave_sum(acc);
        if ((threadIdx.x & 63) == 0) s_dot[threadIdx.x >> 6][i] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < k1; i += 256)
        pd[((size_t)b * gridDim.x + part) * m + i] = ((s_dot[0][i] + s_dot[1][i]) + s_dot[2][i]) + s_dot[3][i];
}

// h_i = sum over the workgroups of pd (fixed order), w -= sum_i h_i v_i; hout[b][i] = h_i (workgroup 0), pn[b][part] = |new w|^2 over the piece
template <bool VEC>
__global__ __launch_bounds__(256) void krylov_update_kernel(float* __restrict__ w, const float* __restrict__ V, size_t vstride, int k1, int n,
                                                           const int* __restrict__ done, const double* __restrict__ pd, int m, double* __restrict__ hout,
                                                           double* __restrict__ pn) {
    const int b = blockIdx.y, part = blockIdx.x, nparts = gridDim.x;
    if (done[b]) return;
    __shared__ float s_h[KR_MAXM];
    __shared__ double s_red[4];
    for (int i = threadIdx.x; i < k1; i += 256) {
        double h = 0.0;
        for (int p = 0; p < nparts; ++p) h += pd[((size_t)b * nparts + p) * m + i];
        s_h[i] = (float)h;
        if (part == 0) hout[(size_t)b * m + i] = h;
    }
    __syncthreads();
    float wr[KR_EPT];
#pragma unroll
    for (int q = 0; q < KR_EPT / 4; ++q) load4<VEC>(w + (size_t)b * n, quad_elem(part, q), n, wr + 4 * q);
    for (int i = 0; i < k1; ++i) {
        const float* vi = V + (size_t)i * vstride + (size_t)b * n;
        const float h = s_h[i];
#pragma unroll
        for (int q = 0; q < KR_EPT / 4; ++q) {
            float v[4];
            load4<VEC>(vi, quad_elem(part, q), n, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) wr[4 * q + j] = fmaf(-h, v[j], wr[4 * q + j]);
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < KR_EPT / 4; ++q) {
        store4<VEC>(w + (size_t)b * n, quad_elem(part, q), n, wr + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = fma((double)wr[4 * q + j], (double)wr[4 * q + j], acc);      // (elements past n were loaded as 0)
    }
    acc = block_sum(acc, s_red);
    if (threadIdx.x == 0) pn[(size_t)b * nparts + part] = acc;
}

// pn[b][part] = |a_b|^2 over the piece (the right-hand side's norm)
template <bool VEC>
__global__ __launch_bounds__(256) void krylov_sqnorm_kernel(const float* __restrict__ a, int n, double* __restrict__ pn) {
    const int b = blockIdx.y, part = blockIdx.x;
    __shared__ double s_red[4];
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < KR_EPT / 4; ++q) {
        float v[4];
        load4<VEC>(a + (size_t)b * n, quad_elem(part, q), n, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = fma((double)v[j], (double)v[j], acc);
    }
    acc = block_sum(acc, s_red);
    if (threadIdx.x == 0) pn[(size_t)b * gridDim.x + part] = acc;
}

// one thread per image: |rhs_b|, the trivial return, beta_0
__global__ void krylov_init_kernel(KrylovState k, int max_iter) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= k.B) return;
    double s = 0.0;
    for (int p = 0; p < k.nparts; ++p) s += k.pn[(size_t)b * k.nparts + p];
    const float bn = (float)sqrt(s);                       // torch.norm of an fp32 vector is an fp32 number
    k.bnorm[b] = (double)bn;
    k.wn[b] = bn;
    const bool trivial = max_iter == 0 || bn < 1e-8f;      // utils.py:995-996
    k.done[b] = trivial ? 1 : 0;
    k.kfin[b] = 0;
    k.beta[(size_t)b * (k.m + 1)] = (double)bn;
}

// dst_b = wn[b] > eps ? src_b / wn[b] : 0   (_safe_normalize, utils.py:1049-1054); dst may be src
template <bool VEC>
__global__ __launch_bounds__(256) void krylov_normalise_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, const float* __restrict__ wn,
                                                              const int* __restrict__ done) {
    const int b = blockIdx.y;
    if (done[b]) return;
    const float nrm = wn[b];
    const bool ok = nrm > 1.1920928955078125e-07f;         // torch.finfo(float32).eps
    const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= n) return;
    float v[4];
    load4<VEC>(src + (size_t)b * n, e, n, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = ok ? v[j] / nrm : 0.f;
    store4<VEC>(dst + (size_t)b * n, e, n, v);
}

// w = rt2[b] * hh + sigma2 * v, each product rounded before the sum (ot_ode.py:124); w may be hh.  Contraction is switched off in the body:
// __fadd_rn(__fmul_rn(..), __fmul_rn(..)) inlines to a plain * and + that the compiler fused into mul + fma - in every lane of the float4
// instantiation and in two of the scalar one's four, so the two disagreed in the last bit and neither rounded as torch does.
template <bool VEC>
__global__ __launch_bounds__(256) void krylov_operator_kernel(const float* __restrict__ hh, const float* __restrict__ v, float* __restrict__ w, int n,
                                                             const float* __restrict__ rt2, float sigma2, const int* __restrict__ done) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    if (done[b]) return;
    const float r2 = rt2[b];
    const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= n) return;
    float a[4], c[4];
    load4<VEC>(hh + (size_t)b * n, e, n, a);
    load4<VEC>(v + (size_t)b * n, e, n, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float p0 = r2 * a[j], p1 = sigma2 * c[j];
        a[j] = p0 + p1;
    }
    store4<VEC>(w + (size_t)b * n, e, n, a);
}

// one thread per image, after the two Gram-Schmidt passes of iteration j: the new Hessenberg column, its rotations, beta, the stop test
// (utils.py:1027-1036, 1092-1109)
__global__ void krylov_givens_kernel(KrylovState k, int j, double tol, double atol) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= k.B || k.done[b]) return;
    const int m = k.m;
    double s = 0.0;
    for (int p = 0; p < k.nparts; ++p) s += k.pn[(size_t)b * k.nparts + p];
    const float wn = (float)sqrt(s);
    k.wn[b] = wn;
    double* col = k.R + (size_t)b * m * m + (size_t)j * m;       // rows 0 .. j of column j
    const double* cs = k.cs + (size_t)b * m; const double* sn = k.sn + (size_t)b * m;
    for (int i = 0; i <= j; ++i) col[i] = k.d1[(size_t)b * m + i] + k.d2[(size_t)b * m + i];
    double sub = (double)wn;                                     // H[j + 1][j]
    for (int i = 0; i < j; ++i) {
        const double a = col[i], c = col[i + 1];
        col[i] = cs[i] * a - sn[i] * c;
        col[i + 1] = cs[i] * c + sn[i] * a;
    }
    const double a = col[j], r = sqrt(a * a + sub * sub);
    const double c_ = a / r, s_ = -sub / r;                      // cal_rotation (utils.py:1079-1089)
    k.cs[(size_t)b * m + j] = c_; k.sn[(size_t)b * m + j] = s_;
    col[j] = c_ * a - s_ * sub;
    double* beta = k.beta + (size_t)b * (m + 1);
    beta[j + 1] = s_ * beta[j];
    beta[j] = c_ * beta[j];
    const double res = fabs(beta[j + 1]);
    k.kfin[b] = j + 1;
    if (res < tol * k.bnorm[b] || res < atol || j + 1 == m || !(res == res)) k.done[b] = 1;
}

// one thread per image: back substitution of the kfin x kfin triangle (utils.py:1037-1038)
__global__ void krylov_triangular_kernel(KrylovState k, int* __restrict__ iters_out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= k.B) return;
    const int m = k.m, kk = k.kfin[b];
    const double* R = k.R + (size_t)b * m * m; const double* beta = k.beta + (size_t)b * (m + 1);
    double* y = k.ycoef + (size_t)b * m;
    for (int i = kk - 1; i >= 0; --i) {
        double s = beta[i];
        for (int c = i + 1; c < kk; ++c) s -= R[i + (size_t)c * m] * y[c];
        y[i] = s / R[i + (size_t)i * m];
    }
    if (iters_out) iters_out[b] = kk;
}

// sol_b = sum_i y_i v_i,b (i ascending), or rhs_b when no iteration ran
template <bool VEC>
__global__ __launch_bounds__(256) void krylov_combine_kernel(const float* __restrict__ V, size_t vstride, const float* __restrict__ rhs, float* __restrict__ sol,
                                                            int n, const int* __restrict__ kfin, const double* __restrict__ ycoef, int m) {
    const int b = blockIdx.y, kk = kfin[b];
    __shared__ float s_y[KR_MAXM];
    for (int i = threadIdx.x; i < kk; i += 256) s_y[i] = (float)ycoef[(size_t)b * m + i];
    __syncthreads();
    const int e = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= n) return;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (kk == 0) load4<VEC>(rhs + (size_t)b * n, e, n, acc);
    for (int i = 0; i < kk; ++i) {
        float v[4];
        load4<VEC>(V + (size_t)i * vstride + (size_t)b * n, e, n, v);
        const float yi = s_y[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(yi, v[j], acc[j]);
    }
    store4<VEC>(sol + (size_t)b * n, e, n, acc);
}

#define KR_LAUNCH(kernel, grid, ...)                                                              \
    do {                                                                                          \
        if (vec) hipLaunchKernelGGL((kernel<true>), grid, dim3(256), 0, s, __VA_ARGS__);          \
        else hipLaunchKernelGGL((kernel<false>), grid, dim3(256), 0, s, __VA_ARGS__);             \
        hipError_t e_ = hipGetLastError();                                                        \
        if (e_ != hipSuccess) return e_;                                                          \
    } while (0)

hipError_t launch_krylov_solve(const DegView& d, const float* rt2, float sigma2, const float* rhs, float* sol, int B, int C, int H, int W, int max_iter,
                               float tol, float atol, float* ws, size_t ws_floats, int* iters_out, hipStream_t s, int* iterations_run) {
    if (iterations_run) *iterations_run = 0;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || max_iter < 0 || max_iter > KR_MAXM || !rt2 || !rhs || !sol || !ws) return hipErrorInvalidValue;
    if (deg_rule_violation(d, H, W) || deg_is_sr(d.kind)) return hipErrorInvalidValue;       // the measurement must have the image's shape
    if ((size_t)C * H * W > (size_t)0x7fffffff - KR_CHUNK) return hipErrorInvalidValue;
    const size_t n = (size_t)C * H * W;
    KrylovState k{};
    if (!krylov_carve(k, ws, ws_floats, B, n, std::max(max_iter, 1))) return hipErrorInvalidValue;
    k.m = std::max(max_iter, 1);
    const bool vec = (n % 4 == 0) && (((uintptr_t)rhs | (uintptr_t)sol) & 15) == 0;      // (the workspace's vectors are aligned: krylov_carve)
    const size_t vstride = k.bn;
    const dim3 gparts(k.nparts, B), gelem((unsigned)((n + 1023) / 1024), B), gimg((B + 63) / 64);
    const int ni = (int)n;

    KR_LAUNCH(krylov_sqnorm_kernel, gparts, rhs, ni, k.pn);
    hipLaunchKernelGGL(krylov_init_kernel, gimg, dim3(64), 0, s, k, max_iter);
    KR_LAUNCH(krylov_normalise_kernel, gelem, rhs, k.V, ni, (const float*)k.wn, (const int*)k.done);

    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
    const bool poll = cap == hipStreamCaptureStatusNone;
    std::vector<int> host_done((size_t)B);
    int j = 0;
    for (; j < max_iter; ++j) {
        float* vj = k.V + (size_t)j * vstride;
        float* w = k.V + (size_t)(j + 1) * vstride;
        hipError_t e = launch_deg_Hadj(d, vj, k.tmp, B, C, H, W, k.scratch, s);
        if (e != hipSuccess) return e;
        if ((e = launch_deg_H(d, k.tmp, w, B, C, H, W, k.scratch, s)) != hipSuccess) return e;
        KR_LAUNCH(krylov_operator_kernel, gelem, (const float*)w, (const float*)vj, w, ni, rt2, sigma2, (const int*)k.done);
        KR_LAUNCH(krylov_multidot_kernel, gparts, (const float*)w, (const float*)k.V, vstride, j + 1, ni, (const int*)k.done, k.pd, k.m);
        KR_LAUNCH(krylov_update_kernel, gparts, w, (const float*)k.V, vstride, j + 1, ni, (const int*)k.done, (const double*)k.pd, k.m, k.d1, k.pn);
        KR_LAUNCH(krylov_multidot_kernel, gparts, (const float*)w, (const float*)k.V, vstride, j + 1, ni, (const int*)k.done, k.pd, k.m);
        KR_LAUNCH(krylov_update_kernel, gparts, w, (const float*)k.V, vstride, j + 1, ni, (const int*)k.done, (const double*)k.pd, k.m, k.d2, k.pn);
        hipLaunchKernelGGL(krylov_givens_kernel, gimg, dim3(64), 0, s, k, j, (double)tol, (double)atol);
        KR_LAUNCH(krylov_normalise_kernel, gelem, (const float*)w, w, ni, (const float*)k.wn, (const int*)k.done);
        if (poll && (j + 1) % KR_POLL == 0 && j + 1 < max_iter) {
            if ((e = hipMemcpyAsync(host_done.data(), k.done, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
            if (std::all_of(host_done.begin(), host_done.end(), [](int v) { return v != 0; })) { ++j; break; }
        }
    }
    if (iterations_run) *iterations_run = j;
    hipLaunchKernelGGL(krylov_triangular_kernel, gimg, dim3(64), 0, s, k, iters_out);
    KR_LAUNCH(krylov_combine_kernel, gelem, (const float*)k.V, vstride, rhs, sol, ni, (const int*)k.kfin, (const double*)k.ycoef, k.m);
    return hipGetLastError();
}

}  // namespace pf
