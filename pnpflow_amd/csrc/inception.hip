// The feature network of the FID: pytorch-fid's "FID Inception" (the reference's pnpflow/models.py:498-820, InceptionV3 with
// use_fid_inception=True) in eval mode, as pnpflow/fid_score.py:21-71 (get_activations) drives it.
//
// Third-party network: torchvision's Inception-v3 with pytorch-fid's patches, restated from the published definition (the layer table
// is csrc/inception_plan.h):
//   x  = bilinear resize to 299 x 299 (align_corners=False, no antialiasing) when resize_input;  x <- 2 x - 1 when normalize_input
//   a layer = relu(BatchNorm_eval(conv(x))), conv without bias, BatchNorm eps 1e-3 on the running statistics
//   average pools: 3 x 3, stride 1, pad 1, count_include_pad=False (the TensorFlow rule); Mixed_7c pools with a MAX (the FID network's own)
//   output block 0 / 1 / 2 / 3 = after the first max pool (64) / the second (192) / Mixed_6e (768) / the global average (2048)
// PARITY UNPINNED for the network: torchvision and the weight file pt_inception-2015-12-05-6726825d.pth are not in the build image;
// the tests compare with a plain-torch restatement of the same table (tests/inception_reference.py) on synthetic weights loaded under
// the published key names.  The Frechet distance on top of the features (pnpflow_amd/fid_score.py) IS pinned against the reference.
//
// Kernels.  Activations are NHWC.  Every conv is one implicit GEMM, M = B Ho Wo pixels, N = Cout, K = KH KW Cin (k = (ky KW + kx) Cin + ci),
// on the fp32-input MFMA v_mfma_f32_32x32x2_f32: products and sums are plain fp32 (a k-ordered fmaf chain), no operand split.  256
// threads = four waves as 2 x 2 over an MT x NT tile (template parameter, chosen by inc::choose_tile).  Both operands go through LDS in
// K-chunks of 16, double-buffered: the global loads of chunk c + 1 are issued before the MFMAs of chunk c and written to the other
// buffer after them, one barrier per chunk.  KH, KW, stride and the two pads are launch arguments.  Every 8 chunks the running
// accumulator is added to a total and cleared (blocked summation: the rounding error of a K = 4032 sum grows like that of a 128-term
// one).  Epilogue: relu(acc * scale[c] + shift[c]) with the BatchNorm folded into scale / shift at weight load, written into channels
// [out_off, out_off + Cout) of a tensor with out_cs channels - a Mixed block's branches fill their slices, no concatenation runs.
// A pixel's arithmetic does not depend on where in M it sits or on the tile: features are bit-equal for any batch split.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "../../include/pnpflow_hip.h"
#include "inception_plan.h"

namespace pf {
namespace inc {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KC = INC_KC;
constexpr int FLUSH = 8;            // chunks between two additions of the running accumulator to the total

struct ConvArgs {
    const float* in; const float* w; const float* scale; const float* shift; float* out;
    int Hi, Wi, Ho, Wo, Cin, in_cs, in_off, Cout, out_cs, out_off, KH, KW, S, PH, PW, K, Kp, M;
};

// VEC: Cin % 16 == 0 and 16-byte aligned pixels - a K-chunk lies inside one tap and a thread loads float4 of channels.  Otherwise (the
// first layer, Cin = 3) one scalar per (pixel, k) with the tap decoded per element and k >= K read as 0.
template <int MT, int NT, bool VEC>
__global__ __launch_bounds__(256) void inc_conv_kernel(const ConvArgs p) {
    constexpr int LDA = MT + 4, LDB = NT + 4;
    constexpr int KL = VEC ? 4 : 1;                   // k values per thread and row of the A stage
    constexpr int LPR = KC / KL;                      // lanes per row
    constexpr int RPP = 256 / LPR;                    // rows per pass
    constexpr int RA = MT / RPP;                      // A rows per thread
    constexpr int BL = NT / 4, BR = 256 / BL, RB = KC / BR;      // B stage: lanes per k-row, k-rows per pass, passes
    constexpr int FM = MT / 64, FN = NT / 64;         // 32 x 32 MFMA tiles per wave
    __shared__ __attribute__((aligned(16))) float As[2][KC][LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][KC][LDB];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * MT, n0 = blockIdx.y * NT;
    const int a_k = (t % LPR) * KL, a_row = t / LPR;
    const int b_n = (t % BL) * 4, b_row = t / BL;

    int pixbase[RA], iy0[RA], ix0[RA];
#pragma unroll
    for (int j = 0; j < RA; ++j) {
        const int m = m0 + a_row + RPP * j;
        if (m < p.M) {
            const int b = m / (p.Ho * p.Wo), r = m - b * p.Ho * p.Wo, oy = r / p.Wo, ox = r - oy * p.Wo;
            pixbase[j] = b * p.Hi * p.Wi; iy0[j] = oy * p.S - p.PH; ix0[j] = ox * p.S - p.PW;
        } else {
            pixbase[j] = 0; iy0[j] = -(1 << 20); ix0[j] = 0;          // every tap of a row past M is out of the image: zeros
        }
    }

    float4 ra[RA], rb[RB];
    auto load_chunk = [&](int c) {
        const int k0 = c * KC;
        if (VEC) {
            const int tap = k0 / p.Cin, ci0 = k0 - tap * p.Cin, ky = tap / p.KW, kx = tap - ky * p.KW;
#pragma unroll
            for (int j = 0; j < RA; ++j) {
                const int iy = iy0[j] + ky, ix = ix0[j] + kx;
                ra[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi)
                    ra[j] = *reinterpret_cast<const float4*>(p.in + (size_t)(pixbase[j] + iy * p.Wi + ix) * p.in_cs + p.in_off + ci0 + a_k);
            }
        } else {
            const int k = k0 + a_k;
            const int tap = k / p.Cin, ci = k - tap * p.Cin, ky = tap / p.KW, kx = tap - ky * p.KW;
#pragma unroll
            for (int j = 0; j < RA; ++j) {
                const int iy = iy0[j] + ky, ix = ix0[j] + kx;
                float v = 0.f;
                if (k < p.K && iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi) v = p.in[(size_t)(pixbase[j] + iy * p.Wi + ix) * p.in_cs + p.in_off + ci];
                ra[j].x = v;
            }
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            const int n = n0 + b_n;
            rb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n < p.Cout) rb[j] = *reinterpret_cast<const float4*>(p.w + (size_t)(k0 + b_row + BR * j) * p.Cout + n);      // Cout % 4 == 0; rows up to Kp exist
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int j = 0; j < RA; ++j) {
            const int row = a_row + RPP * j;
            As[buf][a_k][row] = ra[j].x;
            if (VEC) { As[buf][a_k + 1][row] = ra[j].y; As[buf][a_k + 2][row] = ra[j].z; As[buf][a_k + 3][row] = ra[j].w; }
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) *reinterpret_cast<float4*>(&Bs[buf][b_row + BR * j][b_n]) = rb[j];
    };

    f32x16 acc[FM][FN], tot[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) { acc[i][j][v] = 0.f; tot[i][j][v] = 0.f; }

    const int nchunks = p.Kp / KC;
    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    const int half = lane >> 5, l31 = lane & 31;
    for (int c = 0; c < nchunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < nchunks) load_chunk(c + 1);
#pragma unroll
        for (int kk = 0; kk < KC; kk += 2) {
            float a[FM], b[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) a[i] = As[buf][kk + half][wm * (MT / 2) + i * 32 + l31];
#pragma unroll
            for (int j = 0; j < FN; ++j) b[j] = Bs[buf][kk + half][wn * (NT / 2) + j * 32 + l31];
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (c + 1 < nchunks) store_chunk(buf ^ 1);
        if ((c % FLUSH) == FLUSH - 1 || c + 1 == nchunks) {
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) {
                    tot[i][j] += acc[i][j];
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;
                }
        }
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n0 + wn * (NT / 2) + j * 32 + l31;
        if (n >= p.Cout) continue;
        const float sc = p.scale[n], sh = p.shift[n];
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int m = m0 + wm * (MT / 2) + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * half;
                if (m < p.M) p.out[(size_t)m * p.out_cs + p.out_off + n] = fmaxf(fmaf(tot[i][j][v], sc, sh), 0.f);
            }
    }
}

// 3 x 3 pools on channel slices of NHWC tensors.  MODE 1: max, stride 2, no pad.  2: average, stride 1, pad 1, divided by the number of
// taps inside the image.  3: max, stride 1, pad 1 (the pad never wins: torch pads a max pool with -inf).
template <int MODE>
__global__ __launch_bounds__(256) void inc_pool_kernel(const float* __restrict__ in, int in_cs, int in_off, float* __restrict__ out, int out_cs, int out_off,
                                                      int C, int Hi, int Wi, int Ho, int Wo, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const size_t pix = i / C;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho);
    const size_t b = pix / ((size_t)Wo * Ho);
    const int S = MODE == 1 ? 2 : 1, P = MODE == 1 ? 0 : 1;
    float acc = MODE == 2 ? 0.f : -INFINITY;
    int cnt = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = oy * S - P + dy;
        if (iy < 0 || iy >= Hi) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = ox * S - P + dx;
            if (ix < 0 || ix >= Wi) continue;
            const float v = in[((b * Hi + iy) * Wi + ix) * in_cs + in_off + c];
            if (MODE == 2) { acc += v; ++cnt; } else acc = fmaxf(acc, v);
        }
    }
    out[pix * out_cs + out_off + c] = MODE == 2 ? acc / (float)cnt : acc;
}

// out[b][c] = mean over the HW pixels of in[b][.][c] (NHWC, cs channels per pixel).  256 threads = 64 channels x 4 pixel groups, fp64 sums added
// in a fixed order: one rounding to fp32 at the end, the same bits for an image whatever the batch.
__global__ __launch_bounds__(256) void inc_gap_kernel(const float* __restrict__ in, int cs, int C, int HW, float* __restrict__ out) {
    __shared__ double s[4][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6, c = blockIdx.x * 64 + cl, b = blockIdx.y;
    double acc = 0.0;
    if (c < C)
        for (int pix = g; pix < HW; pix += 4) acc += (double)in[((size_t)b * HW + pix) * cs + c];
    s[g][cl] = acc;
    __syncthreads();
    if (g == 0 && c < C) out[(size_t)b * C + c] = (float)((((s[0][cl] + s[1][cl]) + s[2][cl]) + s[3][cl]) / (double)HW);
}

// NCHW image [B][3][H][W] -> NHWC [B][Ho][Wo][3]; resize: torch's bilinear with align_corners=False (source index (dst + 0.5) * in / out - 0.5,
// clamped at 0; no antialiasing), then 2 x - 1 when normalize.  Without resize Ho = H, Wo = W.
__global__ __launch_bounds__(256) void inc_front_kernel(const float* __restrict__ img, float* __restrict__ out, int H, int W, int Ho, int Wo, int resize,
                                                       int normalize, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho);
    const size_t b = i / ((size_t)Wo * Ho);
    const float* ib = img + b * 3 * (size_t)H * W;
    float v[3];
    if (resize) {
        const float sh = (float)H / (float)Ho, sw = (float)W / (float)Wo;
        // product and difference rounded one after the other, as torch's source index is (a fused multiply-add moves the index by up to half an ulp of 299)
        const float fy = fmaxf(__fsub_rn(__fmul_rn(sh, (float)y + 0.5f), 0.5f), 0.f), fx = fmaxf(__fsub_rn(__fmul_rn(sw, (float)x + 0.5f), 0.5f), 0.f);
        const int y0 = min((int)fy, H - 1), x0 = min((int)fx, W - 1), y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
        const float ly1 = fy - (float)y0, ly0 = 1.f - ly1, lx1 = fx - (float)x0, lx0 = 1.f - lx1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* ip = ib + (size_t)c * H * W;
            v[c] = ly0 * (lx0 * ip[(size_t)y0 * W + x0] + lx1 * ip[(size_t)y0 * W + x1]) + ly1 * (lx0 * ip[(size_t)y1 * W + x0] + lx1 * ip[(size_t)y1 * W + x1]);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = ib[((size_t)c * H + y) * W + x];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = normalize ? 2.f * v[c] - 1.f : v[c];
}

template <int MT, int NT>
static void launch_tile(const ConvArgs& a, bool vec, hipStream_t s) {
    const dim3 grid((a.M + MT - 1) / MT, (a.Cout + NT - 1) / NT);
    if (vec) hipLaunchKernelGGL((inc_conv_kernel<MT, NT, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((inc_conv_kernel<MT, NT, false>), grid, dim3(256), 0, s, a);
}

// nullptr, or why the launch is refused (nothing is launched then)
static const char* launch_conv(const ConvArgs& a, int tile, hipStream_t s) {
    if (a.M <= 0 || a.Cin <= 0 || a.Cout <= 0 || a.KH <= 0 || a.KW <= 0 || a.S <= 0 || a.PH < 0 || a.PW < 0 || a.Ho <= 0 || a.Wo <= 0) return "Inception conv: empty shape";
    if (a.Cout % 4 != 0) return "Inception conv: Cout must be a multiple of 4";
    if (a.out_off < 0 || a.out_off + a.Cout > a.out_cs || a.in_off < 0 || a.in_off + a.Cin > a.in_cs) return "Inception conv: channel slice outside its tensor";
    if (a.Kp % KC != 0 || a.Kp < a.K) return "Inception conv: weights not packed";
    const bool vec = a.Cin % KC == 0 && a.in_cs % 4 == 0 && a.in_off % 4 == 0 && ((uintptr_t)a.in & 15) == 0;
    switch (tile) {
        case T128x128: launch_tile<128, 128>(a, vec, s); break;
        case T128x64: launch_tile<128, 64>(a, vec, s); break;
        case T64x128: launch_tile<64, 128>(a, vec, s); break;
        case T64x64: launch_tile<64, 64>(a, vec, s); break;
        default: return "Inception conv: unknown tile";
    }
    return nullptr;
}

static void launch_pool(int kind, const float* in, int in_cs, int in_off, float* out, int out_cs, int out_off, int B, int C, int Hi, int Wi, int Ho, int Wo,
                        hipStream_t s) {
    const size_t n = (size_t)B * Ho * Wo * C;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (kind == OP_MAXPOOL_S2) hipLaunchKernelGGL(inc_pool_kernel<1>, grid, dim3(256), 0, s, in, in_cs, in_off, out, out_cs, out_off, C, Hi, Wi, Ho, Wo, n);
    else if (kind == OP_AVGPOOL_S1) hipLaunchKernelGGL(inc_pool_kernel<2>, grid, dim3(256), 0, s, in, in_cs, in_off, out, out_cs, out_off, C, Hi, Wi, Ho, Wo, n);
    else hipLaunchKernelGGL(inc_pool_kernel<3>, grid, dim3(256), 0, s, in, in_cs, in_off, out, out_cs, out_off, C, Hi, Wi, Ho, Wo, n);
}

// [Cout][Cin][KH][KW] -> [Kp][Cout], k = (ky KW + kx) Cin + ci, rows K..Kp zero
static std::vector<float> pack_weight(const float* w, int Cout, int Cin, int KH, int KW) {
    const int K = KH * KW * Cin, Kp = (K + KC - 1) / KC * KC;
    std::vector<float> o((size_t)Kp * Cout, 0.f);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int ky = 0; ky < KH; ++ky)
                for (int kx = 0; kx < KW; ++kx)
                    o[(size_t)((ky * KW + kx) * Cin + ci) * Cout + co] = w[(((size_t)co * Cin + ci) * KH + ky) * KW + kx];
    return o;
}

struct Guard { int prev = -1; explicit Guard(int d) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; hipSetDevice(d); } ~Guard() { if (prev >= 0) hipSetDevice(prev); } };

struct LayerW {
    float* w = nullptr; float* scale = nullptr; float* shift = nullptr;
    std::vector<float> bn[4];            // weight, bias, running_mean, running_var as loaded
    bool folded = false;
};

}  // namespace inc
}  // namespace pf

using namespace pf::inc;

struct pf_inception {
    int device = 0;
    std::string err;
    std::vector<LayerW> lw;
    std::vector<void*> allocs;
    float* buf[NUM_BUFS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t cap[NUM_BUFS] = {0, 0, 0, 0, 0, 0};
    bool profile = false;
    std::vector<float> op_ms;            // per launch of the last profiled forward
    std::vector<std::string> op_name;
    std::vector<double> op_flops;        // 2 M K Cout of a conv launch, 0 otherwise
};

int pf_inception_create(int device_id, pf_inception** out) {
    if (!out) return PF_ERR_INVALID;
    auto* l = new pf_inception(); l->device = device_id; l->lw.resize(layers().size());
    *out = l;
    return PF_OK;
}

void pf_inception_destroy(pf_inception* l) {
    if (!l) return;
    Guard g(l->device);
    for (void* p : l->allocs) hipFree(p);
    delete l;
}

const char* pf_inception_last_error(const pf_inception* l) { return l ? l->err.c_str() : ""; }

static int inc_upload(pf_inception* l, float*& dst, const std::vector<float>& host) {
    if (!dst) {
        if (hipMalloc(&dst, host.size() * sizeof(float)) != hipSuccess) { dst = nullptr; l->err = "hipMalloc failed (Inception weights)"; return PF_ERR_HIP; }
        l->allocs.push_back(dst);
    }
    if (hipMemcpy(dst, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { l->err = "hipMemcpy failed (Inception weights)"; return PF_ERR_HIP; }
    return PF_OK;
}

int pf_inception_load_weight(pf_inception* l, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!l || !name || !host || !shape || ndim < 1 || ndim > 4) return PF_ERR_INVALID;
    Guard g(l->device);
    const std::string n(name);
    static const char* SUF[5] = {".conv.weight", ".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var"};
    int which = -1, li = -1;
    for (int k = 0; k < 5 && li < 0; ++k) {
        const std::string suf(SUF[k]);
        if (n.size() > suf.size() && n.compare(n.size() - suf.size(), suf.size(), suf) == 0) { which = k; li = layer_index(n.substr(0, n.size() - suf.size())); }
    }
    if (li < 0) { l->err = "unknown Inception weight " + n; return PF_ERR_WEIGHTS; }
    const Layer& L = layers()[li];
    int64_t cnt = 1;
    for (int i = 0; i < ndim; ++i) cnt *= shape[i];
    if (which == 0) {
        if (ndim != 4 || shape[0] != L.Cout || shape[1] != L.Cin || shape[2] != L.KH || shape[3] != L.KW) { l->err = "shape mismatch for " + n; return PF_ERR_WEIGHTS; }
        return inc_upload(l, l->lw[li].w, pack_weight(host, L.Cout, L.Cin, L.KH, L.KW));
    }
    if (cnt != L.Cout) { l->err = "shape mismatch for " + n; return PF_ERR_WEIGHTS; }
    LayerW& W = l->lw[li];
    W.bn[which - 1].assign(host, host + cnt);
    W.folded = false;
    if (W.bn[0].empty() || W.bn[1].empty() || W.bn[2].empty() || W.bn[3].empty()) return PF_OK;
    // BatchNorm (eval, eps 1e-3) folded in fp64, rounded once: y = x * scale + shift
    std::vector<float> sc(L.Cout), sh(L.Cout);
    for (int c = 0; c < L.Cout; ++c) {
        const double s = (double)W.bn[0][c] / std::sqrt((double)W.bn[3][c] + 1e-3);
        sc[c] = (float)s; sh[c] = (float)((double)W.bn[1][c] - (double)W.bn[2][c] * s);
    }
    int rc = inc_upload(l, W.scale, sc);
    if (rc == PF_OK) rc = inc_upload(l, W.shift, sh);
    W.folded = rc == PF_OK;
    return rc;
}

int pf_inception_forward(pf_inception* l, const float* img, float* out, int B, int H, int W, int resize_input, int normalize_input, int output_block, void* stream) {
    if (!l) return PF_ERR_INVALID;
    if (!img || !out) { l->err = "pf_inception_forward: NULL image or output"; return PF_ERR_INVALID; }
    Guard g(l->device);
    hipStream_t s = (hipStream_t)stream;
    const Plan p = plan(B, H, W, resize_input != 0, output_block);
    if (!p.ok) { l->err = p.err; return PF_ERR_INVALID; }
    for (const Op& o : p.ops)
        if (o.kind == OP_CONV && (!l->lw[o.layer].w || !l->lw[o.layer].folded)) { l->err = "Inception weight not loaded: " + layers()[o.layer].name; return PF_ERR_STATE; }
    for (int b = 0; b < NUM_BUFS; ++b) {
        if (p.buf_floats[b] <= l->cap[b]) continue;
        hipStreamSynchronize(s);                    // launches of an earlier forward may still read the buffer
        if (l->buf[b]) {                            // free + forget first: a failed regrow leaves nothing stale behind
            hipFree(l->buf[b]);
            auto it = std::find(l->allocs.begin(), l->allocs.end(), (void*)l->buf[b]);
            if (it != l->allocs.end()) l->allocs.erase(it);
            l->buf[b] = nullptr; l->cap[b] = 0;
        }
        if (hipMalloc(&l->buf[b], p.buf_floats[b] * sizeof(float)) != hipSuccess) { l->buf[b] = nullptr; l->err = "hipMalloc failed (Inception activations)"; return PF_ERR_HIP; }
        l->allocs.push_back(l->buf[b]); l->cap[b] = p.buf_floats[b];
    }
    std::vector<hipEvent_t> ev;
    auto mark = [&] { if (l->profile) { hipEvent_t e; hipEventCreate(&e); hipEventRecord(e, s); ev.push_back(e); } };
    l->op_name.clear(); l->op_ms.clear(); l->op_flops.clear();
    mark();
    {
        const size_t n = (size_t)B * p.H0 * p.W0;
        hipLaunchKernelGGL(inc_front_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, img, l->buf[BUF_IN0], H, W, p.H0, p.W0, resize_input ? 1 : 0,
                           normalize_input ? 1 : 0, n);
        if (l->profile) { l->op_name.push_back("front"); l->op_flops.push_back(0.0); }
        mark();
    }
    for (const Op& o : p.ops) {
        if (o.kind == OP_CONV) {
            const Layer& L = layers()[o.layer];
            const LayerW& Wt = l->lw[o.layer];
            ConvArgs a;
            a.in = l->buf[o.src]; a.w = Wt.w; a.scale = Wt.scale; a.shift = Wt.shift; a.out = l->buf[o.dst];
            a.Hi = o.Hi; a.Wi = o.Wi; a.Ho = o.Ho; a.Wo = o.Wo; a.Cin = L.Cin; a.in_cs = o.src_cs; a.in_off = o.src_off; a.Cout = L.Cout; a.out_cs = o.dst_cs;
            a.out_off = o.dst_off; a.KH = L.KH; a.KW = L.KW; a.S = L.S; a.PH = L.PH; a.PW = L.PW; a.K = L.KH * L.KW * L.Cin; a.Kp = packed_k(L); a.M = B * o.Ho * o.Wo;
            if (const char* why = launch_conv(a, o.tile, s)) { l->err = std::string(why) + " (" + L.name + ")"; return PF_ERR_INVALID; }
            if (l->profile) { l->op_name.push_back(L.name); l->op_flops.push_back(2.0 * a.M * a.K * a.Cout); }
        } else {
            launch_pool(o.kind, l->buf[o.src], o.src_cs, o.src_off, l->buf[o.dst], o.dst_cs, o.dst_off, B, o.C, o.Hi, o.Wi, o.Ho, o.Wo, s);
            if (l->profile) { l->op_name.push_back(o.kind == OP_AVGPOOL_S1 ? "avgpool" : "maxpool"); l->op_flops.push_back(0.0); }
        }
        mark();
    }
    hipLaunchKernelGGL(inc_gap_kernel, dim3((p.out_C + 63) / 64, B), dim3(256), 0, s, l->buf[p.out_buf], p.out_C, p.out_C, p.out_H * p.out_W, out);
    if (l->profile) { l->op_name.push_back("global_average"); l->op_flops.push_back(0.0); }
    mark();
    if (hipGetLastError() != hipSuccess) { l->err = "Inception kernel launch failed"; return PF_ERR_HIP; }
    if (l->profile) {
        hipError_t e = hipStreamSynchronize(s);
        for (size_t i = 0; i + 1 < ev.size(); ++i) { float ms = 0.f; hipEventElapsedTime(&ms, ev[i], ev[i + 1]); l->op_ms.push_back(ms); }
        for (hipEvent_t x : ev) hipEventDestroy(x);
        if (e != hipSuccess) { l->err = "Inception forward failed on the device"; return PF_ERR_HIP; }
    }
    return PF_OK;
}

int pf_inception_num_layers(void) { return (int)layers().size(); }

int pf_inception_layer(int index, char* name, int name_cap, int32_t* dims) {
    if (index < 0 || index >= (int)layers().size() || !name || !dims || name_cap < 1) return PF_ERR_INVALID;
    const Layer& L = layers()[index];
    const size_t c = std::min(L.name.size(), (size_t)name_cap - 1);
    std::copy(L.name.begin(), L.name.begin() + c, name); name[c] = 0;
    const int32_t v[7] = {L.Cin, L.Cout, L.KH, L.KW, L.S, L.PH, L.PW};
    std::copy(v, v + 7, dims);
    return PF_OK;
}

int pf_inception_profile(pf_inception* l, int enable) {
    if (!l) return PF_ERR_INVALID;
    l->profile = enable != 0;
    return PF_OK;
}

int pf_inception_profile_read(pf_inception* l, int index, char* name, int name_cap, float* ms, double* flops) {
    if (!l || !name || !ms || !flops || name_cap < 1) return PF_ERR_INVALID;
    if (index < 0 || index >= (int)l->op_ms.size()) return PF_ERR_INVALID;
    const std::string& n = l->op_name[index];
    const size_t c = std::min(n.size(), (size_t)name_cap - 1);
    std::copy(n.begin(), n.begin() + c, name); name[c] = 0;
    *ms = l->op_ms[index]; *flops = l->op_flops[index];
    return PF_OK;
}

int pf_inception_conv(const float* in, const float* host_weight, const float* scale, const float* shift, float* out, int B, int Hi, int Wi, int Cin, int Cout,
                      int KH, int KW, int stride, int pad_h, int pad_w, int out_off, int out_cs, int tile, void* stream) {
    if (!in || !host_weight || !scale || !shift || !out || B <= 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad_h < 0 || pad_w < 0)
        return PF_ERR_INVALID;
    const int Ho = conv_out(Hi, KH, stride, pad_h), Wo = conv_out(Wi, KW, stride, pad_w);
    if (Hi + 2 * pad_h < KH || Wi + 2 * pad_w < KW || Ho < 1 || Wo < 1) return PF_ERR_INVALID;
    if ((long long)B * std::max(Hi, Ho) * std::max(Wi, Wo) > (1ll << 31) / 64 || (long long)KH * KW * Cin > (1ll << 24)) return PF_ERR_INVALID;
    if (tile >= NUM_TILES) return PF_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const std::vector<float> packed = pack_weight(host_weight, Cout, Cin, KH, KW);
    float* dw = nullptr;
    if (hipMalloc(&dw, packed.size() * sizeof(float)) != hipSuccess) return PF_ERR_HIP;
    int rc = PF_OK;
    if (hipMemcpy(dw, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = PF_ERR_HIP;
    if (rc == PF_OK) {
        ConvArgs a;
        a.in = in; a.w = dw; a.scale = scale; a.shift = shift; a.out = out;
        a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.Cin = Cin; a.in_cs = Cin; a.in_off = 0; a.Cout = Cout; a.out_cs = out_cs; a.out_off = out_off;
        a.KH = KH; a.KW = KW; a.S = stride; a.PH = pad_h; a.PW = pad_w; a.K = KH * KW * Cin; a.Kp = (a.K + KC - 1) / KC * KC; a.M = B * Ho * Wo;
        if (launch_conv(a, tile < 0 ? choose_tile(a.M, Cout) : tile, s) != nullptr) rc = PF_ERR_INVALID;
        else if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) rc = PF_ERR_HIP;       // the packed weights are freed below: wait for the launch
    }
    hipFree(dw);
    return rc;
}

int pf_inception_pool(const float* in, float* out, int B, int C, int Hi, int Wi, int kind, int in_off, int in_cs, int out_off, int out_cs, void* stream) {
    if (!in || !out || B <= 0 || C <= 0 || Hi <= 0 || Wi <= 0 || kind < OP_MAXPOOL_S2 || kind > OP_MAXPOOL_S1) return PF_ERR_INVALID;
    if (in_off < 0 || in_off + C > in_cs || out_off < 0 || out_off + C > out_cs) return PF_ERR_INVALID;
    const int Ho = kind == OP_MAXPOOL_S2 ? conv_out(Hi, 3, 2, 0) : Hi, Wo = kind == OP_MAXPOOL_S2 ? conv_out(Wi, 3, 2, 0) : Wi;
    if (Hi < (kind == OP_MAXPOOL_S2 ? 3 : 1) || Wi < (kind == OP_MAXPOOL_S2 ? 3 : 1)) return PF_ERR_INVALID;
    launch_pool(kind, in, in_cs, in_off, out, out_cs, out_off, B, C, Hi, Wi, Ho, Wo, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_HIP;
}

int pf_inception_front(const float* img, float* out, int B, int H, int W, int resize_input, int normalize_input, void* stream) {
    if (!img || !out || B <= 0 || H <= 0 || W <= 0) return PF_ERR_INVALID;
    const int Ho = resize_input ? INC_SIDE : H, Wo = resize_input ? INC_SIDE : W;
    const size_t n = (size_t)B * Ho * Wo;
    hipLaunchKernelGGL(inc_front_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, out, H, W, Ho, Wo, resize_input ? 1 : 0,
                       normalize_input ? 1 : 0, n);
    return hipGetLastError() == hipSuccess ? PF_OK : PF_ERR_HIP;
}
