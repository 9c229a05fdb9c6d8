// The engine's random numbers: Philox4x32-10 words and their Box-Muller normals (restated in oracle/pnpflow_oracle.py).  Device code only;
// shared by pointwise.hip (the fills, the interpolation noise) and flow_solvers.hip (the rectified-flow sampler's in-kernel draw).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pf {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                               uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ float4 normal4(uint64_t q, uint64_t seed, uint64_t stream) {
    uint32_t r[4];
    philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)stream, (uint32_t)(stream >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
    const float k = 2.3283064365386963e-10f;  // 2^-32
    const float u0 = ((float)r[0] + 0.5f) * k, u1 = ((float)r[1] + 0.5f) * k;
    const float u2 = ((float)r[2] + 0.5f) * k, u3 = ((float)r[3] + 0.5f) * k;
    const float rad0 = sqrtf(-2.0f * logf(u0)), rad1 = sqrtf(-2.0f * logf(u2));
    float s0, c0, s1, c1;
    sincosf(6.283185307179586f * u1, &s0, &c0);
    sincosf(6.283185307179586f * u3, &s1, &c1);
    return make_float4(rad0 * c0, rad0 * s0, rad1 * c1, rad1 * s1);
}

// normals number [first, first+4) of stream `stream` (normal number e = component e%4 of Philox counter e/4): a shard of a
// multi-GPU run passes first = elem_offset + 4*q, so that it draws exactly the numbers the single-device run at the global
// batch size draws for the same images
__device__ __forceinline__ void normals_at(uint64_t first, uint64_t seed, uint64_t stream, float e[4]) {
    const uint64_t q0 = first >> 2; const int r = (int)(first & 3);
    const float4 a = normal4(q0, seed, stream);
    if (r == 0) { e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w; return; }
    const float4 b2 = normal4(q0 + 1, seed, stream);
    const float v[8] = {a.x, a.y, a.z, a.w, b2.x, b2.y, b2.z, b2.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = v[r + j];
}

}  // namespace pf
