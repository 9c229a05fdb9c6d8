// extern "C" view of pnpflow_amd/csrc/weight_pack.h for tests/test_weight_pack.py (host clang++ only, loaded with ctypes).
// Every wrapper returns the image's size in bytes and copies it to `out` when `cap` holds it.
#include <cstring>

#include "weight_pack.h"

namespace {
template <class V> size_t give(const V& img, void* out, size_t cap) {
    const size_t bytes = img.size() * sizeof(img[0]);
    if (out && bytes <= cap) memcpy(out, img.data(), bytes);
    return bytes;
}
}  // namespace

extern "C" {
void wp_split16(float w, unsigned short* hi_lo) { const wpack::Split s = wpack::split16(w); memcpy(hi_lo, &s.hi, 2); memcpy(hi_lo + 1, &s.lo, 2); }
size_t wp_frag32(const float* w, int O, int I, int kk, int lo, int hi, void* out, size_t cap) { return give(wpack::frag32({w, O, I, kk}, lo, hi), out, cap); }
size_t wp_slice16(const float* w, int O, int I, int kk, int lo, int hi, int terms, void* out, size_t cap) { return give(wpack::slice16({w, O, I, kk}, lo, hi, terms), out, cap); }
size_t wp_chunk_pp(const float* w, int O, int I, int kk, int lo, void* out, size_t cap) { return give(wpack::chunk_pp({w, O, I, kk}, lo), out, cap); }
size_t wp_chunk_sp(const float* w, int O, int I, int kk, int lo, int NT, int terms, void* out, size_t cap) { return give(wpack::chunk_sp({w, O, I, kk}, lo, NT, terms), out, cap); }
size_t wp_edge_frag(const float* w, int O, int I, int kk, int begin, void* out, size_t cap) { return give(wpack::edge_frag({w, O, I, kk}, begin != 0), out, cap); }
size_t wp_adjoint(const float* w, int O, int I, int kk, int lo, int hi, void* out, size_t cap) { return give(wpack::adjoint({w, O, I, kk}, lo, hi), out, cap); }
size_t wp_phase_sums(const float* w, int O, int I, int kk, void* out, size_t cap) { return give(wpack::phase_sums({w, O, I, kk}), out, cap); }
}
