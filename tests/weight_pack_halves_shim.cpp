// extern "C" view of wpack::chunk_sp with its output-row offset (pnpflow_amd/csrc/weight_pack.h) for tests/test_weight_pack_halves.py
// (host clang++ only, loaded with ctypes).  Returns the image's size in bytes and copies it to `out` when `cap` holds it.
#include <cstring>

#include "weight_pack.h"

extern "C" size_t wp_chunk_sp_rows(const float* w, int O, int I, int kk, int lo, int NT, int terms, int row0, void* out, size_t cap) {
    const auto img = wpack::chunk_sp({w, O, I, kk}, lo, NT, terms, row0);
    const size_t bytes = img.size() * sizeof(img[0]);
    if (out && bytes <= cap) memcpy(out, img.data(), bytes);
    return bytes;
}
