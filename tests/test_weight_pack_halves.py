"""CPU test of the N-half weight images of conv_sp's 256-channel form (wpack::chunk_sp with an output-row offset, weight_pack.h).

A 256-channel conv runs as two 128-channel problems over the same pixels; workgroups of half h read, per 16-channel K-chunk, the image
of output rows [128 h, 128 h + 128).  That image must be byte for byte what chunk_sp gives for the 128-row slice of the weight alone
(whose layout test_weight_pack.py::test_chunk_sp checks against the documented formula) - for the split images (terms 3) and the
hi-only ones (terms 1), at a first, a middle and the last chunk of the input channels.  tests/weight_pack_halves_shim.cpp (the one
extern "C" wrapper this needs) is compiled with ROCm's host clang++ like the shim of test_weight_pack.py; a missing compiler is a failure.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_weight_pack import CSRC, ROOT, _host_clang, call, same_bytes, weight


@pytest.fixture(scope="module")
def wph(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("weight_pack_halves") / "libweight_pack_halves_shim.so")
    cmd = [_host_clang(), "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + CSRC, "-o", so, os.path.join(ROOT, "tests", "weight_pack_halves_shim.cpp")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, "weight_pack.h must compile as plain host C++17:\n" + res.stderr
    lib = C.CDLL(so)
    lib.wp_chunk_sp_rows.restype = C.c_size_t
    return lib


@pytest.mark.parametrize("terms", [3, 1])
@pytest.mark.parametrize("kk", [9, 1])
@pytest.mark.parametrize("I,lo", [(48, 0), (48, 16), (48, 32)])
def test_chunk_sp_of_a_row_half_equals_chunk_sp_of_the_row_slice(wph, I, lo, kk, terms):
    w = weight(256, I, kk, seed=7 + I + lo + kk)
    images = []
    for row0 in (0, 128):
        got = call(wph.wp_chunk_sp_rows, w, lo, 4, terms, row0, dtype=np.float16)
        want = call(wph.wp_chunk_sp_rows, w[row0:row0 + 128], lo, 4, terms, 0, dtype=np.float16)      # the 128-row slice as a weight of its own
        assert got.size == kk * (1 if terms == 1 else 2) * 4 * 512
        same_bytes(got, want)
        images.append(got)
    # the two halves are different images (a packer that ignored the offset would pass the first half alone)
    assert (images[0].view(np.uint16) != images[1].view(np.uint16)).any()
