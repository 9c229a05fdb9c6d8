// extern "C" wrappers around pnpflow_amd/csrc/conv_route.h for tests/test_conv_route_host.py (plain host C++17, no HIP).
#include <cstring>

#include "conv_route.h"

namespace {

// shape: 15 ints (nseg, B, H, W, Hs, Ws, Cout, out_cstride, res_cstride, gn_C, residual, addvec, coef, scale, gnb), then 3 segments of 11 ints
// (C, cstride, taps, xform, w_mode, has_w16, has_w16_src, src_lo, src_hi, src_O, src_kk)
pf::RouteShape shape_of(const int* v) {
    pf::RouteShape s;
    s.nseg = v[0]; s.B = v[1]; s.H = v[2]; s.W = v[3]; s.Hs = v[4]; s.Ws = v[5]; s.Cout = v[6]; s.out_cstride = v[7]; s.res_cstride = v[8]; s.gn_C = v[9];
    s.residual = v[10] != 0; s.addvec = v[11] != 0; s.coef = v[12] != 0; s.scale = v[13] != 0; s.gnb = v[14] != 0;
    for (int i = 0; i < 3; ++i) {
        const int* q = v + 15 + 11 * i; pf::RouteSeg& g = s.seg[i];
        g.C = q[0]; g.cstride = q[1]; g.taps = q[2]; g.xform = q[3]; g.w_mode = q[4]; g.has_w16 = q[5] != 0; g.has_w16_src = q[6] != 0;
        g.src_lo = q[7]; g.src_hi = q[8]; g.src_O = q[9]; g.src_kk = q[10];
    }
    return s;
}
pf::RouteEnv env_of(const int* v) { pf::RouteEnv e; e.cu_grid = v[0]; e.pp = v[1]; e.sp = v[2]; e.dma = v[3]; e.upphase = v[4]; return e; }

}  // namespace

extern "C" {

// out: 24 values (family, terms, MT, NT, WM, WN, S, UP, BM, KC, n9, n1, teams, nsplit, res, gnb, grid_x, grid_y, xcd_map, lds_bytes, csv_code, refused != nullptr);
// pre-filled by the caller, every one is overwritten
void cr_route(const int* shape, int stride, int up, int terms, const int* env, long long* out) {
    const pf::ConvRoute r = pf::conv_route(shape_of(shape), stride, up, terms, env_of(env));
    const long long v[22] = {(long long)r.family, r.terms, r.MT, r.NT, r.WM, r.WN, r.S, r.UP, r.BM, r.KC, r.n9, r.n1, r.teams, r.nsplit, r.res, r.gnb,
                             r.grid_x, r.grid_y, r.xcd_map, (long long)r.lds_bytes, r.csv_code, r.refused != nullptr};
    std::memcpy(out, v, sizeof(v));
}
int cr_phase_ok(const int* shape, int terms, const int* env) { return pf::conv_route_phase_ok(shape_of(shape), terms, env_of(env)) ? 1 : 0; }

// the byte counts the kernels use (the same constexpr functions conv_pp.hip / conv_sp.hip include)
int cr_pp_w9(int terms) { return pf::pp_w9(terms); }
int cr_pp_w1(int terms) { return pf::pp_w1(terms); }
int cr_pp_patch() { return pf::pp_patch_bytes(pf::PP_MT); }
int cr_sp_lds(int MT, int NT, int terms) { return pf::sp_lds(MT, NT, terms); }
int cr_family(int which) {
    const pf::ConvFamily f[5] = {pf::ConvFamily::MFMA32, pf::ConvFamily::MFMA16, pf::ConvFamily::DMA, pf::ConvFamily::PP, pf::ConvFamily::SP};
    return (int)f[which];
}

}  // extern "C"
