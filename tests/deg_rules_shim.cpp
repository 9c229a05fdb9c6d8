// extern "C" view of pnpflow_amd/csrc/deg_rules.h for tests/test_deg_rules_host.py (host clang++ only, loaded with ctypes).  With -DDEG_RULES_MAIN the
// file is a program that walks the test's grid once (built with -fsanitize=address,undefined) and prints how many points each predicate accepts.
#include <cstdio>

#include "deg_rules.h"

using namespace pf;

namespace {
DegView view(int kind, int sf, int ntaps, int has_taps, int has_mask) {
    static const float taps_stand_in = 0.f; static const uint8_t mask_stand_in = 0;      // never dereferenced
    pf_degradation d{};
    d.kind = kind; d.half_size_mask = 10; d.sf = sf; d.ntaps = ntaps; d.mask = has_mask ? &mask_stand_in : nullptr; d.taps = has_taps ? &taps_stand_in : nullptr;
    return to_view(&d);
}
}  // namespace

extern "C" {
int dr_sizeof_view() { return (int)sizeof(DegView); }
// the text of the broken rule, or NULL
const char* dr_rule(int kind, int sf, int ntaps, int has_taps, int has_mask, int H, int W) { return deg_rule_violation(view(kind, sf, ntaps, has_taps, has_mask), H, W); }
// the measurement's side; -1 where the rules refuse the operator (deg_out_side is defined after them only)
int dr_out_side(int kind, int sf, int ntaps, int has_taps, int has_mask, int H, int W, int side) {
    const DegView d = view(kind, sf, ntaps, has_taps, has_mask);
    return deg_rule_violation(d, H, W) ? -1 : deg_out_side(d, side);
}
int dr_solve(int kind) { return (int)deg_solve(kind); }
int dr_solve_ok(int kind, int sf, int ntaps, int has_taps, int has_mask, int H, int W) { return deg_solve_violation(view(kind, sf, ntaps, has_taps, has_mask), H, W) == nullptr; }
int dr_sr_solve_shape_ok(int kind, int sf, int ntaps, int has_taps, int has_mask, int H, int W) { return sr_solve_shape_ok(view(kind, sf, ntaps, has_taps, has_mask), H, W); }
int dr_psf_taps_ok(int kind, int sf, int ntaps, int has_taps, int H, int W) { return psf_taps_ok(view(kind, sf, ntaps, has_taps, 0), H, W); }
size_t dr_sr_scratch(int B, int C, int H, int W, int sf) { return sr_solve_scratch_floats(B, C, H, W, sf); }
size_t dr_ode_scratch(int solve, int B, int C, int H, int W, int sf) { return deg_ode_scratch_floats((DegSolve)solve, B, C, H, W, sf); }
}

#ifdef DEG_RULES_MAIN
int main() {
    const int sfs[] = {0, 1, 2, 3, 8, 9, 16}, nts[] = {0, 1, 3, 4, 9, 63, 65, 127, 128}, hw[][2] = {{8, 8}, {64, 64}, {80, 90}, {2048, 2048}, {2049, 64}};
    long points = 0, ok = 0, solve_ok = 0, sr_ok = 0, sides = 0;
    for (int kind = -1; kind <= 10; ++kind) for (int sf : sfs) for (int nt : nts) for (int bits = 0; bits < 4; ++bits) for (auto& s : hw) {
        ++points;
        ok += dr_rule(kind, sf, nt, bits & 1, bits >> 1, s[0], s[1]) == nullptr;
        solve_ok += dr_solve_ok(kind, sf, nt, bits & 1, bits >> 1, s[0], s[1]);
        sr_ok += dr_sr_solve_shape_ok(kind, sf, nt, bits & 1, bits >> 1, s[0], s[1]);
        sides += dr_out_side(kind, sf, nt, bits & 1, bits >> 1, s[0], s[1], s[0]) + dr_solve(kind) + dr_psf_taps_ok(kind, sf, nt, bits & 1, s[0], s[1]);
    }
    for (int sf : {1, 2, 4, 8}) for (int solve = 0; solve <= 4; ++solve) sides += (long)(dr_ode_scratch(solve, 32, 3, 256, 256, sf) & 1);
    printf("%ld %ld %ld %ld %ld\n", points, ok, solve_ok, sr_ok, sides);
    return 0;
}
#endif
