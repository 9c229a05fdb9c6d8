// deg_rules.h -- everything the host decides about a pf_degradation before a kernel sees it: when the operator may be applied to [B, C, H, W], the side of
// its measurement, which linear solve OT-ODE takes for it and how much scratch that solve needs.  Host-only (no HIP type, no device code), pinned on the CPU
// by tests/test_deg_rules_host.py.  A new kind adds: its DEG_ constant and static_assert, its row in deg_rule_violation, its family in deg_is_sr / deg_solve.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/pnpflow_hip.h"

namespace pf {

enum { DEG_DENOISE = 0, DEG_BOX = 1, DEG_MASK = 2, DEG_SR = 3, DEG_BLUR = 4, DEG_SR_FILTER = 5, DEG_BLUR_ZERO = 6 /* same taps, samples outside the image are 0 */,
       DEG_PSF_BLUR = 7 /* circular blur with a square 2-D point-spread function: ntaps = its side K (odd, <= PSF_MAX_SIDE), taps = [K][K] */,
       DEG_PSF_BLUR_ZERO = 8 /* the same taps, samples outside the image are 0 */,
       DEG_PSF_SR = 9 /* the circular blur of DEG_PSF_BLUR sampled at (i sf, j sf): y = (k (*) x) decimated by sf (1 .. PSF_SR_MAX_SF, dividing H and W) */ };
static_assert(DEG_DENOISE == PF_DEG_DENOISING && DEG_BOX == PF_DEG_BOX_INPAINTING && DEG_MASK == PF_DEG_MASK_INPAINTING && DEG_SR == PF_DEG_SUPERRESOLUTION &&
              DEG_BLUR == PF_DEG_GAUSSIAN_BLUR && DEG_SR_FILTER == PF_DEG_SR_FILTERED && DEG_BLUR_ZERO == PF_DEG_GAUSSIAN_BLUR_ZERO &&
              DEG_PSF_BLUR == PF_DEG_PSF_BLUR && DEG_PSF_BLUR_ZERO == PF_DEG_PSF_BLUR_ZERO && DEG_PSF_SR == PF_DEG_PSF_SR,
              "DEG_* (kernels) and PF_DEG_* (the ABI) name the same values of pf_degradation::kind");
constexpr int PSF_MAX_SIDE = 63;
constexpr int PSF_SR_MAX_SF = 8;
inline bool deg_is_psf(int kind) { return kind == DEG_PSF_BLUR || kind == DEG_PSF_BLUR_ZERO || kind == DEG_PSF_SR; }      // the kinds with [K][K] taps (psf_taps_ok)
inline bool deg_is_sr(int kind) { return kind == DEG_SR || kind == DEG_SR_FILTER || kind == DEG_PSF_SR; }                   // the measurement is [H / sf][W / sf]
inline bool deg_is_separable(int kind) { return kind == DEG_BLUR || kind == DEG_SR_FILTER || kind == DEG_BLUR_ZERO; }       // the kinds with [ntaps] 1-D taps

struct DegView {       // device-side view of pf_degradation; embedded in the cached graphs' keys, which are compared bytewise
    int kind, half, sf, ntaps;
    const uint8_t* mask;
    const float* taps;
};
static_assert(sizeof(DegView) == 32, "DegView is part of keys compared with memcmp: four ints and two pointers, no padding bytes");
inline DegView to_view(const pf_degradation* d) {
    DegView v{}; v.kind = d->kind; v.half = d->half_size_mask; v.sf = d->sf; v.ntaps = d->ntaps; v.mask = d->mask; v.taps = d->taps;
    return v;
}

// the 2-D point-spread-function kinds (psf.hip): K odd, 1 .. PSF_MAX_SIDE, device taps, and K <= min(H, W) for the circular kinds; DEG_PSF_SR also
// needs sf in 1 .. PSF_SR_MAX_SF dividing H and W
inline bool psf_taps_ok(const DegView& d, int H, int W) {
    if (!d.taps || d.ntaps < 1 || d.ntaps > PSF_MAX_SIDE || !(d.ntaps & 1)) return false;
    if (d.kind == DEG_PSF_SR) return d.sf >= 1 && d.sf <= PSF_SR_MAX_SF && H % d.sf == 0 && W % d.sf == 0 && d.ntaps <= std::min(H, W);
    return d.kind == DEG_PSF_BLUR_ZERO || (d.kind == DEG_PSF_BLUR && d.ntaps <= std::min(H, W));      // the circular filter must hold the kernel
}

// May H, H_adj or a gradient step of `d` be applied to [B, C, H, W]?  nullptr: yes; otherwise the rule that is broken, as a static text.  The separable
// kinds have no rule between ntaps and the image side (the pass form of blur2 takes K > N).  The kernels' launch geometry (BL_MAXW, B*C <= 65535, in != out,
// a scratch pointer) stays with the launchers.
inline const char* deg_rule_violation(const DegView& d, int H, int W) {
    if (d.kind < DEG_DENOISE || d.kind > DEG_PSF_SR) return "unknown degradation kind";
    if (deg_is_sr(d.kind) && (d.sf < 1 || H % d.sf || W % d.sf)) return "superresolution factor must divide the image size";
    if (deg_is_separable(d.kind) && (!d.taps || d.ntaps < 1 || d.ntaps > 127)) return "the filtered operators need 1..127 device taps";
    if (deg_is_psf(d.kind) && !psf_taps_ok(d, H, W))
        return "the point-spread-function kinds need a device [K][K] taps array with K odd, 1 .. 63, and K <= the image side for the circular kinds; "
               "PF_DEG_PSF_SR also needs sf in 1 .. 8 dividing the image side";
    if (d.kind == DEG_MASK && !d.mask) return "mask inpainting needs a device mask";
    return nullptr;
}

// the side of the measurement along an image side of `side` pixels (after deg_rule_violation: sf >= 1 for the decimating kinds)
inline int deg_out_side(const DegView& d, int side) { return deg_is_sr(d.kind) ? side / d.sf : side; }

// The linear solve (r_t^2 H H^T + sigma^2)^-1 OT-ODE takes for a kind (ot_ode.py:72-130)
enum class DegSolve {
    ClosedForm,           // H H^T is diagonal: identity, masks, plain decimation (launch_ot_ode_vec)
    FourierSeparable,     // circular Gaussian blur: the spectrum is the product of two 1-D tables (launch_ot_ode_vec_blur)
    Krylov,               // the zero-boundary blurs: no closed form, GMRES (launch_krylov_solve)
    FourierPsf,           // circular PSF blur: a 2-D spectrum table
    FourierLowRes         // blur, then decimate (DEG_SR_FILTER, DEG_PSF_SR): H H^T is circulant on the low-resolution grid
};
inline DegSolve deg_solve(int kind) {
    switch (kind) {
        case DEG_BLUR: return DegSolve::FourierSeparable;
        case DEG_BLUR_ZERO: case DEG_PSF_BLUR_ZERO: return DegSolve::Krylov;
        case DEG_PSF_BLUR: return DegSolve::FourierPsf;
        case DEG_SR_FILTER: case DEG_PSF_SR: return DegSolve::FourierLowRes;
        default: return DegSolve::ClosedForm;
    }
}
// deg_rule_violation plus what the kind's solve asks of the shape: the Fourier families transform lines of at most 2048 points, and their filter must fit the
// image (the PSF kinds' own rule already says so)
inline const char* deg_solve_violation(const DegView& d, int H, int W) {
    if (const char* m = deg_rule_violation(d, H, W)) return m;
    const DegSolve s = deg_solve(d.kind);
    if (s == DegSolve::ClosedForm || s == DegSolve::Krylov) return nullptr;
    if (H > 2048 || W > 2048) return "the Fourier solve needs H, W <= 2048";
    if (deg_is_separable(d.kind) && d.ntaps > std::min(H, W)) return "the Fourier solve needs a filter no longer than the image side";
    return nullptr;
}
inline bool sr_solve_shape_ok(const DegView& d, int H, int W) { return deg_solve(d.kind) == DegSolve::FourierLowRes && !deg_solve_violation(d, H, W); }

// The scratch of the blur-then-decimate solves, S = B C H W, Sl = S / sf^2 (the layout: SrScratch, fft2.hip):
//   [S] x1_hat | [2 S] the operator's own scratch | [Sl] H(.), then sol | (+ 1: up to the next 8-byte boundary) [2 Sl] complex plane | [Hl Wl] lam, or the
//   prox's B coefficients | the spectrum's source (launch_sr_aliased_spectrum's tmp)
inline size_t sr_prox_scratch_floats(int B, int C, int H, int W, int sf) {      // launch_fft_prox_sr's: up to the B coefficients (its lam is the caller's)
    const size_t S = (size_t)B * C * H * W, Sl = S / ((size_t)std::max(sf, 1) * std::max(sf, 1));
    return 3 * S + 3 * Sl + 1 + (size_t)B;
}
inline size_t sr_solve_scratch_floats(int B, int C, int H, int W, int sf) {
    sf = std::max(sf, 1);
    return sr_prox_scratch_floats(B, C, H, W, sf) + (size_t)(H / sf) * (W / sf) + std::max((size_t)H * W, 2 * ((size_t)H + W) + 2);
}
// floats of scratch one OT-ODE step needs: launch_ot_ode_vec_blur's of the Fourier families, one image batch (H / H_adj of the PSF kinds) beside the Krylov
// solve's own workspace
inline size_t deg_ode_scratch_floats(DegSolve solve, int B, int C, int H, int W, int sf) {
    const size_t S = (size_t)B * C * H * W;
    switch (solve) {
        case DegSolve::FourierSeparable: return 4 * S + (size_t)H + W;
        case DegSolve::FourierPsf: return 4 * S + (size_t)H * W;
        case DegSolve::Krylov: return S;
        case DegSolve::FourierLowRes: return sr_solve_scratch_floats(B, C, H, W, sf);
        case DegSolve::ClosedForm: break;
    }
    return 0;
}

}  // namespace pf
