// adam_step.h -- the Adam update of ONE element, as torch.optim.Adam's single-tensor form with non-capturable (scalar) steps computes it
// (torch/optim/adam.py _single_tensor_adam, amsgrad / weight_decay / maximize off).  Plain C++: the Flow-Priors kernels (flow_priors.hip)
// and the host test (tests/adam_step_shim.cpp) compile this same text; no HIP header is needed on the host path.
//
//   exp_avg.lerp_(grad, 1 - beta1)                          m += w (g - m), w = fp32(1 - beta1) < 0.5: the small-weight branch of lerp
//   exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)  v = fp32(beta2 v) + (fp32(1 - beta2) g) g, every product rounded
//   denom = (exp_avg_sq.sqrt() / sqrt(bc2)).add_(eps)       bc1 = 1 - beta1^step, bc2 = 1 - beta2^step in double on the host, as torch
//   param.addcdiv_(exp_avg, denom, value=-(lr / bc1))       x += (fp32(-lr / bc1) m) / denom
// Division and square root are the correctly rounded ones (hipcc's default for fp32; no fast-math anywhere in the build).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PF_ADAM_HD __host__ __device__ inline
#else
#define PF_ADAM_HD inline
#endif

namespace pf {

struct AdamCoef {
    float w1;           // fp32(1 - beta1): the lerp weight
    float beta2;        // fp32(beta2)
    float w2;           // fp32(1 - beta2)
    float bc2_sqrt;     // fp32(sqrt(1 - beta2^step))
    float neg_step;     // fp32(-(lr / (1 - beta1^step)))
    float eps;          // fp32(eps)
};

// the scalars of optimiser step `step` (1-based), in double as torch's Python computes them, then rounded once to fp32 as its kernels do
inline AdamCoef adam_coef(double lr, double beta1, double beta2, double eps, int step) {
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    AdamCoef c;
    c.w1 = (float)(1.0 - beta1); c.beta2 = (float)beta2; c.w2 = (float)(1.0 - beta2);
    c.bc2_sqrt = (float)sqrt(bc2); c.neg_step = (float)(-(lr / bc1)); c.eps = (float)eps;
    return c;
}

PF_ADAM_HD void adam_step(float& x, float& m, float& v, float g, const AdamCoef& c) {
#pragma clang fp contract(off)
    m = fmaf(c.w1, g - m, m);                       // lerp, |weight| < 0.5 (ATen Lerp.h: self + weight * diff, an fma in its vector form)
    v = c.beta2 * v + (c.w2 * g) * g;
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    x = x + (c.neg_step * m) / denom;
}

}  // namespace pf
