// extern "C" wrapper around pnpflow_amd/csrc/adam_step.h for tests/test_flow_priors_host.py: compiled as plain host C++17 (no HIP), the
// same text the device kernels of flow_priors.hip execute.
#include <stdint.h>
#include "adam_step.h"

extern "C" void adam_step_array(float* x, float* m, float* v, const float* g, int64_t n, double lr, double beta1, double beta2, double eps, int step) {
    const pf::AdamCoef c = pf::adam_coef(lr, beta1, beta2, eps, step);
    for (int64_t i = 0; i < n; ++i) pf::adam_step(x[i], m[i], v[i], g[i], c);
}
