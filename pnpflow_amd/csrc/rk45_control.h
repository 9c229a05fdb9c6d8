// Host-only step control of scipy.integrate.RK45 (scipy/integrate/_ivp/common.py select_initial_step, _ivp/rk.py RungeKutta._step_impl,
// _ivp/ivp.py solve_ivp's loop), restated.  Plain C++17, no HIP, no engine state - engine_prior_eval.inc drives the likelihood solve
// with it, tests/test_prior_eval_host.py drives a numpy system with it and compares the accepted times and the attempt count with
// solve_ivp's own.
//
// Time and step are fp64.  One attempt = begin() (the signed step h and the end time t_new, clipped so that the last step ends exactly on
// t_bound - there is no dense output), the caller's six stage evaluations and its RMS error norm over the whole state vector with
// scale = atol + rtol max(|y|, |y_new|), then end(norm).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

namespace rk45 {

// Dormand-Prince 5(4) as SciPy tabulates it (rk.py class RK45): stage s is evaluated at t + C[s] h, y + h sum_j A[s][j] K[j];
// y_new = y + h sum_j B[j] K[j]; K[6] = f(t + h, y_new) (FSAL); error estimate h sum_j E[j] K[j].
constexpr int kStages = 6;
constexpr double C[6] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0};
constexpr double A[6][5] = {
    {0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
constexpr double B[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
constexpr double E[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};

constexpr double kSafety = 0.9, kMinFactor = 0.2, kMaxFactor = 10.0, kErrorExponent = -1.0 / 5;      // error_estimator_order 4

// select_initial_step, first half: the probe step.  d0 = rms(y0 / scale), d1 = rms(f0 / scale), scale = atol + |y0| rtol.
inline double initial_probe_step(double d0, double d1, double interval) {
    const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    return std::min(h0, interval);
}
// second half: d2 = rms((f(t0 + h0 dir, y0 + h0 dir f0) - f0) / scale) / h0  ->  the first step's absolute size
inline double initial_step(double h0, double d1, double d2, double interval) {
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? std::max(1e-6, h0 * 1e-3) : std::pow(0.01 / std::max(d1, d2), 1.0 / 5);
    return std::min({100.0 * h0, h1, interval});
}

enum Status { RUNNING = 0, FINISHED = 1, STEP_TOO_SMALL = -1, ATTEMPT_CAP = -2, NON_FINITE = -3 };

struct Controller {
    double t, t_bound, dir, h_abs;
    int64_t max_attempts;
    int64_t accepted = 0, rejected = 0;
    double h = 0.0, t_new = 0.0;     // the open attempt
    double min_step = 0.0;
    bool in_step = false;            // an attempt of the current step was made (and rejected)
    bool step_rejected = false;

    Controller(double t0, double t_end, double h_abs0, int64_t max_attempts_)
        : t(t0), t_bound(t_end), dir(t_end >= t0 ? 1.0 : -1.0), h_abs(h_abs0), max_attempts(max_attempts_) {}

    // opens the next attempt (h, t_new); FINISHED once t has reached t_bound; the errors are final
    Status begin() {
        if (dir * (t - t_bound) >= 0) return FINISHED;
        if (accepted + rejected >= max_attempts) return ATTEMPT_CAP;
        if (!in_step) {      // a new step: SciPy lifts a too small proposal to min_step once, a rejection below it fails
            min_step = 10.0 * std::fabs(std::nextafter(t, dir * std::numeric_limits<double>::infinity()) - t);
            if (h_abs < min_step) h_abs = min_step;
            step_rejected = false;
            in_step = true;
        }
        if (h_abs < min_step) return STEP_TOO_SMALL;
        h = h_abs * dir;
        t_new = t + h;
        if (dir * (t_new - t_bound) > 0) t_new = t_bound;
        h = t_new - t;
        h_abs = std::fabs(h);
        return RUNNING;
    }

    // closes the open attempt with its error norm; *was_accepted tells whether the state advances to t_new
    Status end(double error_norm, bool* was_accepted) {
        *was_accepted = false;
        if (!std::isfinite(error_norm)) return NON_FINITE;
        if (error_norm < 1.0) {
            double factor = error_norm == 0.0 ? kMaxFactor : std::min(kMaxFactor, kSafety * std::pow(error_norm, kErrorExponent));
            if (step_rejected) factor = std::min(1.0, factor);
            h_abs *= factor;
            t = t_new;
            ++accepted;
            in_step = false;
            *was_accepted = true;
        } else {
            h_abs *= std::max(kMinFactor, kSafety * std::pow(error_norm, kErrorExponent));
            ++rejected;
            step_rejected = true;
        }
        return RUNNING;
    }
};

}  // namespace rk45
