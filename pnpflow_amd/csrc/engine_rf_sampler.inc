// engine_rf_sampler.inc -- drawing samples from a rectified-flow prior, on the engine; included at the end of engine.hip after
// engine_prior_eval.inc, whose state (PriorEvalState), prior_begin and PE_LAUNCH it shares.
//
// pf_rf_euler_sampler    euler_sampler of pnpflow/image_generation/sampling.py:69-109 and RectifiedFlow.euler_ode (sde_lib.py:75-94): N
//                        evaluations on the grid num_t = i/N (t_end - t_begin) + t_begin with the step dt = 1/N - NOT the grid spacing
//                        (t_end - t_begin)/N: the reference's quirk, kept - and the Euler-Maruyama form when sigma_var > 0.
// pf_flow_ode_rk45       the plain-state solve dx/dt = v(x, t) under SciPy's RK45 step control (rk45_control.h): rk45_sampler
//                        (sampling.py:111-153) and RectifiedFlow.ode (sde_lib.py:37-72), either direction.
// Either net: the label the net sees is t * e->solver_time_scale (999 for NCSN++, 1 for the U-Net).

extern "C" {

int pf_rf_euler_sampler(pf_engine* e, const pf_rf_sampler_params* prm, const float* x_in, const float* noise, float* x_out, int B, void* stream) {
    if (!e || !prm || !x_in || !x_out || B <= 0) return PF_ERR_INVALID;
    if (prm->n_steps < 1 || !(prm->sigma_var >= 0) || !(prm->noise_scale > 0) || !std::isfinite(prm->sigma_var) || !std::isfinite(prm->noise_scale) ||
        !std::isfinite(prm->t_begin) || !std::isfinite(prm->t_end) || !(prm->t_begin != prm->t_end)) {
        e->err = "rf_euler_sampler: n_steps >= 1, sigma_var >= 0, noise_scale > 0 and finite t_begin != t_end required"; return PF_ERR_INVALID;
    }
    const int N = prm->n_steps;
    const double dt = 1.0 / N;
    // the scalars of every step, before anything is launched (sampling.py:94-105, in Python's double arithmetic and order)
    std::vector<float> label((size_t)N);
    std::vector<RfStepCoef> coef((size_t)N);
    for (int i = 0; i < N; ++i) {
        const double num_t = (double)i / N * (prm->t_end - prm->t_begin) + prm->t_begin;
        const double sigma_t = (1.0 - num_t) * prm->sigma_var;
        RfStepCoef& c = coef[(size_t)i];
        label[(size_t)i] = (float)num_t;
        c.dt = (float)dt;
        c.c0 = c.a1 = c.a2 = c.s = 0.f;
        if (prm->sigma_var > 0) {
            const double c0 = (sigma_t * sigma_t) / (2.0 * (prm->noise_scale * prm->noise_scale) * ((1.0 - num_t) * (1.0 - num_t)));
            if (!std::isfinite(c0)) {
                char buf[200];
                snprintf(buf, sizeof buf, "rf_euler_sampler: step %d is at num_t = %.9g, where the noise term divides by (1 - num_t)^2 = 0", i, num_t);
                e->err = buf; return PF_ERR_INVALID;
            }
            c.c0 = (float)c0; c.a1 = (float)(0.5 * num_t * (1.0 - num_t)); c.a2 = (float)(0.5 * (2.0 - num_t)); c.s = (float)(sigma_t * std::sqrt(dt));
        }
    }
    size_t n = 0;
    int rc = prior_begin(e, "rf_euler_sampler", n);
    if (rc != PF_OK) return rc;
    USE_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ensure_prior(e, B, n, false)) != PF_OK) return rc;
    PriorEvalState* st = e->prior;
    Plan* plan = nullptr;
    if ((rc = build_plan(e, B, false, &plan)) != PF_OK) return rc;
    const int64_t tot = (int64_t)B * (int64_t)n;
    if (x_out != x_in) HIPCHK(e, hipMemcpyAsync(x_out, x_in, (size_t)tot * 4, hipMemcpyDeviceToDevice, s));
    for (int i = 0; i < N; ++i) {          // nothing synchronises: label, forward, fused update
        PE_LAUNCH("time", launch_fill(st->t, B, label[(size_t)i], s));
        if ((rc = run_plan(e, plan, x_out, st->t, st->stage, s, e->solver_time_scale)) != PF_OK) return rc;
        const uint64_t first = (uint64_t)i * (uint64_t)tot;
        PE_LAUNCH("sampler step", launch_rf_euler_step(x_out, st->stage, noise ? noise + (size_t)first : nullptr, coef[(size_t)i], prm->seed, prm->stream_id,
                                                       first, tot, s));
    }
    return PF_OK;
}

int pf_flow_ode_rk45(pf_engine* e, const pf_rk45_params* prm, const float* x_in, float* x_out, int64_t* stats, int B, void* stream) {
    if (!e || !prm || !x_in || !x_out || B <= 0) return PF_ERR_INVALID;
    if (!(prm->rtol > 0) || !(prm->atol > 0) || !(prm->t0 != prm->t1) || !std::isfinite(prm->t0) || !std::isfinite(prm->t1) || prm->max_attempts <= 0) {
        e->err = "flow_ode_rk45: rtol, atol > 0, finite t0 != t1 and max_attempts > 0 required"; return PF_ERR_INVALID;
    }
    size_t n = 0;
    int rc = prior_begin(e, "flow_ode_rk45", n);
    if (rc != PF_OK) return rc;
    USE_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ensure_prior(e, B, n, true)) != PF_OK) return rc;
    PriorEvalState* st = e->prior;
    Plan* plan = nullptr;
    if ((rc = build_plan(e, B, false, &plan)) != PF_OK) return rc;
    const int64_t tot = (int64_t)B * (int64_t)n;
    const double atol = prm->atol, rtol = prm->rtol, count = (double)tot;      // SciPy sees the batch as ONE vector: one norm, one step sequence
    const double interval = std::fabs(prm->t1 - prm->t0), dir = prm->t1 > prm->t0 ? 1.0 : -1.0;
    float* y = st->y; float* y1 = st->y1;
    float* k[7];
    for (int j = 0; j < 7; ++j) k[j] = st->k[j];
    int64_t nfev = 0;
    auto eval = [&](const float* yi, double t, int j) -> int {          // k[j] = v(yi, t)
        PE_LAUNCH("time", launch_fill(st->t, B, (float)t, s));
        ++nfev;
        return run_plan(e, plan, yi, st->t, k[j], s, e->solver_time_scale);
    };
    // RMS over the B*n entries of a - b (or of the error combination `xe`) against atol + rtol max(|ya|, |yb|): one 8-byte readback
    auto rms = [&](const float* a, const float* b, const float* ya, const float* yb, const RkTerms& xe, double& out) -> int {
        PE_LAUNCH("norm", launch_rk_norm(a, b, ya, yb, xe, (float)atol, (float)rtol, st->npart(), st->red(), tot, s));
        double sum = 0.0;
        HIPCHK(e, hipMemcpyAsync(&sum, st->red(), sizeof sum, hipMemcpyDeviceToHost, s));
        HIPCHK(e, hipStreamSynchronize(s));
        out = std::sqrt(sum / count);
        return PF_OK;
    };
    const RkTerms none{};
    HIPCHK(e, hipMemcpyAsync(y, x_in, (size_t)tot * 4, hipMemcpyDeviceToDevice, s));
    if ((rc = eval(y, prm->t0, 0)) != PF_OK) return rc;                     // f0
    double d0, d1, d2;                                                      // select_initial_step
    if ((rc = rms(y, nullptr, y, nullptr, none, d0)) != PF_OK) return rc;
    if ((rc = rms(k[0], nullptr, y, nullptr, none, d1)) != PF_OK) return rc;
    const double h0 = rk45::initial_probe_step(d0, d1, interval);
    { RkTerms c{}; c.n = 1; c.k[0] = k[0]; c.c[0] = (float)(h0 * dir); PE_LAUNCH("initial step", launch_rk_combine(y, c, st->stage, tot, s)); }
    if ((rc = eval(st->stage, prm->t0 + h0 * dir, 1)) != PF_OK) return rc;
    if ((rc = rms(k[1], k[0], y, nullptr, none, d2)) != PF_OK) return rc;
    d2 /= h0;
    if (!std::isfinite(d0) || !std::isfinite(d1) || !std::isfinite(d2)) { e->err = "flow_ode_rk45: non-finite state or velocity at t0"; return PF_ERR_NUMERIC; }
    rk45::Controller ctl(prm->t0, prm->t1, rk45::initial_step(h0, d1, d2, interval), prm->max_attempts);
    for (;;) {
        const rk45::Status bs = ctl.begin();
        if (bs == rk45::FINISHED) break;
        if (bs != rk45::RUNNING) {
            char buf[240];
            snprintf(buf, sizeof buf, "flow_ode_rk45: %s at t = %.9g (|h| = %.3g, %lld accepted, %lld rejected); no result",
                     bs == rk45::ATTEMPT_CAP ? "the cap of max_attempts attempts was exceeded" : "the step size fell below 10 ulp of t", ctl.t, ctl.h_abs,
                     (long long)ctl.accepted, (long long)ctl.rejected);
            e->err = buf; return PF_ERR_NUMERIC;
        }
        const double h = ctl.h;
        for (int sg = 1; sg <= rk45::kStages; ++sg) {          // stages 1..5, then y_new and its velocity (FSAL)
            RkTerms c{}; c.n = sg;
            const bool last = sg == rk45::kStages;
            for (int j = 0; j < sg; ++j) { c.k[j] = k[j]; c.c[j] = (float)((last ? rk45::B[j] : rk45::A[sg][j]) * h); }
            float* yi = last ? y1 : st->stage;
            PE_LAUNCH("stage", launch_rk_combine(y, c, yi, tot, s));
            if ((rc = eval(yi, ctl.t + (last ? 1.0 : rk45::C[sg]) * h, sg)) != PF_OK) return rc;
        }
        RkTerms xe{}; xe.n = 7;
        for (int j = 0; j < 7; ++j) { xe.k[j] = k[j]; xe.c[j] = (float)(rk45::E[j] * h); }
        double norm;
        if ((rc = rms(nullptr, nullptr, y, y1, xe, norm)) != PF_OK) return rc;
        bool ok = false;
        if (ctl.end(norm, &ok) == rk45::NON_FINITE) { e->err = "flow_ode_rk45: non-finite error norm (the state or the velocity is not finite)"; return PF_ERR_NUMERIC; }
        if (ok) { std::swap(y, y1); std::swap(k[0], k[6]); }      // FSAL
    }
    HIPCHK(e, hipMemcpyAsync(x_out, y, (size_t)tot * 4, hipMemcpyDeviceToDevice, s));
    if (stats) { stats[0] = ctl.accepted; stats[1] = ctl.rejected; stats[2] = nfev; }
    HIPCHK(e, hipStreamSynchronize(s));
    return check_flags(e);
}

}  // extern "C"
