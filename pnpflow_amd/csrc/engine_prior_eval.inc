// engine_prior_eval.inc -- what looks at the flow prior itself, on the engine; included at the end of engine.hip.
//
// pf_flow_divergence         value of the Hutchinson trace estimator (pnpflow/utils.py:243-270): eps . (J eps) = eps . (J^T eps), one retained
//                            forward, one backward with vec = eps, a deterministic per-image dot product.
// pf_flow_ode_euler          torchdiffeq's fixed-grid euler (FLOW_MATCHING.generate_samples, pnpflow/train_flow_matching.py:170-198).
// pf_flow_likelihood_rk45    the augmented solve of get_likelihood_fn_rf (image_generation/likelihood.py:172-193) under SciPy's RK45 step
//                            control (rk45_control.h): x in fp32, the B log-densities in fp64 on the device, time and step in fp64 on the host.

struct PriorEvalState {
    int B = 0; size_t n = 0;
    float *y = nullptr, *y1 = nullptr, *stage = nullptr, *k[7] = {}, *g = nullptr;     // [B n]; g: J^T eps (and pf_flow_divergence's v when v_out is NULL: stage)
    float* t = nullptr;                                                               // [B]
    double* dbl = nullptr;       // [7][B] stage divergences, [2][B] logp, [B][64] per-image partials, [64] norm partials, [2] norm sums
    DevBufs mem;
    double* kdiv(int j) const { return dbl + (size_t)j * B; }
    double* logp(int i) const { return dbl + (size_t)(7 + i) * B; }
    double* part() const { return dbl + (size_t)9 * B; }
    double* npart() const { return dbl + (size_t)(9 + 64) * B; }
    double* red() const { return npart() + 64; }
    void reset(pf_engine* e) { mem.release(e); *this = PriorEvalState{}; }
};

// `solve`: the state and stage buffers of the likelihood solve as well (pf_flow_divergence and the sampler need g, stage, t and the doubles only)
static int ensure_prior(pf_engine* e, int B, size_t n, bool solve) {
    if (!e->prior) e->prior = new PriorEvalState();
    PriorEvalState* st = e->prior;
    if (st->B == B && st->n == n && (!solve || st->y)) return PF_OK;
    if (st->B != B || st->n != n) st->reset(e);
    const size_t tot = (size_t)B * n;
    int rc = PF_OK;
    auto get = [&](auto** p, size_t count) { if (rc == PF_OK) rc = st->mem.alloc4(e, p, count); };
    if (!st->g) {
        get(&st->g, tot); get(&st->stage, tot); get(&st->t, (size_t)B); get(&st->dbl, 2 * ((size_t)(9 + 64) * B + 64 + 2));
    }
    if (solve && !st->y) {       // added to the live set
        get(&st->y, tot); get(&st->y1, tot);
        for (float*& k : st->k) get(&k, tot);
    }
    if (rc != PF_OK) { st->reset(e); return rc; }
    st->B = B; st->n = n;
    return PF_OK;
}

#define PE_LAUNCH(what, call) do { hipError_t _r = (call); if (_r != hipSuccess) { e->err = std::string("prior_eval ") + what + ": " + hipGetErrorString(_r); return PF_ERR_HIP; } } while (0)

static int prior_begin(pf_engine* e, const char* who, size_t& n) {
    if (!e->finalized) { e->err = "weights not finalized"; return PF_ERR_STATE; }
    if (e->cfg.output_channels != e->cfg.input_channels) { e->err = std::string(who) + " needs output_channels == input_channels"; return PF_ERR_INVALID; }
    n = (size_t)e->cfg.input_channels * e->cfg.input_height * e->cfg.input_height;
    if (n % 4) { e->err = std::string(who) + ": C*H*W must be a multiple of 4"; return PF_ERR_INVALID; }
    return PF_OK;
}

// v = v(x, t) (retained), g = J^T eps, div[b] = eps_b . g_b
static int enqueue_divergence(pf_engine* e, Plan* pr, const float* x, const float* t, const float* eps, float* v, double* div, hipStream_t s) {
    PriorEvalState* st = e->prior;
    int rc = run_plan(e, pr, x, t, v, s, e->solver_time_scale);
    if (rc != PF_OK) return rc;
    if ((rc = run_backward(e, pr, eps, st->g, s)) != PF_OK) return rc;
    PE_LAUNCH("divergence", launch_image_dot(eps, st->g, st->part(), div, st->B, (int64_t)st->n, s));
    return PF_OK;
}

extern "C" {

int pf_flow_divergence(pf_engine* e, const float* x, const float* t, const float* eps, float* v_out, double* div_out, int B, void* stream) {
    if (!e || !x || !t || !eps || !div_out || B <= 0) return PF_ERR_INVALID;
    size_t n = 0;
    int rc = prior_begin(e, "flow_divergence", n);
    if (rc != PF_OK) return rc;
    USE_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ensure_prior(e, B, n, false)) != PF_OK) return rc;
    PriorEvalState* st = e->prior;
    Plan* pr = nullptr;
    if ((rc = build_plan(e, B, true, &pr)) != PF_OK) return rc;
    e->retained_B = B; e->retained_plan = pr;          // after the call: the retained forward is that of (x, t)
    return enqueue_divergence(e, pr, x, t, eps, v_out ? v_out : st->stage, div_out, s);
}

int pf_flow_ode_euler(pf_engine* e, const float* host_t, int n_points, const float* x_in, float* x_out, int B, void* stream) {
    if (!e || !host_t || !x_in || !x_out || B <= 0) return PF_ERR_INVALID;
    if (n_points < 2) { e->err = "flow_ode_euler: the time grid needs at least 2 points"; return PF_ERR_INVALID; }
    size_t n = 0;
    int rc = prior_begin(e, "flow_ode_euler", n);
    if (rc != PF_OK) return rc;
    USE_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ensure_prior(e, B, n, false)) != PF_OK) return rc;
    PriorEvalState* st = e->prior;
    Plan* plan = nullptr;
    if ((rc = build_plan(e, B, false, &plan)) != PF_OK) return rc;
    const int64_t tot = (int64_t)B * (int64_t)n;
    if (x_out != x_in) HIPCHK(e, hipMemcpyAsync(x_out, x_in, (size_t)tot * 4, hipMemcpyDeviceToDevice, s));
    for (int i = 0; i + 1 < n_points; ++i) {
        const float dt = host_t[i + 1] - host_t[i];
        PE_LAUNCH("time", launch_fill(st->t, B, host_t[i], s));
        if ((rc = run_plan(e, plan, x_out, st->t, st->stage, s, e->solver_time_scale)) != PF_OK) return rc;
        PE_LAUNCH("euler step", launch_dflow_axpy(x_out, st->stage, x_out, dt, tot, s));          // y0 + dt * f0, multiply and add apart
    }
    return PF_OK;
}

int pf_flow_likelihood_rk45(pf_engine* e, const pf_likelihood_params* prm, const float* x_in, const float* eps, float* z_out, double* delta_logp,
                            float* bpd, int64_t* stats, int B, void* stream) {
    if (!e || !prm || !x_in || !eps || !z_out || !delta_logp || B <= 0) return PF_ERR_INVALID;
    if (!(prm->rtol > 0) || !(prm->atol > 0) || !(prm->t0 != prm->t1) || !std::isfinite(prm->t0) || !std::isfinite(prm->t1) || prm->max_attempts <= 0) {
        e->err = "likelihood_rk45: rtol, atol > 0, finite t0 != t1 and max_attempts > 0 required"; return PF_ERR_INVALID;
    }
    size_t n = 0;
    int rc = prior_begin(e, "likelihood_rk45", n);
    if (rc != PF_OK) return rc;
    USE_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ensure_prior(e, B, n, true)) != PF_OK) return rc;
    PriorEvalState* st = e->prior;
    Plan* pr = nullptr;
    if ((rc = build_plan(e, B, true, &pr)) != PF_OK) return rc;
    e->retained_B = B; e->retained_plan = pr;          // after the call: the retained forward of the last evaluation
    const int64_t tot = (int64_t)B * (int64_t)n;
    const double atol = prm->atol, rtol = prm->rtol, count = (double)tot + (double)B;
    const double interval = std::fabs(prm->t1 - prm->t0), dir = prm->t1 > prm->t0 ? 1.0 : -1.0;
    float* y = st->y; float* y1 = st->y1;
    float* k[7]; double* kd[7];
    for (int j = 0; j < 7; ++j) { k[j] = st->k[j]; kd[j] = st->kdiv(j); }
    double* logp = st->logp(0); double* logp1 = st->logp(1);
    int64_t nfev = 0;
    auto eval = [&](const float* yi, double t, int j) -> int {          // k[j] = v(yi, t), kd[j] = eps . J^T eps
        PE_LAUNCH("time", launch_fill(st->t, B, (float)t, s));
        ++nfev;
        return enqueue_divergence(e, pr, yi, st->t, eps, k[j], kd[j], s);
    };
    // RMS over the B*n + B entries: the x part from rk_norm4 (a - b, or the error combination `xe`), the logp part from rk_aug
    auto rms = [&](const float* a, const float* b, const float* ya, const float* yb, const RkTerms& xe, const RkAug& aug, double* lp_new, double& out) -> int {
        PE_LAUNCH("norm", launch_rk_norm(a, b, ya, yb, xe, (float)atol, (float)rtol, st->npart(), st->red(), tot, s));
        PE_LAUNCH("norm", launch_rk_aug(aug, logp, lp_new, atol, rtol, st->red(), st->red() + 1, B, s));
        double sum = 0.0;
        HIPCHK(e, hipMemcpyAsync(&sum, st->red() + 1, sizeof sum, hipMemcpyDeviceToHost, s));
        HIPCHK(e, hipStreamSynchronize(s));
        out = std::sqrt(sum / count);
        return PF_OK;
    };
    const RkTerms none{};
    HIPCHK(e, hipMemcpyAsync(y, x_in, (size_t)tot * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipMemsetAsync(logp, 0, (size_t)B * sizeof(double), s));
    if ((rc = eval(y, prm->t0, 0)) != PF_OK) return rc;                     // f0
    // select_initial_step: d0 = rms(y0 / scale), d1 = rms(f0 / scale), the probe, d2 = rms((f1 - f0) / scale) / h0
    double d0, d1, d2;
    { RkAug a{}; if ((rc = rms(y, nullptr, y, nullptr, none, a, nullptr, d0)) != PF_OK) return rc; }          // logp0 = 0 adds nothing
    { RkAug a{}; a.n = 1; a.k[0] = kd[0]; a.err[0] = 1.0; if ((rc = rms(k[0], nullptr, y, nullptr, none, a, nullptr, d1)) != PF_OK) return rc; }
    const double h0 = rk45::initial_probe_step(d0, d1, interval);
    { RkTerms c{}; c.n = 1; c.k[0] = k[0]; c.c[0] = (float)(h0 * dir); PE_LAUNCH("initial step", launch_rk_combine(y, c, st->stage, tot, s)); }
    if ((rc = eval(st->stage, prm->t0 + h0 * dir, 1)) != PF_OK) return rc;
    { RkAug a{}; a.n = 2; a.k[0] = kd[0]; a.k[1] = kd[1]; a.err[0] = -1.0; a.err[1] = 1.0;
      if ((rc = rms(k[1], k[0], y, nullptr, none, a, nullptr, d2)) != PF_OK) return rc; }
    d2 /= h0;
    if (!std::isfinite(d0) || !std::isfinite(d1) || !std::isfinite(d2)) { e->err = "likelihood_rk45: non-finite state or velocity at t0"; return PF_ERR_NUMERIC; }
    rk45::Controller ctl(prm->t0, prm->t1, rk45::initial_step(h0, d1, d2, interval), prm->max_attempts);
    for (;;) {
        const rk45::Status bs = ctl.begin();
        if (bs == rk45::FINISHED) break;
        if (bs != rk45::RUNNING) {
            char buf[240];
            snprintf(buf, sizeof buf, "likelihood_rk45: %s at t = %.9g (|h| = %.3g, %lld accepted, %lld rejected); no result",
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
        RkTerms xe{}; xe.n = 7; RkAug a{}; a.n = 7;
        for (int j = 0; j < 7; ++j) {
            xe.k[j] = k[j]; xe.c[j] = (float)(rk45::E[j] * h);
            a.k[j] = kd[j]; a.err[j] = rk45::E[j] * h; a.step[j] = j < 6 ? rk45::B[j] * h : 0.0;
        }
        double norm;
        if ((rc = rms(nullptr, nullptr, y, y1, xe, a, logp1, norm)) != PF_OK) return rc;
        bool ok = false;
        if (ctl.end(norm, &ok) == rk45::NON_FINITE) {
            e->err = "likelihood_rk45: non-finite error norm (the state, the velocity or the divergence is not finite)"; return PF_ERR_NUMERIC;
        }
        if (ok) { std::swap(y, y1); std::swap(logp, logp1); std::swap(k[0], k[6]); std::swap(kd[0], kd[6]); }      // FSAL
    }
    HIPCHK(e, hipMemcpyAsync(z_out, y, (size_t)tot * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipMemcpyAsync(delta_logp, logp, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (bpd) PE_LAUNCH("bits/dim", launch_bpd_finish(y, logp, st->part(), bpd, prm->offset, B, (int64_t)n, s));
    if (stats) { stats[0] = ctl.accepted; stats[1] = ctl.rejected; stats[2] = nfev; }
    HIPCHK(e, hipStreamSynchronize(s));
    return check_flags(e);
}

}  // extern "C"
