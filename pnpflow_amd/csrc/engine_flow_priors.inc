// engine_flow_priors.inc -- Flow-Priors (pnpflow/methods/flow_priors.py) on the engine; included at the end of engine.hip.
//
// The method differentiates the Hutchinson trace term eps . J(x) eps with respect to x.  For a fixed probe
//   grad_x (eps . J(x) eps) = d/ds [ J(x + s eps)^T eps ] at s = 0,
// the directional derivative along eps of the first-order VJP the engine has; a central difference of two VJPs at x +- h eps gives it to
// O(h^2) (DESIGN.md section 11).  One inner step is three retained forward + backward pairs:
//   pred = v(x, t), w = H_adj(seed(H(x + pred dt) - y_next)), jw = J(x)^T w;  jp = J(x + h eps)^T eps;  jm = J(x - h eps)^T eps
//   g = (w + dt jw) + dt (jp - jm) / (2 h) + (x on outer iteration 0, grad_xt_lik afterwards), then one Adam step on x.
//
// pf_adam_step            the bare optimiser kernel (adam_step.h)
// pf_flow_priors_grad     one gradient evaluation, no update
// pf_flow_priors_restore  outer iterations [first, stop) of the N x K loop: per outer iteration a fresh Adam state, K inner steps, then the
//                         Euler update x += v(x, t) dt.  Every scalar of an iteration is a kernel argument computed on the host before its
//                         launches; nothing synchronises or reads back inside the loop.

struct FlowPriorsState {
    int B = 0; size_t n = 0, ny = 0;
    float *x = nullptr, *xi = nullptr, *pred = nullptr, *w = nullptr, *jw = nullptr, *xp = nullptr, *xm = nullptr, *jp = nullptr, *jm = nullptr,
          *ep = nullptr, *m = nullptr, *v = nullptr;                                  // [B n]
    float *y = nullptr, *hx = nullptr, *hxi = nullptr, *sd = nullptr;              // [B ny]
    float *scr = nullptr;                                                          // [2 B n]: H / H_adj scratch
    float *t = nullptr;                                                            // [B]
    DevBufs mem;
    void reset(pf_engine* e) { mem.release(e); *this = FlowPriorsState{}; }
};

static int ensure_fprior(pf_engine* e, int B, size_t n, size_t ny) {
    if (!e->fprior) e->fprior = new FlowPriorsState();
    FlowPriorsState* st = e->fprior;
    if (st->B == B && st->n == n && st->ny == ny) return PF_OK;
    st->reset(e);
    const size_t tot = (size_t)B * n, toty = (size_t)B * ny;
    int rc = PF_OK;
    auto get = [&](auto** p, size_t count) { if (rc == PF_OK) rc = st->mem.alloc4(e, p, count); };
    for (float** p : {&st->x, &st->xi, &st->pred, &st->w, &st->jw, &st->xp, &st->xm, &st->jp, &st->jm, &st->ep, &st->m, &st->v}) get(p, tot);
    for (float** p : {&st->y, &st->hx, &st->hxi, &st->sd}) get(p, toty);
    get(&st->scr, 2 * tot); get(&st->t, (size_t)B);
    if (rc != PF_OK) { st->reset(e); return rc; }
    st->B = B; st->n = n; st->ny = ny;
    return PF_OK;
}

#define FP_LAUNCH(what, call) do { hipError_t _r = (call); if (_r != hipSuccess) { e->err = std::string("flow_priors ") + what + ": " + hipGetErrorString(_r); return PF_ERR_HIP; } } while (0)

// the scalars of outer iteration i, with the reference's own expressions (flow_priors.py:63-69, 83-85, 96, 137): Python doubles first, then the
// fp32 roundings torch applies (a Python scalar meets an fp32 tensor as fp32)
struct FpSched { float t, tn, omt, coef; FlowPriorsCoef c; };
static FpSched fp_schedule(const pf_flow_priors_params* prm, int i) {
    const double eps0 = prm->start_time > 0.0 ? prm->start_time : 1e-3;
    const double dt = prm->start_time > 0.0 ? (1.0 - eps0) / prm->N : 1.0 / prm->N;
    const double num_t = (double)i / prm->N * (1.0 - eps0) + eps0;
    FpSched sc{};
    sc.t = (float)num_t;
    sc.tn = sc.t + (float)dt;              // t + dt on the fp32 tensor t
    sc.omt = 1.0f - sc.tn;
    sc.coef = prm->noise_model == 1 ? (float)prm->lmbda : (float)(2.0 * prm->lmbda);
    sc.c.dt = (float)dt; sc.c.fd = (float)(dt / (2.0 * prm->fd_step)); sc.c.num_t = (float)num_t; sc.c.lik = (float)(-1.0 / (1.0 - num_t));
    sc.c.first = i == 0 ? 1 : 0;
    return sc;
}

// one inner step at st->x with the probe `eps`: the three VJPs, then the gradient (written to the out_* that are given) and, with `adam`, the update
static int enqueue_fp_step(pf_engine* e, Plan* pr, const DegView& dv, const pf_flow_priors_params* prm, const FpSched& sc, const float* eps, const AdamCoef* adam,
                           float* out_g, float* out_g_data, float* out_g_trace, hipStream_t s) {
    FlowPriorsState* st = e->fprior;
    const int B = st->B, C = e->cfg.input_channels, H = e->cfg.input_height;
    const int64_t tot = (int64_t)B * (int64_t)st->n, toty = (int64_t)B * (int64_t)st->ny;
    const float ts = (float)prm->time_scale;
    int rc = run_plan(e, pr, st->x, st->t, st->pred, s, ts);
    if (rc != PF_OK) return rc;
    if (dv.kind == DEG_DENOISE || dv.kind == DEG_BOX || dv.kind == DEG_MASK) {
        FP_LAUNCH("residual", launch_fp_residual(dv, st->x, st->pred, st->y, st->hxi, st->w, sc.c.dt, sc.tn, sc.omt, sc.coef, prm->noise_model, B, C, H, H, s));
    } else {
        FP_LAUNCH("x_next", launch_fp_axpy(st->x, st->pred, st->xp, sc.c.dt, tot, s));          // xp: free until the probe shift
        FP_LAUNCH("H", launch_deg_H(dv, st->xp, st->hx, B, C, H, H, st->scr, s));
        FP_LAUNCH("seed", launch_fp_seed(st->hx, st->y, st->hxi, st->sd, sc.tn, sc.omt, sc.coef, prm->noise_model, toty, s));
        FP_LAUNCH("H_adj", launch_deg_Hadj(dv, st->sd, st->w, B, C, H, H, st->scr, s));
    }
    if ((rc = run_backward(e, pr, st->w, st->jw, s)) != PF_OK) return rc;
    FP_LAUNCH("probe shift", launch_fp_shift(st->x, eps, st->xp, st->xm, (float)prm->fd_step, tot, s));
    if ((rc = run_plan(e, pr, st->xp, st->t, st->jp, s, ts)) != PF_OK) return rc;                  // (the velocity itself is not needed: jp is overwritten)
    if ((rc = run_backward(e, pr, eps, st->jp, s)) != PF_OK) return rc;
    if ((rc = run_plan(e, pr, st->xm, st->t, st->jm, s, ts)) != PF_OK) return rc;
    if ((rc = run_backward(e, pr, eps, st->jm, s)) != PF_OK) return rc;
    FP_LAUNCH("gradient", launch_fp_grad_adam(sc.c, adam, st->w, st->jw, st->jp, st->jm, st->pred, st->x, st->m, st->v, out_g, out_g_data, out_g_trace, nullptr, tot, s));
    return PF_OK;
}

// argument checks shared by the two solver calls; fills n, ny
static int fp_begin(pf_engine* e, const pf_degradation* d, const pf_flow_priors_params* prm, int B, size_t& n, size_t& ny) {
    if (!e->finalized) { e->err = "weights not finalized"; return PF_ERR_STATE; }
    if (e->cfg.output_channels != e->cfg.input_channels) { e->err = "flow_priors needs output_channels == input_channels"; return PF_ERR_INVALID; }
    if (prm->N < 1 || prm->K < 1) { e->err = "flow_priors: N >= 1 and K >= 1 required"; return PF_ERR_INVALID; }
    if (!(prm->fd_step > 0.0) || !std::isfinite(prm->fd_step)) { e->err = "flow_priors: fd_step (the finite-difference step h) must be positive"; return PF_ERR_INVALID; }
    if (!(prm->start_time < 1.0)) { e->err = "flow_priors: start_time must be below 1"; return PF_ERR_INVALID; }
    if (prm->noise_model != 0 && prm->noise_model != 1) { e->err = "flow_priors: noise_model must be 0 (gaussian) or 1 (laplace)"; return PF_ERR_INVALID; }
    if (!(prm->time_scale > 0.0)) { e->err = "flow_priors: time_scale must be positive (1 for the OT net, 999 for NCSN++)"; return PF_ERR_INVALID; }
    if (!(prm->lmbda >= 0.0) || !(prm->eta >= 0.0)) { e->err = "flow_priors: lmbda and eta must not be negative"; return PF_ERR_INVALID; }
    // a plan is built per batch size on first use; what no plan can be built for is refused here, before anything is allocated
    if (B < 1 || B > 65535) { e->err = "flow_priors: batch " + std::to_string(B) + " is not one the engine plans for (1..65535 images)"; return PF_ERR_INVALID; }
    const int C = e->cfg.input_channels, H = e->cfg.input_height;
    int Hy = 0;
    const int rc = check_operator(e, "flow_priors", d, H, Hy);
    if (rc != PF_OK) return rc;
    n = (size_t)C * H * H; ny = (size_t)C * Hy * Hy;
    if (n % 4) { e->err = "flow_priors: C*H*W must be a multiple of 4"; return PF_ERR_INVALID; }
    return PF_OK;
}

extern "C" {

int pf_adam_step(float* x, float* m, float* v, const float* g, int64_t n, double lr, double beta1, double beta2, double eps, int step, void* stream) {
    if (!x || !m || !v || !g || n <= 0 || step < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return PF_ERR_INVALID;
    LAUNCHCHK(launch_adam_step(adam_coef(lr, beta1, beta2, eps, step), x, m, v, g, n, (hipStream_t)stream));
    return PF_OK;
}

int pf_flow_priors_grad(pf_engine* e, const pf_degradation* d, const pf_flow_priors_params* prm, const float* x, const float* x_init, const float* y,
                        const float* eps, int iteration, float* out_g, float* out_g_data, float* out_g_trace, float* out_pred, int B, void* stream) {
    if (!e) return PF_ERR_INVALID;
    if (!d || !prm || !x || !x_init || !y || !eps) { e->err = "flow_priors_grad: null argument"; return PF_ERR_INVALID; }
    size_t n = 0, ny = 0;
    int rc = fp_begin(e, d, prm, B, n, ny);
    if (rc != PF_OK) return rc;
    if (iteration < 0 || iteration >= prm->N) { e->err = "flow_priors_grad: iteration must be in [0, N)"; return PF_ERR_INVALID; }
    USE_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ensure_fprior(e, B, n, ny)) != PF_OK) return rc;
    FlowPriorsState* st = e->fprior;
    Plan* pr = nullptr;
    if ((rc = build_plan(e, B, true, &pr)) != PF_OK) return rc;
    e->retained_B = B; e->retained_plan = pr;          // after the call: the retained forward is that of (x - h eps, t)
    const DegView dv = to_view(d);
    const int C = e->cfg.input_channels, H = e->cfg.input_height;
    const size_t tot = (size_t)B * n, toty = (size_t)B * ny;
    const FpSched sc = fp_schedule(prm, iteration);
    HIPCHK(e, hipMemcpyAsync(st->x, x, tot * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipMemcpyAsync(st->y, y, toty * 4, hipMemcpyDeviceToDevice, s));
    FP_LAUNCH("H(x_init)", launch_deg_H(dv, x_init, st->hxi, B, C, H, H, st->scr, s));
    FP_LAUNCH("time", launch_fill(st->t, B, sc.t, s));
    if ((rc = enqueue_fp_step(e, pr, dv, prm, sc, eps, nullptr, out_g, out_g_data, out_g_trace, s)) != PF_OK) return rc;
    if (out_pred) HIPCHK(e, hipMemcpyAsync(out_pred, st->pred, tot * 4, hipMemcpyDeviceToDevice, s));
    return PF_OK;
}

int pf_flow_priors_restore(pf_engine* e, const pf_degradation* d, const pf_flow_priors_params* prm, const float* y, const float* x_init, const float* eps_or_null,
                           float* x_inout, int B, void* stream) {
    if (!e) return PF_ERR_INVALID;
    if (!d || !prm || !y || !x_init || !x_inout) { e->err = "flow_priors_restore: null argument"; return PF_ERR_INVALID; }
    size_t n = 0, ny = 0;
    int rc = fp_begin(e, d, prm, B, n, ny);
    if (rc != PF_OK) return rc;
    const int first = prm->first, stop = prm->stop > 0 ? prm->stop : prm->N;
    if (first < 0 || first > stop || stop > prm->N) { e->err = "flow_priors_restore: 0 <= first <= stop <= N required"; return PF_ERR_INVALID; }
    USE_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = ensure_fprior(e, B, n, ny)) != PF_OK) return rc;
    FlowPriorsState* st = e->fprior;
    // the retained plan first (protected from eviction as e->retained_plan while the forward plan is fetched)
    Plan* pr = nullptr; Plan* pf = nullptr;
    if ((rc = build_plan(e, B, true, &pr)) != PF_OK) return rc;
    e->retained_B = B; e->retained_plan = pr;          // after the call: the retained forward of the last inner step's x - h eps
    if ((rc = build_plan(e, B, false, &pf)) != PF_OK) return rc;
    const DegView dv = to_view(d);
    const int C = e->cfg.input_channels, H = e->cfg.input_height;
    const size_t tot = (size_t)B * n, toty = (size_t)B * ny;
    HIPCHK(e, hipMemcpyAsync(st->x, first == 0 ? x_init : x_inout, tot * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipMemcpyAsync(st->y, y, toty * 4, hipMemcpyDeviceToDevice, s));
    FP_LAUNCH("H(x_init)", launch_deg_H(dv, x_init, st->hxi, B, C, H, H, st->scr, s));
    for (int i = first; i < stop; ++i) {
        const FpSched sc = fp_schedule(prm, i);
        FP_LAUNCH("time", launch_fill(st->t, B, sc.t, s));
        HIPCHK(e, hipMemsetAsync(st->m, 0, tot * 4, s));          // a fresh torch.optim.Adam per outer iteration (flow_priors.py:89)
        HIPCHK(e, hipMemsetAsync(st->v, 0, tot * 4, s));
        for (int k = 0; k < prm->K; ++k) {
            const int64_t slot = (int64_t)i * prm->K + k;
            const float* eps;
            if (eps_or_null) eps = eps_or_null + (size_t)(slot - (int64_t)first * prm->K) * tot;
            else { FP_LAUNCH("probe", launch_fill_rademacher(st->ep, (int64_t)tot, prm->seed, prm->stream_base + (uint64_t)slot, 0, s)); eps = st->ep; }
            const AdamCoef ac = adam_coef(prm->eta, 0.9, 0.999, 1e-8, k + 1);
            if ((rc = enqueue_fp_step(e, pr, dv, prm, sc, eps, &ac, nullptr, nullptr, nullptr, s)) != PF_OK) return rc;
        }
        if ((rc = run_plan(e, pf, st->x, st->t, st->pred, s, (float)prm->time_scale)) != PF_OK) return rc;
        FP_LAUNCH("euler step", launch_fp_axpy(st->x, st->pred, st->x, sc.c.dt, (int64_t)tot, s));          // x + pred * dt: the product, then the sum
    }
    HIPCHK(e, hipMemcpyAsync(x_inout, st->x, tot * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipStreamSynchronize(s));
    return check_flags(e);
}

}  // extern "C"
