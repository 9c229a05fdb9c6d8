// engine_dflow.inc -- D-Flow (pnpflow/methods/d_flow.py) and the dopri5 flow-ODE solve on the engine; included at the end of engine.hip.
//
// pf_d_flow_forward          T(z): steps_euler - 1 explicit midpoint steps of the velocity net (forward_flow_matching, d_flow.py:41-49)
// pf_d_flow_value_and_grad   one LBFGS closure (d_flow.py:110-121): the 10 forward evaluations of T (inputs saved), data term +
//                            regulariser, then the reverse sweep; each VJP re-runs its forward under the retained plan
//                            (checkpoint-and-recompute).  Captured once into a hipGraph, replayed on every closure.
// pf_flow_ode_dopri5         adaptive Dormand-Prince solve of dx/dt = v(x, t) (inverse_flow_matching, d_flow.py:51-60, torchdiffeq
//                            dopri5 rules); host step control, one 8-byte device-to-host read of the error ratio per attempt.

struct DFlowState {
    // buffers of one (B, n, ny, M) configuration; M = steps_euler - 1 midpoint steps
    int B = 0; size_t n = 0, ny = 0; int M = 0;
    float *zs = nullptr;      // [M][B n]: z_0 .. z_{M-1} (z_0: the closure's latent)
    float *us = nullptr;      // [M][B n]: u_i = z_i + delta/2 v(z_i, t_i)
    float *zT = nullptr, *v = nullptr, *g = nullptr, *h = nullptr, *jg = nullptr, *grad = nullptr;   // [B n]
    float *y = nullptr, *hx = nullptr, *r2 = nullptr;    // [B ny]
    float *scr = nullptr;     // [2 B n]: H / H_adj scratch (blur, filtered SR)
    float *tab = nullptr;     // [2M][B]: t_i, then t_i + delta/2
    float *loss = nullptr, *coef = nullptr;              // [B]
    double* part = nullptr;   // [2][B][64]
    std::vector<float> host_tab;
    // cached graphs: T(z) and one closure
    struct FwdKey { const void* plan; int B, M; float delta, half_delta; int pad_; };
    struct VgKey { const void* plan_fwd; const void* plan_ret; DegView deg; int B, M; float delta, half_delta, lmbda; int pad_; };
    static_assert(sizeof(FwdKey) == sizeof(void*) + 6 * sizeof(int), "FwdKey is compared with memcmp: it must have no padding bytes");
    static_assert(sizeof(VgKey) == 4 * sizeof(void*) + 10 * sizeof(int), "VgKey is compared with memcmp: it must have no padding bytes");
    CachedGraph fgraph, vgraph;
    DevBufs mem;
    void reset(pf_engine* e) { fgraph.drop(e); vgraph.drop(e); /* their nodes point into the buffers */ mem.release(e); *this = DFlowState{}; }
};

// dopri5 state of one (B, n): a set of its own beside the closure's, allocated and released independently of it
struct DopriState {
    int B = 0; size_t n = 0;
    float *y = nullptr, *y1 = nullptr, *stage = nullptr, *k[7] = {}, *t = nullptr;
    double* part = nullptr;   // [64] partials + [1] sum
    DevBufs mem;
    void reset(pf_engine* e) { mem.release(e); *this = DopriState{}; }
};

static int ensure_dflow(pf_engine* e, int B, size_t n, size_t ny, int M) {
    if (!e->dflow) e->dflow = new DFlowState();
    DFlowState* st = e->dflow;
    if (st->B == B && st->n == n && st->ny == ny && st->M == M) return PF_OK;
    st->reset(e);
    const size_t tot = (size_t)B * n, toty = (size_t)B * ny;
    int rc = PF_OK;
    auto get = [&](auto** p, size_t count) { if (rc == PF_OK) rc = st->mem.alloc4(e, p, count); };
    for (float** p : {&st->zT, &st->v, &st->g, &st->h, &st->jg, &st->grad}) get(p, tot);
    get(&st->zs, (size_t)M * tot); get(&st->us, (size_t)M * tot);
    for (float** p : {&st->y, &st->hx, &st->r2}) get(p, toty);
    get(&st->scr, 2 * tot); get(&st->tab, (size_t)2 * M * B); get(&st->loss, B); get(&st->coef, B); get(&st->part, (size_t)2 * 2 * B * 64);
    if (rc != PF_OK) { st->reset(e); return rc; }
    st->B = B; st->n = n; st->ny = ny; st->M = M;
    return PF_OK;
}

static int ensure_dopri(pf_engine* e, int B, size_t n) {
    if (!e->dopri) e->dopri = new DopriState();
    DopriState* st = e->dopri;
    if (st->B == B && st->n == n) return PF_OK;
    st->reset(e);
    const size_t tot = (size_t)B * n;
    int rc = PF_OK;
    auto get = [&](auto** p, size_t count) { if (rc == PF_OK) rc = st->mem.alloc4(e, p, count); };
    for (float** p : {&st->y, &st->y1, &st->stage}) get(p, tot);
    for (float*& k : st->k) get(&k, tot);
    get(&st->t, B); get(&st->part, 2 * 72);
    if (rc != PF_OK) { st->reset(e); return rc; }
    st->B = B; st->n = n;
    return PF_OK;
}

static int dflow_check_prm(pf_engine* e, const pf_d_flow_params* prm) {
    if (prm->steps_euler < 2 || prm->steps_euler > 1024 || !prm->host_t || !prm->host_t_mid) {
        e->err = "d_flow: steps_euler must be in [2, 1024] and host_t / host_t_mid given"; return PF_ERR_INVALID;
    }
    return PF_OK;
}

// the B-expanded schedule table: uploaded when it differs from the one on the device (one captured graph serves every call)
static int dflow_upload_tab(pf_engine* e, const pf_d_flow_params* prm, int B, hipStream_t s) {
    DFlowState* st = e->dflow;
    const int M = st->M;
    std::vector<float> tab((size_t)2 * M * B);
    for (int i = 0; i < M; ++i)
        for (int b = 0; b < B; ++b) { tab[(size_t)i * B + b] = prm->host_t[i]; tab[(size_t)(M + i) * B + b] = prm->host_t_mid[i]; }
    if (tab != st->host_tab) {
        st->host_tab = tab;
        HIPCHK(e, hipMemcpyAsync(st->tab, st->host_tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
    }
    return PF_OK;
}

#define DF_LAUNCH(what, call) do { hipError_t _r = (call); if (_r != hipSuccess) { e->err = std::string("d_flow ") + what + ": " + hipGetErrorString(_r); return PF_ERR_HIP; } } while (0)

// z_0 = zs[0] -> zT:  u_i = z_i + delta/2 v(z_i, t_i);  z_{i+1} = z_i + delta v(u_i, t_i + delta/2)
static int enqueue_dflow_forward(pf_engine* e, Plan* plan, const pf_d_flow_params* prm, hipStream_t s) {
    DFlowState* st = e->dflow;
    const size_t tot = (size_t)st->B * st->n;
    for (int i = 0; i < st->M; ++i) {
        float* zi = st->zs + (size_t)i * tot; float* ui = st->us + (size_t)i * tot;
        float* znext = i + 1 < st->M ? st->zs + (size_t)(i + 1) * tot : st->zT;
        int rc = run_plan(e, plan, zi, st->tab + (size_t)i * st->B, st->v, s, e->solver_time_scale);
        if (rc != PF_OK) return rc;
        DF_LAUNCH("midpoint", launch_dflow_axpy(zi, st->v, ui, prm->half_delta, (int64_t)tot, s));
        if ((rc = run_plan(e, plan, ui, st->tab + (size_t)(st->M + i) * st->B, st->v, s, e->solver_time_scale)) != PF_OK) return rc;
        DF_LAUNCH("step", launch_dflow_axpy(zi, st->v, znext, prm->delta, (int64_t)tot, s));
    }
    return PF_OK;
}

static int enqueue_dflow_value_and_grad(pf_engine* e, Plan* pf, Plan* pr, const DegView& dv, const pf_d_flow_params* prm, float lmbda, hipStream_t s) {
    DFlowState* st = e->dflow;
    const int B = st->B, C = e->cfg.input_channels, H = e->cfg.input_height;
    const size_t tot = (size_t)B * st->n;
    int rc = enqueue_dflow_forward(e, pf, prm, s);
    if (rc != PF_OK) return rc;
    DF_LAUNCH("H", launch_deg_H(dv, st->zT, st->hx, B, C, H, H, st->scr, s));
    DF_LAUNCH("objective", launch_dflow_objective(st->hx, st->y, st->r2, st->zs, st->part, st->loss, st->coef, lmbda, B, (int64_t)st->ny, (int64_t)st->n, s));
    DF_LAUNCH("H_adj", launch_deg_Hadj(dv, st->r2, st->g, B, C, H, H, st->scr, s));          // seed: 2 H_adj(r)
    for (int i = st->M - 1; i >= 0; --i) {
        float* zi = st->zs + (size_t)i * tot; float* ui = st->us + (size_t)i * tot;
        if ((rc = run_plan(e, pr, ui, st->tab + (size_t)(st->M + i) * B, st->v, s, e->solver_time_scale)) != PF_OK) return rc;
        if ((rc = run_backward(e, pr, st->g, st->jg, s)) != PF_OK) return rc;                              // J_v(u_i)^T g
        DF_LAUNCH("adjoint scale", launch_dflow_scale(st->jg, st->h, prm->delta, (int64_t)tot, s));      // h = delta J^T g
        if ((rc = run_plan(e, pr, zi, st->tab + (size_t)i * B, st->v, s, e->solver_time_scale)) != PF_OK) return rc;
        if ((rc = run_backward(e, pr, st->h, st->jg, s)) != PF_OK) return rc;                              // J_v(z_i)^T h
        DF_LAUNCH("adjoint accumulate", launch_dflow_adjoint(st->g, st->h, st->jg, prm->half_delta, (int64_t)tot, s));
    }
    DF_LAUNCH("regulariser gradient", launch_dflow_reg_grad(st->g, st->zs, st->coef, lmbda, st->grad, B, (int64_t)st->n, s));
    return PF_OK;
}

static int dflow_begin(pf_engine* e, const pf_d_flow_params* prm, bool need_graph_stream, hipStream_t& s, const pf_degradation* d = nullptr, int* Hy = nullptr) {
    if (!e->finalized) { e->err = "weights not finalized"; return PF_ERR_STATE; }
    int rc = dflow_check_prm(e, prm);
    if (rc != PF_OK) return rc;
    if (e->cfg.output_channels != e->cfg.input_channels) { e->err = "d_flow needs output_channels == input_channels"; return PF_ERR_INVALID; }
    if (d && (rc = check_operator(e, "d_flow", d, e->cfg.input_height, *Hy)) != PF_OK) return rc;      // the operator of the closure, before the stream is swapped
    return graph_stream(e, need_graph_stream, s);
}

extern "C" {

int pf_d_flow_forward(pf_engine* e, const pf_d_flow_params* prm, const float* z, float* x_out, int B, void* stream) {
    if (!e || !prm || !z || !x_out || B <= 0) return PF_ERR_INVALID;
    USE_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const bool can_graph = prm->use_graph && !e->profile;
    int rc = dflow_begin(e, prm, can_graph, s);
    if (rc != PF_OK) return rc;
    const int C = e->cfg.input_channels, H = e->cfg.input_height;
    const size_t n = (size_t)C * H * H;
    if (n % 4) { e->err = "d_flow: C*H*W must be a multiple of 4"; return PF_ERR_INVALID; }
    const int M = prm->steps_euler - 1;
    const size_t ny_keep = e->dflow && e->dflow->B == B && e->dflow->n == n && e->dflow->M == M ? e->dflow->ny : n;
    if ((rc = ensure_dflow(e, B, n, ny_keep, M)) != PF_OK) return rc;
    DFlowState* st = e->dflow;
    Plan* plan = nullptr;
    if ((rc = build_plan(e, B, false, &plan)) != PF_OK) return rc;
    if ((rc = dflow_upload_tab(e, prm, B, s)) != PF_OK) return rc;
    HIPCHK(e, hipMemcpyAsync(st->zs, z, (size_t)B * n * 4, hipMemcpyDeviceToDevice, s));
    if (can_graph) {
        DFlowState::FwdKey key; memset(&key, 0, sizeof key);
        key.plan = plan; key.B = B; key.M = M; key.delta = prm->delta; key.half_delta = prm->half_delta;
        if (!st->fgraph.keep_for(e, key) && (rc = st->fgraph.capture(e, s, key, {plan}, [&] { return enqueue_dflow_forward(e, plan, prm, s); })) != PF_OK) return rc;
        if ((rc = st->fgraph.launch(e, s)) != PF_OK) return rc;
    } else {
        if ((rc = enqueue_dflow_forward(e, plan, prm, s)) != PF_OK) return rc;
    }
    HIPCHK(e, hipMemcpyAsync(x_out, st->zT, (size_t)B * n * 4, hipMemcpyDeviceToDevice, s));
    return PF_OK;
}

int pf_d_flow_value_and_grad(pf_engine* e, const pf_degradation* d, const pf_d_flow_params* prm, const float* z, const float* y, float lmbda,
                             float* loss_per_image, float* grad, int B, void* stream) {
    if (!e || !d || !prm || !z || !y || !loss_per_image || !grad || B <= 0) return PF_ERR_INVALID;
    USE_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const bool can_graph = prm->use_graph && !e->profile;
    int Hy = 0;
    int rc = dflow_begin(e, prm, can_graph, s, d, &Hy);
    if (rc != PF_OK) return rc;
    const int C = e->cfg.input_channels, H = e->cfg.input_height;
    const size_t n = (size_t)C * H * H;
    const size_t ny = (size_t)C * Hy * Hy;
    if (n % 4 || ny % 4) { e->err = "d_flow: C*H*W (and the measurement's C*Hy*Wy) must be multiples of 4"; return PF_ERR_INVALID; }
    const int M = prm->steps_euler - 1;
    if ((rc = ensure_dflow(e, B, n, ny, M)) != PF_OK) return rc;
    DFlowState* st = e->dflow;
    // the retained plan first (protected from eviction as e->retained_plan while the forward plan is fetched)
    Plan* pr = nullptr; Plan* pf = nullptr;
    if ((rc = build_plan(e, B, true, &pr)) != PF_OK) return rc;
    e->retained_B = B; e->retained_plan = pr;          // after the call: the retained forward of the last recompute (z_0, t_0)
    if ((rc = build_plan(e, B, false, &pf)) != PF_OK) return rc;
    if ((rc = dflow_upload_tab(e, prm, B, s)) != PF_OK) return rc;
    HIPCHK(e, hipMemcpyAsync(st->zs, z, (size_t)B * n * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipMemcpyAsync(st->y, y, (size_t)B * ny * 4, hipMemcpyDeviceToDevice, s));
    const DegView dv = to_view(d);
    if (can_graph) {
        DFlowState::VgKey key; memset(&key, 0, sizeof key);
        key.plan_fwd = pf; key.plan_ret = pr; key.deg = dv; key.B = B; key.M = M; key.delta = prm->delta; key.half_delta = prm->half_delta; key.lmbda = lmbda;
        if (!st->vgraph.keep_for(e, key) &&
            (rc = st->vgraph.capture(e, s, key, {pf, pr}, [&] { return enqueue_dflow_value_and_grad(e, pf, pr, dv, prm, lmbda, s); })) != PF_OK) return rc;
        if ((rc = st->vgraph.launch(e, s)) != PF_OK) return rc;
    } else {
        if ((rc = enqueue_dflow_value_and_grad(e, pf, pr, dv, prm, lmbda, s)) != PF_OK) return rc;
    }
    HIPCHK(e, hipMemcpyAsync(loss_per_image, st->loss, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipMemcpyAsync(grad, st->grad, (size_t)B * n * 4, hipMemcpyDeviceToDevice, s));
    return PF_OK;
}

// Dormand-Prince 5(4) tableau (torchdiffeq dopri5.py), rounded to fp32 as torchdiffeq rounds it to the state's dtype
static const double kDpAlpha[6] = {1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
static const double kDpBeta[6][6] = {
    {1.0 / 5, 0, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
    {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};
static const double kDpErr[7] = {35.0 / 384 - 1951.0 / 21600, 0, 500.0 / 1113 - 22642.0 / 50085, 125.0 / 192 - 451.0 / 720,
                                 -2187.0 / 6784 - -12231.0 / 42400, 11.0 / 84 - 649.0 / 6300, -1.0 / 60};
static const double kDpMid[7] = {6025192743.0 / 30085553152 / 2, 0, 51252292925.0 / 65400821598 / 2, -2691868925.0 / 45128329728 / 2,
                                 187940372067.0 / 1594534317056 / 2, -1776094331.0 / 19743644256 / 2, 11237099.0 / 235043384 / 2};

int pf_flow_ode_dopri5(pf_engine* e, const pf_dopri5_params* prm, const float* x_in, float* x_out, int B, int64_t* stats, void* stream) {
    if (!e || !prm || !x_in || !x_out || B <= 0) return PF_ERR_INVALID;
    if (!e->finalized) { e->err = "weights not finalized"; return PF_ERR_STATE; }
    if (!(prm->rtol > 0) || !(prm->atol > 0) || prm->t0 == prm->t1 || prm->max_steps <= 0) {
        e->err = "dopri5: rtol, atol > 0, t0 != t1 and max_steps > 0 required"; return PF_ERR_INVALID;
    }
    if (e->cfg.output_channels != e->cfg.input_channels) { e->err = "dopri5 needs output_channels == input_channels"; return PF_ERR_INVALID; }
    USE_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const int C = e->cfg.input_channels, H = e->cfg.input_height;
    const size_t n = (size_t)C * H * H;
    if (n % 4) { e->err = "dopri5: C*H*W must be a multiple of 4"; return PF_ERR_INVALID; }
    int rc = ensure_dopri(e, B, n);
    if (rc != PF_OK) return rc;
    DopriState* st = e->dopri;
    Plan* plan = nullptr;
    if ((rc = build_plan(e, B, false, &plan)) != PF_OK) return rc;
    const int64_t tot = (int64_t)B * n;
    const float atol = (float)prm->atol, rtol = (float)prm->rtol;
    // decreasing time: s = -t, f(s, y) = -v(y, -s) (torchdiffeq _ReverseFunc); k buffers hold the raw velocities v, the sign is folded
    // into every coefficient (exact: fp32 negation)
    const bool rev = prm->t1 < prm->t0;
    const float sg = rev ? -1.f : 1.f;
    const double s0 = rev ? -prm->t0 : prm->t0, send = rev ? -prm->t1 : prm->t1;
    int64_t accepted = 0, rejected = 0, nfev = 0;
    float* y = st->y; float* y1 = st->y1;
    float** k = st->k;
    double* part = st->part; double* red = st->part + 64;
    auto eval = [&](const float* yi, float s_f32, float* out) -> int {
        DF_LAUNCH("time", launch_fill(st->t, B, rev ? -s_f32 : s_f32, s));
        ++nfev;
        return run_plan(e, plan, yi, st->t, out, s, e->solver_time_scale);
    };
    auto rms = [&](const float* a, const float* b, const float* ya, const float* yb, const RkTerms& err, double& out) -> int {
        DF_LAUNCH("norm", launch_rk_norm(a, b, ya, yb, err, atol, rtol, part, red, tot, s));
        double sum = 0.0;
        HIPCHK(e, hipMemcpyAsync(&sum, red, sizeof sum, hipMemcpyDeviceToHost, s));
        HIPCHK(e, hipStreamSynchronize(s));
        out = (double)(float)std::sqrt(sum / (double)tot);          // torchdiffeq's norm is an fp32 tensor
        return PF_OK;
    };
    const RkTerms none{};
    HIPCHK(e, hipMemcpyAsync(y, x_in, (size_t)tot * 4, hipMemcpyDeviceToDevice, s));
    if ((rc = eval(y, (float)s0, k[0])) != PF_OK) return rc;                 // f0
    // initial step (torchdiffeq _select_initial_step, order 4), in the state's fp32
    double d0, d1, d2;
    if ((rc = rms(y, nullptr, y, nullptr, none, d0)) != PF_OK) return rc;
    if ((rc = rms(k[0], nullptr, y, nullptr, none, d1)) != PF_OK) return rc;
    const float h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6f : (float)(0.01f * (float)d0 / (float)d1);
    { RkTerms t{}; t.n = 1; t.k[0] = k[0]; t.c[0] = sg * h0; DF_LAUNCH("initial step", launch_rk_combine(y, t, st->stage, tot, s)); }
    if ((rc = eval(st->stage, (float)s0 + h0, k[1])) != PF_OK) return rc;
    if ((rc = rms(k[1], k[0], y, nullptr, none, d2)) != PF_OK) return rc;
    d2 = (double)std::fabs((float)d2 / h0);
    float h1;
    if (d1 <= 1e-15 && d2 <= 1e-15) h1 = std::max(1e-6f, h0 * 1e-3f);
    else h1 = std::pow(0.01f / (float)std::max(d1, d2), 1.f / 5.f);
    double dt = (double)std::min(100.f * h0, h1);
    double t = s0;
    while (send > t) {
        if (accepted + rejected >= prm->max_steps) {
            char buf[200];
            snprintf(buf, sizeof buf, "dopri5: step cap of %d attempts exceeded at t = %.9g (dt = %.3g, %lld accepted, %lld rejected); no result",
                     prm->max_steps, rev ? -t : t, dt, (long long)accepted, (long long)rejected);
            e->err = buf; return PF_ERR_NUMERIC;
        }
        if (!(t + dt > t)) { e->err = "dopri5: step size underflow"; return PF_ERR_NUMERIC; }
        const double t1 = t + dt;
        const float tf = (float)t, dtf = (float)dt;
        for (int i = 0; i < 6; ++i) {
            const float ti = kDpAlpha[i] == 1.0 ? (float)t1 : tf + (float)kDpAlpha[i] * dtf;
            RkTerms c{}; c.n = i + 1;
            for (int j = 0; j <= i; ++j) { c.k[j] = k[j]; c.c[j] = sg * ((float)kDpBeta[i][j] * dtf); }
            float* yi = i == 5 ? y1 : st->stage;                   // dopri5's last stage input is the 5th-order solution (FSAL)
            DF_LAUNCH("stage", launch_rk_combine(y, c, yi, tot, s));
            if ((rc = eval(yi, ti, k[i + 1])) != PF_OK) return rc;
        }
        RkTerms err{}; err.n = 7;
        for (int j = 0; j < 7; ++j) { err.k[j] = k[j]; err.c[j] = sg * ((float)kDpErr[j] * dtf); }
        double ratio;
        if ((rc = rms(nullptr, nullptr, y, y1, err, ratio)) != PF_OK) return rc;
        if (!std::isfinite(ratio)) { e->err = "dopri5: non-finite error estimate (the state or the velocity is not finite)"; return PF_ERR_NUMERIC; }
        if (ratio <= 1.0) {
            ++accepted;
            if (send <= t1) {     // last step: 4th-order dense output at send
                RkTerms m{}; m.n = 7;
                for (int j = 0; j < 7; ++j) { m.k[j] = k[j]; m.c[j] = sg * (dtf * (float)kDpMid[j]); }
                DF_LAUNCH("midpoint", launch_rk_combine(y, m, st->stage, tot, s));
                const float x = (float)((send - t) / (t1 - t));
                DF_LAUNCH("dense output", launch_rk_interp(y, y1, st->stage, k[0], k[6], sg, dtf, x, x_out, tot, s));
            }
            t = t1;
            std::swap(y, y1);
            std::swap(k[0], k[6]);          // FSAL: the last stage's velocity is the next step's first
        } else {
            ++rejected;
        }
        // next step (torchdiffeq _optimal_step_size: safety 0.9, ifactor 10, dfactor 0.2, order 5), in fp64
        if (ratio == 0.0) dt = dt * 10.0;
        else dt = dt * std::min(10.0, std::max(0.9 / std::pow(ratio, 1.0 / 5.0), ratio < 1.0 ? 1.0 : 0.2));
    }
    st->y = y; st->y1 = y1;
    if (stats) { stats[0] = accepted; stats[1] = rejected; stats[2] = nfev; }
    HIPCHK(e, hipStreamSynchronize(s));
    return check_flags(e);
}

}  // extern "C"
