// engine_pnp_gs.inc -- Prox-PnP with the gradient-step denoiser (pnpflow/methods/pnp_gs.py, pnpflow/train_denoiser.py) on the engine;
// included at the end of engine.hip.
//
// pf_gs_denoiser_grad   GRADIENT_STEP_DENOISER.calculate_grad (train_denoiser.py:39-57): one retained forward N = UNet(x, sigma), the seed
//                       r = x - N, the hand-written backward J^T r, Dg = r - J^T r (and g = 0.5 sum r^2).
// pf_pnp_gs_restore     iterations [first, stop) of PROX_PNP.solve_ip's loop (pnp_gs.py:132-222) for one batch.  One iteration = retained
//                       forward, seed, backward, combine (+ for hqs deblurring: Fourier prox, the three squared distances and the alpha
//                       decision; for hqs superresolution through a blur kernel, algo 3: the exact prox on the low-resolution grid), captured once into a hipGraph and replayed; the denoiser level of the iteration is read from a device
//                       table through the iteration counter, alpha from a device double.

struct PnpGsState {
    int B = 0; size_t n = 0, ny = 0; int max_iter = 0;
    float *x = nullptr, *z = nullptr, *N = nullptr, *r = nullptr, *JN = nullptr, *rhs = nullptr, *hadj = nullptr;      // [B n]
    float *y = nullptr, *hx = nullptr;                     // [B ny]
    float *scr = nullptr;                                  // [2 B n]: H / H_adj scratch, the FFT's complex plane
    float *pw = nullptr;                                   // [2 H]: separable factors of |fft2 filter|^2
    float *pw2 = nullptr;                                  // [H H]: the spectrum of a point-spread function, allocated by the first hqs call with PF_DEG_PSF_BLUR
    float *srs = nullptr, *lam = nullptr;                  // algo 3, allocated by its first call: launch_fft_prox_sr's scratch [3 B n + 3 B ny + 1 + B], then the spectrum's source, the aliased spectrum [Hy Hy]
    float *tab = nullptr, *cur = nullptr, *coef = nullptr; // [max_iter] level table, [B] level of this iteration, [B] lr / sigma^2
    int* iter = nullptr;
    double* dbl = nullptr;                                 // [0] alpha, [1] |H(x) - y|^2 carried, [2] g, [8 ..) 3 x PNPGS_MAX_PARTS partials, then [max_iter][2] (gap, threshold)
    DevBufs mem;
    struct Key { const void* plan; DegView deg; int B, algo, noise_model, skip, max_iter; float grad_coef; };
    static_assert(sizeof(Key) == 3 * sizeof(void*) + 10 * sizeof(int), "PnpGsState::Key is compared with memcmp: it must have no padding bytes");
    CachedGraph graph;
    void reset(pf_engine* e) { graph.drop(e); /* its nodes point into the buffers */ mem.release(e); *this = PnpGsState{}; }
    double* part(int i) const { return dbl + 8 + (size_t)i * PNPGS_MAX_PARTS; }
    double* log() const { return dbl + 8 + (size_t)3 * PNPGS_MAX_PARTS; }
};

static int ensure_pnpgs(pf_engine* e, int B, size_t n, size_t ny, int max_iter) {
    if (!e->pnpgs) e->pnpgs = new PnpGsState();
    PnpGsState* st = e->pnpgs;
    if (st->B == B && st->n == n && st->ny == ny && st->max_iter >= max_iter) return PF_OK;
    st->reset(e);
    const size_t tot = (size_t)B * n, toty = (size_t)B * ny;
    const int H = e->cfg.input_height;
    int rc = PF_OK;
    auto get = [&](auto** p, size_t count) { if (rc == PF_OK) rc = st->mem.alloc4(e, p, count); };
    for (float** p : {&st->x, &st->z, &st->N, &st->r, &st->JN, &st->rhs, &st->hadj}) get(p, tot);
    for (float** p : {&st->y, &st->hx}) get(p, toty);
    get(&st->scr, 2 * tot); get(&st->pw, (size_t)2 * H); get(&st->tab, (size_t)max_iter); get(&st->cur, (size_t)B); get(&st->coef, (size_t)B);
    get(&st->iter, 64); get(&st->dbl, 2 * ((size_t)8 + 3 * PNPGS_MAX_PARTS + 2 * (size_t)max_iter));
    if (rc != PF_OK) { st->reset(e); return rc; }
    st->B = B; st->n = n; st->ny = ny; st->max_iter = max_iter;
    return PF_OK;
}

__global__ void pnpgs_prep_kernel(const int* iter, const float* tab, float* cur, int B) {
    const float v = tab[*iter];
    for (int b = threadIdx.x; b < B; b += blockDim.x) cur[b] = v;
}

#define GS_LAUNCH(what, call) do { hipError_t _r = (call); if (_r != hipSuccess) { e->err = std::string("pnp_gs ") + what + ": " + hipGetErrorString(_r); return PF_ERR_HIP; } } while (0)

// N = UNet(in, level) retained, r = in - N, JN = J^T r  (train_denoiser.py:49-51)
static int enqueue_gs_grad(pf_engine* e, Plan* pr, const float* in, const float* level, double* partial, hipStream_t s) {
    PnpGsState* st = e->pnpgs;
    const int64_t tot = (int64_t)st->B * (int64_t)st->n;
    int rc = run_plan(e, pr, in, level, st->N, s, e->solver_time_scale);
    if (rc != PF_OK) return rc;
    GS_LAUNCH("seed", launch_pnpgs_seed(in, st->N, st->r, partial, tot, s));
    return run_backward(e, pr, st->r, st->JN, s);
}

// one iteration of pnp_gs.py:133-222 on st->x
static int enqueue_pnpgs_iteration(pf_engine* e, Plan* pr, const DegView& dv, const pf_pnp_gs_params* prm, hipStream_t s) {
    PnpGsState* st = e->pnpgs;
    const int B = st->B, C = e->cfg.input_channels, H = e->cfg.input_height;
    const int64_t tot = (int64_t)B * (int64_t)st->n, toty = (int64_t)B * (int64_t)st->ny;
    double* alpha = st->dbl;
    hipLaunchKernelGGL(pnpgs_prep_kernel, dim3(1), dim3(64), 0, s, (const int*)st->iter, (const float*)st->tab, st->cur, B);
    int rc;
    if (prm->algo == 0) {
        const float* z = st->x;
        if (!prm->skip_grad_step) {      // z = x - lr grad_datafit(x)  (pnp_gs.py:204-208)
            GS_LAUNCH("gradient step", launch_grad_step(dv, st->x, st->y, st->coef, st->z, B, C, H, H, st->scr, prm->noise_model, s));
            z = st->z;
        }
        if ((rc = enqueue_gs_grad(e, pr, z, st->cur, nullptr, s)) != PF_OK) return rc;
        GS_LAUNCH("combine", launch_pnpgs_combine(PNPGS_PGD, z, st->N, st->JN, nullptr, nullptr, alpha, st->x, B, (int64_t)st->n, (int64_t)H * H, s));
    } else if (prm->algo == 1) {
        if ((rc = enqueue_gs_grad(e, pr, st->x, st->cur, nullptr, s)) != PF_OK) return rc;
        GS_LAUNCH("combine", launch_pnpgs_combine(PNPGS_HQS_MASK, st->x, st->N, st->JN, st->y, dv.mask, nullptr, st->x, B, (int64_t)st->n, (int64_t)H * H, s));
    } else if (prm->algo == 3) {
        // pnp_gs.py:180-200 with the exact prox: rhs = alpha H_adj(noisy) + 0.065 alpha Dx + alpha (1 - 0.065 alpha) x, x <- prox; alpha never decays, no gap log
        if ((rc = enqueue_gs_grad(e, pr, st->x, st->cur, nullptr, s)) != PF_OK) return rc;
        GS_LAUNCH("combine", launch_pnpgs_combine(PNPGS_HQS_SR, st->x, st->N, st->JN, st->hadj, nullptr, alpha, st->rhs, B, (int64_t)st->n, (int64_t)H * H, s));
        GS_LAUNCH("prox", launch_fft_prox_sr(dv, st->rhs, alpha, st->lam, st->x, B, C, H, H, st->srs, s));
    } else {
        if ((rc = enqueue_gs_grad(e, pr, st->x, st->cur, nullptr, s)) != PF_OK) return rc;
        GS_LAUNCH("combine", launch_pnpgs_combine(PNPGS_HQS_BLUR, st->x, st->N, st->JN, st->hadj, nullptr, alpha, st->rhs, B, (int64_t)st->n, (int64_t)H * H, s));
        GS_LAUNCH("prox", launch_fft_prox_blur(st->rhs, alpha, st->pw, st->pw + H, st->z, B, C, H, H, st->scr, s, dv.kind == DEG_PSF_BLUR ? st->pw2 : nullptr));       // z: x_new
        GS_LAUNCH("H", launch_deg_H(dv, st->z, st->hx, B, C, H, H, st->scr, s));
        GS_LAUNCH("data term", launch_pnpgs_sqdist(st->hx, st->y, nullptr, st->part(0), toty, s));
        GS_LAUNCH("step length", launch_pnpgs_sqdist(st->z, st->x, st->x, st->part(1), tot, s));                                // and x <- x_new
        GS_LAUNCH("decision", launch_pnpgs_decide(st->part(0), pnpgs_parts(toty / 4), st->part(1), pnpgs_parts(tot / 4), st->dbl + 1, alpha, st->iter,
                                                  st->log(), st->max_iter, s));
    }
    hipLaunchKernelGGL(bump_iter_kernel, dim3(1), dim3(64), 0, s, st->iter);
    GS_LAUNCH("iteration", hipGetLastError());
    return PF_OK;
}

extern "C" {

int pf_gs_denoiser_grad(pf_engine* e, const float* x, const float* sigma, float* Dg, float* N, double* g, int B, void* stream) {
    if (!e || !x || !sigma || !Dg || B <= 0) return PF_ERR_INVALID;
    if (!e->finalized) { e->err = "weights not finalized"; return PF_ERR_STATE; }
    if (e->cfg.output_channels != e->cfg.input_channels) { e->err = "gs_denoiser_grad needs output_channels == input_channels"; return PF_ERR_INVALID; }
    USE_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const int C = e->cfg.input_channels, H = e->cfg.input_height;
    const size_t n = (size_t)C * H * H;
    if (n % 4) { e->err = "gs_denoiser_grad: C*H*W must be a multiple of 4"; return PF_ERR_INVALID; }
    const bool same = e->pnpgs && e->pnpgs->B == B && e->pnpgs->n == n;
    int rc = ensure_pnpgs(e, B, n, same ? e->pnpgs->ny : n, same ? e->pnpgs->max_iter : 1);
    if (rc != PF_OK) return rc;
    PnpGsState* st = e->pnpgs;
    Plan* pr = nullptr;
    if ((rc = build_plan(e, B, true, &pr)) != PF_OK) return rc;
    e->retained_B = B; e->retained_plan = pr;          // after the call: the retained forward is that of (x, sigma)
    const int64_t tot = (int64_t)B * (int64_t)n;
    if ((rc = enqueue_gs_grad(e, pr, x, sigma, g ? st->part(2) : nullptr, s)) != PF_OK) return rc;
    GS_LAUNCH("combine", launch_pnpgs_combine(PNPGS_DG, x, st->N, st->JN, nullptr, nullptr, nullptr, Dg, B, (int64_t)n, (int64_t)H * H, s));
    if (N) HIPCHK(e, hipMemcpyAsync(N, st->N, (size_t)tot * 4, hipMemcpyDeviceToDevice, s));
    if (g) GS_LAUNCH("energy", launch_pnpgs_sum(st->part(2), pnpgs_parts(tot / 4), 0.5, g, s));
    return PF_OK;
}

int pf_pnp_gs_restore(pf_engine* e, const pf_degradation* d, const pf_pnp_gs_params* prm, const float* y, float* x_inout, double* host_alpha_out,
                      double* host_log, int B, void* stream, pf_iter_callback iter_cb, void* user) {
    if (!e || !d || !prm || !y || !x_inout || B <= 0) return PF_ERR_INVALID;
    if (!e->finalized) { e->err = "weights not finalized"; return PF_ERR_STATE; }
    if (e->cfg.output_channels != e->cfg.input_channels) { e->err = "pnp_gs needs output_channels == input_channels"; return PF_ERR_INVALID; }
    if (prm->algo < 0 || prm->algo > 3) { e->err = "pnp_gs: algo must be 0 (pgd), 1 (hqs random_inpainting), 2 (hqs gaussian_deblurring_FFT) or 3 (hqs superresolution through a blur kernel)"; return PF_ERR_INVALID; }
    if (prm->algo == 3 && d->kind != PF_DEG_PSF_SR && d->kind != PF_DEG_SR_FILTERED) { e->err = "pnp_gs: algo 3 (hqs superresolution_blur / superresolution_bicubic) needs a PF_DEG_PSF_SR or PF_DEG_SR_FILTERED operator"; return PF_ERR_INVALID; }
    if (prm->algo == 1 && (d->kind != PF_DEG_MASK_INPAINTING || !d->mask)) { e->err = "pnp_gs: algo 1 (hqs random_inpainting) needs a PF_DEG_MASK_INPAINTING operator with a device mask"; return PF_ERR_INVALID; }
    if (prm->algo == 2 && d->kind == PF_DEG_GAUSSIAN_BLUR_ZERO) {
        e->err = "pnp_gs: algo 2 (hqs) has no zero-boundary form: its prox is a Fourier solve of the CIRCULAR blur (PF_DEG_GAUSSIAN_BLUR); use algo 0 (pgd) with PF_DEG_GAUSSIAN_BLUR_ZERO";
        return PF_ERR_INVALID;
    }
    if (prm->algo == 2 && d->kind == PF_DEG_PSF_BLUR_ZERO) {
        e->err = "pnp_gs: algo 2 (hqs) has no zero-boundary form: its prox is a Fourier solve of the CIRCULAR blur (PF_DEG_PSF_BLUR); use algo 0 (pgd) with PF_DEG_PSF_BLUR_ZERO";
        return PF_ERR_INVALID;
    }
    if (prm->algo == 2 && d->kind != PF_DEG_GAUSSIAN_BLUR && d->kind != PF_DEG_PSF_BLUR) { e->err = "pnp_gs: algo 2 (hqs gaussian_deblurring_FFT) needs a PF_DEG_GAUSSIAN_BLUR operator"; return PF_ERR_INVALID; }
    if (prm->noise_model != 0 && prm->noise_model != 1) { e->err = "pnp_gs: noise_model must be 0 (gaussian) or 1 (laplace)"; return PF_ERR_INVALID; }
    if (prm->noise_model == 1 && prm->algo != 0) { e->err = "pnp_gs: the laplace noise model exists for algo 0 (pgd) only"; return PF_ERR_INVALID; }
    if (prm->max_iter <= 0 || prm->first < 0 || prm->first > prm->stop || prm->stop > prm->max_iter) {
        e->err = "pnp_gs: 0 <= first <= stop <= max_iter and max_iter > 0 required"; return PF_ERR_INVALID;
    }
    if (!prm->host_sigma_den) { e->err = "pnp_gs: host_sigma_den (the denoiser level of every iteration) is required"; return PF_ERR_INVALID; }
    if (!(prm->alpha > 0.0)) { e->err = "pnp_gs: alpha must be positive"; return PF_ERR_INVALID; }
    const int C = e->cfg.input_channels, H = e->cfg.input_height;
    int Hy = 0;
    int rc = check_operator(e, "pnp_gs", d, H, Hy);
    if (rc != PF_OK) return rc;
    if ((d->kind == PF_DEG_GAUSSIAN_BLUR || d->kind == PF_DEG_SR_FILTERED) && d->ntaps > H) { e->err = "pnp_gs: the circular filtered operators need at most as many taps as the image side"; return PF_ERR_INVALID; }
    const size_t n = (size_t)C * H * H, ny = (size_t)C * Hy * Hy;
    if (n % 4 || ny % 4) { e->err = "pnp_gs: C*H*W (and the measurement's C*Hy*Wy) must be multiples of 4"; return PF_ERR_INVALID; }
    if (prm->algo == 1 && (H * H) % 4) { e->err = "pnp_gs: algo 1 needs H*W to be a multiple of 4"; return PF_ERR_INVALID; }
    if ((prm->algo == 2 || prm->algo == 3) && H > 2048) { e->err = "pnp_gs: algo 2 and algo 3 need H <= 2048"; return PF_ERR_INVALID; }
    USE_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const bool can_graph = prm->use_graph && !e->profile;
    if ((rc = graph_stream(e, can_graph, s)) != PF_OK) return rc;
    if ((rc = ensure_pnpgs(e, B, n, ny, prm->max_iter)) != PF_OK) return rc;
    PnpGsState* st = e->pnpgs;
    if (prm->algo == 2 && d->kind == PF_DEG_PSF_BLUR && !st->pw2 && (rc = st->mem.alloc4(e, &st->pw2, (size_t)H * H)) != PF_OK) return rc;
    if (prm->algo == 3 && !st->srs) {      // (ensure_pnpgs resets the state, and these with it, when B, n or ny change)
        if ((rc = st->mem.alloc4(e, &st->srs, sr_solve_scratch_floats(B, C, H, H, d->sf) - (size_t)Hy * Hy)) != PF_OK) return rc;      // (lam has a buffer of its own)
        if ((rc = st->mem.alloc4(e, &st->lam, (size_t)Hy * Hy)) != PF_OK) return rc;
    }
    Plan* pr = nullptr;
    if ((rc = build_plan(e, B, true, &pr)) != PF_OK) return rc;
    e->retained_B = B; e->retained_plan = pr;          // after the call: the retained forward of the last iteration's denoiser input
    const DegView dv = to_view(d);
    const size_t tot = (size_t)B * n, toty = (size_t)B * ny;
    const int first = prm->first;
    const double alpha0 = prm->alpha;
    HIPCHK(e, hipMemcpyAsync(st->tab, prm->host_sigma_den, (size_t)prm->max_iter * 4, hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(st->iter, &first, sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(st->dbl, &alpha0, sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(st->y, y, toty * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipMemcpyAsync(st->x, x_inout, tot * 4, hipMemcpyDeviceToDevice, s));
    GS_LAUNCH("coef", launch_fill(st->coef, B, prm->grad_coef, s));
    if (prm->algo == 2) {
        // once per call: H_adj(noisy), the filter's power spectrum and |H(x) - y|^2 of the entering iterate (afterwards carried by the decision kernel)
        HIPCHK(e, hipMemsetAsync(st->log(), 0, (size_t)2 * prm->max_iter * sizeof(double), s));
        GS_LAUNCH("H_adj", launch_deg_Hadj(dv, st->y, st->hadj, B, C, H, H, st->scr, s));
        if (dv.kind == DEG_PSF_BLUR) GS_LAUNCH("power spectrum", launch_psf_power_spectrum(dv, H, H, st->pw2, s));
        else GS_LAUNCH("power spectrum", launch_blur_power_spectrum(dv, H, H, st->pw, st->pw + H, s));
        GS_LAUNCH("H", launch_deg_H(dv, st->x, st->hx, B, C, H, H, st->scr, s));
        GS_LAUNCH("data term", launch_pnpgs_sqdist(st->hx, st->y, nullptr, st->part(0), (int64_t)toty, s));
        GS_LAUNCH("data term", launch_pnpgs_sum(st->part(0), pnpgs_parts((int64_t)toty / 4), 1.0, st->dbl + 1, s));
    }
    if (prm->algo == 3) {
        // once per call: H_adj(noisy) and the aliased spectrum (its source table goes into the tail of the prox scratch)
        GS_LAUNCH("H_adj", launch_deg_Hadj(dv, st->y, st->hadj, B, C, H, H, st->scr, s));
        GS_LAUNCH("aliased spectrum", launch_sr_aliased_spectrum(dv, H, H, st->lam, st->srs + sr_prox_scratch_floats(B, C, H, H, dv.sf), s));
    }
    HIPCHK(e, hipStreamSynchronize(s));      // the host table may go away after return

    PnpGsState::Key key; memset(&key, 0, sizeof key);
    key.plan = pr; key.deg = dv; key.B = B;
    key.algo = prm->algo; key.noise_model = prm->noise_model; key.skip = prm->skip_grad_step ? 1 : 0; key.max_iter = st->max_iter; key.grad_coef = prm->grad_coef;
    st->graph.keep_for(e, key);
    for (int it = first; it < prm->stop; ++it) {
        // pnp_gs.py:153: the last iteration of hqs random_inpainting leaves x as it is - its denoiser evaluation is dead and skipped
        const bool dead = prm->algo == 1 && it == prm->max_iter - 1;
        if (!dead) {
            if (can_graph && (it > first || st->graph.live())) {
                if (!st->graph.live() && (rc = st->graph.capture(e, s, key, {pr}, [&] { return enqueue_pnpgs_iteration(e, pr, dv, prm, s); })) != PF_OK) return rc;
                if ((rc = st->graph.launch(e, s)) != PF_OK) return rc;
            } else {
                if ((rc = enqueue_pnpgs_iteration(e, pr, dv, prm, s)) != PF_OK) return rc;
            }
        }
        if (iter_cb && (!prm->host_cb_mask || prm->host_cb_mask[it])) {
            HIPCHK(e, hipMemcpyAsync(x_inout, st->x, tot * 4, hipMemcpyDeviceToDevice, s));
            HIPCHK(e, hipStreamSynchronize(s));
            iter_cb(it, user);
        }
    }
    HIPCHK(e, hipMemcpyAsync(x_inout, st->x, tot * 4, hipMemcpyDeviceToDevice, s));
    if (host_alpha_out) HIPCHK(e, hipMemcpyAsync(host_alpha_out, st->dbl, sizeof(double), hipMemcpyDeviceToHost, s));
    if (host_log && prm->algo == 2) HIPCHK(e, hipMemcpyAsync(host_log, st->log(), (size_t)2 * prm->max_iter * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    return check_flags(e);
}

}  // extern "C"
