// NCSN++ input-gradient backward (J^T vec w.r.t. the image; included by engine.hip after the shared backward helpers).
// What OT_ODE asks of the velocity net: torch.autograd.functional.vjp(lambda x: model_forward(x, t), x, vec)  (ot_ode.py:137-138).
// The time conditioning does not depend on x, so only the image path is walked, in reverse over the retained forward's tape:
//   conv3x3 / conv1x1 / NIN        adjoint convs on the same MFMA kernels (transposed, tap-flipped repacks), the (x + h) * s of every
//                                  block as out_scale / add_scale
//   GroupNorm(+SiLU)               the OT net's three-stage backward (first stage fused into the adjoint conv's epilogue where it can)
//   FIR up / down (upfirdn2d)      its adjoint is the same kernel with up <-> down, pad0' = K - 1 - pad0 and the flipped taps
//   input_skip / output_skip       the pyramids' FIR chains and their 3-channel convs (NHWC-32 operands) carry gradient to the image too

// gdst (first write) = FIR^T gsrc, where the forward op resampled gdst's shape to gsrc's shape
static void nx_fir_adj(BwdCtx& c, const Tensor& gsrc, bool fwd_up, const Tensor& gdst) {
    Op op{}; op.kind = OP_NX_FIR;
    FirParams f{}; nx_fir_kernel(c.e->ncfg, fwd_up, f);
    FirParams& a = op.fp;
    a.K = f.K; a.up = f.down; a.down = f.up; a.pad0 = f.K - 1 - f.pad0;
    for (int i = 0; i < f.K * f.K; ++i) a.k2d[i] = f.k2d[f.K * f.K - 1 - i];
    a.src = gsrc.p; a.B = c.B; a.Hs = gsrc.H; a.Ws = gsrc.W; a.H = gdst.H; a.W = gdst.W; a.C = gsrc.C;
    a.out_raw = gdst.p; a.out_act = nullptr; a.coef = nullptr; a.stats_raw = nullptr;
    c.push(op);
}

static int nx_build_backward(pf_engine* e, Plan* plan, Builder& bd) {
    const int B = plan->B;
    const pf_ncsnpp_cfg& cf = e->ncfg;
    const int H0 = cf.image_size, chn = cf.num_channels;
    BwdCtx c{e, plan, &bd, B};
    { Op op{}; op.kind = OP_MEMSET; plan->bops.push_back(op); }        // op 0: zero the backward sums (range filled in below)
    plan->vec_scaled = bd.acquire((size_t)B * chn * H0 * H0);
    plan->vjp_scale = bd.acquire(64); plan->vjp_amax = reinterpret_cast<unsigned int*>(bd.acquire(64));
    const size_t bwd_lo = bd.stats_bytes;
    // v = pyramid[:, :chn] / sigma (ncsnpp.py:378-381).  J^T is linear and per image, so the 1/sigma is applied to the RESULT: the
    // (power-of-two normalised) vec enters the adjoint convs at unit magnitude, where the split-fp16 operands keep their full
    // precision (vec / sigma ~ 1e-3 would push the low halves into fp16 subnormals: 8e-4 relative error, measured)
    {
        GradEntry& gp = c.G(plan->t_last);
        Op op{}; op.kind = OP_NX_IMG_IN; op.O = gp.t.p; op.P[0] = nullptr; op.I[0] = chn; op.I[1] = H0; op.I[2] = H0;
        c.push(op); gp.has = true;
    }
    for (auto it = plan->tape.rbegin(); it != plan->tape.rend(); ++it) {
        const TapeRec& tr = *it;
        GradEntry& gout = c.G(tr.out);
        if (!gout.has) { e->err = "internal: NCSN++ backward reached a tensor without gradient"; return PF_ERR_INVALID; }
        const int H = tr.out.H, Wd = tr.out.W;
        if (tr.kind == TP_ATTN) {
            bwd_attn(c, tr, gout);
        } else if (tr.kind == TP_NX_OUT_SKIP) {
            // pyramid_new = conv3x3(act(GN(h))) [+ upsample(pyramid_old)]  (ncsnpp.py:332-343)
            const int gi = tr.idx, ci = tr.idx + 1, C = tr.in0.C;
            const std::string key = nx_name(ci, "weight") + "#out32";
            Tensor da = c.tmp(C, H, Wd);
            GnBwd g = gn_bwd_begin(c, {tr.in0}, nx_name(gi, ""), true, nx_groups(C));
            ConvParams p = bwd_params(B, H, Wd, H, Wd, C);
            adj_seg(e, p, gout.t.p, 32, 32, 9, key, 0, C);
            p.out = da.p; p.out_cstride = C;
            gn_bwd_fuse(c, g, 0, p);
            c.conv_plain(p);
            gn_bwd_finish(c, g, {da}, {&c.G(tr.in0)}, {nullptr});
            bd.recycle(da.p);
            if (tr.has_old) {
                GradEntry& go = c.G(tr.pyr_old);
                if (go.has) { e->err = "internal: pyramid gradient written twice"; return PF_ERR_INVALID; }
                nx_fir_adj(c, gout.t, true, go.t); go.has = true;
            }
        } else if (tr.kind == TP_NX_PYR_DOWN) {
            GradEntry& gi = c.G(tr.in0);
            if (gi.has) { e->err = "internal: input-pyramid gradient written twice"; return PF_ERR_INVALID; }
            nx_fir_adj(c, gout.t, false, gi.t); gi.has = true;
        } else if (tr.kind == TP_NX_CONV_IN) {
            const std::string key = nx_name(tr.idx, "weight") + "#pad32";
            const int nf = tr.out.C;
            ConvParams p = bwd_params(B, H, Wd, H, Wd, 32);
            adj_seg(e, p, gout.t.p, nf, nf, 9, key, 0, 32);
            c.conv_to(p, c.G(tr.in0));
        } else if (tr.kind == TP_NX_RES) {
            const NxMod& m = e->nx_mods[tr.idx];
            const std::string P = nx_name(tr.idx, "");
            const int cout = m.out_ch, cin = tr.in0.C + (tr.has_in1 ? tr.in1.C : 0);
            const float s = tr.s;
            // out = s * (Conv_1(act(GN_1(h1))) + shortcut) [+ Combine]: d(act1) = s Conv_1^T(gout), GN_1+SiLU backward -> d(h1)
            Tensor t1 = c.tmp(cout, H, Wd);
            GnBwd gn1 = gn_bwd_begin(c, {tr.h1}, P + "GroupNorm_1.", true, nx_groups(cout));
            {
                ConvParams p = bwd_params(B, H, Wd, H, Wd, cout);
                adj_seg(e, p, gout.t.p, cout, cout, 9, P + "Conv_1.weight", 0, cout);
                p.out = t1.p; p.out_cstride = cout; p.out_scale = s;
                gn_bwd_fuse(c, gn1, 0, p);
                c.conv_plain(p);
            }
            GradEntry gh1; gh1.t = c.tmp(cout, H, Wd);
            gn_bwd_finish(c, gn1, {t1}, {&gh1}, {nullptr});
            bd.recycle(t1.p);
            if (tr.has_pyr) {      // h = Conv_0(input_pyramid) + h  (Combine 'sum'): the pyramid's gradient, un-scaled
                const std::string cw = nx_name(tr.idx + 1, "Conv_0.weight");
                const HostTensor& w = W(e, cw);
                const int O = (int)w.shape[0], I = (int)w.shape[1];
                const std::string key = nx_derive(e, cw + "#pad32raw", {O, 32, 1, 1}, [&](std::vector<float>& d) {
                    for (int o = 0; o < O; ++o) for (int i = 0; i < I; ++i) d[(size_t)o * 32 + i] = w.data[(size_t)o * I + i];
                });
                ConvParams p = bwd_params(B, H, Wd, H, Wd, 32);
                adj_seg(e, p, gout.t.p, cout, cout, 1, key, 0, 32);
                c.conv_to(p, c.G(tr.pyr));
            }
            if (!tr.resample) {
                std::vector<Tensor> srcs{tr.in0}; if (tr.has_in1) srcs.push_back(tr.in1);
                std::vector<Tensor> us; std::vector<GradEntry*> dsts; std::vector<const float*> adds;
                GnBwd gn0 = gn_bwd_begin(c, srcs, P + "GroupNorm_0.", true, nx_groups(cin));
                int lo = 0;
                for (size_t sj = 0; sj < srcs.size(); ++sj) {
                    const Tensor& sT = srcs[sj];
                    Tensor u = c.tmp(sT.C, H, Wd);
                    ConvParams p = bwd_params(B, H, Wd, H, Wd, sT.C);
                    adj_seg(e, p, gh1.t.p, cout, cout, 9, P + "Conv_0.weight", lo, lo + sT.C);
                    p.out = u.p; p.out_cstride = sT.C;
                    gn_bwd_fuse(c, gn0, sj, p);
                    c.conv_plain(p);
                    us.push_back(u);
                    GradEntry& gd = c.G(sT);
                    if (cin != cout) {       // s * Conv_2^T(gout) straight into the gradient buffer
                        ConvParams q = bwd_params(B, H, Wd, H, Wd, sT.C);
                        adj_seg(e, q, gout.t.p, cout, cout, 1, P + "Conv_2.weight", lo, lo + sT.C);
                        q.out_scale = s;
                        c.conv_to(q, gd);
                        adds.push_back(nullptr);
                    } else {
                        adds.push_back(gout.t.p);          // identity skip: + s * gout
                    }
                    dsts.push_back(&gd);
                    lo += sT.C;
                }
                gn_bwd_finish(c, gn0, us, dsts, adds, s);
                for (auto& u : us) bd.recycle(u.p);
            } else {
                // h = FIR(act(GN_0(x))), x' = FIR(x)  (layerspp.py:238-254): both gradients go back through the FIR adjoint
                const Tensor& x = tr.in0;
                Tensor dh = c.tmp(x.C, H, Wd);
                {
                    ConvParams p = bwd_params(B, H, Wd, H, Wd, x.C);
                    adj_seg(e, p, gh1.t.p, cout, cout, 9, P + "Conv_0.weight", 0, x.C);
                    p.out = dh.p; p.out_cstride = x.C; c.conv_plain(p);
                }
                Tensor da = c.tmp(x.C, x.H, x.W);
                nx_fir_adj(c, dh, tr.up, da);
                Tensor dxr = c.tmp(x.C, H, Wd);
                {
                    ConvParams q = bwd_params(B, H, Wd, H, Wd, x.C);
                    adj_seg(e, q, gout.t.p, cout, cout, 1, P + "Conv_2.weight", 0, x.C);
                    q.out = dxr.p; q.out_cstride = x.C; q.out_scale = s; c.conv_plain(q);
                }
                Tensor tx = c.tmp(x.C, x.H, x.W);
                nx_fir_adj(c, dxr, tr.up, tx);
                GnBwd gn0 = gn_bwd_begin(c, {x}, P + "GroupNorm_0.", true, nx_groups(x.C));
                gn_bwd_finish(c, gn0, {da}, {&c.G(x)}, {tx.p});
                for (float* q : {dh.p, da.p, dxr.p, tx.p}) bd.recycle(q);
            }
            bd.recycle(gh1.t.p);
        } else {
            e->err = "internal: unexpected tape record in the NCSN++ backward"; return PF_ERR_INVALID;
        }
    }
    // image gradient: the first chn channels of d(x32)
    {
        GradEntry& g0 = c.G(plan->tape.front().in0);
        if (plan->tape.front().kind != TP_NX_CONV_IN || !g0.has) { e->err = "internal: no gradient at the NCSN++ input"; return PF_ERR_INVALID; }
        Op op{}; op.kind = OP_NX_IMG_OUT; op.P[0] = g0.t.p; op.P[1] = cf.scale_by_sigma ? plan->nx_sigma : nullptr; op.I[0] = chn; op.I[1] = H0; op.I[2] = H0; c.push(op);
    }
    plan->bops[0].ptr = (void*)(uintptr_t)(bwd_lo + 1);
    plan->bops[0].bytes = bd.stats_bytes - bwd_lo;
    return PF_OK;
}
