// NCSN++ ("rectified" coupling) on the conv engine: architecture walk + forward plan of
// pnpflow/image_generation/models/ncsnpp.py (included by engine.hip; SURVEY.md 8f N4).
//
// What maps to what
//   conv3x3 / conv1x1 / NIN / Combine     MFMA implicit-GEMM conv launches (conv_mfma16.hip / conv_mfma.hip), GroupNorm+SiLU in
//                                         the staging, bias + Dense_0(act(temb)) + skip in the epilogue, next GroupNorm's
//                                         statistics reduced in the same launch
//   ResnetBlockBigGANpp (layerspp.py:209-274)  two launches; the 1x1 shortcut Conv_2 (and, after a down block, the input-skip
//                                         Combine, ncsnpp.py:283-286) are extra K-segments of the second one; (x + h)/sqrt(2) is
//                                         out_scale / res_scale of that epilogue
//   up / down blocks                      one fir_nhwc launch produces FIR(SiLU(GN_0(x))) and FIR(x) (ncsnpp_ops.hip)
//   AttnBlockpp (layerspp.py:61-94)       attn_block() of the OT net on NIN -> 1x1-conv aliases
//   output_skip pyramid (ncsnpp.py:332-351)   conv C -> 3 padded to 32 output channels, the FIR-upsampled pyramid is its residual
//   image boundary                        NCHW <-> zero-padded NHWC-32 (so the 3-channel convs are ordinary K-segments)

static std::string nx_name(int idx, const char* sub) { return "all_modules." + std::to_string(idx) + "." + sub; }
static int nx_groups(int C) { return std::min(C / 4, 32); }      // nn.GroupNorm(num_groups=min(ch // 4, 32), eps=1e-6)

static int nx_build_arch(pf_engine* e) {
    const pf_ncsnpp_cfg& c = e->ncfg;
    const int nf = c.nf, nlev = c.num_levels, nres = c.num_res_blocks, tdim = 4 * nf, chn = c.num_channels;
    auto in_attn = [&](int res) { for (int i = 0; i < c.num_attn_resolutions; ++i) if (c.attn_resolutions[i] == res) return true; return false; };
    auto push = [&](NxMod::Kind k, int i, int o, bool up = false, bool down = false) {
        NxMod m; m.kind = k; m.in_ch = i; m.out_ch = o; m.up = up; m.down = down;
        const int idx = (int)e->nx_mods.size();
        e->nx_mods.push_back(m);
        auto nm = [&](const char* sub) { return nx_name(idx, sub); };
        switch (k) {
            case NxMod::FOURIER: expect(e, nm("W"), {nf}); break;
            case NxMod::LINEAR: expect(e, nm("weight"), {o, i}); expect(e, nm("bias"), {o}); break;
            case NxMod::CONV_IN: case NxMod::CONV_OUT: expect(e, nm("weight"), {o, i, 3, 3}); expect(e, nm("bias"), {o}); break;
            case NxMod::GN: expect(e, nm("weight"), {i}); expect(e, nm("bias"), {i}); break;
            case NxMod::COMBINE: expect(e, nm("Conv_0.weight"), {o, i, 1, 1}); expect(e, nm("Conv_0.bias"), {o}); break;
            case NxMod::ATTN:
                expect(e, nm("GroupNorm_0.weight"), {i}); expect(e, nm("GroupNorm_0.bias"), {i});
                for (const char* n : {"NIN_0.", "NIN_1.", "NIN_2.", "NIN_3."}) { expect(e, nm(n) + "W", {i, i}); expect(e, nm(n) + "b", {i}); }
                break;
            case NxMod::RES:
                expect(e, nm("GroupNorm_0.weight"), {i}); expect(e, nm("GroupNorm_0.bias"), {i});
                expect(e, nm("Conv_0.weight"), {o, i, 3, 3}); expect(e, nm("Conv_0.bias"), {o});
                expect(e, nm("Dense_0.weight"), {o, tdim}); expect(e, nm("Dense_0.bias"), {o});
                expect(e, nm("GroupNorm_1.weight"), {o}); expect(e, nm("GroupNorm_1.bias"), {o});
                expect(e, nm("Conv_1.weight"), {o, o, 3, 3}); expect(e, nm("Conv_1.bias"), {o});
                if (i != o || up || down) { expect(e, nm("Conv_2.weight"), {o, i, 1, 1}); expect(e, nm("Conv_2.bias"), {o}); }
                break;
        }
    };
    // ncsnpp.py:72-92 (time conditioning), :139-206 (blocks)
    push(NxMod::FOURIER, 0, 0);
    push(NxMod::LINEAR, 2 * nf, tdim); push(NxMod::LINEAR, tdim, tdim);
    push(NxMod::CONV_IN, chn, nf);
    std::vector<int> hs_c{nf};
    int in_ch = nf, res = c.image_size;
    for (int lvl = 0; lvl < nlev; ++lvl) {
        for (int blk = 0; blk < nres; ++blk) {
            const int o = nf * c.ch_mult[lvl];
            push(NxMod::RES, in_ch, o); in_ch = o;
            if (in_attn(res)) push(NxMod::ATTN, in_ch, in_ch);
            hs_c.push_back(in_ch);
        }
        if (lvl != nlev - 1) {
            push(NxMod::RES, in_ch, in_ch, false, true);
            push(NxMod::COMBINE, chn, in_ch);
            hs_c.push_back(in_ch); res /= 2;
        }
    }
    in_ch = hs_c.back();
    push(NxMod::RES, in_ch, in_ch); push(NxMod::ATTN, in_ch, in_ch); push(NxMod::RES, in_ch, in_ch);
    for (int lvl = nlev - 1; lvl >= 0; --lvl) {
        for (int blk = 0; blk < nres + 1; ++blk) {
            const int o = nf * c.ch_mult[lvl];
            push(NxMod::RES, in_ch + hs_c.back(), o); hs_c.pop_back(); in_ch = o;
        }
        if (in_attn(res)) push(NxMod::ATTN, in_ch, in_ch);
        push(NxMod::GN, in_ch, in_ch); push(NxMod::CONV_OUT, in_ch, chn);
        if (lvl != 0) { push(NxMod::RES, in_ch, in_ch, true, false); res *= 2; }
    }
    if (!hs_c.empty()) { e->err = "internal: skip stack not empty"; return PF_ERR_INVALID; }
    // stacked Dense_0 projections, forward order = module order
    int off = 0;
    for (size_t i = 0; i < e->nx_mods.size(); ++i)
        if (e->nx_mods[i].kind == NxMod::RES) { e->temb_off[nx_name((int)i, "")] = off; off += e->nx_mods[i].out_ch; }
    e->temb_total = off;
    return PF_OK;
}

// derived host tensors (built once): 1x1-conv views of NIN weights, channel-padded image convs
static const std::string& nx_derive(pf_engine* e, const std::string& key, std::vector<int64_t> shape, const std::function<void(std::vector<float>&)>& fill) {
    auto it = e->host.find(key);
    if (it == e->host.end()) {
        HostTensor t; t.shape = std::move(shape);
        size_t n = 1; for (auto d : t.shape) n *= (size_t)d;
        t.data.assign(n, 0.f); fill(t.data); t.loaded = true;
        it = e->host.emplace(key, std::move(t)).first;
    }
    return it->first;
}

// NIN (layers.py:546-555): y = x W + b with W [in][out]  ->  1x1 conv weight [out][in][1][1]
static void nx_alias_attn(pf_engine* e, int idx) {
    const std::string P = nx_name(idx, "");
    if (e->host.count(P + "attn_q.weight")) return;
    const char* dst[4] = {"attn_q.", "attn_k.", "attn_v.", "proj_out."};
    const char* src[4] = {"NIN_0.", "NIN_1.", "NIN_2.", "NIN_3."};
    for (int k = 0; k < 4; ++k) {
        const HostTensor& w = W(e, P + src[k] + "W");
        const int I = (int)w.shape[0], O = (int)w.shape[1];
        HostTensor t; t.shape = {O, I, 1, 1}; t.data.resize((size_t)O * I); t.loaded = true;
        for (int o = 0; o < O; ++o) for (int i = 0; i < I; ++i) t.data[(size_t)o * I + i] = w.data[(size_t)i * O + o];
        e->host[P + dst[k] + "weight"] = std::move(t);
        HostTensor b = W(e, P + src[k] + "b"); e->host[P + dst[k] + "bias"] = b;
    }
    e->host[P + "norm.weight"] = W(e, P + "GroupNorm_0.weight");
    e->host[P + "norm.bias"] = W(e, P + "GroupNorm_0.bias");
}

static void nx_fir_kernel(const pf_ncsnpp_cfg& c, bool up, FirParams& f) {
    // _setup_kernel (up_or_down_sampling.py:191-199): outer product, / sum, in fp32; upsampling gains factor^2 (:231)
    const int K = c.fir_taps;
    float k2[64]; float sum = 0.f;
    for (int i = 0; i < K; ++i) for (int j = 0; j < K; ++j) { k2[i * K + j] = c.fir_kernel[i] * c.fir_kernel[j]; }
    { double acc = 0.0; for (int i = 0; i < K * K; ++i) acc += (double)k2[i]; sum = (float)acc; }
    for (int i = 0; i < K * K; ++i) f.k2d[i] = (k2[i] / sum) * (up ? 4.0f : 1.0f);
    const int pd = K - 2;
    f.K = K; f.up = up ? 2 : 1; f.down = up ? 1 : 2;
    f.pad0 = up ? (pd + 1) / 2 + 1 : (pd + 1) / 2;          // upsample_2d :233 / downsample_2d :258  (pad1 follows from the output size)
}

// FIR resampling of `src` by 2: act view (GroupNorm `gn_idx`'s sub-module `gn_sub` + SiLU) and / or raw view
static void nx_fir(Builder& bd, const Tensor& src, bool up, const std::string* gn_prefix, Tensor* out_act, Tensor* out_raw) {
    pf_engine* e = bd.e; Plan* plan = bd.plan;
    const int H = up ? src.H * 2 : src.H / 2, Wd = up ? src.W * 2 : src.W / 2;
    Op op{}; op.kind = OP_NX_FIR;
    FirParams& f = op.fp;
    nx_fir_kernel(e->ncfg, up, f);
    f.src = src.p; f.B = bd.B; f.Hs = src.H; f.Ws = src.W; f.H = H; f.W = Wd; f.C = src.C;
    if (out_act) {
        ensure_coef(bd);
        Op g{}; g.kind = OP_GN_COEF;
        g.gp.nseg = 1; g.gp.st[0] = src.stats; g.gp.C[0] = src.C; g.gp.xform[0] = 2; g.gp.gn_off[0] = 0;
        g.gp.gn_C = src.C; g.gp.gn_cpg = src.C / nx_groups(src.C); g.gp.HW = src.H * src.W; g.gp.eps = 1e-6f;
        g.gp.gamma = upload(e, *gn_prefix + "weight", W(e, *gn_prefix + "weight").data);
        g.gp.beta = upload(e, *gn_prefix + "bias", W(e, *gn_prefix + "bias").data);
        g.gp.coef = plan->coef; g.gp.coef_stride = Plan::COEF_STRIDE; g.gp.scale = nullptr; g.gp.flags = plan->flags; g.gp.id = (int)plan->ops.size();
        plan->ops.push_back(g);
        *out_act = bd.make(src.C, H, Wd, false);
        f.out_act = out_act->p; f.coef = plan->coef; f.coef_stride = Plan::COEF_STRIDE;
    }
    if (out_raw) {
        *out_raw = bd.make(src.C, H, Wd, src.stats != nullptr);
        f.out_raw = out_raw->p; f.stats_raw = out_raw->stats;
    }
    plan->ops.push_back(op);
}

// ResnetBlockBigGANpp.forward (layerspp.py:235-274).  in1: the popped skip (input = cat[in0, in1]); pyr: the down-sampled input
// pyramid whose Combine (module idx + 1) follows a down block (ncsnpp.py:283-286)
static Tensor nx_res_block(Builder& bd, int idx, const Tensor& in0, const Tensor* in1, const Tensor* pyr, float* temb_vec) {
    pf_engine* e = bd.e; const int B = bd.B;
    const NxMod& m = e->nx_mods[idx];
    const std::string P = nx_name(idx, "");
    const int cin = in0.C + (in1 ? in1->C : 0), cout = m.out_ch;
    const float s = e->ncfg.skip_rescale ? 0.70710678118654752440f : 1.0f;
    const bool resample = m.up || m.down;
    Tensor hact{}, xres{};
    if (resample) { const std::string gp = P + "GroupNorm_0."; nx_fir(bd, in0, m.up, &gp, &hact, &xres); }
    const int H = resample ? hact.H : in0.H, Wd = resample ? hact.W : in0.W;
    // Conv_0 (+ Conv_0.bias + Dense_0(act(temb)))
    Tensor h1 = bd.make(cout, H, Wd, true);
    {
        ConvParams p = base_params(B, H, Wd, H, Wd, h1);
        if (resample) {
            packed_seg(e, p, hact, 0, 9, 0, P + "Conv_0.weight", 0, in0.C);
        } else {
            packed_seg(e, p, in0, 2, 9, 0, P + "Conv_0.weight", 0, in0.C);
            if (in1) packed_seg(e, p, *in1, 2, 9, in0.C, P + "Conv_0.weight", in0.C, cin);
            p.gn_C = cin; p.gn_cpg = cin / nx_groups(cin);
            p.gamma = upload(e, P + "GroupNorm_0.weight", W(e, P + "GroupNorm_0.weight").data);
            p.beta = upload(e, P + "GroupNorm_0.bias", W(e, P + "GroupNorm_0.bias").data);
        }
        p.addvec = temb_vec + e->temb_off.at(P); p.addvec_bs = e->temb_total;
        push_conv(bd, p);
    }
    if (resample) bd.release(hact.p);
    // Conv_1 (+ shortcut) -> (x + h) * s  (+ Combine)
    Tensor out = bd.make(cout, H, Wd, true);
    {
        ConvParams p = base_params(B, H, Wd, H, Wd, out);
        packed_seg(e, p, h1, 2, 9, 0, P + "Conv_1.weight", 0, cout);
        p.gn_C = cout; p.gn_cpg = cout / nx_groups(cout);
        p.gamma = upload(e, P + "GroupNorm_1.weight", W(e, P + "GroupNorm_1.weight").data);
        p.beta = upload(e, P + "GroupNorm_1.bias", W(e, P + "GroupNorm_1.bias").data);
        std::vector<float> bias = W(e, P + "Conv_1.bias").data;
        if (cin != cout || resample) {
            const Tensor& x0 = resample ? xres : in0;
            packed_seg(e, p, x0, 0, 1, 0, P + "Conv_2.weight", 0, in0.C);
            if (in1) packed_seg(e, p, *in1, 0, 1, 0, P + "Conv_2.weight", in0.C, cin);
            const auto& sb = W(e, P + "Conv_2.bias").data;
            for (size_t i = 0; i < bias.size(); ++i) bias[i] += sb[i];
        } else {
            p.residual = in0.p; p.res_cstride = in0.C; p.res_scale = s;
        }
        for (auto& v : bias) v *= s;
        p.out_scale = s;
        if (pyr) {
            // h = Conv_0(input_pyramid) + h (Combine 'sum', layerspp.py:44-58): a third K-segment whose weights carry 1/s, because the
            // epilogue scales the whole accumulator by s
            const std::string cw = nx_name(idx + 1, "Conv_0.weight");
            const HostTensor& w = W(e, cw);
            const int O = (int)w.shape[0], I = (int)w.shape[1];
            const float inv = 1.0f / s;
            const std::string key = nx_derive(e, cw + "#pad32", {O, 32, 1, 1}, [&](std::vector<float>& d) {
                for (int o = 0; o < O; ++o) for (int i = 0; i < I; ++i) d[(size_t)o * 32 + i] = w.data[(size_t)o * I + i] * inv;
            });
            if (p.nseg >= 3) { e->err = "internal: too many K-segments"; bd.ok = false; return out; }
            packed_seg(e, p, *pyr, 0, 1, 0, key, 0, 32);
            const auto& cb = W(e, nx_name(idx + 1, "Conv_0.bias")).data;
            for (size_t i = 0; i < bias.size(); ++i) bias[i] += cb[i];
        }
        p.addvec = upload(e, P + "Conv_1.bias+sc", bias); p.addvec_bs = 0;
        push_conv(bd, p);
    }
    bd.release(h1.p);
    if (resample) bd.release(xres.p);
    if (bd.plan->retain) {
        TapeRec tr; tr.kind = TP_NX_RES; tr.idx = idx; tr.in0 = in0; tr.has_in1 = in1 != nullptr; if (in1) tr.in1 = *in1; tr.h1 = h1; tr.out = out;
        tr.resample = resample; tr.up = m.up; tr.hact = hact; tr.xres = xres; tr.has_pyr = pyr != nullptr; if (pyr) tr.pyr = *pyr; tr.s = s;
        bd.plan->tape.push_back(tr);
    }
    return out;
}

static int nx_walk(pf_engine* e, Builder& bd, Plan* plan) {
    const pf_ncsnpp_cfg& c = e->ncfg;
    const int B = bd.B, nf = c.nf, nlev = c.num_levels, nres = c.num_res_blocks, H0 = c.image_size, chn = c.num_channels;
    auto in_attn = [&](int res) { for (int i = 0; i < c.num_attn_resolutions; ++i) if (c.attn_resolutions[i] == res) return true; return false; };
    const float s = c.skip_rescale ? 0.70710678118654752440f : 1.0f;
    char nm[64];
    // op 1: time conditioning (ncsnpp.py:223-246) + all Dense_0 projections
    float* temb_vec = bd.acquire((size_t)B * e->temb_total);
    {
        if (!e->dev.count("nx.temb.wp")) {
            std::vector<float> wp, bp;
            for (size_t i = 0; i < e->nx_mods.size(); ++i) {
                if (e->nx_mods[i].kind != NxMod::RES) continue;
                const std::string P = nx_name((int)i, "");
                const auto& w = W(e, P + "Dense_0.weight").data; wp.insert(wp.end(), w.begin(), w.end());
                const auto& b1 = W(e, P + "Dense_0.bias").data; const auto& b2 = W(e, P + "Conv_0.bias").data;
                for (size_t k = 0; k < b1.size(); ++k) bp.push_back(b1[k] + b2[k]);
            }
            upload(e, "nx.temb.wp", wp); upload(e, "nx.temb.bp", bp);
        }
        Op op{}; op.kind = OP_NX_TEMB;
        NxTembParams& t = op.ntp;
        t.Wf = upload(e, nx_name(0, "W"), W(e, nx_name(0, "W")).data);
        t.w0 = upload(e, nx_name(1, "weight"), W(e, nx_name(1, "weight")).data); t.b0 = upload(e, nx_name(1, "bias"), W(e, nx_name(1, "bias")).data);
        t.w1 = upload(e, nx_name(2, "weight"), W(e, nx_name(2, "weight")).data); t.b1 = upload(e, nx_name(2, "bias"), W(e, nx_name(2, "bias")).data);
        t.wp = e->dev.at("nx.temb.wp"); t.bp = e->dev.at("nx.temb.bp");
        t.out = temb_vec; t.B = B; t.nf = nf; t.total_out = e->temb_total;
        plan->ops.push_back(op);
    }
    int m_idx = 3;
    // image -> NHWC-32; first conv (ncsnpp.py:257-259)
    Tensor pyr_in = bd.make(32, H0, H0, false);
    { Op op{}; op.kind = OP_NX_IMG_IN; op.O = pyr_in.p; op.I[0] = chn; op.I[1] = H0; op.I[2] = H0; plan->ops.push_back(op); }
    std::vector<Tensor> hs;
    {
        const std::string wn = nx_name(m_idx, "weight");
        const HostTensor& w = W(e, wn);
        const std::string key = nx_derive(e, wn + "#pad32", {nf, 32, 3, 3}, [&](std::vector<float>& d) {
            for (int o = 0; o < nf; ++o) for (int i = 0; i < chn; ++i) for (int t = 0; t < 9; ++t) d[((size_t)o * 32 + i) * 9 + t] = w.data[((size_t)o * chn + i) * 9 + t];
        });
        Tensor t0 = bd.make(nf, H0, H0, true);
        ConvParams p = base_params(B, H0, H0, H0, H0, t0);
        packed_seg(e, p, pyr_in, 0, 9, 0, key, 0, 32);
        p.addvec = upload(e, nx_name(m_idx, "bias"), W(e, nx_name(m_idx, "bias")).data); p.addvec_bs = 0;
        push_conv(bd, p);
        hs.push_back(t0); plan->taps.push_back({"conv_in", t0});
        if (plan->retain) { TapeRec tr; tr.kind = TP_NX_CONV_IN; tr.idx = m_idx; tr.in0 = pyr_in; tr.out = t0; plan->tape.push_back(tr); }
        ++m_idx;
    }
    // down path (ncsnpp.py:260-299)
    int res = H0;
    for (int lvl = 0; lvl < nlev; ++lvl) {
        for (int blk = 0; blk < nres; ++blk) {
            Tensor h = nx_res_block(bd, m_idx++, hs.back(), nullptr, nullptr, temb_vec);
            if (in_attn(res)) {
                nx_alias_attn(e, m_idx);
                Tensor a = attn_block(bd, nx_name(m_idx, ""), h, nx_groups(h.C), s); ++m_idx;
                bd.release(h.p); h = a;
            }
            hs.push_back(h);
            snprintf(nm, sizeof nm, "down%d_%d", lvl, blk); plan->taps.push_back({nm, h});
        }
        if (lvl != nlev - 1) {
            // input_pyramid = pyramid_downsample(input_pyramid); h = Combine(input_pyramid, ResnetBlock(down)(hs[-1]))
            Tensor pd{}; nx_fir(bd, pyr_in, false, nullptr, nullptr, &pd);
            if (plan->retain) { TapeRec tr; tr.kind = TP_NX_PYR_DOWN; tr.in0 = pyr_in; tr.out = pd; plan->tape.push_back(tr); }
            bd.release(pyr_in.p); pyr_in = pd;
            Tensor h = nx_res_block(bd, m_idx, hs.back(), nullptr, &pyr_in, temb_vec); m_idx += 2;
            hs.push_back(h); res /= 2;
            snprintf(nm, sizeof nm, "downsample%d", lvl); plan->taps.push_back({nm, h});
        }
    }
    bd.release(pyr_in.p);
    // middle (ncsnpp.py:302-308)
    Tensor h = hs.back(); bool h_owned = false;
    {
        Tensor a = nx_res_block(bd, m_idx++, h, nullptr, nullptr, temb_vec);
        nx_alias_attn(e, m_idx);
        Tensor b2 = attn_block(bd, nx_name(m_idx, ""), a, nx_groups(a.C), s); ++m_idx; bd.release(a.p);
        Tensor c2 = nx_res_block(bd, m_idx++, b2, nullptr, nullptr, temb_vec); bd.release(b2.p);
        h = c2; h_owned = true; plan->taps.push_back({"mid", h});
    }
    // up path with the output-skip pyramid (ncsnpp.py:312-366)
    Tensor pyr{}; bool have_pyr = false;
    for (int lvl = nlev - 1; lvl >= 0; --lvl) {
        for (int blk = 0; blk < nres + 1; ++blk) {
            Tensor skip = hs.back(); hs.pop_back();
            Tensor o = nx_res_block(bd, m_idx++, h, &skip, nullptr, temb_vec);
            if (h_owned) bd.release(h.p);
            bd.release(skip.p);
            h = o; h_owned = true;
            snprintf(nm, sizeof nm, "up%d_%d", lvl, blk); plan->taps.push_back({nm, h});
        }
        if (in_attn(res)) {
            nx_alias_attn(e, m_idx);
            Tensor a = attn_block(bd, nx_name(m_idx, ""), h, nx_groups(h.C), s); ++m_idx;
            bd.release(h.p); h = a;
        }
        {
            // pyramid (+)= conv3x3(act(GroupNorm(h)))  with the C -> num_channels conv padded to 32 output channels
            const int gi = m_idx, ci = m_idx + 1; m_idx += 2;
            const HostTensor& w = W(e, nx_name(ci, "weight"));
            const int I = (int)w.shape[1];
            const std::string key = nx_derive(e, nx_name(ci, "weight") + "#out32", {32, I, 3, 3}, [&](std::vector<float>& d) {
                std::copy(w.data.begin(), w.data.end(), d.begin());
            });
            std::vector<float> b32(32, 0.f);
            { const auto& bb = W(e, nx_name(ci, "bias")).data; std::copy(bb.begin(), bb.end(), b32.begin()); }
            Tensor np = bd.make(32, h.H, h.W, false);
            ConvParams p = base_params(B, h.H, h.W, h.H, h.W, np);
            packed_seg(e, p, h, 2, 9, 0, key, 0, I);
            p.gn_C = h.C; p.gn_cpg = h.C / nx_groups(h.C);
            p.gamma = upload(e, nx_name(gi, "weight"), W(e, nx_name(gi, "weight")).data);
            p.beta = upload(e, nx_name(gi, "bias"), W(e, nx_name(gi, "bias")).data);
            p.addvec = upload(e, nx_name(ci, "bias") + "#32", b32); p.addvec_bs = 0;
            Tensor pu{};
            if (have_pyr) {
                nx_fir(bd, pyr, true, nullptr, nullptr, &pu);       // pyramid_upsample (ncsnpp.py:338)
                bd.release(pyr.p);
                p.residual = pu.p; p.res_cstride = 32;
            }
            push_conv(bd, p);
            if (plan->retain) {
                TapeRec tr; tr.kind = TP_NX_OUT_SKIP; tr.idx = gi; tr.in0 = h; tr.out = np; tr.has_old = have_pyr; if (have_pyr) tr.pyr_old = pyr;
                plan->tape.push_back(tr);
            }
            if (have_pyr) bd.release(pu.p);
            pyr = np; have_pyr = true;
        }
        if (lvl != 0) {
            Tensor o = nx_res_block(bd, m_idx++, h, nullptr, nullptr, temb_vec);
            bd.release(h.p); h = o; res *= 2;
            snprintf(nm, sizeof nm, "upsample%d", lvl); plan->taps.push_back({nm, h});
        }
    }
    if (m_idx != (int)e->nx_mods.size() || !hs.empty()) { e->err = "internal: NCSN++ module walk out of step"; return PF_ERR_INVALID; }
    plan->taps.push_back({"pyramid", pyr});
    if (plan->retain) plan->nx_sigma = bd.acquire((size_t)std::max(B, 64));
    { Op op{}; op.kind = OP_NX_IMG_OUT; op.P[0] = pyr.p; op.O = plan->nx_sigma; op.I[0] = chn; op.I[1] = H0; op.I[2] = H0; op.I[3] = c.scale_by_sigma; plan->ops.push_back(op); }
    plan->t_last = pyr;
    return PF_OK;
}
