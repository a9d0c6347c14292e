// stylegan2.cpp — StyleGAN2 host code: weights -> device layouts, and the launches of the mapping / style chain, the synthesis blocks
// and the discriminator.  The pass that strings them together: engine.cpp run_pass.
#include "engine.h"

#include <math.h>
#include <stdio.h>

int finalize_generator(glass_engine* e) {
    const glass_config& c = e->cfg;
    const int L = c.latent_size;
    char nm[256];
    // mapping network (stylegan2/models.py:566-588): weight coef = lr_mul/sqrt(fan_in), bias coef = lr_mul
    const float lr = 0.01f;
    for (int i = 0; i < c.mapping_layers; ++i) {
        snprintf(nm, sizeof nm, "G_mapping.main.%d.layer.weight", i);
        GET(w, nm);
        REQUIRE(numel(w) == (size_t)L * L, GLASS_ERR_ARG, std::string("bad shape: ") + nm);
        snprintf(nm, sizeof nm, "G_mapping.main.%d.bias", i);
        GET(b, nm);
        REQUIRE(numel(b) == (size_t)L, GLASS_ERR_ARG, std::string("bad shape: ") + nm);
        float *dw, *db;
        int rc = upload(e, &dw, transposed(w->data.data(), L, L, lr / sqrtf((float)L)));
        if (rc) return rc;
        rc = upload(e, &db, scaled(b->data.data(), L, lr));
        if (rc) return rc;
        e->map_wt.push_back(dw);
        e->map_b.push_back(db);
    }
    // layer list (stylegan2/models.py:812-896, 969-1014)
    int style_idx = 0, soff = 0, dsoff = 0, noise_idx = 0;
    for (int b = 0; b < c.n_blocks; ++b) {
        const int res = 4 << b;
        const int nl = b == 0 ? 1 : 2;
        for (int l = 0; l < nl; ++l) {
            GConv g;
            g.up = (b > 0 && l == 0);
            g.cin = (b == 0) ? c.channels[0] : (l == 0 ? c.channels[b - 1] : c.channels[b]);
            g.cout = c.channels[b];
            g.res_out = res;
            g.res_in = g.up ? res / 2 : res;
            g.style_idx = style_idx++;
            g.style_off = soff;
            soff += g.cin;
            g.ds_off = dsoff;
            dsoff += g.cout;
            g.noise_idx = noise_idx++;
            e->gconv.push_back(g);
        }
        GRgb r;
        r.cin = c.channels[b];
        r.res = res;
        r.style_idx = style_idx++;
        r.style_off = soff;
        soff += r.cin;
        e->grgb.push_back(r);
    }
    e->n_style = style_idx;
    e->S_total = soff;
    e->D_total = dsoff;
    // style affines, concatenated: s = w @ (A/sqrt(L))^T + b   (modules.py:879-894, 936)
    std::vector<float> swt((size_t)L * e->S_total), sb((size_t)e->S_total);
    e->style_off.assign(e->n_style, 0);
    e->style_len.assign(e->n_style, 0);
    auto add_style = [&](const std::string& prefix, int sidx, int off, int cin) -> int {
        GET(A, prefix + ".dense.layer.weight");
        GET(Ab, prefix + ".dense.bias");
        REQUIRE(numel(A) == (size_t)cin * L && numel(Ab) == (size_t)cin, GLASS_ERR_ARG, "bad style shape: " + prefix);
        const float coef = 1.0f / sqrtf((float)L);
        for (int i = 0; i < cin; ++i) {
            for (int k = 0; k < L; ++k) swt[(size_t)k * e->S_total + off + i] = A->data[(size_t)i * L + k] * coef;
            sb[off + i] = Ab->data[i];
        }
        e->style_off[sidx] = off;
        e->style_len[sidx] = cin;
        return GLASS_OK;
    };
    {
        GET(cst, "G_synthesis.const");
        const int C0 = c.channels[0];
        REQUIRE(numel(cst) == (size_t)C0 * 16, GLASS_ERR_ARG, "bad shape: G_synthesis.const");
        std::vector<_Float16> h((size_t)16 * C0);
        for (int ch = 0; ch < C0; ++ch)
            for (int p = 0; p < 16; ++p) h[(size_t)p * C0 + ch] = (_Float16)cst->data[(size_t)ch * 16 + p];
        int rc = upload(e, &e->g_const, h);
        if (rc) return rc;
    }
    int gi = 0;
    for (int b = 0; b < c.n_blocks; ++b) {
        const int nl = b == 0 ? 1 : 2;
        for (int l = 0; l < nl; ++l, ++gi) {
            GConv& g = e->gconv[gi];
            snprintf(nm, sizeof nm, "G_synthesis.conv_blocks.%d.conv_block.%d", b, l);
            const std::string p = nm;
            GET(W, p + ".layer.layer.weight");
            GET(bias, p + ".bias");
            GET(ns, p + ".layer.weight");
            REQUIRE(numel(W) == (size_t)g.cout * g.cin * 9 && numel(bias) == (size_t)g.cout && numel(ns) == 1,
                    GLASS_ERR_ARG, "bad conv shape: " + p);
            int rc = add_style(p + ".layer.layer", g.style_idx, g.style_off, g.cin);
            if (rc) return rc;
            std::vector<_Float16> packed;
            if (g.up) glass_fold_upconv(W->data.data(), g.cout, g.cin, packed);
            else glass_pack_conv(W->data.data(), g.cout, g.cin, 3, g.cin, packed);
            rc = upload(e, &g.w, packed);
            if (rc) return rc;
            if (g.up) {
                glass_pack_conv(W->data.data(), g.cout, g.cin, 3, g.cin, packed);
                rc = upload(e, &g.w_up, packed);
                if (rc) return rc;
            }
            // demod table: Wsq[i][o] = sum_taps (W*coef)^2   (modules.py:943-954, SURVEY 8a note 1)
            std::vector<float> wsq((size_t)g.cin * g.cout);
            const float coef2 = 1.0f / ((float)g.cin * 9.f);
            for (int o = 0; o < g.cout; ++o)
                for (int i = 0; i < g.cin; ++i) {
                    const float* w = W->data.data() + ((size_t)o * g.cin + i) * 9;
                    float s = 0.f;
                    for (int t = 0; t < 9; ++t) s += w[t] * w[t];
                    wsq[(size_t)i * g.cout + o] = s * coef2;
                }
            rc = upload(e, &g.wsq, wsq);
            if (rc) return rc;
            rc = upload(e, &g.bias, bias->data);
            if (rc) return rc;
            g.noise_strength = ns->data[0];
        }
        GRgb& r = e->grgb[b];
        snprintf(nm, sizeof nm, "G_synthesis.to_data_layers.%d", b);
        const std::string p = nm;
        GET(W, p + ".layer.weight");
        GET(bias, p + ".bias");
        REQUIRE(numel(W) == (size_t)3 * r.cin && numel(bias) == 3, GLASS_ERR_ARG, "bad toRGB shape: " + p);
        int rc = add_style(p + ".layer", r.style_idx, r.style_off, r.cin);
        if (rc) return rc;
        rc = upload(e, &r.w, scaled(W->data.data(), (size_t)3 * r.cin, 1.0f / sqrtf((float)r.cin)));
        if (rc) return rc;
        rc = upload(e, &r.bias, bias->data);
        if (rc) return rc;
    }
    int rc = upload(e, &e->style_wt, swt);
    if (rc) return rc;
    rc = upload(e, &e->style_b, sb);
    if (rc) return rc;
    rc = upload(e, &e->d_style_off, e->style_off);
    if (rc) return rc;
    rc = upload(e, &e->d_style_len, e->style_len);
    if (rc) return rc;
    // dlatent_avg (stylegan2/models.py:225-226: a buffer of the Generator itself), optional: only the truncation trick reads it
    if (const HostTensor* avg = find(e, "dlatent_avg")) {
        REQUIRE(numel(avg) == (size_t)L, GLASS_ERR_ARG, "bad shape: dlatent_avg (expected [latent_size])");
        e->dlatent_avg = avg->data;
    }
    const LatPlan lp = plan_dlatents(e->latent_space, e->trunc_psi, e->trunc_cutoff, e->n_lat);
    REQUIRE(!lp.expand || !e->dlatent_avg.empty(), GLASS_ERR_STATE, "missing tensor: dlatent_avg (truncation psi != 1 interpolates towards it)");
    const bool sub = e->latent_space == GLASS_LATENT_SUB;
    if (sub) {
        REQUIRE(e->sub_K > 0, GLASS_ERR_STATE, "finalize: latent space sub needs its shape: set_subspace_shape(groups, components) before finalize");
        REQUIRE((long long)c.max_pop * e->sub_G * e->sub_K < (1LL << 31), GLASS_ERR_ARG, "finalize: max_pop * groups * components must stay below 2^31");
    }
    if (e->latent_space == GLASS_LATENT_WPLUS || sub || e->trunc_before_finalize) {
        // per-layer rows: the [max_pop][n_lat][L] buffer, and the (segment, n0) tiles of styles_layered_kernel.  Style layer -> dlatent index
        // (models.py:969-1014): conv i in execution order reads row i; the toRGB of block b reads the row of the next block's first conv,
        // 2 b + 1 — which for the last block is the last row.
        std::vector<int> lat(e->n_style, 0);
        for (size_t i = 0; i < e->gconv.size(); ++i) lat[e->gconv[i].style_idx] = (int)i;
        for (int b = 0; b < c.n_blocks; ++b) lat[e->grgb[b].style_idx] = 2 * b + 1;
        std::vector<StyleTile> tiles;
        for (int j = 0; j < e->n_style; ++j)
            for (int n0 = 0; n0 < e->style_len[j]; n0 += 64)
                tiles.push_back(StyleTile{e->style_off[j] + n0, std::min(64, e->style_len[j] - n0), lat[j], 0});
        e->n_style_tiles = (int)tiles.size();
        if ((rc = upload(e, &e->d_style_tiles, tiles))) return rc;
        if ((rc = dev_alloc(e, &e->d_dlat, (size_t)c.max_pop * e->n_lat * L))) return rc;
    }
    if (sub) {      // coefficient rows, and the operands glass_engine_set_subspace fills
        if ((rc = dev_alloc(e, &e->d_sub_c, (size_t)c.max_pop * e->sub_G * e->sub_K))) return rc;
        if ((rc = dev_alloc(e, &e->d_sub_group, (size_t)e->n_lat))) return rc;
        if ((rc = dev_alloc(e, &e->d_sub_basis, (size_t)e->sub_K * L))) return rc;
        if ((rc = dev_alloc(e, &e->d_sub_base, (size_t)e->n_lat * L))) return rc;
    }
    return lp.expand ? upload_lat_table(e) : GLASS_OK;
}

LatPlan plan_dlatents(int space, float psi, int cutoff, int n_lat) {
    const int ncut = cutoff < 0 ? n_lat : cutoff;
    LatPlan lp;
    lp.map = space == GLASS_LATENT_Z;
    lp.expand = psi != 1.f && ncut > 0;                                          // models.py:276
    lp.layered = space == GLASS_LATENT_WPLUS || space == GLASS_LATENT_SUB || (lp.expand && ncut < n_lat);    // otherwise one row serves every layer
    return lp;
}

size_t latent_row_floats(const glass_engine* e) {
    if (e->latent_space == GLASS_LATENT_SUB) return (size_t)e->sub_G * e->sub_K;      // coefficients, group-major (0 until the shape is set)
    return (size_t)e->cfg.latent_size * (e->latent_space == GLASS_LATENT_WPLUS ? (size_t)e->n_lat : 1);
}

float* latent_rows_dst(const glass_engine* e) {
    switch (e->latent_space) {
        case GLASS_LATENT_SUB: return e->d_sub_c;
        case GLASS_LATENT_WPLUS: return e->d_dlat;
        case GLASS_LATENT_W: return e->d_w0;
        default: return e->d_z;
    }
}

int upload_lat_table(glass_engine* e) {
    const int L = e->cfg.latent_size;
    e->lat_pad = (e->n_lat + 3) / 4 * 4;
    std::vector<float> tab((size_t)e->lat_pad + L, 1.f);
    if (int rc = glass_host_layer_psi(e->n_lat, e->trunc_psi, e->trunc_cutoff, tab.data())) return rc;
    std::copy(e->dlatent_avg.begin(), e->dlatent_avg.end(), tab.begin() + e->lat_pad);
    if (!e->d_lat_tab)
        if (int rc = dev_alloc(e, &e->d_lat_tab, tab.size())) return rc;
    GLASS_HIP(hipMemcpy(e->d_lat_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    return GLASS_OK;
}

int finalize_discriminator(glass_engine* e) {
    const glass_config& c = e->cfg;
    const int n = c.n_blocks;
    char nm[256];
    auto chD = [&](int i) { return c.channels[n - 1 - i]; };  // D order: first (full res) -> last (4x4)
    {
        GET(W, "D.from_data_layers.0.layer.weight");
        GET(b, "D.from_data_layers.0.bias");
        REQUIRE(numel(W) == (size_t)chD(0) * 3 && numel(b) == (size_t)chD(0), GLASS_ERR_ARG, "bad fromRGB shape");
        int rc = upload(e, &e->d_frgb_w, scaled(W->data.data(), numel(W), 1.0f / sqrtf(3.f)));
        if (rc) return rc;
        rc = upload(e, &e->d_frgb_b, b->data);
        if (rc) return rc;
    }
    for (int i = 0; i < n - 1; ++i) {
        DBlock d;
        d.cin = chD(i);
        d.cout = chD(i + 1);
        d.res = e->R >> i;
        snprintf(nm, sizeof nm, "D.conv_blocks.%d", i);
        const std::string p = nm;
        GET(W0, p + ".conv_block.0.layer.weight");
        GET(B0, p + ".conv_block.0.bias");
        GET(W1, p + ".conv_block.1.layer.weight");
        GET(B1, p + ".conv_block.1.bias");
        GET(WS, p + ".projection.weight");
        REQUIRE(numel(W0) == (size_t)d.cin * d.cin * 9 && numel(W1) == (size_t)d.cout * d.cin * 9 &&
                    numel(WS) == (size_t)d.cout * d.cin && numel(B0) == (size_t)d.cin && numel(B1) == (size_t)d.cout,
                GLASS_ERR_ARG, "bad D block shape: " + p);
        std::vector<_Float16> pk;
        glass_pack_conv(W0->data.data(), d.cin, d.cin, 3, d.cin, pk);
        int rc = upload(e, &d.w0, pk);
        if (rc) return rc;
        glass_pack_conv(W1->data.data(), d.cout, d.cin, 3, d.cin, pk);
        rc = upload(e, &d.w1, pk);
        if (rc) return rc;
        glass_pack_conv(WS->data.data(), d.cout, d.cin, 1, d.cin, pk);
        rc = upload(e, &d.wskip, pk);
        if (rc) return rc;
        rc = upload(e, &d.b0, B0->data);
        if (rc) return rc;
        rc = upload(e, &d.b1, B1->data);
        if (rc) return rc;
        e->dblk.push_back(d);
    }
    const int CL = chD(n - 1);
    snprintf(nm, sizeof nm, "D.conv_blocks.%d.1.conv_block.0", n - 1);
    const std::string p = nm;
    GET(WF, p + ".layer.weight");
    GET(BF, p + ".bias");
    REQUIRE(numel(WF) == (size_t)CL * (CL + 1) * 9 && numel(BF) == (size_t)CL, GLASS_ERR_ARG, "bad D final conv shape");
    e->d_final_cpad = ((CL + 1 + 15) / 16) * 16;
    std::vector<_Float16> pk;
    glass_pack_conv(WF->data.data(), CL, CL + 1, 3, e->d_final_cpad, pk);
    int rc = upload(e, &e->d_final_w, pk);
    if (rc) return rc;
    rc = upload(e, &e->d_final_b, BF->data);
    if (rc) return rc;
    GET(W0, "D.dense.0.layer.weight");
    GET(B0, "D.dense.0.bias");
    GET(W1, "D.dense.1.layer.weight");
    GET(B1, "D.dense.1.bias");
    REQUIRE(numel(W0) == (size_t)CL * CL * 16 && numel(B0) == (size_t)CL && numel(W1) == (size_t)CL && numel(B1) == 1,
            GLASS_ERR_ARG, "bad D dense shape");
    // x.view(B,-1) flattens NCHW (models.py:1224): column c*16+p ; our activations are [p][c].
    std::vector<_Float16> d0((size_t)CL * CL * 16);
    const float coef0 = 1.0f / sqrtf((float)CL * 16.f);
    for (int o = 0; o < CL; ++o)
        for (int ch = 0; ch < CL; ++ch)
            for (int px = 0; px < 16; ++px)
                d0[(size_t)o * CL * 16 + (size_t)px * CL + ch] = (_Float16)(W0->data[(size_t)o * CL * 16 + ch * 16 + px] * coef0);
    rc = upload(e, &e->d_dense0_w, d0);
    if (rc) return rc;
    rc = upload(e, &e->d_dense0_b, B0->data);
    if (rc) return rc;
    rc = upload(e, &e->d_dense1_wt, transposed(W1->data.data(), 1, CL, 1.0f / sqrtf((float)CL)));
    if (rc) return rc;
    return upload(e, &e->d_dense1_b, B1->data);
}

int upload_noise(glass_engine* e, int P, int generation, int first_mb, const glass_noise* noise) {
    const glass_config& c = e->cfg;
    const int n_mb = P / c.batch_size;
    if (c.noise_mode == 1) {
        for (size_t l = 0; l < e->gconv.size(); ++l) {
            const int hw = e->gconv[l].res_out * e->gconv[l].res_out;
            Prof pr(e, "noise", 0, (double)n_mb * hw * 4);
            launch_noise(e->d_noise[l], n_mb, hw, (uint32_t)l, (uint32_t)first_mb, (uint32_t)generation, c.noise_seed,
                         e->cur, (uint32_t)e->noise_period);
        }
    } else if (c.noise_mode == 2) {
        REQUIRE(noise && noise->planes, GLASS_ERR_ARG, "noise_mode 2 requires caller-provided noise planes");
        REQUIRE(noise->n_layers == (int)e->gconv.size() && noise->n_minibatches >= n_mb, GLASS_ERR_ARG,
                "noise: wrong number of layers / minibatches");
        for (int m = 0; m < n_mb; ++m)
            for (size_t l = 0; l < e->gconv.size(); ++l) {
                const size_t hw = (size_t)e->gconv[l].res_out * e->gconv[l].res_out;
                const float* src = noise->planes[(size_t)m * noise->n_layers + l];
                REQUIRE(src, GLASS_ERR_ARG, "noise: null plane");
                GLASS_HIP(hipMemcpyAsync(e->d_noise[l] + (size_t)m * hw, src, hw * sizeof(float), hipMemcpyHostToDevice,
                                         e->cur));
            }
        GLASS_HIP(hipStreamSynchronize(e->cur));  // caller's planes may be freed after return
    }
    return GLASS_OK;
}

void run_mapping(glass_engine* e, int P) {
    const glass_config& c = e->cfg;
    const int L = c.latent_size;
    Prof pr(e, "mapping", 2.0 * P * L * L * c.mapping_layers, 4.0 * L * L * c.mapping_layers);
    launch_mapping(e->d_z, e->d_w0, e->d_w1, P, L, 1e-8f, e->map_wt.data(), e->map_b.data(), c.mapping_layers, 0, e->cur);
}

// The uploaded rows are in d_z (space z), d_w0 (w), d_dlat (w+) or d_sub_c (sub): run_pass put them there.
bool run_dlatents(glass_engine* e, int P) {
    const glass_config& c = e->cfg;
    const int L = c.latent_size, NL = e->n_lat;
    const LatPlan lp = plan_dlatents(e->latent_space, e->trunc_psi, e->trunc_cutoff, NL);
    if (lp.layered && !e->d_dlat) {   // (the setters refuse this; a pass never reads a buffer that is not there)
        if (e->launch_error.empty()) e->launch_error = "per-layer dlatents without their buffer";
        return false;
    }
    if (lp.map) run_mapping(e, P);
    const bool sub = e->latent_space == GLASS_LATENT_SUB;
    if (sub) {      // coefficients -> per-layer dlatents, frozen layers included; truncation then runs on them as on w+ rows
        const int G = e->sub_G, K = e->sub_K;
        if (!e->has_subspace) {      // (run_pass and the setters refuse this)
            if (e->launch_error.empty()) e->launch_error = "set_subspace() first";
            return false;
        }
        Prof pr(e, "dlatents.sub", 2.0 * P * G * K * L, 4.0 * ((double)P * G * K + (double)K * L + (double)NL * L + (double)P * NL * L));
        if (!launch_dlatent_subspace(e->d_sub_c, P, G, K, e->d_sub_group, NL, L, e->d_sub_basis, e->d_sub_base, e->d_dlat, e->cur)) {
            pr.drop();
            if (e->launch_error.empty()) e->launch_error = "no kernel accepts layer dlatents.sub (dlatent_subspace: shape outside its limits)";
            return false;
        }
    }
    if (lp.expand) {
        const int nl = lp.layered ? NL : 1;
        Prof pr(e, "dlatents", 3.0 * P * nl * L, 4.0 * L * (P * (double)(nl + (e->latent_space == GLASS_LATENT_WPLUS || sub ? nl : 1)) + 1));
        if (!lp.layered) launch_dlatent_expand(e->d_w0, L, 0, e->d_w0, e->d_lat_tab, e->lat_pad, 1, P, L, e->cur);                       // in place
        else if (e->latent_space == GLASS_LATENT_WPLUS || sub) launch_dlatent_expand(e->d_dlat, (long long)NL * L, L, e->d_dlat, e->d_lat_tab, e->lat_pad, NL, P, L, e->cur);   // in place
        else launch_dlatent_expand(e->d_w0, L, 0, e->d_dlat, e->d_lat_tab, e->lat_pad, NL, P, L, e->cur);
    }
    return true;
}

void run_styles(glass_engine* e, int P) {
    const glass_config& c = e->cfg;
    const int L = c.latent_size, NL = e->n_lat;
    const LatPlan lp = plan_dlatents(e->latent_space, e->trunc_psi, e->trunc_cutoff, NL);
    if (!run_dlatents(e, P)) return;
    {
        Prof pr(e, "styles", 2.0 * P * L * e->S_total, 4.0 * L * e->S_total + (lp.layered ? 4.0 * P * NL * L : 0.0));
        if (lp.layered)
            launch_styles_layered(e->d_dlat, NL, L, P, e->style_wt, e->S_total, e->style_b, e->d_s, e->d_style_tiles, e->n_style_tiles, e->cur);
        else
            launch_dense(e->d_w0, L, P, L, e->style_wt, e->S_total, e->style_b, e->d_s, e->S_total, 0, 0, nullptr, 0, e->cur);
        launch_style_norm(e->d_s, e->S_total, P, e->n_style, e->d_style_off, e->d_style_len, e->d_smax, e->d_epsrow,
                          1e-8f, e->cur);
        launch_bg_to_half(e->d_s, e->d_s16, (long long)P * e->S_total, e->cur);   // fp16 table for the LDS-tiled kernels
    }
    {
        Prof pr(e, "demod", 0, 0);
        launch_dense_multi((const DenseDesc*)e->d_demod_desc, (int)e->gconv.size(), e->demod_max_n, P, 1, 2, e->cur);
    }
    {
        Prof pr(e, "premod_weights", 0, 0);
        for (auto& g : e->gconv)
            if (g.premod)
                launch_modulate_weights(g.up ? g.w_up : g.w, g.welems, g.cin, g.cout, e->d_s + g.style_off, e->S_total,
                                        e->d_dscale + g.ds_off, e->D_total, P, g.wm, e->cur);
    }
}

static ConvParams g_conv_params(glass_engine* e, const GConv& g, int c0, int B, const half_t* x, long long xbs, half_t* out) {
    const glass_config& c = e->cfg;
    ConvParams p = conv_defaults();
    p.x = x; p.x_bstride = xbs; p.B = B; p.H = p.W = g.res_in; p.Cin = g.cin; p.Hc = p.Wc = g.res_in; p.KS = 3; p.pad = 1;
    p.w = g.w; p.w_up = g.w_up; p.Cout = g.cout; p.up = g.up; p.Neff = g.up ? 4 * g.cout : g.cout; p.Ho = p.Wo = g.res_out;
    p.sn = e->d_s + (size_t)c0 * e->S_total + g.style_off; p.sn16 = e->d_s16 + (size_t)c0 * e->S_total + g.style_off; p.sn_stride = e->S_total;
    p.dscale = e->d_dscale + (size_t)c0 * e->D_total + g.ds_off; p.ds_stride = e->D_total;
    if (c.noise_mode != 0) { p.noise = e->d_noise[g.noise_idx] + (size_t)(c0 / c.batch_size) * g.res_out * g.res_out; p.noise_strength = g.noise_strength; }
    p.batch_size = c.batch_size; p.bias = g.bias; p.act = 1; p.y = out;
    if (g.premod) {   // weights already carry style and demod of each sample
        p.sn = nullptr; p.sn16 = nullptr; p.dscale = nullptr; p.w_bstride = g.welems;
        if (g.up) { p.w_up = g.wm + (size_t)c0 * g.welems; p.w = nullptr; }
        else p.w = g.wm + (size_t)c0 * g.welems;
    }
    return p;
}

struct GCost { char tag[48]; double flops, bytes; };
static GCost g_conv_cost(const GConv& g, int B) {
    GCost k;
    k.flops = 2.0 * B * (double)g.res_in * g.res_in * 9.0 * g.cin * g.cout;  // reference count
    k.bytes = 2.0 * B * ((double)g.res_in * g.res_in * g.cin + (double)g.res_out * g.res_out * g.cout) + 2.0 * 9 * g.cin * (g.up ? 4 * g.cout : g.cout);
    snprintf(k.tag, sizeof k.tag, "G.%s.r%d.%dx%d", g.up ? "upconv" : "conv", g.res_out, g.cin, g.cout);
    return k;
}

// upconv -> conv link: the up-conv's only consumer is the block's second conv.
//   post_style: where the fused up-conv kernel runs and that conv modulates on the activation side, its style is applied once, to the
//     up-conv's output.
//   planar: conv_wreg reads its input one 32-channel chunk at a time, so the up-conv writes the map chunk-planar for it (common.h
//     x_planar8) — where the up-conv instance that can runs and conv_wreg takes the consumer as it will be launched.
struct UpLink { bool post_style = false, planar = false; };
// p: the up-conv; next: its consumer as g_conv_params builds it
static UpLink up_link(const ConvParams& p, ConvParams next, bool next_premod) {
    UpLink k;
    k.post_style = !next_premod && choose_conv_upfir(p);
    if (!k.post_style && !next_premod) return k;
    next.sn = nullptr; next.sn16 = nullptr; next.x_planar8 = 1;      // (as run_g_blocks launches it behind a post_style up-conv)
    ConvParams q = p;
    q.y_planar8 = 1;
    k.planar = choose_conv_wreg(next) && choose_conv_upfir(q);
    return k;
}

// toRGB of the block fused into its last conv (common.h).
//   stream_only: the network's LAST conv feeds toRGB only: conv_stream<torgb> writes just the skip image and the 64-byte-per-pixel feature
//     map never goes to HBM.
//   epilogue: up to 128 channels (one n tile per pixel) the conv's epilogue writes the skip image itself; the block still stores its map
//     (the next block reads it) but toRGB no longer re-reads it.
//   partial: blocks wider than that (several 128-wide n tiles per pixel): every n tile's conv epilogue writes the toRGB partial sum of its
//     channels, a 3-value-per-pixel pass adds them (+ bias + the upsampled previous image) — the separate toRGB pass read the whole feature
//     map again (0.19 + 0.09 + 0.03 ms at r128 / r64 / r32).
enum class ToRgb { separate, stream_only, epilogue, partial };

static half_t* trgb_tab(glass_engine* e, int c0, ToRgb form) { return e->d_trgb_tab + (size_t)c0 * 32 * (form == ToRgb::partial ? 512 : 128); }
static ConvParams torgb_conv_params(glass_engine* e, ConvParams q, const GRgb& r, int c0, ToRgb form, const float* yprev, float* yout) {
    q.trgb_w = r.w; q.trgb_b = r.bias;
    q.trgb_sn = e->d_s + (size_t)c0 * e->S_total + r.style_off; q.trgb_sn_stride = e->S_total;
    q.trgb_smax = e->d_smax + (size_t)c0 * e->n_style + r.style_idx; q.trgb_smax_stride = e->n_style;
    if (form == ToRgb::partial) q.trgb_part = e->d_trgb_part;
    else { q.trgb_yprev = yprev; q.trgb_yout = yout; }
    if (form == ToRgb::stream_only) q.y = nullptr;
    else q.trgb_tab = trgb_tab(e, c0, form);
    return q;
}
static void run_trgb_tables(glass_engine* e, const ConvParams& q, half_t* tab) {
    launch_trgb_tables(q.trgb_w, q.trgb_sn, q.trgb_sn_stride, q.trgb_smax, q.trgb_smax_stride, q.B, q.Cout, tab, e->cur);
}
// the form, and for every form but `separate` the kernel that runs the conv in it
static ToRgb choose_torgb(glass_engine* e, const ConvParams& p, const GRgb& r, int c0, bool last_block, const float* yprev, float* yout, ConvKernel* k) {
    if (last_block && (*k = choose_conv_stream(torgb_conv_params(e, p, r, c0, ToRgb::stream_only, yprev, yout)))) return ToRgb::stream_only;
    const bool wide = r.cin > 128;
    if (wide && !(e->d_trgb_part && r.cin % 128 == 0 && r.cin <= 512)) return ToRgb::separate;
    const ToRgb form = wide ? ToRgb::partial : ToRgb::epilogue;
    *k = choose_conv(torgb_conv_params(e, p, r, c0, form, yprev, yout));
    return *k ? form : ToRgb::separate;
}

// ------------------------------------------------------------------------------------
// Synthesis blocks [b_lo, b_hi) for candidates [c0, c0+B).  Low-resolution blocks
// (res <= low_res) run once for the whole population (launch-/latency-bound otherwise),
// high-resolution blocks run per chunk so the working set stays near the caches.
//   x/xbs: input feature map (bstride 0 = the learned const); pp[2]: ping-pong outputs;
//   yprev: skip image of the previous block (nullptr for block 0); yb[2]: skip ping-pong.
// Returns the final feature map / skip image through the out parameters.
// ------------------------------------------------------------------------------------
void run_g_blocks(glass_engine* e, int c0, int B, int b_lo, int b_hi, const half_t* x, long long xbs, half_t* const pp[2],
                  const float* yprev, float* const yb[2], const half_t** x_out, const float** y_out) {
    int yi = 0;
    for (int b = b_lo; b < b_hi; ++b) {
        UpLink link;
        if (b > 0) {
            const GConv &g = e->gconv[2 * b - 1], &next = e->gconv[2 * b];
            half_t* out = pp[(x == pp[0]) ? 1 : 0];
            ConvParams p = g_conv_params(e, g, c0, B, x, xbs, out);
            link = up_link(p, g_conv_params(e, next, c0, B, out, (long long)g.res_out * g.res_out * g.cout, pp[out == pp[0] ? 1 : 0]), next.premod);
            if (link.post_style) { p.post_scale16 = e->d_s16 + (size_t)c0 * e->S_total + next.style_off; p.post_stride = e->S_total; }
            p.y_planar8 = link.planar;
            const GCost k = g_conv_cost(g, B);
            run_conv(e, p, k.tag, k.flops, k.bytes);
            x = out;
            xbs = (long long)g.res_out * g.res_out * g.cout;
        }
        const GConv& g = e->gconv[2 * b];
        const GRgb& r = e->grgb[b];
        half_t* out = pp[(x == pp[0]) ? 1 : 0];
        ConvParams p = g_conv_params(e, g, c0, B, x, xbs, out);
        if (link.post_style) { p.sn = nullptr; p.sn16 = nullptr; }
        p.x_planar8 = link.planar;
        const GCost k = g_conv_cost(g, B);
        const double px = B * (double)r.res * r.res, tflops = k.flops + 2.0 * px * 3 * r.cin, yup = b ? 3.0 : 0.0;
        ConvKernel fused;
        const ToRgb form = choose_torgb(e, p, r, c0, b == e->cfg.n_blocks - 1, yprev, yb[yi], &fused);
        const ConvParams q = torgb_conv_params(e, p, r, c0, form, yprev, yb[yi]);
        x = out;
        xbs = (long long)g.res_out * g.res_out * g.cout;
        switch (form) {
        case ToRgb::stream_only: {
            run_chosen(e, fused, q, k.tag, tflops, 2.0 * B * (double)g.res_in * g.res_in * g.cin + px * (12.0 + yup));
            x = nullptr;   // not produced
            break;
        }
        case ToRgb::epilogue: {
            Prof pr(e, k.tag, tflops, k.bytes + px * (12.0 + yup));
            run_trgb_tables(e, q, trgb_tab(e, c0, form));
            fused.launch(q, e->cur);
            pr.ran(k.tag, fused.name);
            break;
        }
        case ToRgb::partial: {
            Prof pr(e, k.tag, tflops, k.bytes + px * (12.0 * (1 + 2 * (r.cin / 128)) + yup));
            run_trgb_tables(e, q, trgb_tab(e, c0, form));
            fused.launch(q, e->cur);
            launch_trgb_finish(e->d_trgb_part, r.cin / 128, B, r.res, r.bias, yprev, yb[yi], e->cur);
            pr.ran(k.tag, fused.name);
            break;
        }
        case ToRgb::separate: {
            run_conv(e, p, k.tag, k.flops, k.bytes);
            char tag[48];
            snprintf(tag, sizeof tag, "G.torgb.r%d", r.res);
            Prof pr(e, tag, 2.0 * px * 3 * r.cin, px * (2.0 * r.cin + 12.0 + yup));
            const bool ok = launch_torgb(x, B, r.res, r.res, r.cin, r.w, r.bias, q.trgb_sn, e->S_total, q.trgb_smax, e->n_style, yprev, yb[yi], e->cur);
            if (!ok && e->launch_error.empty()) e->launch_error = std::string("toRGB width not instantiated: ") + tag;
            break;
        }
        }
        yprev = yb[yi];
        yi ^= 1;
    }
    *x_out = x;
    *y_out = yprev;
}

void run_fromrgb(glass_engine* e, int B, const float* y, half_t* X) {
    const glass_config& c = e->cfg;
    const int n = c.n_blocks;
    Prof pr(e, "D.fromrgb", 2.0 * B * (double)e->R * e->R * 3 * c.channels[n - 1],
            B * (double)e->R * e->R * (12.0 + 2.0 * c.channels[n - 1]));
    launch_fromrgb(y, B, e->R, c.channels[n - 1], e->d_frgb_w, e->d_frgb_b, X, e->cur);
}

// the whole block from the skip image in one kernel (conv_d0.hip): neither x nor h reaches HBM.  false: the block does not qualify
static bool run_d_block0(glass_engine* e, int B, const DBlock& d, const float* rgb_y, half_t* O, bool planar) {
    char tag[64];
    const int r = d.res, r2 = r / 2;
    snprintf(tag, sizeof tag, "D.block0.r%d.%dx%dx%d", r, d.cin, d.cin, d.cout);
    const double px = (double)B * r * r, px2 = (double)B * r2 * r2;
    Prof pr(e, tag, 2.0 * px * (9.0 * d.cin * d.cin + 3.0 * d.cin) + 2.0 * px2 * 10.0 * d.cin * d.cout, px * 12.0 + px2 * 2.0 * d.cout);
    const char* k = launch_dblock0(rgb_y, e->d_frgb_w, e->d_frgb_b, d.w0, d.b0, d.w1, d.wskip, d.b1, O, B, r, d.cin, d.cout, e->cur, planar);
    if (k) pr.ran(tag, k);
    else pr.drop();
    return k != nullptr;
}

// The block's first conv, h = conv0(x) in Hb, as run_d_conv0 launches it.  XS != nullptr: with the blur-down of x (the skip branch's input) as a by-product
static ConvParams d_conv0_params(int B, const DBlock& d, const half_t* X, bool x_planar, half_t* Hb, half_t* XS) {
    const int r = d.res;
    ConvParams p = conv_defaults();
    p.x = X; p.x_bstride = (long long)r * r * d.cin; p.B = B; p.H = p.W = r; p.Cin = d.cin;
    p.Hc = p.Wc = r; p.KS = 3; p.pad = 1; p.w = d.w0; p.Cout = p.Neff = d.cin; p.Ho = p.Wo = r;
    p.bias = d.b0; p.act = 1; p.y = Hb; p.x_planar8 = x_planar; p.xs_out = XS;
    return p;
}

// First half of a block: h = conv0(x) in Hb.  Returns whether the launch also wrote XS, the blur-down of x that the skip branch reads.
// rgb_y != nullptr: X has NOT been produced yet — the conv builds the fromRGB map from the skip image on the fly and writes it to X
// (or, where the fused second half follows, its blur-down to XS) as a side output (conv_stream<fromrgb>), or, where that kernel does not
// apply, the separate fromRGB pass runs first.
static bool run_d_conv0(glass_engine* e, int B, const DBlock& d, half_t* X, bool x_planar, const float* rgb_y, half_t* Hb, half_t* XS) {
    char tag[64];
    const int r = d.res;
    const ConvParams p = d_conv0_params(B, d, X, x_planar, Hb, nullptr);
    if (rgb_y) {
        const bool fuse_down = conv_down_supported(r, d.cin, d.cout);
        ConvParams q = p;
        q.rgb_y = rgb_y; q.rgb_w = e->d_frgb_w; q.rgb_b = e->d_frgb_b;
        q.rgb_x_out = fuse_down ? nullptr : X;       // the fused second half reads the down-sampled skip input only
        q.rgb_xs_out = fuse_down ? XS : nullptr;
        if (const ConvKernel k = choose_conv_stream(q)) {
            snprintf(tag, sizeof tag, "D.fromrgb+conv0.r%d.%dx%d", r, d.cin, d.cin);
            const double px = (double)B * r * r;
            run_chosen(e, k, q, tag, 2.0 * px * (9.0 * d.cin * d.cin + 3.0 * d.cin), px * (12.0 + 2.0 * d.cin + (fuse_down ? 0.5 : 2.0) * d.cin));
            return fuse_down;
        }
        run_fromrgb(e, B, rgb_y, X);
    }
    const ConvParams qx = d_conv0_params(B, d, X, x_planar, Hb, XS);
    const ConvKernel kx = choose_conv(qx);           // the skip branch's blur-down rides in the first conv where a family does that
    snprintf(tag, sizeof tag, "D.conv0.r%d.%dx%d", r, d.cin, d.cin);
    const double flops = 2.0 * B * (double)r * r * 9 * d.cin * d.cin, bytes = 4.0 * B * (double)r * r * d.cin;
    if (kx) run_chosen(e, kx, qx, tag, flops, bytes + 0.5 * B * (double)r * r * d.cin);
    else run_conv(e, p, tag, flops, bytes);
    return (bool)kx;
}

// Second half of a block: out = (lrelu(conv1 stride 2 (blur(h)) + b1) * sqrt2 + skip(XS)) / sqrt2 in O, from h in Hb and (have_xs) XS
static void run_d_conv1(glass_engine* e, int B, const DBlock& d, const half_t* X, bool have_xs, half_t* Hb, half_t* HB, half_t* XS, half_t* S,
                        half_t* O) {
    char tag[64];
    const int r = d.res, r2 = r / 2;
    if (!have_xs) {
        snprintf(tag, sizeof tag, "D.blurdown.r%d", r);
        Prof pr(e, tag, 2.0 * B * (double)r2 * r2 * d.cin * 16, 2.5 * B * (double)r * r * d.cin);
        launch_blur_down(X, B, r, r, d.cin, XS, e->cur);
    }
    if (conv_down_supported(r, d.cin, d.cout)) {   // blur + skip + stride-2 conv + merge as one kernel
        snprintf(tag, sizeof tag, "D.down.r%d.%dx%d", r2, d.cin, d.cout);
        const double px2 = (double)B * r2 * r2;
        Prof pr(e, tag, 2.0 * px2 * (9.0 + 1.0) * d.cin * d.cout, 2.0 * (B * (double)r * r * d.cin + px2 * (d.cin + d.cout)));
        if (const char* k = launch_conv_down(Hb, XS, d.w1, d.wskip, d.b1, O, B, r, d.cin, d.cout, e->cur)) {
            pr.ran(tag, k);
            return;
        }
        pr.drop();
    }
    ConvParams q = conv_defaults();
    q.x = HB; q.x_bstride = (long long)(r + 1) * (r + 1) * d.cin; q.B = B; q.H = q.W = r + 1; q.Cin = d.cin;
    q.Hc = q.Wc = r2; q.KS = 3; q.stride = 2; q.pad = 0; q.w = d.w1; q.Cout = q.Neff = d.cout; q.Ho = q.Wo = r2;
    q.bias = d.b1; q.act = 1; q.out_scale = 0.70710678118654752440f; q.y = O;
    // skip branch as extra K stages of the stride-2 conv (conv_s2, or conv_tiled<3,2,4,N,skip>) where that kernel applies
    ConvParams qs = q;
    qs.skip_x = XS; qs.skip_w = d.wskip; qs.x_planar32 = 1;
    // blur -> conv_s2 link: that kernel stages its input one 32-channel chunk per K step, so (where it runs) the blur writes 32-channel planes
    const bool hb_planar = blur_pad2_planar32_ok(d.cin) && choose_conv_s2(qs);
    qs.x_planar32 = hb_planar;
    const ConvKernel fused = choose_conv(qs);
    {
        snprintf(tag, sizeof tag, "D.blur.r%d", r);
        Prof pr(e, tag, 2.0 * B * (double)(r + 1) * (r + 1) * d.cin * 16, 4.0 * B * (double)r * r * d.cin);
        launch_blur_pad2(Hb, B, r, r, d.cin, HB, e->cur, hb_planar);
    }
    snprintf(tag, sizeof tag, "D.conv1.r%d.%dx%d", r2, d.cin, d.cout);
    const double f1 = 2.0 * B * (double)r2 * r2 * 9 * d.cin * d.cout, fs = 2.0 * B * (double)r2 * r2 * d.cin * d.cout;
    if (fused) {
        run_chosen(e, fused, qs, tag, f1 + fs, 2.0 * B * ((double)(r + 1) * (r + 1) * d.cin + (double)r2 * r2 * (d.cin + d.cout)));
        return;
    }
    ConvParams s = conv_defaults();
    s.x = XS; s.x_bstride = (long long)r2 * r2 * d.cin; s.B = B; s.H = s.W = r2; s.Cin = d.cin;
    s.Hc = s.Wc = r2; s.KS = 1; s.pad = 0; s.w = d.wskip; s.Cout = s.Neff = d.cout; s.Ho = s.Wo = r2; s.y = S;
    char stag[64];
    snprintf(stag, sizeof stag, "D.skip.r%d.%dx%d", r2, d.cin, d.cout);
    run_conv(e, s, stag, fs, 2.0 * B * (double)r2 * r2 * (d.cin + d.cout));
    q.res = S;
    run_conv(e, q, tag, f1, 2.0 * B * ((double)(r + 1) * (r + 1) * d.cin + 2.0 * r2 * r2 * d.cout));
}

// Discriminator conv blocks [i_lo, i_hi) (D order: block i works at resolution R >> i).
// bufs: five scratch feature maps; X enters in `X`; the result pointer is returned.
// rgb_y != nullptr (only with i_lo == 0): X has NOT been produced yet — the first block starts from the skip image.
half_t* run_d_blocks(glass_engine* e, int B, int i_lo, int i_hi, half_t* X, half_t* const bufs[5], const float* rgb_y) {
    half_t *Hb = bufs[0], *HB = bufs[1], *XS = bufs[2], *S = bufs[3], *O = bufs[4];
    bool x_planar = false;       // X is chunk-planar (common.h x_planar8): written so by the fused first block for conv_wreg
    for (int i = i_lo; i < i_hi; ++i) {
        const DBlock& d = e->dblk[i];
        const float* y = i == 0 ? rgb_y : nullptr;
        // the next block's first conv on conv_wreg (with the blur-down by-product: nothing else reads this map): chunk-planar output
        const bool planar = y && i + 1 < i_hi && e->dblk[i + 1].cin == d.cout && choose_conv_wreg(d_conv0_params(B, e->dblk[i + 1], O, true, Hb, XS));
        const bool whole = y && run_d_block0(e, B, d, y, O, planar);
        if (!whole) {
            const bool have_xs = run_d_conv0(e, B, d, X, x_planar, y, Hb, XS);
            run_d_conv1(e, B, d, X, have_xs, Hb, HB, XS, S, O);
        }
        x_planar = whole && planar;
        std::swap(X, O);
    }
    return X;
}

// D's dense head (stylegan2/models.py:1339-1350) on dfin [P][16 CL]: the launches run_d_head and the diagnostic op share.
GemmParams d_head_dense0(const DHead& h) {
    return gemm_params(h.dfin, h.w0, h.P, h.CL, 16 * h.CL, h.b0, 4, nullptr, h.dh, 1);
}
// M = P rows, K = 16 CL = 8192: the 128 x 64 tiles are 8 workgroups walking 128 K steps each (97 us for 0.5 GFLOP).  Split K into 16
// slices (blockIdx.z) with raw partial sums, finished in a fixed order with bias + activation: 128+ workgroups, 8 steps each; the finish
// and the second dense layer (CL -> 1) are one launch.  nullptr: the shape has no split form (16 CL % 1024, or gemm_tiled refuses it) and
// nothing was launched — d_head_dense0 through gemm_tiled / gemm_direct, then launch_d_head_dense1.
const char* launch_d_head_split(const DHead& h, hipStream_t st) {
    const int S0 = 16;
    const GemmParams g = d_head_dense0(h);
    if (!h.part || g.K % (S0 * 64) != 0) return nullptr;
    GemmParams q = g;
    q.ld = g.K; q.K = g.K / S0; q.batch = S0; q.a_bs = q.K; q.w_bs = q.K; q.o_bs = (long long)h.P * h.CL;
    q.bias = nullptr; q.mode = 3; q.out32 = h.part;
    const char* k = launch_gemm_tiled(q, st);
    if (k) launch_dense01_finish(h.part, S0, q.o_bs, g.bias, h.w1t, h.b1, h.dis, h.P, h.CL, st);
    return k;
}
void launch_d_head_dense1(const DHead& h, hipStream_t st) {
    launch_dense(h.dh, h.CL, h.P, h.CL, h.w1t, 1, h.b1, h.dis, 1, 0, 0, nullptr, 0, st);
}

// mbstd + final conv + dense head for the whole population: X is [P][4][4][C0]
void run_d_head(glass_engine* e, int P, const half_t* X, half_t* scratch) {
    const glass_config& c = e->cfg;
    const int CL = c.channels[0];
    {
        Prof pr(e, "D.mbstd", 0, 4.0 * P * 16 * CL);
        launch_mbstd(X, P, 16, CL, e->d_final_cpad, c.batch_size, c.mbstd_group, 1e-8f, scratch, e->cur);
    }
    ConvParams p = conv_defaults();
    p.x = scratch; p.x_bstride = 16LL * e->d_final_cpad; p.B = P; p.H = p.W = 4; p.Cin = e->d_final_cpad; p.Hc = p.Wc = 4;
    p.KS = 3; p.pad = 1; p.w = e->d_final_w; p.Cout = p.Neff = CL; p.Ho = p.Wo = 4; p.bias = e->d_final_b; p.act = 1;
    p.y = e->d_dfin;
    run_conv(e, p, "D.final_conv", 2.0 * P * 16 * 9.0 * (CL + 1) * CL, 2.0 * 9 * CL * (CL + 1));
    const DHead h = {e->d_dfin, e->d_dense0_w, e->d_dense0_b, e->d_dense1_wt, e->d_dense1_b, e->d_dh_part, e->d_dh, e->d_dis, P, CL};
    if (e->d_dh_part && P <= e->cfg.max_pop) {
        Prof pr(e, "D.dense0", 2.0 * P * 16.0 * CL * CL, 2.0 * 16.0 * CL * CL);
        const char* k = launch_d_head_split(h, e->cur);
        if (k) {
            if (pr.on) pr.pe.name = std::string("D.dense0+1@") + k + "+dense01_finish";
            return;
        }
        pr.drop();
    }
    const GemmParams g = d_head_dense0(h);
    run_gemm(e, g, "D.dense0");
    {
        Prof pr(e, "D.dense1", 2.0 * P * CL, 0);
        launch_d_head_dense1(h, e->cur);
    }
}
