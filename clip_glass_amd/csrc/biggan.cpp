// biggan.cpp — BigGAN-deep generator behind the same engine / C ABI (config C3: DeepMindBigGAN256/512,
// reference call sites models.py:64-86, latent.py:4-24, config.py:31-74).
//
// The network itself lives in pytorch-pretrained-biggan==0.1.1 (absent from /root/reference): the layer
// algebra here follows that package's published BigGAN-deep generator under its state-dict keys
// ("biggan." + key), restated in oracle/biggan_ref.py.  MI355X formulation:
//   * spectral norm folded at load:  W <- weight_orig / (u . W_mat v)       (inference uses the stored u, v)
//   * every BigGANBatchNorm folded to one per-(candidate, channel) affine  y = x*A + S, the tables for ALL
//     56 norms of the network produced by ONE dense launch (cond[P,256] x [256, 2*Ctot]) + one table kernel;
//     the conv biases feeding a norm are folded into its shift
//   * bn1..bn3 + ReLU ride in the epilogue of the conv that produces their input (scale, shift, relu); bn0 + ReLU
//     (and the final bn) ride in the STAGING of the conv that consumes them (relu(x*A + S) on in-bounds pixels);
//     nearest x2 is an addressing mode of conv1's input and of the skip read; the channel-drop skip is a strided
//     residual read in conv3's epilogue -> a GenBlock is exactly 4 MFMA conv launches, nothing else
//   * self-attention = one 1x1 conv for theta|phi|g, a split/max-pool kernel, two batched MFMA GEMMs
//     around an fp32 row softmax, and the output 1x1 conv with gamma folded in and the residual fused
//   * activations NHWC fp16 (fp32 accumulate), images leave as planar fp32 like the StyleGAN2 path.
#include <math.h>
#include <string.h>

#include "engine.h"
#include "kernels.h"

namespace {

// weight_orig / sigma as a flat float vector [rows][cols]
int sn_fold(glass_engine* e, const std::string& prefix, int rows, size_t cols, std::vector<float>& out) {
    const HostTensor* w = find(e, prefix + ".weight_orig");
    const HostTensor* u = find(e, prefix + ".weight_u");
    const HostTensor* v = find(e, prefix + ".weight_v");
    if (!w) {   // already-normalised weight
        const HostTensor* w2 = find(e, prefix + ".weight");
        REQUIRE(w2 != nullptr, GLASS_ERR_STATE, "missing tensor: " + prefix + ".weight_orig");
        REQUIRE(numel(w2) == (size_t)rows * cols, GLASS_ERR_ARG, "bad shape: " + prefix + ".weight");
        out = w2->data;
        return GLASS_OK;
    }
    REQUIRE(u && v, GLASS_ERR_STATE, "missing tensor: " + prefix + ".weight_u / weight_v");
    REQUIRE(numel(w) == (size_t)rows * cols && numel(u) == (size_t)rows && numel(v) == cols, GLASS_ERR_ARG,
            "bad shape: " + prefix + " (spectral-norm weight / u / v)");
    double sigma = 0.0;
    for (int i = 0; i < rows; ++i) {
        double acc = 0.0;
        const float* wr = w->data.data() + (size_t)i * cols;
        for (size_t j = 0; j < cols; ++j) acc += (double)wr[j] * v->data[j];
        sigma += acc * u->data[i];
    }
    REQUIRE(sigma != 0.0, GLASS_ERR_ARG, "zero spectral norm: " + prefix);
    out.resize((size_t)rows * cols);
    const float inv = (float)(1.0 / sigma);
    for (size_t i = 0; i < out.size(); ++i) out[i] = w->data[i] * inv;
    return GLASS_OK;
}

// conv weight [cout][cin][ks][ks] -> [ks*ks][cout_pad][cin] fp16 (rows >= cout are zero)
std::vector<_Float16> pack(const std::vector<float>& W, int cout, int cin, int ks, int cout_pad, float scale = 1.f) {
    std::vector<_Float16> out((size_t)ks * ks * cout_pad * cin, (_Float16)0.f);
    for (int o = 0; o < cout; ++o)
        for (int i = 0; i < cin; ++i)
            for (int t = 0; t < ks * ks; ++t)
                out[((size_t)t * cout_pad + o) * cin + i] = (_Float16)(W[((size_t)o * cin + i) * ks * ks + t] * scale);
    return out;
}

// BigGANBatchNorm: statistics row for this truncation (blend as the package does)
int stat_row(glass_engine* e, const std::string& name, int n_stats, int C, double truncation, std::vector<float>& out) {
    GET(t, name);
    REQUIRE(numel(t) == (size_t)n_stats * C, GLASS_ERR_ARG, "bad shape: " + name);
    const double step = 1.0 / (n_stats - 1);
    double ip = 0.0;
    const double coef = modf(truncation / step, &ip);
    const int start = (int)ip;
    REQUIRE(start >= 0 && start < n_stats && (coef == 0.0 || start + 1 < n_stats), GLASS_ERR_ARG,
            "truncation outside the stored batch-norm statistics");
    out.resize(C);
    for (int c = 0; c < C; ++c) {
        const float a = t->data[(size_t)start * C + c];
        out[c] = coef != 0.0 ? (float)(a * coef + t->data[(size_t)(start + 1) * C + c] * (1 - coef)) : a;
    }
    return GLASS_OK;
}

}  // namespace

int glass_biggan_finalize(glass_engine* e) {
    const glass_config& c = e->cfg;
    BgState& g = e->bg;
    const int ch = c.bg_ch, zd = c.bg_z_dim, nc = c.bg_num_classes, cd = 2 * zd, ns = c.bg_n_stats;
    const std::string G = "biggan.generator.";
    int rc;
    g.zd = zd;
    g.nc = nc;
    g.c0 = 16 * ch;
    {
        GET(E, "biggan.embeddings.weight");
        REQUIRE(numel(E) == (size_t)zd * nc, GLASS_ERR_ARG, "bad shape: biggan.embeddings.weight");
        if ((rc = upload(e, &g.et, transposed(E->data.data(), zd, nc, 1.f)))) return rc;
        std::vector<float> W;
        if ((rc = sn_fold(e, G + "gen_z", 16 * g.c0, cd, W))) return rc;
        if ((rc = upload(e, &g.genz_wt, transposed(W.data(), 16 * g.c0, cd, 1.f)))) return rc;
        GET(b, G + "gen_z.bias");
        REQUIRE(numel(b) == (size_t)16 * g.c0, GLASS_ERR_ARG, "bad shape: gen_z.bias");
        if ((rc = upload(e, &g.genz_b, b->data))) return rc;
    }
    // ---- walk the layer list: block geometry + batch-norm column offsets -----------------------------
    struct BnRef { std::string prefix; int C, off; bool conditional; std::string prebias; };
    std::vector<BnRef> bns;
    int res = 4, m = 0, off = 0;
    g.blocks.clear();
    std::vector<std::string> block_prefix;
    for (int i = 0; i < c.bg_n_layers; ++i) {
        if (i == c.bg_attention_pos) {
            g.attn_before = i;
            g.attn_C = ch * c.bg_layers[i][1];
            g.attn_res = res;
            const std::string p = G + "layers." + std::to_string(m);
            const int C = g.attn_C, c8 = C / 8, c2 = C / 2;
            REQUIRE(C % 64 == 0 && res % 2 == 0, GLASS_ERR_ARG, "unsupported self-attention geometry");
            std::vector<float> Wt, Wp, Wg, Wo;
            if ((rc = sn_fold(e, p + ".snconv1x1_theta", c8, C, Wt))) return rc;
            if ((rc = sn_fold(e, p + ".snconv1x1_phi", c8, C, Wp))) return rc;
            if ((rc = sn_fold(e, p + ".snconv1x1_g", c2, C, Wg))) return rc;
            if ((rc = sn_fold(e, p + ".snconv1x1_o_conv", C, c2, Wo))) return rc;
            std::vector<float> cat;
            cat.insert(cat.end(), Wt.begin(), Wt.end());
            cat.insert(cat.end(), Wp.begin(), Wp.end());
            cat.insert(cat.end(), Wg.begin(), Wg.end());
            if ((rc = upload(e, &g.attn_w_tpg, pack(cat, 2 * c8 + c2, C, 1, 2 * c8 + c2)))) return rc;
            GET(gm, p + ".gamma");
            if ((rc = upload(e, &g.attn_w_o, pack(Wo, C, c2, 1, C, gm->data[0])))) return rc;
            ++m;
        }
        BgBlock b;
        b.up = c.bg_layers[i][0];
        b.cin = ch * c.bg_layers[i][1];
        b.cout = ch * c.bg_layers[i][2];
        b.mid = b.cin / 4;
        b.res_in = res;
        REQUIRE(b.cin % 128 == 0 && b.mid % 32 == 0 && b.cout % 32 == 0, GLASS_ERR_ARG,
                "BigGAN channel widths must keep in/4 and out multiples of 32");
        REQUIRE(b.cin == b.cout || b.cin == 2 * b.cout, GLASS_ERR_ARG,
                "GenBlock: out channels must equal in or in/2 (channel-drop skip)");
        const std::string p = G + "layers." + std::to_string(m);
        const int cins[4] = {b.cin, b.mid, b.mid, b.mid}, couts[4] = {b.mid, b.mid, b.mid, b.cout}, kss[4] = {1, 3, 3, 1};
        for (int k = 0; k < 4; ++k) {
            b.bn_off[k] = off;
            bns.push_back({p + ".bn_" + std::to_string(k), cins[k], off, true,
                           k > 0 ? p + ".conv_" + std::to_string(k - 1) + ".bias" : std::string()});
            off += cins[k];
            std::vector<float> W;
            if ((rc = sn_fold(e, p + ".conv_" + std::to_string(k), couts[k], (size_t)cins[k] * kss[k] * kss[k], W))) return rc;
            if ((rc = upload(e, &b.w[k], pack(W, couts[k], cins[k], kss[k], couts[k])))) return rc;
        }
        GET(b3, p + ".conv_3.bias");
        REQUIRE(numel(b3) == (size_t)b.cout, GLASS_ERR_ARG, "bad shape: conv_3.bias");
        if ((rc = upload(e, &b.b3, b3->data))) return rc;
        g.blocks.push_back(b);
        if (b.up) res *= 2;
        ++m;
    }
    REQUIRE(!g.blocks.empty() && g.blocks[0].cin == g.c0, GLASS_ERR_ARG, "first GenBlock must take 16*ch channels");
    REQUIRE(g.blocks.back().cout == ch, GLASS_ERR_ARG, "last GenBlock must produce `ch` channels");
    g.R = res;
    g.final_bn_off = off;
    bns.push_back({G + "bn", ch, off, false, std::string()});
    off += ch;
    g.Ctot = off;
    // ---- batch-norm tables: dense weights [cd][2*Ctot] ( gain columns | offset columns ) ---------------
    {
        const size_t CT = (size_t)g.Ctot;
        std::vector<float> wt((size_t)cd * 2 * CT, 0.f), bias(2 * CT, 0.f), inv_std(CT), mean(CT), prebias(CT, 0.f);
        for (auto& r : bns) {
            std::vector<float> mu, var;
            if ((rc = stat_row(e, r.prefix + ".running_means", ns, r.C, c.bg_truncation, mu))) return rc;
            if ((rc = stat_row(e, r.prefix + ".running_vars", ns, r.C, c.bg_truncation, var))) return rc;
            for (int k = 0; k < r.C; ++k) {
                mean[r.off + k] = mu[k];
                inv_std[r.off + k] = 1.f / sqrtf(var[k] + c.bg_eps);
            }
            if (r.conditional) {
                std::vector<float> Ws, Wo;
                if ((rc = sn_fold(e, r.prefix + ".scale", r.C, cd, Ws))) return rc;
                if ((rc = sn_fold(e, r.prefix + ".offset", r.C, cd, Wo))) return rc;
                for (int k = 0; k < r.C; ++k) {
                    bias[r.off + k] = 1.f;   // weight = 1 + scale(cond)
                    for (int j = 0; j < cd; ++j) {
                        wt[(size_t)j * 2 * CT + r.off + k] = Ws[(size_t)k * cd + j];
                        wt[(size_t)j * 2 * CT + CT + r.off + k] = Wo[(size_t)k * cd + j];
                    }
                }
            } else {
                GET(w, r.prefix + ".weight");
                GET(b, r.prefix + ".bias");
                REQUIRE(numel(w) == (size_t)r.C && numel(b) == (size_t)r.C, GLASS_ERR_ARG, "bad shape: " + r.prefix);
                for (int k = 0; k < r.C; ++k) {
                    bias[r.off + k] = w->data[k];
                    bias[CT + r.off + k] = b->data[k];
                }
            }
            if (!r.prebias.empty()) {
                GET(pb, r.prebias);
                REQUIRE(numel(pb) == (size_t)r.C, GLASS_ERR_ARG, "bad shape: " + r.prebias);
                for (int k = 0; k < r.C; ++k) prebias[r.off + k] = pb->data[k];
            }
        }
        if ((rc = upload(e, &g.bn_wt, wt))) return rc;
        if ((rc = upload(e, &g.bn_bias, bias))) return rc;
        if ((rc = upload(e, &g.bn_inv_std, inv_std))) return rc;
        if ((rc = upload(e, &g.bn_mean, mean))) return rc;
        if ((rc = upload(e, &g.bn_prebias, prebias))) return rc;
    }
    {   // conv_to_rgb: only the first 3 of `ch` output channels are used (z[:, :3]); padded to rgb_cpad MFMA columns
        std::vector<float> W;
        if ((rc = sn_fold(e, G + "conv_to_rgb", ch, (size_t)ch * 9, W))) return rc;
        W.resize((size_t)3 * ch * 9);
        if ((rc = upload(e, &g.rgb_w, pack(W, 3, ch, 3, g.rgb_cpad)))) return rc;
        GET(b, G + "conv_to_rgb.bias");
        std::vector<float> bb(g.rgb_cpad, 0.f);
        for (int k = 0; k < 3; ++k) bb[k] = b->data[k];
        if ((rc = upload(e, &g.rgb_b, bb))) return rc;
    }
    // ---- activation buffers (per chunk of candidates) ---------------------------------------------------
    const size_t P = c.max_pop, CH = e->chunk;
    size_t mx = 0, mt1 = 0, mtu = 0;
    for (auto& b : g.blocks) {
        const size_t hi = (size_t)b.res_in * b.res_in, ro = (size_t)(b.res_in << b.up), ho = ro * ro;
        mx = std::max(mx, std::max(hi * b.cin, ho * b.cout));
        mt1 = std::max(mt1, hi * b.mid);
        mtu = std::max(mtu, ho * b.mid);
    }
    const size_t RR = (size_t)g.R * g.R;
    mtu = std::max(mtu, RR * g.rgb_cpad);
    if ((rc = dev_alloc(e, &g.cond, P * cd))) return rc;
    if ((rc = dev_alloc(e, &g.tab, P * 2 * g.Ctot))) return rc;
    if ((rc = dev_alloc(e, &g.tab16, P * 2 * g.Ctot))) return rc;
    if ((rc = dev_alloc(e, &g.h32, CH * 16 * g.c0))) return rc;
    for (int i = 0; i < 2; ++i)
        if ((rc = dev_alloc(e, &g.x[i], CH * mx))) return rc;
    if ((rc = dev_alloc(e, &g.t1, CH * mt1))) return rc;
    if ((rc = dev_alloc(e, &g.t2, CH * mtu))) return rc;
    if ((rc = dev_alloc(e, &g.t3, CH * mtu))) return rc;
    if (g.attn_before >= 0) {
        const size_t hw = (size_t)g.attn_res * g.attn_res, hq = hw / 4, C = g.attn_C, c8 = C / 8, c2 = C / 2;
        if ((rc = dev_alloc(e, &g.a_T, CH * hw * (2 * c8 + c2)))) return rc;
        if ((rc = dev_alloc(e, &g.a_theta, CH * hw * c8))) return rc;
        if ((rc = dev_alloc(e, &g.a_phi, CH * hq * c8))) return rc;
        if ((rc = dev_alloc(e, &g.a_gT, CH * c2 * hq))) return rc;
        if ((rc = dev_alloc(e, &g.a_S, CH * hw * hq))) return rc;
        if ((rc = dev_alloc(e, &g.a_P, CH * hw * hq))) return rc;
        if ((rc = dev_alloc(e, &g.a_O, CH * hw * c2))) return rc;
    }
    return GLASS_OK;
}

int glass_biggan_prepare(glass_engine* e, int P) {
    BgState& g = e->bg;
    const int cd = 2 * g.zd;
    {
        Prof pr(e, "bg.cond", 2.0 * P * g.nc * g.zd, 4.0 * ((double)P * e->cfg.latent_size + (double)g.nc * g.zd));
        launch_bg_cond(e->d_z, P, e->cfg.latent_size, g.zd, g.nc, g.et, g.cond, e->cur);
    }
    {
        Prof pr(e, "bg.bn_tables", 2.0 * P * cd * 2.0 * g.Ctot, 4.0 * ((double)cd * 2 * g.Ctot + 2.0 * P * 2 * g.Ctot));
        launch_dense(g.cond, cd, P, cd, g.bn_wt, 2 * g.Ctot, g.bn_bias, g.tab, 2 * g.Ctot, 0, 0, nullptr, 0, e->cur);
        launch_bg_bn_tables(g.tab, P, g.Ctot, g.bn_inv_std, g.bn_mean, g.bn_prebias, e->cur);
        launch_bg_to_half(g.tab, g.tab16, (long long)P * 2 * g.Ctot, e->cur);
    }
    return GLASS_OK;
}

namespace {

// one conv of the BigGAN path: x [B][res >> in_up]^2 [cin] -> y [B][res][res][cout]
//   pre_bn >= 0: batch norm + ReLU of the INPUT applied while staging (x <- relu(x*A + S), padding stays zero)
//   in_up      : the input is read through a nearest x2 upsample
//   bn_off >= 0: batch norm + ReLU of the OUTPUT fused in the epilogue (the next conv's input norm)
//   resid      : residual [B][res >> res_up]^2 [res_cs] (first cout channels), nearest x2 when res_up
struct BgConv {
    int res, cin, cout, ks;
    const half_t* w;
    const half_t* x;
    half_t* y;
    int pre_bn = -1, in_up = 0, bn_off = -1;
    const float* bias = nullptr;
    const half_t* resid = nullptr;
    int res_cs = 0, res_up = 0;
    float* rgb_tanh = nullptr;      // planar tanh(channels 0..2) instead of y (ConvParams::rgb_tanh_out)
};
ConvParams bg_conv_params(glass_engine* e, int c0, int B, const BgConv& q) {
    BgState& g = e->bg;
    ConvParams p = conv_defaults();
    const int rin = q.res >> q.in_up;
    p.x = q.x;
    p.x_bstride = (long long)rin * rin * q.cin;
    p.B = B; p.H = q.res; p.W = q.res; p.Cin = q.cin;
    p.Hc = q.res; p.Wc = q.res; p.Ho = q.res; p.Wo = q.res;
    p.KS = q.ks; p.stride = 1; p.pad = q.ks / 2;
    p.in_up = q.in_up;
    p.w = q.w;
    p.Neff = q.cout; p.Cout = q.cout;
    const float* tab = g.tab + (size_t)c0 * 2 * g.Ctot;
    if (q.pre_bn >= 0) {
        p.sn = tab + q.pre_bn;
        p.pre_shift = tab + g.Ctot + q.pre_bn;
        p.sn16 = g.tab16 + (size_t)c0 * 2 * g.Ctot + q.pre_bn;
        p.pre_shift16 = p.sn16 + g.Ctot;
        p.sn_stride = 2 * g.Ctot;
    }
    if (q.bn_off >= 0) {
        p.dscale = tab + q.bn_off;
        p.shift = tab + g.Ctot + q.bn_off;
        p.ds_stride = 2 * g.Ctot;
        p.act = 2;
    }
    p.bias = q.bias;
    p.res = q.resid;
    p.res_cs = q.res_cs;
    p.res_up = q.res_up;
    p.y = q.y;
    p.rgb_tanh_out = q.rgb_tanh;
    return p;
}
// chosen: the kernel the caller already asked a chooser for (empty: run_conv's order)
void bg_conv(glass_engine* e, const char* tag, int c0, int B, const BgConv& q, const ConvKernel& chosen = ConvKernel()) {
    const int rin = q.res >> q.in_up;
    const double M = (double)B * q.res * q.res, Min = (double)B * rin * rin;
    const double rbytes = q.resid ? M * q.cout / (q.res_up ? 4 : 1) : 0.0;
    const double flops = 2.0 * M * q.cout * q.cin * q.ks * q.ks;
    const double bytes = 2.0 * (Min * q.cin + (q.rgb_tanh ? M * 6.0 : M * q.cout) + rbytes + (double)q.cout * q.cin * q.ks * q.ks);
    const ConvParams p = bg_conv_params(e, c0, B, q);
    if (chosen) run_chosen(e, chosen, p, tag, flops, bytes);
    else run_conv(e, p, tag, flops, bytes);
}

void bg_attention(glass_engine* e, int B, const half_t* x, half_t* y) {
    BgState& g = e->bg;
    const int res = g.attn_res, C = g.attn_C, c8 = C / 8, c2 = C / 2, CT = 2 * c8 + c2;
    const int hw = res * res, hq = hw / 4;
    {
        BgConv q{res, C, CT, 1, g.attn_w_tpg, x, g.a_T};
        bg_conv(e, "bg.attn.theta_phi_g", 0, B, q);
    }
    {
        Prof pr(e, "bg.attn.split_pool", 0, 2.0 * B * ((double)hw * CT + (double)hw * c8 + (double)hq * (c8 + c2)));
        launch_bg_attn_split(g.a_T, B, res, res, c8, c2, g.a_theta, g.a_phi, g.a_gT, e->cur);
    }
    GemmParams q = gemm_params(g.a_theta, g.a_phi, hw, hq, c8, nullptr, 3, nullptr, g.a_S, 0);   // logits = theta . phi^T  (fp32 out)
    q.cand_batch = 1;
    q.batch = B; q.a_bs = (long long)hw * c8; q.w_bs = (long long)hq * c8; q.o_bs = (long long)hw * hq;
    {
        Prof pr(e, "bg.attn.logits", 2.0 * B * hw * (double)hq * c8, B * (2.0 * hw * c8 + 2.0 * hq * c8 + 4.0 * hw * hq));
        const char* k = launch_gemm_tiled(q, e->cur);
        if (!k) k = launch_gemm_direct(q, e->cur);
        if (pr.on) pr.pe.name = std::string("bg.attn.logits@") + k;
    }
    {
        Prof pr(e, "bg.attn.softmax", 0, 6.0 * B * hw * (double)hq);
        launch_bg_softmax(g.a_S, (long long)B * hw, hq, g.a_P, e->cur);
    }
    q = gemm_params(g.a_P, g.a_gT, hw, c2, hq, nullptr, 0, g.a_O, nullptr, 0);   // attn_g = P . g^T
    q.cand_batch = 1;
    q.batch = B; q.a_bs = (long long)hw * hq; q.w_bs = (long long)c2 * hq; q.o_bs = (long long)hw * c2;
    {
        Prof pr(e, "bg.attn.values", 2.0 * B * hw * (double)hq * c2, B * (2.0 * hw * hq + 2.0 * hq * c2 + 2.0 * hw * c2));
        const char* k = launch_gemm_tiled(q, e->cur);
        if (!k) k = launch_gemm_direct(q, e->cur);
        if (pr.on) pr.pe.name = std::string("bg.attn.values@") + k;
    }
    // out = x + gamma * o_conv(attn_g): gamma folded into the weights, x as the fused residual
    BgConv oc{res, c2, C, 1, g.attn_w_o, g.a_O, y};
    oc.resid = x;
    bg_conv(e, "bg.attn.o_conv", 0, B, oc);
}

}  // namespace

static int bg_take_tap(glass_engine* e, const half_t* x, int B, int res, int C) {
    std::vector<_Float16> h((size_t)B * res * res * C);
    GLASS_HIP(hipStreamSynchronize(e->cur));
    GLASS_HIP(hipMemcpy(h.data(), x, h.size() * sizeof(_Float16), hipMemcpyDeviceToHost));
    e->bg_tap_data.resize(h.size());
    for (size_t i = 0; i < h.size(); ++i) e->bg_tap_data[i] = (float)h[i];
    e->bg_tap_dims[0] = B; e->bg_tap_dims[1] = res; e->bg_tap_dims[2] = res; e->bg_tap_dims[3] = C;
    e->bg_tap = -2;   // one-shot, as include/glass.h documents ("the next pass"): later passes run without the sync + copy
    return GLASS_OK;
}

int glass_biggan_chunk(glass_engine* e, int c0, int B, float* y) {
    BgState& g = e->bg;
    const int cd = 2 * g.zd;
    {   // gen_z: cond -> [B][4][4][16ch] (the package views the linear output as NHWC before permuting)
        Prof pr(e, "bg.gen_z", 2.0 * B * cd * 16.0 * g.c0, 4.0 * (double)cd * 16 * g.c0);
        launch_dense(g.cond + (size_t)c0 * cd, cd, B, cd, g.genz_wt, 16 * g.c0, g.genz_b, g.h32, 16 * g.c0, 0, 0, nullptr, 0,
                     e->cur);
        launch_bg_to_half(g.h32, g.x[0], (long long)B * 16 * g.c0, e->cur);
    }
    int cur = 0;
    char tag[64];
    for (size_t i = 0; i < g.blocks.size(); ++i) {
        if ((int)i == g.attn_before) {
            bg_attention(e, B, g.x[cur], g.x[cur ^ 1]);
            cur ^= 1;
            if (e->bg_tap == -1 && c0 == 0) {
                int rc = bg_take_tap(e, g.x[cur], B, g.blocks[i].res_in, g.blocks[i].cin);
                if (rc) return rc;
            }
        }
        const BgBlock& b = g.blocks[i];
        const int ri = b.res_in, ro = b.res_in << b.up;
        const half_t* x = g.x[cur];
        {   // bn0 + relu ride in conv0's staging; bn1 + relu in its epilogue
            BgConv q{ri, b.cin, b.mid, 1, b.w[0], x, g.t1};
            q.pre_bn = b.bn_off[0];
            q.bn_off = b.bn_off[1];
            snprintf(tag, sizeof tag, "bg.b%zu.conv0.r%d.%dx%d", i, ri, b.cin, b.mid);
            bg_conv(e, tag, c0, B, q);
        }
        {   // nearest x2 (up blocks) is an addressing mode of conv1's input
            BgConv q{ro, b.mid, b.mid, 3, b.w[1], g.t1, g.t2};
            q.in_up = b.up;
            q.bn_off = b.bn_off[2];
            snprintf(tag, sizeof tag, "bg.b%zu.conv1.r%d.%dx%d", i, ro, b.mid, b.mid);
            bg_conv(e, tag, c0, B, q);
        }
        {
            BgConv q{ro, b.mid, b.mid, 3, b.w[2], g.t2, g.t3};
            q.bn_off = b.bn_off[3];
            snprintf(tag, sizeof tag, "bg.b%zu.conv2.r%d.%dx%d", i, ro, b.mid, b.mid);
            bg_conv(e, tag, c0, B, q);
        }
        // round 4: the LAST block's conv_3 + skip, the final bn - relu, conv_to_rgb[:3] and tanh in one kernel (bg_tail.hip): the
        // 128-channel full-resolution map between them never exists.  Not when that block's output was asked for as a tap; A/B knob
        // GLASS_BG_NO_TAIL.
        if (i + 1 == g.blocks.size() && e->bg_tap != (int)i && ro == g.R &&
            bg_tail_supported(ro, b.mid, b.cout, b.cin, b.up, g.rgb_cpad)) {
            BgTailParams tp;
            tp.h = g.t3; tp.x0 = x; tp.w3 = b.w[3]; tp.b3 = b.b3;
            tp.tab = g.tab + (size_t)c0 * 2 * g.Ctot; tp.bnf_off = g.final_bn_off; tp.ctot = g.Ctot;
            tp.rgb_w = g.rgb_w; tp.cpad = g.rgb_cpad; tp.rgb_b = g.rgb_b; tp.y = y; tp.B = B; tp.R = ro;
            const double M = (double)B * ro * ro;
            Prof pr(e, "bg.tail.conv3+bn+to_rgb+tanh", 2.0 * M * (32.0 * 128 + 128.0 * 27), M * (2.0 * 32 + 2.0 * 128 / 4 + 12.0));
            launch_bg_tail(tp, e->cur);
            return GLASS_OK;
        }
        {   // skip = x0[:, :cout] (channel drop), nearest x2 when up: read straight from the block input
            BgConv q{ro, b.mid, b.cout, 1, b.w[3], g.t3, g.x[cur ^ 1]};
            q.bias = b.b3;
            q.resid = x;
            q.res_cs = b.cin;
            q.res_up = b.up;
            snprintf(tag, sizeof tag, "bg.b%zu.conv3.r%d.%dx%d", i, ro, b.mid, b.cout);
            bg_conv(e, tag, c0, B, q);
        }
        cur ^= 1;
        if (e->bg_tap == (int)i && c0 == 0) {
            int rc = bg_take_tap(e, g.x[cur], B, ro, b.cout);
            if (rc) return rc;
        }
    }
    {   // bn - relu (staging of the conv) - conv_to_rgb[:3] - tanh
        const int R = g.R, ch = e->cfg.bg_ch;
        BgConv q{R, ch, g.rgb_cpad, 3, g.rgb_w, g.x[cur], g.t2};
        q.pre_bn = g.final_bn_off;
        q.bias = g.rgb_b;
        // round 4: tanh(channels 0..2) straight from the conv's accumulators as planar fp32 — the 32-channel fp16 map (1.07 GB at 512 px,
        // P = 64) and the pass that re-read it are gone.  (Small test geometries the instance does not take keep the two-pass form.)
        BgConv qd = q;
        qd.rgb_tanh = y;
        if (const ConvKernel k = choose_conv(bg_conv_params(e, c0, B, qd))) {
            bg_conv(e, "bg.final.conv_to_rgb+tanh", c0, B, qd, k);
        } else {
            bg_conv(e, "bg.final.conv_to_rgb", c0, B, q);
            Prof pr(e, "bg.final.tanh", 0, B * (double)R * R * (2.0 * g.rgb_cpad + 12.0));
            launch_bg_rgb_tanh(g.t2, B, (long long)R * R, g.rgb_cpad, y, e->cur);
        }
    }
    return GLASS_OK;
}
