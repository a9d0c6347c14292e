// clip.cpp — CLIP behind the engine: the image tower of the fitness pass, the text tower (glass_engine_encode_text) and the image
// preprocessing in front of the patch embedding.  Both towers are the same transformer blocks (run_blocks) over different buffers.
#include <math.h>
#include <string.h>

#include "engine.h"

// The one rule for the CLIP image tower's geometry (host only: no device is touched).  Every kernel of the tower is written in
// terms of the token count, the width and the patch size; what is fixed is the head dimension (the attention kernels are built for
// 64) and the GEMMs' 64-wide N tiles.  The patch-embedding GEMM's K = 3 patch^2 is padded to the K step by the engine.
extern "C" int glass_clip_geometry_supported(int32_t width, int32_t layers, int32_t heads, int32_t patch, int32_t res, int32_t embed) {
    char msg[256];
#define GEOM_REQ(cond, ...)                       \
    if (!(cond)) {                                \
        snprintf(msg, sizeof msg, __VA_ARGS__);   \
        glass_set_error(msg);                     \
        return GLASS_ERR_ARG;                     \
    }
    GEOM_REQ(width > 0 && layers > 0 && heads > 0 && patch > 0 && res > 0 && embed > 0,
             "unsupported CLIP geometry: width, layers, heads, patch, resolution and embed must be positive");
    GEOM_REQ(width % heads == 0 && width / heads == 64,
             "unsupported CLIP geometry: head dim must be 64 (width %d / heads %d)", width, heads);
    GEOM_REQ(res % patch == 0, "unsupported CLIP geometry: resolution %d is not a multiple of patch %d", res, patch);
    GEOM_REQ(patch <= 64 && res / patch <= 63,
             "unsupported CLIP geometry: patch %d / grid %d out of range (patch <= 64, at most 63 x 63 patches)", patch, res / patch);
    GEOM_REQ(layers <= 64 && width <= 4096 && embed <= 4096, "unsupported CLIP geometry: layers %d / width %d / embed %d out of range",
             layers, width, embed);
#undef GEOM_REQ
    return GLASS_OK;
}
// The one rule for a ModifiedResNet image tower (host only).  Every GEMM of the tower has K and N in {w, 2w, ... 32w} (w / 2 only in the stem's
// own kernels), so a stem width that is a multiple of 64 makes all of them multiples of gemm_tiled's 64-wide tiles and K steps, and the
// attention pool (32 w channels, w / 2 heads) has head dimension 64.
extern "C" int glass_clip_resnet_supported(const int32_t layers[4], int32_t width, int32_t res, int32_t embed) {
    char msg[256];
#define GEOM_REQ(cond, ...)                       \
    if (!(cond)) {                                \
        snprintf(msg, sizeof msg, __VA_ARGS__);   \
        glass_set_error(msg);                     \
        return GLASS_ERR_ARG;                     \
    }
    GEOM_REQ(layers != nullptr, "unsupported CLIP ResNet geometry: null layers");
    GEOM_REQ(width > 0 && res > 0 && embed > 0, "unsupported CLIP ResNet geometry: width, resolution and embed must be positive");
    for (int i = 0; i < 4; ++i)
        GEOM_REQ(layers[i] >= 1 && layers[i] <= 64, "unsupported CLIP ResNet geometry: stage %d has %d bottlenecks (1 .. 64)", i + 1, layers[i]);
    GEOM_REQ(width % 64 == 0, "unsupported CLIP ResNet geometry: stem width %d is not a multiple of 64 (RN50x4 / RN50x16, widths 80 / 96, are not "
             "supported: every GEMM K and N must be a multiple of 64 and the attention pool's head dimension 64)", width);
    GEOM_REQ(res % 32 == 0, "unsupported CLIP ResNet geometry: resolution %d is not a multiple of 32 (the tower's total stride)", res);
    GEOM_REQ(width <= 256 && res <= 1024 && embed <= 4096, "unsupported CLIP ResNet geometry: width %d / resolution %d / embed %d out of range "
             "(width <= 256, resolution <= 1024, embed <= 4096)", width, res, embed);
#undef GEOM_REQ
    return GLASS_OK;
}
int clip_patch_k(const glass_config& c) { return (3 * c.clip_patch * c.clip_patch + 63) / 64 * 64; }   // patch rows padded to gemm_tiled's K step

// The one rule for the opt-in CLIP preprocessing (host only).  gen_res: side of the generated image, 0 for an engine without a generator
// (only the ranges of the two fields are checked then).
extern "C" int glass_clip_preprocess_supported(int32_t gen_res, int32_t clip_res, int32_t clip_resize, int32_t clip_normalize) {
    if (clip_resize < 0 || clip_resize > 2) {
        glass_set_error("clip_resize must be 0 (point-sampled bilinear: the reference), 1 (antialiased bilinear) or 2 (antialiased bicubic), got " +
                        std::to_string(clip_resize));
        return GLASS_ERR_ARG;
    }
    if (clip_normalize < 0 || clip_normalize > 1) {
        glass_set_error("clip_normalize must be 0 (none: the reference) or 1 (CLIP mean / std), got " + std::to_string(clip_normalize));
        return GLASS_ERR_ARG;
    }
    if (clip_resize == 0 || gen_res == 0) return GLASS_OK;
    ResizeTaps t;
    std::string why;
    if (!build_resize_taps(gen_res, clip_res, clip_resize, t, why)) {
        glass_set_error(why);
        return GLASS_ERR_ARG;
    }
    return GLASS_OK;
}

// The one rule for crop views (host only), applied by glass_engine_set_clip_views too.  tokens x width: the tower's rows per image and their
// width — a ViT's (res / patch)^2 + 1 tokens of clip_width; for a ResNet tower the (res / 4)^2 positions of layer1 and the stem width, whose
// 4 x width channels make its largest map.  tokens * 4 * width is the largest activation of either tower per image (the MLP's hidden rows).
extern "C" int glass_clip_views_supported(int32_t max_pop, int32_t tokens, int32_t width, int32_t clip_resize, int32_t views, int32_t min_permille) {
    char msg[320];
#define VIEW_REQ(cond, ...)                       \
    if (!(cond)) {                                \
        snprintf(msg, sizeof msg, __VA_ARGS__);   \
        glass_set_error(msg);                     \
        return GLASS_ERR_ARG;                     \
    }
    VIEW_REQ(max_pop > 0 && tokens > 0 && width > 0, "clip views: max_pop, tokens and width must be positive");
    VIEW_REQ(views >= 0 && views <= GLASS_MAX_CLIP_VIEWS, "clip views: views must be in [0, %d] (0: off), got %d", GLASS_MAX_CLIP_VIEWS, views);
    VIEW_REQ(min_permille >= 1 && min_permille <= 1000, "clip views: the smallest crop side must be 1 .. 1000 per mille of the image side, got %d",
             min_permille);
    if (views == 0) return GLASS_OK;
    VIEW_REQ(clip_resize == 0, "clip views need clip_resize 0 (the point-sampled resize), got %d: the antialiased kernels build one tap table per "
             "(image side, CLIP side) at finalize; a table per view is a follow-up", clip_resize);
    const double largest = (double)max_pop * views * tokens * 4.0 * width;      // (in double: the product of five int32 does not fit an int64)
    VIEW_REQ(largest < 2147483648.0, "clip views: max_pop %d x views %d images of %d rows x 4 x width %d are %.3g activation elements, the "
             "tower's kernels index fewer than 2^31: lower max_pop or views", max_pop, views, tokens, width, largest);
#undef VIEW_REQ
    return GLASS_OK;
}

// Philox4x32-10 on the host (common.h philox4x32_10, synth.philox4x32)
static void philox4x32_10_host(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)c[0] * 0xD2511F53ull, p1 = (uint64_t)c[2] * 0xCD9E8D57ull;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
#define CLIP_VIEW_TAG 0x56494557u          // "VIEW", XOR-ed into the key's high word: disjoint from the noise planes' stream and from GPT2_SAMPLE_TAG
// The boxes (x0, y0, s, flip) of a pass: a function of (seed, generation, view) alone — every candidate of a generation is judged through the
// same crops.  View 0 is the whole image; numpy mirror: synth.clip_view_boxes.
extern "C" int glass_host_clip_view_boxes(uint64_t seed, int32_t generation, int32_t views, int32_t gen_res, int32_t min_permille, int32_t flip,
                                          int32_t fixed, int32_t* boxes) {
    REQUIRE(boxes, GLASS_ERR_ARG, "null boxes");
    REQUIRE(views >= 1 && views <= GLASS_MAX_CLIP_VIEWS, GLASS_ERR_ARG, "clip view boxes: views must be in [1, 16]");
    REQUIRE(gen_res >= 2 && gen_res <= 65536, GLASS_ERR_ARG, "clip view boxes: image side out of range");
    REQUIRE(min_permille >= 1 && min_permille <= 1000, GLASS_ERR_ARG, "clip view boxes: min_permille must be in [1, 1000]");
    const uint32_t R = (uint32_t)gen_res;
    const uint32_t smin = std::max<uint32_t>(2u, (uint32_t)(((uint64_t)R * (uint32_t)min_permille + 999) / 1000));
    boxes[0] = 0; boxes[1] = 0; boxes[2] = gen_res; boxes[3] = 0;
    for (int v = 1; v < views; ++v) {
        uint32_t w[4] = {(uint32_t)v, fixed ? 0u : (uint32_t)generation, 0u, 0u};
        philox4x32_10_host(w, (uint32_t)seed, (uint32_t)(seed >> 32) ^ CLIP_VIEW_TAG);
        const uint32_t s = smin + w[0] % (R - smin + 1);
        boxes[4 * v + 0] = (int32_t)(w[1] % (R - s + 1));
        boxes[4 * v + 1] = (int32_t)(w[2] % (R - s + 1));
        boxes[4 * v + 2] = (int32_t)s;
        boxes[4 * v + 3] = flip ? (int32_t)(w[3] & 1u) : 0;
    }
    return GLASS_OK;
}

static int load_clip_blocks(glass_engine* e, const char* prefix, int layers, int W, std::vector<ClipBlock>& out) {
    char nm[256];
    int rc;
    for (int i = 0; i < layers; ++i) {
        snprintf(nm, sizeof nm, "%s%d.", prefix, i);
        const std::string p = nm;
        ClipBlock b;
        GET(l1g, p + "ln_1.weight");
        GET(l1b, p + "ln_1.bias");
        GET(l2g, p + "ln_2.weight");
        GET(l2b, p + "ln_2.bias");
        GET(wq, p + "attn.in_proj_weight");
        GET(bq, p + "attn.in_proj_bias");
        GET(wo, p + "attn.out_proj.weight");
        GET(bo, p + "attn.out_proj.bias");
        GET(wf, p + "mlp.c_fc.weight");
        GET(bf, p + "mlp.c_fc.bias");
        GET(wp, p + "mlp.c_proj.weight");
        GET(bp, p + "mlp.c_proj.bias");
        REQUIRE(numel(wq) == (size_t)3 * W * W && numel(wo) == (size_t)W * W && numel(wf) == (size_t)4 * W * W &&
                    numel(wp) == (size_t)4 * W * W,
                GLASS_ERR_ARG, "bad CLIP block shapes: " + p);
        if ((rc = upload(e, &b.ln1_g, l1g->data))) return rc;
        if ((rc = upload(e, &b.ln1_b, l1b->data))) return rc;
        if ((rc = upload(e, &b.ln2_g, l2g->data))) return rc;
        if ((rc = upload(e, &b.ln2_b, l2b->data))) return rc;
        if ((rc = upload(e, &b.w_qkv, to_half(wq->data.data(), numel(wq))))) return rc;
        if ((rc = upload(e, &b.w_out, to_half(wo->data.data(), numel(wo))))) return rc;
        if ((rc = upload(e, &b.w_fc, to_half(wf->data.data(), numel(wf))))) return rc;
        if ((rc = upload(e, &b.w_proj, to_half(wp->data.data(), numel(wp))))) return rc;
        if ((rc = upload(e, &b.b_qkv, bq->data))) return rc;
        if ((rc = upload(e, &b.b_out, bo->data))) return rc;
        if ((rc = upload(e, &b.b_fc, bf->data))) return rc;
        if ((rc = upload(e, &b.b_proj, bp->data))) return rc;
        out.push_back(b);
    }
    return GLASS_OK;
}

static int finalize_clip_text(glass_engine* e);

std::vector<_Float16> rn_pack_conv(const float* w, int cout, int cin, int ks) {
    std::vector<_Float16> out((size_t)ks * ks * cout * cin);
    for (int o = 0; o < cout; ++o)
        for (int i = 0; i < cin; ++i)
            for (int t = 0; t < ks * ks; ++t) out[((size_t)t * cout + o) * cin + i] = (_Float16)w[((size_t)o * cin + i) * ks * ks + t];
    return out;
}
// inference BatchNorm (eps 1e-5) under `bn` + ".weight / .bias / .running_mean / .running_var" -> fp32 scale and shift on the device
// (computed in float64, kept out of the fp16 weights: a channel with a tiny running variance would cost them their range)
static int load_rn_bn(glass_engine* e, const std::string& bn, int C, float** a_out, float** s_out) {
    GET(g, bn + ".weight");
    GET(b, bn + ".bias");
    GET(mu, bn + ".running_mean");
    GET(var, bn + ".running_var");
    REQUIRE(numel(g) == (size_t)C && numel(b) == (size_t)C && numel(mu) == (size_t)C && numel(var) == (size_t)C, GLASS_ERR_ARG,
            "bad BatchNorm shapes: " + bn);
    std::vector<float> A(C), S(C);
    for (int i = 0; i < C; ++i) {
        REQUIRE(var->data[i] >= 0.f, GLASS_ERR_ARG, "negative running_var: " + bn);
        const double a = (double)g->data[i] / sqrt((double)var->data[i] + 1e-5);
        A[i] = (float)a;
        S[i] = (float)((double)b->data[i] - (double)mu->data[i] * a);
    }
    int rc = upload(e, a_out, A);
    if (rc) return rc;
    return upload(e, s_out, S);
}
static int load_rn_conv(glass_engine* e, const std::string& conv, const std::string& bn, int cin, int cout, int ks, RnConv& c) {
    GET(w, conv + ".weight");
    REQUIRE(numel(w) == (size_t)cout * cin * ks * ks && w->dims.size() == 4 && w->dims[0] == cout, GLASS_ERR_ARG, "bad conv shape: " + conv);
    c.cin = cin; c.cout = cout; c.ks = ks;
    int rc = upload(e, &c.w, rn_pack_conv(w->data.data(), cout, cin, ks));
    if (rc) return rc;
    return load_rn_bn(e, bn, cout, &c.a, &c.s);
}
// the ModifiedResNet tower under the reference's keys (clip/model.py:100-132); num_batches_tracked is never asked for
static int finalize_clip_resnet(glass_engine* e) {
    const glass_config& c = e->cfg;
    const int w = c.clip_width, G = c.clip_res / 32, T = G * G + 1, C = 32 * w, E = c.clip_embed;
    const std::string v = "clip.visual.";
    RnState& rn = e->rn;
    int rc;
    {
        GET(w1, v + "conv1.weight");
        REQUIRE(numel(w1) == (size_t)(w / 2) * 27, GLASS_ERR_ARG, "bad CLIP ResNet stem conv1 shape");
        std::vector<_Float16> t((size_t)27 * (w / 2));       // [ci][ky][kx] rows, output channel contiguous
        for (int o = 0; o < w / 2; ++o)
            for (int k = 0; k < 27; ++k) t[(size_t)k * (w / 2) + o] = (_Float16)w1->data[(size_t)o * 27 + k];
        if ((rc = upload(e, &rn.stem_w1, t))) return rc;
        if ((rc = load_rn_bn(e, v + "bn1", w / 2, &rn.stem_a1, &rn.stem_s1))) return rc;
    }
    if ((rc = load_rn_conv(e, v + "conv2", v + "bn2", w / 2, w / 2, 3, rn.stem2))) return rc;
    if ((rc = load_rn_conv(e, v + "conv3", v + "bn3", w / 2, w, 3, rn.stem3))) return rc;
    int inplanes = w, res = c.clip_res / 4;
    for (int st = 0; st < 4; ++st) {
        const int planes = w << st;
        for (int i = 0; i < c.clip_rn_layers[st]; ++i) {
            char nm[96];
            snprintf(nm, sizeof nm, "layer%d.%d.", st + 1, i);
            const std::string p = v + nm;
            RnBlock b;
            b.stride = (st > 0 && i == 0) ? 2 : 1;
            b.res_in = res;
            b.has_down = b.stride > 1 || inplanes != 4 * planes;
            if ((rc = load_rn_conv(e, p + "conv1", p + "bn1", inplanes, planes, 1, b.c1))) return rc;
            if ((rc = load_rn_conv(e, p + "conv2", p + "bn2", planes, planes, 3, b.c2))) return rc;
            if ((rc = load_rn_conv(e, p + "conv3", p + "bn3", planes, 4 * planes, 1, b.c3))) return rc;
            if (b.has_down && (rc = load_rn_conv(e, p + "downsample.0", p + "downsample.1", inplanes, 4 * planes, 1, b.down))) return rc;
            rn.blocks.push_back(b);
            inplanes = 4 * planes;
            res /= b.stride;
        }
    }
    const std::string ap = v + "attnpool.";
    GET(pos, ap + "positional_embedding");
    GET(qw, ap + "q_proj.weight");
    GET(kw, ap + "k_proj.weight");
    GET(vw, ap + "v_proj.weight");
    GET(cw, ap + "c_proj.weight");
    GET(qb, ap + "q_proj.bias");
    GET(kb, ap + "k_proj.bias");
    GET(vb, ap + "v_proj.bias");
    GET(cb, ap + "c_proj.bias");
    REQUIRE(numel(pos) == (size_t)T * C && numel(qw) == (size_t)C * C && numel(kw) == (size_t)C * C && numel(vw) == (size_t)C * C &&
                numel(cw) == (size_t)E * C && numel(qb) == (size_t)C && numel(kb) == (size_t)C && numel(vb) == (size_t)C && numel(cb) == (size_t)E,
            GLASS_ERR_ARG, "bad CLIP ResNet attention pool shapes");
    std::vector<_Float16> wqkv((size_t)3 * C * C);
    std::vector<float> bqkv((size_t)3 * C);
    const HostTensor* ws[3] = {qw, kw, vw};
    const HostTensor* bs[3] = {qb, kb, vb};
    for (int j = 0; j < 3; ++j) {
        for (size_t i = 0; i < (size_t)C * C; ++i) wqkv[(size_t)j * C * C + i] = (_Float16)ws[j]->data[i];
        std::copy(bs[j]->data.begin(), bs[j]->data.end(), bqkv.begin() + (size_t)j * C);
    }
    if ((rc = upload(e, &rn.w_qkv, wqkv))) return rc;
    if ((rc = upload(e, &rn.b_qkv, bqkv))) return rc;
    if ((rc = upload(e, &rn.pos, pos->data))) return rc;
    if ((rc = upload(e, &rn.cproj_wt, transposed(cw->data.data(), E, C, 1.f)))) return rc;
    if ((rc = upload(e, &rn.cproj_b, cb->data))) return rc;
    return GLASS_OK;
}
int alloc_clip_resnet(glass_engine* e) {
    const glass_config& c = e->cfg;
    if (c.clip_arch != 1) return GLASS_OK;
    const size_t P = clip_max_images(e), w = c.clip_width, G = c.clip_res / 32, T = G * G + 1, C = 32 * w;
    RnState& rn = e->rn;
    // the largest maps: the stem's (res/2)^2 x w and layer1's (res/4)^2 x 4w, the same size; never below 64 rows of the widest map
    rn.cap = std::max(P * (size_t)(c.clip_res / 2) * (c.clip_res / 2) * w, (size_t)64 * C);
    int rc;
    for (int i = 0; i < 7; ++i) {
        if ((rc = dev_alloc(e, &rn.buf[i], rn.cap))) return rc;
        GLASS_HIP(hipMemset(rn.buf[i], 0, rn.cap * sizeof(half_t)));      // (rows past a short M are read by the padded GEMMs: keep them finite)
    }
    const size_t rows = std::max(P * T, (size_t)64);
    if ((rc = dev_alloc(e, &rn.tok, rows * C))) return rc;
    GLASS_HIP(hipMemset(rn.tok, 0, rows * C * sizeof(half_t)));
    if ((rc = dev_alloc(e, &rn.qkv, rows * 3 * C))) return rc;
    if ((rc = dev_alloc(e, &rn.att, rows * C))) return rc;
    if ((rc = dev_alloc(e, &rn.cls, P * C))) return rc;
    GLASS_HIP(hipDeviceSynchronize());      // the fills ran on the null stream; the engine's streams do not wait for it
    return GLASS_OK;
}

int finalize_clip(glass_engine* e) {
    if (e->cfg.clip_arch == 1) {
        int rc = finalize_clip_resnet(e);
        return rc ? rc : finalize_clip_text(e);
    }
    const glass_config& c = e->cfg;
    const int W = c.clip_width, ps = c.clip_patch, G = c.clip_res / ps, T = G * G + 1, E = c.clip_embed;
    const std::string v = "clip.visual.";
    GET(conv1, v + "conv1.weight");
    GET(cls, v + "class_embedding");
    GET(pos, v + "positional_embedding");
    GET(lg, v + "ln_pre.weight");
    GET(lb, v + "ln_pre.bias");
    GET(pg, v + "ln_post.weight");
    GET(pb, v + "ln_post.bias");
    GET(proj, v + "proj");
    REQUIRE(numel(conv1) == (size_t)W * 3 * ps * ps && numel(cls) == (size_t)W && numel(pos) == (size_t)T * W &&
                numel(proj) == (size_t)W * E,
            GLASS_ERR_ARG, "bad CLIP visual shapes");
    const int K = 3 * ps * ps, Kp = clip_patch_k(c);
    std::vector<_Float16> pw = to_half(conv1->data.data(), numel(conv1));
    if (Kp != K) {      // [W][Kp] with zero columns (patch 14: 588 -> 640)
        std::vector<_Float16> padded((size_t)W * Kp, (_Float16)0.f);
        for (int n = 0; n < W; ++n) std::copy(pw.begin() + (size_t)n * K, pw.begin() + (size_t)(n + 1) * K, padded.begin() + (size_t)n * Kp);
        pw.swap(padded);
    }
    int rc = upload(e, &e->c_patch_w, pw);
    if (rc) return rc;
    if ((rc = upload(e, &e->c_cls, cls->data))) return rc;
    if ((rc = upload(e, &e->c_pos, pos->data))) return rc;
    if ((rc = upload(e, &e->c_lnpre_g, lg->data))) return rc;
    if ((rc = upload(e, &e->c_lnpre_b, lb->data))) return rc;
    if ((rc = upload(e, &e->c_lnpost_g, pg->data))) return rc;
    if ((rc = upload(e, &e->c_lnpost_b, pb->data))) return rc;
    if ((rc = upload(e, &e->c_proj, proj->data))) return rc;  // already [K=W][N=E]
    int rc2 = load_clip_blocks(e, "clip.visual.transformer.resblocks.", c.clip_layers, W, e->cblk);
    if (rc2) return rc2;
    return finalize_clip_text(e);
}

// ---- optional text tower (clip/model.py:277-290) ----
static int finalize_clip_text(glass_engine* e) {
    const int E = e->cfg.clip_embed;
    int rc;
    if (find(e, "clip.token_embedding.weight") != nullptr) {
        GET(tok, "clip.token_embedding.weight");
        GET(tpos, "clip.positional_embedding");
        GET(fg, "clip.ln_final.weight");
        GET(fb, "clip.ln_final.bias");
        GET(tp, "clip.text_projection");
        REQUIRE(tok->dims.size() == 2 && tpos->dims.size() == 2 && tpos->dims[1] == tok->dims[1], GLASS_ERR_ARG,
                "bad CLIP text embedding shapes");
        e->t_vocab = (int)tok->dims[0];
        e->t_width = (int)tok->dims[1];
        e->t_ctx = (int)tpos->dims[0];
        REQUIRE(e->t_width % 64 == 0 && numel(tp) == (size_t)e->t_width * E, GLASS_ERR_ARG, "bad CLIP text projection shape");
        int nl = 0;
        char nm2[256];
        for (;; ++nl) {
            snprintf(nm2, sizeof nm2, "clip.transformer.resblocks.%d.ln_1.weight", nl);
            if (!find(e, nm2)) break;
        }
        if ((rc = upload(e, &e->t_tok, tok->data))) return rc;
        if ((rc = upload(e, &e->t_pos, tpos->data))) return rc;
        if ((rc = upload(e, &e->t_lnf_g, fg->data))) return rc;
        if ((rc = upload(e, &e->t_lnf_b, fb->data))) return rc;
        if ((rc = upload(e, &e->t_proj, tp->data))) return rc;
        if ((rc = load_clip_blocks(e, "clip.transformer.resblocks.", nl, e->t_width, e->tblk))) return rc;
    }
    return GLASS_OK;
}

// clip_resize 1 / 2: the tap table of one axis (both axes share it), built on the host in float64 and kept on the device as fp32
int finalize_preprocess(glass_engine* e) {
    const glass_config& c = e->cfg;
    if (c.clip_resize == 0 || e->R == 0) return GLASS_OK;
    ResizeTaps t;
    std::string why;
    REQUIRE(build_resize_taps(e->R, c.clip_res, c.clip_resize, t, why), GLASS_ERR_ARG, why);
    float* d_table = nullptr;
    int rc = upload(e, &d_table, t.table);
    if (rc) return rc;
    e->rz.table = d_table; e->rz.n4 = (int)(t.table.size() / 4); e->rz.ts = t.ts; e->rz.lds_bytes = t.lds_bytes;
    return GLASS_OK;
}

// Transformer blocks [l0, l1) of a tower: LN -> qkv -> attention -> out (+= x) -> LN -> fc (QuickGELU) -> proj (+= x), over `seqs`
// sequences of T rows in x [seqs * T][W].  pfx: the launches' tag prefix ("clip": tags clip.layernorm, clip.qkv, ...; the stream must be
// e->cur then, the profiling scopes record there); nullptr: no scope and no tag_kernel entry, the profile tables are not touched.
static void run_blocks(glass_engine* e, const std::vector<ClipBlock>& blk, int l0, int l1, float* x, half_t* ln16, half_t* qkv, half_t* att,
                       half_t* hid, int T, int seqs, int W, int heads, int causal, hipStream_t st, const char* pfx) {
    const int M = seqs * T;
    char buf[48];
    auto tag = [&](const char* op) -> const char* {
        if (!pfx) return nullptr;
        snprintf(buf, sizeof buf, "%s.%s", pfx, op);
        return buf;
    };
    auto gemm = [&](const GemmParams& g, const char* op) {
        if (pfx) run_gemm(e, g, tag(op));
        else if (!launch_gemm_tiled(g, st)) launch_gemm_direct(g, st);
    };
    auto layernorm = [&](const float* g, const float* b) {
        Prof pr(e, tag("layernorm"), 0, 6.0 * M * W);
        launch_layernorm(x, W, M, W, g, b, ln16, nullptr, st);
    };
    for (int li = l0; li < l1; ++li) {
        const ClipBlock& b = blk[li];
        layernorm(b.ln1_g, b.ln1_b);
        gemm(gemm_params(ln16, b.w_qkv, M, 3 * W, W, b.b_qkv, 0, qkv, nullptr, T), "qkv");
        {
            Prof pr(e, tag("attention"), 4.0 * seqs * heads * (double)T * T * 64, 8.0 * M * W);
            launch_attention(qkv, seqs, T, heads, 64, causal, att, st);
        }
        gemm(gemm_params(att, b.w_out, M, W, W, b.b_out, 2, nullptr, x, T), "attn_out");
        layernorm(b.ln2_g, b.ln2_b);
        gemm(gemm_params(ln16, b.w_fc, M, 4 * W, W, b.b_fc, 1, hid, nullptr, T), "mlp_fc");
        gemm(gemm_params(hid, b.w_proj, M, W, 4 * W, b.b_proj, 2, nullptr, x, T), "mlp_proj");
    }
}

// ---- the ResNet image tower (clip/model.py:134-149, :39-52, :65-89) ----
GemmParams rn_gemm_1x1(const half_t* x, const RnConv& c, int M, int cand_rows, const half_t* res, int relu, half_t* y) {
    GemmParams g = gemm_params(x, c.w, std::max(M, 64), c.cout, c.cin, nullptr, 5, y, nullptr, cand_rows);
    g.bn_a = c.a; g.bn_s = c.s; g.res16 = res; g.bn_relu = relu;
    return g;
}
GemmParams rn_gemm_3x3(const half_t* x, const RnConv& c, int B, int H, int W, half_t* y) {
    GemmParams g = gemm_params(x, c.w, B * H * W, c.cout, 9 * c.cin, nullptr, 5, y, nullptr, H * W);
    g.bn_a = c.a; g.bn_s = c.s; g.bn_relu = 1;
    g.kpt = c.cin; g.w_tap_stride = (long long)c.cout * c.cin;
    g.g_on = 1; g.g_h = H; g.g_w = W; g.g_hc = H; g.g_wc = W; g.g_stride = 1; g.g_pad = 1; g.g_ks = 3; g.g_cin = c.cin;
    g.g_xbs = (long long)H * W * c.cin;
    return g;
}
static void rn_refused(glass_engine* e, const char* tag) {      // a missing kernel is an error of the pass, never another path
    if (e->launch_error.empty()) e->launch_error = std::string("no kernel accepts layer ") + tag;
}
static void rn_gemm(glass_engine* e, const GemmParams& g, const char* tag) {
    const double rows_a = g.g_on ? (double)g.M * g.g_cin : (double)g.M * g.K;     // the map is read once, not once per tap
    Prof pr(e, tag, 2.0 * g.M * g.N * g.K, 2.0 * (rows_a + (double)g.N * g.K + (double)g.M * g.N * (g.res16 ? 2 : 1)));
    const char* k = launch_gemm_tiled(g, e->cur);
    if (!k) { rn_refused(e, tag); k = "(refused)"; }
    pr.ran(tag, k);
}
static void rn_pool(glass_engine* e, const half_t* x, int B, int H, int C, half_t* y, const char* tag) {
    Prof pr(e, tag, 0, 2.5 * B * H * H * C);
    if (!launch_rn_avgpool2(x, B, H, H, C, y, e->cur)) rn_refused(e, tag);
}
static void run_rn_stem(glass_engine* e, int P) {
    const glass_config& c = e->cfg;
    RnState& rn = e->rn;
    const int w = c.clip_width, S = c.clip_res, H = S / 2;
    {
        Prof pr(e, "clip.stem_conv1", 2.0 * P * H * H * 27 * (w / 2), 2.0 * P * (3.0 * S * S + (double)H * H * (w / 2)));
        if (!launch_rn_stem_conv1(e->d_patches, rn.stem_w1, rn.stem_a1, rn.stem_s1, P, S, w / 2, rn.buf[2], e->cur)) rn_refused(e, "clip.stem_conv1");
    }
    auto conv = [&](const RnConv& k, const half_t* x, half_t* y, const char* tag) {
        Prof pr(e, tag, 2.0 * P * H * H * 9 * k.cin * k.cout, 2.0 * ((double)P * H * H * (k.cin + k.cout) + 9.0 * k.cin * k.cout));
        const char* name = launch_rn_conv3x3(x, k.w, k.a, k.s, P, H, H, k.cin, k.cout, y, e->cur);
        if (!name) { rn_refused(e, tag); name = "(refused)"; }
        pr.ran(tag, name);
    };
    conv(rn.stem2, rn.buf[2], rn.buf[3], "clip.stem_conv2");
    conv(rn.stem3, rn.buf[3], rn.buf[2], "clip.stem_conv3");
    rn_pool(e, rn.buf[2], P, H, w, rn.buf[0], "clip.stem_pool");
}
// bottleneck i reads its input from buf[i & 1] and writes buf[(i + 1) & 1]; buf[2 .. 6] are its temporaries
static void run_rn_blocks(glass_engine* e, int P, int l0, int l1) {
    RnState& rn = e->rn;
    for (int i = l0; i < l1; ++i) {
        const RnBlock& b = rn.blocks[i];
        const int H = b.res_in, Ho = H / b.stride, M = P * H * H, Mo = P * Ho * Ho;
        const half_t* x = rn.buf[i & 1];
        half_t* y = rn.buf[(i + 1) & 1];
        rn_gemm(e, rn_gemm_1x1(x, b.c1, M, H * H, nullptr, 1, rn.buf[2]), "clip.rn_conv1");
        rn_gemm(e, rn_gemm_3x3(rn.buf[2], b.c2, P, H, H, rn.buf[3]), "clip.rn_conv2");
        const half_t* t = rn.buf[3];
        if (b.stride > 1) {
            rn_pool(e, rn.buf[3], P, H, b.c2.cout, rn.buf[4], "clip.rn_pool");
            t = rn.buf[4];
        }
        const half_t* id = x;
        if (b.has_down) {
            const half_t* xd = x;
            if (b.stride > 1) {
                rn_pool(e, x, P, H, b.c1.cin, rn.buf[5], "clip.rn_pool");
                xd = rn.buf[5];
            }
            rn_gemm(e, rn_gemm_1x1(xd, b.down, Mo, Ho * Ho, nullptr, 0, rn.buf[6]), "clip.rn_down");
            id = rn.buf[6];
        }
        rn_gemm(e, rn_gemm_1x1(t, b.c3, Mo, Ho * Ho, id, 1, y), "clip.rn_conv3");      // the residual goes in BEFORE the ReLU
    }
}
static void clip_cosine(glass_engine* e, int P, int views) {      // the end of both towers' heads: d_feat [P][embed] against the target
    const glass_engine::PromptSet& ps = e->pset;      // set_target's feature is the set of one
    if (views < 0 || ps.T == 0) return;    // the features alone (the direction source's own encoding; an encode_* call before any target)
    CosineSet a;
    a.feat = e->d_feat, a.targets = ps.d_targets, a.weights = ps.d_weights, a.W = ps.W;
    a.V = std::max(views, 1), a.P = P / a.V, a.T = ps.T, a.D = e->cfg.clip_embed;
    if (views > 0) a.view_sim = e->d_view_sim;
    a.set_sim = ps.d_sim, a.sim = e->d_sim;
    // image editing: the set's entries are directions, the rows move away from the source's
    if (e->edit.has_source && ps.given()) a.src = e->edit.d_src;
    // a pass of an island search with own prompts: the rows' weights by island
    else if (ps.given() && e->island_row0 >= 0 && e->search.own_prompts) a.isl = {ps.d_isl_weights, ps.d_isl_W, e->search.g.pop, e->island_row0};
    if (!launch_cosine_set(a, e->cur) && e->launch_error.empty())
        e->launch_error = a.src ? "no kernel accepts layer clip.head (cosine_set_dir: shape outside its limits)"
                                : "no kernel accepts layer clip.head (cosine_set: shape outside its limits)";
}
static void run_rn_head(glass_engine* e, int P, int views) {
    const glass_config& c = e->cfg;
    RnState& rn = e->rn;
    const int G = c.clip_res / 32, HW = G * G, T = HW + 1, C = 32 * c.clip_width, heads = c.clip_heads, E = c.clip_embed;
    const half_t* x = rn.buf[rn.blocks.size() & 1];
    {
        Prof pr(e, "clip.attnpool_tokens", 0, 2.0 * P * (HW + T) * C + 4.0 * T * C);
        launch_rn_attnpool_tokens(x, rn.pos, P, HW, C, rn.tok, e->cur);
    }
    {
        GemmParams g = gemm_params(rn.tok, rn.w_qkv, std::max(P * T, 64), 3 * C, C, rn.b_qkv, 0, rn.qkv, nullptr, T);
        rn_gemm(e, g, "clip.attnpool_qkv");
    }
    {
        Prof pr(e, "clip.attnpool_attention", 4.0 * P * heads * (double)T * T * 64, 8.0 * P * T * C);
        launch_attention(rn.qkv, P, T, heads, 64, 0, rn.att, e->cur);
    }
    Prof pr(e, "clip.attnpool_head", 2.0 * P * C * E, 4.0 * C * E);
    launch_rn_token0_rows(rn.att, P, T, C, rn.cls, e->cur);
    launch_dense(rn.cls, C, P, C, rn.cproj_wt, E, rn.cproj_b, e->d_feat, E, 0, 0, nullptr, 0, e->cur);
    clip_cosine(e, P, views);
}

// ---- the image tower (declared in engine.h) ----
int clip_n_layers(const glass_engine* e) { return e->cfg.clip_arch == 1 ? (int)e->rn.blocks.size() : (int)e->cblk.size(); }
void run_clip_embed(glass_engine* e, int P) {
    if (e->cfg.clip_arch == 1) return run_rn_stem(e, P);
    const glass_config& c = e->cfg;
    const int W = c.clip_width, G = c.clip_res / c.clip_patch, T = G * G + 1;
    run_gemm(e, gemm_params(e->d_patches, e->c_patch_w, P * G * G, W, clip_patch_k(c), nullptr, 3, nullptr, e->d_pe, G * G), "clip.patch_embed");
    Prof pr(e, "clip.embed_lnpre", 0, 8.0 * P * T * W);
    launch_embed_lnpre(e->d_pe, e->c_cls, e->c_pos, e->c_lnpre_g, e->c_lnpre_b, P, T, W, e->d_x, e->cur);
}
void run_clip_layers(glass_engine* e, int P, int l0, int l1) {
    if (e->cfg.clip_arch == 1) return run_rn_blocks(e, P, l0, std::min(l1, clip_n_layers(e)));
    const glass_config& c = e->cfg;
    const int G = c.clip_res / c.clip_patch;
    run_blocks(e, e->cblk, l0, std::min(l1, (int)e->cblk.size()), e->d_x, e->d_ln16, e->d_qkv, e->d_attn, e->d_hid, G * G + 1, P, c.clip_width, c.clip_heads, 0, e->cur, "clip");
}
void run_clip_head(glass_engine* e, int P, int views) {
    if (e->cfg.clip_arch == 1) return run_rn_head(e, P, views);
    const glass_config& c = e->cfg;
    const int W = c.clip_width, G = c.clip_res / c.clip_patch, T = G * G + 1;
    Prof pr(e, "clip.head", 2.0 * P * W * c.clip_embed, 4.0 * W * c.clip_embed);
    launch_layernorm(e->d_x, (long long)T * W, P, W, e->c_lnpost_g, e->c_lnpost_b, nullptr, e->d_cls, e->cur);
    launch_dense(e->d_cls, W, P, W, e->c_proj, c.clip_embed, nullptr, e->d_feat, c.clip_embed, 0, 0, nullptr, 0,
                 e->cur);
    clip_cosine(e, P, views);
}
void run_clip(glass_engine* e, int P, int views) {
    run_clip_embed(e, P);
    run_clip_layers(e, P, 0, clip_n_layers(e));
    run_clip_head(e, P, views);
}

// Generated images y [B][3][R][R] -> CLIP's patch operand.  The default (clip_resize 0, clip_normalize 0) launches resize_patches_kernel, which
// reads four input pixels per output; the antialiased modes read the whole image.
double clip_resize_bytes(const glass_engine* e, int B) {
    const glass_config& c = e->cfg;
    if (e->views) return (double)B * e->views * 3 * c.clip_res * c.clip_res * (16 + 2);
    const double out = 2.0 * 3 * c.clip_res * c.clip_res;
    return B * ((c.clip_resize ? 4.0 * 3 * e->R * e->R : 16.0 * c.clip_res * c.clip_res * 3) + out);
}
void run_clip_resize(glass_engine* e, const float* y, int B, half_t* patches) {
    const glass_config& c = e->cfg;
    if (e->views)      // (clip_resize is 0 here: glass_clip_views_supported)
        launch_view_patches(y, B, e->R, c.clip_res, c.clip_patch, clip_patch_k(c), c.clip_normalize, e->views, e->view_boxes, patches, e->cur);
    else if (c.clip_resize == 0 && c.clip_normalize == 0)
        launch_resize_patches(y, B, e->R, c.clip_res, c.clip_patch, clip_patch_k(c), patches, e->cur);
    else
        launch_preprocess_patches(y, B, e->R, c.clip_res, c.clip_patch, clip_patch_k(c), c.clip_resize, c.clip_normalize, e->rz, patches, e->cur);
}

void text_work_free(glass_engine* e) {
    for (void* p : e->twork.owned) hipFree(p);
    e->twork = glass_engine::TextWork();
}

// CLIP text tower: token+pos embedding -> causal transformer -> ln_final -> EOT row @ text_projection
extern "C" int glass_engine_encode_text(glass_engine* e, const int32_t* tokens, int32_t n_texts, int32_t ctx, float* out_feat) {
    REQUIRE(e && tokens && out_feat && n_texts > 0, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "finalize() first");
    REQUIRE(e->t_tok != nullptr, GLASS_ERR_STATE, "CLIP text tower weights were not loaded (clip.token_embedding.weight ...)");
    REQUIRE(ctx == e->t_ctx && ctx <= 128, GLASS_ERR_ARG, "context length does not match positional_embedding");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    const int W = e->t_width, heads = W / 64, M = n_texts * ctx, E = e->cfg.clip_embed;
    std::vector<int> eot(n_texts);
    for (int n = 0; n < n_texts; ++n) {       // text.argmax(dim=-1): EOT has the highest id (clip/model.py:318)
        int best = 0;
        for (int t = 0; t < ctx; ++t) {
            const int v = tokens[(size_t)n * ctx + t];
            REQUIRE(v >= 0 && v < e->t_vocab, GLASS_ERR_ARG, "token id out of range");
            if (v > tokens[(size_t)n * ctx + best]) best = t;
        }
        eot[n] = best;
    }
    auto& tw = e->twork;
    hipError_t err = hipSuccess;
    if (tw.n_texts != n_texts) {          // (re)build the workspace for this batch size
        text_work_free(e);
        if (err == hipSuccess) err = owned_alloc(tw.owned, &tw.d_tok, (size_t)M);
        if (err == hipSuccess) err = owned_alloc(tw.owned, &tw.d_rows, (size_t)n_texts);
        if (err == hipSuccess) err = owned_alloc(tw.owned, &tw.x, (size_t)M * W);
        if (err == hipSuccess) err = owned_alloc(tw.owned, &tw.cls, (size_t)n_texts * W);
        if (err == hipSuccess) err = owned_alloc(tw.owned, &tw.feat, (size_t)n_texts * E);
        if (err == hipSuccess) err = owned_alloc(tw.owned, &tw.ln16, (size_t)M * W);
        if (err == hipSuccess) err = owned_alloc(tw.owned, &tw.qkv, (size_t)M * 3 * W);
        if (err == hipSuccess) err = owned_alloc(tw.owned, &tw.att, (size_t)M * W);
        if (err == hipSuccess) err = owned_alloc(tw.owned, &tw.hid, (size_t)M * 4 * W);
        if (err != hipSuccess) {
            text_work_free(e);
            glass_set_error(std::string("encode_text: hipMalloc failed: ") + hipGetErrorString(err));
            return GLASS_ERR_NOMEM;
        }
        tw.n_texts = n_texts;
    }
    for (int n = 0; n < n_texts; ++n) eot[n] += n * ctx;          // row of each text's EOT token in x
    hipStream_t st = e->stream;
    hipMemcpyAsync(tw.d_tok, tokens, (size_t)M * sizeof(int), hipMemcpyHostToDevice, st);
    hipMemcpyAsync(tw.d_rows, eot.data(), (size_t)n_texts * sizeof(int), hipMemcpyHostToDevice, st);
    launch_embed_text(tw.d_tok, e->t_tok, e->t_pos, M, ctx, W, tw.x, st);
    run_blocks(e, e->tblk, 0, (int)e->tblk.size(), tw.x, tw.ln16, tw.qkv, tw.att, tw.hid, ctx, n_texts, W, heads, 1, st, nullptr);
    // ln_final on the EOT row of each text only (row-wise op): one launch over the gathered rows (round 4: it was one launch per text)
    launch_layernorm_rows(tw.x, tw.d_rows, n_texts, W, e->t_lnf_g, e->t_lnf_b, tw.cls, st);
    launch_dense(tw.cls, W, n_texts, W, e->t_proj, E, nullptr, tw.feat, E, 0, 0, nullptr, 0, st);
    err = hipMemcpyAsync(out_feat, tw.feat, (size_t)n_texts * E * sizeof(float), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err == hipSuccess) err = hipGetLastError();
    if (err != hipSuccess) {
        text_work_free(e);
        glass_set_error(std::string("encode_text failed: ") + hipGetErrorString(err));
        return GLASS_ERR_HIP;
    }
    return GLASS_OK;
}

extern "C" int glass_engine_encode_image(glass_engine* e, const float* images, int32_t n, float* out_feat) {
    REQUIRE(e && images && out_feat && n > 0, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "finalize() first");
    REQUIRE(n <= e->cfg.max_pop, GLASS_ERR_ARG, "more images than max_pop");
    const glass_config& c = e->cfg;
    GLASS_HIP(hipSetDevice(c.device));
    const size_t elems = (size_t)n * 3 * c.clip_res * c.clip_res;
    float* d_img = nullptr;
    GLASS_HIP(hipMalloc(&d_img, elems * sizeof(float)));
    hipError_t err = hipMemcpyAsync(d_img, images, elems * sizeof(float), hipMemcpyHostToDevice, e->stream);
    e->cur = e->stream;
    e->launch_error.clear();
    launch_image_patches(d_img, n, c.clip_res, c.clip_patch, clip_patch_k(c), e->d_patches, e->stream);
    run_clip(e, n);
    if (err == hipSuccess)
        err = hipMemcpyAsync(out_feat, e->d_feat, (size_t)n * c.clip_embed * sizeof(float), hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err == hipSuccess) err = hipGetLastError();
    hipFree(d_img);
    e->prof_events.clear();
    e->event_next = 0;
    if (err != hipSuccess) {
        glass_set_error(std::string("encode_image failed: ") + hipGetErrorString(err));
        return GLASS_ERR_HIP;
    }
    if (!e->launch_error.empty()) {      // a launcher of the tower refused a layer
        const std::string msg = e->launch_error;
        e->launch_error.clear();
        glass_set_error(msg);
        return GLASS_ERR_STATE;
    }
    return GLASS_OK;
}

// The feature a generated image with these pixels gets in the pass: the pass's own preprocessing (run_clip_resize's branches without views, so
// the whole image) and the tower.  What makes an image a prompt (glass_engine_set_targets) that is comparable with the candidates.
extern "C" int glass_engine_encode_generated(glass_engine* e, const float* images, int32_t n, float* out_feat) {
    REQUIRE(e && images && out_feat && n > 0, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->R > 0, GLASS_ERR_STATE, "encode_generated: this engine has no generator (GPT-2 / img2txt): there is no generated-image preprocessing to apply");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "finalize() first");
    REQUIRE(n <= e->cfg.max_pop, GLASS_ERR_ARG, "more images than max_pop");
    const glass_config& c = e->cfg;
    GLASS_HIP(hipSetDevice(c.device));
    const int G = c.clip_res / c.clip_patch;
    const size_t img_elems = (size_t)3 * e->R * e->R, img_patches = (size_t)G * G * clip_patch_k(c);
    const int views = e->views;
    const bool prof = e->profiling;
    e->views = 0;             // the whole image through the non-view preprocessing
    e->profiling = false;     // (profile rows belong to a pass)
    e->cur = e->stream;
    e->launch_error.clear();
    hipError_t err = hipSuccess;
    for (int c0 = 0; c0 < n && err == hipSuccess; c0 += e->chunk) {
        const int B = std::min(e->chunk, n - c0);
        err = hipMemcpyAsync(e->ybuf[0], images + (size_t)c0 * img_elems, (size_t)B * img_elems * sizeof(float), hipMemcpyHostToDevice, e->stream);
        run_clip_resize(e, e->ybuf[0], B, e->d_patches + (size_t)c0 * img_patches);
    }
    run_clip(e, n);
    if (err == hipSuccess)
        err = hipMemcpyAsync(out_feat, e->d_feat, (size_t)n * c.clip_embed * sizeof(float), hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err == hipSuccess) err = hipGetLastError();
    e->views = views;
    e->profiling = prof;
    if (err != hipSuccess) {
        glass_set_error(std::string("encode_generated failed: ") + hipGetErrorString(err));
        return GLASS_ERR_HIP;
    }
    if (!e->launch_error.empty()) {      // a launcher of the tower refused a layer
        const std::string msg = e->launch_error;
        e->launch_error.clear();
        glass_set_error(msg);
        return GLASS_ERR_STATE;
    }
    return GLASS_OK;
}
