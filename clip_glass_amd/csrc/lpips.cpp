// lpips.cpp — host side of the perceptual objective: LPIPS on VGG16 (stylegan2/external_models/lpips.py:34-78) between a candidate's
// generated image, area-downscaled as the reference's projector does (stylegan2/project.py:113-122,263), and a target image.
// Here: the rule, the weights, the buffers, the walk over VGG16's thirteen convolutions and the entry points of include/glass.h.
// Kernels: lpips.hip (input, first convolution, max pool, head) and gemm_tiled (the other twelve convolutions).
#include "engine.h"

#include <string.h>

// torchvision's vgg16 `features` (restated: the layer order is the public VGG16 configuration D): index of the convolution, its channels,
// whether a MaxPool2d(2) stands in front of it, and whether the ReLU behind it ends one of LPIPS's five slices ([0:4], [4:9], [9:16], [16:23], [23:30])
static const struct { int key, cin, cout, pool, end; } VGG[13] = {
    {0, 3, 64, 0, 0},     {2, 64, 64, 0, 1},    {5, 64, 128, 1, 0},   {7, 128, 128, 0, 1},  {10, 128, 256, 1, 0}, {12, 256, 256, 0, 0}, {14, 256, 256, 0, 1},
    {17, 256, 512, 1, 0}, {19, 512, 512, 0, 0}, {21, 512, 512, 0, 1}, {24, 512, 512, 1, 0}, {26, 512, 512, 0, 0}, {28, 512, 512, 0, 1}};
static const int SLICE_C[5] = {64, 128, 256, 512, 512};

extern "C" int glass_lpips_supported(int32_t gen_res, int32_t S) {
    REQUIRE(S >= 16 && S <= 512 && S % 16 == 0, GLASS_ERR_ARG,
            "lpips_size must be a multiple of 16 in [16, 512] (VGG16's four max pools need even sides), got " + std::to_string(S));
    if (gen_res == 0) return GLASS_OK;
    REQUIRE(gen_res > 0 && gen_res % S == 0, GLASS_ERR_ARG,
            "lpips_size " + std::to_string(S) + " must divide the generated image's side " + std::to_string(gen_res) +
                " (the area downscale is an exact box mean)");
    REQUIRE(gen_res / S <= 8, GLASS_ERR_ARG,
            "the area downscale's box is at most 8 pixels a side: " + std::to_string(gen_res) + " / " + std::to_string(S) + " = " +
                std::to_string(gen_res / S));
    return GLASS_OK;
}

int finalize_lpips(glass_engine* e) {
    const glass_config& c = e->cfg;
    if (c.lpips_size <= 0) return GLASS_OK;
    LpState& lp = e->lp;
    lp.S = c.lpips_size;
    lp.box = e->R / lp.S;
    lp.sub = std::max(1, std::min(e->chunk, GLASS_LPIPS_SUB));
    int rc;
    const std::string f = "lpips.features.";
    for (int i = 0; i < 13; ++i) {
        const std::string k = f + std::to_string(VGG[i].key);
        GET(w, k + ".weight");
        GET(b, k + ".bias");
        const int cin = VGG[i].cin, cout = VGG[i].cout;
        REQUIRE(numel(w) == (size_t)cout * cin * 9 && w->dims.size() == 4 && w->dims[0] == cout && numel(b) == (size_t)cout, GLASS_ERR_ARG,
                "bad VGG16 conv shape: " + k);
        if (i == 0) {
            std::vector<_Float16> t((size_t)27 * 64);       // [ci][ky][kx] rows, output channel contiguous
            for (int o = 0; o < 64; ++o)
                for (int q = 0; q < 27; ++q) t[(size_t)q * 64 + o] = (_Float16)w->data[(size_t)o * 27 + q];
            if ((rc = upload(e, &lp.w1, t))) return rc;
            if ((rc = upload(e, &lp.b1, b->data))) return rc;
            continue;
        }
        RnConv& cv = lp.conv[i - 1];
        cv.cin = cin; cv.cout = cout; cv.ks = 3;
        if ((rc = upload(e, &cv.w, rn_pack_conv(w->data.data(), cout, cin, 3)))) return rc;
        if ((rc = upload(e, &cv.s, b->data))) return rc;
    }
    if ((rc = upload(e, &lp.ones, std::vector<float>(512, 1.f)))) return rc;
    for (int i = 0; i < 12; ++i) lp.conv[i].a = lp.ones;
    const size_t S = lp.S, sub = lp.sub;
    for (int k = 0; k < 5; ++k) {
        const std::string key = "lpips.lin." + std::to_string(k) + ".weight";
        GET(l, key);
        REQUIRE(numel(l) == (size_t)SLICE_C[k], GLASS_ERR_ARG, "bad LPIPS lin shape: " + key);
        for (float v : l->data) REQUIRE(v >= 0.f, GLASS_ERR_ARG, "negative LPIPS lin weight: " + key);
        if ((rc = upload(e, &lp.lin[k], l->data))) return rc;
        const size_t side = S >> k, elems = side * side * SLICE_C[k];
        if ((rc = dev_alloc(e, &lp.tgt[k], elems))) return rc;
        if ((rc = dev_alloc(e, &lp.pair[k], elems))) return rc;
    }
    if ((rc = dev_alloc(e, &lp.in, sub * S * S * 4))) return rc;
    for (int i = 0; i < 2; ++i)
        if ((rc = dev_alloc(e, &lp.buf[i], sub * S * S * 64))) return rc;
    if ((rc = dev_alloc(e, &lp.stage, 3 * S * S))) return rc;
    if ((rc = dev_alloc(e, &lp.part, sub * ((S * S + GLASS_LPIPS_PIXB - 1) / GLASS_LPIPS_PIXB)))) return rc;
    if ((rc = dev_alloc(e, &lp.d, (size_t)c.max_pop))) return rc;
    if ((rc = dev_alloc(e, &lp.d_one, 1))) return rc;
    return GLASS_OK;
}

static void lp_refused(glass_engine* e, const char* tag) {      // a missing kernel is an error of the pass, never another path
    if (e->launch_error.empty()) e->launch_error = std::string("no kernel accepts layer ") + tag;
}

// VGG16 over the n <= sub images in lp.in, on e->cur.  Behind every slice: save != nullptr: its output (n = 1) is copied to save[k];
// otherwise the head adds the slice's term against ref[k] (one map for every image where ref_shared, else image i's own) into dout[i].
static void lpips_walk(glass_engine* e, int n, half_t* const* save, half_t* const* ref, bool ref_shared, float* dout) {
    LpState& lp = e->lp;
    int H = lp.S, cur = 0, k = 0;
    {
        Prof pr(e, "lpips.conv1", 2.0 * n * H * H * 27 * 64, 2.0 * n * H * H * (4 + 64));
        if (!launch_vgg_conv1(lp.in, lp.w1, lp.b1, n, H, lp.buf[0], e->cur)) lp_refused(e, "lpips.conv1");
        pr.ran("lpips.conv1", "vgg_conv1_kernel");
    }
    for (int i = 1; i < 13; ++i) {
        const RnConv& cv = lp.conv[i - 1];
        if (VGG[i].pool) {
            Prof pr(e, "lpips.pool", 0, 2.5 * n * H * H * cv.cin);
            if (!launch_maxpool2(lp.buf[cur], n, H, H, cv.cin, lp.buf[cur ^ 1], e->cur)) lp_refused(e, "lpips.pool");
            pr.ran("lpips.pool", "maxpool2_kernel");
            H >>= 1;
            cur ^= 1;
        }
        {
            const GemmParams g = rn_gemm_3x3(lp.buf[cur], cv, n, H, H, lp.buf[cur ^ 1]);
            Prof pr(e, "lpips.conv", 2.0 * g.M * g.N * g.K, 2.0 * ((double)g.M * g.g_cin + (double)g.N * g.K + (double)g.M * g.N));
            const char* name = launch_gemm_tiled(g, e->cur);
            if (!name) { lp_refused(e, "lpips.conv"); name = "(refused)"; }
            pr.ran("lpips.conv", name);
            cur ^= 1;
        }
        if (!VGG[i].end) continue;
        const int C = cv.cout, HW = H * H;
        if (save) {
            hipMemcpyAsync(save[k], lp.buf[cur], (size_t)HW * C * sizeof(half_t), hipMemcpyDeviceToDevice, e->cur);
        } else {
            Prof pr(e, "lpips.head", 6.0 * n * HW * C, 2.0 * (n + (ref_shared ? 1 : n)) * (double)HW * C);
            if (!launch_lpips_head(lp.buf[cur], ref[k], ref_shared ? 0 : (long long)HW * C, lp.lin[k], n, HW, C, lp.part, k == 0, dout, e->cur))
                lp_refused(e, "lpips.head");
            pr.ran("lpips.head", "lpips_head_kernel");
        }
        ++k;
    }
}

void run_lpips_chunk(glass_engine* e, const float* y, int c0, int B) {
    LpState& lp = e->lp;
    const size_t img = (size_t)3 * e->R * e->R;
    for (int s0 = 0; s0 < B; s0 += lp.sub) {
        const int n = std::min(lp.sub, B - s0);
        {
            Prof pr(e, "lpips.input", 0, 4.0 * n * img + 8.0 * n * lp.S * lp.S);
            if (!launch_lpips_input(y + (size_t)s0 * img, n, e->R, lp.S, lp.in, e->cur)) lp_refused(e, "lpips.input");
            pr.ran("lpips.input", "lpips_input_kernel");
        }
        lpips_walk(e, n, nullptr, lp.tgt, true, lp.d + c0 + s0);
    }
}

// one caller image [3][S][S] -> lp.in (box 1), on the main stream
static int lpips_stage(glass_engine* e, const float* img) {
    LpState& lp = e->lp;
    const size_t bytes = (size_t)3 * lp.S * lp.S * sizeof(float);
    GLASS_HIP(hipMemcpyAsync(lp.stage, img, bytes, hipMemcpyHostToDevice, e->stream));
    REQUIRE(launch_lpips_input(lp.stage, 1, lp.S, lp.S, lp.in, e->stream), GLASS_ERR_STATE, "no kernel accepts layer lpips.input");
    return GLASS_OK;
}
// the walks outside a pass: no profile rows, the main stream, and the launchers' verdict as the call's status
static int lpips_walk_now(glass_engine* e, half_t* const* save, half_t* const* ref, float* dout) {
    const bool prof = e->profiling;
    e->profiling = false;
    e->cur = e->stream;
    e->launch_error.clear();
    lpips_walk(e, 1, save, ref, true, dout);
    e->profiling = prof;
    GLASS_HIP(hipStreamSynchronize(e->stream));
    GLASS_HIP(hipGetLastError());
    if (!e->launch_error.empty()) {
        const std::string msg = e->launch_error;
        e->launch_error.clear();
        glass_set_error(msg);
        return GLASS_ERR_STATE;
    }
    return GLASS_OK;
}

extern "C" int glass_engine_set_lpips_target(glass_engine* e, const float* img, int32_t S) {
    REQUIRE(e && img, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "finalize() first");
    REQUIRE(e->cfg.lpips_size > 0, GLASS_ERR_STATE, "set_lpips_target: the perceptual objective is off (glass_config::lpips_size = 0)");
    REQUIRE(S == e->cfg.lpips_size, GLASS_ERR_ARG, "set_lpips_target: the target must be [3][lpips_size][lpips_size]");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    int rc = lpips_stage(e, img);
    if (rc) return rc;
    if ((rc = lpips_walk_now(e, e->lp.tgt, nullptr, nullptr))) return rc;
    e->lp.has_target = true;
    return GLASS_OK;
}

extern "C" int glass_engine_lpips(glass_engine* e, const float* x0, const float* x1, int32_t n, float* out) {
    REQUIRE(e && x0 && x1 && out, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "finalize() first");
    REQUIRE(e->cfg.lpips_size > 0, GLASS_ERR_STATE, "lpips: the perceptual objective is off (glass_config::lpips_size = 0)");
    REQUIRE(n > 0, GLASS_ERR_ARG, "lpips: n must be positive");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    LpState& lp = e->lp;
    const size_t img = (size_t)3 * lp.S * lp.S;
    for (int i = 0; i < n; ++i) {      // one pair at a time: x1's five maps, then x0 against them
        int rc = lpips_stage(e, x1 + (size_t)i * img);
        if (rc) return rc;
        if ((rc = lpips_walk_now(e, lp.pair, nullptr, nullptr))) return rc;
        if ((rc = lpips_stage(e, x0 + (size_t)i * img))) return rc;
        if ((rc = lpips_walk_now(e, nullptr, lp.pair, lp.d_one))) return rc;
        GLASS_HIP(hipMemcpy(out + i, lp.d_one, sizeof(float), hipMemcpyDeviceToHost));
    }
    return GLASS_OK;
}

extern "C" int glass_engine_last_lpips(glass_engine* e, int32_t P, float* d) {
    REQUIRE(e && d, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->finalized && e->cfg.lpips_size > 0, GLASS_ERR_STATE, "last_lpips: the perceptual objective is off or the engine is not finalized");
    REQUIRE(P > 0 && P <= e->last_P, GLASS_ERR_ARG, "P exceeds the last evaluated population");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    GLASS_HIP(hipMemcpy(d, e->lp.d, (size_t)P * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}
