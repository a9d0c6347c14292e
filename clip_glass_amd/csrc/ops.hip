// ops.hip — diagnostic per-kernel C ABI (include/glass_ops.h): host fp32 buffers in/out.
#include <string.h>

#include <string>
#include <vector>

#include "../../include/glass_ops.h"
#include "engine.h"
#include "kernels.h"

namespace {
struct Dev {
    std::vector<void*> ptrs;
    ~Dev() {
        for (void* p : ptrs) hipFree(p);
    }
    template <typename T>
    T* alloc(size_t n) {
        void* q = nullptr;
        if (hipMalloc(&q, (n ? n : 1) * sizeof(T)) != hipSuccess) return nullptr;
        ptrs.push_back(q);
        return (T*)q;
    }
    half_t* up16(const float* src, size_t n) {
        if (!src) return nullptr;
        std::vector<_Float16> h(n);
        for (size_t i = 0; i < n; ++i) h[i] = (_Float16)src[i];
        half_t* d = alloc<half_t>(n);
        if (d) hipMemcpy(d, h.data(), n * sizeof(half_t), hipMemcpyHostToDevice);
        return d;
    }
    half_t* up16v(const std::vector<_Float16>& h) {
        half_t* d = alloc<half_t>(h.size());
        if (d) hipMemcpy(d, h.data(), h.size() * sizeof(half_t), hipMemcpyHostToDevice);
        return d;
    }
    float* up32(const float* src, size_t n) {
        if (!src) return nullptr;
        float* d = alloc<float>(n);
        if (d) hipMemcpy(d, src, n * sizeof(float), hipMemcpyHostToDevice);
        return d;
    }
};
int down16(float* dst, const half_t* src, size_t n) {
    std::vector<_Float16> h(n);
    GLASS_HIP(hipMemcpy(h.data(), src, n * sizeof(half_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) dst[i] = (float)h[i];
    return GLASS_OK;
}
int finish() {
    GLASS_HIP(hipDeviceSynchronize());
    GLASS_HIP(hipGetLastError());
    return GLASS_OK;
}
}  // namespace

#define OPREQ(cond, msg)               \
    do {                               \
        if (!(cond)) {                 \
            glass_set_error(msg);      \
            return GLASS_ERR_ARG;      \
        }                              \
    } while (0)

extern "C" int glass_op_conv(int32_t device, const glass_conv_desc* d) {
    OPREQ(d && d->x && d->w && d->y, "null argument");
    OPREQ(d->Cin % 16 == 0, "Cin must be a multiple of 16");
    OPREQ(d->out_scale > 0.f, "out_scale must be positive (the epilogues fold it into the activation constants: max(v k1, v k2))");
    OPREQ(!d->pre_shift || d->sn, "pre_shift needs sn (the input affine is relu(x * sn + pre_shift))");
    OPREQ(d->in_up == 0 || (d->in_up == 1 && d->H % 2 == 0 && d->W % 2 == 0 && !d->up && !d->broadcast_x),
          "in_up: H and W are the upsampled dims and must be even (not with up / broadcast_x)");
    OPREQ(d->res_up == 0 || (d->res_up == 1 && d->res && d->Ho % 2 == 0 && d->Wo % 2 == 0), "res_up: needs res, Ho and Wo even");
    OPREQ(d->res_cs == 0 || (d->res && d->res_cs >= d->Cout), "res_cs: needs res, res_cs >= Cout");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    ConvParams p = conv_defaults();
    const int Hx = d->H >> d->in_up, Wx = d->W >> d->in_up;      // the stored input map
    const size_t xin = (size_t)(d->broadcast_x ? 1 : d->B) * Hx * Wx * d->Cin;
    p.x = dv.up16(d->x, xin);
    p.x_bstride = d->broadcast_x ? 0 : (long long)Hx * Wx * d->Cin;
    p.in_up = d->in_up;
    p.B = d->B; p.H = d->H; p.W = d->W; p.Cin = d->Cin;
    p.KS = d->KS; p.stride = d->stride; p.pad = d->pad; p.up = d->up;
    p.Cout = d->Cout; p.Neff = d->up ? 4 * d->Cout : d->Cout;
    p.Ho = d->Ho; p.Wo = d->Wo;
    p.Hc = d->up ? d->H : d->Ho; p.Wc = d->up ? d->W : d->Wo;
    std::vector<_Float16> pk;
    if (d->up) {
        OPREQ(d->KS == 3 && d->stride == 1 && d->pad == 1 && d->Ho == 2 * d->H, "up conv expects KS 3 / pad 1");
        glass_fold_upconv(d->w, d->Cout, d->Cin, pk);
    } else {
        glass_pack_conv(d->w, d->Cout, d->Cin, d->KS, d->Cin, pk);
    }
    p.w = dv.up16v(pk);
    if (d->up) {
        std::vector<_Float16> pk2;
        glass_pack_conv(d->w, d->Cout, d->Cin, 3, d->Cin, pk2);
        p.w_up = dv.up16v(pk2);
    }
    if (d->pre_shift) {       // one per-candidate table [A | S], fp32 and fp16, as bg_conv points sn / pre_shift / sn16 / pre_shift16 into tab / tab16
        std::vector<float> tab((size_t)d->B * 2 * d->Cin);
        for (int b = 0; b < d->B; ++b)
            for (int c = 0; c < d->Cin; ++c) {
                tab[((size_t)b * 2) * d->Cin + c] = d->sn[(size_t)b * d->Cin + c];
                tab[((size_t)b * 2 + 1) * d->Cin + c] = d->pre_shift[(size_t)b * d->Cin + c];
            }
        const float* t32 = dv.up32(tab.data(), tab.size());
        const half_t* t16 = dv.up16(tab.data(), tab.size());
        OPREQ(t32 && t16, "device allocation failed");
        p.sn = t32; p.pre_shift = t32 + d->Cin; p.sn16 = t16; p.pre_shift16 = t16 + d->Cin; p.sn_stride = 2 * d->Cin;
    } else {
        p.sn = dv.up32(d->sn, (size_t)d->B * d->Cin); p.sn_stride = d->Cin;
        p.sn16 = dv.up16(d->sn, (size_t)d->B * d->Cin);
    }
    if (d->shift) {           // one table [dscale | shift], as bg_conv points dscale / shift into tab
        std::vector<float> tab((size_t)d->B * 2 * d->Cout);
        for (int b = 0; b < d->B; ++b)
            for (int c = 0; c < d->Cout; ++c) {
                tab[((size_t)b * 2) * d->Cout + c] = d->dscale ? d->dscale[(size_t)b * d->Cout + c] : 1.f;
                tab[((size_t)b * 2 + 1) * d->Cout + c] = d->shift[(size_t)b * d->Cout + c];
            }
        const float* t32 = dv.up32(tab.data(), tab.size());
        OPREQ(t32, "device allocation failed");
        p.dscale = d->dscale ? t32 : nullptr; p.shift = t32 + d->Cout; p.ds_stride = 2 * d->Cout;
    } else {
        p.dscale = dv.up32(d->dscale, (size_t)d->B * d->Cout); p.ds_stride = d->Cout;
    }
    p.batch_size = d->batch_size > 0 ? d->batch_size : 1;
    p.noise = dv.up32(d->noise, (size_t)(d->B / p.batch_size) * d->Ho * d->Wo);
    p.noise_strength = d->noise_strength;
    p.bias = dv.up32(d->bias, d->Cout);
    p.act = d->act;
    const size_t nout = (size_t)d->B * d->Ho * d->Wo * d->Cout;
    p.res_cs = d->res_cs; p.res_up = d->res_up;
    p.res = dv.up16(d->res, (size_t)d->B * (d->Ho >> d->res_up) * (d->Wo >> d->res_up) * (d->res_cs ? d->res_cs : d->Cout));
    p.out_scale = d->out_scale;
    half_t* y = dv.alloc<half_t>(nout);
    p.y = y;
    OPREQ(p.x && p.w && y, "device allocation failed");
    if (d->skip_x) {
        OPREQ(d->skip_w, "fused skip branch: skip_x and skip_w");
        std::vector<_Float16> pks;
        glass_pack_conv(d->skip_w, d->Cout, d->Cin, 1, d->Cin, pks);
        p.skip_w = dv.up16v(pks);
        p.skip_x = dv.up16(d->skip_x, (size_t)d->B * d->Ho * d->Wo * d->Cin);
    }
    half_t* xs_dev = nullptr;
    const size_t nxs = (size_t)d->B * (d->H / 2) * (d->W / 2) * d->Cin;
    if (d->xs_out) {
        xs_dev = dv.alloc<half_t>(nxs);
        p.xs_out = xs_dev;
    }
    float* yrgb = nullptr;
    const size_t nrgb = (size_t)d->B * 3 * d->Ho * d->Wo;
    if (d->trgb_yout) {
        OPREQ(d->trgb_w && d->trgb_b && d->trgb_sn && d->trgb_smax, "fused toRGB: all of w / b / sn / smax");
        p.trgb_w = dv.up32(d->trgb_w, 3 * (size_t)d->Cout); p.trgb_b = dv.up32(d->trgb_b, 3);
        p.trgb_sn = dv.up32(d->trgb_sn, (size_t)d->B * d->Cout); p.trgb_sn_stride = d->Cout;
        p.trgb_smax = dv.up32(d->trgb_smax, d->B); p.trgb_smax_stride = 1;
        p.trgb_yprev = dv.up32(d->trgb_yprev, (size_t)d->B * 3 * (d->Ho / 2) * (d->Wo / 2));
        yrgb = dv.alloc<float>(nrgb);
        p.trgb_yout = yrgb;
        if (d->impl == 4 && !d->trgb_keep_map) {
            p.y = nullptr;                       // the streaming form never stores the map
        } else {                                 // the forms that store it too: weight tables from the table kernel
            half_t* tab = dv.alloc<half_t>((size_t)d->B * 32 * d->Cout);
            launch_trgb_tables(p.trgb_w, p.trgb_sn, p.trgb_sn_stride, p.trgb_smax, p.trgb_smax_stride, d->B, d->Cout, tab, 0);
            p.trgb_tab = tab;
        }
    }
    p.x_planar8 = d->x_planar8;
    p.x_planar32 = d->x_planar32;
    p.y_planar8 = d->y_planar8;
    if (d->post_scale) {
        p.post_scale16 = dv.up16(d->post_scale, (size_t)d->B * d->Cout); p.post_stride = d->Cout;
        OPREQ(p.post_scale16, "device allocation failed");
    }
    if (d->premod) {      // per-sample pre-modulated weights, set up as stylegan2.cpp g_conv_params does for a premod layer
        OPREQ(d->sn && d->KS == 3 && !d->broadcast_x, "premod: 3x3 with sn, not with broadcast_x");
        OPREQ(!d->up || d->impl == 3, "premod up-conv: impl 3 only (the folded table is not modulated)");
        const long long welems = 9LL * d->Cin * d->Cout;
        half_t* wm = dv.alloc<half_t>((size_t)d->B * welems);
        OPREQ(wm && p.sn && (p.dscale || !d->dscale), "device allocation failed");
        launch_modulate_weights(d->up ? p.w_up : p.w, welems, d->Cin, d->Cout, p.sn, p.sn_stride, p.dscale, p.ds_stride, d->B, wm, 0);
        p.sn = nullptr; p.sn16 = nullptr; p.dscale = nullptr; p.w_bstride = welems;
        if (d->up) { p.w_up = wm; p.w = nullptr; }
        else p.w = wm;
    }
    float* ytanh = nullptr;
    if (d->rgb_tanh) {
        ytanh = dv.alloc<float>(nrgb);
        OPREQ(ytanh, "device allocation failed");
        GLASS_HIP(hipMemset(ytanh, 0xFF, nrgb * sizeof(float)));        // NaN: a pixel the conv does not write shows
        p.rgb_tanh_out = ytanh;
    }
    float* part = nullptr;
    const float* part_yprev = p.trgb_yprev;
    const int ntn = d->Cout / 128;
    if (d->trgb_partial) {   // toRGB partial sums per 128-wide n tile, as torgb_conv_params sets ToRgb::partial up; launch_trgb_finish below
        OPREQ(yrgb && d->Cout % 128 == 0 && d->Ho == d->Wo, "toRGB partial sums: the trgb inputs, Cout % 128 == 0, Ho == Wo");
        const size_t npart = (size_t)ntn * nrgb;
        part = dv.alloc<float>(npart);
        OPREQ(part, "device allocation failed");
        GLASS_HIP(hipMemset(part, 0xFF, npart * sizeof(float)));      // NaN: a partial the conv does not write shows in the sum
        p.trgb_part = part; p.trgb_yout = nullptr; p.trgb_yprev = nullptr;
    }
    // ask the families of `impl` in order; a refusal names every family asked and the features it lacks
    static const char* const labels[7] = {"no kernel accepts this convolution", "direct conv: unsupported launch", "tiled conv: unsupported shape", "fused up-conv: unsupported shape",
                                          "streaming conv: unsupported shape", "LDS-DMA conv: unsupported shape", "im2col + GEMM conv: unsupported shape"};
    std::string why;
    ConvKernel k;
    auto refused = [&](const char* family, uint32_t outside) {
        why += std::string(why.empty() ? " (" : "; ") + family + (outside ? " does not implement" : " does not take this shape or this combination of");
        for (int bit = 0; bit < CF_COUNT; ++bit)
            if ((outside ? outside : conv_features(p)) >> bit & 1) why += std::string(" [") + conv_feature_name(bit) + "]";
        return false;
    };
    auto ask = [&](const char* family, const ConvKernel& c) { return c ? (k = c, true) : refused(family, c.outside); };
    bool ran = false;
    switch (d->impl) {
    case 1: ask("conv_direct", choose_conv_direct(p)); break;
    case 2: ask("conv_s2", choose_conv_s2(p)) || ask("conv_tiled", choose_conv_tiled(p)); break;
    case 3: ask("upfir", choose_conv_upfir(p)); break;
    case 4: ask("conv_stream", choose_conv_stream(p)); break;
    case 5: p.skip_x ? ask("conv_s2", choose_conv_s2(p, true)) : ask("conv_wreg", choose_conv_wreg(p)) || ask("conv_glds", choose_conv_glds(p)); break;
    case 6: {   // scratch per candidate; room for the four split-K slices the launcher may choose, as the engine's scratch (256 * 4 * cmax floats) always has
        const long long cap_a = (long long)p.Hc * p.Wc * p.KS * p.KS * p.Cin, cap_c = 4LL * p.Hc * p.Wc * p.Neff;
        uint32_t outside = 0;
        ran = conv_gemm_admits(p, cap_a, cap_c, &outside) &&
              launch_conv_gemm(p, dv.alloc<half_t>((size_t)(cap_a * p.B)), cap_a, dv.alloc<float>((size_t)(cap_c * p.B)), cap_c, 0);
        if (!ran) refused("conv_gemm", outside);
    } break;
    default:
        (d->up && ask("upfir", choose_conv_upfir(p))) || ask("conv_stream", choose_conv_stream(p)) || ask("conv_s2", choose_conv_s2(p)) ||
            ask("conv_tiled", choose_conv_tiled(p)) || ask("conv_direct", choose_conv_direct(p));
    }
    if (k) k.launch(p, 0);
    else if (!ran) {   // (the planar tanh keeps the words its earlier refusal had)
        glass_set_error(((ytanh ? "rgb_tanh: conv_tiled only; " : "") + std::string(labels[d->impl >= 1 && d->impl <= 6 ? d->impl : 0]) + why + ")").c_str());
        return GLASS_ERR_ARG;
    }
    int rc = finish();
    if (rc) return rc;
    if (part) {
        launch_trgb_finish(part, ntn, d->B, d->Ho, p.trgb_b, part_yprev, yrgb, 0);
        if ((rc = finish())) return rc;
    }
    if (ytanh) {              // (p.y is not written)
        GLASS_HIP(hipMemcpy(d->rgb_tanh, ytanh, nrgb * sizeof(float), hipMemcpyDeviceToHost));
        return GLASS_OK;
    }
    if (yrgb) {
        GLASS_HIP(hipMemcpy(d->trgb_yout, yrgb, nrgb * sizeof(float), hipMemcpyDeviceToHost));
        return p.y ? down16(d->y, y, nout) : GLASS_OK;      // (the forms that also store the feature map hand it back too)
    }
    if (xs_dev && (rc = down16(d->xs_out, xs_dev, nxs))) return rc;
    return down16(d->y, y, nout);
}

extern "C" int glass_op_gemm(int32_t device, int32_t M, int32_t N, int32_t K, const float* a, const float* w,
                             const float* bias, int32_t mode, int32_t impl, float* out) {
    OPREQ(a && w && out && K % 16 == 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    GemmParams g;
    memset(&g, 0, sizeof g);
    g.a = dv.up16(a, (size_t)M * K); g.w = dv.up16(w, (size_t)N * K); g.M = M; g.N = N; g.K = K;
    g.bias = dv.up32(bias, N); g.mode = mode; g.ldo = N;
    const size_t n = (size_t)M * N;
    half_t* o16 = nullptr; float* o32 = nullptr;
    if (mode <= 1) { o16 = dv.alloc<half_t>(n); g.out16 = o16; }
    else { o32 = mode == 2 ? dv.up32(out, n) : dv.alloc<float>(n); g.out32 = o32; }
    if (impl == 1) launch_gemm_direct(g, 0);
    else if (impl == 2) {
        if (!launch_gemm_tiled(g, 0)) { glass_set_error("tiled gemm: unsupported shape"); return GLASS_ERR_ARG; }
    } else if (!launch_gemm_tiled(g, 0)) launch_gemm_direct(g, 0);
    int rc = finish();
    if (rc) return rc;
    if (o16) return down16(out, o16, n);
    GLASS_HIP(hipMemcpy(out, o32, n * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_gemm_batched(int32_t device, int32_t batch, int32_t M, int32_t N, int32_t K, const float* a, const float* w, int32_t mode,
                                     int32_t cand_batch, int32_t impl, float* out) {
    OPREQ(a && w && out && batch >= 1 && M > 0 && N > 0 && K > 0 && K % 16 == 0, "bad argument (K a multiple of 16)");
    OPREQ(mode == 0 || mode == 3, "batched gemm: mode 0 (fp16 out) or 3 (fp32 out), the self-attention products");
    OPREQ(impl >= 0 && impl <= 2, "impl must lie in [0, 2]");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t n = (size_t)batch * M * N;
    half_t* da = dv.up16(a, (size_t)batch * M * K);
    half_t* dw = dv.up16(w, (size_t)batch * N * K);
    half_t* o16 = mode == 0 ? dv.alloc<half_t>(n) : nullptr;
    float* o32 = mode == 3 ? dv.alloc<float>(n) : nullptr;
    OPREQ(da && dw && (o16 || o32), "device allocation failed");
    GLASS_HIP(hipMemset(o16 ? (void*)o16 : (void*)o32, 0xFF, n * (o16 ? sizeof(half_t) : sizeof(float))));      // NaN: an element nobody stores shows
    GemmParams g = gemm_params(da, dw, M, N, K, nullptr, mode, o16, o32, 0);      // as bg_attention (biggan.cpp)
    g.cand_batch = cand_batch ? 1 : 0;
    g.batch = batch; g.a_bs = (long long)M * K; g.w_bs = (long long)N * K; g.o_bs = (long long)M * N;
    if (impl == 1) launch_gemm_direct(g, 0);
    else if (impl == 2) {
        if (!launch_gemm_tiled(g, 0)) { glass_set_error("tiled gemm: unsupported shape"); return GLASS_ERR_ARG; }
    } else if (!launch_gemm_tiled(g, 0)) launch_gemm_direct(g, 0);
    int rc = finish();
    if (rc) return rc;
    if (o16) return down16(out, o16, n);
    GLASS_HIP(hipMemcpy(out, o32, n * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_dense(int32_t device, int32_t P, int32_t K, int32_t N, const float* x, const float* wt,
                              const float* bias, int32_t in_sq, int32_t mode, const float* eps_row, float* out) {
    OPREQ(x && wt && out, "null argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dx = dv.up32(x, (size_t)P * K); float* dw = dv.up32(wt, (size_t)K * N); float* db = dv.up32(bias, N);
    float* de = dv.up32(eps_row, P); float* dout = dv.alloc<float>((size_t)P * N);
    launch_dense(dx, K, P, K, dw, N, db, dout, N, in_sq, mode, de, 1, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, dout, (size_t)P * N * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_torgb(int32_t device, int32_t B, int32_t H, int32_t C, const float* x, const float* wrgb,
                              const float* bias, const float* sn, const float* smax, const float* yprev, float* yout) {
    OPREQ(x && wrgb && bias && sn && smax && yout, "null argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    half_t* dx = dv.up16(x, (size_t)B * H * H * C);
    float* dw = dv.up32(wrgb, 3 * C); float* db = dv.up32(bias, 3); float* ds = dv.up32(sn, (size_t)B * C);
    float* dm = dv.up32(smax, B); float* dp = dv.up32(yprev, (size_t)B * 3 * (H / 2) * (H / 2));
    float* dy = dv.alloc<float>((size_t)B * 3 * H * H);
    OPREQ(launch_torgb(dx, B, H, H, C, dw, db, ds, C, dm, 1, dp, dy, 0), "toRGB: channel width not instantiated");
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(yout, dy, (size_t)B * 3 * H * H * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_blur(int32_t device, int32_t mode, int32_t B, int32_t H, int32_t C, const float* x, float* out) {
    OPREQ(x && out && C % 8 == 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    half_t* dx = dv.up16(x, (size_t)B * H * H * C);
    OPREQ(mode != 2 || blur_pad2_planar32_ok(C), "blur in 32-channel planes: C must be 32 x a power of two, <= 512");
    const int Ho = mode != 1 ? H + 1 : H / 2;
    half_t* dy = dv.alloc<half_t>((size_t)B * Ho * Ho * C);
    if (mode != 1) launch_blur_pad2(dx, B, H, H, C, dy, 0, mode == 2);
    else launch_blur_down(dx, B, H, H, C, dy, 0);
    int rc = finish();
    if (rc) return rc;
    return down16(out, dy, (size_t)B * Ho * Ho * C);
}

extern "C" int glass_op_dblock_down(int32_t device, int32_t B, int32_t R, int32_t Cin, int32_t Cout, const float* h,
                                    const float* x, const float* w1, const float* wskip, const float* b1, float* y) {
    OPREQ(h && x && w1 && wskip && b1 && y, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    half_t* dh = dv.up16(h, (size_t)B * R * R * Cin);
    half_t* dx = dv.up16(x, (size_t)B * R * R * Cin);
    std::vector<_Float16> pk;
    glass_pack_conv(w1, Cout, Cin, 3, Cin, pk);
    half_t* dw1 = dv.up16v(pk);
    glass_pack_conv(wskip, Cout, Cin, 1, Cin, pk);
    half_t* dws = dv.up16v(pk);
    float* db = dv.up32(b1, Cout);
    const int Ro = R / 2;
    half_t* dxs = dv.alloc<half_t>((size_t)B * Ro * Ro * Cin);
    half_t* dy = dv.alloc<half_t>((size_t)B * Ro * Ro * Cout);
    OPREQ(conv_down_supported(R, Cin, Cout), "conv_down: unsupported shape");
    launch_blur_down(dx, B, R, R, Cin, dxs, 0);          // the skip branch's FIR (pad 1) + ::2 (conv_stream<fromrgb> emits it in the engine)
    OPREQ(launch_conv_down(dh, dxs, dw1, dws, db, dy, B, R, Cin, Cout, 0) != nullptr, "conv_down: unsupported shape");
    int rc = finish();
    if (rc) return rc;
    return down16(y, dy, (size_t)B * Ro * Ro * Cout);
}

extern "C" int glass_op_dblock0(int32_t device, int32_t B, int32_t R, int32_t impl, const float* y, const float* frgb_w, const float* frgb_b,
                                const float* w0, const float* b0, const float* w1, const float* wskip, const float* b1, float* out) {
    OPREQ(y && frgb_w && frgb_b && w0 && b0 && w1 && wskip && b1 && out && B > 0 && R > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const int Cin = 32, Cout = 64, Ro = R / 2;
    float* dy = dv.up32(y, (size_t)B * 3 * R * R);
    float* dfw = dv.up32(frgb_w, Cin * 3); float* dfb = dv.up32(frgb_b, Cin);
    std::vector<_Float16> pk;
    glass_pack_conv(w0, Cin, Cin, 3, Cin, pk);
    half_t* dw0 = dv.up16v(pk);
    glass_pack_conv(w1, Cout, Cin, 3, Cin, pk);
    half_t* dw1 = dv.up16v(pk);
    glass_pack_conv(wskip, Cout, Cin, 1, Cin, pk);
    half_t* dws = dv.up16v(pk);
    float* db0 = dv.up32(b0, Cin); float* db1 = dv.up32(b1, Cout);
    half_t* dout = dv.alloc<half_t>((size_t)B * Ro * Ro * Cout);
    OPREQ(dy && dw0 && dw1 && dws && dout, "device allocation failed");
    if (impl == 0 || impl == 2) {          // conv_d0.hip: the whole block in one kernel (2: chunk-planar output)
        OPREQ(launch_dblock0(dy, dfw, dfb, dw0, db0, dw1, dws, db1, dout, B, R, Cin, Cout, 0, impl == 2) != nullptr, "dblock0: unsupported shape");
    } else {                  // the two-kernel form it replaces: conv_stream<fromrgb> (h + the skip input to HBM) + conv_down
        half_t* dh = dv.alloc<half_t>((size_t)B * R * R * Cin);
        half_t* dxs = dv.alloc<half_t>((size_t)B * Ro * Ro * Cin);
        OPREQ(dh && dxs, "device allocation failed");
        ConvParams p = conv_defaults();
        p.x = dh; p.x_bstride = (long long)R * R * Cin; p.B = B; p.H = p.W = R; p.Cin = Cin; p.Hc = p.Wc = R; p.KS = 3; p.pad = 1;
        p.w = dw0; p.Cout = p.Neff = Cin; p.Ho = p.Wo = R; p.bias = db0; p.act = 1; p.y = dh;
        p.rgb_y = dy; p.rgb_w = dfw; p.rgb_b = dfb; p.rgb_xs_out = dxs;
        const ConvKernel k = choose_conv_stream(p);
        OPREQ(k, "dblock0 (two-kernel form): conv_stream<fromrgb> does not take this shape");
        k.launch(p, 0);
        OPREQ(launch_conv_down(dh, dxs, dw1, dws, db1, dout, B, R, Cin, Cout, 0) != nullptr, "dblock0 (two-kernel form): conv_down does not take this shape");
    }
    int rc = finish();
    if (rc) return rc;
    return down16(out, dout, (size_t)B * Ro * Ro * Cout);
}

extern "C" int glass_op_fromrgb(int32_t device, int32_t B, int32_t R, int32_t Cout, const float* y, const float* w,
                                const float* bias, float* out) {
    OPREQ(y && w && bias && out && Cout % 8 == 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dy = dv.up32(y, (size_t)B * 3 * R * R); float* dw = dv.up32(w, Cout * 3); float* db = dv.up32(bias, Cout);
    half_t* dout = dv.alloc<half_t>((size_t)B * R * R * Cout);
    launch_fromrgb(dy, B, R, Cout, dw, db, dout, 0);
    int rc = finish();
    if (rc) return rc;
    return down16(out, dout, (size_t)B * R * R * Cout);
}

extern "C" int glass_op_mbstd(int32_t device, int32_t B, int32_t hw, int32_t C, int32_t Cpad, int32_t batch_size,
                              int32_t group, const float* x, float* out) {
    OPREQ(x && out && B % batch_size == 0 && batch_size % group == 0 && group <= 8, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    half_t* dx = dv.up16(x, (size_t)B * hw * C);
    half_t* dy = dv.alloc<half_t>((size_t)B * hw * Cpad);
    launch_mbstd(dx, B, hw, C, Cpad, batch_size, group, 1e-8f, dy, 0);
    int rc = finish();
    if (rc) return rc;
    return down16(out, dy, (size_t)B * hw * Cpad);
}

extern "C" int glass_op_resize(int32_t device, int32_t B, int32_t R, int32_t S, int32_t ps, const float* y, float* patches) {
    OPREQ(y && patches && S % ps == 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dy = dv.up32(y, (size_t)B * 3 * R * R);
    const size_t n = (size_t)B * 3 * S * S;
    half_t* dp = dv.alloc<half_t>(n);
    launch_resize_patches(dy, B, R, S, ps, 3 * ps * ps, dp, 0);
    int rc = finish();
    if (rc) return rc;
    return down16(patches, dp, n);
}

extern "C" int glass_op_preprocess(int32_t device, int32_t B, int32_t R, int32_t S, int32_t ps, int32_t resize_mode, int32_t normalize,
                                   const float* y, float* patches) {
    OPREQ(y && patches && B > 0 && R > 0 && ps > 0 && S > 0 && S % ps == 0, "bad argument");
    if (int rc = glass_clip_preprocess_supported(R, S, resize_mode, normalize)) return rc;
    ResizeTaps t;
    std::string why;
    if (resize_mode) OPREQ(build_resize_taps(R, S, resize_mode, t, why), why);
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dy = dv.up32(y, (size_t)B * 3 * R * R);
    const size_t n = (size_t)B * 3 * S * S;
    half_t* dp = dv.alloc<half_t>(n);
    OPREQ(dy && dp, "device allocation failed");
    if (resize_mode == 0 && normalize == 0) {
        launch_resize_patches(dy, B, R, S, ps, 3 * ps * ps, dp, 0);
    } else {
        ResizeTapsDev td;
        if (resize_mode) {
            float* dt = dv.up32(t.table.data(), t.table.size());
            OPREQ(dt, "device allocation failed");
            td.table = dt; td.n4 = (int)(t.table.size() / 4); td.ts = t.ts; td.lds_bytes = t.lds_bytes;
        }
        launch_preprocess_patches(dy, B, R, S, ps, 3 * ps * ps, resize_mode, normalize, td, dp, 0);
    }
    int rc = finish();
    if (rc) return rc;
    return down16(patches, dp, n);
}

extern "C" int glass_op_view_patches(int32_t device, int32_t B, int32_t R, int32_t S, int32_t ps, int32_t normalize, int32_t V, const int32_t* boxes,
                                     const float* y, float* patches) {
    OPREQ(y && patches && boxes && B > 0 && R > 0 && ps > 0 && S > 0 && S % ps == 0 && S <= 4096 && (normalize == 0 || normalize == 1), "bad argument");
    OPREQ(V >= 1 && V <= GLASS_MAX_CLIP_VIEWS, "views must be in [1, 16]");
    ViewBoxes vb = {};
    for (int i = 0; i < 4 * V; ++i) vb.box[i / 4][i % 4] = boxes[i];
    OPREQ(view_boxes_valid(vb, V, R), "a box (x0, y0, s, flip) leaves the image or has flip outside {0, 1}");
    OPREQ((long long)B * V * ((S * S + 255) / 256) < (1LL << 31), "too many images");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dy = dv.up32(y, (size_t)B * 3 * R * R);
    const size_t n = (size_t)B * V * 3 * S * S;
    half_t* dp = dv.alloc<half_t>(n);
    OPREQ(dy && dp, "device allocation failed");
    launch_view_patches(dy, B, R, S, ps, 3 * ps * ps, normalize, V, vb, dp, 0);
    int rc = finish();
    if (rc) return rc;
    return down16(patches, dp, n);
}

extern "C" int glass_op_layernorm(int32_t device, int32_t M, int32_t D, const float* x, const float* g, const float* b, float* out) {
    OPREQ(x && g && b && out, "null argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dx = dv.up32(x, (size_t)M * D); float* dg = dv.up32(g, D); float* db = dv.up32(b, D);
    float* dout = dv.alloc<float>((size_t)M * D);
    launch_layernorm(dx, D, M, D, dg, db, nullptr, dout, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, dout, (size_t)M * D * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_attention(int32_t device, int32_t n_img, int32_t L, int32_t heads, int32_t causal,
                                  const float* qkv, float* out) {
    OPREQ(qkv && out && n_img > 0 && heads > 0 && L >= 1 && L <= 4096, "bad argument (1 <= L <= 4096)");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const int D = heads * 64;
    half_t* dq = dv.up16(qkv, (size_t)n_img * L * 3 * D);
    half_t* dout = dv.alloc<half_t>((size_t)n_img * L * D);
    launch_attention(dq, n_img, L, heads, 64, causal, dout, 0);
    int rc = finish();
    if (rc) return rc;
    return down16(out, dout, (size_t)n_img * L * D);
}

extern "C" int glass_op_noise(int32_t device, int32_t n_mb, int32_t hw, uint32_t layer, uint32_t mb0,
                              uint32_t generation, uint64_t seed, float* out) {
    OPREQ(out, "null argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* d = dv.alloc<float>((size_t)n_mb * hw);
    launch_noise(d, n_mb, hw, layer, mb0, generation, seed, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, d, (size_t)n_mb * hw * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_gpt2_sample(int32_t device, int32_t rows, int32_t V, const float* logits, float temperature, int32_t top_k,
                                    uint64_t seed, int32_t generation, int32_t first_row, int32_t step, int32_t purpose, int32_t* out) {
    OPREQ(logits && out && rows > 0 && V > 0, "bad argument");
    OPREQ(temperature > 0.f && temperature < INFINITY, "temperature must be a finite value > 0");
    OPREQ(top_k >= 0 && top_k <= GPT2_SAMPLE_TOPK_MAX, "top_k must lie in [0, 256]");
    OPREQ(gpt2_sample_supported(V), "vocabulary too large for the sampler (> 131072)");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* d = dv.up32(logits, (size_t)rows * V);
    int* sp = dv.alloc<int>(GPT2_SP_WORDS);
    int* o = dv.alloc<int>(rows);
    OPREQ(d && sp && o, "hipMalloc failed");
    int32_t h[GPT2_SP_WORDS];
    h[GPT2_SP_SEED_LO] = (int32_t)(uint32_t)(seed & 0xFFFFFFFFu);
    h[GPT2_SP_SEED_HI] = (int32_t)(uint32_t)(seed >> 32);
    h[GPT2_SP_GEN] = generation;
    h[GPT2_SP_ROW0] = first_row;
    h[GPT2_SP_PURPOSE] = purpose;
    memcpy(&h[GPT2_SP_TEMP], &temperature, sizeof(float));
    h[GPT2_SP_TOPK] = top_k;
    h[GPT2_SP_STEP] = step;
    GLASS_HIP(hipMemcpy(sp, h, sizeof h, hipMemcpyHostToDevice));
    launch_gpt2_sample(d, rows, V, sp, o, nullptr, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, o, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

// ---- GPT-2 trunk kernels (gpt2.hip), launched exactly as the passes of gpt2_host.cpp launch them ---------------------------------
extern "C" int glass_op_gpt2_gemm(int32_t device, int32_t form, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t mode, int32_t width,
                                  const float* a, const float* w, const float* bias, const float* lng, const float* lnb, const float* pst_in,
                                  int32_t np_in, float* out, float* stats_out, float* pst_out, int32_t* splits) {
    OPREQ(a && w && out && splits, "null argument");
    OPREQ(form >= 0 && form <= 3 && mode >= 0 && mode <= 2, "form must lie in [0, 3], mode in [0, 2]");
    OPREQ(M > 0 && N > 0 && K > 0 && K % 4 == 0 && lda >= K && lda % 4 == 0 && width > 0, "bad shape (K, lda multiples of 4, lda >= K)");
    OPREQ((lng == nullptr) == (lnb == nullptr), "LayerNorm gain and bias come together");
    OPREQ(!lng || form >= 2, "LayerNorm is fused on the operand of forms 2 and 3 only");
    OPREQ(!lng || mode != 2, "the residual products have no fused LayerNorm");
    const bool ln = lng != nullptr;
    if (form == 2) {
        OPREQ(gemm_f32_step_supported(M, K, lda, ln), "launch_gemm_f32_step does not take this shape (M <= 64, K % 64 == 0, K <= 1024 with LayerNorm)");
        OPREQ(!ln || (lda == K && stats_out), "fused LayerNorm: gpt2_finalize_kernel makes the statistics of dense rows (lda == K), returned in stats_out");
        OPREQ(mode != 2 || (N <= 1024 && stats_out), "a residual product is finished by gpt2_finalize_kernel: N <= 1024, statistics returned in stats_out");
    }
    if (form == 3) {
        OPREQ(gemm_f32_rowblk_supported(M, N, K, lda, ln, pst_out != nullptr),
              "launch_gemm_f32_rowblk does not take this shape (M <= 64, N % 32 == 0, K % 768 == 0, K <= 1024 with LayerNorm, N <= 768 with statistics)");
        OPREQ(ln == (pst_in != nullptr), "fused LayerNorm consumes the row partials pst_in [M, np_in, 2]");
        OPREQ(!ln || (np_in >= 1 && np_in <= 24 && K % np_in == 0), "np_in must divide K and lie in [1, 24]");
    }
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t part_elems = (size_t)16 * M * 4 * width;                      // the engine's split-K scratch for a model of this width
    float* da = dv.up32(a, (size_t)M * lda); float* dw = dv.up32(w, (size_t)N * K); float* db = dv.up32(bias, N);
    float* dg = dv.up32(lng, K); float* dlb = dv.up32(lnb, K);
    // the output is followed by guard rows up to the kernels' 64-row granularity: a store of a clamped row (m >= M) lands there and is reported
    const size_t rows_alloc = (size_t)(M + 63) / 64 * 64, n_guard = (rows_alloc - M) * N;
    float* dout = dv.alloc<float>(rows_alloc * N);
    float* part = dv.alloc<float>(part_elems);
    float* dstats = dv.alloc<float>((size_t)M * 2);
    float* dpi = ln && form == 3 ? dv.up32(pst_in, (size_t)M * np_in * 2) : nullptr;
    float* dpo = pst_out ? dv.alloc<float>((size_t)M * (N / 32 + 1) * 2) : nullptr;
    OPREQ(da && dw && dout && part && dstats && (!bias || db) && (!ln || (dg && dlb)) && (!pst_out || dpo), "hipMalloc failed");
    GLASS_HIP(hipMemset(dout, 0xff, rows_alloc * N * sizeof(float)));      // NaN: an element nobody stores shows
    if (mode == 2) GLASS_HIP(hipMemcpy(dout, out, (size_t)M * N * sizeof(float), hipMemcpyHostToDevice));
    int S = 1;
    if (form == 0 || form == 1) {
        launch_gemm_f32(da, dw, db, dout, M, N, K, lda, N, mode, 0, part, part_elems, form == 0);
    } else if (form == 2) {
        if (ln) launch_gpt2_finalize(nullptr, 0, nullptr, da, M, K, dstats, 0);
        const StepGemm c = choose_gemm_f32_step(M, N, K, lda, ln, part_elems, glass_cu_count());
        OPREQ(c, "choose_gemm_f32_step refused the shape");
        launch_gemm_f32_step({da, dw, db, dout, N, mode, part, ln ? dstats : nullptr, dg, dlb}, c, 0);
        S = c.S;
        if (mode == 2) launch_gpt2_finalize(S > 1 ? part : nullptr, S, db, dout, M, N, dstats, 0);
        else if (S > 1) launch_gpt2_reduce(part, S, db, dout, M, N, N, mode, 0);
    } else {
        const StepGemm c = choose_gemm_f32_rowblk(M, N, K, lda, ln, np_in, dpo != nullptr);
        OPREQ(c, "choose_gemm_f32_rowblk refused the shape");
        launch_gemm_f32_rowblk({da, dw, db, dout, N, mode, nullptr, dpi, dg, dlb, dpo}, c, 0);
    }
    int rc = finish();
    if (rc) return rc;
    *splits = S;
    GLASS_HIP(hipMemcpy(out, dout, (size_t)M * N * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<uint32_t> guard(n_guard);
    GLASS_HIP(hipMemcpy(guard.data(), dout + (size_t)M * N, n_guard * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n_guard; ++i)
        if (guard[i] != 0xffffffffu) {
            glass_set_error("gpt2_gemm: the product stored to row " + std::to_string(M + i / N) + " >= M");
            return GLASS_ERR_STATE;
        }
    if (stats_out && form == 2 && (ln || mode == 2)) GLASS_HIP(hipMemcpy(stats_out, dstats, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToHost));
    if (pst_out && form == 3) GLASS_HIP(hipMemcpy(pst_out, dpo, (size_t)M * (N / 32) * 2 * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_gpt2_attention(int32_t device, int32_t form, int32_t P, int32_t nd, int32_t past, int32_t Tmax, int32_t heads, int32_t S,
                                       const float* qkv, const float* bias, float* kc, float* vc, float* out) {
    OPREQ(qkv && kc && vc && out, "null argument");
    OPREQ(form >= 0 && form <= 2, "form must lie in [0, 2]");
    OPREQ(P > 0 && heads > 0 && nd > 0 && past >= 0 && past + nd <= Tmax, "bad shape (past + nd <= Tmax)");
    const int D = heads * 64;
    if (form == 2) {
        OPREQ(nd == 1 && Tmax <= 64, "gpt2_attention_step_kernel: one new position, Tmax <= 64");
        OPREQ(S >= 0 && S <= 16, "S must lie in [0, 16] (0: finished qkv values)");
    } else {
        OPREQ(S == 0 && !bias, "the general kernel takes finished qkv values");
        const int ns = form == 1 ? Tmax : past + nd;      // launch_gpt2_attention's own size
        OPREQ(gpt2_attention_lds_bytes(nd, ns) <= GPT2_ATTENTION_LDS_MAX,
              "gpt2_attention_kernel: nd * 65 + 2 * ns * 65 + nd * (ns + 1) floats exceed 160 KB of LDS");
    }
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t nq = (size_t)(form == 2 && S > 0 ? S : 1) * P * nd * 3 * D, nc = (size_t)P * Tmax * D, no = (size_t)P * nd * D;
    float* dq = dv.up32(qkv, nq); float* db = dv.up32(bias, 3 * D);
    float* dk = dv.up32(kc, nc); float* dvc = dv.up32(vc, nc);
    float* dout = dv.alloc<float>(no);
    int* dpast = dv.alloc<int>(3);
    OPREQ(dq && dk && dvc && dout && dpast && (!bias || db), "hipMalloc failed");
    const int state[3] = {past, 1, 0};
    GLASS_HIP(hipMemcpy(dpast, state, sizeof state, hipMemcpyHostToDevice));
    GLASS_HIP(hipMemset(dout, 0xff, no * sizeof(float)));
    if (form == 2) launch_gpt2_attention_step(dq, S > 0 ? dq : nullptr, S > 0 ? S : 1, db, dk, dvc, P, Tmax, heads, dout, 0, dpast);
    else launch_gpt2_attention(dq, dk, dvc, P, nd, form == 1 ? 0 : past, Tmax, heads, dout, 0, form == 1 ? dpast : nullptr);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, dout, no * sizeof(float), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(kc, dk, nc * sizeof(float), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(vc, dvc, nc * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_gpt2_head(int32_t device, int32_t M, int32_t V, int32_t K, int32_t tail, const float* x, const float* wte, const float* lng,
                                  const float* lnb, const float* wpe, int32_t npos, int32_t past, int32_t step, float* logits, float* pair_val,
                                  int32_t* pair_idx, int32_t* token, float* stats, float* x_next, float* stats_next, int32_t* state) {
    OPREQ(x && wte && lng && lnb && token && stats, "null argument");
    OPREQ(M > 0 && K > 0 && K <= 1024 && gpt2_head_supported(M, V, K, K), "gpt2_head_kernel: M <= 64, K % 64 == 0, K <= 1024, V >= 4096");
    if (tail) OPREQ(wpe && x_next && stats_next && state && past >= 0 && past + 1 < npos && step >= 0, "tail: wpe [npos, K], past + 1 < npos, step >= 0");
    else OPREQ(logits && pair_val && pair_idx, "null argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const int NB = (V + 31) / 32;
    float* dx = dv.up32(x, (size_t)M * K); float* dw = dv.up32(wte, (size_t)V * K); float* dg = dv.up32(lng, K); float* db = dv.up32(lnb, K);
    float* dstats = dv.alloc<float>((size_t)M * 2);
    float* pairs = dv.alloc<float>((size_t)2 * M * NB);
    OPREQ(dx && dw && dg && db && dstats && pairs, "hipMalloc failed");
    launch_gpt2_finalize(nullptr, 0, nullptr, dx, M, K, dstats, 0);            // the statistics the last layer's finalize leaves
    if (!tail) {
        float* dl = dv.alloc<float>((size_t)M * V);
        int* dtok = dv.alloc<int>(M);
        OPREQ(dl && dtok, "hipMalloc failed");
        GLASS_HIP(hipMemset(dl, 0xff, (size_t)M * V * sizeof(float)));
        GLASS_HIP(hipMemset(pairs, 0xff, (size_t)2 * M * NB * sizeof(float)));
        const Gpt2Head h = choose_gpt2_head(M, V, K, K, GPT2_PICK_ARGMAX, true);
        OPREQ(h, "choose_gpt2_head refused the shape");
        launch_gpt2_head({dx, dw, dstats, dg, db, dl, pairs, nullptr, dtok, nullptr}, h, 0);
        int rc = finish();
        if (rc) return rc;
        GLASS_HIP(hipMemcpy(stats, dstats, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToHost));
        GLASS_HIP(hipMemcpy(logits, dl, (size_t)M * V * sizeof(float), hipMemcpyDeviceToHost));
        GLASS_HIP(hipMemcpy(pair_val, pairs, (size_t)M * NB * sizeof(float), hipMemcpyDeviceToHost));
        GLASS_HIP(hipMemcpy(pair_idx, pairs + (size_t)M * NB, (size_t)M * NB * sizeof(int), hipMemcpyDeviceToHost));
        GLASS_HIP(hipMemcpy(token, dtok, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
        return GLASS_OK;
    }
    float* dpe = dv.up32(wpe, (size_t)npos * K);
    int* dgen = dv.alloc<int>((size_t)(step + 1) * M);
    int* dstate = dv.alloc<int>(3);
    OPREQ(dpe && dgen && dstate, "hipMalloc failed");
    const int st0[3] = {past, step, 0};
    GLASS_HIP(hipMemcpy(dstate, st0, sizeof st0, hipMemcpyHostToDevice));
    GLASS_HIP(hipMemcpy(stats, dstats, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToHost));
    // as the engine: the residual stream and its statistics are the head's operands AND the buffers the tail leaves the next step's in
    const Gpt2Head h = choose_gpt2_head(M, V, K, K, GPT2_PICK_ARGMAX_TAIL, false);
    OPREQ(h, "choose_gpt2_head refused the shape");
    launch_gpt2_head({dx, dw, dstats, dg, db, nullptr, pairs, nullptr, dgen, dstate, dw, dpe, dx, dstats}, h, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(token, dgen + (size_t)step * M, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(x_next, dx, (size_t)M * K * sizeof(float), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(stats_next, dstats, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(state, dstate, 3 * sizeof(int), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_gpt2_embed_step(int32_t device, int32_t M, int32_t V, int32_t K, const int32_t* token, const float* wte, const float* wpe,
                                        int32_t npos, int32_t past, int32_t step, float* x, float* stats) {
    OPREQ(token && wte && wpe && x && stats, "null argument");
    OPREQ(M > 0 && V > 0 && K > 0 && K <= 1024 && past >= 0 && past < npos && step >= 1, "bad argument (K <= 1024 with statistics, past < npos, step >= 1)");
    for (int i = 0; i < M; ++i) OPREQ(token[i] >= 0 && token[i] < V, "token id out of range");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dw = dv.up32(wte, (size_t)V * K); float* dpe = dv.up32(wpe, (size_t)npos * K);
    float* dx = dv.alloc<float>((size_t)M * K); float* ds = dv.alloc<float>((size_t)M * 2);
    int* dgen = dv.alloc<int>((size_t)step * M);
    int* dstate = dv.alloc<int>(3);
    OPREQ(dw && dpe && dx && ds && dgen && dstate, "hipMalloc failed");
    const int st0[3] = {past, step, 0};
    GLASS_HIP(hipMemcpy(dstate, st0, sizeof st0, hipMemcpyHostToDevice));
    GLASS_HIP(hipMemcpy(dgen + (size_t)(step - 1) * M, token, (size_t)M * sizeof(int), hipMemcpyHostToDevice));
    launch_gpt2_embed_step(dgen, dstate, M, dw, dpe, K, dx, 0, ds);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(x, dx, (size_t)M * K * sizeof(float), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(stats, ds, (size_t)M * 2 * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

// ---- BigGAN-deep glue kernels (biggan_kernels.hip) and the fused last stage (bg_tail.hip), launched as biggan.cpp launches them ------------
extern "C" int glass_op_bg_cond(int32_t device, int32_t P, int32_t L, int32_t zd, int32_t nc, const float* x, const float* et, float* cond) {
    OPREQ(x && et && cond && P > 0 && zd > 0 && nc > 0 && L >= zd + nc, "bad argument (rows are [z (zd) | class bits (nc)], L >= zd + nc)");
    OPREQ((size_t)(nc + 8) * sizeof(float) <= 64 * 1024, "bg_cond_kernel keeps the class probabilities in LDS: nc + 8 floats <= 64 KB");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dx = dv.up32(x, (size_t)P * L); float* de = dv.up32(et, (size_t)nc * zd);
    float* dc = dv.alloc<float>((size_t)P * 2 * zd);
    OPREQ(dx && de && dc, "device allocation failed");
    GLASS_HIP(hipMemset(dc, 0xFF, (size_t)P * 2 * zd * sizeof(float)));
    launch_bg_cond(dx, P, L, zd, nc, de, dc, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(cond, dc, (size_t)P * 2 * zd * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_bg_bn_tables(int32_t device, int32_t P, int32_t cd, int32_t C, const float* cond, const float* wt, const float* bias,
                                     const float* inv_std, const float* mean, const float* prebias, float* tab, float* tab16) {
    OPREQ(cond && wt && bias && inv_std && mean && prebias && tab && tab16 && P > 0 && cd > 0 && C > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t n = (size_t)P * 2 * C;
    float* dc = dv.up32(cond, (size_t)P * cd); float* dw = dv.up32(wt, (size_t)cd * 2 * C); float* db = dv.up32(bias, 2 * (size_t)C);
    float* di = dv.up32(inv_std, C); float* dm = dv.up32(mean, C); float* dp = dv.up32(prebias, C);
    float* dt = dv.alloc<float>(n);
    half_t* dt16 = dv.alloc<half_t>(n);
    OPREQ(dc && dw && db && di && dm && dp && dt && dt16, "device allocation failed");
    GLASS_HIP(hipMemset(dt16, 0xFF, n * sizeof(half_t)));
    // glass_biggan_prepare's three launches
    launch_dense(dc, cd, P, cd, dw, 2 * C, db, dt, 2 * C, 0, 0, nullptr, 0, 0);
    launch_bg_bn_tables(dt, P, C, di, dm, dp, 0);
    launch_bg_to_half(dt, dt16, (long long)n, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(tab, dt, n * sizeof(float), hipMemcpyDeviceToHost));
    return down16(tab16, dt16, n);
}

extern "C" int glass_op_bg_attn_split(int32_t device, int32_t B, int32_t H, int32_t W, int32_t c8, int32_t c2, const float* T, float* theta,
                                      float* phi, float* gT, int32_t* vec) {
    OPREQ(T && theta && phi && gT && vec && B > 0 && c8 > 0 && c2 > 0, "bad argument");
    OPREQ(H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "bg_attn_split: H and W must be even (2x2 max-pool)");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t hw = (size_t)H * W, hq = hw / 4, CT = 2 * (size_t)c8 + c2;
    half_t* dT = dv.up16(T, (size_t)B * hw * CT);
    half_t* dth = dv.alloc<half_t>((size_t)B * hw * c8);
    half_t* dph = dv.alloc<half_t>((size_t)B * hq * c8);
    half_t* dg = dv.alloc<half_t>((size_t)B * hq * c2);
    OPREQ(dT && dth && dph && dg, "device allocation failed");
    GLASS_HIP(hipMemset(dth, 0xFF, (size_t)B * hw * c8 * sizeof(half_t)));      // NaN: an element nobody stores shows
    GLASS_HIP(hipMemset(dph, 0xFF, (size_t)B * hq * c8 * sizeof(half_t)));
    GLASS_HIP(hipMemset(dg, 0xFF, (size_t)B * hq * c2 * sizeof(half_t)));
    const char* k = launch_bg_attn_split(dT, B, H, W, c8, c2, dth, dph, dg, 0);
    *vec = strcmp(k, "bg_attn_split_vec_kernel") == 0;
    int rc = finish();
    if (rc) return rc;
    if ((rc = down16(theta, dth, (size_t)B * hw * c8))) return rc;
    if ((rc = down16(phi, dph, (size_t)B * hq * c8))) return rc;
    return down16(gT, dg, (size_t)B * hq * c2);
}

extern "C" int glass_op_bg_softmax(int32_t device, int32_t rows, int32_t n, const float* S, float* out) {
    OPREQ(S && out && rows > 0 && n > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t tot = (size_t)rows * n;
    float* ds = dv.up32(S, tot);
    half_t* dp = dv.alloc<half_t>(tot);
    OPREQ(ds && dp, "device allocation failed");
    GLASS_HIP(hipMemset(dp, 0xFF, tot * sizeof(half_t)));
    launch_bg_softmax(ds, rows, n, dp, 0);
    int rc = finish();
    if (rc) return rc;
    return down16(out, dp, tot);
}

extern "C" int glass_op_bg_rgb_tanh(int32_t device, int32_t B, int32_t hw, int32_t C, const float* x, float* y) {
    OPREQ(x && y && B > 0 && hw > 0 && C >= 3, "bad argument (C >= 3)");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    half_t* dx = dv.up16(x, (size_t)B * hw * C);
    float* dy = dv.alloc<float>((size_t)B * 3 * hw);
    OPREQ(dx && dy, "device allocation failed");
    GLASS_HIP(hipMemset(dy, 0xFF, (size_t)B * 3 * hw * sizeof(float)));
    launch_bg_rgb_tanh(dx, B, hw, C, dy, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(y, dy, (size_t)B * 3 * hw * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_bg_to_half(int32_t device, int64_t n, const float* x, float* out) {
    OPREQ(x && out && n > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dx = dv.up32(x, (size_t)n);
    half_t* dy = dv.alloc<half_t>((size_t)n + 4);      // four guard elements behind the output
    OPREQ(dx && dy, "device allocation failed");
    GLASS_HIP(hipMemset(dy, 0xFF, ((size_t)n + 4) * sizeof(half_t)));
    launch_bg_to_half(dx, dy, n, 0);
    int rc = finish();
    if (rc) return rc;
    uint16_t guard[4];
    GLASS_HIP(hipMemcpy(guard, dy + n, sizeof guard, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) OPREQ(guard[i] == 0xFFFFu, "bg_to_half stored past element n");
    return down16(out, dy, (size_t)n);
}

extern "C" int glass_op_bg_tail(int32_t device, int32_t B, int32_t R, int32_t mid, const float* h, const float* x0, const float* w3, const float* b3,
                                const float* bn_a, const float* bn_s, const float* rgb_w, const float* rgb_b, float* y) {
    OPREQ(h && x0 && w3 && b3 && bn_a && bn_s && rgb_w && rgb_b && y && B > 0 && R > 0 && mid > 0, "bad argument");
    const int C = 128, cpad = 32;                           // the last block's width; BgState::rgb_cpad
    OPREQ(bg_tail_supported(R, mid, C, C, 1, cpad), "bg_tail: unsupported shape (R % 32 == 0, R >= 32, mid == 32, 128 -> 128 channels of an up block)");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const int R2 = R / 2;
    std::vector<_Float16> pk((size_t)9 * cpad * C, (_Float16)0.f);      // [tap][cpad][128], rows 0..2 used (biggan.cpp pack())
    for (int o = 0; o < 3; ++o)
        for (int i = 0; i < C; ++i)
            for (int t = 0; t < 9; ++t) pk[((size_t)t * cpad + o) * C + i] = (_Float16)rgb_w[((size_t)o * C + i) * 9 + t];
    std::vector<float> tab(2 * (size_t)C), rb(cpad, 0.f);
    for (int c = 0; c < C; ++c) { tab[c] = bn_a[c]; tab[C + c] = bn_s[c]; }
    for (int c = 0; c < 3; ++c) rb[c] = rgb_b[c];
    BgTailParams tp;
    memset(&tp, 0, sizeof tp);
    tp.h = dv.up16(h, (size_t)B * R * R * mid);
    tp.x0 = dv.up16(x0, (size_t)B * R2 * R2 * C);
    tp.w3 = dv.up16(w3, (size_t)C * mid);
    tp.b3 = dv.up32(b3, C);
    tp.tab = dv.up32(tab.data(), tab.size()); tp.bnf_off = 0; tp.ctot = C;
    tp.rgb_w = dv.up16v(pk); tp.cpad = cpad;
    tp.rgb_b = dv.up32(rb.data(), rb.size());
    const size_t ny = (size_t)B * 3 * R * R;
    float* dy = dv.alloc<float>(ny);
    tp.y = dy; tp.B = B; tp.R = R;
    OPREQ(tp.h && tp.x0 && tp.w3 && tp.b3 && tp.tab && tp.rgb_w && tp.rgb_b && dy, "device allocation failed");
    GLASS_HIP(hipMemset(dy, 0xFF, ny * sizeof(float)));      // NaN: a pixel no tile writes shows
    OPREQ(launch_bg_tail(tp, 0), "bg_tail: the launcher refused the shape");
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(y, dy, ny * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

// ---- the small fp32 kernels around StyleGAN2 and the CLIP towers, each launched as the engine's host code launches it ------------------------
// (tests/test_gpu_small_ops.py against the float64 restatements of tests/small_ops_ref.py).  Strided operands arrive with their padding
// as the caller filled it (NaN); outputs wider than what a kernel writes are uploaded first, so that what it leaves alone comes back unchanged.
extern "C" int glass_op_mapping(int32_t device, int32_t P, int32_t L, int32_t n_layers, const float* z, const float* wt, const float* b,
                                int32_t path, float* out, int32_t* ran) {
    OPREQ(z && wt && b && out && ran && P > 0 && L > 0 && n_layers >= 1 && n_layers <= 8, "bad argument (1 .. 8 layers)");
    OPREQ(path >= 0 && path <= 2, "path must lie in [0, 2]");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t n = (size_t)P * L;
    float* dz = dv.up32(z, n); float* w0 = dv.alloc<float>(n); float* w1 = dv.alloc<float>(n);
    OPREQ(dz && w0 && w1, "device allocation failed");
    std::vector<const float*> dw(n_layers), db(n_layers);
    for (int i = 0; i < n_layers; ++i) {
        dw[i] = dv.up32(wt + (size_t)i * L * L, (size_t)L * L);
        db[i] = dv.up32(b + (size_t)i * L, L);
        OPREQ(dw[i] && db[i], "device allocation failed");
    }
    GLASS_HIP(hipMemset(w0, 0xFF, n * sizeof(float)));      // NaN: an element nobody stores shows
    GLASS_HIP(hipMemset(w1, 0xFF, n * sizeof(float)));
    *ran = launch_mapping(dz, w0, w1, P, L, 1e-8f, dw.data(), db.data(), n_layers, path, 0);
    OPREQ(*ran != 0, "mapping_fused_kernel does not take this network (L = 256 / 512, its LDS within the device's limit)");
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, w0, n * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_pixelnorm(int32_t device, int32_t P, int32_t L, const float* z, float* out) {
    OPREQ(z && out && P > 0 && L > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t n = (size_t)P * L;
    float* dz = dv.up32(z, n); float* dout = dv.alloc<float>(n);
    OPREQ(dz && dout, "device allocation failed");
    GLASS_HIP(hipMemset(dout, 0xFF, n * sizeof(float)));
    launch_pixelnorm(dz, dout, P, L, 1e-8f, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, dout, n * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_dense_splitk(int32_t device, int32_t P, int32_t K, int32_t N, int32_t ldx, int32_t ldo, int32_t mode, const float* x,
                                     const float* wt, const float* bias, float* out) {
    OPREQ(x && wt && out && P > 0 && N > 0, "bad argument");
    OPREQ(K > 0 && K % 64 == 0 && K <= 768, "dense_splitk_kernel: K a multiple of 64, at most 768 (64 KB of LDS)");
    OPREQ(ldx >= K && ldo >= N && (mode == 0 || mode == 1), "ldx >= K, ldo >= N, mode 0 or 1");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dx = dv.up32(x, (size_t)P * ldx); float* dw = dv.up32(wt, (size_t)K * N); float* db = dv.up32(bias, N);
    float* dout = dv.up32(out, (size_t)P * ldo);
    OPREQ(dx && dw && dout && (!bias || db), "device allocation failed");
    launch_dense_splitk(dx, ldx, P, K, dw, N, db, dout, ldo, mode, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, dout, (size_t)P * ldo * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_dense_ex(int32_t device, int32_t P, int32_t K, int32_t N, int32_t ldx, int32_t ldo, const float* x, const float* wt,
                                 const float* bias, int32_t in_sq, int32_t mode, const float* eps_row, int32_t eps_stride, float* out) {
    OPREQ(x && wt && out && P > 0 && K > 0 && N > 0 && ldx >= K && ldo >= N, "bad argument (ldx >= K, ldo >= N)");
    OPREQ(mode >= 0 && mode <= 2 && (mode != 2 || (eps_row && eps_stride >= 1)), "mode 2 reads eps_row [P, eps_stride]");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dx = dv.up32(x, (size_t)P * ldx); float* dw = dv.up32(wt, (size_t)K * N); float* db = dv.up32(bias, N);
    float* de = dv.up32(eps_row, (size_t)P * eps_stride); float* dout = dv.up32(out, (size_t)P * ldo);
    OPREQ(dx && dw && dout && (!bias || db) && (!eps_row || de), "device allocation failed");
    launch_dense(dx, ldx, P, K, dw, N, db, dout, ldo, in_sq, mode, de, eps_stride, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, dout, (size_t)P * ldo * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_dense_multi(int32_t device, int32_t n, int32_t P, int32_t ldx, int32_t ldo, int32_t eps_stride, const int32_t* K,
                                    const int32_t* N, const int32_t* x_off, const int32_t* out_off, const int32_t* eps_idx, const float* x,
                                    const float* wt, const float* eps_rows, float* out) {
    OPREQ(K && N && x_off && out_off && eps_idx && x && wt && eps_rows && out && n > 0 && P > 0 && eps_stride > 0, "bad argument");
    size_t wtot = 0;
    int max_N = 0;
    for (int i = 0; i < n; ++i) {
        OPREQ(K[i] > 0 && N[i] > 0 && x_off[i] >= 0 && x_off[i] + K[i] <= ldx && out_off[i] >= 0 && out_off[i] + N[i] <= ldo &&
                  eps_idx[i] >= 0 && eps_idx[i] < eps_stride, "a problem leaves its table");
        wtot += (size_t)K[i] * N[i];
        max_N = std::max(max_N, N[i]);
    }
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dx = dv.up32(x, (size_t)P * ldx); float* dw = dv.up32(wt, wtot); float* de = dv.up32(eps_rows, (size_t)P * eps_stride);
    float* dout = dv.up32(out, (size_t)P * ldo);
    OPREQ(dx && dw && de && dout, "device allocation failed");
    std::vector<DenseDesc> dd(n);       // as finalize builds the demodulation table (engine.cpp)
    size_t woff = 0;
    for (int i = 0; i < n; ++i) {
        DenseDesc& q = dd[i];
        q.x = dx + x_off[i]; q.ldx = ldx; q.K = K[i]; q.wt = dw + woff; q.N = N[i]; q.bias = nullptr;
        q.out = dout + out_off[i]; q.ldo = ldo; q.eps_row = de + eps_idx[i]; q.eps_stride = eps_stride;
        woff += (size_t)K[i] * N[i];
    }
    DenseDesc* ddev = dv.alloc<DenseDesc>(n);
    OPREQ(ddev, "device allocation failed");
    GLASS_HIP(hipMemcpy(ddev, dd.data(), (size_t)n * sizeof(DenseDesc), hipMemcpyHostToDevice));
    launch_dense_multi(ddev, n, max_N, P, 1, 2, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, dout, (size_t)P * ldo * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_style_norm(int32_t device, int32_t P, int32_t ld, int32_t n_layers, const int32_t* off, const int32_t* len, float* s,
                                   float* smax, float* eps_row) {
    OPREQ(off && len && s && smax && eps_row && P > 0 && n_layers > 0, "bad argument");
    for (int l = 0; l < n_layers; ++l) OPREQ(off[l] >= 0 && len[l] > 0 && off[l] + len[l] <= ld, "a segment leaves the row");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t n = (size_t)P * ld, m = (size_t)P * n_layers;
    float* ds = dv.up32(s, n); float* dm = dv.alloc<float>(m); float* de = dv.alloc<float>(m);
    int* doff = dv.alloc<int>(n_layers); int* dlen = dv.alloc<int>(n_layers);
    OPREQ(ds && dm && de && doff && dlen, "device allocation failed");
    GLASS_HIP(hipMemcpy(doff, off, n_layers * sizeof(int), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemcpy(dlen, len, n_layers * sizeof(int), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemset(dm, 0xFF, m * sizeof(float)));
    GLASS_HIP(hipMemset(de, 0xFF, m * sizeof(float)));
    launch_style_norm(ds, ld, P, n_layers, doff, dlen, dm, de, 1e-8f, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(s, ds, n * sizeof(float), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(smax, dm, m * sizeof(float), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(eps_row, de, m * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_d_head(int32_t device, int32_t P, int32_t CL, const float* dfin, const float* w0, const float* b0, const float* w1,
                               const float* b1, float* dis, int32_t* split) {
    OPREQ(dfin && w0 && b0 && w1 && b1 && dis && split && P > 0 && CL > 0 && CL % 4 == 0, "bad argument (CL a multiple of 4)");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t K = 16 * (size_t)CL;
    DHead h;
    h.dfin = dv.up16(dfin, (size_t)P * K); h.w0 = dv.up16(w0, (size_t)CL * K);
    h.b0 = dv.up32(b0, CL); h.w1t = dv.up32(w1, CL); h.b1 = dv.up32(b1, 1);
    h.part = dv.alloc<float>((size_t)16 * P * CL); h.dh = dv.alloc<float>((size_t)P * CL); h.dis = dv.alloc<float>(P);
    h.P = P; h.CL = CL;
    OPREQ(h.dfin && h.w0 && h.b0 && h.w1t && h.b1 && h.part && h.dh && h.dis, "device allocation failed");
    GLASS_HIP(hipMemset(h.part, 0xFF, (size_t)16 * P * CL * sizeof(float)));      // NaN: a slice element nobody stores shows in the sum
    GLASS_HIP(hipMemset(h.dh, 0xFF, (size_t)P * CL * sizeof(float)));
    GLASS_HIP(hipMemset(h.dis, 0xFF, (size_t)P * sizeof(float)));
    *split = launch_d_head_split(h, 0) != nullptr;
    if (!*split) {                        // as run_d_head: the whole product (run_gemm's order: gemm_tiled, then gemm_direct), then the second layer
        const GemmParams g = d_head_dense0(h);
        if (!launch_gemm_tiled(g, 0)) launch_gemm_direct(g, 0);
        launch_d_head_dense1(h, 0);
    }
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(dis, h.dis, (size_t)P * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_finalize_image(int32_t device, int64_t n, const float* y, float* img) {
    OPREQ(y && img && n > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dy = dv.up32(y, (size_t)n); float* di = dv.alloc<float>((size_t)n + 4);      // four guard elements behind the output
    OPREQ(dy && di, "device allocation failed");
    GLASS_HIP(hipMemset(di, 0xFF, ((size_t)n + 4) * sizeof(float)));
    launch_finalize_image(dy, di, n, 0);
    int rc = finish();
    if (rc) return rc;
    uint32_t guard[4];
    GLASS_HIP(hipMemcpy(guard, di + n, sizeof guard, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) OPREQ(guard[i] == 0xFFFFFFFFu, "finalize_image stored past element n");
    GLASS_HIP(hipMemcpy(img, di, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_embed_lnpre(int32_t device, int32_t P, int32_t T, int32_t D, const float* patch_emb, const float* cls, const float* pos,
                                    const float* g, const float* b, float* x) {
    OPREQ(patch_emb && cls && pos && g && b && x && P > 0 && T >= 2 && D > 0, "bad argument (T = 1 + patches >= 2)");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t n = (size_t)P * T * D;
    float* dpe = dv.up32(patch_emb, (size_t)P * (T - 1) * D); float* dc = dv.up32(cls, D); float* dp = dv.up32(pos, (size_t)T * D);
    float* dg = dv.up32(g, D); float* db = dv.up32(b, D); float* dx = dv.alloc<float>(n);
    OPREQ(dpe && dc && dp && dg && db && dx, "device allocation failed");
    GLASS_HIP(hipMemset(dx, 0xFF, n * sizeof(float)));
    launch_embed_lnpre(dpe, dc, dp, dg, db, P, T, D, dx, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(x, dx, n * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_embed_text(int32_t device, int32_t n_texts, int32_t ctx, int32_t D, int32_t V, const int32_t* tokens, const float* tok_emb,
                                   const float* pos, float* x) {
    OPREQ(tokens && tok_emb && pos && x && n_texts > 0 && ctx > 0 && D > 0 && V > 0, "bad argument");
    const int rows = n_texts * ctx;
    for (int i = 0; i < rows; ++i) OPREQ(tokens[i] >= 0 && tokens[i] < V, "token id out of range");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t n = (size_t)rows * D;
    int* dt = dv.alloc<int>(rows);
    float* de = dv.up32(tok_emb, (size_t)V * D); float* dp = dv.up32(pos, (size_t)ctx * D); float* dx = dv.alloc<float>(n);
    OPREQ(dt && de && dp && dx, "device allocation failed");
    GLASS_HIP(hipMemcpy(dt, tokens, rows * sizeof(int), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemset(dx, 0xFF, n * sizeof(float)));
    launch_embed_text(dt, de, dp, rows, ctx, D, dx, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(x, dx, n * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_layernorm_ex(int32_t device, int32_t M, int32_t D, int64_t row_stride, int32_t half_out, const float* x, const float* g,
                                     const float* b, float* out) {
    OPREQ(x && g && b && out && M > 0 && D > 0 && row_stride >= D, "bad argument (row_stride >= D)");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t n = (size_t)M * D;
    float* dx = dv.up32(x, (size_t)(M - 1) * row_stride + D); float* dg = dv.up32(g, D); float* db = dv.up32(b, D);
    float* o32 = half_out ? nullptr : dv.alloc<float>(n);
    half_t* o16 = half_out ? dv.alloc<half_t>(n) : nullptr;
    OPREQ(dx && dg && db && (o32 || o16), "device allocation failed");
    GLASS_HIP(hipMemset(half_out ? (void*)o16 : (void*)o32, 0xFF, n * (half_out ? sizeof(half_t) : sizeof(float))));
    launch_layernorm(dx, row_stride, M, D, dg, db, o16, o32, 0);
    int rc = finish();
    if (rc) return rc;
    if (o16) return down16(out, o16, n);
    GLASS_HIP(hipMemcpy(out, o32, n * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_layernorm_rows(int32_t device, int32_t n_rows, int32_t M, int32_t D, const float* x, const int32_t* rows, const float* g,
                                       const float* b, float* out) {
    OPREQ(x && rows && g && b && out && n_rows > 0 && M > 0 && D > 0, "bad argument");
    for (int i = 0; i < M; ++i) OPREQ(rows[i] >= 0 && rows[i] < n_rows, "row index out of range");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t n = (size_t)M * D;
    float* dx = dv.up32(x, (size_t)n_rows * D); float* dg = dv.up32(g, D); float* db = dv.up32(b, D); float* dout = dv.alloc<float>(n);
    int* dr = dv.alloc<int>(M);
    OPREQ(dx && dg && db && dout && dr, "device allocation failed");
    GLASS_HIP(hipMemcpy(dr, rows, M * sizeof(int), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemset(dout, 0xFF, n * sizeof(float)));
    launch_layernorm_rows(dx, dr, M, D, dg, db, dout, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, dout, n * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_cosine(int32_t device, int32_t P, int32_t D, const float* feat, const float* target, float* sim) {
    OPREQ(feat && target && sim && P > 0 && D > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* df = dv.up32(feat, (size_t)P * D); float* dt = dv.up32(target, D); float* ds = dv.alloc<float>(P);
    OPREQ(df && dt && ds, "device allocation failed");
    GLASS_HIP(hipMemset(ds, 0xFF, (size_t)P * sizeof(float)));
    launch_cosine(df, dt, P, D, ds, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(sim, ds, (size_t)P * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_cosine_views(int32_t device, int32_t P, int32_t V, int32_t D, const float* feat, const float* target, float* view_sim,
                                     float* sim) {
    OPREQ(feat && target && view_sim && sim && P > 0 && V > 0 && D > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* df = dv.up32(feat, (size_t)P * V * D); float* dt = dv.up32(target, D);
    float* dvs = dv.alloc<float>((size_t)P * V); float* ds = dv.alloc<float>(P);
    OPREQ(df && dt && dvs && ds, "device allocation failed");
    GLASS_HIP(hipMemset(dvs, 0xFF, (size_t)P * V * sizeof(float)));
    GLASS_HIP(hipMemset(ds, 0xFF, (size_t)P * sizeof(float)));
    launch_cosine_views(df, dt, P, V, D, dvs, ds, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(view_sim, dvs, (size_t)P * V * sizeof(float), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(sim, ds, (size_t)P * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_assemble_F(int32_t device, int32_t P, int32_t n_obj, const float* sim, const float* dis, float* F) {
    OPREQ(sim && F && P > 0 && (n_obj == 1 || (n_obj == 2 && dis)), "bad argument (n_obj 1, or 2 with dis)");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t n = (size_t)P * n_obj;
    float* ds = dv.up32(sim, P); float* dd = dv.up32(dis, P); float* dF = dv.alloc<float>(n + 4);      // four guard elements behind the output
    OPREQ(ds && dF && (!dis || dd), "device allocation failed");
    GLASS_HIP(hipMemset(dF, 0xFF, (n + 4) * sizeof(float)));
    launch_assemble_F(ds, dd, P, n_obj, dF, 0);
    int rc = finish();
    if (rc) return rc;
    uint32_t guard[4];
    GLASS_HIP(hipMemcpy(guard, dF + n, sizeof guard, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) OPREQ(guard[i] == 0xFFFFFFFFu, "assemble_F stored past row P");
    GLASS_HIP(hipMemcpy(F, dF, n * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_cosine_set(int32_t device, int32_t P, int32_t V, int32_t T, int32_t D, const float* feat, const float* targets,
                                   const float* weights, float* view_sim, float* set_sim, float* sim) {
    OPREQ(feat && targets && weights && view_sim && set_sim && sim && P > 0 && D > 0, "bad argument");
    OPREQ(V >= 1 && V <= GLASS_PROMPT_MAX_VIEWS && T >= 1 && T <= GLASS_PROMPT_MAX, "cosine_set: V and T must be in [1, 16]");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* df = dv.up32(feat, (size_t)P * V * D); float* dt = dv.up32(targets, (size_t)T * D); float* dw = dv.up32(weights, T);
    float* dvs = dv.alloc<float>((size_t)P * V); float* dss = dv.alloc<float>((size_t)P * T); float* ds = dv.alloc<float>(P);
    OPREQ(df && dt && dw && dvs && dss && ds, "device allocation failed");
    GLASS_HIP(hipMemset(dvs, 0xFF, (size_t)P * V * sizeof(float)));
    GLASS_HIP(hipMemset(dss, 0xFF, (size_t)P * T * sizeof(float)));
    GLASS_HIP(hipMemset(ds, 0xFF, (size_t)P * sizeof(float)));
    OPREQ(launch_cosine_set(df, dt, dw, prompt_weight_sum(weights, T), P, V, T, D, dvs, dss, ds, 0), "cosine_set refused the shape");
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(view_sim, dvs, (size_t)P * V * sizeof(float), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(set_sim, dss, (size_t)P * T * sizeof(float), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(sim, ds, (size_t)P * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_assemble_F_set(int32_t device, int32_t P, int32_t K, const float* set_sim, const float* weights, const float* dis,
                                       const float* lp, float* F) {
    OPREQ(set_sim && weights && F && P > 0 && K >= 1 && K <= GLASS_PROMPT_MAX, "bad argument (K in [1, 16])");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const int n_obj = K + (dis ? 1 : 0) + (lp ? 1 : 0);
    const size_t n = (size_t)P * n_obj;
    float* dss = dv.up32(set_sim, (size_t)P * K); float* dw = dv.up32(weights, K); float* dd = dv.up32(dis, P); float* dl = dv.up32(lp, P);
    float* dF = dv.alloc<float>(n + 4);      // four guard elements behind the output
    OPREQ(dss && dw && dF && (!dis || dd) && (!lp || dl), "device allocation failed");
    GLASS_HIP(hipMemset(dF, 0xFF, (n + 4) * sizeof(float)));
    launch_assemble_F_set(dss, dw, dd, dl, K, P, dF, 0);
    int rc = finish();
    if (rc) return rc;
    uint32_t guard[4];
    GLASS_HIP(hipMemcpy(guard, dF + n, sizeof guard, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) OPREQ(guard[i] == 0xFFFFFFFFu, "assemble_F_set stored past row P");
    GLASS_HIP(hipMemcpy(F, dF, n * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_image_patches(int32_t device, int32_t n, int32_t S, int32_t ps, int32_t ld, const float* img, float sentinel,
                                      float* patches) {
    OPREQ(img && patches && n > 0 && S > 0 && ps > 0 && S % ps == 0 && ld >= 3 * ps * ps, "bad argument (S % ps == 0, ld >= 3 ps ps)");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const int G = S / ps;
    const size_t tot = (size_t)n * G * G * ld;
    float* di = dv.up32(img, (size_t)n * 3 * S * S);
    half_t* dp = dv.up16v(std::vector<_Float16>(tot, (_Float16)sentinel));      // what the kernel does not write keeps the sentinel
    OPREQ(di && dp, "device allocation failed");
    launch_image_patches(di, n, S, ps, ld, dp, 0);
    int rc = finish();
    if (rc) return rc;
    return down16(patches, dp, tot);
}

extern "C" int glass_op_rn_token0_rows(int32_t device, int32_t B, int32_t T, int32_t C, const float* att, float* out) {
    OPREQ(att && out && B > 0 && T > 0 && C > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    half_t* da = dv.up16(att, (size_t)B * T * C); float* dout = dv.alloc<float>((size_t)B * C);
    OPREQ(da && dout, "device allocation failed");
    GLASS_HIP(hipMemset(dout, 0xFF, (size_t)B * C * sizeof(float)));
    launch_rn_token0_rows(da, B, T, C, dout, 0);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, dout, (size_t)B * C * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

__global__ void mfma_probe_kernel(const half_t* a, const half_t* b, float* d) {
    const int lane = threadIdx.x;
    const int r = lane & 31, kh = lane >> 5;
    h8 av, bv;
    for (int j = 0; j < 8; ++j) {
        av[j] = a[r * 16 + kh * 8 + j];       // A[i=r][k]
        bv[j] = b[(kh * 8 + j) * 32 + r];     // B[k][n=r]
    }
    f16x acc;
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    acc = mfma32(av, bv, acc);
    for (int reg = 0; reg < 16; ++reg) d[mfma32_row(reg, lane) * 32 + (lane & 31)] = acc[reg];
}
// ---- CLIP's ResNet towers ----
extern "C" int glass_op_rn_avgpool(int32_t device, int32_t B, int32_t H, int32_t W, int32_t C, const float* x, float* out) {
    OPREQ(x && out && B > 0 && H > 0 && W > 0 && C > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t no = (size_t)B * (H / 2) * (W / 2) * C;
    half_t* dx = dv.up16(x, (size_t)B * H * W * C);
    half_t* dy = dv.alloc<half_t>(no);
    OPREQ(dx && dy, "allocation failed");
    OPREQ(launch_rn_avgpool2(dx, B, H, W, C, dy, 0), "rn_avgpool2: refused (even H and W, C a multiple of 8)");
    int rc = finish();
    return rc ? rc : down16(out, dy, no);
}

extern "C" int glass_op_rn_stem_conv1(int32_t device, int32_t B, int32_t S, int32_t C1, const float* img, const float* w, const float* bn_a,
                                      const float* bn_s, float* out) {
    OPREQ(img && w && bn_a && bn_s && out && B > 0 && S > 0 && S % 32 == 0 && C1 > 0, "bad argument (S a multiple of 32)");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t ni = (size_t)B * 3 * S * S, no = (size_t)B * (S / 2) * (S / 2) * C1;
    std::vector<_Float16> wt((size_t)27 * C1);
    for (int o = 0; o < C1; ++o)
        for (int k = 0; k < 27; ++k) wt[(size_t)k * C1 + o] = (_Float16)w[(size_t)o * 27 + k];
    float* dimg = dv.up32(img, ni);
    half_t* dp = dv.alloc<half_t>(ni);
    half_t* dw = dv.up16v(wt);
    float *da = dv.up32(bn_a, C1), *ds = dv.up32(bn_s, C1);
    half_t* dy = dv.alloc<half_t>(no);
    OPREQ(dimg && dp && dw && da && ds && dy, "allocation failed");
    launch_image_patches(dimg, B, S, 32, 3072, dp, 0);
    OPREQ(launch_rn_stem_conv1(dp, dw, da, ds, B, S, C1, dy, 0), "rn_stem_conv1: refused (C1 a multiple of 8)");
    int rc = finish();
    return rc ? rc : down16(out, dy, no);
}

extern "C" int glass_op_rn_conv_bn(int32_t device, int32_t form, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t relu,
                                   const float* x, const float* w, const float* bn_a, const float* bn_s, const float* res, float* out) {
    OPREQ(x && w && bn_a && bn_s && out && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "bad argument");
    OPREQ((form == 0 && (KS == 1 || KS == 3)) || (form == 1 && KS == 3), "rn_conv_bn: form 0 takes KS 1 or 3, form 1 KS 3");
    OPREQ(KS == 1 || (relu && !res), "rn_conv_bn: the 3 x 3 forms are conv + BN + ReLU without a residual");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const int M = B * H * W, Mp = std::max(M, 64);
    RnConv c;
    c.cin = Cin; c.cout = Cout; c.ks = KS;
    c.w = dv.up16v(rn_pack_conv(w, Cout, Cin, KS));
    c.a = dv.up32(bn_a, Cout);
    c.s = dv.up32(bn_s, Cout);
    // M rows of data in buffers of max(M, 64) rows, the tail zero: what the engine's buffers hold
    half_t* dx = dv.alloc<half_t>((size_t)Mp * Cin);
    half_t* dr = res ? dv.alloc<half_t>((size_t)Mp * Cout) : nullptr;
    half_t* dy = dv.alloc<half_t>((size_t)Mp * Cout);
    OPREQ(c.w && c.a && c.s && dx && dy && (!res || dr), "allocation failed");
    auto fill = [&](half_t* d, const float* src, size_t rowlen) {
        std::vector<_Float16> h((size_t)Mp * rowlen, (_Float16)0.f);
        for (size_t i = 0; i < (size_t)M * rowlen; ++i) h[i] = (_Float16)src[i];
        return hipMemcpy(d, h.data(), h.size() * sizeof(half_t), hipMemcpyHostToDevice);
    };
    GLASS_HIP(fill(dx, x, Cin));
    if (res) GLASS_HIP(fill(dr, res, Cout));
    if (form == 1) {
        OPREQ(launch_rn_conv3x3(dx, c.w, c.a, c.s, B, H, W, Cin, Cout, dy, 0) != nullptr, "rn_conv3x3: refused (Cin % 16, Cout % 32)");
    } else {
        const GemmParams g = KS == 1 ? rn_gemm_1x1(dx, c, M, H * W, dr, relu, dy) : rn_gemm_3x3(dx, c, B, H, W, dy);
        OPREQ(launch_gemm_tiled(g, 0) != nullptr, "rn_conv_bn: gemm_tiled refused the shape (Cin and Cout multiples of 64)");
    }
    int rc = finish();
    return rc ? rc : down16(out, dy, (size_t)M * Cout);
}

extern "C" int glass_op_rn_tokens(int32_t device, int32_t B, int32_t HW, int32_t C, const float* x, const float* pos, float* out) {
    OPREQ(x && pos && out && B > 0 && HW > 0 && C > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t no = (size_t)B * (HW + 1) * C;
    half_t* dx = dv.up16(x, (size_t)B * HW * C);
    float* dp = dv.up32(pos, (size_t)(HW + 1) * C);
    half_t* dy = dv.alloc<half_t>(no);
    OPREQ(dx && dp && dy, "allocation failed");
    launch_rn_attnpool_tokens(dx, dp, B, HW, C, dy, 0);
    int rc = finish();
    return rc ? rc : down16(out, dy, no);
}

// ---- perceptual objective (lpips.hip) ----
extern "C" int glass_op_lpips_input(int32_t device, int32_t B, int32_t R, int32_t S, const float* y, float* out) {
    OPREQ(y && out && B > 0 && R > 0 && S > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t no = (size_t)B * S * S * 4;
    float* dy = dv.up32(y, (size_t)B * 3 * R * R);
    half_t* dout = dv.alloc<half_t>(no);
    OPREQ(dy && dout, "allocation failed");
    OPREQ(launch_lpips_input(dy, B, R, S, dout, 0), "lpips_input: refused (R a multiple of S, box R / S at most 8)");
    int rc = finish();
    return rc ? rc : down16(out, dout, no);
}

extern "C" int glass_op_vgg_conv1(int32_t device, int32_t B, int32_t S, const float* x, const float* w, const float* bias, float* out) {
    OPREQ(x && w && bias && out && B > 0 && S > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t no = (size_t)B * S * S * 64;
    std::vector<_Float16> wt((size_t)27 * 64);
    for (int o = 0; o < 64; ++o)
        for (int k = 0; k < 27; ++k) wt[(size_t)k * 64 + o] = (_Float16)w[(size_t)o * 27 + k];
    half_t* dx = dv.up16(x, (size_t)B * S * S * 4);
    half_t* dw = dv.up16v(wt);
    float* db = dv.up32(bias, 64);
    half_t* dy = dv.alloc<half_t>(no);
    OPREQ(dx && dw && db && dy, "allocation failed");
    OPREQ(launch_vgg_conv1(dx, dw, db, B, S, dy, 0), "vgg_conv1: refused");
    int rc = finish();
    return rc ? rc : down16(out, dy, no);
}

extern "C" int glass_op_maxpool2(int32_t device, int32_t B, int32_t H, int32_t W, int32_t C, const float* x, float* out) {
    OPREQ(x && out && B > 0 && H > 0 && W > 0 && C > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t no = (size_t)B * (H / 2) * (W / 2) * C;
    half_t* dx = dv.up16(x, (size_t)B * H * W * C);
    half_t* dy = dv.alloc<half_t>(no);
    OPREQ(dx && dy, "allocation failed");
    OPREQ(launch_maxpool2(dx, B, H, W, C, dy, 0), "maxpool2: refused (even H and W, C a multiple of 8)");
    int rc = finish();
    return rc ? rc : down16(out, dy, no);
}

extern "C" int glass_op_lpips_head(int32_t device, int32_t n, int32_t HW, int32_t C, int32_t shared_x1, const float* x0, const float* x1, const float* lin,
                                   float* out) {
    OPREQ(x0 && x1 && lin && out && n > 0 && HW > 0 && C > 0, "bad argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t map = (size_t)HW * C, nblk = ((size_t)HW + GLASS_LPIPS_PIXB - 1) / GLASS_LPIPS_PIXB;
    half_t* d0 = dv.up16(x0, (size_t)n * map);
    half_t* d1 = dv.up16(x1, (shared_x1 ? 1 : (size_t)n) * map);
    float* dl = dv.up32(lin, C);
    float* part = dv.alloc<float>((size_t)n * nblk);
    float* dd = dv.alloc<float>(n);
    OPREQ(d0 && d1 && dl && part && dd, "allocation failed");
    GLASS_HIP(hipMemset(dd, 0xFF, (size_t)n * sizeof(float)));
    OPREQ(launch_lpips_head(d0, d1, shared_x1 ? 0 : (long long)map, dl, n, HW, C, part, 1, dd, 0), "lpips_head: refused (C one of 64, 128, 256, 512)");
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(out, dd, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_mfma_probe(int32_t device, const float* a, const float* b, float* d) {
    OPREQ(a && b && d, "null argument");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    half_t* da = dv.up16(a, 32 * 16); half_t* db = dv.up16(b, 16 * 32); float* dd = dv.alloc<float>(32 * 32);
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, 0, da, db, dd);
    int rc = finish();
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(d, dd, 32 * 32 * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_host_pack_conv(const float* w, int32_t Cout, int32_t Cin, int32_t KS, int32_t up, float* out) {
    OPREQ(w && out, "null argument");
    std::vector<_Float16> pk;
    if (up) {
        OPREQ(KS == 3, "up conv is 3x3");
        glass_fold_upconv(w, Cout, Cin, pk);
    } else {
        glass_pack_conv(w, Cout, Cin, KS, Cin, pk);
    }
    for (size_t i = 0; i < pk.size(); ++i) out[i] = (float)pk[i];
    return GLASS_OK;
}

extern "C" int glass_host_resize_taps(int32_t R, int32_t S, int32_t mode, int32_t* start, int32_t* count, float* taps, int32_t max) {
    OPREQ(start && count && taps && max > 0, "bad argument");
    ResizeTaps t;
    std::string why;
    OPREQ(build_resize_taps(R, S, mode, t, why), why);
    OPREQ(t.max_count <= max, "a row needs " + std::to_string(t.max_count) + " taps, more than the caller's " + std::to_string(max));
    for (int i = 0; i < S; ++i) {
        start[i] = t.start[i];
        count[i] = t.count[i];
        for (int k = 0; k < max; ++k) taps[(size_t)i * max + k] = k < GLASS_RESIZE_MAX_TAPS ? t.taps[(size_t)i * GLASS_RESIZE_MAX_TAPS + k] : 0.f;
    }
    return GLASS_OK;
}

extern "C" int glass_host_gpt2_gemm_choice(int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ln, int32_t width, int32_t n_cu, int32_t* S, int32_t* NK) {
    OPREQ(S && NK && M > 0 && N > 0 && K > 0 && width > 0 && n_cu > 0, "bad argument");
    const StepGemm c = choose_gemm_f32_step(M, N, K, lda, ln != 0, (size_t)16 * M * 4 * width, n_cu);
    *S = c.S;
    *NK = c.NK;
    return GLASS_OK;
}

// ---- device search (search.hip) ---------------------------------------------------------------------------------------------------
extern "C" int glass_op_ga_vary(int32_t device, int32_t pop, int32_t n_var, const float* X, const int32_t* rank, const double* cd, double xl, double xu,
                                double eta_c, double eta_m, double prob_m, uint64_t seed, int32_t generation, int32_t row0, int32_t rows, float* out) {
    OPREQ(X && rank && cd && out, "null argument");
    if (int rc = glass_search_supported(pop, n_var, 1, GLASS_SEARCH_NSGA2)) return rc;
    OPREQ(rows > 0 && row0 >= 0 && row0 + rows <= pop, "ga_vary: [row0, row0 + rows) must lie inside the pop offspring rows");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t xn = (size_t)pop * n_var;
    float* dX = dv.up32(X, xn);
    int* dr = dv.alloc<int>(pop); double* dc = dv.alloc<double>(pop);
    float* dO = dv.alloc<float>(xn + 4);      // every offspring row, and four guard elements behind them
    OPREQ(dX && dr && dc && dO, "device allocation failed");
    GLASS_HIP(hipMemcpy(dr, rank, (size_t)pop * sizeof(int), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemcpy(dc, cd, (size_t)pop * sizeof(double), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemset(dO, 0xFF, (xn + 4) * sizeof(float)));
    GaParams g;
    g.pop = pop; g.xl = xl; g.xu = xu; g.eta_c = eta_c; g.eta_m = eta_m; g.prob_m = prob_m; g.seed = seed;
    OPREQ(launch_ga_vary(dX, dr, dc, g, n_var, generation, row0, rows, dO, 0), "ga_vary refused the shape");
    int rc = finish();
    if (rc) return rc;
    uint32_t guard[4];
    GLASS_HIP(hipMemcpy(guard, dO + xn, sizeof guard, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) OPREQ(guard[i] == 0xFFFFFFFFu, "ga_vary stored past the last row");
    GLASS_HIP(hipMemcpy(out, dO + (size_t)row0 * n_var, (size_t)rows * n_var * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_ga_duplicates(int32_t device, int32_t pop, int32_t n_off, int32_t n_var, const float* X, const float* Xoff, int32_t* flags) {
    OPREQ(X && Xoff && flags, "null argument");
    OPREQ(pop >= 1 && pop <= GLASS_SEARCH_MAX_POP && n_off >= 1 && n_off <= GLASS_SEARCH_MAX_POP && n_var >= 1, "ga_duplicates: pop and n_off in [1, 1024]");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    float* dX = dv.up32(X, (size_t)pop * n_var); float* dO = dv.up32(Xoff, (size_t)n_off * n_var);
    int* df = dv.alloc<int>(n_off + 4);
    OPREQ(dX && dO && df, "device allocation failed");
    GLASS_HIP(hipMemset(df, 0xFF, (size_t)(n_off + 4) * sizeof(int)));
    OPREQ(launch_ga_duplicates(dX, dO, pop, n_off, n_var, df, 0), "ga_duplicates refused the shape");
    int rc = finish();
    if (rc) return rc;
    uint32_t guard[4];
    GLASS_HIP(hipMemcpy(guard, df + n_off, sizeof guard, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) OPREQ(guard[i] == 0xFFFFFFFFu, "ga_duplicates stored past row n_off");
    GLASS_HIP(hipMemcpy(flags, df, (size_t)n_off * sizeof(int), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_op_ga_survive(int32_t device, int32_t n_pop, int32_t n_off, int32_t n_obj, int32_t pop_out, int32_t nsga, const float* F,
                                   const int32_t* flags, int32_t* chosen, int32_t* rank, double* cd, float* F_out, int32_t* counts, int32_t n_var,
                                   const float* X, const float* Xoff, float* X_out) {
    OPREQ(F && chosen && rank && cd && F_out && counts, "null argument");
    OPREQ(n_pop >= 1 && n_off >= 0 && n_obj >= 1 && pop_out >= 1, "ga_survive: bad sizes");
    const bool gather = X != nullptr;
    OPREQ(!gather || (X_out && n_var >= 1 && (Xoff || n_off == 0)), "ga_survive: X needs Xoff, X_out and n_var");
    GLASS_HIP(hipSetDevice(device));
    Dev dv;
    const size_t N = (size_t)n_pop + n_off;
    float* dF = dv.up32(F, N * n_obj);
    int* dfl = flags && n_off ? dv.alloc<int>(n_off) : nullptr;
    int* dch = dv.alloc<int>(pop_out + 4); int* drk = dv.alloc<int>(pop_out); double* dcd = dv.alloc<double>(pop_out); int* dcn = dv.alloc<int>(2);
    OPREQ(dF && dch && drk && dcd && dcn && (!(flags && n_off) || dfl), "device allocation failed");
    if (dfl) GLASS_HIP(hipMemcpy(dfl, flags, (size_t)n_off * sizeof(int), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemset(dch, 0xFF, (size_t)(pop_out + 4) * sizeof(int)));
    OPREQ(launch_ga_survive(dF, dfl, n_pop, n_off, n_obj, pop_out, nsga, dch, drk, dcd, dcn, 0),
          "ga_survive refused the shape (up to 2048 merged rows, 6 objectives, pop_out <= 1024 and <= the merged rows)");
    float* dXo = nullptr;
    if (gather) {
        float* dX = dv.up32(X, (size_t)n_pop * n_var); float* dO = n_off ? dv.up32(Xoff, (size_t)n_off * n_var) : nullptr;
        dXo = dv.alloc<float>((size_t)pop_out * n_var);
        OPREQ(dX && dXo && (!n_off || dO), "device allocation failed");
        GLASS_HIP(hipMemset(dXo, 0xFF, (size_t)pop_out * n_var * sizeof(float)));
        launch_ga_gather(dX, dO, dch, n_pop, pop_out, n_var, dXo, 0);
    }
    int rc = finish();
    if (rc) return rc;
    uint32_t guard[4];
    GLASS_HIP(hipMemcpy(guard, dch + pop_out, sizeof guard, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) OPREQ(guard[i] == 0xFFFFFFFFu, "ga_survive stored past slot pop_out");
    GLASS_HIP(hipMemcpy(chosen, dch, (size_t)pop_out * sizeof(int), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(rank, drk, (size_t)pop_out * sizeof(int), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(cd, dcd, (size_t)pop_out * sizeof(double), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(F_out, dF, (size_t)pop_out * n_obj * sizeof(float), hipMemcpyDeviceToHost));
    GLASS_HIP(hipMemcpy(counts, dcn, 2 * sizeof(int), hipMemcpyDeviceToHost));
    if (gather) GLASS_HIP(hipMemcpy(X_out, dXo, (size_t)pop_out * n_var * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}
