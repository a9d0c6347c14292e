// ops.hip — diagnostic per-kernel C ABI (include/glass_ops.h): host fp32 buffers in/out.
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "../../include/glass_ops.h"
#include "engine.h"
#include "kernels.h"

#define OPREQ(cond, msg) REQUIRE(cond, GLASS_ERR_ARG, msg)
#define TRY(call)                        \
    do {                                 \
        if (int rc_ = (call)) return rc_; \
    } while (0)

namespace {
// A device buffer of a Stage: `front` elements that no kernel may touch, n elements, then `guard` more that no kernel may touch either.
// p is the first of the n (the allocation starts at p - front).  Converts to the pointer the launchers take.
template <typename T>
struct Buf {
    T* p = nullptr;
    size_t n = 0, guard = 0, front = 0;
    operator T*() const { return p; }
    T* at(size_t off) const { return p ? p + off : nullptr; }
};

// The device side of one op: it selects the device, every buffer the launches see is made here, and the launches themselves run inside
// run() — which does not call them once an allocation or a copy has failed.  So no entry point checks its device pointers: a launch on
// a null pointer cannot be written.  A null HOST pointer is not a failure: it gives a null device pointer (the optional operands).
struct Stage {
    static constexpr size_t ALL = ~(size_t)0;
    std::vector<void*> owned;
    int failed = GLASS_OK;      // the first failure: GLASS_ERR_NOMEM (allocation) or GLASS_ERR_HIP (device, copy, fill), and its text
    std::string why;
    explicit Stage(int device) { ok(hipSetDevice(device), GLASS_ERR_HIP, "hipSetDevice"); }
    ~Stage() {
        for (void* q : owned) hipFree(q);
    }
    bool ok(hipError_t e, int code, const char* what) {
        if (e != hipSuccess && !failed) {
            failed = code;
            why = std::string(what) + " failed: " + hipGetErrorString(e);
        }
        return e == hipSuccess;
    }

    // outputs and scratch.  raw: whatever the allocation holds.  A front guard is rounded up to whole 4096-byte pages, so that the pointer
    // the launchers get keeps the alignment of an allocation's first byte (the LDS-DMA and 16-byte vector paths rely on it)
    static constexpr size_t FRONT_ALIGN = 4096;
    template <typename T>
    Buf<T> raw(size_t n, size_t guard = 0, size_t front = 0) {
        if constexpr (FRONT_ALIGN % sizeof(T) == 0) front = (front * sizeof(T) + FRONT_ALIGN - 1) / FRONT_ALIGN * (FRONT_ALIGN / sizeof(T));
        else front = 0;      // (a struct that does not divide a page: no front guard)
        void* q = nullptr;
        if (failed || !ok(hipMalloc(&q, std::max<size_t>(front + n + guard, 1) * sizeof(T)), GLASS_ERR_NOMEM, "hipMalloc")) return {};
        owned.push_back(q);      // (the base pointer: what ~Stage frees)
        return {(T*)q + front, n, guard, front};
    }
    // poisoned: every byte 0xFF (NaN as fp16 / fp32, -1 as int32), so that an element nobody stores shows; the guard elements too (intact())
    template <typename T>
    Buf<T> poisoned(size_t n, size_t guard = 0, size_t front = 0) {
        const Buf<T> b = raw<T>(n, guard, front);
        if (b.p) ok(hipMemset(b.p - b.front, 0xFF, (b.front + n + guard) * sizeof(T)), GLASS_ERR_HIP, "hipMemset");
        return b;
    }
    // n host elements to element `off` of b
    template <typename T>
    void put(const Buf<T>& b, size_t off, const T* src, size_t n) {
        if (b.p) ok(hipMemcpy(b.p + off, src, n * sizeof(T), hipMemcpyHostToDevice), GLASS_ERR_HIP, "hipMemcpy");
    }
    // inputs — and the outputs that are preloaded from the caller's array (strided and in-place ones: what the kernel leaves alone comes back)
    template <typename T>
    Buf<T> in(const T* src, size_t n) {
        if (!src) return {};
        const Buf<T> b = raw<T>(n);
        put(b, 0, src, n);
        return b;
    }
    Buf<float> in32(const float* src, size_t n) { return in(src, n); }
    Buf<int32_t> in_i32(const int32_t* src, size_t n) { return in(src, n); }
    Buf<half_t> in16(const std::vector<_Float16>& h) { return in(h.data(), h.size()); }
    Buf<half_t> in16(const float* src, size_t n) {
        if (!src) return {};
        std::vector<_Float16> h(n);
        for (size_t i = 0; i < n; ++i) h[i] = (_Float16)src[i];
        return in16(h);
    }

    // The op's launches (a callable returning nothing, or a status: a launcher's refusal), then the synchronisation.  Not called at all
    // after a failed allocation or copy.
    template <typename F>
    int run(F launches) {
        if (failed) {
            glass_set_error(why);
            return failed;
        }
        if constexpr (std::is_void_v<decltype(launches())>) launches();
        else TRY(launches());
        GLASS_HIP(hipDeviceSynchronize());
        GLASS_HIP(hipGetLastError());
        return GLASS_OK;
    }

    // n (default: all) elements from element `off` of b to the host; an fp16 buffer comes back as float
    template <typename T>
    int fetch(T* dst, const Buf<T>& b, size_t n = ALL, size_t off = 0) {
        GLASS_HIP(hipMemcpy(dst, b.p + off, (n == ALL ? b.n : n) * sizeof(T), hipMemcpyDeviceToHost));
        return GLASS_OK;
    }
    int fetch(float* dst, const Buf<half_t>& b, size_t n = ALL) {
        std::vector<_Float16> h(n == ALL ? b.n : n);
        TRY(fetch(h.data(), b, h.size()));
        for (size_t i = 0; i < h.size(); ++i) dst[i] = (float)h[i];
        return GLASS_OK;
    }
    // the guard elements on both sides of b still hold the poison — or `code`, with behind(i) for the first rear guard element i that does
    // not, before(i) for the front guard element i elements ahead of b's first (the nearest one that does not)
    template <typename T, typename F, typename G>
    int intact(const Buf<T>& b, int code, F behind, G before) {
        std::vector<unsigned char> g(b.guard * sizeof(T));
        GLASS_HIP(hipMemcpy(g.data(), b.p + b.n, g.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < g.size(); ++i) REQUIRE(g[i] == 0xFF, code, behind(i / sizeof(T)));
        g.resize(b.front * sizeof(T));
        GLASS_HIP(hipMemcpy(g.data(), b.p - b.front, g.size(), hipMemcpyDeviceToHost));
        for (size_t i = g.size(); i-- > 0;) REQUIRE(g[i] == 0xFF, code, before(b.front - i / sizeof(T)));
        return GLASS_OK;
    }
    template <typename T, typename F>
    int intact(const Buf<T>& b, int code, F behind) {
        return intact(b, code, behind, [](size_t i) { return "a store " + std::to_string(i) + " elements in front of the buffer"; });
    }
    template <typename T>
    int intact(const Buf<T>& b, const char* msg) {
        return intact(b, GLASS_ERR_ARG, [msg](size_t) { return msg; });
    }
    // the same for a buffer with a name: the message says which buffer, which side and which element
    template <typename T>
    int intact_named(const Buf<T>& b, const std::string& name) {
        return intact(b, GLASS_ERR_STATE,
                      [&](size_t i) { return name + ": a store behind the buffer, at element n + " + std::to_string(i) + " (n = " + std::to_string(b.n) + ")"; },
                      [&](size_t i) { return name + ": a store in front of the buffer, at element -" + std::to_string(i); });
    }
};

// The symbol(s) of the last conv / gemm / gemm_batched / bg_tail / dblock_down / dblock0 launch of the calling thread (glass_op_last_kernel): what ConvKernel::name,
// launch_conv_gemm, launch_conv_down and launch_dblock0 return; two launches of one op are joined by " + ".  Empty: the op launched nothing.
thread_local std::string g_last_kernel;
const char* ran_kernel(const char* name) {
    if (name) g_last_kernel += (g_last_kernel.empty() ? "" : " + ") + std::string(name);
    return name;
}
// the guard on each side of an image-shaped conv output: one tile of the tallest family (conv_glds, Geo::TH = 16 rows) of `row` elements a row
constexpr size_t CONV_GUARD_ROWS = 16;

// a launcher's answer as a status: false / nullptr is its refusal
template <typename R>
int accepted(R answer, const std::string& refusal) {
    OPREQ(answer, refusal);
    return GLASS_OK;
}

// impl 1: gemm_direct; 2: gemm_tiled, a refusal is an error; else gemm_tiled, then gemm_direct where it refuses (run_gemm's order).
// The symbol that ran goes to ran_kernel.
int launch_gemm_impl(const GemmParams& g, int impl) {
    if (impl == 1) ran_kernel(launch_gemm_direct(g, 0));
    else if (impl == 2) return accepted(ran_kernel(launch_gemm_tiled(g, 0)), "tiled gemm: unsupported shape");
    else if (!ran_kernel(launch_gemm_tiled(g, 0))) ran_kernel(launch_gemm_direct(g, 0));
    return GLASS_OK;
}
}  // namespace

extern "C" int glass_op_conv(int32_t device, const glass_conv_desc* d) {
    OPREQ(d && d->x && d->w && d->y, "null argument");
    OPREQ(d->Cin % 16 == 0, "Cin must be a multiple of 16");
    OPREQ(d->out_scale > 0.f, "out_scale must be positive (the epilogues fold it into the activation constants: max(v k1, v k2))");
    OPREQ(!d->pre_shift || d->sn, "pre_shift needs sn (the input affine is relu(x * sn + pre_shift))");
    OPREQ(d->in_up == 0 || (d->in_up == 1 && d->H % 2 == 0 && d->W % 2 == 0 && !d->up && !d->broadcast_x),
          "in_up: H and W are the upsampled dims and must be even (not with up / broadcast_x)");
    OPREQ(d->res_up == 0 || (d->res_up == 1 && d->res && d->Ho % 2 == 0 && d->Wo % 2 == 0), "res_up: needs res, Ho and Wo even");
    OPREQ(d->res_cs == 0 || (d->res && d->res_cs >= d->Cout), "res_cs: needs res, res_cs >= Cout");
    g_last_kernel.clear();
    Stage st(device);
    ConvParams p = conv_defaults();
    const int Hx = d->H >> d->in_up, Wx = d->W >> d->in_up;      // the stored input map
    const size_t xin = (size_t)(d->broadcast_x ? 1 : d->B) * Hx * Wx * d->Cin;
    p.x = st.in16(d->x, xin);
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
    p.w = st.in16(pk);
    if (d->up) {
        std::vector<_Float16> pk2;
        glass_pack_conv(d->w, d->Cout, d->Cin, 3, d->Cin, pk2);
        p.w_up = st.in16(pk2);
    }
    if (d->pre_shift) {       // one per-candidate table [A | S], fp32 and fp16, as bg_conv points sn / pre_shift / sn16 / pre_shift16 into tab / tab16
        std::vector<float> tab((size_t)d->B * 2 * d->Cin);
        for (int b = 0; b < d->B; ++b)
            for (int c = 0; c < d->Cin; ++c) {
                tab[((size_t)b * 2) * d->Cin + c] = d->sn[(size_t)b * d->Cin + c];
                tab[((size_t)b * 2 + 1) * d->Cin + c] = d->pre_shift[(size_t)b * d->Cin + c];
            }
        const auto t32 = st.in32(tab.data(), tab.size());
        const auto t16 = st.in16(tab.data(), tab.size());
        p.sn = t32; p.pre_shift = t32.at(d->Cin); p.sn16 = t16; p.pre_shift16 = t16.at(d->Cin); p.sn_stride = 2 * d->Cin;
    } else {
        p.sn = st.in32(d->sn, (size_t)d->B * d->Cin); p.sn_stride = d->Cin;
        p.sn16 = st.in16(d->sn, (size_t)d->B * d->Cin);
    }
    if (d->shift) {           // one table [dscale | shift], as bg_conv points dscale / shift into tab
        std::vector<float> tab((size_t)d->B * 2 * d->Cout);
        for (int b = 0; b < d->B; ++b)
            for (int c = 0; c < d->Cout; ++c) {
                tab[((size_t)b * 2) * d->Cout + c] = d->dscale ? d->dscale[(size_t)b * d->Cout + c] : 1.f;
                tab[((size_t)b * 2 + 1) * d->Cout + c] = d->shift[(size_t)b * d->Cout + c];
            }
        const auto t32 = st.in32(tab.data(), tab.size());
        p.dscale = d->dscale ? t32.p : nullptr; p.shift = t32.at(d->Cout); p.ds_stride = 2 * d->Cout;
    } else {
        p.dscale = st.in32(d->dscale, (size_t)d->B * d->Cout); p.ds_stride = d->Cout;
    }
    p.batch_size = d->batch_size > 0 ? d->batch_size : 1;
    p.noise = st.in32(d->noise, (size_t)(d->B / p.batch_size) * d->Ho * d->Wo);
    p.noise_strength = d->noise_strength;
    p.bias = st.in32(d->bias, d->Cout);
    p.act = d->act;
    p.res_cs = d->res_cs; p.res_up = d->res_up;
    p.res = st.in16(d->res, (size_t)d->B * (d->Ho >> d->res_up) * (d->Wo >> d->res_up) * (d->res_cs ? d->res_cs : d->Cout));
    p.out_scale = d->out_scale;
    // NaN: an element no thread stores shows; a tile of guard elements on both sides: a store outside the output shows (intact_named below)
    const size_t gy = CONV_GUARD_ROWS * d->Wo * d->Cout;
    const auto y = st.poisoned<half_t>((size_t)d->B * d->Ho * d->Wo * d->Cout, gy, gy);
    p.y = y;
    if (d->skip_x) {
        OPREQ(d->skip_w, "fused skip branch: skip_x and skip_w");
        std::vector<_Float16> pks;
        glass_pack_conv(d->skip_w, d->Cout, d->Cin, 1, d->Cin, pks);
        p.skip_w = st.in16(pks);
        p.skip_x = st.in16(d->skip_x, (size_t)d->B * d->Ho * d->Wo * d->Cin);
    }
    Buf<half_t> xs_dev;
    if (d->xs_out) {
        const size_t gx = CONV_GUARD_ROWS * (d->W / 2) * d->Cin;
        xs_dev = st.poisoned<half_t>((size_t)d->B * (d->H / 2) * (d->W / 2) * d->Cin, gx, gx);
        p.xs_out = xs_dev;
    }
    Buf<float> yrgb;
    Buf<half_t> trgb_tab;
    const size_t nrgb = (size_t)d->B * 3 * d->Ho * d->Wo;
    if (d->trgb_yout) {
        OPREQ(d->trgb_w && d->trgb_b && d->trgb_sn && d->trgb_smax, "fused toRGB: all of w / b / sn / smax");
        p.trgb_w = st.in32(d->trgb_w, 3 * (size_t)d->Cout); p.trgb_b = st.in32(d->trgb_b, 3);
        p.trgb_sn = st.in32(d->trgb_sn, (size_t)d->B * d->Cout); p.trgb_sn_stride = d->Cout;
        p.trgb_smax = st.in32(d->trgb_smax, d->B); p.trgb_smax_stride = 1;
        p.trgb_yprev = st.in32(d->trgb_yprev, (size_t)d->B * 3 * (d->Ho / 2) * (d->Wo / 2));
        yrgb = st.poisoned<float>(nrgb, CONV_GUARD_ROWS * d->Wo * 3, CONV_GUARD_ROWS * d->Wo * 3);
        p.trgb_yout = yrgb;
        if (d->impl == 4 && !d->trgb_keep_map) {
            p.y = nullptr;                       // the streaming form never stores the map
        } else {                                 // the forms that store it too: weight tables from the table kernel (the first launch below)
            trgb_tab = st.poisoned<half_t>((size_t)d->B * 32 * d->Cout);      // (scratch: a row the table kernel leaves out reaches the image as NaN)
            p.trgb_tab = trgb_tab;
        }
    }
    p.x_planar8 = d->x_planar8;
    p.x_planar32 = d->x_planar32;
    p.y_planar8 = d->y_planar8;
    if (d->post_scale) {
        p.post_scale16 = st.in16(d->post_scale, (size_t)d->B * d->Cout); p.post_stride = d->Cout;
    }
    // per-sample pre-modulated weights, set up as stylegan2.cpp g_conv_params does for a premod layer: wm from mod_w / mod_sn / mod_ds (the second launch below)
    const long long welems = 9LL * d->Cin * d->Cout;
    Buf<half_t> wm;
    const half_t* mod_w = nullptr;
    const float *mod_sn = nullptr, *mod_ds = nullptr;
    if (d->premod) {
        OPREQ(d->sn && d->KS == 3 && !d->broadcast_x, "premod: 3x3 with sn, not with broadcast_x");
        OPREQ(!d->up || d->impl == 3, "premod up-conv: impl 3 only (the folded table is not modulated)");
        wm = st.poisoned<half_t>((size_t)d->B * welems);
        mod_w = d->up ? p.w_up : p.w; mod_sn = p.sn; mod_ds = p.dscale;
        p.sn = nullptr; p.sn16 = nullptr; p.dscale = nullptr; p.w_bstride = welems;
        if (d->up) { p.w_up = wm; p.w = nullptr; }
        else p.w = wm;
    }
    Buf<float> ytanh;
    if (d->rgb_tanh) {
        const size_t gt = CONV_GUARD_ROWS * d->Wo;
        ytanh = st.poisoned<float>(nrgb, gt, gt);      // NaN: a pixel the conv does not write shows
        p.rgb_tanh_out = ytanh;
    }
    Buf<float> part;
    const float* part_yprev = p.trgb_yprev;
    const int ntn = d->Cout / 128;
    if (d->trgb_partial) {   // toRGB partial sums per 128-wide n tile, as torgb_conv_params sets ToRgb::partial up; launch_trgb_finish below
        OPREQ(d->trgb_yout && d->Cout % 128 == 0 && d->Ho == d->Wo, "toRGB partial sums: the trgb inputs, Cout % 128 == 0, Ho == Wo");
        part = st.poisoned<float>((size_t)ntn * nrgb);      // NaN: a partial the conv does not write shows in the sum
        p.trgb_part = part; p.trgb_yout = nullptr; p.trgb_yprev = nullptr;
    }
    // impl 6: scratch per candidate; room for the four split-K slices the launcher may choose, as the engine's scratch (256 * 4 * cmax floats) always has
    const long long cap_a = (long long)p.Hc * p.Wc * p.KS * p.KS * p.Cin, cap_c = 4LL * p.Hc * p.Wc * p.Neff;
    uint32_t gemm_outside = 0;
    const bool gemm_admits = d->impl == 6 && conv_gemm_admits(p, cap_a, cap_c, &gemm_outside);
    Buf<half_t> gemm_a;
    Buf<float> gemm_c;
    if (gemm_admits) {
        // poisoned like the engine's reused scratch holds arbitrary bits: an element the GEMM reads and im2col / a split-K slice did not write is NaN
        gemm_a = st.poisoned<half_t>((size_t)(cap_a * p.B));
        gemm_c = st.poisoned<float>((size_t)(cap_c * p.B));
    }
    TRY(st.run([&]() -> int {
        if (trgb_tab) launch_trgb_tables(p.trgb_w, p.trgb_sn, p.trgb_sn_stride, p.trgb_smax, p.trgb_smax_stride, d->B, d->Cout, trgb_tab, 0);
        if (wm) launch_modulate_weights(mod_w, welems, d->Cin, d->Cout, mod_sn, p.sn_stride, mod_ds, p.ds_stride, d->B, wm, 0);
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
        case 6:
            ran = gemm_admits && ran_kernel(launch_conv_gemm(p, gemm_a, cap_a, gemm_c, cap_c, 0));
            if (!ran) refused("conv_gemm", gemm_outside);
            break;
        default:
            (d->up && ask("upfir", choose_conv_upfir(p))) || ask("conv_stream", choose_conv_stream(p)) || ask("conv_s2", choose_conv_s2(p)) ||
                ask("conv_tiled", choose_conv_tiled(p)) || ask("conv_direct", choose_conv_direct(p));
        }
        if (k) ran_kernel(k.name), k.launch(p, 0);
        else   // (the planar tanh keeps the words its earlier refusal had)
            OPREQ(ran, (ytanh ? "rgb_tanh: conv_tiled only; " : "") + std::string(labels[d->impl >= 1 && d->impl <= 6 ? d->impl : 0]) + why + ")");
        return GLASS_OK;
    }));
    if (part) TRY(st.run([&] { launch_trgb_finish(part, ntn, d->B, d->Ho, p.trgb_b, part_yprev, yrgb, 0); }));
    if (ytanh) {                                                 // (p.y is not written: every byte of it still holds the poison)
        TRY(st.fetch(d->rgb_tanh, ytanh));
        TRY(st.intact_named(ytanh, "conv: rgb_tanh"));
        std::vector<_Float16> hy(y.n);
        TRY(st.fetch(hy.data(), y));
        for (size_t i = 0; i < hy.size(); ++i) {
            uint16_t bits;
            memcpy(&bits, &hy[i], sizeof bits);
            REQUIRE(bits == 0xFFFF, GLASS_ERR_STATE, "conv: y (rgb_tanh form, not an output) was written at element " + std::to_string(i));
        }
        return st.intact_named(y, "conv: y (rgb_tanh form, not an output)");
    }
    if (yrgb) {
        TRY(st.fetch(d->trgb_yout, yrgb));
        TRY(st.intact_named(yrgb, "conv: trgb_yout"));
        if (p.y) TRY(st.fetch(d->y, y));                // (the forms that also store the feature map hand it back too)
        return st.intact_named(y, "conv: y");
    }
    if (xs_dev) {
        TRY(st.fetch(d->xs_out, xs_dev));
        TRY(st.intact_named(xs_dev, "conv: xs_out"));
    }
    TRY(st.fetch(d->y, y));
    return st.intact_named(y, "conv: y");
}

// the rows behind an output that no GEMM / attention kernel may touch (one whole m tile of the widest kernel)
constexpr size_t GUARD_ROWS = 128;

extern "C" int glass_op_gemm(int32_t device, int32_t M, int32_t N, int32_t K, const float* a, const float* w,
                             const float* bias, int32_t mode, int32_t impl, float* out) {
    OPREQ(a && w && out && K % 16 == 0, "bad argument");
    g_last_kernel.clear();
    Stage st(device);
    GemmParams g;
    memset(&g, 0, sizeof g);
    g.a = st.in16(a, (size_t)M * K); g.w = st.in16(w, (size_t)N * K); g.M = M; g.N = N; g.K = K;
    g.bias = st.in32(bias, N); g.mode = mode; g.ldo = N;
    const size_t n = (size_t)M * N;
    Buf<half_t> o16;
    Buf<float> o32;
    if (mode <= 1) g.out16 = o16 = st.poisoned<half_t>(n, GUARD_ROWS * N);
    else {
        g.out32 = o32 = st.poisoned<float>(n, GUARD_ROWS * N);
        if (mode == 2) st.put(o32, 0, out, n);
    }
    TRY(st.run([&] { return launch_gemm_impl(g, impl); }));
    TRY(o16 ? st.fetch(out, o16) : st.fetch(out, o32));
    return o16 ? st.intact(o16, "gemm: a store behind the output (row >= M)") : st.intact(o32, "gemm: a store behind the output (row >= M)");
}

// what gemm_direct implements of GemmParams: not the `ld` split-K slices, not the BatchNorm epilogue, not the implicit patch matrix
static bool gemm_direct_implements(const GemmParams& g) { return !g.ld && g.mode != 5 && !g.g_on; }

extern "C" int glass_op_gemm_ex(int32_t device, int32_t batch, int32_t M, int32_t N, int32_t K, int32_t ldo, const float* a, const float* w,
                                const float* bias, int32_t mode, int32_t impl, int32_t cand_rows, int32_t cand_batch, float* out, char* kernel,
                                int32_t cap) {
    OPREQ(a && w && out && kernel, "null argument");
    OPREQ(batch >= 1 && M > 0 && N > 0 && K > 0 && K % 16 == 0 && ldo >= N, "bad shape (batch >= 1, K a multiple of 16, ldo >= N)");
    OPREQ(mode >= 0 && mode <= 4, "mode must lie in [0, 4] (mode 5, the BatchNorm epilogue, and the ld split-K form are gemm_tiled's alone: glass_op_rn_conv_bn, glass_op_d_head)");
    OPREQ(impl >= 0 && impl <= 2, "impl must lie in [0, 2]");
    OPREQ(cand_rows >= 0 && cap >= 64, "cand_rows >= 0, room for 64 characters of kernel name");
    kernel[0] = 0;
    Stage st(device);
    const size_t n = (size_t)batch * M * ldo, guard = GUARD_ROWS * ldo;
    GemmParams g = gemm_params(st.in16(a, (size_t)batch * M * K), st.in16(w, (size_t)batch * N * K), M, N, K, st.in32(bias, N), mode, nullptr, nullptr, cand_rows);
    g.ldo = ldo;
    g.cand_batch = cand_batch ? 1 : 0;
    g.batch = batch; g.a_bs = (long long)M * K; g.w_bs = (long long)N * K; g.o_bs = (long long)M * ldo;
    // the whole [batch][M][ldo] array travels in (mode 2's accumulator, the ldo padding, the caller's sentinels) and comes back
    Buf<half_t> o16;
    Buf<float> o32;
    if (mode <= 1) {
        std::vector<_Float16> h(n);
        for (size_t i = 0; i < n; ++i) h[i] = (_Float16)out[i];      // (a NaN stays a NaN)
        g.out16 = o16 = st.poisoned<half_t>(n, guard);
        st.put(o16, 0, h.data(), n);
    } else {
        g.out32 = o32 = st.poisoned<float>(n, guard);
        st.put(o32, 0, out, n);
    }
    const char* name = nullptr;
    const int rc = st.run([&]() -> int {
        if (impl != 1) name = launch_gemm_tiled(g, 0);
        if (!name && impl == 2) OPREQ(false, "tiled gemm: unsupported shape");
        if (!name) {
            OPREQ(gemm_direct_implements(g), "gemm_tiled refused a form that gemm_direct does not implement");
            name = launch_gemm_direct(g, 0);
        }
        return GLASS_OK;
    });
    if (rc == GLASS_OK || rc == GLASS_ERR_ARG) TRY(o16 ? st.fetch(out, o16) : st.fetch(out, o32));      // (a refusal: what no kernel touched)
    if (rc) return rc;
    snprintf(kernel, (size_t)cap, "%s", name);
    return o16 ? st.intact(o16, GLASS_ERR_STATE, [&](size_t i) { return "gemm_ex: a store " + std::to_string(i) + " elements behind the output"; })
               : st.intact(o32, GLASS_ERR_STATE, [&](size_t i) { return "gemm_ex: a store " + std::to_string(i) + " elements behind the output"; });
}

extern "C" int glass_op_gemm_batched(int32_t device, int32_t batch, int32_t M, int32_t N, int32_t K, const float* a, const float* w, int32_t mode,
                                     int32_t cand_batch, int32_t impl, float* out) {
    OPREQ(a && w && out && batch >= 1 && M > 0 && N > 0 && K > 0 && K % 16 == 0, "bad argument (K a multiple of 16)");
    OPREQ(mode == 0 || mode == 3, "batched gemm: mode 0 (fp16 out) or 3 (fp32 out), the self-attention products");
    OPREQ(impl >= 0 && impl <= 2, "impl must lie in [0, 2]");
    g_last_kernel.clear();
    Stage st(device);
    const size_t n = (size_t)batch * M * N, guard = GUARD_ROWS * N;
    const auto da = st.in16(a, (size_t)batch * M * K), dw = st.in16(w, (size_t)batch * N * K);
    Buf<half_t> o16;
    Buf<float> o32;
    if (mode == 0) o16 = st.poisoned<half_t>(n, guard, guard);      // NaN: an element no tile stores shows
    else o32 = st.poisoned<float>(n, guard, guard);
    GemmParams g = gemm_params(da, dw, M, N, K, nullptr, mode, o16, o32, 0);      // as bg_attention (biggan.cpp)
    g.cand_batch = cand_batch ? 1 : 0;
    g.batch = batch; g.a_bs = (long long)M * K; g.w_bs = (long long)N * K; g.o_bs = (long long)M * N;
    TRY(st.run([&] { return launch_gemm_impl(g, impl); }));
    TRY(o16 ? st.fetch(out, o16) : st.fetch(out, o32));
    return o16 ? st.intact_named(o16, "gemm_batched: out") : st.intact_named(o32, "gemm_batched: out");
}

extern "C" int glass_op_dense(int32_t device, int32_t P, int32_t K, int32_t N, const float* x, const float* wt,
                              const float* bias, int32_t in_sq, int32_t mode, const float* eps_row, float* out) {
    OPREQ(x && wt && out, "null argument");
    Stage st(device);
    const auto dx = st.in32(x, (size_t)P * K), dw = st.in32(wt, (size_t)K * N), db = st.in32(bias, N), de = st.in32(eps_row, P);
    const auto dout = st.raw<float>((size_t)P * N);
    TRY(st.run([&] { launch_dense(dx, K, P, K, dw, N, db, dout, N, in_sq, mode, de, 1, 0); }));
    return st.fetch(out, dout);
}

extern "C" int glass_op_torgb(int32_t device, int32_t B, int32_t H, int32_t C, const float* x, const float* wrgb,
                              const float* bias, const float* sn, const float* smax, const float* yprev, float* yout) {
    OPREQ(x && wrgb && bias && sn && smax && yout, "null argument");
    Stage st(device);
    const auto dx = st.in16(x, (size_t)B * H * H * C);
    const auto dw = st.in32(wrgb, 3 * C), db = st.in32(bias, 3), ds = st.in32(sn, (size_t)B * C), dm = st.in32(smax, B);
    const auto dp = st.in32(yprev, (size_t)B * 3 * (H / 2) * (H / 2));
    const auto dy = st.poisoned<float>((size_t)B * 3 * H * H, GUARD_ROWS * H);      // NaN: a pixel no thread stores shows
    TRY(st.run([&] { return accepted(launch_torgb(dx, B, H, H, C, dw, db, ds, C, dm, 1, dp, dy, 0), "toRGB: channel width not instantiated"); }));
    TRY(st.fetch(yout, dy));
    return st.intact(dy, "toRGB: stored behind the output (pixel >= H W of the last sample)");
}

extern "C" int glass_op_blur(int32_t device, int32_t mode, int32_t B, int32_t H, int32_t C, const float* x, float* out) {
    OPREQ(x && out && C % 8 == 0, "bad argument");
    OPREQ(mode != 2 || blur_pad2_planar32_ok(C), "blur in 32-channel planes: C must be 32 x a power of two, <= 512");
    Stage st(device);
    const int Ho = mode != 1 ? H + 1 : H / 2;
    const auto dx = st.in16(x, (size_t)B * H * H * C);
    const auto dy = st.poisoned<half_t>((size_t)B * Ho * Ho * C, GUARD_ROWS * C);
    TRY(st.run([&] {
        if (mode != 1) launch_blur_pad2(dx, B, H, H, C, dy, 0, mode == 2);
        else launch_blur_down(dx, B, H, H, C, dy, 0);
    }));
    TRY(st.fetch(out, dy));
    return st.intact(dy, "blur: stored behind the output (row >= Ho or column >= Wo of the last sample)");
}

extern "C" int glass_op_dblock_down(int32_t device, int32_t B, int32_t R, int32_t Cin, int32_t Cout, const float* h,
                                    const float* x, const float* w1, const float* wskip, const float* b1, float* y) {
    OPREQ(h && x && w1 && wskip && b1 && y, "bad argument");
    OPREQ(conv_down_supported(R, Cin, Cout), "conv_down: unsupported shape");
    g_last_kernel.clear();
    Stage st(device);
    const auto dh = st.in16(h, (size_t)B * R * R * Cin), dx = st.in16(x, (size_t)B * R * R * Cin);
    std::vector<_Float16> pk;
    glass_pack_conv(w1, Cout, Cin, 3, Cin, pk);
    const auto dw1 = st.in16(pk);
    glass_pack_conv(wskip, Cout, Cin, 1, Cin, pk);
    const auto dws = st.in16(pk);
    const auto db = st.in32(b1, Cout);
    const int Ro = R / 2;
    const size_t gxs = CONV_GUARD_ROWS * Ro * Cin, gy = CONV_GUARD_ROWS * Ro * Cout;
    const auto dxs = st.poisoned<half_t>((size_t)B * Ro * Ro * Cin, gxs, gxs), dy = st.poisoned<half_t>((size_t)B * Ro * Ro * Cout, gy, gy);
    TRY(st.run([&]() -> int {
        launch_blur_down(dx, B, R, R, Cin, dxs, 0);          // the skip branch's FIR (pad 1) + ::2 (conv_stream<fromrgb> emits it in the engine)
        return accepted(ran_kernel(launch_conv_down(dh, dxs, dw1, dws, db, dy, B, R, Cin, Cout, 0)) != nullptr, "conv_down: unsupported shape");
    }));
    TRY(st.fetch(y, dy));
    TRY(st.intact_named(dxs, "dblock_down: xs (the blur-down of x)"));
    return st.intact_named(dy, "dblock_down: y");
}

extern "C" int glass_op_dblock0(int32_t device, int32_t B, int32_t R, int32_t impl, const float* y, const float* frgb_w, const float* frgb_b,
                                const float* w0, const float* b0, const float* w1, const float* wskip, const float* b1, float* out) {
    OPREQ(y && frgb_w && frgb_b && w0 && b0 && w1 && wskip && b1 && out && B > 0 && R > 0, "bad argument");
    g_last_kernel.clear();
    Stage st(device);
    const int Cin = 32, Cout = 64, Ro = R / 2;
    const bool fused = impl == 0 || impl == 2;      // conv_d0.hip: the whole block in one kernel (2: chunk-planar output)
    const auto dy = st.in32(y, (size_t)B * 3 * R * R), dfw = st.in32(frgb_w, Cin * 3), dfb = st.in32(frgb_b, Cin);
    std::vector<_Float16> pk;
    glass_pack_conv(w0, Cin, Cin, 3, Cin, pk);
    const auto dw0 = st.in16(pk);
    glass_pack_conv(w1, Cout, Cin, 3, Cin, pk);
    const auto dw1 = st.in16(pk);
    glass_pack_conv(wskip, Cout, Cin, 1, Cin, pk);
    const auto dws = st.in16(pk);
    const auto db0 = st.in32(b0, Cin), db1 = st.in32(b1, Cout);
    const size_t gout = CONV_GUARD_ROWS * Ro * Cout, gh = CONV_GUARD_ROWS * R * Cin, gxs = CONV_GUARD_ROWS * Ro * Cin;
    const auto dout = st.poisoned<half_t>((size_t)B * Ro * Ro * Cout, gout, gout);
    Buf<half_t> dh, dxs;      // the two-kernel form it replaces: conv_stream<fromrgb> (h + the skip input to HBM) + conv_down
    if (!fused) {             // dh is conv_stream<fromrgb>'s x AND its y: the kernel builds its input from the skip image and never reads x — the poison proves it
        dh = st.poisoned<half_t>((size_t)B * R * R * Cin, gh, gh);
        dxs = st.poisoned<half_t>((size_t)B * Ro * Ro * Cin, gxs, gxs);
    }
    TRY(st.run([&]() -> int {
        if (fused) return accepted(ran_kernel(launch_dblock0(dy, dfw, dfb, dw0, db0, dw1, dws, db1, dout, B, R, Cin, Cout, 0, impl == 2)) != nullptr, "dblock0: unsupported shape");
        ConvParams p = conv_defaults();
        p.x = dh; p.x_bstride = (long long)R * R * Cin; p.B = B; p.H = p.W = R; p.Cin = Cin; p.Hc = p.Wc = R; p.KS = 3; p.pad = 1;
        p.w = dw0; p.Cout = p.Neff = Cin; p.Ho = p.Wo = R; p.bias = db0; p.act = 1; p.y = dh;
        p.rgb_y = dy; p.rgb_w = dfw; p.rgb_b = dfb; p.rgb_xs_out = dxs;
        const ConvKernel k = choose_conv_stream(p);
        OPREQ(k, "dblock0 (two-kernel form): conv_stream<fromrgb> does not take this shape");
        ran_kernel(k.name);
        k.launch(p, 0);
        return accepted(ran_kernel(launch_conv_down(dh, dxs, dw1, dws, db1, dout, B, R, Cin, Cout, 0)) != nullptr, "dblock0 (two-kernel form): conv_down does not take this shape");
    }));
    TRY(st.fetch(out, dout));
    if (!fused) {
        TRY(st.intact_named(dh, "dblock0: h (conv_stream<fromrgb>'s map)"));
        TRY(st.intact_named(dxs, "dblock0: xs (the skip branch's input)"));
    }
    return st.intact_named(dout, "dblock0: out");
}

extern "C" int glass_op_last_kernel(char* buf, int32_t cap) {
    OPREQ(buf && cap > 0, "last_kernel: a buffer of cap > 0 characters");
    OPREQ(g_last_kernel.size() < (size_t)cap, "last_kernel: the name needs " + std::to_string(g_last_kernel.size() + 1) + " characters");
    memcpy(buf, g_last_kernel.c_str(), g_last_kernel.size() + 1);
    return GLASS_OK;
}

extern "C" int glass_op_fromrgb(int32_t device, int32_t B, int32_t R, int32_t Cout, const float* y, const float* w,
                                const float* bias, float* out) {
    OPREQ(y && w && bias && out && Cout % 8 == 0, "bad argument");
    Stage st(device);
    const auto dy = st.in32(y, (size_t)B * 3 * R * R), dw = st.in32(w, Cout * 3), db = st.in32(bias, Cout);
    const auto dout = st.poisoned<half_t>((size_t)B * R * R * Cout, GUARD_ROWS * Cout);
    TRY(st.run([&] { launch_fromrgb(dy, B, R, Cout, dw, db, dout, 0); }));
    TRY(st.fetch(out, dout));
    return st.intact(dout, "fromRGB: stored behind the output (pixel >= R R of the last sample)");
}

extern "C" int glass_op_mbstd(int32_t device, int32_t B, int32_t hw, int32_t C, int32_t Cpad, int32_t batch_size,
                              int32_t group, const float* x, float* out) {
    OPREQ(x && out && B % batch_size == 0 && batch_size % group == 0 && group <= 8, "bad argument");
    Stage st(device);
    const auto dx = st.in16(x, (size_t)B * hw * C);
    const auto dy = st.raw<half_t>((size_t)B * hw * Cpad);
    TRY(st.run([&] { launch_mbstd(dx, B, hw, C, Cpad, batch_size, group, 1e-8f, dy, 0); }));
    return st.fetch(out, dy);
}

extern "C" int glass_op_resize(int32_t device, int32_t B, int32_t R, int32_t S, int32_t ps, const float* y, float* patches) {
    OPREQ(y && patches && S % ps == 0, "bad argument");
    Stage st(device);
    const auto dy = st.in32(y, (size_t)B * 3 * R * R);
    const auto dp = st.raw<half_t>((size_t)B * 3 * S * S);
    TRY(st.run([&] { launch_resize_patches(dy, B, R, S, ps, 3 * ps * ps, dp, 0); }));
    return st.fetch(patches, dp);
}

extern "C" int glass_op_preprocess(int32_t device, int32_t B, int32_t R, int32_t S, int32_t ps, int32_t resize_mode, int32_t normalize,
                                   const float* y, float* patches) {
    OPREQ(y && patches && B > 0 && R > 0 && ps > 0 && S > 0 && S % ps == 0, "bad argument");
    TRY(glass_clip_preprocess_supported(R, S, resize_mode, normalize));
    ResizeTaps t;
    std::string why;
    if (resize_mode) OPREQ(build_resize_taps(R, S, resize_mode, t, why), why);
    Stage st(device);
    const auto dy = st.in32(y, (size_t)B * 3 * R * R);
    const auto dp = st.raw<half_t>((size_t)B * 3 * S * S);
    ResizeTapsDev td;
    if (resize_mode) {
        td.table = st.in32(t.table.data(), t.table.size());
        td.n4 = (int)(t.table.size() / 4); td.ts = t.ts; td.lds_bytes = t.lds_bytes;
    }
    TRY(st.run([&] {
        if (resize_mode == 0 && normalize == 0) launch_resize_patches(dy, B, R, S, ps, 3 * ps * ps, dp, 0);
        else launch_preprocess_patches(dy, B, R, S, ps, 3 * ps * ps, resize_mode, normalize, td, dp, 0);
    }));
    return st.fetch(patches, dp);
}

extern "C" int glass_op_view_patches(int32_t device, int32_t B, int32_t R, int32_t S, int32_t ps, int32_t normalize, int32_t V, const int32_t* boxes,
                                     const float* y, float* patches) {
    OPREQ(y && patches && boxes && B > 0 && R > 0 && ps > 0 && S > 0 && S % ps == 0 && S <= 4096 && (normalize == 0 || normalize == 1), "bad argument");
    OPREQ(V >= 1 && V <= GLASS_MAX_CLIP_VIEWS, "views must be in [1, 16]");
    ViewBoxes vb = {};
    for (int i = 0; i < 4 * V; ++i) vb.box[i / 4][i % 4] = boxes[i];
    OPREQ(view_boxes_valid(vb, V, R), "a box (x0, y0, s, flip) leaves the image or has flip outside {0, 1}");
    OPREQ((long long)B * V * ((S * S + 255) / 256) < (1LL << 31), "too many images");
    Stage st(device);
    const auto dy = st.in32(y, (size_t)B * 3 * R * R);
    const auto dp = st.raw<half_t>((size_t)B * V * 3 * S * S);
    TRY(st.run([&] { launch_view_patches(dy, B, R, S, ps, 3 * ps * ps, normalize, V, vb, dp, 0); }));
    return st.fetch(patches, dp);
}

extern "C" int glass_op_layernorm(int32_t device, int32_t M, int32_t D, const float* x, const float* g, const float* b, float* out) {
    OPREQ(x && g && b && out, "null argument");
    Stage st(device);
    const auto dx = st.in32(x, (size_t)M * D), dg = st.in32(g, D), db = st.in32(b, D);
    const auto dout = st.raw<float>((size_t)M * D);
    TRY(st.run([&] { launch_layernorm(dx, D, M, D, dg, db, nullptr, dout, 0); }));
    return st.fetch(out, dout);
}

extern "C" int glass_op_attention(int32_t device, int32_t n_img, int32_t L, int32_t heads, int32_t causal,
                                  const float* qkv, float* out) {
    OPREQ(qkv && out && n_img > 0 && heads > 0 && L >= 1 && L <= 4096, "bad argument (1 <= L <= 4096)");
    Stage st(device);
    const int D = heads * 64;
    const auto dq = st.in16(qkv, (size_t)n_img * L * 3 * D);
    const auto dout = st.poisoned<half_t>((size_t)n_img * L * D, GUARD_ROWS * D);
    TRY(st.run([&] { launch_attention(dq, n_img, L, heads, 64, causal, dout, 0); }));
    TRY(st.fetch(out, dout));
    return st.intact(dout, "attention: a store behind the output (token >= n_img L)");
}

extern "C" int glass_op_noise(int32_t device, int32_t n_mb, int32_t hw, uint32_t layer, uint32_t mb0,
                              uint32_t generation, uint64_t seed, float* out) {
    OPREQ(out, "null argument");
    Stage st(device);
    const auto d = st.poisoned<float>((size_t)n_mb * hw, GUARD_ROWS * 4);
    TRY(st.run([&] { launch_noise(d, n_mb, hw, layer, mb0, generation, seed, 0); }));
    TRY(st.fetch(out, d));
    return st.intact(d, "noise: stored behind the output (element >= hw of the last plane)");
}

// launch_noise with a period: plane m is that of minibatch (mb0 + m) % period (period 0: glass_op_noise)
extern "C" int glass_op_noise_period(int32_t device, int32_t n_mb, int32_t hw, uint32_t layer, uint32_t mb0, uint32_t generation, uint64_t seed,
                                     uint32_t period, float* out) {
    OPREQ(out && n_mb > 0 && hw > 0, "bad argument");
    Stage st(device);
    const auto d = st.poisoned<float>((size_t)n_mb * hw, GUARD_ROWS * 4);
    TRY(st.run([&] { launch_noise(d, n_mb, hw, layer, mb0, generation, seed, 0, period); }));
    TRY(st.fetch(out, d));
    return st.intact(d, "noise: stored behind the output (element >= hw of the last plane)");
}

extern "C" int glass_op_gpt2_sample(int32_t device, int32_t rows, int32_t V, const float* logits, float temperature, int32_t top_k,
                                    uint64_t seed, int32_t generation, int32_t first_row, int32_t step, int32_t purpose, int32_t* out) {
    OPREQ(logits && out && rows > 0 && V > 0, "bad argument");
    OPREQ(temperature > 0.f && temperature < INFINITY, "temperature must be a finite value > 0");
    OPREQ(top_k >= 0 && top_k <= GPT2_SAMPLE_TOPK_MAX, "top_k must lie in [0, 256]");
    OPREQ(gpt2_sample_supported(V), "vocabulary too large for the sampler (> 131072)");
    Stage st(device);
    int32_t h[GPT2_SP_WORDS];
    h[GPT2_SP_SEED_LO] = (int32_t)(uint32_t)(seed & 0xFFFFFFFFu);
    h[GPT2_SP_SEED_HI] = (int32_t)(uint32_t)(seed >> 32);
    h[GPT2_SP_GEN] = generation;
    h[GPT2_SP_ROW0] = first_row;
    h[GPT2_SP_PURPOSE] = purpose;
    memcpy(&h[GPT2_SP_TEMP], &temperature, sizeof(float));
    h[GPT2_SP_TOPK] = top_k;
    h[GPT2_SP_STEP] = step;
    const auto d = st.in32(logits, (size_t)rows * V);
    const auto sp = st.in_i32(h, GPT2_SP_WORDS);
    const auto o = st.raw<int32_t>(rows);
    TRY(st.run([&] { launch_gpt2_sample(d, rows, V, sp, o, nullptr, 0); }));
    return st.fetch(out, o);
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
    Stage st(device);
    const size_t part_elems = (size_t)16 * M * 4 * width;                      // the engine's split-K scratch for a model of this width
    const auto da = st.in32(a, (size_t)M * lda), dw = st.in32(w, (size_t)N * K), db = st.in32(bias, N), dg = st.in32(lng, K), dlb = st.in32(lnb, K);
    // the output is followed by guard rows up to the kernels' 64-row granularity: a store of a clamped row (m >= M) lands there and is reported
    const auto dout = st.poisoned<float>((size_t)M * N, ((size_t)(M + 63) / 64 * 64 - M) * N);
    if (mode == 2) st.put(dout, 0, out, (size_t)M * N);
    const auto part = st.raw<float>(part_elems), dstats = st.raw<float>((size_t)M * 2);
    Buf<float> dpi, dpo;
    if (ln && form == 3) dpi = st.in32(pst_in, (size_t)M * np_in * 2);
    if (pst_out) dpo = st.raw<float>((size_t)M * (N / 32 + 1) * 2);
    int S = 1;
    TRY(st.run([&]() -> int {
        if (form == 0 || form == 1) {
            launch_gemm_f32(da, dw, db, dout, M, N, K, lda, N, mode, 0, part, part_elems, form == 0);
        } else if (form == 2) {
            if (ln) launch_gpt2_finalize(nullptr, 0, nullptr, da, M, K, dstats, 0);
            const StepGemm c = choose_gemm_f32_step(M, N, K, lda, ln, part_elems, glass_cu_count());
            OPREQ(c, "choose_gemm_f32_step refused the shape");
            launch_gemm_f32_step({da, dw, db, dout, N, mode, part, ln ? dstats.p : nullptr, dg, dlb}, c, 0);
            S = c.S;
            if (mode == 2) launch_gpt2_finalize(S > 1 ? part.p : nullptr, S, db, dout, M, N, dstats, 0);
            else if (S > 1) launch_gpt2_reduce(part, S, db, dout, M, N, N, mode, 0);
        } else {
            const StepGemm c = choose_gemm_f32_rowblk(M, N, K, lda, ln, np_in, dpo.p != nullptr);
            OPREQ(c, "choose_gemm_f32_rowblk refused the shape");
            launch_gemm_f32_rowblk({da, dw, db, dout, N, mode, nullptr, dpi, dg, dlb, dpo}, c, 0);
        }
        return GLASS_OK;
    }));
    *splits = S;
    TRY(st.fetch(out, dout));
    TRY(st.intact(dout, GLASS_ERR_STATE, [&](size_t i) { return "gpt2_gemm: the product stored to row " + std::to_string(M + i / N) + " >= M"; }));
    if (stats_out && form == 2 && (ln || mode == 2)) TRY(st.fetch(stats_out, dstats));
    if (pst_out && form == 3) TRY(st.fetch(pst_out, dpo, (size_t)M * (N / 32) * 2));
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
    Stage st(device);
    const size_t nq = (size_t)(form == 2 && S > 0 ? S : 1) * P * nd * 3 * D, nc = (size_t)P * Tmax * D;
    const int32_t state[3] = {past, 1, 0};
    const auto dq = st.in32(qkv, nq), db = st.in32(bias, 3 * D), dk = st.in32(kc, nc), dvc = st.in32(vc, nc);
    const auto dout = st.poisoned<float>((size_t)P * nd * D);
    const auto dpast = st.in_i32(state, 3);
    TRY(st.run([&] {
        if (form == 2) launch_gpt2_attention_step(dq, S > 0 ? dq.p : nullptr, S > 0 ? S : 1, db, dk, dvc, P, Tmax, heads, dout, 0, dpast);
        else launch_gpt2_attention(dq, dk, dvc, P, nd, form == 1 ? 0 : past, Tmax, heads, dout, 0, form == 1 ? dpast.p : nullptr);
    }));
    TRY(st.fetch(out, dout));
    TRY(st.fetch(kc, dk));
    return st.fetch(vc, dvc);
}

extern "C" int glass_op_gpt2_head(int32_t device, int32_t M, int32_t V, int32_t K, int32_t tail, const float* x, const float* wte, const float* lng,
                                  const float* lnb, const float* wpe, int32_t npos, int32_t past, int32_t step, float* logits, float* pair_val,
                                  int32_t* pair_idx, int32_t* token, float* stats, float* x_next, float* stats_next, int32_t* state) {
    OPREQ(x && wte && lng && lnb && token && stats, "null argument");
    OPREQ(M > 0 && K > 0 && K <= 1024 && gpt2_head_supported(M, V, K, K), "gpt2_head_kernel: M <= 64, K % 64 == 0, K <= 1024, V >= 4096");
    if (tail) OPREQ(wpe && x_next && stats_next && state && past >= 0 && past + 1 < npos && step >= 0, "tail: wpe [npos, K], past + 1 < npos, step >= 0");
    else OPREQ(logits && pair_val && pair_idx, "null argument");
    Stage st(device);
    const size_t NB = (size_t)(V + 31) / 32;
    const int32_t st0[3] = {past, step, 0};
    const auto dx = st.in32(x, (size_t)M * K), dw = st.in32(wte, (size_t)V * K), dg = st.in32(lng, K), db = st.in32(lnb, K);
    const auto dstats = st.raw<float>((size_t)M * 2);
    const auto pairs = tail ? st.raw<float>(2 * M * NB) : st.poisoned<float>(2 * M * NB);
    Buf<float> dl, dpe;
    Buf<int32_t> dgen, dstate;      // the picks: [M], or with the tail the rows of every step so far, this step's last
    if (!tail) {
        dl = st.poisoned<float>((size_t)M * V);
        dgen = st.raw<int32_t>(M);
    } else {
        dpe = st.in32(wpe, (size_t)npos * K);
        dgen = st.raw<int32_t>((size_t)(step + 1) * M);
        dstate = st.in_i32(st0, 3);
    }
    TRY(st.run([&] { launch_gpt2_finalize(nullptr, 0, nullptr, dx, M, K, dstats, 0); }));      // the statistics the last layer's finalize leaves
    TRY(st.fetch(stats, dstats));
    if (!tail) {
        TRY(st.run([&]() -> int {
            const Gpt2Head h = choose_gpt2_head(M, V, K, K, GPT2_PICK_ARGMAX, true);
            OPREQ(h, "choose_gpt2_head refused the shape");
            launch_gpt2_head({dx, dw, dstats, dg, db, dl, pairs, nullptr, dgen, nullptr}, h, 0);
            return GLASS_OK;
        }));
        TRY(st.fetch(logits, dl));
        TRY(st.fetch(pair_val, pairs, M * NB));
        TRY(st.fetch((float*)pair_idx, pairs, M * NB, M * NB));      // (the indices' bits, behind the values)
        return st.fetch(token, dgen);
    }
    // as the engine: the residual stream and its statistics are the head's operands AND the buffers the tail leaves the next step's in
    TRY(st.run([&]() -> int {
        const Gpt2Head h = choose_gpt2_head(M, V, K, K, GPT2_PICK_ARGMAX_TAIL, false);
        OPREQ(h, "choose_gpt2_head refused the shape");
        launch_gpt2_head({dx, dw, dstats, dg, db, nullptr, pairs, nullptr, dgen, dstate, dw, dpe, dx, dstats}, h, 0);
        return GLASS_OK;
    }));
    TRY(st.fetch(token, dgen, M, (size_t)step * M));
    TRY(st.fetch(x_next, dx));
    TRY(st.fetch(stats_next, dstats));
    return st.fetch(state, dstate);
}

extern "C" int glass_op_gpt2_embed_step(int32_t device, int32_t M, int32_t V, int32_t K, const int32_t* token, const float* wte, const float* wpe,
                                        int32_t npos, int32_t past, int32_t step, float* x, float* stats) {
    OPREQ(token && wte && wpe && x && stats, "null argument");
    OPREQ(M > 0 && V > 0 && K > 0 && K <= 1024 && past >= 0 && past < npos && step >= 1, "bad argument (K <= 1024 with statistics, past < npos, step >= 1)");
    for (int i = 0; i < M; ++i) OPREQ(token[i] >= 0 && token[i] < V, "token id out of range");
    Stage st(device);
    const int32_t st0[3] = {past, step, 0};
    const auto dw = st.in32(wte, (size_t)V * K), dpe = st.in32(wpe, (size_t)npos * K);
    const auto dx = st.raw<float>((size_t)M * K), ds = st.raw<float>((size_t)M * 2);
    const auto dgen = st.raw<int32_t>((size_t)step * M);
    st.put(dgen, (size_t)(step - 1) * M, token, M);
    const auto dstate = st.in_i32(st0, 3);
    TRY(st.run([&] { launch_gpt2_embed_step(dgen, dstate, M, dw, dpe, K, dx, 0, ds); }));
    TRY(st.fetch(x, dx));
    return st.fetch(stats, ds);
}

// ---- BigGAN-deep glue kernels (biggan_kernels.hip) and the fused last stage (bg_tail.hip), launched as biggan.cpp launches them ------------
extern "C" int glass_op_bg_cond(int32_t device, int32_t P, int32_t L, int32_t zd, int32_t nc, const float* x, const float* et, float* cond) {
    OPREQ(x && et && cond && P > 0 && zd > 0 && nc > 0 && L >= zd + nc, "bad argument (rows are [z (zd) | class bits (nc)], L >= zd + nc)");
    OPREQ((size_t)(nc + 8) * sizeof(float) <= 64 * 1024, "bg_cond_kernel keeps the class probabilities in LDS: nc + 8 floats <= 64 KB");
    Stage st(device);
    const auto dx = st.in32(x, (size_t)P * L), de = st.in32(et, (size_t)nc * zd);
    const auto dc = st.poisoned<float>((size_t)P * 2 * zd);
    TRY(st.run([&] { launch_bg_cond(dx, P, L, zd, nc, de, dc, 0); }));
    return st.fetch(cond, dc);
}

extern "C" int glass_op_bg_bn_tables(int32_t device, int32_t P, int32_t cd, int32_t C, const float* cond, const float* wt, const float* bias,
                                     const float* inv_std, const float* mean, const float* prebias, float* tab, float* tab16) {
    OPREQ(cond && wt && bias && inv_std && mean && prebias && tab && tab16 && P > 0 && cd > 0 && C > 0, "bad argument");
    Stage st(device);
    const size_t n = (size_t)P * 2 * C;
    const auto dc = st.in32(cond, (size_t)P * cd), dw = st.in32(wt, (size_t)cd * 2 * C), db = st.in32(bias, 2 * (size_t)C);
    const auto di = st.in32(inv_std, C), dm = st.in32(mean, C), dp = st.in32(prebias, C);
    const auto dt = st.poisoned<float>(n);          // NaN: a table entry launch_dense does not write shows in both tables
    const auto dt16 = st.poisoned<half_t>(n);
    TRY(st.run([&] {      // glass_biggan_prepare's three launches
        launch_dense(dc, cd, P, cd, dw, 2 * C, db, dt, 2 * C, 0, 0, nullptr, 0, 0);
        launch_bg_bn_tables(dt, P, C, di, dm, dp, 0);
        launch_bg_to_half(dt, dt16, (long long)n, 0);
    }));
    TRY(st.fetch(tab, dt));
    return st.fetch(tab16, dt16);
}

extern "C" int glass_op_bg_attn_split(int32_t device, int32_t B, int32_t H, int32_t W, int32_t c8, int32_t c2, const float* T, float* theta,
                                      float* phi, float* gT, int32_t* vec) {
    OPREQ(T && theta && phi && gT && vec && B > 0 && c8 > 0 && c2 > 0, "bad argument");
    OPREQ(H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "bg_attn_split: H and W must be even (2x2 max-pool)");
    Stage st(device);
    const size_t hw = (size_t)H * W, hq = hw / 4, CT = 2 * (size_t)c8 + c2;
    const auto dT = st.in16(T, (size_t)B * hw * CT);
    const auto dth = st.poisoned<half_t>((size_t)B * hw * c8), dph = st.poisoned<half_t>((size_t)B * hq * c8), dg = st.poisoned<half_t>((size_t)B * hq * c2);
    TRY(st.run([&] { *vec = strcmp(launch_bg_attn_split(dT, B, H, W, c8, c2, dth, dph, dg, 0), "bg_attn_split_vec_kernel") == 0; }));
    TRY(st.fetch(theta, dth));
    TRY(st.fetch(phi, dph));
    return st.fetch(gT, dg);
}

extern "C" int glass_op_bg_softmax(int32_t device, int32_t rows, int32_t n, const float* S, float* out) {
    OPREQ(S && out && rows > 0 && n > 0, "bad argument");
    Stage st(device);
    const auto ds = st.in32(S, (size_t)rows * n);
    const auto dp = st.poisoned<half_t>((size_t)rows * n);
    TRY(st.run([&] { launch_bg_softmax(ds, rows, n, dp, 0); }));
    return st.fetch(out, dp);
}

extern "C" int glass_op_bg_rgb_tanh(int32_t device, int32_t B, int32_t hw, int32_t C, const float* x, float* y) {
    OPREQ(x && y && B > 0 && hw > 0 && C >= 3, "bad argument (C >= 3)");
    Stage st(device);
    const auto dx = st.in16(x, (size_t)B * hw * C);
    const auto dy = st.poisoned<float>((size_t)B * 3 * hw);
    TRY(st.run([&] { launch_bg_rgb_tanh(dx, B, hw, C, dy, 0); }));
    return st.fetch(y, dy);
}

extern "C" int glass_op_bg_to_half(int32_t device, int64_t n, const float* x, float* out) {
    OPREQ(x && out && n > 0, "bad argument");
    Stage st(device);
    const auto dx = st.in32(x, (size_t)n);
    const auto dy = st.poisoned<half_t>((size_t)n, 4);
    TRY(st.run([&] { launch_bg_to_half(dx, dy, n, 0); }));
    TRY(st.intact(dy, "bg_to_half stored past element n"));
    return st.fetch(out, dy);
}

extern "C" int glass_op_bg_tail(int32_t device, int32_t B, int32_t R, int32_t mid, const float* h, const float* x0, const float* w3, const float* b3,
                                const float* bn_a, const float* bn_s, const float* rgb_w, const float* rgb_b, float* y) {
    OPREQ(h && x0 && w3 && b3 && bn_a && bn_s && rgb_w && rgb_b && y && B > 0 && R > 0 && mid > 0, "bad argument");
    const int C = 128, cpad = 32;                           // the last block's width; BgState::rgb_cpad
    OPREQ(bg_tail_supported(R, mid, C, C, 1, cpad), "bg_tail: unsupported shape (R % 32 == 0, R >= 32, mid == 32, 128 -> 128 channels of an up block)");
    g_last_kernel.clear();
    Stage st(device);
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
    tp.h = st.in16(h, (size_t)B * R * R * mid);
    tp.x0 = st.in16(x0, (size_t)B * R2 * R2 * C);
    tp.w3 = st.in16(w3, (size_t)C * mid);
    tp.b3 = st.in32(b3, C);
    tp.tab = st.in32(tab.data(), tab.size()); tp.bnf_off = 0; tp.ctot = C;
    tp.rgb_w = st.in16(pk); tp.cpad = cpad;
    tp.rgb_b = st.in32(rb.data(), rb.size());
    const size_t gy = CONV_GUARD_ROWS * R;
    const auto dy = st.poisoned<float>((size_t)B * 3 * R * R, gy, gy);      // NaN: a pixel no tile writes shows; 16 image rows of guard on both sides
    tp.y = dy; tp.B = B; tp.R = R;
    TRY(st.run([&]() -> int {
        TRY(accepted(launch_bg_tail(tp, 0), "bg_tail: the launcher refused the shape"));
        ran_kernel("bg_tail_kernel");       // (launch_bg_tail has one instance)
        return GLASS_OK;
    }));
    TRY(st.fetch(y, dy));
    return st.intact_named(dy, "bg_tail: y");
}

// ---- the small fp32 kernels around StyleGAN2 and the CLIP towers, each launched as the engine's host code launches it ------------------------
// (tests/test_gpu_small_ops.py against the float64 restatements of tests/small_ops_ref.py).  Strided operands arrive with their padding
// as the caller filled it (NaN); outputs wider than what a kernel writes are uploaded first, so that what it leaves alone comes back unchanged.
extern "C" int glass_op_mapping(int32_t device, int32_t P, int32_t L, int32_t n_layers, const float* z, const float* wt, const float* b,
                                int32_t path, float* out, int32_t* ran) {
    OPREQ(z && wt && b && out && ran && P > 0 && L > 0 && n_layers >= 1 && n_layers <= 8, "bad argument (1 .. 8 layers)");
    OPREQ(path >= 0 && path <= 2, "path must lie in [0, 2]");
    Stage st(device);
    const size_t n = (size_t)P * L;
    const auto dz = st.in32(z, n);
    const auto w0 = st.poisoned<float>(n), w1 = st.poisoned<float>(n);
    std::vector<const float*> dw(n_layers), db(n_layers);
    for (int i = 0; i < n_layers; ++i) {
        dw[i] = st.in32(wt + (size_t)i * L * L, (size_t)L * L);
        db[i] = st.in32(b + (size_t)i * L, L);
    }
    TRY(st.run([&]() -> int {
        *ran = launch_mapping(dz, w0, w1, P, L, 1e-8f, dw.data(), db.data(), n_layers, path, 0);
        return accepted(*ran != 0, "mapping_fused_kernel does not take this network (L = 256 / 512, its LDS within the device's limit)");
    }));
    return st.fetch(out, w0);
}

extern "C" int glass_op_pixelnorm(int32_t device, int32_t P, int32_t L, const float* z, float* out) {
    OPREQ(z && out && P > 0 && L > 0, "bad argument");
    Stage st(device);
    const auto dz = st.in32(z, (size_t)P * L);
    const auto dout = st.poisoned<float>((size_t)P * L);
    TRY(st.run([&] { launch_pixelnorm(dz, dout, P, L, 1e-8f, 0); }));
    return st.fetch(out, dout);
}

extern "C" int glass_op_dense_splitk(int32_t device, int32_t P, int32_t K, int32_t N, int32_t ldx, int32_t ldo, int32_t mode, const float* x,
                                     const float* wt, const float* bias, float* out) {
    OPREQ(x && wt && out && P > 0 && N > 0, "bad argument");
    OPREQ(K > 0 && K % 64 == 0 && K <= 768, "dense_splitk_kernel: K a multiple of 64, at most 768 (64 KB of LDS)");
    OPREQ(ldx >= K && ldo >= N && (mode == 0 || mode == 1), "ldx >= K, ldo >= N, mode 0 or 1");
    Stage st(device);
    const auto dx = st.in32(x, (size_t)P * ldx), dw = st.in32(wt, (size_t)K * N), db = st.in32(bias, N);
    const auto dout = st.in32(out, (size_t)P * ldo);
    TRY(st.run([&] { launch_dense_splitk(dx, ldx, P, K, dw, N, db, dout, ldo, mode, 0); }));
    return st.fetch(out, dout);
}

extern "C" int glass_op_dense_ex(int32_t device, int32_t P, int32_t K, int32_t N, int32_t ldx, int32_t ldo, const float* x, const float* wt,
                                 const float* bias, int32_t in_sq, int32_t mode, const float* eps_row, int32_t eps_stride, float* out) {
    OPREQ(x && wt && out && P > 0 && K > 0 && N > 0 && ldx >= K && ldo >= N, "bad argument (ldx >= K, ldo >= N)");
    OPREQ(mode >= 0 && mode <= 2 && (mode != 2 || (eps_row && eps_stride >= 1)), "mode 2 reads eps_row [P, eps_stride]");
    Stage st(device);
    const auto dx = st.in32(x, (size_t)P * ldx), dw = st.in32(wt, (size_t)K * N), db = st.in32(bias, N);
    const auto de = st.in32(eps_row, (size_t)P * eps_stride), dout = st.in32(out, (size_t)P * ldo);
    TRY(st.run([&] { launch_dense(dx, ldx, P, K, dw, N, db, dout, ldo, in_sq, mode, de, eps_stride, 0); }));
    return st.fetch(out, dout);
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
    Stage st(device);
    const auto dx = st.in32(x, (size_t)P * ldx), dw = st.in32(wt, wtot), de = st.in32(eps_rows, (size_t)P * eps_stride);
    const auto dout = st.in32(out, (size_t)P * ldo);
    std::vector<DenseDesc> dd(n);       // as finalize builds the demodulation table (engine.cpp)
    size_t woff = 0;
    for (int i = 0; i < n; ++i) {
        DenseDesc& q = dd[i];
        q.x = dx.at(x_off[i]); q.ldx = ldx; q.K = K[i]; q.wt = dw.at(woff); q.N = N[i]; q.bias = nullptr;
        q.out = dout.at(out_off[i]); q.ldo = ldo; q.eps_row = de.at(eps_idx[i]); q.eps_stride = eps_stride;
        woff += (size_t)K[i] * N[i];
    }
    const auto ddev = st.in(dd.data(), dd.size());
    TRY(st.run([&] { launch_dense_multi(ddev, n, max_N, P, 1, 2, 0); }));
    return st.fetch(out, dout);
}

extern "C" int glass_op_style_norm(int32_t device, int32_t P, int32_t ld, int32_t n_layers, const int32_t* off, const int32_t* len, float* s,
                                   float* smax, float* eps_row) {
    OPREQ(off && len && s && smax && eps_row && P > 0 && n_layers > 0, "bad argument");
    for (int l = 0; l < n_layers; ++l) OPREQ(off[l] >= 0 && len[l] > 0 && off[l] + len[l] <= ld, "a segment leaves the row");
    Stage st(device);
    const size_t m = (size_t)P * n_layers;
    const auto ds = st.in32(s, (size_t)P * ld);
    const auto dm = st.poisoned<float>(m), de = st.poisoned<float>(m);
    const auto doff = st.in_i32(off, n_layers), dlen = st.in_i32(len, n_layers);
    TRY(st.run([&] { launch_style_norm(ds, ld, P, n_layers, doff, dlen, dm, de, 1e-8f, 0); }));
    TRY(st.fetch(s, ds));
    TRY(st.fetch(smax, dm));
    return st.fetch(eps_row, de);
}

extern "C" int glass_op_d_head(int32_t device, int32_t P, int32_t CL, const float* dfin, const float* w0, const float* b0, const float* w1,
                               const float* b1, float* dis, int32_t* split) {
    OPREQ(dfin && w0 && b0 && w1 && b1 && dis && split && P > 0 && CL > 0 && CL % 4 == 0, "bad argument (CL a multiple of 4)");
    Stage st(device);
    const size_t K = 16 * (size_t)CL;
    DHead h;
    h.dfin = st.in16(dfin, (size_t)P * K); h.w0 = st.in16(w0, (size_t)CL * K);
    h.b0 = st.in32(b0, CL); h.w1t = st.in32(w1, CL); h.b1 = st.in32(b1, 1);
    h.part = st.poisoned<float>((size_t)16 * P * CL);      // NaN: a slice element nobody stores shows in the sum
    h.dh = st.poisoned<float>((size_t)P * CL);
    const auto ddis = st.poisoned<float>(P);
    h.dis = ddis;
    h.P = P; h.CL = CL;
    TRY(st.run([&] {
        *split = launch_d_head_split(h, 0) != nullptr;
        if (!*split) {                        // as run_d_head: the whole product (run_gemm's order: gemm_tiled, then gemm_direct), then the second layer
            launch_gemm_impl(d_head_dense0(h), 0);
            launch_d_head_dense1(h, 0);
        }
    }));
    return st.fetch(dis, ddis);
}

extern "C" int glass_op_finalize_image(int32_t device, int64_t n, const float* y, float* img) {
    OPREQ(y && img && n > 0, "bad argument");
    Stage st(device);
    const auto dy = st.in32(y, (size_t)n);
    const auto di = st.poisoned<float>((size_t)n, 4);
    TRY(st.run([&] { launch_finalize_image(dy, di, n, 0); }));
    TRY(st.intact(di, "finalize_image stored past element n"));
    return st.fetch(img, di);
}

extern "C" int glass_op_embed_lnpre(int32_t device, int32_t P, int32_t T, int32_t D, const float* patch_emb, const float* cls, const float* pos,
                                    const float* g, const float* b, float* x) {
    OPREQ(patch_emb && cls && pos && g && b && x && P > 0 && T >= 2 && D > 0, "bad argument (T = 1 + patches >= 2)");
    Stage st(device);
    const auto dpe = st.in32(patch_emb, (size_t)P * (T - 1) * D), dc = st.in32(cls, D), dp = st.in32(pos, (size_t)T * D);
    const auto dg = st.in32(g, D), db = st.in32(b, D);
    const auto dx = st.poisoned<float>((size_t)P * T * D);
    TRY(st.run([&] { launch_embed_lnpre(dpe, dc, dp, dg, db, P, T, D, dx, 0); }));
    return st.fetch(x, dx);
}

extern "C" int glass_op_embed_text(int32_t device, int32_t n_texts, int32_t ctx, int32_t D, int32_t V, const int32_t* tokens, const float* tok_emb,
                                   const float* pos, float* x) {
    OPREQ(tokens && tok_emb && pos && x && n_texts > 0 && ctx > 0 && D > 0 && V > 0, "bad argument");
    const int rows = n_texts * ctx;
    for (int i = 0; i < rows; ++i) OPREQ(tokens[i] >= 0 && tokens[i] < V, "token id out of range");
    Stage st(device);
    const auto dt = st.in_i32(tokens, rows);
    const auto de = st.in32(tok_emb, (size_t)V * D), dp = st.in32(pos, (size_t)ctx * D);
    const auto dx = st.poisoned<float>((size_t)rows * D);
    TRY(st.run([&] { launch_embed_text(dt, de, dp, rows, ctx, D, dx, 0); }));
    return st.fetch(x, dx);
}

extern "C" int glass_op_layernorm_ex(int32_t device, int32_t M, int32_t D, int64_t row_stride, int32_t half_out, const float* x, const float* g,
                                     const float* b, float* out) {
    OPREQ(x && g && b && out && M > 0 && D > 0 && row_stride >= D, "bad argument (row_stride >= D)");
    Stage st(device);
    const size_t n = (size_t)M * D;
    const auto dx = st.in32(x, (size_t)(M - 1) * row_stride + D), dg = st.in32(g, D), db = st.in32(b, D);
    Buf<float> o32;
    Buf<half_t> o16;
    if (half_out) o16 = st.poisoned<half_t>(n);
    else o32 = st.poisoned<float>(n);
    TRY(st.run([&] { launch_layernorm(dx, row_stride, M, D, dg, db, o16, o32, 0); }));
    return o16 ? st.fetch(out, o16) : st.fetch(out, o32);
}

extern "C" int glass_op_layernorm_rows(int32_t device, int32_t n_rows, int32_t M, int32_t D, const float* x, const int32_t* rows, const float* g,
                                       const float* b, float* out) {
    OPREQ(x && rows && g && b && out && n_rows > 0 && M > 0 && D > 0, "bad argument");
    for (int i = 0; i < M; ++i) OPREQ(rows[i] >= 0 && rows[i] < n_rows, "row index out of range");
    Stage st(device);
    const auto dx = st.in32(x, (size_t)n_rows * D), dg = st.in32(g, D), db = st.in32(b, D);
    const auto dr = st.in_i32(rows, M);
    const auto dout = st.poisoned<float>((size_t)M * D);
    TRY(st.run([&] { launch_layernorm_rows(dx, dr, M, D, dg, db, dout, 0); }));
    return st.fetch(out, dout);
}

// The five cosine ops: the operands staged, the one launcher (score.hip), the outputs the caller asked for.  weights: [T], or with islands > 0 the
// table [islands, T]; src (nullable): the directional form; refusal: the text of the launcher's `false`
static int cosine_op(int device, int P, int V, int T, int D, const float* feat, const float* targets, const float* weights, int islands, int pop,
                     int row0, const float* src, bool streamed, const char* refusal, float* view_sim, float* set_sim, float* sim) {
    std::vector<float> W(std::max(islands, 1));
    for (size_t i = 0; i < W.size(); ++i) W[i] = prompt_weight_sum(weights + i * T, T);
    Stage st(device);
    CosineSet a;
    a.feat = st.in32(feat, (size_t)P * V * D), a.targets = st.in32(targets, (size_t)T * D), a.src = st.in32(src, (size_t)V * D);
    const auto dw = st.in32(weights, W.size() * T);
    if (islands > 0) a.isl.weights = dw, a.isl.W = st.in32(W.data(), islands), a.isl.pop = pop, a.isl.row0 = row0;
    else a.weights = dw, a.W = W[0];
    a.P = P, a.V = V, a.T = T, a.D = D, a.streamed = streamed;
    const auto dvs = st.poisoned<float>((size_t)P * V), dss = st.poisoned<float>((size_t)P * T), ds = st.poisoned<float>(P);
    a.view_sim = dvs, a.set_sim = dss, a.sim = ds;
    TRY(st.run([&] { return accepted(launch_cosine_set(a, 0), refusal); }));
    if (view_sim) TRY(st.fetch(view_sim, dvs));
    if (set_sim) TRY(st.fetch(set_sim, dss));
    return st.fetch(sim, ds);
}
static const float ONE_WEIGHT[1] = {1.f};      // a single target is the set of one entry of weight 1

extern "C" int glass_op_cosine(int32_t device, int32_t P, int32_t D, const float* feat, const float* target, float* sim) {
    OPREQ(feat && target && sim && P > 0 && D > 0, "bad argument");
    return cosine_op(device, P, 1, 1, D, feat, target, ONE_WEIGHT, 0, 0, 0, nullptr, false, "cosine_set refused the shape", nullptr, nullptr, sim);
}

extern "C" int glass_op_cosine_views(int32_t device, int32_t P, int32_t V, int32_t D, const float* feat, const float* target, float* view_sim,
                                     float* sim) {
    OPREQ(feat && target && view_sim && sim && P > 0 && V > 0 && D > 0, "bad argument");
    OPREQ(V <= GLASS_PROMPT_MAX_VIEWS, "cosine_set: V and T must be in [1, 16]");
    return cosine_op(device, P, V, 1, D, feat, target, ONE_WEIGHT, 0, 0, 0, nullptr, false, "cosine_set refused the shape", view_sim, nullptr, sim);
}

extern "C" int glass_op_assemble_F(int32_t device, int32_t P, int32_t n_obj, const float* sim, const float* dis, float* F) {
    OPREQ(sim && F && P > 0 && (n_obj == 1 || (n_obj == 2 && dis)), "bad argument (n_obj 1, or 2 with dis)");
    Stage st(device);
    AssembleF a;
    a.sim = st.in32(sim, P), a.dis = n_obj == 2 ? st.in32(dis, P) : Buf<float>(), a.P = P, a.n_obj = n_obj;
    const auto dF = st.poisoned<float>((size_t)P * n_obj, 4);
    a.F = dF;
    TRY(st.run([&] { return accepted(launch_assemble_F(a, 0), "assemble_F refused the layout"); }));
    TRY(st.intact(dF, "assemble_F stored past row P"));
    return st.fetch(F, dF);
}

extern "C" int glass_op_cosine_set(int32_t device, int32_t P, int32_t V, int32_t T, int32_t D, const float* feat, const float* targets,
                                   const float* weights, float* view_sim, float* set_sim, float* sim) {
    OPREQ(feat && targets && weights && view_sim && set_sim && sim && P > 0 && D > 0, "bad argument");
    OPREQ(V >= 1 && V <= GLASS_PROMPT_MAX_VIEWS && T >= 1 && T <= GLASS_PROMPT_MAX, "cosine_set: V and T must be in [1, 16]");
    return cosine_op(device, P, V, T, D, feat, targets, weights, 0, 0, 0, nullptr, false, "cosine_set refused the shape", view_sim, set_sim, sim);
}

// the cosine with an island table: row p takes row (row0 + p) / pop of weights [islands, T] (include/glass.h "Device search: islands")
extern "C" int glass_op_cosine_set_islands(int32_t device, int32_t P, int32_t V, int32_t T, int32_t D, const float* feat, const float* targets,
                                           const float* weights, int32_t islands, int32_t pop, int32_t row0, float* view_sim, float* set_sim, float* sim) {
    OPREQ(feat && targets && weights && view_sim && set_sim && sim && P > 0 && D > 0, "bad argument");
    OPREQ(V >= 1 && V <= GLASS_PROMPT_MAX_VIEWS && T >= 1 && T <= GLASS_PROMPT_MAX, "cosine_set: V and T must be in [1, 16]");
    OPREQ(islands >= 1 && islands <= GLASS_SEARCH_MAX_ISLANDS && pop >= 1 && row0 >= 0 && (long long)row0 + P <= (long long)islands * pop,
          "cosine_set_islands: rows [row0, row0 + P) must lie inside the islands * pop rows, islands in [1, 64]");
    return cosine_op(device, P, V, T, D, feat, targets, weights, islands, pop, row0, nullptr, false, "cosine_set refused the shape", view_sim, set_sim, sim);
}

extern "C" int glass_op_assemble_F_set(int32_t device, int32_t P, int32_t K, const float* set_sim, const float* weights, const float* dis,
                                       const float* lp, float* F) {
    OPREQ(set_sim && weights && F && P > 0 && K >= 1 && K <= GLASS_PROMPT_MAX, "bad argument (K in [1, 16])");
    Stage st(device);
    const int n_obj = K + (dis ? 1 : 0) + (lp ? 1 : 0);
    AssembleF a;
    a.set_sim = st.in32(set_sim, (size_t)P * K), a.weights = st.in32(weights, K), a.K = K, a.dis = st.in32(dis, P), a.lp = st.in32(lp, P);
    a.P = P, a.n_obj = n_obj;
    const auto dF = st.poisoned<float>((size_t)P * n_obj, 4);
    a.F = dF;
    TRY(st.run([&] { return accepted(launch_assemble_F(a, 0), "assemble_F_set refused the layout"); }));
    TRY(st.intact(dF, "assemble_F_set stored past row P"));
    return st.fetch(F, dF);
}

extern "C" int glass_op_cosine_set_dir(int32_t device, int32_t P, int32_t V, int32_t T, int32_t D, const float* feat, const float* targets,
                                       const float* weights, const float* src, int32_t streamed, float* view_sim, float* set_sim, float* sim) {
    OPREQ(feat && targets && weights && src && view_sim && set_sim && sim && P > 0 && V > 0 && T > 0 && D > 0, "bad argument");
    OPREQ((int64_t)P * V * D < (1LL << 31) && (int64_t)T * D < (1LL << 31), "cosine_set_dir: operand too large");
    return cosine_op(device, P, V, T, D, feat, targets, weights, 0, 0, 0, src, streamed != 0, "cosine_set_dir refused the shape (V and T must be in [1, 16])",
                     view_sim, set_sim, sim);
}

extern "C" int glass_op_latent_anchor(int32_t device, int32_t P, int32_t n_lat, int32_t L, int32_t layered, const float* w, const float* a, float* d) {
    OPREQ(w && a && d && P > 0 && n_lat > 0 && L > 0, "bad argument");
    OPREQ((int64_t)P * n_lat * L < (1LL << 31), "latent_anchor: operand too large");
    Stage st(device);
    const int nl = layered ? n_lat : 1;      // rows of w per candidate
    const auto dw = st.in32(w, (size_t)P * nl * L), da = st.in32(a, (size_t)n_lat * L);
    const auto dd = st.poisoned<float>(P, 4);
    TRY(st.run([&] {
        return accepted(launch_latent_anchor(dw, (long long)nl * L, layered ? L : 0, da, n_lat, L, P, dd, 0),
                        "latent_anchor refused the shape (n_lat in [1, 64], L in [1, 65536])");
    }));
    TRY(st.intact(dd, "latent_anchor stored past row P"));
    return st.fetch(d, dd);
}

extern "C" int glass_op_dlatent_subspace(int32_t device, const float* c, int32_t P, int32_t G, int32_t K, const int32_t* layer_group, int32_t n_lat,
                                         int32_t L, const float* basis, const float* base, float* out) {
    OPREQ(layer_group && P > 0, "bad argument");
    TRY(glass_subspace_supported(n_lat, L, G, K, layer_group, nullptr, 0));      // (first: an empty operand of a refused shape may be a null pointer)
    OPREQ(c && basis && base && out, "bad argument");
    OPREQ((int64_t)P * G * K < (1LL << 31) && (int64_t)P * n_lat * L < (1LL << 31), "dlatent_subspace: operand too large");
    Stage st(device);
    const auto dc = st.in32(c, (size_t)P * G * K), dB = st.in32(basis, (size_t)K * L), db = st.in32(base, (size_t)n_lat * L);
    const auto dg = st.in_i32(layer_group, n_lat);
    const auto dout = st.poisoned<float>((size_t)P * n_lat * L, 4 * (size_t)L);      // NaN: an element the launch does not write shows
    TRY(st.run([&] { return accepted(launch_dlatent_subspace(dc, P, G, K, dg, n_lat, L, dB, db, dout, 0), "dlatent_subspace refused the shape"); }));
    TRY(st.intact(dout, "dlatent_subspace stored past row P"));
    return st.fetch(out, dout);
}

extern "C" int glass_op_image_patches(int32_t device, int32_t n, int32_t S, int32_t ps, int32_t ld, const float* img, float sentinel,
                                      float* patches) {
    OPREQ(img && patches && n > 0 && S > 0 && ps > 0 && S % ps == 0 && ld >= 3 * ps * ps, "bad argument (S % ps == 0, ld >= 3 ps ps)");
    Stage st(device);
    const int G = S / ps;
    const auto di = st.in32(img, (size_t)n * 3 * S * S);
    const auto dp = st.in16(std::vector<_Float16>((size_t)n * G * G * ld, (_Float16)sentinel));      // what the kernel does not write keeps the sentinel
    TRY(st.run([&] { launch_image_patches(di, n, S, ps, ld, dp, 0); }));
    return st.fetch(patches, dp);
}

extern "C" int glass_op_rn_token0_rows(int32_t device, int32_t B, int32_t T, int32_t C, const float* att, float* out) {
    OPREQ(att && out && B > 0 && T > 0 && C > 0, "bad argument");
    Stage st(device);
    const auto da = st.in16(att, (size_t)B * T * C);
    const auto dout = st.poisoned<float>((size_t)B * C);
    TRY(st.run([&] { launch_rn_token0_rows(da, B, T, C, dout, 0); }));
    return st.fetch(out, dout);
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
// Every output and scratch buffer below is poisoned (an element no thread stores comes back as NaN) and guarded on both sides (a store outside
// it fails the op, intact_named): image-shaped outputs by CONV_GUARD_ROWS image rows, gemm_tiled's rows by one 128-row m tile, the tokens by
// one token row.  Each op clears g_last_kernel and records the symbol it launched (glass_op_last_kernel).
namespace {
constexpr size_t GEMM_GUARD_ROWS = 128;      // one m tile of gemm_tiled
}

extern "C" int glass_op_rn_avgpool(int32_t device, int32_t B, int32_t H, int32_t W, int32_t C, const float* x, float* out) {
    OPREQ(x && out && B > 0 && H > 0 && W > 0 && C > 0, "bad argument");
    g_last_kernel.clear();
    Stage st(device);
    const auto dx = st.in16(x, (size_t)B * H * W * C);
    const size_t gy = CONV_GUARD_ROWS * (W / 2) * C;
    const auto dy = st.poisoned<half_t>((size_t)B * (H / 2) * (W / 2) * C, gy, gy);
    TRY(st.run([&] { return accepted(launch_rn_avgpool2(dx, B, H, W, C, dy, 0) && ran_kernel("rn_avgpool2_kernel"), "rn_avgpool2: refused (even H and W, C a multiple of 8)"); }));
    TRY(st.intact_named(dy, "rn_avgpool: out"));
    return st.fetch(out, dy);
}

extern "C" int glass_op_rn_stem_conv1(int32_t device, int32_t B, int32_t S, int32_t C1, const float* img, const float* w, const float* bn_a,
                                      const float* bn_s, float* out) {
    OPREQ(img && w && bn_a && bn_s && out && B > 0 && S > 0 && S % 32 == 0 && C1 > 0, "bad argument (S a multiple of 32)");
    g_last_kernel.clear();
    Stage st(device);
    const size_t ni = (size_t)B * 3 * S * S;
    std::vector<_Float16> wt((size_t)27 * C1);
    for (int o = 0; o < C1; ++o)
        for (int k = 0; k < 27; ++k) wt[(size_t)k * C1 + o] = (_Float16)w[(size_t)o * 27 + k];
    const auto dimg = st.in32(img, ni);
    const auto dp = st.poisoned<half_t>(ni);      // (the patch operand: a pixel launch_image_patches leaves out reaches the conv as NaN)
    const auto dw = st.in16(wt);
    const auto da = st.in32(bn_a, C1), ds = st.in32(bn_s, C1);
    const size_t gy = CONV_GUARD_ROWS * (S / 2) * C1;
    const auto dy = st.poisoned<half_t>((size_t)B * (S / 2) * (S / 2) * C1, gy, gy);
    TRY(st.run([&]() -> int {
        launch_image_patches(dimg, B, S, 32, 3072, dp, 0);      // (the operand's preparation: not the op's kernel, not recorded)
        return accepted(launch_rn_stem_conv1(dp, dw, da, ds, B, S, C1, dy, 0) && ran_kernel("rn_stem_conv1_kernel"), "rn_stem_conv1: refused (C1 a multiple of 8)");
    }));
    TRY(st.intact_named(dy, "rn_stem_conv1: out"));
    return st.fetch(out, dy);
}

extern "C" int glass_op_rn_conv_bn(int32_t device, int32_t form, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t relu,
                                   const float* x, const float* w, const float* bn_a, const float* bn_s, const float* res, float* out) {
    OPREQ(x && w && bn_a && bn_s && out && B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "bad argument");
    OPREQ((form == 0 && (KS == 1 || KS == 3)) || (form == 1 && KS == 3), "rn_conv_bn: form 0 takes KS 1 or 3, form 1 KS 3");
    OPREQ(KS == 1 || (relu && !res), "rn_conv_bn: the 3 x 3 forms are conv + BN + ReLU without a residual");
    g_last_kernel.clear();
    Stage st(device);
    const int M = B * H * W, Mp = std::max(M, 64);
    RnConv c;
    c.cin = Cin; c.cout = Cout; c.ks = KS;
    c.w = st.in16(rn_pack_conv(w, Cout, Cin, KS));
    c.a = st.in32(bn_a, Cout);
    c.s = st.in32(bn_s, Cout);
    // M rows of data in buffers of max(M, 64) rows.  The tail rows M .. Mp - 1 hold the 0xFF poison (fp16 NaN), not zeros: in the engine they hold
    // whatever the layer before left in its ping-pong buffer.  The 1 x 1 form runs gemm_tiled over all Mp rows, so it reads these rows of x and
    // res and stores them; the gather form may fetch them for lanes past M.  None of the M rows that come back may depend on them: a valid
    // row that does is NaN here.
    auto padded = [&](const float* src, size_t rowlen) {
        std::vector<_Float16> h((size_t)Mp * rowlen);
        memset(h.data(), 0xFF, h.size() * sizeof(_Float16));
        for (size_t i = 0; i < (size_t)M * rowlen; ++i) h[i] = (_Float16)src[i];
        return st.in16(h);
    };
    const auto dx = padded(x, Cin);
    const auto dr = res ? padded(res, Cout) : Buf<half_t>{};
    // guard: the taller of CONV_GUARD_ROWS image rows and one m tile of gemm_tiled, behind the max(M, 64) rows and in front of them
    const size_t gy = std::max(CONV_GUARD_ROWS * W, GEMM_GUARD_ROWS) * Cout;
    const auto dy = st.poisoned<half_t>((size_t)Mp * Cout, gy, gy);
    TRY(st.run([&] {
        if (form == 1) return accepted(ran_kernel(launch_rn_conv3x3(dx, c.w, c.a, c.s, B, H, W, Cin, Cout, dy, 0)) != nullptr, "rn_conv3x3: refused (Cin % 16, Cout % 32)");
        const GemmParams g = KS == 1 ? rn_gemm_1x1(dx, c, M, H * W, dr, relu, dy) : rn_gemm_3x3(dx, c, B, H, W, dy);
        return accepted(ran_kernel(launch_gemm_tiled(g, 0)) != nullptr, "rn_conv_bn: gemm_tiled refused the shape (Cin and Cout multiples of 64)");
    }));
    TRY(st.intact_named(dy, "rn_conv_bn: out"));
    return st.fetch(out, dy, (size_t)M * Cout);      // (the rows of data)
}

extern "C" int glass_op_rn_tokens(int32_t device, int32_t B, int32_t HW, int32_t C, const float* x, const float* pos, float* out) {
    OPREQ(x && pos && out && B > 0 && HW > 0 && C > 0, "bad argument");
    g_last_kernel.clear();
    Stage st(device);
    const auto dx = st.in16(x, (size_t)B * HW * C);
    const auto dp = st.in32(pos, (size_t)(HW + 1) * C);
    const auto dy = st.poisoned<half_t>((size_t)B * (HW + 1) * C, C, C);      // (guard: one token row)
    TRY(st.run([&] {
        launch_rn_attnpool_tokens(dx, dp, B, HW, C, dy, 0);
        ran_kernel("rn_attnpool_tokens_kernel");
    }));
    TRY(st.intact_named(dy, "rn_tokens: out"));
    return st.fetch(out, dy);
}

// ---- perceptual objective (lpips.hip) ----
extern "C" int glass_op_lpips_input(int32_t device, int32_t B, int32_t R, int32_t S, const float* y, float* out) {
    OPREQ(y && out && B > 0 && R > 0 && S > 0, "bad argument");
    g_last_kernel.clear();
    Stage st(device);
    const auto dy = st.in32(y, (size_t)B * 3 * R * R);
    const size_t go = CONV_GUARD_ROWS * S * 4;
    const auto dout = st.poisoned<half_t>((size_t)B * S * S * 4, go, go);
    TRY(st.run([&] { return accepted(launch_lpips_input(dy, B, R, S, dout, 0) && ran_kernel("lpips_input_kernel"), "lpips_input: refused (R a multiple of S, box R / S at most 8)"); }));
    TRY(st.intact_named(dout, "lpips_input: out"));
    return st.fetch(out, dout);
}

extern "C" int glass_op_vgg_conv1(int32_t device, int32_t B, int32_t S, const float* x, const float* w, const float* bias, float* out) {
    OPREQ(x && w && bias && out && B > 0 && S > 0, "bad argument");
    g_last_kernel.clear();
    Stage st(device);
    std::vector<_Float16> wt((size_t)27 * 64);
    for (int o = 0; o < 64; ++o)
        for (int k = 0; k < 27; ++k) wt[(size_t)k * 64 + o] = (_Float16)w[(size_t)o * 27 + k];
    const auto dx = st.in16(x, (size_t)B * S * S * 4);
    const auto dw = st.in16(wt);
    const auto db = st.in32(bias, 64);
    const size_t gy = CONV_GUARD_ROWS * S * 64;
    const auto dy = st.poisoned<half_t>((size_t)B * S * S * 64, gy, gy);
    TRY(st.run([&] { return accepted(launch_vgg_conv1(dx, dw, db, B, S, dy, 0) && ran_kernel("vgg_conv1_kernel"), "vgg_conv1: refused"); }));
    TRY(st.intact_named(dy, "vgg_conv1: out"));
    return st.fetch(out, dy);
}

extern "C" int glass_op_maxpool2(int32_t device, int32_t B, int32_t H, int32_t W, int32_t C, const float* x, float* out) {
    OPREQ(x && out && B > 0 && H > 0 && W > 0 && C > 0, "bad argument");
    g_last_kernel.clear();
    Stage st(device);
    const auto dx = st.in16(x, (size_t)B * H * W * C);
    const size_t gy = CONV_GUARD_ROWS * (W / 2) * C;
    const auto dy = st.poisoned<half_t>((size_t)B * (H / 2) * (W / 2) * C, gy, gy);
    TRY(st.run([&] { return accepted(launch_maxpool2(dx, B, H, W, C, dy, 0) && ran_kernel("maxpool2_kernel"), "maxpool2: refused (even H and W, C a multiple of 8)"); }));
    TRY(st.intact_named(dy, "maxpool2: out"));
    return st.fetch(out, dy);
}

extern "C" int glass_op_lpips_head(int32_t device, int32_t n, int32_t HW, int32_t C, int32_t shared_x1, const float* x0, const float* x1, const float* lin,
                                   float* out) {
    OPREQ(x0 && x1 && lin && out && n > 0 && HW > 0 && C > 0, "bad argument");
    Stage st(device);
    const size_t map = (size_t)HW * C, nblk = ((size_t)HW + GLASS_LPIPS_PIXB - 1) / GLASS_LPIPS_PIXB;
    const auto d0 = st.in16(x0, (size_t)n * map), d1 = st.in16(x1, (shared_x1 ? 1 : (size_t)n) * map);
    const auto dl = st.in32(lin, C);
    const auto part = st.poisoned<float>((size_t)n * nblk);      // NaN: a workgroup sum the head does not write shows in the distance
    const auto dd = st.poisoned<float>(n);
    TRY(st.run([&] { return accepted(launch_lpips_head(d0, d1, shared_x1 ? 0 : (long long)map, dl, n, HW, C, part, 1, dd, 0), "lpips_head: refused (C one of 64, 128, 256, 512)"); }));
    return st.fetch(out, dd);
}

extern "C" int glass_op_mfma_probe(int32_t device, const float* a, const float* b, float* d) {
    OPREQ(a && b && d, "null argument");
    Stage st(device);
    const auto da = st.in16(a, 32 * 16), db = st.in16(b, 16 * 32);
    const auto dd = st.raw<float>(32 * 32);
    TRY(st.run([&] { hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, 0, da.p, db.p, dd.p); }));
    return st.fetch(d, dd);
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
    TRY(glass_search_supported(pop, n_var, 1, GLASS_SEARCH_NSGA2));
    OPREQ(rows > 0 && row0 >= 0 && row0 + rows <= pop, "ga_vary: [row0, row0 + rows) must lie inside the pop offspring rows");
    Stage st(device);
    const auto dX = st.in32(X, (size_t)pop * n_var);
    const auto dr = st.in_i32(rank, pop);
    const auto dc = st.in(cd, pop);
    const auto dO = st.poisoned<float>((size_t)pop * n_var, 4);      // every offspring row, and four guard elements behind them
    GaParams g;
    g.pop = pop; g.xl = xl; g.xu = xu; g.eta_c = eta_c; g.eta_m = eta_m; g.prob_m = prob_m; g.seed = seed;
    TRY(st.run([&] { return accepted(launch_ga_vary(dX, dr, dc, g, 1, n_var, 0, generation, row0, rows, GA_VARY_REAL, dO, 0), "ga_vary refused the shape"); }));
    TRY(st.intact(dO, "ga_vary stored past the last row"));
    return st.fetch(out, dO, (size_t)rows * n_var, (size_t)row0 * n_var);
}

extern "C" int glass_op_ga_vary_mixed(int32_t device, int32_t pop, int32_t n_real, int32_t n_bits, const float* X, const int32_t* rank, const double* cd,
                                      double xl, double xu, double eta_c, double eta_m, double prob_m, double prob_x, double prob_flip, uint64_t seed,
                                      int32_t generation, int32_t row0, int32_t rows, float* out) {
    OPREQ(X && rank && cd && out, "null argument");
    OPREQ(n_real >= 0 && n_bits >= 0 && n_bits <= (1 << 20), "ga_vary_mixed: bad sizes");
    const int n_var = n_real + n_bits;
    TRY(glass_search_supported(pop, n_var, 1, GLASS_SEARCH_NSGA2));
    OPREQ(rows > 0 && row0 >= 0 && row0 + rows <= pop, "ga_vary_mixed: [row0, row0 + rows) must lie inside the pop offspring rows");
    Stage st(device);
    const auto dX = st.in32(X, (size_t)pop * n_var);
    const auto dr = st.in_i32(rank, pop);
    const auto dc = st.in(cd, pop);
    const auto dO = st.poisoned<float>((size_t)pop * n_var, 4);      // every offspring row, and four guard elements behind them
    GaParams g;
    g.pop = pop; g.xl = xl; g.xu = xu; g.eta_c = eta_c; g.eta_m = eta_m; g.prob_m = prob_m; g.seed = seed;
    g.prob_x = prob_x; g.prob_flip = prob_flip;
    TRY(st.run([&] {
        return accepted(launch_ga_vary(dX, dr, dc, g, 1, n_real, n_bits, generation, row0, rows, GA_VARY_BOTH, dO, 0),
                        "ga_vary_mixed refused the shape (n_real >= 1, n_bits in [1, 4096])");
    }));
    TRY(st.intact(dO, "ga_vary_mixed stored past the last row"));
    return st.fetch(out, dO, (size_t)rows * n_var, (size_t)row0 * n_var);
}

extern "C" int glass_op_ga_duplicates(int32_t device, int32_t pop, int32_t n_off, int32_t n_var, const float* X, const float* Xoff, int32_t* flags) {
    OPREQ(X && Xoff && flags, "null argument");
    OPREQ(pop >= 1 && pop <= GLASS_SEARCH_MAX_POP && n_off >= 1 && n_off <= GLASS_SEARCH_MAX_POP && n_var >= 1, "ga_duplicates: pop and n_off in [1, 1024]");
    Stage st(device);
    const auto dX = st.in32(X, (size_t)pop * n_var), dO = st.in32(Xoff, (size_t)n_off * n_var);
    const auto df = st.poisoned<int32_t>(n_off, 4);
    TRY(st.run([&] { return accepted(launch_ga_duplicates(dX, dO, 1, pop, n_off, n_var, df, 0), "ga_duplicates refused the shape"); }));
    TRY(st.intact(df, "ga_duplicates stored past row n_off"));
    return st.fetch(flags, df);
}

extern "C" int glass_op_ga_survive(int32_t device, int32_t n_pop, int32_t n_off, int32_t n_obj, int32_t pop_out, int32_t nsga, const float* F,
                                   const int32_t* flags, int32_t* chosen, int32_t* rank, double* cd, float* F_out, int32_t* counts, int32_t n_var,
                                   const float* X, const float* Xoff, float* X_out) {
    OPREQ(F && chosen && rank && cd && F_out && counts, "null argument");
    OPREQ(n_pop >= 1 && n_off >= 0 && n_obj >= 1 && pop_out >= 1, "ga_survive: bad sizes");
    const bool gather = X != nullptr;
    OPREQ(!gather || (X_out && n_var >= 1 && (Xoff || n_off == 0)), "ga_survive: X needs Xoff, X_out and n_var");
    Stage st(device);
    const auto dF = st.in32(F, ((size_t)n_pop + n_off) * n_obj);
    const auto dfl = st.in_i32(n_off ? flags : nullptr, n_off);
    const auto dch = st.poisoned<int32_t>(pop_out, 4);
    const auto drk = st.raw<int32_t>(pop_out), dcn = st.raw<int32_t>(3);      // (counts [1][3]: the third is the migration's)
    const auto dcd = st.raw<double>(pop_out);
    Buf<float> dX, dO, dXo;
    if (gather) {
        dX = st.in32(X, (size_t)n_pop * n_var);
        dO = st.in32(n_off ? Xoff : nullptr, (size_t)n_off * n_var);
        dXo = st.poisoned<float>((size_t)pop_out * n_var);
    }
    TRY(st.run([&]() -> int {
        OPREQ(launch_ga_survive(dF, dF + (size_t)n_pop * n_obj, dfl, 1, n_pop, n_off, n_obj, pop_out, nsga, 0, dch, drk, dcd, dcn, 0),
              "ga_survive refused the shape (up to 2048 merged rows, 6 objectives, pop_out <= 1024 and <= the merged rows)");
        if (gather) launch_ga_gather(dX, dO, dch, 1, n_pop, pop_out, n_var, dXo, 0);
        return GLASS_OK;
    }));
    TRY(st.intact(dch, "ga_survive stored past slot pop_out"));
    TRY(st.fetch(chosen, dch));
    TRY(st.fetch(rank, drk));
    TRY(st.fetch(cd, dcd));
    TRY(st.fetch(F_out, dF, (size_t)pop_out * n_obj));
    TRY(st.fetch(counts, dcn, 2));
    return gather ? st.fetch(X_out, dXo) : GLASS_OK;
}

// the whole migration of include/glass.h "Device search: islands": ga_migrate_kernel in place, the gated ranking of the islands that accepted a
// row and the gather.  X [islands pop, n_var], F [islands pop, n_obj], rank, cd as survival left them -> the same four after the migration,
// accepted int32 [islands]
extern "C" int glass_op_ga_migrate(int32_t device, int32_t islands, int32_t pop, int32_t n_var, int32_t n_obj, int32_t nsga, int32_t migrants,
                                   const float* X, const float* F, const int32_t* rank, const double* cd, float* X_out, float* F_out, int32_t* rank_out,
                                   double* cd_out, int32_t* accepted) {
    OPREQ(X && F && rank && cd && X_out && F_out && rank_out && cd_out && accepted, "null argument");
    TRY(glass_search_islands_supported(islands, pop, n_var, n_obj, nsga ? GLASS_SEARCH_NSGA2 : GLASS_SEARCH_GA, 1, migrants));
    OPREQ(islands >= 2, "ga_migrate: a ring has at least two islands");
    const size_t R = (size_t)islands * pop;
    Stage st(device);
    const auto dX = st.in32(X, R * n_var), dF = st.in32(F, R * n_obj);
    const auto dr = st.in_i32(rank, R);
    const auto dc = st.in(cd, R);
    const std::vector<int32_t> zero((size_t)3 * islands, 0);
    const auto dcn = st.in_i32(zero.data(), zero.size());
    const auto dch = st.poisoned<int32_t>(R, 4);
    const auto dXo = st.poisoned<float>(R * n_var, 4);
    TRY(st.run([&]() -> int {
        OPREQ(launch_ga_migrate(dX, dF, dr, dc, islands, pop, n_var, n_obj, migrants, dcn, 0), "ga_migrate refused the shape");
        OPREQ(launch_ga_survive(dF, nullptr, nullptr, islands, pop, 0, n_obj, pop, nsga, 1, dch, dr, dc, dcn, 0), "ga_survive refused the shape");
        launch_ga_gather(dX, nullptr, dch, islands, pop, pop, n_var, dXo, 0);
        return GLASS_OK;
    }));
    TRY(st.intact(dch, "ga_survive stored past the last island's slots"));
    TRY(st.intact(dXo, "ga_gather stored past the last island's rows"));
    TRY(st.fetch(X_out, dXo, R * n_var));
    TRY(st.fetch(F_out, dF));
    TRY(st.fetch(rank_out, dr));
    TRY(st.fetch(cd_out, dc));
    std::vector<int32_t> cn((size_t)3 * islands);
    TRY(st.fetch(cn.data(), dcn));
    for (int i = 0; i < islands; ++i) accepted[i] = cn[(size_t)3 * i + 2];
    return GLASS_OK;
}

// ---- device search: sep-CMA-ES (cmaes.hip) -----------------------------------------------------------------------------------------
namespace {
// the device side of a CMA state for one op: state [4][n] (m, d, p_sigma, p_c), the weights, the scratch and the scalars
struct CmaStage {
    CmaState s = {};
    Buf<double> state, w, scratch, part;
    Buf<CmaScalars> sc;
    Buf<int32_t> order, counts;
    Buf<float> best;
    CmaStage(Stage& st, int lambda, int n, const double* state_in, const CmaScalars& scalars, const float* best_in) {
        std::vector<double> wh((size_t)std::max(lambda / 2, 1));
        cma_weights(lambda, wh.data());
        state = st.in(state_in, (size_t)4 * n);
        w = st.in(wh.data(), wh.size());
        scratch = st.poisoned<double>((size_t)2 * n);
        part = st.poisoned<double>((size_t)cma_blocks(n));
        sc = st.in(&scalars, 1);
        order = st.poisoned<int32_t>((size_t)lambda, 4);
        counts = st.poisoned<int32_t>(2);
        best = st.poisoned<float>((size_t)n, 4);
        if (best_in) st.put(best, 0, best_in, (size_t)n);
        s.m = state.at(0); s.d = state.at((size_t)n); s.ps = state.at((size_t)2 * n); s.pc = state.at((size_t)3 * n);
        s.w = w; s.yw = scratch.at(0); s.s2 = scratch.at((size_t)n); s.part = part; s.sc = sc; s.order = order; s.best_X = best; s.counts = counts;
    }
};
}  // namespace

extern "C" int glass_op_cma_sample(int32_t device, int32_t lambda, int32_t n, const double* mean, const double* diag, double sigma, double xl, double xu,
                                   uint64_t seed, int32_t generation, int32_t row0, int32_t rows, float* X) {
    OPREQ(mean && diag && X, "null argument");
    TRY(glass_search_supported(lambda, n, 1, GLASS_SEARCH_CMAES));
    OPREQ(rows > 0 && row0 >= 0 && row0 + rows <= lambda, "cma_sample: [row0, row0 + rows) must lie inside the lambda rows");
    std::vector<double> state((size_t)4 * n, 0.0);
    memcpy(state.data(), mean, (size_t)n * sizeof(double));
    memcpy(state.data() + n, diag, (size_t)n * sizeof(double));
    CmaScalars sc = {};
    sc.sigma = sigma;
    Stage st(device);
    CmaStage cs(st, lambda, n, state.data(), sc, nullptr);
    const auto dX = st.poisoned<float>((size_t)lambda * n, 4);      // every row preloaded from the caller's, and four guard elements behind them
    st.put(dX, 0, X, (size_t)lambda * n);
    const CmaParams p = cma_params(lambda, n, xl, xu, seed);
    TRY(st.run([&] { return accepted(launch_cma_sample(cs.s, p, generation, row0, rows, dX, 0), "cma_sample refused the shape"); }));
    TRY(st.intact(dX, "cma_sample stored past the last row"));
    return st.fetch(X, dX);
}

extern "C" int glass_op_cma_rank(int32_t device, int32_t lambda, const float* F, float best_F, int32_t* order, int32_t* info, float* best_F_out) {
    OPREQ(F && order && info && best_F_out, "null argument");
    TRY(glass_search_supported(lambda, 1, 1, GLASS_SEARCH_CMAES));
    const double zero[4] = {0.0, 1.0, 0.0, 0.0};
    CmaScalars sc = {};
    sc.sigma = 1.0;
    sc.best_F = best_F;
    sc.best_src = -1;
    Stage st(device);
    CmaStage cs(st, lambda, 1, zero, sc, nullptr);
    const auto dF = st.in32(F, (size_t)lambda);
    const CmaParams p = cma_params(lambda, 1, -1.0, 1.0, 0);
    TRY(st.run([&] { return accepted(launch_cma_rank(cs.s, p, dF, 0), "cma_rank refused the shape"); }));
    TRY(st.intact(cs.order, "cma_rank stored past slot lambda"));
    TRY(st.fetch(order, cs.order));
    TRY(st.fetch(&sc, cs.sc));
    int32_t counts[2];
    TRY(st.fetch(counts, cs.counts));
    info[0] = sc.finite; info[1] = sc.updated; info[2] = sc.best_src; info[3] = sc.skipped; info[4] = counts[1];
    *best_F_out = sc.best_F;
    return GLASS_OK;
}

extern "C" int glass_op_cma_update(int32_t device, int32_t lambda, int32_t n, const float* X, const float* F, double* state, double* scalars_d,
                                   int32_t* scalars_i, double xl, double xu, int32_t generation, float* best_X, float* best_F, int32_t* order) {
    OPREQ(X && F && state && scalars_d && scalars_i && best_X && best_F && order, "null argument");
    TRY(glass_search_supported(lambda, n, 1, GLASS_SEARCH_CMAES));
    OPREQ(generation >= 0, "cma_update: a generation is 0, 1, ...");
    CmaScalars sc = {};
    sc.sigma = scalars_d[0]; sc.ps_norm = scalars_d[1];
    sc.h = scalars_i[0]; sc.finite = scalars_i[1]; sc.updated = scalars_i[2]; sc.skipped = scalars_i[3]; sc.updates = scalars_i[4];
    sc.best_F = *best_F;
    sc.best_src = -1;
    Stage st(device);
    CmaStage cs(st, lambda, n, state, sc, best_X);
    const auto dX = st.in32(X, (size_t)lambda * n), dF = st.in32(F, (size_t)lambda);
    const CmaParams p = cma_params(lambda, n, xl, xu, 0);
    TRY(st.run([&]() -> int {
        OPREQ(launch_cma_rank(cs.s, p, dF, 0), "cma_rank refused the shape");
        OPREQ(launch_cma_update(cs.s, p, dX, generation, 0), "cma_update refused the shape");
        return GLASS_OK;
    }));
    TRY(st.intact(cs.order, "cma_rank stored past slot lambda"));
    TRY(st.intact(cs.best, "cma_best stored past variable n"));
    TRY(st.fetch(state, cs.state));
    TRY(st.fetch(order, cs.order));
    TRY(st.fetch(best_X, cs.best));
    TRY(st.fetch(&sc, cs.sc));
    scalars_d[0] = sc.sigma; scalars_d[1] = sc.ps_norm;
    scalars_i[0] = sc.h; scalars_i[1] = sc.finite; scalars_i[2] = sc.updated; scalars_i[3] = sc.skipped; scalars_i[4] = sc.updates; scalars_i[5] = sc.best_src;
    *best_F = sc.best_F;
    return GLASS_OK;
}
