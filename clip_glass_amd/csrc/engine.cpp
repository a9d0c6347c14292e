// engine.cpp — C ABI (include/glass.h) + orchestration of the fitness pass.
//
// Host-side mirror of problem.py:14-29 / generator.py:29-60 / models.py:108-129:
//   latents -> mapping -> styles/demod -> [per chunk: synthesis -> toRGB/skip -> resize -> D] -> CLIP -> F
// One engine per (process, GPU); one private stream; weights repacked once in finalize().
// Here: lifecycle, weight packing, buffers and the pass.  The networks' host code: stylegan2.cpp, clip.cpp, gpt2_host.cpp, biggan.cpp.
#include "engine.h"

#include <math.h>
#include <cmath>
#include <string.h>

#include <stdlib.h>

static thread_local std::string g_err;
void glass_set_error(const std::string& s) { g_err = s; }
extern "C" const char* glass_last_error(void) { return g_err.c_str(); }
extern "C" const char* glass_version(void) { return "clip-glass-amd 0.1 (gfx950)"; }

// ------------------------------------------------------------------------------------
// weight repacking (reference layouts -> kernel layouts)
// ------------------------------------------------------------------------------------
// plain conv: W[o][i][ky][kx] * coef -> [tap][o][i_pad] fp16
void glass_pack_conv(const float* W, int cout, int cin, int ks, int cin_pad, std::vector<_Float16>& out) {
    const float coef = 1.0f / sqrtf((float)cin * ks * ks);  // modules.py:103-108 (gain 1, lr_mul 1)
    out.assign((size_t)ks * ks * cout * cin_pad, (_Float16)0.f);
    for (int o = 0; o < cout; ++o)
        for (int i = 0; i < cin; ++i)
            for (int t = 0; t < ks * ks; ++t)
                out[((size_t)t * cout + o) * cin_pad + i] = (_Float16)(W[((size_t)o * cin + i) * ks * ks + t] * coef);
}

// up conv: conv_transpose2d(stride 2, 3x3) followed by the 4x4 FIR (gain 4, pad 1)
// (modules.py:1089-1139) == 3x3 conv (pad 1) with 4 phase kernels + depth-to-space.
//   1-D: t[q] = sum_i x[i] w[q-2i];  out[p] = sum_j f[j] t[p+j-1]  =>  out[p] = sum_i x[i] g[p-2i],
//   g[r] = sum_j f[j] w[r+j-1], r in [-2,3];  out[2m+ph] = sum_{d=0..2} x[m-1+d] g[(2+ph)-2d].
// Output layout [tap = dy*3+dx][n = (py*2+px)*cout + o][i].
int glass_fold_upconv(const float* W, int cout, int cin, std::vector<_Float16>& out) {
    const float coef = 1.0f / sqrtf((float)cin * 9.f);
    const float f1[4] = {1.f, 3.f, 3.f, 1.f};
    float F[4][4];
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) F[a][b] = f1[a] * f1[b] / 64.f * 4.f;  // modules.py:201-202, up_factor^2
    out.assign((size_t)9 * 4 * cout * cin, (_Float16)0.f);
    std::vector<float> g(36);
    for (int o = 0; o < cout; ++o)
        for (int i = 0; i < cin; ++i) {
            const float* w = W + ((size_t)o * cin + i) * 9;
            for (int ry = -2; ry <= 3; ++ry)
                for (int rx = -2; rx <= 3; ++rx) {
                    float s = 0.f;
                    for (int jy = 0; jy < 4; ++jy) {
                        const int ky = ry + jy - 1;
                        if (ky < 0 || ky > 2) continue;
                        for (int jx = 0; jx < 4; ++jx) {
                            const int kx = rx + jx - 1;
                            if (kx < 0 || kx > 2) continue;
                            s += F[jy][jx] * w[ky * 3 + kx];
                        }
                    }
                    g[(ry + 2) * 6 + (rx + 2)] = s * coef;
                }
            for (int py = 0; py < 2; ++py)
                for (int px = 0; px < 2; ++px)
                    for (int dy = 0; dy < 3; ++dy)
                        for (int dx = 0; dx < 3; ++dx) {
                            const int ry = (2 + py) - 2 * dy, rx = (2 + px) - 2 * dx;
                            out[((size_t)(dy * 3 + dx) * 4 * cout + (size_t)(py * 2 + px) * cout + o) * cin + i] =
                                (_Float16)g[(ry + 2) * 6 + (rx + 2)];
                        }
        }
    return 0;
}

std::vector<_Float16> to_half(const float* p, size_t n, float scale) {
    std::vector<_Float16> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (_Float16)(p[i] * scale);
    return v;
}
std::vector<float> scaled(const float* p, size_t n, float scale) {
    std::vector<float> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = p[i] * scale;
    return v;
}
// W[N][K] * coef -> Wt[K][N]
std::vector<float> transposed(const float* W, int N, int K, float coef) {
    std::vector<float> v((size_t)N * K);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) v[(size_t)k * N + n] = W[(size_t)n * K + k] * coef;
    return v;
}

// ------------------------------------------------------------------------------------
// create / destroy / load
// ------------------------------------------------------------------------------------
extern "C" int glass_engine_create(const glass_config* cfg, glass_engine** out) {
    REQUIRE(cfg && out, GLASS_ERR_ARG, "null argument");
    REQUIRE(cfg->n_blocks >= 0 && cfg->n_blocks <= GLASS_MAX_BLOCKS, GLASS_ERR_ARG, "n_blocks out of range");
    for (int i = 0; i < cfg->n_blocks; ++i) {
        const int ch = cfg->channels[i];    // the toRGB / fromRGB kernels are instantiated for these widths (kernels_misc.hip)
        REQUIRE(ch == 16 || ch == 32 || ch == 64 || ch == 128 || ch == 256 || ch == 512, GLASS_ERR_ARG,
                "channels must be one of 16, 32, 64, 128, 256, 512");
    }
    REQUIRE(cfg->latent_size > 0 && cfg->latent_size % 4 == 0, GLASS_ERR_ARG, "latent_size must be a multiple of 4");
    REQUIRE(cfg->batch_size > 0 && cfg->max_pop > 0, GLASS_ERR_ARG, "batch_size/max_pop must be positive");
    REQUIRE(cfg->max_pop % cfg->batch_size == 0, GLASS_ERR_ARG, "max_pop must be a multiple of batch_size");
    const bool lpips = cfg->lpips_size != 0;      // the perceptual objective (opt-in): its own last column unless lpips_lambda folds it into column 0
    REQUIRE(cfg->sim_columns >= 0 && cfg->sim_columns <= 4, GLASS_ERR_ARG, "sim_columns must be 0 or 1 (one similarity column) or 2 .. 4 (a pareto prompt set)");
    const int K = sim_columns(*cfg);              // similarity columns: 1 unless the engine is made for a pareto prompt set
    // the latent anchor (opt-in): its own rule, which counts every column; the rules below then see n_obj without the anchor's column
    if (int erc = glass_edit_supported(cfg->generator, cfg->n_blocks, cfg->sim_columns, cfg->use_discriminator, lpips && cfg->lpips_lambda == 0.f, cfg->anchor,
                                       cfg->anchor_lambda, cfg->n_obj))
        return erc;
    const int n_obj = cfg->n_obj - anchor_column(*cfg);
    if (K >= 2) {
        REQUIRE(!lpips || cfg->lpips_lambda == 0.f, GLASS_ERR_ARG,
                "lpips_lambda > 0 folds the distance into THE similarity column; with sim_columns >= 2 there is no single one: use lpips_lambda = 0 (its own column)");
        const int want = K + (cfg->use_discriminator ? 1 : 0) + (lpips ? 1 : 0);
        REQUIRE(n_obj == want, GLASS_ERR_ARG,
                "with sim_columns >= 2, n_obj must be sim_columns + use_discriminator + (lpips_size > 0 && lpips_lambda == 0) = " + std::to_string(want) +
                    ", got " + std::to_string(n_obj));
    }
    if (!lpips) {
        REQUIRE(K >= 2 || n_obj == 1 || n_obj == 2, GLASS_ERR_ARG, "n_obj must be 1 or 2");
    } else {
        REQUIRE(cfg->n_blocks > 0 || cfg->generator == GLASS_GEN_BIGGAN_DEEP, GLASS_ERR_ARG,
                "lpips_size > 0 needs a generator: this engine has none (GPT-2 / img2txt), so there is no generated image to compare");
        if (int lrc = glass_lpips_supported(0, cfg->lpips_size)) return lrc;
        REQUIRE(std::isfinite(cfg->lpips_lambda) && cfg->lpips_lambda >= 0.f, GLASS_ERR_ARG, "lpips_lambda must be finite and >= 0");
        const int want = K + (cfg->use_discriminator ? 1 : 0) + (cfg->lpips_lambda == 0.f ? 1 : 0);
        REQUIRE(n_obj == want, GLASS_ERR_ARG,
                "with lpips_size > 0, n_obj must be 1 + use_discriminator + (lpips_lambda == 0) = " + std::to_string(want) + ", got " +
                    std::to_string(n_obj));
    }
    if (cfg->use_discriminator) {
        REQUIRE(cfg->mbstd_group >= 2 && cfg->mbstd_group <= 8 && cfg->batch_size % cfg->mbstd_group == 0, GLASS_ERR_ARG,
                "batch_size must be a multiple of mbstd_group (modules.py:716)");
    }
    if (cfg->clip_arch == 1) {       // ModifiedResNet: its own rule, and the shared fields as include/glass.h defines them for it
        if (int grc = glass_clip_resnet_supported(cfg->clip_rn_layers, cfg->clip_width, cfg->clip_res, cfg->clip_embed)) return grc;
        const int nb = cfg->clip_rn_layers[0] + cfg->clip_rn_layers[1] + cfg->clip_rn_layers[2] + cfg->clip_rn_layers[3];
        REQUIRE(cfg->clip_heads == cfg->clip_width / 2 && cfg->clip_patch == 32 && cfg->clip_layers == nb, GLASS_ERR_ARG,
                "CLIP ResNet: clip_heads must be width * 32 / 64, clip_patch 32 and clip_layers the sum of clip_rn_layers");
    } else {
        REQUIRE(cfg->clip_arch == 0, GLASS_ERR_ARG, "clip_arch must be 0 (ViT) or 1 (ModifiedResNet)");
        if (int grc = glass_clip_geometry_supported(cfg->clip_width, cfg->clip_layers, cfg->clip_heads, cfg->clip_patch, cfg->clip_res,
                                                    cfg->clip_embed))
            return grc;
    }
    REQUIRE(cfg->noise_mode >= 0 && cfg->noise_mode <= 2, GLASS_ERR_ARG, "noise_mode must be 0,1,2");
    int bg_res = 0;
    if (cfg->generator == GLASS_GEN_BIGGAN_DEEP) {
        REQUIRE(cfg->n_blocks == 0 && !cfg->use_discriminator && (lpips || K >= 2 || cfg->n_obj == 1), GLASS_ERR_ARG,
                "BigGAN-deep: n_blocks must be 0, no discriminator, n_obj 1 (config.py:31-74)");
        REQUIRE(cfg->bg_n_layers > 0 && cfg->bg_n_layers <= GLASS_MAX_BG_LAYERS, GLASS_ERR_ARG, "bg_n_layers out of range");
        REQUIRE(cfg->bg_ch > 0 && cfg->bg_ch % 32 == 0 && cfg->bg_z_dim > 0 && cfg->bg_z_dim % 4 == 0 && cfg->bg_num_classes > 0,
                GLASS_ERR_ARG, "BigGAN-deep: bad channel_width / z_dim / num_classes");
        REQUIRE(cfg->latent_size == cfg->bg_z_dim + cfg->bg_num_classes, GLASS_ERR_ARG,
                "BigGAN-deep: latent_size must be z_dim + num_classes (latent.py:16-18)");
        REQUIRE(cfg->bg_n_stats >= 2 && cfg->bg_eps > 0.f && cfg->bg_truncation > 0.f && cfg->bg_truncation <= 1.f,
                GLASS_ERR_ARG, "BigGAN-deep: bad n_stats / eps / truncation");
        bg_res = 4;
        for (int i = 0; i < cfg->bg_n_layers; ++i) {
            const int cin = cfg->bg_ch * cfg->bg_layers[i][1], cout = cfg->bg_ch * cfg->bg_layers[i][2];
            REQUIRE(cin > 0 && cout > 0 && (cin == cout || cin == 2 * cout), GLASS_ERR_ARG,
                    "BigGAN-deep GenBlock: out channels must equal in or in/2 (channel-drop skip)");
            REQUIRE(cin % 128 == 0 && cout % 32 == 0, GLASS_ERR_ARG,
                    "BigGAN-deep GenBlock: in/4 and out channels must be multiples of 32");
            bg_res <<= (cfg->bg_layers[i][0] ? 1 : 0);
        }
        REQUIRE(cfg->bg_layers[0][1] == 16 && cfg->bg_layers[cfg->bg_n_layers - 1][2] == 1, GLASS_ERR_ARG,
                "BigGAN-deep: first GenBlock takes 16*ch channels, last produces ch");
    } else {
        REQUIRE(cfg->generator == GLASS_GEN_STYLEGAN2, GLASS_ERR_ARG, "unknown generator kind");
    }
    const int gen_res = cfg->n_blocks > 0 ? 4 << (cfg->n_blocks - 1) : bg_res;
    if (int prc = glass_clip_preprocess_supported(gen_res, cfg->clip_res, cfg->clip_resize, cfg->clip_normalize)) return prc;
    if (lpips)
        if (int lrc = glass_lpips_supported(gen_res, cfg->lpips_size)) return lrc;
    int ndev = 0;
    GLASS_HIP(hipGetDeviceCount(&ndev));
    REQUIRE(cfg->device >= 0 && cfg->device < ndev, GLASS_ERR_ARG, "no such HIP device");
    GLASS_HIP(hipSetDevice(cfg->device));
    glass_engine* e = new glass_engine();
    e->cfg = *cfg;
    e->R = gen_res;
    e->n_lat = cfg->generator == GLASS_GEN_STYLEGAN2 ? 2 * cfg->n_blocks : 0;
    int chunk = cfg->chunk > 0 ? cfg->chunk : std::max(cfg->batch_size, (64 / cfg->batch_size) * cfg->batch_size);   // 288 GB of HBM: one chunk of 64 candidates (36 GB of activations at 1024 px) keeps every launch large
    chunk = std::min(chunk, cfg->max_pop);
    if (chunk % cfg->batch_size != 0) {
        delete e;
        glass_set_error("chunk must be a multiple of batch_size");
        return GLASS_ERR_ARG;
    }
    e->chunk = chunk;
    // Stream mode: glass_engine_set_overlap() is the only control (bench.py translates GLASS_OVERLAP / GLASS_NO_CLIP_OVERLAP into
    // set_overlap() calls for the measure_* scripts).
    // Chunk pipelining (mode 1) stretches every co-running kernel ~2x, which makes per-kernel profiles meaningless: opt-in.
    e->overlap = false;
    // default (mode 2): CLIP's image tower (short, latency-bound launches) on the second stream next to the discriminator, which only
    // shares the finished image with it
    e->clip_overlap = true;
    hipError_t err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (err == hipSuccess) {
        // the second stream carries CLIP's ~75 short dependent launches beside the discriminator's chip-filling kernels: at the highest
        // priority its workgroups are placed first whenever a CU has room (the main stream's persistent kernels never yield one)
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        err = hipStreamCreateWithPriority(&e->stream_d, hipStreamNonBlocking, prio_hi);
    }
    e->cur = e->stream;
    if (err == hipSuccess) err = hipEventCreate(&e->ev0);
    if (err == hipSuccess) err = hipEventCreate(&e->ev1);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&e->ev_noise, hipEventDisableTiming);
    if (err != hipSuccess) {
        delete e;
        glass_set_error(std::string("stream/event creation failed: ") + hipGetErrorString(err));
        return GLASS_ERR_HIP;
    }
    *out = e;
    return GLASS_OK;
}

extern "C" void glass_engine_destroy(glass_engine* e) {
    if (!e) return;
    hipSetDevice(e->cfg.device);
    if (e->stream) hipStreamSynchronize(e->stream);
    if (e->stream_d) hipStreamSynchronize(e->stream_d);
    gpt2_work_free(e);
    std::swap(e->gwork, e->gwork_alt);
    gpt2_work_free(e);
    text_work_free(e);
    for (void* p : e->allocs) hipFree(p);
    if (e->h_pinned) hipHostFree(e->h_pinned);
    for (auto ev : e->event_pool) hipEventDestroy(ev);
    for (auto ev : e->ev_g) hipEventDestroy(ev);
    for (auto ev : e->ev_d) hipEventDestroy(ev);
    if (e->ev0) hipEventDestroy(e->ev0);
    if (e->ev1) hipEventDestroy(e->ev1);
    if (e->ev_noise) hipEventDestroy(e->ev_noise);
    if (e->stream) hipStreamDestroy(e->stream);
    if (e->stream_d) hipStreamDestroy(e->stream_d);
    delete e;
}

extern "C" int glass_engine_load_tensor(glass_engine* e, const char* name, const float* data, int32_t rank,
                                        const int64_t* dims) {
    REQUIRE(e && name && data && rank >= 0 && (rank == 0 || dims), GLASS_ERR_ARG, "null argument");
    REQUIRE(!e->finalized, GLASS_ERR_STATE, "engine already finalized");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < rank; ++i) {
        REQUIRE(dims[i] > 0, GLASS_ERR_ARG, "non-positive dimension");
        t.dims.push_back(dims[i]);
        n *= (size_t)dims[i];
    }
    t.data.assign(data, data + n);
    e->host[name] = std::move(t);
    return GLASS_OK;
}

static int alloc_buffers(glass_engine* e) {
    const glass_config& c = e->cfg;
    const int P = c.max_pop, L = c.latent_size, CH = e->chunk;
    int rc;
    if ((rc = dev_alloc(e, &e->d_z, (size_t)P * L))) return rc;
    if ((rc = dev_alloc(e, &e->d_w0, (size_t)P * L))) return rc;
    if ((rc = dev_alloc(e, &e->d_w1, (size_t)P * L))) return rc;
    if ((rc = dev_alloc(e, &e->d_s, (size_t)P * e->S_total))) return rc;
    if ((rc = dev_alloc(e, &e->d_s16, (size_t)P * e->S_total))) return rc;
    if ((rc = dev_alloc(e, &e->d_smax, (size_t)P * e->n_style))) return rc;
    if ((rc = dev_alloc(e, &e->d_trgb_tab, (size_t)P * 32 * 512))) return rc;
    {   // toRGB partial sums of the blocks wider than 128 channels: [C / 128][chunk][3][res][res] fp32, the largest block's
        size_t part = 0;
        for (int b = 0; b < c.n_blocks; ++b)
            if (c.channels[b] > 128 && c.channels[b] % 128 == 0 && c.channels[b] <= 512)
                part = std::max(part, (size_t)(c.channels[b] / 128) * (size_t)P * 3 * ((size_t)4 << b) * ((size_t)4 << b));   // (P: the blocks up to 32 x 32 run the whole population)
        if (part && (rc = dev_alloc(e, &e->d_trgb_part, part))) return rc;
    }
    if (e->cfg.generator != GLASS_GEN_BIGGAN_DEEP && e->cfg.n_blocks > 0) {
        // StyleGAN2's low-resolution layers as im2col + GEMM (conv_gemm.hip): conv grids up to 16 x 16 per candidate, widest
        // channel count (151 + 134 MB at P = 64).  The capacities are per candidate: whether a layer takes this path must not
        // depend on how many candidates a launch carries.  (A few OTHER dispatchers do look at the launch size — conv_stream wants
    // enough tiles per workgroup, gemm_tiled picks its tile by M, gpt2's split-K depth follows M — so chunking / sharding
    // invariance holds to fp16 rounding, not to the bit: tests/test_gpu_engine.py::test_pop512_as_eight_shards_of_64.)
        int cmax = 16;
        for (int i = 0; i < e->cfg.n_blocks; ++i) cmax = std::max(cmax, (int)e->cfg.channels[i]);
        e->cap_a = 256LL * 9 * cmax;
        e->cap_c = 256LL * 4 * cmax;
        if ((rc = dev_alloc(e, &e->ws_a, (size_t)(e->cap_a * P)))) return rc;
        if ((rc = dev_alloc(e, &e->ws_c, (size_t)(e->cap_c * P)))) return rc;
        if (e->cfg.use_discriminator) {   // stream mode 1 runs D on the second stream next to G: its own scratch
            if ((rc = dev_alloc(e, &e->ws_a2, (size_t)(e->cap_a * P)))) return rc;
            if ((rc = dev_alloc(e, &e->ws_c2, (size_t)(e->cap_c * P)))) return rc;
        }
    } else if (e->cfg.generator == GLASS_GEN_BIGGAN_DEEP) {
        // BigGAN-deep's 4 x 4 .. 16 x 16 layers (3 x 3 on ch * 4 = 512 channels, 1 x 1 up to ch * 16 outputs) on the same path (round 3:
        // they ran on conv_direct at 64 - 220 TFLOP/s); the walk over the population is chunked, so the scratch holds one chunk
        const int cmax = 4 * e->cfg.bg_ch;
        e->cap_a = 256LL * 9 * cmax;
        e->cap_c = 256LL * 4 * cmax;
        if ((rc = dev_alloc(e, &e->ws_a, (size_t)(e->cap_a * P)))) return rc;
        if ((rc = dev_alloc(e, &e->ws_c, (size_t)(e->cap_c * P)))) return rc;
    }
    if ((rc = dev_alloc(e, &e->d_epsrow, (size_t)P * e->n_style))) return rc;
    if ((rc = dev_alloc(e, &e->d_dscale, (size_t)P * e->D_total))) return rc;
    for (auto& g : e->gconv) {
        // per-sample weights where the tensor is tiny and the tiled / fused kernels (one sample per block) apply
        const bool fused_ok = g.up && g.cin % 32 == 0 && g.cout % 32 == 0 && g.res_in >= 16;
        const bool tiled_ok = !g.up && g.cin % 32 == 0 && g.cout % 32 == 0 && g.res_in % 32 == 0;
        g.welems = 9LL * g.cin * g.cout;
        // at most 500 KB per sample (round 3: the 256 -> 128 up-conv, 590 KB per sample, runs 4 % faster on the shared-weight image grid,
        // and its consumer 5 % faster on the pre-styled output; 1200 was round 2's value)
        g.premod = (fused_ok || tiled_ok) && g.welems * 2 <= (500LL << 10);
        if (g.premod && (rc = dev_alloc(e, &g.wm, (size_t)P * g.welems))) return rc;
    }
    if (c.noise_mode != 0) {
        const int n_mb = P / c.batch_size;
        for (auto& g : e->gconv) {
            float* p;
            if ((rc = dev_alloc(e, &p, (size_t)n_mb * g.res_out * g.res_out))) return rc;
            e->d_noise.push_back(p);
        }
    }
    size_t maxact = 0;
    for (int b = 0; b < c.n_blocks; ++b) {
        const size_t res = 4u << b;
        size_t ch = c.channels[b];
        if (b > 0) ch = std::max<size_t>(ch, c.channels[b - 1]);
        maxact = std::max(maxact, (res + 1) * (res + 1) * ch);
    }
    if (c.n_blocks > 0) maxact = std::max(maxact, (size_t)16 * (c.channels[0] + 16));
    e->act_elems = maxact * CH;
    for (int i = 0; i < 8 && c.n_blocks > 0; ++i)   // [0..5]: D scratch (D stream), [6..7]: G ping-pong (main stream)
        if (i >= 6 || c.use_discriminator)
            if ((rc = dev_alloc(e, &e->act[i], e->act_elems))) return rc;
    for (int i = 0; i < 4; ++i)     // two sets (chunk parity) of skip-image ping-pong
        if ((rc = dev_alloc(e, &e->ybuf[i], (size_t)CH * 3 * e->R * e->R))) return rc;
    // whole-population buffers for the low-resolution phases (res <= low_res)
    if (c.n_blocks > 0) {
        e->n_low = 0;
        while (e->n_low < c.n_blocks && (4 << e->n_low) <= e->low_res) ++e->n_low;
        if (e->n_low < 1) e->n_low = 1;
        const size_t rl = 4u << (e->n_low - 1);
        size_t cmax = 16;
        for (int b = 0; b < e->n_low; ++b) cmax = std::max<size_t>(cmax, c.channels[b]);
        if (e->n_low < c.n_blocks) cmax = std::max<size_t>(cmax, c.channels[e->n_low]);
        const size_t low_elems = (size_t)P * (rl + 1) * (rl + 1) * (cmax + 16);
        const int n_lowbuf = c.use_discriminator ? 6 : 2;
        for (int i = 0; i < n_lowbuf; ++i)
            if ((rc = dev_alloc(e, &e->low[i], low_elems))) return rc;
        for (int i = 0; i < 2; ++i)
            if ((rc = dev_alloc(e, &e->ylow[i], (size_t)P * 3 * rl * rl))) return rc;
    }
    if ((rc = dev_alloc(e, &e->d_img, (size_t)CH * 3 * e->R * e->R))) return rc;
    const int W = c.clip_width, ps = c.clip_patch, G = c.clip_res / ps, T = G * G + 1;
    const size_t Kp = (size_t)clip_patch_k(c);
    const size_t PI = clip_max_images(e);      // the tower's side holds every view of every candidate (max_pop images with the views off)
    if ((rc = dev_alloc(e, &e->d_patches, PI * G * G * Kp))) return rc;
    if (Kp != (size_t)3 * ps * ps) GLASS_HIP(hipMemset(e->d_patches, 0, PI * G * G * Kp * sizeof(half_t)));   // the row tails stay zero: no kernel writes them
    if ((rc = dev_alloc(e, &e->d_pe, PI * G * G * W))) return rc;
    if ((rc = dev_alloc(e, &e->d_x, PI * T * W))) return rc;
    if ((rc = dev_alloc(e, &e->d_ln16, PI * T * W))) return rc;
    if ((rc = dev_alloc(e, &e->d_qkv, PI * T * 3 * W))) return rc;
    if ((rc = dev_alloc(e, &e->d_attn, PI * T * W))) return rc;
    if ((rc = dev_alloc(e, &e->d_hid, PI * T * 4 * W))) return rc;
    if ((rc = dev_alloc(e, &e->d_cls, PI * W))) return rc;
    if ((rc = alloc_clip_resnet(e))) return rc;
    if ((rc = dev_alloc(e, &e->d_feat, PI * c.clip_embed))) return rc;
    if (e->views && (rc = dev_alloc(e, &e->d_view_sim, PI))) return rc;
    if ((rc = dev_alloc(e, &e->d_sim, (size_t)P))) return rc;
    if ((rc = dev_alloc(e, &e->d_dis, (size_t)P))) return rc;
    if ((rc = dev_alloc(e, &e->d_F, (size_t)P * std::max(c.lpips_size ? 3 : 2, c.n_obj)))) return rc;
    if ((rc = dev_alloc(e, &e->pset.d_targets, (size_t)GLASS_PROMPT_MAX * c.clip_embed))) return rc;
    if ((rc = dev_alloc(e, &e->pset.d_weights, (size_t)GLASS_PROMPT_MAX))) return rc;
    if ((rc = dev_alloc(e, &e->pset.d_sim, (size_t)P * GLASS_PROMPT_MAX))) return rc;
    if (c.use_discriminator && c.n_blocks > 0) {
        if ((rc = dev_alloc(e, &e->d_dfin, (size_t)P * 16 * c.channels[0]))) return rc;
        if ((rc = dev_alloc(e, &e->d_dh, (size_t)P * c.channels[0]))) return rc;
        if ((rc = dev_alloc(e, &e->d_dh_part, (size_t)16 * P * c.channels[0]))) return rc;    // split-K slices of D's first dense layer
    }
    {   // descriptor table of the demodulation problems (one launch for all layers)
        std::vector<DenseDesc> dd;
        for (auto& g : e->gconv) {
            DenseDesc q;
            q.x = e->d_s + g.style_off; q.ldx = e->S_total; q.K = g.cin; q.wt = g.wsq; q.N = g.cout; q.bias = nullptr;
            q.out = e->d_dscale + g.ds_off; q.ldo = e->D_total; q.eps_row = e->d_epsrow + g.style_idx; q.eps_stride = e->n_style;
            dd.push_back(q);
            e->demod_max_n = std::max(e->demod_max_n, g.cout);
        }
        DenseDesc* dptr = nullptr;
        if ((rc = upload(e, &dptr, dd))) return rc;
        e->d_demod_desc = dptr;
    }
    GLASS_HIP(hipMemset(e->d_dis, 0, (size_t)P * sizeof(float)));
    e->h_pinned_bytes = std::max((size_t)P * latent_row_floats(e), (size_t)P * (c.clip_embed + 8)) * sizeof(float);
    GLASS_HIP(hipHostMalloc((void**)&e->h_pinned, e->h_pinned_bytes, hipHostMallocDefault));
    return GLASS_OK;
}

extern "C" int glass_engine_finalize(glass_engine* e) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(!e->finalized, GLASS_ERR_STATE, "engine already finalized");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    int rc = GLASS_OK;
    if (e->cfg.n_blocks > 0) {
        if ((rc = finalize_generator(e))) return rc;
        if (e->cfg.use_discriminator && (rc = finalize_discriminator(e))) return rc;
    }
    if (e->cfg.generator == GLASS_GEN_BIGGAN_DEEP && (rc = glass_biggan_finalize(e))) return rc;
    if ((rc = finalize_gpt2(e))) return rc;
    if ((rc = finalize_clip(e))) return rc;
    if ((rc = finalize_preprocess(e))) return rc;
    if ((rc = finalize_lpips(e))) return rc;
    if ((rc = alloc_buffers(e))) return rc;
    if ((rc = alloc_search(e))) return rc;
    e->host.clear();  // host copies no longer needed
    e->finalized = true;
    return GLASS_OK;
}

extern "C" int glass_engine_set_target(glass_engine* e, const float* feat, int32_t n) {
    REQUIRE(e && feat, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "finalize() first");
    REQUIRE(n == e->cfg.clip_embed, GLASS_ERR_ARG, "target feature length != clip_embed");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    REQUIRE(sim_columns(e->cfg) < 2, GLASS_ERR_STATE,
            "set_target: this engine has sim_columns >= 2 (one column per prompt): give it a prompt set with set_targets()");
    glass_engine::PromptSet& ps = e->pset;      // the set of one: entry 0, weight 1, W = 1, mode sum — (0 + 1 c) / 1 is c in fp32
    const float one = 1.f;
    GLASS_HIP(hipMemcpy(ps.d_targets, feat, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemcpy(ps.d_weights, &one, sizeof(float), hipMemcpyHostToDevice));
    ps.W = 1.f;
    ps.T = 1;
    ps.mode = 0;
    ps.single = true;
    return GLASS_OK;
}

// ---- prompt sets --------------------------------------------------------------------------------
extern "C" int glass_prompt_set_supported(int32_t n_entries, int32_t mode, int32_t sim_columns) {
    REQUIRE(n_entries >= 1 && n_entries <= GLASS_PROMPT_MAX, GLASS_ERR_ARG,
            "a prompt set holds 1 .. " + std::to_string(GLASS_PROMPT_MAX) + " entries, got " + std::to_string(n_entries));
    REQUIRE(mode == 0 || mode == 1, GLASS_ERR_ARG, "prompt set mode must be 0 (sum) or 1 (pareto)");
    REQUIRE(sim_columns >= 0 && sim_columns <= 4, GLASS_ERR_ARG, "sim_columns must be in [0, 4]");
    if (mode == 0) {
        REQUIRE(sim_columns <= 1, GLASS_ERR_ARG,
                "mode sum blends the set into one similarity column, and this engine has sim_columns = " + std::to_string(sim_columns) +
                    ": use mode pareto, or an engine with sim_columns 0");
    } else {
        REQUIRE(n_entries >= 2 && n_entries <= 4, GLASS_ERR_ARG,
                "mode pareto gives every entry its own column of F: 2 .. 4 entries, got " + std::to_string(n_entries));
        REQUIRE(n_entries == sim_columns, GLASS_ERR_ARG,
                "mode pareto needs an engine created with sim_columns = the number of entries (" + std::to_string(n_entries) + "), this one has " +
                    std::to_string(sim_columns));
    }
    return GLASS_OK;
}

extern "C" int glass_engine_set_targets(glass_engine* e, const float* feats, const float* weights, int32_t T, int32_t E, int32_t mode) {
    REQUIRE(e && feats && weights, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "finalize() first");
    REQUIRE(E == e->cfg.clip_embed, GLASS_ERR_ARG, "set_targets: feature length != clip_embed");
    if (int rc = glass_prompt_set_supported(T, mode, e->cfg.sim_columns)) return rc;
    for (int t = 0; t < T; ++t)
        REQUIRE(std::isfinite(weights[t]) && weights[t] != 0.f, GLASS_ERR_ARG,
                "set_targets: weight " + std::to_string(t) + " must be finite and non-zero (negative: away from the prompt)");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    glass_engine::PromptSet& ps = e->pset;
    GLASS_HIP(hipMemcpy(ps.d_targets, feats, (size_t)T * E * sizeof(float), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemcpy(ps.d_weights, weights, (size_t)T * sizeof(float), hipMemcpyHostToDevice));
    ps.W = prompt_weight_sum(weights, T);
    ps.T = T;
    ps.mode = mode;
    ps.single = false;
    return GLASS_OK;
}

extern "C" int glass_engine_last_set_details(glass_engine* e, int32_t P, float* set_sim) {
    REQUIRE(e && e->finalized, GLASS_ERR_STATE, "engine not ready");
    REQUIRE(set_sim, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->pset.given(), GLASS_ERR_STATE, "no prompt set is active (glass_engine_set_targets)");
    REQUIRE(P > 0 && P <= e->last_P, GLASS_ERR_ARG, "P exceeds the last evaluated population");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    GLASS_HIP(hipMemcpy(set_sim, e->pset.d_sim, (size_t)P * e->pset.T * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

// ------------------------------------------------------------------------------------
// profiling scopes (hipEvent pair per launch when enabled)
// ------------------------------------------------------------------------------------
void collect_profile(glass_engine* e) {
    std::map<std::string, glass_prof_row> rows;
    std::vector<std::string> order;
    for (auto& pe : e->prof_events) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, pe.e0, pe.e1);
        auto it = rows.find(pe.name);
        if (it == rows.end()) {
            glass_prof_row r;
            memset(&r, 0, sizeof r);
            strncpy(r.name, pe.name.c_str(), sizeof(r.name) - 1);
            it = rows.emplace(pe.name, r).first;
            order.push_back(pe.name);
        }
        it->second.launches += 1;
        it->second.total_ms += ms;
        it->second.flops += pe.flops;
        it->second.bytes += pe.bytes;
    }
    e->prof_rows.clear();
    for (auto& n : order) e->prof_rows.push_back(rows[n]);
    e->prof_events.clear();
    e->event_next = 0;
}

// The order in which the single-kernel conv families are asked, written once; the first that takes the layer runs it.  run_conv goes on to
// conv_gemm (which needs the engine's scratch) and conv_direct where all of them refuse.
ConvKernel choose_conv(const ConvParams& p) {
    ConvKernel k;
    if (p.up && (k = choose_conv_upfir(p))) return k;
    if ((k = choose_conv_stream(p))) return k;
    if ((k = choose_conv_wreg(p))) return k;
    if ((k = choose_conv_glds(p))) return k;
    if ((k = choose_conv_s2(p))) return k;
    return choose_conv_tiled(p);
}

// the epilogues fold the scale into the activation constants, max(v k1, v k2) (common.h act_apply): s > 0 only
static bool out_scale_ok(glass_engine* e, const ConvParams& p, const char* tag) {
    if (p.out_scale > 0.f) return true;
    if (e->launch_error.empty()) e->launch_error = std::string("out_scale must be positive: ") + tag;
    return false;
}

// a walker asked a chooser first and kept the answer: launch that kernel
void run_chosen(glass_engine* e, const ConvKernel& k, const ConvParams& p, const char* tag, double flops, double bytes) {
    if (!out_scale_ok(e, p, tag)) return;
    Prof pr(e, tag, flops, bytes);
    k.launch(p, e->cur);
    pr.ran(tag, k.name);
}

void run_conv(glass_engine* e, const ConvParams& p, const char* tag, double flops, double bytes) {
    if (!out_scale_ok(e, p, tag)) return;
    Prof pr(e, tag, flops, bytes);
    ConvKernel k = choose_conv(p);
    const char* name = k.name;
    if (!k) {
        const bool second = e->cur == e->stream_d && e->ws_a2;
        name = launch_conv_gemm(p, second ? e->ws_a2 : e->ws_a, e->cap_a, second ? e->ws_c2 : e->ws_c, e->cap_c, e->cur);
        if (!name && (k = choose_conv_direct(p))) name = k.name;
    }
    if (k) k.launch(p, e->cur);
    if (!name) {   // no kernel family accepts this layer: remember it, the pass returns an error instead of a wrong result
        if (e->launch_error.empty()) e->launch_error = std::string("no kernel accepts layer ") + tag;
        name = "(refused)";
    }
    pr.ran(tag, name);
}
void run_gemm(glass_engine* e, const GemmParams& p, const char* tag) {
    Prof pr(e, tag, 2.0 * p.M * p.N * p.K, 2.0 * ((double)p.M * p.K + (double)p.N * p.K + (double)p.M * p.N));
    const char* k = launch_gemm_tiled(p, e->cur);
    if (!k) k = launch_gemm_direct(p, e->cur);
    pr.ran(tag, k);
}

ConvParams conv_defaults() {
    ConvParams p;
    memset(&p, 0, sizeof p);
    p.out_scale = 1.f;
    p.batch_size = 1;
    p.stride = 1;
    return p;
}

GemmParams gemm_params(const half_t* a, const half_t* w, int M, int N, int K, const float* bias, int mode, half_t* out16, float* out32,
                       int cand_rows) {
    GemmParams g;
    memset(&g, 0, sizeof g);
    g.a = a; g.w = w; g.M = M; g.N = N; g.K = K; g.bias = bias; g.mode = mode;
    g.out16 = out16; g.out32 = out32; g.ldo = N; g.cand_rows = cand_rows;
    return g;
}

// ------------------------------------------------------------------------------------
// the pass
// ------------------------------------------------------------------------------------
// The wait at the end of a pass: the stream, the launchers' verdict, the profile.
int wait_pass(glass_engine* e, int P) {
    GLASS_HIP(hipStreamSynchronize(e->cur));
    GLASS_HIP(hipGetLastError());
    GLASS_HIP(hipEventElapsedTime(&e->last_ms, e->ev0, e->ev1));
    if (!e->launch_error.empty()) {
        const std::string msg = e->launch_error;
        e->launch_error.clear();
        if (e->profiling) collect_profile(e);
        glass_set_error(msg);
        return GLASS_ERR_STATE;
    }
    e->last_P = P;
    if (e->profiling) collect_profile(e);
    return GLASS_OK;
}

// The end of a pass for both generators, on e->cur (the main stream): CLIP unless it already ran on the second stream (clip_done; the main
// stream waits for it), F, the copy, the wait, the launchers' verdict, the profile.  d_join: the stream the discriminator's head is on when
// that is not the main one (stream mode 1); joined behind CLIP.
// out_F: the rows are copied back to the host and the call waits.  d_F_dst (the device search): they are copied to that device buffer on the
// stream instead, and with no_wait the stream is left running — the caller launches survival behind the pass and calls wait_pass once.
static int finish_pass(glass_engine* e, int P, float* out_F, bool clip_done, hipStream_t d_join, float* d_F_dst = nullptr, bool no_wait = false) {
    const glass_config& c = e->cfg;
    if (out_F || d_F_dst) {
        if (!clip_done) run_clip(e, pass_images(e, P), e->views);
        if (d_join) {   // join: D head finished
            GLASS_HIP(hipEventRecord(e->ev_g[0], d_join));
            GLASS_HIP(hipStreamWaitEvent(e->stream, e->ev_g[0], 0));
        }
        const glass_engine::PromptSet& ps = e->pset;
        const bool pareto = ps.given() && ps.mode == 1;
        AssembleF a;
        a.sim = e->d_sim;
        if (pareto) a.set_sim = ps.d_sim, a.weights = ps.d_weights, a.K = ps.T;
        if (c.lpips_size) a.lp = e->lp.d, a.lp_lambda = c.lpips_lambda;
        if (c.anchor) a.anchor = e->edit.d_dist, a.anchor_lambda = c.anchor_lambda;      // image editing: its own last column, or folded into column 0
        a.P = P, a.n_obj = c.n_obj, a.F = e->d_F;
        // the hinge is the column n_obj has beyond the others: without LPIPS and anchor, glass_engine_create takes n_obj 1 or 2 as it comes
        const int others = (pareto ? ps.T : 1) + (a.lp && !(a.lp_lambda > 0.f) ? 1 : 0) + (a.anchor && !(a.anchor_lambda > 0.f) ? 1 : 0);
        if (c.n_obj > others) a.dis = e->d_dis;
        if (!launch_assemble_F(a, e->cur) && e->launch_error.empty())
            e->launch_error = "no kernel accepts layer assemble_F (assemble_F_edit: the columns do not add up to n_obj)";
        if (d_F_dst)
            GLASS_HIP(hipMemcpyAsync(d_F_dst, e->d_F, (size_t)P * c.n_obj * sizeof(float), hipMemcpyDeviceToDevice, e->cur));
        else
            GLASS_HIP(hipMemcpyAsync(e->h_pinned, e->d_F, (size_t)P * c.n_obj * sizeof(float), hipMemcpyDeviceToHost, e->cur));
    }
    GLASS_HIP(hipEventRecord(e->ev1, e->cur));
    if (no_wait) return GLASS_OK;
    if (int rc = wait_pass(e, P)) return rc;
    if (out_F) memcpy(out_F, e->h_pinned, (size_t)P * c.n_obj * sizeof(float));
    return GLASS_OK;
}

int run_pass(glass_engine* e, const float* latents, int P, int generation, int first_mb, const glass_noise* noise, float* host_F, float* images,
             const float* d_latents, float* d_F_dst, bool no_wait) {
    REQUIRE(e && (latents || d_latents), GLASS_ERR_ARG, "null argument");
    const bool out_F = host_F || d_F_dst;      // a scoring pass
    REQUIRE(e->finalized, GLASS_ERR_STATE, "finalize() first (weights not loaded)");
    const glass_config& c = e->cfg;
    REQUIRE(P > 0 && P <= c.max_pop, GLASS_ERR_ARG, "population size out of range (max_pop)");
    REQUIRE(P % c.batch_size == 0, GLASS_ERR_ARG,
            "population size must be a multiple of batch_size (reference asserts: models.py:112)");
    const bool biggan = c.generator == GLASS_GEN_BIGGAN_DEEP;
    REQUIRE(e->cfg.n_blocks > 0 || biggan, GLASS_ERR_STATE, "this engine was created without a GAN (n_blocks = 0)");
    if (out_F && sim_columns(c) >= 2) REQUIRE(e->pset.given(), GLASS_ERR_STATE, "set_targets() first (this engine has sim_columns >= 2: one column of F per prompt)");
    else if (out_F) REQUIRE(e->pset.T > 0, GLASS_ERR_STATE, "set_target() first");
    const bool lpips = out_F && c.lpips_size > 0;
    if (lpips) REQUIRE(e->lp.has_target, GLASS_ERR_STATE, "set_lpips_target() first");
    const bool anchor = out_F && c.anchor, source = out_F && e->edit.has_source;      // image editing (opt-in)
    if (anchor) REQUIRE(e->edit.has_anchor, GLASS_ERR_STATE, "set_anchor() first (this engine was created with anchor = 1)");
    if (source) REQUIRE(e->pset.given(), GLASS_ERR_STATE, "set_targets() first (a direction source is set: the targets are the directions of a prompt set)");
    REQUIRE(e->latent_space != GLASS_LATENT_SUB || e->has_subspace, GLASS_ERR_STATE, "set_subspace() first (latent space sub: a row is coefficients of a basis the engine does not have yet)");
    GLASS_HIP(hipSetDevice(c.device));
    e->launch_error.clear();      // (a pass that returned early through GLASS_HIP must not leave its message to the next one)
    // the rows go where run_styles reads them: z rows in front of the mapping network, w rows in its output's place, w+ rows per layer
    const size_t row = latent_row_floats(e);
    float* d_rows = latent_rows_dst(e);
    if (latents) memcpy(e->h_pinned, latents, (size_t)P * row * sizeof(float));
    GLASS_HIP(hipEventRecord(e->ev0, e->cur));
    if (latents) {
        GLASS_HIP(hipMemcpyAsync(d_rows, e->h_pinned, (size_t)P * row * sizeof(float), hipMemcpyHostToDevice, e->cur));
        e->latent_uploads += 1;
        e->latent_upload_rows += P;
    } else {      // the device search's rows: already on the device
        GLASS_HIP(hipMemcpyAsync(d_rows, d_latents, (size_t)P * row * sizeof(float), hipMemcpyDeviceToDevice, e->cur));
    }
    const int ps = c.clip_patch, G = c.clip_res / ps;
    const size_t img_elems = (size_t)3 * e->R * e->R;
    // crop views: the boxes of this pass, from (noise_seed, generation) alone — first_mb plays no part, so shards and slices of a population
    // see the same crops; V images per candidate from the resize on
    const int V = std::max(e->views, 1), PV = P * V;
    const char* resize_tag = e->views ? "clip.views" : "clip.resize";
    const size_t cand_patches = (size_t)V * G * G * clip_patch_k(c);      // patch-operand elements per candidate
    if (e->views && out_F) {
        if (int brc = glass_host_clip_view_boxes(c.noise_seed, generation, e->views, e->R, e->view_min_permille, e->view_flip, e->view_fixed,
                                                 &e->view_boxes.box[0][0]))
            return brc;
        REQUIRE(view_boxes_valid(e->view_boxes, e->views, e->R), GLASS_ERR_STATE, "clip views: a box leaves the image");
    }
    // the direction source's rows under this pass's boxes, through the tower's buffers before the candidates' patches go there
    if (source)
        if (int src_rc = refresh_direction_source(e)) return src_rc;
    if (biggan) {
        // BigGAN-deep (models.py:75-86): no noise inputs, no discriminator; candidates are independent, so the
        // reference's minibatch loop has no semantic effect and the population is walked in engine chunks.
        int rc = glass_biggan_prepare(e, P);
        if (rc) return rc;
        for (int c0 = 0; c0 < P; c0 += e->chunk) {
            const int B = std::min(e->chunk, P - c0);
            float* y = e->ybuf[0];
            if ((rc = glass_biggan_chunk(e, c0, B, y))) return rc;
            if (images) {
                launch_finalize_image(y, e->d_img, (long long)B * img_elems, e->cur);
                GLASS_HIP(hipMemcpyAsync(images + (size_t)c0 * img_elems, e->d_img, (size_t)B * img_elems * sizeof(float),
                                         hipMemcpyDeviceToHost, e->cur));
            }
            if (out_F) {
                Prof pr(e, resize_tag, 0, clip_resize_bytes(e, B));
                run_clip_resize(e, y, B, e->d_patches + (size_t)c0 * cand_patches);
            }
            if (lpips) run_lpips_chunk(e, y, c0, B);
        }
        return finish_pass(e, P, host_F, false, nullptr, d_F_dst, no_wait);
    }
    // device-generated noise planes depend on nothing but (seed, generation, minibatch, layer): their 17 short launches run on the
    // second stream next to the mapping network / style / demodulation chain instead of ahead of it
    const bool noise_ov = e->clip_overlap && c.noise_mode == 1;
    int rc;
    if (noise_ov) {
        e->cur = e->stream_d;
        rc = upload_noise(e, P, generation, first_mb, noise);
        e->cur = e->stream;
        if (rc) return rc;
        GLASS_HIP(hipEventRecord(e->ev_noise, e->stream_d));
        run_styles(e, P);
        GLASS_HIP(hipStreamWaitEvent(e->stream, e->ev_noise, 0));
    } else {
        run_styles(e, P);
        rc = upload_noise(e, P, generation, first_mb, noise);
        if (rc) return rc;
    }
    if (anchor) run_anchor(e, P);      // the dlatents run_styles made are in place until the next pass
    const bool want_d = out_F && c.use_discriminator && (c.lpips_size > 0 || sim_columns(c) >= 2 || c.anchor || c.n_obj == 2);      // (with the perceptual objective n_obj counts its column too; so it does with an anchor)
    const int n = c.n_blocks;
    const int nlow = std::min(n, e->n_low);           // G blocks 0..nlow-1 run for the whole population
    const int nd = (int)e->dblk.size();               // D conv blocks (n - 1)
    const int d_hi = want_d ? std::max(0, n - nlow) : 0;  // D blocks 0..d_hi-1 (res > low_res) run per chunk
    // ---- phase A: low-resolution synthesis, whole population ------------------------------
    const half_t* xlow = nullptr;
    const float* ylow = nullptr;
    {
        half_t* const pp[2] = {e->low[0], e->low[1]};
        float* const yb[2] = {e->ylow[0], e->ylow[1]};
        run_g_blocks(e, 0, P, 0, nlow, e->g_const, 0, pp, nullptr, yb, &xlow, &ylow);
    }
    const int res_low = 4 << (nlow - 1);
    const long long xlow_bs = (long long)res_low * res_low * c.channels[nlow - 1];
    // D feature map handed from the chunked phase to the whole-population phase
    half_t* dmid = e->low[5];
    const int res_mid = d_hi < nd ? e->dblk[d_hi].res : 4;
    const long long dmid_bs = (long long)res_mid * res_mid * (d_hi < nd ? e->dblk[d_hi].cin : c.channels[0]);
    // ---- phase B: high-resolution synthesis per chunk on the main stream; resize + high-resolution
    // D of chunk k run on the second stream, overlapping the synthesis of chunk k+1 (memory-bound
    // and matrix-bound phases of the two networks interleave on the CUs).
    const int n_chunks = (P + e->chunk - 1) / e->chunk;
    while ((int)e->ev_g.size() < n_chunks) {
        hipEvent_t a, b2;
        GLASS_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        GLASS_HIP(hipEventCreateWithFlags(&b2, hipEventDisableTiming));
        e->ev_g.push_back(a);
        e->ev_d.push_back(b2);
    }
    const bool overlap = e->overlap && out_F;
    const bool clip_ov = e->clip_overlap && !overlap && out_F && want_d;
    hipStream_t sd = overlap ? e->stream_d : e->stream;
    for (int c0 = 0, k = 0; c0 < P; c0 += e->chunk, ++k) {
        const int B = std::min(e->chunk, P - c0);
        const int set = k & 1;
        e->cur = e->stream;
        if (overlap && k >= 2) GLASS_HIP(hipStreamWaitEvent(e->stream, e->ev_d[k - 2], 0));  // y set re-use
        const float* y = ylow + (size_t)c0 * 3 * res_low * res_low;
        if (nlow < n) {
            half_t* const pp[2] = {e->act[6], e->act[7]};
            float* const yb[2] = {e->ybuf[2 * set], e->ybuf[2 * set + 1]};
            const half_t* xo;
            run_g_blocks(e, c0, B, nlow, n, xlow + (size_t)c0 * xlow_bs, xlow_bs, pp, y, yb, &xo, &y);
        }
        if (images) {
            launch_finalize_image(y, e->d_img, (long long)B * img_elems, e->cur);
            GLASS_HIP(hipMemcpyAsync(images + (size_t)c0 * img_elems, e->d_img, (size_t)B * img_elems * sizeof(float),
                                     hipMemcpyDeviceToHost, e->cur));
        }
        if (out_F) {
            if (overlap) {
                GLASS_HIP(hipEventRecord(e->ev_g[k], e->stream));
                GLASS_HIP(hipStreamWaitEvent(sd, e->ev_g[k], 0));
            }
            e->cur = sd;
            {
                Prof pr(e, resize_tag, 0, clip_resize_bytes(e, B));
                run_clip_resize(e, y, B, e->d_patches + (size_t)c0 * cand_patches);
            }
            if (clip_ov && c0 + e->chunk >= P) {   // last chunk's patches are in place: CLIP starts now
                // its first layers on the MAIN stream (alone on the chip), the rest on the second stream beside the discriminator
                run_clip_embed(e, PV);
                run_clip_layers(e, PV, 0, GLASS_CLIP_SERIAL_LAYERS);
                GLASS_HIP(hipEventRecord(e->ev_g[0], e->stream));
                GLASS_HIP(hipStreamWaitEvent(e->stream_d, e->ev_g[0], 0));
                e->cur = e->stream_d;
                run_clip_layers(e, PV, GLASS_CLIP_SERIAL_LAYERS, c.clip_layers);
                run_clip_head(e, PV, e->views);
                GLASS_HIP(hipEventRecord(e->ev_d[0], e->stream_d));
                e->cur = e->stream;
            }
            if (want_d) {
                if (d_hi > 0) {
                    half_t* const bufs[5] = {e->act[1], e->act[2], e->act[3], e->act[4], e->act[5]};
                    half_t* Xo = run_d_blocks(e, B, 0, d_hi, e->act[0], bufs, y);   // fromRGB rides in the first conv
                    GLASS_HIP(hipMemcpyAsync(dmid + (size_t)c0 * dmid_bs, Xo, (size_t)B * dmid_bs * sizeof(half_t),
                                             hipMemcpyDeviceToDevice, e->cur));
                } else {
                    run_fromrgb(e, B, y, dmid + (size_t)c0 * dmid_bs);
                }
            }
            if (lpips) run_lpips_chunk(e, y, c0, B);      // VGG16 on the discriminator's stream, behind it: the chunk's image is complete
            if (overlap) GLASS_HIP(hipEventRecord(e->ev_d[k], sd));
        }
    }
    // ---- phase C: low-resolution discriminator + head (second stream) || CLIP (main stream) ------
    if (want_d) {
        e->cur = sd;
        half_t* const bufs[5] = {e->low[0], e->low[1], e->low[2], e->low[3], e->low[4]};
        half_t* Xo = run_d_blocks(e, P, d_hi, nd, dmid, bufs);
        run_d_head(e, P, Xo, Xo == e->low[0] ? e->low[1] : e->low[0]);
    }
    if (out_F) {
        if (overlap) {   // patches (written on the second stream) -> CLIP on the main stream
            GLASS_HIP(hipStreamWaitEvent(e->stream, e->ev_d[n_chunks - 1], 0));
        }
        if (clip_ov) GLASS_HIP(hipStreamWaitEvent(e->stream, e->ev_d[0], 0));   // join: CLIP finished on the second stream
    }
    e->cur = e->stream;
    return finish_pass(e, P, host_F, clip_ov, overlap ? sd : nullptr, d_F_dst, no_wait);
}

extern "C" int glass_engine_evaluate(glass_engine* e, const float* latents, int32_t P, int32_t generation,
                                     int32_t first_minibatch, const glass_noise* noise, float* out_F) {
    REQUIRE(out_F, GLASS_ERR_ARG, "null out_F");
    return run_pass(e, latents, P, generation, first_minibatch, noise, out_F, nullptr);
}

extern "C" int glass_engine_generate(glass_engine* e, const float* latents, int32_t P, int32_t generation,
                                     int32_t first_minibatch, const glass_noise* noise, float* images) {
    REQUIRE(images, GLASS_ERR_ARG, "null images");
    return run_pass(e, latents, P, generation, first_minibatch, noise, nullptr, images);
}

extern "C" int glass_engine_last_details(glass_engine* e, int32_t P, float* features, float* dis, float* sim) {
    REQUIRE(e && e->finalized, GLASS_ERR_STATE, "engine not ready");
    REQUIRE(P > 0 && P <= e->last_P, GLASS_ERR_ARG, "P exceeds the last evaluated population");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    const size_t frow = (size_t)e->cfg.clip_embed * sizeof(float);
    if (features && e->views)      // crop views: a candidate's field is view 0's feature — the whole image, as without views
        GLASS_HIP(hipMemcpy2D(features, frow, e->d_feat, frow * e->views, frow, (size_t)P, hipMemcpyDeviceToHost));
    else if (features)
        GLASS_HIP(hipMemcpy(features, e->d_feat, (size_t)P * frow, hipMemcpyDeviceToHost));
    if (dis) GLASS_HIP(hipMemcpy(dis, e->d_dis, (size_t)P * sizeof(float), hipMemcpyDeviceToHost));
    if (sim) GLASS_HIP(hipMemcpy(sim, e->d_sim, (size_t)P * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

extern "C" int glass_engine_set_clip_views(glass_engine* e, int32_t views, int32_t min_permille, int32_t flip, int32_t fixed) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(!e->finalized, GLASS_ERR_STATE, "set_clip_views: the engine is finalized (its buffers are sized in finalize: call it before)");
    REQUIRE(e->R > 0, GLASS_ERR_STATE, "set_clip_views: this engine has no generator (img2txt): there is no generated image to crop");
    REQUIRE((flip == 0 || flip == 1) && (fixed == 0 || fixed == 1), GLASS_ERR_ARG, "set_clip_views: flip and fixed must be 0 or 1");
    const glass_config& c = e->cfg;
    const int G = c.clip_res / c.clip_patch;
    const int tokens = c.clip_arch == 1 ? (c.clip_res / 4) * (c.clip_res / 4) : G * G + 1;
    if (int rc = glass_clip_views_supported(c.max_pop, tokens, c.clip_width, c.clip_resize, views, min_permille)) return rc;
    e->views = views;
    e->view_min_permille = min_permille;
    e->view_flip = flip;
    e->view_fixed = fixed;
    return GLASS_OK;
}

// ---- latent spaces / truncation ----------------------------------------------------------------
extern "C" int glass_host_layer_psi(int32_t n_lat, float psi, int32_t cutoff, float* out) {
    REQUIRE(out && n_lat >= 1, GLASS_ERR_ARG, "layer_psi: null output or no style layers");
    REQUIRE(std::isfinite(psi), GLASS_ERR_ARG, "truncation psi must be finite");
    REQUIRE(psi >= 0.f, GLASS_ERR_ARG, "truncation psi < 0 extrapolates past the average dlatent, away from the candidate: psi must be in [0, 1]");
    REQUIRE(psi <= 1.f, GLASS_ERR_ARG, "truncation psi > 1 extrapolates away from the average dlatent instead of towards it: psi must be in [0, 1]");
    REQUIRE(cutoff >= -1 && cutoff <= n_lat, GLASS_ERR_ARG,
            "truncation cutoff must be in [-1, n_lat] (-1: every layer; n_lat = " + std::to_string(n_lat) + " style layers)");
    const int ncut = cutoff < 0 ? n_lat : cutoff;
    for (int l = 0; l < n_lat; ++l) out[l] = l < ncut ? psi : 1.f;       // stylegan2/models.py:276-284
    return GLASS_OK;
}

extern "C" int glass_engine_set_latent_space(glass_engine* e, int32_t space) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(!e->finalized, GLASS_ERR_STATE, "set_latent_space: the engine is finalized (its buffers are sized in finalize: call it before)");
    REQUIRE(e->n_lat > 0, GLASS_ERR_STATE, "set_latent_space: W / W+ are latent spaces of a StyleGAN2 generator; this engine has none");
    REQUIRE(space == GLASS_LATENT_Z || space == GLASS_LATENT_W || space == GLASS_LATENT_WPLUS || space == GLASS_LATENT_SUB, GLASS_ERR_ARG,
            "set_latent_space: space must be 0 (z), 1 (w), 2 (w+) or 3 (sub)");
    e->latent_space = space;
    if (space != GLASS_LATENT_SUB) e->sub_G = e->sub_K = 0;      // a shape belongs to sub alone
    return GLASS_OK;
}

// ---- latent space sub ----------------------------------------------------------------------------
extern "C" int glass_subspace_supported(int32_t n_lat, int32_t latent_size, int32_t groups, int32_t components, const int32_t* layer_group,
                                        char* why, int32_t why_len) {
    std::string msg;
    const std::string gk = "subspace (groups " + std::to_string(groups) + ", components " + std::to_string(components) + "): ";
    if (n_lat < 1) msg = gk + "n_lat must be at least 1: the subspace is one of a StyleGAN2 generator's W";
    else if (latent_size < 4 || latent_size % 4) msg = gk + "latent_size " + std::to_string(latent_size) + " must be a multiple of 4 (the kernel moves 16 bytes along a dlatent)";
    else if (components < 1) msg = gk + "components must be at least 1";
    else if (components > latent_size) msg = gk + "components must not exceed latent_size " + std::to_string(latent_size) + " (W has no more directions)";
    else if (components > 512) msg = gk + "components must not exceed 512 (a tile of 16 candidates' coefficients is staged in 32 KB of LDS)";
    else if (groups < 1) msg = gk + "groups must be at least 1";
    else if (groups > n_lat) msg = gk + "groups must not exceed n_lat " + std::to_string(n_lat) + " (every group holds at least one style layer)";
    else if (layer_group) {
        std::vector<int> count(groups, 0);
        for (int l = 0; l < n_lat && msg.empty(); ++l) {
            const int g = layer_group[l];
            if (g < -1 || g >= groups)
                msg = gk + "layer_group[" + std::to_string(l) + "] = " + std::to_string(g) + " must be -1 (frozen) or a group index in [0, " + std::to_string(groups) + ")";
            else if (g >= 0) count[g]++;
        }
        for (int g = 0; g < groups && msg.empty(); ++g)
            if (!count[g]) msg = gk + "group " + std::to_string(g) + " is empty: every group needs at least one style layer";
    }
    if (why && why_len > 0) snprintf(why, (size_t)why_len, "%s", msg.c_str());
    REQUIRE(msg.empty(), GLASS_ERR_ARG, msg);
    return GLASS_OK;
}

extern "C" int glass_engine_set_subspace_shape(glass_engine* e, int32_t groups, int32_t components) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(e->n_lat > 0, GLASS_ERR_STATE,
            e->cfg.generator == GLASS_GEN_BIGGAN_DEEP
                ? "set_subspace_shape: the subspace is one of a StyleGAN2 generator's W; a BigGAN-deep engine has none (its row is z and class bits)"
                : "set_subspace_shape: the subspace is one of a StyleGAN2 generator's W; this engine has no generator (GPT-2 / img2txt)");
    REQUIRE(!e->finalized, GLASS_ERR_STATE, "set_subspace_shape: the engine is finalized (its buffers are sized in finalize: call it before)");
    REQUIRE(e->latent_space == GLASS_LATENT_SUB, GLASS_ERR_STATE, "set_subspace_shape: the engine's latent space is not sub: set_latent_space(3) first");
    if (int rc = glass_subspace_supported(e->n_lat, e->cfg.latent_size, groups, components, nullptr, nullptr, 0)) return rc;
    REQUIRE((long long)e->cfg.max_pop * groups * components < (1LL << 31), GLASS_ERR_ARG,
            "set_subspace_shape: max_pop * groups * components must stay below 2^31");
    e->sub_G = groups;
    e->sub_K = components;
    return GLASS_OK;
}

extern "C" int glass_engine_set_subspace(glass_engine* e, const int32_t* layer_group, const float* basis, const float* base) {
    REQUIRE(e && layer_group && basis && base, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->latent_space == GLASS_LATENT_SUB, GLASS_ERR_STATE, "set_subspace: the engine's latent space is not sub (set_latent_space before finalize)");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "set_subspace: finalize() first (it allocates the basis)");
    const int L = e->cfg.latent_size, NL = e->n_lat;
    if (int rc = glass_subspace_supported(NL, L, e->sub_G, e->sub_K, layer_group, nullptr, 0)) return rc;
    for (size_t i = 0; i < (size_t)e->sub_K * L; ++i) REQUIRE(std::isfinite(basis[i]), GLASS_ERR_ARG, "set_subspace: the basis holds a value that is not finite");
    for (size_t i = 0; i < (size_t)NL * L; ++i) REQUIRE(std::isfinite(base[i]), GLASS_ERR_ARG, "set_subspace: the base holds a value that is not finite");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    GLASS_HIP(hipStreamSynchronize(e->stream));
    GLASS_HIP(hipMemcpy(e->d_sub_group, layer_group, (size_t)NL * sizeof(int32_t), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemcpy(e->d_sub_basis, basis, (size_t)e->sub_K * L * sizeof(float), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemcpy(e->d_sub_base, base, (size_t)NL * L * sizeof(float), hipMemcpyHostToDevice));
    e->has_subspace = true;
    return e->edit.has_anchor ? compute_anchor(e) : GLASS_OK;      // the stored anchor is the row's dlatents under the subspace in force
}

// The dlatents the pass makes its styles from, through run_dlatents — the launches of a pass.
extern "C" int glass_engine_expand_latents(glass_engine* e, const float* rows, int32_t P, float* out_dlat) {
    REQUIRE(e && rows && out_dlat, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "finalize() first (weights not loaded)");
    REQUIRE(e->n_lat > 0, GLASS_ERR_STATE, "expand_latents: dlatents belong to a StyleGAN2 generator; this engine has none");
    REQUIRE(P > 0 && P <= e->cfg.max_pop, GLASS_ERR_ARG, "expand_latents: P out of range (1 .. max_pop)");
    REQUIRE(e->latent_space != GLASS_LATENT_SUB || e->has_subspace, GLASS_ERR_STATE, "expand_latents: set_subspace() first");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    const int L = e->cfg.latent_size, NL = e->n_lat;
    const size_t row = latent_row_floats(e);
    e->cur = e->stream;
    e->launch_error.clear();
    memcpy(e->h_pinned, rows, (size_t)P * row * sizeof(float));
    GLASS_HIP(hipMemcpyAsync(latent_rows_dst(e), e->h_pinned, (size_t)P * row * sizeof(float), hipMemcpyHostToDevice, e->cur));
    const bool prof = e->profiling;
    e->profiling = false;           // (profile rows belong to a pass)
    const bool ok = run_dlatents(e, P);
    e->profiling = prof;
    GLASS_HIP(hipStreamSynchronize(e->cur));
    GLASS_HIP(hipGetLastError());
    if (!ok || !e->launch_error.empty()) {
        const std::string msg = e->launch_error.empty() ? "expand_latents: the dlatents were refused" : e->launch_error;
        e->launch_error.clear();
        glass_set_error(msg);
        return GLASS_ERR_STATE;
    }
    const LatPlan lp = plan_dlatents(e->latent_space, e->trunc_psi, e->trunc_cutoff, NL);
    if (lp.layered) {
        GLASS_HIP(hipMemcpy(out_dlat, e->d_dlat, (size_t)P * NL * L * sizeof(float), hipMemcpyDeviceToHost));
    } else {      // one row serves every layer
        const size_t rb = (size_t)L * sizeof(float);
        for (int l = 0; l < NL; ++l)
            GLASS_HIP(hipMemcpy2D(out_dlat + (size_t)l * L, rb * NL, e->d_w0, rb, rb, (size_t)P, hipMemcpyDeviceToHost));
    }
    return GLASS_OK;
}

extern "C" int glass_engine_set_truncation(glass_engine* e, float psi, int32_t cutoff) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(e->n_lat > 0, GLASS_ERR_STATE, "set_truncation: the truncation trick belongs to a StyleGAN2 generator; this engine has none");
    std::vector<float> lp(e->n_lat);
    if (int rc = glass_host_layer_psi(e->n_lat, psi, cutoff, lp.data())) return rc;
    if (!e->finalized) {      // recorded; finalize checks dlatent_avg and sizes the per-layer buffer
        e->trunc_psi = psi;
        e->trunc_cutoff = cutoff;
        e->trunc_before_finalize = true;
        return GLASS_OK;
    }
    const LatPlan plan = plan_dlatents(e->latent_space, psi, cutoff, e->n_lat);
    REQUIRE(!plan.expand || !e->dlatent_avg.empty(), GLASS_ERR_STATE,
            "set_truncation: missing tensor: dlatent_avg (psi != 1 interpolates towards it; load it before finalize)");
    REQUIRE(!plan.layered || e->d_dlat, GLASS_ERR_STATE,
            "set_truncation: a cutoff inside (0, n_lat) gives every style layer its own row, and this engine was finalized without the "
            "per-layer buffer: call set_truncation (any values) before finalize, or use space w+");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    e->trunc_psi = psi;
    e->trunc_cutoff = cutoff;
    if (plan.expand)
        if (int rc = upload_lat_table(e)) return rc;
    return e->edit.has_anchor ? compute_anchor(e) : GLASS_OK;      // the stored anchor is the row's dlatents under the truncation in force
}

extern "C" int glass_engine_latent_row(glass_engine* e, int32_t* floats_per_row, int32_t* n_lat) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    if (floats_per_row) *floats_per_row = (int32_t)latent_row_floats(e);
    if (n_lat) *n_lat = e->n_lat;
    return GLASS_OK;
}

extern "C" int glass_engine_map_latents(glass_engine* e, const float* z, int32_t P, float* out_w) {
    REQUIRE(e && z && out_w, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "finalize() first (weights not loaded)");
    REQUIRE(e->n_lat > 0, GLASS_ERR_STATE, "map_latents: this engine has no StyleGAN2 mapping network");
    REQUIRE(P > 0 && P <= e->cfg.max_pop, GLASS_ERR_ARG, "map_latents: P out of range (1 .. max_pop)");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    const size_t bytes = (size_t)P * e->cfg.latent_size * sizeof(float);
    memcpy(e->h_pinned, z, bytes);
    GLASS_HIP(hipMemcpyAsync(e->d_z, e->h_pinned, bytes, hipMemcpyHostToDevice, e->cur));
    const bool prof = e->profiling;
    e->profiling = false;           // (profile rows belong to a pass)
    run_mapping(e, P);
    e->profiling = prof;
    GLASS_HIP(hipMemcpyAsync(e->h_pinned, e->d_w0, bytes, hipMemcpyDeviceToHost, e->cur));
    GLASS_HIP(hipStreamSynchronize(e->cur));
    GLASS_HIP(hipGetLastError());
    memcpy(out_w, e->h_pinned, bytes);
    return GLASS_OK;
}

extern "C" int glass_engine_last_view_details(glass_engine* e, int32_t P, float* features, float* sims, int32_t* boxes) {
    REQUIRE(e && e->finalized, GLASS_ERR_STATE, "engine not ready");
    REQUIRE(e->views > 0, GLASS_ERR_STATE, "crop views are off (glass_engine_set_clip_views)");
    REQUIRE(P > 0 && P <= e->last_P, GLASS_ERR_ARG, "P exceeds the last evaluated population");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    const size_t n = (size_t)P * e->views;
    if (features) GLASS_HIP(hipMemcpy(features, e->d_feat, n * e->cfg.clip_embed * sizeof(float), hipMemcpyDeviceToHost));
    if (sims) GLASS_HIP(hipMemcpy(sims, e->d_view_sim, n * sizeof(float), hipMemcpyDeviceToHost));
    if (boxes) memcpy(boxes, &e->view_boxes.box[0][0], (size_t)e->views * 4 * sizeof(int32_t));
    return GLASS_OK;
}

extern "C" int glass_engine_last_F_device(glass_engine* e, int32_t P, void** dev_ptr) {
    REQUIRE(e && dev_ptr, GLASS_ERR_ARG, "null argument");
    REQUIRE(P > 0 && P == e->last_P && e->d_F, GLASS_ERR_STATE, "no evaluate() of this population size has run");
    *dev_ptr = e->d_F;
    return GLASS_OK;
}

extern "C" int glass_engine_last_gpu_ms(glass_engine* e, float* ms) {
    REQUIRE(e && ms, GLASS_ERR_ARG, "null argument");
    *ms = e->last_ms;
    return GLASS_OK;
}

extern "C" int glass_engine_set_profiling(glass_engine* e, int32_t on) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    e->profiling = on != 0;
    return GLASS_OK;
}

extern "C" int glass_engine_set_overlap(glass_engine* e, int32_t on) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    // 0: one stream; 1: D + CLIP of chunk k under the synthesis of chunk k + 1; 2: CLIP on the second stream next to D (default)
    e->overlap = on == 1;
    e->clip_overlap = on == 2;
    return GLASS_OK;
}

extern "C" int glass_engine_set_biggan_tap(glass_engine* e, int32_t block) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(e->cfg.generator == GLASS_GEN_BIGGAN_DEEP, GLASS_ERR_STATE, "not a BigGAN-deep engine");
    REQUIRE(block >= -2 && block < (int)e->bg.blocks.size(), GLASS_ERR_ARG, "no such GenBlock");
    e->bg_tap = block;
    e->bg_tap_data.clear();
    return GLASS_OK;
}

extern "C" int glass_engine_get_biggan_tap(glass_engine* e, float* out, int64_t capacity, int32_t dims[4]) {
    REQUIRE(e && dims, GLASS_ERR_ARG, "null argument");
    for (int i = 0; i < 4; ++i) dims[i] = e->bg_tap_dims[i];
    REQUIRE(!e->bg_tap_data.empty(), GLASS_ERR_STATE, "no tap recorded (set_biggan_tap, then evaluate / generate)");
    if (out) {
        REQUIRE(capacity >= (int64_t)e->bg_tap_data.size(), GLASS_ERR_ARG, "tap buffer too small");
        memcpy(out, e->bg_tap_data.data(), e->bg_tap_data.size() * sizeof(float));
    }
    return GLASS_OK;
}

extern "C" int glass_engine_set_profile_filter(glass_engine* e, const char* kernel_substr) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    e->prof_filter = kernel_substr ? kernel_substr : "";
    return GLASS_OK;
}

extern "C" int glass_engine_get_profile(glass_engine* e, glass_prof_row* rows, int32_t max_rows, int32_t* n_rows) {
    REQUIRE(e && n_rows, GLASS_ERR_ARG, "null argument");
    const int n = (int)e->prof_rows.size();
    *n_rows = n;
    if (rows)
        for (int i = 0; i < std::min(n, (int)max_rows); ++i) rows[i] = e->prof_rows[i];
    return GLASS_OK;
}

extern "C" int glass_device_info(int32_t device, char* name, int32_t name_len, int32_t* cus, int64_t* hbm_bytes) {
    hipDeviceProp_t prop;
    GLASS_HIP(hipGetDeviceProperties(&prop, device));
    if (name && name_len > 0)   // the marketing name the driver reports can be generic ("AMD Radeon Graphics"): the ISA name says what it is
        snprintf(name, (size_t)name_len, "%s (%s)", prop.name, prop.gcnArchName);
    if (cus) *cus = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return GLASS_OK;
}
