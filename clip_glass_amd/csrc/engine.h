// engine.h — host-side engine object behind the C ABI (include/glass.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/glass.h"
#include "common.h"
#include "kernels.h"

void glass_set_error(const std::string& s);
#define GLASS_HIP(call)                                                                        \
    do {                                                                                       \
        hipError_t _e = (call);                                                                \
        if (_e != hipSuccess) {                                                                \
            glass_set_error(std::string(#call) + " failed: " + hipGetErrorString(_e) + " at " + \
                            __FILE__ + ":" + std::to_string(__LINE__));                        \
            return GLASS_ERR_HIP;                                                              \
        }                                                                                      \
    } while (0)

struct HostTensor {
    std::vector<int64_t> dims;
    std::vector<float> data;
};

struct GConv {  // one modulated 3x3 conv of the synthesis network
    int cin, cout, res_in, res_out, up;
    int style_idx, style_off, ds_off, noise_idx;
    half_t* w = nullptr;   // [9][Neff][cin]
    half_t* w_up = nullptr;  // up layers: un-folded [9][cout][cin]
    half_t* wm = nullptr;    // pre-modulated per-sample weights [P][welems] (small high-res layers only)
    long long welems = 0;
    bool premod = false;
    float* wsq = nullptr;  // [cin][cout]
    float* bias = nullptr;
    float noise_strength = 0.f;
};
struct GRgb {
    int cin, res, style_idx, style_off;
    float* w = nullptr;  // [3][cin]
    float* bias = nullptr;
};
struct DBlock {
    int cin, cout, res;
    half_t *w0 = nullptr, *w1 = nullptr, *wskip = nullptr;
    float *b0 = nullptr, *b1 = nullptr;
};
struct ClipBlock {
    float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    half_t *w_qkv, *w_out, *w_fc, *w_proj;
    float *b_qkv, *b_out, *b_fc, *b_proj;
};

// CLIP's ModifiedResNet image tower (clip.cpp, clip_resnet.hip; clip/model.py:9-149)
struct RnConv {            // a convolution and the BatchNorm behind it
    int cin = 0, cout = 0, ks = 1;
    half_t* w = nullptr;   // [ks*ks][cout][cin] fp16, un-scaled: BatchNorm is NOT folded in
    float *a = nullptr, *s = nullptr;   // [cout] fp32: A = gamma / sqrt(var + 1e-5), S = beta - mean * A
};
struct RnBlock {           // Bottleneck: 1x1 - 3x3 - [avgpool] - 1x1, + identity or BN(1x1(avgpool(x)))
    int res_in = 0, stride = 1;
    bool has_down = false;
    RnConv c1, c2, c3, down;
};
struct RnState {
    half_t* stem_w1 = nullptr;          // [27][w/2]
    float *stem_a1 = nullptr, *stem_s1 = nullptr;
    RnConv stem2, stem3;
    std::vector<RnBlock> blocks;
    float *pos = nullptr, *b_qkv = nullptr, *cproj_wt = nullptr, *cproj_b = nullptr;   // cproj_wt [C][embed]
    half_t* w_qkv = nullptr;            // [3 C][C]: q_proj | k_proj | v_proj
    // activations: every buffer holds `cap` halfs — the largest map of the tower for max_pop images, at least 64 rows of the widest one
    // (a GEMM of fewer than 64 rows runs on rows padded to 64 in these buffers)
    half_t* buf[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    half_t *tok = nullptr, *qkv = nullptr, *att = nullptr;
    float* cls = nullptr;
    size_t cap = 0;
};

// Perceptual objective: LPIPS on VGG16 (lpips.cpp, lpips.hip; stylegan2/external_models/lpips.py:34-78).  All of it is allocated only
// with glass_config::lpips_size > 0.
struct LpState {
    int S = 0, box = 0, sub = 0;         // VGG input side; R / S; images one walk carries (GLASS_LPIPS_SUB at most — results do not depend on it)
    half_t* w1 = nullptr;                // features.0: [27][64], row (ci, ky, kx)
    float* b1 = nullptr;
    RnConv conv[12];                     // features.2 .. 28 as gemm_tiled's BatchNorm form: a = 1, s = bias
    float* ones = nullptr;               // [512]
    float* lin[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    half_t* in = nullptr;                // [sub][S][S][4]
    half_t* buf[2] = {nullptr, nullptr}; // ping-pong, sub S S 64 halfs each (the first slice's map, the largest)
    half_t* tgt[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};    // the target's five slice outputs (set_lpips_target)
    half_t* pair[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // glass_engine_lpips: x1's maps of the pair in flight
    float *stage = nullptr, *part = nullptr, *d = nullptr, *d_one = nullptr;   // one caller image fp32; head partials; d [max_pop]; the utility's value
    bool has_target = false;
};
#define GLASS_LPIPS_SUB 16

// BigGAN-deep generator (biggan.cpp)
struct BgBlock {   // GenBlock: bn0-relu-conv1x1 / bn1-relu-[up]-conv3x3 / bn2-relu-conv3x3 / bn3-relu-conv1x1 + skip
    int cin, cout, mid, up, res_in;
    int bn_off[4];           // column offsets of the four batch norms in the affine tables
    half_t* w[4] = {nullptr, nullptr, nullptr, nullptr};   // [ks*ks][cout][cin] fp16, spectral norm folded
    float* b3 = nullptr;     // conv_3 bias (the other biases are folded into the next BN's shift)
};
struct BgState {
    int R = 0, Ctot = 0, zd = 0, nc = 0, c0 = 0;
    float *et = nullptr, *genz_wt = nullptr, *genz_b = nullptr;
    float *bn_wt = nullptr, *bn_bias = nullptr, *bn_inv_std = nullptr, *bn_mean = nullptr, *bn_prebias = nullptr;
    std::vector<BgBlock> blocks;
    int attn_before = -1, attn_C = 0, attn_res = 0;
    half_t *attn_w_tpg = nullptr, *attn_w_o = nullptr;
    int final_bn_off = 0, rgb_cpad = 32;
    half_t* rgb_w = nullptr;
    float* rgb_b = nullptr;
    // activations
    half_t* tab16 = nullptr;   // fp16 copy of tab
    float *cond = nullptr, *tab = nullptr, *h32 = nullptr, *a_S = nullptr;
    half_t *x[2] = {nullptr, nullptr}, *t1 = nullptr, *t2 = nullptr, *t3 = nullptr;
    half_t *a_T = nullptr, *a_theta = nullptr, *a_phi = nullptr, *a_gT = nullptr, *a_P = nullptr, *a_O = nullptr;
};
int glass_biggan_finalize(glass_engine* e);       // weights -> device layouts + activation buffers
int glass_biggan_prepare(glass_engine* e, int P); // cond vectors + batch-norm tables for the population in d_z
// synthesize candidates [c0, c0 + B) -> planar fp32 RGB in (-1, 1) at `y` [B][3][R][R]
int glass_biggan_chunk(glass_engine* e, int c0, int B, float* y);

// What one GPT-2 token step launches for a geometry (gpt2_host.cpp, plan_gpt2_step): every choice is made here, before the step runs.
struct Gpt2StepPlan {
    bool fused = false;       // LayerNorm inside the products, residual + statistics passes; false: the unfused step, which takes every shape
    bool rowblk = false;      // o / fc in the complete-output form (no finishing launch behind them)
    bool att_step = false;    // Tmax <= 64: one wave per (sequence, head), which sums the qkv slices itself
    StepGemm qkv, o, fc, pr;  // per layer: qkv, attention output, MLP first, MLP second
    Gpt2Head head;            // head + its pick (a tail where the width allows); empty: `logits`, then launch_argmax / launch_gpt2_sample
    StepGemm logits;
};

struct ProfEvent {
    std::string name;
    double flops, bytes;
    hipEvent_t e0, e1;
};

struct glass_engine {
    glass_config cfg;
    int R = 0;        // output resolution
    int n_style = 0;  // number of style (affine) layers
    int S_total = 0, D_total = 0;
    int chunk = 0;
    bool finalized = false;
    hipStream_t stream = nullptr, stream_d = nullptr, cur = nullptr;  // main, second (D/resize), current target
    bool overlap = false, clip_overlap = false;
    std::vector<hipEvent_t> ev_g, ev_d;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_noise = nullptr;
    float last_ms = 0.f;
    int last_P = 0;
    std::string launch_error;   // a launcher refused a layer during the pass (reported by run_pass; nothing aborts)

    std::map<std::string, HostTensor> host;
    std::vector<void*> allocs;

    // ---- G ----
    std::vector<float*> map_wt, map_b;  // [L][L] transposed, pre-scaled
    float *style_wt = nullptr, *style_b = nullptr;  // [L][S_total], [S_total]
    int *d_style_off = nullptr, *d_style_len = nullptr;
    std::vector<int> style_off, style_len;
    half_t* g_const = nullptr;  // [4][4][C0]
    void* d_demod_desc = nullptr;  // DenseDesc[gconv.size()] for the single-launch demodulation
    int demod_max_n = 0;
    std::vector<GConv> gconv;
    std::vector<GRgb> grgb;
    BgState bg;
    // ---- dlatents: latent space + truncation trick (glass_engine_set_latent_space / set_truncation; stylegan2.cpp plan_dlatents) ----
    int latent_space = GLASS_LATENT_Z, n_lat = 0;   // n_lat = 2 n_blocks style layers (stylegan2/models.py:890-896); 0: not a StyleGAN2 engine
    float trunc_psi = 1.f;
    int trunc_cutoff = -1;
    bool trunc_before_finalize = false;   // set_truncation was called before finalize: the per-layer buffer below is allocated
    std::vector<float> dlatent_avg;       // host [L]; empty: the tensor was not loaded
    float* d_lat_tab = nullptr;           // psi[lat_pad] | dlatent_avg[L]: allocated with the first truncation that needs it
    int lat_pad = 0;
    float* d_dlat = nullptr;              // [max_pop][n_lat][L] per-layer dlatents: only for space W+ or after trunc_before_finalize
    StyleTile* d_style_tiles = nullptr;   // (segment, n0) tiles of styles_layered_kernel, built with d_dlat
    int n_style_tiles = 0;
    // ---- latent space sub (include/glass.h "Subspace latent space"): nothing here is allocated unless the space is GLASS_LATENT_SUB ----
    int sub_G = 0, sub_K = 0;             // glass_engine_set_subspace_shape; 0: not set
    bool has_subspace = false;            // glass_engine_set_subspace was called
    float* d_sub_c = nullptr;             // [max_pop][G][K] coefficient rows: where run_pass puts the rows of a pass
    int* d_sub_group = nullptr;           // [n_lat]
    float *d_sub_basis = nullptr, *d_sub_base = nullptr;   // [K][L], [n_lat][L]
    // ---- D ----
    float *d_frgb_w = nullptr, *d_frgb_b = nullptr;
    std::vector<DBlock> dblk;
    half_t* d_final_w = nullptr;
    float* d_final_b = nullptr;
    int d_final_cpad = 0;
    half_t* d_dense0_w = nullptr;
    float *d_dense0_b = nullptr, *d_dense1_wt = nullptr, *d_dense1_b = nullptr;
    // ---- CLIP ----
    half_t* c_patch_w = nullptr;
    float *c_cls = nullptr, *c_pos = nullptr, *c_lnpre_g = nullptr, *c_lnpre_b = nullptr;
    float *c_lnpost_g = nullptr, *c_lnpost_b = nullptr, *c_proj = nullptr;
    std::vector<ClipBlock> cblk;
    ResizeTapsDev rz;          // clip_resize 1 / 2: the antialiased resize's tap table (finalize_preprocess)
    RnState rn;                // clip_arch 1: the ResNet tower instead of c_* / cblk
    // crop views (glass_engine_set_clip_views; views 0: off — one image per candidate, nothing below is touched)
    int views = 0, view_min_permille = 0, view_flip = 0, view_fixed = 0;
    ViewBoxes view_boxes = {};          // the boxes of the current / last evaluate(): one set for every candidate of the pass
    float* d_view_sim = nullptr;        // [max_pop][views]
    LpState lp;                // perceptual objective (cfg.lpips_size > 0; nothing of it exists otherwise)
    // GPT-2 (optional, fp32; config C5)
    struct Gpt2Block { float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *w_qkv, *b_qkv, *w_o, *b_o, *w_fc, *b_fc, *w_pr, *b_pr; };
    std::vector<Gpt2Block> gblk;
    float *g_wte = nullptr, *g_wpe = nullptr, *g_lnf_g = nullptr, *g_lnf_b = nullptr;
    int g_vocab = 0, g_dim = 0, g_npos = 0;
    // decode workspace, kept between calls (one geometry at a time): buffers + the captured single-token step
    struct Gpt2Work {
        int P = 0, nctx = 0, length = 0;
        int *d_tok = nullptr, *d_gen = nullptr, *d_state = nullptr, *d_samp = nullptr;   // d_samp: the sampler's per-call words (GPT2_SP_*)
        int sample = -1;          // mode the step was planned and its graph recorded in: 0 greedy, 1 stochastic (-1: neither yet)
        Gpt2StepPlan plan;        // the token step of this geometry in that mode
        float *x = nullptr, *ln = nullptr, *qkv = nullptr, *att = nullptr, *hid = nullptr, *last = nullptr, *logits = nullptr,
              *kc = nullptr, *vc = nullptr, *part = nullptr, *stats = nullptr, *pairs = nullptr, *pst = nullptr;   // stats: [P][2] LayerNorm {mean, rstd} of the fused step
        size_t part_elems = 0;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        float last_ms = 0.f;      // device time of the last decode (hipEvents around the passes)
        std::vector<void*> owned; // every buffer above (owned_alloc), freed by gpt2_work_free
    } gwork, gwork_alt;       // current workspace + the previous geometry's (glass_engine_gpt2_decode's row groups: 64 rows and a remainder)
    // text tower (optional)
    std::vector<ClipBlock> tblk;
    float *t_tok = nullptr, *t_pos = nullptr, *t_lnf_g = nullptr, *t_lnf_b = nullptr, *t_proj = nullptr;
    struct TextWork {      // encode_text's activations, kept between calls of the same size (eight hipMalloc / hipFree pairs per call otherwise)
        int n_texts = 0;
        int *d_tok = nullptr, *d_rows = nullptr;
        float *x = nullptr, *cls = nullptr, *feat = nullptr;
        half_t *ln16 = nullptr, *qkv = nullptr, *att = nullptr, *hid = nullptr;
        std::vector<void*> owned;   // every buffer above (owned_alloc), freed by text_work_free
    } twork;
    int t_width = 0, t_ctx = 0, t_vocab = 0;

    // ---- activations / scratch ----
    half_t* d_s16 = nullptr;   // fp16 copy of d_s (normalised styles)
    half_t* ws_a = nullptr;   // conv_gemm.hip scratch: patch matrix of a low-resolution layer (cap_a halfs) and its fp32 product (cap_c)
    float* ws_c = nullptr;
    half_t* ws_a2 = nullptr;  // second scratch set: launches on the second stream never share a buffer with the main stream's
    float* ws_c2 = nullptr;
    long long cap_a = 0, cap_c = 0;
    half_t* d_trgb_tab = nullptr;   // [P][2][16][<= 512] fp16: toRGB weight tables of the fused conv epilogues
    float* d_trgb_part = nullptr;   // [C / 128][chunk][3][res][res]: toRGB partial sums of the blocks wider than 128 channels
    float *d_z = nullptr, *d_w0 = nullptr, *d_w1 = nullptr, *d_s = nullptr, *d_smax = nullptr, *d_epsrow = nullptr,
          *d_dscale = nullptr;
    std::vector<float*> d_noise;  // per noise layer: [n_mb_max][res*res]
    half_t* act[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // per-chunk, high resolution
    half_t* low[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // whole population, res <= low_res
    float* ylow[2] = {nullptr, nullptr};
    int low_res = 32, n_low = 0;
    size_t act_elems = 0;
    float* ybuf[4] = {nullptr, nullptr, nullptr, nullptr};
    float* d_img = nullptr;
    half_t *d_patches = nullptr, *d_ln16 = nullptr, *d_qkv = nullptr, *d_attn = nullptr, *d_hid = nullptr;
    float *d_pe = nullptr, *d_x = nullptr, *d_cls = nullptr, *d_feat = nullptr, *d_sim = nullptr, *d_dis = nullptr,
          *d_F = nullptr, *d_dh = nullptr, *d_dh_part = nullptr;
    half_t* d_dfin = nullptr;
    float* h_pinned = nullptr;
    size_t h_pinned_bytes = 0;

    // ---- BigGAN per-block tap (diagnostic: localises a mismatch to the first wrong GenBlock) ----
    int bg_tap = -2;                       // -2 off; -1 self-attention output; i >= 0: output of GenBlock i
    std::vector<float> bg_tap_data;        // [B][R][R][C] NHWC of the first chunk
    int bg_tap_dims[4] = {0, 0, 0, 0};
    // ---- profiling ----
    bool profiling = false;
    std::string prof_filter;                       // non-empty: only launches of kernels containing this substring
    std::map<std::string, std::string> tag_kernel;  // layer tag -> kernel symbol used in the previous pass
    std::vector<ProfEvent> prof_events;
    std::vector<glass_prof_row> prof_rows;
    std::vector<hipEvent_t> event_pool;
    size_t event_next = 0;
    // ---- the CLIP targets: a prompt set (glass_engine_set_targets), or glass_engine_set_target's one feature as entry 0 with weight 1,
    // W = 1, mode sum (`single`); T 0: none yet.  The head ends in one cosine_set_kernel launch either way (score.hip) ----
    struct PromptSet {
        int T = 0, mode = 0;                // entries; 0 sum, 1 pareto
        bool single = false;                // set_target's set of one: no prompt set as far as the API is concerned
        bool given() const { return T > 0 && !single; }      // a set given by set_targets
        float W = 0.f;                      // sum |w_t|
        float *d_targets = nullptr, *d_weights = nullptr, *d_sim = nullptr;    // [16][clip_embed], [16], [max_pop][16] (rows of T in use): alloc_buffers
        // own prompts of an island search (glass_engine_set_island_weights; allocated by its first call): weights [islands][isl_T], sum |w| [islands]
        float *d_isl_weights = nullptr, *d_isl_W = nullptr;
        int isl_T = 0;
    } pset;
    // ---- device search (glass_engine_set_search; pop 0: off — nothing below is allocated or touched) ----
    struct Search {
        int nsga = 0, n_var = 0, cur = 0;   // cur: which of X[2] holds the population
        int n_real = 0;                     // mixed rows (glass_engine_set_search_mixed): the real columns in front of the bits; 0: all real
        GaParams g = {};                    // g.pop 0: off
        bool ready = false;                 // search_init has run
        int varied_gen = -1;                // the generation whose offspring Xoff holds
        float *X[2] = {nullptr, nullptr}, *Xoff = nullptr, *F = nullptr;   // [pop][n_var] x 3; F [2 pop][n_obj]: population rows, then offspring rows
        int *rank = nullptr, *flags = nullptr, *chosen = nullptr, *counts = nullptr;
        double* cd = nullptr;
        // sep-CMA-ES (algorithm GLASS_SEARCH_CMAES; include/glass.h "Device search: sep-CMA-ES"): the generation's rows are Xoff and their F the
        // offspring half of F, so search_evaluate is the GA's; of the buffers above only Xoff, F and counts are allocated
        bool cma = false;
        CmaState cs = {};                   // cs.m holds m, d, p_sigma, p_c back to back ([4][n_var])
        // islands (include/glass.h "Device search: islands"; glass_engine_set_search_islands): 0 — the setter was never called, which the
        // island entry points, the islands' own prompts and the noise planes of a pass look at.  Every buffer and launch knows k() alone: the
        // buffers hold k() populations of g.pop rows back to back, F is the populations' plane [k() pop][n_obj] followed by the offspring's,
        // counts is [k()][3], and the island is the kernels' last grid dimension — a single search is the one island 0
        int islands = 0, migrate_every = 0, migrants = 1;
        int survived_gen = -1;              // the generation whose survival the populations hold and whose migration has not run
        bool own_prompts = false;           // glass_engine_set_island_weights: pset's island table is in use
        int k() const { return islands ? islands : 1; }
        int rows() const { return k() * g.pop; }
    } search;
    int noise_period = 0;                   // minibatches per island while a pass of an island search runs (upload_noise); 0 otherwise
    int island_row0 = -1;                   // the first search row of such a pass (the rows' islands in the head); -1 otherwise
    long long latent_uploads = 0, latent_upload_rows = 0;   // host-to-device latent copies of the pass so far (glass_engine_latent_uploads)
    // ---- image editing (include/glass.h "Image editing"; edit.cpp).  Nothing below is allocated or touched by an engine that has no
    // anchor (cfg.anchor 0) and never calls glass_engine_set_direction_source ----
    struct Edit {
        // latent anchor
        std::vector<float> anchor_row;      // the caller's row (floats_per_row), kept so that set_truncation can recompute the dlatents
        float* d_anchor = nullptr;          // [n_lat][L]: the row's dlatents, after mapping and truncation
        float* d_dist = nullptr;            // [max_pop]: d of the last pass
        bool has_anchor = false;
        // direction source
        bool has_source = false;            // a source image is set: the similarity is cosine_set_kernel's directional form
        bool rows_valid = false;            // d_src holds the rows of d_img under `boxes`
        float* d_img = nullptr;             // [3][R][R] in [-1, 1]
        float* d_src = nullptr;             // [max(views, 1)][clip_embed] unit rows
        ViewBoxes boxes = {};               // crop views: the boxes d_src was made with
    } edit;
};
inline int anchor_column(const glass_config& c) { return c.anchor && c.anchor_lambda == 0.f ? 1 : 0; }      // the anchor distance is its own (last) column of F

// ------------------------------------------------------------------------------------
// helpers shared by the host files (engine.cpp, stylegan2.cpp, clip.cpp, gpt2_host.cpp, biggan.cpp)
// ------------------------------------------------------------------------------------
#define REQUIRE(cond, code, msg)          \
    do {                                  \
        if (!(cond)) {                    \
            glass_set_error(msg);         \
            return code;                  \
        }                                 \
    } while (0)

// ------------------------------------------------------------------------------------
// allocation / upload helpers
// ------------------------------------------------------------------------------------
// hipMalloc into the list that owns the buffer: the engine's (dev_alloc), or that of a workspace which is rebuilt when its geometry
// changes (TextWork, Gpt2Work), so that the free is a loop over the list
template <typename T>
inline hipError_t owned_alloc(std::vector<void*>& owned, T** p, size_t n) {
    void* q = nullptr;
    const hipError_t err = hipMalloc(&q, n * sizeof(T));
    if (err != hipSuccess) return err;
    owned.push_back(q);
    *p = (T*)q;
    return hipSuccess;
}
template <typename T>
inline int dev_alloc(glass_engine* e, T** p, size_t n) {
    const hipError_t err = owned_alloc(e->allocs, p, std::max<size_t>(n, 1));
    if (err == hipSuccess) return GLASS_OK;
    glass_set_error(std::string("hipMalloc failed: ") + hipGetErrorString(err));
    return GLASS_ERR_NOMEM;
}
template <typename T>
inline int upload(glass_engine* e, T** p, const std::vector<T>& v) {
    int rc = dev_alloc(e, p, v.size());
    if (rc) return rc;
    GLASS_HIP(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return GLASS_OK;
}

inline const HostTensor* find(glass_engine* e, const std::string& name) {
    auto it = e->host.find(name);
    return it == e->host.end() ? nullptr : &it->second;
}
#define GET(var, name)                                                            \
    const HostTensor* var = find(e, name);                                        \
    REQUIRE(var != nullptr, GLASS_ERR_STATE, std::string("missing tensor: ") + (name))

inline size_t numel(const HostTensor* t) {
    size_t n = 1;
    for (auto d : t->dims) n *= (size_t)d;
    return n;
}

// profiling scope (hipEvent pair per launch when enabled)
struct Prof {
    glass_engine* e;
    bool on;
    ProfEvent pe;
    // name == nullptr: no scope (the text tower's launches are never profiled)
    Prof(glass_engine* e_, const char* name, double flops, double bytes) : e(e_), on(name && e_->profiling) {
        if (on && !e->prof_filter.empty()) {   // only launches whose kernel symbol (as of the previous pass) matches
            auto it = e->tag_kernel.find(name);
            on = it != e->tag_kernel.end() && it->second.find(e->prof_filter) != std::string::npos;
        }
        if (!on) return;
        auto get = [&]() {
            if (e->event_next == e->event_pool.size()) {
                hipEvent_t ev;
                hipEventCreate(&ev);
                e->event_pool.push_back(ev);
            }
            return e->event_pool[e->event_next++];
        };
        pe.name = name;
        pe.flops = flops;
        pe.bytes = bytes;
        pe.e0 = get();
        pe.e1 = get();
        hipEventRecord(pe.e0, e->cur);
    }
    ~Prof() {
        if (!on) return;
        hipEventRecord(pe.e1, e->cur);
        e->prof_events.push_back(pe);
    }
    // the launch went to kernel `k`: the row is named tag@k, and set_profile_filter() finds the tag's kernel in the next pass
    void ran(const char* tag, const char* k) {
        if (on) pe.name = std::string(tag) + "@" + k;
        if (e->profiling) e->tag_kernel[tag] = k;
    }
    void drop() { on = false; }   // the launcher refused: nothing ran in this scope
};
// One profile row around `launch`, which launches on e->cur and returns the kernel's name, or nullptr where its launcher refused the shape:
// the row is then dropped and the refusal kept for the wait behind the launches (`why`: what else the refusal can mean).  Whether it ran.
template <class Launch>
bool profiled_launch(glass_engine* e, const char* tag, double bytes, Launch launch, const char* why = "") {
    Prof pr(e, tag, 0, bytes);
    const char* k = launch();
    if (k) pr.ran(tag, k);
    else { pr.drop(); e->launch_error = std::string(tag) + ": the launcher refused the shape" + why; }
    return k != nullptr;
}

void collect_profile(glass_engine* e);
ConvKernel choose_conv(const ConvParams& p);   // the single-kernel conv families in the engine's order; empty: conv_gemm / conv_direct (run_conv)
void run_conv(glass_engine* e, const ConvParams& p, const char* tag, double flops, double bytes);
void run_chosen(glass_engine* e, const ConvKernel& k, const ConvParams& p, const char* tag, double flops, double bytes);   // k: a chooser's answer for p
void run_gemm(glass_engine* e, const GemmParams& p, const char* tag);
ConvParams conv_defaults();
// out[M][N] = a[M][K] x w[N][K]^T (+ bias), written as `mode` says (common.h GemmParams: fp16 to out16 for modes 0 / 1, fp32 to out32 above)
GemmParams gemm_params(const half_t* a, const half_t* w, int M, int N, int K, const float* bias, int mode, half_t* out16, float* out32,
                       int cand_rows);

// ---- StyleGAN2 (stylegan2.cpp) ----
#pragma GCC visibility push(hidden)   // called from engine.cpp only: the library's exported symbols stay what they were
int finalize_generator(glass_engine* e);
int finalize_discriminator(glass_engine* e);
int upload_noise(glass_engine* e, int P, int generation, int first_mb, const glass_noise* noise);
// What a pass launches between the uploaded rows and the style table, decided before anything is launched:
//   map: pixel norm + mapping network (space z).  expand: dlatent_expand_kernel applies layer_psi (psi != 1 on at least one layer).
//   layered: the rows differ per style layer (space w+ or sub, or a cutoff inside (0, n_lat)): [P][n_lat][L] in d_dlat and
//   styles_layered_kernel; otherwise ONE row per candidate in d_w0 and the single launch_dense styles launch.
struct LatPlan { bool map, expand, layered; };
LatPlan plan_dlatents(int space, float psi, int cutoff, int n_lat);
size_t latent_row_floats(const glass_engine* e);   // floats evaluate / generate read per row
float* latent_rows_dst(const glass_engine* e);     // where the rows of a pass go: d_z (z), d_w0 (w), d_dlat (w+), d_sub_c (sub)
int upload_lat_table(glass_engine* e);             // layer_psi | dlatent_avg -> d_lat_tab (allocates it on first use)
void run_mapping(glass_engine* e, int P);          // d_z -> d_w0
bool run_dlatents(glass_engine* e, int P);         // the uploaded rows -> the dlatents the styles are made from (mapping, truncation); false: refused
void run_styles(glass_engine* e, int P);           // run_dlatents, then the style table, demodulation and the per-sample weights
void run_g_blocks(glass_engine* e, int c0, int B, int b_lo, int b_hi, const half_t* x, long long xbs, half_t* const pp[2],
                  const float* yprev, float* const yb[2], const half_t** x_out, const float** y_out);
void run_fromrgb(glass_engine* e, int B, const float* y, half_t* X);
half_t* run_d_blocks(glass_engine* e, int B, int i_lo, int i_hi, half_t* X, half_t* const bufs[5], const float* rgb_y = nullptr);
void run_d_head(glass_engine* e, int P, const half_t* X, half_t* scratch);
// D's dense head as run_d_head launches it, shared with the diagnostic op: dfin [P][16 CL] fp16, w0 [CL][16 CL] fp16, b0 [CL], w1t [CL][1],
// b1 [1]; part: 16 P CL floats (nullptr: no split form), dh [P][CL] (the unsplit form's first layer), dis [P]
struct DHead {
    const half_t *dfin, *w0;
    const float *b0, *w1t, *b1;
    float *part, *dh, *dis;
    int P, CL;
};
GemmParams d_head_dense0(const DHead& h);                         // the first layer as one product (bias + lrelu * sqrt2 -> dh)
const char* launch_d_head_split(const DHead& h, hipStream_t st);  // split-K first layer + dense01_finish; nullptr: not applicable, nothing launched
void launch_d_head_dense1(const DHead& h, hipStream_t st);        // dh -> dis
#pragma GCC visibility pop

// ---- CLIP (clip.cpp) ----
int clip_patch_k(const glass_config& c);     // the patch-embedding GEMM's K: 3 patch^2 padded to gemm_tiled's K step
int finalize_clip(glass_engine* e);
int finalize_preprocess(glass_engine* e);
void text_work_free(glass_engine* e);
double clip_resize_bytes(const glass_engine* e, int B);
void run_clip_resize(glass_engine* e, const float* y, int B, half_t* patches);
// the image tower on e->cur, for the P images whose patch operand is in d_patches: patch embedding + ln_pre, layers [l0, l1), and the
// head (ln_post, projection, cosine against the target); run_clip is all of it.  views > 0 (the pass with crop views): the P images are
// P / views candidates' views, and the head ends in the per-view cosines and their mean per candidate.  views < 0: the features alone, no
// cosine launch (the direction source's own encoding, edit.cpp).
void run_clip_embed(glass_engine* e, int P);
void run_clip_layers(glass_engine* e, int P, int l0, int l1);
void run_clip_head(glass_engine* e, int P, int views = 0);
void run_clip(glass_engine* e, int P, int views = 0);
// images the tower's buffers hold: max_pop, times the views when they are on
inline size_t clip_max_images(const glass_engine* e) { return (size_t)e->cfg.max_pop * (size_t)std::max(e->views, 1); }
inline int pass_images(const glass_engine* e, int P) { return P * std::max(e->views, 1); }      // images of a pass over P candidates
inline int sim_columns(const glass_config& c) { return std::max(c.sim_columns, 1); }      // similarity columns of F (0 and 1: the one of today)
int clip_n_layers(const glass_engine* e);     // what run_clip_layers counts: transformer blocks (ViT) or bottlenecks (ResNet)
int alloc_clip_resnet(glass_engine* e);       // the ResNet tower's activation buffers (clip_arch 1)
// The ResNet tower's GEMMs as the walker sets them up (shared with the diagnostic ops).  1 x 1 conv + BN (+ res) (+ ReLU) over M rows: fewer than
// 64 rows are run as 64 — x, res and y must hold max(M, 64) rows.  3 x 3 (stride 1, pad 1, Cin % 64 == 0) + BN + ReLU through the implicit patch matrix.
GemmParams rn_gemm_1x1(const half_t* x, const RnConv& c, int M, int cand_rows, const half_t* res, int relu, half_t* y);
GemmParams rn_gemm_3x3(const half_t* x, const RnConv& c, int B, int H, int W, half_t* y);
// reference conv weight [cout][cin][ks][ks] -> [ks*ks][cout][cin] fp16
std::vector<_Float16> rn_pack_conv(const float* w, int cout, int cin, int ks);
// Stream mode 2: the patch embedding and this many layers of CLIP's image tower run on the MAIN stream, alone on the chip, before the
// discriminator starts; the rest of the tower runs on the second stream beside it.  Forked right behind the resize (rounds 2-5), the tower's
// first launch raced the discriminator's first kernel — a persistent kernel that fills every CU for 3.9 ms — and lost about every other
// process: 31.0-31.5 ms per pass against 29.6 with the embedding and ONE layer in front (sweep 0 / 1 / 2 / 3 / 4 / 6 / 8 / 10 / 12 layers:
// 29.66 / 29.59 / 29.60 / 29.74 / 29.79 / 29.91 / 29.96 / 30.13 / 30.53 ms, three runs each within 0.1 ms; DESIGN section 5 "Round 6").
#define GLASS_CLIP_SERIAL_LAYERS 1
std::vector<_Float16> to_half(const float* p, size_t n, float scale = 1.f);
std::vector<float> scaled(const float* p, size_t n, float scale);
std::vector<float> transposed(const float* W, int N, int K, float coef);


// ---- perceptual objective (lpips.cpp) ----
// ---- the pass (engine.cpp) and the device search around it (search.cpp) ----
// latents: host rows, uploaded — or nullptr with d_latents: device rows, copied on the stream.  host_F: the rows are copied back and the
// call waits — or nullptr with d_F_dst: they are copied to that device buffer; no_wait then leaves the stream running (finish_search_pass
// waits once, behind whatever the caller launched after the pass)
#pragma GCC visibility push(hidden)
int run_pass(glass_engine* e, const float* latents, int P, int generation, int first_mb, const glass_noise* noise, float* host_F, float* images,
             const float* d_latents = nullptr, float* d_F_dst = nullptr, bool no_wait = false);
int wait_pass(glass_engine* e, int P);        // the wait no_wait left out: synchronise, the launchers' verdict, the profile
int alloc_search(glass_engine* e);            // the search's buffers (nothing without glass_engine_set_search)
int search_ready(glass_engine* e, const char* what, bool need_init);      // the checks in front of every search_* entry point; selects e->cur
int search_wait(glass_engine* e);             // the wait behind launches made outside a pass
// sep-CMA-ES (cmaes.cpp), reached through the search_* entry points of search.cpp when the engine's search is one
int cma_set_search(glass_engine* e, int pop, double xl, double xu, uint64_t seed);
int alloc_cma(glass_engine* e);
int cma_vary(glass_engine* e, int generation);
int cma_survive(glass_engine* e, int generation);
int cma_step(glass_engine* e, int generation);
#pragma GCC visibility pop

// ---- image editing (edit.cpp) ----
#pragma GCC visibility push(hidden)
int compute_anchor(glass_engine* e);          // edit.anchor_row -> edit.d_anchor through the pass's latent path (set_anchor, and set_truncation after it)
// the source rows of this pass (a direction source is set): encodes the image under the pass's boxes where the stored rows are not those; on e->cur
int refresh_direction_source(glass_engine* e);
void run_anchor(glass_engine* e, int P);      // edit.d_dist of the P candidates whose dlatents run_styles left, on e->cur
#pragma GCC visibility pop

int finalize_lpips(glass_engine* e);          // weights -> device layouts + buffers (nothing with lpips_size 0)
// d[c0 + i] for the B candidates whose raw images are at y [B][3][R][R], on e->cur: box mean + VGG16 + head against the stored target
void run_lpips_chunk(glass_engine* e, const float* y, int c0, int B);

// ---- GPT-2 (gpt2_host.cpp) ----
int finalize_gpt2(glass_engine* e);
void gpt2_work_free(glass_engine* e);     // frees e->gwork (buffers + captured step graph) and resets it

// weight packing (engine.cpp), shared with the diagnostic op ABI (ops.hip)
int glass_fold_upconv(const float* W, int cout, int cin, std::vector<_Float16>& out);  // [9][4*cout][cin]
void glass_pack_conv(const float* W, int cout, int cin, int ks, int cin_pad, std::vector<_Float16>& out);  // [ks*ks][cout][cin_pad]
