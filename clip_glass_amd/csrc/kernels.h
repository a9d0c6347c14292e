// kernels.h — host-callable choosers and launch wrappers (one per kernel family).
#pragma once
#include "common.h"

#include <string>
#include <vector>

// --- ConvParams kernel families ------------------------------------------------------------------------------------------------
// One chooser per family: it reads the launch's features (common.h conv_features) and geometry, launches nothing, and returns the kernel
// instance that takes the layer — its profile name and its launch function — or an empty ConvKernel.  What it returns is what runs:
// `k.launch(p, stream)`.  The order in which the engine asks the families is choose_conv (engine.cpp).
ConvKernel choose_conv_direct(const ConvParams& p);    // conv_direct.hip: operands straight from global memory, any shape; the last resort
ConvKernel choose_conv_tiled(const ConvParams& p);     // conv_tiled.hip: the LDS-tiled kernel (W % 32 == 0)
ConvKernel choose_conv_stream(const ConvParams& p);    // conv_stream.hip: persistent streaming 3x3 conv for the 32 -> 32 channel 1024^2 layers
ConvKernel choose_conv_glds(const ConvParams& p);      // conv_glds.hip: LDS-DMA staged 3x3 conv for the MFMA-bound mid-resolution layers (Cin >= 128)
// conv_wreg.hip: 3x3 stride-1 conv 64 -> 64 channels with the WHOLE weight tensor in registers, one wave per SIMD, the patches on a three-tile
// LDS-DMA ring; reads pixel-major or chunk-planar input
ConvKernel choose_conv_wreg(const ConvParams& p);
// conv_s2.hip: the D blocks' stride-2 3x3 conv + fused 1x1 skip branch on an LDS-DMA ring; any_fill: also where the launch does not fill the chip
ConvKernel choose_conv_s2(const ConvParams& p, bool any_fill = false);
ConvKernel choose_conv_upfir(const ConvParams& p);     // upfir.hip: fused transposed-conv + FIR + epilogue
// conv_gemm.hip: the low-resolution layers as im2col + gemm_tiled + finishing pass — several launches and scratch, so admission and launch are
// separate: ws_a / ws_c: scratch of cap_a halfs / cap_c floats PER CANDIDATE; outside: the feature bits the family lacks
bool conv_gemm_admits(const ConvParams& p, long long cap_a, long long cap_c, uint32_t* outside = nullptr);
const char* launch_conv_gemm(const ConvParams& p, half_t* ws_a, long long cap_a, float* ws_c, long long cap_c, hipStream_t st);   // nullptr: refused
// GemmParams launchers return the kernel symbol they launched (for the per-kernel profile); tiled: nullptr when the shape is not supported
const char* launch_gemm_direct(const GemmParams& p, hipStream_t st);
const char* launch_gemm_tiled(const GemmParams& p, hipStream_t st);
// second half of the full-resolution discriminator block in one kernel (conv_down.hip):
//   y = (lrelu(conv3x3 stride 2 (fir_pad2(h)) + b1) * sqrt2 + conv1x1(xs)) / sqrt2, xs = fir_pad1(x)[::2] (32 -> 64 channels);
// nullptr when the shape does not qualify (caller runs the separate passes)
const char* launch_conv_down(const half_t* h, const half_t* xs, const half_t* w1, const half_t* ws, const float* b1, half_t* y,
                             int B, int R, int Cin, int Cout, hipStream_t st);
bool conv_down_supported(int R, int Cin, int Cout);
// the same op at 64 -> 128 channels (conv_down64.hip: weights in registers, rolling column walk); reached through the two above
const char* launch_conv_down64(const half_t* h, const half_t* xs, const half_t* w1, const half_t* ws, const float* b1, half_t* y,
                               int B, int R, int Cin, int Cout, hipStream_t st);
bool conv_down64_supported(int R, int Cin, int Cout);
// the WHOLE full-resolution discriminator block in one kernel (conv_d0.hip): skip image -> fromRGB -> conv3x3 32 -> 32 -> FIR (pad 2) ->
// conv3x3 stride 2 32 -> 64, + the 1x1 skip branch of FIR (pad 1)[::2] of the fromRGB map, merged; x and h never leave the CU.
// nullptr when the block does not qualify (caller: conv_stream<fromrgb> + conv_down)
const char* launch_dblock0(const float* rgb_y, const float* rgb_w, const float* rgb_b, const half_t* w0, const float* b0, const half_t* w1,
                           const half_t* ws, const float* b1, half_t* y, int B, int R, int Cin, int Cout, hipStream_t st, int y_planar8 = 0);
bool dblock0_supported(int R, int Cin, int Cout);

// --- small fp32 ops (mapping network, style affines, demodulation, heads) ---------
void launch_pixelnorm(const float* z, float* out, int P, int L, float eps, hipStream_t st);
// out[p][n] = epi( sum_k f(x[p][k]) * wt[k][n] + bias[n] ); in_sq: f = square;
// mode 0 none, 1 lrelu*sqrt2, 2 rsqrt(v + eps_row[p*eps_stride])
void launch_dense01_finish(const float* part, int S, long long slab, const float* bias0, const float* w1, const float* b1, float* out, int P, int N,
                           hipStream_t st);
void launch_dense_splitk(const float* x, int ldx, int P, int K, const float* wt, int N, const float* bias, float* out, int ldo,
                         int mode, hipStream_t st);   // K % 64 == 0, K <= 768: the mapping-network layers
void launch_dense(const float* x, int ldx, int P, int K, const float* wt, int N, const float* bias,
                  float* out, int ldo, int in_sq, int mode, const float* eps_row, int eps_stride,
                  hipStream_t st);
// pixel norm + every mapping layer in one launch (L = 256 / 512, <= 8 layers); false: not applicable, run the per-layer path
bool launch_mapping_fused(const float* z, float* out, int P, int L, float eps, const float* const* wt, const float* const* b, int n_layers,
                          hipStream_t st);
// The mapping network's launches (stylegan2/models.py:590-627), z [P][L] -> w0 [P][L]; w1: the per-layer path's second [P][L] buffer.
// path 0: mapping_fused_kernel where it applies, else per layer (pixel norm, then dense_splitk_kernel for L % 64 == 0, L <= 768, dense_kernel
// otherwise); 1: per layer; 2: fused or nothing.  Returns the MAP_* bits of what was launched (0: path 2 where the fused kernel refuses).
enum { MAP_FUSED = 1, MAP_PIXELNORM = 2, MAP_SPLITK = 4, MAP_DENSE = 8 };
int launch_mapping(const float* z, float* w0, float* w1, int P, int L, float eps, const float* const* wt, const float* const* b, int n_layers,
                   int path, hipStream_t st);
struct DenseDesc {
    const float* x; int ldx; int K; const float* wt; int N; const float* bias; float* out; int ldo;
    const float* eps_row; int eps_stride;
};
void launch_dense_multi(const DenseDesc* d_desc, int n_desc, int max_N, int P, int in_sq, int mode, hipStream_t st);
// --- dlatents (dlatent.hip): truncation trick, W / W+ latent spaces ------------------
// dst[P][n_layers][L] = lerp(avg, src, psi[l]) with torch.lerp's rule; the row of (p, l) is read at src + p * src_row + l * src_layer
// (src_layer 0: one row per candidate), in place allowed.  tab = psi[n_pad] | avg[L], n_pad = n_layers rounded up to 4.  L % 4 == 0.
void launch_dlatent_expand(const float* src, long long src_row, long long src_layer, float* dst, const float* tab, int n_pad, int n_layers,
                           int P, int L, hipStream_t st);
// latent space `sub`: dst[P][n_lat][L] = base[l] + c[p][layer_group[l]] . B (one fp32 FMA chain over k, then one add); a layer of group -1
// gets base[l].  c [P][G][K], B [K][L], base [n_lat][L].  false: outside the limits (K <= min(L, 512), L % 4 == 0, 1 <= G <= n_lat).
bool launch_dlatent_subspace(const float* c, int P, int G, int K, const int* layer_group, int n_lat, int L, const float* B, const float* base,
                             float* dst, hipStream_t st);
// one 64-wide piece of a style segment: columns [col0, col0 + n) of the [P][S_total] style table read dlatent row `lat`
struct StyleTile { int col0, n, lat, pad; };
// out[p][col] = sum_k dlat[p][lat(col)][k] * wt[k][col] + bias[col] over the tile list: dense_kernel's bits per element
void launch_styles_layered(const float* dlat, int n_lat, int L, int P, const float* wt, int S_total, const float* bias, float* out,
                           const StyleTile* d_tiles, int n_tiles, hipStream_t st);
// per (p, layer): smax = max|s|, s /= smax, eps_row = eps / smax^2
void launch_style_norm(float* s, int ld, int P, int n_layers, const int* d_off, const int* d_len,
                       float* smax, float* eps_row, float eps, hipStream_t st);
// per-sample modulated+demodulated weights: wm[b][e] = w[e] * sn[b][e % Cin] * dscale[b][(e / Cin) % Cout]
void launch_modulate_weights(const half_t* w, long long elems, int Cin, int Cout, const float* sn, int sn_stride,
                              const float* dscale, int ds_stride, int P, half_t* wm, hipStream_t st);
// plane m of the launch is that of minibatch mb0 + m, or with a period > 0 of minibatch (mb0 + m) % period (the device search's islands)
void launch_noise(float* out, int n_mb, int hw, uint32_t layer, uint32_t mb0, uint32_t generation,
                  uint64_t seed, hipStream_t st, uint32_t period = 0);

// --- image-space ops ---------------------------------------------------------------
// y[b][c][p] = bias[c] + smax[b]*sum_i wrgb[c][i]*sn[b][i]*x[b][p][i] + upfir(yprev)
void launch_trgb_tables(const float* wrgb, const float* sn, int sn_stride, const float* smax, int smax_stride, int B, int NT,
                        half_t* tab, hipStream_t st);   // [B][2][16][NT] fp16: A operand of the toRGB fused into a conv epilogue
// skip image from the per-n-tile toRGB partial sums of a conv epilogue (ConvParams::trgb_part [ntn][B][3][R][R])
void launch_trgb_finish(const float* part, int ntn, int B, int R, const float* bias, const float* yprev, float* yout, hipStream_t st);
// false: channel width not instantiated (16 ... 512 in powers of two) — nothing launched
bool launch_torgb(const half_t* x, int B, int H, int W, int C, const float* wrgb, const float* bias,
                  const float* sn, int sn_stride, const float* smax, int smax_stride,
                  const float* yprev, float* yout, hipStream_t st);
// img = clip((y+1)/2, 0, 1)
void launch_finalize_image(const float* y, float* img, long long n, hipStream_t st);
// bilinear (align_corners=False) resize of clip((y+1)/2,0,1) into the patch matrix [B*G*G][3*ps*ps] fp16
void launch_resize_patches(const float* y, int B, int R, int clip_res, int ps, int ld, half_t* patches,
                           hipStream_t st);
// CLIP's own preprocessing (glass_config::clip_resize / clip_normalize): antialiased bilinear (1) / bicubic (2, then clamp to [0, 1]) resize
// through a host-built tap table, and / or Normalize(mean, std) of clip/clip.py:73 before the fp16 store.  Same output layout as
// launch_resize_patches, which stays the kernel of the default (0, 0).
#define GLASS_RESIZE_MAX_TAPS 32   // taps per output pixel and axis (1024 -> 224 bicubic: 19)
#define PREPROCESS_TY 8            // output rows per workgroup
#define PREPROCESS_RB 8            // input rows per load batch
#define PREPROCESS_MAX_R 1024      // one thread per four input columns
struct ResizeTaps {                // one axis, host side
    std::vector<int> start, count; // [S]
    std::vector<float> taps;       // [S][GLASS_RESIZE_MAX_TAPS], zero past count
    std::vector<float> table;      // what the kernel keeps in LDS: taps [S][ts], start [S], count [S]
    int max_count = 0, nr = 0, ts = 0;   // nr: input rows of the tallest band, in whole pairs of load batches
    size_t lds_bytes = 0;
};
struct ResizeTapsDev {
    const float* table = nullptr;  // ResizeTaps::table on the device
    int n4 = 0, ts = 0;            // its length in 16-byte vectors; the taps' row stride
    size_t lds_bytes = 0;
};
// false: (R, S, mode) is outside what preprocess_patches_kernel takes; `why` says which limit
bool build_resize_taps(int R, int S, int mode, ResizeTaps& t, std::string& why);
// resize_mode 0 (with normalize 1): resize_patches_norm_kernel, `t` unused; 1 / 2: preprocess_patches_kernel
void launch_preprocess_patches(const float* y, int B, int R, int clip_res, int ps, int ld, int resize_mode, int normalize,
                               const ResizeTapsDev& t, half_t* patches, hipStream_t st);
// Crop views (glass_engine_set_clip_views): image b seen through box v = (x0, y0, s, flip) of its R x R pixels — launch_resize_patches'
// point-sampled bilinear resize of the s x s crop to clip_res, columns reversed where flip is set — into patch rows (b V + v) G G ...; the
// box (0, 0, R, 0) gives launch_resize_patches' values bit for bit.  normalize: Normalize(mean, std) before the fp16 store.  The boxes travel
// in the kernel arguments; every box must lie inside the image (view_boxes_valid).
#define GLASS_MAX_CLIP_VIEWS 16
struct ViewBoxes {
    int box[GLASS_MAX_CLIP_VIEWS][4];
};
bool view_boxes_valid(const ViewBoxes& vb, int V, int R);
void launch_view_patches(const float* y, int B, int R, int clip_res, int ps, int ld, int normalize, int V, const ViewBoxes& vb, half_t* patches,
                         hipStream_t st);
void launch_fromrgb(const float* y, int B, int R, int Cout, const float* w, const float* bias,
                    half_t* out, hipStream_t st);
// 4x4 FIR [1,3,3,1]^2/64, zero pad 2, stride 1: [B,H,W,C] -> [B,H+1,W+1,C]
void launch_blur_pad2(const half_t* x, int B, int H, int W, int C, half_t* out, hipStream_t st, int planar32 = 0);   // planar32: [C/32][H+1][W+1][32] for conv_s2
bool blur_pad2_planar32_ok(int C);      // the channel counts that form exists for
// 4x4 FIR, zero pad 1, then ::2 subsample: [B,H,W,C] -> [B,H/2,W/2,C]
void launch_blur_down(const half_t* x, int B, int H, int W, int C, half_t* out, hipStream_t st);
// minibatch-std (reference quirk: features are group-mean subtracted): [B,hw,C] -> [B,hw,Cpad]
void launch_mbstd(const half_t* x, int B, int hw, int C, int Cpad, int batch_size, int group, float eps,
                  half_t* out, hipStream_t st);

// --- CLIP --------------------------------------------------------------------------
void launch_embed_lnpre(const float* patch_emb, const float* cls, const float* pos, const float* g,
                        const float* b, int P, int T, int D, float* x, hipStream_t st);
// x[n*ctx + t][:] = tok_emb[tokens[n*ctx+t]][:] + pos[t][:]
void launch_embed_text(const int* tokens, const float* tok_emb, const float* pos, int n_rows, int ctx, int D, float* x,
                       hipStream_t st);
void launch_layernorm(const float* x, long long row_stride, int M, int D, const float* g, const float* b,
                      half_t* out16, float* out32, const LaunchTo& to);
void launch_layernorm_rows(const float* x, const int* rows, int M, int D, const float* g, const float* b, float* out32, hipStream_t st);
void launch_attention(const half_t* qkv, int n_img, int L, int heads, int hd, int causal, half_t* out,
                      hipStream_t st);
// --- the score tail (score.hip): one cosine kernel, one assemble_F kernel ---
#define GLASS_PROMPT_MAX 16         // entries of a set
#define GLASS_PROMPT_MAX_VIEWS 16   // glass_clip_views_supported's limit
// the device search's islands with own prompts: row p combines its entries with row (row0 + p) / pop of weights [islands][T] and that
// island's W [islands] instead of the set's; weights nullptr: none
struct CosineIslands {
    const float* weights = nullptr;
    const float* W = nullptr;
    int pop = 0, row0 = 0;
};
// feat [P][V][D] (V = 1: no views), targets [T][D], weights [T], W = prompt_weight_sum -> view_sim [P][V] (nullable: entry 0's per-view cosines),
// set_sim [P][T] (the ordered means over the views), sim [P] (the combination of mode `sum`).  A single target is T = 1, weight 1, W = 1:
// sim = set_sim = the cosine.  src [V][D] (nullable; unit rows, launch_unit_rows): the directional form — every (row, view, entry) value is the
// cosine between f / max(|f|, 1e-8) - src[v] and the entry, every product and sum rounded on its own.  streamed: the form that reads the set
// from memory at any shape (the launcher chooses it above 64 KB): the same bits
struct CosineSet {
    const float *feat = nullptr, *targets = nullptr, *weights = nullptr;
    float W = 0.f;
    int P = 0, V = 1, T = 0, D = 0;
    const float* src = nullptr;
    float *view_sim = nullptr, *set_sim = nullptr, *sim = nullptr;
    CosineIslands isl;
    bool streamed = false;
};
// One launch; false: a shape outside the limits (V, T in [1, 16], D <= 2^20) or a broken island table, nothing launched
bool launch_cosine_set(const CosineSet& a, hipStream_t st);
float prompt_weight_sum(const float* weights, int T);      // sum |w_t| in fp32, t = 0 .. T - 1 (host)
// F [P][n_obj].  The similarity columns: -sim (lp_lambda > 0: fmaf(lp_lambda, lp, -sim); anchor_lambda > 0: then fmaf(anchor_lambda, anchor, F0))
// — or, with set_sim [P][K] and weights [K], the pareto layout: F[p][t] = w_t < 0 ? set_sim[p][t] : -set_sim[p][t].  Then relu(1 - dis), lp as
// its own column (lp_lambda == 0), anchor as its own LAST column (anchor_lambda == 0); dis / lp / anchor nullable
struct AssembleF {
    const float* sim = nullptr;
    const float *set_sim = nullptr, *weights = nullptr;
    int K = 0;
    const float *dis = nullptr, *lp = nullptr;
    float lp_lambda = 0.f;
    const float* anchor = nullptr;
    float anchor_lambda = 0.f;
    int P = 0, n_obj = 0;
    float* F = nullptr;
};
// false: the columns do not add up to n_obj, or a fold with the pareto layout: nothing launched
bool launch_assemble_F(const AssembleF& a, hipStream_t st);
// --- image editing (edit.hip; include/glass.h "Image editing") ---
#define GLASS_ANCHOR_MAX_LAYERS 64  // style layers of a latent anchor (2 * GLASS_MAX_BLOCKS = 24 at most in an engine)
// out[r] = feat[r] / max(|feat[r]|, 1e-8), n rows of D: the source rows, by the arithmetic the directional cosine applies to a feature row
bool launch_unit_rows(const float* feat, int n, int D, float* out, hipStream_t st);
// d[p] = mean over (l, i) of (w[p * cand_stride + l * layer_stride + i] - a[l * L + i])^2; layer_stride 0: one row for every layer.
// false: n_lat outside [1, GLASS_ANCHOR_MAX_LAYERS], L outside [1, 65536], a layer stride inside (0, L): nothing launched
bool launch_latent_anchor(const float* w, long long cand_stride, int layer_stride, const float* a, int n_lat, int L, int P, float* d, hipStream_t st);

// --- device search (search.hip; include/glass.h "Device search") ---
#define GLASS_SEARCH_MAX_POP 1024      // population rows (2048 merged rows in survival)
#define GLASS_SEARCH_MAX_OBJ 6
#define GLASS_SEARCH_TAG 0x53524348u   // XOR-ed into the Philox key's high word: the search's own stream
#define GLASS_SEARCH_DRAW_TOURNAMENT 0u   // purpose words (the counter's fourth): index = mating, variable = 0
#define GLASS_SEARCH_DRAW_SBX 1u          // index = mating
#define GLASS_SEARCH_DRAW_MUTATION 2u     // index = offspring row
#define GLASS_SEARCH_DRAW_BIT_GATE 3u     // mixed rows: index = mating, variable = 0; the mating exchanges bits iff u0 < prob_x
#define GLASS_SEARCH_DRAW_BIT_KEY 4u      // index = mating, variable = the bit's column; the raw word w0 is the column's key
#define GLASS_SEARCH_DRAW_BIT_FLIP 5u     // index = offspring row, variable = the bit's column; the bit flips iff u0 < prob_flip
#define GLASS_SEARCH_MAX_BITS 4096        // bit columns of a mixed row (the bit kernel's LDS holds one key per column)
struct GaParams {
    int pop;
    double xl, xu, eta_c, eta_m, prob_m;
    uint64_t seed;
    double prob_x, prob_flip;      // mixed rows only: HUX per mating, bit-flip per bit
};
// Every launcher returns the name of the kernel it launched, or nullptr: a shape outside the limits, nothing launched.  Every buffer holds
// `islands` populations back to back, island i runs under seed + i with local indices, and the island is the kernels' last grid dimension
// (include/glass.h "Device search: islands"); a single search is islands = 1.  More than one island: the island search's limits, with as
// many offspring as population rows per island and pop_out = n_pop.
#define GLASS_SEARCH_MAX_ISLANDS 64
// offspring rows [row0, row0 + rows) of every island, generation `generation`, from the populations X [islands g.pop][n_real + n_bits] with
// rank, cd [islands g.pop] -> Xoff rows.  A mixed row is [n_real real | n_bits bit columns] (include/glass.h "Mixed rows"): `parts` chooses
// the real columns' kernel, the bit columns' kernel or both (the engine launches them one by one, under a profile row each); an all-real
// row is n_bits 0 with GA_VARY_REAL.  nullptr also: n_real < 1, n_bits above GLASS_SEARCH_MAX_BITS, GA_VARY_BITS with n_bits < 1, rows
// outside the g.pop offspring rows
enum { GA_VARY_REAL = 1, GA_VARY_BITS = 2, GA_VARY_BOTH = 3 };
const char* launch_ga_vary(const float* X, const int* rank, const double* cd, const GaParams& g, int islands, int n_real, int n_bits, int generation,
                           int row0, int rows, int parts, float* Xoff, hipStream_t st);
// flags[r] = 1: Xoff row r equals, by value in every variable, a row of its island's X [pop] or an Xoff row of its island below r
const char* launch_ga_duplicates(const float* X, const float* Xoff, int islands, int pop, int n_off, int n_var, int* flags, hipStream_t st);
// survival, one workgroup per island, of its n_pop rows of F [islands n_pop][n_obj] with its n_off rows of Foff (a second plane, or F +
// n_pop n_obj behind a single population; flags [islands n_off] nullable): chosen / rank_out / cd_out [islands pop_out], the island's first
// pop_out rows of F rewritten as the survivors', counts [islands][3] = {flagged, non-finite rows, migrants accepted (ga_migrate_kernel's)}.
// nsga 0: GA.  gated (n_off 0 and pop_out = n_pop only): islands whose third counter is 0 keep their state, chosen = identity
const char* launch_ga_survive(float* F, const float* Foff, const int* flags, int islands, int n_pop, int n_off, int n_obj, int pop_out, int nsga, int gated,
                              int* chosen, int* rank_out, double* cd_out, int* counts, hipStream_t st);
void launch_ga_gather(const float* X, const float* Xoff, const int* chosen, int islands, int n_pop, int pop_out, int n_var, float* Xnext, hipStream_t st);
size_t ga_survive_lds_bytes(int n_rows, int n_obj);
// ring migration of the `migrants` best rows of island i - 1 onto the worst rows of island i, X and F in place; writes counts[i][2]
const char* launch_ga_migrate(float* X, float* F, const int* rank, const double* cd, int islands, int pop, int n_var, int n_obj, int migrants, int* counts,
                              hipStream_t st);

// --- device search: sep-CMA-ES (cmaes.hip; include/glass.h "Device search: sep-CMA-ES") ---
#define GLASS_SEARCH_DRAW_NORMAL 6u       // index = sampled row, variable = column; z = sqrt(-2 ln u0) cos(2 pi u1)
#define GLASS_CMA_MIN_POP 4
#define GLASS_CMA_BLOCK 256               // variables per workgroup of the update: the partition of ||p_sigma||^2, a function of n alone
struct CmaParams {      // what a launch takes by value: sizes, bounds, seed and the constants of the header's "Setup" (cma_params)
    int lambda, mu, n;
    double xl, xu;
    uint64_t seed;
    double mu_eff, c_sigma, d_sigma, c_c, c_1, c_mu, chi;
};
struct CmaScalars {     // device; every field has one writer: thread 0 of the rank kernel or thread 0 of block 0 of the second update phase
    double sigma, ps_norm;
    float best_F;
    int best_src;       // the row of this generation that became the best seen, -1: none (the best-row copy then leaves best_X alone)
    int h, finite, updated, skipped, updates;      // updated: this generation had >= mu finite rows; skipped / updates count generations
};
struct CmaState {       // device pointers
    double *m, *d, *ps, *pc;      // [n] each
    double* w;                    // [mu] recombination weights
    double *yw, *s2;              // [n]: y_w and sum w y^2 of the generation, from the first update phase to the second
    double* part;                 // [ceil(n / GLASS_CMA_BLOCK)] partial sums of p_sigma^2
    CmaScalars* sc;
    int* order;                   // [lambda] rows by (F, index)
    float* best_X;                // [n]
    int* counts;                  // nullable int [2] = {0, non-finite rows of the last rank} (glass_engine_search_read's counts)
};
CmaParams cma_params(int lambda, int n, double xl, double xu, uint64_t seed);      // host; the header's constants, in double
void cma_weights(int lambda, double* w /*[lambda / 2]*/);                           // host; normalised, in double
inline int cma_blocks(int n) { return (n + GLASS_CMA_BLOCK - 1) / GLASS_CMA_BLOCK; }
// Every launcher returns the name of the kernel it launched, or nullptr: a shape outside the limits, nothing launched.
// rows [row0, row0 + rows) of generation `generation` from (m, d, sigma) -> X [lambda][n]
const char* launch_cma_sample(const CmaState& s, const CmaParams& p, int generation, int row0, int rows, float* X, hipStream_t st);
// F [lambda] -> order, the finite count, the counters and the best-so-far decision.  One workgroup
const char* launch_cma_rank(const CmaState& s, const CmaParams& p, const float* F, hipStream_t st);
// the two update phases (a kernel boundary stands for the grid-wide dependency on ||p_sigma||) and the best-row copy, from the rank just made
const char* launch_cma_update(const CmaState& s, const CmaParams& p, const float* X, int generation, hipStream_t st);

// --- perceptual objective: LPIPS on VGG16 (lpips.hip); the 3 x 3 convolutions behind the first are gemm_tiled (mode 5, A = 1, S = bias) ---
#define GLASS_LPIPS_PIXB 256      // pixels of one image a workgroup of the head owns
// box mean R -> S (R % S == 0, box <= 8) of planar fp32 y [B][3][R][R], then (v - shift_c) / scale_c -> [B][S][S][4] fp16 (channel 3 = 0)
bool launch_lpips_input(const float* y, int B, int R, int S, half_t* out, hipStream_t st);
// features.0 (3 x 3 pad 1, 3 -> 64, + bias + ReLU): x [B][S][S][4], w [27][64] fp16 with row (ci, ky, kx) -> y [B][S][S][64]
bool launch_vgg_conv1(const half_t* x, const half_t* w, const float* bias, int B, int S, half_t* y, hipStream_t st);
bool launch_maxpool2(const half_t* x, int B, int H, int W, int C, half_t* y, hipStream_t st);      // MaxPool2d(2), NHWC; false: odd side or C % 8
// one slice's term of n images: x0 [n][HW][C] against x1 + i x1_bs (x1_bs 0: one map for all), lin [C]; part: n ceil(HW / GLASS_LPIPS_PIXB)
// floats of scratch; d[i] = term (first) or d[i] += term.  false: C is not one of 64 / 128 / 256 / 512
bool launch_lpips_head(const half_t* x0, const half_t* x1, long long x1_bs, const float* lin, int n, int HW, int C, float* part, int first, float* d,
                       hipStream_t st);

// --- CLIP's ResNet towers (clip_resnet.hip); BatchNorm = fp32 per-channel scale bn_a and shift bn_s in the epilogue ---------------------
// stem conv1 (3 x 3 stride 2 pad 1, 3 -> C1, + BN + ReLU) from the 32-pixel patch operand of an S x S image -> [B][S/2][S/2][C1]; w [27][C1] fp16,
// row (ci, ky, kx).  false: refused (S % 32, C1 % 8)
bool launch_rn_stem_conv1(const half_t* img, const half_t* w, const float* bn_a, const float* bn_s, int B, int S, int C1, half_t* y, hipStream_t st);
// 3 x 3 stride 1 pad 1 + BN + ReLU for Cin % 16 == 0, Cout % 32 == 0 (the stem's conv2 / conv3); w [9][Cout][Cin].  nullptr: refused
const char* launch_rn_conv3x3(const half_t* x, const half_t* w, const float* bn_a, const float* bn_s, int B, int H, int W, int Cin, int Cout, half_t* y,
                              hipStream_t st);
bool launch_rn_avgpool2(const half_t* x, int B, int H, int W, int C, half_t* y, hipStream_t st);      // AvgPool2d(2), NHWC; false: odd side or C % 8
// tok [B][HW + 1][C] = [mean over HW ; the HW pixels] + pos [HW + 1][C]
void launch_rn_attnpool_tokens(const half_t* x, const float* pos, int B, int HW, int C, half_t* tok, hipStream_t st);
void launch_rn_token0_rows(const half_t* att, int B, int T, int C, float* out, hipStream_t st);      // out [B][C] fp32 = att[b T][:]

// --- BigGAN-deep glue (biggan_kernels.hip) ---------------------------------------------------------
void launch_bg_cond(const float* x, int P, int L, int zd, int nc, const float* et, float* cond, hipStream_t st);
void launch_bg_bn_tables(float* tab, int P, int C, const float* inv_std, const float* mean, const float* prebias,
                         hipStream_t st);
// any n: whole 4-element vectors, then the n % 4 tail elements one by one (x and y 16 / 8 byte aligned)
void launch_bg_to_half(const float* x, half_t* y, long long n, hipStream_t st);
// returns the kernel it launched: the vector form where c8 % 8 == 0, c2 % 64 == 0, (H W / 4) % 32 == 0, else the scalar form (H, W even)
const char* launch_bg_attn_split(const half_t* T, int B, int H, int W, int c8, int c2, half_t* theta, half_t* phi, half_t* gT,
                                 hipStream_t st);
void launch_bg_softmax(const float* S, long long rows, int n, half_t* Pm, hipStream_t st);
void launch_bg_rgb_tanh(const half_t* x, int B, long long hw, int C, float* y, hipStream_t st);

// --- BigGAN-deep's last stage in one kernel (bg_tail.hip): conv_3 + skip -> bn -> relu -> conv_to_rgb[:3] -> tanh ---------------
struct BgTailParams {
    const half_t* h;        // [B][R][R][32]: relu(bn_3(conv_2)) of the last block (conv_2's epilogue applied them)
    const half_t* x0;       // [B][R/2][R/2][128]: the block's input (skip source, nearest x2)
    const half_t* w3;       // [128][32] conv_3 weights (spectral norm folded)
    const float* b3;        // [128]
    const float* tab;       // this chunk's first row of the batch-norm affine table: scale at [bnf_off + c], shift at [ctot + bnf_off + c]
    int bnf_off, ctot;
    const half_t* rgb_w;    // [9][cpad][128] conv_to_rgb weights (rows 0..2 of each tap used)
    int cpad;
    const float* rgb_b;     // [>= 3]
    float* y;               // [B][3][R][R] fp32
    int B, R;
};
bool bg_tail_supported(int R, int mid, int cout, int cin, int up, int cpad);
bool launch_bg_tail(const BgTailParams& p, hipStream_t st);
// --- GPT-2 (fp32, gpt2.hip) ----------------------------------------------------------
// Every launcher takes a LaunchTo (common.h): a stream, or a text list that receives the launch's name, grid and block instead.
void launch_gpt2_embed(const int* tok, const float* wte, const float* wpe, int rows, int L, int pos0, int D, float* x,
                       const LaunchTo& to);
// part / part_elems: split-K scratch for the single-token (M <= 64) steps (nullptr = never split)
// prefill: the rows are P sequences x nd > 1 positions — always the tiled kernels, so that the kernel (and with it the summation order)
// a sequence's prefill runs on does not depend on how many sequences the launch holds
void launch_gemm_f32(const float* A, const float* W, const float* bias, float* out, int M, int N, int K, int lda, int ldo,
                     int mode, const LaunchTo& to, float* part = nullptr, size_t part_elems = 0, bool prefill = false);
// A single-token-step product (M <= 64 rows), decided before it is launched.  The choosers (choose_gemm_f32_step: the weight-streaming
// form with a global K split S; choose_gemm_f32_rowblk: the complete-output form, a workgroup = 32 rows x 32 columns over the whole K)
// launch nothing and return the instance's template arguments, its profile name and its grid — or an empty value: refused.  The launchers
// launch exactly that and cannot refuse.
struct StepGemm {
    int S = 0, NK = 1;                // global K split (0: refused), K parts inside a workgroup
    bool LN = false, ONE = false;
    int M = 0, N = 0, K = 0, lda = 0, np_in = 0;
    dim3 grid, block;
    const char* name = nullptr;
    explicit operator bool() const { return S > 0; }
};
struct StepGemmOperands {
    const float *A, *W, *bias;
    float* out;
    int ldo, mode;                    // 0 plain, 1 GELU-tanh, 2 out +=
    float* part;                      // streaming form: the slices' raw sums (S > 1)
    const float *stats, *lng, *lnb;   // LayerNorm fused on A: row statistics [M][2] (streaming form) / row partials [M][np_in][2] (row-block form)
    float* pst_out;                   // row-block form, nullable: the epilogue's row partials [M][N / 32][2]
};
bool gemm_f32_step_supported(int M, int K, int lda, bool ln_fused);   // choose_gemm_f32_step's shape conditions
StepGemm choose_gemm_f32_step(int M, int N, int K, int lda, bool ln_fused, size_t part_elems, int n_cu, bool cand_only = false);
void launch_gemm_f32_step(const StepGemmOperands& o, const StepGemm& c, const LaunchTo& to);
bool gemm_f32_rowblk_supported(int M, int N, int K, int lda, bool ln_fused, bool stats_out);
StepGemm choose_gemm_f32_rowblk(int M, int N, int K, int lda, bool ln_fused, int np_in, bool stats_out);
void launch_gemm_f32_rowblk(const StepGemmOperands& o, const StepGemm& c, const LaunchTo& to);
// vocabulary projection of a single-token step (LayerNorm fused, (max, index) pairs per 32-column block) + the pick behind it; a tail
// also writes the next step's embedding / first LayerNorm statistics and advances the state (state[2] = ticket counter, zero)
enum Gpt2Pick { GPT2_PICK_ARGMAX, GPT2_PICK_ARGMAX_TAIL, GPT2_PICK_SAMPLE, GPT2_PICK_SAMPLE_TAIL };
struct Gpt2Head {
    bool ok = false;
    Gpt2Pick pick = GPT2_PICK_ARGMAX;
    int M = 0, N = 0, K = 0, lda = 0, NB = 0;
    dim3 grid, block, pick_grid, pick_block;
    const char *name = nullptr, *pick_name = nullptr;
    explicit operator bool() const { return ok; }
    bool tail() const { return pick == GPT2_PICK_ARGMAX_TAIL || pick == GPT2_PICK_SAMPLE_TAIL; }
    bool sample() const { return pick == GPT2_PICK_SAMPLE || pick == GPT2_PICK_SAMPLE_TAIL; }
};
struct Gpt2HeadOperands {
    const float *A, *W, *stats_in, *lng, *lnb;
    float *logits, *pairs;            // logits: nullable for the arg-max picks
    const int* sp;                    // sampling picks: the sampler's words
    int *gen, *state;
    const float *wte, *wpe;           // tails
    float *x, *stats_out;
};
bool gpt2_head_supported(int M, int N, int K, int lda);
Gpt2Head choose_gpt2_head(int M, int N, int K, int lda, Gpt2Pick pick, bool logits_stored);
void launch_gpt2_head(const Gpt2HeadOperands& o, const Gpt2Head& h, const LaunchTo& to);
void launch_gpt2_reduce(const float* part, int S, const float* bias, float* out, int M, int N, int ldo, int mode, const LaunchTo& to);
void launch_gpt2_finalize(const float* part, int S, const float* bias, float* x, int M, int D, float* stats, const LaunchTo& to);
#define GPT2_ATTENTION_LDS_MAX (160 * 1024)
size_t gpt2_attention_lds_bytes(int nd, int ns);      // dynamic LDS of one launch_gpt2_attention (ns = history + new positions)
// past_dev / step_dev: device-resident step state {past length, step index} for the captured single-token step
void launch_gpt2_attention(const float* qkv, float* kc, float* vc, int P, int nd, int past, int Tmax, int heads,
                           float* out, const LaunchTo& to, const int* past_dev = nullptr);
void launch_gpt2_attention_step(const float* qkv, const float* part, int S, const float* bias, float* kc, float* vc, int P, int Tmax, int heads,
                                float* out, const LaunchTo& to, const int* past_dev);
void launch_argmax(const float* logits, int rows, int N, int* out, const LaunchTo& to, const int* step_dev = nullptr, float* scratch = nullptr);
void launch_gpt2_embed_step(const int* gen, const int* state, int P, const float* wte, const float* wpe, int D, float* x, const LaunchTo& to,
                            float* stats = nullptr, bool partial_fmt = false);
void launch_gpt2_advance(int* state, const LaunchTo& to);
// stochastic pick (top-k temperature sampling, gpt2.hip): the per-call values are int32 words in device memory, sp[GPT2_SP_WORDS]
// (temperature as its float bits; STEP is read only without a device step state — the diagnostic op)
enum { GPT2_SP_SEED_LO, GPT2_SP_SEED_HI, GPT2_SP_GEN, GPT2_SP_ROW0, GPT2_SP_PURPOSE, GPT2_SP_TEMP, GPT2_SP_TOPK, GPT2_SP_STEP, GPT2_SP_WORDS };
#define GPT2_SAMPLE_TOPK_MAX 256
bool gpt2_sample_supported(int V);
// logits [rows][V] -> out[(state ? state[1] : 0) * rows + row]
void launch_gpt2_sample(const float* logits, int rows, int V, const int* sp, int* out, int* state, const LaunchTo& to);
// NCHW fp32 image [n][3][S][S] -> CLIP patch matrix [n*G*G][3*ps*ps] fp16
void launch_image_patches(const float* img, int n, int S, int ps, int ld, half_t* patches, hipStream_t st);
