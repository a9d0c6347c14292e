/* glass.h — C ABI of the MI355X CLIP-GLaSS fitness-evaluation engine (libglass.so).
 *
 * Drop-in boundary: the reference evaluates a population through
 *   GenerationProblem._evaluate(x, out)            /root/reference/problem.py:14-29
 *     -> Generator.generate / clip_similarity / discriminate   generator.py:29-60
 *     -> models.StyleGAN2.generate / discriminate              models.py:108-129
 * in one Python process on one device.  This library replaces everything below
 * `_evaluate` with one engine object per (process, GPU); the Python shim
 * clip_glass_amd/problem.py keeps the pymoo-facing signature and calls these
 * entry points through ctypes (see INTEGRATION.md for the stub a reference
 * maintainer would add).
 *
 * Conventions: plain pointers and sizes, host buffers owned by the caller, no
 * aliasing retained after return.  Every function returns GLASS_OK (0) or a
 * negative status; glass_last_error() gives the thread-local message.  The
 * engine is not thread-safe; evaluate() is blocking.
 */
#ifndef GLASS_H
#define GLASS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLASS_OK 0
#define GLASS_ERR_ARG -1      /* bad argument / shape (reference: assert, models.py:112,124) */
#define GLASS_ERR_STATE -2    /* call order (weights missing: reference sys.exit(1), models.py:93-101) */
#define GLASS_ERR_HIP -3      /* HIP runtime failure */
#define GLASS_ERR_NOMEM -4

#define GLASS_MAX_BLOCKS 12
#define GLASS_MAX_BG_LAYERS 16
#define GLASS_GEN_STYLEGAN2 0
#define GLASS_GEN_BIGGAN_DEEP 1

typedef struct glass_engine glass_engine;

/* Architecture + semantics.  Mirrors the fields the reference reads from its merged
 * argparse/config Namespace (config.py:80-95; stylegan2/models.py kwargs). */
typedef struct glass_config {
    int32_t device;               /* HIP device ordinal (reference: --device, run.py:17) */
    int32_t n_blocks;             /* number of resolutions, 4*2^(n_blocks-1) px output (9 -> 1024);
                                     0 = no GAN (text-only engine for the GPT2 / img2txt config) */
    int32_t channels[GLASS_MAX_BLOCKS]; /* channels per resolution, LOW -> HIGH res
                                     (reference G order reversed: stylegan2/models.py:748-750) */
    int32_t latent_size;          /* 512 */
    int32_t mapping_layers;       /* 8   (stylegan2/models.py:547) */
    int32_t batch_size;           /* config.batch_size: semantic minibatch — one noise plane per G call
                                     (modules.py:428-452) and mbstd groups per D call (modules.py:726) */
    int32_t mbstd_group;          /* 4   (stylegan2/models.py:1047) */
    int32_t use_discriminator;    /* config.use_discriminator */
    int32_t n_obj;                /* problem_args["n_obj"] (problem.py:21) */
    int32_t max_pop;              /* capacity in candidates (rows of x) */
    int32_t chunk;                /* candidates resident per pass at high resolution (multiple of batch_size; 0 = auto) */
    int32_t clip_width, clip_layers, clip_heads, clip_patch, clip_res, clip_embed; /* 768,12,12,32,224,512 (ViT-B/32); see glass_clip_geometry_supported */
    int32_t noise_mode;           /* 0 none, 1 device Philox N(0,1) planes, 2 caller-provided planes */
    uint64_t noise_seed;
    /* --- BigGAN-deep generator (configs DeepMindBigGAN256/512, config.py:31-74; models.py:64-86 calls
     * pytorch-pretrained-biggan's BigGAN.forward(z, class_label, truncation)).  With generator =
     * GLASS_GEN_BIGGAN_DEEP: n_blocks = 0, use_discriminator = 0, latent_size = bg_z_dim + bg_num_classes
     * (one population row = [z | class bits], latent.py:16-18), output = 4 * 2^(#up layers) px. */
    int32_t generator;            /* GLASS_GEN_STYLEGAN2 (0, default) | GLASS_GEN_BIGGAN_DEEP */
    int32_t bg_ch;                /* channel_width (128) */
    int32_t bg_z_dim;             /* config.dim_z (128) */
    int32_t bg_num_classes;       /* config.num_classes (1000) */
    int32_t bg_n_layers;          /* GenBlocks (14 for biggan-deep-512) */
    int32_t bg_layers[GLASS_MAX_BG_LAYERS][3]; /* (up_sample, in_mult, out_mult) per GenBlock */
    int32_t bg_attention_pos;     /* SelfAttn inserted before this GenBlock index (8); -1 = none */
    int32_t bg_n_stats;           /* stored truncation steps of the batch-norm statistics (51) */
    float bg_eps;                 /* batch-norm eps (1e-4) */
    float bg_truncation;          /* config.truncation (1.0): selects / blends the statistics row */
    /* --- opt-in: score through CLIP's own image preprocessing (clip/clip.py:68-74) instead of the reference's point-sampled resize
     * (generator.py:45).  Appended last: zero, or a caller built against the shorter struct of an older library, selects the reference's
     * behaviour.  See glass_clip_preprocess_supported. */
    int32_t clip_resize;          /* 0: bilinear reading 2 x 2 input pixels per output (the reference, default); 1: antialiased bilinear;
                                     2: antialiased bicubic (a = -0.5), then clamp to [0, 1] — both as torch F.interpolate(antialias=True) */
    int32_t clip_normalize;       /* 0: none (the reference, default); 1: (v - mean_c) / std_c with the constants of clip/clip.py:73,
                                     after the resize (and the clamp), before the fp16 store */
    /* --- CLIP's ResNet image towers (clip/model.py:92-149: RN50, RN101).  Appended last: zero selects the ViT engine.  With clip_arch = 1
     * the fields above mean: clip_width = stem width (64), clip_heads = width * 32 / 64 (the attention pool's heads), clip_layers = number
     * of bottlenecks (the sum of clip_rn_layers), clip_patch = 32 (the tower's total stride: (clip_res / clip_patch)^2 + 1 is the attention
     * pool's token count, as it is for a ViT), clip_res and clip_embed as before.  See glass_clip_resnet_supported. */
    int32_t clip_arch;            /* 0: VisualTransformer (default); 1: ModifiedResNet */
    int32_t clip_rn_layers[4];    /* bottlenecks per stage: (3, 4, 6, 3) RN50, (3, 4, 23, 3) RN101 */
    /* --- opt-in: perceptual distance to a target image (LPIPS on VGG16, stylegan2/external_models/lpips.py:34-78, fed as the reference's
     * projector feeds it, stylegan2/project.py:113-122,263).  Appended last: zero selects today's pass.  See glass_lpips_supported and
     * glass_engine_set_lpips_target.  With lpips_size > 0, n_obj must be 1 + use_discriminator + (lpips_lambda == 0). */
    int32_t lpips_size;           /* 0: off (default); S: the generated image is area-downscaled to S x S in front of VGG16 */
    float lpips_lambda;           /* 0: the distance d is its own LAST column, F = [-sim, (hinge), d]; > 0: no column, F[:,0] = fmaf(lambda, d, -sim) */
    /* --- opt-in: one similarity column per prompt (mode pareto of a prompt set, see "Prompt sets" below).  Appended last: zero, or a caller built
     * against the shorter struct, selects the one similarity column of today. */
    int32_t sim_columns;          /* 0 or 1: one similarity column (default); K in [2, 4]: K columns, n_obj = K + use_discriminator + (lpips_size > 0 &&
                                     lpips_lambda == 0); lpips_lambda > 0 is refused then */
    /* --- opt-in: the latent anchor of image editing (see "Image editing" below).  Appended last: zero selects today's pass. */
    int32_t anchor;               /* 0: off (default); 1: d[p], the mean squared distance between candidate p's dlatents and the anchor's (glass_engine_set_anchor) */
    float anchor_lambda;          /* 0: d is its own LAST column of F, after the LPIPS column; > 0: no column, F[:,0] = fmaf(anchor_lambda, d, F0) after the LPIPS fold */
} glass_config;

/* Caller-provided noise (noise_mode 2): planes[m * n_layers + l] points at a host
 * float32 [res_l, res_l] plane for global minibatch m and noise layer l in execution
 * order (== G.static_noise(noise_tensors=...) order, stylegan2/models.py:945-959). */
typedef struct glass_noise {
    int32_t n_minibatches;
    int32_t n_layers;
    const float* const* planes;
} glass_noise;

const char* glass_last_error(void);
const char* glass_version(void);

/* Which CLIP image towers the engine runs (host only: callable without a GPU).  Any ViT whose head dimension
 * (width / heads) is 64 and whose input resolution is a multiple of its patch size: ViT-B/32, ViT-B/16,
 * ViT-L/14, ViT-L/14@336 among them.  Returns GLASS_OK, or GLASS_ERR_ARG with the reason in
 * glass_last_error().  glass_engine_create applies the same rule. */
int glass_clip_geometry_supported(int32_t width, int32_t layers, int32_t heads, int32_t patch, int32_t res,
                                  int32_t embed);

/* Which ModifiedResNet image towers (glass_config::clip_arch = 1) the engine runs (host only: callable without a GPU): stem width a
 * multiple of 64 (every GEMM K and N of the tower is then a multiple of 64 and the attention pool's head dimension is 64: RN50 and RN101;
 * RN50x4 / x16 with widths 80 / 96 are refused), input resolution a multiple of 32.  layers: bottlenecks per stage.  Returns GLASS_OK, or
 * GLASS_ERR_ARG with the reason in glass_last_error().  glass_engine_create applies the same rule. */
int glass_clip_resnet_supported(const int32_t layers[4], int32_t width, int32_t res, int32_t embed);

/* Whether the engine runs the preprocessing (clip_resize, clip_normalize) from a gen_res x gen_res generated image to clip_res (host
 * only: callable without a GPU; gen_res 0 checks the ranges of the two fields alone).  The antialiased modes take an image side that is a
 * multiple of 4 up to 1024 and at most 32 taps per output pixel and axis (a bicubic down-scale up to 7.5 x, a bilinear one up to 15 x).
 * Returns GLASS_OK, or GLASS_ERR_ARG with the reason in glass_last_error().  glass_engine_create applies the same rule. */
int glass_clip_preprocess_supported(int32_t gen_res, int32_t clip_res, int32_t clip_resize, int32_t clip_normalize);

/* Crop views (opt-in; off unless glass_engine_set_clip_views is called): a pass scores candidate p as the mean, over `views` views of its
 * generated image, of the cosine between the view's CLIP feature and the target: sim[p] = (1 / V) sum_v cos(encode_image(view_v(image_p)),
 * target), summed in fp32 in the order v = 0 .. V - 1; F[p][0] = -sim[p].  The discriminator still sees the whole image.  A view is a box
 * (x0, y0, s, flip) in pixels of the R x R image: the point-sampled bilinear resize of the default pass (F.interpolate(..., "bilinear",
 * align_corners=False)) applied to the crop [y0, y0 + s) x [x0, x0 + s), columns reversed where flip = 1.  The boxes are the same for every
 * candidate of a pass — a function of (noise_seed, generation, view) alone, so candidates are ranked through common crops and chunks, slices
 * and shards of a population agree.  View 0 is the whole image (0, 0, R, 0).  For v >= 1, with smin = max(2, (R * min_permille + 999) / 1000)
 * and (w0, w1, w2, w3) = Philox4x32-10 at counter (v, generation, 0, 0) under key (seed_lo, seed_hi ^ 0x56494557): s = smin + w0 % (R - smin
 * + 1), x0 = w1 % (R - s + 1), y0 = w2 % (R - s + 1), flip = flip_enabled ? w3 & 1 : 0; with fixed = 1 the generation word is 0.
 *
 * glass_clip_views_supported: the one rule (host only: callable without a GPU), applied by the setter too.  views in [0, 16] (0: off),
 * min_permille in [1, 1000], clip_resize 0 (the antialiased modes keep one tap table per image side), and max_pop * views * tokens * 4 *
 * width — the tower's largest activation — below 2^31 elements.  tokens, width: a ViT's (res / patch)^2 + 1 and clip_width; for a ResNet
 * tower (res / 4)^2 and the stem width.  Returns GLASS_OK, or GLASS_ERR_ARG with the reason in glass_last_error(). */
int glass_clip_views_supported(int32_t max_pop, int32_t tokens, int32_t width, int32_t clip_resize, int32_t views, int32_t min_permille);
/* The boxes of a pass, int32 [views][4] = (x0, y0, s, flip) (host only; the function the pass itself calls).  views in [1, 16]. */
int glass_host_clip_view_boxes(uint64_t seed, int32_t generation, int32_t views, int32_t gen_res, int32_t min_permille, int32_t flip,
                               int32_t fixed, int32_t* boxes /*[views][4]*/);

/* Perceptual objective (opt-in, glass_config::lpips_size > 0; departs from what the reference's run.py calls — it never wires its LPIPS in):
 * d[p] = LPIPS_VGG16(pixel_min=-1, pixel_max=1).forward(area(y_p), t).  y_p: the raw generator output [3][R][R], nominally in [-1, 1], before
 * biggan_norm and unclamped; area(): the (R / S) x (R / S) box mean; t: the target [3][S][S] in [-1, 1].  forward: (v - shift_c) / scale_c,
 * the five VGG16 slices features[0:4], [4:9], [9:16], [16:23], [23:30], each followed by x rsqrt(sum_c x^2 + 1e-8), the squared difference
 * averaged over H x W and weighted per channel by the slice's lin vector, the five terms summed.  Activations are fp16, sums fp32 in a fixed
 * order: a candidate's d does not depend on its row, the chunk or the shard.
 * Tensors (glass_engine_load_tensor; finalize names a missing one, GLASS_ERR_STATE): "lpips.features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.
 * {weight,bias}" (torchvision's vgg16 keys) and "lpips.lin.{0..4}.weight" [C_k].
 *
 * glass_lpips_supported: the one rule (host only: callable without a GPU), applied by create too.  lpips_size a multiple of 16 in [16, 512]
 * (four max pools need even sides); gen_res % lpips_size == 0 with a box of at most 8; gen_res 0 checks lpips_size alone.  Returns GLASS_OK,
 * or GLASS_ERR_ARG with the reason in glass_last_error().  An engine without a generator (GPT-2) refuses lpips_size > 0. */
int glass_lpips_supported(int32_t gen_res, int32_t lpips_size);

/* Prompt sets (opt-in; off until glass_engine_set_targets is called; departs from the reference's run.py, which has one target): weighted,
 * negative and image prompts.  A set is T entries, 1 <= T <= 16; entry t is a vector g_t (float32 [clip_embed]) and a weight w_t, finite and
 * non-zero; a negative weight means "away from".
 * One feature row f against entry t: c = xy / max(sqrt(xx) * sqrt(yy), 1e-8), the three sums taken as the single-target pass takes them —
 * lane-strided partial sums (i = lane; i < D; i += 64), then the wave sum: the same bits as the single-target cosine of (f, g_t).
 * Crop views on: cbar[p][t] = (sum_v c[p][v][t]) / V, summed in fp32 in the order v = 0 .. V - 1 (the views' own rule, per entry); without
 * views cbar = c.
 * Mode sum (0, default): sim[p] = acc / W; acc starts at 0 and, for t = 0 .. T - 1, acc = acc + w_t * cbar[p][t], the product and the sum each
 * rounded to fp32 (never one fused multiply-add, so numpy float32 reproduces the bits); W = sum_t |w_t| in fp32 in the order t = 0 .. T - 1.
 * F[:,0] is built from sim exactly as with one target (the lpips_lambda > 0 fold included): T = 1 with w = 1 gives the single target's bits.
 * Mode pareto (1): one column per entry, K = T columns with 2 <= K <= 4 on an engine created with sim_columns = K:
 * F[p][t] = w_t < 0 ? cbar[p][t] : -cbar[p][t] (the weight's magnitude has no meaning on a front), then the hinge column with a discriminator,
 * then the LPIPS distance when it is its own column: n_obj = K + use_discriminator + (lpips_size > 0 && lpips_lambda == 0).  lpips_lambda > 0
 * with K >= 2 is refused: there is no single similarity column to fold into.
 * sim[p], as glass_engine_last_details returns it, is the mode-sum value in both modes; glass_engine_last_view_details reports entry 0's
 * per-view cosines.  The pass launches as many kernels with a set as without one.
 *
 * glass_prompt_set_supported: the one rule (host only: callable without a GPU), applied by the setter too.  n_entries in [1, 16]; mode 0 needs
 * sim_columns <= 1; mode 1 needs n_entries == sim_columns (in [2, 4]).  Returns GLASS_OK, or GLASS_ERR_ARG with the reason. */
int glass_prompt_set_supported(int32_t n_entries, int32_t mode, int32_t sim_columns);
/* Make a prompt set the target (after finalize; any time between passes).  feats host float32 [T][E], weights [T].  GLASS_ERR_ARG for
 * E != clip_embed, a weight that is zero or not finite, and whatever glass_prompt_set_supported refuses.  The buffers of a set (16 entries,
 * [max_pop][16] similarities) are allocated by the first call: an engine that never calls it allocates nothing for sets.
 * glass_engine_set_target clears the set; on an engine with sim_columns >= 2 set_target is refused (GLASS_ERR_STATE) and evaluate() fails
 * (GLASS_ERR_STATE, "set_targets() first") while no set is active. */
int glass_engine_set_targets(glass_engine* e, const float* feats /*[T][E]*/, const float* weights /*[T]*/, int32_t T, int32_t E, int32_t mode);
/* cbar [P][T] of the last evaluate() (GLASS_ERR_STATE without an active set). */
int glass_engine_last_set_details(glass_engine* e, int32_t P, float* set_sim /*[P][T]*/);
/* The feature a generated image with these pixels gets in the pass: images host float32 [n][3][R][R] in [-1, 1] (the generator's raw range) go
 * through the pass's own preprocessing (clip_resize / clip_normalize; crop views are ignored: the whole image) and the image tower; out_feat
 * [n][clip_embed].  n <= max_pop; engines with a generator only (GLASS_ERR_STATE otherwise).  This is what makes an image a prompt that is
 * comparable with the candidates: by default they reach CLIP without mean / std normalisation, so a picture encoded through clip.py's
 * transform (glass_engine_encode_image) sits in another input distribution.  Overwrites the per-candidate outputs of the last evaluate(). */
int glass_engine_encode_generated(glass_engine* e, const float* images /*[n][3][R][R] in [-1,1]*/, int32_t n, float* out_feat);

/* Image editing (opt-in; off unless glass_config::anchor is set or glass_engine_set_direction_source is called; departs from the reference's
 * run.py, which has one text and one objective): a directional CLIP objective relative to a source image, and a latent anchor.
 *
 * Directional similarity (StyleGAN-NADA / StyleCLIP's global direction).  While a direction source is set, the entries g_t of the active prompt
 * set are DIRECTIONS (the host builds them: normalise(g_target - g_source_text)), and feature row f of view v scores against entry t as
 *   x = f / max(|f|, 1e-8) - src[v],   c = (x . g_t) / max(|x| |g_t|, 1e-8),
 * src[v] being the unit-length feature of view v of the source image.  A row with x = 0 gives exactly 0.  The mean over views, the weighted sum
 * acc / W of mode sum and the sign rule of the pareto layout are those of "Prompt sets" above: cbar[p][t] = (sum_v c[p][v][t]) / V in the order
 * v = 0 .. V - 1; acc = acc + w_t * cbar[p][t] for t = 0 .. T - 1, the product and the sum each rounded to fp32; W = sum_t |w_t|;
 * F[p][t] = w_t < 0 ? cbar[p][t] : -cbar[p][t] on a front.
 * Summation order: every sum over the D components — f . f, x . x, x . g_t, g_t . g_t — is taken by one wave as lane-strided partial sums
 * (i = lane; i < D; i += 64), then the butterfly over lane offsets 32, 16, .. 1; x_i is f_i / nf - src[v][i] with nf = max(sqrt(f . f), 1e-8), one
 * correctly rounded division and one subtraction; every product and sum is rounded to fp32 on its own (no fused multiply-add), the divisions
 * and square roots are correctly rounded.  A value is a pure function of (row, view, entry): it does not depend on P, on the row's position,
 * on how entries share a sweep, or on whether the set was staged in LDS (up to 64 KB) or streamed — and numpy float32 written in this order
 * reproduces its bits (tests/edit_ref.py).  The source rows are made by the same arithmetic, f_src / max(|f_src|, 1e-8): a candidate whose
 * feature has the source feature's bits scores exactly 0.  Limits as for a prompt set: V <= 16 views, T <= 16 entries.
 * Near x = 0 the cosine is that of a rounding-noise vector and means nothing; a search started at the source (the Python layer's edit_latent)
 * holds row 0 of generation 0 there on purpose, and every other row a step away.
 *
 * glass_engine_set_direction_source: after finalize, any time between passes; NULL turns it off.  image host float32 [3][R][R] in [-1, 1] (the
 * generator's raw range) is kept on the device and encoded through the pass's own preprocessing and image tower (glass_engine_encode_generated's
 * path) into the unit rows src[v].  Crop views off: once, in this call.  Crop views on: the V features are those of the pass's own boxes, made
 * at the start of evaluate() whenever the boxes differ from the ones the stored rows were made with — every generation unless the views are
 * fixed.  With a source set and no active prompt set, evaluate() fails (GLASS_ERR_STATE, "set_targets() first").  An engine without a
 * generator is refused (GLASS_ERR_STATE); a BigGAN engine is allowed: the source is an image.
 * glass_engine_last_direction_source: the rows the last pass subtracted, feats [max(views, 1)][clip_embed].
 *
 * Latent anchor (StyleCLIP's |w - w_src|^2), glass_config::anchor = 1: d[p] = (1 / (n_lat L)) sum_l sum_i (w[p][l][i] - a[l][i])^2 over the
 * dlatents the styles are made from — after mapping and truncation, per the latent space — and the anchor's, a [n_lat][L].  fp32; one wave per
 * candidate sums the flattened index j = l L + i as lane-strided partial sums (j = lane; j < n_lat L; j += 64), difference, product and sum each
 * rounded on its own, then the butterfly over lane offsets 32, 16, .. 1 and ONE division by float(n_lat L); one writer per candidate.
 * F: anchor_lambda == 0: d is one more, LAST, column (after the LPIPS column); > 0: F[:,0] = fmaf(anchor_lambda, d, F0), F0 being column 0 after
 * the LPIPS fold.  n_obj = max(sim_columns, 1) + use_discriminator + (lpips_size > 0 && lpips_lambda == 0) + (anchor && anchor_lambda == 0).
 *
 * glass_edit_supported: the one rule (host only: callable without a GPU), applied by create too.  generator: GLASS_GEN_*; lpips_column: the
 * LPIPS distance is its own column.  anchor 0 needs anchor_lambda 0 and says nothing about n_obj.  anchor 1: a StyleGAN2 engine (a BigGAN
 * engine and an engine without a generator are refused by name); anchor_lambda finite and >= 0; anchor_lambda > 0 with sim_columns >= 2 is
 * refused (no single column to fold into); n_obj as above.  Returns GLASS_OK, or GLASS_ERR_ARG with the reason in glass_last_error().
 * glass_engine_set_anchor: after finalize, on an engine created with anchor = 1 (GLASS_ERR_STATE otherwise).  row [floats_per_row] goes through
 * the pass's own latent path (pixel norm, mapping and truncation, per the current space) with the kernels the pass uses, and the resulting
 * [n_lat][L] stays on the device: a candidate whose row equals the anchor's gets d = 0 exactly.  glass_engine_set_truncation after it
 * recomputes the stored anchor from the row.  evaluate() on an engine created with anchor = 1 fails (GLASS_ERR_STATE, "set_anchor() first")
 * until it is set.
 * glass_engine_last_anchor: the distances d [P] of the last evaluate() (whether they are a column of F or folded into column 0).
 * The device search needs nothing new: the anchor is one more column of F, and search_evaluate scores through the same pass. */
int glass_edit_supported(int32_t generator, int32_t n_blocks, int32_t sim_columns, int32_t use_discriminator, int32_t lpips_column, int32_t anchor,
                         float anchor_lambda, int32_t n_obj);
int glass_engine_set_anchor(glass_engine* e, const float* row /*[floats_per_row]*/);
int glass_engine_last_anchor(glass_engine* e, int32_t P, float* d);
int glass_engine_set_direction_source(glass_engine* e, const float* image /*[3][R][R] in [-1,1], or NULL*/);
int glass_engine_last_direction_source(glass_engine* e, float* feats /*[max(views,1)][clip_embed]*/);

int glass_engine_create(const glass_config* cfg, glass_engine** out);
/* The target image of the perceptual objective: img host float32 [3][S][S] in [-1, 1], S = lpips_size.  After finalize; runs VGG16 on it once
 * and keeps its five activation maps.  evaluate() fails (GLASS_ERR_STATE, "set_lpips_target() first") while none is set. */
int glass_engine_set_lpips_target(glass_engine* e, const float* img, int32_t S);
/* The reference's forward(x0, x1) on caller images, host float32 [n][3][S][S] each, through the kernels of the pass (box 1, no stored target):
 * out [n].  A utility, and the parity entry point. */
int glass_engine_lpips(glass_engine* e, const float* x0, const float* x1, int32_t n, float* out);
/* The distances d [P] of the last evaluate() (whether they are a column of F or folded into column 0). */
int glass_engine_last_lpips(glass_engine* e, int32_t P, float* d);
/* Turn crop views on (views >= 1; 1 = the whole image alone) or off (0) — between create and finalize, which sizes the CLIP-side buffers for
 * max_pop * views images: GLASS_ERR_STATE after finalize, and for an engine without a generator.  seed of the boxes: glass_config::noise_seed. */
int glass_engine_set_clip_views(glass_engine* e, int32_t views, int32_t min_permille, int32_t flip, int32_t fixed);
void glass_engine_destroy(glass_engine* e);

/* Latent spaces and the truncation trick (StyleGAN2 engines; both depart from what the reference's run.py ever calls — it searches z with
 * the raw generator — and are pinned to what its Generator computes, stylegan2/models.py:264-285, 314-324, 393-458).
 * n_lat = 2 * n_blocks style layers (models.py:890-896): the convs take dlatent indices 0, 1, 2 ... in execution order, the toRGB of a
 * block the index of the next block's first conv, the last toRGB the last index.
 *   GLASS_LATENT_Z (default): rows [latent_size].  Pixel norm + mapping network, then truncation, then synthesis.
 *   GLASS_LATENT_W: rows [latent_size] are dlatents: no pixel norm, no mapping; the row goes to every style layer.
 *   GLASS_LATENT_WPLUS: rows [n_lat * latent_size], layer-major: row l goes to the style layers with index l.
 *   GLASS_LATENT_SUB: rows [groups * components] are coefficients of directions of W per group of style layers ("Subspace latent space" below).
 * Truncation: dlatents = lerp(dlatent_avg, dlatents, layer_psi) with torch.lerp's fp32 rule (weight < 0.5: a + w (b - a), otherwise
 * b - (b - a)(1 - w)); layer_psi[l] = psi for l < cutoff (cutoff -1: every layer), 1 elsewhere; a layer with psi 1 keeps its row bit
 * for bit, and psi = 1 or cutoff = 0 is truncation off (models.py:276).  The engine applies layer_psi in EVERY space, whereas the
 * reference truncates explicit dlatents only when the caller calls truncate() itself: in w / w+, psi = 1 (the default) is the
 * reference's forward(dlatents=d), and psi != 1 is forward(dlatents=G.truncate(d)).
 *
 * glass_engine_set_latent_space: between create and finalize (GLASS_ERR_STATE after it, and for a BigGAN or generator-less engine).
 * glass_engine_set_truncation: any time.  psi must be finite and in [0, 1] (the reference takes any float; psi < 0 or > 1 extrapolates
 * away from the average and is refused, GLASS_ERR_ARG); cutoff in [-1, n_lat].  psi != 1 needs the tensor "dlatent_avg" ([latent_size],
 * optional at finalize): after finalize the call fails without it (GLASS_ERR_STATE), and finalize fails the same way when the setter
 * came first.  Rows that differ per layer (space w+, or psi != 1 with 0 < cutoff < n_lat) need a [max_pop][n_lat][latent_size] fp32
 * buffer, which finalize allocates when the space is w+ or set_truncation was called (with any values) before it; a cutoff that
 * needs the buffer on an engine finalized without it is refused (GLASS_ERR_STATE).
 * glass_host_layer_psi: the one rule the setter and the pass use (host only: callable without a GPU); out [n_lat]. */
#define GLASS_LATENT_Z 0
#define GLASS_LATENT_W 1
#define GLASS_LATENT_WPLUS 2
int glass_host_layer_psi(int32_t n_lat, float psi, int32_t cutoff, float* out);
int glass_engine_set_latent_space(glass_engine* e, int32_t space);
int glass_engine_set_truncation(glass_engine* e, float psi, int32_t cutoff);
/* What evaluate / generate read per row: floats_per_row = latent_size (z, w; BigGAN: z_dim + num_classes), n_lat * latent_size (w+) or
 * groups * components (sub; 0 until glass_engine_set_subspace_shape);
 * n_lat = 0 for an engine that is not a StyleGAN2 one.  Nullable each. */
int glass_engine_latent_row(glass_engine* e, int32_t* floats_per_row, int32_t* n_lat);
/* Pixel norm + mapping network, untruncated, with the kernels the pass uses: z host float32 [P][latent_size] -> out_w [P][latent_size].
 * P in [1, max_pop] (no multiple of batch_size needed).  Seeds W / W+ populations. */
int glass_engine_map_latents(glass_engine* e, const float* z, int32_t P, float* out_w);

/* Subspace latent space (opt-in; off unless glass_engine_set_latent_space(GLASS_LATENT_SUB) is called, and then nothing below is allocated
 * or launched; departs from the reference's run.py, which searches z): a fourth StyleGAN2 space whose rows are COEFFICIENTS of a few
 * directions of W (GANSpace: the principal ones), applied to ranges of style layers only (StyleCLIP's coarse / middle / fine edits).
 *
 * The rule.  The style layers 0 .. n_lat - 1 are assigned to G groups by layer_group[n_lat]: a value in [0, G), or -1 for a frozen layer;
 * every group is non-empty and need not be contiguous.  A row is [G][K] float32 coefficients, group-major: floats_per_row = G K.  With a
 * basis B [K][L], a base [n_lat][L] and g = layer_group[l]:
 *   acc[p][g][j]  = fma(c[p][g][K-1], B[K-1][j], ... fma(c[p][g][1], B[1][j], fma(c[p][g][0], B[0][j], 0.f)) ...)
 *                   ONE fp32 FMA chain, k ascending
 *   dlat[p][l][j] = base[l][j] + acc[p][g][j]      (one fp32 add)          for g >= 0
 *   dlat[p][l][j] = base[l][j]                     (a copy, bit for bit)   for g == -1
 * The truncation trick (layer_psi) then runs on dlat exactly as it does on w+ rows, in place, and everything after it is the w+ path: the
 * layered style affines, the latent anchor on the per-layer dlatents.  A candidate's dlatents depend on its own row alone — not on P, its
 * position in the launch, the chunk or the shard —, the product of (candidate, group) is computed once and written to every layer of the
 * group, and a row of zeros gives base bit for bit.  Numpy mirror: tests/subspace_ref.py.
 *
 * glass_subspace_supported: the one rule (host only: callable without a GPU), applied by both setters.  latent_size % 4 == 0; 1 <=
 * components <= min(latent_size, 512); 1 <= groups <= n_lat; each layer_group value -1 or in [0, groups) and every group non-empty
 * (layer_group NULL: the shape alone).  max_pop * groups * components < 2^31 is checked where max_pop is known (set_subspace_shape,
 * finalize).  Returns GLASS_OK, or GLASS_ERR_ARG with the reason in glass_last_error() and, when why is not NULL, in why[why_len].
 * glass_engine_set_subspace_shape: between set_latent_space(GLASS_LATENT_SUB) and finalize, which sizes the coefficient buffer
 * [max_pop][G K], the per-layer dlatents, the style tiles and the device search's buffers (row width G K); glass_engine_latent_row
 * reports G K after it.  GLASS_ERR_STATE after finalize, in another space, and on a BigGAN or generator-less engine, by name.
 * glass_engine_set_subspace: after finalize, any time between passes, as set_truncation is: validates through the rule and uploads;
 * a stored anchor is recomputed from its row.  evaluate, generate, search_*, expand_latents and set_anchor on a sub engine before it fail
 * (GLASS_ERR_STATE, "set_subspace() first").
 * glass_engine_expand_latents: the dlatents the pass makes its styles from, after truncation, by the kernels of the pass: rows
 * [P][floats_per_row] -> out_dlat [P][n_lat][L], P in [1, max_pop].  Works in every StyleGAN2 space (z goes through the mapping network, w
 * is tiled over the layers, w+ comes back as given where psi = 1).  The parity entry point; its output is a w+ row. */
#define GLASS_LATENT_SUB 3
int glass_subspace_supported(int32_t n_lat, int32_t latent_size, int32_t groups, int32_t components, const int32_t* layer_group, char* why,
                             int32_t why_len);
int glass_engine_set_subspace_shape(glass_engine* e, int32_t groups, int32_t components);
int glass_engine_set_subspace(glass_engine* e, const int32_t* layer_group /*[n_lat]*/, const float* basis /*[K][L]*/, const float* base /*[n_lat][L]*/);
int glass_engine_expand_latents(glass_engine* e, const float* rows, int32_t P, float* out_dlat /*[P][n_lat][L]*/);

/* Hand one reference tensor to the engine: `name` is the reference state-dict key
 * prefixed with its sub-model ("G_mapping.", "G_synthesis.", "D.", "clip."; the generator's own "dlatent_avg" unprefixed), data is
 * host float32, row-major, dims[rank].  Replaces stylegan2.models.load (models.py:183-196)
 * + clip.load/build_model (clip/model.py:363-399).  Tensors are repacked into kernel
 * layouts (pre-scaled, fp16, folded FIR) by glass_engine_finalize. */
int glass_engine_load_tensor(glass_engine* e, const char* name, const float* data,
                             int32_t rank, const int64_t* dims);
int glass_engine_finalize(glass_engine* e);

/* Target text feature, host float32 [clip_embed] (generator.py:23-24: encode_text once). */
int glass_engine_set_target(glass_engine* e, const float* feat, int32_t n);

/* CLIP text tower (clip/model.py:307-320), run once at init by the reference (generator.py:23-24).
 * Available when the text-tower tensors ("clip.token_embedding.weight", "clip.positional_embedding",
 * "clip.transformer.resblocks.*", "clip.ln_final.*", "clip.text_projection") were loaded before
 * finalize().  tokens: host int32 [n_texts, ctx] as produced by clip.tokenize (clip/clip.py:125-138);
 * out_feat: host float32 [n_texts, clip_embed]. */
int glass_engine_encode_text(glass_engine* e, const int32_t* tokens, int32_t n_texts, int32_t ctx, float* out_feat);

/* CLIP image tower on caller-supplied images (generator.py:26-27: the img2txt target), host float32
 * [n,3,clip_res,clip_res] already preprocessed as clip.py:68-74 does; out_feat float32 [n, clip_embed]. */
int glass_engine_encode_image(glass_engine* e, const float* images, int32_t n, float* out_feat);

/* GPT-2 greedy decode (config GPT2 / img2txt: models.py:45-62, gpt2/sample.py:21-36 with sample=False).
 * Needs the "gpt2.transformer.*" tensors (reference GPT2LMHeadModel keys after gpt2/utils.py load_weight).
 * context: host int32 [P, n_ctx_tok] (latent tokens ++ init_text tokens); out: host int32
 * [P, n_ctx_tok + length] = context ++ `length` greedily decoded tokens.  All arithmetic is fp32.
 * Limits (GLASS_ERR_ARG otherwise): n_ctx_tok + length <= min(256, the position table); n_ctx_tok <= 126 — the prefill attention keeps
 * one sequence's keys, values and score matrix in LDS, 4 * (n^2 + 196 n) bytes of the 160 KB a workgroup has.  The same limits hold
 * for glass_engine_gpt2_sample. */
int glass_engine_gpt2_decode(glass_engine* e, const int32_t* context, int32_t P, int32_t n_ctx_tok, int32_t length,
                             int32_t* out_tokens);

/* GPT-2 stochastic decode (config GPT2 with stochastic = True: models.py:45-60, gpt2/sample.py:10-36 with sample=True), same
 * context / output layout as glass_engine_gpt2_decode.  Each step divides the logits by `temperature` (> 0), keeps the entries at or
 * above the top_k-th largest (ties included; top_k in [0, 256], 0 or >= vocabulary keeps all), and draws the next token from their
 * softmax with a uniform from Philox4x32-10 at counter (first_row + row, step, generation, purpose) under `seed` (with a fixed tag in
 * the key's high word, disjoint from the noise planes' stream).  first_row: global index of context row 0, so a population decoded
 * in slices gives the same tokens as one call.  purpose: separates draws of the same generation (0: fitness evaluation, 1: the
 * save callback).  Deterministic for equal arguments.  Vocabulary <= 131072. */
int glass_engine_gpt2_sample(glass_engine* e, const int32_t* context, int32_t P, int32_t n_ctx_tok, int32_t length,
                             float temperature, int32_t top_k, uint64_t seed, int32_t generation, int32_t first_row,
                             int32_t purpose, int32_t* out_tokens);

/* THE HOT PATH — replaces GenerationProblem._evaluate (problem.py:14-29).
 * latents: host float32 [P, floats_per_row] row-major (latent.py:37-38): floats_per_row as glass_engine_latent_row reports it —
 *   latent_size unless glass_engine_set_latent_space chose w+; the library cannot see the buffer's size, the caller checks it;
 * generation: index folded into the device noise stream (noise_mode 1);
 * first_minibatch: global index of this call's first minibatch (population shards);
 * noise: nullable, used when noise_mode == 2;
 * out_F: host float32 [P, n_obj]: F[:,0] = -cosine, F[:,1] = relu(1 - D) (problem.py:23-27); with the perceptual objective and
 *   lpips_lambda == 0 the distance is one more, last, column (n_obj up to 3); with a pareto prompt set, sim_columns similarity columns first.
 * P must be a multiple of batch_size (reference asserts: models.py:112). */
int glass_engine_evaluate(glass_engine* e, const float* latents, int32_t P, int32_t generation,
                          int32_t first_minibatch, const glass_noise* noise, float* out_F);

/* Extra outputs of the same pass (nullable each): CLIP image features [P, clip_embed],
 * raw discriminator logits [P], cosine similarities [P]. Valid after evaluate(). */
int glass_engine_last_details(glass_engine* e, int32_t P, float* features, float* dis, float* sim);
/* Crop views: per-view outputs of the last evaluate() (nullable each): features [P][views][clip_embed], cosines [P][views], and the pass's
 * boxes [views][4].  glass_engine_last_details keeps its shapes then: features[p] is view 0's feature (the whole image), sim[p] the mean. */
int glass_engine_last_view_details(glass_engine* e, int32_t P, float* features, float* sims, int32_t* boxes);

/* Generator.generate (generator.py:29-34): images host float32 [P,3,R,R] NCHW after
 * biggan_norm (utils.py:14-17).  Used by run.py's callbacks (run.py:45,118).  latents: [P, floats_per_row], as for evaluate. */
int glass_engine_generate(glass_engine* e, const float* latents, int32_t P, int32_t generation,
                          int32_t first_minibatch, const glass_noise* noise, float* images);

/* GPU time of the last evaluate() in ms, from hipEvents on the engine's stream. */
int glass_engine_last_gpu_ms(glass_engine* e, float* ms);
/* Device address of the fitness rows [P][n_obj] float32 of the last evaluate() (the buffer evaluate() copied `out_F` from; valid until the
 * engine's next call).  The multi-GPU host code hands it to the one RCCL all-gather of a generation (clip_glass_amd/parallel.py) without
 * bouncing the rows through host memory. */
int glass_engine_last_F_device(glass_engine* e, int32_t P, void** dev_ptr);

/* Per-kernel profile (hipEvent pairs around every launch while enabled).
 * After evaluate(): n rows of {name, launches, total_ms, flops, bytes} — algorithmic
 * flops/bytes per DESIGN.md.  Used by bench.py for the `roofline` object. */
typedef struct glass_prof_row {
    char name[96];             /* "<layer tag>@<kernel symbol>" */
    int64_t launches;
    double total_ms;
    double flops;
    double bytes;
} glass_prof_row;
int glass_engine_set_profiling(glass_engine* e, int32_t on);
/* Restrict the per-launch events to launches of kernels whose symbol contains `kernel_substr`
 * (as resolved in the previous profiled pass); NULL/"" = every launch.  Keeps the event overhead
 * out of a timed region that only needs the dominant kernel. */
int glass_engine_set_profile_filter(glass_engine* e, const char* kernel_substr);
int glass_engine_get_profile(glass_engine* e, glass_prof_row* rows, int32_t max_rows, int32_t* n_rows);

/* Stream mode of evaluate() — this call is the ONLY control (the library reads no environment variable).  2 (default): generator and
 * discriminator on one stream, CLIP's image tower (short latency-bound launches) on a second, highest-priority stream next to the
 * discriminator.  1: synthesis of chunk k+1 || resize + D + CLIP of chunk k.  0: one stream — the mode for clean per-kernel profiles
 * (co-running kernels stretch each other).  Results are identical in every mode. */
int glass_engine_set_overlap(glass_engine* e, int32_t on);
/* BigGAN-deep diagnostic: record the activation after GenBlock `block` (-1: after the self-attention block, -2: off) of the first
 * chunk of the next evaluate / generate; get_biggan_tap returns it as NHWC float32 [dims[0]][dims[1]][dims[2]][dims[3]] (out may
 * be NULL to query dims).  The package behind models.py:64-86 is absent from the reference tree, so this path is checked
 * block by block against the oracle's restatement: a real checkpoint that mismatches fails at the first wrong block. */
int glass_engine_set_biggan_tap(glass_engine* e, int32_t block);
int glass_engine_get_biggan_tap(glass_engine* e, float* out, int64_t capacity, int32_t dims[4]);

/* Device search (opt-in; off unless glass_engine_set_search is called): the GA / NSGA-II generation step — mating, variation, duplicate
 * flags, survival — on the device, between two passes, in static shapes and with no host decision.  The population (pop rows of
 * floats_per_row fp32 variables), its F, rank and crowding distance stay in device buffers; a generation is glass_engine_search_step.
 * Real-valued rows: StyleGAN2 engines in z, w and w+ (glass_engine_set_search).  Mixed rows — real columns, then boolean bit columns: a
 * BigGAN engine's [z | class bits] — through glass_engine_set_search_mixed ("Mixed rows" below); glass_engine_set_search refuses a BigGAN
 * engine by name.  An engine without a generator (GPT-2: integer rows, scored through the host tokenizer every generation) is refused by
 * name and keeps the host search of clip_glass_amd/search.py, which this section restates operator by operator; where it departs from it,
 * it says so.
 *
 * Random numbers.  Philox4x32-10 under key (seed_lo, seed_hi ^ 0x53524348); a draw is u = (word + 0.5) 2^-32, exact in double.  The counter
 * is (index, variable, generation, purpose) and words (w0, w1, w2, w3) give (u0, u1, u2, u3):
 *   purpose 0, tournament: index = mating m, variable = 0.  u0, u1: the contestants of parent A; u2, u3: those of parent B.
 *   purpose 1, crossover:  index = mating m, variable = j.  u0: the SBX spread, u1: the swap, u2: the per-variable gate.
 *   purpose 2, mutation:   index = offspring row r, variable = j.  u0: the perturbation, u1: the gate.
 * A draw is a pure function of (seed, generation, m or r, j, purpose): nothing depends on the launch geometry, and offspring rows produced in
 * one launch or in several agree bit for bit.  Numpy mirror: synth.search_uniforms.
 *
 * Mating.  Offspring rows 2m and 2m + 1 are the two children of mating m (an odd pop drops the last mating's second child).  Each of the two
 * parents is the winner of a binary tournament between population rows a = floor(u n) and b = floor(u' n) (n = pop, double arithmetic): a wins
 * when rank[a] < rank[b], or the ranks are equal and cd[a] >= cd[b]; otherwise b (search.py:221).  GA: rank is 0 and cd is -F[:, 0].
 * This is pymoo's count — pop / 2 matings, both children kept.  search.vary draws pop matings and keeps a random half of their 2 pop
 * children; a child's distribution is the same, the pairing of siblings is not.
 *
 * Variation.  With y1 = min, y2 = max of the parents' variable, d = max(y2 - y1, 1e-300), the scalar bounds xl / xu and u = u0:
 *   betaq(b) = (u alpha)^(1 / (eta_c + 1)) where u <= 1 / alpha, else (1 / max(2 - u alpha, 1e-300))^(1 / (eta_c + 1)); alpha = 2 - b^-(eta_c + 1)
 *   c1 = clip(0.5 ((y1 + y2) - betaq(1 + 2 (y1 - xl) / d) d)), c2 = clip(0.5 ((y1 + y2) + betaq(1 + 2 (xu - y2) / d) d))
 * swapped where u1 < 0.5; the variable is crossed where u2 < 0.5 and y2 - y1 > 1e-14 (child 0 takes c1, child 1 c2), otherwise child 0
 * keeps parent A's value and child 1 parent B's — search.sbx_vectorised with crossover probability 1.  Then search.polynomial_mutation on
 * each child x where u1 < prob_m, with u = u0, span = xu - xl, d1 = (x - xl) / span, d2 = (xu - x) / span:
 *   dq = (2u + (1 - 2u)(1 - d1)^(eta_m + 1))^(1 / (eta_m + 1)) - 1 where u <= 0.5, else 1 - (2(1 - u) + 2(u - 0.5)(1 - d2)^(eta_m + 1))^(1 / (eta_m + 1))
 *   x = clip(x + dq span).
 * All of it is evaluated in double, in search.py's order of operations and without fused multiply-adds, and rounded ONCE to the fp32 row:
 * a float64 mirror agrees to that rounding and the last bit of pow().  xl and xu must be exact in fp32.
 *
 * Mixed rows.  A mixed row is n_real real columns followed by n_bits bit columns (fp32 0.0 / 1.0); n_var = n_real + n_bits, and "variable j"
 * is always the column index in the whole row.  The real columns behave exactly as above — the same tournament, the same draws at counter
 * (index, j, generation, purpose 1 / 2), the same double arithmetic rounded once: columns [0, n_real) of a mixed search equal, bit for bit,
 * the offspring of an all-real search of width n_real with the same seed, generation, ranks and parents' values.  The bit columns take three
 * more purpose words:
 *   purpose 3, bit-crossover gate: index = mating m, variable = 0.  The mating exchanges bits iff u0 < prob_x.
 *   purpose 4, bit key:            index = mating m, variable = j.  The raw 32-bit word w0 is column j's key.
 *   purpose 5, bit-flip:           index = offspring row r, variable = j.  The bit flips iff u0 < prob_flip.
 * Half-uniform crossover (search.hux with prob_hux = 0.5): D is the set of bit columns where the two parents differ by value and n =
 * (|D| + 1) >> 1.  If the gate is open, column j of D is exchanged iff fewer than n columns j' of D have (key[j'], j') < (key[j], j): child 0
 * (row 2m) then takes parent B's bit and child 1 (row 2m + 1) parent A's.  Every other bit column is copied, child 0 from A and child 1 from
 * B.  Independent keys rank D in a uniformly random order, so the exchanged columns are a uniformly random n-subset of D, as
 * rng.permutation(diff)[:n] is; equal keys are broken by the column index, a bias of order |D|^2 / 2^33.  Then bit-flip on each child: x ->
 * 1 - x where the purpose-5 gate fires (search.bitflip).  Bits are never clipped and never touched by SBX or the polynomial mutation.  As
 * for the real columns, a draw is a pure function of (seed, generation, m or r, j, purpose): offspring rows made in one launch or in
 * several, in any grid, agree bit for bit.  An odd pop drops the last mating's second child.  Duplicate flags, survival and the gather do
 * not care what a column means and are used unchanged.  search_init checks on the host that every bit column of X0 holds exactly 0.0 or
 * 1.0 (GLASS_ERR_ARG otherwise, naming the first offending row and column).  Numpy mirror: tests/search_mixed_ref.py.
 *
 * Duplicates.  Offspring row r is flagged when it equals, by value in every variable (-0.0 equals 0.0), a row of the current population or
 * an offspring row with a lower index.  A flagged row is still scored — the shapes stay static — and is left out of survival.  search.py
 * drops such rows and refills the batch with fresh matings instead (and compares with a tolerance of 1e-16): the device search may
 * therefore rank fewer than pop new candidates in a generation.  An offspring row whose F is not finite is left out the same way.  Both
 * counts are readable (glass_engine_search_read).  A population row is never left out: search_init refuses a non-finite F.
 *
 * Survival over the merged rows — the population first, then the offspring that are not left out; "index" is the merged index.
 * GA: the first pop rows by (F[:, 0], index); rank 0, cd = -F[:, 0].
 * NSGA-II, as minimize's survive() with fast_non_dominated_sort and crowding_distance: fronts are peeled from the domination counts until
 * pop rows are ranked; within a front of more than two rows and for every objective k, in the order of (F_k, index), the two ends get an
 * infinite distance and an inner row adds (F_k[next] - F_k[previous]) / (F_k[last] - F_k[first]) where that span is positive; a front of one
 * or two rows is all infinite.  The distance is a double, summed in the order k = 0 .. n_obj - 1 by one writer per row (no atomics: the
 * bits do not depend on the schedule), with -0.0 and 0.0 tied.  The survivors are the fronts in order, rows by index; the front that does
 * not fit is cut by (-cd, index).  Their X, F, rank and cd become the next population, in that order.
 *
 * glass_search_supported: the one rule (host only: callable without a GPU), applied by the setter and by finalize.  algorithm 0 (GA, n_obj
 * 1) or 1 (NSGA-II); pop in [2, 1024] (2048 merged rows are ranked by one workgroup); n_obj in [1, 6]; pop * n_var below 2^31.  (Algorithm
 * 2, sep-CMA-ES, has its own limits: "Device search: sep-CMA-ES" below.)
 *
 * glass_search_mixed_supported: the same for mixed rows (host only) — everything glass_search_supported says for n_var = n_real + n_bits,
 *   n_real >= 1 and 1 <= n_bits <= 4096 (one workgroup ranks a row's differing bits in LDS).
 *
 * glass_engine_set_search: between create and finalize, which sizes the buffers (GLASS_ERR_STATE after it).  pop <= max_pop and a
 * multiple of batch_size; noise_mode 0 or 1 (caller-provided planes would come from the host every pass).  n_var is the engine's
 * floats_per_row.
 * glass_engine_set_search_operators: any time after set_search — the values that size nothing (bounds, eta, prob_m, seed).  The bounds of a
 *   search in w / w+ come from the mapping network and are known only after finalize.
 * glass_engine_set_search_mixed: the same for a BigGAN engine, whose rows are mixed: n_real must be the engine's z_dim (n_bits is then its
 *   num_classes); prob_x (HUX, per mating) and prob_flip (per bit) in [0, 1].  A StyleGAN2 engine (no bits) and an engine without a
 *   generator are refused by name (GLASS_ERR_STATE).  The search_* entry points below work unchanged on a mixed search.
 * glass_engine_set_search_operators_mixed: any time after set_search_mixed — the values that size nothing, prob_x and prob_flip among them.
 * glass_engine_search_init: X0 host float32 [pop][floats_per_row]: uploads it, scores it as generation 0 and ranks (and orders) it as
 *   minimize's first survive() does.
 * glass_engine_search_vary(generation): the offspring of the current population and their duplicate flags.
 * glass_engine_search_evaluate(generation, first_row, rows): scores offspring rows [first_row, first_row + rows) — whole minibatches — as
 *   glass_engine_evaluate would score them with first_minibatch = first_row / batch_size, and writes their F to the offspring's F rows.
 *   Rows scored in one call or in several (or, later, on several GPUs) get the same bits.
 * glass_engine_search_survive(generation): survival and the gather of the surviving rows into the next population.
 * glass_engine_search_step(generation): the three above for all rows — no device-to-host copy and no host wait between them, one wait at
 *   its end.
 * glass_engine_search_read: nullable outputs — the population's X [pop][floats_per_row], F [pop][n_obj], rank int32 [pop], cd double
 *   [pop]; the last offspring's X, F and flags int32 [pop]; counts int32 [2] = {flagged, non-finite} rows of the last survival.
 * Calls out of order (anything before search_init; evaluate / survive without the generation's vary) return GLASS_ERR_STATE by name.
 * glass_engine_latent_uploads: how many host-to-device latent copies the pass has made on this engine, and their rows — a device-search
 * generation makes none. */
#define GLASS_SEARCH_GA 0
#define GLASS_SEARCH_NSGA2 1
int glass_search_supported(int32_t pop, int32_t n_var, int32_t n_obj, int32_t algorithm);
int glass_engine_set_search(glass_engine* e, int32_t algorithm, int32_t pop, double xl, double xu, double eta_c, double eta_m, double prob_m,
                            uint64_t seed);
int glass_engine_set_search_operators(glass_engine* e, double xl, double xu, double eta_c, double eta_m, double prob_m, uint64_t seed);
int glass_search_mixed_supported(int32_t pop, int32_t n_real, int32_t n_bits, int32_t n_obj, int32_t algorithm);
int glass_engine_set_search_mixed(glass_engine* e, int32_t algorithm, int32_t pop, int32_t n_real, double xl, double xu, double eta_c, double eta_m,
                                  double prob_m, double prob_x, double prob_flip, uint64_t seed);
int glass_engine_set_search_operators_mixed(glass_engine* e, double xl, double xu, double eta_c, double eta_m, double prob_m, double prob_x,
                                            double prob_flip, uint64_t seed);
int glass_engine_search_init(glass_engine* e, const float* X0 /*[pop][floats_per_row]*/);
int glass_engine_search_vary(glass_engine* e, int32_t generation);
int glass_engine_search_evaluate(glass_engine* e, int32_t generation, int32_t first_row, int32_t rows);
int glass_engine_search_survive(glass_engine* e, int32_t generation);
int glass_engine_search_step(glass_engine* e, int32_t generation);
int glass_engine_search_read(glass_engine* e, float* pop_X, float* pop_F, int32_t* rank, double* cd, float* off_X, float* off_F, int32_t* flags,
                             int32_t* counts);
int glass_engine_latent_uploads(glass_engine* e, int64_t* calls, int64_t* rows);

/* Device search: islands (opt-in on top of a GA / NSGA-II device search: glass_engine_set_search_islands; without it the engine launches,
 * allocates and returns exactly what the section above says).  K populations evolve side by side in ONE engine — one copy of the weights,
 * one scoring pass per generation — under different seeds, with rare migration round a ring: the island model, the usual remedy for a
 * small population converging into one basin of a multimodal landscape.  Each island is ranked by one workgroup, so the rows of a search
 * are limited by max_pop and no longer by what one workgroup ranks.
 *
 * Layout and seeds.  K islands of pop rows each; pop keeps its meaning and its limits per island ([2, 1024], a multiple of batch_size).
 * Every buffer is island-major: rows live as [K][pop][n_var], and island i owns rows [i pop, (i + 1) pop) of the population, the
 * offspring, F, rank, cd, flags and chosen.  Island i's Philox seed is seed + i (uint64, wrapping), and inside an island every index the
 * rule above speaks of is LOCAL: mating m, offspring row r, population rows a / b, the merged index.  Island i is therefore, bit for bit,
 * the single search glass_engine_set_search(..., seed + i) on its own rows; real-valued and mixed rows alike.
 *
 * Noise.  With noise_mode 1 the noise plane of a minibatch is that of its index WITHIN its island, (first_minibatch + m) mod (pop /
 * batch_size): every island sees the planes a single search of pop rows sees, and the islands are ranked under common noise, as
 * candidates already are under common crop views (whose boxes do not depend on the row).
 *
 * One pass per generation.  Generation g varies all K pop offspring rows in one launch per kernel (the island is a grid dimension), scores
 * them in one pass of K pop rows, runs survival as K workgroups — each reads its island's population F and offspring F, two planes now
 * that the pass writes K pop offspring rows contiguously — and gathers per island.  No host wait and no latent upload in between.
 *
 * Migration.  Ring topology; `migrants` = n rows every `migrate_every` = M generations (M = 0: never).  It is due after the survival of
 * generation g when g >= 1 and g mod M = 0; K = 1 ignores it.
 *   Order: the rows of an island are ordered by (rank, -cd, index), the tournament's order; for the GA that is by F.
 *   Sources: island i receives the n best rows of island (i - 1 + K) mod K; all sources are read from the populations as survival left
 *     them.
 *   Placement: migrant k, the k-th best, is aimed at the receiver's k-th worst row, worst first.
 *   Duplicates: a migrant is dropped when it equals, by value in every variable (-0.0 equals 0.0), a row of the receiving population as
 *     survival left it, or an earlier migrant of the same migration into that island (accepted or not: a dropped one equals a row that
 *     drops the later one too).  Its slot then keeps its row.
 *   An accepted migrant brings its X and its F.  Every island that accepted a migrant is then ranked again by the survival rule over its pop
 *     rows with no offspring, as glass_engine_search_init ranks a population, which also reorders it; an island that accepted none keeps
 *     every bit of its state (ranking it again would reorder a last front that was cut).
 *   1 <= n <= pop / 2, so that the rows an island sends and the rows it replaces are disjoint.  The accepted migrants per island are
 *     readable (glass_engine_search_read_islands).
 * No atomics on floating-point data; the result does not depend on the schedule.  Numpy mirror: tests/search_islands_ref.py.
 *
 * Own prompts (optional).  A prompt set already scores every candidate against every entry in the pass it runs anyway; a weight table
 * [K][T] over the set's T entries lets every island search its own combination: row p of a search pass combines its set_sim with the
 * weights and the sum of |w| of island (first_row + p) / pop, in "Prompt sets"' order of operations.  One non-zero weight of 1 gives the
 * single-target pass against that entry: adding the other entries' +-0 products changes no value.  Mode sum only, and only without a
 * direction source; refused by name with mode pareto, with a direction source and together with migration (a migrant's F would be
 * stale under another island's objective).  A pass outside the search (glass_engine_evaluate) keeps the set's own weights.
 *
 * glass_search_islands_supported (host only): GA and NSGA-II (sep-CMA-ES is refused by name: several distributions are a different
 *   feature); everything glass_search_supported says for (pop, n_var, n_obj); islands in [1, 64]; islands * pop * n_var below 2^31;
 *   migrate_every >= 0; migrants in [1, pop / 2].
 * glass_engine_set_search_islands: after set_search / set_search_mixed and before finalize, which sizes K pop buffers; islands * pop <=
 *   max_pop.  Refused by name: a cmaes search; noise_mode 2 is refused by set_search as before.
 * With islands on: glass_engine_search_init takes [K pop][floats_per_row], island-major, and ranks every island;
 *   glass_engine_search_evaluate(first_row, rows) accepts whole minibatches anywhere in the K pop rows; glass_engine_search_step is vary ->
 *   one pass -> survive -> migrate if due, with one wait at its end; glass_engine_search_read returns K pop rows, island-major, and counts
 *   summed over the islands.
 * glass_engine_set_island_weights: after finalize and glass_engine_set_targets (mode sum): w [islands][T], finite, at least one non-zero
 *   weight per island (zeros are allowed here: an island need not look at every entry); islands and T must be the search's and the set's.
 *   A later set_targets that changes T or the mode makes the next search pass fail by name until the table is set again.
 * glass_engine_search_migrate(generation): the migration as a phase of its own, behind glass_engine_search_survive(generation) (once;
 *   GLASS_ERR_STATE otherwise); it does nothing where the rule has none due.
 * glass_engine_search_read_islands: counts int32 [K][3] = {flagged, non-finite rows of the island's last survival, migrants it accepted in
 *   the last migration}. */
int glass_search_islands_supported(int32_t islands, int32_t pop, int32_t n_var, int32_t n_obj, int32_t algorithm, int32_t migrate_every,
                                   int32_t migrants);
int glass_engine_set_search_islands(glass_engine* e, int32_t islands, int32_t migrate_every, int32_t migrants);
int glass_engine_set_island_weights(glass_engine* e, const float* w /*[islands][T]*/, int32_t islands, int32_t T);
int glass_engine_search_migrate(glass_engine* e, int32_t generation);
int glass_engine_search_read_islands(glass_engine* e, int32_t* counts /*[islands][3]*/);

/* Device search: sep-CMA-ES (opt-in: glass_engine_set_search with algorithm GLASS_SEARCH_CMAES).  The separable CMA-ES of Ros & Hansen
 * (2008) — a diagonal covariance, O(n) state — as a third search rule next to the GA and NSGA-II above: what stays on the device is a
 * distribution, not a population.  One objective, minimised; real-valued rows only (a StyleGAN2 engine in z, w or w+).  With n = n_var,
 * lambda = pop and mu = lambda / 2 (integer division):
 *
 * Setup.  Weights w_i = ln(mu + 1/2) - ln i for i = 1 .. mu, normalised to sum to 1; mu_eff = 1 / sum w_i^2.  Constants:
 *   c_sigma = (mu_eff + 2) / (n + mu_eff + 5)
 *   d_sigma = 1 + 2 max(0, sqrt((mu_eff - 1) / (n + 1)) - 1) + c_sigma
 *   c_c     = (4 + mu_eff / n) / (n + 4 + 2 mu_eff / n)
 *   c_1     = 2 / ((n + 1.3)^2 + mu_eff)
 *   c_mu    = min(1 - c_1, 2 (mu_eff - 2 + 1 / mu_eff) / ((n + 2)^2 + mu_eff))
 *   the separable speed-up: c_1 <- min(1, c_1 (n + 2) / 3), then c_mu <- min(1 - c_1, c_mu (n + 2) / 3)
 *   chi     = sqrt(n) (1 - 1 / (4 n) + 1 / (21 n^2))
 * State, all double: the mean m [n], the diagonal d [n], the paths p_sigma [n] and p_c [n] (zero at the start), the step sigma, and the
 * best row seen (fp32 [n]) with its F (+inf at the start).
 *
 * Generation g = 0, 1, ...
 * 1. Sample.  Row r, column j: z = sqrt(-2 ln u0) cos(2 pi u1) from the Philox draw at counter (r, j, g, purpose 6) — the key and the u =
 *    (word + 0.5) 2^-32 convention of "Random numbers" above; u2 and u3 are unused, 2 pi is the double 6.283185307179586.  x = clip(m_j +
 *    (sigma sqrt(d_j)) z, xl, xu) = min(max(., xl), xu), evaluated in double without fused multiply-adds and rounded ONCE to the fp32 row.  A
 *    draw is a pure function of (seed, g, r, j): rows sampled in one launch or in several agree bit for bit.  Numpy mirror:
 *    synth.search_normals.
 * 2. Score the lambda rows as glass_engine_search_evaluate scores offspring (whole minibatches, first_minibatch = first_row / batch_size).
 * 3. Rank the rows by (F, index); -0.0 ties 0.0; a non-finite F goes last, by index.  If fewer than mu rows have a finite F the generation
 *    updates nothing — every bit of the state stays — and a readable counter (skipped) goes up.  Otherwise the best row seen and its F are
 *    replaced when the generation's best F is strictly smaller.
 * 4. Update from the rows as they were evaluated — the fp32 rows, clipped: clipping is a repair — with y_i = (x_{i:lambda} - m) / sigma for
 *    the mu best, everything per variable j and in this order of operations:
 *      y_w   = sum w_i y_i and s_2 = sum w_i (y_i y_i), both summed in the order i = 1 .. mu by one writer per variable
 *      m       <- m + sigma y_w
 *      p_sigma <- (1 - c_sigma) p_sigma + sqrt(c_sigma (2 - c_sigma) mu_eff) y_w / sqrt(d)              (the old d; left to right)
 *      h       = 1 if ||p_sigma|| / sqrt(1 - (1 - c_sigma)^(2 (g + 1))) < (1.4 + 2 / (n + 1)) chi, else 0
 *      p_c     <- (1 - c_c) p_c + (h sqrt(c_c (2 - c_c) mu_eff)) y_w
 *      d       <- ((1 - c_1) - c_mu) d + c_1 (p_c^2 + (((1 - h) c_c) (2 - c_c)) d) + c_mu s_2                     (the new p_c, the old d)
 *      sigma   <- sigma exp(min(1, (c_sigma / d_sigma) (||p_sigma|| / chi - 1))), then kept inside [1e-10, xu - xl]
 *    ||p_sigma||^2 (of the new p_sigma) is summed from partial sums: variables [256 b, 256 b + 256) form part b, summed in index order, and
 *    the parts are added in the order of b.  The partition is a function of n alone, so the bits do not depend on the grid; there are no
 *    floating-point atomics.  The dependency of p_c, d and sigma on ||p_sigma|| is a kernel boundary.
 * The scalars (sigma, ||p_sigma||, h, the counters) live in a small device struct that one thread writes; nothing in a generation reads
 * the host.  Numpy mirror: tests/cma_ref.py; the host search of clip_glass_amd/search.py ("cmaes" without device=True) is the same rule.
 *
 * glass_search_supported(pop, n_var, n_obj, 2): n_obj = 1, pop in [4, 1024] (mu >= 2; one workgroup ranks the rows), pop * n_var below 2^31.
 * glass_engine_set_search with algorithm 2: as for the GA — between create and finalize, pop <= max_pop and a multiple of batch_size, xl < xu
 *   exact in fp32; eta_c, eta_m and prob_m are ignored.  Refused by name: an engine with n_obj > 1, a BigGAN engine (its bit columns), an
 *   engine without a generator, noise_mode 2.  glass_engine_set_search_operators sets the bounds and the seed, as for the GA.
 * glass_engine_search_init_cma: mean0 [n], diag0 [n] (NULL: ones; every entry positive), sigma0 > 0: the distribution of generation 0.
 *   Zeroes the paths, the counters and the best row.  (glass_engine_search_init is refused by name on a CMA search, and this on a GA one.)
 * glass_engine_search_step(g) is sample -> evaluate -> rank -> update; search_vary(g) is the sample, search_evaluate is unchanged and
 *   search_survive(g) is rank + update.  Calls out of order return GLASS_ERR_STATE by name.
 * glass_engine_search_read keeps its meaning for off_X (the generation's rows), off_F and counts = {0, non-finite rows of the last rank};
 *   the population's outputs (pop_X, pop_F, rank, cd, flags) must be NULL.
 * glass_engine_search_read_cma: nullable outputs — m, d, p_sigma, p_c double [n]; scalars_d double [2] = {sigma, ||p_sigma||}; scalars_i
 *   int32 [5] = {h, finite rows of the last rank, whether it updated, skipped generations, updated generations}; best_X [n]; best_F [1]. */
#define GLASS_SEARCH_CMAES 2
int glass_engine_search_init_cma(glass_engine* e, const double* mean0, const double* diag0, double sigma0);
int glass_engine_search_read_cma(glass_engine* e, double* mean, double* diag, double* p_sigma, double* p_c, double* scalars_d, int32_t* scalars_i,
                                 float* best_X, float* best_F);

/* Device info for bench.py (CU count, name, HBM bytes). */
int glass_device_info(int32_t device, char* name, int32_t name_len, int32_t* cus, int64_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GLASS_H */
