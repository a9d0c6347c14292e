/* glass_ops.h — diagnostic per-kernel entry points of libglass.so.
 *
 * NOT part of the drop-in boundary (that is include/glass.h).  Each function runs ONE
 * device kernel family of the fitness path on host float32 buffers (converted to the
 * kernel's fp16/fp32 layouts internally), so tests/ can compare every kernel against
 * the oracle's corresponding torch op in isolation.  All return GLASS_OK or a negative
 * status (glass_last_error()).  Layouts are NHWC for activations.
 *
 * Families: the convolution forms of the StyleGAN2 and BigGAN hosts (glass_op_conv), the GEMMs (glass_op_gemm, glass_op_gemm_batched,
 * glass_op_gemm_ex: every plain form with the launcher's answer; tests/test_gpu_vit_block_ops.py against tests/vit_block_ref.py),
 * the StyleGAN2 / CLIP glue kernels, the GPT-2 trunk (glass_op_gpt2_*) and the BigGAN-deep glue kernels and fused tail (glass_op_bg_*;
 * tests/test_gpu_biggan_ops.py against the float64 restatements of tests/biggan_ops_ref.py),
 * and the small fp32 kernels of the mapping network, the style path, D's dense head and the CLIP glue (tests/test_gpu_small_ops.py).
 */
#ifndef GLASS_OPS_H
#define GLASS_OPS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct glass_conv_desc {
    int32_t B, H, W, Cin, Cout;
    int32_t KS, stride, pad;
    int32_t up;            /* 1: conv_transpose2d(stride 2) + 4x4 FIR (modules.py:1089-1139), weights folded */
    int32_t Ho, Wo;        /* output size */
    int32_t broadcast_x;   /* x is [1,H,W,Cin], shared by all B (the learned const) */
    int32_t act;           /* leaky-relu 0.2 * sqrt(2) */
    int32_t batch_size;    /* candidates per noise plane */
    int32_t impl;          /* 0 auto, 1 direct, 2 tiled (behind conv_s2 where that fills the chip), 3 fused up-conv, 4 streaming 32->32, 5 LDS-DMA (conv_wreg, conv_glds; conv_s2 with skip_x), 6 im2col + GEMM.
                            * A refusal is an error that names the families asked and the features they lack */
    float noise_strength, out_scale;
    const float* x;        /* [B,H,W,Cin] */
    const float* w;        /* reference layout [Cout,Cin,KS,KS], un-scaled (coef applied inside) */
    const float* sn;       /* [B,Cin] or NULL */
    const float* dscale;   /* [B,Cout] or NULL */
    const float* noise;    /* [B/batch_size,Ho,Wo] or NULL */
    const float* bias;     /* [Cout] or NULL */
    const float* res;      /* [B,Ho,Wo,Cout] or NULL */
    float* y;              /* [B,Ho,Wo,Cout] */
    /* impl 2 / 4 / 5, all or none: toRGB fused into the conv epilogue — trgb_yout is returned; y too by the forms that store the map (2 / 5) */
    const float* trgb_w;     /* [3,Cout] scaled */
    const float* trgb_b;     /* [3] */
    const float* trgb_sn;    /* [B,Cout] normalised toRGB style */
    const float* trgb_smax;  /* [B] */
    const float* trgb_yprev; /* [B,3,Ho/2,Wo/2] or NULL */
    float* trgb_yout;        /* [B,3,Ho,Wo] */
    /* impl 2, stride 2, both or none: the D block's skip branch as extra K stages — y = (act(conv + bias) + conv1x1(skip_x)) * out_scale */
    const float* skip_x;     /* [B,Ho,Wo,Cin] */
    const float* skip_w;     /* [Cout,Cin,1,1] reference layout, un-scaled */
    /* impl 2, 3x3 stride 1, 64 -> 64: FIR 4x4 (pad 1) + ::2 of the INPUT map as a by-product of the staged patch */
    float* xs_out;           /* [B,H/2,W/2,Cin] or NULL */
    /* impl 5, 64 -> 64: x is handed over chunk-planar, [B,Cin/8,H,W,8] (the layout conv_wreg's producers write for it) */
    int32_t x_planar8;
    /* impl 5 with the fused skip branch (conv_s2): x is handed over in 32-channel planes, [B,Cin/32,H,W,32] (the layout the pad-2 blur writes for it) */
    int32_t x_planar32;
    /* The forms only the StyleGAN2 host builds (stylegan2.cpp g_conv_params / up_link / torgb_conv_params).  A launcher that refuses one is an error. */
    /* 3x3, needs sn (dscale optional), not with broadcast_x: launch_modulate_weights on the packed table (w_up for an up-conv), then the
     * launch as g_conv_params sets a premod layer up — no sn / sn16 / dscale, per-sample weights (w_bstride = 9 Cin Cout) */
    int32_t premod;
    const float* post_scale; /* [B,Cout] or NULL: ConvParams::post_scale16 (fp16), the consumer's style applied to the finished output */
    int32_t y_planar8;       /* y is stored, and handed back, chunk-planar: [B,Cout/8,Ho,Wo,8] */
    /* impl 5 with the trgb_* inputs, Cout a multiple of 128, Ho == Wo: the conv writes toRGB partial sums per 128-wide n tile
     * (ConvParams::trgb_part, NaN-filled before the launch), launch_trgb_finish adds them into trgb_yout; y is returned too */
    int32_t trgb_partial;
    /* The forms only the BigGAN host builds (biggan.cpp bg_conv).  A launcher that refuses one is an error. */
    const float* pre_shift;  /* [B,Cin] or NULL, needs sn: x <- relu(x * sn + pre_shift) while staging, the zero padding stays zero.  The op uploads ONE
                              * per-candidate table [sn | pre_shift] (row stride 2 Cin) and its fp16 copy, as bg_conv points into tab / tab16 */
    int32_t in_up;           /* x is [B,H/2,W/2,Cin], read through a nearest x2 upsample; H, W are the upsampled dims */
    const float* shift;      /* [B,Cout] or NULL: added after the bias (act 2 = ReLU then); uploaded as one table [dscale | shift], ds_stride 2 Cout
                              * (the dscale columns are ones where dscale is NULL) */
    int32_t res_cs;          /* channel stride of the residual rows (0 = Cout): the first Cout of res_cs channels are added (channel-drop skip) */
    int32_t res_up;          /* res is [B,Ho/2,Wo/2,res_cs ? res_cs : Cout], read through a nearest x2 upsample */
    float* rgb_tanh;         /* [B,3,Ho,Wo] or NULL: tanh of output channels 0..2 from the accumulators (ConvParams::rgb_tanh_out), y is not written.
                              * Only conv_tiled implements it (impl 0 / 2); any other impl, or a refusal, is an error */
    int32_t trgb_keep_map;   /* impl 4 with the trgb_* inputs: ask for the skip image AND the stored map (conv_stream writes one of them: it refuses) */
} glass_conv_desc;

int glass_op_conv(int32_t device, const glass_conv_desc* d);
/* out[M,N] = epi(a[M,K] @ w[N,K]^T + bias); mode as GemmParams (0 plain,1 quickgelu,2 +=,3 f32,4 lrelu) */
int glass_op_gemm(int32_t device, int32_t M, int32_t N, int32_t K, const float* a, const float* w,
                  const float* bias, int32_t mode, int32_t impl, float* out);
/* `batch` problems out[z] = a[z] [M,K] @ w[z] [N,K]^T set up as bg_attention (biggan.cpp) sets the self-attention products up: blockIdx.z
 * walks the problems a_bs = M K / w_bs = N K / o_bs = M N elements apart, cand_batch as given.  mode 3 (fp32 out) or 0 (fp16 out).
 * impl 0: gemm_tiled, then gemm_direct where it refuses (as the host); 1: gemm_direct; 2: gemm_tiled (error if it refuses) */
int glass_op_gemm_batched(int32_t device, int32_t batch, int32_t M, int32_t N, int32_t K, const float* a, const float* w, int32_t mode,
                          int32_t cand_batch, int32_t impl, float* out);
/* Everything GemmParams exposes for the plain forms, with the launcher's answer: `batch` problems out[z] [M,ldo] = epi(a[z] [M,K] @ w[z] [N,K]^T
 * + bias [N] (nullable, shared)), a_bs = M K / w_bs = N K / o_bs = M ldo elements apart, ldo >= N, modes 0 .. 4 as glass_op_gemm, cand_rows /
 * cand_batch as GemmParams (what launch_gemm_tiled's fill rule looks at).  impl as glass_op_gemm_batched; with impl 0 a form that gemm_direct
 * does not implement is an error, not a launch.  out [batch,M,ldo] is in and out: the device array is preloaded from it (rounded to fp16 for
 * modes 0 / 1: a NaN stays a NaN), so mode 2's accumulator, the ldo padding and whatever the caller put where the kernel should store come
 * back as the kernel left them — also after a refusal (GLASS_ERR_ARG), when nothing ran.  The device array is followed by 128 guard rows
 * that no kernel may touch (GLASS_ERR_STATE).  kernel [cap >= 64] receives the name the launcher returned. */
int glass_op_gemm_ex(int32_t device, int32_t batch, int32_t M, int32_t N, int32_t K, int32_t ldo, const float* a, const float* w,
                     const float* bias, int32_t mode, int32_t impl, int32_t cand_rows, int32_t cand_batch, float* out, char* kernel,
                     int32_t cap);
int glass_op_dense(int32_t device, int32_t P, int32_t K, int32_t N, const float* x, const float* wt /*[K,N]*/,
                   const float* bias, int32_t in_sq, int32_t mode, const float* eps_row, float* out);
/* The StyleGAN2 glue kernels (kernels_misc.hip): glass_op_torgb, glass_op_blur, glass_op_fromrgb and glass_op_noise stage their output
 * poisoned (every byte 0xFF: an element no thread stores comes back as NaN) and followed by guard elements; a store behind the output is
 * an error (GLASS_ERR_ARG, "... stored behind the output").  toRGB has instances for C = 16, 32, 64, 128, 256, 512; another width is
 * refused (GLASS_ERR_ARG), nothing runs. */
int glass_op_torgb(int32_t device, int32_t B, int32_t H, int32_t C, const float* x, const float* wrgb /*[3,C] scaled*/,
                   const float* bias, const float* sn, const float* smax, const float* yprev, float* yout);
int glass_op_blur(int32_t device, int32_t mode /*0: pad2 stride1, 1: pad1 + ::2, 2: pad2 stride1 written as [B,C/32,H+1,H+1,32]*/, int32_t B, int32_t H, int32_t C,
                  const float* x, float* out);
/* second half of a discriminator block in one kernel (conv_down.hip; stylegan2/modules.py:1204-1254, 1587-1601):
 * y = (lrelu(conv3x3 stride 2 (fir pad 2 (h)) + b1) * sqrt2 + conv1x1(fir pad 1 (x)[::2])) / sqrt2.
 * h, x [B,R,R,Cin]; w1 [Cout,Cin,3,3], wskip [Cout,Cin,1,1] (reference layouts, un-scaled); y [B,R/2,R/2,Cout] */
int glass_op_dblock_down(int32_t device, int32_t B, int32_t R, int32_t Cin, int32_t Cout, const float* h, const float* x,
                         const float* w1, const float* wskip, const float* b1, float* y);
/* the discriminator's whole full-resolution block (conv_d0.hip; stylegan2/models.py:1125-1143, modules.py:1204-1254, 1587-1601):
 * y [B,3,R,R] skip image -> denorm(norm(y)) -> fromRGB (3 -> 32) -> conv3x3 (32 -> 32) -> FIR pad 2 -> conv3x3 stride 2 (32 -> 64),
 * + conv1x1 of FIR pad 1 [::2] of the fromRGB map, merged / sqrt2.  frgb_w [32,3] scaled; w0 [32,32,3,3], w1 [64,32,3,3],
 * wskip [64,32,1,1] reference layouts, un-scaled; out [B,R/2,R/2,64].  impl 0: the fused kernel; 1: conv_stream<fromrgb> + conv_down;
 * 2: the fused kernel writing out chunk-planar, [B,8,R/2,R/2,8] */
int glass_op_dblock0(int32_t device, int32_t B, int32_t R, int32_t impl, const float* y, const float* frgb_w, const float* frgb_b,
                     const float* w0, const float* b0, const float* w1, const float* wskip, const float* b1, float* out);
/* glass_op_conv, glass_op_dblock_down and glass_op_dblock0 stage every device output poisoned (every byte 0xFF: an element no thread stores
 * comes back as NaN), and so the scratch one launch of the op writes for the next (toRGB weight tables, pre-modulated weights, the im2col
 * matrix and the split-K slices): a consumer that reads what its producer left out yields NaN.  The image-shaped outputs (y, trgb_yout,
 * xs_out; xs, y; h, xs, out) have one 16-row tile of guard elements in front and behind; a store there is GLASS_ERR_STATE, and the message
 * names the buffer, the side and the element.
 * glass_op_last_kernel: the symbol of the kernel the calling thread's last glass_op_conv / glass_op_dblock_down / glass_op_dblock0 chose
 * (what ConvKernel::name, launch_conv_gemm, launch_conv_down and launch_dblock0 return; the two launches of dblock0 impl 1 joined by
 * " + "), NUL-terminated into buf [cap]; empty if that op launched nothing.  GLASS_ERR_ARG: cap too small. */
int glass_op_last_kernel(char* buf, int32_t cap);
int glass_op_fromrgb(int32_t device, int32_t B, int32_t R, int32_t Cout, const float* y /*[B,3,R,R]*/,
                     const float* w /*[Cout,3] scaled*/, const float* bias, float* out /*[B,R,R,Cout]*/);
int glass_op_mbstd(int32_t device, int32_t B, int32_t hw, int32_t C, int32_t Cpad, int32_t batch_size, int32_t group,
                   const float* x, float* out);
int glass_op_resize(int32_t device, int32_t B, int32_t R, int32_t S, int32_t ps, const float* y /*[B,3,R,R]*/,
                    float* patches /*[B*G*G, 3*ps*ps]*/);
/* The crop-view resize of the engine (glass_engine_set_clip_views) on caller images and boxes int32 [V][4] = (x0, y0, s, flip), each inside
 * the image.  Dense output as glass_op_resize; the row of (image b, view v, patch g) is (b V + v) G G + g. */
int glass_op_view_patches(int32_t device, int32_t B, int32_t R, int32_t S, int32_t ps, int32_t normalize, int32_t V, const int32_t* boxes,
                          const float* y /*[B,3,R,R]*/, float* patches /*[B*V*G*G, 3*ps*ps]*/);
/* The engine's CLIP preprocessing (glass_config::clip_resize / clip_normalize) on caller images: (0, 0) launches what glass_op_resize
 * launches, (0, 1) the normalising instance of that kernel, resize_mode 1 / 2 preprocess_patches_kernel.  Dense output as glass_op_resize. */
int glass_op_preprocess(int32_t device, int32_t B, int32_t R, int32_t S, int32_t ps, int32_t resize_mode, int32_t normalize,
                        const float* y /*[B,3,R,R]*/, float* patches /*[B*G*G, 3*ps*ps]*/);
int glass_op_layernorm(int32_t device, int32_t M, int32_t D, const float* x, const float* g, const float* b, float* out);
int glass_op_attention(int32_t device, int32_t n_img, int32_t L, int32_t heads, int32_t causal, const float* qkv,
                       float* out);
int glass_op_noise(int32_t device, int32_t n_mb, int32_t hw, uint32_t layer, uint32_t mb0, uint32_t generation,
                   uint64_t seed, float* out);
/* The GPT-2 stochastic pick (gpt2.hip, gpt2_sample_kernel, the engine's generic path) on caller logits [rows, V] float32: top-k
 * temperature sampling as glass_engine_gpt2_sample draws it at step `step` for global rows first_row .. first_row + rows - 1
 * (temperature > 0, top_k in [0, 256], 0 = keep all; V <= 131072); out: int32 [rows]. */
int glass_op_gpt2_sample(int32_t device, int32_t rows, int32_t V, const float* logits, float temperature, int32_t top_k,
                         uint64_t seed, int32_t generation, int32_t first_row, int32_t step, int32_t purpose, int32_t* out);
/* The GPT-2 trunk's fp32 kernels (gpt2.hip), each launched as the passes of gpt2_host.cpp launch it.  A shape a launcher does not
 * take is an error (glass_last_error names the condition), never a different kernel.
 *
 * glass_op_gpt2_gemm: out[M,N] = A[M,K] (row stride lda >= K) @ W[N,K]^T (+ bias[N], nullable); mode 0 plain, 1 GELU-tanh, 2 out += (out
 * holds the residual on entry).  form 0: launch_gemm_f32(prefill = true); 1: launch_gemm_f32(prefill = false); 2: choose_gemm_f32_step (with the device's
 * CU count) + launch_gemm_f32_step, finished by launch_gpt2_reduce (modes 0 / 1) or launch_gpt2_finalize (mode 2; N <= 1024); 3: choose_gemm_f32_rowblk + launch_gemm_f32_rowblk.  The split-K scratch
 * holds 16 * M * 4 * width floats, as the engine sizes it for a model of that width.  lng / lnb [K] (forms 2 / 3, modes 0 / 1): the operand
 * is LayerNorm(A) with the row statistics of the device's own producers — form 2: gpt2_finalize_kernel over A (lda == K), returned in
 * stats_out [M,2] = {mean, rstd}; form 3: the (mean, M2) partials pst_in [M, np_in, 2] an earlier form-3 call returned.  stats_out
 * also receives the statistics a form-2 residual product leaves for the next LayerNorm; pst_out [M, N/32, 2] (form 3, nullable) the row
 * partials of the epilogue.  *splits: the global K split the launcher chose (1 for forms 0, 1 and 3).  The device output is followed
 * by guard rows up to the next multiple of 64: a store to a row >= M is an error (GLASS_ERR_STATE). */
int glass_op_gpt2_gemm(int32_t device, int32_t form, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t mode, int32_t width,
                       const float* a, const float* w, const float* bias, const float* lng, const float* lnb, const float* pst_in,
                       int32_t np_in, float* out, float* stats_out, float* pst_out, int32_t* splits);
/* One attention launch over caller caches kc / vc [P, Tmax, D = 64 * heads] (in and out: the call appends rows past .. past + nd - 1).
 * form 0: launch_gpt2_attention with the host's `past`; 1: the same kernel reading `past` from device memory (LDS sized for Tmax);
 * 2: launch_gpt2_attention_step (nd == 1, Tmax <= 64).  qkv: [P * nd, 3 D] finished values (S == 0), or for form 2 with S in [1, 16] the
 * S split-K slices [S, P, 3 D] the kernel sums itself, plus bias [3 D] (nullable).  out: [P * nd, D]. */
int glass_op_gpt2_attention(int32_t device, int32_t form, int32_t P, int32_t nd, int32_t past, int32_t Tmax, int32_t heads, int32_t S,
                            const float* qkv, const float* bias, float* kc, float* vc, float* out);
/* The vocabulary head of a single-token step on x [M, K] (M <= 64, K % 64 == 0, K <= 1024, V >= 4096): launch_gpt2_finalize(part = nullptr)
 * for the row statistics (returned in stats [M,2]), then
 * tail == 0: launch_gpt2_head with the arg-max pick and logits -> logits [M, V], the block (max, lowest index) pairs pair_val / pair_idx [M, ceil(V/32)], token [M];
 * tail != 0: launch_gpt2_head with the arg-max + embed / advance tail at the state {past, step, 0} -> token [M], the next step's embedding x_next [M, K] (wte[token] +
 *            wpe[past + 1]; wpe [npos, K]), its statistics stats_next [M, 2] and the state words state [3] afterwards. */
int glass_op_gpt2_head(int32_t device, int32_t M, int32_t V, int32_t K, int32_t tail, const float* x, const float* wte, const float* lng,
                       const float* lnb, const float* wpe, int32_t npos, int32_t past, int32_t step, float* logits, float* pair_val,
                       int32_t* pair_idx, int32_t* token, float* stats, float* x_next, float* stats_next, int32_t* state);
/* launch_gpt2_embed_step with statistics at the state {past, step}: x [M, K] = wte[token] + wpe[past], stats [M, 2] — the other producer
 * of a step's first operand (token [M] = the previous step's picks). */
int glass_op_gpt2_embed_step(int32_t device, int32_t M, int32_t V, int32_t K, const int32_t* token, const float* wte, const float* wpe,
                             int32_t npos, int32_t past, int32_t step, float* x, float* stats);
/* The BigGAN-deep glue kernels (biggan_kernels.hip) and the fused last stage (bg_tail.hip), each launched as biggan.cpp launches it.
 *
 * glass_op_bg_cond: launch_bg_cond on population rows x [P,L] = [z (zd) | class bits (nc) | ...], et = E^T [nc,zd] -> cond [P, 2 zd].
 * glass_op_bg_bn_tables: the three launches of glass_biggan_prepare — launch_dense (cond [P,cd] x wt [cd,2C] + bias [2C]),
 *   launch_bg_bn_tables (inv_std / mean / prebias [C]) and launch_bg_to_half -> tab [P,2C] = [A | S] fp32 and tab16, its fp16 copy.
 * glass_op_bg_attn_split: T [B,H,W,2 c8 + c2] (theta | phi | g) -> theta [B,HW,c8], phi [B,HW/4,c8], gT [B,c2,HW/4]; *vec = 1 when the
 *   launcher took bg_attn_split_vec_kernel, 0 for bg_attn_split_kernel (H, W even).
 * glass_op_bg_softmax: S [rows,n] fp32 -> row softmax [rows,n] (fp16 values).
 * glass_op_bg_rgb_tanh: x [B,hw,C] (fp16) -> y [B,3,hw] = tanh of channels 0..2.
 * glass_op_bg_to_half: x [n] -> out [n] (fp16 values), any n.
 * glass_op_bg_tail: h [B,R,R,mid], x0 [B,R/2,R/2,128], w3 [128,mid], b3 [128], the final bn's A / S [128], rgb_w [3,128,3,3], rgb_b [3]
 *   -> y [B,3,R,R]; refused where bg_tail_supported says no (R % 32 == 0, mid == 32).  Weights are taken as given (no coefficient). */
int glass_op_bg_cond(int32_t device, int32_t P, int32_t L, int32_t zd, int32_t nc, const float* x, const float* et, float* cond);
int glass_op_bg_bn_tables(int32_t device, int32_t P, int32_t cd, int32_t C, const float* cond, const float* wt, const float* bias,
                          const float* inv_std, const float* mean, const float* prebias, float* tab, float* tab16);
int glass_op_bg_attn_split(int32_t device, int32_t B, int32_t H, int32_t W, int32_t c8, int32_t c2, const float* T, float* theta, float* phi,
                           float* gT, int32_t* vec);
int glass_op_bg_softmax(int32_t device, int32_t rows, int32_t n, const float* S, float* out);
int glass_op_bg_rgb_tanh(int32_t device, int32_t B, int32_t hw, int32_t C, const float* x, float* y);
int glass_op_bg_to_half(int32_t device, int64_t n, const float* x, float* out);
int glass_op_bg_tail(int32_t device, int32_t B, int32_t R, int32_t mid, const float* h, const float* x0, const float* w3, const float* b3,
                     const float* bn_a, const float* bn_s, const float* rgb_w, const float* rgb_b, float* y);
/* CLIP's ResNet image towers (clip_resnet.hip, gemm_tiled.hip mode 5), each piece launched as the tower's walker (clip.cpp) launches it.
 * BatchNorm is given as the fp32 per-channel scale bn_a and shift bn_s the engine keeps.  A launcher that refuses is an error.
 * glass_op_rn_avgpool: AvgPool2d(2) of x [B,H,W,C] -> [B,H/2,W/2,C].
 * glass_op_rn_stem_conv1: img [B,3,S,S] -> launch_image_patches (32-pixel patches, the layout every preprocessing mode writes) -> conv 3x3
 *   stride 2 pad 1 with w [C1,3,3,3] + BN + ReLU -> [B,S/2,S/2,C1].
 * glass_op_rn_conv_bn: out = act(conv(x, w) * bn_a + bn_s (+ res)), x [B,H,W,Cin], w [Cout,Cin,KS,KS], res [B,H,W,Cout] or NULL, stride 1.
 *   form 0, the bottlenecks' convolutions on gemm_tiled: KS 1 (fewer than 64 rows run as 64 in padded buffers), KS 3 through the implicit
 *   patch matrix (Cin % 64 == 0, ReLU, no res); form 1, the stem's conv2 / conv3 kernel: KS 3, Cin % 16 == 0, ReLU, no res.
 * glass_op_rn_tokens: x [B,HW,C], pos [HW+1,C] -> the attention pool's tokens [B,HW+1,C] = [mean ; pixels] + pos. */
int glass_op_rn_avgpool(int32_t device, int32_t B, int32_t H, int32_t W, int32_t C, const float* x, float* out);
int glass_op_rn_stem_conv1(int32_t device, int32_t B, int32_t S, int32_t C1, const float* img, const float* w, const float* bn_a,
                           const float* bn_s, float* out);
int glass_op_rn_conv_bn(int32_t device, int32_t form, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t relu,
                        const float* x, const float* w, const float* bn_a, const float* bn_s, const float* res, float* out);
int glass_op_rn_tokens(int32_t device, int32_t B, int32_t HW, int32_t C, const float* x, const float* pos, float* out);
/* The small fp32 kernels around StyleGAN2 and the CLIP towers (kernels_misc.hip, kernels_clip.hip, clip_resnet.hip), each launched as the
 * engine's host code launches it (tests/test_gpu_small_ops.py against the float64 restatements of tests/small_ops_ref.py).  Operands with a
 * row stride hold whatever the caller put between the rows; an output wider than what the kernel writes is uploaded first and comes back
 * whole, so that the caller sees what the kernel left alone.
 *
 * glass_op_mapping: launch_mapping, the launcher run_mapping calls — z [P,L], wt [n_layers][L(k)][L(n)] (transposed, coefficient folded), b
 *   [n_layers][L] -> out [P,L].  path 0: as run_mapping decides; 1: the per-layer path (pixelnorm_kernel + dense_splitk_kernel, or
 *   dense_kernel where L % 64 != 0 or L > 768); 2: mapping_fused_kernel, an error where it refuses.  *ran: 1 fused | 2 pixelnorm | 4
 *   dense_splitk | 8 dense.
 * glass_op_dense_splitk: launch_dense_splitk (K % 64 == 0, K <= 768; mode 0 / 1) on x [P,ldx], out [P,ldo] (in and out).
 * glass_op_dense_ex: launch_dense with its strides: x [P,ldx], out [P,ldo] (in and out), eps_row [P,eps_stride] (mode 2 reads column 0).
 * glass_op_dense_multi: n problems in one launch_dense_multi (in_sq 1, mode 2, no bias, as the demodulation launch): problem i reads columns
 *   x_off[i] .. + K[i] of x [P,ldx], its weights wt_i [K[i],N[i]] (concatenated in wt) and eps_rows[p, eps_idx[i]] (eps_rows [P,eps_stride]),
 *   and writes columns out_off[i] .. + N[i] of out [P,ldo] (in and out).
 * glass_op_style_norm: launch_style_norm (eps 1e-8) on s [P,ld] in place over the segments (off[l], len[l]) -> smax, eps_row [P,n_layers].
 * glass_op_d_head: D's dense head on dfin [P,16 CL] and w0 [CL,16 CL] (both rounded to fp16), b0 [CL], w1 [CL], b1 [1] -> dis [P], through
 *   the launchers run_d_head calls: the split-K gemm_tiled + dense01_finish_kernel form where it applies (*split = 1), else gemm_tiled /
 *   gemm_direct + dense_kernel (*split = 0).
 * glass_op_layernorm_ex: launch_layernorm on rows row_stride apart (x holds (M - 1) row_stride + D floats); half_out: the fp16 output.
 * glass_op_layernorm_rows: out[m] = LN(x[rows[m]]), x [n_rows,D].
 * glass_op_cosine_views: feat [P,V,D] -> view_sim [P,V], sim [P].
 * glass_op_cosine_set: launch_cosine_set (csrc/score.hip — the one cosine launcher, which glass_op_cosine and glass_op_cosine_views reach with
 *   T = 1 and weight 1, so V <= 16 there too; prompt sets, include/glass.h): feat [P,V,D], targets [T,D], weights [T] (W = their ordered sum of
 *   magnitudes, taken inside) -> view_sim [P,V] (entry 0's cosines), set_sim [P,T], sim [P].  V, T in [1, 16].
 * glass_op_assemble_F_set: the pareto layout: set_sim [P,K], weights [K], dis / lp [P] (nullable each) -> F [P, K + (dis != 0) + (lp != 0)].
 * glass_op_cosine_set_dir: launch_cosine_set with a direction source (image editing, include/glass.h): glass_op_cosine_set's operands plus src [V,D] (unit rows) ->
 *   the same three outputs for x = f / max(|f|, 1e-8) - src[v] in f's place.  streamed 1: the form that streams the set from memory, at any
 *   shape (the launcher chooses it above 64 KB).  A shape the launcher does not take (V or T above 16) is refused by name, nothing launched.
 * glass_op_latent_anchor: launch_latent_anchor: w [P,n_lat,L] (layered 1) or [P,L] (layered 0: the one row serves every layer), a [n_lat,L] ->
 *   d [P], the mean squared difference.
 * glass_op_dlatent_subspace: launch_dlatent_subspace (latent space sub, include/glass.h): c [P,G,K], layer_group [n_lat], basis [K,L], base
 *   [n_lat,L] -> out [P,n_lat,L].  What glass_subspace_supported refuses is refused with its words, nothing launched.
 * glass_op_image_patches: img [n,3,S,S] -> patches [n (S/ps)^2, ld] (fp16 values), pre-filled with `sentinel`.
 * glass_op_rn_token0_rows: att [B,T,C] (fp16) -> out [B,C] = att[b, 0, :]. */
int glass_op_mapping(int32_t device, int32_t P, int32_t L, int32_t n_layers, const float* z, const float* wt, const float* b, int32_t path,
                     float* out, int32_t* ran);
int glass_op_pixelnorm(int32_t device, int32_t P, int32_t L, const float* z, float* out);
int glass_op_dense_splitk(int32_t device, int32_t P, int32_t K, int32_t N, int32_t ldx, int32_t ldo, int32_t mode, const float* x, const float* wt,
                          const float* bias, float* out);
int glass_op_dense_ex(int32_t device, int32_t P, int32_t K, int32_t N, int32_t ldx, int32_t ldo, const float* x, const float* wt, const float* bias,
                      int32_t in_sq, int32_t mode, const float* eps_row, int32_t eps_stride, float* out);
int glass_op_dense_multi(int32_t device, int32_t n, int32_t P, int32_t ldx, int32_t ldo, int32_t eps_stride, const int32_t* K, const int32_t* N,
                         const int32_t* x_off, const int32_t* out_off, const int32_t* eps_idx, const float* x, const float* wt,
                         const float* eps_rows, float* out);
int glass_op_style_norm(int32_t device, int32_t P, int32_t ld, int32_t n_layers, const int32_t* off, const int32_t* len, float* s, float* smax,
                        float* eps_row);
int glass_op_d_head(int32_t device, int32_t P, int32_t CL, const float* dfin, const float* w0, const float* b0, const float* w1, const float* b1,
                    float* dis, int32_t* split);
int glass_op_finalize_image(int32_t device, int64_t n, const float* y, float* img);
int glass_op_embed_lnpre(int32_t device, int32_t P, int32_t T, int32_t D, const float* patch_emb, const float* cls, const float* pos, const float* g,
                         const float* b, float* x);
int glass_op_embed_text(int32_t device, int32_t n_texts, int32_t ctx, int32_t D, int32_t V, const int32_t* tokens, const float* tok_emb,
                        const float* pos, float* x);
int glass_op_layernorm_ex(int32_t device, int32_t M, int32_t D, int64_t row_stride, int32_t half_out, const float* x, const float* g, const float* b,
                          float* out);
int glass_op_layernorm_rows(int32_t device, int32_t n_rows, int32_t M, int32_t D, const float* x, const int32_t* rows, const float* g, const float* b,
                            float* out);
int glass_op_cosine(int32_t device, int32_t P, int32_t D, const float* feat, const float* target, float* sim);
int glass_op_cosine_views(int32_t device, int32_t P, int32_t V, int32_t D, const float* feat, const float* target, float* view_sim, float* sim);
int glass_op_assemble_F(int32_t device, int32_t P, int32_t n_obj, const float* sim, const float* dis, float* F);
int glass_op_cosine_set(int32_t device, int32_t P, int32_t V, int32_t T, int32_t D, const float* feat, const float* targets, const float* weights,
                        float* view_sim, float* set_sim, float* sim);
int glass_op_assemble_F_set(int32_t device, int32_t P, int32_t K, const float* set_sim, const float* weights, const float* dis, const float* lp,
                            float* F);
int glass_op_cosine_set_dir(int32_t device, int32_t P, int32_t V, int32_t T, int32_t D, const float* feat, const float* targets, const float* weights,
                            const float* src, int32_t streamed, float* view_sim, float* set_sim, float* sim);
int glass_op_latent_anchor(int32_t device, int32_t P, int32_t n_lat, int32_t L, int32_t layered, const float* w, const float* a, float* d);
int glass_op_dlatent_subspace(int32_t device, const float* c, int32_t P, int32_t G, int32_t K, const int32_t* layer_group, int32_t n_lat, int32_t L,
                              const float* basis, const float* base, float* out);
int glass_op_image_patches(int32_t device, int32_t n, int32_t S, int32_t ps, int32_t ld, const float* img, float sentinel, float* patches);
int glass_op_rn_token0_rows(int32_t device, int32_t B, int32_t T, int32_t C, const float* att, float* out);
/* The perceptual objective's own kernels (lpips.hip), each through the launcher the walker (lpips.cpp) calls; a shape the launcher does not
 * take is refused by name (GLASS_ERR_ARG).
 * glass_op_lpips_input: y [B,3,R,R] fp32 -> box mean to S (R % S == 0, box <= 8), (v - shift_c) / scale_c -> out [B,S,S,4] (fp16 values; channel 3 = 0).
 * glass_op_vgg_conv1: x [B,S,S,4] (that layout), w [64,3,3,3], bias [64] -> relu(conv3x3 pad 1 + bias) [B,S,S,64].
 * glass_op_maxpool2: MaxPool2d(2) of x [B,H,W,C] -> [B,H/2,W/2,C].
 * glass_op_lpips_head: x0 [n,HW,C], x1 [n,HW,C] (shared_x1 = 0) or [1,HW,C] (1: one map for all), lin [C] -> out[i] = sum_c lin_c
 *   mean_hw (x0 / |x0| - x1 / |x1|)^2, one slice's term. */
int glass_op_lpips_input(int32_t device, int32_t B, int32_t R, int32_t S, const float* y, float* out);
int glass_op_vgg_conv1(int32_t device, int32_t B, int32_t S, const float* x, const float* w, const float* bias, float* out);
int glass_op_maxpool2(int32_t device, int32_t B, int32_t H, int32_t W, int32_t C, const float* x, float* out);
int glass_op_lpips_head(int32_t device, int32_t n, int32_t HW, int32_t C, int32_t shared_x1, const float* x0, const float* x1, const float* lin,
                        float* out);
/* The device search's kernels (search.hip; include/glass.h "Device search"), each through the launcher the engine calls; a shape the launcher
 * does not take is refused by name (GLASS_ERR_ARG).
 * glass_op_ga_vary: X [pop,n_var], rank int32 [pop], cd double [pop] -> offspring rows [row0, row0 + rows) of `generation`, out [rows,n_var].
 * glass_op_ga_vary_mixed: the same for mixed rows of n_real real columns and n_bits bit columns (0.0 / 1.0), X and out [.,n_real + n_bits]:
 *   both kernels of launch_ga_vary (parts GA_VARY_BOTH).  These four run one island, as a single search does.
 * glass_op_ga_duplicates: X [pop,n_var], Xoff [n_off,n_var] -> flags int32 [n_off].
 * glass_op_ga_survive: F [n_pop + n_off, n_obj] (population first), flags int32 [n_off] (nullable) -> chosen int32 [pop_out] (merged indices in
 *   survival order), rank int32 [pop_out], cd double [pop_out], F_out [pop_out,n_obj], counts int32 [2] = {flagged, non-finite rows}; with X
 *   [n_pop,n_var] and Xoff [n_off,n_var] (nullable together) the gathered rows X_out [pop_out,n_var] too.  nsga 0: GA. */
int glass_op_ga_vary(int32_t device, int32_t pop, int32_t n_var, const float* X, const int32_t* rank, const double* cd, double xl, double xu,
                     double eta_c, double eta_m, double prob_m, uint64_t seed, int32_t generation, int32_t row0, int32_t rows, float* out);
int glass_op_ga_vary_mixed(int32_t device, int32_t pop, int32_t n_real, int32_t n_bits, const float* X, const int32_t* rank, const double* cd, double xl,
                           double xu, double eta_c, double eta_m, double prob_m, double prob_x, double prob_flip, uint64_t seed, int32_t generation,
                           int32_t row0, int32_t rows, float* out);
int glass_op_ga_duplicates(int32_t device, int32_t pop, int32_t n_off, int32_t n_var, const float* X, const float* Xoff, int32_t* flags);
int glass_op_ga_survive(int32_t device, int32_t n_pop, int32_t n_off, int32_t n_obj, int32_t pop_out, int32_t nsga, const float* F,
                        const int32_t* flags, int32_t* chosen, int32_t* rank, double* cd, float* F_out, int32_t* counts, int32_t n_var, const float* X,
                        const float* Xoff, float* X_out);
/* The island kernels (search.hip; include/glass.h "Device search: islands").
 * glass_op_ga_migrate: the whole migration — ga_migrate_kernel, then launch_ga_survive gated and launch_ga_gather over the islands, as the
 *   engine launches them:
 *   X [islands pop,n_var], F [islands pop,n_obj], rank int32 and cd double [islands pop] as survival left them -> the same four after the
 *   migration, accepted int32 [islands].  islands >= 2, migrants in [1, pop / 2].
 * glass_op_noise_period: glass_op_noise with launch_noise's period: plane m is that of minibatch (mb0 + m) % period (period 0: mb0 + m). */
int glass_op_ga_migrate(int32_t device, int32_t islands, int32_t pop, int32_t n_var, int32_t n_obj, int32_t nsga, int32_t migrants, const float* X,
                        const float* F, const int32_t* rank, const double* cd, float* X_out, float* F_out, int32_t* rank_out, double* cd_out,
                        int32_t* accepted);
/* glass_op_cosine_set_islands: glass_op_cosine_set with launch_cosine_set's island table: weights [islands,T], row p takes row (row0 + p) / pop. */
int glass_op_cosine_set_islands(int32_t device, int32_t P, int32_t V, int32_t T, int32_t D, const float* feat, const float* targets,
                                const float* weights, int32_t islands, int32_t pop, int32_t row0, float* view_sim, float* set_sim, float* sim);
int glass_op_noise_period(int32_t device, int32_t n_mb, int32_t hw, uint32_t layer, uint32_t mb0, uint32_t generation, uint64_t seed,
                          uint32_t period, float* out);
/* The sep-CMA-ES kernels (cmaes.hip; include/glass.h "Device search: sep-CMA-ES") on caller-supplied state and F, each through the launcher
 * the engine calls; the weights and constants are the library's own for (lambda, n).
 * glass_op_cma_sample: mean [n], diag [n], sigma -> rows [row0, row0 + rows) of `generation` into X [lambda,n], which comes in with the
 *   caller's values: every other row comes back untouched.
 * glass_op_cma_rank: F [lambda] and the best F seen so far -> order int32 [lambda] (rows by (F, index), non-finite last), info int32 [5] =
 *   {finite rows, updated (finite >= mu), the row that became the best seen or -1, skipped generations (0 / 1), non-finite rows},
 *   best_F_out [1].
 * glass_op_cma_update: rank, both update phases and the best-row copy.  X [lambda,n] and F [lambda] are the generation's rows as they were
 *   evaluated; in and out: state double [4,n] = (m, d, p_sigma, p_c), scalars_d double [2] = {sigma, ||p_sigma||}, scalars_i int32 [6] = {h,
 *   finite, updated, skipped, updates, best row of this generation or -1 (out only)}, best_X [n], best_F [1]; out: order int32 [lambda]. */
int glass_op_cma_sample(int32_t device, int32_t lambda, int32_t n, const double* mean, const double* diag, double sigma, double xl, double xu,
                        uint64_t seed, int32_t generation, int32_t row0, int32_t rows, float* X);
int glass_op_cma_rank(int32_t device, int32_t lambda, const float* F, float best_F, int32_t* order, int32_t* info, float* best_F_out);
int glass_op_cma_update(int32_t device, int32_t lambda, int32_t n, const float* X, const float* F, double* state, double* scalars_d,
                        int32_t* scalars_i, double xl, double xu, int32_t generation, float* best_X, float* best_F, int32_t* order);
/* raw MFMA layout probe: D = A[32x16] * B[16x32] through the fragment mapping of common.h */
int glass_op_mfma_probe(int32_t device, const float* a /*[32,16]*/, const float* b /*[16,32]*/, float* d /*[32,32]*/);

/* Host-only (no GPU): the weight repacking finalize() applies, for CPU tests.
 * out: [KS*KS][Neff][Cin] float32 (values already rounded to fp16), Neff = up ? 4*Cout : Cout. */
int glass_host_pack_conv(const float* w, int32_t Cout, int32_t Cin, int32_t KS, int32_t up, float* out);
/* Host-only (no GPU): the tap table finalize() builds for one axis of the antialiased resize R -> S (mode 1 bilinear, 2 bicubic): output
 * i reads inputs start[i] .. start[i] + count[i] - 1 with weights taps[i * max + k] (fp32 roundings of the float64 weights; zero past count).
 * GLASS_ERR_ARG when (R, S, mode) is refused (glass_clip_preprocess_supported) or a row needs more than `max` taps. */
int glass_host_resize_taps(int32_t R, int32_t S, int32_t mode, int32_t* start, int32_t* count, float* taps, int32_t max);
/* Host-only (no GPU): choose_gemm_f32_step's answer for one product — what glass_op_gpt2_gemm's form 2 would launch on a device of n_cu compute
 * units with the scratch of a model of that width: the global K split *S (0: the shape is refused) and the K parts per workgroup *NK. */
int glass_host_gpt2_gemm_choice(int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ln, int32_t width, int32_t n_cu, int32_t* S, int32_t* NK);
/* Host-only (no GPU): what one GPT-2 token step launches for rows P (one group: <= 64), width D, vocabulary V, n_layer blocks, sequence
 * length Tmax (context + generated) and the pick (sample != 0: the stochastic one), with the grids weighed against n_cu compute units
 * (the engine passes the device's).  out receives one line per launch, in launch order: "<kernel's profile name> grid=x,y,z block=x,y,z".
 * The lines come from the step's own host code (gpt2_host.cpp) run into a text instead of a stream.  GLASS_ERR_ARG when cap is too small. */
int glass_host_gpt2_step_plan(int32_t P, int32_t D, int32_t V, int32_t n_layer, int32_t Tmax, int32_t sample, int32_t n_cu, char* out,
                              int32_t cap);

#ifdef __cplusplus
}
#endif
#endif
