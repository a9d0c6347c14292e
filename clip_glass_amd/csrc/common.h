// common.h — shared types for the gfx950 kernels (wave64, MFMA f16 -> f32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <string>
#include <stdio.h>
#include <stdlib.h>

typedef _Float16 half_t;
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16x __attribute__((ext_vector_type(16)));

#define GLASS_SQRT2 1.41421356237309504880f

// v_mfma_f32_32x32x16_f16: D[32x32] += A[32x16] * B[16x32].
// lane l holds A[i = l&31][k = (l>>5)*8 + j] and B[k = (l>>5)*8 + j][n = l&31], j = 0..7;
// D register r of lane l is D[row = (r&3) + 8*(r>>2) + 4*(l>>5)][col = l&31].
__device__ __forceinline__ f16x mfma32(h8 a, h8 b, f16x c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int mfma32_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
// Philox4x32-10 (counter c, key {k0, k1}) in place — the noise planes (kernels_misc.hip) and the GPT-2 sampler (gpt2.hip);
// numpy mirror: synth.philox4x32
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)c[0] * 0xD2511F53ull, p1 = (uint64_t)c[2] * 0xCD9E8D57ull;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// ---- wave64 reductions: the butterfly over offsets 32, 16, .. 1 leaves the result in every lane.  The ONE wave sum of the library: values
// that tests compare bit for bit across kernels (the cosines of score.hip, unit_rows_kernel) are summed in this order
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// acc + a * b.  FUSED: one rounding (fmaf).  Otherwise the product and the sum are rounded on their own, as numpy float32 does — the operators
// are written in a block with contraction off (HIP's __fmul_rn / __fadd_rn are plain * and + and fuse where contraction is on)
template <bool FUSED>
__device__ __forceinline__ float mac(float acc, float a, float b) {
    if constexpr (FUSED) return fmaf(a, b, acc);
    else {
#pragma clang fp contract(off)
        const float prod = a * b;
        return acc + prod;
    }
}
// max(|f|, 1e-8) of one row by one wave: lane-strided partial sums (i = lane; i < D; i += 64) of separately rounded products, then the wave
// sum.  unit_rows_kernel (edit.hip) and the directional cosine (score.hip) both divide by it: a feature with the source's bits gives x = 0
__device__ __forceinline__ float unit_row_norm(const float* __restrict__ f, int D, int lane) {
    float xx = 0.f;
    for (int i = lane; i < D; i += 64) xx = mac<false>(xx, f[i], f[i]);
    return fmaxf(sqrtf(wave_sum(xx)), 1e-8f);
}

// ---- toRGB applied to a wave's output tile while it is still in registers (conv_stream / conv_tiled / conv_glds) -------------
// The activated fp16 quads a lane holds after the epilogue math (lane (px, kh): channels j*32 + 8g + 4kh + q of pixel px) are a
// valid MFMA B operand as they stand — the K order of an MFMA is free as long as A uses the same one.  A = 16-row weight table
// per image row i of the wave: rows 0-2 (i = 0) / 4-6 (i = 1) the fp16 hi part of w[c][.] * style, rows 8-10 / 12-14 the lo part
// * 2^11; after the MFMAs lane half kh holds image row kh: registers 0-2 hi, 4-6 lo.
// Table element (tab, n, hidx), hidx = ((j*2 + gp)*2 + kh)*8 + e  <->  channel j*32 + 8*(2gp + (e>>2)) + 4kh + (e&3).
__device__ __forceinline__ int trgb_channel(int hidx) {
    const int chunk = hidx >> 3, e = hidx & 7;
    return (chunk >> 2) * 32 + 8 * (2 * ((chunk >> 1) & 1) + (e >> 2)) + 4 * (chunk & 1) + (e & 3);
}
__device__ __forceinline__ half_t trgb_table_value(int tab, int n, float w) {
    if ((n & 3) == 3 || ((n >> 2) & 1) != tab) return (half_t)0.f;
    const half_t hv = (half_t)w;
    return (n & 8) ? (half_t)((w - (float)hv) * 2048.f) : hv;
}
// FIR-upsampled skip image (modules.py:580-602; zero-insert, pad [3,1], 4x4 FIR * 4): out[2m] = .75 x[m-1] + .25 x[m],
// out[2m+1] = .25 x[m-1] + .75 x[m]; taps t[dy*2+dx] = yprev[my-1+dy][mx-1+dx] (clamped loads, zero weight outside)
__device__ __forceinline__ float trgb_skip(const float t[4], int oy, int ox) {
    const int my = oy >> 1, mx = ox >> 1;
    const float wy0 = (oy & 1) ? 0.25f : 0.75f, wx0 = (ox & 1) ? 0.25f : 0.75f;
    float s = 0.f;
    s += ((my >= 1 && mx >= 1) ? wy0 * wx0 : 0.f) * t[0];
    s += (my >= 1 ? wy0 * (1.f - wx0) : 0.f) * t[1];
    s += (mx >= 1 ? (1.f - wy0) * wx0 : 0.f) * t[2];
    s += (1.f - wy0) * (1.f - wx0) * t[3];
    return s;
}

// ---- per-device launch set-up (function attributes, CU counts): one engine per (process, GPU), but ONE process may drive
// several GPUs — a function-local `static bool` would configure the first device only (VERDICT r2 / ADVICE r2) ------------------
// Engines on one GPU may be driven from different host threads: first() is true until SOME caller has come back from the set-up
// block it guards (the set-up calls are idempotent, so a race repeats them; it never lets a thread launch before the attribute is
// set — ADVICE r4: `exchange(true)` marked the device done before the winner's hipFuncSetAttribute had run).  Usage:
//     static DevOnce once;  once.run([&] { hipFuncSetAttribute(...); });
struct DevOnce {
    std::atomic<bool> done[32] = {};
    static int dev() {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 32) return -1;
        return d;
    }
    bool first() const {        // true while the current device's set-up has not been completed by anyone
        const int d = dev();
        return d < 0 || !done[d].load(std::memory_order_acquire);
    }
    void set() {
        const int d = dev();
        if (d >= 0) done[d].store(true, std::memory_order_release);
    }
    template <class F> void run(F&& setup) {     // the usual form: once.run([&] { hipFuncSetAttribute(...); });
        if (first()) {
            setup();
            set();
        }
    }
};
// Where a launcher sends its kernel: a stream — or, with `list` set, a text that receives one line per launch (the kernel's profile name, its
// grid and its block) while nothing is launched and no pointer is followed: the same host code then tells what it would run.
struct LaunchTo {
    hipStream_t st = nullptr;
    std::string* list = nullptr;
    LaunchTo(hipStream_t s) : st(s) {}
    explicit LaunchTo(std::string* l) : list(l) {}
};
template <class... P, class... A>
inline void launch_kernel(const LaunchTo& to, const char* name, void (*kernel)(P...), dim3 g, dim3 b, size_t lds, A... args) {
    if (to.list) {
        char line[192];
        snprintf(line, sizeof line, "%s grid=%u,%u,%u block=%u,%u,%u\n", name, g.x, g.y, g.z, b.x, b.y, b.z);
        *to.list += line;
        return;
    }
    hipLaunchKernelGGL(kernel, g, b, lds, to.st, static_cast<P>(args)...);
}
struct GlassDevProps { int cus, lds_optin; };
inline GlassDevProps glass_dev_props() {   // CU count and the largest dynamic-LDS block a kernel may opt in to, current device
    static std::atomic<int> cus[32] = {}, lds[32] = {};
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 32) d = 0;
    if (!cus[d].load()) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess) {
            lds[d].store((int)prop.sharedMemPerBlockOptin > 0 ? (int)prop.sharedMemPerBlockOptin : (int)prop.sharedMemPerBlock);
            cus[d].store(prop.multiProcessorCount);
        }
    }
    return GlassDevProps{cus[d].load() > 0 ? cus[d].load() : 256, lds[d].load() > 0 ? lds[d].load() : 64 * 1024};
}
inline int glass_cu_count() { return glass_dev_props().cus; }
// Launchers of kernels that opt in to more than the default 64 KB of dynamic LDS ask this first and REFUSE the layer (nullptr /
// false: the dispatcher falls through to the next kernel family) when the device does not offer the block — instead of launching
// into an asynchronous failure that only surfaces as a generic HIP error at the pass's final synchronisation.
// A refusal is reported once per (device, size) on stderr: a runtime that advertises less LDS than gfx950 has (160 KiB) would
// otherwise move every large-LDS family onto its slow fallback in silence.
inline bool glass_lds_fits(int bytes) {
    const GlassDevProps dp = glass_dev_props();
    if (bytes <= dp.lds_optin) return true;
    static std::mutex mu;
    static int seen_dev[16], seen_bytes[16], n_seen = 0;
    int d = 0;
    (void)hipGetDevice(&d);
    std::lock_guard<std::mutex> lk(mu);
    for (int i = 0; i < n_seen; ++i)
        if (seen_dev[i] == d && seen_bytes[i] == bytes) return false;
    if (n_seen == 16) return false;            // table full: the last line printed said so
    seen_dev[n_seen] = d;
    seen_bytes[n_seen++] = bytes;
    if (n_seen == 16) fprintf(stderr, "libglass: further LDS refusals are not reported\n");
    fprintf(stderr, "libglass: device %d offers %d B of opt-in LDS per workgroup; a kernel family that needs %d B is refused and its "
                    "layers fall back to a slower kernel (expected on gfx950: 163840 B)\n", d, dp.lds_optin, bytes);
    return false;
}

// Launch-size thresholds ("does this grid fill the chip?") are evaluated at this NOMINAL population, never at the launch's own
// candidate count: the kernel instance a layer runs on is then a function of the layer geometry alone, and a population scored
// in one call, in chunks or as shards on several GPUs goes through the same arithmetic — bitwise equal rows (tests:
// test_pop512_as_eight_shards_of_64, test_full_size_ffhq_full_population, test_full_size_offset_shards).  64 = the headline
// population per GPU (BASELINE.json configs[1], configs[3]).
#define GLASS_NOMINAL_POP 64

__device__ __forceinline__ float lrelu_sqrt2(float v) { return (v > 0.f ? v : 0.2f * v) * GLASS_SQRT2; }
// Branch-free activation + output scale for the conv epilogues (s > 0): max(v k1, v k2) with
//   act 1 (lrelu 0.2 * sqrt2): (sqrt2 s, 0.2 sqrt2 s);  act 2 (relu): (s, 0);  none: (s, s).
// As f4 arithmetic it compiles to v_pk_mul_f32 pairs + v_max_f32 — a third of the per-value compare / select / multiply chains
// the epilogues spent before (they are VALU-issue bound: every wave of the workgroup is in its epilogue at the same time).
struct ActK { float k1, k2; };
__device__ __forceinline__ ActK act_consts(int act, float s) {
    return ActK{(act == 1 ? GLASS_SQRT2 : 1.f) * s, (act == 1 ? 0.2f * GLASS_SQRT2 : act == 2 ? 0.f : 1.f) * s};
}
__device__ __forceinline__ f4 act_apply(f4 v, ActK k) { return __builtin_elementwise_max(v * k.k1, v * k.k2); }

// Parameters of one convolution launch (implicit GEMM, NHWC fp16 activations).
// GEMM view: M = B*Hc*Wc (conv grid), N = Neff, K = KS*KS*Cin.
struct ConvParams {
    const half_t* x;        // input  [B][H][W][Cin]
    long long x_bstride;    // elements between images (0 = broadcast, e.g. the learned const)
    int B, H, W, Cin;
    int Hc, Wc;             // conv grid (== output grid unless up)
    int KS, stride, pad;
    const half_t* w;        // [KS*KS][Neff][Cin], Cin contiguous
    const half_t* w_up;     // up only: un-folded weights [9][Cout][Cin] for the fused path (nullable)
    long long w_bstride;    // elements between per-sample weight sets (0 = shared weights); pre-modulated path
    int Neff, Cout;         // Neff = Cout * (up ? 4 : 1); n = phase*Cout + o
    int up;                 // 1: depth-to-space 2x2 (folded transposed conv + FIR)
    int Ho, Wo;             // output grid
    const float* sn;        // [B][sn_stride] normalised style (nullable)
    int sn_stride;
    const half_t* sn16;     // fp16 copy of sn, same indexing: what the LDS-tiled kernels read (one 16-byte load per chunk, no
                            // convert on the load path — a convert there would make the kernel wait for its own prefetch)
    const half_t* pre_shift16;  // fp16 copy of pre_shift
    const float* pre_shift; // [B][sn_stride] (nullable; needs sn): x <- relu(x * sn + pre_shift) on the way in, in-bounds
                            // pixels only (zero padding stays zero) — BigGAN batch norm + ReLU ahead of the conv
    int in_up;              // 1: the input is read through a nearest x2 upsample (H, W = upsampled dims; x holds H/2 x W/2)
    const float* dscale;    // [B][ds_stride] demod * smax (nullable)
    int ds_stride;
    const float* noise;     // [n_minibatch][Ho][Wo] (nullable)
    float noise_strength;
    int batch_size;         // candidates per noise plane
    const float* bias;      // [Cout] (nullable)
    const float* shift;     // [B][ds_stride] per-sample per-channel shift added after bias (nullable; BigGAN conditional BN)
    int act;                // 1: leaky-relu(0.2) * sqrt(2); 2: relu
    const half_t* res;      // residual [B][Ho][Wo][res_cs] added after activation (nullable)
    int res_cs;             // channel stride of the residual rows (0 = Cout): first Cout of res_cs channels are used
    int res_up;             // 1: the residual is read through a nearest x2 upsample (it holds Ho/2 x Wo/2)
    float out_scale;
    // conv_stream only: build the 32-channel input map on the fly from the skip image (D fromRGB fused into the first D conv)
    const float* rgb_y;     // [B][3][H][W] fp32 (nullable: normal input x)
    const float* rgb_w;     // [32][3]
    const float* rgb_b;     // [32]
    half_t* rgb_x_out;      // [B][H][W][32]: the fromRGB map, written as a side output (skip path input; nullable)
    half_t* rgb_xs_out;     // [B][H/2][W/2][32]: FIR (pad 1) + ::2 of the fromRGB map — the D block's skip-branch input, taken
                            // from the tile already staged in LDS (nullable)
    // conv_stream only: the generator's LAST conv feeds nothing but toRGB (stylegan2/models.py:852-870, 1004-1013), so the
    // kernel applies it to the activated tile in its accumulators and writes the skip image only — the feature map never
    // reaches HBM.  trgb_yout != nullptr selects this mode (p.y is not written).
    const float* trgb_w;    // [3][Cout] toRGB weights (runtime coefficient applied)
    const float* trgb_b;    // [3]
    const float* trgb_sn;   // [B][trgb_sn_stride] normalised style of the toRGB layer
    int trgb_sn_stride;
    const float* trgb_smax; // [B * trgb_smax_stride]: the style's normaliser (toRGB has no demod to cancel it)
    int trgb_smax_stride;
    const float* trgb_yprev;// [B][3][Ho/2][Wo/2] skip image of the previous block (nullable)
    float* trgb_yout;       // [B][3][Ho][Wo]
    float* rgb_tanh_out;    // conv_tiled (3x3, one 32-wide n tile, fast path): [B][3][Ho][Wo] = tanh of output channels 0..2 taken from the fp32
                            // accumulators (BigGAN's conv_to_rgb[:, :3] + tanh, oracle/biggan_ref.py generator()); p.y is NOT written
    float* trgb_part;       // conv_glds persistent form, layers with SEVERAL 128-wide n tiles: [NTn][B][3][Ho][Wo] fp32 — every n tile writes the toRGB
                            // partial sum of its 128 channels (no bias, no skip image); launch_trgb_finish adds them in n-tile order
    const half_t* trgb_tab; // conv_tiled / conv_glds (their output map IS stored too): [B][2][16][Neff] fp16 weight tables from
                            // launch_trgb_tables (the MFMA A operand of the 1x1 conv in accumulator-lane channel order)
    // conv_tiled<3,1,8,N> only: FIR 4x4 (pad 1) + ::2 of the INPUT map [B][H/2][W/2][Cin] as a by-product of the staged patch — the D
    // block's skip-branch input (modules.py:1238-1254 via 1587-1601), which is a function of the same tensor the block's first conv reads
    half_t* xs_out;
    // upfir only: per-(sample, channel) factor applied to the finished output — the NEXT layer's style, so that the consumer runs
    // without its activation-side modulation (x * s is the same product wherever it is formed)
    const half_t* post_scale16;   // [B][post_stride] (nullable)
    int post_stride;
    // conv_tiled stride 2 only: the D block's skip branch (1x1 conv of the down-sampled block input, modules.py:1238-1254) as extra
    // K stages of the same kernel — after the 3x3 stages the activation is applied IN the accumulators and the skip MFMAs land on
    // top of it (no separate 1x1 pass, no fp16 round trip of its result)
    const half_t* skip_x;   // [B][Ho][Wo][Cin] (nullable)
    const half_t* skip_w;   // [Neff][Cin]
    // chunk-planar activation maps [B][C / 8][H][W][8] (round 6): conv_wreg stages the 16-channel chunks of its input at different times,
    // and in the pixel-major layout the pieces of every 128-byte line crossed the fabric once per chunk (the first LDS-resident form of this layer, two
    // 32-channel chunks: 4.6 GB fetched per launch for 2.15 GB of input, PMC).  With 8-channel planes a line belongs to ONE chunk and a
    // 64-lane LDS-DMA piece (16 B per lane) is 1 KB of contiguous memory.  Only the producer / consumer pairs that implement the layout
    // accept the flags (upfir2<false> / dblock0 write it, conv_wreg reads it); every other launcher refuses them.
    int x_planar32;        // conv_s2 only (round 6): its blurred input map is [B][Cin / 32][H][W][32] — written so by blur_kernel for it.  The kernel
                            // stages ONE 32-channel chunk of a patch per K step; pixel-major, the 64-byte pieces of a 128-byte line belong to two K
                            // steps and every line crossed the fabric twice (PMC traffic 1.59 x the algorithmic bytes: the r256 layer ran at 5.6 TB/s)
    int x_planar8;         // the input map is chunk-planar
    int y_planar8;         // the output map is written chunk-planar
    int row_walk;           // conv_stream: row-major walk of the persistent workgroups (the fromRGB form) instead of down the columns
    half_t* y;              // output [B][Ho][Wo][Cout] fp16 (or)
    float* y32;             // output fp32, same layout
};

// What a launch asks for beyond what every conv family does (bias, act, out_scale): one bit per capability.  A family states the mask it
// implements next to its kernel and refuses `conv_features(p) & ~mask` before it looks at the geometry — a feature is refused, never ignored.
enum ConvFeature : uint32_t {
    CF_UP = 1u << 0,           // up
    CF_STYLE = 1u << 1,        // sn / sn16: activation-side style
    CF_PRE_SHIFT = 1u << 2,    // pre_shift / pre_shift16
    CF_IN_UP = 1u << 3,        // in_up
    CF_DEMOD = 1u << 4,        // dscale
    CF_SHIFT = 1u << 5,        // shift
    CF_NOISE = 1u << 6,        // noise
    CF_RES = 1u << 7,          // res
    CF_RES_CS = 1u << 8,       // res_cs: the residual's rows are wider than Cout
    CF_RES_UP = 1u << 9,       // res_up
    CF_Y32 = 1u << 10,         // y32: fp32 output
    CF_SAMPLE_W = 1u << 11,    // w_bstride: per-sample weights
    CF_BCAST_X = 1u << 12,     // x_bstride == 0 with B > 1: one input map for every candidate
    CF_FROMRGB = 1u << 13,     // rgb_y: the input map built from the skip image
    CF_TORGB = 1u << 14,       // trgb_yout: toRGB image out
    CF_NO_MAP = 1u << 15,      // trgb_yout without y: the feature map is not stored
    CF_TORGB_PART = 1u << 16,  // trgb_part: toRGB partial sums per n tile
    CF_RGB_TANH = 1u << 17,    // rgb_tanh_out: planar tanh of channels 0..2
    CF_XS_OUT = 1u << 18,      // xs_out: blur-down of the input as a by-product
    CF_POST_SCALE = 1u << 19,  // post_scale16
    CF_SKIP = 1u << 20,        // skip_x: the D block's 1x1 skip branch as extra K stages
    CF_X_PLANAR8 = 1u << 21,   // x_planar8
    CF_Y_PLANAR8 = 1u << 22,   // y_planar8
    CF_X_PLANAR32 = 1u << 23,  // x_planar32
    CF_COUNT = 24
};
inline uint32_t conv_features(const ConvParams& p) {
    uint32_t f = 0;
    if (p.up) f |= CF_UP;
    if (p.sn || p.sn16) f |= CF_STYLE;
    if (p.pre_shift || p.pre_shift16) f |= CF_PRE_SHIFT;
    if (p.in_up) f |= CF_IN_UP;
    if (p.dscale) f |= CF_DEMOD;
    if (p.shift) f |= CF_SHIFT;
    if (p.noise) f |= CF_NOISE;
    if (p.res) f |= CF_RES;
    if (p.res_cs) f |= CF_RES_CS;
    if (p.res_up) f |= CF_RES_UP;
    if (p.y32) f |= CF_Y32;
    if (p.w_bstride) f |= CF_SAMPLE_W;
    if (p.x_bstride == 0 && p.B > 1) f |= CF_BCAST_X;
    if (p.rgb_y) f |= CF_FROMRGB;
    if (p.trgb_yout) f |= CF_TORGB;
    if (p.trgb_yout && !p.y) f |= CF_NO_MAP;
    if (p.trgb_part) f |= CF_TORGB_PART;
    if (p.rgb_tanh_out) f |= CF_RGB_TANH;
    if (p.xs_out) f |= CF_XS_OUT;
    if (p.post_scale16) f |= CF_POST_SCALE;
    if (p.skip_x) f |= CF_SKIP;
    if (p.x_planar8) f |= CF_X_PLANAR8;
    if (p.y_planar8) f |= CF_Y_PLANAR8;
    if (p.x_planar32) f |= CF_X_PLANAR32;
    return f;
}
// the name of a feature bit as a refusal message spells it (the diagnostic ops' argument names)
inline const char* conv_feature_name(int bit) {
    static const char* const names[CF_COUNT] = {
        "up", "sn (activation-side style)", "pre_shift", "in_up", "dscale", "shift", "noise", "res", "res_cs", "res_up", "y32 (fp32 output)",
        "premod (per-sample weights)", "broadcast_x", "rgb_y (fused fromRGB)", "trgb_yout (fused toRGB)", "trgb_yout without y (map not stored)",
        "trgb_partial", "rgb_tanh", "xs_out", "post_scale", "skip_x (fused skip)", "x_planar8", "y_planar8", "x_planar32"};
    return bit >= 0 && bit < CF_COUNT ? names[bit] : "?";
}

// A chooser's answer: the kernel instance that takes the launch (its profile name) and the function that launches it, or an empty value —
// the family refuses; `outside` then holds the feature bits its mask lacks (0: the geometry or a combination of features it does not do).
struct ConvKernel {
    const char* name = nullptr;
    void (*launch)(const ConvParams&, hipStream_t) = nullptr;
    uint32_t outside = 0;
    explicit operator bool() const { return launch != nullptr; }
};
inline ConvKernel conv_refused(uint32_t outside = 0) { ConvKernel k; k.outside = outside; return k; }

struct GemmParams {
    const half_t* a;  // [M][K]
    const half_t* w;  // [N][K]
    int M, N, K;
    const float* bias;  // [N] nullable
    int mode;           // 0: out16 = v ; 1: out16 = quickgelu(v) ; 2: x32 += v (in place) ; 3: out32 = v ; 4: out32 = lrelu(v)*sqrt2 ; 5: BatchNorm epilogue (bn_* below)
    half_t* out16;
    float* out32;
    int ldo;
    int kpt;                // 0: w rows are K long.  > 0: w is a packed conv weight [K / kpt][N][kpt] (K steps never straddle a tap)
    long long w_tap_stride; // elements between the taps of such a weight
    int batch;              // 0/1: single problem; >1: blockIdx.z walks problems a_bs / w_bs / o_bs elements apart
    long long a_bs, w_bs, o_bs;
    int cand_rows;          // rows of M one candidate contributes (0: M does not scale with the population) and
    int cand_batch;         // 1: blockIdx.z walks candidates — the tile-width choice is made at the nominal population (GLASS_NOMINAL_POP)
    // implicit patch matrix (conv_gemm.hip, round 6; gemm_tiled only): row m = (b, oy, ox) of the conv grid, column k = (tap, ci) —
    // A[m][k] = x[b][oy * g_stride + ty - g_pad][ox * g_stride + tx - g_pad][ci] (zero outside the image), a = x, K steps never straddle a tap
    int g_on, g_h, g_w, g_hc, g_wc, g_stride, g_pad, g_ks, g_cin;
    long long g_xbs;        // elements between the images of x
    int ld;                 // 0: rows of a and w are K long.  > 0: their row stride (a K slice of longer rows: split-K as `batch` slices,
                            // a_bs = w_bs = K, raw partial sums to out32 + z * o_bs; gemm_tiled only.  With kpt: w_bs = 0, slice z starts at k = z * K of the tap walk)
    // mode 5 (gemm_tiled only): out16 = act(v * bn_a[n] + bn_s[n] (+ res16[m][n])) — inference BatchNorm as an fp32 per-channel scale and shift,
    // the residual added BEFORE the ReLU (CLIP's ResNet bottlenecks, clip/model.py:39-52); bias is not read
    const float* bn_a;      // [N]
    const float* bn_s;      // [N]
    const half_t* res16;    // [M][ldo] (nullable)
    int bn_relu;            // 1: ReLU, 0: none
};
