// conv_d0.hip — the discriminator's WHOLE full-resolution block in one kernel (gfx950):
//     y (3-channel skip image, fp32) -> biggan denorm(norm(y)) -> fromRGB 1x1 (3 -> 32) + bias + lrelu*sqrt2          = x
//     x -> conv3x3 (32 -> 32) + bias + lrelu*sqrt2                                                                    = h
//     h -> FIR 4x4 (pad 2) -> conv3x3 stride 2 (32 -> 64) + bias + lrelu*sqrt2 \
//     x -> FIR 4x4 (pad 1) -> ::2 -> conv1x1 (32 -> 64)                        +-> (a + b) / sqrt2                     = out
// (stylegan2/models.py:1125-1143, 1193-1230; modules.py:1204-1254 ConvDownLayer, 1587-1601 DiscriminatorConvBlock.forward;
// utils.py:14-21).  Round 2/3 ran this block as two kernels — conv_stream<fromrgb> (x on the fly, h and FIR(x)[::2] to HBM) and
// conv_down (h and the skip input back from HBM): 4.3 GB of h written and read again per 64-candidate population, a full
// store epilogue and a full staging prologue per 64-byte pixel in kernels that are bound by instruction issue, 4.3 ms.  Here only
// the 12-byte-per-pixel image comes in and the 128-byte-per-pixel block output goes out; x and h exist in LDS only.
//
// Geometry.  A step produces 2 output rows x 29 output columns (of the R/2 grid).  It needs h rows 4k-2 .. 4k+5 and columns
// 58tx-2 .. 58tx+59 (an 8 x 62 window inside the 64 columns = two 32-pixel MFMA blocks a row is computed on),
// and for the NEW rows of that window the fromRGB map x on rows 4k+1 .. 4k+6 x columns 58tx-3 .. 58tx+60 (the patch F, 6 x 64 pixels =
// twelve 32-pixel blocks, three per wave; rounds 4-5 used 30-column tiles: a 6 x 66 patch with a thirteenth, 12-pixel block).
// Steps walk DOWN a tile column, so 4 of the 8 window rows are carried from the previous step: a step computes 4 new h rows.  The
// skip-branch input of an output row needs x rows 2o-1 .. 2o+2: the patch of step k holds them for rows 2k+1 and 2k+2, so that input
// runs one row AHEAD of the stride-2 conv, through a 3-row ring.  A workgroup's range starts (and every column starts) with a
// PRIMING step that only computes what the first real step finds carried.
//
// 256-thread workgroups, TWO per CU (79 KB of LDS each), ALL weights in registers: a wave owns one new h row (conv0: one 32-channel
// n block, 18 weight fragments = 72 VGPRs) and later one (output row, 32-channel n half) of the stride-2 conv (18 + 2 fragments = 80
// VGPRs).  D's weights are the same for every candidate, so the fragments are loaded once per workgroup lifetime and the MFMA
// loops read ONE LDS fragment (the pixels) per MFMA — the LDS-fed ceiling of conv_stream / conv_down was 1.5 reads per MFMA.
// (Round 4's first two versions were ONE 512-thread workgroup per CU with 4-row steps: every phase below is bound by a different
// unit — VALU, LDS, MFMA — and with a single workgroup the phases add up: 4.7 ms, then 4.3 ms after a VALU diet, = the two kernels
// it replaces.  Two independent workgroups per CU interleave their phases.)
//
// Phases of a step (4 workgroup barriers):
//   P1  image values (prefetched one step ahead) -> fromRGB AS AN MFMA (K = r, g, b, 1 of 16 slots; the weight / bias rows are one
//       register-resident fragment; masked pixels are all-zero operands, so the zero padding of conv0 costs two selects) -> F.
//       Round 4's first version did this in packed fp16 on the VALU: 340 of the step's 1240 VALU instructions per wave, in a kernel
//       that is bound by VALU issue (the two kernels it replaces spend 7900 wave-instructions on the same area, v1 spent 9900)
//   P2  skip-branch input: FIR (pad 1) + ::2 of F for output rows 2k+1, 2k+2 -> XS ring (MFMA B fragments of the skip conv)
//   P3  conv0: wave w = new h row 4k+2+w, 2 blocks x 18 MFMAs; bias + lrelu in packed fp16 exactly as conv_stream did it; h is zeroed
//       outside the image (the FIR's padding); the row goes through the wave's own row image and the HORIZONTAL FIR runs wave-locally
//       (LDS is in order per wave: no workgroup barrier), de-interleaved (even | odd blurred columns) into the 8-row ring HB
//   P4  vertical FIR over the ring -> operand image A of the stride-2 conv (5 rows; aliases F)
//   P5  stride-2 conv: wave (row r, n half): 18 MFMAs; bias + lrelu in the accumulators; + 2 skip MFMAs (the skip rows carry the
//       merge's 1/sqrt2, the activation's sqrt2 cancels against it); transposition through the wave's row image; 16-byte stores.
// Index-level CPU emulation of the whole scheme (patch / ring / priming / masks / fragment addresses): tests/emu_ops.py dblock0
// (tests/test_host.py::test_dblock0_index_emulation).
#include "common.h"
#include "kernels.h"
#include <stdio.h>
#include <stdlib.h>

namespace {
constexpr int NW = 4, NTHR = 64 * NW;                 // waves = new h rows per step
constexpr int TW = 29, XW = 2 * TW;                    // output columns per tile, h / x columns a tile advances by (round 6: 30 -> 29, see NFB)
constexpr int FP = 66, FR = NW + 2, FC = 64;          // patch: 6 rows x 64 columns at a pitch of 66 (the swizzle key is the column only: any pitch works)
constexpr int RING = 8, AR = 5, XSR = 3;              // h window rows (4 carried + 4 new), operand rows, skip-input ring rows
constexpr int F_BYTES = FR * FP * 64;                 // 25344: fromRGB patch; the operand image A (5 x 4096) aliases it
constexpr int ROWB = 64 * 64;                         // one 64-slot row of 64-byte pixels
constexpr int OFF_RT = F_BYTES;                       // per-wave row image (4 x 4096)
constexpr int OFF_HB = OFF_RT + NW * ROWB;            // ring of 8 horizontally blurred, de-interleaved h rows
constexpr int OFF_XS = OFF_HB + RING * ROWB;          // skip-branch input ring [3 rows][32 px][32 ch]
constexpr int OFF_C = OFF_XS + XSR * 32 * 64;         // bias0 [32] f32, bias1 [64] f32
constexpr int LDS_BYTES = OFF_C + 32 * 4 + 64 * 4;    // 81024 -> two workgroups per CU
constexpr int NFB [[maybe_unused]] = FR * FC / 32;                     // 12 blocks of 32 patch pixels: three per wave (block i belongs to wave i % 4).  With 30-column tiles
// the h window was 64 columns wide and the patch 66: a thirteenth block of 12 pixels, wave 0's fourth, kept the other three waves at the barrier
// behind P1 for a quarter of the phase.  29-column tiles cover 512 columns with the same 18 tiles; the window needs 62 h columns (the MFMA
// blocks still compute 64: columns 62 / 63 read patch columns 64 / 65 that nobody writes — finite or not, a pixel's lane never meets another
// pixel's, and the blurred columns 59 / 60 they reach are neither written to the ring nor read by a stored output).
static_assert(FR * FC == 32 * 3 * NW, "three full patch blocks per wave");
static_assert(AR * ROWB <= F_BYTES, "operand image aliases the patch");
static_assert(2 * ((LDS_BYTES + 511) / 512 * 512) <= 160 * 1024, "two workgroups per CU");

// patch image: pixel (pr, pc) at row pr * FP + pc, 16-byte chunk XOR-swizzled by the COLUMN only (conv_stream.hip's layout)
__device__ __forceinline__ int swa(int pr, int pc, int chunk) { return ((pr * FP + pc) << 6) + ((chunk ^ ((pc >> 2) & 3)) << 4); }
// dense 64-byte rows, chunk XOR-swizzled by the row / slot (conflict-free 32-lane fragment walks)
__device__ __forceinline__ int swz(int row, int chunk) { return (row << 6) + ((chunk ^ ((row >> 2) & 3)) << 4); }
// row image for the horizontal FIR: column rotated inside its aligned group of 4 (conv_down.hip's vaddr: stride-4 sliding-window
// reads and stride-1 writes both conflict-free)
__device__ __forceinline__ int vrot(int col, int cg) { return (((col & ~3) | ((col + (col >> 2)) & 3)) << 6) + (cg << 4); }
__device__ __forceinline__ h8 fir4(h8 a, h8 b, h8 c, h8 d) {   // [1,3,3,1]/8, packed fp16
    return (a + d) * (half_t)0.125f + (b + c) * (half_t)0.375f;
}
__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+v"(v)); return v; }
typedef unsigned u2x __attribute__((ext_vector_type(2)));
typedef unsigned u4x __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
}  // namespace

struct D0Params {
    const float* rgb_y;   // [B][3][R][R] skip image
    const float* rgb_w;   // [32][3] fromRGB weights (runtime coefficient applied)
    const float* rgb_b;   // [32]
    const half_t* w0;     // [9][32][32]
    const float* b0;      // [32]
    const half_t* w1;     // [9][64][32]
    const half_t* ws;     // [64][32]
    const float* b1;      // [64]
    half_t* y;            // [B][R/2][R/2][64], or chunk-planar [B][8][R/2][R/2][8] (common.h x_planar8: the consumer is conv_wreg)
    int B, R;
    int y_planar8;
};

__global__ __launch_bounds__(NTHR, 2) void dblock0_kernel(D0Params p, int tiles_x, int tiles_y, int n_steps, int per_block) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Cb0 = (float*)(smem + OFF_C);
    float* Cb1 = Cb0 + 32;
    const int R = p.R, Ro = R >> 1;
    const int first = blockIdx.x * per_block;
    const int last = min(first + per_block, n_steps);
    if (first >= last) return;
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    // ---- resident constants (LDS) and weight fragments (registers) -----------------------------------------------------------------
    h8 W0f[9][2], W1f[9][2], Wsf[2], Wrgb;
    {
        const int t = threadIdx.x;
        if (t < 32) Cb0[t] = p.b0[t];
        if (t < 64) Cb1[t] = p.b1[t];
        {   // fromRGB as an MFMA: A row n = (w[n][r], w[n][g], w[n][b], bias[n]) * sqrt2 in k slots 0 .. 3 (lane half 0), zeros elsewhere
            const int n = t & 31;
            Wrgb = zero;
            if (((t >> 5) & 1) == 0) {
                Wrgb[0] = (half_t)(p.rgb_w[n * 3] * GLASS_SQRT2);
                Wrgb[1] = (half_t)(p.rgb_w[n * 3 + 1] * GLASS_SQRT2);
                Wrgb[2] = (half_t)(p.rgb_w[n * 3 + 2] * GLASS_SQRT2);
                Wrgb[3] = (half_t)(p.rgb_b[n] * GLASS_SQRT2);
            }
        }
        // lane (n = lr, k half kh) holds W[tap][n][kk * 16 + kh * 8 .. + 7]: the A operand of mfma32 (common.h)
        const int lr = t & 31, kh = (t >> 5) & 1, nh = (t >> 6) & 1;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                W0f[tap][kk] = *(const h8*)(p.w0 + ((long long)tap * 32 + lr) * 32 + kk * 16 + kh * 8);
                W1f[tap][kk] = *(const h8*)(p.w1 + ((long long)tap * 64 + nh * 32 + lr) * 32 + kk * 16 + kh * 8);
            }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            // (lrelu(a + b1) * sqrt2 + skip) / sqrt2 = lrelu(a + b1) + skip / sqrt2: the skip rows carry the 1/sqrt2 (conv_down.hip)
            const h8 w = *(const h8*)(p.ws + ((long long)nh * 32 + lr) * 32 + kk * 16 + kh * 8);
#pragma unroll
            for (int q = 0; q < 8; ++q) Wsf[kk][q] = (half_t)((float)w[q] * 0.70710678118654752440f);
        }
    }

    // ---- lane-constant LDS offsets, computed ONCE and kept opaque (left to the compiler they were rebuilt in every step: ~250 of the first
    // version's 1240 VALU instructions per wave and step were address arithmetic; row / block / tap-row steps are immediate offsets) ------
    int fb[3][2], sb[3][2], rtw, p4off;      // (the once-per-step addresses — P2, horizontal FIR, ring and transposition
    // writes — are rebuilt per step: keeping them too left ONE fragment register for the MFMA loops, every MFMA behind its own LDS round trip)
    {
        const int t = threadIdx.x, lr = t & 31, kh = (t >> 5) & 1, lane = t & 63, wave = t >> 6;
        const int r = wave >> 1, nh = wave & 1;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                fb[kx][kk] = opaque(swa(wave, lr + kx, kk * 2 + kh));                                            // P3: + ky * FP * 64 + blk * 2048
                sb[kx][kk] = opaque(2 * r * ROWB + swz((kx == 1 ? 31 : (kx >> 1)) + lr, kk * 2 + kh));            // P5: + ky * ROWB
            }
        (void)lane; (void)nh;
        rtw = opaque(OFF_RT + wave * ROWB + vrot(lr, 0) + kh * 8);                                                // conv0 row image: + g * 16 + blk * 2048
        p4off = opaque(swz(min(t, 239) >> 2, t & 3));
    }

    // ---- the walk: steps (b, tx, k), k fastest (down a tile column); a priming item (k - 1, no output) opens every range / column ---
    struct Item { int b, tx, k, prime; };
    const int tpi = tiles_x * tiles_y;
    int it = first;
    int cb = uni(first / tpi);
    int ctx, ck;
    {
        const int rem = first - cb * tpi;
        ctx = uni(rem / tiles_y);
        ck = uni(rem - ctx * tiles_y);
    }
    bool need_prime = true;
    auto next_item = [&]() {
        Item r;
        if (need_prime) {
            r.b = cb; r.tx = ctx; r.k = ck - 1; r.prime = 1;
            need_prime = false;
            return r;
        }
        r.b = cb; r.tx = ctx; r.k = ck; r.prime = 0;
        ++it;
        if (++ck == tiles_y) {
            ck = 0;
            need_prime = true;
            if (++ctx == tiles_x) { ctx = 0; ++cb; }
        }
        return r;
    };

    // image values of an item's patch: patch pixel 32 * (wave + 4u) + lr for u = 0 .. 3 (both lane halves fetch the same pixel: the
    // MFMA operand of a pixel lives in lane half 0); unconditional loads at clamped coordinates (the zero padding is a mask applied
    // when the operand is built)
    float yv[3][3];
    auto load_image = [&](const Item& c) {
        const int t = opaque(threadIdx.x);
        const int y0 = 4 * c.k + 1, x0 = XW * c.tx - 3;
        const long long hw = (long long)R * R;
        const float* yb = p.rgb_y + (long long)c.b * 3 * hw;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int px = 32 * ((t >> 6) + NW * u) + (t & 31);
            const int fr = px / FC, fc = px - fr * FC;
            const int iy = min(max(y0 + fr, 0), R - 1), ix = min(max(x0 + fc, 0), R - 1);
            const int off = iy * R + ix;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) yv[u][ch] = yb[ch * hw + off];
        }
    };

    auto step = [&](const Item& c, const Item& nx) {
        const int b = c.b, tx = c.tx, k = c.k;
        const int y0 = 4 * k + 1, x0 = XW * tx - 3;
        __syncthreads();       // B0: every wave is done with the previous item's operand image / patch / XS
        // ---- P1: fromRGB of this wave's patch blocks -> F: one MFMA per 32 pixels, lrelu in packed fp16, four 8-byte stores per lane -------
        {
            const int t = opaque(threadIdx.x), lr1 = t & 31, kh1 = (t >> 5) & 1, wv = uni(t >> 6);
            f16x zacc;
#pragma unroll
            for (int q = 0; q < 16; ++q) zacc[q] = 0.f;
            // the three blocks of a wave side by side (no early exit between them: as a loop with a uniform break every block was its own
            // basic block and ran its whole chain — operand, MFMA latency, conversion, activation, stores — before the next one started)
            f16x z[3];
            int fr3[3], fc3[3];
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const int px = 32 * (wv + NW * u) + lr1;
                const int fr = px / FC, fc = px - fr * FC;
                fr3[u] = fr; fc3[u] = fc;
                const int iy = y0 + fr, ix = x0 + fc;
                const bool ok = kh1 == 0 && (unsigned)iy < (unsigned)R && (unsigned)ix < (unsigned)R;
                h8 cf = zero;                                                          // (r, g, b, 1, 0, 0, 0, 0) or all zero
                // biggan_denorm(biggan_norm(y)) = clamp((y + 1) / 2, 0, 1) * 2 - 1 = clamp(y, -1, 1) (utils.py:14-21): ONE v_med3_f32 per value
                // where the literal form took five VALU instructions (r05; the two differ by fp32 rounding of (y + 1), <= 6e-8, before
                // the value is rounded to its fp16 MFMA operand anyway)
                cf[0] = (half_t)__builtin_amdgcn_fmed3f(yv[u][0], -1.f, 1.f);
                cf[1] = (half_t)__builtin_amdgcn_fmed3f(yv[u][1], -1.f, 1.f);
                cf[2] = (half_t)__builtin_amdgcn_fmed3f(yv[u][2], -1.f, 1.f);
                cf[3] = (half_t)1.f;
                if (!ok) cf = zero;
                z[u] = mfma32(Wrgb, cf, zacc);                                         // z[4g + q] = x[channel 8g + 4kh + q] of pixel lr, fp32
            }
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                char* dst = smem + ((fr3[u] * FP + fc3[u]) << 6) + kh1 * 8;
                const int key = (fc3[u] >> 2) & 3;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    h4 v;
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = (half_t)z[u][g * 4 + q];
                    v = __builtin_elementwise_max(v, v * (half_t)0.2f);
                    *(h4*)(dst + ((g ^ key) << 4)) = v;
                }
            }
        }
        __syncthreads();       // B1: patch complete
        const int tm = opaque(threadIdx.x), lr = tm & 31, kh = (tm >> 5) & 1, lane = tm & 63, wave = uni(tm >> 6);
        // ---- P2: skip-branch input: FIR 4x4 (pad 1) + ::2 of the fromRGB map, output row 2k + 1 + r (one row ahead of P5).  The wave's 32
        // pixels x 2 chunks are dealt (pixel = lane / 2, chunk = nh * 2 + lane % 2): a stride-2 pixel walk touches every other 64-byte
        // window, so sixteen consecutive lanes must bring two chunks each to cover all sixteen 16-byte bank groups (the image goes
        // through LDS to the skip MFMAs anyway, so this phase's lane mapping is free) ----
        {
            const int r = wave >> 1, nh = wave & 1, ch = nh * 2 + (lane & 1), lrx = lane >> 1;
            h8 hr[4];
            const int fc0 = min(2 * lrx + 2, FC - 4);                                  // (lanes past the tile's 29 columns: any columns that exist)
            int xa[4];
#pragma unroll
            for (int jx = 0; jx < 4; ++jx) xa[jx] = swa(2 * r, fc0 + jx, ch);
#pragma unroll
            for (int half = 0; half < 2; ++half) {                                     // eight reads in flight, then their two FIRs
                h8 a[2][4];
#pragma unroll
                for (int j2 = 0; j2 < 2; ++j2)
#pragma unroll
                    for (int jx = 0; jx < 4; ++jx) a[j2][jx] = *(const h8*)(smem + xa[jx] + (2 * half + j2) * (FP * 64));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j2 = 0; j2 < 2; ++j2) hr[2 * half + j2] = fir4(a[j2][0], a[j2][1], a[j2][2], a[j2][3]);
            }
            const int xslot = uni((2 * k + 1 + r + 3) % 3);                             // ring slot of output row o: o mod 3 (k >= -1)
            *(h8*)(smem + OFF_XS + xslot * 2048 + swz(lrx, ch)) = fir4(hr[0], hr[1], hr[2], hr[3]);
        }
        // ---- P3: conv0 of new h row 8k + 2 + wave -> row image -> horizontal FIR -> ring -------------------------------------------------
        {
            const int yh = 4 * k + 2 + wave;                                           // uniform per wave
            char* ring = smem + OFF_HB + ((yh + 2 + RING) & (RING - 1)) * ROWB;        // slot of h row y: (y + 2) mod 8
            const int jj = lane >> 2, cgl = lane & 3;
            int hw4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) hw4[i] = swz(((i & 1) ? 31 : 0) + 2 * jj + (i >> 1), cgl);        // blurred column 4jj + i: even | odd slots
            if ((unsigned)yh >= (unsigned)R) {                                         // outside the image: the FIR's zero padding
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (4 * jj + i <= XW) *(h8*)(ring + hw4[i]) = zero;
            } else {
                // the accumulators START at the bias (lane (px, kh) owns channels 8g + 4kh + q): the first version read the bias quads in the
                // epilogue, eight LDS round trips in a row with nothing to overlap them (2400 of the step's 12 900 clocks)
                f16x acc[2];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f4 bb = *(const f4*)(Cb0 + 8 * g + 4 * kh);
#pragma unroll
                    for (int q = 0; q < 4; ++q) { acc[0][g * 4 + q] = bb[q]; acc[1][g * 4 + q] = bb[q]; }
                }
                // Software-pipelined by hand: the four fragments of tap t + 1 are requested before the four MFMAs of tap t issue.  Left to
                // the scheduler (at ~250 live VGPRs it minimises pressure) every MFMA sat behind its own LDS round trip: ds_read,
                // s_waitcnt lgkmcnt(0), v_mfma, 36 times per step (r04 v3 ISA) — with two waves per SIMD nothing hides that.
                h8 xq[2][4];
                auto rd4 = [&](int tap, h8 (&d)[4]) {
                    const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                        for (int blk = 0; blk < 2; ++blk) d[kk * 2 + blk] = *(const h8*)(smem + fb[kx][kk] + ky * (FP * 64) + blk * 2048);
                };
                rd4(0, xq[0]);
                __builtin_amdgcn_s_setprio(1);
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    if (tap + 1 < 9) rd4(tap + 1, xq[(tap + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                        for (int blk = 0; blk < 2; ++blk) acc[blk] = mfma32(W0f[tap][kk], xq[tap & 1][kk * 2 + blk], acc[blk]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                __builtin_amdgcn_s_setprio(0);
                // bias + lrelu * sqrt2 exactly as conv_stream<fromrgb> formed h: fp32 sum -> fp16 -> max(v k1, v k2) in packed fp16
                // (r05: moving the sqrt2 gain into conv1's weight fragments saves 16 of the step's ~880 VALU instructions, changes no
                // timing — the kernel is not bound by VALU issue, DESIGN section 5 — and re-rounds the weights: D error 5.4e-4 -> 8.1e-4; not kept)
                const half_t k1 = (half_t)GLASS_SQRT2, k2 = (half_t)(0.2f * GLASS_SQRT2);
                const bool edge = tx == 0 || XW * tx + 62 > R;                          // uniform: only the first / last tile column masks
                auto epi0 = [&](bool masked) {
#pragma unroll
                    for (int blk = 0; blk < 2; ++blk) {
                        const bool colok = !masked || (unsigned)(XW * tx - 2 + blk * 32 + lr) < (unsigned)R;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            h4 v;
#pragma unroll
                            for (int q = 0; q < 4; ++q) v[q] = (half_t)acc[blk][g * 4 + q];
                            h4 hq = __builtin_elementwise_max(v * k1, v * k2);
                            if (masked && !colok) hq = h4{0, 0, 0, 0};
                            *(h4*)(smem + rtw + ((g ^ ((lr >> 2) & 3)) << 4) + blk * 2048) = hq;    // chunk XOR-swizzled by the column group: the
                            // 32 lanes of a half-wave write 8 bytes each at the SAME offset of 32 different pixels — 8-way conflicts unswizzled
                        }
                    }
                };
                if (edge) epi0(true);
                else epi0(false);
                __builtin_amdgcn_wave_barrier();
                h8 v[7];
#pragma unroll
                for (int q = 0; q < 7; ++q) {
                    const int colq = min(4 * jj + q, 63);
                    v[q] = *(const h8*)(smem + OFF_RT + wave * ROWB + vrot(colq, cgl ^ ((colq >> 2) & 3)));
                    if (q >= 4 && jj == 15) v[q] = zero;                               // window columns 64 .. 66 do not exist
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (4 * jj + i <= XW) *(h8*)(ring + hw4[i]) = fir4(v[i], v[i + 1], v[i + 2], v[i + 3]);
                __builtin_amdgcn_wave_barrier();
            }
        }
        load_image(nx);        // the next item's image values travel during P4 / P5 (issued here, not before conv0: twelve fewer live
                               // registers in the step's tightest loop)
        if (c.prime) return;
        __syncthreads();       // B2: ring complete; every wave is done reading F
        // ---- P4: vertical FIR over the ring -> operand image A (rows 0 .. 4 = blurred rows 4k .. 4k + 4) -----------------------------------
        {
            const int t = opaque(threadIdx.x);
            if (t < 240) {                                           // ring slots 0 .. 59 (even columns 0 .. 58 | 30 unused | odd columns 1 .. 57)
                const int base = uni((4 * k + RING) & (RING - 1));                      // ring slot of window row 0 (h row 4k - 2)
                h8 v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = *(const h8*)(smem + OFF_HB + ((base + i) & (RING - 1)) * ROWB + p4off);
#pragma unroll
                for (int j = 0; j < AR; ++j) *(h8*)(smem + j * ROWB + p4off) = fir4(v[j], v[j + 1], v[j + 2], v[j + 3]);
            }
        }
        __syncthreads();       // B3: operand image complete
        // ---- P5: stride-2 conv + skip, wave = (output row 2k + r, n half nh) ----------------------------------------------------------------
        {
            const int r = wave >> 1, nh = wave & 1;
            f16x acc;                                                               // starts at the bias (see conv0)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f4 bb = *(const f4*)(Cb1 + nh * 32 + 8 * g + 4 * kh);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[g * 4 + q] = bb[q];
            }
            // (pipelined like conv0's loop: the fragments of taps t + 1 and t + 2 are in flight while tap t's two MFMAs issue)
            h8 xq[3][2];
            auto rd2 = [&](int tap, h8 (&d)[2]) {
                const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) d[kk] = *(const h8*)(smem + sb[kx][kk] + ky * ROWB);
            };
            rd2(0, xq[0]);
            rd2(1, xq[1]);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                if (tap + 2 < 9) rd2(tap + 2, xq[(tap + 2) % 3]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) acc = mfma32(W1f[tap][kk], xq[tap % 3][kk], acc);
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_s_setprio(0);
            // lrelu; its sqrt2 gain cancels against the merge's 1/sqrt2.  As f4 arithmetic: v_pk_mul_f32 + v_max_f32 (24 instructions; the
            // scalar fmaxf form compiled to 48: a canonicalising v_max per operand)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f4 v4 = {acc[g * 4], acc[g * 4 + 1], acc[g * 4 + 2], acc[g * 4 + 3]};
                v4 = __builtin_elementwise_max(v4, v4 * 0.2f);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[g * 4 + q] = v4[q];
            }
            const int xslot = uni((2 * k + r) % 3);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                acc = mfma32(Wsf[kk], *(const h8*)(smem + OFF_XS + xslot * 2048 + swz(lr, kk * 2 + kh)), acc);
            const int orow = 2 * k + r;
            if (p.y_planar8) {
                // chunk-planar output (four planes of 8 channels per n half): lane (px, kh) holds channels 4kh .. 4kh + 3 of planes g = 0 .. 3 —
                // v_permlane32_swap hands a lane pair one whole plane each (lower lane: plane 2 pr, upper lane: plane 2 pr + 1) and the 16-byte
                // stores leave from the registers: 32 lanes x 16 contiguous bytes per plane, no trip through the row image (round 6)
                const long long plane = (long long)Ro * Ro * 8;
                half_t* ypx = p.y + ((((long long)b * 8 + nh * 4 + kh) * Ro + orow) * Ro + TW * tx + lr) * 8;
                const bool on = lr < TW && TW * tx + lr < Ro && orow < Ro;
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    u2x lo, hi;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        h2 a = {(half_t)acc[(2 * pr) * 4 + 2 * e], (half_t)acc[(2 * pr) * 4 + 2 * e + 1]};
                        h2 c = {(half_t)acc[(2 * pr + 1) * 4 + 2 * e], (half_t)acc[(2 * pr + 1) * 4 + 2 * e + 1]};
                        const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, c), false, false);
                        lo[e] = sw[0];
                        hi[e] = sw[1];
                    }
                    const u4x d = {lo[0], lo[1], hi[0], hi[1]};
                    if (on) *(u4x*)(ypx + 2 * pr * plane) = d;
                }
            } else {
            // transposition through the wave's row image (32 px x 64 B), then 16-byte stores in row order
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                h4 o;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = (half_t)acc[g * 4 + q];
                *(h4*)(smem + OFF_RT + wave * ROWB + swz(lr, g) + kh * 8) = o;
            }
            __builtin_amdgcn_wave_barrier();
            half_t* yrow = p.y + (((long long)b * Ro + orow) * Ro + TW * tx) * 64 + nh * 32;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int v = lane + 64 * u, pix = v >> 2, chv = v & 3;
                const h8 d = *(const h8*)(smem + OFF_RT + wave * ROWB + swz(pix, chv));
                if (pix < TW && TW * tx + pix < Ro && orow < Ro) *(h8*)(yrow + pix * 64 + chv * 8) = d;
            }
            __builtin_amdgcn_wave_barrier();
            }
        }
    };

    __syncthreads();           // constants staged
    Item cur = next_item();
    load_image(cur);
    for (;;) {
        const bool more = it < last;
        const Item nxt = more ? next_item() : cur;
        step(cur, nxt);
        if (!more) break;
        cur = nxt;
    }
}

bool dblock0_supported(int R, int Cin, int Cout) {
    return glass_lds_fits(LDS_BYTES) && R % 4 == 0 && R >= 16 && Cin == 32 && Cout == 64 && 3LL * R * R < (1LL << 31);
}

// Returns the kernel symbol, or nullptr when the block does not qualify (caller runs the two-kernel form).
const char* launch_dblock0(const float* rgb_y, const float* rgb_w, const float* rgb_b, const half_t* w0, const float* b0, const half_t* w1,
                           const half_t* ws, const float* b1, half_t* y, int B, int R, int Cin, int Cout, hipStream_t st, int y_planar8) {
    if (!dblock0_supported(R, Cin, Cout)) return nullptr;
    D0Params p;
    p.rgb_y = rgb_y; p.rgb_w = rgb_w; p.rgb_b = rgb_b; p.w0 = w0; p.b0 = b0; p.w1 = w1; p.ws = ws; p.b1 = b1; p.y = y; p.B = B; p.R = R;
    p.y_planar8 = y_planar8;
    const int Ro = R / 2, tiles_x = (Ro + TW - 1) / TW, tiles_y = R / 4;
    const long long n_steps = (long long)B * tiles_x * tiles_y;
    if (n_steps >= (1LL << 30)) return nullptr;
    static DevOnce once;
    once.run([&] { (void)hipFuncSetAttribute((const void*)dblock0_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES); });
    const int slots = 2 * glass_cu_count();       // two 256-thread workgroups per CU (79 KB of LDS each)
    const int per_block = (int)((n_steps + slots - 1) / slots);
    const int grid = (int)((n_steps + per_block - 1) / per_block);
    hipLaunchKernelGGL(dblock0_kernel, dim3(grid), dim3(NTHR), LDS_BYTES, st, p, tiles_x, tiles_y, (int)n_steps, per_block);
    return "dblock0_kernel";
}
