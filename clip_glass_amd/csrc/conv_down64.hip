// conv_down64.hip — the second half of the discriminator's 64 -> 128 block (the 512^2 block of ffhq) in ONE kernel (gfx950):
//     h  [B][R][R][64]     -> FIR 4x4 (pad 2) -> conv3x3 stride 2 (64 -> 128) + bias + lrelu*sqrt2 \
//     xs [B][R/2][R/2][64] -> conv1x1 (64 -> 128, no bias / activation)                             +-> (a + b) / sqrt2
// (stylegan2/modules.py:1204-1254 ConvDownLayer, 1587-1601 DiscriminatorConvBlock.forward) — conv_down.hip's semantics at twice
// the channels.  As blur_kernel + conv_s2 the block moved ~8 GB per 64-candidate population for maps that are 2.4 GB in and
// 1.1 GB out: the blurred map was written once and read 1.13 times.  Here it never leaves the CU.
//
// What makes the consumer-side FIR fit (DESIGN.md §5 round 5 item 4 (d) failed on LDS): the weights are NOT in LDS.  A wave owns
// one 32-channel output block and keeps its 9 x 4 main + 4 skip MFMA A fragments (160 VGPRs) for the kernel's lifetime, as
// conv_wreg / dblock0 P5 do; LDS holds activations only (120.5 KB).
//
// Geometry (one persistent 512-thread workgroup per CU, 8 waves at 256 registers):
//   * a STEP is 2 output rows x 29 output columns; a workgroup walks a contiguous range of steps DOWN a tile column
//     (sample, tile column, row pair).  29 columns need 2 * 29 + 4 = 62 raw columns: thread (window column 0..63, 8-channel
//     group 0..7) covers them with no edge-column side path (columns 62, 63 are loaded clamped and never used);
//   * a step needs blurred rows 4s .. 4s + 4.  Row 4s is the previous step's last row and stays in the operand ring; the four
//     new ones need raw rows 4s - 1 .. 4s + 5, of which the thread CARRIES 4s - 1 .. 4s + 1 in registers and loads 4s + 2 .. 4s + 5:
//     every raw row crosses the fabric once per tile column (62 / 58 horizontal halo, no vertical one);
//   * the 4 window loads + 1 skip-input load of a step are requested TWO steps ahead into two named register sets (unconditional,
//     clamped coordinates; the zero padding is a mask applied at use on border steps only);
//   * FIR ORDER: VERTICAL first (registers, packed fp16, on the thread's window column), result to LDS; then HORIZONTAL (lane
//     (4 output columns, channel group) slides over 7 columns of one row) into the operand ring, whose rows hold the even
//     blurred columns in slots 0..29 and the odd ones in slots 32..60 (the stride-2 fragment walk is then a unit-stride one),
//     16-byte chunks XOR-swizzled by the slot.  Both passes are fma(b + c, 3/8, (a + d) / 8) written out (not left to -ffp-contract);
//   * the ring has 8 row slots, blurred row j in slot j & 7: step s writes slots of rows 4s + 1 .. 4s + 4 and reads 4s .. 4s + 4;
//   * MFMA: wave (output row r = wave / 4, n block = wave % 4) issues 9 taps x 4 k steps + 4 skip k steps of
//     v_mfma_f32_32x32x16_f16 per step, one ds_read_b128 pixel fragment each (pixels 29..31 of the 32 are computed and dropped);
//     the skip input of the step travels with the window set and sits in a small LDS image;
//   * epilogue: bias + lrelu in the accumulators (the sqrt2 gain cancels against the merge's 1/sqrt2, which the skip weights carry),
//     skip MFMAs on top, transposition through LDS, and the workgroup stores whole 256-byte pixels in row order;
//   * PRIMING: a range that starts at step s0 of a column first runs step s0 - 1 with its stores masked: that step's four loads are
//     exactly the raw rows of blurred row 4 s0, the one row step s0 takes from the ring, and they become the carry.  Its other three
//     blurred rows are built from a stale carry and land in ring slots that step s0 does not read.
// Four workgroup barriers per step: B0 (previous step's operand / skip images are read), B1 (vertical image complete),
// B2 (operand rows complete), B3 (output image complete).  No LDS-DMA, no hand-placed vmcnt.
// The loop has no exit between its two steps (conv_down.hip's header says why); an odd count is padded with a masked step.
#include "common.h"
#include "kernels.h"

namespace {
constexpr int TW = 29, CIN = 64, COUT = 128;
constexpr int ROWB = 64 * 128;               // one image row: 64 column slots x 64 channels
constexpr int V_BYTES = 4 * ROWB;            // vertical-pass image: 4 new blurred rows x 64 window columns
constexpr int A_BYTES = 8 * ROWB;            // operand ring: 8 row slots
constexpr int XS_BYTES = 2 * 32 * 128;       // skip input: 2 rows x 32 pixels
constexpr int O_BYTES = 2 * 32 * 256;        // output image: 2 rows x 32 pixels x 128 channels
constexpr int OFF_A = V_BYTES, OFF_XS = OFF_A + A_BYTES, OFF_O = OFF_XS + XS_BYTES, OFF_C = OFF_O + O_BYTES;
constexpr int LDS_BYTES = OFF_C + COUT * 4;  // 123392

// vertical-pass image: columns swapped in pairs inside every second group of four (the sliding-window reads of two neighbouring
// lanes, 4 columns = 512 bytes apart, then fall into different halves of the 256-byte bank row)
__device__ __forceinline__ int vaddr(int row, int col, int cg) { return row * ROWB + ((col ^ ((col >> 2) & 1)) << 7) + (cg << 4); }
// operand ring / skip image: 16-byte chunk XOR-swizzled by the slot pair (16 consecutive slots x one chunk = 16 distinct bank groups)
__device__ __forceinline__ int aaddr(int rslot, int slot, int lc) { return rslot * ROWB + (slot << 7) + ((lc ^ ((slot >> 1) & 7)) << 4); }
// output image: 256-byte pixels, chunk XOR-swizzled by the pixel
__device__ __forceinline__ int oaddr(int row, int px, int c16) { return row * (32 * 256) + (px << 8) + ((c16 ^ (px & 15)) << 4); }
__device__ __forceinline__ h8 fir4(h8 a, h8 b, h8 c, h8 d) {   // [1,3,3,1]/8, packed fp16, explicit operations
    const half_t q = (half_t)0.125f, t = (half_t)0.375f;
    const h8 k125 = {q, q, q, q, q, q, q, q}, k375 = {t, t, t, t, t, t, t, t};
    return __builtin_elementwise_fma(b + c, k375, (a + d) * k125);
}
__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
struct RSet { h8 a[4]; h8 x; int b, tx, s, valid; };   // 4 new window rows, skip-input vector, step (SGPRs)
}  // namespace

struct Down64Params {
    const half_t* h;    // [B][R][R][64]       first conv's output, pixel-major
    const half_t* xs;   // [B][R/2][R/2][64]   block input after FIR (pad 1) + ::2
    const half_t* w1;   // [9][128][64]
    const half_t* ws;   // [128][64]
    const float* b1;    // [128]
    half_t* y;          // [B][R/2][R/2][128]
    int B, R;
};

__global__ __launch_bounds__(512, 1) void conv_down64_kernel(Down64Params p, int tiles_x, int SY, int n_steps, int per_block) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Vs = smem;
    char* As = smem + OFF_A;
    char* Xs = smem + OFF_XS;
    char* Os = smem + OFF_O;
    float* Cb = (float*)(smem + OFF_C);
    const int R = p.R, Ro = R >> 1;
    const int first = blockIdx.x * per_block;
    const int last = min(first + per_block, n_steps);
    if (first >= last) return;
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    // ---- the walk: step index -> (sample, tile column, row pair), row pair fastest; a priming step ahead of every column segment ----
    int nx_left = last - first, nx_prime = 1, nx_b, nx_tx, nx_s;
    {
        const int per_img = tiles_x * SY;
        nx_b = uni(first / per_img);
        const int rem = first - nx_b * per_img;
        nx_tx = uni(rem / SY);
        nx_s = uni(rem - nx_tx * SY);
    }
    const int total = nx_left + 1 + (nx_s + nx_left - 1) / SY;     // real steps + one priming step per column segment

    auto issue = [&](RSet& Rg) {
        Rg.b = nx_b; Rg.tx = nx_tx;
        if (nx_prime) {
            Rg.s = nx_s - 1; Rg.valid = 0; nx_prime = 0;
        } else {
            Rg.s = nx_s; Rg.valid = nx_left > 0;
            if (nx_left > 1) {         // advance (uniform); after the last real step the walk stays where it is (masked steps re-read it)
                if (++nx_s == SY) { nx_s = 0; nx_prime = 1; if (++nx_tx == tiles_x) { nx_tx = 0; ++nx_b; } }
            }
            if (nx_left > 0) --nx_left;
        }
        const int t = opaque(threadIdx.x), cg = t & 7, cs = t >> 3;
        const half_t* img = p.h + (long long)Rg.b * R * R * CIN;                      // uniform
        const int xo = min(max(2 * TW * Rg.tx - 2 + cs, 0), R - 1) * CIN + cg * 8;    // R * R * 64 < 2^31: 32-bit element offsets
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int iy = min(max(4 * Rg.s + 2 + k, 0), R - 1);                      // uniform
            Rg.a[k] = *(const h8*)(img + iy * (R * CIN) + xo);
        }
        // skip input: thread (row, pixel, chunk) of the step's 2 x 29 x 8 vectors
        const int v = min(t, 2 * TW * 8 - 1), row = v >= TW * 8, rem = v - row * (TW * 8);
        const int yy = min(max(2 * Rg.s + row, 0), Ro - 1), xx = min(TW * Rg.tx + (rem >> 3), Ro - 1);
        Rg.x = *(const h8*)(p.xs + (((long long)Rg.b * Ro + yy) * Ro + xx) * CIN + (rem & 7) * 8);
    };

    // ---- resident weights: this wave's n block as MFMA A fragments in registers; bias in LDS ------------------------------------
    h8 Wm[9][4], Wk[4];
    {
        const int t = threadIdx.x, lr = t & 31, kh = (t >> 5) & 1, nb = (t >> 6) & 3;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) Wm[tap][kk] = *(const h8*)(p.w1 + ((tap * COUT + nb * 32 + lr) * CIN + kk * 16 + kh * 8));
        // (lrelu(a + b1) * sqrt2 + skip) / sqrt2 = lrelu(a + b1) + skip / sqrt2: the skip weights carry the 1/sqrt2
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const h8 wv = *(const h8*)(p.ws + ((nb * 32 + lr) * CIN + kk * 16 + kh * 8));
#pragma unroll
            for (int q = 0; q < 8; ++q) Wk[kk][q] = (half_t)((float)wv[q] * 0.70710678118654752440f);
        }
        if (t < COUT) Cb[t] = p.b1[t];
    }

    h8 c0 = zero, c1 = zero, c2 = zero;      // carried raw rows 4s - 1 .. 4s + 1 of this thread's window column

    auto step = [&](RSet& Rg) {
        const int b = Rg.b, tx = Rg.tx, s = Rg.s, valid = Rg.valid;
        const int ox = 2 * TW * tx - 2, oy = 4 * s + 2;     // raw coordinates of window column 0 / of the first new row
        __syncthreads();       // B0: every wave is done with the previous step's operand rows and skip image
        // ---- vertical FIR on this thread's window column -> LDS; skip vector -> LDS ---------------------------------------------
        {
            const int t = opaque(threadIdx.x), cg = t & 7, cs = t >> 3;
            const bool border = ox < 0 || ox + 64 > R || oy < 0 || oy + 4 > R;     // uniform: interior steps need no padding mask
            if (border) {
                const bool colok = (unsigned)(ox + cs) < (unsigned)R;
#pragma unroll
                for (int k = 0; k < 4; ++k) Rg.a[k] = (colok && (unsigned)(oy + k) < (unsigned)R) ? Rg.a[k] : zero;
            }
            *(h8*)(Vs + vaddr(0, cs, cg)) = fir4(c0, c1, c2, Rg.a[0]);
            *(h8*)(Vs + vaddr(1, cs, cg)) = fir4(c1, c2, Rg.a[0], Rg.a[1]);
            *(h8*)(Vs + vaddr(2, cs, cg)) = fir4(c2, Rg.a[0], Rg.a[1], Rg.a[2]);
            *(h8*)(Vs + vaddr(3, cs, cg)) = fir4(Rg.a[0], Rg.a[1], Rg.a[2], Rg.a[3]);
            c0 = Rg.a[1]; c1 = Rg.a[2]; c2 = Rg.a[3];
            if (t < 2 * TW * 8) {
                const int row = t >= TW * 8, rem = t - row * (TW * 8);
                *(h8*)(Xs + aaddr(0, row * 32 + (rem >> 3), rem & 7)) = Rg.x;
            }
        }
        issue(Rg);             // refill: two steps of loads stay in flight
        __syncthreads();       // B1: vertical-pass image complete
        // ---- horizontal FIR: wave (row, half), lane (4 blurred columns, channel group) -> operand ring -------------------------
        {
            const int t = opaque(threadIdx.x), lane = t & 63, wave = uni(t >> 6);
            const int row = wave >> 1, j = (wave & 1) * 8 + (lane >> 3), cg = lane & 7;
            if (j < 15) {          // blurred columns 4j .. 4j + 3 <= 59 (58 is the last one used)
                h8 v[7];
#pragma unroll
                for (int k = 0; k < 7; ++k) v[k] = *(const h8*)(Vs + vaddr(row, 4 * j + k, cg));
                const int rslot = (4 * s + 1 + row) & 7;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = 4 * j + i;
                    const int slot = (c & 1) ? 32 + (c >> 1) : (c >> 1);
                    *(h8*)(As + aaddr(rslot, slot, cg)) = fir4(v[i], v[i + 1], v[i + 2], v[i + 3]);
                }
            }
        }
        __syncthreads();       // B2: operand rows complete
        // ---- MFMA: 9 taps x 4 k16 steps; wave = (output row 2s + r, n block nb) ----------------------------------------------------
        const int tm = opaque(threadIdx.x), lr = tm & 31, kh = (tm >> 5) & 1, wave = uni(tm >> 6), r = wave >> 2, nb = wave & 3;
        f16x acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int rslot = (4 * s + 2 * r + ky) & 7;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const h8 xf = *(const h8*)(As + aaddr(rslot, (kx == 1 ? 32 : (kx >> 1)) + lr, kk * 2 + kh));
                    acc = mfma32(Wm[ky * 3 + kx][kk], xf, acc);
                    if (kk == 3 && (kx & 1) == (ky & 1)) __builtin_amdgcn_sched_barrier(0);   // at most two taps' fragments live (the weights own the registers)
                }
        }
        // ---- activation in the accumulators, then the skip branch on top ----------------------------------------------------------
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f4 bb = *(const f4*)(Cb + nb * 32 + 8 * g + 4 * kh);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float v = acc[g * 4 + q] + bb[q];
                acc[g * 4 + q] = fmaxf(v, 0.2f * v);        // lrelu; its sqrt2 gain cancels against the merge's 1/sqrt2
            }
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc = mfma32(Wk[kk], *(const h8*)(Xs + aaddr(0, r * 32 + lr, kk * 2 + kh)), acc);
        // ---- epilogue: lane = (pixel lr, channels nb * 32 + 8g + 4kh ..+3) -> output image -> 256-byte pixels in row order --------
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            h4 out;
#pragma unroll
            for (int q = 0; q < 4; ++q) out[q] = (half_t)acc[g * 4 + q];
            *(h4*)(Os + oaddr(r, lr, nb * 4 + g) + kh * 8) = out;
        }
        __syncthreads();       // B3: output image complete
        if (valid) {
            const int t = opaque(threadIdx.x);
            const int npx = min(TW, Ro - TW * tx);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int v = t + 512 * k;
                const int row = v >= TW * 16, rem = v - row * (TW * 16), px = rem >> 4, ch = rem & 15;
                if (v < 2 * TW * 16 && px < npx)
                    *(h8*)(p.y + (((long long)b * Ro + 2 * s + row) * Ro + TW * tx + px) * COUT + ch * 8) = *(const h8*)(Os + oaddr(row, px, ch));
            }
        }
    };

    RSet r0, r1;
    issue(r0);
    issue(r1);
    for (int it = 0; it < total; it += 2) {     // no exit between the two steps
        step(r0);
        step(r1);
    }
}

// Pure function of the layer (never of the launch size): the block runs on this kernel whatever the population is.
bool conv_down64_supported(int R, int Cin, int Cout) {
    return Cin == CIN && Cout == COUT && R >= 16 && R % 4 == 0 && (long long)R * R * Cin < (1LL << 31) && glass_lds_fits(LDS_BYTES);
}

const char* launch_conv_down64(const half_t* h, const half_t* xs, const half_t* w1, const half_t* ws, const float* b1, half_t* y,
                               int B, int R, int Cin, int Cout, hipStream_t st) {
    if (!conv_down64_supported(R, Cin, Cout)) return nullptr;
    Down64Params p;
    p.h = h; p.xs = xs; p.w1 = w1; p.ws = ws; p.b1 = b1; p.y = y; p.B = B; p.R = R;
    const int Ro = R / 2, tiles_x = (Ro + TW - 1) / TW, SY = Ro / 2;
    const long long steps = (long long)B * tiles_x * SY;
    if (steps >= (1LL << 30)) return nullptr;
    static DevOnce once;
    once.run([&] { (void)hipFuncSetAttribute((const void*)conv_down64_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES); });
    const int slots = glass_cu_count();
    const int per_block = (int)((steps + slots - 1) / slots);
    const int grid = (int)((steps + per_block - 1) / per_block);
    hipLaunchKernelGGL(conv_down64_kernel, dim3(grid), dim3(512), LDS_BYTES, st, p, tiles_x, SY, (int)steps, per_block);
    return "conv_down64_kernel";
}
