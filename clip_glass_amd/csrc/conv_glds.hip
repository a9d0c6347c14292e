// conv_glds.hip — 3x3 stride-1 convolution for the MFMA-bound mid-resolution layers (Cin >= 128, 128-wide n tiles),
// staged by LDS-DMA (`global_load_lds_dwordx4`) instead of registers.
//
// conv_tiled.hip sits at the VGPR cap (256) with a ONE-stage register prefetch: the loads of stage s+1 get the
// MFMA block of stage s (~0.64 us) to cover ~1-2 us of loaded L2/HBM latency, and every stage stalls.  A deeper
// register ring does not fit.  Here nothing is staged through registers:
//   * block = 512 threads (8 waves, 2 per SIMD), tile = 16 rows x 32 px x 128 channels (twice conv_tiled's pixels per
//     weight stage -> half the weight traffic per FLOP);
//   * weights: ring of THREE LDS slots (one (chunk, tap-row) stage each, 24 KB), filled two stages ahead;
//   * input patch (18 x 34 px x 32 ch, 39 KB): TWO LDS buffers, the next chunk's patch issued a whole chunk ahead;
//   * LDS images are dense 64-byte rows (LDS-DMA writes lane-linear); fragment reads stay conflict-free through an
//     XOR swizzle of the 16-byte chunk index, applied on the SOURCE address of each lane's load;
//   * out-of-image patch pixels read a 64-byte zero page;
//   * raw s_barrier + counted `s_waitcnt vmcnt(N)` (a __syncthreads() would drain the DMA queue every stage).
//   * activation-side style modulation is applied to the weight fragments (same product W*s*x; rounding of W*s instead
//     of x*s), so modulated G layers qualify too; inputs needing a pre-activation (BigGAN bn+relu staging) do not.
// Epilogue = conv_tiled's fast path.
#include "common.h"
#include "kernels.h"
#include <stdlib.h>
#include <type_traits>

namespace {
constexpr int NT = 128, NTHR = 512;
// Geometry<TW>: TW = 32 -> tile 16 rows x 32 px (two 32-lane rows per wave); TW = 16 -> tile 16 rows x 16 px (one 32-lane
// row = two image rows per wave) for the 16 x 16 layers, one whole image per workgroup.
template <int TW>
struct Geo {
    static constexpr int RW = TW == 32 ? 2 : 1;                 // 32-lane rows per wave
    static constexpr int TH = 8 * RW * (32 / TW);                // image rows per tile (16)
    static constexpr int PH = TH + 2, PW = TW + 2;
    static constexpr int NVA = PH * PW * 4;                      // 16-byte vectors in a patch
    static constexpr int NA = (NVA + NTHR - 1) / NTHR;           // DMA loads per thread per chunk (5 / 3)
    static constexpr int A_BYTES = NA * NTHR * 16;
    static constexpr int OFF_B = 2 * A_BYTES;
    static constexpr int OFF_C = OFF_B + 3 * (3 * NT * 64);      // epilogue constants [3][NT] floats
    static constexpr int OFF_S = OFF_C + 3 * NT * 4;             // this sample's style row, Cin <= 1024 halfs
    static constexpr int OFF_T = OFF_S + 2048;                   // TRGB: compact toRGB weight rows [hi r,g,b | lo r,g,b][NT] fp16
    static constexpr int OFF_N = OFF_T + 6 * NT * 2 + 512;       // persistent form: the tile's noise values [8 waves][2 rows][32 px] fp32 (+ 512: the idle lanes of the table's second full-wave piece)
    static constexpr int LDS_BYTES = OFF_N + 8 * 64 * 4;
    static_assert(LDS_BYTES <= 163840, "one workgroup per CU");
};
constexpr int NB = 3 * NT * 4 / NTHR;                    // 3 DMA loads per thread per stage
constexpr int B_BYTES = 3 * NT * 64;                     // 24576
constexpr int OROW = NT * 2 + 16;

__device__ __attribute__((aligned(64))) half_t g_zero_page[32];   // zero-initialised: source of the zero padding

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_void;

__device__ __forceinline__ void dma16(const half_t* src, char* lds_wave_base) {
    // LDS destination = wave-uniform base + lane * 16
    __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ void dma4(const float* src, char* lds_wave_base) {     // LDS destination = wave-uniform base + lane * 4
    __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)lds_wave_base, 4, 0, 0);
}

__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+v"(v)); return v; }

#define WAIT_VM(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")
__device__ __forceinline__ void wait_vm(int n) {   // n in {0, 3, 5, 8, 9}: the queue depths this pipeline produces
    if (n >= 9) WAIT_VM(9);
    else if (n >= 8) WAIT_VM(8);
    else if (n >= 5) WAIT_VM(5);
    else if (n >= 3) WAIT_VM(3);
    else WAIT_VM(0);
}
}  // namespace

// TRGB (TW = 32, one n tile = all output channels): toRGB + skip-image sum applied to the finished tile in registers (common.h).
template <int TW, bool TRGB = false>
__global__ __launch_bounds__(512, 1) void conv_glds_kernel(ConvParams p, int NTn, int tiles_x, int tiles_y, int PT) {
    using G = Geo<TW>;
    constexpr int RW = G::RW, TH = G::TH, PW = G::PW, NVA = G::NVA, NA = G::NA, A_BYTES = G::A_BYTES, OFF_B = G::OFF_B,
                  OFF_C = G::OFF_C, OFF_S = G::OFF_S;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lr = lane & 31, kh = lane >> 5;
    const int tpi = tiles_x * tiles_y;
    // work item -> (pixel tile, n tile): the n tiles of one pixel tile sit on one XCD (id % 8) and share its L2
    const int id = blockIdx.x;
    const int lo = id & 7, rest = id >> 3;
    const int nt = rest % NTn, pt = (rest / NTn) * 8 + lo;
    if (pt >= PT) return;
    const int b = pt / tpi, trem = pt - b * tpi;
    const int ty0 = (trem / tiles_x) * TH, tx0 = (trem % tiles_x) * TW;
    const int n0 = nt * NT;
    // this lane's pixel within a 32-lane row: TW = 32 -> (0, lr); TW = 16 -> (lr >> 4, lr & 15)
    const int l_row = TW == 32 ? 0 : lr >> 4, l_col = TW == 32 ? lr : lr & 15;
    constexpr int RPL = 32 / TW;              // image rows per 32-lane row

    // ---- per-thread DMA sources -----------------------------------------------------------------------------
    // vector v = k * 512 + t of an LDS image sits at byte v * 16: row = v >> 2, physical chunk = v & 3 and holds the
    // row's LOGICAL 8-channel chunk (v & 3) ^ ((row >> 2) & 3)
    const half_t* xb = p.x + (long long)b * p.x_bstride;
    long long a_src[NA];      // element offset into the image, or -1 = zero page
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const int v = k * NTHR + t, pix = v >> 2;
        const int pr = pix / PW, pc = pix - pr * PW;
        const int iy = ty0 - 1 + pr, ix = tx0 - 1 + pc;
        const int lc = (v & 3) ^ ((pix >> 2) & 3);
        const bool ok = v < NVA && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
        a_src[k] = ok ? ((long long)iy * p.W + ix) * p.Cin + lc * 8 : -1;
    }
    const half_t* wb = p.w + (long long)b * p.w_bstride;
    long long b_src[NB];      // element offset of (tap-in-row tx, n, chunk) within one tap row, without ty / c0
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int v = k * NTHR + t, row = v >> 2;          // row = tx * 128 + n
        const int tx = row >> 7, n = row & 127;
        const int lc = (v & 3) ^ ((row >> 2) & 3);
        b_src[k] = ((long long)tx * p.Neff + n0 + n) * p.Cin + lc * 8;
    }
    auto issue_a = [&](int c, int buf) {
        char* dst = smem + buf * A_BYTES + wave * 1024;
#pragma unroll
        for (int k = 0; k < NA; ++k)
            dma16(a_src[k] >= 0 ? xb + a_src[k] + c * 32 : g_zero_page + (t & 3) * 8, dst + k * (NTHR * 16));
    };
    auto issue_b = [&](int c, int ty, int slot) {
        char* dst = smem + OFF_B + slot * B_BYTES + wave * 1024;
        const half_t* src = wb + (long long)ty * 3 * p.Neff * p.Cin + c * 32;
#pragma unroll
        for (int k = 0; k < NB; ++k) dma16(src + b_src[k], dst + k * (NTHR * 16));
    };

    f16x acc[RW][4];
#pragma unroll
    for (int i = 0; i < RW; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    const int n_chunks = p.Cin >> 5;
    const int n_stages = n_chunks * 3;
    // Activation-side modulation (x * s[b,i]) is applied to the WEIGHT fragments instead — same product, and the patch
    // needs no transformation on its way into LDS.  The sample's style row is parked in LDS before the first DMA.
    const half_t* Ss = (const half_t*)(smem + OFF_S);
    if (p.sn16) {
        if (t < (p.Cin >> 3)) *(h8*)(smem + OFF_S + t * 16) = *(const h8*)(p.sn16 + (long long)b * p.sn_stride + t * 8);
        __syncthreads();
    }
    // prologue: patch of chunk 0, weights of stages 0 and 1
    issue_a(0, 0);
    issue_b(0, 0, 0);
    if (n_stages > 1) issue_b(0, 1, 1);

    int c = 0, ty = 0;
    for (int s = 0; s < n_stages; ++s) {
        // DMA loads issued after those this stage needs (B(s), and A(c) which is older): B(s+1) [3], and the next chunk's
        // patch [5] when it was issued after B(s), i.e. during the two preceding stages
        int younger = (s + 1 < n_stages) ? NB : 0;
        if (ty != 0 && c + 1 < n_chunks) younger += NA;
        wait_vm(younger);
        __builtin_amdgcn_s_barrier();      // data of this stage visible to every wave; slot (s+2)%3 and patch buffer
                                           // (c+1)&1 are no longer being read by anyone
        if (s + 2 < n_stages) {
            int c2 = c, t2 = ty + 2;
            if (t2 >= 3) { t2 -= 3; c2 = c + 1; }
            issue_b(c2, t2, (s + 2) % 3);
        }
        if (ty == 0 && c + 1 < n_chunks) issue_a(c + 1, (c + 1) & 1);

        const char* As = smem + (c & 1) * A_BYTES;
        const char* Bs = smem + OFF_B + (s % 3) * B_BYTES;
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int lc = kk * 2 + kh;
                h8 wf[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int row = tx * NT + j * 32 + lr;
                    wf[j] = *(const h8*)(Bs + row * 64 + ((lc ^ ((row >> 2) & 3)) << 4));
                }
                if (p.sn16) {
                    const h8 sv = *(const h8*)(Ss + c * 32 + lc * 8);
#pragma unroll
                    for (int j = 0; j < 4; ++j) wf[j] = wf[j] * sv;   // 16 x v_pk_mul_f16 per 8 MFMAs
                }
#pragma unroll
                for (int i = 0; i < RW; ++i) {
                    const int pix = ((wave * RW + i) * RPL + l_row + ty) * PW + l_col + tx;
                    const h8 xf = *(const h8*)(As + pix * 64 + ((lc ^ ((pix >> 2) & 3)) << 4));
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = mfma32(wf[j], xf, acc[i][j]);
                }
            }
        }
        if (++ty == 3) { ty = 0; ++c; }
    }

    // ---- epilogue (conv_tiled's fast path): constants via LDS, batched noise / residual loads, row-order stores -----
    float* Cc = (float*)(smem + OFF_C);
    char* Os = smem + wave * (RW * 32 * OROW);
    const int oyb = ty0 + wave * RW * RPL + l_row, ox = tx0 + l_col;     // lane's pixel of 32-lane row i: (oyb + i * RPL, ox)
    float c_d = 1.f, c_b = 0.f, c_s = 0.f;
    if (t < NT) {
        const int o = n0 + t;
        if (p.dscale) c_d = p.dscale[(long long)b * p.ds_stride + o];
        if (p.bias) c_b = p.bias[o];
        if (p.shift) c_s = p.shift[(long long)b * p.ds_stride + o];
    }
    float nzr[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        nzr[i] = 0.f;
        if (p.noise) nzr[i] = p.noise_strength * p.noise[((long long)(b / p.batch_size) * p.Ho + oyb + i * RPL) * p.Wo + ox];
    }
    float ytap[3][4];                      // TRGB: skip-image taps of this lane's pixel (row kh of the wave's pair, column lr)
    if (TRGB) {
        static_assert(!TRGB || (RW == 2 && TW == 32), "lane half kh owns tile row kh of the wave");
        // the six non-zero rows of the weight table (hi / lo of r, g, b for tile row 0); lanes pick theirs by row below
        if (t < 6 * (NT / 8)) {
            const int row6 = t / (NT / 8), piece = t % (NT / 8);
            const int n = row6 < 3 ? row6 : 8 + (row6 - 3);
            *(h8*)(smem + G::OFF_T + row6 * (NT * 2) + piece * 16) = *(const h8*)(p.trgb_tab + ((long long)b * 32 + n) * NT + piece * 8);
        }
        if (p.trgb_yprev) {
            const int my = (oyb + kh) >> 1, mx = ox >> 1, h2 = p.Ho >> 1, w2 = p.Wo >> 1;
            const float* yp = p.trgb_yprev + (long long)b * 3 * h2 * w2;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    ytap[c][q] = yp[(c * h2 + max(my - 1 + (q >> 1), 0)) * w2 + max(mx - 1 + (q & 1), 0)];
        }
    }
    if (t < NT) { Cc[t] = c_d; Cc[NT + t] = c_b + c_s; }
    __syncthreads();                       // every wave is done with the patch / weight images (Os overlays them)
    const int rcs = p.res_cs ? p.res_cs : p.Cout;
    const ActK ak = act_consts(p.act, p.out_scale);
    f16x rgb;
#pragma unroll
    for (int q = 0; q < 16; ++q) rgb[q] = 0.f;
    // A-operand row of this lane: n = lr & 15 -> colour n & 3, tile row (n >> 2) & 1, lo part n & 8
    const int tn = lr & 15;
    const char* Trow = smem + G::OFF_T + (((tn >> 3) & 1) * 3 + min(tn & 3, 2)) * (NT * 2) + kh * 16;
    const bool trow_ok = (tn & 3) < 3;
    const h8 hzero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        h4 va[RW][4];                      // TRGB: the finished quads of this slice, the 1x1 conv's B operand
        h4 rq[4][RW];
        if (p.res) {
#pragma unroll
            for (int i = 0; i < RW; ++i) {
                const int oy = oyb + i * RPL;
                const half_t* rp = p.res + (p.res_up ? (((long long)b * (p.Ho >> 1) + (oy >> 1)) * (p.Wo >> 1) + (ox >> 1)) * rcs
                                                     : (((long long)b * p.Ho + oy) * p.Wo + ox) * rcs) + n0 + j * 32 + 4 * kh;
#pragma unroll
                for (int g = 0; g < 4; ++g) rq[g][i] = *(const h4*)(rp + 8 * g);
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int nl = j * 32 + 8 * g + 4 * kh;
            const f4 d = *(const f4*)(Cc + nl), bb = *(const f4*)(Cc + NT + nl);      // bb = bias + shift
#pragma unroll
            for (int i = 0; i < RW; ++i) {
                const f4 a = {acc[i][j][g * 4], acc[i][j][g * 4 + 1], acc[i][j][g * 4 + 2], acc[i][j][g * 4 + 3]};
                f4 v = act_apply(a * d + bb + nzr[i], ak);
                if (p.res) v += f4{(float)rq[g][i][0], (float)rq[g][i][1], (float)rq[g][i][2], (float)rq[g][i][3]} * p.out_scale;
                h4 out;
#pragma unroll
                for (int q = 0; q < 4; ++q) out[q] = (half_t)v[q];
                *(h4*)(Os + (i * 32 + lr) * OROW + nl * 2) = out;
                if (TRGB) va[i][g] = out;
            }
        }
        if (TRGB) {
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                const h8 wt = *(const h8*)(Trow + ((j * 2 + gp) * 2) * 16);
#pragma unroll
                for (int i = 0; i < RW; ++i) {
                    const h8 wi = (trow_ok && ((tn >> 2) & 1) == i) ? wt : hzero;
                    rgb = mfma32(wi, __builtin_shufflevector(va[i][2 * gp], va[i][2 * gp + 1], 0, 1, 2, 3, 4, 5, 6, 7), rgb);
                }
            }
        }
    }
    if (TRGB) {
        const long long hw = (long long)p.Ho * p.Wo;
        float* yo = p.trgb_yout + (long long)b * 3 * hw + (long long)(oyb + kh) * p.Wo + ox;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float r = p.trgb_b[c] + (rgb[c] + rgb[4 + c] * (1.f / 2048.f));
            if (p.trgb_yprev) r += trgb_skip(ytap[c], oyb + kh, ox);
            yo[c * hw] = r;
        }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < RW; ++i) {
#pragma unroll
        for (int k = 0; k < NT / 16; ++k) {
            const int v = lane + 64 * k;
            const int pix = v >> 4, chv = v & 15;       // pixel `pix` of the 32-lane row, 8-channel piece chv
            const int prow = TW == 32 ? 0 : pix >> 4, pcol = TW == 32 ? pix : pix & 15;
            half_t* dst = p.y + (((long long)b * p.Ho + ty0 + (wave * RW + i) * RPL + prow) * p.Wo + tx0 + pcol) * p.Cout + n0;
            *(h8*)(dst + chv * 8) = *(const h8*)(Os + (i * 32 + pix) * OROW + chv * 16);
        }
    }
}

// ---- persistent form (TW = 32, an even number of 32-channel chunks) -------------------------------------------------------------
// One 512-thread workgroup per CU means nothing covers a tile's pipeline fill (first DMA round trip), its epilogue and the
// dispatch of the next workgroup: 48 S + B = 134.7 us, 24 S + B = 72.9 us and 12 S + B = 43 us per tile on the 512 / 256 / 128
// channel layers give S = 2.6 us per stage and B = 11 us per tile — a quarter of the 128-channel layers' time.  Here a workgroup
// walks work items id, id + gridDim.x, ... and the DMA ring never drains: with 3 * n_chunks stages per tile (slot rotation period 3)
// and an even chunk count (patch buffer parity), stages 0 and 1 and chunk 0 of the NEXT tile are exactly what "two stages ahead" /
// "one chunk ahead" mean at the end of a tile.  The epilogue therefore runs while those loads are in flight, in the one patch
// buffer and nowhere else: the output transposition goes through it in four 32-channel slices (4 KB + pad per wave).
// XS: ConvParams::xs_out — FIR 4x4 (pad 1) + ::2 of the INPUT map (the D block's skip-branch input) from the patch of each chunk as it
// becomes visible: 8 x 16 pixels x 4 parts = one vector per thread per chunk (chunk c by the pixel tile's n tile c % NTn); its store is one more op in the queue.
// ST: the layer is modulated (ConvParams::sn16) — a template parameter so that the K loop is ONE straight-line body.
//
// Round 6: the K loop is a PING-PONG of the workgroup's two wave groups (waves 0-3 | 4-7: one wave of each per SIMD).  Rounds 2-5 ran
// every wave through the same software-pipelined stage (48 MFMAs, fragment reads rolled in between them, one barrier per stage) and
// sat at 52-62 % MFMA-busy: two in-order waves on a SIMD that both interleave LDS reads, waits and MFMAs leave the matrix pipe idle
// whenever both wait.  Now a PHASE = one tap of one 32-channel chunk = 16 MFMAs per wave on 12 fragments, and each group alternates
//     load interval:  this phase's 12 ds_read_b128, lgkmcnt(0)
//     barrier
//     MFMA interval:  16 back-to-back MFMAs from registers at s_setprio 1, the <= 2 LDS-DMA pieces of the ring issued behind the 4th
//     barrier
// with group 1 ONE barrier behind group 0: on every SIMD one wave streams MFMAs while its partner fetches (the guide's 8-phase GEMM
// schedule, cdna_hip_programming.md section 5 "256^2 8-phase template").  Measured (DESIGN section 5 "Round 6"): the 512-channel layer
// spends 1.385 M shader clocks where MFMAs + barriers alone spend 1.377 M — the loop is matrix-pipe-bound in CYCLES; what is left is
// the clock: 1.60-1.69 GHz with fragment reads and the ring running, 2.2 GHz without them (the chip's power budget).  Ring pieces at the
// top of the load interval (the first form) cost 12 % against rounds 2-5; inside the MFMA interval the family is 8 % faster than it was.
// Ring rules in phase units (q = phase within a chunk, 0..8; all fragment reads of a phase are complete before that phase's first
// barrier, so a buffer is free one barrier after its last reading phase):
//     weights of stage s + 2 (slot (s + 2) % 3, last read in stage s - 1): one piece in each phase of stage s;
//     patch of chunk c + 1 (buffer (c + 1) & 1, last read in chunk c - 1): one piece in each of the chunk's phases 0..4;
//     the wave's pieces of stage s + 1 (and, before a chunk's first stage, of its patch) are waited for in stage s's LAST phase, ahead of
//     its first barrier: every wave passes that barrier before any wave reads stage s + 1.  In-order vmcnt: the pieces issued behind
//     the last piece of stage s + 1 at that point are 4 (q = 2) / 5 (q = 5) / 2 (q = 8) — constants, because the ring never branches:
//     the last item of a workgroup "prefetches" itself again, into buffers nobody reads any more.
// Epilogue operands (per-channel constants, noise, toRGB table) are LDS-DMA pieces too, requested at q = 6 of the last chunk AHEAD of
// that phase's ring piece: the q = 8 wait covers them, the next item's stage-1 weights stay in flight through the epilogue (rounds 2-5:
// vmcnt(0) at the top of every epilogue), and no register of the kernel is the destination of a global load while the ring runs.
template <bool TRGB, bool XS = false, bool ST = true>
__global__ __launch_bounds__(512, 1) void conv_gldsp_kernel(ConvParams p, int NTn, int tiles_x, int tiles_y, int PT) {
    constexpr int TW = 32;
    using G = Geo<TW>;
    constexpr int RW = G::RW, TH = G::TH, PW = G::PW, NVA = G::NVA, NA = G::NA, A_BYTES = G::A_BYTES, OFF_B = G::OFF_B,
                  OFF_C = G::OFF_C, OFF_S = G::OFF_S;
    static_assert(RW == 2 && 8 * RW * 32 * 80 <= A_BYTES, "the sliced output image fits one patch buffer");
    static_assert(NA == 5 && NB == 3, "ring pieces per phase: one weight piece per phase of a stage, one patch piece in phases 0..4 of a chunk");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // (lane geometry is re-derived per phase from an opaque copy of the thread id: as invariants of the item loop these values and
    // every address built from them are hoisted above the K loop, where the register file is full, and spilled)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = wave >> 2;                 // 0: waves 0-3 lead; 1: waves 4-7 run one barrier behind
    const int tpi = tiles_x * tiles_y;
    const int n_work = ((PT + 7) & ~7) * NTn;
    struct Item { int b, ty0, tx0, n0, valid; };   // (no padding bytes: a struct copy with padding goes through scratch = VMEM ops in the ring)
    auto decode = [&](int id) {   // work item -> (pixel tile, n tile): the n tiles of one pixel tile sit on one XCD (id % 8)
        Item w;
        const int lo = id & 7, rest = id >> 3;
        const int nt = rest % NTn, pt = (rest / NTn) * 8 + lo;
        w.valid = id < n_work && pt < PT;
        const int ptc = w.valid ? pt : 0;
        w.b = ptc / tpi;
        const int trem = ptc - w.b * tpi;
        w.ty0 = (trem / tiles_x) * TH;
        w.tx0 = (trem % tiles_x) * TW;
        w.n0 = nt * NT;
        return w;
    };
    int id = blockIdx.x;
    Item cur = decode(id);
    while (id < n_work && !cur.valid) { id += gridDim.x; cur = decode(id); }
    if (id >= n_work) return;

    // ---- DMA sources of the item being LOADED (the current item, or the next one near the end of a tile) ----------------
    const half_t* xb = p.x;
    const half_t* wb = p.w;
    int a_src[NA];            // element offset into the image (< 2^31: launcher), or -1 = zero page
    int b_src[NB];            // element offset of (tap-in-row tx, n, chunk) within one tap row, without ty / c0
    auto aim_a = [&](const Item& w) {
        const int t = opaque(threadIdx.x);
        xb = p.x + (long long)w.b * p.x_bstride;
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            const int v = k * NTHR + t, pix = v >> 2;
            const int pr = pix / PW, pc = pix - pr * PW;
            const int iy = w.ty0 - 1 + pr, ix = w.tx0 - 1 + pc;
            const int lc = (v & 3) ^ ((pix >> 2) & 3);
            const bool ok = v < NVA && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            a_src[k] = ok ? (iy * p.W + ix) * p.Cin + lc * 8 : -1;
        }
    };
    auto aim_b = [&](const Item& w) {
        const int t = opaque(threadIdx.x);
        wb = p.w + (long long)w.b * p.w_bstride;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const int v = k * NTHR + t, row = v >> 2;          // row = tx * 128 + n
            const int tx = row >> 7, n = row & 127;
            const int lc = (v & 3) ^ ((row >> 2) & 3);
            b_src[k] = (tx * p.Neff + w.n0 + n) * p.Cin + lc * 8;
        }
    };
    auto issue_a1 = [&](int k, int c, int buf) {       // piece k of a patch (k is a constant wherever this is called)
        char* dst = smem + buf * A_BYTES + wave * 1024 + k * (NTHR * 16);
        dma16(a_src[k] >= 0 ? xb + a_src[k] + c * 32 : g_zero_page + (threadIdx.x & 3) * 8, dst);
    };
    auto issue_b1 = [&](int k, int c, int ty, int slot) {   // piece k of a weight stage
        char* dst = smem + OFF_B + slot * B_BYTES + wave * 1024 + k * (NTHR * 16);
        dma16(wb + (long long)ty * 3 * p.Neff * p.Cin + c * 32 + b_src[k], dst);
    };
    const int n_chunks = p.Cin >> 5;          // even (launcher)
    const half_t* Ss = (const half_t*)(smem + OFF_S);
    auto park_style = [&](int b) {            // the sample's style row (applied to the weight fragments)
        const int t = threadIdx.x;
        if (t < (p.Cin >> 3)) *(h8*)(smem + OFF_S + t * 16) = *(const h8*)(p.sn16 + (long long)b * p.sn_stride + t * 8);
    };

    aim_a(cur);
    aim_b(cur);
    if (p.sn16) park_style(cur.b);
    {   // operand arrays the layer does not have keep their neutral values for the kernel's lifetime (the epilogue reads all of them)
        const int t = threadIdx.x;
        float* Cc = (float*)(smem + OFF_C);
        if (t < NT) {
            if (!p.dscale) Cc[t] = 1.f;
            if (!p.bias) Cc[NT + t] = 0.f;
            if (!p.shift) Cc[2 * NT + t] = 0.f;
        }
        if (!p.noise) *(float*)(smem + G::OFF_N + t * 4) = 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NA; ++k) issue_a1(k, 0, 0);
#pragma unroll
    for (int k = 0; k < NB; ++k) issue_b1(k, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < NB; ++k) issue_b1(k, 0, 1, 1);
    WAIT_VM(3);                                // chunk 0's patch and stage 0 landed (stage 1 travels on)
    __builtin_amdgcn_s_barrier();
    for (;;) {
        int nid = id + gridDim.x;
        Item nxt = decode(nid);
        while (nid < n_work && !nxt.valid) { nid += gridDim.x; nxt = decode(nid); }
        const bool has_next = nid < n_work;
        if (!has_next) nxt = cur;              // the ring never branches: the last item re-requests itself (nobody reads those buffers)
        const int b = cur.b, ty0 = cur.ty0, tx0 = cur.tx0, n0 = cur.n0;

        f16x acc[RW][4];
#pragma unroll
        for (int i = 0; i < RW; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

        // Epilogue operands (per-channel constants, the tile's noise values, the toRGB table) travel by LDS-DMA too, requested under the
        // LAST stage's MFMAs ahead of that phase's ring piece: the q = 8 wait covers them, and the kernel has NO load into registers
        // while the ring is in flight (hipcc guards every use of such a register with a wait it counts itself — vmcnt(0) here, which
        // drained the next item's stage-1 weights at the top of every epilogue).
        auto prefetch_epilogue = [&]() {
            const int t = opaque(threadIdx.x), lr = t & 31, kh = (t >> 5) & 1;
            if (wave < 2) {                    // channels n0 + t, t < NT = 128: [dscale | bias | shift][NT] fp32
                char* cc = smem + OFF_C + wave * 256;
                if (p.dscale) dma4(p.dscale + (long long)b * p.ds_stride + n0 + t, cc);
                if (p.bias) dma4(p.bias + n0 + t, cc + NT * 4);
                if (p.shift) dma4(p.shift + (long long)b * p.ds_stride + n0 + t, cc + 2 * NT * 4);
            }
            if (p.noise) dma4(p.noise + ((long long)(b / p.batch_size) * p.Ho + ty0 + wave * RW + kh) * p.Wo + tx0 + lr, smem + G::OFF_N + wave * 256);
            if (TRGB && wave < 2) {            // two FULL-wave pieces (96 vectors + 32 idle lanes fed from the zero page into the slack behind the table:
                                               // an LDS-DMA under a lane mask is what hipcc mis-merged in conv_wreg.hip, DESIGN "Round 6")
                const int row6 = min(t / (NT / 8), 5), piece = t % (NT / 8);
                const int n = row6 < 3 ? row6 : 8 + (row6 - 3);
                dma16(t < 6 * (NT / 8) ? p.trgb_tab + ((long long)b * 32 + n) * p.Neff + n0 + piece * 8 : g_zero_page, smem + G::OFF_T + wave * 1024);     // (rows of Neff entries: this n tile's 128)
            }
        };
        if (grp) __builtin_amdgcn_s_barrier();     // group 1 falls one barrier behind: its load intervals face group 0's MFMA intervals
        // (the last chunk is a second copy of the body: its ring pieces belong to the NEXT item, the sources are re-aimed and the epilogue
        // operands are requested there — as run-time cases of ONE body the address arithmetic of aim_a / aim_b sat behind an
        // s_waitcnt vmcnt(0), hipcc's guard for registers that the operand loads of "an earlier iteration" might still be writing)
        auto chunk_body = [&](const int c, auto lastc_tag) {
            constexpr bool lastc = decltype(lastc_tag)::value;
            const char* As = smem + (c & 1) * A_BYTES;
#pragma unroll
            for (int ty = 0; ty < 3; ++ty) {
#pragma unroll
                for (int tx = 0; tx < 3; ++tx) {
                    const int q = ty * 3 + tx;
                    // ---- load interval ------------------------------------------------------------------------------------
                    auto ring_pieces = [&]() {
                        if (q == 6 && lastc) prefetch_epilogue();
                        {   // weights: piece tx of stage s + 2 -> slot (ty + 2) % 3
                            const int t2 = (ty + 2) % 3;
                            int c2 = ty == 0 ? c : c + 1;
                            if (ty != 0 && lastc) {            // runs on into the next item (n_stages % 3 == 0: same slots)
                                if (q == 3) aim_b(nxt);
                                c2 = 0;
                            }
                            issue_b1(tx, c2, t2, t2);
                        }
                        if (q < 5) {    // patch: piece q of chunk c + 1 (n_chunks even: chunk 0 of the next item lives in buffer 0 too)
                            if (q == 0 && lastc) aim_a(nxt);
                            issue_a1(q, lastc ? 0 : c + 1, lastc ? 0 : (c + 1) & 1);
                        }
                    };
                    // (the by-product of chunk c is written by the pixel tile's n tile c % NTn: with every chunk on n tile 0 the workgroups that
                    // walk n tile 0 — a workgroup keeps its n tile from item to item — carried all of it and the others waited for them)
                    if (XS && q == 0 && c % NTn == (n0 >> 7)) {
                        const int tq = opaque(threadIdx.x), part = tq & 3, pix = tq >> 2, ly = pix >> 4, lx = pix & 15;
                        h8 s03, s12;                                     // rows 0 + 3, rows 1 + 2 of the horizontal pass
                        h8 k125, k375;
#pragma unroll
                        for (int e = 0; e < 8; ++e) { k125[e] = (half_t)0.125f; k375[e] = (half_t)0.375f; }
#pragma unroll
                        for (int jy = 0; jy < 4; ++jy) {
                            h8 a[4];
#pragma unroll
                            for (int jx = 0; jx < 4; ++jx) {
                                const int P = (2 * ly + jy) * PW + 2 * lx + jx;
                                a[jx] = *(const h8*)(As + P * 64 + ((part ^ ((P >> 2) & 3)) << 4));
                            }
                            // (explicit FMA forms: left to -ffp-contract the compiler fused a different product from row to row and from build to
                            // build — one fp16 ulp of the by-product, enough to move the D-logit regression guards)
                            const h8 hr = __builtin_elementwise_fma(a[0] + a[3], k125, (a[1] + a[2]) * k375);
                            if (jy == 0) s03 = hr;
                            else if (jy == 1) s12 = hr;
                            else if (jy == 2) s12 = s12 + hr;
                            else s03 = s03 + hr;
                        }
                        const h8 o = __builtin_elementwise_fma(s12, k375, s03 * k125);
                        *(h8*)(p.xs_out + (((long long)b * (p.H >> 1) + (ty0 >> 1) + ly) * (p.W >> 1) + (tx0 >> 1) + lx) * p.Cin + c * 32 + part * 8) = o;
                    }
                    h8 wf[2][4], xf[2][RW];
                    {
                        const int tm = opaque(threadIdx.x), lr = tm & 31, kh = (tm >> 5) & 1;
                        const char* Bs = smem + OFF_B + ty * B_BYTES;        // slot of stage s = 3 c + ty
#pragma unroll
                        for (int kk = 0; kk < 2; ++kk) {
                            const int lc = kk * 2 + kh;
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int row = tx * NT + j * 32 + lr;
                                wf[kk][j] = *(const h8*)(Bs + row * 64 + ((lc ^ ((row >> 2) & 3)) << 4));
                            }
#pragma unroll
                            for (int i = 0; i < RW; ++i) {
                                const int pix = (wave * RW + i + ty) * PW + lr + tx;
                                xf[kk][i] = *(const h8*)(As + pix * 64 + ((lc ^ ((pix >> 2) & 3)) << 4));
                            }
                            if (ST) {
                                const h8 sv = *(const h8*)(Ss + c * 32 + lc * 8);
#pragma unroll
                                for (int j = 0; j < 4; ++j) wf[kk][j] = wf[kk][j] * sv;
                            }
                        }
                    }
                    // the wave's ring pieces of stage s + 1 (and of the next chunk's patch, older) have landed before ANY wave passes this
                    // phase's first barrier; pieces issued behind them: 6 / 6 / 3 (the by-product's store is not counted: conservative)
                    if (tx == 2) { if (ty == 2) WAIT_VM(2); else if (ty == 1) WAIT_VM(5); else WAIT_VM(4); }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_barrier();
                    // ---- MFMA interval ------------------------------------------------------------------------------------
                    __builtin_amdgcn_s_setprio(1);
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
#pragma unroll
                            for (int i = 0; i < RW; ++i) acc[i][j] = mfma32(wf[kk][j], xf[kk][i], acc[i][j]);
                            if (kk == 0 && j == 1) { __builtin_amdgcn_sched_barrier(0); ring_pieces(); __builtin_amdgcn_sched_barrier(0); }
                        }
                    __builtin_amdgcn_s_setprio(0);
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_barrier();
                }
            }
        };
        for (int c = 0; c + 1 < n_chunks; ++c) chunk_body(c, std::false_type{});
        chunk_body(n_chunks - 1, std::true_type{});

        // ---- epilogue: constants via LDS, batched noise / residual loads, row-order stores through patch buffer 1 -------------
        // Group 0 is one barrier ahead: it re-aligns here (group 1 runs its last MFMA interval meanwhile).  Every fragment read of the
        // item was complete before the barrier both groups have passed by then, and the q = 8 wait + barrier made the operands visible.
        if (!grp) __builtin_amdgcn_s_barrier();
        const int t = opaque(threadIdx.x), lane = t & 63, lr = lane & 31, kh = lane >> 5;
        const float* Cc = (const float*)(smem + OFF_C);
        constexpr int OP = 80;                                      // bytes per staged pixel slice (64 + 16: bank spread)
        char* Os = smem + A_BYTES + wave * (RW * 32 * OP);
        const int oyb = ty0 + wave * RW, ox = tx0 + lr;              // lane's pixel of tile row i: (oyb + i, ox)
        const int rcs = p.res_cs ? p.res_cs : p.Cout;
        const ActK ak = act_consts(p.act, p.out_scale);
        // loads into registers start HERE (the ring has three pieces in flight and is not waited for): values used at the END of the epilogue
        float ytap[3][4];
        h8 nsty;
        if (TRGB && p.trgb_yprev) {
            const int my = (oyb + kh) >> 1, mx = ox >> 1, h2 = p.Ho >> 1, w2 = p.Wo >> 1;
            const float* yp = p.trgb_yprev + (long long)b * 3 * h2 * w2;
#pragma unroll
            for (int cc = 0; cc < 3; ++cc)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    ytap[cc][q] = yp[(cc * h2 + max(my - 1 + (q >> 1), 0)) * w2 + max(mx - 1 + (q & 1), 0)];
        }
        if (ST && t < (p.Cin >> 3)) nsty = *(const h8*)(p.sn16 + (long long)nxt.b * p.sn_stride + t * 8);
        float nzr[RW];
#pragma unroll
        for (int i = 0; i < RW; ++i) nzr[i] = p.noise_strength * *(const float*)(smem + G::OFF_N + (wave * 64 + i * 32 + lr) * 4);
        f16x rgb;
#pragma unroll
        for (int q = 0; q < 16; ++q) rgb[q] = 0.f;
        const int tn = lr & 15;
        const char* Trow = smem + G::OFF_T + (((tn >> 3) & 1) * 3 + min(tn & 3, 2)) * (NT * 2) + kh * 16;
        const bool trow_ok = (tn & 3) < 3;
        const h8 hzero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h4 va[RW][4];
            h4 rq[4][RW];
            if (p.res) {
#pragma unroll
                for (int i = 0; i < RW; ++i) {
                    const int oy = oyb + i;
                    const half_t* rp = p.res + (p.res_up ? (((long long)b * (p.Ho >> 1) + (oy >> 1)) * (p.Wo >> 1) + (ox >> 1)) * rcs
                                                         : (((long long)b * p.Ho + oy) * p.Wo + ox) * rcs) + n0 + j * 32 + 4 * kh;
#pragma unroll
                    for (int g = 0; g < 4; ++g) rq[g][i] = *(const h4*)(rp + 8 * g);
                }
            }
            // this slice's eight constant quads as ONE batch of LDS reads: read quad by quad (the compiler's order at 224 live VGPRs)
            // every quad sat behind its own LDS round trip — 32 per item, with all eight waves of the workgroup in the epilogue together
            constexpr int GB = TRGB ? 2 : 4;                 // (the toRGB instance has 16 fewer registers to spare)
#pragma unroll
            for (int g0 = 0; g0 < 4; g0 += GB) {
            f4 dq[GB], bq[GB];
#pragma unroll
            for (int g = 0; g < GB; ++g) {
                const int nl = j * 32 + 8 * (g0 + g) + 4 * kh;
                dq[g] = *(const f4*)(Cc + nl);
                bq[g] = *(const f4*)(Cc + NT + nl) + *(const f4*)(Cc + 2 * NT + nl);      // bias + shift
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = g0; g < g0 + GB; ++g) {
                const f4 d = dq[g - g0], bb = bq[g - g0];
#pragma unroll
                for (int i = 0; i < RW; ++i) {
                    const f4 a = {acc[i][j][g * 4], acc[i][j][g * 4 + 1], acc[i][j][g * 4 + 2], acc[i][j][g * 4 + 3]};
                    f4 v = act_apply(a * d + bb + nzr[i], ak);
                    if (p.res) v += f4{(float)rq[g][i][0], (float)rq[g][i][1], (float)rq[g][i][2], (float)rq[g][i][3]} * p.out_scale;
                    h4 out;
#pragma unroll
                    for (int q = 0; q < 4; ++q) out[q] = (half_t)v[q];
                    *(h4*)(Os + (i * 32 + lr) * OP + (8 * g + 4 * kh) * 2) = out;
                    if (TRGB) va[i][g] = out;
                }
            }
            }
            if (TRGB) {
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) {
                    const h8 wt = *(const h8*)(Trow + ((j * 2 + gp) * 2) * 16);
#pragma unroll
                    for (int i = 0; i < RW; ++i) {
                        const h8 wi = (trow_ok && ((tn >> 2) & 1) == i) ? wt : hzero;
                        rgb = mfma32(wi, __builtin_shufflevector(va[i][2 * gp], va[i][2 * gp + 1], 0, 1, 2, 3, 4, 5, 6, 7), rgb);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();        // LDS is in-order per wave: only pin the compiler's order
#pragma unroll
            for (int k = 0; k < 4; ++k) {           // 2 rows x 32 px x four 16-byte pieces of this 32-channel slice
                const int v = lane + 64 * k, i = v >> 7, pix = (v >> 2) & 31, piece = v & 3;
                half_t* dst = p.y + (((long long)b * p.Ho + oyb + i) * p.Wo + tx0 + pix) * p.Cout + n0 + j * 32 + piece * 8;
                *(h8*)dst = *(const h8*)(Os + (i * 32 + pix) * OP + piece * 16);
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (TRGB) {
            const long long hw = (long long)p.Ho * p.Wo;
            if (p.trgb_part) {       // several n tiles per pixel: this tile's partial sum over its 128 channels (launch_trgb_finish adds them up)
                float* yo = p.trgb_part + ((long long)(n0 >> 7) * p.B + b) * 3 * hw + (long long)(oyb + kh) * p.Wo + ox;
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) yo[cc * hw] = rgb[cc] + rgb[4 + cc] * (1.f / 2048.f);
            } else {
                float* yo = p.trgb_yout + (long long)b * 3 * hw + (long long)(oyb + kh) * p.Wo + ox;
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) {
                    float r = p.trgb_b[cc] + (rgb[cc] + rgb[4 + cc] * (1.f / 2048.f));
                    if (p.trgb_yprev) r += trgb_skip(ytap[cc], oyb + kh, ox);
                    yo[cc * hw] = r;
                }
            }
        }
        if (ST && t < (p.Cin >> 3)) *(h8*)(smem + OFF_S + t * 16) = nsty;     // (every wave left the K loop, the style row's only reader, two barriers ago)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();          // every wave is done with patch buffer 1 (the output slices) and the constants
        if (!has_next) break;
        id = nid;
        cur = nxt;
    }
    WAIT_VM(0);                                // the last item's self-prefetch
}


// what conv_glds_kernel / conv_gldsp_kernel implement (style from the fp16 table, applied to the weight fragments)
static constexpr uint32_t GLDS_FEATURES = CF_STYLE | CF_DEMOD | CF_SHIFT | CF_NOISE | CF_RES | CF_RES_CS | CF_RES_UP | CF_SAMPLE_W | CF_TORGB |
                                          CF_TORGB_PART | CF_XS_OUT;

static int glds_cus() { return glass_cu_count() - glass_cu_count() % 8; }       // a workgroup keeps its XCD (id % 8) across items
template <int TW, bool TRGB>
static void launch_glds(const ConvParams& p, hipStream_t st) {
    using G = Geo<TW>;
    static DevOnce once;                       // (one per template instance)
    once.run([&] { (void)hipFuncSetAttribute((const void*)conv_glds_kernel<TW, TRGB>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_BYTES); });
    const int tiles_x = p.Wc / TW, tiles_y = p.Hc / G::TH, PT = p.B * tiles_x * tiles_y, NTn = p.Neff / NT;
    hipLaunchKernelGGL((conv_glds_kernel<TW, TRGB>), dim3((PT + 7) / 8 * 8 * NTn), dim3(NTHR), G::LDS_BYTES, st, p, NTn, tiles_x, tiles_y, PT);
}
template <bool TRGB, bool XS, bool ST>
static void launch_gldsp(const ConvParams& p, hipStream_t st) {
    using G = Geo<32>;
    static DevOnce once;
    once.run([&] { (void)hipFuncSetAttribute((const void*)conv_gldsp_kernel<TRGB, XS, ST>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS_BYTES); });
    const int tiles_x = p.Wc / 32, tiles_y = p.Hc / G::TH, PT = p.B * tiles_x * tiles_y, NTn = p.Neff / NT;
    hipLaunchKernelGGL((conv_gldsp_kernel<TRGB, XS, ST>), dim3(glds_cus()), dim3(NTHR), G::LDS_BYTES, st, p, NTn, tiles_x, tiles_y, PT);
}

// the persistent form where the launch has >= 2 work items per CU, else the one-item-per-workgroup form `name`
template <int TW, bool TRGB = false>
static ConvKernel glds_inst(const ConvParams& p, const char* name) {
    // (>= 2 work items per CU at the NOMINAL population, common.h: this branch also decides whether the blur-down by-product exists,
    // so it must be a function of the layer geometry only)
    const long long work_nominal = (long long)GLASS_NOMINAL_POP * (p.Wc / TW) * (p.Hc / Geo<TW>::TH) * (p.Neff / NT);
    if (TW == 32 && (p.Cin & 63) == 0 && work_nominal >= 2 * glds_cus()) {   // ring parity needs an even chunk count
        // (reported under the symbol that runs, so that the per-kernel profile lines up with rocprofv3's kernel names)
        const bool sty = p.sn16 != nullptr;
        if (p.xs_out && !TRGB) return sty ? ConvKernel{"conv_gldsp_kernel<false,true,true>", launch_gldsp<false, true, true>}
                                          : ConvKernel{"conv_gldsp_kernel<false,true,false>", launch_gldsp<false, true, false>};
        if (TRGB) return sty ? ConvKernel{"conv_gldsp_kernel<true,false,true>", launch_gldsp<true, false, true>}
                             : ConvKernel{"conv_gldsp_kernel<true,false,false>", launch_gldsp<true, false, false>};
        return sty ? ConvKernel{"conv_gldsp_kernel<false,false,true>", launch_gldsp<false, false, true>}
                   : ConvKernel{"conv_gldsp_kernel<false,false,false>", launch_gldsp<false, false, false>};
    }
    if (p.xs_out || p.trgb_part) return conv_refused();   // (the blur-down by-product and the toRGB partial sums exist in the persistent form only)
    return {name, launch_glds<TW, TRGB>};
}

ConvKernel choose_conv_glds(const ConvParams& p) {
    const uint32_t f = conv_features(p);
    if (f & ~GLDS_FEATURES) return conv_refused(f & ~GLDS_FEATURES);
    if (!glass_lds_fits(Geo<32>::LDS_BYTES) || !glass_lds_fits(Geo<16>::LDS_BYTES)) return conv_refused();
    if (((f & CF_XS_OUT) && ((f & (CF_STYLE | CF_TORGB | CF_TORGB_PART)) || p.Wc % 32 != 0)) || !p.y || p.KS != 3 || p.stride != 1 || p.pad != 1)
        return conv_refused();
    if (((f & CF_STYLE) && !p.sn16) || p.Cin > 1024) return conv_refused();
    if (p.Cin % 32 != 0 || p.Cin < 128 || p.Neff % NT != 0 || (p.Cout & 7) || p.Hc % 16 != 0) return conv_refused();
    if ((long long)p.H * p.W * p.Cin >= (1LL << 31)) return conv_refused();
    if (f & CF_TORGB_PART) {   // toRGB partial sums per 128-wide n tile (persistent form only: the caller falls back to the separate pass otherwise)
        if (!p.trgb_tab || (f & CF_TORGB) || p.trgb_yprev || p.Neff != p.Cout || p.Wc % 32 != 0) return conv_refused();
        return glds_inst<32, true>(p, nullptr);
    }
    if (f & CF_TORGB) {   // fused toRGB: only where one workgroup holds every output channel of its pixels
        if (!p.trgb_tab || !p.trgb_b || p.Neff != NT || p.Cout != NT || p.Wc % 32 != 0) return conv_refused();
        return glds_inst<32, true>(p, "conv_glds_kernel<32,true>");
    }
    if (p.Wc % 32 == 0) return glds_inst<32>(p, "conv_glds_kernel<32>");
    if (p.Wc % 16 == 0) return glds_inst<16>(p, "conv_glds_kernel<16>");
    return conv_refused();
}
