// lpips.hip — the kernels of the perceptual objective (LPIPS on VGG16, stylegan2/external_models/lpips.py:34-78) that no other family has:
// the input (box mean of the generated image + `_scale`), the 3 -> 64 first convolution (K = 27, below gemm_tiled's 64-channel gather
// step), the 2 x 2 max pool and the head (channel norms, weighted squared difference, mean over pixels).  Activations are NHWC fp16, i.e.
// GEMM rows; the other twelve convolutions are gemm_tiled through its implicit patch matrix (mode 5 with A = 1, S = bias); the walker is
// lpips.cpp.  Every sum below has a fixed order that depends on the pixel / channel index alone: a candidate's distance is the same bits
// wherever it sits in a launch.
#include "common.h"
#include "kernels.h"

// ---- input: F.interpolate(mode="area") for R % S == 0 (a box x box mean, project.py:113-122), then (v - shift_c) / scale_c ----------------
// y: planar fp32 [B][3][R][R] (the raw generator output, before biggan_norm, unclamped).  out: [B][S][S][4] fp16, channel 3 = 0 (the first
// convolution reads a pixel as one 8-byte vector).  One thread = one output pixel; the box is summed row by row, left to right, in fp32.
__global__ __launch_bounds__(256) void lpips_input_kernel(const float* y, int B, int R, int S, half_t* out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * S * S) return;
    const int box = R / S;
    const int ox = (int)(idx % S), oy = (int)((idx / S) % S), b = (int)(idx / ((long long)S * S));
    const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
    const float inv = 1.f / (float)(box * box);
    h4 o;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* p = y + (((long long)b * 3 + c) * R + (long long)oy * box) * R + (long long)ox * box;
        float s = 0.f;
        for (int dy = 0; dy < box; ++dy)
            for (int dx = 0; dx < box; ++dx) s += p[(long long)dy * R + dx];
        o[c] = (half_t)((s * inv - shift[c]) / scale[c]);
    }
    o[3] = (half_t)0.f;
    *(h4*)(out + idx * 4) = o;
}
bool launch_lpips_input(const float* y, int B, int R, int S, half_t* out, hipStream_t st) {
    if (B <= 0 || S <= 0 || R < S || R % S != 0 || R / S > 8) return false;
    const long long total = (long long)B * S * S;
    hipLaunchKernelGGL(lpips_input_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, y, B, R, S, out);
    return true;
}

// ---- VGG16 features.0: 3 x 3, pad 1, 3 -> 64 channels, + bias + ReLU --------------------------------------------------------------------
// x [B][S][S][4] fp16 (lpips_input_kernel's layout), w [27][64] fp16 with row (ci, ky, kx), y [B][S][S][64].  One thread = one output pixel x
// 8 output channels; the 27 x 64 weights sit in LDS as fp32 (6.9 KB; the eight channel groups of a pixel are neighbouring lanes, so a wave
// reads eight LDS rows of 32 bytes per tap: broadcast within a group, no bank conflict across groups).
__global__ __launch_bounds__(256) void vgg_conv1_kernel(const half_t* x, const half_t* w, const float* bias, int B, int S, half_t* y) {
    __shared__ float ws[27 * 64];
    for (int i = threadIdx.x; i < 27 * 64; i += 256) ws[i] = (float)w[i];
    __syncthreads();
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * S * S * 8) return;
    const int cg = (int)(idx & 7);
    const long long pix = idx >> 3;
    const int ox = (int)(pix % S), oy = (int)((pix / S) % S), b = (int)(pix / ((long long)S * S));
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy + ky - 1;
        if ((unsigned)iy >= (unsigned)S) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox + kx - 1;
            if ((unsigned)ix >= (unsigned)S) continue;
            const h4 px = *(const h4*)(x + (((long long)b * S + iy) * S + ix) * 4);
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const float v = (float)px[ci];
                const float* wr = ws + (ci * 9 + ky * 3 + kx) * 64 + cg * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += v * wr[j];
            }
        }
    }
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)fmaxf(acc[j] + bias[cg * 8 + j], 0.f);
    *(h8*)(y + pix * 64 + cg * 8) = o;
}
bool launch_vgg_conv1(const half_t* x, const half_t* w, const float* bias, int B, int S, half_t* y, hipStream_t st) {
    if (B <= 0 || S <= 0) return false;
    const long long total = (long long)B * S * S * 8;
    hipLaunchKernelGGL(vgg_conv1_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, w, bias, B, S, y);
    return true;
}

// ---- MaxPool2d(2) on NHWC fp16 (exact): one thread = one output pixel x 8 channels ------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool2_kernel(const half_t* x, int B, int H, int W, int C, half_t* y) {
    const int ng = C >> 3, Ho = H >> 1, Wo = W >> 1;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * Ho * Wo * ng) return;
    const int cg = (int)(idx % ng);
    const long long pix = idx / ng;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), b = (int)(pix / ((long long)Ho * Wo));
    const half_t* p = x + (((long long)b * H + 2 * oy) * W + 2 * ox) * C + cg * 8;
    const h8 v00 = *(const h8*)p, v01 = *(const h8*)(p + C), v10 = *(const h8*)(p + (long long)W * C), v11 = *(const h8*)(p + (long long)W * C + C);
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)fmaxf(fmaxf((float)v00[j], (float)v01[j]), fmaxf((float)v10[j], (float)v11[j]));
    *(h8*)(y + pix * C + cg * 8) = o;
}
bool launch_maxpool2(const half_t* x, int B, int H, int W, int C, half_t* y, hipStream_t st) {
    if (B <= 0 || C <= 0 || C % 8 != 0 || (H & 1) || (W & 1) || H < 2 || W < 2) return false;
    const long long total = (long long)B * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(maxpool2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, B, H, W, C, y);
    return true;
}

// ---- head of one slice: sum over pixels of sum_c lin_c (x0_c rsqrt(|x0|^2 + 1e-8) - x1_c rsqrt(|x1|^2 + 1e-8))^2, / HW ------------------
// A workgroup owns GLASS_LPIPS_PIXB consecutive pixels of ONE image.  G = C / 8 neighbouring lanes (8 .. 64, inside one wave) share a pixel:
// each holds 8 consecutive channels of both maps (one 16-byte load each).  Order of every sum: the lane's 8 channels in index order; across the
// G lanes a butterfly (the same adds in every lane: a + b is commutative); a lane group adds its pixels g, g + 256 / G, ... in index order;
// thread 0 adds the groups' sums in group order.  lpips_reduce_kernel then adds an image's workgroup sums in block order, divides by HW and
// adds the slice term to d[image] (or sets it, for the first slice): no float atomics anywhere.
template <int G>
__global__ __launch_bounds__(256) void lpips_head_kernel(const half_t* x0, const half_t* x1, long long x1_bs, const float* lin, int HW, float* part) {
    constexpr int C = G * 8, NG = 256 / G;
    __shared__ float red[NG];
    const int t = threadIdx.x, g = t / G, l = t % G;
    const int img = blockIdx.y, pix0 = blockIdx.x * GLASS_LPIPS_PIXB;
    const int npix = min(GLASS_LPIPS_PIXB, HW - pix0);      // >= 1: the grid is ceil(HW / PIXB)
    const half_t* a = x0 + ((long long)img * HW + pix0) * C + l * 8;
    const half_t* b = x1 + (long long)img * x1_bs + (long long)pix0 * C + l * 8;
    const f4 lw0 = *(const f4*)(lin + l * 8), lw1 = *(const f4*)(lin + l * 8 + 4);
    float acc = 0.f;
    for (int i = g; i < GLASS_LPIPS_PIXB; i += NG) {         // the same trip count in every lane: the shuffles below are wave-wide
        const bool ok = i < npix;
        const long long off = (long long)(ok ? i : 0) * C;   // (a valid address either way)
        const h8 va = *(const h8*)(a + off), vb = *(const h8*)(b + off);
        float fa[8], fb[8], s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            fa[j] = (float)va[j];
            fb[j] = (float)vb[j];
            s0 += fa[j] * fa[j];
            s1 += fb[j] * fb[j];
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            s0 += __shfl_xor(s0, o);
            s1 += __shfl_xor(s1, o);
        }
        const float r0 = 1.f / sqrtf(s0 + 1e-8f), r1 = 1.f / sqrtf(s1 + 1e-8f);
        float ds = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float df;
            {
#pragma clang fp contract(off)
                // two rounded products, then the difference — fused into fma(fa, r0, -(fb r1)) equal maps would leave the product's rounding error
                const float p0 = fa[j] * r0, p1 = fb[j] * r1;
                df = p0 - p1;
            }
            ds += (j < 4 ? lw0[j & 3] : lw1[j & 3]) * (df * df);
        }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) ds += __shfl_xor(ds, o);
        if (ok) acc += ds;
    }
    if (l == 0) red[g] = acc;
    __syncthreads();
    if (t == 0) {
        float s = 0.f;
        for (int k = 0; k < NG; ++k) s += red[k];
        part[(long long)img * gridDim.x + blockIdx.x] = s;
    }
}
// d[i] (first ? = : +=) (sum of image i's workgroup sums in block order) / HW: one thread per image
__global__ void lpips_reduce_kernel(const float* part, int n, int nblk, float inv_hw, int first, float* d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += part[(long long)i * nblk + k];
    s *= inv_hw;
    d[i] = first ? s : d[i] + s;
}
bool launch_lpips_head(const half_t* x0, const half_t* x1, long long x1_bs, const float* lin, int n, int HW, int C, float* part, int first, float* d,
                       hipStream_t st) {
    if (n <= 0 || HW <= 0 || n > 65535) return false;
    const int nblk = (HW + GLASS_LPIPS_PIXB - 1) / GLASS_LPIPS_PIXB;
    const dim3 grid(nblk, n);
    switch (C) {
        case 64: hipLaunchKernelGGL(lpips_head_kernel<8>, grid, dim3(256), 0, st, x0, x1, x1_bs, lin, HW, part); break;
        case 128: hipLaunchKernelGGL(lpips_head_kernel<16>, grid, dim3(256), 0, st, x0, x1, x1_bs, lin, HW, part); break;
        case 256: hipLaunchKernelGGL(lpips_head_kernel<32>, grid, dim3(256), 0, st, x0, x1, x1_bs, lin, HW, part); break;
        case 512: hipLaunchKernelGGL(lpips_head_kernel<64>, grid, dim3(256), 0, st, x0, x1, x1_bs, lin, HW, part); break;
        default: return false;      // VGG16's widths
    }
    hipLaunchKernelGGL(lpips_reduce_kernel, dim3((n + 63) / 64), dim3(64), 0, st, part, n, nblk, 1.f / (float)HW, first, d);
    return true;
}
