// clip_resnet.hip — the kernels of CLIP's ModifiedResNet image towers (clip/model.py:9-149: RN50, RN101) that no other family has:
// the stem (conv1 3 -> w/2 stride 2 from the resized image; conv2 / conv3 with w/2 input channels, below gemm_tiled's 64-channel gather
// step), the 2 x 2 average pool, the attention pool's token builder and the pick of its token-0 rows.  Activations are NHWC fp16, i.e.
// GEMM rows; BatchNorm is an fp32 per-channel scale and shift in every epilogue (A = gamma / sqrt(var + eps), S = beta - mean A).
// The bottlenecks' 1 x 1 and 3 x 3 convolutions are gemm_tiled (mode 5, and its implicit patch matrix); the walker is clip.cpp.
#include "common.h"
#include "kernels.h"

// ---- stem conv1: 3 x 3, stride 2, pad 1, 3 -> C1 channels, + BN + ReLU ---------------------------------------------------------------
// The image is read where every preprocessing mode of the engine leaves it: the patch operand of a 32-pixel patch grid,
// img[(b G + Y / 32) G + X / 32][(c 32 + Y % 32) 32 + X % 32], G = S / 32 (launch_resize_patches, launch_preprocess_patches,
// launch_image_patches with ps = 32).  One thread = one output pixel x 8 output channels; the 27 C1 weights sit in LDS as fp32.
__global__ __launch_bounds__(256) void rn_stem_conv1_kernel(const half_t* img, const half_t* w, const float* bn_a, const float* bn_s, int B, int S,
                                                            int C1, half_t* y) {
    extern __shared__ float rn_ws[];      // [27][C1], row (ci, ky, kx)
    for (int i = threadIdx.x; i < 27 * C1; i += 256) rn_ws[i] = (float)w[i];
    __syncthreads();
    const int ng = C1 >> 3, Ho = S >> 1, G = S >> 5;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)B * Ho * Ho * ng) return;
    const int cg = (int)(idx % ng);
    const long long pix = idx / ng;
    const int ox = (int)(pix % Ho), oy = (int)((pix / Ho) % Ho), b = (int)(pix / ((long long)Ho * Ho));
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy + ky - 1;
        if ((unsigned)iy >= (unsigned)S) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox + kx - 1;
            if ((unsigned)ix >= (unsigned)S) continue;
            const half_t* px = img + (((long long)b * G + (iy >> 5)) * G + (ix >> 5)) * 3072 + (iy & 31) * 32 + (ix & 31);
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const float v = (float)px[ci * 1024];
                const float* wr = rn_ws + (ci * 9 + ky * 3 + kx) * C1 + cg * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += v * wr[j];
            }
        }
    }
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)fmaxf(acc[j] * bn_a[cg * 8 + j] + bn_s[cg * 8 + j], 0.f);
    *(h8*)(y + pix * C1 + cg * 8) = o;
}
bool launch_rn_stem_conv1(const half_t* img, const half_t* w, const float* bn_a, const float* bn_s, int B, int S, int C1, half_t* y, hipStream_t st) {
    if (S % 32 != 0 || C1 % 8 != 0 || C1 > 512) return false;
    const long long total = (long long)B * (S / 2) * (S / 2) * (C1 / 8);
    hipLaunchKernelGGL(rn_stem_conv1_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 27 * C1 * sizeof(float), st, img, w, bn_a, bn_s, B, S, C1, y);
    return true;
}

// ---- stem conv2 / conv3: 3 x 3, stride 1, pad 1, Cin % 16 == 0, + BN + ReLU ----------------------------------------------------------
// Implicit GEMM on MFMA 32x32x16 with both operands straight from global memory (the map's 8-channel pieces and the weight rows are 16-byte
// loads; the weights, 18 - 36 KB, stay in L2 / L1).  A wave owns 32 consecutive pixels and 32 NJ output channels; the weight rows are the MFMA's
// A operand, so a lane ends up with quads of consecutive channels of ONE pixel (8-byte stores), as in gemm_tiled.  w: [tap][Cout][Cin].
template <int NJ>
__global__ __launch_bounds__(256) void rn_conv3x3_kernel(const half_t* x, const half_t* w, const float* bn_a, const float* bn_s, int B, int H, int W,
                                                         int Cin, int Cout, half_t* y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 31, kh = lane >> 5;
    const long long M = (long long)B * H * W;
    const long long m = (long long)blockIdx.x * 128 + wave * 32 + lr;
    const int n0 = blockIdx.y * (32 * NJ);
    const bool mvalid = m < M;
    const long long mc = mvalid ? m : M - 1;
    const int hw = H * W, b = (int)(mc / hw), rem = (int)(mc - (long long)b * hw), oy = rem / W, ox = rem - oy * W;
    f16x acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
        const bool ok = mvalid && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        const half_t* xp = x + (((long long)b * H + (ok ? iy : oy)) * W + (ok ? ix : ox)) * Cin + kh * 8;      // (a valid address either way)
        const half_t* wp = w + ((long long)tap * Cout + n0 + lr) * Cin + kh * 8;
        for (int c0 = 0; c0 < Cin; c0 += 16) {
            const h8 xv = *(const h8*)(xp + c0);
            const h8 xf = ok ? xv : zero;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const h8 wf = *(const h8*)(wp + (long long)j * 32 * Cin + c0);
                acc[j] = mfma32(wf, xf, acc[j]);
            }
        }
    }
    if (!mvalid) return;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = n0 + j * 32 + 8 * g + 4 * kh;
            const f4 a = *(const f4*)(bn_a + n), s = *(const f4*)(bn_s + n);
            h4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = (half_t)fmaxf(acc[j][g * 4 + q] * a[q] + s[q], 0.f);
            *(h4*)(y + m * Cout + n) = o;
        }
}
const char* launch_rn_conv3x3(const half_t* x, const half_t* w, const float* bn_a, const float* bn_s, int B, int H, int W, int Cin, int Cout, half_t* y,
                              hipStream_t st) {
    if (Cin % 16 != 0 || Cout % 32 != 0 || B <= 0 || H <= 0 || W <= 0) return nullptr;
    const unsigned gx = (unsigned)(((long long)B * H * W + 127) / 128);
    if (Cout % 64 == 0) {
        hipLaunchKernelGGL(rn_conv3x3_kernel<2>, dim3(gx, Cout / 64), dim3(256), 0, st, x, w, bn_a, bn_s, B, H, W, Cin, Cout, y);
        return "rn_conv3x3_kernel<2>";
    }
    hipLaunchKernelGGL(rn_conv3x3_kernel<1>, dim3(gx, Cout / 32), dim3(256), 0, st, x, w, bn_a, bn_s, B, H, W, Cin, Cout, y);
    return "rn_conv3x3_kernel<1>";
}

// ---- AvgPool2d(2) on NHWC fp16, fp32 sum: one thread = one output pixel x 8 channels -------------------------------------------------
__global__ __launch_bounds__(256) void rn_avgpool2_kernel(const half_t* x, int B, int H, int W, int C, half_t* y) {
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
    for (int j = 0; j < 8; ++j) o[j] = (half_t)((((float)v00[j] + (float)v01[j]) + ((float)v10[j] + (float)v11[j])) * 0.25f);
    *(h8*)(y + pix * C + cg * 8) = o;
}
bool launch_rn_avgpool2(const half_t* x, int B, int H, int W, int C, half_t* y, hipStream_t st) {
    if (C % 8 != 0 || (H & 1) || (W & 1) || H < 2 || W < 2) return false;
    const long long total = (long long)B * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(rn_avgpool2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, B, H, W, C, y);
    return true;
}

// ---- attention pool tokens (clip/model.py:66-68): tok[b][0] = mean over the HW pixels, tok[b][1 + i] = pixel i, + positional_embedding ---
// One thread = one (image, channel): it walks the HW pixels once, fp32 sum; consecutive threads are consecutive channels.
__global__ __launch_bounds__(256) void rn_attnpool_tokens_kernel(const half_t* x, const float* pos, int B, int HW, int C, half_t* tok) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= C) return;
    const half_t* xb = x + (long long)b * HW * C + c;
    half_t* tb = tok + (long long)b * (HW + 1) * C + c;
    float sum = 0.f;
    for (int i = 0; i < HW; ++i) {
        const float v = (float)xb[(long long)i * C];
        sum += v;
        tb[(long long)(i + 1) * C] = (half_t)(v + pos[(long long)(i + 1) * C + c]);
    }
    tb[0] = (half_t)(sum / (float)HW + pos[c]);
}
void launch_rn_attnpool_tokens(const half_t* x, const float* pos, int B, int HW, int C, half_t* tok, hipStream_t st) {
    hipLaunchKernelGGL(rn_attnpool_tokens_kernel, dim3((C + 255) / 256, B), dim3(256), 0, st, x, pos, B, HW, C, tok);
}

// token 0 of every image's attention output as fp32 rows: the operand of c_proj (the pool returns x[0] only, clip/model.py:89)
__global__ __launch_bounds__(256) void rn_token0_rows_kernel(const half_t* att, int T, int C, float* out) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c < C) out[(long long)b * C + c] = (float)att[(long long)b * T * C + c];
}
void launch_rn_token0_rows(const half_t* att, int B, int T, int C, float* out, hipStream_t st) {
    hipLaunchKernelGGL(rn_token0_rows_kernel, dim3((C + 255) / 256, B), dim3(256), 0, st, att, T, C, out);
}
