// kernels_misc.hip — the non-GEMM kernels of the fitness path (fp32 heads, image ops,
// FIR filters, minibatch-std).  All memory-bound; vectorised 16-byte accesses on the
// NHWC fp16 activations, wave64 reductions.
#include "common.h"
#include "kernels.h"
#include "dense_body.h"
#include <stdlib.h>
#include <string.h>

#include <algorithm>

// ---- mapping network input normalisation: stylegan2/models.py:625-626 --------------
__global__ void pixelnorm_kernel(const float* z, float* out, int L, float eps) {
    const int p = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int i = lane; i < L; i += 64) { const float v = z[(long long)p * L + i]; s += v * v; }
    s = wave_sum(s);
    const float k = rsqrtf(s / (float)L + eps);
    for (int i = lane; i < L; i += 64) out[(long long)p * L + i] = z[(long long)p * L + i] * k;
}
void launch_pixelnorm(const float* z, float* out, int P, int L, float eps, hipStream_t st) {
    hipLaunchKernelGGL(pixelnorm_kernel, dim3(P), dim3(64), 0, st, z, out, L, eps);
}

// ---- small-M fp32 dense: DenseLayer (modules.py:786-798) for the mapping network,
// the 26 style affines (one launch), demodulation coefficients, CLIP proj, D dense1.  The tile itself: dense_body.h.
__global__ __launch_bounds__(256) void dense_kernel(const float* x, int ldx, int P, int K, const float* wt,
                                                    int N, const float* bias, float* out, int ldo, int in_sq,
                                                    int mode, const float* eps_row, int eps_stride) {
    dense_body(x, ldx, P, K, wt, N, N, bias, out, ldo, in_sq, mode, eps_row, eps_stride, blockIdx.x, blockIdx.y);
}
// many independent small problems in ONE launch (blockIdx.z = problem): the 17 demodulation tables
__global__ __launch_bounds__(256) void dense_multi_kernel(const DenseDesc* d, int P, int in_sq, int mode) {
    const DenseDesc q = d[blockIdx.z];
    if ((int)blockIdx.x * 64 >= q.N) return;
    dense_body(q.x, q.ldx, P, q.K, q.wt, q.N, q.N, q.bias, q.out, q.ldo, in_sq, mode, q.eps_row, q.eps_stride, blockIdx.x,
               blockIdx.y);
}
void launch_dense_multi(const DenseDesc* d_desc, int n_desc, int max_N, int P, int in_sq, int mode, hipStream_t st) {
    dim3 g((max_N + 63) / 64, (P + DENSE_PB - 1) / DENSE_PB, n_desc);
    hipLaunchKernelGGL(dense_multi_kernel, g, dim3(256), 0, st, d_desc, P, in_sq, mode);
}
// Mapping-network layers (K = N = latent size, 16 candidates per workgroup): dense_body walks K in ONE chain per thread — 32
// batches of L2 round trips, 37 us per layer for 34 MFLOP.  Here the four waves of a workgroup each take a quarter of K for all
// 16 candidates (8 batches) and the partial sums meet in LDS: fixed order (q0 + q1) + (q2 + q3), independent of P.
__global__ __launch_bounds__(256) void dense_splitk_kernel(const float* x, int ldx, int P, int K, const float* wt, int N,
                                                           const float* bias, float* out, int ldo, int mode) {
    extern __shared__ float dsm[];
    float* xs = dsm;                          // [16][K]
    float* red = dsm + 16 * K;                // [4][16][64]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = blockIdx.x * 64 + lane, p0 = blockIdx.y * DENSE_PB;
    for (int e = t; e < DENSE_PB * K; e += 256) {
        const int pr = e / K, kk = e - pr * K;
        xs[e] = p0 + pr < P ? x[(long long)(p0 + pr) * ldx + kk] : 0.f;
    }
    __syncthreads();
    float acc[DENSE_PB];
#pragma unroll
    for (int j = 0; j < DENSE_PB; ++j) acc[j] = 0.f;
    const int kq = K >> 2, kb = wave * kq;
    const int nc = min(n, N - 1);
    for (int kk = 0; kk < kq; kk += 16) {
        float w[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) w[u] = wt[(long long)(kb + kk + u) * N + nc];
#pragma unroll
        for (int u = 0; u < 16; ++u)
#pragma unroll
            for (int j = 0; j < DENSE_PB; ++j) acc[j] = __builtin_fmaf(w[u], xs[j * K + kb + kk + u], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < DENSE_PB; ++j) red[(wave * DENSE_PB + j) * 64 + lane] = acc[j];
    __syncthreads();
    // 16 x 64 outputs, 4 per thread
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j = wave * 4 + u, p = p0 + j;
        float v = (red[(0 * DENSE_PB + j) * 64 + lane] + red[(1 * DENSE_PB + j) * 64 + lane]) +
                  (red[(2 * DENSE_PB + j) * 64 + lane] + red[(3 * DENSE_PB + j) * 64 + lane]);
        if (p >= P || n >= N) continue;
        v += bias ? bias[n] : 0.f;
        if (mode == 1) v = lrelu_sqrt2(v);
        out[(long long)p * ldo + n] = v;
    }
}
void launch_dense_splitk(const float* x, int ldx, int P, int K, const float* wt, int N, const float* bias, float* out, int ldo,
                         int mode, hipStream_t st) {
    const size_t lds = (size_t)(16 * K + 4 * 16 * 64) * sizeof(float);
    dim3 g((N + 63) / 64, (P + DENSE_PB - 1) / DENSE_PB);
    hipLaunchKernelGGL(dense_splitk_kernel, g, dim3(256), lds, st, x, ldx, P, K, wt, N, bias, out, ldo, mode);
}
// The whole mapping network (stylegan2/models.py:590-627: pixel norm + n_layers x [dense L -> L, bias, lrelu * sqrt2]) as ONE launch:
// eight dependent 34-MFLOP launches cost 35 us each (launch gap + ramp + an L2-latency-bound K walk).  A workgroup owns four
// candidates for all layers; its 16 waves each walk 1/16 of K for every output column (float4 columns per lane, 16 independent
// 16-byte loads in flight per thread), partial sums meet in LDS in a fixed order — a candidate's result does not depend on P.
struct MapDesc { const float* wt[8]; const float* b[8]; int n; };
template <int NC>   // L = 256 * NC
__global__ __launch_bounds__(1024) void mapping_fused_kernel(const float* z, float* out, int P, float eps, MapDesc d) {
    constexpr int L = 256 * NC, KQ = L / 16;
    extern __shared__ float msm[];
    float* xs = msm;                          // [4][L]
    float* red = msm + 4 * L;                 // [16][4][L]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int p0 = blockIdx.x * 4;
    if (wave < 4) {
        const int p = p0 + wave;
        float s = 0.f;
        for (int i = lane; i < L; i += 64) { const float v = p < P ? z[(long long)p * L + i] : 0.f; s += v * v; }
        s = wave_sum(s);
        const float k = rsqrtf(s / (float)L + eps);
        for (int i = lane; i < L; i += 64) xs[wave * L + i] = p < P ? z[(long long)p * L + i] * k : 0.f;
    }
    __syncthreads();
    const int kb = wave * KQ;
    for (int layer = 0; layer < d.n; ++layer) {
        const float* wt = d.wt[layer];
        f4 acc[4][NC];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[r][c] = f4{0.f, 0.f, 0.f, 0.f};
        for (int kk = 0; kk < KQ; kk += 8) {
            f4 w[8][NC];
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int c = 0; c < NC; ++c) w[u][c] = *(const f4*)(wt + (long long)(kb + kk + u) * L + (c * 64 + lane) * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f4 xa = *(const f4*)(xs + r * L + kb + kk), xb = *(const f4*)(xs + r * L + kb + kk + 4);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float xv = u < 4 ? xa[u & 3] : xb[u & 3];
#pragma unroll
                    for (int c = 0; c < NC; ++c) acc[r][c] = __builtin_elementwise_fma(w[u][c], f4{xv, xv, xv, xv}, acc[r][c]);   // (explicit FMA, as in dense_body)
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < NC; ++c) *(f4*)(red + (wave * 4 + r) * L + (c * 64 + lane) * 4) = acc[r][c];
        __syncthreads();
        float vout[(4 * L) / 1024];
#pragma unroll
        for (int j = 0; j < (4 * L) / 1024; ++j) {
            const int e = t + 1024 * j, r = e / L, n = e - r * L;
            float q[16];
#pragma unroll
            for (int w2 = 0; w2 < 16; ++w2) q[w2] = red[(w2 * 4 + r) * L + n];
#pragma unroll
            for (int st = 1; st < 16; st <<= 1)
#pragma unroll
                for (int w2 = 0; w2 < 16; w2 += 2 * st) q[w2] += q[w2 + st];          // fixed pairwise order
            vout[j] = lrelu_sqrt2(q[0] + d.b[layer][n]);
        }
        __syncthreads();                       // every partial sum has been read
#pragma unroll
        for (int j = 0; j < (4 * L) / 1024; ++j) xs[t + 1024 * j] = vout[j];
        __syncthreads();
    }
    for (int e = t; e < 4 * L; e += 1024) {
        const int r = e / L, n = e - r * L;
        if (p0 + r < P) out[(long long)(p0 + r) * L + n] = xs[e];
    }
}
bool launch_mapping_fused(const float* z, float* out, int P, int L, float eps, const float* const* wt, const float* const* b, int n_layers,
                          hipStream_t st) {
    if ((L != 256 && L != 512) || n_layers < 1 || n_layers > 8) return false;
    if (!glass_lds_fits((int)((4 + 64) * L * sizeof(float)))) return false;     // 136 KB at L = 512: per-layer path where the opt-in is smaller
    MapDesc d;
    d.n = n_layers;
    for (int i = 0; i < n_layers; ++i) { d.wt[i] = wt[i]; d.b[i] = b[i]; }
    const size_t lds = (size_t)(4 + 64) * L * sizeof(float);
    static DevOnce once;
    once.run([&] {
        (void)hipFuncSetAttribute((const void*)mapping_fused_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((4 + 64) * 256 * sizeof(float)));
        (void)hipFuncSetAttribute((const void*)mapping_fused_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((4 + 64) * 512 * sizeof(float)));
    });
    if (L == 256) hipLaunchKernelGGL(mapping_fused_kernel<1>, dim3((P + 3) / 4), dim3(1024), lds, st, z, out, P, eps, d);
    else hipLaunchKernelGGL(mapping_fused_kernel<2>, dim3((P + 3) / 4), dim3(1024), lds, st, z, out, P, eps, d);
    return true;
}
// D's head in one launch (stylegan2/models.py:1339-1350: dense CL -> CL + lrelu, dense CL -> 1): row p of the first layer is finished from
// its split-K slices (bias, lrelu * sqrt2) and goes straight into the second layer's dot product — one workgroup per candidate, block sum
// in a fixed order (lanes xor tree, then waves 0..3); the separate N = 1 dense launch walked K = 512 in one chain per thread (37 us).
__global__ __launch_bounds__(256) void dense01_finish_kernel(const float* part, int S, long long slab, const float* bias0, const float* w1,
                                                             const float* b1, float* out, int N) {
    __shared__ float red[4];
    const int p = blockIdx.x, t = threadIdx.x;
    float acc = 0.f;
    for (int n = t; n < N; n += 256) {
        float v = 0.f;
        for (int z0 = 0; z0 < S; z0 += 8) {      // eight slices' loads in flight together, added in slice order
            float pv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) pv[u] = z0 + u < S ? part[(long long)(z0 + u) * slab + (long long)p * N + n] : 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u) v += pv[u];
        }
        v = lrelu_sqrt2(v + (bias0 ? bias0[n] : 0.f));
        acc += v * w1[n];
    }
    acc = wave_sum(acc);
    if ((t & 63) == 0) red[t >> 6] = acc;
    __syncthreads();
    if (t == 0) out[p] = ((red[0] + red[1]) + (red[2] + red[3])) + (b1 ? b1[0] : 0.f);
}
void launch_dense01_finish(const float* part, int S, long long slab, const float* bias0, const float* w1, const float* b1, float* out, int P, int N,
                           hipStream_t st) {
    hipLaunchKernelGGL(dense01_finish_kernel, dim3(P), dim3(256), 0, st, part, S, slab, bias0, w1, b1, out, N);
}
void launch_dense(const float* x, int ldx, int P, int K, const float* wt, int N, const float* bias,
                  float* out, int ldo, int in_sq, int mode, const float* eps_row, int eps_stride,
                  hipStream_t st) {
    dim3 g((N + 63) / 64, (P + DENSE_PB - 1) / DENSE_PB);
    hipLaunchKernelGGL(dense_kernel, g, dim3(256), 0, st, x, ldx, P, K, wt, N, bias, out, ldo, in_sq, mode,
                       eps_row, eps_stride);
}

int launch_mapping(const float* z, float* w0, float* w1, int P, int L, float eps, const float* const* wt, const float* const* b, int n_layers,
                   int path, hipStream_t st) {
    if (path != 1 && n_layers >= 1 && launch_mapping_fused(z, w0, P, L, eps, wt, b, n_layers, st)) return MAP_FUSED;
    if (path == 2) return 0;
    int ran = MAP_PIXELNORM;
    launch_pixelnorm(z, w0, P, L, eps, st);
    float *a = w0, *o = w1;
    for (int i = 0; i < n_layers; ++i) {
        if (L % 64 == 0 && L <= 768) { launch_dense_splitk(a, L, P, L, wt[i], L, b[i], o, L, 1, st); ran |= MAP_SPLITK; }
        else { launch_dense(a, L, P, L, wt[i], L, b[i], o, L, 0, 1, nullptr, 0, st); ran |= MAP_DENSE; }
        std::swap(a, o);
    }
    if (a != w0)  // result must end in w0
        hipMemcpyAsync(w0, a, (size_t)P * L * sizeof(float), hipMemcpyDeviceToDevice, st);
    return ran;
}

// ---- style normalisation: keeps x*s inside fp16 range; exact algebra:
//   d*conv(x*s) == (d*smax) * conv(x * (s/smax)),  d*smax = rsqrt(sum (s/smax)^2 Wsq + eps/smax^2)
__global__ void style_norm_kernel(float* s, int ld, const int* off, const int* len, int n_layers, float* smax,
                                  float* eps_row, float eps) {
    const int p = blockIdx.x, l = blockIdx.y, lane = threadIdx.x;
    float* sp = s + (long long)p * ld + off[l];
    const int n = len[l];
    float m = 0.f;
    for (int i = lane; i < n; i += 64) m = fmaxf(m, fabsf(sp[i]));
    m = fmaxf(wave_max(m), 1e-20f);
    const float inv = 1.f / m;
    for (int i = lane; i < n; i += 64) sp[i] *= inv;
    if (lane == 0) {
        smax[(long long)p * n_layers + l] = m;
        eps_row[(long long)p * n_layers + l] = eps * inv * inv;
    }
}
void launch_style_norm(float* s, int ld, int P, int n_layers, const int* d_off, const int* d_len, float* smax,
                       float* eps_row, float eps, hipStream_t st) {
    hipLaunchKernelGGL(style_norm_kernel, dim3(P, n_layers), dim3(64), 0, st, s, ld, d_off, d_len, n_layers,
                       smax, eps_row, eps);
}

// ---- per-sample weights for the high-resolution layers: the reference's own formulation
// (modules.py:940-958: w * style, * demod), materialised once per pass where the weight
// tensor is tiny (<= ~1 MB); removes the modulation VALU work from the conv staging loop.
__global__ void modulate_weights_kernel(const half_t* w, long long elems, int Cin, int Cout, const float* sn,
                                        int sn_stride, const float* dscale, int ds_stride, half_t* wm) {
    const int b = blockIdx.y;
    const long long e8 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (e8 >= elems) return;
    const int i = (int)(e8 % Cin);
    const int o = (int)((e8 / Cin) % Cout);
    const h8 v = *(const h8*)(w + e8);
    const float d = dscale ? dscale[(long long)b * ds_stride + o] : 1.f;
    const float* s = sn + (long long)b * sn_stride + i;
    h8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (half_t)((float)v[j] * s[j] * d);
    *(h8*)(wm + (long long)b * elems + e8) = r;
}
void launch_modulate_weights(const half_t* w, long long elems, int Cin, int Cout, const float* sn, int sn_stride,
                              const float* dscale, int ds_stride, int P, half_t* wm, hipStream_t st) {
    dim3 g((unsigned)((elems / 8 + 255) / 256), P);
    hipLaunchKernelGGL(modulate_weights_kernel, g, dim3(256), 0, st, w, elems, Cin, Cout, sn, sn_stride, dscale,
                       ds_stride, wm);
}

// ---- noise planes: Philox4x32-10 (common.h) + Box-Muller (numpy mirror: clip_glass_amd/synth.py) --
// plane blockIdx.y is that of minibatch mb0 + blockIdx.y; period > 0 (include/glass.h "Device search: islands"): of (mb0 + blockIdx.y) % period
__global__ void noise_kernel(float* out, int hw, uint32_t layer, uint32_t mb0, uint32_t generation, uint32_t k0,
                             uint32_t k1, uint32_t period) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    const int nq = (hw + 3) / 4;
    if (q >= nq) return;
    const uint32_t mb = period ? (mb0 + blockIdx.y) % period : mb0 + blockIdx.y;
    uint32_t c[4] = {(uint32_t)q, layer, mb, generation};
    philox4x32_10(c, k0, k1);
    float u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] = ((float)c[j] + 0.5f) * 2.3283064365386963e-10f;
    float o[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float rad = sqrtf(-2.0f * logf(u[2 * j]));
        const float ang = 6.283185307179586f * u[2 * j + 1];
        o[2 * j] = rad * cosf(ang);
        o[2 * j + 1] = rad * sinf(ang);
    }
    float* op = out + (long long)blockIdx.y * hw;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (q * 4 + j < hw) op[q * 4 + j] = o[j];
}
void launch_noise(float* out, int n_mb, int hw, uint32_t layer, uint32_t mb0, uint32_t generation, uint64_t seed,
                  hipStream_t st, uint32_t period) {
    const int nq = (hw + 3) / 4;
    hipLaunchKernelGGL(noise_kernel, dim3((nq + 255) / 256, n_mb), dim3(256), 0, st, out, hw, layer, mb0,
                       generation, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), period);
}

// ---- toRGB (1x1 modulated conv, no demod: stylegan2/models.py:852-870) fused with the
// FIR-upsampled skip sum (models.py:1004-1013; Upsample.forward modules.py:580-602).
// Upsample taps (zero-insert, pad [3,1], 4x4 FIR*4): out[2m] = .75 x[m-1] + .25 x[m],
// out[2m+1] = .25 x[m-1] + .75 x[m]  (derived + checked in tests/test_host_math.py).
// Layout: LPP = C/8 lanes per pixel, each lane reads ONE 16-byte vector (8 channels), so a
// wave's loads are 1 KiB contiguous; the 3 partial dot products are reduced over the LPP
// lanes with xor-shuffles and lane 0 of the group writes the pixel (+ upsampled skip).
template <int LPP>
__global__ __launch_bounds__(256) void torgb_kernel(const half_t* x, int H, int W, int C, const float* wrgb,
                                                    const float* bias, const float* sn, int sn_stride,
                                                    const float* smax, int smax_stride, const float* yprev,
                                                    float* yout) {
    const int b = blockIdx.y;
    const int sub = threadIdx.x % LPP;                   // which 8-channel group of the pixel
    const float sm = smax[(long long)b * smax_stride];
    float w0[8], w1[8], w2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float s = sn[(long long)b * sn_stride + sub * 8 + j] * sm;
        w0[j] = wrgb[sub * 8 + j] * s;
        w1[j] = wrgb[C + sub * 8 + j] * s;
        w2[j] = wrgb[2 * C + sub * 8 + j] * s;
    }
    const int hw = H * W, h2 = H >> 1, w2_ = W >> 1;
    constexpr int PPB = 256 / LPP;                       // pixels per block per sub-step
    constexpr int U = 8;                                 // pixels per thread per iteration: U feature loads (+ 4 U skip
    const int cch = sub < 3 ? sub : 0;                   // taps on lanes 0..2 of a pixel) in flight, all unconditional
    const float bc = bias[cch];
    const float* yp = yprev ? yprev + ((long long)b * 3 + cch) * h2 * w2_ : nullptr;
    for (int base = blockIdx.x * PPB * U; base < hw; base += gridDim.x * PPB * U) {
        h8 v[U];
        float ys[U][4], wt[U][4];
        int pixv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int pix = base + u * PPB + threadIdx.x / LPP;
            pixv[u] = pix;
            const int pc = min(pix, hw - 1);
            v[u] = *(const h8*)(x + ((long long)b * hw + pc) * C + sub * 8);
            if (yp) {
                const int py = pc / W, px = pc - py * W;
                const int my = py >> 1, mx = px >> 1;
                const float wy0 = (py & 1) ? 0.25f : 0.75f, wx0 = (px & 1) ? 0.25f : 0.75f;
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int sy = my - 1 + dy, sx = mx - 1 + dx;
                        wt[u][dy * 2 + dx] = (sy >= 0 && sx >= 0) ? (dy ? 1.f - wy0 : wy0) * (dx ? 1.f - wx0 : wx0) : 0.f;
                        ys[u][dy * 2 + dx] = yp[max(sy, 0) * w2_ + max(sx, 0)];
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float f = (float)v[u][j];
                a0 += f * w0[j]; a1 += f * w1[j]; a2 += f * w2[j];
            }
#pragma unroll
            for (int o = LPP / 2; o > 0; o >>= 1) {
                a0 += __shfl_xor(a0, o); a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o);
            }
            float r = (cch == 0 ? a0 : cch == 1 ? a1 : a2) + bc;   // lane c of the pixel finishes output channel c
            if (yp) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) s += wt[u][q] * ys[u][q];
                r += s;
            }
            if (sub < 3 && pixv[u] < hw) yout[((long long)b * 3 + sub) * hw + pixv[u]] = r;
        }
    }
}
// Thread-per-pixel variant: best for C <= 64 (a pixel's channels are <= 128 contiguous bytes).  C is a template
// parameter so the pixel's C/8 16-byte loads are all issued before the first use (a runtime loop keeps ONE load in
// flight per thread), and the skip-image taps are unconditional (clamped index, zero weight) for the same reason.
template <int C>
__global__ __launch_bounds__(256) void torgb_pix_kernel(const half_t* x, int H, int W, const float* wrgb,
                                                        const float* bias, const float* sn, int sn_stride,
                                                        const float* smax, int smax_stride, const float* yprev,
                                                        float* yout) {
    __shared__ float wl[3 * C];  // modulated weights of this sample
    const int b = blockIdx.y;
    const float sm = smax[(long long)b * smax_stride];
    for (int e = threadIdx.x; e < 3 * C; e += 256) wl[e] = wrgb[e] * sn[(long long)b * sn_stride + e % C] * sm;
    __syncthreads();
    const int hw = H * W;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const half_t* xp = x + ((long long)b * hw + pix) * C;
    h8 v[C / 8];
#pragma unroll
    for (int i = 0; i < C / 8; ++i) v[i] = *(const h8*)(xp + i * 8);
    float ys[3][4];      // skip-image taps (previous resolution), fetched alongside
    float wt[4];
    if (yprev) {
        const int py = pix / W, px = pix - py * W;
        const int h2 = H >> 1, w2_ = W >> 1;
        const int my = py >> 1, mx = px >> 1;
        const float wy0 = (py & 1) ? 0.25f : 0.75f, wx0 = (px & 1) ? 0.25f : 0.75f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int sy = my - 1 + dy, sx = mx - 1 + dx;
                wt[dy * 2 + dx] = (sy >= 0 && sx >= 0) ? (dy ? 1.f - wy0 : wy0) * (dx ? 1.f - wx0 : wx0) : 0.f;
                const int off = max(sy, 0) * w2_ + max(sx, 0);
#pragma unroll
                for (int c = 0; c < 3; ++c) ys[c][dy * 2 + dx] = yprev[((long long)b * 3 + c) * h2 * w2_ + off];
            }
    }
    float r[3] = {bias[0], bias[1], bias[2]};
#pragma unroll
    for (int i = 0; i < C / 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = (float)v[i][j];
            r[0] += f * wl[i * 8 + j]; r[1] += f * wl[C + i * 8 + j]; r[2] += f * wl[2 * C + i * 8 + j];
        }
    if (yprev) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float s = 0.f;   // same accumulation order as before: (dy, dx) = (0,0), (0,1), (1,0), (1,1)
#pragma unroll
            for (int q = 0; q < 4; ++q) s += wt[q] * ys[c][q];
            r[c] += s;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) yout[((long long)b * 3 + c) * hw + pix] = r[c];
}
template <int LPP>
static void launch_torgb_t(const half_t* x, int B, int H, int W, int C, const float* wrgb, const float* bias,
                           const float* sn, int sn_stride, const float* smax, int smax_stride, const float* yprev,
                           float* yout, hipStream_t st) {
    const int ppb = (256 / LPP) * 8;                     // U = 8 pixels per thread per iteration
    int gx = (H * W + ppb - 1) / ppb;
    if (gx > 2048) gx = 2048;                            // grid-stride the rest
    hipLaunchKernelGGL(torgb_kernel<LPP>, dim3(gx, B), dim3(256), 0, st, x, H, W, C, wrgb, bias, sn, sn_stride, smax,
                       smax_stride, yprev, yout);
}
bool launch_torgb(const half_t* x, int B, int H, int W, int C, const float* wrgb, const float* bias,
                  const float* sn, int sn_stride, const float* smax, int smax_stride, const float* yprev,
                  float* yout, hipStream_t st) {
#define TORGB_PIX(CC) if (C == CC) { hipLaunchKernelGGL(torgb_pix_kernel<CC>, dim3((H * W + 255) / 256, B), dim3(256), 0, st, x, H, W, \
                                                       wrgb, bias, sn, sn_stride, smax, smax_stride, yprev, yout); return true; }
    TORGB_PIX(16) TORGB_PIX(32) TORGB_PIX(64)
#undef TORGB_PIX
#define TORGB_CASE(L) case L: launch_torgb_t<L>(x, B, H, W, C, wrgb, bias, sn, sn_stride, smax, smax_stride, yprev, yout, st); break;
    if (C % 8 != 0) return false;
    switch (C / 8) {      // (C = 16, 32, 64 left above: lanes-per-pixel instances below 16 lanes would be unreachable)
        TORGB_CASE(16) TORGB_CASE(32) TORGB_CASE(64)
        default: return false;  // not instantiated (the engine checks its channel widths at creation; the diagnostic ABI reports it)
    }
#undef TORGB_CASE
    return true;
}

// toRGB weight tables for the fused conv epilogues (common.h: trgb_channel / trgb_table_value): [B][2][16][NT] fp16
__global__ __launch_bounds__(256) void trgb_tables_kernel(const float* wrgb, const float* sn, int sn_stride, const float* smax,
                                                          int smax_stride, int NT, half_t* tab) {
    const int b = blockIdx.x;
    const float sm = smax[(long long)b * smax_stride];
    for (int e = threadIdx.x; e < 32 * NT; e += 256) {
        const int tsel = e / (16 * NT), n = (e / NT) & 15, hidx = e % NT;
        const int ch = trgb_channel(hidx), c = n & 3;
        const float w = c < 3 ? wrgb[c * NT + ch] * sn[(long long)b * sn_stride + ch] * sm : 0.f;
        tab[(long long)b * 32 * NT + e] = trgb_table_value(tsel, n, w);
    }
}
void launch_trgb_tables(const float* wrgb, const float* sn, int sn_stride, const float* smax, int smax_stride, int B, int NT,
                        half_t* tab, hipStream_t st) {
    hipLaunchKernelGGL(trgb_tables_kernel, dim3(B), dim3(256), 0, st, wrgb, sn, sn_stride, smax, smax_stride, NT, tab);
}

// toRGB partial sums -> skip image (stylegan2/models.py:852-870, modules.py:580-602): y = bias + sum over the layer's 128-wide n tiles (in
// n-tile order: deterministic) of the conv epilogues' partial sums + the FIR-upsampled previous image.  3 floats per pixel in and out per
// tile instead of the separate toRGB pass's read of the whole feature map.
__global__ __launch_bounds__(256) void trgb_finish_kernel(const float* part, int ntn, int B, int R, const float* bias, const float* yprev, float* yout) {
    const long long hw = (long long)R * R, n = (long long)B * 3 * hw;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int px = (int)(i % R), py = (int)((i / R) % R), c = (int)((i / hw) % 3);
    const long long b = i / (3 * hw);
    float r = bias[c];
    for (int t = 0; t < ntn; ++t) r += part[(long long)t * n + i];
    if (yprev) {
        const int h2 = R >> 1, my = py >> 1, mx = px >> 1;
        const float* yp = yprev + (b * 3 + c) * (long long)h2 * h2;
        float tap[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) tap[q] = yp[(long long)max(my - 1 + (q >> 1), 0) * h2 + max(mx - 1 + (q & 1), 0)];
        r += trgb_skip(tap, py, px);
    }
    yout[i] = r;
}
void launch_trgb_finish(const float* part, int ntn, int B, int R, const float* bias, const float* yprev, float* yout, hipStream_t st) {
    const long long n = (long long)B * 3 * R * R;
    hipLaunchKernelGGL(trgb_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, ntn, B, R, bias, yprev, yout);
}

// ---- biggan_norm: utils.py:14-17 ---------------------------------------------------
__global__ void finalize_image_kernel(const float* y, float* img, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) img[i] = fminf(fmaxf((y[i] + 1.f) * 0.5f, 0.f), 1.f);
}
void launch_finalize_image(const float* y, float* img, long long n, hipStream_t st) {
    hipLaunchKernelGGL(finalize_image_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, y, img, n);
}

// ---- kornia.resize(x,(224,224)) (generator.py:45) on biggan_norm(y), written straight
// into the patch-embedding GEMM operand: row = b*G*G + gy*G + gx, col = c*ps*ps + iy*ps + ix
// (conv1.weight.reshape(width, -1) order, clip/model.py:206,219).  ld = elements per row (>= 3 ps ps: the engine pads its rows to the
// GEMM's K step and keeps the tail zero).
__global__ void resize_patches_kernel(const float* y, int B, int R, int S, int ps, int ld, half_t* patches) {
    const int G = S / ps;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // over b, c, Y, X
    const int X = (int)(idx % S);
    const int Y = (int)((idx / S) % S);
    const int c = (int)((idx / ((long long)S * S)) % 3);
    const int b = (int)(idx / ((long long)S * S * 3));
    if (b >= B) return;
    const float scale = (float)R / (float)S;
    float sy = scale * ((float)Y + 0.5f) - 0.5f, sx = scale * ((float)X + 0.5f) - 0.5f;
    sy = fmaxf(sy, 0.f); sx = fmaxf(sx, 0.f);
    const int y0 = min((int)sy, R - 1), x0 = min((int)sx, R - 1);
    const int y1 = min(y0 + 1, R - 1), x1 = min(x0 + 1, R - 1);
    const float ly = sy - (float)y0, lx = sx - (float)x0;
    const float* yp = y + ((long long)b * 3 + c) * R * R;
    auto nrm = [](float v) { return fminf(fmaxf((v + 1.f) * 0.5f, 0.f), 1.f); };
    const float v00 = nrm(yp[(long long)y0 * R + x0]), v01 = nrm(yp[(long long)y0 * R + x1]);
    const float v10 = nrm(yp[(long long)y1 * R + x0]), v11 = nrm(yp[(long long)y1 * R + x1]);
    const float v = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
    const int gy = Y / ps, iy = Y - gy * ps, gx = X / ps, ix = X - gx * ps;
    const long long row = ((long long)b * G + gy) * G + gx;
    patches[row * ld + ((long long)c * ps + iy) * ps + ix] = (half_t)v;
}
void launch_resize_patches(const float* y, int B, int R, int clip_res, int ps, int ld, half_t* patches, hipStream_t st) {
    const long long n = 3LL * clip_res * clip_res;  // per image
    const long long total = n * B;
    hipLaunchKernelGGL(resize_patches_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, y, B, R,
                       clip_res, ps, ld, patches);
}

// ---- CLIP's own preprocessing (clip/clip.py:68-74), opt-in: glass_config::clip_resize / clip_normalize -----------------
// Normalize((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)), clip/clip.py:73
__device__ __forceinline__ float clip_normalize_px(float v, int c) {
    const float mean = c == 0 ? 0.48145466f : c == 1 ? 0.4578275f : 0.40821073f;
    const float std = c == 0 ? 0.26862954f : c == 1 ? 0.26130258f : 0.27577711f;
    return (v - mean) / std;
}
// clip_resize 0 with clip_normalize 1: resize_patches_kernel's arithmetic, then Normalize before the fp16 store
__global__ void resize_patches_norm_kernel(const float* y, int B, int R, int S, int ps, int ld, half_t* patches) {
    const int G = S / ps;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;  // over b, c, Y, X
    const int X = (int)(idx % S);
    const int Y = (int)((idx / S) % S);
    const int c = (int)((idx / ((long long)S * S)) % 3);
    const int b = (int)(idx / ((long long)S * S * 3));
    if (b >= B) return;
    const float scale = (float)R / (float)S;
    float sy = scale * ((float)Y + 0.5f) - 0.5f, sx = scale * ((float)X + 0.5f) - 0.5f;
    sy = fmaxf(sy, 0.f); sx = fmaxf(sx, 0.f);
    const int y0 = min((int)sy, R - 1), x0 = min((int)sx, R - 1);
    const int y1 = min(y0 + 1, R - 1), x1 = min(x0 + 1, R - 1);
    const float ly = sy - (float)y0, lx = sx - (float)x0;
    const float* yp = y + ((long long)b * 3 + c) * R * R;
    auto nrm = [](float v) { return fminf(fmaxf((v + 1.f) * 0.5f, 0.f), 1.f); };
    const float v00 = nrm(yp[(long long)y0 * R + x0]), v01 = nrm(yp[(long long)y0 * R + x1]);
    const float v10 = nrm(yp[(long long)y1 * R + x0]), v11 = nrm(yp[(long long)y1 * R + x1]);
    const float v = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
    const int gy = Y / ps, iy = Y - gy * ps, gx = X / ps, ix = X - gx * ps;
    const long long row = ((long long)b * G + gy) * G + gx;
    patches[row * ld + ((long long)c * ps + iy) * ps + ix] = (half_t)clip_normalize_px(v, c);
}

// ---- crop views (opt-in: glass_engine_set_clip_views): resize_patches_kernel's resize applied to the crop [y0, y0 + s) x [x0, x0 + s) of image b,
// F.interpolate(img01[:, :, y0:y0+s, x0:x0+s], (S, S), "bilinear", align_corners=False), mirrored left-right where flip is set, written to
// the patch rows of (image b, view v).  A workgroup works on ONE (image, view): the box is four scalars.  One thread = one output pixel of all
// three channels: the coordinates are computed once and the twelve loads go out as one unconditional batch (a thread past the last pixel
// reads the last pixel's taps and stores nothing).  The coordinates are the crop's own, so with the box (0, 0, R, 0) every expression is
// resize_patches_kernel's — rounded where the compiler rounds that kernel's — and the values are equal bit for bit.
__global__ __launch_bounds__(256) void view_patches_kernel(const float* y, int R, int S, int ps, int ld, int normalize, int V, int nb, ViewBoxes vb,
                                                           half_t* patches) {
    const int G = S / ps;
    const int bv = blockIdx.x / nb, b = bv / V, v = bv - b * V;      // uniform
    const int bx0 = vb.box[v][0], by0 = vb.box[v][1], bs = vb.box[v][2], flip = vb.box[v][3];
    const int idx = (blockIdx.x - bv * nb) * 256 + threadIdx.x;
    const int pix = min(idx, S * S - 1);
    const int Y = pix / S, X = pix - Y * S;
    const int Xs = flip ? S - 1 - X : X;             // out[X] = unflipped[S - 1 - X]
    const float scale = (float)bs / (float)S;
    float sy = __fmaf_rn(scale, (float)Y + 0.5f, -0.5f), sx = __fmaf_rn(scale, (float)Xs + 0.5f, -0.5f);      // scale (i + 0.5) - 0.5, fused as it is there
    sy = fmaxf(sy, 0.f); sx = fmaxf(sx, 0.f);
    const int y0 = min((int)sy, bs - 1), x0 = min((int)sx, bs - 1);
    const int y1 = min(y0 + 1, bs - 1), x1 = min(x0 + 1, bs - 1);
    const float ly = sy - (float)y0, lx = sx - (float)x0;
    const float* yp = y + (long long)b * 3 * R * R;
    const long long o00 = (long long)(by0 + y0) * R + bx0 + x0, o01 = (long long)(by0 + y0) * R + bx0 + x1;
    const long long o10 = (long long)(by0 + y1) * R + bx0 + x0, o11 = (long long)(by0 + y1) * R + bx0 + x1;
    float t[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* yc = yp + (long long)c * R * R;
        t[c][0] = yc[o00]; t[c][1] = yc[o01]; t[c][2] = yc[o10]; t[c][3] = yc[o11];
    }
    if (idx >= S * S) return;
    auto nrm = [](float v) { return fminf(fmaxf((v + 1.f) * 0.5f, 0.f), 1.f); };
    const int gy = Y / ps, iy = Y - gy * ps, gx = X / ps, ix = X - gx * ps;
    const long long row = ((long long)bv * G + gy) * G + gx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v00 = nrm(t[c][0]), v01 = nrm(t[c][1]);
        const float v10 = nrm(t[c][2]), v11 = nrm(t[c][3]);
        // v = (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11), with the roundings spelled out as the compiler contracts that
        // expression in resize_patches_kernel (one fused product per row — the lx term above, the 1 - lx term below — and a plain sum of the
        // two rounded row products): left to itself it contracts this loop differently, and the whole-image view must equal the default
        // pass to the bit (tests/test_gpu_clip_views.py holds the two kernels against each other)
        const float top = __fmaf_rn(lx, v01, __fmul_rn(1.f - lx, v00));
        const float bot = __fmaf_rn(1.f - lx, v10, __fmul_rn(lx, v11));
        const float v = __fadd_rn(__fmul_rn(1.f - ly, top), __fmul_rn(ly, bot));
        patches[row * ld + ((long long)c * ps + iy) * ps + ix] = (half_t)(normalize ? clip_normalize_px(v, c) : v);
    }
}
bool view_boxes_valid(const ViewBoxes& vb, int V, int R) {
    if (V < 1 || V > GLASS_MAX_CLIP_VIEWS) return false;
    for (int v = 0; v < V; ++v) {
        const int x0 = vb.box[v][0], y0 = vb.box[v][1], s = vb.box[v][2], flip = vb.box[v][3];
        if (x0 < 0 || y0 < 0 || s < 1 || s > R || x0 > R - s || y0 > R - s || (flip != 0 && flip != 1)) return false;
    }
    return true;
}
void launch_view_patches(const float* y, int B, int R, int clip_res, int ps, int ld, int normalize, int V, const ViewBoxes& vb, half_t* patches,
                         hipStream_t st) {
    const int nb = (clip_res * clip_res + 255) / 256;      // workgroups per (image, view)
    hipLaunchKernelGGL(view_patches_kernel, dim3((unsigned)((long long)B * V * nb)), dim3(256), 0, st, y, R, clip_res, ps, ld, normalize, V, nb, vb,
                       patches);
}

// The tap table of one axis of an antialiased resize R -> S, as torch's upsample_bilinear2d_aa / upsample_bicubic2d_aa build it
// (align_corners = False): scale = R / S, m = max(scale, 1), support = r m (r = 1 triangle, 2 cubic with a = -0.5); for output i:
// c = scale (i + 0.5), taps j in [max(int(c - support + 0.5), 0), min(int(c + support + 0.5), R)) with weight f((j - c + 0.5) / m),
// divided by their sum.  Computed in float64, stored as fp32; both axes use the same table (the images are square).
bool build_resize_taps(int R, int S, int mode, ResizeTaps& t, std::string& why) {
    char msg[256];
    if (mode != 1 && mode != 2) {
        why = "clip_resize must be 0 (point-sampled bilinear), 1 (antialiased bilinear) or 2 (antialiased bicubic)";
        return false;
    }
    if (R <= 0 || S <= 0 || R % 4 != 0 || R > PREPROCESS_MAX_R) {
        snprintf(msg, sizeof msg, "antialiased resize %d -> %d: the image size must be a positive multiple of 4, at most %d", R, S, PREPROCESS_MAX_R);
        why = msg;
        return false;
    }
    const double scale = (double)R / (double)S, m = scale > 1.0 ? scale : 1.0, support = (mode == 2 ? 2.0 : 1.0) * m;
    auto f = [mode](double u) {
        u = u < 0 ? -u : u;
        if (mode == 1) return u < 1.0 ? 1.0 - u : 0.0;
        const double a = -0.5;
        if (u < 1.0) return ((a + 2.0) * u - (a + 3.0)) * u * u + 1.0;
        if (u < 2.0) return (((u - 5.0) * u + 8.0) * u - 4.0) * a;
        return 0.0;
    };
    t.start.assign(S, 0);
    t.count.assign(S, 0);
    t.taps.assign((size_t)S * GLASS_RESIZE_MAX_TAPS, 0.f);
    t.max_count = 0;
    for (int i = 0; i < S; ++i) {
        const double c = scale * (i + 0.5);
        const int lo = std::max((int)(c - support + 0.5), 0), hi = std::min((int)(c + support + 0.5), R), n = hi - lo;
        if (n < 1 || n > GLASS_RESIZE_MAX_TAPS) {
            snprintf(msg, sizeof msg, "antialiased resize %d -> %d (clip_resize %d) needs %d taps per output pixel: at most %d are supported", R, S,
                     mode, n, GLASS_RESIZE_MAX_TAPS);
            why = msg;
            return false;
        }
        double w[GLASS_RESIZE_MAX_TAPS], sum = 0.0;
        for (int j = 0; j < n; ++j) sum += (w[j] = f((lo + j - c + 0.5) / m));
        for (int j = 0; j < n; ++j) t.taps[(size_t)i * GLASS_RESIZE_MAX_TAPS + j] = (float)(w[j] / sum);
        t.start[i] = lo;
        t.count[i] = n;
        t.max_count = std::max(t.max_count, n);
    }
    // input rows a band of PREPROCESS_TY output rows reads, rounded up to whole load batches
    t.nr = 0;
    for (int y0 = 0; y0 < S; y0 += PREPROCESS_TY) {
        const int yl = std::min(y0 + PREPROCESS_TY, S) - 1;
        t.nr = std::max(t.nr, t.start[yl] + t.count[yl] - t.start[y0]);
    }
    t.nr = (t.nr + 2 * PREPROCESS_RB - 1) / (2 * PREPROCESS_RB) * (2 * PREPROCESS_RB);
    t.ts = t.max_count | 1;      // odd LDS row stride of the taps: neighbouring outputs' taps fall into different banks
    // the image the kernel copies into LDS as it is: taps [S][ts], start [S], count [S] (int bits), padded to whole 16-byte vectors
    t.table.assign(((size_t)S * t.ts + 2 * (size_t)S + 3) / 4 * 4, 0.f);
    for (int i = 0; i < S; ++i) {
        for (int k = 0; k < t.count[i]; ++k) t.table[(size_t)i * t.ts + k] = t.taps[(size_t)i * GLASS_RESIZE_MAX_TAPS + k];
        memcpy(&t.table[(size_t)S * t.ts + i], &t.start[i], sizeof(int));
        memcpy(&t.table[(size_t)S * t.ts + S + i], &t.count[i], sizeof(int));
    }
    t.lds_bytes = sizeof(float) * (t.table.size() + (size_t)PREPROCESS_TY * R + (size_t)t.nr * PREPROCESS_TY);
    if (t.lds_bytes > 64 * 1024) {
        snprintf(msg, sizeof msg, "antialiased resize %d -> %d (clip_resize %d): the kernel's tables need %zu bytes of LDS, more than 64 KB", R, S, mode,
                 t.lds_bytes);
        why = msg;
        return false;
    }
    return true;
}

// Antialiased bilinear / bicubic resize of clip((y+1)/2, 0, 1) [B][3][R][R] into the patch matrix, optionally CLIP-normalised.  Unlike
// resize_patches_kernel it reads EVERY input pixel, so it is an HBM stream (unconditional batched 16-byte loads, the next
// batch issued before the current one is consumed, the tap tables in LDS).  A workgroup owns PREPROCESS_TY output rows of one (image, channel)
// plane.  Vertical pass first, in registers: thread t holds columns 4t .. 4t+3, streams the band's input rows and accumulates all
// PREPROCESS_TY output rows against a dense weight matrix Wt[input row][output row] (zero outside a row's support; wave-uniform broadcast
// reads from LDS).  The band's PREPROCESS_TY x R fp32 rows then go through LDS for the horizontal pass, one thread per output pixel.
// The halo rows two neighbouring bands share are read twice; the block index is re-dealt so that neighbours run back to back on one XCD and
// the second read comes from its L2.
struct PreprocessParams {
    const float* y;
    const float* table;    // ResizeTaps::table, n4 16-byte vectors
    int B, R, S, ps, ld, n4, ts, clamp01, normalize;
    half_t* patches;
};
__global__ __launch_bounds__(256) void preprocess_patches_kernel(PreprocessParams p) {
    extern __shared__ __align__(16) float pp_lds[];
    constexpr int TY = PREPROCESS_TY, RB = PREPROCESS_RB;
    static_assert(TY == 8, "the vertical pass reads a row's weights as two 16-byte vectors");
    const int R = p.R, S = p.S, nt = blockDim.x, tid = threadIdx.x;
    float* tl = pp_lds;                        // [S][ts] taps
    const int* sl = (const int*)(tl + S * p.ts);     // start [S], count [S]
    float* tmp = pp_lds + p.n4 * 4;            // [TY][R] vertically reduced rows
    float* Wt = tmp + TY * R;                  // [input row of the band][TY]
    // blocks i, i + 8, i + 16 ... share an XCD: give each XCD a contiguous run of (plane, band) indices
    const int n = gridDim.x, q = n >> 3, rem = n & 7, xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int L = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + slot;
    const int nb = (S + TY - 1) / TY;
    const int band = L % nb, plane = L / nb, Y0 = band * TY;
    const int r0 = __float_as_int(p.table[S * p.ts + Y0]);
    const float* src = p.y + (long long)plane * R * R + min(tid * 4, R - 4);
    auto load = [&](int it, f4* v) {
#pragma unroll
        for (int j = 0; j < RB; ++j) v[j] = *(const f4*)(src + (long long)min(r0 + it * RB + j, R - 1) * R);
    };
    f4 a[RB], b[RB];
    load(0, a);
    for (int e0 = 0; e0 < p.n4; e0 += 4 * nt) {      // the table, four independent 16-byte loads per thread and round
        f4 tv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) tv[u] = ((const f4*)p.table)[min(e0 + u * nt + tid, p.n4 - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e0 + u * nt + tid < p.n4) ((f4*)pp_lds)[e0 + u * nt + tid] = tv[u];
    }
    __syncthreads();
    const int Yl = min(Y0 + TY, S) - 1;
    const int nit = (sl[Yl] + sl[S + Yl] - r0 + RB - 1) / RB;      // load batches of this band
    const int nit2 = (nit + 1) & ~1;                               // (the loop below takes two per round; 2 RB | nr, so nit2 RB <= nr)
    for (int e = tid; e < nit2 * RB * TY; e += nt) {
        const int j = e / TY, Y = Y0 + (e % TY);
        float w = 0.f;
        if (Y < S) {
            const int k = r0 + j - sl[Y];
            if (k >= 0 && k < sl[S + Y]) w = tl[Y * p.ts + k];
        }
        Wt[e] = w;
    }
    __syncthreads();
    f4 acc[TY];
#pragma unroll
    for (int yy = 0; yy < TY; ++yy) acc[yy] = f4{0.f, 0.f, 0.f, 0.f};
    auto consume = [&](int it, const f4* v8) {
#pragma unroll
        for (int j = 0; j < RB; ++j) {
            f4 v = (v8[j] + 1.f) * 0.5f;       // biggan_norm on load (utils.py:14-17)
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = fminf(fmaxf(v[u], 0.f), 1.f);
            const f4 w0 = *(const f4*)(Wt + (it * RB + j) * TY), w1 = *(const f4*)(Wt + (it * RB + j) * TY + 4);
#pragma unroll
            for (int yy = 0; yy < 4; ++yy) {
                acc[yy] += w0[yy] * v;
                acc[yy + 4] += w1[yy] * v;
            }
        }
    };
    // two register sets in turn, the next batch issued before the current one is consumed; every load is unconditional (row index
    // clamped: rows past the band carry zero weights, and the last round re-reads rows it already has, which hit the cache)
    for (int it = 0; it < nit2; it += 2) {
        load(it + 1, b);
        __builtin_amdgcn_sched_barrier(0);     // (the scheduler otherwise sinks the batch below the arithmetic it is meant to run under)
        consume(it, a);
        __builtin_amdgcn_sched_barrier(0);
        load(it + 2, a);
        __builtin_amdgcn_sched_barrier(0);
        consume(it + 1, b);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (tid * 4 < R) {
#pragma unroll
        for (int yy = 0; yy < TY; ++yy) *(f4*)(tmp + yy * R + tid * 4) = acc[yy];
    }
    __syncthreads();
    const int G = S / p.ps, c = plane % 3, img = plane / 3;
    for (int o = tid; o < TY * S; o += nt) {
        const int yy = o / S, X = o - yy * S, Y = Y0 + yy;
        if (Y >= S) break;
        const int cn = sl[S + X];
        const float* row = tmp + yy * R + sl[X];
        const float* t = tl + X * p.ts;
        float s = 0.f;
        for (int k = 0; k < cn; ++k) s += row[k] * t[k];
        if (p.clamp01) s = fminf(fmaxf(s, 0.f), 1.f);
        if (p.normalize) s = clip_normalize_px(s, c);
        const int gy = Y / p.ps, iy = Y - gy * p.ps, gx = X / p.ps, ix = X - gx * p.ps;
        const long long prow = ((long long)img * G + gy) * G + gx;
        p.patches[prow * p.ld + ((long long)c * p.ps + iy) * p.ps + ix] = (half_t)s;
    }
}
void launch_preprocess_patches(const float* y, int B, int R, int clip_res, int ps, int ld, int resize_mode, int normalize,
                               const ResizeTapsDev& t, half_t* patches, hipStream_t st) {
    if (resize_mode == 0) {
        const long long total = 3LL * clip_res * clip_res * B;
        hipLaunchKernelGGL(resize_patches_norm_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, y, B, R, clip_res, ps, ld, patches);
        return;
    }
    PreprocessParams p;
    p.y = y; p.table = t.table;
    p.B = B; p.R = R; p.S = clip_res; p.ps = ps; p.ld = ld; p.n4 = t.n4; p.ts = t.ts;
    p.clamp01 = resize_mode == 2; p.normalize = normalize;
    p.patches = patches;
    const int nb = (clip_res + PREPROCESS_TY - 1) / PREPROCESS_TY;
    const int nt = std::min(256, (R / 4 + 63) / 64 * 64);     // one thread per four columns (R <= PREPROCESS_MAX_R = 1024)
    hipLaunchKernelGGL(preprocess_patches_kernel, dim3((unsigned)(B * 3 * nb)), dim3(nt), t.lds_bytes, st, p);
}

// ---- D fromRGB: biggan_denorm (utils.py:19-21) + 1x1 conv 3->C + bias + lrelu*sqrt2
// (stylegan2/models.py:1125-1143).  One thread per pixel, 16-byte NHWC stores.
__global__ __launch_bounds__(256) void fromrgb_kernel(const float* y, int hw, int Cout, const float* w,
                                                      const float* bias, half_t* out) {
    extern __shared__ float wl[];  // [Cout][3], bias[Cout], then the per-wave output image [4][64 px][Cout*2 + 16 B]
    for (int e = threadIdx.x; e < Cout * 3; e += 256) wl[e] = w[e];
    for (int e = threadIdx.x; e < Cout; e += 256) wl[Cout * 3 + e] = bias[e];
    __syncthreads();
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pix0 = blockIdx.x * 256 + wave * 64;             // first pixel of this wave
    const int pix = min(pix0 + lane, hw - 1);
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float n = fminf(fmaxf((y[((long long)b * 3 + c) * hw + pix] + 1.f) * 0.5f, 0.f), 1.f);
        v[c] = n * 2.f - 1.f;
    }
    // one thread computes all channels of its pixel; the wave's 64 x Cout block goes through LDS and leaves as
    // 16-byte vectors in row order (whole 64-byte lines per store instruction instead of 64 scattered pieces)
    const int orow = Cout * 2 + 16;
    char* Os = (char*)(wl + Cout * 4) + wave * 64 * orow;
    for (int o = 0; o < Cout; o += 8) {
        h8 r;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float* wp = wl + (o + j) * 3;
            r[j] = (half_t)lrelu_sqrt2(wp[0] * v[0] + wp[1] * v[1] + wp[2] * v[2] + wl[Cout * 3 + o + j]);
        }
        *(h8*)(Os + lane * orow + o * 2) = r;
    }
    __builtin_amdgcn_wave_barrier();
    const int cg = Cout >> 3;
    half_t* ob = out + ((long long)b * hw + pix0) * Cout;
    for (int u = lane; u < 64 * cg; u += 64) {
        const int p = u / cg, g = u - p * cg;
        if (pix0 + p < hw) *(h8*)(ob + (long long)p * Cout + g * 8) = *(const h8*)(Os + p * orow + g * 16);
    }
}
void launch_fromrgb(const float* y, int B, int R, int Cout, const float* w, const float* bias, half_t* out,
                    hipStream_t st) {
    const int hw = R * R;
    const size_t lds = Cout * 4 * sizeof(float) + 4 * 64 * (Cout * 2 + 16);
    hipLaunchKernelGGL(fromrgb_kernel, dim3((hw + 255) / 256, B), dim3(256), lds, st, y, hw, Cout, w, bias, out);
}

// ---- FIR filters of the D down path (modules.py:1204-1220, 499-523) -----------------
// separable [1,3,3,1]/8 per axis; thread = (pixel, 8-channel group).
// Each thread owns one (output column, 8-channel group) and walks RS output rows with a
// sliding window: per input row 4 loads -> horizontal sum, the last 4 horizontal sums ->
// vertical sum.  (RS + 3) * 4 loads per RS outputs instead of 16 per output.
template <int PAD, int STRIDE, int RS>
__global__ __launch_bounds__(256) void blur_kernel(const half_t* x, int H, int W, int C, int Ho, int Wo,
                                                   half_t* out, int planar32) {
    const int cg = C >> 3;
    const int idx = blockIdx.x * 256 + threadIdx.x;      // over (ox, channel group)
    if (!planar32 && idx >= Wo * cg) return;
    const int b = blockIdx.z;
    // thread -> (output column, 8-channel group): groups fastest (a wave loads and stores 1 KB of consecutive pixels' channels).
    // 32-channel-plane output, measured per channel count (us per launch, pixel-major output = 774 / 410 / 224 / 136 at C = 64 / 128 / 256 / 512):
    //   groups fastest (stores of 64-byte pieces into 2 .. 16 planes):                        830 / 453 / 268 / 172
    //   the workgroup's columns and groups re-dealt inside it, a plane's four groups fastest
    //   (a wave stores consecutive pixels of ONE plane, loads 64-byte pieces of each pixel):    937 / 494 / 230 / 139
    //   planes dealt over the whole grid:                                                       942 / 533 / 277 / 149
    // -> the first form for C <= 128, the second from 256 channels on.
    int g = idx % cg, ox = idx / cg;
    if (planar32 && idx >= Wo * cg && cg < 32) return;
    if (planar32 && cg >= 32) {
        const int P = 256 / cg;                 // columns of this workgroup (cg divides 256: C is a power of two here; checked by the launcher)
        const int t = threadIdx.x, pl = (t >> 2) / P;
        g = pl * 4 + (t & 3);
        ox = blockIdx.x * P + (t >> 2) % P;
        if (ox >= Wo) return;
    }
    const int oy0 = blockIdx.y * RS;
    const float f[4] = {0.125f, 0.375f, 0.375f, 0.125f};
    const half_t* xb = x + (long long)b * H * W * C + g * 8;
    // output: pixel-major [Ho][Wo][C], or 32-channel planes [C / 32][Ho][Wo][32] for conv_s2 (common.h x_planar32)
    const int opix = planar32 ? 32 : C;
    half_t* ob = out + (long long)b * Ho * Wo * C + (planar32 ? (long long)(g >> 2) * Ho * Wo * 32 + (g & 3) * 8 : g * 8);
    // Loads are UNCONDITIONAL (clamped column / row, the tap weight carries the zero padding): a load under a
    // branch makes the compiler wait for it at the join, i.e. one load in flight per thread.
    int xoff[4];
    float fx[4];
#pragma unroll
    for (int jx = 0; jx < 4; ++jx) {
        const int ix = ox * STRIDE + jx - PAD;
        const bool ok = ix >= 0 && ix < W;
        xoff[jx] = (ok ? ix : 0) * C;
        fx[jx] = ok ? f[jx] : 0.f;
    }
    constexpr int NR = (RS - 1) * STRIDE + 4;            // input rows touched by this strip
    constexpr int RB = STRIDE == 1 ? 2 : 2;              // input rows fetched per batch (RB * 4 loads in flight)
    float hs[4][8];                                      // sliding window of horizontal sums
    const int iy0 = oy0 * STRIDE - PAD;
#pragma unroll
    for (int r0 = 0; r0 < NR; r0 += RB) {
        h8 v[RB][4];
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            const int iy = min(max(iy0 + r0 + q, 0), H - 1);
#pragma unroll
            for (int jx = 0; jx < 4; ++jx) v[q][jx] = *(const h8*)(xb + (long long)iy * W * C + xoff[jx]);
        }
#pragma unroll
        for (int q = 0; q < RB; ++q) {
            const int r = r0 + q;
            if (r >= NR) break;
            const int iy = iy0 + r;
            const float rw = (iy >= 0 && iy < H) ? 1.f : 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                hs[r & 3][j] = rw * (fx[0] * (float)v[q][0][j] + fx[1] * (float)v[q][1][j] + fx[2] * (float)v[q][2][j] +
                                     fx[3] * (float)v[q][3][j]);
            // output row whose 4-row window ends at input row r
            if (r >= 3 && (r - 3) % STRIDE == 0) {
                const int oy = oy0 + (r - 3) / STRIDE;
                if (oy < Ho) {
                    h8 o;
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        o[j] = (half_t)(f[0] * hs[(r - 3) & 3][j] + f[1] * hs[(r - 2) & 3][j] + f[2] * hs[(r - 1) & 3][j] +
                                        f[3] * hs[r & 3][j]);
                    *(h8*)(ob + ((long long)oy * Wo + ox) * opix) = o;
                }
            }
        }
    }
}
bool blur_pad2_planar32_ok(int C) { return C % 32 == 0 && (C >> 3) <= 64 && 256 % (C >> 3) == 0; }
void launch_blur_pad2(const half_t* x, int B, int H, int W, int C, half_t* out, hipStream_t st, int planar32) {
    const int Ho = H + 1, Wo = W + 1;
    constexpr int RS = 16;
    dim3 g((Wo * (C >> 3) + 255) / 256, (Ho + RS - 1) / RS, B);
    if (planar32 && !blur_pad2_planar32_ok(C)) abort();       // (the caller asks blur_pad2_planar32_ok first: a silent pixel-major map would be mis-read)
    hipLaunchKernelGGL((blur_kernel<2, 1, RS>), g, dim3(256), 0, st, x, H, W, C, Ho, Wo, out, planar32);
}
void launch_blur_down(const half_t* x, int B, int H, int W, int C, half_t* out, hipStream_t st) {
    const int Ho = H / 2, Wo = W / 2;
    constexpr int RS = 8;
    dim3 g((Wo * (C >> 3) + 255) / 256, (Ho + RS - 1) / RS, B);
    hipLaunchKernelGGL((blur_kernel<1, 2, RS>), g, dim3(256), 0, st, x, H, W, C, Ho, Wo, out, 0);
}

// ---- MinibatchStd (modules.py:701-747).  Per D call (minibatch of batch_size), groups of
// `group`: sample s belongs to sub-group s % (batch_size/group).  Emits the group-mean-
// subtracted features (reference in-place quirk, see oracle/stylegan2_ref.py) + std channel.
__global__ __launch_bounds__(256) void mbstd_kernel(const half_t* x, int hw, int C, int Cpad, int batch_size,
                                                    int group, float eps, half_t* out) {
    __shared__ float red[4];
    const int nsub = batch_size / group;
    const int mb = blockIdx.x / nsub, j = blockIdx.x % nsub;
    const int n = hw * C;
    float sum = 0.f;
    for (int e = threadIdx.x; e < n; e += 256) {
        float v[8];
        float mean = 0.f;
        for (int g = 0; g < group; ++g) {
            const int s = mb * batch_size + j + g * nsub;
            v[g] = (float)x[(long long)s * n + e];
            mean += v[g];
        }
        mean /= (float)group;
        float var = 0.f;
        const int pix = e / C, c = e - pix * C;
        for (int g = 0; g < group; ++g) {
            const int s = mb * batch_size + j + g * nsub;
            const float d = v[g] - mean;
            var += d * d;
            out[((long long)s * hw + pix) * Cpad + c] = (half_t)d;
        }
        sum += sqrtf(var / (float)group + eps);
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    const float stdv = (red[0] + red[1] + red[2] + red[3]) / (float)n;
    for (int e = threadIdx.x; e < group * hw * (Cpad - C); e += 256) {
        const int cc = e % (Cpad - C);
        const int pix = (e / (Cpad - C)) % hw;
        const int g = e / ((Cpad - C) * hw);
        const int s = mb * batch_size + j + g * nsub;
        out[((long long)s * hw + pix) * Cpad + C + cc] = (half_t)(cc == 0 ? stdv : 0.f);
    }
}
// Vector form (C and Cpad multiples of 8, group <= 8): a thread owns eight channels of one pixel for the whole group — one 16-byte load per
// group member, all in flight together (the scalar form walked 32 x group two-byte loads per thread: 59 us for 0.5 MB).  Sums in the same
// order per element; the block sum of the per-element deviations runs lanes -> waves in a fixed order.
__global__ __launch_bounds__(1024) void mbstd_vec_kernel(const half_t* x, int hw, int C, int Cpad, int batch_size, int group, float eps,
                                                        half_t* out) {
    __shared__ float red[16];
    const int nsub = batch_size / group;
    const int mb = blockIdx.x / nsub, j = blockIdx.x % nsub;
    const int n = hw * C, c8n = C >> 3;
    float sum = 0.f;
    for (int e8 = threadIdx.x; e8 < hw * c8n; e8 += 1024) {
        const int pix = e8 / c8n, c8 = e8 - pix * c8n;
        h8 v[8];
#pragma unroll
        for (int g = 0; g < 8; ++g)
            if (g < group) v[g] = *(const h8*)(x + (long long)(mb * batch_size + j + g * nsub) * n + (long long)e8 * 8);
        float mean[8], var[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float m = 0.f;
#pragma unroll
            for (int g = 0; g < 8; ++g)
                if (g < group) m += (float)v[g][q];
            mean[q] = m / (float)group;
            var[q] = 0.f;
        }
#pragma unroll
        for (int g = 0; g < 8; ++g)
            if (g < group) {
                h8 o;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float d = (float)v[g][q] - mean[q];
                    var[q] += d * d;
                    o[q] = (half_t)d;
                }
                *(h8*)(out + ((long long)(mb * batch_size + j + g * nsub) * hw + pix) * Cpad + c8 * 8) = o;
            }
#pragma unroll
        for (int q = 0; q < 8; ++q) sum += sqrtf(var[q] / (float)group + eps);
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += red[w];
    const float stdv = tot / (float)n;
    for (int e = threadIdx.x; e < group * hw * (Cpad - C); e += 1024) {
        const int cc = e % (Cpad - C);
        const int pix = (e / (Cpad - C)) % hw;
        const int g = e / ((Cpad - C) * hw);
        const int s = mb * batch_size + j + g * nsub;
        out[((long long)s * hw + pix) * Cpad + C + cc] = (half_t)(cc == 0 ? stdv : 0.f);
    }
}
void launch_mbstd(const half_t* x, int B, int hw, int C, int Cpad, int batch_size, int group, float eps,
                  half_t* out, hipStream_t st) {
    const int nsub = batch_size / group;
    if ((C & 7) == 0 && (Cpad & 7) == 0 && group <= 8) {
        hipLaunchKernelGGL(mbstd_vec_kernel, dim3((B / batch_size) * nsub), dim3(1024), 0, st, x, hw, C, Cpad, batch_size, group, eps, out);
        return;
    }
    hipLaunchKernelGGL(mbstd_kernel, dim3((B / batch_size) * nsub), dim3(256), 0, st, x, hw, C, Cpad, batch_size,
                       group, eps, out);
}
