// dense_body.h — the small-M fp32 dense tile shared by dense_kernel / dense_multi_kernel (kernels_misc.hip) and
// styles_layered_kernel (dlatent.hip): one body, so that an output element has the same bits whichever kernel computes it.
#pragma once
#include "common.h"

#define DENSE_PB 16
#define DENSE_KT 128
__device__ __forceinline__ void dense_body(const float* x, int ldx, int P, int K, const float* wt, int N, int ldw,
                                           const float* bias, float* out, int ldo, int in_sq, int mode,
                                           const float* eps_row, int eps_stride, int bx, int by) {
    __shared__ float xs[DENSE_PB][DENSE_KT];
    const int t = threadIdx.x;
    const int n = bx * 64 + (t & 63);
    const int pg = t >> 6;
    const int p0 = by * DENSE_PB;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += DENSE_KT) {
        for (int e = t; e < DENSE_PB * DENSE_KT; e += 256) {
            const int pr = e / DENSE_KT, kk = e - pr * DENSE_KT;
            float v = 0.f;
            if (p0 + pr < P && k0 + kk < K) v = x[(long long)(p0 + pr) * ldx + k0 + kk];
            xs[pr][kk] = in_sq ? v * v : v;
        }
        __syncthreads();
        if (n < N) {
            const int kmax = min(DENSE_KT, K - k0);
            int kk = 0;
            for (; kk + 16 <= kmax; kk += 16) {      // 16 weight loads in flight (a one-load-per-iteration loop is a chain
                float w[16];                         // of L2 round trips: 512 of them per mapping layer)
#pragma unroll
                for (int u = 0; u < 16; ++u) w[u] = wt[(long long)(k0 + kk + u) * ldw + n];
#pragma unroll
                for (int u = 0; u < 16; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(w[u], xs[pg * 4 + j][kk + u], acc[j]);   // explicit FMA for every row:
                // left to -ffp-contract the compiler packed rows (0, 1) as v_pk_fma_f32 and rows (2, 3) as mul + add, so a row's last bit
                // depended on its POSITION in the launch (found by the full-size text-tower test, r04)
            }
            for (; kk < kmax; ++kk) {
                const float w = wt[(long long)(k0 + kk) * ldw + n];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(w, xs[pg * 4 + j][kk], acc[j]);
            }
        }
        __syncthreads();
    }
    if (n >= N) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + pg * 4 + j;
        if (p >= P) continue;
        float v = acc[j] + (bias ? bias[n] : 0.f);
        if (mode == 1) v = lrelu_sqrt2(v);
        else if (mode == 2) v = rsqrtf(v + eps_row[(long long)p * eps_stride]);
        out[(long long)p * ldo + n] = v;
    }
}
