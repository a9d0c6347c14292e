// edit.hip — image editing (include/glass.h "Image editing"): the unit rows of the direction source and the latent anchor.  The directional
// cosine and the layout of F with the anchor in it are forms of the one cosine kernel and the one assemble_F kernel (score.hip).
#include "common.h"
#include "kernels.h"

// Every product and every sum in this file is rounded on its own (no fused multiply-add), so that numpy
// float32 written in the documented order reproduces the bits; fp32 division and square root are correctly rounded (hipcc's default).
#pragma clang fp contract(off)

// out[r] = f[r] / max(|f[r]|, 1e-8): the source rows, by the arithmetic the directional cosine (score.hip) applies to a feature row — a
// candidate whose feature has the source's bits then has x = 0 in every component.  One wave per row.
__global__ void unit_rows_kernel(const float* __restrict__ feat, int D, float* __restrict__ out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const float* f = feat + (long long)r * D;
    const float nf = unit_row_norm(f, D, lane);
    for (int i = lane; i < D; i += 64) out[(long long)r * D + i] = f[i] / nf;
}
bool launch_unit_rows(const float* feat, int n, int D, float* out, hipStream_t st) {
    if (n < 1 || D < 1 || D > (1 << 20)) return false;
    hipLaunchKernelGGL(unit_rows_kernel, dim3(n), dim3(64), 0, st, feat, D, out);
    return true;
}

// d[p] = (sum_j (w[p][j] - a[j])^2) / (n_lat L) over the flattened j = l L + i: one wave per candidate, lane-strided partial sums
// (j = lane; j < n_lat L; j += 64), the wave sum, one division by float(n_lat L); lane 0 is the candidate's one writer.
// w[p][l][i] is at w[p * cand_stride + l * layer_stride + i]: layer_stride 0 reads one row for every layer.
__global__ void latent_anchor_kernel(const float* __restrict__ w, long long cand_stride, int layer_stride, const float* __restrict__ a, int n_lat,
                                     int L, float* __restrict__ d) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const float* wp = w + (long long)p * cand_stride;
    float acc = 0.f;
    int l = lane / L, i = lane - l * L;              // (l, i) of j, advanced without a division per element
    for (int j = lane; j < n_lat * L; j += 64) {
        const float x = wp[(long long)l * layer_stride + i] - a[j];
        acc += x * x;
        i += 64;
        while (i >= L) { i -= L; ++l; }
    }
    acc = wave_sum(acc);
    if (lane == 0) d[p] = acc / (float)(n_lat * L);
}
bool launch_latent_anchor(const float* w, long long cand_stride, int layer_stride, const float* a, int n_lat, int L, int P, float* d, hipStream_t st) {
    if (P < 1 || n_lat < 1 || n_lat > GLASS_ANCHOR_MAX_LAYERS || L < 1 || L > (1 << 16) || cand_stride < 0 || (layer_stride != 0 && layer_stride < L))
        return false;
    hipLaunchKernelGGL(latent_anchor_kernel, dim3(P), dim3(64), 0, st, w, cand_stride, layer_stride, a, n_lat, L, d);
    return true;
}
