// dlatent.hip — the dlatents of a pass (truncation trick, W / W+ latent spaces) and the style affines over per-layer rows.
// Reference: stylegan2/models.py:264-285 (set_truncation), :314-324 (truncate), :393-458 (forward(dlatents=...)).
#include "common.h"
#include "kernels.h"
#include "dense_body.h"

// dst[p][l][:] = lerp(avg, src[p][l][:], psi[l])   (models.py:323; utils.py:123-125 calls torch.lerp for fp32 tensors)
//   src row of (p, l) at src + p * src_row + l * src_layer floats (src_layer 0: one row per candidate feeds every layer), dst is dense
//   [P][n_layers][L].  In place (src == dst with the same strides) is fine: a thread reads the 16 bytes it writes and no others.
//   tab = psi[n_pad] | avg[L] (n_pad: n_layers rounded up to 4, so avg stays 16-byte aligned).
// torch.lerp's two-branch rule, with the FMA its vectorised CPU kernel uses: weight < 0.5: a + w (b - a); otherwise b - (b - a)(1 - w).
// psi = 1 copies the row bit for bit (the reference's lerp shortcut, and what forward(dlatents=...) does without truncate()).
// One 16-byte load of src and of avg and one 16-byte store per thread, all loads unconditional (the select comes after them): a
// candidate's result depends on its own row alone, never on P.
__global__ __launch_bounds__(256) void dlatent_expand_kernel(const float* src, long long src_row, long long src_layer, float* dst,
                                                             const float* tab, int n_pad, int n_layers, int L4, long long total4) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int k4 = (int)(i % L4);
    const long long pl = i / L4;
    const int l = (int)(pl % n_layers);
    const long long p = pl / n_layers;
    const f4 b = *(const f4*)(src + p * src_row + l * src_layer + 4 * k4);
    const f4 a = *(const f4*)(tab + n_pad + 4 * k4);
    const float w = tab[l];
    const float coeff = w < 0.5f ? w : w - 1.f;
    f4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float v = __builtin_fmaf(coeff, b[j] - a[j], w < 0.5f ? a[j] : b[j]);
        o[j] = w == 1.f ? b[j] : v;
    }
    *(f4*)(dst + i * 4) = o;
}
void launch_dlatent_expand(const float* src, long long src_row, long long src_layer, float* dst, const float* tab, int n_pad, int n_layers,
                           int P, int L, hipStream_t st) {
    const long long total4 = (long long)P * n_layers * (L / 4);
    hipLaunchKernelGGL(dlatent_expand_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, src, src_row, src_layer, dst, tab,
                       n_pad, n_layers, L / 4, total4);
}

// Style affines when the dlatent rows differ per layer: columns [col0, col0 + n) of the concatenated [P][S_total] table — one 64-wide
// piece of one style segment — read dlatent row `lat` of their candidate.  blockIdx.x walks the (segment, n0) tile list built at
// finalize (StyleTile: no workgroup starts only to leave), blockIdx.y the groups of 16 candidates.  The tile is dense_body's, so an
// output element has the bits dense_kernel gives for the same input row: one FMA chain over k = 0 .. L - 1, then + bias.
__global__ __launch_bounds__(256) void styles_layered_kernel(const float* dlat, int n_lat, int L, const float* wt, int S_total,
                                                             const float* bias, float* out, const StyleTile* tiles, int P) {
    const StyleTile t = tiles[blockIdx.x];
    dense_body(dlat + (long long)t.lat * L, n_lat * L, P, L, wt + t.col0, t.n, S_total, bias + t.col0, out + t.col0, S_total, 0, 0, nullptr,
               0, 0, blockIdx.y);
}
void launch_styles_layered(const float* dlat, int n_lat, int L, int P, const float* wt, int S_total, const float* bias, float* out,
                           const StyleTile* d_tiles, int n_tiles, hipStream_t st) {
    hipLaunchKernelGGL(styles_layered_kernel, dim3(n_tiles, (P + DENSE_PB - 1) / DENSE_PB), dim3(256), 0, st, dlat, n_lat, L, wt, S_total,
                       bias, out, d_tiles, P);
}
