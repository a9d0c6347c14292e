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

// Latent space `sub` (include/glass.h "Subspace latent space"): dst[p][l][:] = base[l][:] + sum_k c[p][g][k] B[k][:], g = layer_group[l];
// a frozen layer (g = -1) gets base[l][:] bit for bit.  c [P][G][K], B [K][L], base [n_lat][L], dst dense [P][n_lat][L].
//   blockIdx.z: a tile of SUB_PB = 16 candidates, whose K coefficients of group blockIdx.y are staged once in LDS as cs[k][candidate]
//   (K <= 512: 32 KB), so that one 16-byte LDS read gives a k's coefficients of four candidates to every lane at once;
//   wave w of the workgroup owns the columns [256 (4 blockIdx.x + w), + 256), four per lane: one 16-byte load of B[k][j .. j + 3] feeds
//   the 64 FMAs of all 16 candidates — a B element is loaded once per (group, candidate tile) and never per layer.
// The product of (candidate, group) is ONE fp32 FMA chain over k = 0 .. K - 1 from 0.f (explicit FMAs: see dense_body.h on what
// -ffp-contract does to rows otherwise), held in registers and then added to base[l] for every layer l of the group: one fp32 add and one
// 16-byte store per layer.  The workgroups of group 0 copy the frozen layers too — the launch writes every element of dst[0 .. P).  A
// candidate's values depend on its own row alone: not on P, its slot in the tile or the tile.
#define SUB_PB 16
#define SUB_KMAX 512
__global__ __launch_bounds__(256) void dlatent_subspace_kernel(const float* __restrict__ c, int G, int K, const int* __restrict__ layer_group,
                                                               int n_lat, int L, const float* __restrict__ B, const float* __restrict__ base,
                                                               float* __restrict__ dst, int P) {
    __shared__ f4 cs[SUB_KMAX][SUB_PB / 4];
    const int t = threadIdx.x, g = blockIdx.y, p0 = blockIdx.z * SUB_PB;
    float* csf = (float*)cs;
    for (int e = t; e < SUB_PB * K; e += 256) {      // coalesced along k; a slot past P holds zeros and is never stored
        const int pr = e / K, k = e - pr * K;
        csf[k * SUB_PB + pr] = p0 + pr < P ? c[((long long)(p0 + pr) * G + g) * K + k] : 0.f;
    }
    __syncthreads();
    const int j = (blockIdx.x * 4 + (t >> 6)) * 256 + (t & 63) * 4;
    if (j >= L) return;      // (after the only barrier; L % 4 == 0: a lane's four columns are inside or outside together)
    f4 acc[SUB_PB];
#pragma unroll
    for (int q = 0; q < SUB_PB; ++q) acc[q] = f4{0.f, 0.f, 0.f, 0.f};
    const float* Bj = B + j;
    int k = 0;
    for (; k + 4 <= K; k += 4) {      // four 16-byte loads of B in flight
        f4 b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = *(const f4*)(Bj + (long long)(k + u) * L);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q4 = 0; q4 < SUB_PB / 4; ++q4) {
                const f4 cv = cs[k + u][q4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[q4 * 4 + q][i] = __builtin_fmaf(cv[q], b[u][i], acc[q4 * 4 + q][i]);
            }
    }
    for (; k < K; ++k) {
        const f4 b = *(const f4*)(Bj + (long long)k * L);
#pragma unroll
        for (int q4 = 0; q4 < SUB_PB / 4; ++q4) {
            const f4 cv = cs[k][q4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[q4 * 4 + q][i] = __builtin_fmaf(cv[q], b[i], acc[q4 * 4 + q][i]);
        }
    }
    const int np = min(SUB_PB, P - p0);
    for (int l = 0; l < n_lat; ++l) {
        const int lg = layer_group[l];      // uniform over the workgroup
        if (lg != g && !(lg < 0 && g == 0)) continue;
        const f4 bs = *(const f4*)(base + (long long)l * L + j);
#pragma unroll
        for (int q = 0; q < SUB_PB; ++q) {
            f4 o = bs;
            if (lg >= 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = bs[i] + acc[q][i];
            }
            if (q < np) *(f4*)(dst + ((long long)(p0 + q) * n_lat + l) * L + j) = o;      // (no break: acc stays in registers under a full unroll)
        }
    }
}
// false: the shape is outside the kernel's limits (glass_subspace_supported's, which the engine has asked before), nothing launched
bool launch_dlatent_subspace(const float* c, int P, int G, int K, const int* layer_group, int n_lat, int L, const float* B, const float* base,
                             float* dst, hipStream_t st) {
    if (P < 1 || G < 1 || G > n_lat || K < 1 || K > SUB_KMAX || K > L || L % 4 || (P + SUB_PB - 1) / SUB_PB > 65535) return false;
    hipLaunchKernelGGL(dlatent_subspace_kernel, dim3((L + 1023) / 1024, G, (P + SUB_PB - 1) / SUB_PB), dim3(256), 0, st, c, G, K, layer_group,
                       n_lat, L, B, base, dst, P);
    return true;
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
