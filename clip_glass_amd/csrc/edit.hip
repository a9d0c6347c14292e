// edit.hip — image editing (include/glass.h "Image editing"): the directional cosine of every feature row with every entry of the set, the
// latent anchor, and the layout of F with the anchor in it.  Passes without a direction source and without an anchor do not come here:
// they keep cosine_kernel / cosine_views_kernel / cosine_set_kernel and assemble_F*_kernel.
#include "common.h"
#include "kernels.h"

// Every product and every sum in this file is rounded on its own (no fused multiply-add but the explicit fmaf of the folds), so that numpy
// float32 written in the documented order reproduces the bits; fp32 division and square root are correctly rounded (hipcc's default).
#pragma clang fp contract(off)

// cosine_kernel's wave sum (kernels_clip.hip wsum): the butterfly over offsets 32, 16, .. 1
__device__ __forceinline__ float ed_wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// max(|f|, 1e-8) of one row by one wave: lane-strided partial sums (i = lane; i < D; i += 64), then the wave sum
__device__ __forceinline__ float ed_row_norm(const float* __restrict__ f, int D, int lane) {
    float xx = 0.f;
    for (int i = lane; i < D; i += 64) {
        const float a = f[i];
        xx += a * a;
    }
    return fmaxf(sqrtf(ed_wsum(xx)), 1e-8f);
}

// One workgroup per candidate, four waves, cosine_set_kernel's shape.  Wave w takes the feature rows v = w, w + 4, ...: nf = max(|f|, 1e-8)
// once per row, then |x|^2 of x_i = f_i / nf - src[v][i], then the entries four at a time — four independent accumulator pairs per lane
// (x.g_t and g_t.g_t), each one running i = lane, lane + 64, ... and the wave sum; x_i is formed again from f_i, nf and src in every sweep (the
// same three operations, the same bits).  STAGED: the T D floats of the set are copied to LDS once per workgroup; otherwise (more than 64 KB)
// they stream from L2.  After one barrier, lane t of wave 0 forms entry t's mean over v = 0 .. V - 1 and the wave combines them in the order
// t = 0 .. T - 1, as cosine_set_kernel does.
template <bool STAGED>
__global__ __launch_bounds__(256) void cosine_set_dir_kernel(const float* __restrict__ feat, const float* __restrict__ targets,
                                                             const float* __restrict__ weights, float W, int V, int T, int D,
                                                             const float* __restrict__ src, float* __restrict__ view_sim,
                                                             float* __restrict__ set_sim, float* __restrict__ sim) {
    extern __shared__ float ed_targets[];                               // STAGED: [T][D]
    __shared__ float c[GLASS_PROMPT_MAX_VIEWS][GLASS_PROMPT_MAX];       // c[v][t]
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (STAGED) {
        for (int i = tid; i < T * D; i += 256) ed_targets[i] = targets[i];
        __syncthreads();
    }
    for (int v = wave; v < V; v += 4) {
        const float* f = feat + ((long long)p * V + v) * D;
        const float* s = src + (long long)v * D;
        const float nf = ed_row_norm(f, D, lane);
        float xx = 0.f;
        for (int i = lane; i < D; i += 64) {
            const float x = f[i] / nf - s[i];
            xx += x * x;
        }
        const float nx = sqrtf(ed_wsum(xx));
        for (int t0 = 0; t0 < T; t0 += 4) {
            float xy[4] = {0.f, 0.f, 0.f, 0.f}, yy[4] = {0.f, 0.f, 0.f, 0.f};
            int off[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) off[j] = min(t0 + j, T - 1) * D;       // (a group's tail re-reads the last entry; its values are dropped)
            for (int i = lane; i < D; i += 64) {
                const float x = f[i] / nf - s[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float b = STAGED ? ed_targets[off[j] + i] : targets[off[j] + i];
                    xy[j] += x * b;
                    yy[j] += b * b;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (t0 + j >= T) break;
                const float a = ed_wsum(xy[j]), y = ed_wsum(yy[j]);
                if (lane == 0) c[v][t0 + j] = a / fmaxf(nx * sqrtf(y), 1e-8f);
            }
        }
    }
    __syncthreads();
    if (wave != 0) return;
    float cb = 0.f;
    if (lane < T) {
        cb = c[0][lane];
        if (V > 1) {                      // the views' mean, in the order v = 0 .. V - 1
            float acc = 0.f;
            for (int v = 0; v < V; ++v) acc += c[v][lane];
            cb = acc / (float)V;
        }
        set_sim[(long long)p * T + lane] = cb;
    }
    if (view_sim && lane < V) view_sim[(long long)p * V + lane] = c[lane][0];
    float acc = 0.f;
    for (int t = 0; t < T; ++t) {         // the product and the sum rounded separately ("Prompt sets")
        const float prod = weights[t] * __shfl(cb, t);
        acc = acc + prod;
    }
    if (lane == 0) sim[p] = acc / W;
}

bool launch_cosine_set_dir(const float* feat, const float* targets, const float* weights, float W, int P, int V, int T, int D, const float* src,
                           float* view_sim, float* set_sim, float* sim, hipStream_t st) {
    if (P < 1 || V < 1 || V > GLASS_PROMPT_MAX_VIEWS || T < 1 || T > GLASS_PROMPT_MAX || D < 1 || D > (1 << 20) || !src) return false;
    const size_t bytes = (size_t)T * D * sizeof(float);
    if (bytes <= (64u << 10)) {
        static DevOnce once;
        once.run([&] { (void)hipFuncSetAttribute((const void*)cosine_set_dir_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 << 10); });
        hipLaunchKernelGGL(cosine_set_dir_kernel<true>, dim3(P), dim3(256), bytes, st, feat, targets, weights, W, V, T, D, src, view_sim, set_sim, sim);
    } else {
        hipLaunchKernelGGL(cosine_set_dir_kernel<false>, dim3(P), dim3(256), 0, st, feat, targets, weights, W, V, T, D, src, view_sim, set_sim, sim);
    }
    return true;
}

// The streamed form at a shape the staged one takes too (the diagnostic op's: the two must agree bit for bit)
bool launch_cosine_set_dir_streamed(const float* feat, const float* targets, const float* weights, float W, int P, int V, int T, int D,
                                    const float* src, float* view_sim, float* set_sim, float* sim, hipStream_t st) {
    if (P < 1 || V < 1 || V > GLASS_PROMPT_MAX_VIEWS || T < 1 || T > GLASS_PROMPT_MAX || D < 1 || D > (1 << 20) || !src) return false;
    hipLaunchKernelGGL(cosine_set_dir_kernel<false>, dim3(P), dim3(256), 0, st, feat, targets, weights, W, V, T, D, src, view_sim, set_sim, sim);
    return true;
}

// out[r] = f[r] / max(|f[r]|, 1e-8): the source rows, by the arithmetic cosine_set_dir_kernel applies to a feature row — a candidate whose
// feature has the source's bits then has x = 0 in every component.  One wave per row.
__global__ void unit_rows_kernel(const float* __restrict__ feat, int D, float* __restrict__ out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const float* f = feat + (long long)r * D;
    const float nf = ed_row_norm(f, D, lane);
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
    acc = ed_wsum(acc);
    if (lane == 0) d[p] = acc / (float)(n_lat * L);
}
bool launch_latent_anchor(const float* w, long long cand_stride, int layer_stride, const float* a, int n_lat, int L, int P, float* d, hipStream_t st) {
    if (P < 1 || n_lat < 1 || n_lat > GLASS_ANCHOR_MAX_LAYERS || L < 1 || L > (1 << 16) || cand_stride < 0 || (layer_stride != 0 && layer_stride < L))
        return false;
    hipLaunchKernelGGL(latent_anchor_kernel, dim3(P), dim3(64), 0, st, w, cand_stride, layer_stride, a, n_lat, L, d);
    return true;
}

// F with the anchor in it ("Image editing"): the similarity columns (K = 1: -sim, with the LPIPS fold where lp_lambda > 0; K >= 2: the pareto
// layout from set_sim and the weights' signs), the hinge with a discriminator, the LPIPS distance as its own column, then the anchor distance
// as its own LAST column (anchor_lambda == 0) or folded into column 0 behind the LPIPS fold (anchor_lambda > 0; K = 1 only).
__global__ void assemble_F_edit_kernel(const float* sim, const float* set_sim, const float* weights, int K, const float* dis, const float* lp,
                                       float lp_lambda, const float* anchor, float anchor_lambda, int P, int n_obj, float* F) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    float* row = F + (long long)p * n_obj;
    if (K >= 2) {
        for (int t = 0; t < K; ++t) {
            const float cb = set_sim[(long long)p * K + t];
            row[t] = weights[t] < 0.f ? cb : -cb;
        }
    } else {
        float f0 = (lp && lp_lambda > 0.f) ? fmaf(lp_lambda, lp[p], -sim[p]) : -sim[p];
        if (anchor_lambda > 0.f) f0 = fmaf(anchor_lambda, anchor[p], f0);
        row[0] = f0;
    }
    int col = K >= 2 ? K : 1;
    if (dis) row[col++] = fmaxf(1.f - dis[p], 0.f);
    if (lp && !(lp_lambda > 0.f)) row[col++] = lp[p];
    if (!(anchor_lambda > 0.f)) row[col] = anchor[p];
}
bool launch_assemble_F_edit(const float* sim, const float* set_sim, const float* weights, int K, const float* dis, const float* lp, float lp_lambda,
                            const float* anchor, float anchor_lambda, int P, int n_obj, float* F, hipStream_t st) {
    const int k = K >= 2 ? K : 1;
    const int want = k + (dis ? 1 : 0) + (lp && !(lp_lambda > 0.f) ? 1 : 0) + (!(anchor_lambda > 0.f) ? 1 : 0);
    if (P < 1 || !anchor || n_obj != want || (k >= 2 ? (!set_sim || !weights || anchor_lambda > 0.f || (lp && lp_lambda > 0.f)) : !sim)) return false;
    hipLaunchKernelGGL(assemble_F_edit_kernel, dim3((P + 63) / 64), dim3(64), 0, st, sim, set_sim, weights, k, dis, lp, lp_lambda, anchor, anchor_lambda,
                       P, n_obj, F);
    return true;
}
