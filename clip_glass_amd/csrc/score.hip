// score.hip — the tail of every scoring pass: the cosine of every feature row with every entry of the target set, their ordered means over
// the views, the weighted combination (include/glass.h "Prompt sets", "Image editing", "Device search: islands"), and the rows of F.  One
// cosine kernel and one assemble_F kernel: a single target (glass_engine_set_target) is the set of one entry of weight 1.
// Reference: generator.py:51 (torch.cosine_similarity: x.y / max(|x||y|, 1e-8)), problem.py:21-27 (F).
#include "common.h"
#include "kernels.h"

// One workgroup per candidate, four waves.  Wave w takes the feature rows v = w, w + 4, ...: |x|^2 once per row, then the entries four at a
// time (four independent accumulator pairs per lane, x.y_t and y_t.y_t; each one runs i = lane, lane + 64, ... and the wave sum).
// DIR (a direction source, src [V][D] of unit rows): x_i = f_i / nf - src[v][i] with nf = max(|f|, 1e-8), formed again from f_i, nf and src in
// every sweep (the same three operations, the same bits); every product and sum is rounded on its own, so that numpy float32 written in this
// order reproduces the bits.  Otherwise x = f and the sums are fused multiply-adds.
// STAGED: the T D floats of the set are copied to LDS once per workgroup; otherwise (more than 64 KB) they stream from L2.  After one barrier,
// lane t of wave 0 forms entry t's mean over v = 0 .. V - 1 and the wave combines them in the order t = 0 .. T - 1, product and sum rounded
// separately in both forms.
// isl.weights (own prompts of an island search): candidate p belongs to island (isl.row0 + p) / isl.pop and combines its entries with that
// island's row of the table [islands][T] and its sum of |w|; nullptr: weights and W.
template <bool STAGED, bool DIR>
__global__ __launch_bounds__(256) void cosine_set_kernel(const float* __restrict__ feat, const float* __restrict__ targets,
                                                         const float* __restrict__ weights, float W, int V, int T, int D,
                                                         const float* __restrict__ src, float* __restrict__ view_sim,
                                                         float* __restrict__ set_sim, float* __restrict__ sim, CosineIslands isl) {
    extern __shared__ float staged[];                                   // STAGED: [T][D]
    __shared__ float c[GLASS_PROMPT_MAX_VIEWS][GLASS_PROMPT_MAX];       // c[v][t]
    constexpr bool FUSED = !DIR;
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (isl.weights) {
        const int island = (isl.row0 + p) / isl.pop;
        weights = isl.weights + (size_t)island * T;
        W = isl.W[island];
    }
    if (STAGED) {
        for (int i = tid; i < T * D; i += 256) staged[i] = targets[i];
        __syncthreads();
    }
    for (int v = wave; v < V; v += 4) {
        const float* f = feat + ((long long)p * V + v) * D;
        const float* s = DIR ? src + (long long)v * D : nullptr;
        const float nf = DIR ? unit_row_norm(f, D, lane) : 1.f;
        const auto x_at = [&](int i) {
            if constexpr (DIR) return f[i] / nf - s[i];
            else return f[i];
        };
        float xx = 0.f;
        for (int i = lane; i < D; i += 64) {
            const float x = x_at(i);
            xx = mac<FUSED>(xx, x, x);
        }
        const float nx = sqrtf(wave_sum(xx));
        for (int t0 = 0; t0 < T; t0 += 4) {
            float xy[4] = {0.f, 0.f, 0.f, 0.f}, yy[4] = {0.f, 0.f, 0.f, 0.f};
            int off[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) off[j] = min(t0 + j, T - 1) * D;       // (a group's tail re-reads the last entry; its values are dropped)
            for (int i = lane; i < D; i += 64) {
                const float x = x_at(i);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float b = STAGED ? staged[off[j] + i] : targets[off[j] + i];
                    xy[j] = mac<FUSED>(xy[j], x, b);
                    yy[j] = mac<FUSED>(yy[j], b, b);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (t0 + j >= T) break;
                const float a = wave_sum(xy[j]), y = wave_sum(yy[j]);
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
    for (int t = 0; t < T; ++t) acc = mac<false>(acc, weights[t], __shfl(cb, t));
    if (lane == 0) sim[p] = acc / W;
}

float prompt_weight_sum(const float* weights, int T) {
    float W = 0.f;
    for (int t = 0; t < T; ++t) W += fabsf(weights[t]);
    return W;
}

template <bool DIR>
static void launch_cosine_set_form(const CosineSet& a, hipStream_t st) {
    const size_t bytes = (size_t)a.T * a.D * sizeof(float);
    if (!a.streamed && bytes <= (64u << 10)) {
        constexpr auto kernel = cosine_set_kernel<true, DIR>;
        static DevOnce once;
        once.run([&] { (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 << 10); });
        hipLaunchKernelGGL(kernel, dim3(a.P), dim3(256), bytes, st, a.feat, a.targets, a.weights, a.W, a.V, a.T, a.D, a.src, a.view_sim, a.set_sim,
                           a.sim, a.isl);
    } else {
        constexpr auto kernel = cosine_set_kernel<false, DIR>;
        hipLaunchKernelGGL(kernel, dim3(a.P), dim3(256), 0, st, a.feat, a.targets, a.weights, a.W, a.V, a.T, a.D, a.src, a.view_sim, a.set_sim, a.sim,
                           a.isl);
    }
}
bool launch_cosine_set(const CosineSet& a, hipStream_t st) {
    if (a.isl.weights && (!a.isl.W || a.isl.pop < 1 || a.isl.row0 < 0)) return false;
    if (a.P < 1 || a.V < 1 || a.V > GLASS_PROMPT_MAX_VIEWS || a.T < 1 || a.T > GLASS_PROMPT_MAX || a.D < 1 || a.D > (1 << 20)) return false;
    if (a.src) launch_cosine_set_form<true>(a, st);
    else launch_cosine_set_form<false>(a, st);
    return true;
}

// problem.py:23-27 and what the project added to it.  The similarity columns: one, -sim, with the LPIPS fold where lp_lambda > 0 and then the
// anchor fold where anchor_lambda > 0 — or, with set_sim, the pareto layout, K columns by the weights' signs.  Then the hinge with a
// discriminator, the LPIPS distance as its own column (lp_lambda == 0), the anchor distance as its own LAST column (anchor_lambda == 0).
__global__ void assemble_F_kernel(AssembleF a) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.P) return;
    float* row = a.F + (long long)p * a.n_obj;
    int col = 1;
    if (a.set_sim) {
        for (int t = 0; t < a.K; ++t) {
            const float cb = a.set_sim[(long long)p * a.K + t];
            row[t] = a.weights[t] < 0.f ? cb : -cb;
        }
        col = a.K;
    } else {
        float f0 = (a.lp && a.lp_lambda > 0.f) ? fmaf(a.lp_lambda, a.lp[p], -a.sim[p]) : -a.sim[p];
        if (a.anchor && a.anchor_lambda > 0.f) f0 = fmaf(a.anchor_lambda, a.anchor[p], f0);
        row[0] = f0;
    }
    if (a.dis) row[col++] = fmaxf(1.f - a.dis[p], 0.f);
    if (a.lp && !(a.lp_lambda > 0.f)) row[col++] = a.lp[p];
    if (a.anchor && !(a.anchor_lambda > 0.f)) row[col] = a.anchor[p];
}
bool launch_assemble_F(const AssembleF& a, hipStream_t st) {
    const bool lp_fold = a.lp && a.lp_lambda > 0.f, anchor_fold = a.anchor && a.anchor_lambda > 0.f;
    const int want = (a.set_sim ? a.K : 1) + (a.dis ? 1 : 0) + (a.lp && !lp_fold ? 1 : 0) + (a.anchor && !anchor_fold ? 1 : 0);
    if (a.P < 1 || !a.F || a.n_obj != want || (a.set_sim ? (a.K < 1 || !a.weights || lp_fold || anchor_fold) : !a.sim)) return false;
    hipLaunchKernelGGL(assemble_F_kernel, dim3((a.P + 63) / 64), dim3(64), 0, st, a);
    return true;
}
