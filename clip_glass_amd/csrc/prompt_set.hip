// prompt_set.hip — prompt sets (include/glass.h "Prompt sets"): the cosine of every feature row with every entry of the set, their ordered
// means over the views, the weighted combination, and the pareto layout of F.  The default pass (one target) does not come here: it keeps
// cosine_kernel / cosine_views_kernel / assemble_F_kernel (kernels_clip.hip).
#include "common.h"
#include "kernels.h"

// cosine_kernel's wave sum (kernels_clip.hip wsum): the same butterfly, so that a (row, entry) value has the same bits
__device__ __forceinline__ float ps_wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One workgroup per candidate, four waves.  Wave w takes the feature rows v = w, w + 4, ...: xx once per row, then the entries four at a time
// (four independent accumulator pairs per lane; each one runs i = lane, lane + 64, ... and the wave sum, cosine_kernel's order).  STAGED: the
// T D floats of the set are copied to LDS once per workgroup; otherwise (more than 64 KB) they stream from L2.  After one barrier, lane t of wave 0
// forms entry t's mean over v = 0 .. V - 1 and the wave combines them in the order t = 0 .. T - 1.
// isl.weights (include/glass.h "Device search: islands", own prompts): candidate p belongs to island (isl.row0 + p) / isl.pop and combines its
// entries with that island's row of the table [islands][T] and its sum of |w|; nullptr: weights and W, as ever.
template <bool STAGED>
__global__ __launch_bounds__(256) void cosine_set_kernel(const float* __restrict__ feat, const float* __restrict__ targets,
                                                         const float* __restrict__ weights, float W, int V, int T, int D,
                                                         float* __restrict__ view_sim, float* __restrict__ set_sim, float* __restrict__ sim,
                                                         CosineIslands isl) {
    extern __shared__ float ps_targets[];                               // STAGED: [T][D]
    __shared__ float c[GLASS_PROMPT_MAX_VIEWS][GLASS_PROMPT_MAX];       // c[v][t]
    const int p = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (isl.weights) {
        const int island = (isl.row0 + p) / isl.pop;
        weights = isl.weights + (size_t)island * T;
        W = isl.W[island];
    }
    if (STAGED) {
        for (int i = tid; i < T * D; i += 256) ps_targets[i] = targets[i];
        __syncthreads();
    }
    for (int v = wave; v < V; v += 4) {
        const float* f = feat + ((long long)p * V + v) * D;
        float xx = 0.f;
        for (int i = lane; i < D; i += 64) {
            const float a = f[i];
            xx += a * a;
        }
        const float nx = sqrtf(ps_wsum(xx));
        for (int t0 = 0; t0 < T; t0 += 4) {
            float xy[4] = {0.f, 0.f, 0.f, 0.f}, yy[4] = {0.f, 0.f, 0.f, 0.f};
            int off[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) off[j] = min(t0 + j, T - 1) * D;       // (a group's tail re-reads the last entry; its values are dropped)
            for (int i = lane; i < D; i += 64) {
                const float a = f[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float b = STAGED ? ps_targets[off[j] + i] : targets[off[j] + i];
                    xy[j] += a * b;
                    yy[j] += b * b;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (t0 + j >= T) break;
                const float x = ps_wsum(xy[j]), y = ps_wsum(yy[j]);
                if (lane == 0) c[v][t0 + j] = x / fmaxf(nx * sqrtf(y), 1e-8f);
            }
        }
    }
    __syncthreads();
    if (wave != 0) return;
    float cb = 0.f;
    if (lane < T) {
        cb = c[0][lane];
        if (V > 1) {                      // cosine_views_kernel's mean
            float acc = 0.f;
            for (int v = 0; v < V; ++v) acc += c[v][lane];
            cb = acc / (float)V;
        }
        set_sim[(long long)p * T + lane] = cb;
    }
    if (view_sim && lane < V) view_sim[(long long)p * V + lane] = c[lane][0];
    float acc = 0.f;
    {
        // the product and the sum are rounded separately (include/glass.h).  HIP's __fmul_rn / __fadd_rn are plain * and + inside the header,
        // where contraction is on: the pair came out as one fused multiply-add (measured: one ulp off numpy float32 in 1 of 5 rows).  The
        // operators are therefore written here, in a block with contraction off
#pragma clang fp contract(off)
        for (int t = 0; t < T; ++t) {
            const float prod = weights[t] * __shfl(cb, t);
            acc = acc + prod;
        }
    }
    if (lane == 0) sim[p] = acc / W;
}

float prompt_weight_sum(const float* weights, int T) {
    float W = 0.f;
    for (int t = 0; t < T; ++t) W += fabsf(weights[t]);
    return W;
}

bool launch_cosine_set(const float* feat, const float* targets, const float* weights, float W, int P, int V, int T, int D, float* view_sim,
                       float* set_sim, float* sim, hipStream_t st, CosineIslands isl) {
    if (isl.weights && (!isl.W || isl.pop < 1 || isl.row0 < 0)) return false;
    if (P < 1 || V < 1 || V > GLASS_PROMPT_MAX_VIEWS || T < 1 || T > GLASS_PROMPT_MAX || D < 1 || D > (1 << 20)) return false;
    const size_t bytes = (size_t)T * D * sizeof(float);
    if (bytes <= (64u << 10)) {
        static DevOnce once;
        once.run([&] { (void)hipFuncSetAttribute((const void*)cosine_set_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 << 10); });
        hipLaunchKernelGGL(cosine_set_kernel<true>, dim3(P), dim3(256), bytes, st, feat, targets, weights, W, V, T, D, view_sim, set_sim, sim, isl);
    } else {
        hipLaunchKernelGGL(cosine_set_kernel<false>, dim3(P), dim3(256), 0, st, feat, targets, weights, W, V, T, D, view_sim, set_sim, sim, isl);
    }
    return true;
}

// pareto layout: F[p] = (K similarity columns, the hinge with a discriminator, the perceptual distance as its own column)
__global__ void assemble_F_set_kernel(const float* set_sim, const float* weights, const float* dis, const float* lp, int K, int P, int n_obj, float* F) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    float* row = F + (long long)p * n_obj;
    for (int t = 0; t < K; ++t) {
        const float cb = set_sim[(long long)p * K + t];
        row[t] = weights[t] < 0.f ? cb : -cb;
    }
    int col = K;
    if (dis) row[col++] = fmaxf(1.f - dis[p], 0.f);
    if (lp) row[col] = lp[p];
}
void launch_assemble_F_set(const float* set_sim, const float* weights, const float* dis, const float* lp, int K, int P, float* F, hipStream_t st) {
    const int n_obj = K + (dis ? 1 : 0) + (lp ? 1 : 0);
    hipLaunchKernelGGL(assemble_F_set_kernel, dim3((P + 63) / 64), dim3(64), 0, st, set_sim, weights, dis, lp, K, P, n_obj, F);
}
