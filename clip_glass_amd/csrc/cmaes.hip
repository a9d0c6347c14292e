// cmaes.hip — the separable CMA-ES generation step on the device (include/glass.h "Device search: sep-CMA-ES"): the sample
// (cma_sample_kernel), the rank of a generation's rows in ONE workgroup (cma_rank_kernel), the update in two phases with a kernel boundary
// where the whole grid needs ||p_sigma|| (cma_update_a_kernel, cma_update_b_kernel) and the copy of a new best row (cma_best_kernel).
// Double arithmetic without fused multiply-adds, in the header's order of operations; no floating-point atomics, no cooperative launch.
// Numpy mirror: tests/cma_ref.py.
#include <math.h>

#include "../../include/glass.h"
#include "common.h"
#include "kernels.h"

namespace {
// z = sqrt(-2 ln u0) cos(2 pi u1) of the Philox draw at counter (row, column, generation, purpose 6) under the search's key
__device__ __forceinline__ double cma_normal(uint64_t seed, uint32_t row, uint32_t col, uint32_t generation) {
#pragma clang fp contract(off)
    uint32_t c[4] = {row, col, generation, GLASS_SEARCH_DRAW_NORMAL};
    philox4x32_10(c, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32) ^ GLASS_SEARCH_TAG);
    const double u0 = ((double)c[0] + 0.5) * (1.0 / 4294967296.0), u1 = ((double)c[1] + 0.5) * (1.0 / 4294967296.0);
    return sqrt(-2.0 * log(u0)) * cos(6.283185307179586 * u1);
}

// grid (ceil(n / (256 VEC)), rows): row r = row0 + blockIdx.y.  VEC 4 where n % 4 == 0 (every row is then 16-byte aligned), 1 otherwise.
// Nothing depends on the grid: a draw is a function of (seed, generation, row, column).
template <int VEC>
__global__ __launch_bounds__(256) void cma_sample_kernel(const double* __restrict__ m, const double* __restrict__ d, const CmaScalars* __restrict__ sc,
                                                         CmaParams p, int generation, int row0, float* __restrict__ X) {
#pragma clang fp contract(off)
    const int r = row0 + blockIdx.y, j0 = (blockIdx.x * 256 + threadIdx.x) * VEC;
    if (j0 >= p.n) return;
    const double sigma = sc->sigma;
    float* out = X + (size_t)r * p.n + j0;
    float o[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const int j = j0 + i;
        const double z = cma_normal(p.seed, (uint32_t)r, (uint32_t)j, (uint32_t)generation);
        o[i] = (float)fmin(fmax(m[j] + (sigma * sqrt(d[j])) * z, p.xl), p.xu);
    }
    if (VEC == 4) *(f4*)out = f4{o[0], o[1], o[2], o[3]};
    else out[0] = o[0];
}

__device__ __forceinline__ uint32_t cma_fkey(float f) {      // order-preserving bits of a float; -0.0 and 0.0 share a key (they tie, by index)
    const uint32_t u = __float_as_uint(f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline int cma_pow2(int n) { int p = 2; while (p < n) p <<= 1; return p; }

// One workgroup.  Keys (F's order-preserving bits, index) — a non-finite F takes the largest high word, so it goes last, by index — are
// sorted in LDS (bitonic, ascending; the keys are distinct).  Thread 0 then writes the scalars: the finite count, whether this generation
// updates (>= mu finite rows) and which row, if any, is the new best seen (strictly smaller than the best so far).
__global__ __launch_bounds__(1024) void cma_rank_kernel(const float* __restrict__ F, int lambda, int mu, CmaScalars* __restrict__ sc,
                                                        int* __restrict__ order, int* __restrict__ counts) {
    __shared__ unsigned long long keys[GLASS_SEARCH_MAX_POP];
    __shared__ int s_fin;
    const int N2 = cma_pow2(lambda), T = blockDim.x, tid = threadIdx.x;
    if (tid == 0) s_fin = 0;
    __syncthreads();
    for (int i = tid; i < N2; i += T) {
        unsigned long long k = ~0ull;
        if (i < lambda) {
            const float f = F[i];
            const bool fin = isfinite(f);
            if (fin) atomicAdd(&s_fin, 1);
            k = ((unsigned long long)(fin ? cma_fkey(f) : 0xFFFFFFFFu) << 32) | (unsigned)i;
        }
        keys[i] = k;
    }
    __syncthreads();
    for (int k = 2; k <= N2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (N2 >> 1); t += T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = keys[i], b = keys[l];
                if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
    for (int s = tid; s < lambda; s += T) order[s] = (int)(keys[s] & 0xFFFFFFFFu);
    if (tid == 0) {
        const int fin = s_fin;
        sc->finite = fin;
        if (counts) { counts[0] = 0; counts[1] = lambda - fin; }
        if (fin < mu) {
            sc->updated = 0;
            sc->skipped = sc->skipped + 1;
            sc->best_src = -1;
        } else {
            const int b = (int)(keys[0] & 0xFFFFFFFFu);
            const float fb = F[b];
            sc->updated = 1;
            sc->updates = sc->updates + 1;
            if (fb < sc->best_F) { sc->best_F = fb; sc->best_src = b; }
            else sc->best_src = -1;
        }
    }
}

// First phase, one thread per variable j (workgroup b owns variables [256 b, 256 b + 256)): y_i = (x_{i:lambda} - m) / sigma of the mu best
// rows — row after row, each read coalesced over j — y_w and sum w y^2 in the order i = 1 .. mu, then m and p_sigma.  Thread 0 adds the
// workgroup's p_sigma^2 in index order into part[b].  A generation that does not update (sc->updated 0) stores nothing.
__global__ __launch_bounds__(GLASS_CMA_BLOCK) void cma_update_a_kernel(const float* __restrict__ X, CmaState s, CmaParams p) {
#pragma clang fp contract(off)
    __shared__ double sw[GLASS_SEARCH_MAX_POP / 2], sq[GLASS_CMA_BLOCK];
    __shared__ int so[GLASS_SEARCH_MAX_POP / 2];
    if (!s.sc->updated) return;      // (uniform over the grid)
    const int tid = threadIdx.x, j = blockIdx.x * GLASS_CMA_BLOCK + tid;
    for (int i = tid; i < p.mu; i += GLASS_CMA_BLOCK) { sw[i] = s.w[i]; so[i] = s.order[i]; }
    __syncthreads();
    double q = 0.0;
    if (j < p.n) {
        const double mj = s.m[j], sigma = s.sc->sigma;
        double yw = 0.0, s2 = 0.0;
        for (int i = 0; i < p.mu; ++i) {
            const double y = ((double)X[(size_t)so[i] * p.n + j] - mj) / sigma;
            yw = yw + sw[i] * y;
            s2 = s2 + sw[i] * (y * y);
        }
        s.m[j] = mj + sigma * yw;
        const double ps = (1.0 - p.c_sigma) * s.ps[j] + sqrt(p.c_sigma * (2.0 - p.c_sigma) * p.mu_eff) * yw / sqrt(s.d[j]);
        s.ps[j] = ps;
        s.yw[j] = yw;
        s.s2[j] = s2;
        q = ps * ps;
    }
    sq[tid] = q;
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int t = 0; t < GLASS_CMA_BLOCK; ++t) acc = acc + sq[t];      // (the zeros behind variable n - 1 change no bit)
        s.part[blockIdx.x] = acc;
    }
}

// Second phase: every workgroup adds the partial sums in workgroup order (the same bits everywhere), decides h, then p_c and d per
// variable; thread 0 of workgroup 0 writes sigma, ||p_sigma|| and h.  Nothing here reads sigma: y_w came over from the first phase.
__global__ __launch_bounds__(GLASS_CMA_BLOCK) void cma_update_b_kernel(CmaState s, CmaParams p, int generation) {
#pragma clang fp contract(off)
    __shared__ double s_norm;
    __shared__ int s_h;
    if (!s.sc->updated) return;      // (uniform over the grid)
    const int tid = threadIdx.x, j = blockIdx.x * GLASS_CMA_BLOCK + tid;
    if (tid == 0) {
        double acc = 0.0;
        const int nb = (p.n + GLASS_CMA_BLOCK - 1) / GLASS_CMA_BLOCK;
        for (int b = 0; b < nb; ++b) acc = acc + s.part[b];
        const double norm = sqrt(acc);
        const double denom = sqrt(1.0 - pow(1.0 - p.c_sigma, 2.0 * ((double)generation + 1.0)));
        s_norm = norm;
        s_h = norm / denom < (1.4 + 2.0 / ((double)p.n + 1.0)) * p.chi ? 1 : 0;
    }
    __syncthreads();
    const double h = (double)s_h;
    if (j < p.n) {
        const double dj = s.d[j];
        const double pc = (1.0 - p.c_c) * s.pc[j] + (h * sqrt(p.c_c * (2.0 - p.c_c) * p.mu_eff)) * s.yw[j];
        s.pc[j] = pc;
        s.d[j] = ((1.0 - p.c_1) - p.c_mu) * dj + p.c_1 * (pc * pc + (((1.0 - h) * p.c_c) * (2.0 - p.c_c)) * dj) + p.c_mu * s.s2[j];
    }
    if (blockIdx.x == 0 && tid == 0) {
        const double norm = s_norm;
        const double sig = s.sc->sigma * exp(fmin(1.0, (p.c_sigma / p.d_sigma) * (norm / p.chi - 1.0)));
        s.sc->sigma = fmin(fmax(sig, 1e-10), p.xu - p.xl);
        s.sc->ps_norm = norm;
        s.sc->h = s_h;
    }
}

// best_X = the row the rank kernel named (sc->best_src), where it named one
__global__ __launch_bounds__(256) void cma_best_kernel(const float* __restrict__ X, const CmaScalars* __restrict__ sc, int lambda, int n,
                                                       float* __restrict__ best_X) {
    const int src = sc->best_src, j = blockIdx.x * 256 + threadIdx.x;
    if (src < 0 || src >= lambda || j >= n) return;
    best_X[j] = X[(size_t)src * n + j];
}
}  // namespace

void cma_weights(int lambda, double* w) {
    const int mu = lambda / 2;
    double sum = 0.0;
    for (int i = 0; i < mu; ++i) {
        w[i] = log((double)mu + 0.5) - log((double)(i + 1));
        sum += w[i];
    }
    for (int i = 0; i < mu; ++i) w[i] /= sum;
}

CmaParams cma_params(int lambda, int n, double xl, double xu, uint64_t seed) {
    CmaParams p = {};
    p.lambda = lambda; p.mu = lambda / 2; p.n = n;
    p.xl = xl; p.xu = xu; p.seed = seed;
    std::vector<double> w((size_t)std::max(p.mu, 1));
    cma_weights(lambda, w.data());
    double s2 = 0.0;
    for (int i = 0; i < p.mu; ++i) s2 += w[i] * w[i];
    const double N = (double)n, me = 1.0 / s2;
    p.mu_eff = me;
    p.c_sigma = (me + 2.0) / (N + me + 5.0);
    p.d_sigma = 1.0 + 2.0 * fmax(0.0, sqrt((me - 1.0) / (N + 1.0)) - 1.0) + p.c_sigma;
    p.c_c = (4.0 + me / N) / (N + 4.0 + 2.0 * me / N);
    double c1 = 2.0 / ((N + 1.3) * (N + 1.3) + me);
    double cmu = fmin(1.0 - c1, 2.0 * (me - 2.0 + 1.0 / me) / ((N + 2.0) * (N + 2.0) + me));
    c1 = fmin(1.0, c1 * (N + 2.0) / 3.0);      // the separable speed-up (Ros & Hansen 2008)
    cmu = fmin(1.0 - c1, cmu * (N + 2.0) / 3.0);
    p.c_1 = c1;
    p.c_mu = cmu;
    p.chi = sqrt(N) * (1.0 - 1.0 / (4.0 * N) + 1.0 / (21.0 * N * N));
    return p;
}

static bool cma_shape_ok(const CmaParams& p) {
    return p.lambda >= GLASS_CMA_MIN_POP && p.lambda <= GLASS_SEARCH_MAX_POP && p.mu == p.lambda / 2 && p.n >= 1 &&
           (long long)p.n * p.lambda < (1LL << 31);
}

const char* launch_cma_sample(const CmaState& s, const CmaParams& p, int generation, int row0, int rows, float* X, hipStream_t st) {
    if (!cma_shape_ok(p) || rows <= 0 || row0 < 0 || row0 + rows > p.lambda) return nullptr;
    if (p.n % 4 == 0) {
        hipLaunchKernelGGL(cma_sample_kernel<4>, dim3((p.n / 4 + 255) / 256, rows), dim3(256), 0, st, s.m, s.d, s.sc, p, generation, row0, X);
        return "cma_sample_kernel<4>";
    }
    hipLaunchKernelGGL(cma_sample_kernel<1>, dim3((p.n + 255) / 256, rows), dim3(256), 0, st, s.m, s.d, s.sc, p, generation, row0, X);
    return "cma_sample_kernel<1>";
}

const char* launch_cma_rank(const CmaState& s, const CmaParams& p, const float* F, hipStream_t st) {
    if (!cma_shape_ok(p)) return nullptr;
    hipLaunchKernelGGL(cma_rank_kernel, dim3(1), dim3(1024), 0, st, F, p.lambda, p.mu, s.sc, s.order, s.counts);
    return "cma_rank_kernel";
}

const char* launch_cma_update(const CmaState& s, const CmaParams& p, const float* X, int generation, hipStream_t st) {
    if (!cma_shape_ok(p) || generation < 0) return nullptr;
    const int nb = cma_blocks(p.n);
    hipLaunchKernelGGL(cma_update_a_kernel, dim3(nb), dim3(GLASS_CMA_BLOCK), 0, st, X, s, p);
    hipLaunchKernelGGL(cma_update_b_kernel, dim3(nb), dim3(GLASS_CMA_BLOCK), 0, st, s, p, generation);
    hipLaunchKernelGGL(cma_best_kernel, dim3((p.n + 255) / 256), dim3(256), 0, st, X, s.sc, p.lambda, p.n, s.best_X);
    return "cma_update_a_kernel + cma_update_b_kernel + cma_best_kernel";
}
