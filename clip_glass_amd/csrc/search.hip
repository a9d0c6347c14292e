// search.hip — the GA / NSGA-II generation step on the device (include/glass.h "Device search"): binary tournament + bounded SBX +
// polynomial mutation (ga_vary_kernel), HUX + bit-flip on the bit columns of a mixed row (ga_vary_bits_kernel), exact duplicate flags
// (ga_duplicates_kernel), rank-and-crowding / fitness survival in ONE workgroup (ga_survive_kernel) and the gather of the surviving rows
// (ga_gather_kernel).  Numpy mirrors: tests/search_device_ref.py, tests/search_mixed_ref.py.
#include <math.h>

#include "../../include/glass.h"
#include "common.h"
#include "kernels.h"

namespace {
// ---- draws: u = (word + 0.5) 2^-32 of Philox4x32-10 at counter (index, variable, generation, purpose) under (seed_lo, seed_hi ^ tag) ----
struct Draw4 { double u[4]; };
__device__ __forceinline__ Draw4 ga_draw(const GaParams& g, uint32_t index, uint32_t var, uint32_t generation, uint32_t purpose) {
    uint32_t c[4] = {index, var, generation, purpose};
    philox4x32_10(c, (uint32_t)(g.seed & 0xFFFFFFFFu), (uint32_t)(g.seed >> 32) ^ GLASS_SEARCH_TAG);
    Draw4 d;
#pragma unroll
    for (int i = 0; i < 4; ++i) d.u[i] = ((double)c[i] + 0.5) * (1.0 / 4294967296.0);
    return d;
}
// the raw first word of the same block (the bit key of a mixed row's HUX)
__device__ __forceinline__ uint32_t ga_word(const GaParams& g, uint32_t index, uint32_t var, uint32_t generation, uint32_t purpose) {
    uint32_t c[4] = {index, var, generation, purpose};
    philox4x32_10(c, (uint32_t)(g.seed & 0xFFFFFFFFu), (uint32_t)(g.seed >> 32) ^ GLASS_SEARCH_TAG);
    return c[0];
}

// the winner of a binary tournament between rows a and b: lower rank, then larger crowding distance, `>=` going to a (search.py:221)
__device__ __forceinline__ int ga_better(const int* rank, const double* cd, int a, int b) {
    const int ra = rank[a], rb = rank[b];
    return (ra < rb || (ra == rb && cd[a] >= cd[b])) ? a : b;
}
__device__ __forceinline__ void ga_parents(const GaParams& g, const int* rank, const double* cd, int m, uint32_t generation, int* pa, int* pb) {
    const Draw4 d = ga_draw(g, (uint32_t)m, 0u, generation, GLASS_SEARCH_DRAW_TOURNAMENT);
    int idx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) idx[i] = min((int)floor(d.u[i] * (double)g.pop), g.pop - 1);
    *pa = ga_better(rank, cd, idx[0], idx[1]);
    *pb = ga_better(rank, cd, idx[2], idx[3]);
}

// One variable of one offspring row: the child of (pa, pb) this row keeps (child 0: the first, 1: the second), mutated, rounded ONCE to
// fp32.  Double arithmetic in search.py's own order of operations, without fused multiply-adds: a float64 mirror then agrees to the last
// bits of pow().
__device__ float ga_vary_one(const GaParams& g, float paf, float pbf, int m, int r, int j, uint32_t generation) {
#pragma clang fp contract(off)
    const double pa = (double)paf, pb = (double)pbf, xl = g.xl, xu = g.xu;
    const Draw4 s = ga_draw(g, (uint32_t)m, (uint32_t)j, generation, GLASS_SEARCH_DRAW_SBX);      // u[0] beta, u[1] swap, u[2] per-variable gate
    const double y1 = fmin(pa, pb), y2 = fmax(pa, pb);
    double x = (r & 1) ? pb : pa;
    if (s.u[2] < 0.5 && (y2 - y1) > 1e-14) {
        const double d = fmax(y2 - y1, 1e-300), u = s.u[0], ex = 1.0 / (g.eta_c + 1.0);
        const double bound1 = 1.0 + 2.0 * (y1 - xl) / d, bound2 = 1.0 + 2.0 * (xu - y2) / d;
        const double alpha1 = 2.0 - pow(bound1, -(g.eta_c + 1.0)), alpha2 = 2.0 - pow(bound2, -(g.eta_c + 1.0));
        const double bq1 = u <= 1.0 / alpha1 ? pow(u * alpha1, ex) : pow(1.0 / fmax(2.0 - u * alpha1, 1e-300), ex);
        const double bq2 = u <= 1.0 / alpha2 ? pow(u * alpha2, ex) : pow(1.0 / fmax(2.0 - u * alpha2, 1e-300), ex);
        const double c1 = fmin(fmax(0.5 * ((y1 + y2) - bq1 * d), xl), xu);
        const double c2 = fmin(fmax(0.5 * ((y1 + y2) + bq2 * d), xl), xu);
        const bool swap = s.u[1] < 0.5;
        x = ((r & 1) != 0) == swap ? c1 : c2;      // child 0 keeps c1 unless swapped, child 1 keeps c2 unless swapped
    }
    const Draw4 q = ga_draw(g, (uint32_t)r, (uint32_t)j, generation, GLASS_SEARCH_DRAW_MUTATION);  // u[0] the perturbation, u[1] the gate
    if (q.u[1] < g.prob_m) {
        const double span = xu - xl, u = q.u[0], ep = g.eta_m + 1.0, mpow = 1.0 / ep;
        const double d1 = (x - xl) / span, d2 = (xu - x) / span;
        const double dq = u <= 0.5 ? pow(2.0 * u + (1.0 - 2.0 * u) * pow(1.0 - d1, ep), mpow) - 1.0
                                   : 1.0 - pow(2.0 * (1.0 - u) + 2.0 * (u - 0.5) * pow(1.0 - d2, ep), mpow);
        x = fmin(fmax(x + dq * span, xl), xu);
    }
    return (float)x;
}

// grid (ceil(n_var / (256 VEC)), rows): offspring row r = row0 + blockIdx.y is child r & 1 of mating r >> 1.  The rows are `stride` floats
// apart and columns [0, n_var) of them are varied (an all-real row: stride = n_var; a mixed row: its real columns).  VEC 4 where n_var % 4
// == 0 and stride % 4 == 0 (every row is then 16-byte aligned), 1 otherwise.  Nothing depends on the grid: a draw is a function of (seed,
// generation, row, variable).
template <int VEC>
__device__ __forceinline__ void ga_vary_row(const float* __restrict__ X, const int* __restrict__ rank, const double* __restrict__ cd, const GaParams& g,
                                            int n_var, int stride, int generation, int r, float* __restrict__ Xoff) {
    const int m = r >> 1;
    const int j0 = (blockIdx.x * 256 + threadIdx.x) * VEC;
    if (j0 >= n_var) return;
    int ia, ib;
    ga_parents(g, rank, cd, m, (uint32_t)generation, &ia, &ib);
    const float* pa = X + (size_t)ia * stride + j0;
    const float* pb = X + (size_t)ib * stride + j0;
    float* out = Xoff + (size_t)r * stride + j0;
    if (VEC == 4) {
        const f4 a = *(const f4*)pa, b = *(const f4*)pb;
        f4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = ga_vary_one(g, a[i], b[i], m, r, j0 + i, (uint32_t)generation);
        *(f4*)out = o;
    } else {
        out[0] = ga_vary_one(g, pa[0], pb[0], m, r, j0, (uint32_t)generation);
    }
}
// The island is the last grid dimension in every kernel of a phase (include/glass.h "Device search: islands"), here grid (ceil(n_var / (256
// VEC)), rows, islands): island i = blockIdx.z works on rows [i pop, (i + 1) pop) of every buffer under seed + i, and every index inside is
// local to the island.  A single search is the one island 0.
template <int VEC>
__global__ __launch_bounds__(256) void ga_vary_kernel(const float* __restrict__ X, const int* __restrict__ rank, const double* __restrict__ cd,
                                                      GaParams g, int n_var, int stride, int generation, int row0, float* __restrict__ Xoff) {
    const size_t o = (size_t)blockIdx.z * g.pop;
    g.seed += (uint64_t)blockIdx.z;
    ga_vary_row<VEC>(X + o * stride, rank + o, cd + o, g, n_var, stride, generation, row0 + blockIdx.y, Xoff + o * stride);
}

// One workgroup per offspring row r; its four waves walk the candidate rows (the population, then offspring rows BELOW r — "earlier" is the
// row index, whatever the schedule).  A pair is compared 64 VEC variables at a time and left at the first chunk that differs, which for
// unrelated rows is the first: the whole of both rows is read only for a pair that is equal.  Equality is by value (-0.0 == 0.0).
// whether row a equals, by value in every variable, row b: the whole wave compares 64 VEC variables at a time and leaves at the first chunk
// that differs (uniform over the wave)
template <int VEC>
__device__ __forceinline__ bool ga_rows_equal(const float* __restrict__ a, const float* __restrict__ b, int n_var, int lane) {
    bool eq = true;
    for (int j0 = 0; j0 < n_var && eq; j0 += 64 * VEC) {
        const int j = j0 + lane * VEC;
        bool ne = false;
        if (j < n_var) {
            if (VEC == 4) {
                const f4 va = *(const f4*)(a + j), vb = *(const f4*)(b + j);
                ne = !(va[0] == vb[0] && va[1] == vb[1] && va[2] == vb[2] && va[3] == vb[3]);
            } else {
                ne = !(a[j] == b[j]);
            }
        }
        eq = __ballot(ne) == 0ull;
    }
    return eq;
}
template <int VEC>
__device__ __forceinline__ void ga_duplicates_row(const float* __restrict__ X, const float* __restrict__ Xoff, int pop, int n_var, int r,
                                                  int* __restrict__ flags) {
    __shared__ int hit[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* a = Xoff + (size_t)r * n_var;
    bool found = false;
    for (int c = wave; c < pop + r && !found; c += 4)
        found = ga_rows_equal<VEC>(a, c < pop ? X + (size_t)c * n_var : Xoff + (size_t)(c - pop) * n_var, n_var, lane);
    if (lane == 0) hit[wave] = found ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) flags[r] = hit[0] | hit[1] | hit[2] | hit[3];
}
// grid (n_off, islands): an offspring row is compared with its own island's rows only
template <int VEC>
__global__ __launch_bounds__(256) void ga_duplicates_kernel(const float* __restrict__ X, const float* __restrict__ Xoff, int pop, int n_off, int n_var,
                                                            int* __restrict__ flags) {
    const size_t o = (size_t)blockIdx.y * pop, oo = (size_t)blockIdx.y * n_off;
    ga_duplicates_row<VEC>(X + o * n_var, Xoff + oo * n_var, pop, n_var, blockIdx.x, flags + oo);
}

// ---- survival: one workgroup, everything in LDS -------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ga_fkey(float f) {      // order-preserving bits of a float; -0.0 and 0.0 share a key (they tie, by index)
    const uint32_t u = __float_as_uint(f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ void ga_sort(unsigned long long* keys, int N2) {      // bitonic, ascending; the keys are distinct (they end in the row index)
    for (int k = 2; k <= N2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (N2 >> 1); t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long a = keys[i], b = keys[l];
                if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
}
__device__ __forceinline__ bool ga_dominates(const float* Fs, int M, int i, int j) {
    bool all_le = true, any_lt = false;
    for (int k = 0; k < M; ++k) {
        const float a = Fs[i * M + k], b = Fs[j * M + k];
        all_le = all_le && a <= b;
        any_lt = any_lt || a < b;
    }
    return all_le && any_lt;
}

__host__ __device__ inline int ga_pow2(int n) { int p = 2; while (p < n) p <<= 1; return p; }

// The bit columns [n_real, n_real + n_bits) of offspring row r = row0 + blockIdx.x (include/glass.h "Mixed rows"): half-uniform crossover of
// the mating's parents, then bit-flip.  One workgroup per row; both children of a mating redo the selection, so a slice of rows stands
// alone.  The differing columns D go to LDS as (key << 32 | column) in whatever order the atomics give — only the keys' ranks matter —
// padded to a power of two and sorted; the first (|D| + 1) >> 1 of them are exchanged.  LDS holds the worst case (|D| = n_bits <=
// GLASS_SEARCH_MAX_BITS), the sort runs over the actual |D|.
__device__ __forceinline__ void ga_vary_bits_row(const float* __restrict__ X, const int* __restrict__ rank, const double* __restrict__ cd,
                                                 const GaParams& g, int n_real, int n_bits, int generation, int r, float* __restrict__ Xoff) {
#pragma clang fp contract(off)
    __shared__ unsigned long long keys[GLASS_SEARCH_MAX_BITS];
    __shared__ unsigned char xchg[GLASS_SEARCH_MAX_BITS];
    __shared__ int s_n;
    const int m = r >> 1, child = r & 1, stride = n_real + n_bits, tid = threadIdx.x;
    int ia, ib;
    ga_parents(g, rank, cd, m, (uint32_t)generation, &ia, &ib);
    const float* A = X + (size_t)ia * stride + n_real;
    const float* B = X + (size_t)ib * stride + n_real;
    float* out = Xoff + (size_t)r * stride + n_real;
    const bool open = ga_draw(g, (uint32_t)m, 0u, (uint32_t)generation, GLASS_SEARCH_DRAW_BIT_GATE).u[0] < g.prob_x;      // uniform over the workgroup
    if (tid == 0) s_n = 0;
    for (int j = tid; j < n_bits; j += 256) xchg[j] = 0;
    __syncthreads();
    if (open) {
        for (int j = tid; j < n_bits; j += 256)
            if (A[j] != B[j]) {
                const uint32_t col = (uint32_t)(n_real + j);
                keys[atomicAdd(&s_n, 1)] = ((unsigned long long)ga_word(g, (uint32_t)m, col, (uint32_t)generation, GLASS_SEARCH_DRAW_BIT_KEY) << 32) | col;
            }
        __syncthreads();
        const int nD = s_n, take = (nD + 1) >> 1;
        if (nD > 1) {      // (one differing column is exchanged whatever its key)
            const int N2 = ga_pow2(nD);
            for (int i = nD + tid; i < N2; i += 256) keys[i] = ~0ull;
            __syncthreads();
            ga_sort(keys, N2);
        }
        for (int p = tid; p < take; p += 256) xchg[(int)(keys[p] & 0xFFFFFFFFu) - n_real] = 1;
        __syncthreads();
    }
    for (int j = tid; j < n_bits; j += 256) {
        const float a = A[j], b = B[j];
        float x = (child != 0) == (xchg[j] != 0) ? a : b;      // child 0 keeps A's bit and child 1 B's, unless the column is exchanged
        if (ga_draw(g, (uint32_t)r, (uint32_t)(n_real + j), (uint32_t)generation, GLASS_SEARCH_DRAW_BIT_FLIP).u[0] < g.prob_flip) x = 1.0f - x;
        out[j] = x;
    }
}
// grid (rows, islands): local rows and matings under seed + island
__global__ __launch_bounds__(256) void ga_vary_bits_kernel(const float* __restrict__ X, const int* __restrict__ rank, const double* __restrict__ cd,
                                                           GaParams g, int n_real, int n_bits, int generation, int row0, float* __restrict__ Xoff) {
    const size_t o = (size_t)blockIdx.y * g.pop, stride = (size_t)(n_real + n_bits);
    g.seed += (uint64_t)blockIdx.y;
    ga_vary_bits_row(X + o * stride, rank + o, cd + o, g, n_real, n_bits, generation, row0 + blockIdx.x, Xoff + o * stride);
}

// The merged rows are Fpop [n_pop][M], the population's, then Foff [n_off][M], the offspring's.  Left out of survival: offspring rows with a
// flag or a non-finite F.  Out: chosen [pop_out] merged indices in survival order (-1: fewer rows than pop_out were eligible), their rank
// and distance, and Fout's first pop_out rows written as the survivors' (Fout may be Fpop: the workgroup has read every F before it
// writes).  counts = {flagged, non-finite rows} (nullable).
__device__ __forceinline__ void ga_survive_rows(const float* Fpop, const float* Foff, float* Fout, const int* __restrict__ flags, int n_pop, int n_off,
                                                int M, int pop_out, int nsga, int* __restrict__ chosen, int* __restrict__ rank_out,
                                                double* __restrict__ cd_out, int* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_ncur, s_cnt[2];
    const int N = n_pop + n_off, N2 = ga_pow2(N), T = blockDim.x, tid = threadIdx.x;
    unsigned long long* keys = (unsigned long long*)smem;        // [N2]
    double* cd = (double*)(keys + N2);                           // [N]
    float* Fs = (float*)(cd + N);                                // [N][M]
    int* rk = (int*)(Fs + (size_t)N * M);                        // [N]: front, -1 not ranked, -2 left out
    int* nd = rk + N;                                            // [N]: rows that dominate it and are not ranked yet
    int* cur = nd + N;                                           // [N]: the current front; later the survivors by slot
    int* seg = cur + N;                                          // [N + 2]: first sorted position of every front
    for (int i = tid; i < N * M; i += T) Fs[i] = i < n_pop * M ? Fpop[i] : Foff[i - n_pop * M];
    if (tid == 0) s_cnt[0] = s_cnt[1] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += T) {
        bool fin = true;
        for (int k = 0; k < M; ++k) fin = fin && isfinite(Fs[i * M + k]);
        const bool flg = i >= n_pop && flags && flags[i - n_pop] != 0;
        if (flg) atomicAdd(&s_cnt[0], 1);
        if (!fin) atomicAdd(&s_cnt[1], 1);
        rk[i] = (i < n_pop || (!flg && fin)) ? -1 : -2;
        cd[i] = 0.0;
    }
    __syncthreads();
    if (!nsga) {      // GA: the first pop_out rows by (F0, index); rank 0, distance -F0
        for (int i = tid; i < N2; i += T)
            keys[i] = (i < N && rk[i] == -1) ? (((unsigned long long)ga_fkey(Fs[i * M]) << 32) | (unsigned)i) : ~0ull;
        __syncthreads();
        ga_sort(keys, N2);
        for (int s = tid; s < pop_out; s += T) {
            const bool ok = s < N2 && keys[s] != ~0ull;
            const int i = ok ? (int)(keys[s] & 0xFFFFFFFFu) : -1;
            cur[s] = i;
            if (ok) { rk[i] = 0; cd[i] = -(double)Fs[i * M]; }
        }
        __syncthreads();
    } else {
        // domination counts
        for (int j = tid; j < N; j += T) {
            int c = 0;
            if (rk[j] == -1)
                for (int i = 0; i < N; ++i) c += (rk[i] == -1 && ga_dominates(Fs, M, i, j)) ? 1 : 0;
            nd[j] = c;
        }
        // front peeling, until pop_out rows are ranked: a chain of short steps between workgroup barriers
        int r = 0, ranked = 0;
        while (true) {
            if (tid == 0) s_ncur = 0;
            __syncthreads();
            for (int j = tid; j < N; j += T)
                if (rk[j] == -1 && nd[j] == 0) cur[atomicAdd(&s_ncur, 1)] = j;
            __syncthreads();
            const int ncur = s_ncur;
            if (ncur == 0) break;
            for (int p = tid; p < ncur; p += T) rk[cur[p]] = r;
            __syncthreads();
            ranked += ncur;
            ++r;
            if (ranked >= pop_out) break;
            for (int j = tid; j < N; j += T)
                if (rk[j] == -1) {
                    int c = 0;
                    for (int p = 0; p < ncur; ++p) c += ga_dominates(Fs, M, cur[p], j) ? 1 : 0;
                    nd[j] -= c;
                }
            __syncthreads();
        }
        const int n_fronts = r;
        __syncthreads();
        // crowding of every front at once: one sort per objective keyed (front, F_k, index); the distance is summed in objective order
        for (int k = 0; k < M; ++k) {
            for (int i = tid; i < N2; i += T)
                keys[i] = (i < N && rk[i] >= 0)
                              ? (((unsigned long long)rk[i] << 44) | ((unsigned long long)ga_fkey(Fs[i * M + k]) << 12) | (unsigned)i) : ~0ull;
            __syncthreads();
            ga_sort(keys, N2);
            if (k == 0) {
                for (int p = tid; p < ranked; p += T) {
                    const int rr = (int)(keys[p] >> 44);
                    if (p == 0 || (int)(keys[p - 1] >> 44) != rr) seg[rr] = p;
                }
                if (tid == 0) seg[n_fronts] = ranked;
                __syncthreads();
            }
            for (int p = tid; p < ranked; p += T) {
                const int rr = (int)(keys[p] >> 44), i = (int)(keys[p] & 0xFFFu), s0 = seg[rr], s1 = seg[rr + 1];
                if (s1 - s0 <= 2 || p == s0 || p == s1 - 1) {
                    cd[i] = INFINITY;
                } else {
                    const double span = (double)Fs[(int)(keys[s1 - 1] & 0xFFFu) * M + k] - (double)Fs[(int)(keys[s0] & 0xFFFu) * M + k];
                    if (span > 0.0)
                        cd[i] += ((double)Fs[(int)(keys[p + 1] & 0xFFFu) * M + k] - (double)Fs[(int)(keys[p - 1] & 0xFFFu) * M + k]) / span;
                }
            }
            __syncthreads();
        }
        // slots: the fronts in order, rows by index; the front that does not fit is cut by (-distance, index)
        for (int s = tid; s < pop_out; s += T) cur[s] = -1;
        __syncthreads();
        for (int i = tid; i < N; i += T) {
            const int rr = rk[i];
            if (rr < 0 || seg[rr] >= pop_out) continue;
            const bool cut = seg[rr + 1] > pop_out;
            const double ci = cd[i];
            int c = 0;
            for (int o = 0; o < N; ++o)
                if (rk[o] == rr) c += cut ? ((cd[o] > ci || (cd[o] == ci && o < i)) ? 1 : 0) : (o < i ? 1 : 0);
            if (seg[rr] + c < pop_out) cur[seg[rr] + c] = i;
        }
        __syncthreads();
    }
    for (int s = tid; s < pop_out; s += T) {
        const int i = cur[s];
        chosen[s] = i;
        rank_out[s] = i >= 0 ? rk[i] : -1;
        cd_out[s] = i >= 0 ? cd[i] : 0.0;
        if (i >= 0)
            for (int k = 0; k < M; ++k) Fout[s * M + k] = Fs[i * M + k];
    }
    if (tid == 0 && counts) { counts[0] = s_cnt[0]; counts[1] = s_cnt[1]; }
}
// One workgroup per island: island i ranks its n_pop population rows of F with its n_off offspring rows of Foff — two planes, the pass
// writes the islands' offspring F contiguously; a single search's Foff is F + n_pop M, which aliases F (hence no __restrict__ on the two:
// the barriers of ga_survive_rows stand between every read and the writes) — and rewrites its first pop_out rows of F, chosen, rank and cd.
// counts [islands][3] = {flagged, non-finite, migrants accepted}.  gated (the ranking behind a migration; n_off 0, pop_out = n_pop): an
// island that accepted no migrant keeps every bit of its state — ranking a population again would reorder a cut last front — and gets the
// identity for the gather; the first two counters stay the generation's.
__global__ __launch_bounds__(1024) void ga_survive_kernel(float* F, const float* Foff, const int* __restrict__ flags, int n_pop, int n_off, int M,
                                                          int pop_out, int nsga, int gated, int* __restrict__ chosen, int* __restrict__ rank_out,
                                                          double* __restrict__ cd_out, int* __restrict__ counts) {
    // (a nullable pointer is null only where its island stride is 0 or the island is 0 — the launcher sees to it — so the offsets need no test)
    const size_t isl = blockIdx.x, o = isl * pop_out;
    int* cnt = counts + isl * 3;
    if (gated && cnt[2] == 0) {      // (uniform over the workgroup, ahead of every barrier)
        for (int s = threadIdx.x; s < pop_out; s += blockDim.x) chosen[o + s] = s;
        return;
    }
    F += isl * n_pop * M;
    ga_survive_rows(F, Foff + isl * n_off * M, F, flags + isl * n_off, n_pop, n_off, M, pop_out, nsga, chosen + o, rank_out + o, cd_out + o,
                    gated ? nullptr : cnt);
}

// Xnext[s] = the merged row chosen[s] of (X ; Xoff), island by island: chosen holds island-local merged indices and an island's offspring
// rows lie n_pop rows apart, as its population's.  grid (ceil(n_var / (256 VEC)), pop_out, islands)
template <int VEC>
__global__ __launch_bounds__(256) void ga_gather_kernel(const float* __restrict__ X, const float* __restrict__ Xoff, const int* __restrict__ chosen,
                                                        int n_pop, int pop_out, int n_var, float* __restrict__ Xnext) {
    const size_t o = (size_t)blockIdx.z * n_pop, oo = (size_t)blockIdx.z * pop_out;
    const int s = blockIdx.y, j0 = (blockIdx.x * 256 + threadIdx.x) * VEC, i = chosen[oo + s];
    if (j0 >= n_var || i < 0) return;
    const float* src = (i < n_pop ? X + (o + i) * n_var : Xoff + (o + i - n_pop) * n_var) + j0;
    float* dst = Xnext + (oo + s) * n_var + j0;
    if (VEC == 4) *(f4*)dst = *(const f4*)src;
    else dst[0] = src[0];
}

// ---- migration (include/glass.h "Device search: islands") -----------------------------------------------------------------------
// position of row a in the tournament's order (rank, -cd, index) of an island whose rank / cd lie in LDS
__device__ __forceinline__ int ga_order_pos(const int* rk, const double* cd, int pop, int a) {
    const int ra = rk[a];
    const double ca = cd[a];
    int c = 0;
    for (int b = 0; b < pop; ++b) {
        const int rb = rk[b];
        const double cb = cd[b];
        c += (rb < ra || (rb == ra && (cb > ca || (cb == ca && b < a)))) ? 1 : 0;
    }
    return c;
}
// One workgroup per RECEIVING island i; its source is island (i - 1 + K) mod K.  Candidate k is the source's k-th best row and is aimed at
// the receiver's k-th worst.  Sixteen waves walk the candidates; a candidate is compared (ga_rows_equal) with the receiver's pop rows and
// with the candidates below k, and only then — behind a barrier — are the accepted rows and their F copied.  With n <= pop / 2 the rows a
// workgroup writes (its island's n worst) are never rows another workgroup reads (that island's n best, and only the receiver reads the
// rest), so every source is read as survival left it whatever the schedule.  counts[i][2] = accepted migrants.
template <int VEC>
__global__ __launch_bounds__(1024) void ga_migrate_kernel(float* X, float* F, const int* __restrict__ rank,
                                                          const double* __restrict__ cd, int K, int pop, int n_var, int M, int n,
                                                          int* __restrict__ counts) {
    __shared__ double s_cd[GLASS_SEARCH_MAX_POP];
    __shared__ int s_rk[GLASS_SEARCH_MAX_POP];
    __shared__ int s_src[GLASS_SEARCH_MAX_POP / 2], s_dst[GLASS_SEARCH_MAX_POP / 2];
    __shared__ int s_ok[GLASS_SEARCH_MAX_POP / 2];
    const int isl = blockIdx.x, from = (isl - 1 + K) % K, tid = threadIdx.x, T = blockDim.x;
    const size_t o_to = (size_t)isl * pop, o_from = (size_t)from * pop;
    // the source's n best rows
    for (int a = tid; a < pop; a += T) { s_rk[a] = rank[o_from + a]; s_cd[a] = cd[o_from + a]; }
    __syncthreads();
    for (int a = tid; a < pop; a += T) {
        const int p = ga_order_pos(s_rk, s_cd, pop, a);
        if (p < n) s_src[p] = a;
    }
    __syncthreads();
    // the receiver's n worst rows, worst first
    for (int a = tid; a < pop; a += T) { s_rk[a] = rank[o_to + a]; s_cd[a] = cd[o_to + a]; }
    __syncthreads();
    for (int a = tid; a < pop; a += T) {
        const int p = pop - 1 - ga_order_pos(s_rk, s_cd, pop, a);
        if (p < n) s_dst[p] = a;
    }
    __syncthreads();
    const float* Xs = X + o_from * n_var;
    float* Xr = X + o_to * n_var;
    const int wave = tid >> 6, lane = tid & 63;
    for (int k = wave; k < n; k += (T >> 6)) {
        const float* a = Xs + (size_t)s_src[k] * n_var;
        bool found = false;
        for (int c = 0; c < pop + k && !found; ++c)
            found = ga_rows_equal<VEC>(a, c < pop ? Xr + (size_t)c * n_var : Xs + (size_t)s_src[c - pop] * n_var, n_var, lane);
        if (lane == 0) s_ok[k] = found ? 0 : 1;
    }
    __syncthreads();
    int accepted = 0;
    for (int k = 0; k < n; ++k) {
        if (!s_ok[k]) continue;
        ++accepted;
        const float* src = Xs + (size_t)s_src[k] * n_var;
        float* dst = Xr + (size_t)s_dst[k] * n_var;
        for (int j = tid * VEC; j < n_var; j += T * VEC) {
            if (VEC == 4) *(f4*)(dst + j) = *(const f4*)(src + j);
            else dst[j] = src[j];
        }
        if (tid < M) F[(o_to + s_dst[k]) * M + tid] = F[(o_from + s_src[k]) * M + tid];
    }
    if (tid == 0) counts[isl * 3 + 2] = accepted;
}
}  // namespace

size_t ga_survive_lds_bytes(int n_rows, int n_obj) {
    const size_t N = (size_t)n_rows, N2 = (size_t)ga_pow2(n_rows);
    return N2 * 8 + N * 8 + N * (size_t)n_obj * 4 + 3 * N * 4 + (N + 2) * 4;
}

// One island: nothing beyond each launcher's own limits (a single search, and the diagnostic ops' shapes).  More: the island search's
// limits (include/glass.h "Device search: islands").  nullptr from a launcher: the shape is outside them, nothing was launched.
static bool ga_islands_ok(int islands, int pop, int n_var) {
    return islands == 1 || (islands >= 2 && islands <= GLASS_SEARCH_MAX_ISLANDS && pop >= 2 && pop <= GLASS_SEARCH_MAX_POP && n_var >= 1 &&
                            (long long)islands * pop * n_var < (1LL << 31));
}

const char* launch_ga_vary(const float* X, const int* rank, const double* cd, const GaParams& g, int islands, int n_real, int n_bits, int generation,
                           int row0, int rows, int parts, float* Xoff, hipStream_t st) {
    const int stride = n_real + n_bits;
    if (rows <= 0 || row0 < 0 || row0 + rows > g.pop || n_real < 1 || n_bits < 0 || n_bits > GLASS_SEARCH_MAX_BITS || !(parts & GA_VARY_BOTH) ||
        ((parts & GA_VARY_BITS) && n_bits < 1) || !ga_islands_ok(islands, g.pop, stride))
        return nullptr;
    const bool v4 = n_real % 4 == 0 && stride % 4 == 0;      // (every row is then 16-byte aligned)
    if (parts & GA_VARY_REAL) {
        if (v4)
            hipLaunchKernelGGL(ga_vary_kernel<4>, dim3((n_real / 4 + 255) / 256, rows, islands), dim3(256), 0, st, X, rank, cd, g, n_real, stride, generation,
                               row0, Xoff);
        else
            hipLaunchKernelGGL(ga_vary_kernel<1>, dim3((n_real + 255) / 256, rows, islands), dim3(256), 0, st, X, rank, cd, g, n_real, stride, generation,
                               row0, Xoff);
    }
    if (parts & GA_VARY_BITS)
        hipLaunchKernelGGL(ga_vary_bits_kernel, dim3(rows, islands), dim3(256), 0, st, X, rank, cd, g, n_real, n_bits, generation, row0, Xoff);
    if (!(parts & GA_VARY_BITS)) return v4 ? "ga_vary_kernel<4>" : "ga_vary_kernel<1>";
    if (!(parts & GA_VARY_REAL)) return "ga_vary_bits_kernel";
    return v4 ? "ga_vary_kernel<4> + ga_vary_bits_kernel" : "ga_vary_kernel<1> + ga_vary_bits_kernel";
}

const char* launch_ga_duplicates(const float* X, const float* Xoff, int islands, int pop, int n_off, int n_var, int* flags, hipStream_t st) {
    if (pop < 0 || n_off <= 0 || n_var <= 0 || !ga_islands_ok(islands, pop, n_var) || (islands > 1 && n_off != pop)) return nullptr;
    if (n_var % 4 == 0) {
        hipLaunchKernelGGL(ga_duplicates_kernel<4>, dim3(n_off, islands), dim3(256), 0, st, X, Xoff, pop, n_off, n_var, flags);
        return "ga_duplicates_kernel<4>";
    }
    hipLaunchKernelGGL(ga_duplicates_kernel<1>, dim3(n_off, islands), dim3(256), 0, st, X, Xoff, pop, n_off, n_var, flags);
    return "ga_duplicates_kernel<1>";
}

const char* launch_ga_survive(float* F, const float* Foff, const int* flags, int islands, int n_pop, int n_off, int n_obj, int pop_out, int nsga, int gated,
                              int* chosen, int* rank_out, double* cd_out, int* counts, hipStream_t st) {
    const int N = n_pop + n_off;
    if (n_pop < 1 || n_off < 0 || N > 2 * GLASS_SEARCH_MAX_POP || n_obj < 1 || n_obj > GLASS_SEARCH_MAX_OBJ || pop_out < 1 || pop_out > N ||
        pop_out > GLASS_SEARCH_MAX_POP || (n_off && !Foff) || (gated && (n_off || pop_out != n_pop || !counts)))
        return nullptr;
    // (more islands: an island's first pop_out rows of F stay inside its own n_pop, and the kernel offsets flags and counts untested)
    if (!ga_islands_ok(islands, n_pop, 1) || (islands > 1 && ((n_off && (n_off != n_pop || !flags)) || pop_out != n_pop || !counts))) return nullptr;
    const size_t lds = ga_survive_lds_bytes(N, n_obj);
    if (lds > 64 * 1024) {
        if (!glass_lds_fits((int)lds)) return nullptr;
        static DevOnce once;
        once.run([&] {
            (void)hipFuncSetAttribute((const void*)ga_survive_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)ga_survive_lds_bytes(2 * GLASS_SEARCH_MAX_POP, GLASS_SEARCH_MAX_OBJ));
        });
    }
    hipLaunchKernelGGL(ga_survive_kernel, dim3(islands), dim3(1024), lds, st, F, Foff, flags, n_pop, n_off, n_obj, pop_out, nsga, gated, chosen, rank_out,
                       cd_out, counts);
    return "ga_survive_kernel";
}

void launch_ga_gather(const float* X, const float* Xoff, const int* chosen, int islands, int n_pop, int pop_out, int n_var, float* Xnext, hipStream_t st) {
    if (n_var % 4 == 0)
        hipLaunchKernelGGL(ga_gather_kernel<4>, dim3((n_var / 4 + 255) / 256, pop_out, islands), dim3(256), 0, st, X, Xoff, chosen, n_pop, pop_out, n_var,
                           Xnext);
    else
        hipLaunchKernelGGL(ga_gather_kernel<1>, dim3((n_var + 255) / 256, pop_out, islands), dim3(256), 0, st, X, Xoff, chosen, n_pop, pop_out, n_var, Xnext);
}

const char* launch_ga_migrate(float* X, float* F, const int* rank, const double* cd, int islands, int pop, int n_var, int n_obj, int migrants, int* counts,
                              hipStream_t st) {
    if (islands < 2 || !ga_islands_ok(islands, pop, n_var) || migrants < 1 || migrants > pop / 2 || n_obj < 1 || n_obj > GLASS_SEARCH_MAX_OBJ) return nullptr;
    if (n_var % 4 == 0) {
        hipLaunchKernelGGL(ga_migrate_kernel<4>, dim3(islands), dim3(1024), 0, st, X, F, rank, cd, islands, pop, n_var, n_obj, migrants, counts);
        return "ga_migrate_kernel<4>";
    }
    hipLaunchKernelGGL(ga_migrate_kernel<1>, dim3(islands), dim3(1024), 0, st, X, F, rank, cd, islands, pop, n_var, n_obj, migrants, counts);
    return "ga_migrate_kernel<1>";
}
