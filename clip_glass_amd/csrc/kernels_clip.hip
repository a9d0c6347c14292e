// kernels_clip.hip — CLIP ViT glue kernels: token assembly + ln_pre, LayerNorm,
// multi-head attention (whole-sequence MFMA kernels for L <= 96: 50 visual tokens, 77 text tokens; a streaming one above that).
// GEMMs live in conv_direct.hip / gemm_tiled.hip; the cosine and the rows of F in score.hip.
// Reference: clip/model.py:152-187 (LayerNorm, QuickGELU, ResidualAttentionBlock),
// :218-235 (VisualTransformer.forward).
#include "common.h"
#include "kernels.h"
#include <stdlib.h>

// One wave per row; two-pass mean/variance in fp32 (clip/model.py:152-158, eps 1e-5).  Rows up to 1024 wide are read from
// global memory ONCE and held in registers (16 values per lane) for the three passes.
template <typename LoadF>
__device__ __forceinline__ void ln_row(LoadF load, int D, const float* g, const float* b, half_t* o16, float* o32) {
    const int lane = threadIdx.x & 63;
    if (D <= 1024) {
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = lane + 64 * k < D ? load(lane + 64 * k) : 0.f;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += v[k];
        const float mean = wave_sum(s) / (float)D;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) { const float d = lane + 64 * k < D ? v[k] - mean : 0.f; q += d * d; }
        const float rstd = rsqrtf(wave_sum(q) / (float)D + 1e-5f);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = lane + 64 * k;
            if (i < D) {
                const float o = (v[k] - mean) * rstd * g[i] + b[i];
                if (o16) o16[i] = (half_t)o;
                if (o32) o32[i] = o;
            }
        }
        return;
    }
    float s = 0.f;
    for (int i = lane; i < D; i += 64) s += load(i);
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int i = lane; i < D; i += 64) { const float d = load(i) - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + 1e-5f);
    for (int i = lane; i < D; i += 64) {
        const float v = (load(i) - mean) * rstd * g[i] + b[i];
        if (o16) o16[i] = (half_t)v;
        if (o32) o32[i] = v;
    }
}

// x[p][0] = class_embedding + pos[0]; x[p][1+t] = patch_emb[p*T0+t] + pos[1+t]; then ln_pre.
__global__ __launch_bounds__(256) void embed_lnpre_kernel(const float* pe, const float* cls, const float* pos,
                                                          const float* g, const float* b, int P, int T, int D,
                                                          float* x) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= P * T) return;
    const int p = row / T, t = row - p * T;
    const float* src = t == 0 ? cls : pe + ((long long)p * (T - 1) + (t - 1)) * D;
    const float* ps = pos + (long long)t * D;
    ln_row([&](int i) { return src[i] + ps[i]; }, D, g, b, nullptr, x + (long long)row * D);
}
void launch_embed_lnpre(const float* patch_emb, const float* cls, const float* pos, const float* g,
                        const float* b, int P, int T, int D, float* x, hipStream_t st) {
    hipLaunchKernelGGL(embed_lnpre_kernel, dim3((P * T + 3) / 4), dim3(256), 0, st, patch_emb, cls, pos, g, b, P,
                       T, D, x);
}

// token + positional embedding of the text tower (clip/model.py:308-310)
__global__ void embed_text_kernel(const int* tokens, const float* tok_emb, const float* pos, int ctx, int D, float* x) {
    const int row = blockIdx.x;
    const float* te = tok_emb + (long long)tokens[row] * D;
    const float* pe = pos + (long long)(row % ctx) * D;
    for (int i = threadIdx.x; i < D; i += blockDim.x) x[(long long)row * D + i] = te[i] + pe[i];
}
void launch_embed_text(const int* tokens, const float* tok_emb, const float* pos, int n_rows, int ctx, int D, float* x,
                       hipStream_t st) {
    hipLaunchKernelGGL(embed_text_kernel, dim3(n_rows), dim3(128), 0, st, tokens, tok_emb, pos, ctx, D, x);
}

__global__ __launch_bounds__(256) void layernorm_kernel(const float* x, long long row_stride, int M, int D,
                                                        const float* g, const float* b, half_t* o16, float* o32) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + (long long)row * row_stride;
    ln_row([&](int i) { return xr[i]; }, D, g, b, o16 ? o16 + (long long)row * D : nullptr,
           o32 ? o32 + (long long)row * D : nullptr);
}
void launch_layernorm(const float* x, long long row_stride, int M, int D, const float* g, const float* b,
                      half_t* out16, float* out32, const LaunchTo& to) {
    launch_kernel(to, "layernorm_kernel", layernorm_kernel, dim3((M + 3) / 4), dim3(256), 0, x, row_stride, M, D, g, b, out16, out32);
}

// LayerNorm of gathered rows: out[m] = LN(x[rows[m]]) (the text tower's ln_final on each text's EOT row, clip/model.py:316-318)
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float* x, const int* rows, int M, int D, const float* g, const float* b, float* o32) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const float* xr = x + (long long)rows[m] * D;
    ln_row([&](int i) { return xr[i]; }, D, g, b, nullptr, o32 + (long long)m * D);
}
void launch_layernorm_rows(const float* x, const int* rows, int M, int D, const float* g, const float* b, float* out32, hipStream_t st) {
    hipLaunchKernelGGL(layernorm_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, st, x, rows, M, D, g, b, out32);
}

// nn.MultiheadAttention forward: softmax(q k^T / sqrt(hd) [+causal]) v per (image, head).
// qkv: [n_img*L][3*heads*hd] fp16 (q | k | v), out: [n_img*L][heads*hd] fp16.  hd == 64.
// MFMA form for L <= 64 (the visual tower's 50 tokens; a scalar LDS-fed fp32 kernel spent 49 us per layer here).
// TWO waves per (image, head): wave qb owns 32 queries and all 64 key slots.
//   S^T[key][query] = K Q^T: both operands are 16-byte global loads of a token's 8 consecutive head dims — no staging;
//   the softmax runs in the accumulator registers (a query's keys live in one lane pair: 32 registers + one xor-32 shuffle);
//   O^T[d][query] = V^T P: the MFMA's K order is free, so P stays where the softmax left it (lane half kh, registers 8g+4kh+q)
//   and V^T goes to LDS once per pair with its keys permuted to match (144-byte rows: conflict-free 16-byte reads);
//   P is split hi + lo * 2^-11 in fp16 so the product keeps the fp32 softmax (fp16 x fp16 products are exact in the fp32
//   accumulator: the scores themselves are the scalar kernel's up to summation order).
// NKB = key (and query) blocks of 32: 2 for L <= 64 — two (image, head) pairs per workgroup, two waves each; 3 for L <= 96 (round 4: the text
// tower's 77 tokens ran on that scalar kernel, 111 us per layer) — one pair per workgroup, waves 0..2 own 32 queries each, wave 3
// only helps staging V^T.
template <int NKB>
__global__ __launch_bounds__(256) void attention_mfma_kernel(const half_t* qkv, int L, int heads, int n_pairs, int causal,
                                                             half_t* out) {
    constexpr int PP = NKB == 2 ? 2 : 1;                // pairs per workgroup
    constexpr int WP = 4 / PP;                          // waves per pair
    constexpr int VROW = NKB * 64 + 16;                 // bytes per V^T row: 32 NKB keys + pad (144 / 208: conflict-free 16-byte reads)
    __shared__ __attribute__((aligned(16))) char vts[PP][64 * VROW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 31, kh = lane >> 5;
    const int pair = blockIdx.x * PP + wave / WP, qb = wave % WP;
    const int pc = min(pair, n_pairs - 1);
    const int img = pc / heads, h = pc - img * heads, D = heads * 64;
    const half_t* base = qkv + (long long)img * L * 3 * D + h * 64;
    const long long ts = 3LL * D;                       // token stride
    const int query = qb * 32 + lr;
    const bool qwave = qb < NKB;                        // (NKB = 3: the fourth wave has no queries)
    h8 qf[4], kf[NKB][4];
    if (qwave) {
        const half_t* qp = base + min(query, L - 1) * ts + kh * 8;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) qf[kk] = *(const h8*)(qp + kk * 16);
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            const half_t* kp = base + min(kb * 32 + lr, L - 1) * ts + D + kh * 8;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) kf[kb][kk] = *(const h8*)(kp + kk * 16);
        }
    }
    constexpr int TP = 64 * WP;                         // threads of a pair
    constexpr int NV = NKB * 32 * 8 / TP;               // V vectors per thread (4 / 3)
    const int pt = t % TP;                              // thread within the pair
    h8 vv[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int e = pt + TP * u, tok = e >> 3, d8 = e & 7;
        vv[u] = *(const h8*)(base + min(tok, L - 1) * ts + 2 * D + d8 * 8);
    }
    char* vt = vts[wave / WP];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int e = pt + TP * u, tok = e >> 3, d8 = e & 7;
        // key tok = kb*32 + 8g + 4kh' + q sits at K position (kb*2 + (g>>1))*16 + kh'*8 + (g&1)*4 + q of its row
        const int r = tok & 31, g = r >> 3;
        const int pos = ((tok >> 5) * 2 + (g >> 1)) * 16 + ((r >> 2) & 1) * 8 + (g & 1) * 4 + (r & 3);
#pragma unroll
        for (int j = 0; j < 8; ++j) *(half_t*)(vt + (d8 * 8 + j) * VROW + pos * 2) = tok < L ? vv[u][j] : (half_t)0.f;
    }
    f16x s[NKB];
    float inv = 0.f;
    if (qwave) {
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) s[kb] = mfma32(kf[kb][kk], qf[kk], s[kb]);
        }
        float m = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                float v = s[kb][r] * 0.125f;                // hd^-0.5, hd = 64
                if (key >= L || (causal && key > query)) v = -INFINITY;
                s[kb][r] = v;
                m = fmaxf(m, v);
            }
        m = fmaxf(m, __shfl_xor(m, 32));
        float z = 0.f;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e2 = __expf(s[kb][r] - m);
                s[kb][r] = e2;
                z += e2;
            }
        z += __shfl_xor(z, 32);
        inv = 1.f / z;
    }
    __syncthreads();                                    // V^T of the workgroup's pairs is in place
    if (!qwave) return;
    f16x o[2], ol[2];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) { o[db][r] = 0.f; ol[db][r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < 2 * NKB; ++ks) {
        h8 ph, pl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float pv = s[ks >> 1][(2 * (ks & 1) + (e >> 2)) * 4 + (e & 3)] * inv;
            ph[e] = (half_t)pv;
            pl[e] = (half_t)((pv - (float)ph[e]) * 2048.f);
        }
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            const h8 vf = *(const h8*)(vt + (db * 32 + lr) * VROW + (ks * 16 + kh * 8) * 2);
            o[db] = mfma32(vf, ph, o[db]);
            ol[db] = mfma32(vf, pl, ol[db]);
        }
    }
    if (pair < n_pairs && query < L) {
        half_t* op = out + ((long long)img * L + query) * D + h * 64 + 4 * kh;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                h4 w;
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = (half_t)(o[db][g * 4 + q] + ol[db][g * 4 + q] * (1.f / 2048.f));
                *(h4*)(op + db * 32 + 8 * g) = w;
            }
    }
}

// Streaming form of the kernel above for any L (the larger image towers: 197 / 257 / 577 tokens): the same two products on the same
// lane layout, with the keys walked in tiles of 64 and the softmax kept online — no buffer anywhere grows with L.
//   One workgroup = one (image, head) and 128 queries: wave w owns queries qblk*128 + 32w .. +31 (Q^T in registers, 16-byte global loads).
//   Per key tile: S^T[key][query] = K Q^T (K from LDS, 144-byte rows: conflict-free 16-byte reads), running max m and running sum z per
//   query in fp32 registers (a query's 64 scores of the tile sit in one lane pair), O^T and z rescaled by exp(m_old - m_new) when the
//   max moves, O^T[d][query] += V^T P with V^T in LDS in the permuted key order of the kernel above and P split hi + lo * 2^-11.
//   One division per query at the end.
//   K / V^T tiles are double-buffered and staged through registers once per workgroup: the global loads of tile t+1 are issued right
//   after the QK^T MFMAs of tile t and written to the other LDS buffer after its PV MFMAs, in front of the tile's one barrier.
//   V is transposed on the way in: a thread loads the same 8 dims of two adjacent keys (adjacent K positions) and writes 8 dwords.
//   LDS: 2 x (64 x 144 K + 64 x 144 V^T) = 36,864 bytes per workgroup.
//   Key slots >= L carry -inf (their K / V loads are clamped / zeroed), query rows >= L are computed on a clamped row and not stored;
//   waves whose 32 queries all lie past L only help staging.  causal: the workgroup stops at the last tile its queries can see, a
//   wave skips tiles wholly above its diagonal, and tile 0 always holds key 0 <= query, so no row's running max stays -inf.
__global__ __launch_bounds__(256, 2) void attention_stream_kernel(const half_t* qkv, int L, int heads, int causal, half_t* out) {
    constexpr int ROW = 144, TILE = 64 * ROW;
    __shared__ __attribute__((aligned(16))) char kls[2][TILE];
    __shared__ __attribute__((aligned(16))) char vls[2][TILE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 31, kh = lane >> 5;
    const int nqb = (L + 127) / 128;
    const int pair = blockIdx.x / nqb, qblk = blockIdx.x - pair * nqb;
    const int img = pair / heads, h = pair - img * heads, D = heads * 64;
    const half_t* base = qkv + (long long)img * L * 3 * D + h * 64;
    const long long ts = 3LL * D;                       // token stride
    const int q0 = qblk * 128 + wave * 32, query = q0 + lr;
    int nkt = (L + 63) / 64;                            // key tiles the workgroup walks
    if (causal) nkt = min(nkt, (min(qblk * 128 + 127, L - 1) >> 6) + 1);
    const int wkt = q0 >= L ? 0 : causal ? min(nkt, ((q0 + 31) >> 6) + 1) : nkt;   // ... and the ones this wave computes on
    // staging roles: K piece u = (key (t >> 3) + 32u, dims 8 (t & 7) ..): 8 lanes per 128-byte line, 16-byte LDS writes.
    // V piece u = (key 2 (t & 31) + u, dims 8 (t >> 5) ..): the 32 lanes of a dword-store group hold the 32 key pairs of ONE dim
    // group, so their 32 dwords of a V^T row are 32 different banks (dims across the lanes put 8 lanes on one bank: row stride 36 dwords)
    const int sk = t >> 3, sd8 = t & 7, vtok = 2 * (t & 31), vd8 = t >> 5;
    const int vr_ = vtok & 31, vg = vr_ >> 3;
    const int vpos = ((vtok >> 5) * 2 + (vg >> 1)) * 16 + ((vr_ >> 2) & 1) * 8 + (vg & 1) * 4 + (vr_ & 3);   // K position of key vtok (even)
    h8 kr[2], vr[2];
    auto stage_load = [&](int kt) {
        const int k0 = kt * 64;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            kr[u] = *(const h8*)(base + (long long)min(k0 + sk + 32 * u, L - 1) * ts + D + sd8 * 8);
            vr[u] = *(const h8*)(base + (long long)min(k0 + vtok + u, L - 1) * ts + 2 * D + vd8 * 8);
        }
    };
    auto stage_write = [&](int kt, int buf) {
        const int k0 = kt * 64;
#pragma unroll
        for (int u = 0; u < 2; ++u) *(h8*)(kls[buf] + (sk + 32 * u) * ROW + sd8 * 16) = kr[u];
        const bool ok0 = k0 + vtok < L, ok1 = k0 + vtok + 1 < L;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            h2 w;
            w[0] = ok0 ? vr[0][j] : (half_t)0.f;
            w[1] = ok1 ? vr[1][j] : (half_t)0.f;
            *(h2*)(vls[buf] + (vd8 * 8 + j) * ROW + vpos * 2) = w;
        }
    };
    h8 qf[4];
    {
        const half_t* qp = base + (long long)min(query, L - 1) * ts + kh * 8;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) qf[kk] = *(const h8*)(qp + kk * 16);
    }
    f16x o[2], ol[2];
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) { o[db][r] = 0.f; ol[db][r] = 0.f; }
    float m = -INFINITY, z = 0.f;                       // z: this lane's half of the query's running sum
    stage_load(0);
    stage_write(0, 0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int buf = kt & 1;
        const bool work = kt < wkt;                     // wave-uniform
        f16x s[2];
        if (work) {
            const char* kl = kls[buf];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const h8 kf = *(const h8*)(kl + (kb * 32 + lr) * ROW + (kk * 16 + kh * 8) * 2);
                    s[kb] = mfma32(kf, qf[kk], s[kb]);
                }
            }
        }
        if (kt + 1 < nkt) stage_load(kt + 1);
        if (work) {
            const int k0 = kt * 64;
            float mt = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    float v = s[kb][r] * 0.125f;            // hd^-0.5, hd = 64
                    if (key >= L || (causal && key > query)) v = -INFINITY;
                    s[kb][r] = v;
                    mt = fmaxf(mt, v);
                }
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float mn = fmaxf(m, mt);                  // finite from tile 0 on (key 0 is visible to every query)
            const float alpha = __expf(m - mn);
            m = mn;
            float zt = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float e2 = __expf(s[kb][r] - mn);
                    s[kb][r] = e2;
                    zt += e2;
                }
            z = z * alpha + zt;
            if (__any(alpha != 1.f)) {
#pragma unroll
                for (int db = 0; db < 2; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { o[db][r] *= alpha; ol[db][r] *= alpha; }
            }
            const char* vl = vls[buf];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                h8 ph, pl;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float pv = s[ks >> 1][(2 * (ks & 1) + (e >> 2)) * 4 + (e & 3)];
                    ph[e] = (half_t)pv;
                    pl[e] = (half_t)((pv - (float)ph[e]) * 2048.f);
                }
#pragma unroll
                for (int db = 0; db < 2; ++db) {
                    const h8 vf = *(const h8*)(vl + (db * 32 + lr) * ROW + (ks * 16 + kh * 8) * 2);
                    o[db] = mfma32(vf, ph, o[db]);
                    ol[db] = mfma32(vf, pl, ol[db]);
                }
            }
        }
        if (kt + 1 < nkt) stage_write(kt + 1, buf ^ 1);    // (that buffer's readers passed the previous tile's barrier)
        __syncthreads();
    }
    if (query < L) {
        z += __shfl_xor(z, 32);
        const float inv = 1.f / z;
        half_t* op = out + ((long long)img * L + query) * D + h * 64 + 4 * kh;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                h4 w;
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = (half_t)((o[db][g * 4 + q] + ol[db][g * 4 + q] * (1.f / 2048.f)) * inv);
                *(h4*)(op + db * 32 + 8 * g) = w;
            }
    }
}

void launch_attention(const half_t* qkv, int n_img, int L, int heads, int hd, int causal, half_t* out,
                      hipStream_t st) {
    (void)hd;  // 64 (asserted by the engine)
    if (L <= 64) {
        const int n_pairs = n_img * heads;
        hipLaunchKernelGGL(attention_mfma_kernel<2>, dim3((n_pairs + 1) / 2), dim3(256), 0, st, qkv, L, heads, n_pairs, causal, out);
        return;
    }
    if (L <= 96) {          // the text tower's context (77)
        const int n_pairs = n_img * heads;
        hipLaunchKernelGGL(attention_mfma_kernel<3>, dim3(n_pairs), dim3(256), 0, st, qkv, L, heads, n_pairs, causal, out);
        return;
    }
    const int nqb = (L + 127) / 128;     // any longer sequence: ViT-B/16 197 tokens, ViT-L/14 257, ViT-L/14@336 577
    hipLaunchKernelGGL(attention_stream_kernel, dim3((unsigned)((long long)n_img * heads * nqb)), dim3(256), 0, st, qkv, L, heads, causal, out);
}

// images already resized / normalised by the caller (clip.py:68-74 preprocess) -> patch-embedding operand
__global__ void image_patches_kernel(const float* img, int n, int S, int ps, int ld, half_t* patches) {
    const int G = S / ps;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)n * 3 * S * S) return;
    const int X = (int)(idx % S), Y = (int)((idx / S) % S);
    const int c = (int)((idx / ((long long)S * S)) % 3), b = (int)(idx / ((long long)S * S * 3));
    const int gy = Y / ps, iy = Y - gy * ps, gx = X / ps, ix = X - gx * ps;
    const long long row = ((long long)b * G + gy) * G + gx;
    patches[row * ld + ((long long)c * ps + iy) * ps + ix] = (half_t)img[idx];
}
void launch_image_patches(const float* img, int n, int S, int ps, int ld, half_t* patches, hipStream_t st) {
    const long long total = (long long)n * 3 * S * S;
    hipLaunchKernelGGL(image_patches_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, img, n, S, ps, ld, patches);
}
