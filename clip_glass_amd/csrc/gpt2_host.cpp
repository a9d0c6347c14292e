// gpt2_host.cpp — GPT-2 behind the engine (optional, fp32; config C5): weights, the decode workspace and the decode entry points.
#include <math.h>
#include <string.h>

#include "engine.h"

// ------------------------------------------------------------------------------------
// GPT-2 (optional): Conv1D weights are [nx][nf] (gpt2/model.py:30-43) -> transposed to [nf][nx]
// ------------------------------------------------------------------------------------
int finalize_gpt2(glass_engine* e) {
    if (!find(e, "gpt2.transformer.wte.weight")) return GLASS_OK;
    GET(wte, "gpt2.transformer.wte.weight");
    GET(wpe, "gpt2.transformer.wpe.weight");
    GET(lg, "gpt2.transformer.ln_f.weight");
    GET(lb, "gpt2.transformer.ln_f.bias");
    REQUIRE(wte->dims.size() == 2 && wpe->dims.size() == 2 && wpe->dims[1] == wte->dims[1], GLASS_ERR_ARG, "bad GPT-2 embedding shapes");
    e->g_vocab = (int)wte->dims[0];
    e->g_dim = (int)wte->dims[1];
    e->g_npos = (int)wpe->dims[0];
    const int D = e->g_dim;
    REQUIRE(D % 64 == 0, GLASS_ERR_ARG, "GPT-2 width must be a multiple of the 64-wide head");
    int rc;
    if ((rc = upload(e, &e->g_wte, wte->data))) return rc;
    if ((rc = upload(e, &e->g_wpe, wpe->data))) return rc;
    if ((rc = upload(e, &e->g_lnf_g, lg->data))) return rc;
    if ((rc = upload(e, &e->g_lnf_b, lb->data))) return rc;
    char nm[256];
    auto tr = [](const HostTensor* w, int nx, int nf) { return transposed(w->data.data(), nx, nf, 1.f); };   // [nx][nf] -> [nf][nx]
    for (int i = 0;; ++i) {
        snprintf(nm, sizeof nm, "gpt2.transformer.h.%d.", i);
        const std::string p = nm;
        if (!find(e, p + "ln_1.weight")) break;
        glass_engine::Gpt2Block b;
        GET(l1g, p + "ln_1.weight"); GET(l1b, p + "ln_1.bias"); GET(l2g, p + "ln_2.weight"); GET(l2b, p + "ln_2.bias");
        GET(wa, p + "attn.c_attn.weight"); GET(ba, p + "attn.c_attn.bias");
        GET(wo, p + "attn.c_proj.weight"); GET(bo, p + "attn.c_proj.bias");
        GET(wf, p + "mlp.c_fc.weight"); GET(bf, p + "mlp.c_fc.bias");
        GET(wp, p + "mlp.c_proj.weight"); GET(bp, p + "mlp.c_proj.bias");
        REQUIRE(numel(wa) == (size_t)3 * D * D && numel(wo) == (size_t)D * D && numel(wf) == (size_t)4 * D * D &&
                    numel(wp) == (size_t)4 * D * D, GLASS_ERR_ARG, "bad GPT-2 block shapes: " + p);
        if ((rc = upload(e, &b.ln1_g, l1g->data))) return rc;
        if ((rc = upload(e, &b.ln1_b, l1b->data))) return rc;
        if ((rc = upload(e, &b.ln2_g, l2g->data))) return rc;
        if ((rc = upload(e, &b.ln2_b, l2b->data))) return rc;
        if ((rc = upload(e, &b.w_qkv, tr(wa, D, 3 * D)))) return rc;
        if ((rc = upload(e, &b.b_qkv, ba->data))) return rc;
        if ((rc = upload(e, &b.w_o, tr(wo, D, D)))) return rc;
        if ((rc = upload(e, &b.b_o, bo->data))) return rc;
        if ((rc = upload(e, &b.w_fc, tr(wf, D, 4 * D)))) return rc;
        if ((rc = upload(e, &b.b_fc, bf->data))) return rc;
        if ((rc = upload(e, &b.w_pr, tr(wp, 4 * D, D)))) return rc;
        if ((rc = upload(e, &b.b_pr, bp->data))) return rc;
        e->gblk.push_back(b);
    }
    return GLASS_OK;
}

void gpt2_work_free(glass_engine* e) {
    auto& w = e->gwork;
    if (w.exec) hipGraphExecDestroy(w.exec);
    if (w.graph) hipGraphDestroy(w.graph);
    for (void* p : w.owned) hipFree(p);
    w = glass_engine::Gpt2Work();
}

// samp: the sampler's GPT2_SP_* words (host), nullptr = greedy
static int gpt2_decode_group(glass_engine* e, const int32_t* context, int32_t P, int32_t nctx, int32_t length, int32_t* out_tokens,
                             const int32_t* samp) {
    REQUIRE(e && context && out_tokens && P > 0 && nctx > 0 && length > 0, GLASS_ERR_ARG, "bad argument");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "finalize() first");
    REQUIRE(e->g_wte != nullptr, GLASS_ERR_STATE, "GPT-2 weights were not loaded (gpt2.transformer.*)");
    const int D = e->g_dim, V = e->g_vocab, heads = D / 64, Tmax = nctx + length;
    REQUIRE(Tmax <= e->g_npos && Tmax <= 256, GLASS_ERR_ARG, "sequence longer than the position table / 256");
    // the prefill attention holds a sequence's keys, values and its whole score matrix in LDS: 4 * (n^2 + 196 n) bytes of the 160 KB
    REQUIRE(gpt2_attention_lds_bytes(nctx, nctx) <= GPT2_ATTENTION_LDS_MAX, GLASS_ERR_ARG,
            "context longer than 126 tokens (the prefill attention keeps 4 * (n^2 + 196 n) bytes per sequence in 160 KB of LDS)");
    for (long long i = 0; i < (long long)P * nctx; ++i)
        REQUIRE(context[i] >= 0 && context[i] < V, GLASS_ERR_ARG, "token id out of range");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    const int nl = (int)e->gblk.size();
    const size_t rows = (size_t)P * nctx;
    auto& w = e->gwork;
    hipStream_t st = e->stream;
    auto fits = [&](const glass_engine::Gpt2Work& g) { return g.P == P && g.nctx == nctx && g.length == length; };
    if (!fits(w)) std::swap(e->gwork, e->gwork_alt);   // second slot: a ragged population alternates between a 64-row group and its
                                                       // remainder — each keeps its buffers and its captured step graph
    if (!fits(w)) {      // (re)build the workspace for this geometry
        gpt2_work_free(e);
        // split-K scratch for the single-token steps (M = P <= 64 rows: each weight is streamed once per step, so the number
        // of workgroups pulling on HBM is what matters), device-resident tokens and step state {past length, step index}
        w.part_elems = (size_t)16 * P * 4 * D;
        hipError_t err = owned_alloc(w.owned, &w.d_tok, rows);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.d_gen, (size_t)P * length);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.d_state, 3);      // {past length, step index, ticket counter of the fused step tail}
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.d_samp, GPT2_SP_WORDS);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.x, rows * D);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.ln, rows * D);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.qkv, rows * 3 * D);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.att, rows * D);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.hid, rows * 4 * D);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.last, (size_t)P * D);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.logits, (size_t)P * V);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.kc, (size_t)nl * P * Tmax * D);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.vc, (size_t)nl * P * Tmax * D);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.part, w.part_elems);
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.pairs, (size_t)2 * P * ((V + 31) / 32));   // (max, index) per (row, 32-column block)
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.stats, (size_t)P * (2 + 2 * 32));
        if (err == hipSuccess) err = owned_alloc(w.owned, &w.pst, (size_t)P * 24 * 2);   // row partials (mean, M2) of the complete-output step products   // + the two-stage arg-max's (value, index) pairs
        if (err != hipSuccess) {
            gpt2_work_free(e);
            glass_set_error(std::string("gpt2_decode: hipMalloc failed: ") + hipGetErrorString(err));
            return GLASS_ERR_NOMEM;
        }
        w.P = P; w.nctx = nctx; w.length = length;
    }
    // the captured step graph belongs to the mode it was recorded in: greedy never replays a sampling step, nor the reverse
    const int sample = samp ? 1 : 0;
    if (w.sample != sample) {
        if (w.exec) { hipGraphExecDestroy(w.exec); w.exec = nullptr; }
        if (w.graph) { hipGraphDestroy(w.graph); w.graph = nullptr; }
        w.sample = sample;
    }
    // one transformer pass over `nd` new positions per sequence; step_state != nullptr: single-token step whose past length /
    // step index are read from device memory (the form that is captured into a hipGraph and replayed)
    // single-token steps, fused form (round 3): LayerNorm applied on the activation operand of the next
    // product from row statistics, products with complete outputs (no split-K reduce launch) except the MLP's second one, whose
    // split-K slices of the residual products finished together with the residual add and the next statistics: 9 launches per layer
    // instead of 11 (complete-output products — 72 / 24 / 96 workgroups walking three chunks each — were 21 us against 9 + 4: dropped)
    // (the launcher's own shape conditions, asked through the launcher's predicate: a product it refuses returns 0 slices and nothing written)
    const bool fuse_ok = gemm_f32_step_supported(P, D, D, true) && gemm_f32_step_supported(P, 4 * D, 4 * D, false);
    bool step_refused = false;
    // fused step tail (round 4): the pick also writes the NEXT step's embedding + first LayerNorm statistics and advances the state — a step
    // starts at layer 0's qkv product; the first step's embedding is one eager launch after the prefill.
    const bool tail_fused = fuse_ok && D <= 1024 && gpt2_head_supported(P, V, D, D);
    auto pass = [&](int nd, int past, const int* step_state) {
        const int M = P * nd;
        // round 4 (gpt2.hip): the attention output product and the MLP's first product in the complete-output form — no slices, so no
        // gpt2_finalize / splitk_reduce launch behind them: 6 launches per layer instead of 8.  (The qkv product and the MLP's second one
        // stay split: complete, they were 12-14 us against 9.5 and 34 against 12 + 5.)
        const bool rowblk = step_state && fuse_ok && D % 32 == 0 && D / 32 <= 24 &&
                            gemm_f32_rowblk_supported(P, D, D, D, false, true) && gemm_f32_rowblk_supported(P, 4 * D, D, D, true, false);
        if (step_state) { if (!tail_fused) launch_gpt2_embed_step(w.d_gen, step_state, P, e->g_wte, e->g_wpe, D, w.x, st, fuse_ok ? w.stats : nullptr); }
        else launch_gpt2_embed(w.d_tok, e->g_wte, e->g_wpe, M, nd, past, D, w.x, st);
        if (step_state && fuse_ok) {      // (the embedding kernel left the first layer's LayerNorm statistics)
            for (int l = 0; l < nl; ++l) {
                const auto& b = e->gblk[l];
                float* kcl = w.kc + (size_t)l * P * Tmax * D;
                float* vcl = w.vc + (size_t)l * P * Tmax * D;
                int S = launch_gemm_f32_step(w.x, b.w_qkv, b.b_qkv, w.qkv, P, 3 * D, D, D, 3 * D, 0, st, w.part, w.part_elems, w.stats, b.ln1_g, b.ln1_b);
                step_refused |= S == 0;
                if (Tmax <= 64) {      // one wave per (sequence, head); it sums the product's slices itself
                    launch_gpt2_attention_step(w.qkv, S > 1 ? w.part : nullptr, S, b.b_qkv, kcl, vcl, P, Tmax, heads, w.att, st, step_state);
                } else {
                    if (S > 1) launch_gpt2_reduce(w.part, S, b.b_qkv, w.qkv, P, 3 * D, 3 * D, 0, st);
                    launch_gpt2_attention(w.qkv, kcl, vcl, P, 1, past, Tmax, heads, w.att, st, step_state);
                }
                if (rowblk) {       // x += att @ Wo + b (row partials of LayerNorm 2 in the epilogue); hid = gelu(LN2(x) @ Wfc + b)
                    bool ok = launch_gemm_f32_rowblk(w.att, b.w_o, b.b_o, w.x, P, D, D, D, D, 2, st, nullptr, 0, nullptr, nullptr, w.pst);
                    ok &= launch_gemm_f32_rowblk(w.x, b.w_fc, b.b_fc, w.hid, P, 4 * D, D, D, 4 * D, 1, st, w.pst, D / 32, b.ln2_g, b.ln2_b, nullptr);
                    step_refused |= !ok;
                } else {
                    S = launch_gemm_f32_step(w.att, b.w_o, b.b_o, w.x, P, D, D, D, D, 2, st, w.part, w.part_elems, nullptr, nullptr, nullptr);
                    step_refused |= S == 0;
                    launch_gpt2_finalize(S > 1 ? w.part : nullptr, S, b.b_o, w.x, P, D, w.stats, st);       // residual + LayerNorm 2 statistics
                    S = launch_gemm_f32_step(w.x, b.w_fc, b.b_fc, w.hid, P, 4 * D, D, D, 4 * D, 1, st, w.part, w.part_elems, w.stats, b.ln2_g, b.ln2_b);
                    step_refused |= S == 0;
                    if (S > 1) launch_gpt2_reduce(w.part, S, b.b_fc, w.hid, P, 4 * D, 4 * D, 1, st);
                }
                S = launch_gemm_f32_step(w.hid, b.w_pr, b.b_pr, w.x, P, D, 4 * D, 4 * D, D, 2, st, w.part, w.part_elems, nullptr, nullptr, nullptr);
                step_refused |= S == 0;
                launch_gpt2_finalize(S > 1 ? w.part : nullptr, S, b.b_pr, w.x, P, D, w.stats, st);      // residual + next LayerNorm's statistics
            }
            if (tail_fused) {
                if (samp)       // the sampling twin: logits written too, the sampler from the pairs, the same embed / advance tail
                    step_refused |= !launch_gpt2_head_sample(w.x, e->g_wte, P, V, D, D, w.stats, e->g_lnf_g, e->g_lnf_b, w.logits, w.pairs, w.d_samp,
                                                             w.d_gen, w.d_state, true, e->g_wte, e->g_wpe, w.x, w.stats, st);
                else
                    step_refused |= !launch_gpt2_head_tail(w.x, e->g_wte, P, V, D, D, w.stats, e->g_lnf_g, e->g_lnf_b, w.pairs, w.d_gen, w.d_state, e->g_wte,
                                                           e->g_wpe, w.x, w.stats, st);
                return;
            }
            const bool head = samp ? launch_gpt2_head_sample(w.x, e->g_wte, P, V, D, D, w.stats, e->g_lnf_g, e->g_lnf_b, w.logits, w.pairs,
                                                             w.d_samp, w.d_gen, w.d_state, false, nullptr, nullptr, nullptr, nullptr, st)
                                   : launch_gpt2_head(w.x, e->g_wte, P, V, D, D, w.stats, e->g_lnf_g, e->g_lnf_b, nullptr, w.pairs, w.d_gen,
                                                      w.d_state, st);
            if (!head) {
                // ln_f fused; the real vocabulary (1571 column blocks) is never split, a small one may be
                const int S = launch_gemm_f32_step(w.x, e->g_wte, nullptr, w.logits, P, V, D, D, V, 0, st, w.part, w.part_elems, w.stats, e->g_lnf_g, e->g_lnf_b);
                step_refused |= S == 0;
                if (S > 1) launch_gpt2_reduce(w.part, S, nullptr, w.logits, P, V, V, 0, st);
                if (samp) launch_gpt2_sample(w.logits, P, V, w.d_samp, w.d_gen, w.d_state, st);
                else launch_argmax(w.logits, P, V, w.d_gen, st, w.d_state, w.stats + 2 * P);
            }
            launch_gpt2_advance(w.d_state, st);
            return;
        }
        for (int l = 0; l < nl; ++l) {
            const auto& b = e->gblk[l];
            float* kcl = w.kc + (size_t)l * P * Tmax * D;
            float* vcl = w.vc + (size_t)l * P * Tmax * D;
            launch_layernorm(w.x, D, M, D, b.ln1_g, b.ln1_b, nullptr, w.ln, st);
            launch_gemm_f32(w.ln, b.w_qkv, b.b_qkv, w.qkv, M, 3 * D, D, D, 3 * D, 0, st, w.part, w.part_elems, nd > 1);
            launch_gpt2_attention(w.qkv, kcl, vcl, P, nd, past, Tmax, heads, w.att, st, step_state);
            launch_gemm_f32(w.att, b.w_o, b.b_o, w.x, M, D, D, D, D, 2, st, w.part, w.part_elems, nd > 1);
            launch_layernorm(w.x, D, M, D, b.ln2_g, b.ln2_b, nullptr, w.ln, st);
            launch_gemm_f32(w.ln, b.w_fc, b.b_fc, w.hid, M, 4 * D, D, D, 4 * D, 1, st, w.part, w.part_elems, nd > 1);
            launch_gemm_f32(w.hid, b.w_pr, b.b_pr, w.x, M, D, 4 * D, 4 * D, D, 2, st, w.part, w.part_elems, nd > 1);
        }
        // ln_f on the last position of each sequence, tied lm_head, greedy pick -> d_gen[step][P]
        launch_layernorm(w.x + (size_t)(nd - 1) * D, (long long)nd * D, P, D, e->g_lnf_g, e->g_lnf_b, nullptr, w.last, st);
        launch_gemm_f32(w.last, e->g_wte, nullptr, w.logits, P, V, D, D, V, 0, st, w.part, w.part_elems);
        if (samp) launch_gpt2_sample(w.logits, P, V, w.d_samp, w.d_gen, w.d_state, st);
        else launch_argmax(w.logits, P, V, w.d_gen, st, w.d_state, w.stats + 2 * P);
        launch_gpt2_advance(w.d_state, st);
    };
    std::vector<int32_t> gen((size_t)P * length);
    GLASS_HIP(hipEventRecord(e->ev0, st));
    hipMemcpyAsync(w.d_tok, context, rows * sizeof(int), hipMemcpyHostToDevice, st);
    const int state0[3] = {0, 0, 0}, state1[3] = {nctx, 1, 0};
    hipMemcpyAsync(w.d_state, state0, sizeof state0, hipMemcpyHostToDevice, st);
    if (samp) hipMemcpyAsync(w.d_samp, samp, GPT2_SP_WORDS * sizeof(int), hipMemcpyHostToDevice, st);
    pass(nctx, 0, nullptr);                                 // prefill = step 0 (writes d_gen[0 .. P))
    hipMemcpyAsync(w.d_state, state1, sizeof state1, hipMemcpyHostToDevice, st);
    if (tail_fused && length > 1) launch_gpt2_embed_step(w.d_gen, w.d_state, P, e->g_wte, e->g_wpe, D, w.x, st, w.stats);   // step 1's embedding (later ones: the step tail)
    hipError_t err = hipSuccess;
    if (length > 1) {
        // the 29 single-token steps are the same ~190 launches each: capture one step once, replay it (launch latency, not work,
        // is what the un-graphed loop spent its time on)
        if (!w.exec) {
            err = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
            if (err == hipSuccess) {
                pass(1, 0, w.d_state);
                err = hipStreamEndCapture(st, &w.graph);
                if (err == hipSuccess) err = hipGraphInstantiate(&w.exec, w.graph, nullptr, nullptr, 0);
            }
            if (err != hipSuccess) {       // capture unavailable: eager steps (same kernels, same device-side state)
                (void)hipGetLastError();
                if (w.exec) { hipGraphExecDestroy(w.exec); w.exec = nullptr; }
                if (w.graph) { hipGraphDestroy(w.graph); w.graph = nullptr; }
                err = hipSuccess;
            }
        }
        for (int step = 1; step < length && err == hipSuccess; ++step) {
            if (w.exec) err = hipGraphLaunch(w.exec, st);
            else pass(1, 0, w.d_state);
        }
    }
    if (err == hipSuccess) err = hipEventRecord(e->ev1, st);
    if (err == hipSuccess) err = hipMemcpyAsync(gen.data(), w.d_gen, (size_t)P * length * sizeof(int), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err == hipSuccess) err = hipGetLastError();
    if (err != hipSuccess) {
        gpt2_work_free(e);
        glass_set_error(std::string("gpt2_decode failed: ") + hipGetErrorString(err));
        return GLASS_ERR_HIP;
    }
    if (step_refused) {        // fuse_ok and the launcher disagreed about a shape: buffers were consumed unwritten — never a silent result
        gpt2_work_free(e);
        glass_set_error("gpt2_decode: a fused step product refused its shape (launch_gemm_f32_step returned 0)");
        return GLASS_ERR_STATE;
    }
    (void)hipEventElapsedTime(&w.last_ms, e->ev0, e->ev1);
    e->last_ms = w.last_ms;
    for (int p = 0; p < P; ++p) {
        for (int t = 0; t < nctx; ++t) out_tokens[(size_t)p * Tmax + t] = context[(size_t)p * nctx + t];
        for (int s2 = 0; s2 < length; ++s2) out_tokens[(size_t)p * Tmax + nctx + s2] = gen[(size_t)s2 * P + p];
    }
    return GLASS_OK;
}

// Sequences are independent, and the single-token step kernels hold at most 64 rows: a longer population is decoded in row groups of
// 64, each through exactly the launches a 64-row call makes — a row's tokens do not depend on how many rows the call (or a shard) holds.
// samp (nullptr = greedy): the sampler's words for the call's first row; each group gets its own first global row.
static int gpt2_decode_groups(glass_engine* e, const int32_t* context, int32_t P, int32_t nctx, int32_t length, int32_t* out_tokens,
                              int32_t* samp) {
    REQUIRE(e && context && out_tokens && P > 0 && nctx > 0 && length > 0, GLASS_ERR_ARG, "bad argument");
    const int32_t row0 = samp ? samp[GPT2_SP_ROW0] : 0;
    float total_ms = 0.f;
    for (int g0 = 0; g0 < P; g0 += 64) {
        if (samp) samp[GPT2_SP_ROW0] = row0 + g0;
        const int rc = gpt2_decode_group(e, context + (size_t)g0 * nctx, std::min(64, P - g0), nctx, length,
                                         out_tokens + (size_t)g0 * (nctx + length), samp);
        if (rc) return rc;
        total_ms += e->gwork.last_ms;
    }
    e->gwork.last_ms = total_ms;
    e->last_ms = total_ms;
    return GLASS_OK;
}

extern "C" int glass_engine_gpt2_decode(glass_engine* e, const int32_t* context, int32_t P, int32_t nctx, int32_t length,
                                        int32_t* out_tokens) {
    return gpt2_decode_groups(e, context, P, nctx, length, out_tokens, nullptr);
}

// Stochastic decode: the same row groups, each group's first global row in the sampler's words — a row's draws depend on its global index,
// the step, (seed, generation, purpose) and its own logits only.
extern "C" int glass_engine_gpt2_sample(glass_engine* e, const int32_t* context, int32_t P, int32_t nctx, int32_t length, float temperature,
                                        int32_t top_k, uint64_t seed, int32_t generation, int32_t first_row, int32_t purpose,
                                        int32_t* out_tokens) {
    REQUIRE(e && context && out_tokens && P > 0 && nctx > 0 && length > 0, GLASS_ERR_ARG, "bad argument");
    REQUIRE(temperature > 0.f && temperature < INFINITY, GLASS_ERR_ARG, "temperature must be a finite value > 0");
    REQUIRE(top_k >= 0 && top_k <= GPT2_SAMPLE_TOPK_MAX, GLASS_ERR_ARG, "top_k must lie in [0, 256]");
    REQUIRE(first_row >= 0 && (long long)first_row + P <= 0x7fffffffLL, GLASS_ERR_ARG, "first_row out of range");
    REQUIRE(e->g_wte == nullptr || gpt2_sample_supported(e->g_vocab), GLASS_ERR_ARG, "vocabulary too large for the sampler (> 131072)");
    int32_t samp[GPT2_SP_WORDS];
    samp[GPT2_SP_SEED_LO] = (int32_t)(uint32_t)(seed & 0xFFFFFFFFu);
    samp[GPT2_SP_SEED_HI] = (int32_t)(uint32_t)(seed >> 32);
    samp[GPT2_SP_GEN] = generation;
    samp[GPT2_SP_ROW0] = first_row;
    samp[GPT2_SP_PURPOSE] = purpose;
    memcpy(&samp[GPT2_SP_TEMP], &temperature, sizeof(float));
    samp[GPT2_SP_TOPK] = top_k;
    samp[GPT2_SP_STEP] = 0;
    return gpt2_decode_groups(e, context, P, nctx, length, out_tokens, samp);
}
