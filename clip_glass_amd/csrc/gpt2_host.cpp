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

// What a token step of this geometry launches, decided from the launchers' own choosers before anything runs.  Fused step (round 3):
// LayerNorm applied on the activation operand of the next product from row statistics, split-K slices of the residual products finished
// together with the residual add and the next statistics.  Round 4: the attention output product and the MLP's first product in the
// complete-output form where the width allows — no slices, so no finishing launch behind them: 6 launches per layer instead of 8 (the qkv
// product and the MLP's second one stay split: complete, they were 12-14 us against 9.5 and 34 against 12 + 5) — and the pick also writes
// the NEXT step's embedding + first LayerNorm statistics and advances the state: a step starts at layer 0's qkv product.  A product
// a chooser refuses leaves the step unfused: that path takes every shape.
Gpt2StepPlan plan_gpt2_step(int P, int D, int V, int Tmax, bool sample, size_t part_elems, int n_cu) {
    Gpt2StepPlan pl;
    pl.qkv = choose_gemm_f32_step(P, 3 * D, D, D, true, part_elems, n_cu);
    pl.pr = choose_gemm_f32_step(P, D, 4 * D, 4 * D, false, part_elems, n_cu);
    if (D % 32 == 0 && D / 32 <= 24) {       // x += att @ Wo + b with the row partials of LayerNorm 2 in the epilogue; hid = gelu(LN2(x) @ Wfc + b)
        pl.o = choose_gemm_f32_rowblk(P, D, D, D, false, 0, true);
        pl.fc = choose_gemm_f32_rowblk(P, 4 * D, D, D, true, D / 32, false);
    }
    pl.rowblk = pl.o && pl.fc;
    if (!pl.rowblk) {
        pl.o = choose_gemm_f32_step(P, D, D, D, false, part_elems, n_cu);
        pl.fc = choose_gemm_f32_step(P, 4 * D, D, D, true, part_elems, n_cu);
    }
    pl.head = choose_gpt2_head(P, V, D, D, sample ? GPT2_PICK_SAMPLE_TAIL : GPT2_PICK_ARGMAX_TAIL, sample);
    if (!pl.head) pl.head = choose_gpt2_head(P, V, D, D, sample ? GPT2_PICK_SAMPLE : GPT2_PICK_ARGMAX, sample);
    // ln_f fused; the real vocabulary (1571 column blocks) is never split, a small one may be
    if (!pl.head) pl.logits = choose_gemm_f32_step(P, V, D, D, true, part_elems, n_cu);
    pl.fused = pl.qkv && pl.o && pl.fc && pl.pr && (pl.head || pl.logits);
    pl.att_step = pl.fused && Tmax <= 64;
    return pl;
}

static float* layer_cache(float* cache, const glass_engine::Gpt2Work& w, int l, int D) { return cache + (size_t)l * w.P * (w.nctx + w.length) * D; }

// One unfused transformer pass over the nd new positions per sequence that lie embedded in w.x, and the pick -> d_gen[step][P].
// state == nullptr: the prefill (past = 0); else a single-token step whose past length / step index are read from device memory.
static void gpt2_layers_unfused(const glass_engine* e, const glass_engine::Gpt2Work& w, int nd, const int* state, const LaunchTo& to) {
    const int P = w.P, D = e->g_dim, V = e->g_vocab, heads = D / 64, Tmax = w.nctx + w.length, M = P * nd;
    for (size_t l = 0; l < e->gblk.size(); ++l) {
        const auto& b = e->gblk[l];
        launch_layernorm(w.x, D, M, D, b.ln1_g, b.ln1_b, nullptr, w.ln, to);
        launch_gemm_f32(w.ln, b.w_qkv, b.b_qkv, w.qkv, M, 3 * D, D, D, 3 * D, 0, to, w.part, w.part_elems, nd > 1);
        launch_gpt2_attention(w.qkv, layer_cache(w.kc, w, l, D), layer_cache(w.vc, w, l, D), P, nd, 0, Tmax, heads, w.att, to, state);
        launch_gemm_f32(w.att, b.w_o, b.b_o, w.x, M, D, D, D, D, 2, to, w.part, w.part_elems, nd > 1);
        launch_layernorm(w.x, D, M, D, b.ln2_g, b.ln2_b, nullptr, w.ln, to);
        launch_gemm_f32(w.ln, b.w_fc, b.b_fc, w.hid, M, 4 * D, D, D, 4 * D, 1, to, w.part, w.part_elems, nd > 1);
        launch_gemm_f32(w.hid, b.w_pr, b.b_pr, w.x, M, D, 4 * D, 4 * D, D, 2, to, w.part, w.part_elems, nd > 1);
    }
    // ln_f on the last position of each sequence, tied lm_head, pick
    launch_layernorm(w.x + (size_t)(nd - 1) * D, (long long)nd * D, P, D, e->g_lnf_g, e->g_lnf_b, nullptr, w.last, to);
    launch_gemm_f32(w.last, e->g_wte, nullptr, w.logits, P, V, D, D, V, 0, to, w.part, w.part_elems);
    if (w.sample) launch_gpt2_sample(w.logits, P, V, w.d_samp, w.d_gen, w.d_state, to);
    else launch_argmax(w.logits, P, V, w.d_gen, to, w.d_state, w.stats + 2 * P);
    launch_gpt2_advance(w.d_state, to);
}

static void gpt2_prefill(const glass_engine* e, const glass_engine::Gpt2Work& w, int nd, const LaunchTo& to) {
    launch_gpt2_embed(w.d_tok, e->g_wte, e->g_wpe, w.P * nd, nd, 0, e->g_dim, w.x, to);
    gpt2_layers_unfused(e, w, nd, nullptr, to);
}

static void gpt2_step_unfused(const glass_engine* e, const glass_engine::Gpt2Work& w, const LaunchTo& to) {
    launch_gpt2_embed_step(w.d_gen, w.d_state, w.P, e->g_wte, e->g_wpe, e->g_dim, w.x, to);
    gpt2_layers_unfused(e, w, 1, w.d_state, to);
}

// The fused token step: w.plan, launched.  Every product was chosen by plan_gpt2_step: nothing here can refuse.
static void gpt2_step_fused(const glass_engine* e, const glass_engine::Gpt2Work& w, const LaunchTo& to) {
    const Gpt2StepPlan& pl = w.plan;
    const int P = w.P, D = e->g_dim, V = e->g_vocab, heads = D / 64, Tmax = w.nctx + w.length;
    auto slices = [&](const StepGemm& c) { return c.S > 1 ? w.part : nullptr; };
    // (a tail left this step's embedding and the first layer's LayerNorm statistics; the first step's come from one eager launch after the prefill)
    if (!pl.head.tail()) launch_gpt2_embed_step(w.d_gen, w.d_state, P, e->g_wte, e->g_wpe, D, w.x, to, w.stats);
    for (size_t l = 0; l < e->gblk.size(); ++l) {
        const auto& b = e->gblk[l];
        float *kcl = layer_cache(w.kc, w, l, D), *vcl = layer_cache(w.vc, w, l, D);
        launch_gemm_f32_step({w.x, b.w_qkv, b.b_qkv, w.qkv, 3 * D, 0, w.part, w.stats, b.ln1_g, b.ln1_b}, pl.qkv, to);
        if (pl.att_step) {
            launch_gpt2_attention_step(w.qkv, slices(pl.qkv), pl.qkv.S, b.b_qkv, kcl, vcl, P, Tmax, heads, w.att, to, w.d_state);
        } else {
            if (pl.qkv.S > 1) launch_gpt2_reduce(w.part, pl.qkv.S, b.b_qkv, w.qkv, P, 3 * D, 3 * D, 0, to);
            launch_gpt2_attention(w.qkv, kcl, vcl, P, 1, 0, Tmax, heads, w.att, to, w.d_state);
        }
        if (pl.rowblk) {
            launch_gemm_f32_rowblk({w.att, b.w_o, b.b_o, w.x, D, 2, nullptr, nullptr, nullptr, nullptr, w.pst}, pl.o, to);
            launch_gemm_f32_rowblk({w.x, b.w_fc, b.b_fc, w.hid, 4 * D, 1, nullptr, w.pst, b.ln2_g, b.ln2_b}, pl.fc, to);
        } else {
            launch_gemm_f32_step({w.att, b.w_o, b.b_o, w.x, D, 2, w.part}, pl.o, to);
            launch_gpt2_finalize(slices(pl.o), pl.o.S, b.b_o, w.x, P, D, w.stats, to);        // residual + LayerNorm 2 statistics
            launch_gemm_f32_step({w.x, b.w_fc, b.b_fc, w.hid, 4 * D, 1, w.part, w.stats, b.ln2_g, b.ln2_b}, pl.fc, to);
            if (pl.fc.S > 1) launch_gpt2_reduce(w.part, pl.fc.S, b.b_fc, w.hid, P, 4 * D, 4 * D, 1, to);
        }
        launch_gemm_f32_step({w.hid, b.w_pr, b.b_pr, w.x, D, 2, w.part}, pl.pr, to);
        launch_gpt2_finalize(slices(pl.pr), pl.pr.S, b.b_pr, w.x, P, D, w.stats, to);         // residual + next LayerNorm's statistics
    }
    if (pl.head) {      // a sampling pick reads the logits, so the head stores them too; a tail writes the next step's x / statistics
        launch_gpt2_head({w.x, e->g_wte, w.stats, e->g_lnf_g, e->g_lnf_b, w.sample ? w.logits : nullptr, w.pairs, w.d_samp, w.d_gen, w.d_state, e->g_wte,
                          e->g_wpe, w.x, w.stats}, pl.head, to);
        if (pl.head.tail()) return;
    } else {
        launch_gemm_f32_step({w.x, e->g_wte, nullptr, w.logits, V, 0, w.part, w.stats, e->g_lnf_g, e->g_lnf_b}, pl.logits, to);
        if (pl.logits.S > 1) launch_gpt2_reduce(w.part, pl.logits.S, nullptr, w.logits, P, V, V, 0, to);
        if (w.sample) launch_gpt2_sample(w.logits, P, V, w.d_samp, w.d_gen, w.d_state, to);
        else launch_argmax(w.logits, P, V, w.d_gen, to, w.d_state, w.stats + 2 * P);
    }
    launch_gpt2_advance(w.d_state, to);
}

static void gpt2_step(const glass_engine* e, const glass_engine::Gpt2Work& w, const LaunchTo& to) {
    if (w.plan.fused) gpt2_step_fused(e, w, to);
    else gpt2_step_unfused(e, w, to);
}

// Host only: the launches of one token step, one line each in launch order — the step functions above, run into a text instead of a stream
// over a workspace of placeholder pointers that nothing follows.
extern "C" int glass_host_gpt2_step_plan(int32_t P, int32_t D, int32_t V, int32_t n_layer, int32_t Tmax, int32_t sample, int32_t n_cu, char* out,
                                         int32_t cap) {
    REQUIRE(out && cap > 0, GLASS_ERR_ARG, "bad argument");
    REQUIRE(P > 0 && P <= 64 && D > 0 && D % 64 == 0 && V > 0 && n_layer > 0 && Tmax >= 2 && Tmax <= 256 && n_cu > 0, GLASS_ERR_ARG,
            "bad geometry (1 <= P <= 64 rows of a group, D % 64 == 0, 2 <= Tmax <= 256)");
    static float nowhere;
    static int nowhere_i;
    glass_engine e;
    e.g_dim = D; e.g_vocab = V;
    e.gblk.assign(n_layer, glass_engine::Gpt2Block());
    auto& w = e.gwork;
    w.P = P; w.nctx = 1; w.length = Tmax - 1; w.sample = sample ? 1 : 0;
    w.part_elems = (size_t)16 * P * 4 * D;
    w.d_tok = w.d_gen = w.d_state = w.d_samp = &nowhere_i;
    w.x = w.ln = w.qkv = w.att = w.hid = w.last = w.logits = w.kc = w.vc = w.part = w.stats = w.pairs = w.pst = &nowhere;
    w.plan = plan_gpt2_step(P, D, V, Tmax, sample != 0, w.part_elems, n_cu);
    std::string text;
    gpt2_step(&e, w, LaunchTo(&text));
    REQUIRE(text.size() < (size_t)cap, GLASS_ERR_ARG, "the plan needs " + std::to_string(text.size() + 1) + " bytes, more than the caller's " + std::to_string(cap));
    memcpy(out, text.c_str(), text.size() + 1);
    return GLASS_OK;
}

// samp: the sampler's GPT2_SP_* words (host), nullptr = greedy
static int gpt2_decode_group(glass_engine* e, const int32_t* context, int32_t P, int32_t nctx, int32_t length, int32_t* out_tokens,
                             const int32_t* samp) {
    REQUIRE(e && context && out_tokens && P > 0 && nctx > 0 && length > 0, GLASS_ERR_ARG, "bad argument");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "finalize() first");
    REQUIRE(e->g_wte != nullptr, GLASS_ERR_STATE, "GPT-2 weights were not loaded (gpt2.transformer.*)");
    const int D = e->g_dim, V = e->g_vocab, Tmax = nctx + length;
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
        w.plan = plan_gpt2_step(P, D, V, Tmax, sample != 0, w.part_elems, glass_cu_count());
    }
    std::vector<int32_t> gen((size_t)P * length);
    GLASS_HIP(hipEventRecord(e->ev0, st));
    hipMemcpyAsync(w.d_tok, context, rows * sizeof(int), hipMemcpyHostToDevice, st);
    const int state0[3] = {0, 0, 0}, state1[3] = {nctx, 1, 0};
    hipMemcpyAsync(w.d_state, state0, sizeof state0, hipMemcpyHostToDevice, st);
    if (samp) hipMemcpyAsync(w.d_samp, samp, GPT2_SP_WORDS * sizeof(int), hipMemcpyHostToDevice, st);
    gpt2_prefill(e, w, nctx, st);                           // prefill = step 0 (writes d_gen[0 .. P))
    hipMemcpyAsync(w.d_state, state1, sizeof state1, hipMemcpyHostToDevice, st);
    if (w.plan.fused && w.plan.head.tail() && length > 1) launch_gpt2_embed_step(w.d_gen, w.d_state, P, e->g_wte, e->g_wpe, D, w.x, st, w.stats);   // step 1's embedding (later ones: the step tail)
    hipError_t err = hipSuccess;
    if (length > 1) {
        // the 29 single-token steps are the same ~190 launches each: capture one step once, replay it (launch latency, not work,
        // is what the un-graphed loop spent its time on)
        if (!w.exec) {
            err = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
            if (err == hipSuccess) {
                gpt2_step(e, w, st);
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
            else gpt2_step(e, w, st);
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
