// edit.cpp — image editing (include/glass.h "Image editing"): the latent anchor and the direction source around the pass.  Kernels: edit.hip.
#include <math.h>
#include <string.h>

#include <string>

#include "engine.h"

extern "C" int glass_edit_supported(int32_t generator, int32_t n_blocks, int32_t sim_columns, int32_t use_discriminator, int32_t lpips_column,
                                    int32_t anchor, float anchor_lambda, int32_t n_obj) {
    REQUIRE(anchor == 0 || anchor == 1, GLASS_ERR_ARG, "anchor must be 0 (off) or 1");
    REQUIRE(std::isfinite(anchor_lambda) && anchor_lambda >= 0.f, GLASS_ERR_ARG, "anchor_lambda must be finite and >= 0");
    if (!anchor) {
        REQUIRE(anchor_lambda == 0.f, GLASS_ERR_ARG, "anchor_lambda > 0 folds the anchor distance into the similarity, and anchor is 0: set anchor = 1");
        return GLASS_OK;      // n_obj is what it is without an anchor
    }
    REQUIRE(generator != GLASS_GEN_BIGGAN_DEEP, GLASS_ERR_ARG,
            "anchor: the latent anchor is a distance between dlatents of a StyleGAN2 generator; a BigGAN-deep engine has none (its row is z and class bits)");
    REQUIRE(generator == GLASS_GEN_STYLEGAN2 && n_blocks > 0, GLASS_ERR_ARG,
            "anchor: the latent anchor is a distance between dlatents of a StyleGAN2 generator; this engine has no generator (GPT-2 / img2txt)");
    REQUIRE(sim_columns >= 0 && sim_columns <= 4, GLASS_ERR_ARG, "sim_columns must be in [0, 4]");
    const int K = std::max(sim_columns, 1);
    REQUIRE(K < 2 || anchor_lambda == 0.f, GLASS_ERR_ARG,
            "anchor_lambda > 0 folds the distance into THE similarity column; with sim_columns >= 2 there is no single one: use anchor_lambda = 0 (its own column)");
    const int want = K + (use_discriminator ? 1 : 0) + (lpips_column ? 1 : 0) + (anchor_lambda == 0.f ? 1 : 0);
    REQUIRE(n_obj == want, GLASS_ERR_ARG,
            "with anchor = 1, n_obj must be max(sim_columns, 1) + use_discriminator + (lpips own column) + (anchor_lambda == 0) = " + std::to_string(want) +
                ", got " + std::to_string(n_obj));
    REQUIRE(n_obj <= GLASS_SEARCH_MAX_OBJ + 1, GLASS_ERR_ARG, "n_obj out of range");
    return GLASS_OK;
}

// ---- latent anchor ---------------------------------------------------------------------------------
// The row goes where a pass puts row 0 of a population and through run_dlatents — the launches a pass makes for its rows — and the resulting
// dlatents of every style layer are kept.  A candidate with the same row gets the same bits, so its distance is 0 exactly.
int compute_anchor(glass_engine* e) {
    glass_engine::Edit& ed = e->edit;
    const int L = e->cfg.latent_size, NL = e->n_lat;
    const size_t row = latent_row_floats(e);
    REQUIRE(ed.anchor_row.size() == row, GLASS_ERR_STATE, "anchor: no row is stored");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    e->cur = e->stream;
    e->launch_error.clear();
    float* d_rows = latent_rows_dst(e);
    memcpy(e->h_pinned, ed.anchor_row.data(), row * sizeof(float));
    GLASS_HIP(hipMemcpyAsync(d_rows, e->h_pinned, row * sizeof(float), hipMemcpyHostToDevice, e->cur));
    const bool prof = e->profiling;
    e->profiling = false;           // (profile rows belong to a pass)
    const bool ok = run_dlatents(e, 1);
    e->profiling = prof;
    if (ok) {
        const LatPlan lp = plan_dlatents(e->latent_space, e->trunc_psi, e->trunc_cutoff, NL);
        if (lp.layered) {
            GLASS_HIP(hipMemcpyAsync(ed.d_anchor, e->d_dlat, (size_t)NL * L * sizeof(float), hipMemcpyDeviceToDevice, e->cur));
        } else {
            for (int l = 0; l < NL; ++l)      // one row serves every layer
                GLASS_HIP(hipMemcpyAsync(ed.d_anchor + (size_t)l * L, e->d_w0, (size_t)L * sizeof(float), hipMemcpyDeviceToDevice, e->cur));
        }
    }
    GLASS_HIP(hipStreamSynchronize(e->cur));
    GLASS_HIP(hipGetLastError());
    if (!e->launch_error.empty()) {
        const std::string msg = e->launch_error;
        e->launch_error.clear();
        glass_set_error(msg);
        return GLASS_ERR_STATE;
    }
    ed.has_anchor = true;
    return GLASS_OK;
}

extern "C" int glass_engine_set_anchor(glass_engine* e, const float* row) {
    REQUIRE(e && row, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "set_anchor: finalize() first (the row goes through the mapping network)");
    REQUIRE(e->cfg.anchor, GLASS_ERR_STATE, "set_anchor: this engine was created without an anchor (glass_config::anchor = 0): F has no place for the distance");
    REQUIRE(e->latent_space != GLASS_LATENT_SUB || e->has_subspace, GLASS_ERR_STATE, "set_anchor: set_subspace() first (the row's dlatents are base + coefficients . basis)");
    glass_engine::Edit& ed = e->edit;
    GLASS_HIP(hipSetDevice(e->cfg.device));
    if (!ed.d_anchor) {
        int rc;
        if ((rc = dev_alloc(e, &ed.d_anchor, (size_t)e->n_lat * e->cfg.latent_size))) return rc;
        if ((rc = dev_alloc(e, &ed.d_dist, (size_t)e->cfg.max_pop))) return rc;
    }
    ed.anchor_row.assign(row, row + latent_row_floats(e));
    ed.has_anchor = false;
    return compute_anchor(e);
}

void run_anchor(glass_engine* e, int P) {
    const int L = e->cfg.latent_size, NL = e->n_lat;
    const LatPlan lp = plan_dlatents(e->latent_space, e->trunc_psi, e->trunc_cutoff, NL);
    Prof pr(e, "anchor", 3.0 * P * NL * L, 4.0 * L * (P * (double)(lp.layered ? NL : 1) + NL));
    const bool ok = lp.layered ? launch_latent_anchor(e->d_dlat, (long long)NL * L, L, e->edit.d_anchor, NL, L, P, e->edit.d_dist, e->cur)
                               : launch_latent_anchor(e->d_w0, L, 0, e->edit.d_anchor, NL, L, P, e->edit.d_dist, e->cur);
    if (!ok) {
        pr.drop();
        if (e->launch_error.empty()) e->launch_error = "no kernel accepts layer anchor (latent_anchor: shape outside its limits)";
        return;
    }
    pr.ran("anchor", "latent_anchor_kernel");
}

extern "C" int glass_engine_last_anchor(glass_engine* e, int32_t P, float* d) {
    REQUIRE(e && e->finalized, GLASS_ERR_STATE, "engine not ready");
    REQUIRE(d, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->cfg.anchor && e->edit.has_anchor, GLASS_ERR_STATE, "no anchor is set (glass_config::anchor, glass_engine_set_anchor)");
    REQUIRE(P > 0 && P <= e->last_P, GLASS_ERR_ARG, "P exceeds the last evaluated population");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    GLASS_HIP(hipMemcpy(d, e->edit.d_dist, (size_t)P * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}

// ---- direction source ------------------------------------------------------------------------------
extern "C" int glass_engine_set_direction_source(glass_engine* e, const float* image) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(e->R > 0, GLASS_ERR_STATE,
            "set_direction_source: this engine has no generator (GPT-2 / img2txt): there is no generated image to move away from a source");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "set_direction_source: finalize() first (the image goes through the image tower)");
    glass_engine::Edit& ed = e->edit;
    if (!image) {             // off: the head ends in the kernels it ended in before
        ed.has_source = false;
        ed.rows_valid = false;
        return GLASS_OK;
    }
    GLASS_HIP(hipSetDevice(e->cfg.device));
    const size_t img = (size_t)3 * e->R * e->R;
    if (!ed.d_img) {
        int rc;
        if ((rc = dev_alloc(e, &ed.d_img, img))) return rc;
        if ((rc = dev_alloc(e, &ed.d_src, (size_t)std::max(e->views, 1) * e->cfg.clip_embed))) return rc;
    }
    GLASS_HIP(hipStreamSynchronize(e->stream));
    GLASS_HIP(hipMemcpy(ed.d_img, image, img * sizeof(float), hipMemcpyHostToDevice));
    ed.has_source = true;
    ed.rows_valid = false;
    if (e->views) return GLASS_OK;      // crop views: the rows are those of a pass's own boxes, made when the pass knows them
    e->cur = e->stream;
    e->launch_error.clear();
    const bool prof = e->profiling;
    e->profiling = false;               // (profile rows belong to a pass)
    const int rrc = refresh_direction_source(e);
    e->profiling = prof;
    if (rrc) return rrc;
    GLASS_HIP(hipStreamSynchronize(e->cur));
    GLASS_HIP(hipGetLastError());
    if (!e->launch_error.empty()) {
        const std::string msg = e->launch_error;
        e->launch_error.clear();
        ed.rows_valid = false;
        glass_set_error(msg);
        return GLASS_ERR_STATE;
    }
    return GLASS_OK;
}

static bool same_boxes(const ViewBoxes& a, const ViewBoxes& b, int views) {
    return memcmp(&a.box[0][0], &b.box[0][0], (size_t)views * 4 * sizeof(int32_t)) == 0;
}

// The image through the pass's own preprocessing (whole image, or the views of e->view_boxes) and tower, in the first image slots of the
// tower's buffers — before the pass writes its candidates' patches there —, then unit rows.
int refresh_direction_source(glass_engine* e) {
    glass_engine::Edit& ed = e->edit;
    const int V = std::max(e->views, 1);
    if (ed.rows_valid && (!e->views || same_boxes(ed.boxes, e->view_boxes, e->views))) return GLASS_OK;
    {
        Prof pr(e, "edit.source_resize", 0, clip_resize_bytes(e, 1));
        run_clip_resize(e, ed.d_img, 1, e->d_patches);
    }
    run_clip(e, V, -1);       // the features alone: no cosine
    {
        Prof pr(e, "edit.source_rows", 0, 8.0 * V * e->cfg.clip_embed);
        if (!launch_unit_rows(e->d_feat, V, e->cfg.clip_embed, ed.d_src, e->cur) && e->launch_error.empty())
            e->launch_error = "no kernel accepts layer edit.source_rows";
    }
    ed.boxes = e->view_boxes;
    ed.rows_valid = true;
    return GLASS_OK;
}

extern "C" int glass_engine_last_direction_source(glass_engine* e, float* feats) {
    REQUIRE(e && e->finalized, GLASS_ERR_STATE, "engine not ready");
    REQUIRE(feats, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->edit.has_source, GLASS_ERR_STATE, "no direction source is set (glass_engine_set_direction_source)");
    REQUIRE(e->edit.rows_valid, GLASS_ERR_STATE, "the source rows are made by the first evaluate() after set_direction_source when crop views are on");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    GLASS_HIP(hipStreamSynchronize(e->stream));
    GLASS_HIP(hipMemcpy(feats, e->edit.d_src, (size_t)std::max(e->views, 1) * e->cfg.clip_embed * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}
