// cmaes.cpp — the sep-CMA-ES device search's host side (include/glass.h "Device search: sep-CMA-ES"): the distribution stays in device
// buffers and a generation is sample, one scoring pass, rank and update on the engine's stream with one wait at its end.  The search_*
// entry points of search.cpp come here when the engine's search is a CMA one.  Kernels: cmaes.hip.
#include <math.h>
#include <string.h>

#include <limits>
#include <string>
#include <vector>

#include "engine.h"

int cma_set_search(glass_engine* e, int pop, double xl, double xu, uint64_t seed) {
    REQUIRE(e->cfg.n_obj == 1, GLASS_ERR_STATE,
            "set_search: cmaes minimises one objective and this engine has " + std::to_string(e->cfg.n_obj) +
                ": use nsga2, or an engine without the discriminator column and with the LPIPS / anchor distance folded in (lambda > 0)");
    REQUIRE(e->cfg.generator != GLASS_GEN_BIGGAN_DEEP, GLASS_ERR_STATE,
            "set_search: cmaes samples real-valued rows; a BigGAN row holds boolean class bits: use set_search_mixed with ga");
    REQUIRE(e->n_lat > 0, GLASS_ERR_STATE,
            "set_search: cmaes samples real-valued latent rows of a StyleGAN2 generator; this engine has none (GPT-2 rows are integers): it keeps "
            "the host search");
    REQUIRE(e->cfg.noise_mode != 2, GLASS_ERR_STATE, "set_search: caller-provided noise planes (noise_mode 2) come from the host every pass; use noise_mode 0 or 1");
    if (int rc = glass_search_supported(pop, 1, e->cfg.n_obj, GLASS_SEARCH_CMAES)) return rc;
    REQUIRE(pop <= e->cfg.max_pop && pop % e->cfg.batch_size == 0, GLASS_ERR_ARG,
            "set_search: pop must be a multiple of batch_size and at most max_pop (a generation's rows are scored in one pass)");
    REQUIRE(isfinite(xl) && isfinite(xu) && xl < xu && (double)(float)xl == xl && (double)(float)xu == xu, GLASS_ERR_ARG,
            "set_search: xl < xu, both finite and exact in fp32 (the rows are fp32 and are clipped to the bounds)");
    glass_engine::Search& s = e->search;
    s.cma = true;
    s.nsga = 0;
    s.g = {};
    s.g.pop = pop;
    s.g.xl = xl; s.g.xu = xu;
    s.g.eta_c = s.g.eta_m = 3.0; s.g.prob_m = 0.5;      // (unused; what set_search_operators would check)
    s.g.seed = seed;
    return GLASS_OK;
}

int alloc_cma(glass_engine* e) {
    glass_engine::Search& s = e->search;
    const int pop = s.g.pop, M = e->cfg.n_obj, n = s.n_var;
    if (int rc = glass_search_supported(pop, n, M, GLASS_SEARCH_CMAES)) return rc;
    int rc;
    CmaState& c = s.cs;
    if ((rc = dev_alloc(e, &s.Xoff, (size_t)pop * n))) return rc;
    if ((rc = dev_alloc(e, &s.F, (size_t)2 * pop * M))) return rc;      // the GA's layout: a generation's F is the second half
    if ((rc = dev_alloc(e, &s.counts, (size_t)3))) return rc;           // the GA's layout, [1][3]: the generation's two counters, the third unused
    if ((rc = dev_alloc(e, &c.m, (size_t)4 * n))) return rc;
    c.d = c.m + n; c.ps = c.m + 2 * (size_t)n; c.pc = c.m + 3 * (size_t)n;
    if ((rc = dev_alloc(e, &c.yw, (size_t)2 * n))) return rc;
    c.s2 = c.yw + n;
    if ((rc = dev_alloc(e, &c.part, (size_t)cma_blocks(n)))) return rc;
    if ((rc = dev_alloc(e, &c.sc, (size_t)1))) return rc;
    if ((rc = dev_alloc(e, &c.order, (size_t)pop))) return rc;
    if ((rc = dev_alloc(e, &c.best_X, (size_t)n))) return rc;
    c.counts = s.counts;
    std::vector<double> w((size_t)pop / 2);
    cma_weights(pop, w.data());
    if ((rc = upload(e, &c.w, w))) return rc;
    GLASS_HIP(hipMemset(s.counts, 0, 3 * sizeof(int)));
    GLASS_HIP(hipMemset(s.F, 0, (size_t)2 * pop * M * sizeof(float)));
    GLASS_HIP(hipMemset(c.order, 0, (size_t)pop * sizeof(int)));
    GLASS_HIP(hipMemset(c.sc, 0, sizeof(CmaScalars)));
    return GLASS_OK;
}

namespace {
CmaParams params_of(const glass_engine* e) {
    const glass_engine::Search& s = e->search;
    return cma_params(s.g.pop, s.n_var, s.g.xl, s.g.xu, s.g.seed);
}
// the launches of the phases, on e->cur; nothing here waits
void launch_sample(glass_engine* e, int generation) {
    glass_engine::Search& s = e->search;
    profiled_launch(e, "search.cma_sample", (double)s.g.pop * s.n_var * sizeof(float),
                    [&] { return launch_cma_sample(s.cs, params_of(e), generation, 0, s.g.pop, s.Xoff, e->cur); });
    s.varied_gen = generation;
}
void launch_rank_update(glass_engine* e, int generation) {
    glass_engine::Search& s = e->search;
    const CmaParams p = params_of(e);
    const float* F = s.F + (size_t)s.g.pop * e->cfg.n_obj;
    // (no rank: no update either — it would read an order nobody wrote)
    if (!profiled_launch(e, "search.cma_rank", (double)s.g.pop * sizeof(float), [&] { return launch_cma_rank(s.cs, p, F, e->cur); })) return;
    profiled_launch(e, "search.cma_update", (0.5 * s.g.pop + 1.0) * s.n_var * sizeof(float) + 10.0 * s.n_var * sizeof(double),
                    [&] { return launch_cma_update(s.cs, p, s.Xoff, generation, e->cur); });
}
}  // namespace

int cma_vary(glass_engine* e, int generation) {
    REQUIRE(generation >= 0, GLASS_ERR_ARG, "search_vary: a cmaes generation is 0, 1, ...");
    e->launch_error.clear();
    launch_sample(e, generation);
    return search_wait(e);
}

int cma_survive(glass_engine* e, int generation) {
    e->launch_error.clear();
    launch_rank_update(e, generation);
    e->search.varied_gen = -1;      // the rows are spent: the next update needs a new search_vary
    return search_wait(e);
}

int cma_step(glass_engine* e, int generation) {
    REQUIRE(generation >= 0, GLASS_ERR_ARG, "search_step: a cmaes generation is 0, 1, ...");
    glass_engine::Search& s = e->search;
    const int pop = s.g.pop;
    e->launch_error.clear();
    launch_sample(e, generation);
    const std::string refused = e->launch_error;      // (run_pass clears the message on entry)
    if (int rc = run_pass(e, nullptr, pop, generation, 0, nullptr, nullptr, nullptr, s.Xoff, s.F + (size_t)pop * e->cfg.n_obj, true)) return rc;
    if (!refused.empty()) e->launch_error = refused;
    launch_rank_update(e, generation);
    s.varied_gen = -1;
    return wait_pass(e, pop);
}

extern "C" int glass_engine_search_init_cma(glass_engine* e, const double* mean0, const double* diag0, double sigma0) {
    if (int rc = search_ready(e, "search_init_cma", false)) return rc;
    glass_engine::Search& s = e->search;
    REQUIRE(s.cma, GLASS_ERR_STATE, "search_init_cma: this engine's search is ga / nsga2 (glass_engine_set_search with algorithm 2 before finalize): search_init");
    REQUIRE(mean0, GLASS_ERR_ARG, "search_init_cma: null mean");
    REQUIRE(isfinite(sigma0) && sigma0 > 0.0, GLASS_ERR_ARG, "search_init_cma: sigma0 must be finite and positive");
    const int n = s.n_var;
    std::vector<double> st((size_t)4 * n, 0.0);
    for (int j = 0; j < n; ++j) {
        REQUIRE(isfinite(mean0[j]), GLASS_ERR_ARG, "search_init_cma: mean0[" + std::to_string(j) + "] is not finite");
        const double d = diag0 ? diag0[j] : 1.0;
        REQUIRE(isfinite(d) && d > 0.0, GLASS_ERR_ARG, "search_init_cma: diag0[" + std::to_string(j) + "] must be finite and positive");
        st[j] = mean0[j];
        st[(size_t)n + j] = d;
    }
    s.ready = false;
    s.varied_gen = -1;
    CmaScalars sc = {};
    sc.sigma = sigma0;
    sc.best_F = std::numeric_limits<float>::infinity();
    sc.best_src = -1;
    GLASS_HIP(hipStreamSynchronize(e->stream));
    GLASS_HIP(hipMemcpy(s.cs.m, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemcpy(s.cs.sc, &sc, sizeof sc, hipMemcpyHostToDevice));
    GLASS_HIP(hipMemset(s.cs.best_X, 0, (size_t)n * sizeof(float)));
    GLASS_HIP(hipMemset(s.counts, 0, 2 * sizeof(int)));
    s.ready = true;
    return GLASS_OK;
}

extern "C" int glass_engine_search_read_cma(glass_engine* e, double* mean, double* diag, double* p_sigma, double* p_c, double* scalars_d,
                                            int32_t* scalars_i, float* best_X, float* best_F) {
    if (int rc = search_ready(e, "search_read_cma", true)) return rc;
    const glass_engine::Search& s = e->search;
    REQUIRE(s.cma, GLASS_ERR_STATE, "search_read_cma: this engine's search is ga / nsga2: search_read");
    const size_t nb = (size_t)s.n_var * sizeof(double);
    GLASS_HIP(hipStreamSynchronize(e->stream));
    if (mean) GLASS_HIP(hipMemcpy(mean, s.cs.m, nb, hipMemcpyDeviceToHost));
    if (diag) GLASS_HIP(hipMemcpy(diag, s.cs.d, nb, hipMemcpyDeviceToHost));
    if (p_sigma) GLASS_HIP(hipMemcpy(p_sigma, s.cs.ps, nb, hipMemcpyDeviceToHost));
    if (p_c) GLASS_HIP(hipMemcpy(p_c, s.cs.pc, nb, hipMemcpyDeviceToHost));
    if (scalars_d || scalars_i || best_F) {
        CmaScalars sc;
        GLASS_HIP(hipMemcpy(&sc, s.cs.sc, sizeof sc, hipMemcpyDeviceToHost));
        if (scalars_d) { scalars_d[0] = sc.sigma; scalars_d[1] = sc.ps_norm; }
        if (scalars_i) { scalars_i[0] = sc.h; scalars_i[1] = sc.finite; scalars_i[2] = sc.updated; scalars_i[3] = sc.skipped; scalars_i[4] = sc.updates; }
        if (best_F) *best_F = sc.best_F;
    }
    if (best_X) GLASS_HIP(hipMemcpy(best_X, s.cs.best_X, (size_t)s.n_var * sizeof(float), hipMemcpyDeviceToHost));
    return GLASS_OK;
}
