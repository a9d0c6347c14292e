// search.cpp — the device search's entry points (include/glass.h "Device search"): the population stays in device buffers and a generation is
// variation, one scoring pass and survival on the engine's stream with one wait at its end.  Kernels: search.hip.
#include <math.h>
#include <string.h>

#include <string>

#include "engine.h"

extern "C" int glass_search_supported(int32_t pop, int32_t n_var, int32_t n_obj, int32_t algorithm) {
    REQUIRE(algorithm == GLASS_SEARCH_GA || algorithm == GLASS_SEARCH_NSGA2 || algorithm == GLASS_SEARCH_CMAES, GLASS_ERR_ARG,
            "device search: algorithm must be 0 (ga), 1 (nsga2) or 2 (cmaes)");
    if (algorithm == GLASS_SEARCH_CMAES) {
        REQUIRE(n_obj == 1, GLASS_ERR_ARG,
                "device search: cmaes minimises one objective and this search has " + std::to_string(n_obj) + " (use nsga2, or fold the others into one)");
        REQUIRE(pop >= GLASS_CMA_MIN_POP && pop <= GLASS_SEARCH_MAX_POP, GLASS_ERR_ARG,
                "device search: cmaes takes pop in [" + std::to_string(GLASS_CMA_MIN_POP) + ", " + std::to_string(GLASS_SEARCH_MAX_POP) +
                    "] (mu = pop / 2 >= 2 rows recombine; one workgroup ranks the rows), got " + std::to_string(pop));
        REQUIRE(n_var >= 1 && (long long)n_var * pop < (1LL << 31), GLASS_ERR_ARG, "device search: n_var must be positive with pop * n_var below 2^31");
        return GLASS_OK;
    }
    REQUIRE(pop >= 2 && pop <= GLASS_SEARCH_MAX_POP, GLASS_ERR_ARG,
            "device search: pop must be in [2, " + std::to_string(GLASS_SEARCH_MAX_POP) + "] (survival ranks 2 pop merged rows in one workgroup), got " +
                std::to_string(pop));
    REQUIRE(n_var >= 1 && (long long)n_var * pop < (1LL << 31), GLASS_ERR_ARG, "device search: n_var must be positive with pop * n_var below 2^31");
    REQUIRE(n_obj >= 1 && n_obj <= GLASS_SEARCH_MAX_OBJ, GLASS_ERR_ARG,
            "device search: n_obj must be in [1, " + std::to_string(GLASS_SEARCH_MAX_OBJ) + "], got " + std::to_string(n_obj));
    REQUIRE(algorithm == GLASS_SEARCH_NSGA2 || n_obj == 1, GLASS_ERR_ARG, "device search: ga ranks by F[:, 0] alone and needs n_obj = 1 (use nsga2)");
    return GLASS_OK;
}

extern "C" int glass_search_mixed_supported(int32_t pop, int32_t n_real, int32_t n_bits, int32_t n_obj, int32_t algorithm) {
    REQUIRE(n_real >= 1, GLASS_ERR_ARG, "device search: a mixed row needs at least one real column in front of its bits (n_real >= 1), got " + std::to_string(n_real));
    REQUIRE(n_bits >= 1 && n_bits <= GLASS_SEARCH_MAX_BITS, GLASS_ERR_ARG,
            "device search: a mixed row has n_bits in [1, " + std::to_string(GLASS_SEARCH_MAX_BITS) + "] (the bit kernel ranks them in one workgroup's LDS), got " +
                std::to_string(n_bits));
    return glass_search_supported(pop, n_real + n_bits, n_obj, algorithm);
}

// what the operators take, whichever setter brings it
static int check_operators(const char* what, double xl, double xu, double eta_c, double eta_m, double prob_m) {
    REQUIRE(isfinite(xl) && isfinite(xu) && xl < xu && (double)(float)xl == xl && (double)(float)xu == xu, GLASS_ERR_ARG,
            std::string(what) + ": xl < xu, both finite and exact in fp32 (the rows are fp32 and are clipped to the bounds)");
    REQUIRE(eta_c >= 0.0 && eta_m >= 0.0 && isfinite(eta_c) && isfinite(eta_m), GLASS_ERR_ARG, std::string(what) + ": eta_c and eta_m must be finite and >= 0");
    REQUIRE(prob_m >= 0.0 && prob_m <= 1.0, GLASS_ERR_ARG, std::string(what) + ": prob_m must be in [0, 1]");
    return GLASS_OK;
}
static int check_bit_operators(const char* what, double prob_x, double prob_flip) {
    REQUIRE(prob_x >= 0.0 && prob_x <= 1.0 && prob_flip >= 0.0 && prob_flip <= 1.0, GLASS_ERR_ARG, std::string(what) + ": prob_x and prob_flip must be in [0, 1]");
    return GLASS_OK;
}
// the checked operators into GaParams (prob_x and prob_flip are the mixed setters' own and stay what they are under the others)
static void store_operators(GaParams& g, double xl, double xu, double eta_c, double eta_m, double prob_m, uint64_t seed) {
    g.xl = xl; g.xu = xu; g.eta_c = eta_c; g.eta_m = eta_m; g.prob_m = prob_m;
    g.seed = seed;
}

extern "C" int glass_engine_set_search(glass_engine* e, int32_t algorithm, int32_t pop, double xl, double xu, double eta_c, double eta_m,
                                       double prob_m, uint64_t seed) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(!e->finalized, GLASS_ERR_STATE, "set_search: the engine is finalized (its buffers are sized in finalize: call it before)");
    if (algorithm == GLASS_SEARCH_CMAES) return cma_set_search(e, pop, xl, xu, seed);      // (eta_c, eta_m and prob_m belong to the GA's operators)
    REQUIRE(e->cfg.generator != GLASS_GEN_BIGGAN_DEEP, GLASS_ERR_STATE,
            "set_search: this setter varies real-valued rows; a BigGAN row holds boolean class bits (HUX / bit-flip): use set_search_mixed");
    REQUIRE(e->n_lat > 0, GLASS_ERR_STATE,
            "set_search: the device search varies real-valued latent rows of a StyleGAN2 generator; this engine has none (GPT-2 rows are integers): "
            "it keeps the host search");
    REQUIRE(e->cfg.noise_mode != 2, GLASS_ERR_STATE, "set_search: caller-provided noise planes (noise_mode 2) come from the host every pass; use noise_mode 0 or 1");
    if (int rc = glass_search_supported(pop, 1, e->cfg.n_obj, algorithm)) return rc;
    REQUIRE(pop <= e->cfg.max_pop && pop % e->cfg.batch_size == 0, GLASS_ERR_ARG,
            "set_search: pop must be a multiple of batch_size and at most max_pop (a generation's offspring are scored in one pass)");
    if (int rc = check_operators("set_search", xl, xu, eta_c, eta_m, prob_m)) return rc;
    glass_engine::Search& s = e->search;
    s.nsga = algorithm == GLASS_SEARCH_NSGA2;
    s.g.pop = pop;
    store_operators(s.g, xl, xu, eta_c, eta_m, prob_m, seed);
    return GLASS_OK;
}

extern "C" int glass_engine_set_search_mixed(glass_engine* e, int32_t algorithm, int32_t pop, int32_t n_real, double xl, double xu, double eta_c,
                                             double eta_m, double prob_m, double prob_x, double prob_flip, uint64_t seed) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(!e->finalized, GLASS_ERR_STATE, "set_search_mixed: the engine is finalized (its buffers are sized in finalize: call it before)");
    REQUIRE(e->n_lat == 0, GLASS_ERR_STATE, "set_search_mixed: a StyleGAN2 row has no bit columns: use set_search");
    REQUIRE(e->cfg.generator == GLASS_GEN_BIGGAN_DEEP, GLASS_ERR_STATE,
            "set_search_mixed: the device search varies the latent rows of a generator; this engine has none (GPT-2 rows are integers): it keeps the host "
            "search");
    REQUIRE(n_real == e->cfg.bg_z_dim, GLASS_ERR_ARG,
            "set_search_mixed: a BigGAN row is [z | class bits]: n_real must be z_dim = " + std::to_string(e->cfg.bg_z_dim) + ", got " + std::to_string(n_real));
    if (int rc = glass_search_mixed_supported(pop, n_real, e->cfg.bg_num_classes, e->cfg.n_obj, algorithm)) return rc;
    REQUIRE(pop <= e->cfg.max_pop && pop % e->cfg.batch_size == 0, GLASS_ERR_ARG,
            "set_search_mixed: pop must be a multiple of batch_size and at most max_pop (a generation's offspring are scored in one pass)");
    if (int rc = check_operators("set_search_mixed", xl, xu, eta_c, eta_m, prob_m)) return rc;
    if (int rc = check_bit_operators("set_search_mixed", prob_x, prob_flip)) return rc;
    glass_engine::Search& s = e->search;
    s.nsga = algorithm == GLASS_SEARCH_NSGA2;
    s.n_real = n_real;
    s.g.pop = pop;
    store_operators(s.g, xl, xu, eta_c, eta_m, prob_m, seed);
    s.g.prob_x = prob_x; s.g.prob_flip = prob_flip;
    return GLASS_OK;
}

extern "C" int glass_engine_set_search_operators_mixed(glass_engine* e, double xl, double xu, double eta_c, double eta_m, double prob_m, double prob_x,
                                                       double prob_flip, uint64_t seed) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(e->search.g.pop > 0 && e->search.n_real > 0, GLASS_ERR_STATE,
            "set_search_operators_mixed: no mixed device search is on (glass_engine_set_search_mixed before finalize)");
    if (int rc = check_operators("set_search_operators_mixed", xl, xu, eta_c, eta_m, prob_m)) return rc;
    if (int rc = check_bit_operators("set_search_operators_mixed", prob_x, prob_flip)) return rc;
    GaParams& g = e->search.g;
    store_operators(g, xl, xu, eta_c, eta_m, prob_m, seed);
    g.prob_x = prob_x; g.prob_flip = prob_flip;
    return GLASS_OK;
}

extern "C" int glass_engine_set_search_operators(glass_engine* e, double xl, double xu, double eta_c, double eta_m, double prob_m, uint64_t seed) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(e->search.g.pop > 0, GLASS_ERR_STATE, "set_search_operators: the device search is off (glass_engine_set_search before finalize)");
    if (int rc = check_operators("set_search_operators", xl, xu, eta_c, eta_m, prob_m)) return rc;
    store_operators(e->search.g, xl, xu, eta_c, eta_m, prob_m, seed);
    return GLASS_OK;
}

// ---- islands (include/glass.h "Device search: islands") ----
extern "C" int glass_search_islands_supported(int32_t islands, int32_t pop, int32_t n_var, int32_t n_obj, int32_t algorithm, int32_t migrate_every,
                                              int32_t migrants) {
    REQUIRE(algorithm != GLASS_SEARCH_CMAES, GLASS_ERR_ARG,
            "device search islands: cmaes keeps one distribution, not populations; islands of distributions are a different feature (use ga or nsga2)");
    if (int rc = glass_search_supported(pop, n_var, n_obj, algorithm)) return rc;
    REQUIRE(islands >= 1 && islands <= GLASS_SEARCH_MAX_ISLANDS, GLASS_ERR_ARG,
            "device search islands: islands must be in [1, " + std::to_string(GLASS_SEARCH_MAX_ISLANDS) + "], got " + std::to_string(islands));
    REQUIRE((long long)islands * pop * n_var < (1LL << 31), GLASS_ERR_ARG,
            "device search islands: islands * pop * n_var must be below 2^31, got " + std::to_string((long long)islands * pop * n_var));
    REQUIRE(migrate_every >= 0, GLASS_ERR_ARG, "device search islands: migrate_every must be >= 0 (0: never), got " + std::to_string(migrate_every));
    REQUIRE(migrants >= 1 && migrants <= pop / 2, GLASS_ERR_ARG,
            "device search islands: migrants must be in [1, pop / 2 = " + std::to_string(pop / 2) +
                "] (an island's best rows leave and its worst are replaced: the two must be disjoint), got " + std::to_string(migrants));
    return GLASS_OK;
}

extern "C" int glass_engine_set_search_islands(glass_engine* e, int32_t islands, int32_t migrate_every, int32_t migrants) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(!e->finalized, GLASS_ERR_STATE, "set_search_islands: the engine is finalized (its buffers are sized in finalize: call it before)");
    glass_engine::Search& s = e->search;
    REQUIRE(s.g.pop > 0, GLASS_ERR_STATE, "set_search_islands: the device search is off (glass_engine_set_search or set_search_mixed first)");
    REQUIRE(!s.cma, GLASS_ERR_STATE,
            "set_search_islands: this is a cmaes search, which keeps one distribution, not populations; islands of distributions are a different feature");
    if (int rc = glass_search_islands_supported(islands, s.g.pop, 1, e->cfg.n_obj, s.nsga, migrate_every, migrants)) return rc;
    REQUIRE((long long)islands * s.g.pop <= e->cfg.max_pop, GLASS_ERR_ARG,
            "set_search_islands: islands * pop = " + std::to_string((long long)islands * s.g.pop) + " rows are scored in one pass and max_pop is " +
                std::to_string(e->cfg.max_pop));
    s.islands = islands;
    s.migrate_every = migrate_every;
    s.migrants = migrants;
    return GLASS_OK;
}

extern "C" int glass_engine_set_island_weights(glass_engine* e, const float* w, int32_t islands, int32_t T) {
    REQUIRE(e && w, GLASS_ERR_ARG, "null argument");
    REQUIRE(e->finalized, GLASS_ERR_STATE, "set_island_weights: finalize() and set_targets() first (the weights are over the entries of a prompt set)");
    glass_engine::Search& s = e->search;
    glass_engine::PromptSet& ps = e->pset;
    REQUIRE(s.islands >= 1, GLASS_ERR_STATE, "set_island_weights: this search has no islands (glass_engine_set_search_islands before finalize)");
    REQUIRE(islands == s.islands, GLASS_ERR_ARG,
            "set_island_weights: the table has " + std::to_string(islands) + " rows and the search " + std::to_string(s.islands) + " islands");
    REQUIRE(ps.given(), GLASS_ERR_STATE, "set_island_weights: set_targets() first (the islands' prompts are the entries of a prompt set)");
    REQUIRE(T == ps.T, GLASS_ERR_ARG,
            "set_island_weights: the table has " + std::to_string(T) + " columns and the prompt set " + std::to_string(ps.T) + " entries");
    REQUIRE(ps.mode == 0, GLASS_ERR_STATE,
            "set_island_weights: own prompts combine the entries per island in mode sum; this prompt set is in mode pareto (one column of F per entry)");
    REQUIRE(!e->edit.has_source, GLASS_ERR_STATE,
            "set_island_weights: own prompts are not combined with a direction source (the set's entries are then directions from one source)");
    REQUIRE(!(s.islands > 1 && s.migrate_every > 0), GLASS_ERR_STATE,
            "set_island_weights: own prompts are not combined with migration (a migrant's F would be stale under another island's objective): "
            "set_search_islands with migrate_every 0");
    float W[GLASS_SEARCH_MAX_ISLANDS];
    for (int i = 0; i < islands; ++i) {
        for (int t = 0; t < T; ++t)
            REQUIRE(isfinite(w[(size_t)i * T + t]), GLASS_ERR_ARG, "set_island_weights: island " + std::to_string(i) + " weight " + std::to_string(t) + " is not finite");
        W[i] = prompt_weight_sum(w + (size_t)i * T, T);
        REQUIRE(W[i] > 0.f, GLASS_ERR_ARG, "set_island_weights: island " + std::to_string(i) + " has no non-zero weight");
    }
    GLASS_HIP(hipSetDevice(e->cfg.device));
    if (!ps.d_isl_weights) {
        int rc;
        if ((rc = dev_alloc(e, &ps.d_isl_weights, (size_t)GLASS_SEARCH_MAX_ISLANDS * GLASS_PROMPT_MAX))) return rc;
        if ((rc = dev_alloc(e, &ps.d_isl_W, (size_t)GLASS_SEARCH_MAX_ISLANDS))) return rc;
    }
    GLASS_HIP(hipMemcpy(ps.d_isl_weights, w, (size_t)islands * T * sizeof(float), hipMemcpyHostToDevice));
    GLASS_HIP(hipMemcpy(ps.d_isl_W, W, (size_t)islands * sizeof(float), hipMemcpyHostToDevice));
    ps.isl_T = T;
    s.own_prompts = true;
    return GLASS_OK;
}

int alloc_search(glass_engine* e) {
    glass_engine::Search& s = e->search;
    if (!s.g.pop) return GLASS_OK;
    const int pop = s.g.pop, M = e->cfg.n_obj;
    s.n_var = (int)latent_row_floats(e);
    REQUIRE(!(s.cma && s.islands), GLASS_ERR_STATE, "finalize: a cmaes search keeps one distribution and has no islands (set_search_islands is for ga / nsga2)");
    if (s.cma) return alloc_cma(e);
    REQUIRE(s.rows() <= e->cfg.max_pop, GLASS_ERR_ARG, "finalize: islands * pop rows are scored in one pass and exceed max_pop");
    if (int rc = s.n_real ? glass_search_mixed_supported(pop, s.n_real, s.n_var - s.n_real, M, s.nsga) : glass_search_supported(pop, s.n_var, M, s.nsga))
        return rc;
    if (s.islands)
        if (int rc = glass_search_islands_supported(s.islands, pop, s.n_var, M, s.nsga, s.migrate_every, s.migrants)) return rc;
    int rc;
    const size_t R = (size_t)s.rows(), xn = R * s.n_var, nc = (size_t)3 * s.k();
    if ((rc = dev_alloc(e, &s.X[0], xn))) return rc;
    if ((rc = dev_alloc(e, &s.X[1], xn))) return rc;
    if ((rc = dev_alloc(e, &s.Xoff, xn))) return rc;
    if ((rc = dev_alloc(e, &s.F, 2 * R * M))) return rc;
    if ((rc = dev_alloc(e, &s.rank, R))) return rc;
    if ((rc = dev_alloc(e, &s.cd, R))) return rc;
    if ((rc = dev_alloc(e, &s.flags, R))) return rc;
    if ((rc = dev_alloc(e, &s.chosen, R))) return rc;
    if ((rc = dev_alloc(e, &s.counts, nc))) return rc;
    GLASS_HIP(hipMemset(s.flags, 0, R * sizeof(int)));
    GLASS_HIP(hipMemset(s.counts, 0, nc * sizeof(int)));
    GLASS_HIP(hipMemset(s.F, 0, 2 * R * M * sizeof(float)));
    return GLASS_OK;
}

int search_ready(glass_engine* e, const char* what, bool need_init) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    REQUIRE(e->finalized, GLASS_ERR_STATE, std::string(what) + ": finalize() first");
    REQUIRE(e->search.g.pop > 0, GLASS_ERR_STATE, std::string(what) + ": the device search is off (glass_engine_set_search before finalize)");
    REQUIRE(e->latent_space != GLASS_LATENT_SUB || e->has_subspace, GLASS_ERR_STATE, std::string(what) + ": set_subspace() first (latent space sub)");
    if (need_init && e->search.cma)
        REQUIRE(e->search.ready, GLASS_ERR_STATE, std::string(what) + ": search_init_cma() first (there is no distribution on the device)");
    if (need_init) REQUIRE(e->search.ready, GLASS_ERR_STATE, std::string(what) + ": search_init() first (there is no population on the device)");
    GLASS_HIP(hipSetDevice(e->cfg.device));
    e->cur = e->stream;
    return GLASS_OK;
}
namespace {
// the launches of the three phases, on e->cur; nothing here waits
void launch_vary(glass_engine* e, int generation) {
    glass_engine::Search& s = e->search;
    const int pop = s.g.pop, K = s.k(), n_real = s.n_real ? s.n_real : s.n_var, n_bits = s.n_var - n_real;
    const double xbytes = (double)s.rows() * s.n_var * sizeof(float);
    const double real_share = (double)n_real / s.n_var;
    profiled_launch(e, "search.vary", 3 * xbytes * real_share,
                    [&] { return launch_ga_vary(s.X[s.cur], s.rank, s.cd, s.g, K, n_real, n_bits, generation, 0, pop, GA_VARY_REAL, s.Xoff, e->cur); });
    if (n_bits)      // mixed rows: HUX and bit-flip on the bit columns behind the real ones
        profiled_launch(e, "search.vary_bits", 3 * xbytes * (1.0 - real_share),
                        [&] { return launch_ga_vary(s.X[s.cur], s.rank, s.cd, s.g, K, n_real, n_bits, generation, 0, pop, GA_VARY_BITS, s.Xoff, e->cur); });
    profiled_launch(e, "search.duplicates", 2 * xbytes, [&] { return launch_ga_duplicates(s.X[s.cur], s.Xoff, K, pop, pop, s.n_var, s.flags, e->cur); });
    s.varied_gen = generation;
}
// survival of every island and the gather of the survivors' rows, under one profile row.  rerank (n_off 0, behind a migration): only the
// islands that accepted a migrant, ranked (and ordered) again as search_init ranks a population
bool launch_survive(glass_engine* e, int n_off, bool rerank = false) {
    glass_engine::Search& s = e->search;
    const int pop = s.g.pop, K = s.k(), M = e->cfg.n_obj;
    return profiled_launch(e, rerank ? "search.rerank" : "search.survive", 2.0 * s.rows() * s.n_var * sizeof(float), [&] {
        const char* k = launch_ga_survive(s.F, s.F + (size_t)s.rows() * M, n_off ? s.flags : nullptr, K, pop, n_off, M, pop, s.nsga, rerank, s.chosen, s.rank,
                                          s.cd, s.counts, e->cur);
        if (k) {
            launch_ga_gather(s.X[s.cur], s.Xoff, s.chosen, K, pop, pop, s.n_var, s.X[s.cur ^ 1], e->cur);
            s.cur ^= 1;
        }
        return k;
    }, " (or the device offers too little LDS)");
}
// whether the rule has a migration behind the survival of this generation
bool migration_due(const glass_engine::Search& s, int generation) {
    return s.islands > 1 && s.migrate_every > 0 && generation >= 1 && generation % s.migrate_every == 0;
}
// migration in place, then the islands that accepted a row ranked (and ordered) again as search_init ranks a population
void launch_migrate(glass_engine* e) {
    glass_engine::Search& s = e->search;
    const int K = s.k();
    if (profiled_launch(e, "search.migrate", 2.0 * K * s.migrants * s.n_var * sizeof(float), [&] {
            return launch_ga_migrate(s.X[s.cur], s.F, s.rank, s.cd, K, s.g.pop, s.n_var, e->cfg.n_obj, s.migrants, s.counts, e->cur);
        }))
        launch_survive(e, 0, true);
}
// a scoring pass of search rows [first_row, first_row + P): with islands the noise planes are those of the minibatch's index within its island
int search_pass(glass_engine* e, int P, int generation, int first_row, const float* d_rows, float* d_F, bool no_wait) {
    const glass_engine::Search& s = e->search;
    if (s.own_prompts)
        REQUIRE(e->pset.given() && e->pset.T == e->pset.isl_T && e->pset.mode == 0 && !e->edit.has_source, GLASS_ERR_STATE,
                "device search islands: the islands' own weights were set for a prompt set of " + std::to_string(e->pset.isl_T) +
                    " entries in mode sum without a direction source, and the engine's targets have changed: set_island_weights again");
    e->noise_period = s.islands ? s.g.pop / e->cfg.batch_size : 0;
    e->island_row0 = s.islands ? first_row : -1;
    const int rc = run_pass(e, nullptr, P, generation, first_row / e->cfg.batch_size, nullptr, nullptr, nullptr, d_rows, d_F, no_wait);
    e->noise_period = 0;
    e->island_row0 = -1;
    return rc;
}
}  // namespace
// the wait behind launches made outside a pass
int search_wait(glass_engine* e) {
    GLASS_HIP(hipStreamSynchronize(e->cur));
    GLASS_HIP(hipGetLastError());
    if (e->profiling) collect_profile(e);
    if (!e->launch_error.empty()) {
        const std::string msg = e->launch_error;
        e->launch_error.clear();
        glass_set_error(msg);
        return GLASS_ERR_STATE;
    }
    return GLASS_OK;
}
// counts [2] = {flagged, non-finite} rows of the last survival, summed over the islands; per_island [islands][3]; both nullable
static int read_counts(glass_engine* e, int* counts, int* per_island) {
    const glass_engine::Search& s = e->search;
    const int K = s.k();
    int h[3 * GLASS_SEARCH_MAX_ISLANDS];
    GLASS_HIP(hipMemcpy(h, s.counts, (size_t)3 * K * sizeof(int), hipMemcpyDeviceToHost));
    if (counts) counts[0] = counts[1] = 0;
    for (int i = 0; i < K && counts; ++i) { counts[0] += h[3 * i]; counts[1] += h[3 * i + 1]; }
    if (per_island) memcpy(per_island, h, (size_t)3 * K * sizeof(int));
    return GLASS_OK;
}
namespace {
int check_rows(glass_engine* e, const char* what, int generation, int first_row, int rows) {
    const glass_engine::Search& s = e->search;
    REQUIRE(s.varied_gen == generation, GLASS_ERR_STATE,
            std::string(what) + ": the offspring buffer holds generation " + std::to_string(s.varied_gen) + " (search_vary of this generation first)");
    REQUIRE(rows > 0 && first_row >= 0 && first_row + rows <= s.rows() && first_row % e->cfg.batch_size == 0 && rows % e->cfg.batch_size == 0,
            GLASS_ERR_ARG, std::string(what) + ": [first_row, first_row + rows) must be whole minibatches inside the offspring rows");
    return GLASS_OK;
}
}  // namespace

extern "C" int glass_engine_search_init(glass_engine* e, const float* X0) {
    if (int rc = search_ready(e, "search_init", false)) return rc;
    REQUIRE(X0, GLASS_ERR_ARG, "search_init: null population");
    REQUIRE(!e->search.cma, GLASS_ERR_STATE,
            "search_init: a cmaes search keeps a distribution, not a population: search_init_cma(mean, diag, sigma)");
    glass_engine::Search& s = e->search;
    const int pop = s.rows();      // (islands: every island's rows, island-major)
    s.ready = false;
    s.cur = 0;
    s.varied_gen = s.survived_gen = -1;
    if (s.n_real)      // mixed rows: a bit column holds exactly 0.0 or 1.0
        for (int r = 0; r < pop; ++r)
            for (int j = s.n_real; j < s.n_var; ++j) {
                const float v = X0[(size_t)r * s.n_var + j];
                REQUIRE(v == 0.0f || v == 1.0f, GLASS_ERR_ARG,
                        "search_init: row " + std::to_string(r) + " column " + std::to_string(j) + " is a bit column and holds " + std::to_string(v) +
                            " (a bit is exactly 0.0 or 1.0)");
            }
    GLASS_HIP(hipMemcpy(s.X[0], X0, (size_t)pop * s.n_var * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = search_pass(e, pop, 0, 0, s.X[0], s.F, true)) return rc;
    launch_survive(e, 0);      // ranks (and orders) the initial population, as minimize's first survive() does
    if (int rc = wait_pass(e, pop)) return rc;
    int counts[2];
    if (int rc = read_counts(e, counts, nullptr)) return rc;
    REQUIRE(counts[1] == 0, GLASS_ERR_STATE,
            "search_init: " + std::to_string(counts[1]) + " rows of the initial population have a non-finite F: a population row is never left out");
    s.ready = true;
    return GLASS_OK;
}

extern "C" int glass_engine_search_vary(glass_engine* e, int32_t generation) {
    if (int rc = search_ready(e, "search_vary", true)) return rc;
    if (e->search.cma) return cma_vary(e, generation);
    e->launch_error.clear();
    launch_vary(e, generation);
    return search_wait(e);
}

extern "C" int glass_engine_search_evaluate(glass_engine* e, int32_t generation, int32_t first_row, int32_t rows) {
    if (int rc = search_ready(e, "search_evaluate", true)) return rc;
    if (int rc = check_rows(e, "search_evaluate", generation, first_row, rows)) return rc;
    glass_engine::Search& s = e->search;
    return search_pass(e, rows, generation, first_row, s.Xoff + (size_t)first_row * s.n_var, s.F + (size_t)(s.rows() + first_row) * e->cfg.n_obj, false);
}

extern "C" int glass_engine_search_survive(glass_engine* e, int32_t generation) {
    if (int rc = search_ready(e, "search_survive", true)) return rc;
    REQUIRE(e->search.varied_gen == generation, GLASS_ERR_STATE, "search_survive: search_vary and search_evaluate of this generation first");
    if (e->search.cma) return cma_survive(e, generation);
    e->launch_error.clear();
    launch_survive(e, e->search.g.pop);
    e->search.varied_gen = -1;      // the offspring are spent: the next survival needs a new search_vary
    e->search.survived_gen = generation;
    return search_wait(e);
}

extern "C" int glass_engine_search_migrate(glass_engine* e, int32_t generation) {
    if (int rc = search_ready(e, "search_migrate", true)) return rc;
    glass_engine::Search& s = e->search;
    REQUIRE(s.islands >= 1, GLASS_ERR_STATE, "search_migrate: this search has no islands (glass_engine_set_search_islands before finalize)");
    REQUIRE(s.survived_gen == generation, GLASS_ERR_STATE,
            "search_migrate: search_survive of this generation first (migration follows a generation's survival, once)");
    s.survived_gen = -1;
    if (!migration_due(s, generation)) return GLASS_OK;
    e->launch_error.clear();
    launch_migrate(e);
    return search_wait(e);
}

extern "C" int glass_engine_search_step(glass_engine* e, int32_t generation) {
    if (int rc = search_ready(e, "search_step", true)) return rc;
    if (e->search.cma) return cma_step(e, generation);
    glass_engine::Search& s = e->search;
    const int pop = s.rows();
    e->launch_error.clear();
    launch_vary(e, generation);
    const std::string refused = e->launch_error;      // (run_pass clears the message on entry)
    if (int rc = search_pass(e, pop, generation, 0, s.Xoff, s.F + (size_t)pop * e->cfg.n_obj, true)) return rc;
    if (!refused.empty()) e->launch_error = refused;
    launch_survive(e, s.g.pop);
    s.varied_gen = s.survived_gen = -1;
    if (migration_due(s, generation) && e->launch_error.empty()) launch_migrate(e);
    return wait_pass(e, pop);
}

extern "C" int glass_engine_search_read(glass_engine* e, float* pop_X, float* pop_F, int32_t* rank, double* cd, float* off_X, float* off_F,
                                        int32_t* flags, int32_t* counts) {
    if (int rc = search_ready(e, "search_read", true)) return rc;
    const glass_engine::Search& s = e->search;
    REQUIRE(!s.cma || !(pop_X || pop_F || rank || cd || flags), GLASS_ERR_STATE,
            "search_read: a cmaes search has no population, ranks, distances or flags: its rows are off_X / off_F, its state search_read_cma");
    const size_t pop = (size_t)s.rows(), xb = pop * s.n_var * sizeof(float), fb = pop * e->cfg.n_obj * sizeof(float);
    GLASS_HIP(hipStreamSynchronize(e->stream));
    if (pop_X) GLASS_HIP(hipMemcpy(pop_X, s.X[s.cur], xb, hipMemcpyDeviceToHost));
    if (pop_F) GLASS_HIP(hipMemcpy(pop_F, s.F, fb, hipMemcpyDeviceToHost));
    if (rank) GLASS_HIP(hipMemcpy(rank, s.rank, pop * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (cd) GLASS_HIP(hipMemcpy(cd, s.cd, pop * sizeof(double), hipMemcpyDeviceToHost));
    if (off_X) GLASS_HIP(hipMemcpy(off_X, s.Xoff, xb, hipMemcpyDeviceToHost));
    if (off_F) GLASS_HIP(hipMemcpy(off_F, s.F + pop * e->cfg.n_obj, fb, hipMemcpyDeviceToHost));
    if (flags) GLASS_HIP(hipMemcpy(flags, s.flags, pop * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (counts)
        if (int rc = read_counts(e, counts, nullptr)) return rc;
    return GLASS_OK;
}

extern "C" int glass_engine_search_read_islands(glass_engine* e, int32_t* counts) {
    if (int rc = search_ready(e, "search_read_islands", true)) return rc;
    REQUIRE(e->search.islands >= 1, GLASS_ERR_STATE, "search_read_islands: this search has no islands (glass_engine_set_search_islands before finalize)");
    REQUIRE(counts, GLASS_ERR_ARG, "search_read_islands: null counts");
    GLASS_HIP(hipStreamSynchronize(e->stream));
    return read_counts(e, nullptr, counts);
}

extern "C" int glass_engine_latent_uploads(glass_engine* e, int64_t* calls, int64_t* rows) {
    REQUIRE(e, GLASS_ERR_ARG, "null engine");
    if (calls) *calls = e->latent_uploads;
    if (rows) *rows = e->latent_upload_rows;
    return GLASS_OK;
}
