// extern "C" boundary of libadmm_hip.so (see include/admm_hip.h): every function describes its call (call_args.h) and makes it (calls.h).
#include "calls.h"
#include "comm.h"
#include "inproc.h"
#include "test_hooks.h"

using namespace admm;

template <typename F>
static int guarded(F&& f) {
    try {
        check_option_overlay();
        f();
        return ADMM_OK;
    } catch (const Error& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("host allocation failed");
        return ADMM_ERR_INTERNAL;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return ADMM_ERR_INTERNAL;
    }
}

// The lambda-path arguments every path entry point carries, in the header's order; alpha < 0: the plain Lasso.
#define PATH_SPEC(alpha) PathSpec{lambda_in, nlambda_in, nlambda_auto, lmin_ratio, standardize, intercept, (alpha), opts}
#define PATH_OUT PathOut{lambda_out, beta_out, niter_out, stats}
// What every dense entry point (basis pursuit, LAD and the losses on LAD's loop) writes to, by the header's parameter names: the
// plain form, with the decision trace, and with the trace and the iterate dump.
#define DENSE_OUT DenseOut{beta_out, niter_out, stats}
#define DENSE_OUT_TRACED DenseOut{beta_out, niter_out, stats, {trace_out, trace_cap, ntrace_out}}
#define DENSE_OUT_STATE DenseOut{beta_out, niter_out, stats, {trace_out, trace_cap, ntrace_out}, {state_out, state_cap, nstate_out}}

static LassoPlan& plan_of(admm_hip_plan* plan) {
    PlanHandle* h = reinterpret_cast<PlanHandle*>(plan);
    ADMM_REQUIRE(h != nullptr && h->plan, "plan is NULL");
    return *h->plan;
}
static void plan_out_set(PlanHandle* h, admm_hip_plan** plan_out, int* nlambda_out) {
    *plan_out = reinterpret_cast<admm_hip_plan*>(h);
    if (nlambda_out) *nlambda_out = h->nlam;
}

// The tall-only penalties: the path arguments (PATH_SPEC) plus what each adds, p being the length of its per-column arrays.
static PathSpec group_spec(PathSpec s, int p, const int* group, const double* group_weight, int ngroups) {
    s.penalty = Penalty::GROUP; s.cols = p; s.group = group; s.group_weight = group_weight; s.ngroups = ngroups;
    return s;
}
static PathSpec sgl_spec(PathSpec s, int p, const int* group, const double* group_weight, int ngroups, const double* l1_weight, double mix) {
    s = group_spec(s, p, group, group_weight, ngroups);
    s.penalty = Penalty::SGL; s.l1_weight = l1_weight; s.sgl_mix = mix;
    return s;
}
static PathSpec box_spec(PathSpec s, int p, const double* lower, const double* upper, const double* penalty_factor) {
    s.penalty = Penalty::BOX; s.cols = p; s.lower = lower; s.upper = upper; s.penalty_factor = penalty_factor;
    return s;
}
static PathSpec mt_spec(PathSpec s, int p, int m, const double* row_weight) {
    s.penalty = Penalty::MULTITASK; s.cols = p; s.nresp = m; s.row_weight = row_weight;
    return s;
}
// ... and how a *_plan_create entry point hands its plan out
static void plan_create(const double* x, const double* y, int n, int p, int mem, const PathSpec& spec, admm_hip_plan** plan_out, int* nlambda_out) {
    ADMM_REQUIRE(plan_out != nullptr, "plan_out must not be NULL");
    plan_out_set(create_plan(x, y, n, p, mem, spec, 0), plan_out, nlambda_out);
}

extern "C" {

int admm_hip_lasso(const double* x, const double* y, int n, int p, int mem,
                   const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                   int standardize, int intercept, const admm_opts* opts,
                   double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { lasso_family(x, y, n, p, mem, PATH_SPEC(-1.0), 0, Shard(), PATH_OUT); });
}

int admm_hip_enet(const double* x, const double* y, int n, int p, int mem,
                  const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                  int standardize, int intercept, double alpha, const admm_opts* opts,
                  double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] {
        PathSpec spec = PATH_SPEC(alpha);
        spec.enet_only = true;
        lasso_family(x, y, n, p, mem, spec, 0, Shard(), PATH_OUT);
    });
}

int admm_hip_lasso_cv(const double* x, const double* y, int n, int p, int mem, const int* fold_id, int nfolds,
                      const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                      int standardize, int intercept, double alpha, const admm_opts* opts,
                      double* lambda_out, float* beta_out, int* niter_out,
                      double* cv_mean, double* cv_se, double* fold_mse, int* fold_niter, float* fold_beta,
                      int* idx_min, int* idx_1se, admm_stats* stats) {
    return guarded([&] {
        lasso_cv(x, y, n, p, mem, fold_id, nfolds, PATH_SPEC(alpha), PATH_OUT, CvOut{cv_mean, cv_se, fold_mse, fold_niter, fold_beta, idx_min, idx_1se});
    });
}

int admm_hip_lasso_multi(const double* x, const double* Y, int n, int p, int m, int mem,
                         const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                         int standardize, int intercept, double alpha, const admm_opts* opts,
                         double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { lasso_multi(x, Y, n, p, m, mem, PATH_SPEC(alpha), PATH_OUT); });
}

int admm_hip_parlasso(const double* x, const double* y, int n, int p, int mem,
                      const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                      int standardize, int intercept, int nthread, const admm_opts* opts,
                      double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { parlasso(x, y, n, p, mem, PATH_SPEC(-1.0), nthread, PATH_OUT); });
}

int admm_hip_lad(const double* x, const double* y, int n, int p, int mem, int intercept,
                 const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { lad(x, y, n, p, mem, intercept, opts, DENSE_OUT); });
}

int admm_hip_lad_traced(const double* x, const double* y, int n, int p, int mem, int intercept, const admm_opts* opts,
                        double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out) {
    return guarded([&] { lad(x, y, n, p, mem, intercept, opts, DENSE_OUT_TRACED); });
}

int admm_hip_lad_state(const double* x, const double* y, int n, int p, int mem, int intercept, const admm_opts* opts,
                       double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out,
                       double* state_out, long long state_cap, long long* nstate_out) {
    return guarded([&] { lad(x, y, n, p, mem, intercept, opts, DENSE_OUT_STATE); });
}

int admm_hip_quantreg(const double* x, const double* y, int n, int p, int mem, int intercept, const double* tau, int ntau,
                      const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { quantreg(x, y, n, p, mem, intercept, tau, ntau, opts, DENSE_OUT); });
}

int admm_hip_quantreg_state(const double* x, const double* y, int n, int p, int mem, int intercept, double tau, const admm_opts* opts,
                            double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out,
                            double* state_out, long long state_cap, long long* nstate_out) {
    return guarded([&] { quantreg(x, y, n, p, mem, intercept, &tau, 1, opts, DENSE_OUT_STATE); });
}

int admm_hip_huber(const double* x, const double* y, int n, int p, int mem, int intercept, const double* delta, const double* tau, int nfit,
                   const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { huber(x, y, n, p, mem, intercept, delta, tau, nfit, opts, DENSE_OUT); });
}

int admm_hip_huber_state(const double* x, const double* y, int n, int p, int mem, int intercept, double delta, double tau, const admm_opts* opts,
                         double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out,
                         double* state_out, long long state_cap, long long* nstate_out) {
    return guarded([&] { huber(x, y, n, p, mem, intercept, &delta, &tau, 1, opts, DENSE_OUT_STATE); });
}

int admm_hip_logit(const double* x, const double* y, int n, int p, int mem, int intercept, const admm_opts* opts, double* beta_out, int* niter_out,
                   admm_stats* stats) {
    return guarded([&] { logit(x, y, n, p, mem, intercept, opts, DENSE_OUT); });
}

int admm_hip_logit_state(const double* x, const double* y, int n, int p, int mem, int intercept, const admm_opts* opts, double* beta_out, int* niter_out,
                         admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out, double* state_out, long long state_cap,
                         long long* nstate_out) {
    return guarded([&] { logit(x, y, n, p, mem, intercept, opts, DENSE_OUT_STATE); });
}

int admm_hip_logit_multi(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const admm_opts* opts, double* beta_out,
                         int* niter_out, admm_stats* stats) {
    return guarded([&] { logit_multi(x, y, n, p, k, mem, intercept, opts, DENSE_OUT); });
}

int admm_hip_logit_ridge(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const double* lambda, int nlambda, const admm_opts* opts,
                         double* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { logit_ridge(x, y, n, p, k, mem, intercept, lambda, nlambda, opts, DENSE_OUT); });
}

int admm_hip_logit_ridge_state(const double* x, const double* y, int n, int p, int mem, int intercept, double lambda, const admm_opts* opts, double* beta_out,
                               int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out, double* state_out,
                               long long state_cap, long long* nstate_out) {
    return guarded([&] { logit_ridge(x, y, n, p, 1, mem, intercept, &lambda, 1, opts, DENSE_OUT_STATE); });
}

int admm_hip_logit_enet(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const double* lambda, const double* alpha, int ncell,
                        const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { logit_enet(x, y, n, p, k, mem, intercept, lambda, alpha, ncell, opts, DENSE_OUT); });
}

int admm_hip_logit_enet_lambda_max(const double* x, const double* y, int n, int p, int k, int mem, int intercept, double* out) {
    return guarded([&] { logit_enet_lambda_max(x, y, n, p, k, mem, intercept, out); });
}

int admm_hip_logit_enet_state(const double* x, const double* y, int n, int p, int mem, int intercept, double lambda, double alpha, const admm_opts* opts,
                              double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out,
                              double* state_out, long long state_cap, long long* nstate_out) {
    return guarded([&] { logit_enet(x, y, n, p, 1, mem, intercept, &lambda, &alpha, 1, opts, DENSE_OUT_STATE); });
}

int admm_hip_poisson(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const double* lambda, const double* alpha, int ncell,
                     const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { poisson(x, y, n, p, k, mem, intercept, lambda, alpha, ncell, opts, DENSE_OUT); });
}

int admm_hip_poisson_lambda_max(const double* x, const double* y, int n, int p, int k, int mem, int intercept, double* out) {
    return guarded([&] { poisson_lambda_max(x, y, n, p, k, mem, intercept, out); });
}

int admm_hip_poisson_state(const double* x, const double* y, int n, int p, int mem, int intercept, double lambda, double alpha, const admm_opts* opts,
                           double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out,
                           double* state_out, long long state_cap, long long* nstate_out) {
    return guarded([&] { poisson(x, y, n, p, 1, mem, intercept, &lambda, &alpha, 1, opts, DENSE_OUT_STATE); });
}

#define GLM_CV_OUT GlmCvOut{cv_mean, cv_se, fold_dev, fold_niter, fold_beta, idx_min, idx_1se}

int admm_hip_logit_enet_cv(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const int* fold_id, int nfolds, const double* lambda,
                           const double* alpha, int ncell, const admm_opts* opts, double* beta_out, int* niter_out, double* cv_mean, double* cv_se, double* fold_dev,
                           int* fold_niter, double* fold_beta, int* idx_min, int* idx_1se, admm_stats* stats) {
    return guarded([&] { glm_cv(false, x, y, n, p, k, mem, intercept, fold_id, nfolds, -2, lambda, alpha, ncell, opts, DENSE_OUT, GLM_CV_OUT); });
}

int admm_hip_poisson_cv(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const int* fold_id, int nfolds, const double* lambda,
                        const double* alpha, int ncell, const admm_opts* opts, double* beta_out, int* niter_out, double* cv_mean, double* cv_se, double* fold_dev,
                        int* fold_niter, double* fold_beta, int* idx_min, int* idx_1se, admm_stats* stats) {
    return guarded([&] { glm_cv(true, x, y, n, p, k, mem, intercept, fold_id, nfolds, -2, lambda, alpha, ncell, opts, DENSE_OUT, GLM_CV_OUT); });
}

int admm_hip_logit_enet_cv_state(const double* x, const double* y, int n, int p, int mem, int intercept, const int* fold_id, int nfolds, int fold, double lambda,
                                 double alpha, const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap,
                                 long long* ntrace_out, double* state_out, long long state_cap, long long* nstate_out) {
    return guarded([&] {
        ADMM_REQUIRE(fold >= -1, "fold must be within [-1, nfolds)");
        glm_cv(false, x, y, n, p, 1, mem, intercept, fold_id, nfolds, fold, &lambda, &alpha, 1, opts, DENSE_OUT_STATE, GlmCvOut{});
    });
}

int admm_hip_poisson_cv_state(const double* x, const double* y, int n, int p, int mem, int intercept, const int* fold_id, int nfolds, int fold, double lambda,
                              double alpha, const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap,
                              long long* ntrace_out, double* state_out, long long state_cap, long long* nstate_out) {
    return guarded([&] {
        ADMM_REQUIRE(fold >= -1, "fold must be within [-1, nfolds)");
        glm_cv(true, x, y, n, p, 1, mem, intercept, fold_id, nfolds, fold, &lambda, &alpha, 1, opts, DENSE_OUT_STATE, GlmCvOut{});
    });
}

int admm_hip_bp(const double* x, const double* y, int n, int p, int mem,
                const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { bp(x, y, n, p, mem, opts, DENSE_OUT); });
}

int admm_hip_bp_traced(const double* x, const double* y, int n, int p, int mem, const admm_opts* opts,
                       double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out) {
    return guarded([&] { bp(x, y, n, p, mem, opts, DENSE_OUT_TRACED); });
}

int admm_hip_bp_state(const double* x, const double* y, int n, int p, int mem, const admm_opts* opts,
                      double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out,
                      double* state_out, long long state_cap, long long* nstate_out) {
    return guarded([&] { bp(x, y, n, p, mem, opts, DENSE_OUT_STATE); });
}

int admm_hip_dantzig_traced(const double* x, const double* y, int n, int p, int mem,
                            const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                            int standardize, int intercept, const admm_opts* opts,
                            double* lambda_out, double* beta_out, int* niter_out, admm_stats* stats,
                            double* trace_out, long long trace_cap, long long* ntrace_out) {
    return guarded([&] {
        dantzig(x, y, n, p, mem, PATH_SPEC(-1.0), PathOutT<double>{lambda_out, beta_out, niter_out, stats}, TraceOut{trace_out, trace_cap, ntrace_out});
    });
}

int admm_hip_dantzig(const double* x, const double* y, int n, int p, int mem,
                     const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                     int standardize, int intercept, const admm_opts* opts,
                     double* lambda_out, double* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { dantzig(x, y, n, p, mem, PATH_SPEC(-1.0), PathOutT<double>{lambda_out, beta_out, niter_out, stats}, TraceOut{}); });
}

int admm_hip_parbp(const double* x, const double* y, int n, int p, int mem, int nthread, const admm_opts* opts,
                   double* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { parbp(x, y, n, p, mem, nthread, opts, DenseOut{beta_out, niter_out, stats}); });
}

int admm_hip_parbp_traced(const double* x, const double* y, int n, int p, int mem, int nthread, const admm_opts* opts,
                          double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out) {
    return guarded([&] { parbp(x, y, n, p, mem, nthread, opts, DenseOut{beta_out, niter_out, stats, {trace_out, trace_cap, ntrace_out}}); });
}

int admm_hip_parbp_dist(const double* x_cols, const double* y, int n, int p_local, long long p_total, long long col_offset, int mem, int nthread,
                        const admm_opts* opts, double* beta_local_out, int* niter_out, admm_stats* stats) {
    return guarded([&] {
        parbp_dist(x_cols, y, n, p_local, p_total, col_offset, mem, nthread, opts, DenseOut{beta_local_out, niter_out, stats});
    });
}

int admm_hip_lasso_plan_create(const double* x, const double* y, int n, int p, int mem,
                               const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                               int standardize, int intercept, double alpha, int nthread, const admm_opts* opts,
                               admm_hip_plan** plan_out, int* nlambda_out) {
    return guarded([&] {
        ADMM_REQUIRE(plan_out != nullptr, "plan_out must not be NULL");
        // the reference has no parallel elastic net (R/40_admm_enet.R:50-64 always calls admm_enet): refuse instead of silently running a consensus Lasso
        ADMM_REQUIRE(!(alpha >= 0.0 && nthread > 1), "the consensus solver has no elastic-net variant: alpha >= 0 cannot be combined with nthread > 1");
        plan_out_set(create_plan(x, y, n, p, mem, PATH_SPEC(alpha), nthread > 1 ? nthread : 0), plan_out, nlambda_out);
    });
}

int admm_hip_lasso_plan_create_dist(const double* x_local, const double* y_local, int n_local, long long n_total, int p, int mem,
                                    const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                    int standardize, int intercept, int nthread, const admm_opts* opts,
                                    admm_hip_plan** plan_out, int* nlambda_out) {
    return guarded([&] {
        ADMM_REQUIRE(plan_out != nullptr, "plan_out must not be NULL");
        plan_out_set(create_plan(x_local, y_local, n_local, p, mem, PATH_SPEC(-1.0), nthread, Shard::rows(n_total)), plan_out, nlambda_out);
    });
}

int admm_hip_lasso_dist(const double* x_local, const double* y_local, int n_local, long long n_total, int p, int mem,
                        const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                        int standardize, int intercept, double alpha, const admm_opts* opts,
                        double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { lasso_family(x_local, y_local, n_local, p, mem, PATH_SPEC(alpha), 0, Shard::rows(n_total), PATH_OUT); });
}

int admm_hip_parlasso_dist(const double* x_local, const double* y_local, int n_local, long long n_total, int p, int mem,
                           const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                           int standardize, int intercept, int nthread, const admm_opts* opts,
                           double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { lasso_family(x_local, y_local, n_local, p, mem, PATH_SPEC(-1.0), nthread, Shard::rows(n_total), PATH_OUT); });
}

int admm_hip_lasso_dist_cols(const double* x_cols, const double* y, int n, int p_local, long long p_total, long long col_offset, int mem,
                             const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                             int standardize, int intercept, double alpha, const admm_opts* opts,
                             double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { lasso_family(x_cols, y, n, p_local, mem, PATH_SPEC(alpha), 0, Shard::cols(p_total, col_offset), PATH_OUT); });
}

int admm_hip_lasso_plan_create_dist_cols(const double* x_cols, const double* y, int n, int p_local, long long p_total, long long col_offset, int mem,
                                         const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                         int standardize, int intercept, double alpha, const admm_opts* opts,
                                         admm_hip_plan** plan_out, int* nlambda_out) {
    return guarded([&] {
        ADMM_REQUIRE(plan_out != nullptr, "plan_out must not be NULL");
        plan_out_set(create_plan(x_cols, y, n, p_local, mem, PATH_SPEC(alpha), 0, Shard::cols(p_total, col_offset)), plan_out, nlambda_out);
    });
}

// admm_hip_grplasso: the Lasso's path arguments plus the grouping of the columns
int admm_hip_grplasso(const double* x, const double* y, int n, int p, int mem,
                      const int* group, const double* group_weight, int ngroups,
                      const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                      int standardize, int intercept, const admm_opts* opts,
                      double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { lasso_family(x, y, n, p, mem, group_spec(PATH_SPEC(-1.0), p, group, group_weight, ngroups), 0, Shard(), PATH_OUT); });
}

int admm_hip_grplasso_plan_create(const double* x, const double* y, int n, int p, int mem,
                                  const int* group, const double* group_weight, int ngroups,
                                  const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                  int standardize, int intercept, const admm_opts* opts,
                                  admm_hip_plan** plan_out, int* nlambda_out) {
    return guarded([&] { plan_create(x, y, n, p, mem, group_spec(PATH_SPEC(-1.0), p, group, group_weight, ngroups), plan_out, nlambda_out); });
}

// admm_hip_sgl: the group lasso's arguments plus the l1 weight of every column and the mixing parameter
int admm_hip_sgl(const double* x, const double* y, int n, int p, int mem,
                 const int* group, const double* group_weight, int ngroups, const double* l1_weight, double alpha,
                 const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                 int standardize, int intercept, const admm_opts* opts,
                 double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { lasso_family(x, y, n, p, mem, sgl_spec(PATH_SPEC(-1.0), p, group, group_weight, ngroups, l1_weight, alpha), 0, Shard(), PATH_OUT); });
}

int admm_hip_sgl_plan_create(const double* x, const double* y, int n, int p, int mem,
                             const int* group, const double* group_weight, int ngroups, const double* l1_weight, double alpha,
                             const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                             int standardize, int intercept, const admm_opts* opts,
                             admm_hip_plan** plan_out, int* nlambda_out) {
    return guarded([&] { plan_create(x, y, n, p, mem, sgl_spec(PATH_SPEC(-1.0), p, group, group_weight, ngroups, l1_weight, alpha), plan_out, nlambda_out); });
}

// admm_hip_boxenet: the elastic net's path arguments (alpha < 0: the Lasso prox) plus the box and the penalty factors
int admm_hip_boxenet(const double* x, const double* y, int n, int p, int mem,
                     const double* lower, const double* upper, const double* penalty_factor, double alpha,
                     const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                     int standardize, int intercept, const admm_opts* opts,
                     double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { lasso_family(x, y, n, p, mem, box_spec(PATH_SPEC(alpha), p, lower, upper, penalty_factor), 0, Shard(), PATH_OUT); });
}

int admm_hip_boxenet_plan_create(const double* x, const double* y, int n, int p, int mem,
                                 const double* lower, const double* upper, const double* penalty_factor, double alpha,
                                 const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                 int standardize, int intercept, const admm_opts* opts,
                                 admm_hip_plan** plan_out, int* nlambda_out) {
    return guarded([&] { plan_create(x, y, n, p, mem, box_spec(PATH_SPEC(alpha), p, lower, upper, penalty_factor), plan_out, nlambda_out); });
}

// admm_hip_mtlasso: the Lasso's path arguments plus the number of responses and the row weights
int admm_hip_mtlasso(const double* x, const double* Y, int n, int p, int m, int mem,
                     const double* row_weight,
                     const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                     int standardize, int intercept, const admm_opts* opts,
                     double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { lasso_family(x, Y, n, p, mem, mt_spec(PATH_SPEC(-1.0), p, m, row_weight), 0, Shard(), PATH_OUT); });
}

int admm_hip_mtlasso_plan_create(const double* x, const double* Y, int n, int p, int m, int mem,
                                 const double* row_weight,
                                 const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                 int standardize, int intercept, const admm_opts* opts,
                                 admm_hip_plan** plan_out, int* nlambda_out) {
    return guarded([&] { plan_create(x, Y, n, p, mem, mt_spec(PATH_SPEC(-1.0), p, m, row_weight), plan_out, nlambda_out); });
}

int admm_hip_options_default(admm_hip_options* o) {
    return guarded([&] {
        ADMM_REQUIRE(o != nullptr, "options must not be NULL");
        std::memset(o, 0, sizeof(*o));
        o->struct_size = (int)sizeof(*o);
    });
}
int admm_hip_options_reset(void) { return guarded([&] { thread_options() = ThreadOptions(); }); }
int admm_hip_option_set(const char* name, const char* value) {
    return guarded([&] {
        ADMM_REQUIRE(name != nullptr && name[0] != 0, "option name must not be empty");
        Opt id;
        ADMM_REQUIRE(opt_find(name, &id), std::string("unknown option '") + name + "' (INTEGRATION.md section 5 lists the names)");
        opt_set_thread(id, value);
    });
}
const char* admm_hip_option_get(const char* name) {
    Opt id;
    return name && opt_find(name, &id) ? opt_text(id) : nullptr;
}
int admm_hip_options_set(const admm_hip_options* o) {
    return guarded([&] {
        ThreadOptions n;                          // built aside: a refused field leaves the thread's settings as they were
        if (o == nullptr) { thread_options() = n; return; }
        ADMM_REQUIRE(o->struct_size >= (int)(2 * sizeof(int)) && o->struct_size <= (int)sizeof(admm_hip_options), "options: bad struct_size");
        admm_hip_options v;
        std::memset(&v, 0, sizeof(v));
        std::memcpy(&v, o, (size_t)o->struct_size);
        auto set = [&](Opt k, const char* val) { opt_parse(k, val, &n.v[(int)k]); n.has[(int)k] = true; };
        auto num = [&](Opt k, int val) { set(k, std::to_string(val).c_str()); };
        if (v.gram_backend == 1) set(Opt::GRAM, "rocblas");
        if (v.gram_split) { ADMM_REQUIRE(v.gram_split >= 1 && v.gram_split <= 3, "options: gram_split"); set(Opt::GRAM_SPLIT, v.gram_split == 1 ? "0" : (v.gram_split == 2 ? "f16x2" : "bf16x3")); }
        if (v.factor_backend == 1) set(Opt::FACTOR, "rocsolver");
        if (v.inverse_precision) { ADMM_REQUIRE(v.inverse_precision == 1 || v.inverse_precision == 2, "options: inverse_precision"); set(Opt::INVERSE, v.inverse_precision == 1 ? "f32" : "f64"); }
        if (v.tall_xupdate) { ADMM_REQUIRE(v.tall_xupdate == 1 || v.tall_xupdate == 2, "options: tall_xupdate"); set(Opt::XUPDATE, v.tall_xupdate == 1 ? "gemv" : "sym"); }
        if (v.tall_refine) set(Opt::REFINE, "1");
        if (v.consensus_two_pass) set(Opt::PAR_ONEPASS, "0");
        if (v.consensus_unfused >= 1) set(Opt::PAR_FUSE_PZ, "0");
        if (v.consensus_unfused >= 2) set(Opt::PAR_BATCH, "0");
        if (v.bp_two_pass) set(Opt::BP_ONEPASS, "0");
        if (v.lad_no_hat) set(Opt::LAD_HAT, "0");
        if (v.wide_no_persist == 1) set(Opt::WIDE_PERSIST, "0");
        if (v.wide_no_persist == 2) set(Opt::WIDE_PERSIST_COLS, "0");
        if (v.wide_unfused) set(Opt::WIDE_FUSE, "0");
        if (v.wide_gram_sprad) set(Opt::WIDE_SPRAD, "gram");
        if (v.sharing_bp_direct) set(Opt::SBP_GRAM, "0");
        if (v.cv_downdate) set(Opt::CV_DOWNDATE, v.cv_downdate == 1 ? "1" : "0");
        if (v.peer_exchange) set(Opt::PEER_FUSED, v.peer_exchange == 1 ? "2" : "0");
        if (v.batch_iters > 0) num(Opt::BATCH_ITERS, v.batch_iters);
        if (v.profile_stride > 0) num(Opt::PROFILE_STRIDE, v.profile_stride);
        if (v.pool_mb) num(Opt::POOL_MB, v.pool_mb < 0 ? 0 : v.pool_mb);
        if (v.lad_two_pass) set(Opt::LAD_ONEPASS, "0");
        if (v.par_devices) {
            ADMM_REQUIRE(v.par_devices >= -1 && v.par_devices <= 64, "options: par_devices");
            std::string l;
            for (int d = 0; d < v.par_devices; ++d) l += (d ? "," : "") + std::to_string(d);
            set(Opt::PAR_DEVICES, v.par_devices == -1 ? "all" : l.c_str());
        }
        if (v.screen) {
            ADMM_REQUIRE(v.screen >= 1 && v.screen <= 3, "options: screen");
            set(Opt::WIDE_SCREEN, v.screen == 1 ? "16" : (v.screen == 3 ? "8" : "0"));
            set(Opt::SBP_SCREEN, v.screen == 2 ? "0" : "1");
        }
        thread_options() = n;
    });
}
int admm_hip_comm_unique_id(void* id_out) {
    return guarded([&] { ADMM_REQUIRE(id_out != nullptr, "id_out must not be NULL"); comm_unique_id(id_out); });
}
int admm_hip_comm_init(int nranks, int rank, const void* id) {
    return guarded([&] { ADMM_REQUIRE(id != nullptr, "id must not be NULL"); require_device(); comm_init(nranks, rank, id); });
}
int admm_hip_comm_finalize(void) {
    return guarded([&] { comm_finalize(); });
}
int admm_hip_comm_info(int* nranks_out, int* rank_out, int* backend_out) {
    return guarded([&] {
        const CommInfo ci = comm_info_live();
        if (nranks_out) *nranks_out = ci.active ? ci.nranks : 1;
        if (rank_out) *rank_out = ci.active ? ci.rank : 0;
        if (backend_out) *backend_out = ci.active ? ci.backend : 0;
    });
}
int admm_hip_comm_peer_prepare(int nranks, void* handle_out) {
    return guarded([&] { ADMM_REQUIRE(handle_out != nullptr, "handle_out must not be NULL"); require_device(); comm_peer_prepare(nranks, handle_out); });
}
int admm_hip_comm_init_peer(int nranks, int rank, const void* handles) {
    return guarded([&] { ADMM_REQUIRE(handles != nullptr, "handles must not be NULL"); require_device(); comm_init_peer(nranks, rank, handles); });
}
int admm_hip_comm_init_shm(int nranks, int rank, const char* name, unsigned long long token) {
    return guarded([&] { require_device(); comm_init_shm(nranks, rank, name, token); });
}
int admm_hip_comm_test_allreduce(float* fbuf, long long nf, double* dbuf, long long nd, int mem) {
    return guarded([&] {
        ADMM_REQUIRE(nf >= 0 && nd >= 0 && (nf == 0 || fbuf) && (nd == 0 || dbuf), "bad arguments");
        ADMM_REQUIRE(comm_info().active, "no communicator");
        require_device();
        Stream st;
        DevBuf<float> df; DevBuf<double> dd;
        float* pf = fbuf; double* pd = dbuf;
        if (mem == ADMM_MEM_HOST) {
            df.alloc((size_t)nf); dd.alloc((size_t)nd);
            if (nf) ADMM_HIP_CHECK(hipMemcpyAsync(df.get(), fbuf, (size_t)nf * sizeof(float), hipMemcpyHostToDevice, st.s));
            if (nd) ADMM_HIP_CHECK(hipMemcpyAsync(dd.get(), dbuf, (size_t)nd * sizeof(double), hipMemcpyHostToDevice, st.s));
            pf = df.get(); pd = dd.get();
        }
        if (nf && nd) allreduce_sum_f32_f64(pf, (size_t)nf, pd, (size_t)nd, st.s);
        else if (nf) allreduce_sum_f32(pf, (size_t)nf, st.s);
        else if (nd) allreduce_sum_f64(pd, (size_t)nd, st.s);
        if (mem == ADMM_MEM_HOST) {
            if (nf) ADMM_HIP_CHECK(hipMemcpyAsync(fbuf, pf, (size_t)nf * sizeof(float), hipMemcpyDeviceToHost, st.s));
            if (nd) ADMM_HIP_CHECK(hipMemcpyAsync(dbuf, pd, (size_t)nd * sizeof(double), hipMemcpyDeviceToHost, st.s));
        }
        st.sync();
        comm_check();
    });
}

int admm_hip_comm_test_reduce_scatter(const float* send, long long count, float* recv) {
    return guarded([&] {
        ADMM_REQUIRE(count > 0 && count % 4 == 0 && send && recv, "bad arguments (count must be a positive multiple of 4)");
        require_device();
        const CommInfo ci = comm_info();
        const size_t nr = (size_t)(ci.active ? ci.nranks : 1);
        Stream st;
        DevBuf<float> ds(nr * (size_t)count), dr((size_t)count);
        ADMM_HIP_CHECK(hipMemcpyAsync(ds.get(), send, nr * (size_t)count * sizeof(float), hipMemcpyHostToDevice, st.s));
        reduce_scatter_sum_f32(ds.get(), dr.get(), (size_t)count, st.s);
        ADMM_HIP_CHECK(hipMemcpyAsync(recv, dr.get(), (size_t)count * sizeof(float), hipMemcpyDeviceToHost, st.s));
        st.sync();
        comm_check();
    });
}

int admm_hip_lasso_plan_run(admm_hip_plan* plan, double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats) {
    return guarded([&] { run_plan(reinterpret_cast<PlanHandle*>(plan), PATH_OUT, 0.0); });
}

int admm_hip_lasso_plan_destroy(admm_hip_plan* plan) {
    return guarded([&] { delete reinterpret_cast<PlanHandle*>(plan); });
}

int admm_hip_lasso_plan_trace_enable(admm_hip_plan* plan, long long capacity_records) {
    return guarded([&] {
        ADMM_REQUIRE(capacity_records > 0 && capacity_records <= (1ll << 26), "trace capacity must be within [1, 2^26] records");
        plan_of(plan).enable_trace(capacity_records);
    });
}

int admm_hip_lasso_plan_trace_read(admm_hip_plan* plan, double* out, long long cap_records, long long* nrecords_out) {
    return guarded([&] {
        ADMM_REQUIRE(out != nullptr && nrecords_out != nullptr && cap_records >= 0, "bad trace output arguments");
        *nrecords_out = plan_of(plan).read_trace(out, cap_records);
    });
}

int admm_hip_lasso_plan_state_enable(admm_hip_plan* plan, long long capacity_records) {
    return guarded([&] {
        ADMM_REQUIRE(capacity_records > 0 && capacity_records <= (1ll << 22), "state capacity must be within [1, 2^22] records");
        plan_of(plan).enable_state(capacity_records);
    });
}

int admm_hip_lasso_plan_state_read(admm_hip_plan* plan, float* out, long long cap_records, long long* nrecords_out, long long* record_floats_out) {
    return guarded([&] {
        ADMM_REQUIRE(nrecords_out != nullptr && cap_records >= 0 && (out != nullptr || cap_records == 0), "bad state output arguments");
        *nrecords_out = plan_of(plan).read_state(out, cap_records, record_floats_out);
    });
}

int admm_hip_lasso_plan_data_read(admm_hip_plan* plan, float* x_out, long long ld, float* y_out) {
    return guarded([&] {
        plan_of(plan).read_data(x_out, ld, y_out);
    });
}

int admm_hip_lasso_plan_system_read(admm_hip_plan* plan, float* out, long long ld) {
    return guarded([&] {
        plan_of(plan).read_system(out, ld);
    });
}

int admm_hip_last_parallel_layout(int* nranks, int* devices, int cap) {
    return guarded([&] {
        ADMM_REQUIRE(nranks != nullptr && cap >= 0 && (cap == 0 || devices != nullptr), "bad layout arguments");
        *nranks = (int)last_layout().size();
        for (int r = 0; r < std::min(cap, *nranks); ++r) devices[r] = last_layout()[r];
    });
}

int admm_hip_parallel_assign(int nblocks, const char* par_devices, int device_count, int* nranks, int* devices, int cap) {
    return guarded([&] {
        ADMM_REQUIRE(nblocks >= 1 && device_count >= 0, "nblocks must be >= 1 and device_count >= 0");
        ADMM_REQUIRE(nranks != nullptr && cap >= 0 && (cap == 0 || devices != nullptr), "bad layout arguments");
        const std::vector<int> lay = par_layout(nblocks, parse_par_devices(par_devices, device_count));
        *nranks = lay.empty() ? 1 : (int)lay.size();
        for (int r = 0; r < std::min(cap, (int)lay.size()); ++r) devices[r] = lay[r];
    });
}

const char* admm_hip_last_error(void) { return last_error_ref().c_str(); }
const char* admm_hip_version(void) { return "admm_hip 0.3 (gfx950)"; }
int admm_hip_trim_memory(void) {
    admm::pool_trim();
    return ADMM_OK;
}

int admm_hip_device_count(void) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}
int admm_hip_set_device(int device) {
    return guarded([&] { ADMM_HIP_CHECK(hipSetDevice(device)); });
}
int admm_hip_device_synchronize(void) {
    return guarded([&] { ADMM_HIP_CHECK(hipDeviceSynchronize()); });
}

// Host-only helper used by the CPU test-suite: runs the Lanczos host logic (lanczos.hip) against a
// dense symmetric matrix held in host memory.  Not part of any solver path.
int admm_hip_host_lanczos(const float* A, int n, float* eig_out, int* nmatop_out) {
    return guarded([&] {
        ADMM_REQUIRE(A && eig_out && n >= 3, "bad arguments");
        auto op = [&](const float* v, float* w) {
            for (int i = 0; i < n; ++i) w[i] = 0.f;
            for (int j = 0; j < n; ++j) {
                const float vj = v[j];
                const float* col = A + (size_t)j * n;
                for (int i = 0; i < n; ++i) w[i] += col[i] * vj;
            }
        };
        *eig_out = lanczos_largest_f32(op, n, nmatop_out);
    });
}

// Host-only helper used by the CPU test-suite: lambda_0 of the sparse-group lasso's automatic grid (sgl_host.h) from a given X'y.
int admm_hip_host_sgl_lambda0(const float* xy, int p, const int* group, const double* group_weight, int ngroups,
                              const double* l1_weight, double alpha, float* out) {
    return guarded([&] {
        ADMM_REQUIRE(xy && out && p > 0, "bad arguments");
        const PathSpec s = sgl_spec(PathSpec(), p, group, group_weight, ngroups, l1_weight, alpha);
        s.check_sgl_args(p);
        const std::vector<int> start = s.group_starts();
        std::vector<double> l1, wg;
        sgl_prepare(alpha, l1_weight, group_weight, start, l1, wg);
        *out = sgl_lambda0(xy, start, l1, wg);
    });
}

// Host-only helper used by the CPU test-suite: lambda_0 of the box-constrained elastic net's automatic grid (box_host.h) from a given
// X'y and bounds already in the solver's units.
int admm_hip_host_box_lambda0(const float* xy, int p, const float* lower_std, const float* upper_std, const double* penalty_factor,
                              double alpha, float* out) {
    return guarded([&] {
        ADMM_REQUIRE(xy && out && p > 0, "bad arguments");
        PathSpec s = box_spec(PathSpec(), p, nullptr, nullptr, penalty_factor);
        s.alpha = alpha;
        s.check_box_args(p);
        for (int j = 0; j < p; ++j)
            ADMM_REQUIRE((!lower_std || lower_std[j] <= 0.f) && (!upper_std || upper_std[j] >= 0.f), "the box must hold zero");
        float l0 = box_lambda0(xy, p, lower_std, upper_std, penalty_factor);
        if (s.enet()) l0 = box_lambda0_enet(l0, alpha);
        *out = l0;
    });
}

int admm_hip_test_symv(const float* A, int p, const float* v0, const float* v1, float* y0, float* y1) {
    return guarded([&] {
        ADMM_REQUIRE(A && v0 && v1 && y0 && y1 && p > 0, "bad arguments");
        test_symv(A, p, v0, v1, y0, y1);
    });
}

int admm_hip_test_symv_multi(const float* A, int p, const float* V, int nr, int rhs_per_pass, float* Yout) {
    return guarded([&] {
        ADMM_REQUIRE(A && V && Yout && p > 0 && nr >= 1 && nr <= 64, "bad arguments");
        test_symv_multi(A, p, V, nr, rhs_per_pass, Yout);
    });
}

// The four hooks of the x-update's variants refuse what they cannot run before they look for a device (tests/test_symv_plan_host.py).
int admm_hip_test_symv_plan(int p, int cus, int part, int nparts, int* sched_out, long long* info_out, int* tiles_out, int tile_capacity) {
    return guarded([&] {
        ADMM_REQUIRE(sched_out && info_out && tiles_out, "symv plan hook: sched_out, info_out and tiles_out must not be NULL");
        ADMM_REQUIRE(p >= 1 && p <= kSymvHookMaxP && cus <= 65536 && nparts >= 1 && nparts <= 64 && part >= 0 && part < nparts && tile_capacity >= 1,
                     "symv plan hook: p in 1 .. 32768, cus <= 65536, nparts in 1 .. 64, part in 0 .. nparts - 1, tile_capacity >= 1");
        test_symv_plan(p, cus, part, nparts, sched_out, info_out, tiles_out, tile_capacity);
    });
}

int admm_hip_test_symv_ex(const float* A, int p, const float* v0, const float* v1, int variant, int part, int nparts, float* y0, float* y1,
                          int* sched_out) {
    return guarded([&] {
        ADMM_REQUIRE(A && v0 && v1 && y0 && y1 && sched_out, "symv_ex hook: A, v0, v1, y0, y1 and sched_out must not be NULL");
        ADMM_REQUIRE(p >= 1 && p <= kSymvHookMaxP && variant >= 0 && variant <= 2 && nparts >= 1 && nparts <= 64 && part >= 0 && part < nparts,
                     "symv_ex hook: p in 1 .. 32768, variant in 0 .. 2, nparts in 1 .. 64, part in 0 .. nparts - 1");
        test_symv_ex(A, p, v0, v1, variant, part, nparts, y0, y1, sched_out);
    });
}

int admm_hip_test_symv_one(const float* A, int p, const float* v0, const float* v1, int gate, int nt, unsigned int fill, float* y,
                           float* dot_out, float* axp_out, long long plane_capacity, long long* info_out, int* sched_out) {
    return guarded([&] {
        ADMM_REQUIRE(A && v0 && v1 && y && info_out && sched_out, "symv_one hook: A, v0, v1, y, info_out and sched_out must not be NULL");
        ADMM_REQUIRE((dot_out == nullptr) == (axp_out == nullptr), "symv_one hook: dot_out and axp_out are given together or not at all");
        ADMM_REQUIRE(p >= 1 && p <= kSymvHookMaxP && gate >= 0 && gate <= 3 && (nt == 0 || nt == 1) && plane_capacity >= 0,
                     "symv_one hook: p in 1 .. 32768, gate in 0 .. 3, nt 0 or 1, plane_capacity >= 0");
        test_symv_one(A, p, v0, v1, gate, nt, fill, y, dot_out, axp_out, plane_capacity, info_out, sched_out);
    });
}

int admm_hip_test_symv_pack_host(const unsigned int* bits, int nchunks, int* base_io, unsigned int* stream_out, unsigned int* esc_out, int esc_cap,
                                 long long* nesc_out, unsigned int* decoded_out) {
    return guarded([&] {
        ADMM_REQUIRE(bits && base_io && stream_out && nesc_out && decoded_out && (esc_out || esc_cap == 0),
                     "symv_pack_host hook: bits, base_io, stream_out, nesc_out and decoded_out must not be NULL, esc_out only with esc_cap 0");
        ADMM_REQUIRE(nchunks >= 1 && nchunks <= 4096 && *base_io <= 127 && esc_cap >= 0, "symv_pack_host hook: nchunks in 1 .. 4096, base <= 127, esc_cap >= 0");
        test_symv_pack_host(bits, nchunks, base_io, stream_out, esc_out, esc_cap, nesc_out, decoded_out);
    });
}

int admm_hip_test_symv_packed(const float* A, int p, const float* v0, const float* v1, int gate, int nt, unsigned int fill, int esc_cap, float* y,
                              float* dot_out, float* axp_out, long long plane_capacity, long long* info_out, int* sched_out) {
    return guarded([&] {
        ADMM_REQUIRE(A && v0 && v1 && y && info_out && sched_out, "symv_packed hook: A, v0, v1, y, info_out and sched_out must not be NULL");
        ADMM_REQUIRE((dot_out == nullptr) == (axp_out == nullptr), "symv_packed hook: dot_out and axp_out are given together or not at all");
        ADMM_REQUIRE(p >= 1 && p <= kSymvHookMaxP && gate >= 0 && gate <= 2 && (nt == 0 || nt == 1) && esc_cap >= 0 && esc_cap <= 4096 && plane_capacity >= 0,
                     "symv_packed hook: p in 1 .. 32768, gate in 0 .. 2, nt 0 or 1, esc_cap in 0 .. 4096, plane_capacity >= 0");
        test_symv_packed(A, p, v0, v1, gate, nt, fill, esc_cap, y, dot_out, axp_out, plane_capacity, info_out, sched_out);
    });
}

int admm_hip_test_symv_packed_time(const float* A, int p, const float* v0, int reps, float* us_out, long long* info_out) {
    return guarded([&] {
        ADMM_REQUIRE(A && v0 && us_out && info_out, "symv_packed_time hook: A, v0, us_out and info_out must not be NULL");
        ADMM_REQUIRE(p >= 1 && p <= kSymvHookMaxP && reps >= 2 && reps <= 1000 && reps % 2 == 0, "symv_packed_time hook: p in 1 .. 32768, reps even, 2 .. 1000");
        test_symv_packed_time(A, p, v0, reps, us_out, info_out);
    });
}

int admm_hip_test_symv_multi_ex(const float* A, int p, const float* V, int nr, int rhs_per_pass, int nt, int finish, float* Yout, int* sched_out) {
    return guarded([&] {
        ADMM_REQUIRE(A && V && Yout && sched_out, "symv_multi_ex hook: A, V, Yout and sched_out must not be NULL");
        ADMM_REQUIRE(p >= 1 && p <= kSymvHookMaxP && nr >= 1 && nr <= 64 && test_symv_rhs_built(rhs_per_pass) && (nt == 0 || nt == 1) && (finish == 0 || finish == 1),
                     "symv_multi_ex hook: p in 1 .. 32768, nr in 1 .. 64, rhs_per_pass one of the built widths (2, 4, 8, 12), nt and finish 0 or 1");
        test_symv_multi_ex(A, p, V, nr, rhs_per_pass, nt, finish, Yout, sched_out);
    });
}

int admm_hip_test_symv_f64acc(const float* A, int p, const float* v0, const float* v1, double* y0, double* y1, int* sched_out) {
    return guarded([&] {
        ADMM_REQUIRE(A && v0 && v1 && y0 && y1 && sched_out, "symv_f64acc hook: A, v0, v1, y0, y1 and sched_out must not be NULL");
        ADMM_REQUIRE(p >= 1 && p <= kSymvHookMaxP, "symv_f64acc hook: p in 1 .. 32768");
        test_symv_f64acc(A, p, v0, v1, y0, y1, sched_out);
    });
}

int admm_hip_test_tall_early_exits(long long* count) {
    return guarded([&] {
        ADMM_REQUIRE(count != nullptr, "bad arguments");
        *count = tall_last_early_exits();
    });
}

int admm_hip_test_tall_pack_info(long long* info_out) {
    return guarded([&] {
        ADMM_REQUIRE(info_out != nullptr, "bad arguments");
        tall_last_pack_info(info_out);
    });
}

int admm_hip_test_tall_gate(const double* ctl_d, const int* ctl_i, const double* compact, int nwg, int maxit, int nlam, double* sums_out, int* answer_out) {
    return guarded([&] {
        ADMM_REQUIRE(ctl_d && ctl_i && compact && sums_out && answer_out, "tall_gate hook: no argument may be NULL");
        ADMM_REQUIRE(nwg >= 1 && nwg <= kTallGateHookMaxNwg && maxit >= 1 && nlam >= 1, "tall_gate hook: nwg in 1 .. 65536, maxit and nlam >= 1");
        require_device();
        test_tall_gate(ctl_d, ctl_i, compact, nwg, maxit, nlam, sums_out, answer_out);
    });
}

int admm_hip_test_tall_norms(const double* rows, int nwg, double* sums_out) {
    return guarded([&] {
        ADMM_REQUIRE(rows && sums_out, "tall_norms hook: rows and sums_out must not be NULL");
        ADMM_REQUIRE(nwg >= 1 && nwg <= kTallGateHookMaxNwg, "tall_norms hook: nwg in 1 .. 65536");
        require_device();
        test_tall_norms(rows, nwg, sums_out);
    });
}

int admm_hip_test_logit_prox(const double* v, long long m, double t, double* out) {
    return guarded([&] {
        ADMM_REQUIRE(v && out && m > 0 && t > 0.0 && std::isfinite(t), "logit prox hook: v and out must not be NULL, m > 0, t positive and finite");
        require_device();
        test_logit_prox(v, m, t, out);
    });
}

int admm_hip_test_poisson_prox(const double* v, const double* y, long long m, double t, double* out) {
    return guarded([&] {
        ADMM_REQUIRE(v && y && out && m > 0 && t > 0.0 && std::isfinite(t), "poisson prox hook: v, y and out must not be NULL, m > 0, t positive and finite");
        for (long long i = 0; i < m; ++i) ADMM_REQUIRE(std::isfinite(v[i]) && std::isfinite(y[i]) && y[i] >= 0.0, "poisson prox hook: v finite, y finite and non-negative");
        require_device();
        test_poisson_prox(v, y, m, t, out);
    });
}

int admm_hip_test_gram(const void* A, int rows, int cols, int atA, int is_double, void* G) {
    return guarded([&] {
        ADMM_REQUIRE(A && G && rows > 0 && cols > 0, "bad arguments");
        if (is_double) test_gram<double>(static_cast<const double*>(A), rows, cols, atA != 0, static_cast<double*>(G));
        else test_gram<float>(static_cast<const float*>(A), rows, cols, atA != 0, static_cast<float*>(G));
    });
}

int admm_hip_test_gemv_t(const void* A, int rows, int cols, int is_double, const void* v, void* y) {
    return guarded([&] {
        ADMM_REQUIRE(A && v && y && rows > 0 && cols > 0, "bad arguments");
        if (is_double) test_gemv_t<double>(static_cast<const double*>(A), rows, cols, static_cast<const double*>(v), static_cast<double*>(y));
        else test_gemv_t<float>(static_cast<const float*>(A), rows, cols, static_cast<const float*>(v), static_cast<float*>(y));
    });
}

// The three hooks below refuse what they cannot run before they look for a device (tests/test_cabi_refusals.py).
int admm_hip_test_gemv_t_ex(int is_double, int form, int nrhs, int nt, int max_seg_rows, int lda_extra, unsigned long long fill, int count,
                            const int* m, const int* k, const void* const* A, const void* const* v, const int* from, const int* skip,
                            void* const* part_out, long long part_capacity, void* const* y_out, long long* info_out) {
    return guarded([&] {
        ADMM_REQUIRE(m && k && A && v && part_out && info_out, "gemv_t_ex hook: m, k, A, v, part_out and info_out must not be NULL");
        ADMM_REQUIRE((is_double == 0 || is_double == 1) && form >= 0 && form <= 3 && (nrhs == 1 || nrhs == 2) && nt >= -1 && nt <= 1 &&
                         max_seg_rows >= 0 && lda_extra >= 0 && lda_extra <= 4096 && lda_extra % 32 == 0 && part_capacity >= 1,
                     "gemv_t_ex hook: is_double 0 or 1, form in 0 .. 3, nrhs 1 or 2, nt in -1 .. 1, max_seg_rows >= 0, lda_extra a multiple of 32 "
                     "in 0 .. 4096, part_capacity >= 1");
        ADMM_REQUIRE(nrhs == 1 || form == 0, "gemv_t_ex hook: two right-hand sides are built for form 0 only");
        ADMM_REQUIRE(form == 3 ? (count >= 1 && count <= kGemvHookMaxCount) : count == (form == 2 ? 2 : 1),
                     "gemv_t_ex hook: forms 0 and 1 take one product, form 2 two, form 3 one to eight");
        ADMM_REQUIRE(from == nullptr || form == 3, "gemv_t_ex hook: from belongs to form 3 (form 2 chains its two products itself)");
        for (int i = 0; i < count; ++i) {
            ADMM_REQUIRE(m[i] >= 1 && k[i] >= 1 && m[i] <= (1 << 20) && k[i] <= (1 << 20) &&
                             ((long long)m[i] + 31 + lda_extra) * (long long)k[i] <= (1ll << 28) && part_capacity <= (1ll << 28),
                         "gemv_t_ex hook: m and k in 1 .. 2^20, at most 2^28 elements of storage per matrix and per partial buffer");
            ADMM_REQUIRE(A[i] && part_out[i], "gemv_t_ex hook: every A[i] and part_out[i] must not be NULL");
            ADMM_REQUIRE(skip == nullptr || skip[i] == 0 || skip[i] == 1, "gemv_t_ex hook: skip values are 0 or 1");
            const int f = from ? from[i] : -1;
            ADMM_REQUIRE(f == -1 || (f >= 0 && f < count && f != i && from[f] == -1 && k[f] == m[i]),
                         "gemv_t_ex hook: from[i] is -1 or a product that is not chained itself and has k[from[i]] == m[i]");
            ADMM_REQUIRE(v[i] || f >= 0 || (form == 2 && i == 1), "gemv_t_ex hook: every product that is not chained needs its v[i]");
        }
        ADMM_REQUIRE(form != 2 || m[1] == k[0], "gemv_t_ex hook: a chain needs m[1] == k[0]");
        ADMM_REQUIRE((form != 1 && form != 2) || (y_out && y_out[count - 1]), "gemv_t_ex hook: forms 1 and 2 need y_out of the last product");
        const GemvExRequest q{form, nrhs, nt, max_seg_rows, lda_extra, count, fill, m, k, A, v, from, skip, part_out, part_capacity, y_out, info_out};
        if (is_double) test_gemv_t_ex<double>(q);
        else test_gemv_t_ex<float>(q);
    });
}

int admm_hip_test_wide_op(const float* X, int n, int p, const float* v, float* w) {
    return guarded([&] {
        ADMM_REQUIRE(X && v && w, "wide_op hook: X, v and w must not be NULL");
        ADMM_REQUIRE(n >= 1 && p >= 1 && n <= (1 << 20) && p <= (1 << 20) && ((long long)n + 31) * (long long)p <= (1ll << 28),
                     "wide_op hook: n and p in 1 .. 2^20, at most 2^28 elements of storage");
        test_wide_op(X, n, p, v, w);
    });
}

int admm_hip_test_block_sprad(const double* A, int n, int p, int nblocks, double* out, int* nsteps_out) {
    return guarded([&] {
        ADMM_REQUIRE(A && out && nsteps_out, "block_sprad hook: A, out and nsteps_out must not be NULL");
        ADMM_REQUIRE(n >= 1 && n <= 16384 && p >= 1 && p <= (1 << 20) && ((long long)n + 31) * (long long)p <= (1ll << 27),
                     "block_sprad hook: n in 1 .. 16384, p in 1 .. 2^20, at most 2^27 elements of storage");
        ADMM_REQUIRE(nblocks >= 1 && nblocks <= 64 && nblocks <= p, "block_sprad hook: nblocks in 1 .. min(64, p)");
        ADMM_REQUIRE(block_sprad_bytes(n, nblocks) <= 3.0e9, "block_sprad hook: the blocks must fit one batch of Lanczos runs (3 GB of Gram matrices and bases)");
        test_block_sprad(A, n, p, nblocks, out, nsteps_out);
    });
}

int admm_hip_test_wide_screen_prep(const float* X, int n, int p, int fmt, int nw, unsigned pad_fill, void* copy_out, long long copy_capacity,
                                   float* s_out, float* scale_out, double* rate_out, long long* info_out) {
    return guarded([&] {
        ADMM_REQUIRE(X && copy_out && s_out && rate_out && info_out, "wide_screen_prep hook: X, copy_out, s_out, rate_out and info_out must not be NULL");
        ADMM_REQUIRE(fmt == 8 || fmt == 16, "wide_screen_prep hook: fmt is 8 or 16");
        ADMM_REQUIRE(fmt == 16 || scale_out, "wide_screen_prep hook: the 8-bit code needs scale_out");
        ADMM_REQUIRE(n >= 1 && p >= 1 && nw >= 1 && n <= (1 << 20) && p <= (1 << 20) && nw <= (1 << 20) && ((long long)n + 15) * (long long)p <= (1ll << 28),
                     "wide_screen_prep hook: n, p and nw in 1 .. 2^20, at most 2^28 elements of storage");
        ADMM_REQUIRE(copy_capacity >= (long long)p * wide_screen_layout(n, p, fmt, nw).ldh, "wide_screen_prep hook: copy_capacity below p * ldh elements");
        test_wide_screen_prep(X, n, p, fmt, nw, pad_fill, copy_out, s_out, scale_out, rate_out, info_out);
    });
}

int admm_hip_test_sbp_screen_prep(const double* A, int n, int pl, int lda_extra, unsigned pad_fill, unsigned short* copy_out, long long copy_capacity,
                                  float* s_out, long long* info_out) {
    return guarded([&] {
        ADMM_REQUIRE(A && copy_out && s_out && info_out, "sbp_screen_prep hook: A, copy_out, s_out and info_out must not be NULL");
        ADMM_REQUIRE(n >= 1 && pl >= 1 && n <= (1 << 20) && pl <= (1 << 20) && lda_extra >= 0 && lda_extra <= 4096 &&
                         ((long long)n + 31 + lda_extra) * (long long)pl <= (1ll << 27),
                     "sbp_screen_prep hook: n and pl in 1 .. 2^20, lda_extra in 0 .. 4096, at most 2^27 elements of storage");
        ADMM_REQUIRE(copy_capacity >= (long long)pl * sbp_screen_ldh(n), "sbp_screen_prep hook: copy_capacity below pl * ldh elements");
        test_sbp_screen_prep(A, n, pl, lda_extra, pad_fill, copy_out, s_out, info_out);
    });
}

int admm_hip_test_gather(const void* A, int rows, int cols, int is_double, const void* v, double* y) {
    return guarded([&] {
        ADMM_REQUIRE(A && v && y && rows > 0 && cols > 0, "bad arguments");
        if (is_double) test_gather<double>(static_cast<const double*>(A), rows, cols, static_cast<const double*>(v), y);
        else test_gather<float>(static_cast<const float*>(A), rows, cols, static_cast<const float*>(v), y);
    });
}

int admm_hip_test_spd_inverse(const void* A, int n, int precision, void* Ainv) {
    return guarded([&] {
        ADMM_REQUIRE(A && Ainv && n > 0 && precision >= 0 && precision <= 2, "bad arguments");
        if (precision == 1) test_spd_inverse<double>(static_cast<const double*>(A), n, static_cast<double*>(Ainv), false);
        else test_spd_inverse<float>(static_cast<const float*>(A), n, static_cast<float*>(Ainv), precision == 2);
    });
}

int admm_hip_test_spd_inverse_shift(const float* A, int n, double diag, float* Ainv) {
    return guarded([&] {
        ADMM_REQUIRE(A && Ainv && n > 0 && std::isfinite(diag), "bad arguments");
        test_spd_inverse_shift(A, n, diag, Ainv);
    });
}

int admm_hip_test_cholesky_linvt(int is_double, const void* A, int n, void* L, void* U) {
    return guarded([&] {
        ADMM_REQUIRE(A && L && U && n > 0, "bad arguments");
        if (is_double) test_cholesky_linvt<double>(static_cast<const double*>(A), n, static_cast<double*>(L), static_cast<double*>(U));
        else test_cholesky_linvt<float>(static_cast<const float*>(A), n, static_cast<float*>(L), static_cast<float*>(U));
    });
}

int admm_hip_test_gemm_nt(int is_double, int lower, int mirror, int kstart_row, int b_lower, int in_place, int M, int N, int K,
                          double alpha, double beta, const void* A, const void* B, void* C) {
    return guarded([&] {
        ADMM_REQUIRE(A && B && C, "gemm_nt hook: A, B and C must not be NULL");
        ADMM_REQUIRE(M > 0 && N > 0 && K > 0 && M <= 16384 && N <= 16384 && K <= (1 << 20), "gemm_nt hook: M, N in 1 .. 16384 and K in 1 .. 2^20");
        ADMM_REQUIRE(std::isfinite(alpha) && std::isfinite(beta), "gemm_nt hook: alpha and beta must be finite");
        ADMM_REQUIRE(!lower || M == N, "gemm_nt hook: lower needs a square output (M == N)");
        ADMM_REQUIRE(!mirror || lower, "gemm_nt hook: the mirrored store belongs to lower launches");
        ADMM_REQUIRE(!b_lower || (is_double && !lower), "gemm_nt hook: b_lower (the K loop ended at the tile's last column) is double only and not for lower launches");
        ADMM_REQUIRE(!in_place || (N <= 128 && K == 128 && !lower), "gemm_nt hook: in_place needs N <= 128, K == 128 and a full (not lower) launch");
        if (is_double)
            test_gemm_nt<double>(lower != 0, mirror != 0, kstart_row != 0, b_lower != 0, in_place != 0, M, N, K, alpha, beta, static_cast<const double*>(A),
                                 static_cast<const double*>(B), static_cast<double*>(C));
        else
            test_gemm_nt<float>(lower != 0, mirror != 0, kstart_row != 0, false, in_place != 0, M, N, K, alpha, beta, static_cast<const float*>(A),
                                static_cast<const float*>(B), static_cast<float*>(C));
    });
}

int admm_hip_test_cv_fold_system(const double* x, const double* y, int n, int p, const int* fold_id, int nfolds, int fold,
                                 int standardize, int intercept, float* gram, float* xy, float* mean_x, float* scale_x, float* mean_scale_y) {
    return guarded([&] { test_cv_fold_system(x, y, n, p, fold_id, nfolds, fold, standardize, intercept, gram, xy, mean_x, scale_x, mean_scale_y); });
}

}  // extern "C"
