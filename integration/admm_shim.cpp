// Rcpp shim that a maintainer of yixuan/ADMM adds to src/ in place of Lasso.cpp, Enet.cpp, ParLasso.cpp,
// LAD.cpp and BP.cpp.  It keeps the five `.Call` symbols the R code looks up by name (and supplies admm_parbp / admm_dantzig)
// (R/30_admm_lasso.R:140,149; R/40_admm_enet.R:53; R/20_admm_lad.R:60; R/10_admm_bp.R:104,111; R/50_admm_dantzig.R:38) and forwards the
// unpacked arguments to libadmm_hip.so (include/admm_hip.h).  R/ stays untouched.
//
// src/Makevars:   PKG_CPPFLAGS = -I/path/to/admm-mi355x/include
//                 PKG_LIBS     = -L/path/to/admm-mi355x/admm_amd/lib -ladmm_hip -Wl,-rpath,/path/to/admm-mi355x/admm_amd/lib
// (R is not available in the build image of this repository, so this file is compile-checked only where R exists.)
#include <Rcpp.h>
#include <vector>
#include "admm_hip.h"

using Rcpp::as;
using Rcpp::IntegerVector;
using Rcpp::List;
using Rcpp::Named;
using Rcpp::NumericMatrix;
using Rcpp::NumericVector;

static admm_opts unpack_opts(SEXP opts_) {
    List opts(opts_);
    admm_opts o;
    o.maxit = as<int>(opts["maxit"]);
    o.eps_abs = as<double>(opts["eps_abs"]);
    o.eps_rel = as<double>(opts["eps_rel"]);
    o.rho = as<double>(opts["rho"]);
    return o;
}

static void check(int rc) {
    if (rc != ADMM_OK) Rcpp::stop("libadmm_hip: %s", admm_hip_last_error());
}

// (p+1) x nlambda dense -> dgCMatrix with row 0 always stored (Lasso.cpp:22-30,131)
template <typename T>
static Rcpp::S4 to_dgCMatrix(const std::vector<T>& beta, int nrow, int ncol) {
    std::vector<int> ip(1, 0), ii;
    std::vector<double> xx;
    for (int j = 0; j < ncol; ++j) {
        for (int i = 0; i < nrow; ++i) {
            const T v = beta[(size_t)j * nrow + i];
            if (i == 0 || v != T(0)) { ii.push_back(i); xx.push_back((double)v); }
        }
        ip.push_back((int)ii.size());
    }
    Rcpp::S4 m("dgCMatrix");
    m.slot("i") = IntegerVector(ii.begin(), ii.end());
    m.slot("p") = IntegerVector(ip.begin(), ip.end());
    m.slot("x") = NumericVector(xx.begin(), xx.end());
    m.slot("Dim") = IntegerVector::create(nrow, ncol);
    return m;
}

static SEXP lasso_family(int which, SEXP x_, SEXP y_, SEXP lambda_, SEXP nlambda_, SEXP lmin_ratio_,
                         SEXP standardize_, SEXP intercept_, double alpha, int nthread, SEXP opts_) {
    NumericMatrix x(x_);
    NumericVector y(y_), lambda(lambda_);
    const int n = x.nrow(), p = x.ncol();
    const int nl_in = lambda.size();
    const int nl = nl_in > 0 ? nl_in : as<int>(nlambda_);
    admm_opts o = unpack_opts(opts_);
    NumericVector lambda_out(nl);
    IntegerVector niter(nl);
    std::vector<float> beta((size_t)(p + 1) * nl);
    const double* lam = nl_in > 0 ? lambda.begin() : nullptr;
    int rc;
    if (which == 0)
        rc = admm_hip_lasso(x.begin(), y.begin(), n, p, ADMM_MEM_HOST, lam, nl_in, as<int>(nlambda_), as<double>(lmin_ratio_),
                            as<bool>(standardize_), as<bool>(intercept_), &o, lambda_out.begin(), beta.data(), niter.begin(), nullptr);
    else if (which == 1)
        rc = admm_hip_enet(x.begin(), y.begin(), n, p, ADMM_MEM_HOST, lam, nl_in, as<int>(nlambda_), as<double>(lmin_ratio_),
                           as<bool>(standardize_), as<bool>(intercept_), alpha, &o, lambda_out.begin(), beta.data(), niter.begin(), nullptr);
    else
        rc = admm_hip_parlasso(x.begin(), y.begin(), n, p, ADMM_MEM_HOST, lam, nl_in, as<int>(nlambda_), as<double>(lmin_ratio_),
                               as<bool>(standardize_), as<bool>(intercept_), nthread, &o, lambda_out.begin(), beta.data(), niter.begin(), nullptr);
    check(rc);
    return List::create(Named("lambda") = lambda_out, Named("beta") = to_dgCMatrix(beta, p + 1, nl), Named("niter") = niter);
}

RcppExport SEXP admm_lasso(SEXP x_, SEXP y_, SEXP lambda_, SEXP nlambda_, SEXP lmin_ratio_,
                           SEXP standardize_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    return lasso_family(0, x_, y_, lambda_, nlambda_, lmin_ratio_, standardize_, intercept_, 1.0, 0, opts_);
END_RCPP
}

RcppExport SEXP admm_enet(SEXP x_, SEXP y_, SEXP lambda_, SEXP nlambda_, SEXP lmin_ratio_,
                          SEXP standardize_, SEXP intercept_, SEXP alpha_, SEXP opts_) {
BEGIN_RCPP
    return lasso_family(1, x_, y_, lambda_, nlambda_, lmin_ratio_, standardize_, intercept_, as<double>(alpha_), 0, opts_);
END_RCPP
}

RcppExport SEXP admm_parlasso(SEXP x_, SEXP y_, SEXP lambda_, SEXP nlambda_, SEXP lmin_ratio_,
                              SEXP standardize_, SEXP intercept_, SEXP nthread_, SEXP opts_) {
BEGIN_RCPP
    return lasso_family(2, x_, y_, lambda_, nlambda_, lmin_ratio_, standardize_, intercept_, 1.0, as<int>(nthread_), opts_);
END_RCPP
}

// Group lasso (not in the reference; include/admm_hip.h, admm_hip_grplasso): the arguments of admm_lasso plus `group`, the 0-based
// group id of every column (non-decreasing, no gaps: the columns of a group adjacent), and `group_weight`, one weight per group or
// numeric(0) for sqrt(group size).  n > p only.
RcppExport SEXP admm_grplasso(SEXP x_, SEXP y_, SEXP lambda_, SEXP nlambda_, SEXP lmin_ratio_,
                              SEXP standardize_, SEXP intercept_, SEXP group_, SEXP group_weight_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericVector y(y_), lambda(lambda_), group_weight(group_weight_);
    IntegerVector group(group_);
    const int n = x.nrow(), p = x.ncol();
    if (group.size() != p) Rcpp::stop("group should have length ncol(x)");
    const int ngroups = p > 0 ? group[p - 1] + 1 : 0;
    if (group_weight.size() != 0 && group_weight.size() != ngroups) Rcpp::stop("group_weight should have one entry per group");
    const int nl_in = lambda.size();
    const int nl = nl_in > 0 ? nl_in : as<int>(nlambda_);
    admm_opts o = unpack_opts(opts_);
    NumericVector lambda_out(nl);
    IntegerVector niter(nl);
    std::vector<float> beta((size_t)(p + 1) * nl);
    check(admm_hip_grplasso(x.begin(), y.begin(), n, p, ADMM_MEM_HOST, group.begin(), group_weight.size() ? group_weight.begin() : nullptr, ngroups,
                            nl_in > 0 ? lambda.begin() : nullptr, nl_in, as<int>(nlambda_), as<double>(lmin_ratio_),
                            as<bool>(standardize_), as<bool>(intercept_), &o, lambda_out.begin(), beta.data(), niter.begin(), nullptr));
    return List::create(Named("lambda") = lambda_out, Named("beta") = to_dgCMatrix(beta, p + 1, nl), Named("niter") = niter);
END_RCPP
}

// Sparse-group lasso (not in the reference; include/admm_hip.h, admm_hip_sgl): the arguments of admm_grplasso plus `l1_weight`, one l1
// weight per column or numeric(0) for all 1, and the mixing parameter `alpha` in [0, 1] (0 = group lasso, 1 = Lasso with penalty
// factors l1_weight).  n > p only.
RcppExport SEXP admm_sgl(SEXP x_, SEXP y_, SEXP lambda_, SEXP nlambda_, SEXP lmin_ratio_,
                         SEXP standardize_, SEXP intercept_, SEXP group_, SEXP group_weight_, SEXP l1_weight_, SEXP alpha_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericVector y(y_), lambda(lambda_), group_weight(group_weight_), l1_weight(l1_weight_);
    IntegerVector group(group_);
    const int n = x.nrow(), p = x.ncol();
    if (group.size() != p) Rcpp::stop("group should have length ncol(x)");
    const int ngroups = p > 0 ? group[p - 1] + 1 : 0;
    if (group_weight.size() != 0 && group_weight.size() != ngroups) Rcpp::stop("group_weight should have one entry per group");
    if (l1_weight.size() != 0 && l1_weight.size() != p) Rcpp::stop("l1_weight should have one entry per column");
    const int nl_in = lambda.size();
    const int nl = nl_in > 0 ? nl_in : as<int>(nlambda_);
    admm_opts o = unpack_opts(opts_);
    NumericVector lambda_out(nl);
    IntegerVector niter(nl);
    std::vector<float> beta((size_t)(p + 1) * nl);
    check(admm_hip_sgl(x.begin(), y.begin(), n, p, ADMM_MEM_HOST, group.begin(), group_weight.size() ? group_weight.begin() : nullptr, ngroups,
                       l1_weight.size() ? l1_weight.begin() : nullptr, as<double>(alpha_),
                       nl_in > 0 ? lambda.begin() : nullptr, nl_in, as<int>(nlambda_), as<double>(lmin_ratio_),
                       as<bool>(standardize_), as<bool>(intercept_), &o, lambda_out.begin(), beta.data(), niter.begin(), nullptr));
    return List::create(Named("lambda") = lambda_out, Named("beta") = to_dgCMatrix(beta, p + 1, nl), Named("niter") = niter);
END_RCPP
}

// Box-constrained, weighted elastic net (not in the reference; include/admm_hip.h, admm_hip_boxenet): the arguments of admm_enet plus
// `lower` / `upper`, bounds on the coefficients on the original scale (one per column or numeric(0) for none; lower <= 0 <= upper,
// -Inf / Inf allowed), and `penalty_factor`, one factor per column or numeric(0) for all 1.  alpha < 0 selects the Lasso prox.  n > p only.
RcppExport SEXP admm_boxenet(SEXP x_, SEXP y_, SEXP lambda_, SEXP nlambda_, SEXP lmin_ratio_,
                             SEXP standardize_, SEXP intercept_, SEXP lower_, SEXP upper_, SEXP penalty_factor_, SEXP alpha_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericVector y(y_), lambda(lambda_), lower(lower_), upper(upper_), penalty_factor(penalty_factor_);
    const int n = x.nrow(), p = x.ncol();
    if (lower.size() != 0 && lower.size() != p) Rcpp::stop("lower should have one entry per column");
    if (upper.size() != 0 && upper.size() != p) Rcpp::stop("upper should have one entry per column");
    if (penalty_factor.size() != 0 && penalty_factor.size() != p) Rcpp::stop("penalty_factor should have one entry per column");
    const int nl_in = lambda.size();
    const int nl = nl_in > 0 ? nl_in : as<int>(nlambda_);
    admm_opts o = unpack_opts(opts_);
    NumericVector lambda_out(nl);
    IntegerVector niter(nl);
    std::vector<float> beta((size_t)(p + 1) * nl);
    check(admm_hip_boxenet(x.begin(), y.begin(), n, p, ADMM_MEM_HOST, lower.size() ? lower.begin() : nullptr, upper.size() ? upper.begin() : nullptr,
                           penalty_factor.size() ? penalty_factor.begin() : nullptr, as<double>(alpha_),
                           nl_in > 0 ? lambda.begin() : nullptr, nl_in, as<int>(nlambda_), as<double>(lmin_ratio_),
                           as<bool>(standardize_), as<bool>(intercept_), &o, lambda_out.begin(), beta.data(), niter.begin(), nullptr));
    return List::create(Named("lambda") = lambda_out, Named("beta") = to_dgCMatrix(beta, p + 1, nl), Named("niter") = niter);
END_RCPP
}

// Multi-task lasso (not in the reference; include/admm_hip.h, admm_hip_mtlasso): the arguments of admm_lasso with an n x m matrix Y
// in the place of y, plus `row_weight`, one weight per column of x or numeric(0) for all 1.  n > p only, m <= ADMM_HIP_MT_MAX.
// beta: a (p + 1) x (m * nlambda) dgCMatrix, column l * m + k = response k at lambda l (intercept first).
RcppExport SEXP admm_mtlasso(SEXP x_, SEXP Y_, SEXP lambda_, SEXP nlambda_, SEXP lmin_ratio_,
                             SEXP standardize_, SEXP intercept_, SEXP row_weight_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_), Y(Y_);
    NumericVector lambda(lambda_), row_weight(row_weight_);
    const int n = x.nrow(), p = x.ncol(), m = Y.ncol();
    if (Y.nrow() != n) Rcpp::stop("nrow(x) should be equal to nrow(Y)");
    if (row_weight.size() != 0 && row_weight.size() != p) Rcpp::stop("row_weight should have one entry per column of x");
    const int nl_in = lambda.size();
    const int nl = nl_in > 0 ? nl_in : as<int>(nlambda_);
    admm_opts o = unpack_opts(opts_);
    NumericVector lambda_out(nl);
    IntegerVector niter(nl);
    std::vector<float> beta((size_t)(p + 1) * (size_t)(m > 0 ? m : 1) * nl);
    check(admm_hip_mtlasso(x.begin(), Y.begin(), n, p, m, ADMM_MEM_HOST, row_weight.size() ? row_weight.begin() : nullptr,
                           nl_in > 0 ? lambda.begin() : nullptr, nl_in, as<int>(nlambda_), as<double>(lmin_ratio_),
                           as<bool>(standardize_), as<bool>(intercept_), &o, lambda_out.begin(), beta.data(), niter.begin(), nullptr));
    return List::create(Named("lambda") = lambda_out, Named("beta") = to_dgCMatrix(beta, p + 1, m * nl), Named("niter") = niter);
END_RCPP
}

RcppExport SEXP admm_lad(SEXP x_, SEXP y_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericVector y(y_);
    admm_opts o = unpack_opts(opts_);
    NumericVector beta(x.ncol() + 1);
    int niter = 0;
    check(admm_hip_lad(x.begin(), y.begin(), x.nrow(), x.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), &o, beta.begin(), &niter, nullptr));
    return List::create(Named("beta") = beta, Named("niter") = niter);
END_RCPP
}

// Quantile regression (not in the reference): .Call("admm_quantreg", x, y, tau, intercept, opts) -> beta: (p + 1) x length(tau)
// numeric matrix, column k = tau[k], intercept first; niter: integer vector.  The intercept is fitted, not recovered as admm_lad's.
RcppExport SEXP admm_quantreg(SEXP x_, SEXP y_, SEXP tau_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericVector y(y_), tau(tau_);
    admm_opts o = unpack_opts(opts_);
    const int ntau = tau.size();
    NumericMatrix beta(x.ncol() + 1, ntau);
    IntegerVector niter(ntau);
    check(admm_hip_quantreg(x.begin(), y.begin(), x.nrow(), x.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), tau.begin(), ntau, &o,
                            beta.begin(), niter.begin(), nullptr));
    return List::create(Named("tau") = tau, Named("beta") = beta, Named("niter") = niter);
END_RCPP
}

// Huber / expectile regression (not in the reference): .Call("admm_huber", x, y, delta, tau, intercept, opts) with delta
// and tau of one common length (delta in the units of y, Inf = expectile regression) -> beta: (p + 1) x length(delta), intercept first.
RcppExport SEXP admm_huber(SEXP x_, SEXP y_, SEXP delta_, SEXP tau_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericVector y(y_), delta(delta_), tau(tau_);
    admm_opts o = unpack_opts(opts_);
    const int nfit = delta.size();
    if (tau.size() != nfit) Rcpp::stop("delta and tau should have the same length");
    NumericMatrix beta(x.ncol() + 1, nfit);
    IntegerVector niter(nfit);
    check(admm_hip_huber(x.begin(), y.begin(), x.nrow(), x.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), delta.begin(), tau.begin(), nfit, &o,
                         beta.begin(), niter.begin(), nullptr));
    return List::create(Named("delta") = delta, Named("tau") = tau, Named("beta") = beta, Named("niter") = niter);
END_RCPP
}

// Logistic regression (not in the reference): .Call("admm_logit", x, y, intercept, opts) with y holding labels 0 / 1
// -> beta: p + 1, intercept first; niter = maxit + 1 when the fit has not converged (separable labels).
RcppExport SEXP admm_logit(SEXP x_, SEXP y_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericVector y(y_);
    admm_opts o = unpack_opts(opts_);
    NumericVector beta(x.ncol() + 1);
    int niter = 0;
    check(admm_hip_logit(x.begin(), y.begin(), x.nrow(), x.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), &o, beta.begin(), &niter, nullptr));
    return List::create(Named("beta") = beta, Named("niter") = niter);
END_RCPP
}

// Logistic regression for the columns of a label matrix on one setup (not in the reference):
// .Call("admm_logit_multi", x, Y, intercept, opts) with Y n x k holding labels 0 / 1 -> beta: (p + 1) x k, intercept first; niter: k.
RcppExport SEXP admm_logit_multi(SEXP x_, SEXP y_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericMatrix y(y_);
    if (y.nrow() != x.nrow()) Rcpp::stop("nrow(x) should be equal to nrow(Y)");
    admm_opts o = unpack_opts(opts_);
    NumericMatrix beta(x.ncol() + 1, y.ncol());
    IntegerVector niter(y.ncol());
    check(admm_hip_logit_multi(x.begin(), y.begin(), x.nrow(), x.ncol(), y.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), &o, beta.begin(), niter.begin(), nullptr));
    return List::create(Named("beta") = beta, Named("niter") = niter);
END_RCPP
}

// Ridge logistic regression for the columns of a label matrix and a grid of lambda (not in the reference):
// .Call("admm_logit_ridge", x, Y, lambda, intercept, opts) -> beta: (p + 1) x (k nlambda), column l k + c = (lambda l, label column c),
// intercept first -- dim(res$beta) <- c(p + 1, k, nlambda) gives the array; niter: k nlambda, entry l k + c.  lambda is on the
// standardised scale and used in the order given.
RcppExport SEXP admm_logit_ridge(SEXP x_, SEXP y_, SEXP lambda_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericMatrix y(y_);
    NumericVector lambda(lambda_);
    if (y.nrow() != x.nrow()) Rcpp::stop("nrow(x) should be equal to nrow(Y)");
    admm_opts o = unpack_opts(opts_);
    const int nlambda = lambda.size();
    NumericMatrix beta(x.ncol() + 1, y.ncol() * nlambda);
    IntegerVector niter(y.ncol() * nlambda);
    check(admm_hip_logit_ridge(x.begin(), y.begin(), x.nrow(), x.ncol(), y.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), lambda.begin(), nlambda, &o,
                               beta.begin(), niter.begin(), nullptr));
    return List::create(Named("beta") = beta, Named("niter") = niter, Named("lambda") = lambda);
END_RCPP
}

// Elastic-net logistic regression for the columns of a label matrix and (lambda, alpha) PAIRS (not in the reference):
// .Call("admm_logit_enet", x, Y, lambda, alpha, intercept, opts) -> beta: (p + 1) x (k ncell), column l k + c = (cell l, label column c),
// intercept first, exact zeros where the penalty removes a coefficient; niter: k ncell.  alpha: as long as lambda, or one value for
// every lambda.  lambda is on the standardised scale (glmnet's lambda times nrow(x)).
RcppExport SEXP admm_logit_enet(SEXP x_, SEXP y_, SEXP lambda_, SEXP alpha_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericMatrix y(y_);
    NumericVector lambda(lambda_);
    NumericVector alpha_in(alpha_);
    if (y.nrow() != x.nrow()) Rcpp::stop("nrow(x) should be equal to nrow(Y)");
    const int ncell = lambda.size();
    if (alpha_in.size() != ncell && alpha_in.size() != 1) Rcpp::stop("alpha must have one value or as many as lambda");
    NumericVector alpha(ncell);
    for (int l = 0; l < ncell; ++l) alpha[l] = alpha_in[alpha_in.size() == 1 ? 0 : l];
    admm_opts o = unpack_opts(opts_);
    NumericMatrix beta(x.ncol() + 1, y.ncol() * ncell);
    IntegerVector niter(y.ncol() * ncell);
    check(admm_hip_logit_enet(x.begin(), y.begin(), x.nrow(), x.ncol(), y.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), lambda.begin(), alpha.begin(), ncell, &o,
                              beta.begin(), niter.begin(), nullptr));
    return List::create(Named("beta") = beta, Named("niter") = niter, Named("lambda") = lambda, Named("alpha") = alpha);
END_RCPP
}

// lambda_1 per label column: .Call("admm_logit_enet_lambda_max", x, Y, intercept) -> numeric k; a cell's lambda_max is this over its alpha
RcppExport SEXP admm_logit_enet_lambda_max(SEXP x_, SEXP y_, SEXP intercept_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericMatrix y(y_);
    if (y.nrow() != x.nrow()) Rcpp::stop("nrow(x) should be equal to nrow(Y)");
    NumericVector out(y.ncol());
    check(admm_hip_logit_enet_lambda_max(x.begin(), y.begin(), x.nrow(), x.ncol(), y.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), out.begin()));
    return out;
END_RCPP
}

// One label vector and one cell with the decision trace (ADMM_TRACE_FIELDS doubles per record, at most maxit + 2 records):
// .Call("admm_logit_enet_state", x, y, lambda, alpha, intercept, opts) -> beta (p + 1), niter, trace (ADMM_TRACE_FIELDS x records)
RcppExport SEXP admm_logit_enet_state(SEXP x_, SEXP y_, SEXP lambda_, SEXP alpha_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericVector y(y_);
    if (y.size() != x.nrow()) Rcpp::stop("nrow(x) should be equal to length(y)");
    admm_opts o = unpack_opts(opts_);
    NumericVector beta(x.ncol() + 1);
    int niter = 0;
    const long long cap = (long long)o.maxit + 2;
    NumericMatrix trace(ADMM_TRACE_FIELDS, (int)cap);
    long long ntrace = 0;
    check(admm_hip_logit_enet_state(x.begin(), y.begin(), x.nrow(), x.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), as<double>(lambda_), as<double>(alpha_), &o,
                                    beta.begin(), &niter, nullptr, trace.begin(), cap, &ntrace, nullptr, 0, nullptr));
    return List::create(Named("beta") = beta, Named("niter") = niter, Named("trace") = trace, Named("ntrace") = (double)ntrace);
END_RCPP
}

// Poisson regression with the elastic-net penalty for the columns of a count matrix and (lambda, alpha) PAIRS (not in the reference;
// INTEGRATION.md): .Call("admm_poisson", x, Y, lambda, alpha, intercept, opts) -> beta: (p + 1) x (k ncell), column l k + c = (cell l,
// count column c), intercept first, exact zeros where the penalty removes a coefficient; niter: k ncell.  alpha: as long as lambda, or
// one value for every lambda.  lambda is on the standardised scale (glmnet's lambda times nrow(x)); 0 is the plain GLM.
RcppExport SEXP admm_poisson(SEXP x_, SEXP y_, SEXP lambda_, SEXP alpha_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericMatrix y(y_);
    NumericVector lambda(lambda_);
    NumericVector alpha_in(alpha_);
    if (y.nrow() != x.nrow()) Rcpp::stop("nrow(x) should be equal to nrow(Y)");
    const int ncell = lambda.size();
    if (alpha_in.size() != ncell && alpha_in.size() != 1) Rcpp::stop("alpha must have one value or as many as lambda");
    NumericVector alpha(ncell);
    for (int l = 0; l < ncell; ++l) alpha[l] = alpha_in[alpha_in.size() == 1 ? 0 : l];
    admm_opts o = unpack_opts(opts_);
    NumericMatrix beta(x.ncol() + 1, y.ncol() * ncell);
    IntegerVector niter(y.ncol() * ncell);
    check(admm_hip_poisson(x.begin(), y.begin(), x.nrow(), x.ncol(), y.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), lambda.begin(), alpha.begin(), ncell, &o,
                           beta.begin(), niter.begin(), nullptr));
    return List::create(Named("beta") = beta, Named("niter") = niter, Named("lambda") = lambda, Named("alpha") = alpha);
END_RCPP
}

// lambda_1 per count column: .Call("admm_poisson_lambda_max", x, Y, intercept) -> numeric k; a cell's lambda_max is this over its alpha
RcppExport SEXP admm_poisson_lambda_max(SEXP x_, SEXP y_, SEXP intercept_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericMatrix y(y_);
    if (y.nrow() != x.nrow()) Rcpp::stop("nrow(x) should be equal to nrow(Y)");
    NumericVector out(y.ncol());
    check(admm_hip_poisson_lambda_max(x.begin(), y.begin(), x.nrow(), x.ncol(), y.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), out.begin()));
    return out;
END_RCPP
}

// One count vector and one cell with the decision trace (ADMM_TRACE_FIELDS doubles per record, at most maxit + 2 records):
// .Call("admm_poisson_state", x, y, lambda, alpha, intercept, opts) -> beta (p + 1), niter, trace (ADMM_TRACE_FIELDS x records)
RcppExport SEXP admm_poisson_state(SEXP x_, SEXP y_, SEXP lambda_, SEXP alpha_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericVector y(y_);
    if (y.size() != x.nrow()) Rcpp::stop("nrow(x) should be equal to length(y)");
    admm_opts o = unpack_opts(opts_);
    NumericVector beta(x.ncol() + 1);
    int niter = 0;
    const long long cap = (long long)o.maxit + 2;
    NumericMatrix trace(ADMM_TRACE_FIELDS, (int)cap);
    long long ntrace = 0;
    check(admm_hip_poisson_state(x.begin(), y.begin(), x.nrow(), x.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), as<double>(lambda_), as<double>(alpha_), &o,
                                 beta.begin(), &niter, nullptr, trace.begin(), cap, &ntrace, nullptr, 0, nullptr));
    return List::create(Named("beta") = beta, Named("niter") = niter, Named("trace") = trace, Named("ntrace") = (double)ntrace);
END_RCPP
}

// K-fold cross-validation of the two calls above by held-out deviance, every fit on the full-data setup (not in the reference;
// INTEGRATION.md): .Call("admm_logit_enet_cv", x, Y, lambda, alpha, fold_id, nfolds, intercept, opts) -> beta, niter of the full-data fit
// as admm_logit_enet's; cv_mean, cv_se: k x ncell; fold_dev: (k ncell) x nfolds, row l k + c; idx_min, idx_1se: per column the 1-based
// cell; lambda_min, lambda_1se.  fold_id: integer(0) = row i in fold (i - 1) mod nfolds, else nrow(x) 0-based fold numbers.
static SEXP glm_cv_call(decltype(&admm_hip_logit_enet_cv) entry, SEXP x_, SEXP y_, SEXP lambda_, SEXP alpha_, SEXP fold_id_, SEXP nfolds_, SEXP intercept_, SEXP opts_) {
    NumericMatrix x(x_);
    NumericMatrix y(y_);
    NumericVector lambda(lambda_);
    NumericVector alpha_in(alpha_);
    IntegerVector fold_id(fold_id_);
    if (y.nrow() != x.nrow()) Rcpp::stop("nrow(x) should be equal to nrow(Y)");
    if (fold_id.size() != 0 && fold_id.size() != x.nrow()) Rcpp::stop("fold_id must be empty or as long as nrow(x)");
    const int ncell = lambda.size(), k = y.ncol(), nfolds = as<int>(nfolds_);
    if (alpha_in.size() != ncell && alpha_in.size() != 1) Rcpp::stop("alpha must have one value or as many as lambda");
    if (nfolds < 2) Rcpp::stop("nfolds must be at least 2");
    NumericVector alpha(ncell);
    for (int l = 0; l < ncell; ++l) alpha[l] = alpha_in[alpha_in.size() == 1 ? 0 : l];
    admm_opts o = unpack_opts(opts_);
    NumericMatrix beta(x.ncol() + 1, k * ncell), cv_mean(k, ncell), cv_se(k, ncell), fold_dev(k * ncell, nfolds);
    IntegerVector niter(k * ncell), idx_min(k), idx_1se(k);
    check(entry(x.begin(), y.begin(), x.nrow(), x.ncol(), k, ADMM_MEM_HOST, as<bool>(intercept_), fold_id.size() ? fold_id.begin() : nullptr, nfolds, lambda.begin(),
                alpha.begin(), ncell, &o, beta.begin(), niter.begin(), cv_mean.begin(), cv_se.begin(), fold_dev.begin(), nullptr, nullptr, idx_min.begin(), idx_1se.begin(),
                nullptr));
    NumericVector lambda_min(k), lambda_1se(k);
    for (int c = 0; c < k; ++c) { lambda_min[c] = lambda[idx_min[c]]; lambda_1se[c] = lambda[idx_1se[c]]; ++idx_min[c]; ++idx_1se[c]; }
    return List::create(Named("beta") = beta, Named("niter") = niter, Named("lambda") = lambda, Named("alpha") = alpha, Named("cv_mean") = cv_mean, Named("cv_se") = cv_se,
                        Named("fold_dev") = fold_dev, Named("idx_min") = idx_min, Named("idx_1se") = idx_1se, Named("lambda_min") = lambda_min,
                        Named("lambda_1se") = lambda_1se);
}
RcppExport SEXP admm_logit_enet_cv(SEXP x_, SEXP y_, SEXP lambda_, SEXP alpha_, SEXP fold_id_, SEXP nfolds_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    return glm_cv_call(admm_hip_logit_enet_cv, x_, y_, lambda_, alpha_, fold_id_, nfolds_, intercept_, opts_);
END_RCPP
}
RcppExport SEXP admm_poisson_cv(SEXP x_, SEXP y_, SEXP lambda_, SEXP alpha_, SEXP fold_id_, SEXP nfolds_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    return glm_cv_call(admm_hip_poisson_cv, x_, y_, lambda_, alpha_, fold_id_, nfolds_, intercept_, opts_);
END_RCPP
}

// One vector, one cell and one fold held out (fold = -1: none) with the decision trace, as admm_logit_enet_state / admm_poisson_state:
// .Call("admm_logit_enet_cv_state", x, y, lambda, alpha, fold_id, nfolds, fold, intercept, opts) -> beta (p + 1), niter, trace, ntrace
static SEXP glm_cv_state_call(decltype(&admm_hip_logit_enet_cv_state) entry, SEXP x_, SEXP y_, SEXP lambda_, SEXP alpha_, SEXP fold_id_, SEXP nfolds_, SEXP fold_,
                              SEXP intercept_, SEXP opts_) {
    NumericMatrix x(x_);
    NumericVector y(y_);
    IntegerVector fold_id(fold_id_);
    if (y.size() != x.nrow()) Rcpp::stop("nrow(x) should be equal to length(y)");
    if (fold_id.size() != 0 && fold_id.size() != x.nrow()) Rcpp::stop("fold_id must be empty or as long as nrow(x)");
    admm_opts o = unpack_opts(opts_);
    NumericVector beta(x.ncol() + 1);
    int niter = 0;
    const long long cap = (long long)o.maxit + 2;
    NumericMatrix trace(ADMM_TRACE_FIELDS, (int)cap);
    long long ntrace = 0;
    check(entry(x.begin(), y.begin(), x.nrow(), x.ncol(), ADMM_MEM_HOST, as<bool>(intercept_), fold_id.size() ? fold_id.begin() : nullptr, as<int>(nfolds_), as<int>(fold_),
                as<double>(lambda_), as<double>(alpha_), &o, beta.begin(), &niter, nullptr, trace.begin(), cap, &ntrace, nullptr, 0, nullptr));
    return List::create(Named("beta") = beta, Named("niter") = niter, Named("trace") = trace, Named("ntrace") = (double)ntrace);
}
RcppExport SEXP admm_logit_enet_cv_state(SEXP x_, SEXP y_, SEXP lambda_, SEXP alpha_, SEXP fold_id_, SEXP nfolds_, SEXP fold_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    return glm_cv_state_call(admm_hip_logit_enet_cv_state, x_, y_, lambda_, alpha_, fold_id_, nfolds_, fold_, intercept_, opts_);
END_RCPP
}
RcppExport SEXP admm_poisson_cv_state(SEXP x_, SEXP y_, SEXP lambda_, SEXP alpha_, SEXP fold_id_, SEXP nfolds_, SEXP fold_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    return glm_cv_state_call(admm_hip_poisson_cv_state, x_, y_, lambda_, alpha_, fold_id_, nfolds_, fold_, intercept_, opts_);
END_RCPP
}

// The symbol R/50_admm_dantzig.R:38 asks for and the reference never builds (src/TODO/Dantzig.cpp:32-99): doubles throughout.
RcppExport SEXP admm_dantzig(SEXP x_, SEXP y_, SEXP lambda_, SEXP nlambda_, SEXP lmin_ratio_, SEXP standardize_, SEXP intercept_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericVector y(y_), lambda(lambda_);
    const int n = x.nrow(), p = x.ncol();
    const int nl_in = lambda.size();
    const int nl = nl_in > 0 ? nl_in : as<int>(nlambda_);
    admm_opts o = unpack_opts(opts_);
    NumericVector lambda_out(nl);
    IntegerVector niter(nl);
    // `beta` must be a dgCMatrix: R builds the result with do.call(ADMM_Dantzig_fit, res), and ADMM_Dantzig_fit contains
    // ADMM_Lasso_fit, whose field is beta = "dgCMatrix" (R/30_admm_lasso.R:18-21) -- a plain matrix would fail at object
    // construction.  TODO/Dantzig.cpp builds `SpMat beta(p + 1, nlambda)` through write_beta_matrix, row 0 always stored.
    std::vector<double> beta((size_t)(p + 1) * nl);
    check(admm_hip_dantzig(x.begin(), y.begin(), n, p, ADMM_MEM_HOST, nl_in > 0 ? lambda.begin() : nullptr, nl_in, as<int>(nlambda_),
                           as<double>(lmin_ratio_), as<bool>(standardize_), as<bool>(intercept_), &o, lambda_out.begin(), beta.data(),
                           niter.begin(), nullptr));
    return List::create(Named("lambda") = lambda_out, Named("beta") = to_dgCMatrix(beta, p + 1, nl), Named("niter") = niter);
END_RCPP
}

// Shared by admm_bp and admm_parbp: the p x 1 dgCMatrix of the non-zeros (BP.cpp:38-43, ParBP.cppp:58-61)
static Rcpp::S4 sparse_column(const std::vector<double>& b) {
    const int p = (int)b.size();
    std::vector<int> ii; std::vector<double> xx;
    for (int i = 0; i < p; ++i) if (b[i] != 0.0) { ii.push_back(i); xx.push_back(b[i]); }
    Rcpp::S4 m("dgCMatrix");
    m.slot("i") = IntegerVector(ii.begin(), ii.end());
    m.slot("p") = IntegerVector::create(0, (int)ii.size());
    m.slot("x") = NumericVector(xx.begin(), xx.end());
    m.slot("Dim") = IntegerVector::create(p, 1);
    return m;
}

// The symbol R/10_admm_bp.R:111 asks for and the reference never builds (src/TODO/ParBP.cppp:26-71): opts carries rho_ratio.
RcppExport SEXP admm_parbp(SEXP x_, SEXP y_, SEXP nthread_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericVector y(y_);
    List opts(opts_);
    admm_opts o;
    o.maxit = as<int>(opts["maxit"]); o.eps_abs = as<double>(opts["eps_abs"]); o.eps_rel = as<double>(opts["eps_rel"]);
    o.rho = as<double>(opts["rho_ratio"]);
    const int p = x.ncol();
    std::vector<double> b(p);
    int niter = 0;
    check(admm_hip_parbp(x.begin(), y.begin(), x.nrow(), p, ADMM_MEM_HOST, as<int>(nthread_), &o, b.data(), &niter, nullptr));
    return List::create(Named("beta") = sparse_column(b), Named("niter") = niter);
END_RCPP
}

RcppExport SEXP admm_bp(SEXP x_, SEXP y_, SEXP opts_) {
BEGIN_RCPP
    NumericMatrix x(x_);
    NumericVector y(y_);
    admm_opts o = unpack_opts(opts_);
    const int p = x.ncol();
    std::vector<double> b(p);
    int niter = 0;
    check(admm_hip_bp(x.begin(), y.begin(), x.nrow(), p, ADMM_MEM_HOST, &o, b.data(), &niter, nullptr));
    return List::create(Named("beta") = sparse_column(b), Named("niter") = niter);
END_RCPP
}

// Not in the reference (it keeps nothing between calls): libadmm_hip keeps EMPTY device blocks >= 32 MB for its next call
// (include/admm_hip.h, admm_hip_trim_memory).  The package would call this from .onUnload(libpath) -- and may offer it to users
// who share the GPU with other libraries:  .Call("admm_trim_memory", PACKAGE = "ADMM").
RcppExport SEXP admm_trim_memory() {
BEGIN_RCPP
    check(admm_hip_trim_memory());
    return R_NilValue;
END_RCPP
}
