// What a lambda-path call asks for and where its results go: built once by each extern "C" function (api.hip) from its arguments and
// handed down as they are.  The solvers keep taking LassoProblem (solvers.h), which PathSpec::problem() fills.
#pragma once
#include "solvers.h"
#include "sgl_host.h"
#include "box_host.h"

namespace admm {

struct PathSpec {
    const double* lambda_in = nullptr;   // the caller's grid (nlambda_in entries), or an automatic one of nlambda_auto values
    int nlambda_in = 0, nlambda_auto = 0;
    double lmin_ratio = 0;
    int standardize = 0, intercept = 0;
    double alpha = -1.0;                 // as the ABI passes it: >= 0 means elastic net (and then <= 1), anything else the plain Lasso
    const admm_opts* opts = nullptr;
    bool enet_only = false;              // admm_hip_enet has no Lasso form: it refuses a negative alpha too (R/40_admm_enet.R:38-39)
    // the tall-only penalties (solvers.h: Penalty): which one this call asks for, p (the length of the per-column arrays below), and the
    // arguments of each as the ABI passes them
    Penalty penalty = Penalty::PLAIN;
    int cols = 0;
    // GROUP, SGL: the group id of every column and the groups' weights; SGL: the mixing parameter (its own name: `alpha` above means
    // elastic net) and the l1 weight of every column (NULL: all 1)
    const int* group = nullptr; const double* group_weight = nullptr; int ngroups = 0;
    double sgl_mix = 0.0;
    const double* l1_weight = nullptr;
    // MULTITASK: the number of responses and the p row weights
    int nresp = 0;
    const double* row_weight = nullptr;
    // BOX: the bounds on the original coefficient scale and the penalty factors (each p long; NULL: no lower bounds / no upper bounds /
    // all factors 1); `alpha` above selects the prox
    const double* lower = nullptr; const double* upper = nullptr; const double* penalty_factor = nullptr;

    bool enet() const { return alpha >= 0.0; }
    double alpha_eff() const { return enet() ? alpha : 1.0; }
    int nlam() const { return nlambda_in > 0 ? nlambda_in : nlambda_auto; }
    void check() const {
        ADMM_REQUIRE(enet() ? alpha <= 1.0 : !enet_only, "alpha must be within [0, 1]");
        ADMM_REQUIRE(nlambda_in >= 0, "nlambda_in must be >= 0");
        ADMM_REQUIRE(nlambda_in > 0 ? lambda_in != nullptr : nlambda_auto > 0, "need a lambda grid or nlambda_auto > 0");
        if (nlambda_in == 0) ADMM_REQUIRE(lmin_ratio > 0 && lmin_ratio < 1, "lambda_min_ratio must be within (0, 1)");
        for (int i = 0; i < nlambda_in; ++i) ADMM_REQUIRE(lambda_in[i] > 0, "lambda must be positive");
    }
    // ... of a grouped call, once check_common has passed (p > 0): ids 0 .. ngroups - 1 in runs of at most ADMM_HIP_GROUP_MAX
    void check_group_ids(int p) const {
        ADMM_REQUIRE(group != nullptr, "group must not be NULL");
        ADMM_REQUIRE(group[0] == 0, "group ids must start at 0");
        int run = 1;
        for (int j = 1; j < p; ++j) {
            ADMM_REQUIRE(group[j] >= group[j - 1], "group ids must be non-decreasing (the columns of a group are adjacent)");
            ADMM_REQUIRE(group[j] <= group[j - 1] + 1, "group ids must have no gaps");
            run = group[j] == group[j - 1] ? run + 1 : 1;
            ADMM_REQUIRE(run <= ADMM_HIP_GROUP_MAX, "a group has more than ADMM_HIP_GROUP_MAX (1024) columns");
        }
        ADMM_REQUIRE(ngroups == group[p - 1] + 1, "ngroups does not match the group ids");
    }
    // ... of a group-lasso call: the ids, usable weights, n > p
    void check_groups(int n, int p) const {
        check_group_ids(p);
        bool any = group_weight == nullptr;
        for (int g = 0; group_weight != nullptr && g < ngroups; ++g) {
            ADMM_REQUIRE(std::isfinite(group_weight[g]) && group_weight[g] >= 0, "group weights must be finite and non-negative");
            any = any || group_weight[g] > 0;
        }
        ADMM_REQUIRE(any, "at least one group weight must be positive");
        ADMM_REQUIRE(n > p, "the group lasso is built for n > p only");
    }
    // ... of a sparse-group call: the ids, the mixing parameter in [0, 1], usable weights of both kinds, and a penalty that is not
    // identically zero (coordinate j of group g is penalised when alpha u_j > 0 or (1 - alpha) w_g > 0)
    void check_sgl_args(int p) const {
        check_group_ids(p);
        ADMM_REQUIRE(std::isfinite(sgl_mix) && sgl_mix >= 0.0 && sgl_mix <= 1.0, "the mixing parameter alpha must be finite and within [0, 1]");
        for (int g = 0; group_weight != nullptr && g < ngroups; ++g)
            ADMM_REQUIRE(std::isfinite(group_weight[g]) && group_weight[g] >= 0, "group weights must be finite and non-negative");
        for (int j = 0; l1_weight != nullptr && j < p; ++j)
            ADMM_REQUIRE(std::isfinite(l1_weight[j]) && l1_weight[j] >= 0, "l1 weights must be finite and non-negative");
        bool any = false;
        for (int j = 0; j < p && !any; ++j)
            any = sgl_mix * (l1_weight ? l1_weight[j] : 1.0) > 0 || (1.0 - sgl_mix) * (group_weight ? group_weight[group[j]] : 1.0) > 0;
        ADMM_REQUIRE(any, "at least one coordinate must carry a positive penalty");
    }
    // ... of a multi-task call, once check_common has passed: 1 <= m <= ADMM_HIP_MT_MAX, usable weights, n > p
    void check_mt(int n, int p) const {
        ADMM_REQUIRE(nresp >= 1 && nresp <= ADMM_HIP_MT_MAX, "the number of responses must be within [1, ADMM_HIP_MT_MAX (16)]");
        bool any = row_weight == nullptr;
        for (int j = 0; row_weight != nullptr && j < p; ++j) {
            ADMM_REQUIRE(std::isfinite(row_weight[j]) && row_weight[j] >= 0, "row weights must be finite and non-negative");
            any = any || row_weight[j] > 0;
        }
        ADMM_REQUIRE(any, "at least one row weight must be positive");
        ADMM_REQUIRE(n > p, "the multi-task lasso is built for n > p only");
    }
    // ... of a box-constrained call, once check_common has passed: a box that holds zero, usable factors, an alpha that names a prox
    // (check() lets NaN through as "the Lasso")
    void check_box_args(int p) const {
        for (int j = 0; lower != nullptr && j < p; ++j)
            ADMM_REQUIRE(lower[j] <= 0, "lower bounds must be <= 0 (zero must be feasible) and not NaN");
        for (int j = 0; upper != nullptr && j < p; ++j)
            ADMM_REQUIRE(upper[j] >= 0, "upper bounds must be >= 0 (zero must be feasible) and not NaN");
        bool any = penalty_factor == nullptr;
        for (int j = 0; penalty_factor != nullptr && j < p; ++j) {
            ADMM_REQUIRE(std::isfinite(penalty_factor[j]) && penalty_factor[j] >= 0, "penalty factors must be finite and non-negative");
            any = any || penalty_factor[j] > 0;
        }
        ADMM_REQUIRE(any, "at least one penalty factor must be positive");
        ADMM_REQUIRE(!std::isnan(alpha) && alpha <= 1.0, "alpha must be negative (the Lasso prox) or within [0, 1] (the elastic net's)");
    }
    // ... of the penalty this call asks for, once check_common has passed: its arguments, then n > p
    void check_penalty(int n, int p) const {
        switch (penalty) {
        case Penalty::PLAIN: break;
        case Penalty::GROUP: check_groups(n, p); break;
        case Penalty::SGL: check_sgl_args(p); ADMM_REQUIRE(n > p, "the sparse-group lasso is built for n > p only"); break;
        case Penalty::MULTITASK: check_mt(n, p); break;
        case Penalty::BOX:
            check_box_args(p);
            ADMM_REQUIRE(n > p, "the box-constrained elastic net is built for n > p only: the wide solver is not built for bounds");
            break;
        }
    }
    LassoProblem problem(int nworkers, bool dist) const {
        LassoProblem pb;
        pb.opts = *opts;
        pb.lambda_in.assign(lambda_in, lambda_in + nlambda_in);
        pb.nlambda_auto = nlambda_auto;
        pb.lmin_ratio = lmin_ratio;
        pb.enet = enet();
        pb.alpha = alpha_eff();
        pb.nworkers = nworkers;
        pb.dist = dist;
        pb.batch_iters = (int)opt_int(Opt::BATCH_ITERS, 0);
        pb.profile_stride = (int)opt_int(Opt::PROFILE_STRIDE, 0);
        pb.penalty = penalty;
        const double inf = std::numeric_limits<double>::infinity();
        switch (penalty) {                  // (checked: check_penalty)
        case Penalty::PLAIN: break;
        case Penalty::GROUP:
            pb.group_start = group_starts();
            for (int g = 0; g < ngroups; ++g)
                pb.group_weight.push_back(group_weight ? group_weight[g] : std::sqrt((double)(pb.group_start[g + 1] - pb.group_start[g])));
            break;
        case Penalty::SGL:                  // the device's weights, not the caller's
            pb.group_start = group_starts();
            sgl_prepare(sgl_mix, l1_weight, group_weight, pb.group_start, pb.l1_weight, pb.group_weight);
            break;
        case Penalty::MULTITASK:
            pb.nresp = nresp;
            for (int j = 0; j < cols; ++j) pb.row_weight.push_back(row_weight ? row_weight[j] : 1.0);
            break;
        case Penalty::BOX:
            for (int j = 0; j < cols; ++j) {
                pb.box_lower.push_back(lower ? lower[j] : -inf);
                pb.box_upper.push_back(upper ? upper[j] : inf);
                pb.penalty_factor.push_back(penalty_factor ? penalty_factor[j] : 1.0);
            }
            break;
        }
        return pb;
    }
    std::vector<int> group_starts() const {                       // group g holds columns [start[g], start[g + 1])
        std::vector<int> start;
        for (int j = 0; j < cols; ++j)
            if (j == 0 || group[j] != group[j - 1]) start.push_back(j);
        start.push_back(cols);
        return start;
    }
    PathSpec on_grid(const std::vector<double>& lam) const {      // the same call on a grid that an earlier fit fixed
        PathSpec s = *this;
        s.lambda_in = lam.data(); s.nlambda_in = (int)lam.size(); s.nlambda_auto = 0;
        return s;
    }
};

template <typename B>
struct PathOutT {
    double* lambda_out; B* beta_out; int* niter_out; admm_stats* stats;
    void require() const { ADMM_REQUIRE(lambda_out && beta_out && niter_out, "output pointers must not be NULL"); }
};
using PathOut = PathOutT<float>;

struct TraceOut {
    double* out = nullptr; long long cap = 0; long long* n_out = nullptr;
    void check() const { ADMM_REQUIRE(cap == 0 || (out != nullptr && n_out != nullptr && cap > 0), "bad trace arguments"); }
    void store(const std::vector<double>& trace) const {
        if (cap <= 0) return;
        std::memcpy(out, trace.data(), trace.size() * sizeof(double));
        *n_out = (long long)(trace.size() / ADMM_TRACE_FIELDS);
    }
};

}  // namespace admm
