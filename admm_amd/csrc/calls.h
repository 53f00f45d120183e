// What the C boundary (api.hip) calls: plan creation and path runs, the replica drivers (multi-response here, cross-validation in
// cv.hip), the dense solvers and the Dantzig selector.  Everything takes the call as call_args.h describes it and throws Error.
#pragma once
#include "call_args.h"

namespace admm {

void check_common(const double* x, const double* y, int n, int p, int mem, const admm_opts* opts);

// How the caller's data are spread over the ranks of the attached communicator (or of an in-process group).
struct Shard {
    enum Kind { NONE, ROWS, COLS } kind = NONE;
    long long n_total = 0, ldx = 0;            // ROWS: rows of the whole problem; ldx > n: x is a row slice of a matrix with this leading dimension
    long long p_total = 0, col_offset = 0;     // COLS: this rank holds columns [col_offset, col_offset + p) of p_total (the wide solver)
    static Shard rows(long long n_total, long long ldx = 0) { Shard s; s.kind = ROWS; s.n_total = n_total; s.ldx = ldx; return s; }
    static Shard cols(long long p_total, long long col_offset) { Shard s; s.kind = COLS; s.p_total = p_total; s.col_offset = col_offset; return s; }
};

struct PlanHandle {
    Stream st;
    std::unique_ptr<LassoPlan> plan;
    int p = 0, nlam = 0;
    int nresp = 1;                             // coefficient columns per lambda (admm_hip_mtlasso: its responses)
    double t_create = 0;
};
// nworkers > 0: the row-block consensus solver; otherwise the tall or the wide one by shape (Lasso.cpp:73)
PlanHandle* create_plan(const double* x, const double* y, int n, int p, int mem, const PathSpec& spec, int nworkers, const Shard& shard = Shard());
void run_plan(PlanHandle* h, const PathOut& out, double t_extra);
// create_plan + run_plan: admm_hip_lasso / _enet and the _dist entry points
void lasso_family(const double* x, const double* y, int n, int p, int mem, const PathSpec& spec, int nworkers, const Shard& shard, const PathOut& out);
// admm_hip_parlasso: over in-process ranks when PAR_DEVICES lists several devices, else lasso_family
void parlasso(const double* x, const double* y, int n, int p, int mem, const PathSpec& spec, int nthread, const PathOut& out);

// The replica drivers (cross-validation folds, responses) keep one resident double copy of host input; device input is used in place.
struct Resident {
    DevBuf<double> own;
    const double* p;
    Resident(const double* src, size_t count, int mem) : p(src) {
        if (mem != ADMM_MEM_HOST) return;
        own.alloc(count);
        write_device(own.get(), src, count * sizeof(double));
        p = own.get();
    }
};
// ... and deal their units out to the ranks (unit u on rank u mod nranks, zeroed tables elsewhere): the results are the sums over
// the ranks of the double tables a and b (equal length) and of the nf host floats at f (may be NULL).  One rank: nothing to do.
void sum_over_ranks(std::vector<double>& a, std::vector<double>& b, float* f, size_t nf, hipStream_t st);

void lasso_multi(const double* x, const double* Y, int n, int p, int m, int mem, const PathSpec& spec, const PathOut& out);
struct CvOut { double* cv_mean; double* cv_se; double* fold_mse; int* fold_niter; float* fold_beta; int* idx_min; int* idx_1se; };
void lasso_cv(const double* x, const double* y, int n, int p, int mem, const int* fold_id, int nfolds, const PathSpec& spec,
              const PathOut& out, const CvOut& cv);

// Iterate dump of a LAD / BP run (admm_hip_lad_state / admm_hip_bp_state)
struct StateOut { double* out = nullptr; long long cap = 0; long long* n_out = nullptr; };
struct DenseOut { double* beta_out; int* niter_out; admm_stats* stats; TraceOut trace = {}; StateOut state = {}; };
void lad(const double* x, const double* y, int n, int p, int mem, int intercept, const admm_opts* opts, const DenseOut& out);
// out.beta_out: (p + 1) x ntau, out.niter_out: ntau; trace / state for ntau = 1 only
void quantreg(const double* x, const double* y, int n, int p, int mem, int intercept, const double* tau, int ntau, const admm_opts* opts, const DenseOut& out);
// tau = NULL: 0.5 for every fit; out as quantreg's with nfit columns
void huber(const double* x, const double* y, int n, int p, int mem, int intercept, const double* delta, const double* tau, int nfit, const admm_opts* opts,
           const DenseOut& out);
// y: labels, exactly 0.0 or 1.0, both present; out.beta_out: p + 1, out.niter_out: 1
void logit(const double* x, const double* y, int n, int p, int mem, int intercept, const admm_opts* opts, const DenseOut& out);
// y: n x k labels, column-major, every column as logit's; out.beta_out: (p + 1) x k, out.niter_out: k; no trace / state
void logit_multi(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const admm_opts* opts, const DenseOut& out);
// the same with a ridge penalty: nlambda values, used in the order given; out.beta_out: (p + 1) x k x nlambda, out.niter_out: k x nlambda;
// trace / state for k = 1 and nlambda = 1 only
void logit_ridge(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const double* lambda, int nlambda, const admm_opts* opts,
                 const DenseOut& out);
// the same with the elastic-net penalty: ncell (lambda, alpha) pairs, used in the order given, all on one inverse; out.beta_out:
// (p + 1) x k x ncell, out.niter_out: k x ncell; trace / state for k = 1 and ncell = 1 only
void logit_enet(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const double* lambda, const double* alpha, int ncell,
                const admm_opts* opts, const DenseOut& out);
// out[k]: per label column max_j |x~_j'(y_c - mean)| on the standardised columns (lambda_max of a cell is this over its alpha)
void logit_enet_lambda_max(const double* x, const double* y, int n, int p, int k, int mem, int intercept, double* out);
// admm_hip_poisson: the same call shape with count columns (finite, >= 0, a positive sum each) and the Poisson likelihood; lambda >= 0
// (0: the plain GLM, n > p + intercept); trace / state for k = 1 and ncell = 1 only
void poisson(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const double* lambda, const double* alpha, int ncell,
             const admm_opts* opts, const DenseOut& out);
// out[k]: per count column max_j |x~_j'(y_c - mean(y_c))| with the intercept, max_j |x~_j'(y_c - 1)| without it
void poisson_lambda_max(const double* x, const double* y, int n, int p, int k, int mem, int intercept, double* out);
// admm_hip_logit_enet_cv / admm_hip_poisson_cv: K-fold cross-validation of the (column, cell) grid on the full-data setup.  fold_id: n
// host ints in [0, nfolds), or NULL = i mod nfolds.  fold < -1: the grid call -- out: the full-data fit as logit_enet's / poisson's, cv:
// the tables (k x ncell; fold_*: fold-major, may be NULL; idx_*: k, may be NULL).  fold >= -1: the state form, k = ncell = 1, ONE fit
// holding out that fold (-1: none); cv is not read.
struct GlmCvOut { double* cv_mean; double* cv_se; double* fold_dev; int* fold_niter; double* fold_beta; int* idx_min; int* idx_1se; };
void glm_cv(bool pois, const double* x, const double* y, int n, int p, int k, int mem, int intercept, const int* fold_id, int nfolds, int fold, const double* lambda,
            const double* alpha, int ncell, const admm_opts* opts, const DenseOut& out, const GlmCvOut& cv);
void bp(const double* x, const double* y, int n, int p, int mem, const admm_opts* opts, const DenseOut& out);
// admm_hip_parbp(_traced): over in-process ranks when PAR_DEVICES lists several devices; parbp_dist: this rank's columns of p_total
void parbp(const double* x, const double* y, int n, int p, int mem, int nthread, const admm_opts* opts, const DenseOut& out);
void parbp_dist(const double* x_cols, const double* y, int n, int p_local, long long p_total, long long col_offset, int mem, int nthread,
                const admm_opts* opts, const DenseOut& out);
void dantzig(const double* x, const double* y, int n, int p, int mem, const PathSpec& spec, const PathOutT<double>& out, const TraceOut& trace);

}  // namespace admm
