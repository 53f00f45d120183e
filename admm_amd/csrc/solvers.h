// Solver entry points behind the C ABI (one per reference problem class).
#pragma once
#include "prep.h"
#include <algorithm>
#include <memory>

namespace admm {

// What is penalised besides the plain l1 norm (or the elastic net's): one of the tall-only penalties, single device, no REFINE.
enum class Penalty { PLAIN, GROUP, SGL, MULTITASK, BOX };

struct LassoProblem {
    admm_opts opts{};
    std::vector<double> lambda_in;   // user grid (may be empty -> automatic)
    int nlambda_auto = 100;
    double lmin_ratio = 1e-4;
    bool enet = false;
    double alpha = 1.0;
    int nworkers = 0;                // > 0: row-block consensus (admm_parlasso)
    bool dist = false;               // consensus blocks / rows of the tall solver spread over the ranks of the attached communicator
    long long p_total = 0;           // > 0: COLUMN-sharded wide solver -- this rank holds columns [col_offset, col_offset + p) of p_total
    long long col_offset = 0;
    int batch_iters = 0;             // iterations enqueued per host poll (0 = default)
    int profile_stride = 0;          // > 0: time every stride-th x-update launch with HIP events
    // the tall-only penalty; each kind fills its own vectors below and leaves the others empty
    Penalty penalty = Penalty::PLAIN;
    // GROUP (admm_hip_grplasso): group g holds columns [group_start[g], group_start[g + 1]) and is penalised by group_weight[g] * its
    // Euclidean norm.  SGL (admm_hip_sgl; sgl_host.h): group_weight holds wg_g = (1 - alpha) w_g and l1_weight [p] l1_j = alpha u_j
    std::vector<int> group_start;
    std::vector<double> group_weight, l1_weight;
    // MULTITASK (admm_hip_mtlasso): nresp responses share the design (DeviceData.Ymt), row j of the p x nresp coefficient matrix is
    // penalised by row_weight[j] * its Euclidean norm
    int nresp = 0;
    std::vector<double> row_weight;
    // BOX (admm_hip_boxenet; box_host.h): box_lower / box_upper [p] are the caller's bounds on the ORIGINAL coefficient scale (+-infinity
    // where there is none), penalty_factor [p] the factors u_j; `enet` / `alpha` above select the prox as for admm_hip_lasso / admm_hip_enet
    std::vector<double> box_lower, box_upper, penalty_factor;
};

struct LassoResult {
    std::vector<double> lambda;
    std::vector<float> beta;         // (p+1) x nlambda column-major, row 0 = intercept
    std::vector<int> niter;
    admm_stats stats{};
    // optional: the caller's coefficient buffer ((p+1) x nlambda floats).  A solver that fills it directly sets beta_written and leaves
    // `beta` empty (the wide solver: its coefficient matrix is 80 MB of mostly zeros at BASELINE configs[2])
    float* beta_dst = nullptr;
    bool beta_written = false;
};

// Lasso.cpp:78-89
std::vector<double> make_lambda_grid(const LassoProblem& pb, double lambda0, int n, double scaleY);

// Read-out of a device-side recorder (decision trace or iterate dump, `rec_len` values per record): the first min(taken, capacity, cap)
// records, where `taken` is the number of decisions the loop took and `capacity` what the recorder was given.  Returns how many.
template <typename T>
long long read_records(T* out, long long cap, const T* dev, long long rec_len, long long taken, long long capacity, hipStream_t st) {
    const long long nrec = std::min(std::min(taken, capacity), cap);
    if (nrec > 0) read_back(out, dev, (size_t)nrec * rec_len * sizeof(T), st);
    return nrec;
}
template <typename T>      // ... into a result's vector, sized to what was recorded
void collect_records(std::vector<T>& out, const T* dev, long long rec_len, long long taken, long long capacity, hipStream_t st) {
    out.assign((size_t)(std::max(std::min(taken, capacity), 0ll) * rec_len), T(0));
    read_records(out.data(), capacity, dev, rec_len, taken, capacity, st);
}

// A prepared problem: construction does the one-time work (X'y, Gram, rho, factorisation ...),
// run() executes one cold-started warm-chained lambda path and may be called repeatedly.
struct LassoPlan {
    virtual ~LassoPlan() = default;
    virtual void run(LassoResult& res) = 0;
    // The recorders, written once for every plan: the per-decision trace of the iteration control (admm_hip_lasso_plan_trace_*) and the
    // per-iteration iterate dump (admm_hip_lasso_plan_state_*), record s = the iterates trace record s judged.  A plan supplies its
    // stream, the floats of one iterate record and where its parameter block takes the buffers and their capacities (records()), and
    // sets `decisions` at the end of run() by its own rule.
    struct Records { hipStream_t st; long long rec_floats; double** trace; long long* trace_cap; float** state; long long* state_cap; };
    virtual Records records() = 0;
    void enable_trace(long long cap) {
        const Records r = records();
        trace_buf.alloc((size_t)cap * ADMM_TRACE_FIELDS);
        decisions = 0;
        *r.trace = trace_buf.get(); *r.trace_cap = cap;
    }
    long long read_trace(double* out, long long cap) {
        const Records r = records();
        return read_records(out, cap, trace_buf.get(), ADMM_TRACE_FIELDS, decisions, *r.trace_cap, r.st);
    }
    void enable_state(long long cap) {
        const Records r = records();
        state_buf.alloc((size_t)cap * r.rec_floats);
        // on the solver's own (non-blocking) stream: a null-stream memset is not ordered against it and, on a busy device, landed
        // AFTER run() had copied record 0 into the dump (suspected cause of the one unreadable record 0 of the 40-process soak, case 546:23)
        state_buf.zero(r.st);
        *r.state = state_buf.get(); *r.state_cap = cap;
    }
    long long read_state(float* out, long long cap, long long* rec_floats) {
        const Records r = records();
        if (rec_floats) *rec_floats = r.rec_floats;
        if (!out) return std::min(decisions, *r.state_cap);                          // size query
        return read_records(out, cap, state_buf.get(), r.rec_floats, decisions, *r.state_cap, r.st);      // one record per decision, same numbering as the trace
    }
    // the float system matrix X'X + rho I the x-update solves, p x p column-major (admm_hip_lasso_plan_system_read): only
    // the tall solver with ADMM_HIP_REFINE=1 keeps it
    // the standardised data (X n x p column-major with leading dimension ld, Y) as the solver holds them (admm_hip_lasso_plan_data_read): wide solver
    virtual void read_data(float*, long long, float*) { throw Error(ADMM_ERR_INVALID_ARG, "this plan does not keep its standardised data (wide solver only)"); }
    virtual void read_system(float*, long long) { throw Error(ADMM_ERR_INVALID_ARG, "this plan does not keep its system matrix (tall solver with ADMM_HIP_REFINE=1 only)"); }
protected:
    long long decisions = 0;         // decisions the last run() took: records of the trace and the dump that are valid
    DevBuf<double> trace_buf;
    DevBuf<float> state_buf;
};
std::unique_ptr<LassoPlan> make_tall_plan(DeviceData<float>&& d, const LassoProblem& pb, hipStream_t st);
std::unique_ptr<LassoPlan> make_wide_plan(DeviceData<float>&& d, const LassoProblem& pb, hipStream_t st);
std::unique_ptr<LassoPlan> make_par_plan(DeviceData<float>&& d, const LassoProblem& pb, hipStream_t st);

struct DenseResult {
    std::vector<double> beta;
    int niter = 0;
    admm_stats stats{};
    long long trace_cap = 0;         // > 0: record up to this many decisions (admm_hip_lad_traced / admm_hip_bp_traced)
    std::vector<double> trace;       // [nrec][ADMM_TRACE_FIELDS]
    long long state_cap = 0;         // > 0: also dump the iterates of up to this many decisions (admm_hip_lad_state / admm_hip_bp_state)
    std::vector<double> state;       // [nrec][5][state_dim]  x | z | y | adj_z | adj_y
    long long state_dim = 0;
};
void solve_lad(const DeviceData<double>& d, const admm_opts& opts, DenseResult& res, hipStream_t st);
void solve_bp(const DeviceData<double>& d, const admm_opts& opts, DenseResult& res, hipStream_t st);
// admm_hip_quantreg (fadmm_dense.hip): LAD's loop with the prox of the check loss, one cold-started loop per quantile on ONE setup;
// on the one-pass branch several quantiles per pass over X (QUANT_SLOTS).  d: the standardised data (DataStd flag 3 with the
// intercept, 1 without); with the intercept the loop fits a further column of ones, which solve_quantreg appends to d.X.
// beta: (p + 1) x ntau column-major, row 0 = intercept.  dense: stats, and for a single quantile the trace / iterate dump.
struct QuantResult {
    DenseResult dense;
    std::vector<double> beta;
    std::vector<int> niter;
};
void solve_quantreg(DeviceData<double>& d, bool intercept, const admm_opts& opts, const double* tau, int ntau, QuantResult& res, hipStream_t st);
// admm_hip_huber (fadmm_dense.hip): the same scaffolding with the Huber form of the prox, one fit per (delta[k], tau[k]); delta in the
// units of y (the loop uses delta / scaleY), +inf = expectile regression.
void solve_huber(DeviceData<double>& d, bool intercept, const admm_opts& opts, const double* delta, const double* tau, int nfit, QuantResult& res,
                 hipStream_t st);
// admm_hip_logit (fadmm_dense.hip): logistic regression as LAD's loop on diag(2 y - 1) [X | 1] with a zero response and the Newton prox
// of log(1 + e^-z).  d: the standardised data as for solve_quantreg (its Y is zeroed, its X sign-folded); y_dev: the caller's labels on
// the device, exactly 0.0 / 1.0 with both classes present (logit_count_labels counts the offenders and the ones).  res.beta: p + 1.
void solve_logit(DeviceData<double>& d, bool intercept, const double* y_dev, const admm_opts& opts, DenseResult& res, hipStream_t st);
void logit_count_labels(const double* y_dev, int n, long long* bad, long long* ones, hipStream_t st);
// admm_hip_logit_multi (fadmm_dense.hip): ncol label columns on ONE setup.  The matrix stays unfolded ([X | 1], zero response) and the
// prox takes the row's sign itself, so the setup is shared and, on the one-pass branch, several columns advance per pass over X
// (QUANT_SLOTS, as solve_huber).  y_dev: n x ncol labels on the device (leading dimension n), every column validated as solve_logit's.
// res.beta: (p + 1) x ncol, res.niter: ncol; column k equals solve_logit on column k.
void solve_logit_multi(DeviceData<double>& d, bool intercept, const double* y_dev, int ncol, const admm_opts& opts, QuantResult& res, hipStream_t st);
// admm_hip_logit_ridge (fadmm_dense.hip): the same with the ridge penalty lambda / 2 sum b_j^2 on the standardised coefficients (never the
// intercept), as p more rows sqrt(lambda) e_j' with a zero response and a square loss (kProxLogitR), so the cached inverse does not
// depend on rho.  One upload, standardisation, data-row Gram matrix and transpose per call; per lambda (in the order given, every fit
// cold) the inverse and the ncol columns.  No n > p condition.  res.beta: (p + 1) x ncol x nlambda, res.niter: ncol x nlambda; dense: the
// stats, and for one column and one lambda the trace / iterate dump of the augmented loop (n + p rows).
void solve_logit_ridge(DeviceData<double>& d, bool intercept, const double* y_dev, int ncol, const double* lambda, int nlambda, const admm_opts& opts, QuantResult& res,
                       hipStream_t st);
// admm_hip_logit_enet (fadmm_dense.hip): the same with the elastic-net penalty lambda (alpha sum |b_j| + (1 - alpha) / 2 sum b_j^2), as p
// more rows sqrt(n) e_j' whose loss carries the cell's constants (kProxLogitE): ONE Gram matrix, inverse and transpose per call, and the
// ncol x ncell fits (cell-major) as one grid of run_lad_fits.  The penalised coefficients are read from the penalty rows of the last z
// (exact zeros), the intercept from get_x.  res.beta: (p + 1) x ncol x ncell, res.niter: ncol x ncell; dense: as solve_logit_ridge.
void solve_logit_enet(DeviceData<double>& d, bool intercept, const double* y_dev, int ncol, const double* lambda, const double* alpha, int ncell, const admm_opts& opts,
                      QuantResult& res, hipStream_t st);
// out[c] = max_j |x_j'(y_c - mean[c])| over the columns of d (standardised, before any ones column); y_dev: n x ncol on the device,
// mean / out: ncol host values
void logit_enet_lambda_one(const DeviceData<double>& d, const double* y_dev, int ncol, const double* mean, double* out, hipStream_t st);
// admm_hip_poisson (fadmm_dense.hip): solve_logit_enet with the Poisson loss exp(eta) - y eta on the data rows (kProxPoisE): the count
// matrix stands where the sign matrix stood, -1.0 marking the penalty rows.  y_dev: n x ncol validated counts (finite, >= 0) on the
// device, leading dimension n.  lambda >= 0 (0: the plain GLM, the caller checks n > p + intercept).  res as solve_logit_enet's.
void solve_poisson(DeviceData<double>& d, bool intercept, const double* y_dev, int ncol, const double* lambda, const double* alpha, int ncell, const admm_opts& opts,
                   QuantResult& res, hipStream_t st);
// admm_hip_logit_enet_cv / admm_hip_poisson_cv (fadmm_dense.hip): solve_logit_enet / solve_poisson with the folds as further columns of
// the tag matrix -- a held-out row carries a tag whose prox is the identity, so every fold's fit runs on the full-data matrix, Gram
// matrix, inverse and transpose.  folds.id: n validated fold ids in [0, nfolds).  Slots: 0 = nothing held out, s >= 1 = fold s - 1;
// res.beta: (p + 1) x ncol x (nfolds + 1) x ncell, res.niter: ncol x (nfolds + 1) x ncell (cell-major, then slot, then column).
// fold_dev (may be NULL): nfolds x ncell x ncol, the mean held-out deviance of fold f under its own fit, formed on the device.
// folds.single >= -1: ONE slot, holding out that fold (-1: none) -- the state forms; no deviance.
struct GlmFolds {
    const std::vector<int>* id = nullptr;
    int nfolds = 0;
    int single = -2;
};
void solve_glm_cv(bool pois, DeviceData<double>& d, bool intercept, const double* y_dev, int ncol, const GlmFolds& folds, const double* lambda, const double* alpha, int ncell,
                  const admm_opts& opts, QuantResult& res, std::vector<double>* fold_dev, hipStream_t st);
// one reduction per column of the n x ncol counts on the device: *bad = the entries that are not finite or lie below zero (all columns),
// sums[c] = column c's sum (ncol host values; the same bits on every run)
void pois_column_stats(const double* y_dev, int n, int ncol, long long* bad, double* sums, hipStream_t st);
// admm_dantzig (dantzig.hip): the Dantzig selector path in double.  res.beta: (p + 1) x nlambda column-major, row 0 = intercept.
struct DantzigResult {
    std::vector<double> lambda, beta;
    std::vector<int> niter;
    admm_stats stats{};
    long long trace_cap = 0;
    std::vector<double> trace;
};
void solve_dantzig(DeviceData<double>& d, const LassoProblem& pb, DantzigResult& res, hipStream_t st);
// admm_parbp: basis pursuit with the columns in `nblocks` blocks (sharing ADMM, sharing_bp.hip).  d holds this rank's columns
// [col_offset, col_offset + d.p) of p_total (whole blocks); opts.rho carries rho_ratio.  res.beta: this rank's coefficients.
void solve_parbp(const DeviceData<double>& d, const admm_opts& opts, int nblocks, long long p_total, long long col_offset,
                 DenseResult& res, hipStream_t st);

}  // namespace admm
