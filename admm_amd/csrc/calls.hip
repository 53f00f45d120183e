// The calls behind the C boundary (calls.h): lambda grid, plan creation and runs, the multi-response driver, the dense solvers.
#include "calls.h"
#include "comm.h"
#include "inproc.h"
#include <cmath>

namespace admm {

std::vector<double> make_lambda_grid(const LassoProblem& pb, double lambda0, int n, double scaleY) {
    if (!pb.lambda_in.empty()) return pb.lambda_in;
    // Lasso.cpp:78-89: lmax = lambda0 / n * scaleY; log-spaced down to lmin_ratio * lmax
    const int nl = pb.nlambda_auto;
    const double lmax = lambda0 / n * scaleY;
    const double lmin = pb.lmin_ratio * lmax;
    std::vector<double> lam(nl);
    const double lo = std::log(lmax), hi = std::log(lmin);
    for (int i = 0; i < nl; ++i) {
        const double t = nl > 1 ? lo + (hi - lo) * ((double)i / (double)(nl - 1)) : lo;
        lam[i] = std::exp(i == nl - 1 && nl > 1 ? hi : t);
    }
    return lam;
}

void check_common(const double* x, const double* y, int n, int p, int mem, const admm_opts* opts) {
    ADMM_REQUIRE(x != nullptr && y != nullptr, "x and y must not be NULL");
    ADMM_REQUIRE(n > 0 && p > 0, "n and p must be positive");
    ADMM_REQUIRE(mem == ADMM_MEM_HOST || mem == ADMM_MEM_DEVICE, "mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE");
    ADMM_REQUIRE(opts != nullptr, "opts must not be NULL");
    ADMM_REQUIRE(opts->maxit > 0, "maxit should be positive");                                  // R/30_admm_lasso.R:119-120
    ADMM_REQUIRE(opts->eps_abs >= 0 && opts->eps_rel >= 0, "eps_abs and eps_rel should be nonnegative");
}

// What create_plan says about each tall-only penalty, by Penalty: its name, its refusal of REFINE (the sparse-group lasso answers as
// the group lasso) and its refusal of an attached communicator (NULL: not refused -- the two grouped calls do not look)
namespace {
struct PenaltyText { const char* name; const char* refine; const char* comm; };
const PenaltyText kPenaltyText[] = {
    {"the Lasso", nullptr, nullptr},
    {"the group lasso", "the group lasso has no refined x-update: unset REFINE", nullptr},
    {"the sparse-group lasso", "the group lasso has no refined x-update: unset REFINE", nullptr},
    {"the multi-task lasso", "the multi-task lasso has no refined x-update: unset REFINE",
     "the multi-task lasso runs on a single device: detach the communicator (admm_hip_comm_finalize)"},
    {"the box-constrained elastic net", "the box-constrained elastic net has no refined x-update: unset REFINE",
     "the box-constrained elastic net runs on a single device: detach the communicator (admm_hip_comm_finalize)"},
};
}  // namespace

PlanHandle* create_plan(const double* x, const double* y, int n, int p, int mem, const PathSpec& spec, int nworkers, const Shard& shard) {
    const bool rows = shard.kind == Shard::ROWS, cols = shard.kind == Shard::COLS;
    if (rows) ADMM_REQUIRE(shard.n_total >= n && n > 0, "n_total must be >= n_local > 0");
    check_common(x, y, n, p, mem, spec.opts);
    spec.check();
    if (cols) {
        ADMM_REQUIRE(shard.p_total >= p && shard.col_offset >= 0 && shard.col_offset + p <= shard.p_total, "column block outside [0, p_total)");
        ADMM_REQUIRE(shard.p_total < (1ll << 31) - 1, "p_total too large");
        ADMM_REQUIRE((long long)n <= shard.p_total, "the column-sharded solver is the wide one: it needs n <= p_total (Lasso.cpp:73)");
        ADMM_REQUIRE(comm_info().active, "no communicator: call admm_hip_comm_init first");
    } else if (rows) {
        ADMM_REQUIRE(nworkers >= 0, "nthread must be >= 0");
        ADMM_REQUIRE(comm_info().active, "no communicator: call admm_hip_comm_init first");
        if (nworkers == 0) ADMM_REQUIRE(shard.n_total > p, "the row-sharded serial solver is the tall one: it needs n_total > p");
    } else if (nworkers > 0) {
        ADMM_REQUIRE(nworkers <= n, "more row blocks than rows");
    }
    if (spec.penalty != Penalty::PLAIN) {                   // the tall solver on one device, nothing else (MULTITASK: y is Y, n x m)
        const PenaltyText& t = kPenaltyText[(int)spec.penalty];
        ADMM_REQUIRE(shard.kind == Shard::NONE && nworkers <= 0 && (spec.penalty == Penalty::BOX || !spec.enet()),
                     std::string("internal: ") + t.name + " has no sharded or consensus form, and only the box an elastic-net one");
        spec.check_penalty(n, p);
        ADMM_REQUIRE(!opt_on(Opt::REFINE), t.refine);
        ADMM_REQUIRE(t.comm == nullptr || !comm_info().active, t.comm);
    }
    require_device();
    const double t0 = now_s();
    std::unique_ptr<PlanHandle> h(new PlanHandle());
    LassoProblem pb = spec.problem(cols ? 0 : nworkers, rows);
    if (cols) { pb.p_total = shard.p_total; pb.col_offset = shard.col_offset; pb.profile_stride = 0; }
    DeviceData<float> d;
    const bool std_x = spec.standardize != 0, icpt = spec.intercept != 0;
    // Host input of a large tall problem: standardisation and X'X run under the PCIe transfer (bit-identical result).
    const bool pipelined = mem == ADMM_MEM_HOST && shard.kind == Shard::NONE && nworkers <= 0 && n > p && p >= 4096 && !opt_set(Opt::GRAM) && spec.penalty != Penalty::MULTITASK;
    if (pipelined) upload_standardize_gram_f32(d, x, y, n, p, std_x, icpt, h->st.s);
    else upload_standardize<float>(d, x, y, n, p, mem, std_x, icpt, h->st.s, shard.n_total, shard.ldx);   // COLS: column moments are local, y is replicated
    if (spec.penalty == Penalty::MULTITASK) {               // X went up with the first response; now all of them, standardised together
        const Resident yr(y, (size_t)n * spec.nresp, mem);
        if (mem == ADMM_MEM_HOST) comm_stream_sync(h->st.s);
        standardize_responses_f32(d, yr.p, spec.nresp, h->st.s);
        h->nresp = spec.nresp;
    }
    if (cols) h->plan = make_wide_plan(std::move(d), pb, h->st.s);
    else if (nworkers > 0) h->plan = make_par_plan(std::move(d), pb, h->st.s);
    else if ((rows ? shard.n_total : (long long)n) > p) h->plan = make_tall_plan(std::move(d), pb, h->st.s);      // Lasso.cpp:73
    else h->plan = make_wide_plan(std::move(d), pb, h->st.s);
    h->p = cols ? (int)shard.p_total : p;
    h->nlam = spec.nlam();
    h->t_create = now_s() - t0;
    return h.release();
}

void run_plan(PlanHandle* h, const PathOut& out, double t_extra) {
    ADMM_REQUIRE(h != nullptr && h->plan, "plan is NULL");
    out.require();
    const double t0 = now_s();
    LassoResult res;
    res.beta_dst = out.beta_out;
    h->plan->run(res);
    const int nl = (int)res.lambda.size();
    for (int i = 0; i < nl; ++i) { out.lambda_out[i] = res.lambda[i]; out.niter_out[i] = res.niter[i]; }
    if (!res.beta_written) std::memcpy(out.beta_out, res.beta.data(), sizeof(float) * (size_t)(h->p + 1) * h->nresp * nl);
    res.stats.t_total = now_s() - t0 + t_extra;
    if (out.stats) *out.stats = res.stats;
}

void lasso_family(const double* x, const double* y, int n, int p, int mem, const PathSpec& spec, int nworkers, const Shard& shard, const PathOut& out) {
    out.require();
    std::unique_ptr<PlanHandle> h(create_plan(x, y, n, p, mem, spec, nworkers, shard));
    run_plan(h.get(), out, h->t_create);
}

void parlasso(const double* x, const double* y, int n, int p, int mem, const PathSpec& spec, int nthread, const PathOut& out) {
    ADMM_REQUIRE(nthread >= 1, "nthread must be >= 1");
    const std::vector<int> devs = par_devices_for(nthread);
    if (devs.empty()) {
        record_single_layout();
        lasso_family(x, y, n, p, mem, spec, nthread, Shard(), out);
        return;
    }
    // in-process ranks: rank r holds the rows of its K / N whole blocks (admm_amd/dist.py row_partition)
    out.require();
    check_common(x, y, n, p, mem, spec.opts);
    spec.check();
    ADMM_REQUIRE(nthread <= n, "more row blocks than rows");
    const int nl = spec.nlam();
    run_inproc(devs, input_device(x, mem), [&](int rank, int nranks) {
        const long long chunk = n / nthread, per = nthread / nranks;
        const long long lo = rank * per * chunk, hi = rank == nranks - 1 ? n : (rank + 1) * per * chunk;
        std::vector<double> lam_own; std::vector<float> beta_own; std::vector<int> nit_own;
        admm_stats st_own;
        PathOut mine = out;
        if (rank != 0) {                                  // every rank computes the full result; the caller gets rank 0's
            lam_own.resize(nl); beta_own.resize((size_t)(p + 1) * nl); nit_own.resize(nl);
            mine = PathOut{lam_own.data(), beta_own.data(), nit_own.data(), &st_own};
        }
        lasso_family(x + lo, y + lo, (int)(hi - lo), p, mem, spec, nthread, Shard::rows(n, n), mine);
    });
}

void sum_over_ranks(std::vector<double>& a, std::vector<double>& b, float* f, size_t nf, hipStream_t st) {
    const CommInfo ci = comm_info();
    if (!ci.active || ci.nranks <= 1) return;
    const size_t na = a.size();
    DevBuf<double> t(2 * na);
    ADMM_HIP_CHECK(hipMemcpyAsync(t.get(), a.data(), na * sizeof(double), hipMemcpyHostToDevice, st));
    ADMM_HIP_CHECK(hipMemcpyAsync(t.get() + na, b.data(), na * sizeof(double), hipMemcpyHostToDevice, st));
    allreduce_sum_f64(t.get(), 2 * na, st);
    ADMM_HIP_CHECK(hipMemcpyAsync(a.data(), t.get(), na * sizeof(double), hipMemcpyDeviceToHost, st));
    ADMM_HIP_CHECK(hipMemcpyAsync(b.data(), t.get() + na, na * sizeof(double), hipMemcpyDeviceToHost, st));
    comm_stream_sync(st);
    comm_check();
    if (!f) return;
    DevBuf<float> fb(nf);
    ADMM_HIP_CHECK(hipMemcpyAsync(fb.get(), f, nf * sizeof(float), hipMemcpyHostToDevice, st));
    allreduce_sum_f32(fb.get(), nf, st);
    read_back(f, fb.get(), nf * sizeof(float), st);
    comm_stream_sync(st);
    comm_check();
}

// Several responses of one design matrix ("batched / multi-response"): response j is the ordinary
// fit of (x, Y[:, j]) -- bit-identical to admm_hip_lasso / admm_hip_enet on that pair -- but x is uploaded, converted and
// standardised once, and for the tall solver X'X is formed once (it does not depend on y; the cached inverse does, through
// rho, and is rebuilt per response).  With a communicator the responses are dealt out to the ranks (response j on rank
// j mod nranks, independent replicas) and the outputs are summed over the ranks at the end.
void lasso_multi(const double* x, const double* Y, int n, int p, int m, int mem, const PathSpec& spec, const PathOut& out) {
    check_common(x, Y, n, p, mem, spec.opts);
    ADMM_REQUIRE(m >= 1, "the number of responses must be >= 1");
    out.require();
    spec.check();
    require_device();
    const int nlam = spec.nlam();
    const size_t bsz = (size_t)(p + 1) * nlam;
    Stream st;
    const Resident xr(x, (size_t)n * p, mem), yr(Y, (size_t)n * m, mem);
    if (mem == ADMM_MEM_HOST) comm_stream_sync(st.s);
    const double* xd = xr.p; const double* yd = yr.p;
    const CommInfo ci = comm_info();
    const int nranks = ci.active ? ci.nranks : 1, rank = ci.active ? ci.rank : 0;
    std::vector<double> lam((size_t)m * nlam, 0.0), nit((size_t)m * nlam, 0.0);
    std::memset(out.beta_out, 0, sizeof(float) * bsz * m);
    if (out.stats) std::memset(out.stats, 0, sizeof(admm_stats) * (size_t)m);
    LassoProblem pb = spec.problem(0, false);
    pb.profile_stride = 0;

    const bool tall = n > p;                                           // Lasso.cpp:73
    DeviceData<float> base;
    DevBuf<float> G;
    long long ldg = 0;
    double t_shared = 0;
    int first = -1;
    for (int j = 0; j < m; ++j) if (j % nranks == rank) { first = j; break; }
    if (first >= 0) {
        const double t0 = now_s();
        upload_standardize<float>(base, xd, yd + (size_t)first * n, n, p, ADMM_MEM_DEVICE, spec.standardize != 0, spec.intercept != 0, st.s, 0);
        if (tall) {
            ldg = round_up(p, 128);
            G.alloc((size_t)ldg * ldg); G.zero(st.s);
            gram_full<float>(base.X.get(), base.ldx, n, p, true, G.get(), ldg, st.s);
            comm_stream_sync(st.s);
        }
        t_shared = now_s() - t0;
    }
    for (int j = 0; j < m; ++j) {
        if (j % nranks != rank) continue;
        const double t0 = now_s();
        DeviceData<float> d;
        clone_with_response_f32(d, base, tall ? G.get() : nullptr, ldg, yd + (size_t)j * n, st.s);
        std::unique_ptr<LassoPlan> plan = tall ? make_tall_plan(std::move(d), pb, st.s) : make_wide_plan(std::move(d), pb, st.s);
        LassoResult res;
        plan->run(res);
        ADMM_REQUIRE((int)res.lambda.size() == nlam, "internal: unexpected path length");
        for (int l = 0; l < nlam; ++l) { lam[(size_t)j * nlam + l] = res.lambda[l]; nit[(size_t)j * nlam + l] = res.niter[l]; }
        std::memcpy(out.beta_out + (size_t)j * bsz, res.beta.data(), sizeof(float) * bsz);
        if (out.stats) { out.stats[j] = res.stats; out.stats[j].t_total = now_s() - t0 + (j == first ? t_shared : 0.0); }
    }
    sum_over_ranks(lam, nit, out.beta_out, bsz * m, st.s);             // the other ranks' responses
    for (size_t k = 0; k < lam.size(); ++k) { out.lambda_out[k] = lam[k]; out.niter_out[k] = (int)std::llround(nit[k]); }
}

// ---- the dense solvers (LAD, BP, ParBP) and the Dantzig selector: double precision, one solve per call
namespace {
template <typename R>
void begin_result(R& res, const DeviceData<double>& d, const TraceOut& trace) {
    res.trace_cap = trace.cap;
    res.stats.t_h2d = d.t_h2d;
    res.stats.t_standardize = d.t_std;
}
template <typename R>
void finish_result(R& res, double t0, const TraceOut& trace, admm_stats* stats) {
    trace.store(res.trace);
    res.stats.t_total = now_s() - t0;
    if (stats) *stats = res.stats;
}

// What LAD, BP and ParBP share.  The standardise flags are fixed by the reference per solver; shape_ok / shape_msg is the solver's
// precondition on the shape, blocks_ok ParBP's on nthread; `solve` fills res.beta with ncoef coefficients.
using DenseSolve = std::function<void(const DeviceData<double>&, DenseResult&, hipStream_t)>;
void check_dense(const double* x, const double* y, int n, int p, int mem, const admm_opts* opts, bool shape_ok, const char* shape_msg, bool blocks_ok,
                 const DenseOut& out) {
    const StateOut& so = out.state;
    out.trace.check();
    ADMM_REQUIRE(so.cap == 0 || (so.out != nullptr && so.n_out != nullptr && so.cap > 0 && out.trace.cap > 0), "bad state arguments (the iterate dump needs the trace)");
    check_common(x, y, n, p, mem, opts);
    ADMM_REQUIRE(out.beta_out && out.niter_out, "output pointers must not be NULL");
    ADMM_REQUIRE(shape_ok, shape_msg);
    ADMM_REQUIRE(opts->rho > 0, "rho should be positive");
    ADMM_REQUIRE(blocks_ok, "nthread must be within [1, ncol(x)]");
}
void store_state(const DenseResult& res, const StateOut& so) {
    if (so.cap <= 0) return;
    std::memcpy(so.out, res.state.data(), res.state.size() * sizeof(double));
    *so.n_out = res.state_dim > 0 ? (long long)(res.state.size() / (5 * (size_t)res.state_dim)) : 0;
}
void run_dense(const double* x, const double* y, int n, int p, int mem, const admm_opts* opts, bool standardize, bool intercept,
               bool shape_ok, const char* shape_msg, bool blocks_ok, int ncoef, const DenseSolve& solve, const DenseOut& out) {
    const StateOut& so = out.state;
    check_dense(x, y, n, p, mem, opts, shape_ok, shape_msg, blocks_ok, out);
    require_device();
    const double t0 = now_s();
    Stream st;
    DeviceData<double> d;
    upload_standardize<double>(d, x, y, n, p, mem, standardize, intercept, st.s);
    DenseResult res;
    begin_result(res, d, out.trace);
    res.state_cap = so.cap;
    solve(d, res, st.s);
    for (int i = 0; i < ncoef; ++i) out.beta_out[i] = res.beta[i];
    out.niter_out[0] = res.niter;
    store_state(res, so);
    finish_result(res, t0, out.trace, out.stats);
}
}  // namespace

void lad(const double* x, const double* y, int n, int p, int mem, int intercept, const admm_opts* opts, const DenseOut& out) {
    run_dense(x, y, n, p, mem, opts, true, intercept != 0,                           // LAD.cpp:34: standardize always TRUE
              n > p, "nrow(x) must be greater than ncol(x)", true, p + 1,            // R/20_admm_lad.R:21-22
              [&](const DeviceData<double>& d, DenseResult& res, hipStream_t st) { solve_lad(d, *opts, res, st); }, out);
}

namespace {
// the checks of a call whose intercept is FITTED (a column of ones behind the standardised X): n > p + intercept
void check_fitted(const double* x, const double* y, int n, int p, int mem, bool icpt, const admm_opts* opts, const DenseOut& out) {
    check_dense(x, y, n, p, mem, opts, (long long)n > (long long)p + (icpt ? 1 : 0),
                icpt ? "nrow(x) must be greater than ncol(x) + 1 (the intercept is fitted)" : "nrow(x) must be greater than ncol(x)", true, out);
}
// the label validation of a k-column call (first offending column, 0-based); ones: per column the count of labels 1.0, or NULL.
// Host labels are checked here, device labels by one reduction kernel per column, without a copy to the host.
void check_label_columns(const double* y, int n, int k, int mem, std::vector<long long>* ones_out) {
    for (int c = 0; c < k; ++c) {
        const double* yc = y + (size_t)c * n;
        long long bad = 0, ones = 0;
        if (mem == ADMM_MEM_HOST) {
            for (int i = 0; i < n; ++i) { if (yc[i] == 1.0) ++ones; else if (!(yc[i] == 0.0)) ++bad; }
        } else {
            require_device();
            Stream cs;
            logit_count_labels(yc, n, &bad, &ones, cs.s);
        }
        ADMM_REQUIRE(bad == 0, "column " + std::to_string(c) + " of y: every label must be exactly 0 or 1");
        ADMM_REQUIRE(ones > 0 && ones < n, "column " + std::to_string(c) + " of y must hold both classes");
        if (ones_out) (*ones_out)[c] = ones;
    }
}
// What the grid calls on the LAD loop share behind their own argument checks: LAD's standardisation (always), the caller's ycols
// columns of y resident on the device for the solver (labels, counts; 0: it needs the standardised response only -- with columns the
// response the upload standardises, column 0, is replaced by zeros there), every fit's coefficients and iterations out.
// store: what goes to the caller's coefficient and iteration tables; none: every fit's, in the solver's order.
using GridSolve = std::function<void(DeviceData<double>&, const double*, QuantResult&, hipStream_t)>;
using GridStore = std::function<void(const QuantResult&)>;
void run_lad_grid(const double* x, const double* y, int n, int p, int ycols, int mem, bool icpt, const admm_opts* opts, const GridSolve& solve, const DenseOut& out,
                  const GridStore& store = nullptr) {
    require_device();
    const double t0 = now_s();
    Stream st;
    DeviceData<double> d;
    upload_standardize<double>(d, x, y, n, p, mem, true, icpt, st.s);
    const Resident cols(y, (size_t)n * ycols, mem);
    QuantResult res;
    begin_result(res.dense, d, out.trace);
    res.dense.state_cap = out.state.cap;
    solve(d, cols.p, res, st.s);
    if (store) store(res);
    else {
        std::memcpy(out.beta_out, res.beta.data(), res.beta.size() * sizeof(double));
        for (size_t k = 0; k < res.niter.size(); ++k) out.niter_out[k] = res.niter[k];
    }
    store_state(res.dense, out.state);
    finish_result(res.dense, t0, out.trace, out.stats);
}
}  // namespace

// admm_hip_quantreg: LAD's checks and standardisation (always TRUE), one loop per quantile on one setup (solve_quantreg).  The
// intercept is FITTED (a column of ones behind the standardised X), not recovered from the means as LAD's: n > p + intercept.
void quantreg(const double* x, const double* y, int n, int p, int mem, int intercept, const double* tau, int ntau, const admm_opts* opts, const DenseOut& out) {
    ADMM_REQUIRE(tau != nullptr, "tau must not be NULL");
    ADMM_REQUIRE(ntau >= 1 && ntau <= 4096, "the number of quantiles must be within [1, 4096]");
    for (int k = 0; k < ntau; ++k) ADMM_REQUIRE(std::isfinite(tau[k]) && tau[k] > 0.0 && tau[k] < 1.0, "every tau must lie strictly between 0 and 1");
    ADMM_REQUIRE(ntau == 1 || out.trace.cap == 0, "the decision trace is recorded for a single tau");
    const bool icpt = intercept != 0;
    check_fitted(x, y, n, p, mem, icpt, opts, out);
    run_lad_grid(x, y, n, p, 0, mem, icpt, opts, [&](DeviceData<double>& d, const double*, QuantResult& res, hipStream_t st) { solve_quantreg(d, icpt, *opts, tau, ntau, res, st); }, out);
}

// admm_hip_huber: the same call with the Huber form of the prox, one fit per (delta[k], tau[k]); tau = NULL: the symmetric Huber loss.
void huber(const double* x, const double* y, int n, int p, int mem, int intercept, const double* delta, const double* tau, int nfit, const admm_opts* opts,
           const DenseOut& out) {
    ADMM_REQUIRE(delta != nullptr, "delta must not be NULL");
    ADMM_REQUIRE(nfit >= 1 && nfit <= 4096, "the number of fits must be within [1, 4096]");
    for (int k = 0; k < nfit; ++k) ADMM_REQUIRE(!std::isnan(delta[k]) && delta[k] > 0.0, "every delta must be positive (+inf: expectile regression)");
    for (int k = 0; tau != nullptr && k < nfit; ++k)
        ADMM_REQUIRE(std::isfinite(tau[k]) && tau[k] > 0.0 && tau[k] < 1.0, "every tau must lie strictly between 0 and 1");
    ADMM_REQUIRE(nfit == 1 || out.trace.cap == 0, "the decision trace is recorded for a single fit");
    std::vector<double> t(nfit, 0.5);
    if (tau != nullptr) t.assign(tau, tau + nfit);
    const bool icpt = intercept != 0;
    check_fitted(x, y, n, p, mem, icpt, opts, out);
    run_lad_grid(x, y, n, p, 0, mem, icpt, opts, [&](DeviceData<double>& d, const double*, QuantResult& res, hipStream_t st) { solve_huber(d, icpt, *opts, delta, t.data(), nfit, res, st); }, out);
}

// admm_hip_logit: logistic regression on the LAD loop (solve_logit).  The shape rule of the fitted intercept and LAD's standardisation
// of x (always); y holds labels, exactly 0.0 or 1.0 with both classes present -- host labels are checked here, device labels by one
// reduction kernel, without a copy to the host.  The signs come from the caller's y, not from the standardised one.
void logit(const double* x, const double* y, int n, int p, int mem, int intercept, const admm_opts* opts, const DenseOut& out) {
    const bool icpt = intercept != 0;
    check_fitted(x, y, n, p, mem, icpt, opts, out);
    long long bad = 0, ones = 0;
    if (mem == ADMM_MEM_HOST) {
        for (int i = 0; i < n; ++i) { if (y[i] == 1.0) ++ones; else if (!(y[i] == 0.0)) ++bad; }
    } else {
        require_device();
        Stream cs;
        logit_count_labels(y, n, &bad, &ones, cs.s);
    }
    ADMM_REQUIRE(bad == 0, "every label in y must be exactly 0 or 1");
    ADMM_REQUIRE(ones > 0 && ones < n, "y must hold both classes");
    require_device();
    const double t0 = now_s();
    Stream st;
    DeviceData<double> d;
    upload_standardize<double>(d, x, y, n, p, mem, true, icpt, st.s);
    Resident labels(y, (size_t)n, mem);
    DenseResult res;
    begin_result(res, d, out.trace);
    res.state_cap = out.state.cap;
    solve_logit(d, icpt, labels.p, *opts, res, st.s);
    for (int i = 0; i < p + 1; ++i) out.beta_out[i] = res.beta[i];
    out.niter_out[0] = res.niter;
    store_state(res, out.state);
    finish_result(res, t0, out.trace, out.stats);
}

// admm_hip_logit_multi: k label columns on one setup (solve_logit_multi).  logit's checks, every column validated as its vector; a
// refusal names the first offending column.  No trace / state form.
void logit_multi(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const admm_opts* opts, const DenseOut& out) {
    const bool icpt = intercept != 0;
    ADMM_REQUIRE(k >= 1, "y must have at least one column");
    check_fitted(x, y, n, p, mem, icpt, opts, out);
    check_label_columns(y, n, k, mem, nullptr);
    run_lad_grid(x, y, n, p, k, mem, icpt, opts, [&](DeviceData<double>& d, const double* labels, QuantResult& res, hipStream_t st) { solve_logit_multi(d, icpt, labels, k, *opts, res, st); }, out);
}

// admm_hip_logit_ridge: logit_multi with the ridge penalty lambda / 2 sum b_j^2 (solve_logit_ridge), one fit per (column, lambda).  The
// penalty makes the augmented matrix of full column rank for any n: no n > p condition, separable labels have an estimate.
void logit_ridge(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const double* lambda, int nlambda, const admm_opts* opts,
                 const DenseOut& out) {
    const bool icpt = intercept != 0;
    ADMM_REQUIRE(k >= 1, "y must have at least one column");
    ADMM_REQUIRE(lambda != nullptr, "lambda must not be NULL");
    ADMM_REQUIRE(nlambda >= 1, "lambda must have at least one value");
    for (int l = 0; l < nlambda; ++l)
        ADMM_REQUIRE(std::isfinite(lambda[l]) && lambda[l] > 0.0, "every lambda must be finite and positive (lambda = 0 is admm_hip_logit_multi)");
    ADMM_REQUIRE((k == 1 && nlambda == 1) || out.trace.cap == 0, "the decision trace is recorded for a single column and a single lambda");
    check_dense(x, y, n, p, mem, opts, n >= 2, "nrow(x) must be at least 2", true, out);
    check_label_columns(y, n, k, mem, nullptr);
    run_lad_grid(x, y, n, p, k, mem, icpt, opts,
                 [&](DeviceData<double>& d, const double* labels, QuantResult& res, hipStream_t st) { solve_logit_ridge(d, icpt, labels, k, lambda, nlambda, *opts, res, st); }, out);
}

// admm_hip_logit_enet: logit_ridge's call with (lambda, alpha) cells in place of the lambda grid (solve_logit_enet): one fit per
// (column, cell), all of them on ONE inverse.
static void check_logit_enet(const double* x, const double* y, int n, int p, int k, int mem, const double* lambda, const double* alpha, int ncell, const admm_opts* opts,
                             const DenseOut& out) {
    ADMM_REQUIRE(k >= 1, "y must have at least one column");
    ADMM_REQUIRE(lambda != nullptr && alpha != nullptr, "lambda and alpha must not be NULL");
    ADMM_REQUIRE(ncell >= 1, "lambda must have at least one value");
    for (int l = 0; l < ncell; ++l) ADMM_REQUIRE(std::isfinite(lambda[l]) && lambda[l] > 0.0, "every lambda must be finite and positive");
    for (int l = 0; l < ncell; ++l) ADMM_REQUIRE(alpha[l] >= 0.0 && alpha[l] <= 1.0, "every alpha must lie in [0, 1]");
    ADMM_REQUIRE((k == 1 && ncell == 1) || out.trace.cap == 0, "the decision trace is recorded for a single column and a single cell");
    check_dense(x, y, n, p, mem, opts, n >= 2, "nrow(x) must be at least 2", true, out);
    check_label_columns(y, n, k, mem, nullptr);
}
void logit_enet(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const double* lambda, const double* alpha, int ncell,
                const admm_opts* opts, const DenseOut& out) {
    const bool icpt = intercept != 0;
    check_logit_enet(x, y, n, p, k, mem, lambda, alpha, ncell, opts, out);
    run_lad_grid(x, y, n, p, k, mem, icpt, opts,
                 [&](DeviceData<double>& d, const double* labels, QuantResult& res, hipStream_t st) { solve_logit_enet(d, icpt, labels, k, lambda, alpha, ncell, *opts, res, st); }, out);
}

// admm_hip_logit_enet_lambda_max: lambda_1 per label column on the standardised columns, max_j |x~_j'(y_c - mean)|, mean = the column's
// share of ones with the intercept and 1/2 without (the gradient of the likelihood at b = 0 with the fitted, or the absent, intercept)
void logit_enet_lambda_max(const double* x, const double* y, int n, int p, int k, int mem, int intercept, double* out) {
    const bool icpt = intercept != 0;
    ADMM_REQUIRE(k >= 1, "y must have at least one column");
    ADMM_REQUIRE(x != nullptr && y != nullptr, "x and y must not be NULL");
    ADMM_REQUIRE(n > 0 && p > 0, "n and p must be positive");
    ADMM_REQUIRE(mem == ADMM_MEM_HOST || mem == ADMM_MEM_DEVICE, "mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE");
    ADMM_REQUIRE(out != nullptr, "output pointers must not be NULL");
    ADMM_REQUIRE(n >= 2, "nrow(x) must be at least 2");
    std::vector<long long> ones(k);
    check_label_columns(y, n, k, mem, &ones);
    require_device();
    Stream st;
    DeviceData<double> d;
    upload_standardize<double>(d, x, y, n, p, mem, true, icpt, st.s);
    Resident labels(y, (size_t)n * k, mem);
    std::vector<double> mean(k), lam1(k);
    for (int c = 0; c < k; ++c) mean[c] = icpt ? (double)ones[c] / (double)n : 0.5;
    logit_enet_lambda_one(d, labels.p, k, mean.data(), lam1.data(), st.s);
    for (int c = 0; c < k; ++c) out[c] = lam1[c];
}

// the count validation of admm_hip_poisson: every entry finite and >= 0 (non-integers pass: quasi-likelihood use), every column with a
// positive sum.  Host counts are checked here, device counts by one reduction kernel per call, without a copy to the host.
static void check_count_columns(const double* y, int n, int k, int mem) {
    long long bad = 0;
    std::vector<double> sums(k, 0.0);
    if (mem == ADMM_MEM_HOST) {
        for (int c = 0; c < k; ++c) {
            const double* yc = y + (size_t)c * n;
            for (int i = 0; i < n; ++i) { if (!(yc[i] >= 0.0) || std::isinf(yc[i])) ++bad; else sums[c] += yc[i]; }
        }
    } else {
        require_device();
        Stream cs;
        pois_column_stats(y, n, k, &bad, sums.data(), cs.s);
    }
    ADMM_REQUIRE(bad == 0, "every y must be finite and non-negative");
    for (int c = 0; c < k; ++c) ADMM_REQUIRE(sums[c] > 0.0, "every column of y must have a positive sum");
}

// admm_hip_poisson: logit_enet's call with count columns and the Poisson likelihood (solve_poisson): one fit per (column, cell), all of
// them on ONE inverse.  lambda = 0 is accepted -- the plain Poisson GLM -- and then needs a design of full column rank by shape.
static void check_poisson(const double* x, const double* y, int n, int p, int k, int mem, bool icpt, const double* lambda, const double* alpha, int ncell, const admm_opts* opts,
                          const DenseOut& out) {
    ADMM_REQUIRE(k >= 1, "y must have at least one column");
    ADMM_REQUIRE(lambda != nullptr && alpha != nullptr, "lambda and alpha must not be NULL");
    ADMM_REQUIRE(ncell >= 1, "lambda must have at least one value");
    bool unpenalised = false;
    for (int l = 0; l < ncell; ++l) {
        ADMM_REQUIRE(std::isfinite(lambda[l]) && lambda[l] >= 0.0, "every lambda must be finite and non-negative");
        unpenalised = unpenalised || lambda[l] == 0.0;
    }
    for (int l = 0; l < ncell; ++l) ADMM_REQUIRE(alpha[l] >= 0.0 && alpha[l] <= 1.0, "every alpha must lie in [0, 1]");
    ADMM_REQUIRE((k == 1 && ncell == 1) || out.trace.cap == 0, "the decision trace is recorded for a single column and a single cell");
    check_dense(x, y, n, p, mem, opts, n >= 2, "nrow(x) must be at least 2", true, out);
    ADMM_REQUIRE(!unpenalised || (long long)n > (long long)p + (icpt ? 1 : 0), "lambda = 0 needs nrow(x) > ncol(x) + intercept");
    check_count_columns(y, n, k, mem);
}
void poisson(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const double* lambda, const double* alpha, int ncell,
             const admm_opts* opts, const DenseOut& out) {
    const bool icpt = intercept != 0;
    check_poisson(x, y, n, p, k, mem, icpt, lambda, alpha, ncell, opts, out);
    run_lad_grid(x, y, n, p, k, mem, icpt, opts,
                 [&](DeviceData<double>& d, const double* counts, QuantResult& res, hipStream_t st) { solve_poisson(d, icpt, counts, k, lambda, alpha, ncell, *opts, res, st); }, out);
}

// admm_hip_poisson_lambda_max: lambda_1 per count column on the standardised columns, max_j |x~_j'(y_c - mu)|: mu = mean(y_c) with the
// intercept (the fitted intercept at b = 0 is log mean(y_c)), mu = 1 without it (eta = 0).  The column means are formed on the device
// from the resident counts, for host and device input alike.
void poisson_lambda_max(const double* x, const double* y, int n, int p, int k, int mem, int intercept, double* out) {
    const bool icpt = intercept != 0;
    ADMM_REQUIRE(k >= 1, "y must have at least one column");
    ADMM_REQUIRE(x != nullptr && y != nullptr, "x and y must not be NULL");
    ADMM_REQUIRE(n > 0 && p > 0, "n and p must be positive");
    ADMM_REQUIRE(mem == ADMM_MEM_HOST || mem == ADMM_MEM_DEVICE, "mem must be ADMM_MEM_HOST or ADMM_MEM_DEVICE");
    ADMM_REQUIRE(out != nullptr, "output pointers must not be NULL");
    ADMM_REQUIRE(n >= 2, "nrow(x) must be at least 2");
    check_count_columns(y, n, k, mem);
    require_device();
    Stream st;
    DeviceData<double> d;
    upload_standardize<double>(d, x, y, n, p, mem, true, icpt, st.s);
    Resident counts(y, (size_t)n * k, mem);
    std::vector<double> mean(k, 1.0), lam1(k);
    if (icpt) {
        long long bad = 0;
        pois_column_stats(counts.p, n, k, &bad, mean.data(), st.s);
        for (int c = 0; c < k; ++c) mean[c] /= (double)n;
    }
    logit_enet_lambda_one(d, counts.p, k, mean.data(), lam1.data(), st.s);
    for (int c = 0; c < k; ++c) out[c] = lam1[c];
}

// admm_hip_logit_enet_cv / admm_hip_poisson_cv (and their _state forms: fold >= -1, one column, one cell): K-fold cross-validation of
// the (column, cell) grid on ONE setup (solve_glm_cv).  The public call's own checks, then the folds': every fold non-empty, every
// training set a valid problem of its own in every column.  Nothing is written before every check has passed.
// Slot 0 of the solver's grid is the full-data fit (out.beta_out, out.niter_out: admm_hip_logit_enet's / admm_hip_poisson's numbers),
// slot f + 1 fold f's.  cv_mean / cv_se: the unweighted mean over the folds and the sample sd / sqrt(F), admm_hip_lasso_cv's convention.
void glm_cv(bool pois, const double* x, const double* y, int n, int p, int k, int mem, int intercept, const int* fold_id, int nfolds, int fold, const double* lambda,
            const double* alpha, int ncell, const admm_opts* opts, const DenseOut& out, const GlmCvOut& cv) {
    const bool icpt = intercept != 0, grid = fold < -1;
    if (pois) check_poisson(x, y, n, p, k, mem, icpt, lambda, alpha, ncell, opts, out);
    else check_logit_enet(x, y, n, p, k, mem, lambda, alpha, ncell, opts, out);
    ADMM_REQUIRE(!grid || (cv.cv_mean != nullptr && cv.cv_se != nullptr), "cv_mean and cv_se must not be NULL");
    ADMM_REQUIRE(nfolds >= 2 && nfolds <= n, "nfolds must be within [2, n]");
    ADMM_REQUIRE(grid || fold < nfolds, "fold must be within [-1, nfolds)");
    std::vector<int> fid(n), cnt(nfolds, 0);
    for (int i = 0; i < n; ++i) {
        fid[i] = fold_id ? fold_id[i] : i % nfolds;
        ADMM_REQUIRE(fid[i] >= 0 && fid[i] < nfolds, "fold_id entries must be within [0, nfolds)");
        ++cnt[fid[i]];
    }
    int min_tr = n;
    for (int f = 0; f < nfolds; ++f) {
        ADMM_REQUIRE(cnt[f] > 0, "every fold needs at least one held-out row");
        min_tr = std::min(min_tr, n - cnt[f]);
    }
    {   // every training set: both classes (logit), a positive count (Poisson), in every column -- on a host copy of y (n x k)
        std::vector<double> hy;
        const double* yh = y;
        if (mem != ADMM_MEM_HOST) {
            require_device();
            Stream cs;
            hy.resize((size_t)n * k);
            read_back(hy.data(), y, hy.size() * sizeof(double), cs.s);
            yh = hy.data();
        }
        std::vector<long long> in(nfolds);
        for (int c = 0; c < k; ++c) {
            long long all = 0;
            std::fill(in.begin(), in.end(), 0);
            for (int i = 0; i < n; ++i) if (pois ? yh[(size_t)c * n + i] > 0.0 : yh[(size_t)c * n + i] == 1.0) { ++all; ++in[fid[i]]; }
            for (int f = 0; f < nfolds; ++f) {
                const long long tr = all - in[f];
                if (pois) ADMM_REQUIRE(tr > 0, "column " + std::to_string(c) + " of y has a zero sum over the training rows of fold " + std::to_string(f));
                else ADMM_REQUIRE(tr > 0 && tr < n - cnt[f], "column " + std::to_string(c) + " of y lacks a class in the training rows of fold " + std::to_string(f));
            }
        }
    }
    if (pois)
        for (int l = 0; l < ncell; ++l) ADMM_REQUIRE(lambda[l] != 0.0 || (long long)min_tr > (long long)p + (icpt ? 1 : 0), "lambda = 0 needs more training rows than ncol(x) + intercept in every fold");

    GlmFolds folds;
    folds.id = &fid; folds.nfolds = nfolds; folds.single = grid ? -2 : fold;
    std::vector<double> dev;
    const GridSolve solve = [&](DeviceData<double>& d, const double* cols, QuantResult& res, hipStream_t st) {
        solve_glm_cv(pois, d, icpt, cols, k, folds, lambda, alpha, ncell, *opts, res, grid ? &dev : nullptr, st);
    };
    if (!grid) {                                                 // one fit: run_lad_grid's own store
        run_lad_grid(x, y, n, p, k, mem, icpt, opts, solve, out);
        return;
    }
    // the solver's fits are cell-major, then slot, then column: slot 0 to the caller's tables, slot f + 1 to fold f's
    const int nslot = nfolds + 1;
    const size_t bcol = (size_t)p + 1, npair = (size_t)k * ncell;
    run_lad_grid(x, y, n, p, k, mem, icpt, opts, solve, out, [&](const QuantResult& res) {
        for (int l = 0; l < ncell; ++l)
            for (int s = 0; s < nslot; ++s)
                for (int c = 0; c < k; ++c) {
                    const size_t fit = ((size_t)l * nslot + s) * k + c, pair = (size_t)l * k + c;
                    const double* b = res.beta.data() + fit * bcol;
                    if (s == 0) {
                        std::memcpy(out.beta_out + pair * bcol, b, bcol * sizeof(double));
                        out.niter_out[pair] = res.niter[fit];
                    } else {
                        if (cv.fold_beta) std::memcpy(cv.fold_beta + ((size_t)(s - 1) * npair + pair) * bcol, b, bcol * sizeof(double));
                        if (cv.fold_niter) cv.fold_niter[(size_t)(s - 1) * npair + pair] = res.niter[fit];
                    }
                }
    });
    if (cv.fold_dev) std::memcpy(cv.fold_dev, dev.data(), dev.size() * sizeof(double));
    for (size_t q = 0; q < npair; ++q) {
        double m = 0;
        for (int f = 0; f < nfolds; ++f) m += dev[(size_t)f * npair + q];
        m /= nfolds;
        double v = 0;
        for (int f = 0; f < nfolds; ++f) { const double e = dev[(size_t)f * npair + q] - m; v += e * e; }
        cv.cv_mean[q] = m;
        cv.cv_se[q] = std::sqrt(v / (nfolds - 1) / nfolds);
    }
    for (int c = 0; c < k; ++c) {
        int imin = 0;
        for (int l = 1; l < ncell; ++l) if (cv.cv_mean[(size_t)l * k + c] < cv.cv_mean[(size_t)imin * k + c]) imin = l;
        // the one-standard-error rule among the cells of the minimum's alpha: the largest lambda within one standard error
        const double bound = cv.cv_mean[(size_t)imin * k + c] + cv.cv_se[(size_t)imin * k + c];
        int i1se = imin;
        for (int l = 0; l < ncell; ++l)
            if (alpha[l] == alpha[imin] && lambda[l] > lambda[i1se] && cv.cv_mean[(size_t)l * k + c] <= bound) i1se = l;
        if (cv.idx_min) cv.idx_min[c] = imin;
        if (cv.idx_1se) cv.idx_1se[c] = i1se;
    }
}

void bp(const double* x, const double* y, int n, int p, int mem, const admm_opts* opts, const DenseOut& out) {
    run_dense(x, y, n, p, mem, opts, false, false,                                   // BP.cpp:24-27: no standardisation
              p > n, "ncol(x) must be greater than nrow(x)", true, p,                // R/10_admm_bp.R:30-31
              [&](const DeviceData<double>& d, DenseResult& res, hipStream_t st) { solve_bp(d, *opts, res, st); }, out);
}

// admm_parbp (R/10_admm_bp.R:111-116; TODO/ParBP.cppp:26-71): opts->rho carries rho_ratio.
static void parbp_cols(const double* x_cols, const double* y, int n, int p_local, long long p_total, long long col_offset, int mem, int nthread,
                       const admm_opts* opts, const DenseOut& out) {
    run_dense(x_cols, y, n, p_local, mem, opts, false, false,                        // ParBP.cppp:36-37: no standardisation
              p_total > n, "ncol(x) must be greater than nrow(x)", nthread >= 1 && nthread <= p_total, p_local,
              [&](const DeviceData<double>& d, DenseResult& res, hipStream_t st) { solve_parbp(d, *opts, nthread, p_total, col_offset, res, st); }, out);
}

void parbp(const double* x, const double* y, int n, int p, int mem, int nthread, const admm_opts* opts, const DenseOut& out) {
    const std::vector<int> devs = nthread >= 1 ? par_devices_for(nthread) : std::vector<int>();
    if (devs.empty()) {
        record_single_layout();
        parbp_cols(x, y, n, p, p, 0, mem, nthread, opts, out);
        return;
    }
    // in-process ranks: rank r holds its whole blocks of columns (admm_amd/dist.py parbp_partition)
    out.trace.check();
    ADMM_REQUIRE(x != nullptr && out.beta_out && out.niter_out, "x and the output pointers must not be NULL");
    ADMM_REQUIRE(n > 0 && p > 0, "n and p must be positive");
    ADMM_REQUIRE(nthread >= 1 && nthread <= p, "nthread must be within [1, ncol(x)]");
    run_inproc(devs, input_device(x, mem), [&](int rank, int nranks) {
        const long long chunk = p / nthread, per = nthread / nranks;
        const long long lo = rank * per * chunk, hi = rank == nranks - 1 ? p : (rank + 1) * per * chunk;
        int nit = 0;
        admm_stats st_own;
        const DenseOut mine = {out.beta_out + lo, &nit, rank == 0 ? out.stats : &st_own, rank == 0 ? out.trace : TraceOut{}, out.state};
        parbp_cols(x + (size_t)lo * n, y, n, (int)(hi - lo), p, lo, mem, nthread, opts, mine);
        if (rank == 0) out.niter_out[0] = nit;
    });
}

void parbp_dist(const double* x_cols, const double* y, int n, int p_local, long long p_total, long long col_offset, int mem, int nthread,
                const admm_opts* opts, const DenseOut& out) {
    ADMM_REQUIRE(comm_info().active, "no communicator: call admm_hip_comm_init first");
    ADMM_REQUIRE(p_total >= p_local && col_offset >= 0 && col_offset + p_local <= p_total, "column block outside [0, p_total)");
    parbp_cols(x_cols, y, n, p_local, p_total, col_offset, mem, nthread, opts, out);
}

// admm_dantzig (R/50_admm_dantzig.R:30-46; TODO/Dantzig.cpp:32-99)
void dantzig(const double* x, const double* y, int n, int p, int mem, const PathSpec& spec, const PathOutT<double>& out, const TraceOut& trace) {
    trace.check();
    check_common(x, y, n, p, mem, spec.opts);
    out.require();
    spec.check();
    ADMM_REQUIRE(p >= 3, "the spectral-radius estimate needs at least 3 columns");
    require_device();
    const double t0 = now_s();
    Stream st;
    DeviceData<double> d;
    upload_standardize<double>(d, x, y, n, p, mem, spec.standardize != 0, spec.intercept != 0, st.s);     // Dantzig.cpp:52-55
    const LassoProblem pb = spec.problem(0, false);
    DantzigResult res;
    begin_result(res, d, trace);
    solve_dantzig(d, pb, res, st.s);
    const int nl = (int)res.lambda.size();
    for (int i = 0; i < nl; ++i) { out.lambda_out[i] = res.lambda[i]; out.niter_out[i] = res.niter[i]; }
    std::memcpy(out.beta_out, res.beta.data(), sizeof(double) * (size_t)(p + 1) * nl);
    finish_result(res, t0, trace, out.stats);
}

}  // namespace admm
