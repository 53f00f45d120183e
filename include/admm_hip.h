/*
 * admm_hip.h -- C ABI of libadmm_hip.so, the MI355X (gfx950) replacement for the
 * numeric part of the reference's five `.Call` entry points (yixuan/ADMM 1.0).
 *
 * Boundary: R calls `.Call("<sym>", ..., PACKAGE = "ADMM")`
 * by name; each RcppExport function unpacks SEXPs, runs the solver and builds an R
 * list.  The functions below take exactly the unpacked values of those calls
 * (plain pointers and sizes, column-major double like R memory), run the whole
 * solve on the GPU and fill caller-owned output arrays.  An Rcpp shim that keeps
 * the reference's symbol names and forwards here is shown in INTEGRATION.md.
 *
 *   admm_hip_lasso     replaces  admm_lasso     /root/reference/src/Lasso.cpp:32-137
 *   admm_hip_enet      replaces  admm_enet      /root/reference/src/Enet.cpp:31-137
 *   admm_hip_parlasso  replaces  admm_parlasso  /root/reference/src/ParLasso.cpp:33-110
 *   admm_hip_lad       replaces  admm_lad       /root/reference/src/LAD.cpp:16-47
 *   admm_hip_bp        replaces  admm_bp        /root/reference/src/BP.cpp:20-45
 *
 * Conventions
 *   - x: n x p column-major (leading dimension n), y: length n.  Borrowed and
 *     read-only for the duration of the call (the reference copies or maps them:
 *     Lasso.cpp:42-50, LAD.cpp:20-21, BP.cpp:24-27).  `mem` says where they live:
 *     ADMM_MEM_HOST (what R hands over) or ADMM_MEM_DEVICE (already resident in
 *     HBM on the current HIP device; used by bench.py so that PCIe is not in the
 *     timed region).
 *   - Return value: 0 on success, an ADMM_ERR_* code otherwise; the message is
 *     available from admm_hip_last_error().  Nothing throws across the ABI and
 *     nothing calls the R API.  There is no CPU fallback: without a usable HIP
 *     device every solver returns ADMM_ERR_NO_DEVICE.
 *   - No state survives a call (the reference creates and destroys its solver
 *     inside the .Call: Lasso.cpp:74-76,126-129).
 */
#ifndef ADMM_HIP_H
#define ADMM_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with -fvisibility=hidden; only the functions below are exported */
#if defined(__GNUC__)
#define ADMM_HIP_API __attribute__((visibility("default")))
#else
#define ADMM_HIP_API
#endif

#define ADMM_OK 0
#define ADMM_ERR_INVALID_ARG 1
#define ADMM_ERR_NO_DEVICE 2
#define ADMM_ERR_HIP 3
#define ADMM_ERR_BLAS 4
#define ADMM_ERR_NOT_SPD 5      /* Cholesky of the Gram (+rho I) failed; the reference never checks LLT::info() */
#define ADMM_ERR_EIGS 6         /* Lanczos produced no converged Ritz value (the reference then reads evals[0] of an empty vector) */
#define ADMM_ERR_COMM 7
#define ADMM_ERR_INTERNAL 8
#define ADMM_ERR_MEMORY 9       /* the problem does not fit the device: the tall solver caches a p x p inverse (4 p^2 bytes, 160 GB at p = 2e5) --
                                   use the consensus solver ($parallel(): row blocks, Woodbury form) or the wide solver's shape instead */

#define ADMM_MEM_HOST 0
#define ADMM_MEM_DEVICE 1

/* The R `opts` list: list(maxit=, eps_abs=, eps_rel=, rho=)  (R/30_admm_lasso.R:139-146).
 * rho <= 0 means "choose automatically" (ADMMLassoTall.h:194-202, ADMMLassoWide.h:227-228,
 * PADMMLasso.h:199-200); LAD/BP use it as given (R default 1.0). */
typedef struct admm_opts {
    int maxit;
    double eps_abs;
    double eps_rel;
    double rho;
} admm_opts;

/* Optional per-call measurements (may be NULL). Times are seconds. */
typedef struct admm_stats {
    double t_h2d;          /* host -> device copies (0 for ADMM_MEM_DEVICE inputs) */
    double t_standardize;  /* convert + DataStd */
    double t_gram;         /* X'X or XX' */
    double t_eigs;         /* Lanczos lambda_max estimate */
    double t_factor;       /* Cholesky + cached inverse / triangular solves */
    double t_loop;         /* the ADMM iterations over all lambdas (wall, host clock around a device sync) */
    double t_total;
    double loop_ms_events; /* same loop measured with HIP events on the solver's stream */
    double xupdate_ms_avg; /* average duration of the x-update kernel, HIP events on the solver's stream (sampled launches) */
    long long xupdate_samples;
    long long total_iter;  /* sum of niter */
    long long xupdate_launches;
    double rho;            /* rho actually used (first lambda) */
    double eig_est;        /* the loose Lanczos value (lambda_max or spectral-radius estimate) */
    int branch;            /* 0 tall (Cholesky), 1 wide (linearised), 2 consensus; 6 admm_parbp (column-block sharing); 7 admm_dantzig */
    int xupdate_variant;   /* admm_hip_lad: 1 = one pass over the rows of X per iteration (general branch, p <= 6144), 0 = two products / hat matrix;
                              wide path: 1 / 2 = the regular steps ran screened through the fp16 copy / the 8-bit code of X (+ the exact step on the
                              few columns the bound does not settle: bit-identical iterates, 2np / np instead of 4np bytes), 0 = unscreened;
                              tall path: 0 = full-matrix mat-vec (4p^2 B), 1 = lower-triangle symmetric mat-vec (2p^2 B),
                              2 = the same with the tiles dealt out to the ranks + one all-reduce of 2p floats (admm_hip_lasso_dist),
                              (3, a single-launch iteration, existed in rounds 3 - 5: measured slower, removed in round 6);
                              admm_hip_parbp: + 4 = the regular iterations ran screened (as the wide path's);
                              0 = every active-set iteration streams the non-zero columns twice, 1 = active-set iterations
                              in Gram space (one |U| x |U| mat-vec each; xupdate_launches = stretches of nine that ran so, persist_iter =
                              times the column set U was rebuilt), 2 = 1 except for stretches of 100, 200, 400, ... iterations after the non-zeros
                              outgrew the Gram matrix, which ran as 0 */
    int exchange_variant;  /* sharded solvers: how the per-iteration exchange ran -- 0 none, 1 the exchange layer's all-reduce, 2 PEER slots written /
                              read by the solver's own kernels (producer and consumer launches), 3 the same with producer and consumer in ONE
                              launch (chosen only when that launch is resident as a whole: its workgroups wait for one another) */
    int refine;            /* tall path: 1 = every x-update refined once with a double-precision residual (ADMM_HIP_REFINE=1) */
    long long persist_iter;/* wide path: iterations that ran inside persistent active-set launches (of total_iter); -1: a hand-over of a stretch timed out and the whole path was run again without stretches */
    double factor_flops;   /* row-sharded tall solver: flops of the Cholesky + inverse THIS rank performed when the factorisation is
                              distributed over the ranks (block columns dealt out, panels broadcast); 0 when every
                              rank factorises the whole matrix */
} admm_stats;

/* lambda_in: user grid of length nlambda_in (sorted decreasing by the R wrapper), or NULL/0
 * for the automatic log-spaced grid of nlambda_auto values from lambda_0 * scaleY / n down to
 * lmin_ratio times that (Lasso.cpp:78-89).
 * Outputs (nl = nlambda_in > 0 ? nlambda_in : nlambda_auto):
 *   lambda_out[nl]            the grid used
 *   beta_out[(p+1) * nl]      column-major dense float, row 0 = intercept, on the ORIGINAL scale
 *                             (DataStd::recover; the reference returns this as a dgCMatrix whose
 *                             structural zeros are exactly the zeros here, Lasso.cpp:22-30)
 *   niter_out[nl]             ADMM iterations per lambda
 */
ADMM_HIP_API int admm_hip_lasso(const double* x, const double* y, int n, int p, int mem,
                   const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                   int standardize, int intercept, const admm_opts* opts,
                   double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats);

/* As admm_hip_lasso with the elastic-net mixing weight alpha (Enet.cpp:63, ADMMEnet.h:24-57). */
ADMM_HIP_API int admm_hip_enet(const double* x, const double* y, int n, int p, int mem,
                  const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                  int standardize, int intercept, double alpha, const admm_opts* opts,
                  double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats);

/* K-fold cross-validation of the lambda path of admm_hip_lasso (alpha < 0) / admm_hip_enet (alpha in [0, 1]).
 * SURVEY.md section 8(f) row n4 ("cross-validation folds as independent replicas across GPUs"); the reference package has
 * no CV driver, so there is no reference interface to cite -- the fold fits are the admm_lasso / admm_enet path
 * (/root/reference/src/Lasso.cpp:32-135, Enet.cpp:31-34) on row subsets.
 *   grid      the full data's (lambda_in, or the automatic grid of the full-data fit, Lasso.cpp:78-89), used by every fold;
 *   fold f    fitted on the rows with fold_id[i] != f by the SAME plan a direct call on that row subset gets (coefficients
 *             bit-identical to it), scored on the rows with fold_id[i] == f: mean squared prediction error per lambda, on
 *             the original scale, computed in double on the device.  fold_id NULL: i mod nfolds;
 *   ranks     with a communicator attached, fold f runs on rank f mod nranks (every rank is handed the full x, y;
 *             nothing is exchanged on the data path) and the tables are summed over the ranks at the end: all ranks
 *             return identical outputs.
 * Outputs: lambda_out[nlam]; beta_out (p+1) x nlam and niter_out[nlam] of the full-data fit (either may be NULL);
 * cv_mean[nlam]; cv_se[nlam] = sample sd over the folds / sqrt(nfolds); fold_mse[nfolds x nlam] (fold-major),
 * fold_niter[nfolds x nlam], fold_beta[nfolds x (p+1) x nlam] (each may be NULL); idx_min = argmin cv_mean;
 * idx_1se = index of the largest lambda with cv_mean <= cv_mean[idx_min] + cv_se[idx_min].  stats: the full-data fit's,
 * with t_total = the whole call. */
ADMM_HIP_API int admm_hip_lasso_cv(const double* x, const double* y, int n, int p, int mem, const int* fold_id, int nfolds,
                      const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                      int standardize, int intercept, double alpha, const admm_opts* opts,
                      double* lambda_out, float* beta_out, int* niter_out,
                      double* cv_mean, double* cv_se, double* fold_mse, int* fold_niter, float* fold_beta,
                      int* idx_min, int* idx_1se, admm_stats* stats);

/* Several responses of one design matrix: Y is n x m column-major, response j is the ordinary admm_hip_lasso (alpha < 0) /
 * admm_hip_enet (alpha in [0, 1]) fit of (x, Y[:, j]) -- coefficients, grids and iteration counts bit-identical to that call
 * -- but x is uploaded, converted and standardised once and, for the tall solver (n > p), X'X is formed once (it does not
 * depend on y; the cached inverse does, through rho, and is rebuilt per response).  SURVEY.md section 8(f) row n4; the
 * reference has no multi-response entry (its fits are one .Call each, /root/reference/src/Lasso.cpp:32-135).  With a
 * communicator attached response j runs on rank j mod nranks (every rank is handed the full x, Y; nothing is exchanged on
 * the data path) and the outputs are summed over the ranks at the end: all ranks return identical outputs.
 * Outputs (response-major): lambda_out[m x nlam], beta_out[m x (p+1) x nlam], niter_out[m x nlam], stats[m] (may be NULL;
 * the one-time shared work is charged to the first response of each rank; entries of responses fitted by other ranks stay zero). */
ADMM_HIP_API int admm_hip_lasso_multi(const double* x, const double* Y, int n, int p, int m, int mem,
                         const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                         int standardize, int intercept, double alpha, const admm_opts* opts,
                         double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats);

/* Row-block consensus ADMM with `nthread` blocks (ParLasso.cpp:33-36,71-72: nthread only sets the
 * number of blocks K).  By default all K blocks run on the current device.
 * In-process multi-device mode (option PAR_DEVICES / admm_hip_options.par_devices, off by default): with D devices listed the call
 * runs N = the largest divisor of K that is <= D ranks, one host thread per rank, rank r on the r-th listed device.  Each rank
 * uploads only its row slice of x (admm_hip_parlasso_dist's partition: K / N whole blocks per rank) and runs the distributed
 * consensus solver; the ranks exchange through the PEER one-shot all-reduce over device pointers (peer access between the listed
 * devices is enabled by the call).  The outputs are rank 0's (every rank holds the full result).  N = 1: the default path.  Refused
 * (ADMM_ERR_INVALID_ARG) while a process-wide communicator is attached.  mem = ADMM_MEM_DEVICE: ranks on other devices read their
 * slice over peer access (refused when there is none).  A failing rank ends every rank's call (ADMM_ERR_COMM or its own code). */
ADMM_HIP_API int admm_hip_parlasso(const double* x, const double* y, int n, int p, int mem,
                      const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                      int standardize, int intercept, int nthread, const admm_opts* opts,
                      double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats);

/* beta_out[p+1] (row 0 = intercept), niter_out[1]. Requires n > p (R/20_admm_lad.R:21-22). */
ADMM_HIP_API int admm_hip_lad(const double* x, const double* y, int n, int p, int mem, int intercept,
                 const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats);

/* beta_out[p], niter_out[1]. Requires p > n (R/10_admm_bp.R:30-31). */
ADMM_HIP_API int admm_hip_bp(const double* x, const double* y, int n, int p, int mem,
                const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats);

/* The Dantzig selector path, min ||beta||_1 s.t. ||X'(X beta - y)||_inf <= lambda -- what R's admm_dantzig(x, y)$fit() asks for,
 * .Call("admm_dantzig", x, y, lambda, nlambda, lambda_min_ratio, standardize, intercept, opts) (R/50_admm_dantzig.R:30-46), a
 * symbol the reference never builds (src/TODO/Dantzig.cpp:32-99, src/TODO/ADMMDantzig.h against an older ADMMBase).  Restated
 * on the current ADMMBase::solve (admm_amd/csrc/dantzig.hip, oracle/solvers.py Dantzig).  Arguments as admm_hip_lasso; opts->rho
 * <= 0: automatic (1 / loose Lanczos value of X'X).  Everything is double: beta_out[(p + 1) * nl] column-major, row 0 = intercept.
 * niter_out[l] = maxit + 1 when lambda l did not converge.  NOTE (tests/test_oracle_dantzig.py): the iteration converges on
 * comfortably tall problems (n >= 5 p) and does not for p > n -- the algorithm as the reference holds it.
 * _traced: decision records, layout ADMM_TRACE_* ([0] lambda index, [11] internal lambda; CONVERGED / CONTINUE). */
ADMM_HIP_API int admm_hip_dantzig(const double* x, const double* y, int n, int p, int mem,
                                  const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                  int standardize, int intercept, const admm_opts* opts,
                                  double* lambda_out, double* beta_out, int* niter_out, admm_stats* stats);
ADMM_HIP_API int admm_hip_dantzig_traced(const double* x, const double* y, int n, int p, int mem,
                                         const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                         int standardize, int intercept, const admm_opts* opts,
                                         double* lambda_out, double* beta_out, int* niter_out, admm_stats* stats,
                                         double* trace_out, long long trace_cap, long long* ntrace_out);

/* Basis pursuit with the COLUMNS of x in `nthread` blocks -- what R's admm_bp(x, y)$parallel(nthread)$fit() asks for:
 * .Call("admm_parbp", x, y, nthread, list(maxit, eps_abs, eps_rel, rho_ratio = rho)) (R/10_admm_bp.R:111-116), a symbol the
 * reference never builds (src/TODO/ParBP.cppp:26-71, src/TODO/PADMMBP.h against a base class that no longer exists).  The
 * feature-split "sharing" ADMM of that source, restated on the current PADMMBase_Master loop (admm_amd/csrc/sharing_bp.hip,
 * oracle/solvers.py SharingBP).  opts->rho carries rho_ratio (R default 1): rho = 1 / (rho_ratio * mean_i lambda_max(A_i'A_i)).
 * Partition as PADMMBP.h:150-167: nthread - 1 blocks of p div nthread columns, the last takes the remainder.  n <= 16384.
 * beta_out[p] dense doubles (the reference returns a one-column dgCMatrix), niter_out[1] (maxit + 1 when not converged, as
 * PADMMBase_Master::solve returns).  _traced: decision records as for admm_hip_bp_traced ([11] = 1 on a regular iteration,
 * outcome ADMM_TRACE_CONVERGED / ADMM_TRACE_CONTINUE).
 * _dist: the blocks spread over the ranks of the attached communicator -- this rank passes columns
 * [col_offset, col_offset + p_local) of the p_total, whole blocks of the partition above, and gets their coefficients back;
 * one sum all-reduce of n + O(n / 32) doubles per iteration (the "all-reduce of X_i beta_i" of SURVEY.md section 8f row n2). */
/* admm_hip_parbp / _traced with PAR_DEVICES (as admm_hip_parlasso above): N = the largest divisor of nthread that is <= the number of
 * listed devices; rank r runs admm_hip_parbp_dist on its whole blocks of columns on its own device; beta_out is assembled from the
 * ranks' column blocks, niter_out / stats / the trace are rank 0's (the decisions are replicated on every rank). */
ADMM_HIP_API int admm_hip_parbp(const double* x, const double* y, int n, int p, int mem, int nthread, const admm_opts* opts,
                                double* beta_out, int* niter_out, admm_stats* stats);
ADMM_HIP_API int admm_hip_parbp_traced(const double* x, const double* y, int n, int p, int mem, int nthread, const admm_opts* opts,
                                       double* beta_out, int* niter_out, admm_stats* stats,
                                       double* trace_out, long long trace_cap, long long* ntrace_out);
ADMM_HIP_API int admm_hip_parbp_dist(const double* x_cols, const double* y, int n, int p_local, long long p_total, long long col_offset,
                                     int mem, int nthread, const admm_opts* opts, double* beta_local_out, int* niter_out,
                                     admm_stats* stats);

/* admm_hip_lad / admm_hip_bp that also return the decision trace (layout below, ADMM_TRACE_*; lambda index 0):
 * trace_out receives min(decisions taken, trace_cap) records of ADMM_TRACE_FIELDS doubles, *ntrace_out their number. */
ADMM_HIP_API int admm_hip_lad_traced(const double* x, const double* y, int n, int p, int mem, int intercept, const admm_opts* opts,
                        double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out);
ADMM_HIP_API int admm_hip_bp_traced(const double* x, const double* y, int n, int p, int mem, const admm_opts* opts,
                       double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out);

/* admm_hip_lad_traced / admm_hip_bp_traced that also return the ITERATE DUMP (test / diagnosis facility, oracle/stepcheck.py):
 * state_out receives min(decisions taken, state_cap) records of 5 * dim doubles  x | z | y | adj_z | adj_y  (main_x, aux_z, dual_y
 * and the extrapolated pair the iteration started from, FADMMBase.h:185-211; dim = n for LAD, ADMMLAD.h:62-107, p for BP,
 * ADMMBP.h:48-93), record s = the iterates trace record s judged; record 0 (the cold start) carries in its x slot the data
 * vector as the library holds it (LAD: the standardised y; BP: A'(AA')^-1 b, ADMMBP.h:170).  Needs trace_cap > 0. */
ADMM_HIP_API int admm_hip_lad_state(const double* x, const double* y, int n, int p, int mem, int intercept, const admm_opts* opts,
                       double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out,
                       double* state_out, long long state_cap, long long* nstate_out);
ADMM_HIP_API int admm_hip_bp_state(const double* x, const double* y, int n, int p, int mem, const admm_opts* opts,
                      double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out,
                      double* state_out, long long state_cap, long long* nstate_out);

/* Quantile regression (no counterpart in the reference): minimise sum_i rho_tau(y_i - b0 - x_i'b), rho_tau(r) = tau r for r >= 0 and
 * (tau - 1) r below, for every tau[k] of a grid -- admm_hip_lad's loop (ADMMLAD.h with z = X b - y) with the prox of
 * g(z) = 2 sum rho_tau(-z_i): thresholds 2 (1 - tau) / rho above and 2 tau / rho below; tau = 0.5 without intercept is admm_hip_lad
 * bit for bit.  The setup (X'X, its inverse, the hat matrix for n <= 2000) is paid once per call; every tau runs from a cold start.
 * n > 2000 and p + intercept <= 6144: several quantiles advance per pass over X (option QUANT_SLOTS) -- every column is bit-identical
 * to the same tau fitted alone.
 * INTERCEPT: unlike admm_hip_lad, which recovers it as mean(y) - mean(x)'b (LAD.cpp:41: right for no tau but by symmetry of the
 * noise), the intercept is FITTED: x is standardised as LAD's (DataStd flag 3 / 1), a column of ones is appended and the loop fits
 * p + 1 coefficients.  Hence n > p + intercept.
 * tau[ntau] (1 <= ntau <= 4096) strictly inside (0, 1), in any order, repeats allowed.  beta_out[(p + 1) * ntau]: column k = tau[k],
 * intercept first (0 when intercept = 0); niter_out[ntau] as admm_hip_lad's.  stats->xupdate_variant: 0 / 1 as admm_hip_lad when the
 * quantiles ran one after another, 8 + S when S >= 2 ran per pass.
 * _state: one tau with the decision trace and (state_cap > 0) the iterate dump, layouts as admm_hip_lad_state (dim = n). */
ADMM_HIP_API int admm_hip_quantreg(const double* x, const double* y, int n, int p, int mem, int intercept, const double* tau, int ntau,
                      const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats);
ADMM_HIP_API int admm_hip_quantreg_state(const double* x, const double* y, int n, int p, int mem, int intercept, double tau, const admm_opts* opts,
                            double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out,
                            double* state_out, long long state_cap, long long* nstate_out);

/* Huber and expectile regression (no counterpart in the reference): minimise sum_i w_tau(r_i) H_delta(r_i), r_i = y_i - b0 - x_i'b, with
 * H_delta(r) = r^2 / 2 for |r| <= delta and delta |r| - delta^2 / 2 beyond, w_tau(r) = 2 tau for r >= 0 and 2 (1 - tau) below, for
 * every pair (delta[k], tau[k]) -- admm_hip_quantreg's loop, setup, fitted intercept (n > p + intercept) and slots (option QUANT_SLOTS)
 * with the prox of the weighted Huber function.  tau = 0.5: the Huber loss; delta = +inf: expectile regression (asymmetric least
 * squares); both: least squares.  delta is in the units of y (no scale is estimated), > 0, +inf allowed; tau strictly inside (0, 1),
 * tau = NULL: 0.5 for every fit.  1 <= nfit <= 4096, any order, repeats allowed; every fit runs from a cold start.
 * beta_out[(p + 1) * nfit]: column k = fit k, intercept first (0 when intercept = 0); niter_out[nfit]; stats->xupdate_variant as
 * admm_hip_quantreg's (0 / 1 serial, 8 + S with S fits per pass over X).
 * _state: one fit with the decision trace and (state_cap > 0) the iterate dump, as admm_hip_quantreg_state; record 0 of the dump
 * (the standardised y in its x slot) also carries the knee the loop ran with, delta / scaleY, as the first entry of its z slot. */
ADMM_HIP_API int admm_hip_huber(const double* x, const double* y, int n, int p, int mem, int intercept, const double* delta, const double* tau, int nfit,
                   const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats);
ADMM_HIP_API int admm_hip_huber_state(const double* x, const double* y, int n, int p, int mem, int intercept, double delta, double tau, const admm_opts* opts,
                         double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out,
                         double* state_out, long long state_cap, long long* nstate_out);

/* Logistic regression (no counterpart in the reference): minimise sum_i log(1 + exp(-s_i (b0 + x_i'b))), s_i = 2 y_i - 1, the binomial
 * negative log-likelihood, unpenalised -- admm_hip_lad's loop on the sign-folded matrix diag(s) [x_std | 1] with a ZERO response and the
 * prox of g(z) = sum log(1 + e^-z_i), which has no closed form: per row the root of z - v - sigma(-z) / rho by a clamped Newton
 * iteration (float seed, double polish; within 1e-13 max(1, |v|, 1 / rho) of the exact root for 1e-3 <= rho <= 1e3, any finite v; a
 * smaller rho only takes more steps, none is refused).  Setup, the three branches (hat matrix for n <= 2000, one pass over X to 6144
 * columns, two passes beyond) and the control are admm_hip_lad's.  x is standardised as admm_hip_quantreg's, always, and the intercept
 * is FITTED (ones column): n > p + intercept.
 * y[n]: labels, every one exactly 0.0 or 1.0 (anything else, NaN included: ADMM_ERR_INVALID_ARG) and both classes present; labels in
 * device memory are checked on the device.  One label vector per call: no grid, no slots (the folded matrix depends on the labels),
 * no class or observation weights, no penalty on b, no multi-GPU form.
 * beta_out[p + 1]: intercept first (0 when intercept = 0); niter_out[1] as admm_hip_lad's: a fit that has not converged within
 * opts->maxit returns ADMM_OK with maxit + 1 and finite coefficients -- perfectly separable labels end there, the maximum-likelihood
 * estimate does not exist.  stats->xupdate_variant: 0 (hat matrix, two passes) or 1 (one pass).
 * _state: the decision trace and (state_cap > 0) the iterate dump, layouts as admm_hip_lad_state (dim = n); record 0 of the dump
 * carries the zero response in its x slot and the n signs s_i the loop ran with in its z slot. */
ADMM_HIP_API int admm_hip_logit(const double* x, const double* y, int n, int p, int mem, int intercept, const admm_opts* opts,
                   double* beta_out, int* niter_out, admm_stats* stats);
ADMM_HIP_API int admm_hip_logit_state(const double* x, const double* y, int n, int p, int mem, int intercept, const admm_opts* opts,
                         double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out,
                         double* state_out, long long state_cap, long long* nstate_out);

/* Logistic regression for k label columns of one design matrix (one-vs-rest multiclass, multi-label): column c of the result is
 * admm_hip_logit(x, column c of y), number for number (niter and every coefficient equal; only the sign of an exact zero may differ),
 * but the upload, the standardisation, the Gram matrix, its inverse, the transpose and the hat matrix are formed ONCE.  Nothing is
 * folded into the matrix here: the loop runs on [x_std | 1] with a zero response and the prox takes the row's sign itself,
 * s logit2(s v, 1 / rho) -- multiplication by +-1 is exact and rounding is symmetric in sign.  On the one-pass branch (n > 2000, up to
 * 5120 columns with the intercept) several columns advance on one pass over the rows of x ("slots", as admm_hip_huber's): option
 * QUANT_SLOTS, 0 = automatic (as many as the layout admits: measured), 1 = serial, 2 ... 8 = at most that many,
 * clipped to what the shape's register layout holds (4 to 3072 columns, 2 to 4096, 1 beyond) and to k, and only while the n x k vectors stay under 2 GB.
 * y[n * k]: column-major labels in the memory space `mem` names; every column as admm_hip_logit's y.  A refusal names the first
 * offending column, 0-based ("column 3 of y: every label must be exactly 0 or 1", "column 3 of y must hold both classes"); k < 1:
 * "y must have at least one column".  A refusal touches no output.
 * beta_out[(p + 1) * k]: column-major, intercept first in each column; niter_out[k].  stats->xupdate_variant: 8 + slots on the slotted
 * route, else 1 (one pass) or 0 (hat matrix, two passes).  There is no trace / state form.  Not offered: a softmax / multinomial
 * likelihood, class or observation weights, any penalty on b, warm starts between columns, a multi-GPU form. */
ADMM_HIP_API int admm_hip_logit_multi(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const admm_opts* opts,
                         double* beta_out, int* niter_out, admm_stats* stats);

/* Ridge (L2-penalised) logistic regression for k label columns and a grid of nlambda penalties.  Per label column c and lambda_l:
 *     minimise  sum_i log(1 + exp(-s_i (b0 + x~_i'b))) + (lambda_l / 2) sum_j b_j^2,   s = 2 y - 1,
 * x~ the library's standardised columns (always standardised, as admm_hip_logit), b on the standardised scale, the intercept never
 * penalised; scikit-learn's C is 1 / lambda on standardised x.  Unlike the unpenalised calls it has a unique answer on perfectly
 * separable labels and there is NO n > p condition (n >= 2).  The penalty is not written on b: it becomes p more rows sqrt(lambda) e_j'
 * with a zero response and the loss z^2 / 2, so the Gram matrix of the augmented matrix is X'X + lambda D whatever rho does, and the
 * loop is admm_hip_logit_multi's (hat matrix for n + p <= 2000, else one pass / two passes, QUANT_SLOTS as there) with one more case
 * in the prox: a row of sign 0 takes z = v (rho / (1 + rho)).  The upload, the standardisation, the Gram matrix of the data rows and the
 * transpose are formed once per call; the inverse (and the hat matrix) once per lambda.  lambda is used in the order given and EVERY
 * fit starts cold.  The ridge rows are stored and streamed dense: p / (n + p) more bytes per iteration than admm_hip_logit_multi.
 * y[n * k]: column-major labels as admm_hip_logit_multi's, with its refusals; further "lambda must not be NULL", "lambda must have at
 * least one value", "every lambda must be finite and positive (lambda = 0 is admm_hip_logit_multi)", "nrow(x) must be at least 2".
 * A refusal touches no output.
 * beta_out[(p + 1) * k * nlambda]: entry ((l * k + c) * (p + 1) + j), intercept first, on the caller's scale; niter_out[k * nlambda]:
 * entry l * k + c, maxit + 1 = not converged.  stats->xupdate_variant: 8 + slots on the slotted route, else 1 (one pass) or 0.
 * QUANT_SLOTS = 0 (automatic) takes as many slots as the layout admits (4 to 3072 columns counting the intercept, 2 to 4096, 1 beyond),
 * clipped to k: measured + 31 ... + 60 % over the serial route (profiles/logit_ridge.md).
 * An l1 / elastic-net penalty is admm_hip_logit_enet's, below.  Not offered: observation or class weights, softmax, warm starts along
 * the grid, a multi-GPU form. */
ADMM_HIP_API int admm_hip_logit_ridge(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const double* lambda, int nlambda,
                         const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats);
/* One label vector and one lambda, with the decision trace and the iterate dump of the AUGMENTED loop: records x | z | y | adj_z | adj_y
 * of n + p entries each (state_out: state_cap * 5 * (n + p) doubles); record 0 carries the zero response in its x slot and, in its z
 * slot, the n + p "signs" the loop ran with: 2 y - 1, then p zeros (the ridge rows). */
ADMM_HIP_API int admm_hip_logit_ridge_state(const double* x, const double* y, int n, int p, int mem, int intercept, double lambda, const admm_opts* opts,
                         double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap, long long* ntrace_out,
                         double* state_out, long long state_cap, long long* nstate_out);

/* Elastic-net (l1 / l1 + l2) logistic regression for k label columns and ncell (lambda, alpha) PAIRS, as admm_hip_huber's (delta, tau)
 * are pairs.  Per label column c and cell l:
 *     minimise  sum_i log(1 + exp(-s_i (b0 + x~_i'b))) + lambda_l (alpha_l sum_j |b_j| + (1 - alpha_l) / 2 sum_j b_j^2),   s = 2 y - 1,
 * x~ the library's standardised columns, b on the standardised scale, the intercept never penalised: glmnet family = "binomial" with
 * its lambda times n, scikit-learn penalty = "l1" / "elasticnet".  alpha = 1 is the lasso, alpha = 0 admm_hip_logit_ridge's problem.
 * n >= 2; there is no n > p condition.  The penalty is admm_hip_logit_ridge's p more rows with the penalty's constants moved from the
 * row into the prox: the rows are sqrt(n) e_j' for EVERY cell (sqrt(n): a standardised column's norm; unit rows cost 10 - 100 times
 * the iterations) and a row of sign 0 takes z = soft(v, t) / d, t = (lambda alpha / sqrt(n)) / rho, d = 1 + (lambda (1 - alpha) / n) / rho.
 * So the Gram matrix is X'X + n D for every lambda, alpha and rho: ONE Gram matrix, ONE inverse (and hat matrix, n + p <= 2000) and ONE
 * transpose per call, and all k * ncell fits run as one grid of the loop -- on the one-pass branch the QUANT_SLOTS slots refill across
 * the whole grid.  Every fit starts cold, cells in the order given.  Returned: b_j = z_{n + j} / sqrt(n) from the penalty rows of the
 * LAST z (the prox output of the final iteration: coefficients the penalty removes are exactly 0.0), the intercept from the loop's
 * coefficient read-out, recovered to the caller's scale as admm_hip_logit_multi does.
 * y[n * k]: as admm_hip_logit_ridge's, with its refusals; further "lambda and alpha must not be NULL", "lambda must have at least one
 * value" (ncell < 1), "every lambda must be finite and positive", "every alpha must lie in [0, 1]", "nrow(x) must be at least 2".
 * A refusal touches no output.
 * beta_out[(p + 1) * k * ncell]: entry ((l * k + c) * (p + 1) + j), intercept first; niter_out[k * ncell]: entry l * k + c, maxit + 1 =
 * not converged (the last z is returned all the same).  stats->xupdate_variant: 8 + slots on the slotted route, else 1 (one pass) or 0.
 * QUANT_SLOTS = 0 (automatic) takes as many slots as the layout admits (4 to 2048 columns counting the intercept, 3 to 3072, 2 to 4096,
 * 1 beyond), clipped to k * ncell: measured + 33 ... + 57 % over the serial route (profiles/logit_enet.md); 2 ... 8 take up to that many.
 * lambda = lambda_max exactly (admm_hip_logit_enet_lambda_max over alpha) is degenerate for the loop: ask for the empty model above it.
 * Not offered: penalty factors, observation or class weights, softmax, warm starts along the grid, strong-rule screening, a multi-GPU form. */
ADMM_HIP_API int admm_hip_logit_enet(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const double* lambda, const double* alpha,
                         int ncell, const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats);
/* out[k]: per label column lambda_1 = max_j |x~_j'(y_c - mean(y_c))| with the intercept, max_j |x~_j'(y_c - 1/2)| without it -- one
 * product with k right-hand sides on the standardised matrix.  For a cell with alpha > 0 the optimum has b = 0 from lambda_1 / alpha on.
 * The label validation is admm_hip_logit_enet's. */
ADMM_HIP_API int admm_hip_logit_enet_lambda_max(const double* x, const double* y, int n, int p, int k, int mem, int intercept, double* out);
/* One label vector and one cell, with the decision trace and the iterate dump of the augmented loop, in the shape of
 * admm_hip_logit_ridge_state: records of n + p entries, record 0 with the zero response in its x slot and 2 y - 1, then p zeros, in
 * its z slot. */
ADMM_HIP_API int admm_hip_logit_enet_state(const double* x, const double* y, int n, int p, int mem, int intercept, double lambda, double alpha,
                         const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap,
                         long long* ntrace_out, double* state_out, long long state_cap, long long* nstate_out);

/* Poisson regression (count data) with the elastic-net penalty, for k count columns and ncell (lambda, alpha) PAIRS.  Per count column
 * c and cell l:
 *     minimise  sum_i [exp(eta_i) - y_ic eta_i] + lambda_l (alpha_l sum_j |b_j| + (1 - alpha_l) / 2 sum_j b_j^2),   eta_i = b0 + x~_i'b,
 * x~ the library's standardised columns, b on the standardised scale, the intercept never penalised: glmnet family = "poisson" with its
 * lambda times n.  lambda = 0 is the plain Poisson GLM (log link).  It is admm_hip_logit_enet's restatement with another loss on the
 * data rows: p more rows sqrt(n) e_j' for EVERY cell, whose prox is z = soft(v, t) / d, t = (lambda alpha / sqrt(n)) / rho,
 * d = 1 + (lambda (1 - alpha) / n) / rho, and on a data row the root of z + e^z / rho = v + y / rho (Newton from the right of the root,
 * within 1e-13 max(1, |v|, y / rho, 1 / rho) of it; nothing overflows for any finite v).  So the Gram matrix is X'X + n D for every
 * lambda, alpha and rho: ONE Gram matrix, ONE inverse (and hat matrix, n + p <= 2000) and ONE transpose per call, all k * ncell fits one
 * grid of the loop, every fit from a cold start, cells in the order given.  Returned: b_j = z_{n + j} / sqrt(n) from the penalty rows of
 * the LAST z (coefficients the penalty removes are exactly 0.0), the intercept from the loop's coefficient read-out, on the caller's
 * scale, intercept first.
 * y[n * k]: column-major counts, finite and >= 0; non-integers are accepted (quasi-likelihood use).  Refusals, each touching no output:
 * the argument checks of admm_hip_logit_enet and "every y must be finite and non-negative", "every column of y must have a positive
 * sum", "every lambda must be finite and non-negative", "every alpha must lie in [0, 1]", "lambda = 0 needs nrow(x) > ncol(x) +
 * intercept", "nrow(x) must be at least 2".
 * beta_out[(p + 1) * k * ncell]: entry ((l * k + c) * (p + 1) + j); niter_out[k * ncell]: entry l * k + c, maxit + 1 = not converged
 * (the last z is returned all the same).  stats->xupdate_variant: 8 + slots on the slotted route, else 1 (one pass) or 0.
 * QUANT_SLOTS = 2 ... 8 take up to that many slots on the one-pass branch (4 to 2048 columns counting the intercept, 3 to 3072, 2 to
 * 4096, 1 beyond), clipped to k * ncell; 0 (automatic) takes as many as the layout admits: measured + 33 ... + 62 % over the serial
 * route (profiles/poisson.md).
 * Not offered: an exposure offset, observation weights, penalty factors, negative-binomial or other dispersion models, warm starts
 * along the grid, strong-rule screening, a multi-GPU form. */
ADMM_HIP_API int admm_hip_poisson(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const double* lambda, const double* alpha,
                         int ncell, const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats);
/* out[k]: per count column lambda_1 = max_j |x~_j'(y_c - mean(y_c))| with the intercept, max_j |x~_j'(y_c - 1)| without it (mu = 1 at
 * eta = 0) -- one product with k right-hand sides on the standardised matrix.  For a cell with alpha > 0 the optimum has b = 0 from
 * lambda_1 / alpha on.  The count validation is admm_hip_poisson's. */
ADMM_HIP_API int admm_hip_poisson_lambda_max(const double* x, const double* y, int n, int p, int k, int mem, int intercept, double* out);
/* One count vector and one cell, with the decision trace and the iterate dump of the augmented loop: records x | z | y | adj_z | adj_y of
 * n + p entries each; record 0 carries the zero response in its x slot and the counts followed by p entries of -1.0 (the penalty rows'
 * marker) in its z slot. */
ADMM_HIP_API int admm_hip_poisson_state(const double* x, const double* y, int n, int p, int mem, int intercept, double lambda, double alpha,
                         const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats, double* trace_out, long long trace_cap,
                         long long* ntrace_out, double* state_out, long long state_cap, long long* nstate_out);

/* K-fold cross-validation of admm_hip_logit_enet's / admm_hip_poisson's (column, cell) grid: cv.glmnet for family = "binomial" /
 * "poisson", by held-out deviance.  A held-out row is a row whose loss is zero, and the prox of the zero function is the identity: a
 * fold's fit runs on the FULL augmented matrix with its held-out rows tagged (2.0 among the signs, -2.0 among the counts), which is
 * exactly the training rows' problem.  So the upload, the standardisation, the Gram matrix X'X + n D, the inverse (hat matrix) and the
 * transpose are the full-data call's, formed ONCE, and the k * ncell * (nfolds + 1) fits are one grid of the loop: cell-major, then
 * fold slot (0 = nothing held out, f + 1 = fold f), then column; slots (QUANT_SLOTS) refill across all of them.
 * A fold's stop thresholds are the training rows' too: its held-out rows stay out of the norms that scale them and out of their sqrt(rows).
 * fold_id[n]: host ints in [0, nfolds), or NULL = i mod nfolds (admm_hip_lasso_cv's default).
 * beta_out[(p + 1) * k * ncell], niter_out[k * ncell]: the full-data fit, number for number what admm_hip_logit_enet / admm_hip_poisson
 * return for the same arguments.
 * fold_dev[nfolds * ncell * k], entry ((f * ncell + l) * k + c): the MEAN deviance of fold f's rows under fold f's fit of (c, l), formed
 * on the device in double from the standardised coefficients and the matrix the loop holds, eta_i = b0 + x~_i'b --
 *     binomial: 2 (max(-s eta, 0) + log1p(exp(-|eta|))), s = 2 y - 1;    Poisson: 2 (y log(y / mu) - (y - mu)), mu = exp(eta), 0 log 0 = 0
 * -- every sum in a fixed order (no atomics): the same bits on every run.  Non-finite values are returned as they are.
 * cv_mean[k * ncell], cv_se[k * ncell], entry l * k + c: the unweighted mean over the folds and the sample sd over the folds / sqrt(nfolds)
 * (admm_hip_lasso_cv's convention).  idx_min[k]: per column the cell of the smallest cv_mean (the first on ties).  idx_1se[k]: among the
 * cells with alpha = alpha[idx_min], the one with the largest lambda whose cv_mean <= cv_mean[idx_min] + cv_se[idx_min].
 * fold_niter[nfolds * ncell * k], fold_beta[nfolds * ncell * k * (p + 1)]: fold-major, then as niter_out / beta_out.  fold_dev,
 * fold_niter, fold_beta, idx_min and idx_1se may be NULL.
 * Refusals (ADMM_ERR_INVALID_ARG, no output touched): the checks of admm_hip_logit_enet / admm_hip_poisson, and nfolds outside [2, n], a
 * fold_id outside [0, nfolds), an empty fold, a training set that lacks a class (zero sum of counts) in some column, lambda = 0 (Poisson)
 * with some training set of at most p + intercept rows.
 * Limits: the folds use the FULL-data standardisation and c^2 = n (lambda means the same in every fold and in the final fit; glmnet
 * re-standardises per fold); a fold's fit streams all n rows; every fit starts cold; deviance only; no observation weights, no
 * multi-GPU form, no cross-validation of admm_hip_logit_ridge. */
ADMM_HIP_API int admm_hip_logit_enet_cv(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const int* fold_id, int nfolds,
                         const double* lambda, const double* alpha, int ncell, const admm_opts* opts, double* beta_out, int* niter_out, double* cv_mean,
                         double* cv_se, double* fold_dev, int* fold_niter, double* fold_beta, int* idx_min, int* idx_1se, admm_stats* stats);
ADMM_HIP_API int admm_hip_poisson_cv(const double* x, const double* y, int n, int p, int k, int mem, int intercept, const int* fold_id, int nfolds,
                         const double* lambda, const double* alpha, int ncell, const admm_opts* opts, double* beta_out, int* niter_out, double* cv_mean,
                         double* cv_se, double* fold_dev, int* fold_niter, double* fold_beta, int* idx_min, int* idx_1se, admm_stats* stats);
/* One column, one cell, one fold of the calls above (fold = -1: nothing held out; the folds' checks are those of the grid call), with the
 * decision trace and the iterate dump exactly as admm_hip_logit_enet_state / admm_hip_poisson_state: record 0's z slot carries the tags
 * the loop ran with, the held-out marker (2.0 / -2.0) on the rows of the fold. */
ADMM_HIP_API int admm_hip_logit_enet_cv_state(const double* x, const double* y, int n, int p, int mem, int intercept, const int* fold_id, int nfolds, int fold,
                         double lambda, double alpha, const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats, double* trace_out,
                         long long trace_cap, long long* ntrace_out, double* state_out, long long state_cap, long long* nstate_out);
ADMM_HIP_API int admm_hip_poisson_cv_state(const double* x, const double* y, int n, int p, int mem, int intercept, const int* fold_id, int nfolds, int fold,
                         double lambda, double alpha, const admm_opts* opts, double* beta_out, int* niter_out, admm_stats* stats, double* trace_out,
                         long long trace_cap, long long* ntrace_out, double* state_out, long long state_cap, long long* nstate_out);

/* Prepared-problem variant of the Lasso family (the "persistent context" anticipated for a
 * re-fitting caller; the R shim does not need it).  create = everything the reference does
 * before its lambda loop (copy/convert, DataStd, X'y, Gram, Spectra, factorisation:
 * Lasso.cpp:42-76 + ADMM*::init); run = the warm-started lambda loop of Lasso.cpp:97-124 from a
 * cold start, repeatable; destroy frees all device memory.  alpha < 0 selects the Lasso prox,
 * 0 <= alpha <= 1 the elastic net; nthread > 1 selects the consensus solver (Lasso only: alpha >= 0 with nthread > 1 is
 * ADMM_ERR_INVALID_ARG -- the reference has no parallel elastic net).
 * bench.py times run() only (ADMM iterations/s excludes the one-time setup). */
typedef struct admm_hip_plan admm_hip_plan;
ADMM_HIP_API int admm_hip_lasso_plan_create(const double* x, const double* y, int n, int p, int mem,
                               const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                               int standardize, int intercept, double alpha, int nthread, const admm_opts* opts,
                               admm_hip_plan** plan_out, int* nlambda_out);
ADMM_HIP_API int admm_hip_lasso_plan_run(admm_hip_plan* plan, double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats);
ADMM_HIP_API int admm_hip_lasso_plan_destroy(admm_hip_plan* plan);

/* Group lasso on the tall path (n > p only; not in the reference package):
 *     minimise 1/2 ||y_s - X_s b||^2 + lambda_int sum_g w_g ||b_g||_2
 * in the solver's internal units (standardised data, lambda_int = lambda n / scaleY as for admm_hip_lasso).  The iteration is the
 * tall solver's fast ADMM with the z-update replaced by a block soft-threshold (lasso_tall.hip, tall_group_tail_kernel); the lambda
 * path, the stopping rule, niter (maxit + 1 on exhaustion) and the outputs are admm_hip_lasso's.
 * group[p]: the group id of every column -- 0 .. ngroups - 1, non-decreasing, starting at 0, without gaps (groups are runs of
 * adjacent columns).  group_weight[ngroups] >= 0, at least one > 0; NULL selects sqrt(group size).  A group of one column with weight
 * w is a Lasso coefficient with penalty factor w; weight 0 leaves a group unpenalised.  A group holds at most ADMM_HIP_GROUP_MAX
 * columns; larger groups are refused.  Single device; the row-sharded, refined (REFINE), cross-validated and multi-response forms of
 * the Lasso do not exist for it (REFINE set: refused).
 * Automatic grid: lambda_0 = max over the groups with w_g > 0 of ||(X_s'y_s)_g||_2 / w_g.  With unpenalised groups present the
 * first lambda of that grid is NOT guaranteed to give an empty penalised model (the unpenalised columns have not been fitted
 * when lambda_0 is taken): pass a grid of your own there.
 * The plan is an ordinary admm_hip_plan: admm_hip_lasso_plan_run / _trace_* / _state_* / _destroy work on it. */
#define ADMM_HIP_GROUP_MAX 1024
ADMM_HIP_API int admm_hip_grplasso(const double* x, const double* y, int n, int p, int mem,
                                   const int* group, const double* group_weight, int ngroups,
                                   const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                   int standardize, int intercept, const admm_opts* opts,
                                   double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats);
ADMM_HIP_API int admm_hip_grplasso_plan_create(const double* x, const double* y, int n, int p, int mem,
                                               const int* group, const double* group_weight, int ngroups,
                                               const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                               int standardize, int intercept, const admm_opts* opts,
                                               admm_hip_plan** plan_out, int* nlambda_out);

/* Sparse-group lasso on the tall path (n > p only; not in the reference package; Simon, Friedman, Hastie and Tibshirani 2013, the R
 * packages SGL and sparsegl): groups are selected and so are coefficients inside the groups that stay,
 *     minimise 1/2 ||y_s - X_s b||^2 + lambda_int [ alpha sum_j u_j |b_j| + (1 - alpha) sum_g w_g ||b_g||_2 ]
 * in the solver's internal units, as admm_hip_grplasso.  The iteration is the group lasso's with the z-update  soft-threshold every
 * coordinate by lambda alpha u_j / rho, then block soft-threshold every group by lambda (1 - alpha) w_g / rho  (the exact prox of the
 * sum; lasso_tall.hip, tall_group_tail_kernel<., true>); the lambda path, the stopping rule, niter and the outputs are admm_hip_lasso's.
 * group, group_weight, ngroups: as admm_hip_grplasso (group_weight NULL = sqrt(group size); a weight of 0 leaves only the l1 part).
 * l1_weight[p] >= 0: one l1 weight per column, NULL = all 1.  0 <= alpha <= 1.  Coordinate j of group g is unpenalised when
 * alpha u_j = 0 and (1 - alpha) w_g = 0; a call in which no coordinate carries a positive penalty is refused.
 * alpha = 0 is admm_hip_grplasso bit for bit (grid, coefficients, niter, decision trace).  alpha = 1 is the Lasso with the penalty
 * factors u on the tall path: with u = 1 it is admm_hip_lasso bit for bit for any grouping, and with a general u
 * admm_hip_grplasso on one-column groups of weights u.  (A call in which no group carries a block weight -- alpha = 1, or every
 * w_g = 0 -- has no block structure left and runs on the Lasso tail's tiling, every column a one-column group of weight alpha u_j.)
 * Limits as admm_hip_grplasso: groups of at most ADMM_HIP_GROUP_MAX columns, single device; no row-sharded, consensus, elastic-net,
 * refined (REFINE set: refused), cross-validated or multi-response form.
 * Automatic grid: lambda_0 = max_g lambda_g, lambda_g the smallest lambda at which the prox empties group g started from c = X_s'y_s:
 * the root of  sum_{j in g} max(|c_j| - lambda alpha u_j, 0)^2 = ((1 - alpha) w_g lambda)^2 , solved exactly over its breakpoints
 * (sgl_host.h); groups that no lambda empties are left out.  With unpenalised coordinates present the first lambda of that grid is
 * NOT guaranteed to give an empty penalised model (the unpenalised columns have not been fitted when lambda_0 is taken): pass a
 * grid of your own there.
 * The plan is an ordinary admm_hip_plan: admm_hip_lasso_plan_run / _trace_* / _state_* / _destroy work on it. */
ADMM_HIP_API int admm_hip_sgl(const double* x, const double* y, int n, int p, int mem,
                              const int* group, const double* group_weight, int ngroups, const double* l1_weight, double alpha,
                              const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                              int standardize, int intercept, const admm_opts* opts,
                              double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats);
ADMM_HIP_API int admm_hip_sgl_plan_create(const double* x, const double* y, int n, int p, int mem,
                                          const int* group, const double* group_weight, int ngroups, const double* l1_weight, double alpha,
                                          const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                          int standardize, int intercept, const admm_opts* opts,
                                          admm_hip_plan** plan_out, int* nlambda_out);

/* Box-constrained, weighted elastic net on the tall path (n > p only; not in the reference package; glmnet's lower.limits /
 * upper.limits / penalty.factor for family = "gaussian", scikit-learn's positive = True):
 *     minimise 1/2 ||y_s - X_s b||^2 + lambda_int sum_j u_j [ alpha |b_j| + (1 - alpha)/2 b_j^2 ]   subject to   lo_j <= b_j <= hi_j
 * in the solver's internal units (standardised X_s, y_s; lambda_int = lambda n / scaleY), as admm_hip_lasso.  The iteration is the
 * Lasso's with the z-update  prox of coordinate j's penalty, then clamp to [lo_j, hi_j]  -- the exact minimiser of the one-dimensional
 * convex problem, because the box holds zero (lasso_tall.hip, tall_box_tail_kernel); the lambda path, the stopping rule, niter and the
 * outputs are admm_hip_lasso's.
 * alpha < 0 selects the Lasso prox (admm_hip_lasso's: compare in double), 0 <= alpha <= 1 the elastic net's (admm_hip_enet's: float
 * threshold and denominator), the convention of admm_hip_lasso_cv; alpha > 1 or NaN is refused.
 * penalty_factor[p] >= 0: u_j multiplies the WHOLE penalty of column j, both parts (glmnet's penalty.factor, not rescaled); NULL = all
 * 1; 0 leaves the column unpenalised; a call without a positive factor is refused.
 * lower[p], upper[p]: bounds on the ORIGINAL coefficient scale, NULL = none, -+infinity entries allowed.  lower_j <= 0 <= upper_j is
 * required and NaN refused (glmnet's rule: zero stays feasible, so the cold start and the empty model at lambda_0 stay valid);
 * lower_j = upper_j = 0 excludes column j.  The bounds go into the solver's units once, lower_j scaleX_j / scaleY in double, rounded to
 * float towards the inside of the box.  Every returned coefficient is clamped to the caller's bounds rounded inwards to float, and the
 * intercept is computed from the clamped coefficients: lower_j <= beta_j <= upper_j holds exactly in beta_out.
 * Without bounds and factors the call is admm_hip_lasso (alpha < 0) or admm_hip_enet bit for bit (grid, coefficients, niter, decision
 * trace); with factors alone and alpha < 0 it is admm_hip_sgl at alpha = 1 with l1_weight = penalty_factor.
 * Limits: single device; no wide (n <= p), row-sharded, consensus, refined (REFINE set: refused), cross-validated or multi-response
 * form; an attached communicator is refused; bounds that exclude zero are refused.  The group, sparse-group and multi-task penalties
 * take no bounds (a clamp after a block shrink is not their prox).
 * Automatic grid: with c = X_s'y_s, lambda_0 = max over u_j > 0 of g_j / u_j, g_j = max(c_j if upper_j > 0 else 0, -c_j if lower_j < 0
 * else 0) -- the smallest lambda at which no penalised coordinate may leave zero -- in double from the float c, rounded to float; the
 * elastic net divides by alpha + 1e-4 as admm_hip_enet.  With unpenalised columns present the first lambda of that grid is NOT
 * guaranteed to give an empty penalised model (the unpenalised columns have not been fitted when lambda_0 is taken): pass a grid of
 * your own there.
 * The plan is an ordinary admm_hip_plan: admm_hip_lasso_plan_run / _trace_* / _state_* / _destroy work on it. */
ADMM_HIP_API int admm_hip_boxenet(const double* x, const double* y, int n, int p, int mem,
                                  const double* lower, const double* upper, const double* penalty_factor, double alpha,
                                  const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                  int standardize, int intercept, const admm_opts* opts,
                                  double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats);
ADMM_HIP_API int admm_hip_boxenet_plan_create(const double* x, const double* y, int n, int p, int mem,
                                              const double* lower, const double* upper, const double* penalty_factor, double alpha,
                                              const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                              int standardize, int intercept, const admm_opts* opts,
                                              admm_hip_plan** plan_out, int* nlambda_out);

/* Multi-task lasso on the tall path (n > p only; not in the reference package; glmnet's family = "mgaussian", scikit-learn's
 * MultiTaskLasso): m responses on one design, one row-wise penalty that selects a feature for all responses at once,
 *     minimise over b0 (m), B (p x m):  1/(2n) ||Y - 1 b0' - X B||_F^2 + lambda sum_j w_j ||B_j.||_2 ,
 * internally 1/2 ||Y_s - X_s B||_F^2 + lambda_int sum_j w_j ||B_j.||_2 with lambda_int = lambda n / scaleY as for admm_hip_lasso.
 * It is the group lasso on X (x) I_m with p groups of m, solved with ONE rho and therefore one cached inverse: every iteration streams
 * the inverse's triangle ceil(2m / NR) times for all responses (symvn_lower_kernel, NR right-hand sides per pass: option MT_RHS)
 * where m independent fits stream it m times, and the z-update is a block soft-threshold across the responses of a row
 * (tall_mt_tail_kernel).  One stopping rule over all p m coordinates: one niter per lambda (maxit + 1 on exhaustion).
 * Y: n x m column-major doubles in the same memory as x, 1 <= m <= ADMM_HIP_MT_MAX.  x is standardised as for admm_hip_lasso; with
 * `intercept` every response is centred by its own mean; with `standardize` ALL responses are divided by one common scale,
 * sqrt(sum_k ||y_k - mean_k||^2 / (n m)) (flag combinations as DataStd's: standardize without intercept takes the norm about the mean
 * without centring), which keeps their relative sizes (glmnet's default).  m = 1 with NULL weights is admm_hip_lasso bit for bit.
 * row_weight[p] >= 0, at least one > 0; NULL = all 1 (not sqrt(m): m = 1 is then the Lasso with penalty factors).  Weight 0 leaves a
 * row unpenalised.  Automatic grid: lambda_0 = max over rows with w_j > 0 of ||(X_s'Y_s)_j.||_2 / w_j; with unpenalised rows its first
 * lambda is NOT guaranteed to give an empty penalised model (as for admm_hip_grplasso): pass a grid of your own there.
 * beta_out[nlam][m][p + 1]: for lambda l and response k the intercept followed by the p coefficients, coef_k = z_k / scaleX * scaleY,
 * b0_k = meanY_k - sum_j coef_jk meanX_j.  lambda_out[nlam], niter_out[nlam].
 * Single device; REFINE set, an attached communicator, elastic net: refused.  No wide (n <= p), cross-validated or consensus form.
 * The plan is an ordinary admm_hip_plan: admm_hip_lasso_plan_run / _trace_* / _state_* / _destroy work on it; a state record holds
 * 5 p m floats laid out [5][m][p]. */
#define ADMM_HIP_MT_MAX 16
ADMM_HIP_API int admm_hip_mtlasso(const double* x, const double* Y, int n, int p, int m, int mem,
                                  const double* row_weight,
                                  const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                  int standardize, int intercept, const admm_opts* opts,
                                  double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats);
ADMM_HIP_API int admm_hip_mtlasso_plan_create(const double* x, const double* Y, int n, int p, int m, int mem,
                                              const double* row_weight,
                                              const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                              int standardize, int intercept, const admm_opts* opts,
                                              admm_hip_plan** plan_out, int* nlambda_out);

/* Decision trace of a prepared Lasso-family problem (tall, wide and consensus solvers): what the reference's commented-out iteration table
 * (print_row, FADMMBase.h:135-170, ADMMBase.h:111-146) would print, recorded on the device by the iteration control itself, one record
 * per decision (the cold-start decision first, then one per ADMM iteration, over all lambdas of a run in order).
 * enable() before run(); read() afterwards returns min(records of the last run, capacity, cap_records) records of
 * ADMM_TRACE_FIELDS doubles:
 *   [0] lambda index  [1] iteration i within the lambda  [2] eps_primal  [3] eps_dual  (the thresholds iteration i was tested against)
 *   [4] resid_primal  [5] resid_dual  [6] c = rho r_p^2 + rho ||z - adj_z||^2 (0 when converged)  [7] c_old (adj_c before)
 *   [8] outcome ADMM_TRACE_*  [9] rho the iteration ran with  [10] rho after this decision (the adaptation of
 *   FADMMBase.h:109-133 / ADMMBase.h:85-109 where the solver adapts: wide, LAD, BP)  [11] the penalty lambda the iteration
 *   ran with, in the solver's internal units (lambda n / scaleY, Lasso.cpp:99; 0 for LAD / BP)
 * Wide solver (ADMMBase::solve, rho adaptation ADMMBase.h:85-109): [6] rho AFTER this decision's adaptation, [7] kind of
 * the x-update that follows (0 zero, 1 regular, 2 active set), [9] rho before; consensus solver: [6] = [9] = rho, [7] = 0.
 * The parity tests use it to show that a lambda whose iteration count differs from the oracle's diverged at a
 * threshold test decided inside rounding noise, instead of excusing count differences wholesale. */
#define ADMM_TRACE_FIELDS 12
#define ADMM_TRACE_COLD (-1)        /* first decision of a run: nothing to test yet */
#define ADMM_TRACE_CONVERGED 0      /* r_p < eps_p and r_d < eps_d  (FADMMBase.h:213-217,237-238) */
#define ADMM_TRACE_ACCELERATE 1     /* c < 0.999 c_old              (FADMMBase.h:243-249) */
#define ADMM_TRACE_RESTART 2        /* otherwise                    (FADMMBase.h:250-256) */
#define ADMM_TRACE_CONTINUE 1       /* wide / consensus solvers (no acceleration): not converged    (ADMMBase.h:206-207, PADMMBase.h:230-231) */
ADMM_HIP_API int admm_hip_lasso_plan_trace_enable(admm_hip_plan* plan, long long capacity_records);
ADMM_HIP_API int admm_hip_lasso_plan_trace_read(admm_hip_plan* plan, double* out, long long cap_records, long long* nrecords_out);
/* Iterate dump of a prepared problem (tall, wide and consensus solvers; test / diagnosis facility): the vectors every ADMM
 * iteration leaves behind, in the solver's own (standardised) units, one record per decision with the SAME numbering as
 * the decision trace -- record s holds the iterates whose residuals trace record s judged (record 0, the cold start, is
 * zero).  Tall solver (FADMMBase.h:185-211): 5 p floats  x | z | y | adj_z | adj_y  (main_x, aux_z, dual_y and the
 * extrapolated pair the iteration started from).  Consensus solver (PADMMBase.h:174-214), K row blocks:
 * (1 + 2 K) p floats  z | x_0 .. x_{K-1} | y_0 .. y_{K-1}.  Wide solver (ADMMBase.h:158-216, ADMMLassoWide.h:129-170; single process):
 * p + 3 n floats  x | A x | z | y  (main_x, cache_Ax, aux_z, dual_y), written by the two-launch path and by the persistent
 * active-set launches alike; record 0 is zero.  With it a test can replay the reference's arithmetic for
 * ONE iteration from the library's own previous iterates (oracle/stepcheck.py): every step of a run is then checked on its
 * own, however far two executions have drifted apart over hundreds of iterations at the rounding floor.
 * enable() before run(); read() afterwards (out may be NULL with cap_records = 0 to query the sizes). */
/* Test hook: the float system matrix X'X + rho I (p x p, column-major, leading dimension ld >= p) the tall solver's x-update solves,
 * as THIS library formed it (its Gram rounds differently from anybody else's).  Only kept with ADMM_HIP_REFINE=1. */
ADMM_HIP_API int admm_hip_lasso_plan_system_read(admm_hip_plan* plan, float* out, long long ld);
/* Test hook: the standardised data as the WIDE solver holds them -- X (n x p floats, column-major, leading dimension ld >= n) and
 * Y (n floats): DataStd's statistics are accumulated in double here, so the library's X differs from any other
 * standardisation in the last bit, and a stepwise replay of its mat-vecs needs ITS matrix.  Either output may be NULL. */
ADMM_HIP_API int admm_hip_lasso_plan_data_read(admm_hip_plan* plan, float* x_out, long long ld, float* y_out);
ADMM_HIP_API int admm_hip_lasso_plan_state_enable(admm_hip_plan* plan, long long capacity_records);
ADMM_HIP_API int admm_hip_lasso_plan_state_read(admm_hip_plan* plan, float* out, long long cap_records, long long* nrecords_out,
                                                long long* record_floats_out);

/* ---- variant selectors and tuning values (round 6: replaces the ADMM_HIP_* environment variables of earlier rounds).
 * Options belong to the CALLING THREAD and are read by the entry points when they run (a prepared problem reads them when it is
 * created): two threads can run two different variants at the same time, and nothing reads the environment per call.  The typed
 * struct carries the selectors that choose between numerically different (all parity-tested) paths; admm_hip_option_set reaches the
 * long tail of tuning / diagnostic values by name (INTEGRATION.md lists them).  Every field 0 = the library's default.
 * Values are checked when they are set: an unknown name, or a value outside what the option accepts, is refused with
 * ADMM_ERR_INVALID_ARG (the message names the option and what it takes) and the thread's settings stay as they were.
 * Debugging aid: ADMM_HIP_<NAME> environment variables present when the library is FIRST used form a process-wide overlay under
 * the thread's own settings (read once; changing the environment afterwards has no effect).  Variables that name no option are
 * ignored; a known name with a malformed value makes every entry point return ADMM_ERR_INVALID_ARG, naming the variable. */
typedef struct admm_hip_options {
    int struct_size;          /* sizeof(admm_hip_options): lets the library accept older, shorter structs */
    int gram_backend;         /* 0 hand-written matrix-core kernels, 1 rocBLAS (dlopen) */
    int gram_split;           /* tall Gram of order >= ~4000: 0 default (fp16 x 2 planes), 1 exact fp32 kernel, 2 fp16 x 2, 3 bf16 x 3 */
    int factor_backend;       /* 0 hand-written blocked Cholesky + inverse, 1 rocSOLVER (dlopen) */
    int inverse_precision;    /* cached inverse: 0 default (built in double below order 4096), 1 always float, 2 always double */
    int tall_xupdate;         /* tall x-update: 0 default (symmetric lower-triangle kernel for p >= 2048), 1 full-matrix mat-vec, 2 symmetric */
    int tall_refine;          /* 1: mixed-precision refinement of the tall x-update */
    int consensus_two_pass;   /* 1: the reference's two products per Woodbury worker (default: one-pass form) */
    int consensus_unfused;    /* 1: `pack` and `z` as two launches; 2: also one launch per worker and product */
    int bp_two_pass;          /* 1: basis pursuit with the reference's two products (default: one-pass form) */
    int lad_no_hat;           /* 1: LAD never forms the n x n hat matrix (the reference does for n <= 2000) */
    int wide_no_persist;      /* 1: wide solver without the persistent active-set stretch; 2: only the column-sharded solver without it */
    int wide_unfused;         /* 1: wide solver with three launches per iteration */
    int wide_gram_sprad;      /* 1: spectral radius from the explicit n x n Gram (default single process: Gram-free) */
    int sharing_bp_direct;    /* 1: column-block basis pursuit without Gram-space stretches */
    int cv_downdate;          /* cross-validation folds as down-dates of the full-data Gram: 0 default (when the Gram is what setup costs), 1 always, 2 never */
    int peer_exchange;        /* PEER back-end: 0 default (producer + consumer in one launch when resident), 1 two launches, 2 through the exchange layer */
    int batch_iters;          /* iterations enqueued between two host polls (0: default 16) */
    int profile_stride;       /* time every k-th x-update launch with HIP events (0: off) */
    int pool_mb;              /* cache of released device blocks: -1 off, 0 default (min(16 GB, memory / 8)), > 0 megabytes */
    int screen;               /* wide solver and admm_hip_parbp: regular steps screened through a 1- or 2-byte copy of the matrix (bit-identical
                                 iterates, a quarter to a half of the bytes): 0 default (when the matrix streams from HBM; the wide solver
                                 picks the 8-bit code where its bounds are tight enough, else fp16), 1 always (fp16), 2 never, 3 always, wide
                                 solver with the 8-bit code */
    int lad_two_pass;         /* 1: LAD with the reference's two products per iteration (default: one pass over the rows of X, p <= 6144) */
    int par_devices;          /* admm_hip_parlasso / admm_hip_parbp in-process over several devices (named option PAR_DEVICES):
                                 0 off (default), -1 every device (PAR_DEVICES=all), k > 0 devices 0 .. k-1 */
    int reserved[9];
} admm_hip_options;
ADMM_HIP_API int admm_hip_options_default(admm_hip_options* o);               /* zero-fills and sets struct_size */
ADMM_HIP_API int admm_hip_options_set(const admm_hip_options* o);             /* NULL: back to the defaults (keeps nothing of the thread's earlier settings) */
ADMM_HIP_API int admm_hip_option_set(const char* name, const char* value);    /* one value by name ("GRAM_SPLIT", "f16x2"; case-insensitive,
                                                                                 ADMM_HIP_ prefix optional); value NULL: back to the default;
                                                                                 unknown name / malformed value: ADMM_ERR_INVALID_ARG, nothing changed */
ADMM_HIP_API int admm_hip_options_reset(void);
ADMM_HIP_API const char* admm_hip_option_get(const char* name);               /* value in force for this thread, or NULL (library default) */

/* ---- one process per GPU: consensus Lasso with its row blocks spread over ranks (RCCL over xGMI).
 * Bootstrap: rank 0 calls admm_hip_comm_unique_id and ships the ADMM_HIP_UNIQUE_ID_BYTES bytes to the
 * other ranks over any channel (bench.py uses torch.distributed); every rank then calls
 * admm_hip_comm_init on its own device.  In the *_dist entry points x/y are this rank's contiguous
 * ROW SLICE of the global n_total x p problem, in the reference's partition (PADMMLasso.h:163-179:
 * nthread blocks of n_total / nthread rows, the last block takes the remainder; rank r owns blocks
 * [r * nthread / nranks, (r+1) * nthread / nranks)).  Standardisation uses the global column moments
 * (the reference standardises before it splits, ParLasso.cpp:68-72); per ADMM iteration the ranks
 * exchange ONE grouped all-reduce: the consensus sum (p floats) and three squared norms.  Every rank
 * returns the full result.  nthread >= 1 in these two entry points. */
#define ADMM_HIP_UNIQUE_ID_BYTES 128
ADMM_HIP_API int admm_hip_comm_unique_id(void* id_out);
ADMM_HIP_API int admm_hip_comm_init(int nranks, int rank, const void* id);
ADMM_HIP_API int admm_hip_comm_finalize(void);
/* What the attached communicator REALLY holds (RCCL: ncclCommCount / ncclCommUserRank of the live communicator; SHM: ranks attached to
 * the segment; PEER: exchange buffers mapped): *nranks_out = 1, *rank_out = 0, *backend_out = 0 when none is attached;
 * backend 1 RCCL, 2 SHM, 3 PEER.  A launcher (bench.py) checks this against the number of GPUs it was asked to use. */
ADMM_HIP_API int admm_hip_comm_info(int* nranks_out, int* rank_out, int* backend_out);
/* Two more exchange backends behind the same entry points (one of the three is attached at a time; comm.h):
 *  - PEER: one-shot all-reduce over peer-mapped device memory.  Every rank calls admm_hip_comm_peer_prepare on its own
 *    device (allocates its exchange buffer, returns its ADMM_HIP_PEER_HANDLE_BYTES-byte hipIpc handle), the caller
 *    gathers the handles of all ranks in rank order over any channel, then every rank calls admm_hip_comm_init_peer.
 *    The ranks may be processes on different GPUs of one node (xGMI) or -- for tests -- on the same GPU.
 *  - SHM: through a POSIX shared-memory segment `name` ("/something", the same on every rank of one host) carrying the
 *    job's `token` (a non-zero number every rank received over the caller's channel, e.g. drawn by rank 0 and broadcast:
 *    a segment of that name left by a crashed run or owned by a concurrent job is never attached to).  Slow; lets the
 *    multi-rank code run as several processes on ONE GPU without RCCL, bit-identical to PEER.
 * Every wait is bounded: the per-iteration exchanges of a solve by ADMM_HIP_COMM_TIMEOUT_S (20 s), setup reductions and
 * the one join of the replica modes (cross-validation folds, several responses -- ranks are unbalanced there by design) by
 * ADMM_HIP_COMM_PATIENT_TIMEOUT_S (one hour); a missing rank yields ADMM_ERR_COMM from the running call, never a hang.
 * RCCL: the host waits of the solvers poll (stream / event queries + ncclCommGetAsyncError) under the same two bounds; on an
 * asynchronous error or a timed-out wait the communicator is aborted (ncclCommAbort) and the call returns ADMM_ERR_COMM.
 * Ranks should synchronise (barrier) before admm_hip_comm_finalize. */
#define ADMM_HIP_PEER_HANDLE_BYTES 64
ADMM_HIP_API int admm_hip_comm_peer_prepare(int nranks, void* handle_out);
ADMM_HIP_API int admm_hip_comm_init_peer(int nranks, int rank, const void* handles_all_ranks);
ADMM_HIP_API int admm_hip_comm_init_shm(int nranks, int rank, const char* name, unsigned long long token);
/* Test hook: in-place sum all-reduce of a device (mem = ADMM_MEM_DEVICE) or host float / double pair through the
 * attached backend, synchronous.  nf / nd may be 0. */
ADMM_HIP_API int admm_hip_comm_test_allreduce(float* fbuf, long long nf, double* dbuf, long long nd, int mem);
/* Test hook: sum reduce-scatter of host floats through the attached backend -- `send` holds nranks chunks of `count` floats (chunk q
 * is what rank q receives), `recv` (count floats) gets the sum over the ranks of this rank's chunk.  count: a positive multiple of 4.
 * Without a communicator: a copy of chunk 0.  (The exchange of the row-sharded tall solver's split-K Gram) */
ADMM_HIP_API int admm_hip_comm_test_reduce_scatter(const float* send, long long count, float* recv);
ADMM_HIP_API int admm_hip_parlasso_dist(const double* x_local, const double* y_local, int n_local, long long n_total, int p, int mem,
                           const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                           int standardize, int intercept, int nthread, const admm_opts* opts,
                           double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats);
ADMM_HIP_API int admm_hip_lasso_plan_create_dist(const double* x_local, const double* y_local, int n_local, long long n_total, int p, int mem,
                                    const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                    int standardize, int intercept, int nthread, const admm_opts* opts,
                                    admm_hip_plan** plan_out, int* nlambda_out);
/* The SERIAL tall solver (admm_lasso / admm_enet with n_total > p) spread over the ranks -- not in the reference, whose
 * serial solvers are single-threaded; it gives the headline configuration a multi-GPU path.
 * x_local / y_local: any contiguous row slice of the global problem (the slices of all ranks tile the rows; unlike the
 * consensus solver the algorithm does not depend on the split).  Setup: global-moment standardisation, X'y and the
 * Gram matrix as split-K sums over the ranks' row blocks (one all-reduce each), Lanczos value / rho replicated; the
 * Cholesky factorisation and the cached inverse DISTRIBUTED for p >= 4096 (block columns dealt out to the ranks, panels
 * broadcast, every rank forms only the tiles of the inverse its x-update share reads -- bit-identical to the replicated
 * factorisation; ADMM_HIP_DIST_FACTOR=0 switches back to it), replicated below.  Per ADMM iteration every rank streams 1/nranks of the lower-triangle tiles of the inverse and the ranks
 * exchange ONE all-reduce of 2p floats; the element-wise tail and all decisions run replicated on identical numbers.
 * The iterates equal the single-GPU ones up to the summation order of that all-reduce.  alpha < 0: Lasso, else
 * elastic net.  admm_hip_lasso_plan_create_dist with nthread == 0 prepares the same solver for repeated runs. */
ADMM_HIP_API int admm_hip_lasso_dist(const double* x_local, const double* y_local, int n_local, long long n_total, int p, int mem,
                        const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                        int standardize, int intercept, double alpha, const admm_opts* opts,
                        double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats);

/* The serial WIDE solver (admm_lasso / admm_enet with n <= p_total: ADMMLassoWide / ADMMEnetWide, linearised ADMM with
 * active-set iterations) with its COLUMNS spread over the ranks -- the "column-block consensus ... all-reduce of X_i beta_i"
 * of the problem statement.  The compiled reference has no such solver (its only column-block code is the dead
 * src/TODO/PADMMBP.h:137-156); this is the SAME algorithm as ADMMLassoWide.h:86-186 executed in blocks: rank i holds the
 * columns X_i (x_cols: n x p_local column-major, the global columns [col_offset, col_offset + p_local)) and x_i, and the
 * full y.  Everything of length p is local (X_i't, the prox, the active set, DataStd's column moments); everything of
 * length n (z, the dual, t = Ax + z + y/rho, every decision) is replicated; per ADMM iteration the ranks exchange ONE
 * all-reduce of A x = sum_i X_i x_i (n floats).  Setup: lambda_0 is the max over ranks, X X' = sum_i X_i X_i' one
 * all-reduce, the Lanczos value replicated.  The iterates equal the single-GPU ones up to the summation order of A x.
 * Every rank returns the full (p_total + 1) x nl coefficient matrix.  alpha < 0: Lasso, else elastic net. */
ADMM_HIP_API int admm_hip_lasso_dist_cols(const double* x_cols, const double* y, int n, int p_local, long long p_total, long long col_offset, int mem,
                             const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                             int standardize, int intercept, double alpha, const admm_opts* opts,
                             double* lambda_out, float* beta_out, int* niter_out, admm_stats* stats);

/* prepared-problem form of the above (run with admm_hip_lasso_plan_run; beta_out there is (p_total + 1) x nl) */
ADMM_HIP_API int admm_hip_lasso_plan_create_dist_cols(const double* x_cols, const double* y, int n, int p_local, long long p_total, long long col_offset, int mem,
                                         const double* lambda_in, int nlambda_in, int nlambda_auto, double lmin_ratio,
                                         int standardize, int intercept, double alpha, const admm_opts* opts,
                                         admm_hip_plan** plan_out, int* nlambda_out);

/* In-process multi-device mode (admm_hip_parlasso / admm_hip_parbp with PAR_DEVICES):
 * admm_hip_last_parallel_layout: the rank-to-device layout of the CALLING THREAD's last admm_hip_parlasso / admm_hip_parbp call
 *   (thread-local): *nranks = its number of ranks (1: the single-device path, 0: no such call yet), devices[r] = rank r's device
 *   for r < min(*nranks, cap).
 * admm_hip_parallel_assign: the same layout for `nblocks` blocks and a PAR_DEVICES value, computed on the host without touching a
 *   device ("all" means device_count devices).  Returns ADMM_ERR_INVALID_ARG for a malformed list or a device >= device_count.
 *   *nranks = 1 when the mode is off ("0", "" or NULL) or only one rank fits. */
ADMM_HIP_API int admm_hip_last_parallel_layout(int* nranks, int* devices, int cap);
ADMM_HIP_API int admm_hip_parallel_assign(int nblocks, const char* par_devices, int device_count, int* nranks, int* devices, int cap);

ADMM_HIP_API const char* admm_hip_last_error(void);
ADMM_HIP_API const char* admm_hip_version(void);
/* The library keeps large device blocks (>= 32 MB) it has released for re-use by its next call -- at most ADMM_HIP_POOL_MB megabytes,
 * default 24576, 0 = off -- because hipMalloc / hipFree of multi-GB buffers cost up to a quarter of a second per call on some hosts.
 * No solver STATE survives a call (Lasso.cpp:74-76,126-129: neither does the reference's); only empty memory does.  This returns it
 * all to the driver (an R session would call it from a finalizer or `gc()` hook; a failed allocation does it by itself). */
ADMM_HIP_API int admm_hip_trim_memory(void);
ADMM_HIP_API int admm_hip_device_count(void);
ADMM_HIP_API int admm_hip_set_device(int device);
/* hipDeviceSynchronize on the current device (bench.py brackets its timed region with it). */
ADMM_HIP_API int admm_hip_device_synchronize(void);


/* ---- test hooks: exported so that the test-suite can put single kernels / host routines under the oracle through
 * the C ABI.  Not used by any solver entry point above. ---- */

/* The host logic of the loose Lanczos call (ADMMLassoTall.h:196-201 -> SymEigsSolver.h) against a dense symmetric
 * float matrix in HOST memory (n x n, column-major).  Runs without a GPU (CPU test-suite). */
ADMM_HIP_API int admm_hip_host_lanczos(const float* A, int n, float* eig_out, int* nmatop_out);

/* lambda_0 of admm_hip_sgl's automatic grid from a given c = X_s'y_s (xy, HOST, length p), arguments as admm_hip_sgl: the host
 * routine the plan calls (sgl_host.h).  Runs without a GPU (CPU test-suite). */
ADMM_HIP_API int admm_hip_host_sgl_lambda0(const float* xy, int p, const int* group, const double* group_weight, int ngroups,
                                           const double* l1_weight, double alpha, float* out);

/* lambda_0 of admm_hip_boxenet's automatic grid from a given c = X_s'y_s (xy, HOST, length p) and bounds ALREADY in the solver's units
 * (lower_std, upper_std: HOST floats, length p, NULL = none), penalty_factor and alpha as admm_hip_boxenet: the host routine the plan
 * calls (box_host.h), with the elastic net's division for alpha >= 0.  Runs without a GPU (CPU test-suite). */
ADMM_HIP_API int admm_hip_host_box_lambda0(const float* xy, int p, const float* lower_std, const float* upper_std,
                                           const double* penalty_factor, double alpha, float* out);

/* The tall x-update mat-vec exactly as the solver runs it for p >= 2048: symv2_lower_kernel on the lower triangle of
 * the symmetric p x p float matrix A (HOST, column-major, leading dimension p) against the two right-hand sides
 * v0, v1 (HOST, length p), followed by the tail kernel's ordered partial reduction.  y0 = A v0, y1 = A v1 (HOST). */
ADMM_HIP_API int admm_hip_test_symv(const float* A, int p, const float* v0, const float* v1, float* y0, float* y1);
/* The multi-task lasso's multi-vector form of it: Yout[r] = A V[r] for the nr (<= 64) vectors V [nr][p], rhs_per_pass (a built width:
 * 2, 4, 8 or 12) of them per pass over the triangle; vectors 2k and 2k + 1 share the partial sums of one "response".  Yout [nr][p]. */
ADMM_HIP_API int admm_hip_test_symv_multi(const float* A, int p, const float* V, int nr, int rhs_per_pass, float* Yout);
/* The host half of the tall x-update's plan, without a device: the column-segment schedule and the tile list a plan for order p gets on
 * a device with `cus` compute units (<= 0: 256) under the calling thread's SYMV_SCHED, for rank `part` of `nparts` of the row-sharded
 * solver (1: all tiles).  sched_out[3]: width of the long strips' segments, of the short strips', first long strip.  info_out[6]: row
 * strips, p rounded up to 32, leading dimension of the partial arrays, rows of the axpy partial arrays, 1 where the plan streams with
 * non-temporal loads, number of tiles.  tiles_out: one int[4] record per tile in launch order (row strip, first column, width, segment
 * of the strip); tile_capacity records fit (too few: ADMM_ERR_INVALID_ARG, the message says how many are needed). */
ADMM_HIP_API int admm_hip_test_symv_plan(int p, int cus, int part, int nparts, int* sched_out, long long* info_out, int* tiles_out,
                                         int tile_capacity);
/* admm_hip_test_symv with the instantiation and the share of the tiles chosen: variant 0 plain loads, 1 non-temporal loads, 2 the form
 * that also looks for the verdict between the chunks of a tile, given a verdict that can never say "discard" (a tile that leaves all
 * the same: ADMM_ERR_INTERNAL); only the tiles of rank `part` of `nparts` are launched, into zeroed partial arrays, so the results of
 * the parts add up to the product.  sched_out[3]: the schedule the plan used, as above.  p <= 32768. */
ADMM_HIP_API int admm_hip_test_symv_ex(const float* A, int p, const float* v0, const float* v1, int variant, int part, int nparts,
                                       float* y0, float* y1, int* sched_out);
/* The one-vector kernel of the decide-first x-update (ADMM_HIP_SYMV_VERDICT=3) with its gate forced: gate 0 / 1 multiplies v0 / v1 into
 * plane 0 of the partial arrays, 2 makes every tile leave (nothing written, every tile counted); 3 runs the two-vector kernel of
 * admm_hip_test_symv_ex (variant 0, or 1 with nt = 1) on the same storage, for comparison.  All four partial arrays are pre-filled with
 * the 32-bit pattern `fill`.  y [2][p]: y[0] = plane 0 through the one-plane sum of the solver's tails (gate 3: y[0], y[1] = the
 * two-plane sum of both products).  dot_out, axp_out (both or neither): [2][plane_capacity] floats, planes 0 and 1 of the dot / axpy
 * partial arrays as the launch left them (info_out[2] / info_out[3] floats each; a plane_capacity below the larger:
 * ADMM_ERR_INVALID_ARG).  info_out[4]: tiles, tiles that left early, floats of a dot plane, of an axpy plane.  p <= 32768. */
ADMM_HIP_API int admm_hip_test_symv_one(const float* A, int p, const float* v0, const float* v1, int gate, int nt, unsigned int fill,
                                        float* y, float* dot_out, float* axp_out, long long plane_capacity, long long* info_out,
                                        int* sched_out);
/* The exact 29-bit record format of the packed x-update stream, on the host alone.  bits [nchunks][64][32]: per lane of a wave the 32
 * entries (4 k + c: column k of an 8-column chunk, component c of the lane's float4) of a record, as 32-bit patterns.  They are encoded
 * against *base_io (negative: the largest upper-seven-bit exponent among the finite non-zero entries, which is handed back) into
 * stream_out [nchunks][1856] dwords, the memory image of the wave's chunks.  Entries that do not fit go to esc_out as pairs
 * (chunk << 11 | lane << 5 | entry, bits) while they fit esc_cap and are all counted in *nesc_out.  decoded_out [nchunks][64][32]: the
 * image decoded again, escapes as +0.0. */
ADMM_HIP_API int admm_hip_test_symv_pack_host(const unsigned int* bits, int nchunks, int* base_io, unsigned int* stream_out,
                                              unsigned int* esc_out, int esc_cap, long long* nesc_out, unsigned int* decoded_out);
/* admm_hip_test_symv_one (gates 0, 1, 2) on the 29-bit copy of the plan's tiles: the tiles are packed with escape lists of esc_cap entries
 * per tile and the one-vector kernel streams the copy.  info_out[8]: tiles, tiles that left early, floats of a dot plane, of an axpy
 * plane, escapes met, tiles whose escape list overflowed, bytes of the packed stream, 1 if the packed kernel ran (after an overflow it
 * does not: the planes keep `fill` and this is 0). */
ADMM_HIP_API int admm_hip_test_symv_packed(const float* A, int p, const float* v0, const float* v1, int gate, int nt, unsigned int fill,
                                           int esc_cap, float* y, float* dot_out, float* axp_out, long long plane_capacity,
                                           long long* info_out, int* sched_out);
/* The bare one-vector tile loops on the fp32 matrix and on its 29-bit copy, event-timed launch by launch.  us_out [4][reps] microseconds:
 * fp32 and packed, each launch behind a pass over a buffer larger than the Infinity Cache; fp32 and packed replayed back to back (two
 * alternating blocks of reps / 2 launches, two untimed launches in front of each).  info_out[4]: tiles, escapes met, tiles overflowed,
 * bytes of the packed stream. */
ADMM_HIP_API int admm_hip_test_symv_packed_time(const float* A, int p, const float* v0, int reps, float* us_out, long long* info_out);
/* admm_hip_test_symv_multi with the non-temporal instantiations forced (nt = 1) or not (0), and the consumer chosen: finish 0 sums the
 * partials pair by pair (as admm_hip_test_symv_multi), 1 in chunks of pairs with the routine and the walk of the multi-task tail. */
ADMM_HIP_API int admm_hip_test_symv_multi_ex(const float* A, int p, const float* V, int nr, int rhs_per_pass, int nt, int finish,
                                             float* Yout, int* sched_out);
/* The double-accumulating form of the refined x-update (ADMM_HIP_REFINE): the same products of the float matrix and float vectors
 * with every product and sum in double, on double partial arrays, summed as the refinement's residual kernel sums them.  y0, y1 double. */
ADMM_HIP_API int admm_hip_test_symv_f64acc(const float* A, int p, const float* v0, const float* v1, double* y0, double* y1, int* sched_out);
/* Tiles of the tall x-update that left early because the launch they belonged to was known to be discarded (the first launch after a
 * converged lambda, the launch of the last decision; ADMM_HIP_SYMV_VERDICT=0: none), counted over the most recent tall lasso /
 * elastic-net / group-lasso path run by the CALLING THREAD.  At the default level 3 every tile takes the decision itself before it
 * streams, so the count is exact: tiles x discarded launches.  At levels 1 and 2 how many leave is a matter of timing; the results
 * depend on it at no level. */
ADMM_HIP_API int admm_hip_test_tall_early_exits(long long* count);
/* The stream of the x-update of the most recent tall plan (lasso, elastic net, group, sparse-group, box) created by the CALLING THREAD.
 * info_out[4]: 1 if it streams the exact 29-bit copy of the inverse's tiles (ADMM_HIP_SYMV_PACK, the default) and 0 if the fp32 matrix;
 * entries met outside their tile's exponent window while packing; tiles whose list of such entries overflowed (any: the fp32 stream);
 * bytes of the copy.  All 0 where no copy was attempted. */
ADMM_HIP_API int admm_hip_test_tall_pack_info(long long* info_out);
/* The decision of the decide-first x-update as ONE tile takes it in its prologue, on caller-supplied HOST inputs: the control block
 * (ctl_d[9]: rho, lam, eps_primal, eps_dual, adj_a, adj_c, tau, a_next, tau_next; ctl_i[9]: mode, restart, iter, lam_idx, done, first,
 * total, fin_idx, fin_niter) and the compact copy [3][nwg] of the norm partials r^2, dz^2, daz^2 of nwg tail workgroups.
 * sums_out[3]: the three sums the tile formed; *answer_out: -1 leave (the launch's products are not used), 0 multiply u, 1 multiply w. */
ADMM_HIP_API int admm_hip_test_tall_gate(const double* ctl_d, const int* ctl_i, const double* compact, int nwg, int maxit, int nlam,
                                         double* sums_out, int* answer_out);
/* The six norm sums as the x-update's deciding workgroup forms them from the rows [nwg][8] of the norm partials (HOST); sums_out[6]. */
ADMM_HIP_API int admm_hip_test_tall_norms(const double* rows, int nwg, double* sums_out);
/* The device prox of admm_hip_logit alone: out[k] = the root z of z - v[k] - t / (1 + e^z), t = 1 / rho > 0, over HOST arrays of
 * length m, by the device function the tail and rows kernels call. */
ADMM_HIP_API int admm_hip_test_logit_prox(const double* v, long long m, double t, double* out);
/* The device prox of admm_hip_poisson's data rows alone: out[k] = the root z of z + t e^z - (v[k] + t y[k]), t = 1 / rho > 0, over HOST
 * arrays of length m (v finite, y finite and >= 0), by the device function the tail and rows kernels call. */
ADMM_HIP_API int admm_hip_test_poisson_prox(const double* v, const double* y, long long m, double t, double* out);

/* The one-time matrix-core kernels as the solvers call them (Linalg::cross_prod_lower / tcross_prod_lower,
 * BlasWrapper.h:73-154; LLT, ADMMLassoTall.h:204-205), on HOST matrices (column-major, tight leading dimensions):
 * G = A'A (atA != 0, order cols) or AA' (order rows), both triangles, float (is_double == 0) or double;
 * Ainv = inverse of the SPD matrix A of order n: precision 0 = float, 1 = double, 2 = float matrix inverted in double
 * and rounded once (ADMM_HIP_INVERSE=f64). */
ADMM_HIP_API int admm_hip_test_gram(const void* A, int rows, int cols, int atA, int is_double, void* G);
/* y = A' v with the streaming mat-vec every other product of the solvers uses (X'y, the wide regular step, the consensus /
 * LAD / BP products, the tall x-update below p = 2048): A HOST rows x cols column-major (leading dimension rows). */
ADMM_HIP_API int admm_hip_test_gemv_t(const void* A, int rows, int cols, int is_double, const void* v, void* y);
/* Every launch form of that mat-vec (gemv_kernels.h) on `count` products y_i = A_i' v_i: A[i] HOST m[i] x k[i] column-major (leading
 * dimension m[i]), float or double (is_double), v[i] HOST [nrhs][m[i]].  On the device a matrix is stored as the callers hold it: leading
 * dimension round_up(m, 32) + lda_extra (a multiple of 32), rows [m, round_up(m, 32)) zero, every row beyond and the tail of v NaN.
 * form 0: launch_gemv_t, partial rows only (count 1; nrhs 1 or 2, the two-vector instantiation of the tall fallback's body).
 * form 1: GemvT::run (count 1): the one-segment shortcut straight into y, or partial rows and the reduce launch.
 * form 2: a chain (count 2, m[1] == k[0]): GemvT::run_partials on product 0, GemvT::run_from on product 1, whose right-hand side is the
 *         un-reduced partial rows of product 0 -- staged in the kernel, or behind a reduce launch beyond 12 rows, as the struct decides.
 * form 3: gemv_t_batch_kernel, one launch of `count` (<= 8) argument blocks as wide as the widest; from (NULL: none) names for product i
 *         the product (from[i] >= 0, itself not chained, k[from[i]] == m[i]) whose partial rows are its right-hand side: those products
 *         go into a second batched launch behind the first.  v[i] is not read for a chained product.
 * nt: 0 plain loads, 1 non-temporal loads, -1 the plan's own choice.  max_seg_rows: 0 the default plan, otherwise the cap on the rows of
 * a segment handed to plan_gemv_t (2048 is what GemvT::init takes for fp64 operands beyond the cache).  skip (NULL: zeros): the value
 * of product i's device skip flag.  Every partial and output buffer is pre-filled with the pattern `fill` (float: its low 32 bits).
 * part_out[i]: [nrhs][part_capacity] elements, the partial rows [nseg][round_up(k, 32)] as the launch left them and `fill` behind (a
 * part_capacity below nseg rows: ADMM_ERR_INVALID_ARG).  y_out (forms 1 and 2, the last product): round_up(k, 32) elements.
 * info_out [count][8]: nseg, seg_len, groups_per_wg, grid, 1 if non-temporal loads ran, the route of the right-hand side (0 a plain
 * vector, 1 partial rows summed in the kernel, 2 summed by a reduce launch into a single row), the partial rows it arrived in, and the
 * width of the launch (form 3: of the batched launch).  Inconsistent requests: ADMM_ERR_INVALID_ARG before any launch. */
ADMM_HIP_API int admm_hip_test_gemv_t_ex(int is_double, int form, int nrhs, int nt, int max_seg_rows, int lda_extra, unsigned long long fill,
                                         int count, const int* m, const int* k, const void* const* A, const void* const* v, const int* from,
                                         const int* skip, void* const* part_out, long long part_capacity, void* const* y_out,
                                         long long* info_out);
/* w = X (X' v), the Gram-free operator under the wide solver's spectral-radius estimate (GramFreeWideOp: the streaming mat-vec above,
 * then gemv_n_partial_kernel and its ordered sum): X HOST n x p float column-major (leading dimension n), v and w HOST length n. */
ADMM_HIP_API int admm_hip_test_wide_op(const float* X, int n, int p, const float* v, float* w);
/* The spectral radii admm_hip_parbp takes for its column blocks: out[b] = its estimate of lambda_max(A_b'A_b) for the nblocks blocks of
 * the solver's own partition of the p columns (nblocks - 1 blocks of p div nblocks columns, the last takes the rest) of the HOST double
 * matrix A (n x p column-major, leading dimension n), all blocks in ONE batch of Lanczos runs in lockstep; nsteps_out[b]: the steps
 * block b was judged on.  ADMM_ERR_EIGS as the solver raises it. */
ADMM_HIP_API int admm_hip_test_block_sprad(const double* A, int n, int p, int nblocks, double* out, int* nsteps_out);
/* The setup of the wide solver's safe screen (wide_screen_prep_kernel for fmt 16, wide_screen_prep8_kernel for fmt 8, and
 * wide_screen_rate8_kernel, which picks the format) on the HOST float matrix X (n x p column-major, leading dimension n), stored on the
 * device as the plan stores it: leading dimension ldx = round_up(n, 16), rows [n, ldx) of every column set to the 32-bit pattern
 * pad_fill.  nw stands for the plan's number of waves NW.  copy_out: the raw copy, p * ldh elements of 2 bytes (fmt 16, ldh =
 * round_up(n, 8)) or 1 byte (fmt 8, ldh = round_up(n, 16)), pre-filled with 0xff bytes; copy_capacity: its size in elements.  s_out,
 * scale_out (fmt 8 only; may be NULL for fmt 16): the raw [nw * S] arrays, S = round_up(ceil(p / nw), 64), cleared before the launch as
 * the plan clears them; column j is at [(j % nw) * S + j / nw].  rate_out: the ceil(p / 4) partial sums of wide_screen_rate8_kernel.
 * info_out [4]: ldh, S, nw, ldx. */
ADMM_HIP_API int admm_hip_test_wide_screen_prep(const float* X, int n, int p, int fmt, int nw, unsigned pad_fill, void* copy_out,
                                                long long copy_capacity, float* s_out, float* scale_out, double* rate_out, long long* info_out);
/* The same for the sharing basis pursuit's screen (sbp_screen_prep_kernel): HOST double A (n x pl column-major, leading dimension n) stored
 * with leading dimension round_up(n, 32) + lda_extra, every row beyond n set to pad_fill in both halves of the double.  copy_out: pl * ldh
 * fp16 values, ldh = round_up(n, 8), pre-filled with 0xff bytes; s_out [pl]; info_out [2]: ldh, lda. */
ADMM_HIP_API int admm_hip_test_sbp_screen_prep(const double* A, int n, int pl, int lda_extra, unsigned pad_fill, unsigned short* copy_out,
                                               long long copy_capacity, float* s_out, long long* info_out);
/* y = A v over the NON-ZERO entries of v with the gather mat-vec of the one-pass consensus workers and of basis pursuit (the product
 * that replaces the reference's first streaming pass, PADMMLasso.h:25 / ADMMBP.h:65): A HOST rows x cols column-major (leading
 * dimension rows), v length cols in A's type, y length rows in double (the kernel's accumulation type). */
ADMM_HIP_API int admm_hip_test_gather(const void* A, int rows, int cols, int is_double, const void* v, double* y);
ADMM_HIP_API int admm_hip_test_spd_inverse(const void* A, int n, int precision, void* Ainv);
/* (A + diag I)^-1 of the float matrix A (order n) through the double route of precision 2 above with the caller's shift: the
 * tall path's rho, added to the float diagonal as a FLOAT addition before the matrix is widened (ADMMLassoTall.h:204). */
ADMM_HIP_API int admm_hip_test_spd_inverse_shift(const float* A, int n, double diag, float* Ainv);
/* The blocked factorisation under those inverses alone: L (order n, tight) = A overwritten by its Cholesky factor in the lower
 * triangle (the strict upper triangle stays the caller's), U = L^-T (upper triangular).  Float or double (is_double);
 * ADMM_ERR_NOT_SPD names the first failing pivot (1-based). */
ADMM_HIP_API int admm_hip_test_cholesky_linvt(int is_double, const void* A, int n, void* L, void* U);
/* One launch of the matrix-core NT-GEMM every step of that chain runs: C = alpha A B' + beta C on 128 x 128 tiles.  HOST operands,
 * column-major with the output index contiguous and tight leading dimensions: A is M x K, B is N x K, C is M x N (read and
 * written); the hook stores them on the device as the callers do (leading dimension rounded up to 128, K zero padded to the K tile:
 * 16 float, 8 double).  lower: only the tiles on or below the diagonal of a square C (M == N); mirror (with lower): the transposed
 * tile is stored too; kstart_row: the K loop of a tile starts at its first row (upper-triangular operands: U U'); b_lower (double,
 * not lower): the K loop ends after the tile's last column (lower-triangular B); in_place (N <= 128, K == 128, not lower): the
 * device copy of A is the output as well, as in the factorisation's panel updates -- the host C is then only written.
 * Inconsistent requests: ADMM_ERR_INVALID_ARG before any launch.  A launch that changes the device C outside M x N (a NaN guard
 * band up to the padded storage; the remaining columns of A when in place): ADMM_ERR_INTERNAL, with C still copied back. */
ADMM_HIP_API int admm_hip_test_gemm_nt(int is_double, int lower, int mirror, int kstart_row, int b_lower, int in_place, int M, int N, int K,
                                       double alpha, double beta, const void* A, const void* B, void* C);
/* The system admm_hip_lasso_cv hands the tall solver for fold `fold` when it forms the folds as down-dates of the full-data
 * Gram (cv.hip): x, y HOST column-major doubles, fold_id as in admm_hip_lasso_cv (NULL: i mod nfolds).  Out (HOST): gram p x p
 * float (X_T'X_T of the training rows standardised by THEIR statistics), xy p floats, mean_x / scale_x p floats, and
 * mean_scale_y[2]. */
ADMM_HIP_API int admm_hip_test_cv_fold_system(const double* x, const double* y, int n, int p, const int* fold_id, int nfolds, int fold,
                                              int standardize, int intercept, float* gram, float* xy, float* mean_x, float* scale_x,
                                              float* mean_scale_y);

#ifdef __cplusplus
}
#endif
#endif /* ADMM_HIP_H */
