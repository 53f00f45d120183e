"""Host-side mirror of the reference's R interface for the GPU path.

R is not available in this image, so the builder chain of the package is mirrored in Python with
the same names, argument meaning, defaults and error behaviour:

    admm_lasso(x, y)$penalty(...)$parallel(...)$opts(...)$fit()     R/30_admm_lasso.R
    admm_enet(x, y)$penalty(..., alpha)$opts(...)$fit()             R/40_admm_enet.R
    admm_lad(x, y, intercept)$opts(...)$fit()                       R/20_admm_lad.R
    admm_bp(x, y)$opts(...)$fit()                                   R/10_admm_bp.R
    admm_grplasso(x, y, group)$penalty(..., group_weights)$opts(...)$fit()      (not in the reference: admm_hip_grplasso)
    admm_sgl(x, y, group, alpha)$penalty(..., group_weights, l1_weights)$opts(...)$fit()      (not in the reference: admm_hip_sgl)
    admm_mtlasso(x, Y)$penalty(..., row_weights)$opts(...)$fit()                (not in the reference: admm_hip_mtlasso)
    admm_boxenet(x, y, lower, upper)$penalty(..., alpha, penalty_factor)$opts(...)$fit()      (not in the reference: admm_hip_boxenet)

`fit()` forwards to the C ABI of libadmm_hip.so exactly where the R `$fit()` does its
`.Call("admm_*", ...)` (R/30_admm_lasso.R:136-160 etc.).  All numerics run in the HIP library;
nothing here computes.  x may be a host array or a `DevicePtr` (column-major float64 in HBM).
"""
import ctypes

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import AdmmOpts, AdmmStats, DevicePtr, as_input, check


def _stop(msg):
    raise ValueError(msg)


def _shape(x, n, p):
    if isinstance(x, DevicePtr):
        if n is None or p is None:
            _stop("n and p are required with a DevicePtr")
        return int(n), int(p)
    a = np.asarray(x)
    if a.ndim != 2:
        _stop("x must be a matrix")
    return a.shape


def _devices_option(devices):
    """PAR_DEVICES value of $parallel(devices=...): None, "all", "0,1" or a sequence of device numbers."""
    if devices is None:
        return None
    if isinstance(devices, str):
        return devices
    return ",".join(str(int(d)) for d in devices)


def _par_devices(model):
    """The calling thread's PAR_DEVICES for the duration of one parallel fit (restored afterwards, also on error)."""
    dev = getattr(model, "devices", None)
    return _lib.options(PAR_DEVICES=dev) if dev is not None else _lib.options()


def _beta_to_csc(beta_dense):
    """(p+1) x nlambda dense -> CSC holding row 0 always plus the non-zeros (Lasso.cpp:22-30)."""
    p1, nl = beta_dense.shape
    indptr = [0]
    indices, data = [], []
    for j in range(nl):
        col = beta_dense[:, j]
        nz = np.nonzero(col[1:])[0] + 1
        idx = np.concatenate([[0], nz])
        indices.append(idx)
        data.append(col[idx].astype(np.float64))
        indptr.append(indptr[-1] + idx.size)
    return sp.csc_matrix((np.concatenate(data), np.concatenate(indices), np.array(indptr)), shape=(p1, nl))


class ADMM_Lasso_fit:
    """Fields lambda, beta (dgCMatrix-like CSC, (p+1) x nlambda), niter (R/30_admm_lasso.R:18-22)."""

    def __init__(self, lam, beta_dense, niter, stats):
        self.lambda_ = lam
        self.beta_dense = beta_dense
        self._beta = None
        self.niter = niter
        self.stats = stats

    @property
    def beta(self):
        """dgCMatrix-like CSC, built on first use."""
        if self._beta is None:
            self._beta = _beta_to_csc(self.beta_dense)
        return self._beta

    def __repr__(self):
        return (f"{getattr(self, '_title', 'ADMM Lasso fitting result')}\n\n$lambda\n{self.lambda_}\n\n$beta\n<{self.beta.shape[0]} x "
                f"{self.beta.shape[1]}> sparse matrix\n\n$niter\n{self.niter}")

    def show(self):
        """ADMM_Lasso_fit$show (R/30_admm_lasso.R:181-186)."""
        print(repr(self))

    def path_data(self):
        """What ADMM_Lasso_fit$plot draws (R/30_admm_lasso.R:189-214): log(lambda) and, per variable that is non-zero for
        at least one lambda (intercept excluded), its coefficient along the path.  Returns (loglambda [nl], coef [nl, nvar])."""
        if self.lambda_.size < 2:
            _stop("need to have at least two lambda values")
        inc = np.any(self.beta_dense != 0, axis=1)
        inc[0] = False
        return np.log(self.lambda_), self.beta_dense[inc].T.astype(np.float64)

    def plot(self, ax=None):
        """Solution-path plot (the reference uses ggplot2; here matplotlib, same axes and title)."""
        loglambda, coef = self.path_data()
        import matplotlib
        if ax is None:
            matplotlib.use("Agg", force=False)
            import matplotlib.pyplot as plt
            _, ax = plt.subplots()
        ax.plot(loglambda, coef)
        ax.set_xlabel("log(lambda)")
        ax.set_ylabel("Coefficients")
        ax.set_title("Solution path")
        return ax


class ADMM_Lasso:
    _name = "ADMM Lasso model"

    def __init__(self, x, y, intercept=True, standardize=True, n=None, p=None):
        n_, p_ = _shape(x, n, p)
        ylen = n_ if isinstance(y, DevicePtr) else len(y)
        if n_ != ylen:
            _stop("nrow(x) should be equal to length(y)")                       # R/30_admm_lasso.R:34-35
        self.x, self.y, self.n, self.p = x, y, int(n_), int(p_)
        self.intercept = bool(intercept)
        self.standardize = bool(standardize)
        self.lambda_ = np.zeros(0)
        self.nlambda = 100
        self.lambda_min_ratio = 0.01 if n_ < p_ else 0.0001
        self.nthread = 1
        self.maxit = 10000
        self.eps_abs = 1e-5
        self.eps_rel = 1e-5
        self.rho = -1.0

    def penalty(self, lambda_=None, nlambda=100, lambda_min_ratio=None, **kw):
        if "lambda" in kw:
            lambda_ = kw["lambda"]
        lam = np.sort(np.atleast_1d(np.asarray(lambda_, dtype=np.float64)))[::-1] if lambda_ is not None else np.zeros(0)
        if np.any(lam <= 0):
            _stop("lambda must be positive")
        if nlambda <= 0:
            _stop("nlambda must be a positive integer")
        lmr = (0.01 if self.n < self.p else 0.0001) if lambda_min_ratio is None else float(lambda_min_ratio)
        if lmr >= 1 or lmr <= 0:
            _stop("lambda_min_ratio must be within (0, 1)")
        self.lambda_ = lam
        self.nlambda = int(nlambda)
        self.lambda_min_ratio = lmr
        return self

    def parallel(self, nthread=2, devices=None):
        """devices (not in R): spread the nthread blocks over devices in this process -- "all", a list such as [0, 1] or "0,1"
        (repeats put several ranks on one device: a test / diagnostic form), None = the single-device default.  Sets the option
        PAR_DEVICES around the fit only (include/admm_hip.h, admm_hip_parlasso)."""
        nt = int(nthread)
        if nt < 1:
            nt = 1
        if nt >= self.p / 5:
            _stop("nthread cannot exceed ncol(x)/5")                             # R/30_admm_lasso.R:105-106
        self.nthread = nt
        self.devices = _devices_option(devices)
        return self

    def opts(self, maxit=10000, eps_abs=1e-5, eps_rel=1e-5, rho=None):
        if maxit <= 0:
            _stop("maxit should be positive")
        if eps_abs < 0 or eps_rel < 0:
            _stop("eps_abs and eps_rel should be nonnegative")
        if rho is not None and rho <= 0:
            _stop("rho should be positive")
        self.maxit = int(maxit)
        self.eps_abs = float(eps_abs)
        self.eps_rel = float(eps_rel)
        self.rho = -1.0 if rho is None else float(rho)
        return self

    # -- .Call marshalling
    def _common(self):
        lib = _lib.load()
        xp, xmem, xk = as_input(self.x)
        yp, ymem, yk = as_input(self.y)
        if xmem != ymem:
            _stop("x and y must live in the same memory space")
        nl = self.lambda_.size if self.lambda_.size else self.nlambda
        lam_in = np.ascontiguousarray(self.lambda_, dtype=np.float64)
        o = AdmmOpts(self.maxit, self.eps_abs, self.eps_rel, self.rho)
        lam_out = np.zeros(nl, dtype=np.float64)
        beta = self._beta_buffer(nl)
        niter = np.zeros(nl, dtype=np.int32)
        stats = AdmmStats()
        head = (xp, yp, self.n, self.p, xmem,
                ctypes.c_void_p(lam_in.ctypes.data if lam_in.size else 0), int(lam_in.size), self.nlambda,
                self.lambda_min_ratio, int(self.standardize), int(self.intercept))
        tail = (ctypes.byref(o), lam_out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                beta.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                niter.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(stats))
        keep = (xk, yk, lam_in)
        return lib, head, tail, lam_out, beta, niter, stats, keep

    def fit_responses(self, Y, m=None):
        """Fit this model for several responses of the same x at once (admm_hip_lasso_multi; not in the reference package):
        Y is n x m (a host matrix, or a DevicePtr to column-major doubles together with m); returns one ADMM_Lasso_fit per
        column, each bit-identical to a separate fit() with that column as y."""
        lib, head, tail, lam_out, beta, niter, stats, keep = self._common()
        if isinstance(Y, DevicePtr):
            if m is None:
                _stop("m (the number of responses) is needed with a device pointer")
            yp, ymem, yk = as_input(Y)
            m = int(m)
        else:
            Ya = np.asfortranarray(Y, dtype=np.float64)
            if Ya.ndim != 2 or Ya.shape[0] != self.n:
                _stop("Y should be a matrix with nrow(x) rows")
            m = Ya.shape[1]
            yp, ymem, yk = as_input(Ya)
        if ymem != head[4]:
            _stop("x and Y must live in the same memory space")
        nl = lam_out.size
        lam_all = np.zeros((m, nl))
        beta_all = np.zeros((m, nl, self.p + 1), dtype=np.float32)
        nit_all = np.zeros((m, nl), dtype=np.int32)
        st_all = (AdmmStats * m)()
        alpha = float(getattr(self, "alpha", -1.0))
        check(lib.admm_hip_lasso_multi(head[0], yp, head[2], head[3], m, head[4], *head[5:], alpha, tail[0],
                                       lam_all.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                       beta_all.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                       nit_all.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), st_all))
        return [ADMM_Lasso_fit(lam_all[j].copy(), np.asfortranarray(beta_all[j].T), nit_all[j].copy(), st_all[j].as_dict()) for j in range(m)]

    def cv(self, nfolds=10, fold_id=None, keep_fold_beta=False):
        """K-fold cross-validation of this model's lambda path (admm_hip_lasso_cv; not in the reference package).
        fold_id: integer array of length n with values in [0, nfolds) (default: i mod nfolds)."""
        lib, head, tail, lam_out, beta, niter, stats, keep = self._common()
        nl = lam_out.size
        fid = None if fold_id is None else np.ascontiguousarray(fold_id, dtype=np.int32)
        if fid is not None and fid.size != self.n:
            _stop("fold_id should have length nrow(x)")
        cvm, cvse = np.zeros(nl), np.zeros(nl)
        fmse = np.zeros((nfolds, nl))
        fnit = np.zeros((nfolds, nl), dtype=np.int32)
        fbeta = np.zeros((nfolds, nl, self.p + 1), dtype=np.float32) if keep_fold_beta else None
        imin, i1se = ctypes.c_int(0), ctypes.c_int(0)
        dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        alpha = float(getattr(self, "alpha", -1.0))
        check(lib.admm_hip_lasso_cv(*head[:5], ip(fid) if fid is not None else None, int(nfolds), *head[5:], alpha, tail[0],
                                    tail[1], tail[2], tail[3], dp(cvm), dp(cvse), dp(fmse), ip(fnit),
                                    fbeta.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if keep_fold_beta else None,
                                    ctypes.byref(imin), ctypes.byref(i1se), tail[4]))
        fit = ADMM_Lasso_fit(lam_out, beta, niter, stats.as_dict())
        if fbeta is not None:
            fbeta = np.transpose(fbeta, (0, 2, 1))                               # [fold][p + 1][lambda]
        return ADMM_Lasso_cv(fit, cvm, cvse, fmse, fnit, fbeta, imin.value, i1se.value)

    # -- what LassoPlan asks of a model: the entry point that creates its plan with the arguments between the path's and opts, the
    # coefficient buffer of a path of nl lambdas and the result object
    _plan_entry = "admm_hip_lasso_plan_create"

    def _plan_args(self, head):
        return head + (-1.0, int(self.nthread))

    def _beta_buffer(self, nl):
        return np.zeros((self.p + 1, nl), dtype=np.float32, order="F")

    def _result(self, lam, beta, niter, stats):
        return ADMM_Lasso_fit(lam, beta, niter, stats)

    def fit(self):
        lib, head, tail, lam_out, beta, niter, stats, keep = self._common()
        if self.nthread <= 1:
            check(lib.admm_hip_lasso(*head, *tail))                              # .Call("admm_lasso", ...)
        else:
            with _par_devices(self):
                check(lib.admm_hip_parlasso(*head, self.nthread, *tail))         # .Call("admm_parlasso", ...)
        return ADMM_Lasso_fit(lam_out, beta, niter, stats.as_dict())


class ADMM_Lasso_cv:
    """Result of ADMM_Lasso.cv / ADMM_Enet.cv: the full-data fit plus the K-fold table (admm_hip_lasso_cv)."""

    def __init__(self, fit, cvm, cvse, fold_mse, fold_niter, fold_beta, idx_min, idx_1se):
        self.fit = fit
        self.lambda_ = fit.lambda_
        self.cvm, self.cvse = cvm, cvse
        self.fold_mse, self.fold_niter, self.fold_beta = fold_mse, fold_niter, fold_beta
        self.idx_min, self.idx_1se = int(idx_min), int(idx_1se)
        self.lambda_min, self.lambda_1se = float(fit.lambda_[idx_min]), float(fit.lambda_[idx_1se])

    def __repr__(self):
        return (f"ADMM cross-validation: {self.fold_mse.shape[0]} folds x {self.lambda_.size} lambdas\n"
                f"lambda.min = {self.lambda_min:.6g} (cvm {self.cvm[self.idx_min]:.6g}), lambda.1se = {self.lambda_1se:.6g}")


class ADMM_Enet(ADMM_Lasso):
    _name = "ADMM Elastic Net model"

    def parallel(self, nthread=2):
        """The reference's $parallel() on an elastic-net model only sets a field that ADMM_Enet$fit never reads
        (R/40_admm_enet.R:50-64 always calls admm_enet): kept as a no-op with the same validation."""
        super().parallel(nthread)
        self.nthread = 1
        return self

    def __init__(self, x, y, intercept=True, standardize=True, n=None, p=None):
        super().__init__(x, y, intercept, standardize, n, p)
        self.alpha = 1.0

    def penalty(self, lambda_=None, nlambda=100, lambda_min_ratio=None, alpha=1, **kw):
        super().penalty(lambda_, nlambda, lambda_min_ratio, **kw)
        if alpha < 0 or alpha > 1:
            _stop("alpha must be within [0, 1]")                                 # R/40_admm_enet.R:38-39
        self.alpha = float(alpha)
        return self

    def _plan_args(self, head):
        return head + (float(self.alpha), int(self.nthread))

    def fit(self):
        lib, head, tail, lam_out, beta, niter, stats, keep = self._common()
        check(lib.admm_hip_enet(*head, self.alpha, *tail))                       # .Call("admm_enet", ...)
        return ADMM_Lasso_fit(lam_out, beta, niter, stats.as_dict())


class _Records(np.ndarray):
    """A record buffer that carries its own capacity (`cap`, 0 = disabled): a one-record request is not mistaken for 'off'
    (the capacity used to be inferred from shape[0] > 1)."""
    cap = 0


def _records(shape, cap):
    a = np.zeros(shape, dtype=np.float64).view(_Records)
    a.cap = int(cap)
    return a


def _trace_buffers(maxit):
    cap = maxit + 8 if maxit > 0 else 0
    return _records((max(cap, 1), _lib.TRACE_FIELDS), cap), ctypes.c_longlong(0)


def _trace_args(tr, ntr):
    if tr.cap == 0:
        return None, 0, None
    return tr.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), tr.cap, ctypes.byref(ntr)


def _state_buffers(nrec, dim):
    nrec = int(nrec) if nrec else 0
    return _records((max(nrec, 1), 5, dim), nrec), ctypes.c_longlong(0)


def _state_args(sbuf, nst):
    if sbuf.cap == 0:
        return None, 0, None
    return sbuf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), sbuf.cap, ctypes.byref(nst)


# ---- the dense builders: basis pursuit, LAD and the losses on LAD's loop.  What they share is written once, here: the call into the
# library (_dense_call), the argument rules of the builders and the base of the result classes.

def _dense_call(model, entry, lead, grid, nfit, dim, trace=False, state=0, k=None, width=None, records_only=False, tables=()):
    """The one path from a dense builder's fit() into the library.  `entry` is admm_hip_<loss>; `lead` its arguments between mem and
    the grid (the intercept flag; nthread for admm_hip_parbp); `grid` the loss's parameter arrays, one fit per entry (k fits where the
    symbol takes `k`); `nfit` the number of fits; `dim` the length of one iterate (None: the symbol has a _traced form only).
    Without trace this calls `entry`(x, y, n, p[, k], mem, lead..., grid arrays..., their length, opts, beta, niter, stats); with
    trace -- and always with records_only: ADMM_BP and ADMM_LAD use no other form -- `entry`_state, which takes the FIRST value of every
    grid array, never k or a length, and then the trace block and the state block (`state` records; ignored without trace).
    `tables`: further output arrays of the grid form, between niter and stats (the cross-validation tables of <loss>_cv).
    -> (beta: flat float64, nfit times `width` (default p + 1); niter: int32 nfit; stats: dict; trace records or None; state records or None)."""
    lib = _lib.load()
    xp, xmem, xk = as_input(model.x)
    yp, ymem, yk = as_input(model.y)
    if xmem != ymem:
        _stop("x and y must live in the same memory space")
    o = AdmmOpts(model.maxit, model.eps_abs, model.eps_rel, model.rho)
    beta = np.zeros((model.p + 1 if width is None else width) * nfit, dtype=np.float64)
    niter = np.zeros(nfit, dtype=np.int32)
    stats = AdmmStats()
    dp = ctypes.POINTER(ctypes.c_double)
    out = (ctypes.byref(o), beta.ctypes.data_as(dp), niter.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(stats))
    sbuf = None
    if trace or records_only:
        tr, ntr = _trace_buffers(model.maxit if trace else 0)
        records = _trace_args(tr, ntr)
        if dim is not None:
            sbuf, nst = _state_buffers(state if trace else 0, dim)
            records += _state_args(sbuf, nst)
        check(getattr(lib, entry + ("_traced" if dim is None else "_state"))(xp, yp, model.n, model.p, xmem, *lead, *(float(g[0]) for g in grid), *out, *records))
    else:
        ip = ctypes.POINTER(ctypes.c_int)
        check(getattr(lib, entry)(xp, yp, model.n, model.p, *(() if k is None else (k,)), xmem, *lead, *(g.ctypes.data_as(dp) for g in grid),
                                  *((int(grid[0].size),) if grid else ()), *out[:3], *(t.ctypes.data_as(ip if t.dtype == np.int32 else dp) for t in tables), out[3]))
    # every buffer whose address went into the call -- x and y as converted (xk, yk), the grid arrays, beta, niter and the record buffers -- is
    # a local of this frame and so alive until the call has returned: fit() passes its arrays in, never bare pointers
    return (beta, niter, stats.as_dict(), tr[:ntr.value].copy() if trace else None,
            sbuf[:nst.value].copy() if (trace and state and sbuf is not None) else None)


def _with_records(fit, trace, state):
    fit.trace, fit.state = trace, state
    return fit


def _fitted_intercept_shape(x, n, p, intercept):
    """The losses that fit the intercept as a column of ones: nrow(x) must exceed ncol(x) + intercept."""
    n_, p_ = _shape(x, n, p)
    if n_ <= p_ + (1 if intercept else 0):
        _stop("nrow(x) must be greater than ncol(x) + 1 (the intercept is fitted)" if intercept else "nrow(x) must be greater than ncol(x)")


def _label_matrix(Y, k, nrow=None):
    """-> (Y, k): Y as an n x k column-major matrix (a vector is one column), or the DevicePtr it was, which needs k.  nrow: the row
    count to insist on here (the builders that go through ADMM_LAD.__init__ leave that to its length(y) check)."""
    if isinstance(Y, DevicePtr):
        if k is None:
            _stop("k is required with a DevicePtr")
        k = int(k)
    else:
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[:, None]
        if Y.ndim != 2:
            _stop("Y must be a matrix")
        Y = np.asfortranarray(Y)
        k = Y.shape[1]
        if nrow is not None and Y.shape[0] != nrow:
            _stop("nrow(x) should be equal to nrow(Y)")
    if k < 1:
        _stop("y must have at least one column")
    return Y, k


def _binary_columns(Y):
    """Every column of a host label matrix holds exactly 0 and 1, and both (labels behind a DevicePtr are checked by the library)."""
    if isinstance(Y, DevicePtr):
        return
    for c in range(Y.shape[1]):
        col = Y[:, c]
        if not np.all((col == 0.0) | (col == 1.0)):
            _stop(f"column {c} of y: every label must be exactly 0 or 1")
        if np.all(col == 0.0) or np.all(col == 1.0):
            _stop(f"column {c} of y must hold both classes")


def _ovr_indicator(labels):
    """An integer label vector -> (n x classes indicator matrix, the sorted classes): the one-vs-rest builders' Y."""
    lab = np.asarray(labels)
    if lab.ndim != 1:
        _stop("labels must be a vector")
    if not (np.issubdtype(lab.dtype, np.integer) or np.issubdtype(lab.dtype, np.bool_)):
        if not (np.issubdtype(lab.dtype, np.floating) and np.all(np.isfinite(lab)) and np.all(lab == np.round(lab))):
            _stop("labels must be integers")
        lab = lab.astype(np.int64)
    classes = np.unique(lab)
    if classes.size < 2:
        _stop("labels must hold at least two classes")
    return (lab[:, None] == classes[None, :]).astype(np.float64), classes


def _lad_defaults(model, intercept):
    model.maxit = 10000
    model.eps_abs = 1e-4
    model.eps_rel = 1e-4
    model.rho = 1.0
    model.intercept = bool(intercept)


class _DenseFit:
    """What the dense builders' results share: the fields beta, niter and stats, show(), and a repr made of `_title`, the grid fields
    `_grid` (label, attribute), beta -- the values, or its shape and `_beta_noun` -- and niter."""
    _title = _beta_noun = None
    _grid = ()

    def __init__(self, beta, niter, stats):
        self.beta = beta
        self.niter = niter
        self.stats = stats

    def __repr__(self):
        beta = self.beta if self._beta_noun is None else f"<{' x '.join(str(s) for s in np.shape(self.beta))}> {self._beta_noun}"
        blocks = [(label, getattr(self, attr)) for label, attr in self._grid] + [("beta", beta), ("niter", self.niter)]
        return "\n\n".join([self._title] + [f"${label}\n{value}" for label, value in blocks])

    def show(self):
        print(repr(self))


class ADMM_BP_fit(_DenseFit):                                                # ADMM_BP_fit$show (R/10_admm_bp.R:125-133)
    _title, _beta_noun = "ADMM Basis Pursuit fitting result", "sparse matrix"


class ADMM_BP:
    def __init__(self, x, y, n=None, p=None):
        n_, p_ = _shape(x, n, p)
        if n_ >= p_:
            _stop("ncol(x) must be greater than nrow(x)")                        # R/10_admm_bp.R:30-31
        ylen = n_ if isinstance(y, DevicePtr) else len(y)
        if n_ != ylen:
            _stop("nrow(x) should be equal to length(y)")
        self.x, self.y, self.n, self.p = x, y, int(n_), int(p_)
        self.nthread = 1
        self.maxit = 10000
        self.eps_abs = 1e-4
        self.eps_rel = 1e-4
        self.rho = 1.0

    def parallel(self, nthread=2, devices=None):
        """ADMM_BP$parallel (R/10_admm_bp.R:65-76) only stores nthread; $fit() with nthread > 1 then calls the C symbol
        `admm_parbp`, which the reference never builds (it lives in src/TODO/ParBP.cppp) -- the R call fails there; here it
        runs the column-block sharing solver (admm_hip_parbp).  The setter clamps to >= 1 and stores, exactly like R (no
        ncol(x)/5 check here: only ADMM_Lasso$parallel has one, R/30_admm_lasso.R:119-124).  ADMM_LAD inherits this method
        as in R (`contains = "ADMM_BP"`, R/20_admm_lad.R:4) and, as in R, its fit() ignores nthread.  devices: as for
        ADMM_Lasso.parallel (PAR_DEVICES around the admm_hip_parbp call)."""
        self.nthread = max(1, int(nthread))
        self.devices = _devices_option(devices)
        return self

    def opts(self, maxit=10000, eps_abs=1e-4, eps_rel=1e-4, rho=1.0):
        if maxit <= 0:
            _stop("maxit should be positive")
        if eps_abs < 0 or eps_rel < 0:
            _stop("eps_abs and eps_rel should be nonnegative")
        if rho is not None and rho <= 0:
            _stop("rho should be positive")
        self.maxit, self.eps_abs, self.eps_rel = int(maxit), float(eps_abs), float(eps_rel)
        self.rho = 1.0 if rho is None else float(rho)
        return self

    def fit(self, trace=False, state=0):
        """trace=True also returns the decision trace (fit.trace, layout of include/admm_hip.h ADMM_TRACE_*); state = N > 0 (serial
        solver only) also the iterate dump of the first N decisions (fit.state: (records, 5, p) -- x | z | y | adj_z | adj_y,
        admm_hip_bp_state)."""
        if getattr(self, "nthread", 1) > 1:
            # .Call("admm_parbp", x, y, nthread, list(maxit, eps_abs, eps_rel, rho_ratio = rho)), R/10_admm_bp.R:111-116 -- the
            # symbol the reference never builds; here the column-block sharing solver of admm_amd/csrc/sharing_bp.hip
            with _par_devices(self):
                beta, niter, stats, tr, st = _dense_call(self, "admm_hip_parbp", (int(self.nthread),), (), 1, None, trace, width=self.p, records_only=True)
        else:
            beta, niter, stats, tr, st = _dense_call(self, "admm_hip_bp", (), (), 1, self.p, trace, state, width=self.p, records_only=True)
        fit = ADMM_BP_fit(sp.csc_matrix(beta.reshape(-1, 1)), int(niter[0]), stats)             # dgCMatrix p x 1 (BP.cpp:38-43)
        return _with_records(fit, tr, st)


class ADMM_LAD_fit(_DenseFit):
    """beta: numeric p + 1, intercept first (LAD.cpp:40-45)."""
    _title = "ADMM LAD fitting result"


class ADMM_LAD(ADMM_BP):
    def __init__(self, x, y, intercept=True, n=None, p=None):
        n_, p_ = _shape(x, n, p)
        if n_ <= p_:
            _stop("nrow(x) must be greater than ncol(x)")                        # R/20_admm_lad.R:21-22
        ylen = n_ if isinstance(y, DevicePtr) else len(y)
        if n_ != ylen:
            _stop("nrow(x) should be equal to length(y)")
        self.x, self.y, self.n, self.p = x, y, int(n_), int(p_)
        _lad_defaults(self, intercept)

    def fit(self, trace=False, state=0):
        """trace / state as ADMM_BP.fit (the iterate dump has dimension n: admm_hip_lad_state)."""
        beta, niter, stats, tr, st = _dense_call(self, "admm_hip_lad", (int(self.intercept),), (), 1, self.n, trace, state, records_only=True)
        return _with_records(ADMM_LAD_fit(beta, int(niter[0]), stats), tr, st)


class ADMM_QuantReg_fit(_DenseFit):
    _title, _grid, _beta_noun = "ADMM quantile regression fitting result", (("tau", "tau"),), "matrix"

    def __init__(self, tau, beta, niter, stats):
        self.tau = tau              # numeric ntau
        self.beta = beta            # (p + 1) x ntau, column k = tau[k], intercept first
        self.niter = niter          # integer ntau
        self.stats = stats


class ADMM_QuantReg(ADMM_LAD):
    """Quantile regression on LAD's loop (admm_hip_quantreg): one fit per entry of `tau`, the setup paid once.  Unlike ADMM_LAD the
    intercept is fitted (a column of ones), so nrow(x) must exceed ncol(x) + intercept."""

    def __init__(self, x, y, tau=0.5, intercept=True, n=None, p=None):
        _fitted_intercept_shape(x, n, p, intercept)
        ADMM_LAD.__init__(self, x, y, intercept, n, p)
        t = np.atleast_1d(np.asarray(tau, dtype=np.float64))
        if t.ndim != 1 or t.size < 1 or t.size > 4096:
            _stop("tau must hold between 1 and 4096 values")
        if not (np.all(np.isfinite(t)) and np.all(t > 0) and np.all(t < 1)):
            _stop("every tau must lie strictly between 0 and 1")
        self.tau = np.ascontiguousarray(t)

    def fit(self, trace=False, state=0):
        """-> ADMM_QuantReg_fit.  trace / state (as ADMM_LAD.fit, admm_hip_quantreg_state) for a single tau only."""
        ntau = int(self.tau.size)
        if (trace or state) and ntau != 1:
            _stop("trace and state are recorded for a single tau")
        beta, niter, stats, tr, st = _dense_call(self, "admm_hip_quantreg", (int(self.intercept),), (self.tau,), ntau, self.n, trace, state)
        return _with_records(ADMM_QuantReg_fit(self.tau.copy(), beta.reshape(ntau, self.p + 1).T.copy(), niter.copy(), stats), tr, st)


class ADMM_Huber_fit(_DenseFit):
    _title, _grid, _beta_noun = "ADMM Huber regression fitting result", (("delta", "delta"), ("tau", "tau")), "matrix"

    def __init__(self, delta, tau, beta, niter, stats):
        self.delta = delta          # numeric nfit
        self.tau = tau              # numeric nfit
        self.beta = beta            # (p + 1) x nfit, column k = (delta[k], tau[k]), intercept first
        self.niter = niter          # integer nfit
        self.stats = stats


class ADMM_Huber(ADMM_LAD):
    """Huber / expectile regression on LAD's loop (admm_hip_huber): one fit per pair (delta[k], tau[k]), the setup paid once.  delta is in
    the units of y (inf: expectile regression), tau = 0.5 the symmetric Huber loss.  The intercept is fitted as ADMM_QuantReg's."""

    def __init__(self, x, y, delta=1.345, tau=0.5, intercept=True, n=None, p=None):
        _fitted_intercept_shape(x, n, p, intercept)
        ADMM_LAD.__init__(self, x, y, intercept, n, p)
        dl = np.atleast_1d(np.asarray(delta, dtype=np.float64))
        t = np.atleast_1d(np.asarray(tau, dtype=np.float64))
        if dl.ndim != 1 or t.ndim != 1:
            _stop("delta and tau must be scalars or 1-D arrays")
        if dl.size != t.size and dl.size != 1 and t.size != 1:
            _stop("delta and tau must have one common length (or length 1)")
        nfit = max(dl.size, t.size)
        if min(dl.size, t.size) < 1 or nfit > 4096:
            _stop("delta and tau must hold between 1 and 4096 fits")
        if np.any(np.isnan(dl)) or not np.all(dl > 0):
            _stop("every delta must be positive (inf: expectile regression)")
        if not (np.all(np.isfinite(t)) and np.all(t > 0) and np.all(t < 1)):
            _stop("every tau must lie strictly between 0 and 1")
        self.delta = np.array(np.broadcast_to(dl, (nfit,)))
        self.tau = np.array(np.broadcast_to(t, (nfit,)))

    def fit(self, trace=False, state=0):
        """-> ADMM_Huber_fit.  trace / state (as ADMM_LAD.fit, admm_hip_huber_state) for a single fit only."""
        nfit = int(self.tau.size)
        if (trace or state) and nfit != 1:
            _stop("trace and state are recorded for a single fit")
        beta, niter, stats, tr, st = _dense_call(self, "admm_hip_huber", (int(self.intercept),), (self.delta, self.tau), nfit, self.n, trace, state)
        return _with_records(ADMM_Huber_fit(self.delta.copy(), self.tau.copy(), beta.reshape(nfit, self.p + 1).T.copy(), niter.copy(), stats), tr, st)


class ADMM_Logit_fit(_DenseFit):
    """beta: numeric p + 1, intercept first; niter = maxit + 1: not converged (separable labels end there)."""
    _title = "ADMM logistic regression fitting result"


class ADMM_Logit(ADMM_LAD):
    """Logistic regression on LAD's loop (admm_hip_logit): y holds labels, every one exactly 0 or 1, both classes present.  The
    intercept is fitted as ADMM_QuantReg's, so nrow(x) must exceed ncol(x) + intercept.  Labels behind a DevicePtr are checked by the
    library."""

    def __init__(self, x, y, intercept=True, n=None, p=None):
        _fitted_intercept_shape(x, n, p, intercept)
        if not isinstance(y, DevicePtr):
            y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel())
        ADMM_LAD.__init__(self, x, y, intercept, n, p)
        if not isinstance(y, DevicePtr):
            if not np.all((y == 0.0) | (y == 1.0)):
                _stop("every label in y must be exactly 0 or 1")
            if np.all(y == 0.0) or np.all(y == 1.0):
                _stop("y must hold both classes")

    def fit(self, trace=False, state=0):
        """-> ADMM_Logit_fit.  trace / state as ADMM_LAD.fit (admm_hip_logit_state): record 0 of the iterate dump carries the zero response
        in its x slot and the signs 2 y - 1 in its z slot."""
        beta, niter, stats, tr, st = _dense_call(self, "admm_hip_logit", (int(self.intercept),), (), 1, self.n, trace, state)
        return _with_records(ADMM_Logit_fit(beta, int(niter[0]), stats), tr, st)


class ADMM_LogitMulti_fit(_DenseFit):
    """beta: (p + 1) x k, column c = label column c, intercept first; niter: integer k, maxit + 1: that column has not converged."""
    _title, _beta_noun = "ADMM logistic regression fitting result", "matrix"


class ADMM_LogitMulti(ADMM_LAD):
    """Logistic regression for the k columns of a label matrix on ONE setup (admm_hip_logit_multi): column c of the fit is
    admm_logit(x, Y[:, c]), number for number.  Y is n x k (a vector is one column), every label exactly 0 or 1 and both classes present
    in every column; behind a DevicePtr it is column-major, k is required and the library checks the labels."""

    def __init__(self, x, Y, intercept=True, n=None, p=None, k=None):
        _fitted_intercept_shape(x, n, p, intercept)
        Y, k_ = _label_matrix(Y, k)
        ADMM_LAD.__init__(self, x, Y, intercept, n, p)
        self.k = k_
        _binary_columns(Y)

    def fit(self):
        """-> ADMM_LogitMulti_fit (there is no trace / state form)."""
        beta, niter, stats, _, _ = _dense_call(self, "admm_hip_logit_multi", (int(self.intercept),), (), self.k, self.n, k=self.k)
        return ADMM_LogitMulti_fit(beta.reshape((self.p + 1, self.k), order="F"), niter, stats)


class ADMM_LogitOvR(ADMM_LogitMulti):
    """One-vs-rest on ADMM_LogitMulti: `labels` is an integer vector with at least two distinct values; `classes` holds them sorted and
    column c of the fit separates classes[c] from the rest.  No softmax, no calibration: k independent binary fits."""

    def __init__(self, x, labels, intercept=True, n=None, p=None):
        Y, classes = _ovr_indicator(labels)
        ADMM_LogitMulti.__init__(self, x, Y, intercept, n, p)
        self.classes = classes

    def fit(self):
        """-> ADMM_LogitMulti_fit with `classes`."""
        fit = ADMM_LogitMulti.fit(self)
        fit.classes = self.classes
        return fit


def _penalised_fit(model, fit_class, entry, grid, trace, state):
    """fit() of the penalised losses: k label columns times the cells of `grid`, iterates of n + p (the penalty rows behind the data
    rows).  The grid form returns beta as (p + 1) x k x cells and niter as k x cells, the trace form the vector p + 1 and a scalar."""
    ncell = int(grid[0].size)
    beta, niter, stats, tr, st = _dense_call(model, entry, (int(model.intercept),), grid, model.k * ncell, model.n + model.p, trace, state, k=model.k)
    if trace:
        fit = fit_class(*(g.copy() for g in grid), beta, int(niter[0]), stats)
    else:
        fit = fit_class(*(g.copy() for g in grid), beta.reshape((model.p + 1, model.k, ncell), order="F"), niter.reshape((model.k, ncell), order="F"), stats)
    return _with_records(fit, tr, st)


class ADMM_LogitRidge_fit(_DenseFit):
    _title, _grid, _beta_noun = "ADMM ridge logistic regression fitting result", (("lambda", "lam"),), "array"

    def __init__(self, lam, beta, niter, stats):
        self.lam = lam              # numeric nlambda, in the order given
        self.beta = beta            # (p + 1) x k x nlambda, intercept first          (fit(trace=True): p + 1)
        self.niter = niter          # integer k x nlambda; maxit + 1: not converged   (fit(trace=True): a scalar)
        self.stats = stats


class ADMM_LogitRidge(ADMM_LAD):
    """Ridge logistic regression (admm_hip_logit_ridge): per label column c and lambda l
        minimise  sum_i log(1 + exp(-s_i (b0 + x~_i'b))) + lam[l] / 2 sum_j b_j^2,   s = 2 Y[:, c] - 1,
    on the library's standardised columns x~ (scikit-learn's C is 1 / lam on standardised x), the intercept not penalised, the
    coefficients returned on the caller's scale.  Y as ADMM_LogitMulti's; lam: a positive scalar or vector, used in the order given,
    every fit from a cold start.  There is no condition on nrow(x) against ncol(x), and separable labels have an estimate."""

    def __init__(self, x, Y, lam, intercept=True, n=None, p=None, k=None):
        n_, p_ = _shape(x, n, p)
        if n_ < 2:
            _stop("nrow(x) must be at least 2")
        Y, k_ = _label_matrix(Y, k, n_)
        lm = np.atleast_1d(np.asarray(lam, dtype=np.float64))
        if lm.ndim != 1 or lm.size < 1:
            _stop("lam must hold at least one value")
        if not (np.all(np.isfinite(lm)) and np.all(lm > 0)):
            _stop("every lambda must be finite and positive (lambda = 0 is admm_logit_multi)")
        _binary_columns(Y)
        self.x, self.y, self.n, self.p, self.k = x, Y, int(n_), int(p_), k_
        self.lam = np.ascontiguousarray(lm)
        _lad_defaults(self, intercept)

    def fit(self, trace=False, state=0):
        """-> ADMM_LogitRidge_fit.  trace / state (admm_hip_logit_ridge_state) for one column and one lambda only: beta is then the
        vector p + 1 and niter a scalar, and the iterate dump has dimension n + p (the ridge rows behind the data rows); its record 0
        carries the zero response in its x slot and [2 y - 1, 0 ... 0] in its z slot."""
        if (trace or state) and (self.k != 1 or self.lam.size != 1):
            _stop("trace and state are recorded for a single label column and a single lambda")
        return _penalised_fit(self, ADMM_LogitRidge_fit, "admm_hip_logit_ridge", (self.lam,), trace, state)


class ADMM_LogitRidgeOvR(ADMM_LogitRidge):
    """One-vs-rest on ADMM_LogitRidge: the indicator matrix of ADMM_LogitOvR, `classes` sorted, column c separates classes[c] from the rest."""

    def __init__(self, x, labels, lam, intercept=True, n=None, p=None):
        Y, classes = _ovr_indicator(labels)
        ADMM_LogitRidge.__init__(self, x, Y, lam, intercept, n, p)
        self.classes = classes

    def fit(self, trace=False, state=0):
        """-> ADMM_LogitRidge_fit with `classes`."""
        fit = ADMM_LogitRidge.fit(self, trace, state)
        fit.classes = self.classes
        return fit


class ADMM_LogitEnet_fit(_DenseFit):
    _title, _grid, _beta_noun = "ADMM elastic-net logistic regression fitting result", (("lambda", "lam"), ("alpha", "alpha")), "array"

    def __init__(self, lam, alpha, beta, niter, stats):
        self.lam = lam              # numeric ncell, in the order given
        self.alpha = alpha          # numeric ncell: cell l is the pair (lam[l], alpha[l])
        self.beta = beta            # (p + 1) x k x ncell, intercept first            (fit(trace=True): p + 1)
        self.niter = niter          # integer k x ncell; maxit + 1: not converged     (fit(trace=True): a scalar)
        self.stats = stats


class ADMM_LogitEnet(ADMM_LAD):
    """Elastic-net logistic regression (admm_hip_logit_enet): per label column c and cell l = (lam[l], alpha[l])
        minimise  sum_i log(1 + exp(-s_i (b0 + x~_i'b))) + lam[l] (alpha[l] sum_j |b_j| + (1 - alpha[l]) / 2 sum_j b_j^2),   s = 2 Y[:, c] - 1,
    on the library's standardised columns x~ (glmnet's lambda times n), the intercept not penalised, the coefficients returned on the
    caller's scale with exact zeros.  Y as ADMM_LogitMulti's.  lam: None, a positive scalar or a vector; alpha: a scalar in [0, 1] (every
    cell's) or a vector as long as lam (cells are PAIRS).  lam = None: nlambda values log-spaced from max_c lambda_1(c) / alpha down to
    lambda_min_ratio times that (admm_lasso's defaults: 100 values, ratio 1e-4, or 1e-2 when nrow(x) < ncol(x)); it needs a scalar
    alpha > 0 and asks the device for lambda_1 (admm_hip_logit_enet_lambda_max) when fit() or lambda_one() is called.  Every fit starts
    cold, all of them on one inverse; there is no condition on nrow(x) against ncol(x)."""

    # what a loss on these (lam, alpha) cells names: its entry point, its result, the noun of a column of Y and the two rules below
    _entry, _fit_class, _column = "admm_hip_logit_enet", ADMM_LogitEnet_fit, "label column"

    def _check_lambda(self, lm, n, p, intercept):
        if not (np.all(np.isfinite(lm)) and np.all(lm > 0)):
            _stop("every lambda must be finite and positive")

    def _check_response(self, Y):
        _binary_columns(Y)

    def __init__(self, x, Y, lam=None, alpha=1.0, intercept=True, nlambda=100, lambda_min_ratio=None, n=None, p=None, k=None):
        n_, p_ = _shape(x, n, p)
        if n_ < 2:
            _stop("nrow(x) must be at least 2")
        Y, k_ = _label_matrix(Y, k, n_)
        al = np.asarray(alpha, dtype=np.float64)
        if al.ndim > 1 or al.size < 1:
            _stop("alpha must be a scalar or a vector")
        if not np.all((al >= 0.0) & (al <= 1.0)):
            _stop("every alpha must lie in [0, 1]")
        if lam is None:
            if al.ndim != 0 or not float(al) > 0.0:
                _stop("the automatic lambda grid needs one alpha > 0 (alpha = 0 has no lambda_max: pass lam)")
            if int(nlambda) <= 0:
                _stop("nlambda must be a positive integer")
            lmr = (0.01 if n_ < p_ else 0.0001) if lambda_min_ratio is None else float(lambda_min_ratio)
            if lmr <= 0 or lmr >= 1:
                _stop("lambda_min_ratio must be within (0, 1)")
            self.lam, self.alpha = None, np.full(int(nlambda), float(al))
            self.nlambda, self.lambda_min_ratio = int(nlambda), lmr
        else:
            lm = np.atleast_1d(np.asarray(lam, dtype=np.float64))
            if lm.ndim != 1 or lm.size < 1:
                _stop("lam must hold at least one value")
            self._check_lambda(lm, n_, p_, intercept)
            if al.ndim == 1 and al.size != lm.size:
                _stop("alpha must be a scalar or as long as lam (cells are pairs)")
            self.lam = np.ascontiguousarray(lm)
            self.alpha = np.ascontiguousarray(np.broadcast_to(al, lm.shape), dtype=np.float64)
            self.nlambda, self.lambda_min_ratio = int(lm.size), None
        self._check_response(Y)
        self.x, self.y, self.n, self.p, self.k = x, Y, int(n_), int(p_), k_
        _lad_defaults(self, intercept)

    def lambda_one(self):
        """-> (k,) lambda_1 per label column: max_j |x~_j'(y_c - mean(y_c))| (intercept) or |x~_j'(y_c - 1/2)| (none), on the device.
        For alpha > 0 the coefficients of column c are all zero from lambda_1[c] / alpha on."""
        lib = _lib.load()
        xp, xmem, xk = as_input(self.x)
        yp, ymem, yk = as_input(self.y)                # (xk, yk keep the converted buffers alive during the call)
        if xmem != ymem:
            _stop("x and y must live in the same memory space")
        out = np.zeros(self.k, dtype=np.float64)
        check(getattr(lib, self._entry + "_lambda_max")(xp, yp, self.n, self.p, self.k, xmem, int(self.intercept), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return out

    def _cells(self):
        if self.lam is not None:
            return self.lam, self.alpha
        top = float(self.lambda_one().max()) / float(self.alpha[0])
        lam = np.exp(np.linspace(np.log(top), np.log(top * self.lambda_min_ratio), self.nlambda))
        return np.ascontiguousarray(lam), self.alpha

    def fit(self, trace=False, state=0):
        """-> ADMM_LogitEnet_fit.  trace / state (admm_hip_logit_enet_state) for one column and one cell only: beta is then the vector
        p + 1 and niter a scalar, and the iterate dump has dimension n + p (the penalty rows behind the data rows); its record 0
        carries the zero response in its x slot and [2 y - 1, 0 ... 0] in its z slot."""
        if (trace or state) and (self.k != 1 or self.nlambda != 1):
            _stop(f"trace and state are recorded for a single {self._column} and a single cell")
        return _penalised_fit(self, self._fit_class, self._entry, self._cells(), trace, state)        # _cells() may ask the device: after the refusal


class ADMM_LogitEnetOvR(ADMM_LogitEnet):
    """One-vs-rest on ADMM_LogitEnet: the indicator matrix of ADMM_LogitOvR, `classes` sorted, column c separates classes[c] from the rest."""

    def __init__(self, x, labels, lam=None, alpha=1.0, intercept=True, nlambda=100, lambda_min_ratio=None, n=None, p=None):
        Y, classes = _ovr_indicator(labels)
        ADMM_LogitEnet.__init__(self, x, Y, lam, alpha, intercept, nlambda, lambda_min_ratio, n, p)
        self.classes = classes

    def fit(self, trace=False, state=0):
        """-> ADMM_LogitEnet_fit with `classes`."""
        fit = ADMM_LogitEnet.fit(self, trace, state)
        fit.classes = self.classes
        return fit


class ADMM_Poisson_fit(ADMM_LogitEnet_fit):
    _title = "ADMM Poisson regression fitting result"


class ADMM_Poisson(ADMM_LogitEnet):
    """Poisson regression with the elastic-net penalty (admm_hip_poisson): per count column c and cell l = (lam[l], alpha[l])
        minimise  sum_i [exp(eta_i) - Y[i, c] eta_i] + lam[l] (alpha[l] sum_j |b_j| + (1 - alpha[l]) / 2 sum_j b_j^2),   eta_i = b0 + x~_i'b,
    on the library's standardised columns x~ (glmnet family = "poisson" with its lambda times n), the intercept not penalised, the
    coefficients returned on the caller's scale with exact zeros.  Y: n counts or an n x k matrix of them, finite and >= 0 (non-integers
    are accepted), every column with a positive sum.  lam: None, a scalar >= 0 or a vector (0: the plain Poisson GLM, which needs
    nrow(x) > ncol(x) + intercept); alpha: a scalar in [0, 1] (every cell's) or a vector as long as lam (cells are PAIRS).  lam = None:
    nlambda values log-spaced from max_c lambda_1(c) / alpha down to lambda_min_ratio times that, as ADMM_LogitEnet builds them.  Every
    fit starts cold, all of them on one inverse."""

    _entry, _fit_class, _column = "admm_hip_poisson", ADMM_Poisson_fit, "count column"

    def _check_lambda(self, lm, n, p, intercept):
        if not (np.all(np.isfinite(lm)) and np.all(lm >= 0)):
            _stop("every lambda must be finite and non-negative")
        if np.any(lm == 0) and not n > p + int(bool(intercept)):
            _stop("lambda = 0 needs nrow(x) > ncol(x) + intercept")

    def _check_response(self, Y):
        if not isinstance(Y, DevicePtr):
            if not (np.all(np.isfinite(Y)) and np.all(Y >= 0.0)):
                _stop("every y must be finite and non-negative")
            if not np.all(Y.sum(axis=0) > 0.0):
                _stop("every column of y must have a positive sum")

    def lambda_one(self):
        """-> (k,) lambda_1 per count column: max_j |x~_j'(y_c - mean(y_c))| (intercept) or |x~_j'(y_c - 1)| (none), on the device.
        For alpha > 0 the coefficients of column c are all zero from lambda_1[c] / alpha on."""
        return ADMM_LogitEnet.lambda_one(self)

    def fit(self, trace=False, state=0):
        """-> ADMM_Poisson_fit.  trace / state (admm_hip_poisson_state) for one column and one cell only: beta is then the vector p + 1
        and niter a scalar, and the iterate dump has dimension n + p (the penalty rows behind the data rows); its record 0 carries the
        zero response in its x slot and [y, -1 ... -1] in its z slot."""
        return ADMM_LogitEnet.fit(self, trace, state)


class ADMM_LogitEnetCV_fit(ADMM_LogitEnet_fit):
    """The full-data fit (lam, alpha, beta, niter as ADMM_LogitEnet_fit's) and the cross-validation tables: cv_mean, cv_se (k x ncell),
    fold_dev, fold_niter (nfolds x k x ncell), fold_beta (nfolds x (p + 1) x k x ncell), idx_min, idx_1se (k: cell indices), lambda_min,
    lambda_1se (k: lam at those cells), fold_id (n).  A fit with trace carries none of them."""
    _title = "ADMM elastic-net logistic regression cross-validation result"


class ADMM_PoissonCV_fit(ADMM_LogitEnetCV_fit):
    _title = "ADMM Poisson regression cross-validation result"


def _cv_folds(model, nfolds, fold_id):
    """The folds of a cross-validation builder: nfolds within [2, n]; fold_id None (row i in fold i mod nfolds) or n integers in
    [0, nfolds), every fold present."""
    nfolds = int(nfolds)
    if nfolds < 2 or nfolds > model.n:
        _stop("nfolds must be within [2, nrow(x)]")
    if fold_id is not None:
        fold_id = np.asarray(fold_id)
        if fold_id.shape != (model.n,) or not np.issubdtype(fold_id.dtype, np.integer):
            _stop("fold_id must hold nrow(x) integers")
        if fold_id.min() < 0 or fold_id.max() >= nfolds:
            _stop("fold_id entries must be within [0, nfolds)")
        if np.unique(fold_id).size != nfolds:
            _stop("every fold needs at least one held-out row")
        fold_id = np.ascontiguousarray(fold_id, dtype=np.int32)
    model.nfolds, model.fold_id = nfolds, fold_id


def _cv_fit(model, trace, state, fold):
    """fit() of the cross-validation builders: <entry>_cv for the grid, <entry>_cv_state for one column, one cell and one fold."""
    ip = ctypes.POINTER(ctypes.c_int)
    folds = (None if model.fold_id is None else model.fold_id.ctypes.data_as(ip), model.nfolds)
    fold = int(fold)
    if trace or state:
        if model.k != 1 or model.nlambda != 1:
            _stop(f"trace and state are recorded for a single {model._column} and a single cell")
        if fold < -1 or fold >= model.nfolds:
            _stop("fold must be within [-1, nfolds)")
    grid = model._cells()
    ncell, k, p, F = int(grid[0].size), model.k, model.p, model.nfolds
    if trace:
        beta, niter, stats, tr, st = _dense_call(model, model._entry + "_cv", (int(model.intercept), *folds, fold), grid, 1, model.n + p, trace, state)
        return _with_records(model._cv_fit_class(*(g.copy() for g in grid), beta, int(niter[0]), stats), tr, st)
    tables = [np.zeros(k * ncell), np.zeros(k * ncell), np.zeros(F * k * ncell), np.zeros(F * k * ncell, dtype=np.int32), np.zeros(F * k * ncell * (p + 1)),
              np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.int32)]
    beta, niter, stats, _, _ = _dense_call(model, model._entry + "_cv", (int(model.intercept), *folds), grid, k * ncell, model.n + p, k=k, tables=tables)
    fit = model._cv_fit_class(*(g.copy() for g in grid), beta.reshape((p + 1, k, ncell), order="F"), niter.reshape((k, ncell), order="F"), stats)
    fit.cv_mean, fit.cv_se = (t.reshape((k, ncell), order="F") for t in tables[:2])
    fit.fold_dev, fit.fold_niter = (t.reshape((F, ncell, k)).transpose(0, 2, 1) for t in tables[2:4])
    fit.fold_beta = tables[4].reshape((F, ncell, k, p + 1)).transpose(0, 3, 2, 1)
    fit.idx_min, fit.idx_1se = tables[5], tables[6]
    fit.lambda_min, fit.lambda_1se = fit.lam[fit.idx_min], fit.lam[fit.idx_1se]
    fit.fold_id = np.arange(model.n, dtype=np.int32) % F if model.fold_id is None else model.fold_id.copy()
    return _with_records(fit, None, None)


class ADMM_LogitEnetCV(ADMM_LogitEnet):
    """K-fold cross-validation of ADMM_LogitEnet's (column, cell) grid by held-out binomial deviance (admm_hip_logit_enet_cv): all
    k x ncell x (nfolds + 1) fits on the full-data setup -- a held-out row is a row without loss.  fold_id: None (row i is in fold
    i mod nfolds) or n integers in [0, nfolds).  The folds use the full-data standardisation; deviance is the only measure."""
    _cv_fit_class = ADMM_LogitEnetCV_fit

    def __init__(self, x, Y, lam=None, alpha=1.0, nfolds=10, fold_id=None, intercept=True, nlambda=100, lambda_min_ratio=None, n=None, p=None, k=None):
        ADMM_LogitEnet.__init__(self, x, Y, lam, alpha, intercept, nlambda, lambda_min_ratio, n, p, k)
        _cv_folds(self, nfolds, fold_id)

    def fit(self, trace=False, state=0, fold=-1):
        """-> ADMM_LogitEnetCV_fit.  trace / state (admm_hip_logit_enet_cv_state) for one column and one cell only, with `fold` held
        out (-1: none): record 0's z slot then carries the tags the loop ran with, 2.0 on the held-out rows."""
        return _cv_fit(self, trace, state, fold)


class ADMM_PoissonCV(ADMM_Poisson):
    """K-fold cross-validation of ADMM_Poisson's grid by held-out Poisson deviance (admm_hip_poisson_cv), as ADMM_LogitEnetCV."""
    _cv_fit_class = ADMM_PoissonCV_fit

    def __init__(self, x, Y, lam=None, alpha=1.0, nfolds=10, fold_id=None, intercept=True, nlambda=100, lambda_min_ratio=None, n=None, p=None, k=None):
        ADMM_Poisson.__init__(self, x, Y, lam, alpha, intercept, nlambda, lambda_min_ratio, n, p, k)
        _cv_folds(self, nfolds, fold_id)

    def fit(self, trace=False, state=0, fold=-1):
        """-> ADMM_PoissonCV_fit.  trace / state (admm_hip_poisson_cv_state) as ADMM_LogitEnetCV.fit; the held-out tag is -2.0."""
        return _cv_fit(self, trace, state, fold)


class LassoPlan:
    """Prepared problem (admm_hip_lasso_plan_*): setup once, run the lambda path repeatedly.

    Built from a configured ADMM_Lasso / ADMM_Enet object; used by bench.py to time the ADMM
    loop without the one-time Gram/factorisation."""

    def __init__(self, model):
        if isinstance(model, ADMM_Dantzig):
            _stop(ADMM_Dantzig._missing)
        lib = _lib.load()
        self._lib = lib
        self.model = model
        xp, xmem, xk = as_input(model.x)
        yp, ymem, yk = as_input(model.y)
        lam_in = np.ascontiguousarray(model.lambda_, dtype=np.float64)
        o = AdmmOpts(model.maxit, model.eps_abs, model.eps_rel, model.rho)
        h = ctypes.c_void_p()
        nl = ctypes.c_int()
        head = (xp, yp, model.n, model.p, xmem, ctypes.c_void_p(lam_in.ctypes.data if lam_in.size else 0), int(lam_in.size),
                model.nlambda, model.lambda_min_ratio, int(model.standardize), int(model.intercept))
        check(getattr(lib, model._plan_entry)(*model._plan_args(head), ctypes.byref(o), ctypes.byref(h), ctypes.byref(nl)))
        self._h = h
        self.nlambda = nl.value

    def run(self):
        m = self.model
        lam_out = np.zeros(self.nlambda, dtype=np.float64)
        beta = m._beta_buffer(self.nlambda)
        niter = np.zeros(self.nlambda, dtype=np.int32)
        stats = AdmmStats()
        check(self._lib.admm_hip_lasso_plan_run(self._h, lam_out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                beta.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                niter.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(stats)))
        return m._result(lam_out, beta, niter, stats.as_dict())

    def enable_trace(self, capacity=1 << 18):
        """Record one decision record per ADMM iteration of the following run() calls (tall path only)."""
        check(self._lib.admm_hip_lasso_plan_trace_enable(self._h, int(capacity)))
        self._trace_cap = int(capacity)

    def read_trace(self):
        """(nrecords, TRACE_FIELDS) float64 array of the last run(): see include/admm_hip.h."""
        buf = np.zeros((self._trace_cap, _lib.TRACE_FIELDS), dtype=np.float64)
        n = ctypes.c_longlong()
        check(self._lib.admm_hip_lasso_plan_trace_read(self._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                       self._trace_cap, ctypes.byref(n)))
        return buf[:n.value].copy()

    def enable_state(self, capacity):
        """Also dump the iterates of every iteration of the following run() calls (tall and consensus solvers; include/admm_hip.h,
        admm_hip_lasso_plan_state_*): record s = the iterates trace record s judged."""
        check(self._lib.admm_hip_lasso_plan_state_enable(self._h, int(capacity)))
        self._state_cap = int(capacity)

    def read_state(self):
        """(nrecords, record_floats) float32 array of the last run()."""
        n, rf = ctypes.c_longlong(), ctypes.c_longlong()
        check(self._lib.admm_hip_lasso_plan_state_read(self._h, None, 0, ctypes.byref(n), ctypes.byref(rf)))     # size query
        nrec = max(int(n.value), 1)
        buf = np.zeros((nrec, rf.value), dtype=np.float32)
        check(self._lib.admm_hip_lasso_plan_state_read(self._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), nrec,
                                                       ctypes.byref(n), ctypes.byref(rf)))
        return buf[:n.value]

    def read_data(self):
        """(X, Y): the standardised float32 data as the wide solver holds them (admm_hip_lasso_plan_data_read)."""
        m = self.model
        X = np.zeros((m.n, m.p), dtype=np.float32, order="F")
        Y = np.zeros(m.n, dtype=np.float32)
        check(self._lib.admm_hip_lasso_plan_data_read(self._h, X.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), m.n,
                                                      Y.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return X, Y

    def read_system(self):
        """(p, p) float32: the system matrix X'X + rho I as this library formed it (tall solver, ADMM_HIP_REFINE=1 only)."""
        p = self.model.p
        out = np.zeros((p, p), dtype=np.float32, order="F")
        check(self._lib.admm_hip_lasso_plan_system_read(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), p))
        return out

    def close(self):
        if self._h:
            check(self._lib.admm_hip_lasso_plan_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def admm_lasso(x, y, intercept=True, standardize=True, **kw):
    return ADMM_Lasso(x, y, intercept, standardize, **kw)


def admm_enet(x, y, intercept=True, standardize=True, **kw):
    return ADMM_Enet(x, y, intercept, standardize, **kw)


def admm_lad(x, y, intercept=True, **kw):
    return ADMM_LAD(x, y, intercept, **kw)


def admm_quantreg(x, y, tau=0.5, intercept=True, **kw):
    return ADMM_QuantReg(x, y, tau, intercept, **kw)


def admm_huber(x, y, delta=1.345, tau=0.5, intercept=True, **kw):
    return ADMM_Huber(x, y, delta, tau, intercept, **kw)


def admm_logit(x, y, intercept=True, **kw):
    return ADMM_Logit(x, y, intercept, **kw)


def admm_logit_multi(x, Y, intercept=True, **kw):
    return ADMM_LogitMulti(x, Y, intercept, **kw)


def admm_logit_ovr(x, labels, intercept=True, **kw):
    return ADMM_LogitOvR(x, labels, intercept, **kw)


def admm_logit_ridge(x, Y, lam, intercept=True, **kw):
    return ADMM_LogitRidge(x, Y, lam, intercept, **kw)


def admm_logit_ridge_ovr(x, labels, lam, intercept=True, **kw):
    return ADMM_LogitRidgeOvR(x, labels, lam, intercept, **kw)


def admm_logit_enet(x, Y, lam=None, alpha=1.0, intercept=True, nlambda=100, lambda_min_ratio=None, **kw):
    return ADMM_LogitEnet(x, Y, lam, alpha, intercept, nlambda, lambda_min_ratio, **kw)


def admm_logit_enet_ovr(x, labels, lam=None, alpha=1.0, intercept=True, nlambda=100, lambda_min_ratio=None, **kw):
    return ADMM_LogitEnetOvR(x, labels, lam, alpha, intercept, nlambda, lambda_min_ratio, **kw)


def admm_poisson(x, Y, lam=None, alpha=1.0, intercept=True, nlambda=100, lambda_min_ratio=None, **kw):
    return ADMM_Poisson(x, Y, lam, alpha, intercept, nlambda, lambda_min_ratio, **kw)


def admm_logit_enet_cv(x, Y, lam=None, alpha=1.0, nfolds=10, fold_id=None, intercept=True, nlambda=100, lambda_min_ratio=None, **kw):
    return ADMM_LogitEnetCV(x, Y, lam, alpha, nfolds, fold_id, intercept, nlambda, lambda_min_ratio, **kw)


def admm_poisson_cv(x, Y, lam=None, alpha=1.0, nfolds=10, fold_id=None, intercept=True, nlambda=100, lambda_min_ratio=None, **kw):
    return ADMM_PoissonCV(x, Y, lam, alpha, nfolds, fold_id, intercept, nlambda, lambda_min_ratio, **kw)


def admm_bp(x, y, **kw):
    return ADMM_BP(x, y, **kw)


class ADMM_Dantzig(ADMM_Lasso):
    """`admm_dantzig` is exported by the reference (NAMESPACE:13, R/50_admm_dantzig.R) but its `.Call("admm_dantzig", ...)`
    names a symbol the package never builds: the solver lives in src/TODO/ (Dantzig.cpp, ADMMDantzig.h, written against an
    older ADMMBase) and is not compiled, so `$fit()` fails in R.  Here fit() runs that algorithm restated on the current
    ADMMBase::solve (admm_hip_dantzig; admm_amd/csrc/dantzig.hip, oracle/solvers.py Dantzig) -- double precision like its
    `typedef double Scalar`.  It converges on comfortably tall problems (n >= 5 p) and, as the restated algorithm itself, not for
    p > n (tests/test_oracle_dantzig.py): niter = maxit + 1 marks such a lambda.  The builder chain is ADMM_Lasso's
    (R/50_admm_dantzig.R:2 `contains = "ADMM_Lasso"`): $parallel stores nthread as there and, as there, $fit ignores it."""
    _name = "ADMM Dantzig Selector model"

    _missing = "not available for the Dantzig selector (the reference has no such entry point)"

    def fit(self, trace=False):
        lib, head, tail, lam_out, _, niter, stats, keep = self._common()
        beta = np.zeros((self.p + 1, lam_out.size), dtype=np.float64, order="F")
        tr, ntr = _trace_buffers(self.maxit * lam_out.size + 2 * lam_out.size if trace else 0)
        check(lib.admm_hip_dantzig_traced(*head, tail[0], tail[1], beta.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), tail[3], tail[4],
                                          *_trace_args(tr, ntr)))
        fit = ADMM_Lasso_fit(lam_out, beta, niter, stats.as_dict())
        fit._title = "ADMM Dantzig Selector fitting result"                     # ADMM_Dantzig_fit$show, R/50_admm_dantzig.R:52-58
        fit.trace = tr[:ntr.value].copy() if trace else None
        return fit

    # the extensions of this build that ride on ADMM_Lasso (cross-validation, several responses, prepared problems, row blocks)
    # must not run a plain Lasso under a Dantzig label
    def cv(self, *a, **kw):
        _stop(self._missing)

    def fit_responses(self, *a, **kw):
        _stop(self._missing)


def admm_dantzig(x, y, intercept=True, standardize=True, **kw):
    return ADMM_Dantzig(x, y, intercept, standardize, **kw)


def _weights(a, size, size_msg, bad_msg, positive_msg=None):
    """A weight argument of a tall-only penalty as the library takes it: `size` float64 values, finite and non-negative and, where
    positive_msg is given, not all zero."""
    w = np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())
    if w.size != size:
        _stop(size_msg)
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        _stop(bad_msg)
    if positive_msg is not None and not np.any(w > 0):
        _stop(positive_msg)
    return w


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if a is not None else None


class _TallOnly(ADMM_Lasso):
    """What the builders of the tall-only penalties share (n > p, one device): the refusals and one fit() / plan creation, driven by
    per-class data -- _entry (the C entry point; its plan form is <_entry>_plan_create), _tall_only and _missing (the refusals' texts),
    _title (of the fit; None: the result has its own) -- and by _extra_args(head), which replace head[_extra_at:5] of the Lasso's
    arguments.  _beta_buffer and _result are ADMM_Lasso's hooks."""
    _extra_at = 5
    _title = None

    def __init__(self, x, y, intercept=True, standardize=True, n=None, p=None):
        super().__init__(x, y, intercept, standardize, n, p)
        if self.n <= self.p:
            _stop("nrow(x) must be greater than ncol(x): " + self._tall_only)

    def parallel(self, *a, **kw):
        _stop(self._missing)

    def cv(self, *a, **kw):
        _stop(self._missing)

    def fit_responses(self, *a, **kw):
        _stop(self._missing)

    @property
    def _plan_entry(self):
        return self._entry + "_plan_create"

    def _plan_args(self, head):                                      # (what leads the arguments of a fit too)
        return head[:self._extra_at] + tuple(self._extra_args(head)) + head[5:]

    def fit(self):
        lib, head, tail, lam_out, beta, niter, stats, keep = self._common()
        check(getattr(lib, self._entry)(*self._plan_args(head), *tail))
        fit = self._result(lam_out, beta, niter, stats.as_dict())
        if self._title is not None:
            fit._title = self._title
        return fit


class ADMM_GrpLasso(_TallOnly):
    """Group lasso on the tall path (admm_hip_grplasso; n > p only, one device): `group` gives one label per column, columns with
    the same label enter or leave the model together.  Labels are arbitrary; the groups are numbered in order of first appearance
    (`group_labels`), and that is the order of `group_weights`.  The library wants the columns of a group adjacent: host input
    with scattered groups is reordered here and the coefficients are put back in the caller's column order; a DevicePtr is used in
    place, so scattered groups are refused for it."""
    _name = "ADMM Group Lasso model"
    _missing = "not available for the group lasso (single-device tall solver only)"
    _tall_only = "the group lasso is built for n > p only"
    _entry, _title = "admm_hip_grplasso", "ADMM Group Lasso fitting result"

    def __init__(self, x, y, group, intercept=True, standardize=True, n=None, p=None):
        super().__init__(x, y, intercept, standardize, n, p)
        g = np.asarray(group).ravel()
        if g.size != self.p:
            _stop("group should have length ncol(x)")
        labels, first, inverse = np.unique(g, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")                    # groups in order of first appearance
        rank = np.empty(order.size, dtype=np.int64)
        rank[order] = np.arange(order.size)
        ids = rank[np.asarray(inverse).ravel()]
        self.group_labels = labels[order]
        self.ngroups = int(order.size)
        self._perm = None
        if np.any(np.diff(ids) < 0):
            if isinstance(x, DevicePtr):
                _stop("the columns of a group must be adjacent with a DevicePtr (host input is reordered automatically)")
            self._perm = np.argsort(ids, kind="stable")              # library column k = caller's column _perm[k]
            self.x = np.asfortranarray(np.asarray(x, dtype=np.float64)[:, self._perm])
            ids = ids[self._perm]
        self.group = np.ascontiguousarray(ids, dtype=np.int32)
        self.group_sizes = np.bincount(self.group, minlength=self.ngroups)
        if self.group_sizes.max() > _lib.GROUP_MAX:
            _stop(f"a group has more than {_lib.GROUP_MAX} columns")
        self.group_weights = None                                    # library default: sqrt(group size)

    def penalty(self, lambda_=None, nlambda=100, lambda_min_ratio=None, group_weights=None, **kw):
        super().penalty(lambda_, nlambda, lambda_min_ratio, **kw)
        self.group_weights = None if group_weights is None else self._group_weights(group_weights, "at least one group weight must be positive")
        return self

    def _group_weights(self, w, positive_msg=None):
        return _weights(w, self.ngroups, "group_weights should have one entry per group (in order of first appearance)",
                        "group_weights must be finite and non-negative", positive_msg)

    def effective_weights(self):
        return np.sqrt(self.group_sizes.astype(np.float64)) if self.group_weights is None else self.group_weights

    def _group_args(self):
        return self.group.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dp(self.group_weights), self.ngroups

    def _extra_args(self, head):
        return self._group_args()

    def _restore(self, beta):
        """Coefficient rows back into the caller's column order (row 0 is the intercept)."""
        if self._perm is None:
            return beta
        out = np.zeros_like(beta)
        out[0] = beta[0]
        out[1 + self._perm] = beta[1:]
        return out

    def _result(self, lam, beta, niter, stats):
        return ADMM_Lasso_fit(lam, self._restore(beta), niter, stats)


def admm_grplasso(x, y, group, intercept=True, standardize=True, **kw):
    return ADMM_GrpLasso(x, y, group, intercept, standardize, **kw)


class ADMM_SGL(ADMM_GrpLasso):
    """Sparse-group lasso on the tall path (admm_hip_sgl; n > p only, one device): the group lasso's model with the penalty
    lambda (alpha sum_j u_j |b_j| + (1 - alpha) sum_g w_g ||b_g||_2), which selects groups and coefficients inside the groups it keeps.
    `group` as for admm_grplasso; `l1_weights` (u, one per column, default 1) are given in the CALLER's column order and travel with the
    columns when scattered groups are reordered.  alpha = 0 is the group lasso, alpha = 1 the Lasso with penalty factors u."""
    _name = "ADMM Sparse-Group Lasso model"
    _missing = "not available for the sparse-group lasso (single-device tall solver only)"
    _entry, _title = "admm_hip_sgl", "ADMM Sparse-Group Lasso fitting result"

    def __init__(self, x, y, group, alpha=0.95, intercept=True, standardize=True, n=None, p=None):
        super().__init__(x, y, group, intercept, standardize, n, p)
        a = float(alpha)
        if not (np.isfinite(a) and 0.0 <= a <= 1.0):
            _stop("alpha must be within [0, 1]")
        self.alpha = a
        self.l1_weights = None                                       # library default: 1 for every column

    def penalty(self, lambda_=None, nlambda=100, lambda_min_ratio=None, group_weights=None, l1_weights=None, **kw):
        ADMM_Lasso.penalty(self, lambda_, nlambda, lambda_min_ratio, **kw)
        w = None if group_weights is None else self._group_weights(group_weights)
        u = None
        if l1_weights is not None:
            u = _weights(l1_weights, self.p, "l1_weights should have one entry per column", "l1_weights must be finite and non-negative")
            u = np.ascontiguousarray(u if self._perm is None else u[self._perm])      # library column k = caller's column _perm[k]
        wg = (1.0 - self.alpha) * (np.ones(self.ngroups) if w is None else w)
        l1 = self.alpha * (np.ones(self.p) if u is None else u)
        if not (np.any(l1 > 0) or np.any(wg > 0)):
            _stop("at least one coordinate must carry a positive penalty")
        self.group_weights, self.l1_weights = w, u
        return self

    def _group_args(self):
        return super()._group_args() + (_dp(self.l1_weights), self.alpha)


def admm_sgl(x, y, group, alpha=0.95, intercept=True, standardize=True, **kw):
    return ADMM_SGL(x, y, group, alpha, intercept, standardize, **kw)


class ADMM_BoxEnet(_TallOnly):
    """Box-constrained, weighted elastic net on the tall path (admm_hip_boxenet; n > p only, one device): the Lasso (alpha=None) or the
    elastic net (0 <= alpha <= 1) with a penalty factor per column and bounds lower_j <= beta_j <= upper_j on the ORIGINAL coefficient
    scale -- glmnet's lower.limits / upper.limits / penalty.factor, scikit-learn's positive=True as lower=0.  `lower` <= 0 <= `upper`
    (zero must stay feasible; lower = upper = 0 excludes a column); scalars are broadcast to all columns, None means no bound.
    penalty_factor multiplies the whole penalty of its column; 0 leaves it unpenalised."""
    _name = "ADMM Box-Constrained Elastic Net model"
    _missing = "not available for the box-constrained elastic net (single-device tall solver only)"
    _tall_only = "the box-constrained elastic net is built for n > p only (the wide solver is not built for bounds)"
    _entry, _title = "admm_hip_boxenet", "ADMM Box-Constrained Elastic Net fitting result"

    def __init__(self, x, y, lower=None, upper=None, intercept=True, standardize=True, n=None, p=None):
        super().__init__(x, y, intercept, standardize, n, p)
        self.lower = self._per_column(lower, "lower")
        self.upper = self._per_column(upper, "upper")
        if self.lower is not None and not np.all(self.lower <= 0):
            _stop("lower bounds must be <= 0 (zero must be feasible) and not NaN")
        if self.upper is not None and not np.all(self.upper >= 0):
            _stop("upper bounds must be >= 0 (zero must be feasible) and not NaN")
        self.alpha = None                                            # the Lasso prox
        self.penalty_factor = None                                   # library default: 1 for every column

    def _per_column(self, v, name):
        if v is None:
            return None
        a = np.asarray(v, dtype=np.float64).ravel()
        if a.size == 1:
            a = np.full(self.p, float(a[0]))
        if a.size != self.p:
            _stop(f"{name} should be a scalar or have one entry per column")
        return np.ascontiguousarray(a)

    def penalty(self, lambda_=None, nlambda=100, lambda_min_ratio=None, alpha=None, penalty_factor=None, **kw):
        super().penalty(lambda_, nlambda, lambda_min_ratio, **kw)
        if alpha is not None:
            alpha = float(alpha)
            if not 0.0 <= alpha <= 1.0:                                  # (NaN fails both comparisons)
                _stop("alpha must be None (the Lasso prox) or within [0, 1] (the elastic net's)")
        u = self._per_column(penalty_factor, "penalty_factor")
        if u is not None:                                                # (_per_column fixed its length)
            u = _weights(u, self.p, None, "penalty factors must be finite and non-negative", "at least one penalty factor must be positive")
        self.alpha, self.penalty_factor = alpha, u
        return self

    def _box_args(self):
        return _dp(self.lower), _dp(self.upper), _dp(self.penalty_factor), -1.0 if self.alpha is None else self.alpha

    def _extra_args(self, head):
        return self._box_args()


def admm_boxenet(x, y, lower=None, upper=None, intercept=True, standardize=True, **kw):
    return ADMM_BoxEnet(x, y, lower, upper, intercept, standardize, **kw)


class ADMM_MTLasso_fit:
    """Fields lambda, beta_dense ((m, p + 1, nlambda): response, intercept + coefficients, lambda), niter (one count per lambda)."""

    def __init__(self, lam, beta_lmp, niter, stats):
        self.lambda_ = lam
        self.beta_dense = np.ascontiguousarray(np.transpose(beta_lmp, (1, 2, 0)))      # the library writes [nlambda][m][p + 1]
        self.niter = niter
        self.stats = stats

    @property
    def beta(self):
        """One dgCMatrix-like CSC ((p + 1) x nlambda) per response."""
        return [_beta_to_csc(b) for b in self.beta_dense]

    def __repr__(self):
        m, p1, nl = self.beta_dense.shape
        return (f"ADMM multi-task Lasso fitting result\n\n$lambda\n{self.lambda_}\n\n$beta\n{m} responses, each <{p1} x {nl}>\n\n$niter\n{self.niter}")

    def show(self):
        print(repr(self))


class ADMM_MTLasso(_TallOnly):
    """Multi-task lasso on the tall path (admm_hip_mtlasso; n > p only, one device): Y is n x m, one row-wise penalty
    lambda sum_j w_j ||B_j.||_2 selects a column of x for all responses at once.  All responses share one cached inverse, so an
    iteration streams it once for several of them (option MT_RHS).  With a DevicePtr for Y pass m."""
    _name = "ADMM multi-task Lasso model"
    _missing = "not available for the multi-task lasso (single-device tall solver only)"
    _tall_only = "the multi-task lasso is built for n > p only"
    _entry, _extra_at = "admm_hip_mtlasso", 4                       # m goes before mem, the weights after it

    def __init__(self, x, Y, intercept=True, standardize=True, n=None, p=None, m=None):
        if isinstance(Y, DevicePtr):
            if m is None:
                _stop("m (the number of responses) is needed with a device pointer")
            m = int(m)
        else:
            Y = np.asarray(Y, dtype=np.float64)
            if Y.ndim == 1:
                Y = Y.reshape(-1, 1)
            if Y.ndim != 2:
                _stop("Y should be a matrix with nrow(x) rows")
            Y = np.asfortranarray(Y)
            m = Y.shape[1]
        super().__init__(x, Y, intercept, standardize, n, p)
        if m < 1 or m > _lib.MT_MAX:
            _stop(f"the number of responses must be within [1, {_lib.MT_MAX}]")
        self.m = m
        self.row_weights = None                                      # library default: 1 for every row

    def penalty(self, lambda_=None, nlambda=100, lambda_min_ratio=None, row_weights=None, **kw):
        super().penalty(lambda_, nlambda, lambda_min_ratio, **kw)
        if row_weights is not None:
            row_weights = _weights(row_weights, self.p, "row_weights should have one entry per column of x",
                                   "row_weights must be finite and non-negative", "at least one row weight must be positive")
        self.row_weights = row_weights
        return self

    def _weight_arg(self):
        return _dp(self.row_weights)

    def _extra_args(self, head):
        return self.m, head[4], self._weight_arg()

    def _beta_buffer(self, nl):
        return np.zeros((nl, self.m, self.p + 1), dtype=np.float32)

    def _result(self, lam, beta, niter, stats):
        return ADMM_MTLasso_fit(lam, beta, niter, stats)


def admm_mtlasso(x, Y, intercept=True, standardize=True, **kw):
    return ADMM_MTLasso(x, Y, intercept, standardize, **kw)
