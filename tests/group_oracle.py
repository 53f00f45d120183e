"""NumPy restatement of the group lasso of admm_hip_grplasso (TEST INFRASTRUCTURE): the tall solver's fast ADMM
(oracle/solvers.py LassoTall, unchanged) with the z-update replaced by a block soft-threshold and lambda_0 by the largest
weighted group norm of X'y, plus a path driver and the group KKT figures.

In the solver's internal units (standardised X_s, y_s; lambda_int = lambda n / scaleY) the problem is
    minimise 1/2 ||y_s - X_s b||^2 + lambda_int sum_g w_g ||b_g||_2 .
next_z, with v = x + adj_y / rho (in T) and pen_g = lambda_int w_g / rho (double):
    size 1:  the Lasso's soft-threshold (double compare, (T)(v -+ pen));
    size > 1:  nrm = sqrt(sum (double) v_i^2),  s = nrm > pen ? 1 - pen / nrm : 0,  z_i = (T)((double) v_i s).
T is float32 as the library computes; float64 gives the reference optimum of the distance test."""
import numpy as np
import scipy.linalg as sla

from oracle.datastd import DataStd
from oracle.solvers import LassoTall, _soft_d
from oracle.spectra import sym_eigs_largest

F = np.float32


def group_starts(sizes):
    sizes = np.asarray(sizes, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def default_weights(sizes):
    return np.sqrt(np.asarray(sizes, dtype=np.float64))


def group_prox(vec, sizes, weights, lam, rho, T=F):
    """next_z of the group lasso on v = vec (dtype T).  Returns (z, nrm, pen): the norms (double; |v| for singletons) and
    thresholds per group."""
    sizes = np.asarray(sizes, dtype=np.int64)
    st = group_starts(sizes)
    gid = np.repeat(np.arange(sizes.size), sizes)
    pen = np.float64(lam) * np.asarray(weights, dtype=np.float64) / np.float64(rho)
    v = vec.astype(np.float64)
    nrm = np.sqrt(np.add.reduceat(v * v, st[:-1]))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(nrm > pen, 1.0 - pen / nrm, 0.0)
    z = (v * s[gid]).astype(T)
    single = (sizes == 1)[gid]
    if single.any():
        z[single] = _soft_d(vec[single], pen[gid][single], T)
    return z, nrm, pen


class GroupLassoTall(LassoTall):
    """LassoTall with groups.  `T` is the working type (float32 as the library, float64 for the reference optimum); LassoTall
    hard-codes float32 in init / next_x, so those two are restated here in T with the same rounding of the right-hand side."""

    def __init__(self, X, Y, eps_abs, eps_rel, sizes, weights=None, T=F):
        self.T = T
        self.X, self.Y = X, Y
        self.p = X.shape[1]
        self.eps_abs, self.eps_rel = eps_abs, eps_rel
        self.alpha = None
        self.info = {}
        self.sizes = np.asarray(sizes, dtype=np.int64)
        assert self.sizes.sum() == self.p and self.sizes.min() >= 1
        self.weights = default_weights(self.sizes) if weights is None else np.asarray(weights, dtype=np.float64)
        self.XY = (X.T @ Y).astype(T)
        xy = self.XY.astype(np.float64)
        gn = np.sqrt(np.add.reduceat(xy * xy, group_starts(self.sizes)[:-1]))
        pos = self.weights > 0
        self.lambda0 = T(np.max(gn[pos] / self.weights[pos]))

    def init(self, lam, rho):
        T, p = self.T, self.p
        self.main_x = np.zeros(p, T)
        self.aux_z = np.zeros(p, T)
        self.dual_y = np.zeros(p, T)
        self.adj_z = np.zeros(p, T)
        self.adj_y = np.zeros(p, T)
        self.lam = T(lam)
        self.rho = float(rho)
        XX = (self.X.T @ self.X).astype(T)
        if self.rho <= 0:
            ev = sym_eigs_largest(lambda v: XX @ v, p, 3, 10, 0.1, T, self.info)
            self.lmax_est = ev
            self.rho = float(np.float64(ev) ** (1.0 / 3) * np.float64(self.lam) ** (2.0 / 3))
        XX[np.arange(p), np.arange(p)] += T(self.rho)
        self.chol = sla.cho_factor(XX, lower=True, check_finite=False)
        self.eps_primal = self.eps_dual = 0.0
        self.resid_primal = self.resid_dual = 9999.0
        self._init_accel()

    def init_warm(self, lam):
        self.lam = self.T(lam)
        self.eps_primal = self.eps_dual = 0.0
        self.resid_primal = self.resid_dual = 9999.0

    def next_x(self):
        T = self.T
        rhs = (self.XY - self.adj_y).astype(T)
        rhs = (rhs.astype(np.float64) + self.rho * self.adj_z.astype(np.float64)).astype(T)
        return sla.cho_solve(self.chol, rhs, check_finite=False).astype(T)

    def next_z(self):
        T = self.T
        vec = (self.main_x + self.adj_y / T(self.rho)).astype(T)
        return group_prox(vec, self.sizes, self.weights, self.lam, self.rho, T)[0]


def grp_path(x, y, sizes, weights=None, lam=None, nlambda=10, lmin_ratio=0.01, standardize=True, intercept=True,
             maxit=10000, eps=1e-5, rho=-1.0, T=F):
    """The lambda path as admm_hip_grplasso runs it (the driver of oracle/entry.py _lasso_family with the group solver).
    Returns a dict: lambda, lam_int, beta ((p + 1) x nlambda, original scale), beta_std (p x nlambda, the solver's z), niter, and
    the standardised data Xs, Ys with the solver."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, p = x.shape
    Xs = np.array(x, dtype=T, order="F")
    Ys = np.array(y, dtype=T)
    std = DataStd(n, p, standardize, intercept, T)
    std.standardize(Xs, Ys)
    solver = GroupLassoTall(Xs, Ys, eps, eps, sizes, weights, T)
    if lam is None:
        lmax = np.float64(solver.lambda0) / n * np.float64(std.scaleY)
        lam = np.exp(np.linspace(np.log(lmax), np.log(lmin_ratio * lmax), int(nlambda)))
    lam = np.atleast_1d(np.asarray(lam, dtype=np.float64))
    nl = lam.size
    beta = np.zeros((p + 1, nl), dtype=T)
    beta_std = np.zeros((p, nl), dtype=T)
    niter = np.zeros(nl, dtype=np.int32)
    lam_int = lam * n / np.float64(std.scaleY)
    for i in range(nl):
        solver.lam_idx = i
        if i == 0:
            solver.init(lam_int[i], rho)
        else:
            solver.init_warm(lam_int[i])
        niter[i] = solver.solve(maxit)
        beta_std[:, i] = solver.get_coef()
        b0, coef = std.recover(solver.get_coef())
        beta[0, i] = b0
        beta[1:, i] = coef
    return dict(lam=lam, lam_int=lam_int, beta=beta, beta_std=beta_std, niter=niter, Xs=Xs, Ys=Ys, std=std, solver=solver)


def to_standardised(beta, std):
    """Coefficients on the original scale ((p + 1) x nlambda, row 0 the intercept) back into the solver's units."""
    b = np.asarray(beta, dtype=np.float64)[1:]
    return b * np.asarray(std.scaleX, dtype=np.float64)[:, None] / np.float64(std.scaleY)


def group_kkt(Xs, Ys, beta_std, lam_int, sizes, weights):
    """Group KKT figures per lambda, in the standardised space, in double.  With g = X_s'(y_s - X_s b):
      viol = max over penalised groups of ||g_g|| / (lambda w_g);
      on   = max over active penalised groups of ||g_g - lambda w_g b_g / ||b_g|| || / (lambda w_g);
      unp  = max over unpenalised groups of ||g_g|| / lambda_int[0].
    Returns three arrays of length nlambda (0 where a class of groups is empty)."""
    X = np.asarray(Xs, dtype=np.float64)
    Y = np.asarray(Ys, dtype=np.float64)
    B = np.asarray(beta_std, dtype=np.float64)
    st = group_starts(sizes)
    w = np.asarray(weights, dtype=np.float64)
    nl = B.shape[1]
    viol, on, unp = np.zeros(nl), np.zeros(nl), np.zeros(nl)
    for l in range(nl):
        g = X.T @ (Y - X @ B[:, l])
        for k in range(len(w)):
            gg, bg = g[st[k]:st[k + 1]], B[st[k]:st[k + 1], l]
            if w[k] > 0:
                lw = lam_int[l] * w[k]
                viol[l] = max(viol[l], np.linalg.norm(gg) / lw)
                nb = np.linalg.norm(bg)
                if nb > 0:
                    on[l] = max(on[l], np.linalg.norm(gg - lw * bg / nb) / lw)
            else:
                unp[l] = max(unp[l], np.linalg.norm(gg) / lam_int[0])
    return viol, on, unp


def kkt_maxima(viol, on, unp, lam):
    """Path-wide maxima of (viol - 1) ratio, on ratio and unp, with ratio = lambda / lambda[0]."""
    ratio = np.asarray(lam) / lam[0]
    return float(np.max((viol - 1.0) * ratio)), float(np.max(on * ratio)), float(np.max(unp))


# ---- the two shapes of the tests
S1_SIZES = [1, 2, 31, 32, 33, 1, 1, 70, 5, 4, 3, 8, 8, 8, 16, 7]          # p = 230: straddles, exactly 32, 33, 70 (multi-pass), singletons


def s2_sizes():
    """p = 2100 (symmetric x-update, p >= 2048): the S1 pattern repeated, one group of 200, a tail of singletons."""
    sizes = S1_SIZES * 8 + [200]
    return sizes + [1] * (2100 - sum(sizes))


def synth_groups(n, sizes, seed, nactive=4, sd_noise=2.0):
    """Gaussian columns with a shared within-group component, a few active groups, noise sd 2."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes)
    p = int(sizes.sum())
    gid = np.repeat(np.arange(sizes.size), sizes)
    shared = rng.standard_normal((n, sizes.size))
    x = rng.standard_normal((n, p)) + 0.6 * shared[:, gid]
    b = np.zeros(p)
    big = np.nonzero(sizes > 1)[0]
    act = rng.choice(big, size=min(nactive, big.size), replace=False)
    for g in act:
        b[gid == g] = rng.standard_normal(int(sizes[g])) / np.sqrt(sizes[g])
    y = x @ b + sd_noise * rng.standard_normal(n)
    return x, y
