"""NumPy restatement of the box-constrained, weighted elastic net of admm_hip_boxenet (TEST INFRASTRUCTURE): tests/group_oracle.py's
solver (imported, not edited) with the z-update replaced by the per-coordinate prox followed by a clamp and lambda_0 by the box's
rule, plus a path driver, the KKT figure of the bounded problem and a projected coordinate descent that knows nothing of ADMM.

In the solver's internal units (standardised X_s, y_s; lambda_int = lambda n / scaleY) the problem is
    minimise 1/2 ||y_s - X_s b||^2 + lambda_int sum_j u_j [ alpha |b_j| + (1 - alpha)/2 b_j^2 ]   subject to   lo_j <= b_j <= hi_j ,
lo_j <= 0 <= hi_j.  next_z, with v = x + adj_y / rho (in T) and pen_j = lambda u_j / rho (double, in this order):
    alpha None:  z = clamp(soft(v, pen_j))                 (the Lasso's soft-threshold: double compare, (T)(v -+ pen));
    alpha:       thresh = (T)(alpha pen_j), denom = (T)(1 + pen_j (1 - alpha)), z = clamp((v -+ thresh) / denom beyond thresh, else 0),
                 alpha rounded to float first as the library holds it;
    clamp(z) = min(max(z, lo_j), hi_j) in T.
The caller's bounds are on the original coefficient scale; in solver units they are lower_j scaleX_j / scaleY, formed in double and
rounded to T towards the inside of the box."""
import numpy as np

from oracle.datastd import DataStd
from oracle.solvers import _soft_d

import group_oracle as go

F = np.float32


def _alpha_d(alpha):
    return np.float64(F(alpha))


def box_prox(vec, u, lo, hi, lam, rho, alpha=None, T=F):
    """next_z on v = vec (dtype T); u double, lo / hi in T (solver units)."""
    pen = np.float64(lam) * np.asarray(u, dtype=np.float64) / np.float64(rho)
    if alpha is None:
        z = _soft_d(vec, pen, T)
    else:
        a = _alpha_d(alpha)
        thresh = (a * pen).astype(T)
        denom = (1.0 + pen * (1.0 - a)).astype(T)
        v = vec.astype(T)
        z = np.where(v > thresh, (v - thresh) / denom, np.where(v < -thresh, (v + thresh) / denom, T(0))).astype(T)
    return np.minimum(np.maximum(z, np.asarray(lo, dtype=T)), np.asarray(hi, dtype=T)).astype(T)


def round_inwards(lo64, hi64, T=F):
    """Double bounds to T without leaving the box: the lower bound not below, the upper bound not above the double."""
    lo64, hi64 = np.asarray(lo64, dtype=np.float64), np.asarray(hi64, dtype=np.float64)
    if T is np.float64:
        return lo64 + 0.0, hi64 + 0.0
    with np.errstate(over="ignore"):
        lo, hi = lo64.astype(T), hi64.astype(T)
    lo = np.where(lo.astype(np.float64) < lo64, np.nextafter(lo, T(np.inf)), lo).astype(T)
    hi = np.where(hi.astype(np.float64) > hi64, np.nextafter(hi, T(-np.inf)), hi).astype(T)
    return lo + T(0), hi + T(0)


def std_bounds(lower, upper, scaleX, scaleY, p, T=F):
    """The caller's bounds (None: none; scalars broadcast) in solver units, rounded inwards to T."""
    lo = np.full(p, -np.inf) if lower is None else np.broadcast_to(np.asarray(lower, dtype=np.float64), (p,)).copy()
    hi = np.full(p, np.inf) if upper is None else np.broadcast_to(np.asarray(upper, dtype=np.float64), (p,)).copy()
    sx, sy = np.asarray(scaleX, dtype=np.float64), np.float64(scaleY)
    with np.errstate(invalid="ignore"):
        lo_s = np.where(np.isinf(lo), lo, lo * sx / sy)
        hi_s = np.where(np.isinf(hi), hi, hi * sx / sy)
    return round_inwards(lo_s, hi_s, T)


def library_scales(x, y, standardize=True, intercept=True):
    """(scaleX [p], scaleY) as the library's standardisation forms them (float data, sums in double, each statistic rounded to float
    once, the factor 1 / sqrt(n) from a double square root): the restatement of the bounds' conversion needs these floats and no
    entry point returns them.  They differ from DataStd's only in where the sums accumulate."""
    X = np.asarray(x, dtype=np.float64).astype(F)
    Y = np.asarray(y, dtype=np.float64).astype(F)
    n, p = X.shape
    flag = int(bool(standardize)) + 2 * int(bool(intercept))
    if flag == 0:
        return np.ones(p, F), F(1)
    n_invsqrt = F(1.0 / np.sqrt(np.float64(F(n))))

    def scale(cols):
        m = (cols.astype(np.float64).sum(axis=0) / np.float64(n)).astype(F) if flag & 2 else np.zeros(cols.shape[1], F)
        c = (cols - m[None, :]).astype(F).astype(np.float64)
        return (np.sqrt((c * c).sum(axis=0)).astype(F) * n_invsqrt).astype(F)

    sy = scale(Y[:, None])[0]
    return (scale(X) if flag & 1 else np.ones(p, F)), sy


def box_lambda0(xy, u, lo, hi, alpha=None, T=F):
    """lambda_0 of the automatic grid: max over u_j > 0 of max(c_j if hi_j > 0 else 0, -c_j if lo_j < 0 else 0) / u_j in double, rounded
    to T; the elastic net divides by alpha + 1e-4 and rounds again."""
    c = np.asarray(xy).astype(np.float64)
    u = np.asarray(u, dtype=np.float64)
    g = np.maximum(np.where(np.asarray(hi) > 0, c, 0.0), np.where(np.asarray(lo) < 0, -c, 0.0))
    pos = u > 0
    l0 = T(np.max(g[pos] / u[pos]))
    if alpha is not None:
        l0 = T(np.float64(l0) / (_alpha_d(alpha) + 0.0001))
    return l0


class BoxTall(go.GroupLassoTall):
    """GroupLassoTall (every column a group of its own) with the box prox and its lambda_0.  lo, hi: solver units, dtype T."""

    def __init__(self, X, Y, eps_abs, eps_rel, u, lo, hi, alpha=None, T=F):
        p = X.shape[1]
        super().__init__(X, Y, eps_abs, eps_rel, np.ones(p, dtype=np.int64), np.ones(p), T)
        self.u = np.ones(p) if u is None else np.broadcast_to(np.asarray(u, dtype=np.float64), (p,)).copy()
        self.lo, self.hi = np.asarray(lo, dtype=T), np.asarray(hi, dtype=T)
        self.box_alpha = alpha
        self.weights = None                                           # (the parent's group weights have no meaning here)
        self.lambda0 = box_lambda0(self.XY, self.u, self.lo, self.hi, alpha, T)

    def next_z(self):
        T = self.T
        vec = (self.main_x + self.adj_y / T(self.rho)).astype(T)
        return box_prox(vec, self.u, self.lo, self.hi, self.lam, self.rho, self.box_alpha, T)


def box_path(x, y, lower=None, upper=None, u=None, alpha=None, lam=None, nlambda=10, lmin_ratio=0.01, standardize=True, intercept=True,
             maxit=10000, eps=1e-5, rho=-1.0, T=F):
    """The lambda path as admm_hip_boxenet runs it (group_oracle.grp_path's driver with the box solver; the bounds go through this
    driver's own DataStd).  Same dict, plus lo / hi (solver units) and u; beta is clamped to the caller's box as the library's is."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, p = x.shape
    Xs = np.array(x, dtype=T, order="F")
    Ys = np.array(y, dtype=T)
    std = DataStd(n, p, standardize, intercept, T)
    std.standardize(Xs, Ys)
    lo, hi = std_bounds(lower, upper, std.scaleX, std.scaleY, p, T)
    out_lo, out_hi = std_bounds(lower, upper, np.ones(p), 1.0, p, T)      # the caller's own box, rounded inwards
    solver = BoxTall(Xs, Ys, eps, eps, u, lo, hi, alpha, T)
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
        inside = np.minimum(np.maximum(coef, out_lo), out_hi).astype(T)
        if np.any(inside != coef) and std.flag & 2:                    # the intercept of the clamped coefficients
            b0 = T(std.meanY - T((inside * std.meanX).sum(dtype=T)))
        beta[0, i] = b0
        beta[1:, i] = inside
    return dict(lam=lam, lam_int=lam_int, beta=beta, beta_std=beta_std, niter=niter, Xs=Xs, Ys=Ys, std=std, solver=solver,
                lo=lo, hi=hi, u=solver.u)


def box_kkt(Xs, Ys, beta_std, lam_int, u, lo, hi, alpha=None):
    """Violation of the optimality conditions of the bounded problem per lambda, in the standardised space, in double, in units of
    lambda_int[0].  With a = 1 for alpha None, g = X_s'(y_s - X_s b) - lambda u (1 - a) b and t = lambda u a:
      inside the box (lo < b < hi):   |g - t sign(b)| for b != 0,  max(|g| - t, 0) for b = 0;
      at a positive upper bound:      max(t - g, 0)        (g >= t);
      at a negative lower bound:      max(g + t, 0)        (g <= -t);
      at a zero upper bound (lo < 0): max(-t - g, 0)       (g >= -t);
      at a zero lower bound (hi > 0): max(g - t, 0)        (g <= t);
      nothing where lo = hi.
    A coordinate counts as AT a bound when it is within four float spacings of it (coefficients that went to the original scale and
    back in float do not return to the same bits).  Returns an array of length nlambda."""
    X = np.asarray(Xs, dtype=np.float64)
    Y = np.asarray(Ys, dtype=np.float64)
    B = np.asarray(beta_std, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    a = 1.0 if alpha is None else _alpha_d(alpha)
    out = np.zeros(B.shape[1])
    with np.errstate(invalid="ignore"):
        slack_hi = np.where(np.isinf(hi), 0.0, 4.0 * np.spacing(np.abs(np.where(np.isinf(hi), 0.0, hi)).astype(F)).astype(np.float64))
        slack_lo = np.where(np.isinf(lo), 0.0, 4.0 * np.spacing(np.abs(np.where(np.isinf(lo), 0.0, lo)).astype(F)).astype(np.float64))
    for l in range(B.shape[1]):
        b = B[:, l]
        g = X.T @ (Y - X @ b) - lam_int[l] * u * (1.0 - a) * b
        t = lam_int[l] * u * a
        fixed = lo == hi
        at_hi, at_lo = (b >= hi - slack_hi) & ~fixed, (b <= lo + slack_lo) & ~fixed
        inside = ~(fixed | at_hi | at_lo)
        v = np.zeros_like(b)
        nz = inside & (b != 0)
        v[nz] = np.abs(g[nz] - t[nz] * np.sign(b[nz]))
        z = inside & (b == 0)
        v[z] = np.maximum(np.abs(g[z]) - t[z], 0.0)
        k = at_hi & (hi > 0)
        v[k] = np.maximum(t[k] - g[k], 0.0)
        k = at_lo & (lo < 0)
        v[k] = np.maximum(g[k] + t[k], 0.0)
        k = at_hi & (hi == 0)
        v[k] = np.maximum(-t[k] - g[k], 0.0)
        k = at_lo & (lo == 0)
        v[k] = np.maximum(g[k] - t[k], 0.0)
        out[l] = np.max(v) / lam_int[0]
    return out


def box_cd_optimum(Xs, Ys, lam_int, u, lo, hi, alpha=None, sweeps=20000, tol=1e-13):
    """Plain float64 projected coordinate descent on the same objective at one lambda (cold start): coordinate j's exact minimiser
    is clamp(soft(r_j, lambda u_j a) / (G_jj + lambda u_j (1 - a))) with r_j = X_j'(y - X b) + G_jj b_j.  No ADMM, no rho."""
    X = np.asarray(Xs, dtype=np.float64)
    Y = np.asarray(Ys, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    a = 1.0 if alpha is None else _alpha_d(alpha)
    G = X.T @ X
    c = X.T @ Y
    p = X.shape[1]
    b = np.zeros(p)
    grad = c.copy()                                                   # c - G b
    t, d = lam_int * u * a, np.diag(G) + lam_int * u * (1.0 - a)
    for _ in range(sweeps):
        worst = 0.0
        for j in range(p):
            r = grad[j] + G[j, j] * b[j]
            new = min(max(np.sign(r) * max(abs(r) - t[j], 0.0) / d[j], lo[j]), hi[j])
            if new != b[j]:
                grad -= G[:, j] * (new - b[j])
                worst = max(worst, abs(new - b[j]))
                b[j] = new
        if worst <= tol:
            break
    return b


# ---- the data, the pattern and the two shapes of the tests
def synth_box(n, p, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, p)) + 0.5 * rng.standard_normal((n, 1))
    act = rng.choice(p, size=16, replace=False)
    b = np.zeros(p)
    b[act] = np.where(rng.random(16) < 0.5, -1.0, 1.0) * rng.uniform(0.3, 1.2, 16)
    y = x @ b + 2.0 * rng.standard_normal(n) + 3.0
    return x, y


def box_pattern(p):
    """(lower, upper, u): j % 4 == 0 lower 0; 1 upper 0.25; 2 [-0.1, 0.1]; 3 free; j % 37 == 5 excluded; u uniform in [0.5, 2] with two
    unpenalised columns."""
    j = np.arange(p)
    lower, upper = np.full(p, -np.inf), np.full(p, np.inf)
    lower[j % 4 == 0] = 0.0
    upper[j % 4 == 1] = 0.25
    lower[j % 4 == 2], upper[j % 4 == 2] = -0.1, 0.1
    ex = j % 37 == 5
    lower[ex], upper[ex] = 0.0, 0.0
    u = np.random.default_rng(31).uniform(0.5, 2.0, p)
    u[7] = u[20] = 0.0
    return lower, upper, u


B1 = (600, 230, 11)          # gemv tail; the last workgroup holds 6 of 32 coordinates
B2 = (2304, 2100, 11)        # symv tail (p >= 2048)
