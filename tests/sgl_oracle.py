"""NumPy restatement of the sparse-group lasso of admm_hip_sgl (TEST INFRASTRUCTURE): tests/group_oracle.py's solver (imported, not
edited) with the z-update replaced by the two-level prox and lambda_0 by the root of the group's emptiness condition, found here by
plain bisection -- independent of the library's closed form over the breakpoints -- plus a path driver and the KKT figures.

In the solver's internal units the problem is
    minimise 1/2 ||y_s - X_s b||^2 + lambda_int [ alpha sum_j u_j |b_j| + (1 - alpha) sum_g w_g ||b_g||_2 ] .
Three weights, in double, as the library's host prepares them:  l1_j = alpha u_j,  wg_g = (1 - alpha) w_g,  ws_j = l1_j + wg_g.
next_z, with v = x + adj_y / rho (in T); every threshold is lambda * weight / rho in double, in that order:
    size 1:    z = soft(v, lambda ws_j / rho)                       (the Lasso's soft-threshold: double compare, (T)(v -+ pen));
    size > 1:  s_j = soft(v_j, lambda l1_j / rho)  rounded to T,  nrm = sqrt(sum (double) s_j^2),  pen = lambda wg_g / rho,
               shrink = nrm > pen ? 1 - pen / nrm : 0,  z_j = (T)((double) s_j shrink)."""
import numpy as np

from oracle.datastd import DataStd
from oracle.solvers import _soft_d

import group_oracle as go

F = np.float32


def sgl_weights(sizes, alpha, u=None, w=None):
    """(l1 [p], wg [ngroups], ws [p]) from the caller's u (None: ones) and w (None: sqrt(size))."""
    sizes = np.asarray(sizes, dtype=np.int64)
    p = int(sizes.sum())
    alpha = np.float64(alpha)
    u = np.ones(p) if u is None else np.asarray(u, dtype=np.float64)
    w = go.default_weights(sizes) if w is None else np.asarray(w, dtype=np.float64)
    l1 = alpha * u
    wg = (np.float64(1.0) - alpha) * w
    ws = l1 + np.repeat(wg, sizes)
    return l1, wg, ws


def sgl_prox(vec, sizes, l1, wg, lam, rho, T=F):
    """next_z on v = vec (dtype T).  Returns (z, s, nrm, pen): s the element-wise thresholded vector (v itself in one-column groups),
    nrm the groups' norms of s in double and pen their block thresholds."""
    sizes = np.asarray(sizes, dtype=np.int64)
    st = go.group_starts(sizes)
    gid = np.repeat(np.arange(sizes.size), sizes)
    single = (sizes == 1)[gid]
    lam, rho = np.float64(lam), np.float64(rho)
    l1 = np.asarray(l1, dtype=np.float64)
    wg = np.asarray(wg, dtype=np.float64)
    s = _soft_d(vec, lam * l1 / rho, T)
    s[single] = vec[single]
    pen = lam * wg / rho
    sd = s.astype(np.float64)
    nrm = np.sqrt(np.add.reduceat(sd * sd, st[:-1]))
    with np.errstate(divide="ignore", invalid="ignore"):
        shrink = np.where(nrm > pen, 1.0 - pen / nrm, 0.0)
    z = (sd * shrink[gid]).astype(T)
    if single.any():
        ws = l1 + wg[gid]
        z[single] = _soft_d(vec[single], lam * ws[single] / rho, T)
    return z, s, nrm, pen


def _group_lambda(c, a, b):
    """The smallest lambda with f(lambda) = sum max(|c_j| - lambda a_j, 0)^2 - (b lambda)^2 <= 0, by bisection down to adjacent
    doubles; None for a group that no lambda empties."""
    c = np.abs(np.asarray(c, dtype=np.float64))
    if not np.any(c > 0):
        return 0.0
    live = c > 0
    if b > 0:
        hi = float(np.sqrt(np.sum(c * c)) / b) * (1.0 + 1e-12)      # f <= 0 there even without the l1 part
    else:
        if np.any(a[live] == 0):
            return None
        hi = float(np.max(c[live] / a[live])) * (1.0 + 1e-12)

    def f(lam):
        r = np.maximum(c - lam * a, 0.0)
        return float(np.sum(r * r) - (b * lam) ** 2)

    lo = 0.0
    assert f(hi) <= 0
    while True:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            return hi
        if f(mid) <= 0:
            hi = mid
        else:
            lo = mid


def sgl_lambda0(xy, sizes, l1, wg):
    """max_g lambda_g as a double (the library rounds it to float)."""
    st = go.group_starts(sizes)
    xy = np.asarray(xy, dtype=np.float64)
    best = 0.0
    for g in range(len(sizes)):
        lg = _group_lambda(xy[st[g]:st[g + 1]], np.asarray(l1, dtype=np.float64)[st[g]:st[g + 1]], float(wg[g]))
        if lg is not None:
            best = max(best, lg)
    return best


class SGLTall(go.GroupLassoTall):
    """GroupLassoTall with the two-level prox and its lambda_0."""

    def __init__(self, X, Y, eps_abs, eps_rel, sizes, alpha, u=None, w=None, T=F):
        super().__init__(X, Y, eps_abs, eps_rel, sizes, None, T)
        self.l1, self.wg, self.ws = sgl_weights(sizes, alpha, u, w)
        self.weights = None                                           # (the parent's single weight vector has no meaning here)
        self.lambda0 = T(sgl_lambda0(self.XY, self.sizes, self.l1, self.wg))

    def next_z(self):
        T = self.T
        vec = (self.main_x + self.adj_y / T(self.rho)).astype(T)
        return sgl_prox(vec, self.sizes, self.l1, self.wg, self.lam, self.rho, T)[0]


def sgl_path(x, y, sizes, alpha, u=None, w=None, lam=None, nlambda=10, lmin_ratio=0.01, standardize=True, intercept=True,
             maxit=10000, eps=1e-5, rho=-1.0, T=F):
    """The lambda path as admm_hip_sgl runs it (group_oracle.grp_path's driver with the sparse-group solver); same dict."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, p = x.shape
    Xs = np.array(x, dtype=T, order="F")
    Ys = np.array(y, dtype=T)
    std = DataStd(n, p, standardize, intercept, T)
    std.standardize(Xs, Ys)
    solver = SGLTall(Xs, Ys, eps, eps, sizes, alpha, u, w, T)
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


def sgl_kkt(Xs, Ys, beta_std, lam_int, sizes, l1, wg):
    """KKT figures per lambda, in the standardised space, in double.  With g = X_s'(y_s - X_s b) and S the soft-threshold:
      off = over the groups with b_g = 0, the largest max(||S(g_g, lambda l1)|| - lambda wg_g, 0) / lambda;
      on  = over the active groups, with r = g_g - lambda wg_g b_g / ||b_g||, the largest of |r_j - lambda l1_j sign(b_j)| over b_j != 0
            and max(|r_j| - lambda l1_j, 0) over b_j = 0, divided by lambda;
      unp = over the groups that hold unpenalised coordinates (l1_j = 0 and wg_g = 0), the largest norm of g over those coordinates
            divided by lambda_int[0] (group_oracle.group_kkt's unp; such coordinates are left out of off and on).
    Returns three arrays of length nlambda (0 where a class is empty)."""
    X = np.asarray(Xs, dtype=np.float64)
    Y = np.asarray(Ys, dtype=np.float64)
    B = np.asarray(beta_std, dtype=np.float64)
    st = go.group_starts(sizes)
    l1 = np.asarray(l1, dtype=np.float64)
    wg = np.asarray(wg, dtype=np.float64)
    nl = B.shape[1]
    off, on, unp = np.zeros(nl), np.zeros(nl), np.zeros(nl)
    for l in range(nl):
        lam = lam_int[l]
        g = X.T @ (Y - X @ B[:, l])
        for k in range(len(wg)):
            gg, bg, a = g[st[k]:st[k + 1]], B[st[k]:st[k + 1], l], l1[st[k]:st[k + 1]]
            free = (a == 0) & (wg[k] == 0)
            if free.any():
                unp[l] = max(unp[l], np.linalg.norm(gg[free]) / lam_int[0])
            gg, bg, a = gg[~free], bg[~free], a[~free]
            if gg.size == 0:
                continue
            nb = np.linalg.norm(bg)
            if nb == 0:
                sg = np.sign(gg) * np.maximum(np.abs(gg) - lam * a, 0.0)
                off[l] = max(off[l], max(np.linalg.norm(sg) - lam * wg[k], 0.0) / lam)
            else:
                r = gg - lam * wg[k] * bg / nb
                nz = bg != 0
                fig = 0.0
                if nz.any():
                    fig = max(fig, np.max(np.abs(r[nz] - lam * a[nz] * np.sign(bg[nz]))))
                if (~nz).any():
                    fig = max(fig, np.max(np.maximum(np.abs(r[~nz]) - lam * a[~nz], 0.0)))
                on[l] = max(on[l], fig / lam)
    return off, on, unp


def sgl_kkt_maxima(off, on, unp, lam):
    """Path-wide maxima of off ratio, on ratio and unp, with ratio = lambda / lambda[0] (unp is already taken against lambda[0])."""
    ratio = np.asarray(lam) / lam[0]
    return float(np.max(off * ratio)), float(np.max(on * ratio)), float(np.max(unp))


def mixed_groups(beta_col, sizes):
    """Indices of the multi-column groups that hold zero and non-zero coefficients side by side."""
    st = go.group_starts(sizes)
    out = []
    for k in range(len(sizes)):
        nz = np.asarray(beta_col[st[k]:st[k + 1]]) != 0
        if sizes[k] > 1 and nz.any() and not nz.all():
            out.append(k)
    return out


def active_groups(beta_col, sizes):
    st = go.group_starts(sizes)
    return sum(bool(np.any(np.asarray(beta_col[st[k]:st[k + 1]]) != 0)) for k in range(len(sizes)))
