"""Helper of the ridge logistic tests (tests/test_logit_ridge_host.py, tests/test_gpu_logit_ridge.py): the CPU restatement of
admm_hip_logit_ridge on the oracle's LAD class, the penalised objective, a float64 ridge Newton (IRLS) optimum, and the replay of an
iterate dump of the augmented loop.

The fit, per label column and lambda:  minimise  sum_i log(1 + exp(-s_i (b0 + x~_i'b))) + lambda / 2 sum_j b_j^2,  s = 2 y - 1, on the
standardised columns x~, the intercept not penalised.  The penalty is not written on b (the x-update's matrix would be X'X + (lambda /
rho) D and change with rho): it becomes p more ROWS sqrt(lambda) e_j' behind [X_std | 1], with a zero response and the loss z^2 / 2.  The
Gram matrix of the augmented matrix is X'X + lambda D, D = 1 on the user columns, whatever rho does; the loop is
logit_multi_oracle.LogitS with "signs" [2 y - 1, 0 ... 0], and a row of sign 0 takes the prox of z^2 / (2 rho): v (rho / (1 + rho)),
in this association."""
import numpy as np

import logit_multi_oracle as lm
import logit_oracle as lo
from oracle.entry import _attach
from oracle.solvers import LAD
from quantile_oracle import strip_cold


def square_prox(v, rho):
    return v * (rho / (1.0 + rho))


class LogitRidge(LAD):
    """LAD on the augmented [X_std | 1] with Y = 0: the signed Newton prox where sign != 0, the square loss's prox where sign == 0."""

    def __init__(self, X, signs, rho, eps_abs, eps_rel):
        LAD.__init__(self, X, np.zeros(X.shape[0]), rho, eps_abs, eps_rel)
        self.signs = signs
        self.logistic = signs != 0.0

    def next_z(self):
        v = self.main_x - self.Y + self.adj_y / self.rho
        z = square_prox(v, self.rho)
        s = self.signs[self.logistic]
        z[self.logistic] = s * lo.prox(s * v[self.logistic], self.rho)
        return z


def augmented(x, lam, intercept):
    """-> ([X_std | 1] with the p rows sqrt(lam) e_j' behind it (zero in the ones column), the DataStd of x)."""
    X, std = lm.unfolded(x, intercept)
    p = np.asarray(x).shape[1]
    R = np.zeros((p, X.shape[1]))
    R[np.arange(p), np.arange(p)] = np.sqrt(float(lam))
    return np.asfortranarray(np.vstack([X, R])), std


def signs_of(y, p):
    return np.concatenate([2.0 * np.asarray(y, dtype=np.float64) - 1.0, np.zeros(p)])


def logit_ridge(x, Y, lam, intercept, opts, details=None):
    """The restatement of admm_hip_logit_ridge: per lambda (in the order given) and label column one cold LogitRidge loop.
    details: None, or details[l][c] a dict as oracle.entry's `detail`.  -> {"beta": (p + 1) x k x nlambda, "niter": k x nlambda}"""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    lam = np.atleast_1d(np.asarray(lam, dtype=np.float64))
    p = np.asarray(x).shape[1]
    k = Y.shape[1]
    beta = np.zeros((p + 1, k, lam.size))
    niter = np.zeros((k, lam.size), dtype=np.int64)
    for l, lv in enumerate(lam):
        X, std = augmented(x, lv, intercept)
        for c in range(k):
            solver = LogitRidge(X, signs_of(Y[:, c], p), float(opts["rho"]), float(opts["eps_abs"]), float(opts["eps_rel"]))
            d = None if details is None else details[l][c]
            _attach(solver, d)
            niter[c, l] = solver.solve(int(opts["maxit"]))
            b = solver.get_coef()
            beta[:, c, l] = lo.recover(std, b, p, intercept)
            if d is not None:
                d.update(solver=solver, std=std)
    return {"beta": beta, "niter": niter}


def standardized_design(x, intercept):
    """-> (X_std without the ones column, the DataStd): what `objective` and `ridge_irls` work on."""
    X, std = lm.unfolded(x, intercept)
    return np.ascontiguousarray(X[:, :np.asarray(x).shape[1]]), std


def to_std(std, beta, intercept):
    """The caller-scale coefficients (intercept first) on the standardised scale: b_j = beta_j scaleX_j, b0 = beta_0 + sum beta_j meanX_j."""
    b = beta[1:] * std.scaleX
    b0 = beta[0] + float((beta[1:] * std.meanX).sum()) if intercept else 0.0
    return b0, b


def objective(x_std, y, b0, b, lam):
    """sum log(1 + exp(-s (b0 + x~'b))) + lam / 2 |b|^2 on the standardised scale, stable for any margin."""
    m = (2.0 * np.asarray(y, dtype=np.float64) - 1.0) * (x_std @ b + b0)
    return float(np.sum(np.maximum(-m, 0.0) + np.log1p(np.exp(-np.abs(m)))) + 0.5 * float(lam) * float(b @ b))


def objective_of(x, y, beta, lam, intercept):
    """`objective` of caller-scale coefficients."""
    xs, std = standardized_design(x, intercept)
    b0, b = to_std(std, np.asarray(beta, dtype=np.float64), intercept)
    return objective(xs, y, b0, b, lam)


def ridge_irls(x_std, y, lam, intercept, maxit=200):
    """Float64 Newton with step halving on the strictly convex penalised objective, to a relative step below 1e-13; the gradient is
    checked as logit_oracle.logit_irls checks its own.  -> (b0, b on the standardised scale, optimum, steps)"""
    s = 2.0 * np.asarray(y, dtype=np.float64) - 1.0
    n, p = x_std.shape
    A = np.hstack([np.ones((n, 1)), x_std]) if intercept else x_std
    B = A * s[:, None]
    D = np.concatenate([[0.0], np.ones(p)]) if intercept else np.ones(p)

    def f(b):
        m = B @ b
        return float(np.sum(np.maximum(-m, 0.0) + np.log1p(np.exp(-np.abs(m)))) + 0.5 * lam * float((D * b) @ b))

    b = np.zeros(A.shape[1])
    step, steps = np.inf, 0
    for steps in range(1, maxit + 1):
        q = lo._sigma_neg(B @ b)
        g = -(B.T @ q) + lam * D * b
        H = (A * (q * (1.0 - q))[:, None]).T @ A + lam * np.diag(D)
        dlt = np.linalg.solve(H, -g)
        a, f0 = 1.0, f(b)
        while f(b + a * dlt) > f0 and a > 1e-10:
            a *= 0.5
        bn = b + a * dlt
        step = float(np.max(np.abs(bn - b)) / max(np.max(np.abs(bn)), 1e-300))
        b = bn
        if step < 1e-13:
            break
    assert step < 1e-13, ("ridge IRLS did not settle", step)
    q = lo._sigma_neg(B @ b)
    grad = float(np.max(np.abs(-(B.T @ q) + lam * D * b)))
    scale = float(np.max(np.abs(B).T @ q + lam * D * np.abs(b)))
    assert grad <= 1e-9 * max(scale, 1.0), ("ridge IRLS gradient", grad, scale)
    b0, bb = (b[0], b[1:]) if intercept else (0.0, b)
    return float(b0), bb, objective(x_std, y, b0, bb, lam), steps


def separable_labels(x, seed):
    x = np.asarray(x, dtype=np.float64)
    rng = np.random.default_rng(seed)
    return ((x - 0.3) @ rng.standard_normal(x.shape[1]) > 0).astype(np.float64)


def followed(fit_beta, fit_niter, trace, x, y, lam, intercept, opts, tol=1e-8, band=8.0, label=""):
    """The restatement follows the library's decision trace (oracle.solvers.FADMM follow mode): niter identical, beta within tol."""
    t = strip_cold(trace)
    d = {"follow": t, "follow_band": band}
    ref = logit_ridge(x, y, lam, intercept, opts, [[d]])
    beta = ref["beta"][:, 0, 0]
    assert d["solver"].ndecisions == len(t), (label, d["solver"].ndecisions, len(t))
    assert int(fit_niter) == int(ref["niter"][0, 0]), (label, fit_niter, ref["niter"])
    err = float(np.max(np.abs(np.asarray(fit_beta) - beta)) / max(np.max(np.abs(beta)), 1e-300))
    print(f"[logit ridge {label}] {len(t)} decisions, {len(d['forced'])} near-ties taken from the library; niter identical ({int(fit_niter)}); beta err {err:.2e}")
    assert err < tol, (label, err)
    return dict(forced=d["forced"], err=err, beta=beta)


def replay(trace, state, y, p, label=""):
    """Every record of the iterate dump of the augmented loop (x | z | y | adj_z | adj_y, n + p entries each).  Record 0 carries the zero
    response in its x slot and the signs the loop ran with in its z slot: [2 y - 1, 0 ... 0] exactly.  For every iteration k >= 1, from
    its x, adj_y and the rho the trace says it ran with (trace[k - 1][10]): on the logistic rows z recomputed within
    logit_oracle.prox_tol of the dumped one; on the ridge rows within 4 ulp of v (rho / (1 + rho)); y = adj_y + rho (x - z_dump) bit for
    bit from the DUMPED z."""
    t = np.asarray(trace, dtype=np.float64)
    s = np.asarray(state, dtype=np.float64)
    n = len(y)
    assert s.ndim == 3 and s.shape[1] == 5 and s.shape[2] == n + p and len(s) >= 2, (label, s.shape)
    d = s[0, 0]
    assert not np.any(d) and not np.any(s[0, 2:]), label
    sg = signs_of(y, p)
    assert np.array_equal(s[0, 1], sg), label
    nrec = min(len(s), len(t))
    bad, worst, worst_ulp = [], 0.0, 0.0
    for k in range(1, nrec):
        rho = t[k - 1, 10]
        x, z, yv, adjy = s[k, 0], s[k, 1], s[k, 2], s[k, 4]
        v = x - d + adjy / rho
        z2 = sg[:n] * lo.prox(sg[:n] * v[:n], rho)
        rel = float(np.max(np.abs(z2 - z[:n]) / lo.prox_tol(v[:n], rho)))
        zr = square_prox(v[n:], rho)
        ulps = float(np.max(np.abs(zr - z[n:]) / np.spacing(np.maximum(np.abs(zr), np.finfo(np.float64).tiny))))
        worst, worst_ulp = max(worst, rel), max(worst_ulp, ulps)
        y2 = adjy + rho * (x - d - z)
        if rel > 1.0 or ulps > 4.0 or not np.array_equal(y2, yv) or not np.all(np.isfinite(z)):
            bad.append((k, rel, ulps, int(np.sum(y2 != yv))))
    print(f"[logit ridge replay {label}] {nrec - 1} iterations replayed: {len(bad)} off; worst |z - z_dump| = {worst:.2e} of the tolerance "
          f"(logistic rows), {worst_ulp:.1f} ulp (ridge rows)")
    assert not bad, (label, bad[:5])
    return nrec - 1
