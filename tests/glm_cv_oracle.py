"""Helper of the cross-validation tests of the penalised GLMs (tests/test_glm_cv_host.py, tests/test_gpu_glm_cv.py): the masked
restatement of admm_hip_logit_enet_cv / admm_hip_poisson_cv on the oracle's LogitEnet / PoisEnet classes, the replay of an iterate dump
with held-out rows, the NumPy deviance and the summary tables with the one-standard-error rule.

A fold's fit runs on the FULL augmented matrix: the rows of the fold carry a tag of their own in the loop's "sign" vector (2.0 among the
signs, -2.0 among the counts) and take z = v, the prox of the zero function.  Their duals are y = adj_y + rho (x - z) = adj_y - rho
(adj_y / rho): zero up to rounding after the first iteration, so the rows leave the residuals and the fit is the training rows' problem
-- with the FULL data's standardisation and c^2 = n, so lambda means what it means in the full-data fit.  The stop thresholds are the
training rows' too: the held-out rows stay out of the norms that scale them and out of their sqrt(rows) (_LiveRows)."""
import numpy as np

import logit_enet_oracle as le
import logit_oracle as lo
import logit_ridge_oracle as lr
import poisson_oracle as po
from oracle.entry import _attach
from quantile_oracle import strip_cold

HELD = {"logit": 2.0, "poisson": -2.0}


def fold_ids(n, nfolds, fold_id=None):
    return np.arange(n) % nfolds if fold_id is None else np.asarray(fold_id)


def tags_of(loss, y, p, held):
    """the loop's tag vector: signs_of / counts_of with the held-out marker on the rows of the boolean mask `held` (n entries)"""
    t = lr.signs_of(y, p) if loss == "logit" else po.counts_of(y, p)
    t[:len(y)][np.asarray(held, dtype=bool)] = HELD[loss]
    return t


class _LiveRows:
    """The stop thresholds of a fold's loop: a held-out row is no row of the fold's problem, so it stays out of ||x||, ||z||, ||y|| and
    out of sqrt(rows).  The residuals keep every row."""

    def _live(self, v):
        w = v.copy()
        w[self.held] = 0.0
        return w

    def compute_eps_primal(self):
        r = max(np.linalg.norm(self._live(self.main_x)), np.linalg.norm(self._live(self.aux_z)), self.ynorm)
        return r * self.eps_rel + np.sqrt(float(self.n - int(self.held.sum()))) * self.eps_abs

    def compute_eps_dual(self):
        return np.linalg.norm(self._live(self.dual_y)) * self.eps_rel + np.sqrt(float(self.n - int(self.held.sum()))) * self.eps_abs


class MaskedLogitEnet(_LiveRows, le.LogitEnet):
    """LogitEnet in which a row tagged 2.0 takes z = v."""

    def __init__(self, X, tags, rho, eps_abs, eps_rel, c_hi, c_lo):
        le.LogitEnet.__init__(self, X, tags, rho, eps_abs, eps_rel, c_hi, c_lo)
        self.held = tags == HELD["logit"]
        self.logistic = (tags != 0.0) & ~self.held

    def next_z(self):
        z = le.LogitEnet.next_z(self)
        v = self.main_x - self.Y + self.adj_y / self.rho
        z[self.held] = v[self.held]
        return z


class MaskedPoisEnet(_LiveRows, po.PoisEnet):
    """PoisEnet in which a row tagged -2.0 takes z = v."""

    def __init__(self, X, tags, rho, eps_abs, eps_rel, c_hi, c_lo):
        po.PoisEnet.__init__(self, X, tags, rho, eps_abs, eps_rel, c_hi, c_lo)
        self.held = tags == HELD["poisson"]

    def next_z(self):
        z = po.PoisEnet.next_z(self)
        v = self.main_x - self.Y + self.adj_y / self.rho
        z[self.held] = v[self.held]
        return z


SOLVER = {"logit": MaskedLogitEnet, "poisson": MaskedPoisEnet}


def masked_fit(loss, x, y, lam, alpha, intercept, opts, held, detail=None):
    """One cold masked loop on the full augmented matrix.  -> {"beta": p + 1 on the caller's scale, "niter", "std"}"""
    n, p = np.asarray(x).shape
    X, std = le.augmented(x, intercept)
    c_hi, c_lo = le.constants(lam, alpha, n)
    solver = SOLVER[loss](X, tags_of(loss, y, p, held), float(opts["rho"]), float(opts["eps_abs"]), float(opts["eps_rel"]), c_hi, c_lo)
    _attach(solver, detail)
    niter = solver.solve(int(opts["maxit"]))
    b = solver.get_coef()
    b[:p] = solver.aux_z[n:] / np.sqrt(float(n))
    if detail is not None:
        detail.update(solver=solver, std=std)
    return {"beta": lo.recover(std, b, p, intercept), "niter": int(niter), "std": std}


def training_optimum(loss, x, y, lam, alpha, intercept, held):
    """-> (b0, b, optimum, x_std of the training rows, y of the training rows): the reference optimum of the TRAINING rows' objective on
    the full data's standardised columns"""
    xs, _ = lr.standardized_design(x, intercept)
    tr = ~np.asarray(held, dtype=bool)
    xt, yt = np.ascontiguousarray(xs[tr]), np.asarray(y, dtype=np.float64)[tr]
    opt = (le.enet_optimum if loss == "logit" else po.poisson_optimum)(xt, yt, lam, alpha, intercept)
    return opt + (xt, yt)


def training_excess(loss, x, beta, lam, alpha, intercept, opt):
    """The sibling tests' excess of caller-scale coefficients on the training rows: objective / optimum - 1 (logit), the share of the
    null model's gap (Poisson)."""
    _, _, best, xt, yt = opt
    _, std = lr.standardized_design(x, intercept)
    b0, b = lr.to_std(std, np.asarray(beta, dtype=np.float64), intercept)
    if loss == "logit":
        return le.objective(xt, yt, b0, b, lam, alpha) / best - 1.0
    return (po.objective(xt, yt, b0, b, lam, alpha) - best) / (po.null_objective(yt, intercept) - best)


def followed(loss, fit_beta, fit_niter, trace, x, y, lam, alpha, intercept, opts, held, tol=1e-8, band=8.0, label=""):
    """The masked restatement follows the library's decision trace: niter identical, beta within tol."""
    t = strip_cold(trace)
    d = {"follow": t, "follow_band": band}
    ref = masked_fit(loss, x, y, lam, alpha, intercept, opts, held, d)
    assert d["solver"].ndecisions == len(t), (label, d["solver"].ndecisions, len(t))
    assert int(fit_niter) == ref["niter"], (label, fit_niter, ref["niter"])
    err = float(np.max(np.abs(np.asarray(fit_beta) - ref["beta"])) / max(np.max(np.abs(ref["beta"])), 1e-300))
    print(f"[glm cv {loss} {label}] {len(t)} decisions, {len(d['forced'])} near-ties taken from the library; niter identical ({int(fit_niter)}); beta err {err:.2e}")
    assert err < tol, (label, err)
    return err


def replay(loss, trace, state, y, p, lam, alpha, held, label=""):
    """The siblings' replay with held-out rows.  Record 0's z slot carries the tags the loop ran with, the marker on exactly the rows of
    `held`.  For every iteration: the training rows' z within the loss's prox_tol, the penalty rows within 4 ulp with exact zeros
    exact, every HELD-OUT row's z equal to v = x + adj_y / rho bit for bit, y = adj_y + rho (x - z_dump) bit for bit."""
    t = np.asarray(trace, dtype=np.float64)
    s = np.asarray(state, dtype=np.float64)
    n = len(y)
    held = np.asarray(held, dtype=bool)
    assert s.ndim == 3 and s.shape[1] == 5 and s.shape[2] == n + p and len(s) >= 2, (label, s.shape)
    d = s[0, 0]
    assert not np.any(d) and not np.any(s[0, 2:]), label
    tg = tags_of(loss, y, p, held)
    assert np.array_equal(s[0, 1], tg), label
    assert np.array_equal(s[0, 1][:n] == HELD[loss], held) and not np.any(s[0, 1][n:] == HELD[loss]), label
    c_hi, c_lo = le.constants(lam, alpha, n)
    tr = np.flatnonzero(~held)
    nrec = min(len(s), len(t))
    bad, worst, worst_ulp = [], 0.0, 0.0
    for k in range(1, nrec):
        rho = t[k - 1, 10]
        x, z, yv, adjy = s[k, 0], s[k, 1], s[k, 2], s[k, 4]
        v = x - d + adjy / rho
        if loss == "logit":
            z2 = tg[tr] * lo.prox(tg[tr] * v[tr], rho)
            rel = float(np.max(np.abs(z2 - z[tr]) / lo.prox_tol(v[tr], rho)))
        else:
            z2 = po.prox(v[tr], tg[tr], rho)
            rel = float(np.max(np.abs(z2 - z[tr]) / po.prox_tol(v[tr], tg[tr], rho)))
        zr = le.enet_prox(v[n:], rho, c_hi, c_lo)
        ulps = float(np.max(np.abs(zr - z[n:]) / np.spacing(np.maximum(np.abs(zr), np.finfo(np.float64).tiny))))
        zeros_kept = bool(np.all(z[n:][zr == 0.0] == 0.0))
        identity = bool(np.array_equal(z[:n][held], v[:n][held]))
        worst, worst_ulp = max(worst, rel), max(worst_ulp, ulps)
        y2 = adjy + rho * (x - d - z)
        if rel > 1.0 or ulps > 4.0 or not zeros_kept or not identity or not np.array_equal(y2, yv) or not np.all(np.isfinite(z)):
            bad.append((k, rel, ulps, zeros_kept, identity, int(np.sum(y2 != yv))))
    print(f"[glm cv {loss} replay {label}] {nrec - 1} iterations replayed: {len(bad)} off; worst |z - z_dump| = {worst:.2e} of the tolerance (training rows), "
          f"{worst_ulp:.1f} ulp (penalty rows), {int(held.sum())} held-out rows z == v")
    assert not bad, (label, bad[:5])
    return nrec - 1


def row_deviance(loss, eta, y):
    """binomial: 2 (max(-s eta, 0) + log1p(exp(-|eta|))), s = 2 y - 1;  Poisson: 2 (y log(y / mu) - (y - mu)), mu = exp(eta), 0 log 0 = 0"""
    eta, y = np.asarray(eta, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if loss == "logit":
        return 2.0 * (np.maximum(-(2.0 * y - 1.0) * eta, 0.0) + np.log1p(np.exp(-np.abs(eta))))
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):          # (non-finite values are returned, not hidden)
        mu = np.exp(eta)
        ylog = np.where(y > 0.0, y * np.log(np.where(y > 0.0, y, 1.0) / mu), 0.0)
        return 2.0 * (ylog - (y - mu))


def fold_deviance(loss, x, Y, fold_beta, fid):
    """fold_beta: F x (p + 1) x k x ncell on the caller's scale -> F x k x ncell: the mean deviance of fold f's rows under fold f's fits"""
    x, Y = np.asarray(x, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    F, _, k, ncell = fold_beta.shape
    out = np.zeros((F, k, ncell))
    for f in range(F):
        rows = np.flatnonzero(fid == f)
        for c in range(k):
            for l in range(ncell):
                b = fold_beta[f, :, c, l]
                out[f, c, l] = row_deviance(loss, b[0] + x[rows] @ b[1:], Y[rows, c]).mean()
    return out


def cv_summary(fold_dev, lam, alpha):
    """fold_dev: F x k x ncell -> (cv_mean, cv_se: k x ncell; idx_min, idx_1se: k).  The unweighted mean over the folds, the sample sd
    over the folds / sqrt(F); the first cell of the smallest mean; among the cells of ITS alpha the largest lambda whose mean is within
    one standard error of the smallest."""
    fold_dev = np.asarray(fold_dev, dtype=np.float64)
    lam, alpha = np.asarray(lam, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    F, k, ncell = fold_dev.shape
    mean = np.zeros((k, ncell))
    for f in range(F):
        mean += fold_dev[f]
    mean /= F
    var = np.zeros((k, ncell))
    for f in range(F):
        var += (fold_dev[f] - mean) ** 2
    se = np.sqrt(var / (F - 1) / F)
    idx_min, idx_1se = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
    for c in range(k):
        i = int(np.argmin(mean[c]))
        best = i
        for l in range(ncell):
            if alpha[l] == alpha[i] and lam[l] > lam[best] and mean[c, l] <= mean[c, i] + se[c, i]:
                best = l
        idx_min[c], idx_1se[c] = i, best
    return mean, se, idx_min, idx_1se
