"""Helper of the elastic-net logistic tests (tests/test_logit_enet_host.py, tests/test_gpu_logit_enet.py): the CPU restatement of
admm_hip_logit_enet on the oracle's LAD class, the penalised objective, lambda_1, a float64 reference optimum that asserts its own KKT
conditions, and the replay of an iterate dump of the augmented loop.

The fit, per label column and cell (lambda, alpha):
    minimise  sum_i log(1 + exp(-s_i (b0 + x~_i'b))) + lambda (alpha sum_j |b_j| + (1 - alpha) / 2 sum_j b_j^2),  s = 2 y - 1,
on the standardised columns x~, the intercept not penalised.  It is logit_ridge_oracle's restatement with the penalty's constants moved
from the rows into the prox: the p penalty rows are c e_j' with c = sqrt(n) for EVERY cell (n: the data rows; a standardised column has
squared norm n), z_{n + j} = c b_j, and their loss is c_hi |z| + c_lo z^2 / 2 with c_hi = lambda alpha / c, c_lo = lambda (1 - alpha) /
c^2.  The Gram matrix of the augmented matrix is X'X + n D whatever lambda, alpha and rho are.  A row of sign 0 takes
    t = c_hi / rho,  d = 1 + c_lo / rho,  z = soft(v, t) / d
in this association.  Returned: b_j = z_{n + j} / c of the LAST z (exact zeros), the intercept from get_coef."""
import numpy as np

import logit_oracle as lo
import logit_ridge_oracle as lr
from oracle.entry import _attach
from quantile_oracle import strip_cold


def enet_prox(v, rho, c_hi, c_lo):
    t = c_hi / rho
    d = 1.0 + c_lo / rho
    return np.where(v > t, v - t, np.where(v < -t, v + t, 0.0)) / d


def constants(lam, alpha, n):
    """-> (c_hi, c_lo) of a cell, formed as the library forms them"""
    c2 = float(n)
    c = np.sqrt(c2)
    return float(lam) * float(alpha) / c, float(lam) * (1.0 - float(alpha)) / c2


class LogitEnet(lr.LogitRidge):
    """LogitRidge with the elastic net's prox where sign == 0."""

    def __init__(self, X, signs, rho, eps_abs, eps_rel, c_hi, c_lo):
        lr.LogitRidge.__init__(self, X, signs, rho, eps_abs, eps_rel)
        self.c_hi, self.c_lo = c_hi, c_lo

    def next_z(self):
        v = self.main_x - self.Y + self.adj_y / self.rho
        z = enet_prox(v, self.rho, self.c_hi, self.c_lo)
        s = self.signs[self.logistic]
        z[self.logistic] = s * lo.prox(s * v[self.logistic], self.rho)
        return z


def augmented(x, intercept):
    """-> ([X_std | 1] with the p rows sqrt(n) e_j' behind it, the DataStd of x): one matrix for every cell"""
    return lr.augmented(x, float(np.asarray(x).shape[0]), intercept)


def logit_enet(x, Y, lam, alpha, intercept, opts, details=None):
    """The restatement of admm_hip_logit_enet: per cell (lam[l], alpha[l]), in the order given, and label column one cold LogitEnet loop
    on the one augmented matrix.  details: None, or details[l][c] a dict as oracle.entry's `detail`.
    -> {"beta": (p + 1) x k x ncell, "niter": k x ncell}"""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    lam = np.atleast_1d(np.asarray(lam, dtype=np.float64))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), lam.shape)
    n, p = np.asarray(x).shape
    k = Y.shape[1]
    c = np.sqrt(float(n))
    X, std = augmented(x, intercept)
    beta = np.zeros((p + 1, k, lam.size))
    niter = np.zeros((k, lam.size), dtype=np.int64)
    for l in range(lam.size):
        c_hi, c_lo = constants(lam[l], alpha[l], n)
        for col in range(k):
            solver = LogitEnet(X, lr.signs_of(Y[:, col], p), float(opts["rho"]), float(opts["eps_abs"]), float(opts["eps_rel"]), c_hi, c_lo)
            d = None if details is None else details[l][col]
            _attach(solver, d)
            niter[col, l] = solver.solve(int(opts["maxit"]))
            b = solver.get_coef()
            b[:p] = solver.aux_z[n:] / c
            beta[:, col, l] = lo.recover(std, b, p, intercept)
            if d is not None:
                d.update(solver=solver, std=std, dense=solver.get_coef())
    return {"beta": beta, "niter": niter}


def objective(x_std, y, b0, b, lam, alpha):
    """sum log(1 + exp(-s (b0 + x~'b))) + lam (alpha |b|_1 + (1 - alpha) / 2 |b|^2) on the standardised scale, stable for any margin."""
    m = (2.0 * np.asarray(y, dtype=np.float64) - 1.0) * (x_std @ b + b0)
    return float(np.sum(np.maximum(-m, 0.0) + np.log1p(np.exp(-np.abs(m))))
                 + float(lam) * (float(alpha) * float(np.abs(b).sum()) + 0.5 * (1.0 - float(alpha)) * float(b @ b)))


def objective_of(x, y, beta, lam, alpha, intercept):
    """`objective` of caller-scale coefficients."""
    xs, std = lr.standardized_design(x, intercept)
    b0, b = lr.to_std(std, np.asarray(beta, dtype=np.float64), intercept)
    return objective(xs, y, b0, b, lam, alpha)


def lambda_one(x, Y, intercept):
    """-> (k,) max_j |x~_j'(y_c - mean(y_c))| with the intercept, |x~_j'(y_c - 1/2)| without: from lambda_1 / alpha on the optimum has b = 0"""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    xs, _ = lr.standardized_design(x, intercept)
    r = Y - (Y.mean(axis=0)[None, :] if intercept else 0.5)
    return np.max(np.abs(xs.T @ r), axis=0)


def _kkt(A, B, D, b, lam, alpha):
    """-> (the worst violation, the scale it is measured against) of the optimality conditions at b: with g the gradient of the
    likelihood, |g_j + lam (1 - alpha) b_j| <= lam alpha where b_j = 0, g_j + lam (1 - alpha) b_j + lam alpha sign(b_j) = 0 elsewhere,
    g = 0 for the intercept"""
    q = lo._sigma_neg(B @ b)
    g = -(B.T @ q) + lam * (1.0 - alpha) * D * b
    pen = D > 0
    zero = pen & (b == 0.0)
    viol = np.where(zero, np.maximum(np.abs(g) - lam * alpha, 0.0), np.abs(g + lam * alpha * D * np.sign(b)))
    scale = max(float(np.max(np.abs(B).T @ q + lam * (1.0 - alpha) * D * np.abs(b))), lam * alpha, 1.0)
    return float(np.max(viol)), scale


def enet_optimum(x_std, y, lam, alpha, intercept, maxit=400000):
    """Float64 reference optimum: FISTA with restart on the smooth part (likelihood + ridge term) and the soft threshold, and every
    `every` iterations a Newton polish of the smooth problem on the current support with its signs held (the l1 term is linear there);
    a polished point is accepted only when it keeps those signs and satisfies the KKT conditions of the WHOLE problem to 1e-9 of scale,
    which is asserted.  -> (b0, b on the standardised scale, optimum)"""
    lam, alpha = float(lam), float(alpha)
    s = 2.0 * np.asarray(y, dtype=np.float64) - 1.0
    n, p = x_std.shape
    A = np.hstack([np.ones((n, 1)), x_std]) if intercept else x_std
    B = A * s[:, None]
    D = np.concatenate([[0.0], np.ones(p)]) if intercept else np.ones(p)
    pen = D > 0
    L = 0.25 * float(np.linalg.norm(A, 2)) ** 2 + lam * (1.0 - alpha)

    def smooth_grad(b):
        return -(B.T @ lo._sigma_neg(B @ b)) + lam * (1.0 - alpha) * D * b

    def full(b):
        m = B @ b
        return float(np.sum(np.maximum(-m, 0.0) + np.log1p(np.exp(-np.abs(m)))) + lam * (alpha * float(np.abs(D * b).sum()) + 0.5 * (1.0 - alpha) * float((D * b) @ b)))

    def polish(b):
        S = ~pen | (b != 0.0)
        sg = np.sign(b[S]) * D[S]
        AS, BS, DS = A[:, S], B[:, S], D[S]
        u = b[S].copy()

        def h(w):
            m = BS @ w
            return float(np.sum(np.maximum(-m, 0.0) + np.log1p(np.exp(-np.abs(m)))) + 0.5 * lam * (1.0 - alpha) * float((DS * w) @ w) + lam * alpha * float(sg @ w))

        for _ in range(60):
            q = lo._sigma_neg(BS @ u)
            g = -(BS.T @ q) + lam * (1.0 - alpha) * DS * u + lam * alpha * sg
            H = (AS * (q * (1.0 - q))[:, None]).T @ AS + lam * (1.0 - alpha) * np.diag(DS)
            try:
                step = np.linalg.solve(H, -g)
            except np.linalg.LinAlgError:
                return None
            a, h0 = 1.0, h(u)
            while h(u + a * step) > h0 and a > 1e-10:
                a *= 0.5
            un = u + a * step
            moved = float(np.max(np.abs(un - u)) / max(float(np.max(np.abs(un))), 1e-300))
            u = un
            if moved < 1e-14:
                break
        if np.any(np.sign(u) * DS != sg):
            return None
        out = np.zeros_like(b)
        out[S] = u
        return out

    b = np.zeros(A.shape[1])
    w, tk, every = b.copy(), 1.0, 500
    thr = lam * alpha / L
    for it in range(1, maxit + 1):
        v = w - smooth_grad(w) / L
        bn = np.where(pen, np.sign(v) * np.maximum(np.abs(v) - thr, 0.0), v)
        if float((w - bn) @ (bn - b)) > 0.0:                       # gradient restart
            tk, w = 1.0, bn.copy()
        else:
            tn = 0.5 + 0.5 * np.sqrt(1.0 + 4.0 * tk * tk)
            w = bn + ((tk - 1.0) / tn) * (bn - b)
            tk = tn
        b = bn
        if it % every == 0:
            cand = polish(b)
            if cand is not None:
                viol, scale = _kkt(A, B, D, cand, lam, alpha)
                if viol <= 1e-9 * scale:
                    b = cand
                    break
    viol, scale = _kkt(A, B, D, b, lam, alpha)
    assert viol <= 1e-9 * scale, ("the elastic-net reference optimum misses its KKT conditions", viol, scale, lam, alpha)
    b0, bb = (float(b[0]), b[1:]) if intercept else (0.0, b)
    best = objective(x_std, y, b0, bb, lam, alpha)
    assert abs(best - full(b)) <= 1e-12 * max(1.0, abs(best))
    return b0, bb, best


def followed(fit_beta, fit_niter, trace, x, y, lam, alpha, intercept, opts, tol=1e-8, band=8.0, label=""):
    """The restatement follows the library's decision trace (oracle.solvers.FADMM follow mode): niter identical, beta within tol, and
    the zero pattern of the penalised coefficients identical wherever the restatement's |z| is not within tol of its threshold's edge
    (reported, not excused: a differing zero is counted in the error, being a coefficient the other side does not have)."""
    t = strip_cold(trace)
    d = {"follow": t, "follow_band": band}
    ref = logit_enet(x, y, lam, alpha, intercept, opts, [[d]])
    beta = ref["beta"][:, 0, 0]
    assert d["solver"].ndecisions == len(t), (label, d["solver"].ndecisions, len(t))
    assert int(fit_niter) == int(ref["niter"][0, 0]), (label, fit_niter, ref["niter"])
    err = float(np.max(np.abs(np.asarray(fit_beta) - beta)) / max(np.max(np.abs(beta)), 1e-300))
    zeros = int(np.sum((np.asarray(fit_beta)[1:] == 0.0) != (beta[1:] == 0.0)))
    print(f"[logit enet {label}] {len(t)} decisions, {len(d['forced'])} near-ties taken from the library; niter identical ({int(fit_niter)}); beta err {err:.2e}; "
          f"{zeros} zeros differ")
    assert err < tol, (label, err)
    return dict(forced=d["forced"], err=err, beta=beta, zeros=zeros)


def replay(trace, state, y, p, lam, alpha, label=""):
    """Every record of the iterate dump of the augmented loop (x | z | y | adj_z | adj_y, n + p entries each).  Record 0 carries the zero
    response in its x slot and the signs the loop ran with in its z slot: [2 y - 1, 0 ... 0] exactly.  For every iteration k >= 1, from
    its x, adj_y and the rho the trace says it ran with (trace[k - 1][10]): on the logistic rows z recomputed within
    logit_oracle.prox_tol of the dumped one; on the penalty rows within 4 ulp of soft(v, t) / d in the stated association, and an entry
    the restatement makes exactly 0 exactly 0; y = adj_y + rho (x - z_dump) bit for bit from the DUMPED z."""
    t = np.asarray(trace, dtype=np.float64)
    s = np.asarray(state, dtype=np.float64)
    n = len(y)
    assert s.ndim == 3 and s.shape[1] == 5 and s.shape[2] == n + p and len(s) >= 2, (label, s.shape)
    d = s[0, 0]
    assert not np.any(d) and not np.any(s[0, 2:]), label
    sg = lr.signs_of(y, p)
    assert np.array_equal(s[0, 1], sg), label
    c_hi, c_lo = constants(lam, alpha, n)
    nrec = min(len(s), len(t))
    bad, worst, worst_ulp, nzero = [], 0.0, 0.0, 0
    for k in range(1, nrec):
        rho = t[k - 1, 10]
        x, z, yv, adjy = s[k, 0], s[k, 1], s[k, 2], s[k, 4]
        v = x - d + adjy / rho
        z2 = sg[:n] * lo.prox(sg[:n] * v[:n], rho)
        rel = float(np.max(np.abs(z2 - z[:n]) / lo.prox_tol(v[:n], rho)))
        zr = enet_prox(v[n:], rho, c_hi, c_lo)
        ulps = float(np.max(np.abs(zr - z[n:]) / np.spacing(np.maximum(np.abs(zr), np.finfo(np.float64).tiny))))
        zeros_kept = bool(np.all(z[n:][zr == 0.0] == 0.0))
        nzero += int(np.sum(zr == 0.0))
        worst, worst_ulp = max(worst, rel), max(worst_ulp, ulps)
        y2 = adjy + rho * (x - d - z)
        if rel > 1.0 or ulps > 4.0 or not zeros_kept or not np.array_equal(y2, yv) or not np.all(np.isfinite(z)):
            bad.append((k, rel, ulps, zeros_kept, int(np.sum(y2 != yv))))
    print(f"[logit enet replay {label}] {nrec - 1} iterations replayed: {len(bad)} off; worst |z - z_dump| = {worst:.2e} of the tolerance "
          f"(logistic rows), {worst_ulp:.1f} ulp (penalty rows, {nzero} exact zeros)")
    assert not bad, (label, bad[:5])
    return nrec - 1
