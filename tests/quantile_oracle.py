"""Helper of the quantile-regression tests (tests/test_quantreg_host.py, tests/test_gpu_quantreg.py): the CPU restatement of
admm_hip_quantreg on the oracle's LAD class, the quantile linear programme, and the replay of an iterate dump.

The fit:  minimise sum_i rho_tau(y_i - b0 - x_i'b),  rho_tau(r) = tau r (r >= 0), (tau - 1) r (r < 0).  In the ADMM form of ADMMLAD.h
(z = X b - y) the loop uses g(z) = 2 sum rho_tau(-z_i) -- the factor 2 makes tau = 0.5 LAD's ||z||_1 -- whose prox is the asymmetric
soft-threshold with c_hi / rho above and c_lo / rho below, c_hi = 2 (1 - tau), c_lo = 2 tau.  Everything else is oracle.solvers.LAD.
The intercept is FITTED: a column of ones behind the standardised matrix (DataStd flag 3), one more coefficient b_{p+1}, and
beta_0 = (meanY - sum beta_j meanX_j) + scaleY b_{p+1}."""
import numpy as np

from oracle.datastd import DataStd
from oracle.entry import _attach
from oracle.solvers import LAD


def prox(v, rho, tau):
    """z of the iteration: thresholds computed as c_hi / rho and c_lo / rho."""
    hi = (2.0 * (1.0 - tau)) / rho
    lo = (2.0 * tau) / rho
    return np.where(v > hi, v - hi, np.where(v < -lo, v + lo, 0.0))


class QuantReg(LAD):
    def __init__(self, X, Y, rho, eps_abs, eps_rel, tau):
        LAD.__init__(self, X, Y, rho, eps_abs, eps_rel)
        self.tau_q = float(tau)

    def next_z(self):
        return prox(self.main_x - self.Y + self.adj_y / self.rho, self.rho, self.tau_q)


def standardized(x, y, intercept):
    """-> (X as the loop sees it: standardised, with the ones column when the intercept is fitted; y standardised; the DataStd)."""
    x = np.array(x, dtype=np.float64, order="F")
    y = np.array(y, dtype=np.float64)
    n, p = x.shape
    std = DataStd(n, p, True, intercept, np.float64)
    std.standardize(x, y)
    if intercept:
        x = np.asfortranarray(np.hstack([x, np.ones((n, 1))]))
    return x, y, std


def quantreg(x, y, tau, intercept, opts, detail=None):
    """The restatement of admm_hip_quantreg for ONE tau.  detail: as oracle.entry (follow / follow_band / forced / trace / state)."""
    p = np.asarray(x).shape[1]
    X, Y, std = standardized(x, y, intercept)
    solver = QuantReg(X, Y, float(opts["rho"]), float(opts["eps_abs"]), float(opts["eps_rel"]), tau)
    _attach(solver, detail)
    niter = solver.solve(int(opts["maxit"]))
    b = solver.get_coef()
    beta0, coef = std.recover(b[:p])
    if intercept:
        beta0 = beta0 + std.scaleY * b[p]
    if detail is not None:
        detail.update(solver=solver, std=std)
    return {"beta": np.concatenate([[beta0], coef]), "niter": niter}


def check_loss(x, y, beta, tau):
    r = np.asarray(y) - np.asarray(x) @ beta[1:] - beta[0]
    return float(np.sum(np.where(r >= 0, tau * r, (tau - 1.0) * r)))


def neg_fraction(x, y, beta):
    r = np.asarray(y) - np.asarray(x) @ beta[1:] - beta[0]
    return float(np.mean(r < 0))


def quantile_lp(x, y, tau, intercept):
    """min tau 1'u + (1 - tau) 1'v  s.t.  [X 1] b + u - v = y, u, v >= 0 (HiGHS) -> (beta with the intercept first, optimum)."""
    import scipy.sparse as sp
    from scipy.optimize import linprog
    x = np.asarray(x, dtype=np.float64)
    n, p = x.shape
    A0 = np.hstack([x, np.ones((n, 1))]) if intercept else x
    k = A0.shape[1]
    A = sp.hstack([sp.csr_matrix(A0), sp.identity(n), -sp.identity(n)]).tocsc()
    c = np.concatenate([np.zeros(k), tau * np.ones(n), (1.0 - tau) * np.ones(n)])
    res = linprog(c, A_eq=A, b_eq=y, bounds=[(None, None)] * k + [(0, None)] * (2 * n), method="highs")
    assert res.status == 0, res.message
    beta = np.concatenate([[res.x[p] if intercept else 0.0], res.x[:p]])
    return beta, float(res.fun)


def issue_data(n, p, seed):
    """x = 2 N(0,1) + 0.3,  y = x b + t_3 (1 + 0.3 |x_1|) + 1.5: heteroscedastic, so the quantile planes are not parallel."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, p)) * 2 + 0.3
    b = rng.uniform(size=p)
    y = x @ b + rng.standard_t(3, size=n) * (1 + 0.3 * np.abs(x[:, 0])) + 1.5
    return x, y


def strip_cold(trace):
    t = np.asarray(trace, dtype=np.float64)
    return t[1:] if len(t) and t[0, 8] == -1 else t


def followed(fit_beta, fit_niter, trace, x, y, tau, intercept, opts, tol=1e-8, band=8.0, label=""):
    """The restatement follows the library's decision trace (oracle.solvers.FADMM follow mode): niter identical, beta within tol."""
    t = strip_cold(trace)
    d = {"follow": t, "follow_band": band}
    ref = quantreg(x, y, tau, intercept, opts, d)
    assert d["solver"].ndecisions == len(t), (label, d["solver"].ndecisions, len(t))
    assert int(fit_niter) == int(ref["niter"]), (label, fit_niter, ref["niter"])
    err = float(np.max(np.abs(np.asarray(fit_beta) - ref["beta"])) / max(np.max(np.abs(ref["beta"])), 1e-300))
    print(f"[quantreg {label}] {len(t)} decisions, {len(d['forced'])} near-ties taken from the library; niter identical ({int(fit_niter)}); beta err {err:.2e}")
    assert err < tol, (label, err)
    return dict(forced=d["forced"], err=err, ref=ref)


def replay(trace, state, tau, label=""):
    """Every record of the iterate dump (x | z | y | adj_z | adj_y; record 0 carries d in its x slot): from its x, adj_y and the rho the
    trace says the iteration ran with, z by the asymmetric prox and y = adj_y + rho (x - d - z), both expected bit for bit.
    Record s holds the iterates that trace record s judged; they were formed with rho = trace[s - 1][10] (record 0: the cold start)."""
    t = np.asarray(trace, dtype=np.float64)
    s = np.asarray(state, dtype=np.float64)
    assert s.ndim == 3 and s.shape[1] == 5 and len(s) >= 2, (label, s.shape)
    d = s[0, 0]
    nrec = min(len(s), len(t))
    bad = []
    for k in range(1, nrec):
        rho = t[k - 1, 10]
        x, z, yv, adjy = s[k, 0], s[k, 1], s[k, 2], s[k, 4]
        z2 = prox(x - d + adjy / rho, rho, tau)
        y2 = adjy + rho * (x - d - z2)
        if not (np.array_equal(z2, z) and np.array_equal(y2, yv)):
            bad.append((k, int(np.sum(z2 != z)), int(np.sum(y2 != yv))))
    print(f"[quantreg replay {label}] {nrec - 1} iterations replayed: {len(bad)} with a z or y that differs")
    assert not bad, (label, bad[:5])
    return nrec - 1
