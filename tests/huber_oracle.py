"""Helper of the Huber-regression tests (tests/test_huber_host.py, tests/test_gpu_huber.py): the CPU restatement of admm_hip_huber on
the oracle's LAD class, the loss, a float64 IRLS optimum, and the replay of an iterate dump.

The fit:  minimise sum_i w_tau(r_i) H_delta(r_i),  r_i = y_i - b0 - x_i'b,  H_delta(r) = r^2 / 2 (|r| <= delta), delta |r| - delta^2 / 2
beyond,  w_tau(r) = 2 tau (r >= 0), 2 (1 - tau) (r < 0).  In the ADMM form of ADMMLAD.h (z = X b - y = -r) the loop uses
g(z) = sum w(z_i) H_delta(z_i) with w = c_hi = 2 (1 - tau) for z > 0 and c_lo = 2 tau for z < 0, whose prox is `prox` below.  Everything
else is oracle.solvers.LAD; data, standardisation and the fitted intercept are tests/quantile_oracle.py's.  The loop runs on the
standardised response, so it uses delta / scaleY (H is positively homogeneous in (r, delta))."""
import numpy as np

from oracle.entry import _attach
from oracle.solvers import LAD
from quantile_oracle import issue_data, standardized, strip_cold  # noqa: F401  (issue_data: re-exported for the tests)


def prox(v, rho, tau, delta):
    """z of the iteration = argmin_z w(z) H_delta(z) / rho + (z - v)^2 / 2: every operation rounded on its own, in this order."""
    pen_hi = (2.0 * (1.0 - tau)) / rho
    pen_lo = (2.0 * tau) / rho
    with np.errstate(invalid="ignore"):      # (inf - inf in a branch np.where does not take, delta = inf)
        return np.where(v > delta * (1.0 + pen_hi), v - delta * pen_hi,
                        np.where(v < -(delta * (1.0 + pen_lo)), v + delta * pen_lo,
                                 np.where(v >= 0.0, v / (1.0 + pen_hi), v / (1.0 + pen_lo))))


class Huber(LAD):
    def __init__(self, X, Y, rho, eps_abs, eps_rel, tau, delta):
        LAD.__init__(self, X, Y, rho, eps_abs, eps_rel)
        self.tau_q = float(tau)
        self.delta_s = float(delta)          # in the units of the standardised response

    def next_z(self):
        return prox(self.main_x - self.Y + self.adj_y / self.rho, self.rho, self.tau_q, self.delta_s)


def huber(x, y, delta, tau, intercept, opts, detail=None):
    """The restatement of admm_hip_huber for ONE (delta, tau).  detail: as oracle.entry (follow / follow_band / forced / trace / state)."""
    p = np.asarray(x).shape[1]
    X, Y, std = standardized(x, y, intercept)
    solver = Huber(X, Y, float(opts["rho"]), float(opts["eps_abs"]), float(opts["eps_rel"]), tau, float(delta) / std.scaleY)
    _attach(solver, detail)
    niter = solver.solve(int(opts["maxit"]))
    b = solver.get_coef()
    beta0, coef = std.recover(b[:p])
    if intercept:
        beta0 = beta0 + std.scaleY * b[p]
    if detail is not None:
        detail.update(solver=solver, std=std)
    return {"beta": np.concatenate([[beta0], coef]), "niter": niter}


def huber_loss(x, y, beta, delta, tau):
    r = np.asarray(y) - np.asarray(x) @ beta[1:] - beta[0]
    a = np.abs(r)
    with np.errstate(invalid="ignore", over="ignore"):
        h = np.where(a <= delta, 0.5 * r * r, delta * a - 0.5 * delta * delta)
    return float(np.sum(np.where(r >= 0, 2.0 * tau, 2.0 * (1.0 - tau)) * h))


def huber_irls(x, y, delta, tau, intercept, maxit=5000):
    """Float64 optimum by iteratively re-weighted least squares, weights w_tau(r) min(1, delta / |r|), to a step below 1e-13 (relative);
    checked by max |gradient| of the loss -> (beta with the intercept first, optimum)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n, p = x.shape
    A = np.hstack([np.ones((n, 1)), x]) if intercept else x
    b = np.linalg.lstsq(A, y, rcond=None)[0]

    def weights(r):
        a = np.maximum(np.abs(r), 1e-300)
        return np.where(r >= 0, 2.0 * tau, 2.0 * (1.0 - tau)) * np.minimum(1.0, delta / a)

    step = np.inf
    for _ in range(maxit):
        w = weights(y - A @ b)
        Aw = A * w[:, None]
        bn = np.linalg.solve(A.T @ Aw, Aw.T @ y)
        step = float(np.max(np.abs(bn - b)) / max(np.max(np.abs(bn)), 1e-300))
        b = bn
        if step < 1e-13:
            break
    assert step < 1e-13, ("IRLS did not settle", delta, tau, step)
    r = y - A @ b
    psi = weights(r) * r                                       # w_tau(r) H'_delta(r)
    grad = float(np.max(np.abs(A.T @ psi)))
    scale = float(np.max(np.abs(A).T @ np.abs(psi)))
    assert grad <= 1e-9 * max(scale, 1.0), ("IRLS gradient", delta, tau, grad, scale)
    beta = b if intercept else np.concatenate([[0.0], b])
    return beta, huber_loss(x, y, beta, delta, tau)


def followed(fit_beta, fit_niter, trace, x, y, delta, tau, intercept, opts, tol=1e-8, band=8.0, label=""):
    """The restatement follows the library's decision trace (oracle.solvers.FADMM follow mode): niter identical, beta within tol."""
    t = strip_cold(trace)
    d = {"follow": t, "follow_band": band}
    ref = huber(x, y, delta, tau, intercept, opts, d)
    assert d["solver"].ndecisions == len(t), (label, d["solver"].ndecisions, len(t))
    assert int(fit_niter) == int(ref["niter"]), (label, fit_niter, ref["niter"])
    err = float(np.max(np.abs(np.asarray(fit_beta) - ref["beta"])) / max(np.max(np.abs(ref["beta"])), 1e-300))
    print(f"[huber {label}] {len(t)} decisions, {len(d['forced'])} near-ties taken from the library; niter identical ({int(fit_niter)}); beta err {err:.2e}")
    assert err < tol, (label, err)
    return dict(forced=d["forced"], err=err, ref=ref)


def replay(trace, state, delta_s, tau, label=""):
    """Every record of the iterate dump (x | z | y | adj_z | adj_y; record 0 carries d in its x slot and the knee the loop ran with as
    the first entry of its z slot): from its x, adj_y and the rho the trace says the iteration ran with, z by the prox and
    y = adj_y + rho (x - d - z), both expected bit for bit.  delta_s: the knee in the units of the standardised response, delta over
    the oracle's scaleY; the library's own (delta over ITS scaleY, whose sum of squares is added in another order) must agree with it
    to 1e-14 relative and is the one replayed.  Record s holds the iterates that trace record s judged; they were formed with
    rho = trace[s - 1][10] (record 0: the cold start)."""
    t = np.asarray(trace, dtype=np.float64)
    s = np.asarray(state, dtype=np.float64)
    assert s.ndim == 3 and s.shape[1] == 5 and len(s) >= 2, (label, s.shape)
    d = s[0, 0]
    held = float(s[0, 1, 0])
    assert not np.any(s[0, 1, 1:]) and not np.any(s[0, 2:]), label
    if np.isinf(delta_s):
        assert held == delta_s, (label, held)
    else:
        assert abs(held - delta_s) <= 1e-14 * delta_s, (label, held, delta_s)
    print(f"[huber replay {label}] knee of the loop {held!r}, delta / scaleY of the oracle {delta_s!r}")
    delta_s = held
    nrec = min(len(s), len(t))
    bad = []
    for k in range(1, nrec):
        rho = t[k - 1, 10]
        x, z, yv, adjy = s[k, 0], s[k, 1], s[k, 2], s[k, 4]
        z2 = prox(x - d + adjy / rho, rho, tau, delta_s)
        y2 = adjy + rho * (x - d - z2)
        if not (np.array_equal(z2, z) and np.array_equal(y2, yv)):
            bad.append((k, int(np.sum(z2 != z)), int(np.sum(y2 != yv))))
    print(f"[huber replay {label}] {nrec - 1} iterations replayed: {len(bad)} with a z or y that differs")
    assert not bad, (label, bad[:5])
    return nrec - 1


def scale_y(x, y, intercept):
    """scaleY of the standardisation the library applies (DataStd): delta / scale_y is the knee the loop runs with."""
    return float(standardized(x, y, intercept)[2].scaleY)
