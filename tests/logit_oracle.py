"""Helper of the logistic-regression tests (tests/test_logit_host.py, tests/test_gpu_logit.py): the CPU restatement of admm_hip_logit on
the oracle's LAD class, the negative log-likelihood, a float64 IRLS (Newton) optimum, and the replay of an iterate dump.

The fit:  minimise sum_i log(1 + exp(-s_i (b0 + x_i'b))),  s_i = 2 y_i - 1,  y_i in {0, 1}.  With the signs folded into the matrix,
X~ = diag(s) [X_std | 1], it is  min g(z)  s.t.  X~ b - z = 0,  g(z) = sum log(1 + e^-z_i): oracle.solvers.LAD with a ZERO response and
the prox below.  X~'X~ = [X 1]'[X 1].  The response is not a scale: recovery with scaleY = 1 and meanY = 0.

The prox:  prox_{g / rho}(v) is the root of h(z) = z - v - t sigma(-z),  t = 1 / rho,  sigma(-z) = 1 / (1 + e^z), inside [v, v + t]; h is
increasing with 1 <= h' <= 1 + t / 4.  `prox` is Newton's iteration as the library runs it in double (same start, same clamp, same
stable form of sigma, every operation rounded on its own); the library seeds it with two float steps and its exp is another
implementation, so the two agree to rounding of h, not bit for bit.  `prox_exact` is bisection to a closed bracket."""
import numpy as np

from oracle.entry import _attach
from oracle.solvers import LAD
from quantile_oracle import standardized, strip_cold


def _sigma_neg(z):
    """sigma(-z) = 1 / (1 + e^z) from e = exp(-|z|): nothing overflows."""
    e = np.exp(-np.abs(z))
    return np.where(z >= 0.0, e, 1.0) / (1.0 + e)


def prox(v, rho, maxit=200):
    """z of the iteration.  Start: v where v > 0, v + t where v + t < 0, else 0; Newton steps clamped to [v, v + t]; an element stops
    moving once its step is at most 2^-50 max(1, |z|, |v|) (the step is applied), and the iteration ends when no element moves."""
    v = np.asarray(v, dtype=np.float64)
    t = 1.0 / rho
    hi = v + t
    z = np.where(v > 0.0, v, np.where(hi < 0.0, hi, 0.0))
    live = np.ones(z.shape, dtype=bool)
    for _ in range(maxit):
        if not live.any():
            break
        s = _sigma_neg(z)
        h = z - v - t * s
        d = 1.0 + t * s * (1.0 - s)
        zn = np.minimum(np.maximum(z - h / d, v), hi)
        moved = np.abs(zn - z)
        z = np.where(live, zn, z)
        live = live & ~(moved <= 2.0 ** -50 * np.maximum(1.0, np.maximum(np.abs(z), np.abs(v))))
    assert not live.any(), ("the Newton prox did not settle", rho, int(live.sum()))
    return z


def prox_exact(v, rho):
    """The root of h by bisection on [v, v + t] until the bracket is closed (its ends adjacent doubles, or equal)."""
    v = np.asarray(v, dtype=np.float64)
    t = 1.0 / rho
    lo, hi = v.copy(), v + t
    for _ in range(2200):
        mid = lo + 0.5 * (hi - lo)
        if np.all((mid == lo) | (mid == hi)):
            break
        below = mid - v - t * _sigma_neg(mid) < 0.0
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    hl = np.abs(lo - v - t * _sigma_neg(lo))
    hh = np.abs(hi - v - t * _sigma_neg(hi))
    return np.where(hl <= hh, lo, hi)


def prox_tol(v, rho):
    return 1e-13 * np.maximum(1.0, np.maximum(np.abs(v), 1.0 / rho))


class Logit(LAD):
    """LAD on the sign-folded matrix with Y = 0 and the Newton prox."""

    def next_z(self):
        return prox(self.main_x - self.Y + self.adj_y / self.rho, self.rho)


def folded(x, y, intercept):
    """-> (X~ = diag(2 y - 1) [X_std | 1], the signs, the DataStd of x)."""
    y = np.asarray(y, dtype=np.float64)
    X, _, std = standardized(x, y.copy(), intercept)
    s = 2.0 * y - 1.0
    return np.asfortranarray(X * s[:, None]), s, std


def recover(std, b, p, intercept):
    """beta_j = b_j / scaleX_j;  beta_0 = -sum beta_j meanX_j + b_{p+1}: DataStd's recovery without a response scale or mean."""
    coef = b[:p] / std.scaleX
    beta0 = 0.0
    if intercept:
        beta0 = (0.0 - float((coef * std.meanX).sum())) + b[p]
    return np.concatenate([[beta0], coef])


def logit(x, y, intercept, opts, detail=None):
    """The restatement of admm_hip_logit.  detail: as oracle.entry (follow / follow_band / forced / trace / state)."""
    p = np.asarray(x).shape[1]
    X, s, std = folded(x, y, intercept)
    solver = Logit(X, np.zeros(X.shape[0]), float(opts["rho"]), float(opts["eps_abs"]), float(opts["eps_rel"]))
    _attach(solver, detail)
    niter = solver.solve(int(opts["maxit"]))
    b = solver.get_coef()
    if detail is not None:
        detail.update(solver=solver, std=std, signs=s)
    return {"beta": recover(std, b, p, intercept), "niter": niter}


def nll(x, y, beta):
    """sum log(1 + exp(-s (b0 + x'b))), stable for any margin."""
    m = (2.0 * np.asarray(y, dtype=np.float64) - 1.0) * (np.asarray(x) @ beta[1:] + beta[0])
    return float(np.sum(np.maximum(-m, 0.0) + np.log1p(np.exp(-np.abs(m)))))


def logit_irls(x, y, intercept, maxit=100):
    """Float64 maximum likelihood by Newton's method (IRLS) with step halving, to a relative step below 1e-13; checked by max |gradient|
    -> (beta with the intercept first, optimum, steps)."""
    x = np.asarray(x, dtype=np.float64)
    s = 2.0 * np.asarray(y, dtype=np.float64) - 1.0
    n, p = x.shape
    A = np.hstack([np.ones((n, 1)), x]) if intercept else x
    B = A * s[:, None]

    def f(b):
        m = B @ b
        return float(np.sum(np.maximum(-m, 0.0) + np.log1p(np.exp(-np.abs(m)))))

    b = np.zeros(A.shape[1])
    step, steps = np.inf, 0
    for steps in range(1, maxit + 1):
        q = _sigma_neg(B @ b)                                    # sigma(-margin)
        g = -(B.T @ q)
        H = (A * (q * (1.0 - q))[:, None]).T @ A
        dlt = np.linalg.solve(H, -g)
        a, f0 = 1.0, f(b)
        while f(b + a * dlt) > f0 and a > 1e-10:
            a *= 0.5
        bn = b + a * dlt
        step = float(np.max(np.abs(bn - b)) / max(np.max(np.abs(bn)), 1e-300))
        b = bn
        if step < 1e-13:
            break
    assert step < 1e-13, ("IRLS did not settle", step)
    q = _sigma_neg(B @ b)
    grad = float(np.max(np.abs(B.T @ q)))
    scale = float(np.max(np.abs(B).T @ q))
    assert grad <= 1e-9 * max(scale, 1.0), ("IRLS gradient", grad, scale)
    beta = b if intercept else np.concatenate([[0.0], b])
    return beta, nll(x, y, beta), steps


def followed(fit_beta, fit_niter, trace, x, y, intercept, opts, tol=1e-8, band=8.0, label=""):
    """The restatement follows the library's decision trace (oracle.solvers.FADMM follow mode): niter identical, beta within tol."""
    t = strip_cold(trace)
    d = {"follow": t, "follow_band": band}
    ref = logit(x, y, intercept, opts, d)
    assert d["solver"].ndecisions == len(t), (label, d["solver"].ndecisions, len(t))
    assert int(fit_niter) == int(ref["niter"]), (label, fit_niter, ref["niter"])
    err = float(np.max(np.abs(np.asarray(fit_beta) - ref["beta"])) / max(np.max(np.abs(ref["beta"])), 1e-300))
    print(f"[logit {label}] {len(t)} decisions, {len(d['forced'])} near-ties taken from the library; niter identical ({int(fit_niter)}); beta err {err:.2e}")
    assert err < tol, (label, err)
    return dict(forced=d["forced"], err=err, ref=ref)


def replay(trace, state, y, label=""):
    """Every record of the iterate dump (x | z | y | adj_z | adj_y; record 0 carries the zero response in its x slot and the n signs the
    loop ran with in its z slot, which must be 2 y - 1 exactly).  For every iteration k >= 1, from its x, adj_y and the rho the trace
    says it ran with (trace[k - 1][10]): z recomputed within 1e-13 max(1, |v|, 1 / rho) of the dumped one, elementwise, and
    y = adj_y + rho (x - z_dump) bit for bit from the DUMPED z."""
    t = np.asarray(trace, dtype=np.float64)
    s = np.asarray(state, dtype=np.float64)
    assert s.ndim == 3 and s.shape[1] == 5 and len(s) >= 2, (label, s.shape)
    d = s[0, 0]
    assert not np.any(d) and not np.any(s[0, 2:]), label
    assert np.array_equal(s[0, 1], 2.0 * np.asarray(y, dtype=np.float64) - 1.0), label
    nrec = min(len(s), len(t))
    bad, worst = [], 0.0
    for k in range(1, nrec):
        rho = t[k - 1, 10]
        x, z, yv, adjy = s[k, 0], s[k, 1], s[k, 2], s[k, 4]
        v = x - d + adjy / rho
        z2 = prox(v, rho)
        rel = float(np.max(np.abs(z2 - z) / prox_tol(v, rho)))
        worst = max(worst, rel)
        y2 = adjy + rho * (x - d - z)
        if rel > 1.0 or not np.array_equal(y2, yv) or not np.all(np.isfinite(z)):
            bad.append((k, rel, int(np.sum(y2 != yv))))
    print(f"[logit replay {label}] {nrec - 1} iterations replayed: {len(bad)} off; worst |z - z_dump| = {worst:.2e} of the tolerance")
    assert not bad, (label, bad[:5])
    return nrec - 1


def logit_data(n, p, seed):
    """x = 2 N(0, 1) + 0.3,  eta = 0.5 x b - 0.4 with b = U(-1, 1) / sqrt(p),  y = U(0, 1) < sigma(eta): about 40 % ones, not separable
    while p / n stays well below one half."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, p)) * 2 + 0.3
    b = rng.uniform(-1.0, 1.0, size=p) / np.sqrt(p)
    eta = 0.5 * (x @ b) - 0.4
    y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    return x, y
