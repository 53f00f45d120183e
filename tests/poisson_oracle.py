"""Helper of the Poisson tests (tests/test_poisson_host.py, tests/test_gpu_poisson.py): the NumPy statement of the device prox, the CPU
restatement of admm_hip_poisson on the oracle's LAD class, the penalised objective, lambda_1, a float64 reference optimum that asserts its
own KKT conditions, and the replay of an iterate dump of the augmented loop.

The fit, per count column and cell (lambda, alpha):
    minimise  sum_i [exp(eta_i) - y_i eta_i] + lambda (alpha sum_j |b_j| + (1 - alpha) / 2 sum_j b_j^2),  eta_i = b0 + x~_i'b,
on the standardised columns x~, the intercept not penalised.  It is logit_enet_oracle's restatement with another loss on the data rows:
the p penalty rows are c e_j' with c = sqrt(n) for EVERY cell, z_{n + j} = c b_j, their loss is c_hi |z| + c_lo z^2 / 2 with
c_hi = lambda alpha / c, c_lo = lambda (1 - alpha) / c^2, prox soft(v, c_hi / rho) / (1 + c_lo / rho).  A data row takes the prox of
(e^z - y z) / rho: the root of h(z) = z + t e^z - w, t = 1 / rho, w = v + t y (`prox`).  The loop's "sign" vector carries the counts,
and -1.0 on the penalty rows.  Returned: b_j = z_{n + j} / c of the LAST z (exact zeros), the intercept from get_coef."""
import numpy as np

import logit_enet_oracle as le
import logit_oracle as lo
import logit_ridge_oracle as lr
from oracle.entry import _attach
from quantile_oracle import strip_cold

LN2 = 0.6931471805599453


def _ilogb(a):
    return np.frexp(a)[1] - 1


def prox_start(v, y, rho):
    """The start of the iteration, right of the root: min(w, 0) where w < t (the root is negative); else min(w, L), L an upper estimate
    of ln(w / t) -- the FLOAT logarithm of the quotient plus 2^-18 (1 + ln), and beyond 2^100 (ilogb(w) - ilogb(t) + 1) ln 2."""
    v = np.asarray(v, dtype=np.float64)
    t = 1.0 / rho
    w = v + t * np.asarray(y, dtype=np.float64)
    big = w >= t
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        q = np.where(big, w / t, 1.0)
        small_q = q < 2.0 ** 100
        lf = np.log(np.where(small_q, q, 1.0).astype(np.float32)).astype(np.float64)
        wide = (_ilogb(np.where(big, w, 1.0)) - _ilogb(t) + 1).astype(np.float64) * LN2
    up = np.where(small_q, lf + 2.0 ** -18 * (1.0 + lf), wide)
    return np.where(big, np.minimum(w, up), np.minimum(w, 0.0)), w, t


def prox(v, y, rho, maxit=200, steps=None):
    """z of the iteration as the library runs it in double: Newton steps from `prox_start`, clamped to <= w; an element stops moving once
    its step is at most 2^-50 max(1, |z|, |w|) (the step is applied), and the iteration ends when no element moves.  The library's exp and
    float logarithm are other implementations: the two agree to the rounding of h, not bit for bit.  steps: a list that receives the
    number of sweeps."""
    z, w, t = prox_start(v, y, rho)
    live = np.ones(z.shape, dtype=bool)
    n = 0
    for n in range(maxit + 1):
        if not live.any():
            break
        e = t * np.exp(z)
        h = z + e - w
        d = 1.0 + e
        zn = np.minimum(z - h / d, w)
        moved = np.abs(zn - z)
        z = np.where(live, zn, z)
        live = live & ~(moved <= 2.0 ** -50 * np.maximum(1.0, np.maximum(np.abs(z), np.abs(w))))
    assert not live.any(), ("the Poisson prox did not settle", rho, int(live.sum()))
    if steps is not None:
        steps.append(n)
    return z


def prox_exact(v, y, rho):
    """The root of h by bisection until the bracket is closed (its ends adjacent doubles, or equal).  Bracket: h(w) = t e^w > 0;
    w >= t: h(0) <= 0; else h(min(w, 0) - t) <= 0 (t e^z <= t there)."""
    v = np.asarray(v, dtype=np.float64)
    t = 1.0 / rho
    w = v + t * np.asarray(y, dtype=np.float64)
    lo_ = np.where(w >= t, 0.0, np.minimum(w, 0.0) - t)
    hi = np.maximum(w, lo_)

    def h(z):
        with np.errstate(over="ignore"):
            return z + t * np.exp(z) - w

    for _ in range(2200):
        mid = lo_ + 0.5 * (hi - lo_)
        if np.all((mid == lo_) | (mid == hi)):
            break
        below = h(mid) < 0.0
        lo_ = np.where(below, mid, lo_)
        hi = np.where(below, hi, mid)
    return np.where(np.abs(h(lo_)) <= np.abs(h(hi)), lo_, hi)


def prox_tol(v, y, rho):
    """h' >= 1: the root moves by at most the rounding of w = v + y / rho"""
    v, y = np.asarray(v, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return 1e-13 * np.maximum(np.maximum(1.0, np.abs(v)), np.maximum(y / rho, 1.0 / rho))


def counts_of(y, p):
    """what the loop's "sign" vector holds: the counts, and the marker -1.0 on the p penalty rows"""
    return np.concatenate([np.asarray(y, dtype=np.float64), -np.ones(p)])


class PoisEnet(lr.LogitRidge):
    """LogitRidge's loop with the Poisson prox where the entry is a count (>= 0) and the elastic net's where it is the marker -1."""

    def __init__(self, X, counts, rho, eps_abs, eps_rel, c_hi, c_lo):
        lr.LogitRidge.__init__(self, X, counts, rho, eps_abs, eps_rel)
        self.data = counts >= 0.0
        self.c_hi, self.c_lo = c_hi, c_lo

    def next_z(self):
        v = self.main_x - self.Y + self.adj_y / self.rho
        z = le.enet_prox(v, self.rho, self.c_hi, self.c_lo)
        z[self.data] = prox(v[self.data], self.signs[self.data], self.rho)
        return z


def poisson(x, Y, lam, alpha, intercept, opts, details=None):
    """The restatement of admm_hip_poisson: per cell (lam[l], alpha[l]), in the order given, and count column one cold PoisEnet loop on
    the one augmented matrix.  details: None, or details[l][c] a dict as oracle.entry's `detail`.
    -> {"beta": (p + 1) x k x ncell, "niter": k x ncell}"""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    lam = np.atleast_1d(np.asarray(lam, dtype=np.float64))
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), lam.shape)
    n, p = np.asarray(x).shape
    k = Y.shape[1]
    c = np.sqrt(float(n))
    X, std = le.augmented(x, intercept)
    beta = np.zeros((p + 1, k, lam.size))
    niter = np.zeros((k, lam.size), dtype=np.int64)
    for l in range(lam.size):
        c_hi, c_lo = le.constants(lam[l], alpha[l], n)
        for col in range(k):
            solver = PoisEnet(X, counts_of(Y[:, col], p), float(opts["rho"]), float(opts["eps_abs"]), float(opts["eps_rel"]), c_hi, c_lo)
            d = None if details is None else details[l][col]
            _attach(solver, d)
            niter[col, l] = solver.solve(int(opts["maxit"]))
            b = solver.get_coef()
            b[:p] = solver.aux_z[n:] / c
            beta[:, col, l] = lo.recover(std, b, p, intercept)
            if d is not None:
                d.update(solver=solver, std=std, dense=solver.get_coef())
    return {"beta": beta, "niter": niter}


def poisson_data(n, p, seed, b0=0.7):
    """x = N(0, 1),  y = Poisson(exp(b0 + 0.5 x_0 - 0.4 x_1 + 0.3 x_2)): mean count about 2.6 at b0 = 0.7, 0.18 (83 % zeros) at -2, 68 at 4"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, p))
    y = rng.poisson(np.exp(b0 + 0.5 * x[:, 0] - 0.4 * x[:, 1] + 0.3 * x[:, 2])).astype(np.float64)
    return x, y


K = 7


def count_matrix(x, seed):
    """n x 7, column-major counts on the design x, each column drawn from the data's model with its own generator.  Columns 0 - 3:
    b0 = 0.7, 0.0, -2.0 (about 83 % zeros) and 1.5 (mean about 6); columns 4 and 5: one further column (b0 = 1.2), twice; column 6:
    three times column 0."""
    x = np.asarray(x, dtype=np.float64)
    eta = 0.5 * x[:, 0] - 0.4 * x[:, 1] + 0.3 * x[:, 2]

    def column(j, b0):
        return np.random.default_rng(1000 * seed + j).poisson(np.exp(b0 + eta)).astype(np.float64)

    cols = [column(0, 0.7), column(1, 0.0), column(2, -2.0), column(3, 1.5), column(4, 1.2)]
    return np.asfortranarray(np.column_stack(cols + [cols[4], 3.0 * cols[0]]))


def objective(x_std, y, b0, b, lam, alpha):
    """sum [exp(eta) - y eta] + lam (alpha |b|_1 + (1 - alpha) / 2 |b|^2) on the standardised scale"""
    eta = x_std @ b + b0
    return float(np.sum(np.exp(eta) - np.asarray(y, dtype=np.float64) * eta)
                 + float(lam) * (float(alpha) * float(np.abs(b).sum()) + 0.5 * (1.0 - float(alpha)) * float(b @ b)))


def objective_of(x, y, beta, lam, alpha, intercept):
    """`objective` of caller-scale coefficients."""
    xs, std = lr.standardized_design(x, intercept)
    b0, b = lr.to_std(std, np.asarray(beta, dtype=np.float64), intercept)
    return objective(xs, y, b0, b, lam, alpha)


def null_objective(y, intercept):
    """the objective of the empty model: b = 0 with b0 = log mean(y) (the fitted intercept), or eta = 0 without it"""
    y = np.asarray(y, dtype=np.float64)
    if not intercept:
        return float(len(y))
    m = float(y.mean())
    return float(len(y) * m - y.sum() * np.log(m))


def lambda_one(x, Y, intercept):
    """-> (k,) max_j |x~_j'(y_c - mean(y_c))| with the intercept, |x~_j'(y_c - 1)| without (mu = 1 at eta = 0)"""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    xs, _ = lr.standardized_design(x, intercept)
    r = Y - (Y.mean(axis=0)[None, :] if intercept else 1.0)
    return np.max(np.abs(xs.T @ r), axis=0)


def _kkt(A, y, D, b, lam, alpha):
    """-> (the worst violation, the scale it is measured against) of the optimality conditions at b: with g the gradient of the
    likelihood plus the ridge term, |g_j| <= lam alpha where a penalised b_j = 0, g_j + lam alpha sign(b_j) = 0 elsewhere, g = 0 for
    the intercept"""
    mu = np.exp(A @ b)
    g = A.T @ (mu - y) + lam * (1.0 - alpha) * D * b
    zero = (D > 0) & (b == 0.0)
    viol = np.where(zero, np.maximum(np.abs(g) - lam * alpha, 0.0), np.abs(g + lam * alpha * D * np.sign(b)))
    scale = max(float(np.max(np.abs(A).T @ (mu + y) + lam * (1.0 - alpha) * D * np.abs(b))), lam * alpha, 1.0)
    return float(np.max(viol)), scale


def poisson_optimum(x_std, y, lam, alpha, intercept, maxit=400):
    """Float64 reference optimum by proximal Newton: the quadratic model of the smooth part (likelihood + ridge term) at b with the l1
    term kept, minimised by coordinate descent, then a backtracking line search on the objective; after every outer step a Newton polish
    of the smooth problem on the current support with its signs held (the l1 term is linear there).  A polished point is accepted only
    when it keeps those signs and satisfies the KKT conditions of the WHOLE problem to 1e-9 of scale, which is asserted.
    -> (b0, b on the standardised scale, optimum)"""
    lam, alpha = float(lam), float(alpha)
    y = np.asarray(y, dtype=np.float64)
    n, p = x_std.shape
    A = np.hstack([np.ones((n, 1)), x_std]) if intercept else x_std
    D = np.concatenate([[0.0], np.ones(p)]) if intercept else np.ones(p)
    pen = D > 0
    l1, l2 = lam * alpha, lam * (1.0 - alpha)
    m = A.shape[1]

    def full(b):
        eta = A @ b
        with np.errstate(over="ignore"):
            return float(np.sum(np.exp(eta) - y * eta) + l1 * float(np.abs(D * b).sum()) + 0.5 * l2 * float((D * b) @ b))

    def polish(b):
        S = ~pen | (b != 0.0)
        sg = np.sign(b[S]) * D[S]
        AS, DS = A[:, S], D[S]
        u = b[S].copy()

        def hS(w):
            eta = AS @ w
            with np.errstate(over="ignore"):
                return float(np.sum(np.exp(eta) - y * eta) + 0.5 * l2 * float((DS * w) @ w) + l1 * float(sg @ w))

        for _ in range(60):
            mu = np.exp(AS @ u)
            g = AS.T @ (mu - y) + l2 * DS * u + l1 * sg
            H = (AS * mu[:, None]).T @ AS + l2 * np.diag(DS)
            try:
                step = np.linalg.solve(H, -g)
            except np.linalg.LinAlgError:
                return None
            a, h0 = 1.0, hS(u)
            while not hS(u + a * step) <= h0 and a > 1e-10:
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

    b = np.zeros(m)
    if intercept:
        b[0] = np.log(y.mean())
    done = False
    for _ in range(maxit):
        mu = np.exp(A @ b)
        g = A.T @ (mu - y) + l2 * D * b
        H = (A * mu[:, None]).T @ A + l2 * np.diag(D)
        hd = np.maximum(np.diag(H), 1e-300)
        bb = b.copy()                                             # the model's minimiser so far (exact zeros kept)
        q = g.copy()                                              # g + H (bb - b)
        for _sweep in range(2000):
            worst = 0.0
            for j in range(m):
                u = bb[j] - q[j] / hd[j]
                new = np.sign(u) * max(abs(u) - l1 / hd[j], 0.0) if pen[j] else u
                dj = new - bb[j]
                if dj != 0.0:
                    bb[j] = new
                    q += dj * H[:, j]
                    worst = max(worst, abs(dj) * np.sqrt(hd[j]))
            if worst <= 1e-12 * max(1.0, float(np.max(np.abs(bb) * np.sqrt(hd)))):
                break
        a, f0 = 1.0, full(b)
        while not full(b + a * (bb - b)) <= f0 and a > 1e-12:
            a *= 0.5
        bn = bb if a == 1.0 else b + a * (bb - b)
        step = float(np.max(np.abs(bn - b)) / max(float(np.max(np.abs(bn))), 1e-300))
        b = bn
        cand = polish(b)
        if cand is not None:
            viol, scale = _kkt(A, y, D, cand, lam, alpha)
            if viol <= 1e-9 * scale:
                b, done = cand, True
                break
        if step == 0.0:
            break
    viol, scale = _kkt(A, y, D, b, lam, alpha)
    assert done and viol <= 1e-9 * scale, ("the Poisson reference optimum misses its KKT conditions", viol, scale, lam, alpha)
    b0, bb = (float(b[0]), b[1:]) if intercept else (0.0, b)
    best = objective(x_std, y, b0, bb, lam, alpha)
    assert abs(best - full(b)) <= 1e-12 * max(1.0, abs(best))
    return b0, bb, best


def followed(fit_beta, fit_niter, trace, x, y, lam, alpha, intercept, opts, tol=1e-8, band=8.0, label=""):
    """The restatement follows the library's decision trace (oracle.solvers.FADMM follow mode): niter identical, beta within tol; a zero
    that differs is counted in the error, being a coefficient the other side does not have."""
    t = strip_cold(trace)
    d = {"follow": t, "follow_band": band}
    ref = poisson(x, y, lam, alpha, intercept, opts, [[d]])
    beta = ref["beta"][:, 0, 0]
    assert d["solver"].ndecisions == len(t), (label, d["solver"].ndecisions, len(t))
    assert int(fit_niter) == int(ref["niter"][0, 0]), (label, fit_niter, ref["niter"])
    err = float(np.max(np.abs(np.asarray(fit_beta) - beta)) / max(np.max(np.abs(beta)), 1e-300))
    zeros = int(np.sum((np.asarray(fit_beta)[1:] == 0.0) != (beta[1:] == 0.0)))
    print(f"[poisson {label}] {len(t)} decisions, {len(d['forced'])} near-ties taken from the library; niter identical ({int(fit_niter)}); beta err {err:.2e}; "
          f"{zeros} zeros differ")
    assert err < tol, (label, err)
    return dict(forced=d["forced"], err=err, beta=beta, zeros=zeros)


def replay(trace, state, y, p, lam, alpha, label=""):
    """Every record of the iterate dump of the augmented loop (x | z | y | adj_z | adj_y, n + p entries each).  Record 0 carries the zero
    response in its x slot and what the loop ran with in its z slot: the counts, then p entries of -1.0, exactly.  For every iteration
    k >= 1, from its x, adj_y and the rho the trace says it ran with (trace[k - 1][10]): on the data rows z recomputed within prox_tol
    of the dumped one; on the penalty rows within 4 ulp of soft(v, t) / d in the stated association, and an entry the restatement
    makes exactly 0 exactly 0; y = adj_y + rho (x - z_dump) bit for bit from the DUMPED z."""
    t = np.asarray(trace, dtype=np.float64)
    s = np.asarray(state, dtype=np.float64)
    n = len(y)
    assert s.ndim == 3 and s.shape[1] == 5 and s.shape[2] == n + p and len(s) >= 2, (label, s.shape)
    d = s[0, 0]
    assert not np.any(d) and not np.any(s[0, 2:]), label
    cnt = counts_of(y, p)
    assert np.array_equal(s[0, 1], cnt), label
    c_hi, c_lo = le.constants(lam, alpha, n)
    nrec = min(len(s), len(t))
    bad, worst, worst_ulp, nzero = [], 0.0, 0.0, 0
    for k in range(1, nrec):
        rho = t[k - 1, 10]
        x, z, yv, adjy = s[k, 0], s[k, 1], s[k, 2], s[k, 4]
        v = x - d + adjy / rho
        z2 = prox(v[:n], cnt[:n], rho)
        rel = float(np.max(np.abs(z2 - z[:n]) / prox_tol(v[:n], cnt[:n], rho)))
        zr = le.enet_prox(v[n:], rho, c_hi, c_lo)
        ulps = float(np.max(np.abs(zr - z[n:]) / np.spacing(np.maximum(np.abs(zr), np.finfo(np.float64).tiny))))
        zeros_kept = bool(np.all(z[n:][zr == 0.0] == 0.0))
        nzero += int(np.sum(zr == 0.0))
        worst, worst_ulp = max(worst, rel), max(worst_ulp, ulps)
        y2 = adjy + rho * (x - d - z)
        if rel > 1.0 or ulps > 4.0 or not zeros_kept or not np.array_equal(y2, yv) or not np.all(np.isfinite(z)):
            bad.append((k, rel, ulps, zeros_kept, int(np.sum(y2 != yv))))
    print(f"[poisson replay {label}] {nrec - 1} iterations replayed: {len(bad)} off; worst |z - z_dump| = {worst:.2e} of the tolerance "
          f"(data rows), {worst_ulp:.1f} ulp (penalty rows, {nzero} exact zeros)")
    assert not bad, (label, bad[:5])
    return nrec - 1
