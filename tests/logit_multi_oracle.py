"""Helper of the multi-column logistic tests (tests/test_logit_multi_host.py, tests/test_gpu_logit_multi.py): the label matrices, and the
CPU restatement of admm_hip_logit_multi's loop -- the UNFOLDED one.

admm_hip_logit folds the label signs into the matrix, X~ = diag(s) [X_std | 1], s = 2 y - 1 (tests/logit_oracle.py).  The multi-column
call leaves the matrix alone and takes the sign inside the prox:  prox of log(1 + e^(-s z)) / rho at v  =  s prox(s v)  with logit_oracle's
`prox`.  Multiplication by +-1 is exact and IEEE rounding is symmetric in sign, so every n-vector of the unfolded loop (x, z, y, adj_z,
adj_y) is s times the folded loop's and every X'v, norm and decision is equal: `LogitS` below, on [X_std | 1] with a zero response, must
reproduce `logit_oracle.logit` number for number (only the sign of an exact zero may differ)."""
import numpy as np

import logit_oracle as lo
from oracle.entry import _attach
from oracle.solvers import LAD
from quantile_oracle import standardized

K = 7
# share of ones of the four threshold columns, and the seeds of their score vectors' coefficients and noise
SHARES = (0.5, 0.3, 0.7, 0.15)


def label_matrix(x, seed):
    """n x 7, column-major, labels 0.0 / 1.0.  Columns 0 - 3: a noisy linear score of x (own coefficients and logistic noise per column)
    thresholded at the quantile that leaves the column's share of ones; columns 4 and 5: one further such column, twice; column 6:
    1 - column 0."""
    x = np.asarray(x, dtype=np.float64)
    n, p = x.shape

    def column(j, share):
        rng = np.random.default_rng(1000 * seed + j)
        b = rng.uniform(-1.0, 1.0, size=p) / np.sqrt(p)
        score = (0.5 + 0.25 * j) * (x @ b) + rng.logistic(size=n)
        return (score > np.quantile(score, 1.0 - share)).astype(np.float64)

    cols = [column(j, share) for j, share in enumerate(SHARES)]
    twice = column(4, 0.4)
    cols += [twice, twice.copy(), 1.0 - cols[0]]
    return np.asfortranarray(np.stack(cols, axis=1))


class LogitS(LAD):
    """LAD on the unfolded matrix with Y = 0 and the signed Newton prox."""

    def __init__(self, X, signs, rho, eps_abs, eps_rel):
        LAD.__init__(self, X, np.zeros(X.shape[0]), rho, eps_abs, eps_rel)
        self.signs = signs

    def next_z(self):
        return self.signs * lo.prox(self.signs * (self.main_x - self.Y + self.adj_y / self.rho), self.rho)


def unfolded(x, intercept):
    """-> ([X_std | 1], the DataStd of x): what every label column shares."""
    X, _, std = standardized(x, np.linspace(0.0, 1.0, np.asarray(x).shape[0]), intercept)      # (the response is not used: it is zero in the loop)
    return np.asfortranarray(X), std


def logit_multi(x, Y, intercept, opts, details=None):
    """The restatement of admm_hip_logit_multi: one LogitS loop per column of Y on the shared matrix.  details: a list of K dicts as
    oracle.entry's `detail` (trace / state), or None.  -> {"beta": (p + 1) x k, "niter": k}"""
    Y = np.asarray(Y, dtype=np.float64)
    p = np.asarray(x).shape[1]
    X, std = unfolded(x, intercept)
    beta, niter = [], []
    for c in range(Y.shape[1]):
        s = 2.0 * Y[:, c] - 1.0
        solver = LogitS(X, s, float(opts["rho"]), float(opts["eps_abs"]), float(opts["eps_rel"]))
        _attach(solver, None if details is None else details[c])
        niter.append(solver.solve(int(opts["maxit"])))
        beta.append(lo.recover(std, solver.get_coef(), p, intercept))
    return {"beta": np.stack(beta, axis=1), "niter": np.asarray(niter)}
