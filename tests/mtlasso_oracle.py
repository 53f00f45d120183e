"""NumPy restatement of the multi-task lasso of admm_hip_mtlasso (TEST INFRASTRUCTURE).

Nothing new is trusted here: the problem
    minimise 1/2 ||Y_s - X_s B||_F^2 + lambda_int sum_j w_j ||B_j.||_2
is the group lasso on the design kron(X_s, I_m) with the response Y_s.reshape(-1) and p groups of m, so the path is driven by
tests/group_oracle.py's GroupLassoTall (coordinate j m + k is B[j, k]).  What this file adds is the standardisation of several
responses: X by oracle/datastd.py's DataStd as for every solver; every response centred by its own mean (with `intercept`), all of
them divided by ONE scale, DataStd's arithmetic with the sums of squares of all responses added and n m in the place of n
(m = 1: DataStd's scaleY exactly, for the four flag values)."""
import numpy as np

import group_oracle as go
from oracle.datastd import DataStd

F = np.float32


def standardise(x, Y, standardize=True, intercept=True, T=F):
    """-> (Xs (n x p, T, column-major), Ys (n x m, T), std, meanYs (m, T)); std is the DataStd of X with the COMMON scaleY."""
    x = np.asarray(x, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y.reshape(-1, 1)
    n, p = x.shape
    m = Y.shape[1]
    Xs = np.array(x, dtype=T, order="F")
    Ys = np.array(Y, dtype=T, order="F")
    std = DataStd(n, p, standardize, intercept, T)
    if m == 1:                                           # DataStd itself, verbatim
        y0 = Ys[:, 0].copy()
        std.standardize(Xs, y0)
        return Xs, np.asfortranarray(y0.reshape(-1, 1)), std, np.array([std.meanY], dtype=T)
    std.standardize(Xs, Ys[:, 0].copy())                 # X's statistics (the response passed here is a scratch copy)
    A = std.acc or T
    flag = std.flag
    meanYs = np.zeros(m, dtype=T)
    std.meanY, std.scaleY = T(0), T(1)
    if flag != 0:
        ss = A(0)
        for k in range(m):
            mean = T(Ys[:, k].mean(dtype=A))
            if flag == 1:                                # the norm about the mean, without centring (DataStd._sd_n)
                vc = (Ys[:, k] - mean).astype(T)
            else:
                meanYs[k] = mean
                Ys[:, k] -= mean
                vc = Ys[:, k]
            ss = A(ss + (vc.astype(A) ** 2).sum(dtype=A))
        if flag == 1:                                    # _sd_n divides by sqrt(n), standardize() multiplies by its inverse
            scale = T(T(np.sqrt(ss)) / T(np.sqrt(T(n * m))))
        else:
            scale = T(T(np.sqrt(ss)) * T(1.0 / np.sqrt(T(n * m))))
        Ys /= scale
        std.scaleY = scale
        std.meanY = meanYs[0]
    return Xs, Ys, std, meanYs


def kron_problem(Xs, Ys):
    """The group-lasso form: design kron(X_s, I_m) (column-major, like grp_path's X), response Y_s row by row."""
    m = Ys.shape[1]
    K = np.asfortranarray(np.kron(Xs, np.eye(m, dtype=Xs.dtype)))
    return K, np.ascontiguousarray(Ys).reshape(-1).copy()


def mt_path(x, Y, weights=None, lam=None, nlambda=10, lmin_ratio=0.01, standardize=True, intercept=True,
            maxit=10000, eps=1e-5, rho=-1.0, T=F):
    """The lambda path as admm_hip_mtlasso runs it.  Returns a dict: lam, lam_int, beta ((m, p + 1, nlambda), original scale),
    beta_std ((p m) x nlambda in the Kronecker order j m + k), niter, K, yv (the Kronecker problem), sizes, weights, std, meanYs."""
    Xs, Ys, std, meanYs = standardise(x, Y, standardize, intercept, T)
    n, p = Xs.shape
    m = Ys.shape[1]
    w = np.ones(p) if weights is None else np.asarray(weights, dtype=np.float64)
    sizes = [m] * p
    K, yv = kron_problem(Xs, Ys)
    solver = go.GroupLassoTall(K, yv, eps, eps, sizes, w, T)
    if lam is None:
        lmax = np.float64(solver.lambda0) / n * np.float64(std.scaleY)
        lam = np.exp(np.linspace(np.log(lmax), np.log(lmin_ratio * lmax), int(nlambda)))
    lam = np.atleast_1d(np.asarray(lam, dtype=np.float64))
    nl = lam.size
    lam_int = lam * n / np.float64(std.scaleY)
    beta = np.zeros((m, p + 1, nl), dtype=T)
    beta_std = np.zeros((p * m, nl), dtype=T)
    niter = np.zeros(nl, dtype=np.int32)
    for i in range(nl):
        solver.lam_idx = i
        if i == 0:
            solver.init(lam_int[i], rho)
        else:
            solver.init_warm(lam_int[i])
        niter[i] = solver.solve(maxit)
        z = solver.get_coef()
        beta_std[:, i] = z
        for k in range(m):
            std.meanY = meanYs[k]
            b0, coef = std.recover(z.reshape(p, m)[:, k])
            beta[k, 0, i] = b0
            beta[k, 1:, i] = coef
    std.meanY = meanYs[0]
    return dict(lam=lam, lam_int=lam_int, beta=beta, beta_std=beta_std, niter=niter, K=K, yv=yv, sizes=sizes, weights=w, std=std,
                meanYs=meanYs, solver=solver, Xs=Xs, Ys=Ys)


def to_standardised(beta_dense, std):
    """(m, p + 1, nlambda) coefficients on the original scale -> (p m) x nlambda in the solver's units, Kronecker order."""
    b = np.asarray(beta_dense, dtype=np.float64)[:, 1:, :]                        # (m, p, nl)
    b = b * np.asarray(std.scaleX, dtype=np.float64)[None, :, None] / np.float64(std.scaleY)
    m, p, nl = b.shape
    return np.transpose(b, (1, 0, 2)).reshape(p * m, nl)


def synth_mt(n, p, m, seed, nactive=5, sd_noise=1.5):
    """Correlated Gaussian columns, a few active rows shared by all responses, responses of different size and offset."""
    rng = np.random.default_rng(seed)
    shared = rng.standard_normal((n, 1))
    x = rng.standard_normal((n, p)) * (1.0 + rng.uniform(size=p)) + 0.5 * shared + rng.uniform(-2, 2, size=p)
    B = np.zeros((p, m))
    act = rng.choice(p, size=min(nactive, p), replace=False)
    B[act] = rng.standard_normal((act.size, m))
    Y = x @ B + sd_noise * rng.standard_normal((n, m))
    Y = Y * (1.0 + np.arange(m)) + 3.0 * np.arange(m)
    return np.asfortranarray(x), np.asfortranarray(Y)
