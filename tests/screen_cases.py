"""Problems whose columns sit ON the threshold of a regular step, with a rounding error of the screen's copy that is parallel to the
vector the screen multiplies by -- the only place where the safe screens' bound s_j decides anything (tests/test_gpu_screen_threshold.py
on the GPU, tests/test_screen_threshold_host.py the same counts from the oracle alone).

Wide Lasso / elastic net (standardize = intercept = False, one user lambda, user rho): step 0 has t = 0, steps 1 and 2 are active-set steps
on an empty support, so at the regular step 3 x is still zero and t = c Y with c a function of rho alone.  Sharing basis pursuit: x stays
zero through step 9, so at the regular step 10 v = -11 b / N.  A special column is X_j = C_j + alpha_j kappa w with C_j exactly
representable in the copy format (the copy IS C_j), kappa = 0.49 ulp of that format, |w_i| <= 1 parallel to Y (to b), alpha_j laddered
over [0.3, 0.98], and C_j chosen so that X_j'Y = T0 up to one step of the format's grid: with lambda set to put the threshold at |c| T0
every special column is within that step of its threshold, its copy's product is below it by alpha_j kappa w'Y, and Cauchy-Schwarz is
tight -- |copy_j't| + ||X_j - C_j|| ||t|| reaches the threshold to the same step.  A bound 10 % too small then zeroes columns the exact
step keeps."""
import numpy as np

F = np.float32
P, NSPECIAL = 2000, 400
RHO = 0.05
ENET_ALPHA = 0.6
U24 = 2.0 ** -24


def _on_threshold_columns(rng, u, w, grid, lo, hi, T0, kappa, alphas, row0=None):
    """Columns C_j + alpha_j kappa w (float64) and the C_j: entries of C_j are +-(k grid), k an integer in [lo, hi], the signs and then
    single grid steps chosen greedily so that C_j'u = T0 - alpha_j kappa w'u as nearly as the grid allows; row0: the value of row 0
    (where u must be 0)."""
    n = len(u)
    C = np.zeros((n, len(alphas)))
    for j, a in enumerate(alphas):
        k = rng.integers(lo + (hi - lo) // 4, hi - (hi - lo) // 4, n).astype(np.float64)      # the middle of the range: room for the steps
        sgn = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        if row0 is not None:
            k[0], sgn[0] = row0 / grid, 1.0
        target = T0 - a * kappa * float(w @ u)
        cur = float((sgn * k * grid) @ u)
        for i in rng.permutation(n):                        # signs: to within one entry's weight
            new = cur - 2.0 * sgn[i] * k[i] * grid * u[i]
            if u[i] != 0 and abs(new - target) < abs(cur - target):
                sgn[i], cur = -sgn[i], new
        for _ in range(200):                                # single grid steps: to within half a step of the lightest entry
            moved = False
            for i in rng.permutation(n):
                if u[i] == 0:
                    continue
                step = 1.0 if (target - cur) * sgn[i] * u[i] > 0 else -1.0
                new = cur + step * sgn[i] * grid * u[i]
                if lo <= k[i] + step <= hi and abs(new - target) < abs(cur - target):
                    k[i], cur, moved = k[i] + step, new, True
            if not moved:
                break
        C[:, j] = sgn * k * grid
    return C + np.asarray(alphas)[None, :] * kappa * w[:, None], C


def fp16_copy(X):
    """what the fp16 screens multiply by, in float64 (a rounding that is not finite is stored as zero)"""
    with np.errstate(all="ignore"):
        h = np.asarray(X, dtype=F).astype(np.float16).astype(np.float64)
    h[~np.isfinite(h)] = 0.0
    return h


def code8_copy(X):
    """scale_j q_ij of the 8-bit code, in float64: q = round(x / scale) in [-127, 127], scale = max|x| / 127 in float"""
    X = np.asarray(X, dtype=F)
    sc = (np.abs(X).max(axis=0) / F(127)).astype(F)
    with np.errstate(all="ignore"):
        q = np.where(sc > 0, np.clip(np.rint(X / sc), -127, 127), 0.0)
    return sc.astype(np.float64) * q


def wide_t3(Y, rho):
    """t before the regular step 3 while x is zero, in the reference's float arithmetic (ADMMBase::solve: z = (Y + y + rho A x) / (-1 - rho),
    y += rho (A x + z); t = A x + z + y / rho)"""
    Y = np.asarray(Y, dtype=F)
    z, y = np.zeros_like(Y), np.zeros_like(Y)
    for _ in range(3):
        z = ((Y + y) / F(-1 - rho)).astype(F)
        y = (y + F(rho) * z).astype(F)
    return (z + y / F(rho)).astype(F)


_CASES = {}


def wide_case(n, fmt, enet):
    """dict: x (n x P float64 holding float values), y, lambda (user units), rho, alpha, special (bool [P]), C (the special columns' copies),
    c, T0, threshold (on |X_j't|)."""
    key = ("wide", n, fmt, enet)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(7000 + 10 * n + fmt + (1 if enet else 0))
    Y = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 1.0, n)).astype(F)
    Y[0] = 0
    Y64 = Y.astype(np.float64)
    T0 = 2.3 * np.sqrt(n)
    alphas = np.linspace(0.3, 0.98, NSPECIAL)
    if fmt == 16:        # entries +-[1, 2): one ulp is 2^-10 throughout
        grid = 2.0 ** -10
        Xs, C = _on_threshold_columns(rng, Y64, Y64, grid, 1024, 2047, T0, 0.49 * grid, alphas)
    else:                # integers times 2^-6, row 0 = 127 * 2^-6 pins the column maximum: scale = 2^-6 exactly
        grid = 2.0 ** -6
        Xs, C = _on_threshold_columns(rng, Y64, Y64, grid, 1, 126, T0, 0.49 * grid, alphas, row0=127 * grid)
    Xs = Xs.astype(F)
    assert np.array_equal((fp16_copy if fmt == 16 else code8_copy)(Xs), C), "the copy of a special column must be its C_j"
    X = rng.standard_normal((n, P)).astype(F)
    special = np.zeros(P, bool)
    special[rng.permutation(P)[:NSPECIAL]] = True
    X[:, special] = Xs
    t = wide_t3(Y, RHO).astype(np.float64)
    c = float(t @ Y64) / float(Y64 @ Y64)
    thr = abs(c) * T0
    lam_internal = RHO * thr / (ENET_ALPHA if enet else 1.0)
    case = dict(x=np.asfortranarray(X.astype(np.float64)), y=Y64.copy(), lam=lam_internal / n, rho=RHO, alpha=ENET_ALPHA if enet else None, special=special,
                C=C, c=c, T0=T0, threshold=thr, n=n, fmt=fmt)
    _CASES[key] = case
    return case


def wide_problem(case, maxit):
    """the oracle's arguments"""
    from oracle import entry
    return dict(x=case["x"], y=case["y"], lam=[case["lam"]], nlambda=1, lmin_ratio=0.01, standardize=False, intercept=False,
                opts=dict(entry.LASSO_OPTS, maxit=maxit, rho=case["rho"]), alpha=case["alpha"])


def wide_G(lam_f, rho, gamma_f, alpha):
    """the screen's right-hand side gamma * threshold * (1 - 4.8e-7) as wide_x_kernel forms it (lam, gamma floats; elastic net: the float threshold)"""
    pen_d = np.float64(F(lam_f)) / (np.float64(rho) * np.float64(F(gamma_f)))
    thr = pen_d if alpha is None else np.float64(F(np.float64(F(alpha)) * pen_d))
    return float(np.float64(F(gamma_f)) * thr * (1.0 - 4.8e-7))


def screen_populations(X64, copy64, t64, G, gamma_term, special, nonzero_after):
    """In float64, with the copy the screen reads: `saved` = special columns the exact step made non-zero although |copy_j't| <= G (only
    s_j keeps the screen off them), `stay` = special columns that stay zero, `nonzero` = all non-zero columns, `may_be_exact` = columns
    that violate |copy_j't| + s2_j ||t|| <= G with the gamma term of s_j DOUBLED (that extra term is the float product's own worst-case
    rounding: a column that passes with so much room is screened whatever the order of the float sums) and s_j at the upper end
    (1 + 1.2e-6) of what the setup kernel may return."""
    prod = np.abs(copy64.T @ t64)
    e = np.sqrt(((X64 - copy64) ** 2).sum(axis=0))
    big = np.sqrt(np.maximum((X64 ** 2).sum(axis=0), (copy64 ** 2).sum(axis=0)))
    s2 = (e + 2.0 * gamma_term * big) * (1 + 1.2e-6)
    tn = float(np.sqrt(t64 @ t64)) * (1 + 1e-12)
    nz = np.asarray(nonzero_after, bool)
    return dict(saved=int((special & nz & (prod <= G)).sum()), stay=int((special & ~nz).sum()), nonzero=int(nz.sum()),
                may_be_exact=int((prod + s2 * tn > G).sum()), special_nonzero=int((special & nz).sum()),
                copy_above=int((special & nz & (prod > G)).sum()))


def wide_populations(case, t3, x_after3, lam_f, gamma_f):
    X64 = case["x"]
    copy = (fp16_copy if case["fmt"] == 16 else code8_copy)(X64)
    G = wide_G(lam_f, case["rho"], gamma_f, case["alpha"])
    return screen_populations(X64, copy, np.asarray(t3, dtype=np.float64), G, 2.0 * 1.001 * case["n"] * U24, case["special"], np.asarray(x_after3) != 0)


def sbp_case(n, N):
    """dict: A (n x P float64), b, N, rho (the oracle's), special, v (before the regular step 10), T0."""
    key = ("sbp", n, N)
    if key in _CASES:
        return _CASES[key]
    from oracle.solvers import SharingBP
    rng = np.random.default_rng(9000 + 10 * n + N)
    u = np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 1.0, n)
    w = u / np.abs(u).max()
    T0 = 2.3 * np.sqrt(n)
    grid = 2.0 ** -10
    Xs, C = _on_threshold_columns(rng, u, w, grid, 1024, 2047, T0, 0.49 * grid, np.linspace(0.3, 0.98, NSPECIAL))
    assert np.array_equal(fp16_copy(Xs), C), "the copy of a special column must be its C_j"
    A = rng.standard_normal((n, P))
    special = np.zeros(P, bool)
    special[rng.permutation(P)[:NSPECIAL]] = True
    A[:, special] = Xs
    A = np.asfortranarray(A)
    s = SharingBP(A, u, N, 1e-4, 1e-4)
    s.init(1.0)
    b = u * (N / (11.0 * s.rho * T0))                       # 11 T0 / N = 1 / rho: the special columns' |A_j'v| on the threshold
    case = dict(A=A, b=b, N=N, rho=s.rho, special=special, C=C, T0=T0, n=n, v=-11.0 * b / N)
    _CASES[key] = case
    return case


def sbp_populations(case, rho):
    """as screen_populations, from v = -11 b / N and the threshold 1 / rho on |A_j'v|; `nonzero`: columns beyond the threshold by more than
    the rounding of a double inner product (1e-12 relative: n 2^-53 ||A_j|| ||v|| is below 1e-12 |A_j'v| for these columns), `near`: the others
    within that band (either outcome is the exact step's)."""
    A, v, n = case["A"], case["v"], case["n"]
    thr = 1.0 / rho
    prod = np.abs(A.T @ v)
    nz, near = prod > thr * (1 + 1e-12), np.abs(prod - thr) <= thr * 1e-12
    pops = screen_populations(A, fp16_copy(A), v, thr * (1.0 - 1e-9), 1.01 * (n + 4.0) * U24, case["special"], nz)
    pops["stay"] = int((case["special"] & ~nz & ~near).sum())
    pops["near"] = int(near.sum())
    pops["may_be_nonzero"] = nz | near
    return pops
