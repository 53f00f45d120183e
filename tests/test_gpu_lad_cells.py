"""GPU: the cells of the LAD loop's kernel table (admm_amd/csrc/fadmm_dense.hip, kProxKinds) that no other test file launches.

The rows kernels are selected by (kind, NPT) on the serial one-pass route and by (kind, NPT, S) on the slotted route, NPT = the double2 a
thread holds per row = ceil(round_up(p + intercept, 32) / 1024), S = the slots.  The loss's own test files reach all 42 serial cells (the
one-pass BRANCHES shape and the five LAYOUTS of tests/test_gpu_quantreg.py, on every kind) and 46 of the 61 slotted ones: NPT = 1 with
S = 2, 3, 4 and, on the LAYOUTS, S = 2 (quantile, Huber), the layout's largest S and 2 (logit-multi, logit-ridge) or the layout's
largest, 2 and 4 clipped (logit-enet, Poisson).  The 15 cells below are the rest.  Each runs at the smallest shape that selects it:
p + 1 = 1024 (NPT - 1) + 1 columns with the ones column, LAD_HAT=0 so that n <= 2000 does not take the hat-matrix branch, n = p + 40
rows where the call needs n > p + 1 and 64 data rows where the penalty rows make up the rank.  S + 1 fits, so that a slot refills;
MAXIT iterations -- the comparison needs no convergence.

Asserted per cell: the slotted route ran (xupdate_variant == 8 + S) and its coefficients and iteration counts are those of the serial
route (QUANT_SLOTS=1, xupdate_variant == 1) of the same call, byte for byte."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAXIT = 30
# kind -> {NPT: the S that no other file launches}
CELLS = {"quantreg": {2: (3, 4), 3: (3, 4), 4: (3,)},
         "huber": {2: (3, 4), 3: (3, 4)},
         "logit_multi": {2: (3,), 3: (3,)},
         "logit_ridge": {2: (3,), 3: (3,)},
         "logit_enet": {2: (3,)},
         "poisson": {2: (3,)}}
PENALTY_ROWS = ("logit_ridge", "logit_enet", "poisson")

_cache = {}


def _npt(p):
    return ((p + 1 + 31) // 32 * 32 // 2 + 511) // 512


def _problem(kind, npt):
    """-> (x, Y): p = 1024 (NPT - 1) columns; Y: five columns (responses are used one at a time, labels and counts as a matrix)"""
    p = 1024 * (npt - 1)
    n = 64 if kind in PENALTY_ROWS else p + 40
    key = ("problem", n, p)
    if key not in _cache:
        rng = np.random.default_rng(7 * npt + n)
        x = np.asfortranarray(rng.standard_normal((n, p)))
        eta = x[:, :8] @ rng.uniform(0.5, 1.0, size=8)
        _cache[key] = (x, eta, rng.integers(0, 2 ** 31))
    x, eta, seed = _cache[key]
    rng = np.random.default_rng(seed)
    if kind in ("quantreg", "huber"):
        return x, eta + rng.standard_t(3, size=n)
    if kind == "poisson":
        return x, np.asfortranarray(rng.poisson(np.exp(0.3 * eta[:, None] / np.abs(eta).max() + 0.5), size=(n, 5)).astype(np.float64))
    Y = (rng.uniform(size=(n, 5)) < 1.0 / (1.0 + np.exp(-eta[:, None] / np.abs(eta).max()))).astype(np.float64)
    Y[0], Y[1] = 0.0, 1.0                                   # both classes in every column
    return x, np.asfortranarray(Y)


def _fit(kind, x, Y, nfit, slots):
    import admm_amd
    from admm_amd import options
    with options(LAD_HAT="0", QUANT_SLOTS=slots):
        if kind == "quantreg":
            m = admm_amd.admm_quantreg(x, Y, (0.2, 0.7, 0.45, 0.9, 0.5)[:nfit])
        elif kind == "huber":
            m = admm_amd.admm_huber(x, Y, (1.345, 0.8, np.inf, 2.0, 1.345)[:nfit], (0.5, 0.3, 0.7, 0.5, 0.2)[:nfit])
        elif kind == "logit_multi":
            m = admm_amd.admm_logit_multi(x, Y[:, :nfit])
        elif kind == "logit_ridge":
            m = admm_amd.admm_logit_ridge(x, Y[:, :nfit], 1.0)
        elif kind == "logit_enet":
            m = admm_amd.admm_logit_enet(x, Y[:, :nfit], 2.0, alpha=0.5)
        else:
            m = admm_amd.admm_poisson(x, Y[:, :nfit], 2.0, alpha=0.5)
        return m.opts(maxit=MAXIT).fit()


def _serial(kind, npt, nfit):
    key = ("serial", kind, npt, nfit)
    if key not in _cache:
        f = _fit(kind, *_problem(kind, npt), nfit, 1)
        assert f.stats["xupdate_variant"] == 1
        _cache[key] = (f.beta.copy(), f.niter.copy())
    return _cache[key]


def _cases():
    for kind, by_npt in CELLS.items():
        for npt, slots in by_npt.items():
            for s in slots:
                yield pytest.param(kind, npt, s, id=f"{kind}-npt{npt}-slots{s}")


@pytest.mark.parametrize("kind,npt,slots", list(_cases()))
def test_a_slotted_cell_is_byte_identical_to_the_serial_route(kind, npt, slots):
    x, Y = _problem(kind, npt)
    assert _npt(x.shape[1]) == npt
    beta1, niter1 = _serial(kind, npt, slots + 1)
    fit = _fit(kind, x, Y, slots + 1, slots)
    assert fit.stats["xupdate_variant"] == 8 + slots
    assert fit.niter.tobytes() == niter1.tobytes() and fit.beta.tobytes() == beta1.tobytes()
    assert np.all(np.isfinite(fit.beta)) and np.any(fit.beta != 0.0)
