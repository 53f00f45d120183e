"""GPU: quantile regression (admm_hip_quantreg) -- the asymmetric prox through the three LAD branches, and the slotted loop that advances
several quantiles per pass over X (quant_rows_kernel, quant_head_kernel) held bit-identical to the same quantiles fitted alone.
The CPU restatement, the LP and the replay are tests/quantile_oracle.py."""
import numpy as np
import pytest

import quantile_oracle as qo
from helpers import dense_state_records

pytestmark = pytest.mark.gpu

OPTS = {"maxit": 10000, "eps_abs": 1e-4, "eps_rel": 1e-4, "rho": 1.0}
# (n, p, seed, LAD_ONEPASS): the hat-matrix branch (n <= 2000), the one-pass branch, the two-pass branch
BRANCHES = {"hat": (400, 8, 1, None), "onepass": (2100, 40, 2, None), "twopass": (2100, 40, 2, "0")}
# the LAD test's shapes: 2 ... 6 double2 per thread and row (with the ones column), ragged row runs
LAYOUTS = [(2600, 1100, 60), (4100, 2300, 30), (4300, 3300, 25), (5203, 4200, 25), (6200, 5300, 20)]
GRID = (0.9, 0.1, 0.5, 0.25, 0.5, 0.75, 0.05)

_cache = {}


def _data(n, p, seed):
    key = ("data", n, p, seed)
    if key not in _cache:
        _cache[key] = qo.issue_data(n, p, seed)
    return _cache[key]


def _layout_data(n, p):
    key = ("layout", n, p)
    if key not in _cache:
        rng = np.random.default_rng(100 + p)
        x = rng.standard_normal((n, p)) * 2 + 0.3
        b = rng.uniform(size=p) / np.sqrt(p)
        _cache[key] = (x, x @ b + rng.standard_t(3, size=n) * (1 + 0.3 * np.abs(x[:, 0])) + 1.5)
    return _cache[key]


def _lp(n, p, seed, tau, intercept):
    key = ("lp", n, p, seed, tau, intercept)
    if key not in _cache:
        _cache[key] = qo.quantile_lp(*_data(n, p, seed), tau, intercept)
    return _cache[key]


def _fit(x, y, tau, intercept=True, maxit=10000, trace=False, state=0, **opt):
    from admm_amd import admm_quantreg, options
    with options(**opt):
        return admm_quantreg(x, y, tau, intercept=intercept).opts(maxit=maxit).fit(trace=trace, state=state)


def _single(tag, x, y, tau, maxit):
    """tau fitted alone (one loop on the one-pass branch's serial route), shared by the slot tests"""
    key = ("single", tag, tau, maxit)
    if key not in _cache:
        f = _fit(x, y, tau, maxit=maxit)
        assert f.stats["xupdate_variant"] == 1
        _cache[key] = (f.beta[:, 0].copy(), int(f.niter[0]))
    return _cache[key]


@pytest.mark.parametrize("branch", list(BRANCHES))
def test_median_without_intercept_is_lad_bit_for_bit(branch):
    from admm_amd import admm_lad, options
    n, p, seed, onepass = BRANCHES[branch]
    x, y = _data(n, p, seed)
    nst = dense_state_records(n, 10000)
    with options(LAD_ONEPASS=onepass):
        lad = admm_lad(x, y, intercept=False).fit(trace=True, state=nst)
    q = _fit(x, y, 0.5, intercept=False, trace=True, state=nst, LAD_ONEPASS=onepass)
    assert q.stats["xupdate_variant"] == lad.stats["xupdate_variant"] == (1 if branch == "onepass" else 0)
    assert q.beta.shape == (p + 1, 1) and q.tau.tolist() == [0.5]
    assert int(q.niter[0]) == lad.niter
    assert np.array_equal(q.beta[:, 0], lad.beta)
    assert np.array_equal(q.trace, lad.trace)
    assert np.array_equal(q.state, lad.state)


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("tau", [0.1, 0.9])
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_other_quantiles_against_the_restatement_and_the_lp(branch, tau, intercept):
    n, p, seed, onepass = BRANCHES[branch]
    x, y = _data(n, p, seed)
    label = f"{branch} n={n} p={p} tau={tau} icpt={int(intercept)}"
    fit = _fit(x, y, tau, intercept=intercept, trace=True, state=dense_state_records(n, 10000), LAD_ONEPASS=onepass)
    beta = fit.beta[:, 0]
    rep = qo.followed(beta, fit.niter[0], fit.trace, x, y, tau, intercept, OPTS, tol=1e-8, label=label)
    print(f"[quantreg {label}] near-ties: {len(rep['forced'])}")
    qo.replay(fit.trace, fit.state, tau, label=label)
    _, best = _lp(n, p, seed, tau, intercept)
    excess = qo.check_loss(x, y, beta, tau) / best - 1.0
    frac = qo.neg_fraction(x, y, beta)
    print(f"[quantreg {label}] niter {int(fit.niter[0])}, objective +{excess:.2e} over the LP, negative residuals {frac:.4f}")
    assert -1e-9 <= excess <= 1e-3
    if intercept:
        assert abs(frac - tau) <= 0.01
    else:
        assert beta[0] == 0.0


@pytest.mark.parametrize("n,p,maxit", LAYOUTS)
def test_every_register_layout_of_the_rows_kernel_with_the_asymmetric_prox(n, p, maxit):
    x, y = _layout_data(n, p)
    label = f"layout n={n} p={p} tau=0.2"
    fit = _fit(x, y, 0.2, maxit=maxit, trace=True, state=dense_state_records(n, maxit))
    assert fit.stats["xupdate_variant"] == 1
    qo.followed(fit.beta[:, 0], fit.niter[0], fit.trace, x, y, 0.2, True, dict(OPTS, maxit=maxit), tol=1e-8, label=label)
    assert qo.replay(fit.trace, fit.state, 0.2, label=label) >= maxit - 1


@pytest.mark.parametrize("maxit", [10000, 400])
@pytest.mark.parametrize("slots", [2, 3, 4])
def test_slots_equal_single_runs(slots, maxit):
    """Seven quantiles, unsorted, one of them twice.  Default maxit: all converge, at different iterations, so the slots refill at
    different times; maxit = 400: some converge and some run out of iterations."""
    n, p, seed, _ = BRANCHES["onepass"]
    x, y = _data(n, p, seed)
    key = ("serial grid", maxit)
    if key not in _cache:
        _cache[key] = _fit(x, y, GRID, maxit=maxit, QUANT_SLOTS=1)
    serial = _cache[key]
    assert serial.stats["xupdate_variant"] == 1
    fit = _fit(x, y, GRID, maxit=maxit, QUANT_SLOTS=slots)
    assert fit.stats["xupdate_variant"] == 8 + slots
    assert fit.beta.shape == (p + 1, len(GRID))
    print(f"[quantreg slots={slots} maxit={maxit}] niter {fit.niter.tolist()}")
    for k, tau in enumerate(GRID):
        beta1, niter1 = _single("onepass", x, y, tau, maxit)
        assert int(fit.niter[k]) == niter1 == int(serial.niter[k]), (k, tau, fit.niter[k], niter1, serial.niter[k])
        assert np.array_equal(fit.beta[:, k], beta1), (k, tau)
        assert np.array_equal(fit.beta[:, k], serial.beta[:, k]), (k, tau)
    assert np.array_equal(fit.beta[:, 2], fit.beta[:, 4]) and fit.niter[2] == fit.niter[4]
    if maxit == 400:
        assert (fit.niter == maxit + 1).any() and (fit.niter <= maxit).any()
    else:
        assert (fit.niter <= maxit).all() and len(set(fit.niter.tolist())) >= 4


@pytest.mark.parametrize("n,p,maxit", LAYOUTS)
def test_slots_on_every_register_layout(n, p, maxit):
    """Nothing converges within the small maxit: the first two quantiles finish in the same iteration (two slots refill at once: one
    takes the third quantile, the other goes idle).  Six double2 per thread and row leave no registers for a second slot: serial."""
    x, y = _layout_data(n, p)
    taus = (0.2, 0.7, 0.45)
    fit = _fit(x, y, taus, maxit=maxit, QUANT_SLOTS=2)
    assert fit.stats["xupdate_variant"] == (10 if p + 1 <= 5120 else 1)
    assert fit.niter.tolist() == [maxit + 1] * 3
    for k, tau in enumerate(taus):
        beta1, niter1 = _single(("layout", n, p), x, y, tau, maxit)
        assert niter1 == maxit + 1
        assert np.array_equal(fit.beta[:, k], beta1), (n, p, tau)


@pytest.mark.parametrize("branch", ["hat", "twopass"])
def test_grid_on_the_other_branches_equals_single_runs(branch):
    n, p, seed, onepass = BRANCHES[branch]
    x, y = _data(n, p, seed)
    taus = (0.8, 0.3, 0.5)
    fit = _fit(x, y, taus, QUANT_SLOTS=4, LAD_ONEPASS=onepass)
    assert fit.stats["xupdate_variant"] == 0
    for k, tau in enumerate(taus):
        one = _fit(x, y, tau, LAD_ONEPASS=onepass)
        assert int(fit.niter[k]) == int(one.niter[0])
        assert np.array_equal(fit.beta[:, k], one.beta[:, 0])


def test_slot_corners():
    n, p, seed, _ = BRANCHES["onepass"]
    x, y = _data(n, p, seed)
    one = _fit(x, y, 0.3, QUANT_SLOTS=4)
    assert one.stats["xupdate_variant"] == 1                     # a single tau runs the serial route
    two = _fit(x, y, (0.3, 0.6), QUANT_SLOTS=4)
    assert two.stats["xupdate_variant"] == 10                    # two quantiles: two slots
    assert np.array_equal(two.beta[:, 0], one.beta[:, 0]) and two.niter[0] == one.niter[0]
    a = _fit(x, y, GRID, QUANT_SLOTS=3)
    b = _fit(x, y, GRID, QUANT_SLOTS=3)
    assert a.beta.tobytes() == b.beta.tobytes() and a.niter.tobytes() == b.niter.tobytes()
