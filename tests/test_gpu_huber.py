"""GPU: Huber / expectile regression (admm_hip_huber) -- the Huber form of the prox through the three LAD branches and every register
layout of the rows kernel, and the slotted loop (quant_rows_kernel's Huber instantiations, quant_head_kernel's refill) held bit-identical
to the same (delta, tau) pairs fitted alone.  The CPU restatement, the IRLS optimum and the replay are tests/huber_oracle.py; shapes
are those of tests/test_gpu_quantreg.py: the smallest that reach each branch and each layout.

Bounds: the follow tolerance 1e-8 is the loop's (tests/test_gpu_quantreg.py); the objective's excess over IRLS is capped at 1e-4, where
the restatement's measured worst case on these inputs is 1.07e-5 (tests/test_huber_host.py); least squares within 1e-8 (the restatement
is within 5e-15 of lstsq, the library follows the restatement within 1e-8)."""
import numpy as np
import pytest

import huber_oracle as ho
from helpers import dense_state_records
from test_gpu_quantreg import BRANCHES, LAYOUTS, _data, _layout_data

pytestmark = pytest.mark.gpu

OPTS = {"maxit": 10000, "eps_abs": 1e-4, "eps_rel": 1e-4, "rho": 1.0}
INF = float("inf")
PAIRS = [(0.5, 1.345), (0.2, 0.3), (0.9, INF)]                     # (tau, delta)
# (delta, tau), unsorted, one pair twice; restated iteration counts with the intercept: 16, 10, 50, 20, 16, 24, 31
GRID = [(0.3, 0.5), (INF, 0.5), (0.3, 0.9), (1.345, 0.2), (0.3, 0.5), (5.0, 0.2), (1.345, 0.9)]

_cache = {}


def huber_max_slots(cols):
    """The Huber instantiations of quant_rows_kernel that compile without scratch (fadmm_dense.hip, kProxKinds[kProxHuber].max_slots): by the double2
    a thread holds per row, 4 slots up to 3, 2 up to 5 (3 at 4 spilled and fell away), none beside the first at 6."""
    npt = ((cols + 31) // 32 * 32 // 2 + 511) // 512
    return 4 if npt <= 3 else (2 if npt <= 5 else 1)


def _fit(x, y, delta, tau, intercept=True, maxit=10000, trace=False, state=0, **opt):
    from admm_amd import admm_huber, options
    with options(**opt):
        return admm_huber(x, y, delta, tau, intercept=intercept).opts(maxit=maxit).fit(trace=trace, state=state)


def _single(tag, x, y, delta, tau, maxit):
    """one pair fitted alone (one loop on the one-pass branch's serial route), shared by the slot tests"""
    key = ("single", tag, delta, tau, maxit)
    if key not in _cache:
        f = _fit(x, y, delta, tau, maxit=maxit)
        assert f.stats["xupdate_variant"] == 1
        _cache[key] = (f.beta[:, 0].copy(), int(f.niter[0]))
    return _cache[key]


def _irls(n, p, seed, delta, tau, intercept):
    key = ("irls", n, p, seed, delta, tau, intercept)
    if key not in _cache:
        _cache[key] = ho.huber_irls(*_data(n, p, seed), delta, tau, intercept)
    return _cache[key]


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("tau,delta", PAIRS)
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_three_branches_against_the_restatement_and_irls(branch, tau, delta, intercept):
    n, p, seed, onepass = BRANCHES[branch]
    x, y = _data(n, p, seed)
    label = f"{branch} n={n} p={p} tau={tau} delta={delta} icpt={int(intercept)}"
    fit = _fit(x, y, delta, tau, intercept=intercept, trace=True, state=dense_state_records(n, 10000), LAD_ONEPASS=onepass)
    assert fit.stats["xupdate_variant"] == (1 if branch == "onepass" else 0)
    assert fit.beta.shape == (p + 1, 1) and fit.delta.tolist() == [delta] and fit.tau.tolist() == [tau]
    beta = fit.beta[:, 0]
    ho.followed(beta, fit.niter[0], fit.trace, x, y, delta, tau, intercept, OPTS, tol=1e-8, label=label)
    assert ho.replay(fit.trace, fit.state, delta / ho.scale_y(x, y, intercept), tau, label=label) >= 8
    _, best = _irls(n, p, seed, delta, tau, intercept)
    excess = ho.huber_loss(x, y, beta, delta, tau) / best - 1.0
    print(f"[huber {label}] niter {int(fit.niter[0])}, objective +{excess:.2e} over IRLS")
    assert -1e-9 <= excess <= 1e-4
    if not intercept:
        assert beta[0] == 0.0


@pytest.mark.parametrize("intercept", [True, False])
def test_tau_half_delta_inf_is_least_squares(intercept):
    n, p, seed, _ = BRANCHES["onepass"]
    x, y = _data(n, p, seed)
    fit = _fit(x, y, INF, 0.5, intercept=intercept)
    assert fit.stats["xupdate_variant"] == 1
    A = np.hstack([np.ones((n, 1)), x]) if intercept else x
    b = np.linalg.lstsq(A, y, rcond=None)[0]
    ref = b if intercept else np.concatenate([[0.0], b])
    err = float(np.max(np.abs(fit.beta[:, 0] - ref)) / np.max(np.abs(ref)))
    print(f"[huber = lstsq icpt={int(intercept)}] niter {int(fit.niter[0])}, err {err:.2e}")
    assert err <= 1e-8


@pytest.mark.parametrize("n,p,maxit", LAYOUTS)
def test_every_register_layout_of_the_rows_kernel_with_the_huber_prox(n, p, maxit):
    x, y = _layout_data(n, p)
    label = f"layout n={n} p={p} tau=0.2 delta=1.345"
    fit = _fit(x, y, 1.345, 0.2, maxit=maxit, trace=True, state=dense_state_records(n, maxit))
    assert fit.stats["xupdate_variant"] == 1
    ho.followed(fit.beta[:, 0], fit.niter[0], fit.trace, x, y, 1.345, 0.2, True, dict(OPTS, maxit=maxit), tol=1e-8, label=label)
    assert ho.replay(fit.trace, fit.state, 1.345 / ho.scale_y(x, y, True), 0.2, label=label) >= 8


@pytest.mark.parametrize("maxit", [10000, 18])
@pytest.mark.parametrize("slots", [2, 3, 4])
def test_slots_equal_single_runs(slots, maxit):
    """Seven pairs, unsorted, one of them twice.  Default maxit: all converge, at different iterations, so the slots refill at different
    times; maxit = 18: some converge and some run out of iterations (no restated count is 17, 18 or 19: no near tie flips the split)."""
    n, p, seed, _ = BRANCHES["onepass"]
    x, y = _data(n, p, seed)
    deltas, taus = [d for d, _ in GRID], [t for _, t in GRID]
    key = ("serial grid", maxit)
    if key not in _cache:
        _cache[key] = _fit(x, y, deltas, taus, maxit=maxit, QUANT_SLOTS=1)
    serial = _cache[key]
    assert serial.stats["xupdate_variant"] == 1
    fit = _fit(x, y, deltas, taus, maxit=maxit, QUANT_SLOTS=slots)
    assert fit.stats["xupdate_variant"] == 8 + slots
    assert fit.beta.shape == (p + 1, len(GRID))
    print(f"[huber slots={slots} maxit={maxit}] niter {fit.niter.tolist()}")
    for k, (delta, tau) in enumerate(GRID):
        beta1, niter1 = _single("onepass", x, y, delta, tau, maxit)
        assert int(fit.niter[k]) == niter1 == int(serial.niter[k]), (k, delta, tau, fit.niter[k], niter1, serial.niter[k])
        assert np.array_equal(fit.beta[:, k], beta1), (k, delta, tau)
        assert np.array_equal(fit.beta[:, k], serial.beta[:, k]), (k, delta, tau)
    assert np.array_equal(fit.beta[:, 0], fit.beta[:, 4]) and fit.niter[0] == fit.niter[4]
    if maxit == 18:
        assert (fit.niter == maxit + 1).any() and (fit.niter <= maxit).any()
    else:
        assert (fit.niter <= maxit).all() and len(set(fit.niter.tolist())) >= 4


@pytest.mark.parametrize("n,p,maxit", LAYOUTS)
def test_slots_on_every_register_layout(n, p, maxit):
    """Three pairs on two slots: whichever slot finishes first takes the third pair.  Six double2 per thread and row leave no
    registers for a second slot: serial."""
    x, y = _layout_data(n, p)
    pairs = [(1.345, 0.2), (0.4, 0.7), (INF, 0.45)]
    fit = _fit(x, y, [d for d, _ in pairs], [t for _, t in pairs], maxit=maxit, QUANT_SLOTS=2)
    assert fit.stats["xupdate_variant"] == (8 + 2 if huber_max_slots(p + 1) >= 2 else 1)
    for k, (delta, tau) in enumerate(pairs):
        beta1, niter1 = _single(("layout", n, p), x, y, delta, tau, maxit)
        assert int(fit.niter[k]) == niter1
        assert np.array_equal(fit.beta[:, k], beta1), (n, p, delta, tau)


@pytest.mark.parametrize("branch", ["hat", "twopass"])
def test_grid_on_the_other_branches_equals_single_runs(branch):
    n, p, seed, onepass = BRANCHES[branch]
    x, y = _data(n, p, seed)
    pairs = [(0.3, 0.8), (INF, 0.3), (1.345, 0.5)]
    fit = _fit(x, y, [d for d, _ in pairs], [t for _, t in pairs], QUANT_SLOTS=4, LAD_ONEPASS=onepass)
    assert fit.stats["xupdate_variant"] == 0
    for k, (delta, tau) in enumerate(pairs):
        one = _fit(x, y, delta, tau, LAD_ONEPASS=onepass)
        assert int(fit.niter[k]) == int(one.niter[0])
        assert np.array_equal(fit.beta[:, k], one.beta[:, 0])


def test_automatic_slots_are_what_the_layout_admits_and_equal_the_serial_route():
    """QUANT_SLOTS=0 (the default): measured fastest at every layout (profiles/huber_loss.md), so the grid takes as many slots as the
    Huber table admits; two fits take two."""
    n, p, seed, _ = BRANCHES["onepass"]
    x, y = _data(n, p, seed)
    deltas, taus = [d for d, _ in GRID], [t for _, t in GRID]
    auto = _fit(x, y, deltas, taus)
    serial = _fit(x, y, deltas, taus, QUANT_SLOTS=1)
    assert auto.stats["xupdate_variant"] == 8 + huber_max_slots(p + 1) and serial.stats["xupdate_variant"] == 1
    assert np.array_equal(auto.beta, serial.beta) and np.array_equal(auto.niter, serial.niter)
    assert _fit(x, y, deltas[:2], taus[:2]).stats["xupdate_variant"] == 10
    assert _fit(x, y, deltas, taus, LAD_ONEPASS="0").stats["xupdate_variant"] == 0


def test_slot_corners():
    n, p, seed, _ = BRANCHES["onepass"]
    x, y = _data(n, p, seed)
    one = _fit(x, y, 0.3, 0.3, QUANT_SLOTS=4)
    assert one.stats["xupdate_variant"] == 1                     # a single pair runs the serial route
    deltas, taus = [d for d, _ in GRID], [t for _, t in GRID]
    a = _fit(x, y, deltas, taus, QUANT_SLOTS=3)
    b = _fit(x, y, deltas, taus, QUANT_SLOTS=3)
    assert a.beta.tobytes() == b.beta.tobytes() and a.niter.tobytes() == b.niter.tobytes()
