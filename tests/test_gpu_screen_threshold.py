"""Columns that only the bound saves: the safe screens of the wide Lasso / elastic net (wide_x_kernel, fp16 copy and 8-bit code) and of
the sharing basis pursuit (sbp_xreg_screen_kernel) on the problems of screen_cases.py, where 400 columns sit on the threshold of the
first regular step with a non-zero right-hand side, the product with their copy is below it, and the copy's rounding error is parallel to
the vector they are multiplied by -- so that |copy_j't| + s_j ||t|| reaches the threshold only with the whole of s_j.  The Gaussian
problems of the other screen tests pass with a bound half the size.

Per case: the screened and the unscreened run are bit-identical (iteration counts, coefficients, every trace record and, wide solver,
every dumped iterate), stopped right after that step and again later; on the run's own iterates at least 50 special columns became
non-zero although |copy_j't| <= G, and at least 50 stayed zero (conditions on the inputs, tests/test_screen_threshold_host.py has them
without a GPU); and the screen's own count of exact steps lies between the number of columns that became non-zero and the number that
violate the inequality in float64 with the gamma term of s_j doubled -- a screen that screens nothing would be bit-identical too.
Figures are printed ("screen_threshold ..." lines, pytest -s): profiles/screen_tests.md."""
import re

import numpy as np
import pytest

import screen_cases as sc
from helpers import traced_fit

pytestmark = pytest.mark.gpu
F = np.float32


def _show(capfd, request, text):
    """print, past the capfd fixture under pytest -s (the fixture would otherwise keep the line to itself)"""
    if request.config.getoption("capture") == "no":
        with capfd.disabled():
            print(text)
    else:
        print(text)


def _wide_run(case, maxit, screen, stats=False):
    from admm_amd import admm_enet, admm_lasso, options
    opt = dict(WIDE_SCREEN=screen)
    if stats:
        opt["WIDE_SCREEN_STATS"] = "1"
    with options(**opt):
        m = (admm_enet if case["alpha"] is not None else admm_lasso)(case["x"], case["y"], intercept=False, standardize=False)
        m = m.penalty([case["lam"]], alpha=case["alpha"]) if case["alpha"] is not None else m.penalty([case["lam"]])
        return traced_fit(m.opts(maxit=maxit, rho=case["rho"]), capacity=64, state=64)


def _same_run(a, b, what):
    (fa, ta, sa), (fb, tb, sb) = a, b
    assert list(fa.niter) == list(fb.niter), (what, fa.niter, fb.niter)
    assert np.array_equal(fa.beta_dense, fb.beta_dense), (what, "coefficients", int((fa.beta_dense != fb.beta_dense).sum()))
    assert ta.shape == tb.shape and np.array_equal(ta, tb), (what, "trace")
    assert sa.shape == sb.shape and sa.tobytes() == sb.tobytes(), (what, "iterate dump", np.nonzero((sa != sb).any(axis=1))[0][:4])


@pytest.mark.parametrize("enet", [False, True])
@pytest.mark.parametrize("fmt", [16, 8])
@pytest.mark.parametrize("n", [120, 300])
def test_wide_columns_on_the_threshold_that_only_the_bound_saves(n, fmt, enet, capfd, request):
    case = sc.wide_case(n, fmt, enet)
    p, rho = sc.P, case["rho"]
    what = f"wide n {n} fmt {fmt} enet {enet}"
    off4 = _wide_run(case, 4, "0")
    capfd.readouterr()
    on4 = _wide_run(case, 4, str(fmt), stats=True)
    line = capfd.readouterr().err
    assert on4[0].stats["xupdate_variant"] == (2 if fmt == 8 else 1) and off4[0].stats["xupdate_variant"] == 0 and on4[0].stats["branch"] == 1
    _same_run(on4, off4, what + " maxit 4")
    fit, trace, st = on4
    assert list(fit.niter) == [5] and [int(k) for k in trace[:4, 7]] == [1, 2, 2, 1], (what, fit.niter, trace[:, 7])     # regular, active set twice, regular
    # the run's own iterates: record k + 1 holds x | A x | z | y after step k
    assert not st[3][:p].any(), "x must still be zero before step 3"
    ax, z, y = st[3][p:p + n], st[3][p + n:p + 2 * n], st[3][p + 2 * n:]
    t3 = ((ax + z) + y / F(rho)).astype(F)
    assert float(trace[4, 9]) == rho
    pops = sc.wide_populations(case, t3, st[4][:p], trace[4, 11], fit.stats["eig_est"])
    m = re.search(r"\[wide screen\] (\d+)-bit copy: (\d+) columns screened on regular steps, (\d+) took the exact path", line)
    assert m, (what, "no [wide screen] line", line)
    seen, exact = int(m.group(2)), int(m.group(3))
    _show(capfd, request, f"screen_threshold {what}: {pops}; screen saw {seen}, exact path {exact}")
    assert int(m.group(1)) == fmt and seen == 2 * p                                   # the regular steps 0 and 3
    assert pops["saved"] >= 50 and pops["stay"] >= 50, pops
    assert pops["nonzero"] <= exact <= pops["may_be_exact"], (what, exact, pops)
    # ... and with regular steps on a non-zero x (step 15)
    on20, off20 = _wide_run(case, 20, str(fmt)), _wide_run(case, 20, "0")
    assert on20[0].stats["xupdate_variant"] == (2 if fmt == 8 else 1) and off20[0].stats["xupdate_variant"] == 0
    _same_run(on20, off20, what + " maxit 20")
    assert on20[2][:5].tobytes() == st[:5].tobytes() and np.count_nonzero(on20[0].beta_dense) > 0


def _sbp_run(case, maxit, screen, stats=False):
    import admm_amd
    opt = dict(SBP_SCREEN=screen)
    if stats:
        opt["SBP_SCREEN_STATS"] = "1"
    with admm_amd.options(**opt):
        return admm_amd.admm_bp(case["A"], case["b"]).parallel(case["N"]).opts(maxit=maxit).fit(trace=True)


@pytest.mark.parametrize("N", [3, 4])
@pytest.mark.parametrize("n", [120, 300])
def test_sbp_columns_on_the_threshold_that_only_the_bound_saves(n, N, capfd, request):
    case = sc.sbp_case(n, N)
    what = f"sbp n {n} N {N}"
    fits = {}
    for maxit in (12, 25):
        off = _sbp_run(case, maxit, "0")
        capfd.readouterr()
        on = _sbp_run(case, maxit, "1", stats=maxit == 12)
        if maxit == 12:
            line = capfd.readouterr().err
        assert on.stats["xupdate_variant"] >= 4 and off.stats["xupdate_variant"] < 4
        assert on.niter == off.niter == maxit + 1, (what, maxit, on.niter, off.niter)
        assert np.array_equal(on.trace, off.trace), (what, maxit, "trace")
        assert np.array_equal(on.beta.toarray(), off.beta.toarray()), (what, maxit, "coefficients")
        fits[maxit] = on
    on = fits[12]
    rho = on.stats["rho"]
    assert abs(rho / case["rho"] - 1) < 1e-9, (rho, case["rho"])                       # the library's Lanczos value against the exact one
    pops = sc.sbp_populations(case, rho)
    may = pops.pop("may_be_nonzero")
    m = re.search(r"\[parbp screen\] (\d+) columns screened on regular iterations, (\d+) took the exact step", line)
    assert m, (what, "no [parbp screen] line", line)
    seen, exact = int(m.group(1)), int(m.group(2))
    _show(capfd, request, f"screen_threshold {what}: rho {rho:.6e}, {pops}; screen saw {seen}, exact step {exact}; non-zeros after 12 / 25 steps "
                          f"{np.count_nonzero(on.beta.toarray())} / {np.count_nonzero(fits[25].beta.toarray())}")
    assert seen == 2 * sc.P                                                            # the regular iterations 0 and 10
    assert pops["saved"] >= 50 and pops["stay"] >= 50, pops
    assert pops["nonzero"] <= exact <= pops["may_be_exact"] + pops["near"], (what, exact, pops)
    nz = on.beta.toarray().ravel() != 0                                                # after step 11, an active-set step: nothing new can have come in
    assert not (nz & ~may).any(), (what, "a column is non-zero that step 10 cannot have kept")
