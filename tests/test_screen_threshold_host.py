"""The inputs of tests/test_gpu_screen_threshold.py are what they claim, from the oracle alone (no GPU): at the first regular step with a
non-zero t (step 3 of the wide solver, step 10 of the sharing basis pursuit) at least 50 of the 400 special columns become non-zero
although the product with their copy stays below the screen's right-hand side -- the columns that only the bound s_j keeps exact -- and at
least 50 stay zero.  screen_cases.py has the construction."""
import numpy as np
import pytest

import screen_cases as sc

F = np.float32


@pytest.mark.parametrize("enet", [False, True])
@pytest.mark.parametrize("fmt", [16, 8])
@pytest.mark.parametrize("n", [120, 300])
def test_wide_special_columns_straddle_the_threshold_of_step_3(n, fmt, enet):
    from oracle import entry
    case = sc.wide_case(n, fmt, enet)
    prob = sc.wide_problem(case, maxit=4)
    d = {"state": [], "types": []}
    args = (prob["x"], prob["y"], prob["lam"], 1, 0.01, False, False)
    ref = entry.admm_enet(*args, case["alpha"], prob["opts"], d) if enet else entry.admm_lasso(*args, prob["opts"], d)
    assert d["types"] == [1, 2, 2, 1] and int(ref["niter"][0]) == 5           # regular, two active-set steps on nothing, regular; ran into maxit
    p = sc.P
    st = d["state"]
    assert not st[2][:p].any(), "x must still be zero before step 3"
    ax, z, y = st[2][p:p + n], st[2][p + n:p + 2 * n], st[2][p + 2 * n:]
    t3 = ((ax + z) + y / F(case["rho"])).astype(F)
    assert np.array_equal(t3, sc.wide_t3(case["y"], case["rho"])), "t before step 3 is a function of Y and rho alone"
    assert np.abs(t3.astype(np.float64) - case["c"] * case["y"]).max() <= 8 * np.spacing(F(abs(case["c"])))         # t = c Y to float rounding
    solver = d["solver"]
    assert float(solver.rho) == case["rho"]
    pops = sc.wide_populations(case, t3, st[3][:p], solver.lam, solver.sprad)
    print(f"screen_threshold host wide n {n} fmt {fmt} enet {enet}: c {case['c']:.6f}, threshold {case['threshold']:.6f}, {pops}")
    assert pops["saved"] >= 50 and pops["stay"] >= 50, pops
    assert pops["nonzero"] <= pops["may_be_exact"], pops


@pytest.mark.parametrize("N", [3, 4])
@pytest.mark.parametrize("n", [120, 300])
def test_sbp_special_columns_straddle_the_threshold_of_step_10(n, N):
    from oracle.solvers import SharingBP
    case = sc.sbp_case(n, N)
    s = SharingBP(case["A"], case["b"], N, 1e-4, 1e-4)
    s.init(1.0)
    assert s.rho == case["rho"]
    s.trace = []
    assert s.solve(10) == 11 and not s.get_x().any(), "x must still be zero before step 10"
    assert np.abs((s.y / s.rho + s.r) - case["v"]).max() <= 64 * np.spacing(np.abs(case["v"]).max()), "v before step 10 is -11 b / N"
    s.init(1.0)
    assert s.solve(11) == 12                                                    # steps 0 .. 10
    nz = s.get_x() != 0
    pops = sc.sbp_populations(case, case["rho"])
    may = pops.pop("may_be_nonzero")
    print(f"screen_threshold host sbp n {n} N {N}: rho {case['rho']:.6e}, {pops}")
    assert not (nz & ~may).any() and int(nz.sum()) >= pops["nonzero"], "the oracle's support after step 10 is the one v = -11 b / N gives"
    assert pops["saved"] >= 50 and pops["stay"] >= 50, pops
    assert pops["nonzero"] <= pops["may_be_exact"], pops
