"""GPU: the decision a tile of the decide-first x-update takes in its prologue (lasso_tall.hip: TallGate -- tall_norms_request,
tall_norms_sum, tall_outcome) through the hooks admm_hip_test_tall_gate and admm_hip_test_tall_norms, on caller-supplied inputs.

The requests of the norm partials are branch-free: a thread without a row asks for the last row and adds +0.0 in its place.  That must
not move a bit: the three sums a tile forms from the compact copy are required to EQUAL, bit for bit, columns 0 .. 2 of the six sums
the deciding workgroup forms from the rows of P (a tile that decided otherwise than block 0 would multiply the wrong vector), and both
are held against float64 math.fsum.  nwg (workgroups of the tail = rows of partials, 256 threads summing them):
   1, 63, 64, 65      a partly live first row (and whole waves without a row);
   255, 256, 257      the last / no / the first live thread of the second requested row;
   511, 512, 513      the same for the loop path behind the two requested rows;  1000: four rows, the last one ragged.
The partials span 30 orders of magnitude, so the order of the additions shows in the last bits.

Tolerance: a thread adds at most ceil(nwg / 256) terms, the block sum 6 + 3 more levels: fewer than nwg additions of non-negative
terms in any order are within (nwg - 1) * 2^-53 relative of the exact sum; the test allows nwg * 2^-52.

The answer (-1 leave, 0 multiply u, 1 multiply w) is held against tall_outcome restated in NumPy, on control blocks whose thresholds are
placed 1e-6 relative -- seven orders above the sums' error -- or further from the values they are compared with, so that the reference
alone decides every case."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NWG = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000]
LEAVE = -1
_dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
_cache = {}


def _rows(nwg):
    """[nwg][8] non-negative partials over 30 orders of magnitude (columns 6, 7 are padding the kernels never read: NaN)."""
    if nwg not in _cache:
        rng = np.random.default_rng(1000 + nwg)
        rows = 10.0 ** rng.uniform(-15.0, 15.0, size=(nwg, 8))
        rows[:, 6:] = np.nan
        rows.setflags(write=False)
        _cache[nwg] = rows
    return _cache[nwg]


def _block0_sums(rows):
    from admm_amd import _lib
    out = np.zeros(6)
    rows = np.ascontiguousarray(rows)
    _lib.check(_lib.load().admm_hip_test_tall_norms(rows.ctypes.data_as(_dp), rows.shape[0], out.ctypes.data_as(_dp)))
    return out


CTL_D = ("rho", "lam", "eps_primal", "eps_dual", "adj_a", "adj_c", "tau", "a_next", "tau_next")
CTL_I = ("mode", "restart", "iter", "lam_idx", "done", "first", "total", "fin_idx", "fin_niter")


def _gate(ctl, rows, maxit, nlam):
    from admm_amd import _lib
    compact = np.ascontiguousarray(rows[:, :3].T)                       # [3][nwg]: a column of P consecutive
    cd = np.array([ctl[k] for k in CTL_D], dtype=np.float64)
    ci = np.array([ctl[k] for k in CTL_I], dtype=np.int32)
    sums, ans = np.zeros(3), ctypes.c_int(99)
    _lib.check(_lib.load().admm_hip_test_tall_gate(cd.ctypes.data_as(_dp), ci.ctypes.data_as(_ip), compact.ctypes.data_as(_dp), rows.shape[0],
                                                   maxit, nlam, sums.ctypes.data_as(_dp), ctypes.byref(ans)))
    return sums, int(ans.value)


def _ctl(**kw):
    c = dict(rho=1.7, lam=0.3, eps_primal=0.0, eps_dual=0.0, adj_a=1.0, adj_c=9999.0, tau=0.0, a_next=1.618, tau_next=0.0,
             mode=1, restart=0, iter=3, lam_idx=1, done=0, first=0, total=17, fin_idx=-1, fin_niter=0)
    c.update(kw)
    return c


def _outcome(c, r2, dz2, daz2, maxit, nlam):
    """lasso_tall.hip: tall_outcome and TallGate::decide, restated."""
    if c["done"]:
        return LEAVE
    if c["first"]:
        return 0
    rp, rd = math.sqrt(r2), c["rho"] * math.sqrt(dz2)
    fin = done = False
    if rp < c["eps_primal"] and rd < c["eps_dual"]:
        converged, restart, fin = True, False, True
    else:
        converged = False
        comb = c["rho"] * rp * rp + c["rho"] * daz2
        restart = not (comb < 0.999 * c["adj_c"])
        if c["iter"] + 1 >= maxit:
            fin = True
    if fin and c["lam_idx"] + 1 >= nlam:
        done = True
    if converged or done:
        return LEAVE
    return 1 if restart else 0


def _cases(r2, dz2, daz2):
    """(name, control block, maxit, nlam): every branch of the rule, the thresholds 1e-6 relative or further from what they meet."""
    rho = 1.7
    rp, rd = math.sqrt(r2), rho * math.sqrt(dz2)
    comb = rho * rp * rp + rho * daz2
    up, dn = 1.0 + 1e-6, 1.0 - 1e-6
    open_ = dict(eps_primal=rp * 0.5, eps_dual=rd * 0.5)                # far from converged
    return [
        ("converged", _ctl(eps_primal=rp * 2, eps_dual=rd * 2), 100, 8),
        ("converged-by-1e-6", _ctl(eps_primal=rp * up, eps_dual=rd * up), 100, 8),
        ("primal-misses-by-1e-6-accelerate", _ctl(eps_primal=rp * dn, eps_dual=rd * 2, adj_c=comb / 0.999 * 2), 100, 8),
        ("dual-misses-by-1e-6-restart", _ctl(eps_primal=rp * 2, eps_dual=rd * dn, adj_c=comb / 0.999 * 0.5), 100, 8),
        ("accelerate-by-1e-6", _ctl(adj_c=comb / 0.999 * up, **open_), 100, 8),
        ("restart-by-1e-6", _ctl(adj_c=comb / 0.999 * dn, **open_), 100, 8),
        ("cold-start", _ctl(first=1, eps_primal=rp * 2, eps_dual=rd * 2), 100, 8),
        ("done", _ctl(done=1, **open_), 100, 8),
        ("capped-middle-lambda-restart", _ctl(iter=99, lam_idx=1, adj_c=comb / 0.999 * 0.5, **open_), 100, 8),
        ("capped-middle-lambda-accelerate", _ctl(iter=99, lam_idx=1, adj_c=comb / 0.999 * 2, **open_), 100, 8),
        ("capped-last-lambda", _ctl(iter=99, lam_idx=7, adj_c=comb / 0.999 * 2, **open_), 100, 8),
        ("converged-last-lambda", _ctl(lam_idx=7, eps_primal=rp * 2, eps_dual=rd * 2), 100, 8),
        ("last-lambda-goes-on", _ctl(lam_idx=7, adj_c=comb / 0.999 * 0.5, **open_), 100, 8),
    ]


@pytest.mark.parametrize("nwg", NWG)
def test_a_tile_forms_block_zeros_sums_and_takes_the_reference_decision(nwg):
    rows = _rows(nwg)
    exact = [math.fsum(rows[:, k]) for k in range(6)]
    b0 = _block0_sums(rows)
    tol = nwg * 2.0 ** -52
    err0 = [abs(b0[k] - exact[k]) / exact[k] for k in range(6)]
    print(f"nwg={nwg}: block-0 sums against fsum, relative {['%.2e' % e for e in err0]} (allowed {tol:.2e})")
    assert max(err0) <= tol, (err0, tol)
    answers = set()
    for name, ctl, maxit, nlam in _cases(*exact[:3]):
        sums, ans = _gate(ctl, rows, maxit, nlam)
        assert sums.tobytes() == b0[:3].tobytes(), (name, sums, b0[:3])     # the same bits as block 0, whatever the control block says
        want = _outcome(ctl, exact[0], exact[1], exact[2], maxit, nlam)
        assert ans == want, (name, ans, want)
        answers.add(ans)
    assert answers == {LEAVE, 0, 1}


def test_a_different_order_of_the_additions_would_show():
    """The inputs can tell summation orders apart: the plain left-to-right sum of a column differs from the kernels' in some column
    for the larger nwg (otherwise `bit-equal` above would hold for any order)."""
    differ = 0
    for nwg in (257, 513, 1000):
        rows = _rows(nwg)
        b0 = _block0_sums(rows)
        seq = [float(np.add.accumulate(rows[:, k])[-1]) for k in range(3)]
        differ += sum(1 for k in range(3) if seq[k] != b0[k])
    assert differ >= 1
