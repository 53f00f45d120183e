"""GPU: the decide-first x-update of the tall path (ADMM_HIP_SYMV_VERDICT=3, the default; lasso_tall.hip: TallGate, tall_outcome;
symv_kernels.h: symv1_lower_kernel).  Every tile of a launch takes that launch's decision itself, from what earlier launches wrote,
before it streams: it multiplies the one vector the tail will read into plane 0 of the partials, or leaves.  What a path returns must
be what the two-vector form without any early exit (level 0) returns, to the bit -- lambda, niter, beta and the decision trace -- and,
because nothing depends on timing any more, the number of tiles that left is exactly tiles x discarded launches.

Data: test_gpu_tall_early_exit.py's (rng(n + p), 8 lambdas, lambda_min_ratio 0.01).  n = 2500, p = 2304 under the default schedule
is resident as a whole; n = 4400, p = 4200 in 32-column segments is 1220 tiles, more than the 1024 workgroups a 256-CU device holds.
The CPU oracle (oracle.entry.admm_lasso) takes 341 decisions on the first: 8 converged, 36 accelerate, 297 restart; with maxit = 35
its iteration counts are 23, 36, 36, 36, 36, 36, 28, 36 -- five middle lambdas and the last end by the cap.  The tests assert such
facts from the device's own trace and niter, so that a change of the data cannot hollow them out."""
import ctypes

import numpy as np
import pytest

import box_oracle as bo

pytestmark = pytest.mark.gpu

NLAM, LMR = 8, 0.01
SHAPES = [(2500, 2304, None), (4400, 4200, "32,32,0")]
CONVERGED, ACCELERATE, RESTART = 0.0, 1.0, 2.0      # ADMM_TRACE_* (record field 8)
_cache = {}


def _data(n, p):
    if (n, p) not in _cache:
        rng = np.random.default_rng(n + p)
        x = np.asfortranarray(rng.standard_normal((n, p)) * 2.0)
        beta = np.zeros(p)
        beta[:p // 20] = rng.uniform(size=p // 20)
        _cache[(n, p)] = (x, x @ beta + rng.standard_normal(n))
    return _cache[(n, p)]


def _groups(p):
    """Adjacent groups of mixed sizes: singletons, small ones, one that spans several workgroups of the tail."""
    sizes, out, g = [1, 2, 5, 40, 3, 1, 17, 64], [], 0
    while len(out) < p:
        out += [g] * min(sizes[g % len(sizes)], p - len(out))
        g += 1
    return np.asarray(out)


def _model(kind, x, y, maxit=None):
    import admm_amd
    pen = dict(nlambda=NLAM, lambda_min_ratio=LMR)
    if kind == "lasso":
        m = admm_amd.admm_lasso(x, y).penalty(**pen)
    elif kind == "enet":
        m = admm_amd.admm_enet(x, y).penalty(alpha=0.5, **pen)
    elif kind == "grplasso":
        m = admm_amd.admm_grplasso(x, y, _groups(x.shape[1])).penalty(**pen)
    else:
        lower, upper, u = bo.box_pattern(x.shape[1])
        m = admm_amd.admm_boxenet(x, y, lower, upper).penalty(alpha=0.5, penalty_factor=u, **pen)
    return m if maxit is None else m.opts(maxit=maxit)


def _early_exits():
    from admm_amd import _lib
    n = ctypes.c_longlong(-1)
    _lib.check(_lib.load().admm_hip_test_tall_early_exits(ctypes.byref(n)))
    return int(n.value)


def _tiles(p):
    """Tiles of the x-update's plan for order p on this device under the calling thread's schedule (the host half of the plan)."""
    import torch
    from admm_amd import _lib
    so, info = (ctypes.c_int * 3)(), (ctypes.c_longlong * 6)()
    rec = np.zeros((1 << 15, 4), np.int32)
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    _lib.check(_lib.load().admm_hip_test_symv_plan(p, cus, 0, 1, so, info, rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), rec.shape[0]))
    return int(info[5])


def _plan(kind, n, p, sched, level, maxit=None):
    from admm_amd import options
    from admm_amd.api import LassoPlan
    x, y = _data(n, p)
    opts = {} if sched is None else {"SYMV_SCHED": sched}
    with options(SYMV_VERDICT=level, **opts):
        plan = LassoPlan(_model(kind, x, y, maxit))
        ntiles = _tiles(p)
    plan.enable_trace(1 << 13)
    return plan, ntiles


def _run(plan):
    fit = plan.run()
    return fit, plan.read_trace(), _early_exits()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_fit(a, b):
    return _same(a.lambda_, b.lambda_) and _same(a.niter, b.niter) and _same(a.beta_dense, b.beta_dense)


def _discarded_launches(trace, nlam):
    """One per lambda that converged (the launch that takes that decision), and the launch of the final decision if the last lambda
    ended by maxit instead.  The launch that finishes a capped lambda in the middle of the path is consumed."""
    code = trace[:, 8]
    last_capped = code[-1] != CONVERGED
    assert int(trace[-1, 0]) == nlam - 1
    return int((code == CONVERGED).sum()) + (1 if last_capped else 0)


def _check(kind, n, p, sched, maxit=None):
    on, ntiles = _plan(kind, n, p, sched, 3, maxit)
    off, _ = _plan(kind, n, p, sched, 0, maxit)
    try:
        (f3, t3, e3), (f0, t0, e0), (f3b, t3b, e3b) = _run(on), _run(off), _run(on)
    finally:
        on.close()
        off.close()
    kinds = {c: int((t0[:, 8] == c).sum()) for c in (CONVERGED, ACCELERATE, RESTART)}
    print(f"{kind} n={n} p={p} sched={sched} maxit={maxit}: niter {list(map(int, f3.niter))}, {len(t0)} decisions "
          f"(converged / accelerate / restart {kinds[CONVERGED]} / {kinds[ACCELERATE]} / {kinds[RESTART]}), {ntiles} tiles, "
          f"tiles that left: level 3 {e3}, again {e3b}, level 0 {e0}")
    assert int(f3.stats["xupdate_variant"]) == 1                        # the lower-triangle kernels
    assert min(kinds.values()) >= 1, kinds                              # both picks and the leave were exercised
    assert int(f0.niter.min()) >= 1
    for f, t in ((f0, t0), (f3b, t3b)):
        assert _same_fit(f3, f)
        assert len(t) == len(t3) > NLAM and _same(t, t3)
    assert e0 == 0
    assert e3 == e3b == ntiles * _discarded_launches(t3, NLAM), (e3, e3b, ntiles, _discarded_launches(t3, NLAM))
    return f3, t3


@pytest.mark.parametrize("n,p,sched", SHAPES, ids=["resident", "two-rounds"])
@pytest.mark.parametrize("kind", ["lasso", "enet", "grplasso", "boxenet"])
def test_level_3_is_level_0_to_the_bit_and_the_leave_count_is_exact(kind, n, p, sched):
    fit, trace = _check(kind, n, p, sched)
    assert int((trace[:, 8] == CONVERGED).sum()) == NLAM                # every lambda converged: one discarded launch each


def test_lambdas_that_end_by_maxit():
    """maxit = 35: a middle lambda and the last end by the cap, others converge.  The launch that takes the capping decision of a middle
    lambda is consumed (no tile leaves it); the one of the last lambda is the end of the path (every tile leaves)."""
    maxit = 35
    fit, trace = _check("lasso", 2500, 2304, None, maxit)
    niter = np.asarray(fit.niter).astype(int)
    capped = niter == maxit + 1
    assert capped[-1] and capped[1:-1].any() and (~capped).any(), niter
    assert int((trace[:, 8] == CONVERGED).sum()) == int((~capped).sum())


def test_a_stale_plane_one_is_never_read():
    """A level-0 path leaves both planes of partials full; a level-3 plan created next takes its storage from the same pool.  Then the
    other way round.  Nothing on the decide-first path may read plane 1, nothing on the two-vector path may miss it."""
    fits = []
    for level in (0, 3, 0, 3):
        plan, _ = _plan("lasso", 2500, 2304, None, level)
        try:
            fits.append(_run(plan))
        finally:
            plan.close()
    for f, t, _ in fits[1:]:
        assert _same_fit(fits[0][0], f) and _same(fits[0][1], t)
