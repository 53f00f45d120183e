"""GPU: the tile prologue of the decide-first x-update and the Lasso tail after their requests were put into one batch each
(symv_kernels.h: symv1_tile, symv_sum_partials1; lasso_tall.hip: tall_norms_request / tall_norms_sum, tall_tail_kernel).  Nothing a path
returns may move: ADMM_HIP_SYMV_VERDICT=3 -- on the 29-bit copy (the default) and on the fp32 matrix (SYMV_PACK=0) -- against the
two-vector form without any early exit (level 0), to the bit in lambda, niter, beta and the decision trace, and the tiles that left are
exactly tiles x discarded launches.

The way and the host data recipe are test_gpu_tall_decide_first.py's, whose shapes (p = 2304 resident, p = 4200 in two rounds, all four
tails) stay there.  Here:
  p =  8200, n =  8300 (host data):   257 workgroups of the tail -- the gate's second row of norm partials has ONE live thread, the
                                      branch-free request of every other thread is clamped to the last row -- and the last workgroup
                                      of the tail is ragged (8200 = 256 * 32 + 8);
  p = 16416, n = 16448 (device data, generated as bench.py generates it): 513 workgroups -- the first thread takes the gate's loop path
                                      behind the two requested rows -- and a triangle beyond the Infinity Cache: the non-temporal
                                      instantiations of both x-update kernels.
Three lambdas; maxit caps a lambda so that a case stays within seconds (setup included) while both picks and the leave still occur,
which the test asserts from the device's own trace."""
import numpy as np
import pytest

import test_gpu_tall_decide_first as df

pytestmark = pytest.mark.gpu

NLAM, LMR, MAXIT = 3, 0.05, 60


def _host_model(n, p):
    import admm_amd
    x, y = df._data(n, p)
    return admm_amd.admm_lasso(x, y), None


def _device_model(n, p):
    """bench.py's recipe: X generated in HBM as xt (p x n row-major == n x p column-major), beta* = U(0, 1) on the first m, y = X beta* + N(0, 1)."""
    import torch
    import admm_amd
    from admm_amd._lib import DevicePtr
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(n + p)
    xt = torch.empty((p, n), dtype=torch.float64, device=dev)
    chunk = max(1, (1 << 27) // n)
    for c0 in range(0, p, chunk):
        c1 = min(p, c0 + chunk)
        xt[c0:c1] = torch.randn((c1 - c0, n), generator=g, device=dev, dtype=torch.float64) * 2.0
    m = p // 20
    beta_true = torch.zeros(p, dtype=torch.float64, device=dev)
    beta_true[:m] = torch.rand(m, generator=g, device=dev, dtype=torch.float64)
    y = beta_true @ xt + torch.randn(n, generator=g, device=dev, dtype=torch.float64)
    torch.cuda.synchronize()
    return admm_amd.admm_lasso(DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr()), n=n, p=p), (xt, y)


def _streams_packed():
    """1 if the calling thread's most recent tall plan streams the 29-bit copy (admm_hip_test_tall_pack_info)."""
    import ctypes
    from admm_amd import _lib
    info = (ctypes.c_longlong * 4)()
    _lib.check(_lib.load().admm_hip_test_tall_pack_info(info))
    return int(info[0])


def _paths(make, n, p):
    """(fit, trace, tiles that left, tiles) of the three forms on one data set, each plan closed before the next is made."""
    from admm_amd import options
    from admm_amd.api import LassoPlan
    model, keep = make(n, p)
    model = model.penalty(nlambda=NLAM, lambda_min_ratio=LMR).opts(maxit=MAXIT)
    out = {}
    for name, opts in (("packed", dict(SYMV_VERDICT=3)), ("fp32", dict(SYMV_VERDICT=3, SYMV_PACK=0)), ("two-vector", dict(SYMV_VERDICT=0))):
        with options(**opts):
            plan = LassoPlan(model)
            ntiles = df._tiles(p)
        try:
            assert _streams_packed() == (1 if name == "packed" else 0), name
            plan.enable_trace(1 << 12)
            out[name] = df._run(plan) + (ntiles,)
        finally:
            plan.close()
    del keep
    return out


@pytest.mark.parametrize("make,n,p,nwg", [(_host_model, 8300, 8200, 257), (_device_model, 16448, 16416, 513)], ids=["p8200-nwg257", "p16416-nwg513-nt"])
def test_decide_first_is_the_two_vector_path_to_the_bit(make, n, p, nwg):
    assert (p + 31) // 32 == nwg
    r = _paths(make, n, p)
    f0, t0, e0, ntiles = r["two-vector"]
    kinds = {c: int((t0[:, 8] == c).sum()) for c in (df.CONVERGED, df.ACCELERATE, df.RESTART)}
    print(f"n={n} p={p}: niter {list(map(int, f0.niter))}, {len(t0)} decisions (converged / accelerate / restart "
          f"{kinds[df.CONVERGED]} / {kinds[df.ACCELERATE]} / {kinds[df.RESTART]}), {ntiles} tiles, left: "
          + ", ".join(f"{k} {v[2]}" for k, v in r.items()))
    assert int(f0.stats["xupdate_variant"]) == 1                         # the lower-triangle kernels
    assert kinds[df.ACCELERATE] >= 1 and kinds[df.RESTART] >= 1          # both picks were taken ...
    discarded = df._discarded_launches(t0, NLAM)
    assert discarded >= 1                                                # ... and at least one launch was left
    assert int(f0.niter.min()) >= 1 and e0 == 0
    for name in ("packed", "fp32"):
        f, t, e, nt = r[name]
        assert nt == ntiles
        assert df._same_fit(f0, f), name
        assert len(t) == len(t0) > NLAM and df._same(t, t0), name
        assert e == ntiles * discarded, (name, e, ntiles, discarded)
