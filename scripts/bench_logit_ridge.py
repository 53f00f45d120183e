#!/usr/bin/env python
"""Measure admm_hip_logit_ridge (ridge logistic regression: k label columns x a lambda grid on one setup) at n = 50000, k = 8, fp64,
device-resident input, intercept FALSE, on the data of scripts/bench_logit_multi.py, with p = 1000 (one double2 per thread and row: up to
four slots) and p = 5000 (five: no second slot).  `--p` takes other layouts (2000, 3000: four slots; 4000: two).

Fixed work: maxit = `--maxit` with eps so small that no fit converges, one warm-up and `--repeats` timed repeats, median and spread
(max - min) / median of
  * "multi S=1" / "multi S=auto": admm_logit_multi on the same data, serial and as it runs by default -- the unpenalised loop, n rows;
  * "ridge S=1": the ridge call (lambda = 1) on its serial route, n + p rows.  rate(multi S=1) / rate(ridge S=1) - 1 is the price of
    the ridge rows, to compare with p / (n + p) more bytes per iteration (they are streamed dense);
  * "ridge S=s" for every s >= 2 the layout's register table admits: the slotted route against the serial one;
  * "grid": one call with five lambda against five calls with one lambda each (serial route, wall time): what the shared upload,
    standardisation, data-row Gram matrix and transpose save.
Prints one JSON line per measurement.
Usage: bench_logit_ridge.py [--n N --p P[,P...] --k K --repeats R --maxit M]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--p", default="1000,5000")
ap.add_argument("--k", type=int, default=8)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--maxit", type=int, default=100)
args = ap.parse_args()
n, k = args.n, args.k
PS = [int(v) for v in str(args.p).split(",")]
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before libadmm_hip)
from admm_amd import DevicePtr, admm_logit_multi, admm_logit_ridge, options  # noqa: E402

dev = torch.device("cuda", 0)
RIDGE_MAX_SLOTS = {1: 4, 2: 4, 3: 4, 4: 2, 5: 1, 6: 1}      # fadmm_dense.hip, kProxKinds[kProxLogitR].max_slots
GRID = (100.0, 10.0, 1.0, 0.1, 0.01)


def make(p):
    """scripts/bench_logit_multi.py's data: x = 2 N(0, 1) as p x n row-major (= n x p column-major) and k label columns (k x n row-major)
    drawn from k logistic models with their own coefficients and class balances."""
    g = torch.Generator(device=dev)
    g.manual_seed(123)
    xt = torch.empty((p, n), dtype=torch.float64, device=dev)
    chunk = max(1, (1 << 27) // n)
    for c0 in range(0, p, chunk):
        c1 = min(p, c0 + chunk)
        xt[c0:c1] = torch.randn((c1 - c0, n), generator=g, device=dev, dtype=torch.float64) * 2.0
    b = torch.rand(p, generator=g, device=dev, dtype=torch.float64)
    _ = b @ xt + torch.randn(n, generator=g, device=dev, dtype=torch.float64) * (1 + 0.3 * xt[0].abs())      # (the Huber response there: keeps the generator in step)
    lab = torch.empty((k, n), dtype=torch.float64, device=dev)
    for c in range(k):
        bc = (2 * torch.rand(p, generator=g, device=dev, dtype=torch.float64) - 1) / p ** 0.5
        eta = 0.5 * (bc @ xt) - 0.8 + 1.6 * c / max(1, k - 1)
        lab[c] = (torch.rand(n, generator=g, device=dev, dtype=torch.float64) < torch.sigmoid(eta)).to(torch.float64)
    torch.cuda.synchronize()
    return xt, lab


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def fixed(builder):
    f = builder().opts(maxit=args.maxit, eps_abs=1e-100, eps_rel=1e-100).fit()
    niter = [int(v) for v in f.niter.ravel()]
    assert niter == [args.maxit + 1] * len(niter), niter
    return f


for p in PS:
    xt, lab = make(p)
    X, L = DevicePtr(xt.data_ptr()), DevicePtr(lab.data_ptr())
    npt = ((p + 31) // 32 * 32 // 2 + 511) // 512

    def multi(slots):
        def run():
            t0 = time.perf_counter()
            with options(QUANT_SLOTS=slots):
                f = fixed(lambda: admm_logit_multi(X, L, intercept=False, n=n, p=p, k=k))
            return time.perf_counter() - t0, f.stats["t_loop"], int(f.stats["xupdate_variant"]), k
        return run

    def ridge(slots, lam=1.0):
        def run():
            t0 = time.perf_counter()
            with options(QUANT_SLOTS=slots):
                f = fixed(lambda: admm_logit_ridge(X, L, lam, intercept=False, n=n, p=p, k=k))
            return time.perf_counter() - t0, f.stats["t_loop"], int(f.stats["xupdate_variant"]), k * len(f.lam)
        return run

    def five_calls():
        t0, loop, variant = time.perf_counter(), 0.0, None
        for lam in GRID:
            _, lp, variant, _ = ridge(1, lam)()
            loop += lp
        return time.perf_counter() - t0, loop, variant, k * len(GRID)

    routes = ([("multi S=1", multi(1)), ("multi S=auto", multi(None)), ("ridge S=1", ridge(1))]
              + [(f"ridge S={s}", ridge(s)) for s in range(2, min(RIDGE_MAX_SLOTS[npt], k) + 1)]
              + [("ridge S=auto", ridge(None)), ("grid: one call, 5 lambda", ridge(1, GRID)), ("grid: 5 calls, 1 lambda", five_calls)])
    med = {}
    for name, run in routes:
        walls, rates, variant = [], [], None
        for r in range(args.repeats + 1):
            wall, loop, variant, nfit = run()
            if r:
                walls.append(wall)
                rates.append(nfit * args.maxit / loop)
        med[name] = (statistics.median(walls), statistics.median(rates))
        print(json.dumps({"run": "fixed work", "route": name, "n": n, "p": p, "k": k, "npt": npt, "maxit": args.maxit, "variant": variant,
                          "wall_s": med[name][0], "wall_spread": spread(walls), "column_iters_per_s": med[name][1], "rate_spread": spread(rates),
                          "walls": walls, "rates": rates}), flush=True)
    print(json.dumps({"p": p, "npt": npt, "p_over_n_plus_p": p / (n + p),
                      "ridge_rows_price_serial": med["multi S=1"][1] / med["ridge S=1"][1] - 1.0,
                      "rate_over_ridge_serial": {r: med[r][1] / med["ridge S=1"][1] for r in med if r.startswith("ridge")},
                      "grid_wall_one_call_over_five": med["grid: one call, 5 lambda"][0] / med["grid: 5 calls, 1 lambda"][0]}), flush=True)
    del xt, lab, X, L
    torch.cuda.empty_cache()
