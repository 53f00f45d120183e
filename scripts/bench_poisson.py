#!/usr/bin/env python
"""Measure admm_hip_poisson (Poisson regression with the elastic-net penalty: k count columns x (lambda, alpha) cells on ONE inverse) at
n = 50000, k = 8, fp64, device-resident input, intercept FALSE, at p = 1000 ... 5000 (one to five double2 per thread and row: 4, 4, 3,
2 slots, none at 5000).

Data: x = N(0, 1); count column c = Poisson(exp(b0_c + x b_c)), b_c = U(-1, 1) / sqrt(p) scaled so that the linear predictor has
standard deviation about 0.5, b0_c spread over -1.5 ... 2 (mean counts about 0.25 ... 8).

Grids: five lambda = f lambda_1 / alpha, f = 0.5, 0.3, 0.2, 0.1, 0.05 (lambda_1 the largest over the k columns, from
admm_hip_poisson_lambda_max), at every alpha of `--alpha`: 40 fits per call.

  * "fixed work": maxit = `--maxit` with eps so small that no fit converges, one warm-up and `--repeats` timed repeats, median and
    spread (max - min) / median of the loop's rate (fit-iterations per second, stats.t_loop) and of the wall time, for "S=1" and
    "S=s" for every s >= 2 the layout's register table admits, and "S=auto": the slotted route against the serial one.
  * "converged": the grids with the default stop rule (eps 1e-4), as QUANT_SLOTS=0 runs them: wall time and the iteration counts per
    cell (min / median / max over the k columns).
Prints one JSON line per measurement.
Usage: bench_poisson.py [--n N --p P[,P...] --k K --repeats R --maxit M --alpha A[,A...]]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--p", default="1000,2000,3000,4000,5000")
ap.add_argument("--k", type=int, default=8)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--maxit", type=int, default=100)
ap.add_argument("--alpha", default="1.0,0.5")
args = ap.parse_args()
n, k = args.n, args.k
PS = [int(v) for v in str(args.p).split(",")]
ALPHAS = [float(v) for v in str(args.alpha).split(",")]
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before libadmm_hip)
from admm_amd import DevicePtr, admm_poisson, options  # noqa: E402

dev = torch.device("cuda", 0)
POIS_MAX_SLOTS = {1: 4, 2: 4, 3: 3, 4: 2, 5: 1, 6: 1}      # fadmm_dense.hip, kProxKinds[kProxPoisE].max_slots
FRACTIONS = (0.5, 0.3, 0.2, 0.1, 0.05)


def make(p):
    """x as p x n row-major (= n x p column-major) and k count columns (k x n row-major)"""
    g = torch.Generator(device=dev)
    g.manual_seed(123)
    xt = torch.empty((p, n), dtype=torch.float64, device=dev)
    chunk = max(1, (1 << 27) // n)
    for c0 in range(0, p, chunk):
        c1 = min(p, c0 + chunk)
        xt[c0:c1] = torch.randn((c1 - c0, n), generator=g, device=dev, dtype=torch.float64)
    cnt = torch.empty((k, n), dtype=torch.float64, device=dev)
    for c in range(k):
        bc = (2 * torch.rand(p, generator=g, device=dev, dtype=torch.float64) - 1) / p ** 0.5
        eta = 0.87 * (bc @ xt) - 1.5 + 3.5 * c / max(1, k - 1)
        cnt[c] = torch.poisson(torch.exp(eta), generator=g)
    torch.cuda.synchronize()
    return xt, cnt


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def fixed(builder):
    f = builder().opts(maxit=args.maxit, eps_abs=1e-100, eps_rel=1e-100).fit()
    niter = [int(v) for v in f.niter.ravel()]
    assert niter == [args.maxit + 1] * len(niter), niter
    return f


for p in PS:
    xt, cnt = make(p)
    X, C = DevicePtr(xt.data_ptr()), DevicePtr(cnt.data_ptr())
    npt = ((p + 31) // 32 * 32 // 2 + 511) // 512
    lam1 = float(admm_poisson(X, C, 1.0, intercept=False, n=n, p=p, k=k).lambda_one().max())
    print(json.dumps({"p": p, "npt": npt, "lambda_1": lam1, "mean_counts": [float(v) for v in cnt.mean(dim=1).cpu()]}), flush=True)

    def route(slots, alpha):
        lam = [f * lam1 / alpha for f in FRACTIONS]

        def run():
            t0 = time.perf_counter()
            with options(QUANT_SLOTS=slots):
                f = fixed(lambda: admm_poisson(X, C, lam, alpha=alpha, intercept=False, n=n, p=p, k=k))
            return time.perf_counter() - t0, f.stats["t_loop"], int(f.stats["xupdate_variant"]), k * len(lam)
        return run

    routes = []
    for alpha in ALPHAS:
        routes.append((f"alpha={alpha} S=1", route(1, alpha)))
        routes += [(f"alpha={alpha} S={s}", route(s, alpha)) for s in range(2, POIS_MAX_SLOTS[npt] + 1)]
        routes.append((f"alpha={alpha} S=auto", route(None, alpha)))
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
                          "wall_s": med[name][0], "wall_spread": spread(walls), "fit_iters_per_s": med[name][1], "rate_spread": spread(rates),
                          "walls": walls, "rates": rates}), flush=True)
    print(json.dumps({"p": p, "npt": npt, "rate_over_serial": {r: med[r][1] / med[r.split(" S=")[0] + " S=1"][1] for r in med}}), flush=True)
    for alpha in ALPHAS:
        lam = [f * lam1 / alpha for f in FRACTIONS]
        walls, f = [], None
        for r in range(2):
            t0 = time.perf_counter()
            f = admm_poisson(X, C, lam, alpha=alpha, intercept=False, n=n, p=p, k=k).fit()
            walls.append(time.perf_counter() - t0)
        nz = (f.beta[1:] != 0.0).sum(axis=0)
        print(json.dumps({"run": "converged", "p": p, "alpha": alpha, "variant": int(f.stats["xupdate_variant"]), "wall_s": walls[1], "t_loop": f.stats["t_loop"],
                          "niter_min_median_max_per_cell": [[int(f.niter[:, l].min()), int(np.median(f.niter[:, l])), int(f.niter[:, l].max())] for l in range(len(lam))],
                          "nonzeros_median_per_cell": [int(np.median(nz[:, l])) for l in range(len(lam))]}), flush=True)
    del xt, cnt, X, C
    torch.cuda.empty_cache()
