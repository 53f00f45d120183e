#!/usr/bin/env python
"""Measure the quantile grid of admm_hip_quantreg at the C5 LAD shape (n = 50000, p = 5000 fp64, device-resident input, intercept
FALSE), tau = 0.1 ... 0.9: what QUANT_SLOTS=0 should pick.

Run 1 (fixed work): maxit = 200 with eps so small that nothing converges -- every route does the same 9 x 200 tau-iterations.  For
QUANT_SLOTS = 1 and every S the register layout of the shape admits: setup seconds and tau-iterations/s of the loop, one warm-up and
`--repeats` timed repeats, median and spread (max - min) / median.  Beside them admm_lad's iterations/s on the same build.
Run 2 (default eps / maxit): wall time of the loops to the last tau, per route -- what refilling buys when the iteration counts differ.
Prints one JSON line per measurement and a last line {"auto": S}: the fastest S, or 1 when no S >= 2 beats the serial route by more
than the spread of the repeats.  Usage: bench_quantreg.py [--n N --p P --repeats K --skip-converged]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before libadmm_hip)
import numpy as np  # noqa: E402
from admm_amd import DevicePtr, admm_lad, admm_quantreg, options  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--p", type=int, default=5000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--maxit", type=int, default=200)
ap.add_argument("--skip-converged", action="store_true")
args = ap.parse_args()
n, p = args.n, args.p
TAUS = np.round(np.arange(1, 10) / 10.0, 1)

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(123)
xt = torch.empty((p, n), dtype=torch.float64, device=dev)
chunk = max(1, (1 << 27) // n)
for c0 in range(0, p, chunk):
    c1 = min(p, c0 + chunk)
    xt[c0:c1] = torch.randn((c1 - c0, n), generator=g, device=dev, dtype=torch.float64) * 2.0
b = torch.rand(p, generator=g, device=dev, dtype=torch.float64)
noise = torch.randn(n, generator=g, device=dev, dtype=torch.float64)
y = b @ xt + noise * (1 + 0.3 * xt[0].abs())          # heteroscedastic: the quantiles of the grid differ in more than the intercept
torch.cuda.synchronize()
X, Y = DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr())


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def grid(slots, maxit, eps):
    with options(QUANT_SLOTS=slots):
        return admm_quantreg(X, Y, TAUS, intercept=False, n=n, p=p).opts(maxit=maxit, eps_abs=eps, eps_rel=eps).fit()


npt = ((p + 31) // 32 * 32 // 2 + 511) // 512
max_slots = 4 if npt <= 3 else (3 if npt == 4 else (2 if npt == 5 else 1))
routes = [1] + list(range(2, min(max_slots, len(TAUS)) + 1))

# admm_lad on the same build and data: iterations/s of its loop
rates = []
for r in range(args.repeats + 1):
    f = admm_lad(X, Y, intercept=False, n=n, p=p).opts(maxit=args.maxit, eps_abs=1e-100, eps_rel=1e-100).fit()
    if r:
        rates.append((f.niter - 1) / f.stats["t_loop"])
lad = {"run": "admm_lad", "n": n, "p": p, "maxit": args.maxit, "iters_per_s": statistics.median(rates), "spread": spread(rates)}
print(json.dumps(lad), flush=True)

fixed = {}
for s in routes:
    rates, setup = [], []
    for r in range(args.repeats + 1):
        f = grid(s, args.maxit, 1e-100)
        assert (f.niter == args.maxit + 1).all(), f.niter
        if r:
            rates.append(len(TAUS) * args.maxit / f.stats["t_loop"])
            setup.append(f.stats["t_gram"] + f.stats["t_factor"] + f.stats["t_standardize"])
    fixed[s] = {"run": "fixed work", "quant_slots": s, "variant": int(f.stats["xupdate_variant"]), "tau_iters_per_s": statistics.median(rates),
                "spread": spread(rates), "setup_s": statistics.median(setup), "rates": rates}
    print(json.dumps(fixed[s]), flush=True)

if not args.skip_converged:
    for s in routes:
        walls = []
        for r in range(2):
            f = grid(s, 10000, 1e-4)
            if r:
                walls.append(f.stats["t_loop"])
        print(json.dumps({"run": "default eps / maxit", "quant_slots": s, "loops_wall_s": walls[0], "niter": f.niter.tolist(), "total_s": f.stats["t_total"]}), flush=True)

best = max(fixed, key=lambda s: fixed[s]["tau_iters_per_s"])
noise_band = max(fixed[1]["spread"], fixed[best]["spread"])
auto = best if best != 1 and fixed[best]["tau_iters_per_s"] > fixed[1]["tau_iters_per_s"] * (1 + noise_band) else 1
print(json.dumps({"auto": auto, "serial_tau_iters_per_s": fixed[1]["tau_iters_per_s"], "best": best, "best_tau_iters_per_s": fixed[best]["tau_iters_per_s"]}), flush=True)
