#!/usr/bin/env python
"""Measure admm_hip_huber at the C5 LAD shape (n = 50000, p = 5000 fp64, device-resident input, intercept FALSE) on a grid of seven
(delta, tau) pairs: what QUANT_SLOTS=0 should pick for the Huber form, and whether admm_lad's loop is what it was.

Run 1 (fixed work): maxit = 200 with eps so small that nothing converges -- every route does the same 7 x 200 fit-iterations.  For
QUANT_SLOTS = 1 and every S the Huber slot table admits at the shape: setup seconds and fit-iterations/s of the loop, one warm-up and
`--repeats` timed repeats, median and spread (max - min) / median.
Run 2 (default eps / maxit): wall time of the loops to the last fit, per route.
Run 3 (`--parent-tree DIR`: a built checkout of the parent commit): admm_lad's iterations/s on this tree and on the parent's, in
`--rounds` alternating rounds, each measurement in a fresh process that imports admm_amd from its own tree.  LAD's kernels are meant
to be unchanged: the rate of this tree must lie within the spread of the parent's repeats.
Prints one JSON line per measurement, {"lad_ab": ...} and a last line {"auto": S}: the fastest S, or 1 when no S >= 2 beats the serial
route by more than the spread of the repeats.
Usage: bench_huber.py [--n N --p P --repeats K --rounds R --parent-tree DIR --skip-converged]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--p", type=int, default=5000)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--maxit", type=int, default=200)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--skip-converged", action="store_true")
ap.add_argument("--lad-child", default=None, help="(internal) measure admm_lad with the package of this tree and print one JSON line")
args = ap.parse_args()
n, p = args.n, args.p
TREE = os.path.abspath(args.lad_child) if args.lad_child else ROOT
sys.path.insert(0, TREE)
import torch  # noqa: E402  (before libadmm_hip)
import numpy as np  # noqa: E402
import admm_amd  # noqa: E402
from admm_amd import DevicePtr, admm_lad, options  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(admm_amd.__file__))) == TREE, admm_amd.__file__
INF = float("inf")
GRID = [(0.3, 0.5), (INF, 0.5), (0.3, 0.9), (1.345, 0.2), (0.3, 0.5), (5.0, 0.2), (1.345, 0.9)]      # (delta, tau)
DELTAS, TAUS = np.array([d for d, _ in GRID]), np.array([t for _, t in GRID])

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
y = b @ xt + noise * (1 + 0.3 * xt[0].abs())          # heteroscedastic, as scripts/bench_quantreg.py
torch.cuda.synchronize()
X, Y = DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr())


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def lad_rates(repeats):
    rates = []
    for r in range(repeats + 1):
        f = admm_lad(X, Y, intercept=False, n=n, p=p).opts(maxit=args.maxit, eps_abs=1e-100, eps_rel=1e-100).fit()
        if r:
            rates.append((f.niter - 1) / f.stats["t_loop"])
    return rates


if args.lad_child:
    print(json.dumps({"tree": TREE, "rates": lad_rates(args.repeats)}), flush=True)
    sys.exit(0)

from admm_amd import admm_huber  # noqa: E402


def grid(slots, maxit, eps):
    with options(QUANT_SLOTS=slots):
        return admm_huber(X, Y, DELTAS, TAUS, intercept=False, n=n, p=p).opts(maxit=maxit, eps_abs=eps, eps_rel=eps).fit()


npt = ((p + 31) // 32 * 32 // 2 + 511) // 512
max_slots = 4 if npt <= 3 else (2 if npt <= 5 else 1)      # kProxKinds[kProxHuber].max_slots (fadmm_dense.hip)
routes = [1] + list(range(2, min(max_slots, len(GRID)) + 1))

rates = lad_rates(args.repeats)
print(json.dumps({"run": "admm_lad", "n": n, "p": p, "maxit": args.maxit, "iters_per_s": statistics.median(rates), "spread": spread(rates)}), flush=True)

fixed = {}
for s in routes:
    rates, setup = [], []
    for r in range(args.repeats + 1):
        f = grid(s, args.maxit, 1e-100)
        assert (f.niter == args.maxit + 1).all(), f.niter
        if r:
            rates.append(len(GRID) * args.maxit / f.stats["t_loop"])
            setup.append(f.stats["t_gram"] + f.stats["t_factor"] + f.stats["t_standardize"])
    fixed[s] = {"run": "fixed work", "quant_slots": s, "variant": int(f.stats["xupdate_variant"]), "fit_iters_per_s": statistics.median(rates),
                "spread": spread(rates), "setup_s": statistics.median(setup), "rates": rates}
    print(json.dumps(fixed[s]), flush=True)

if not args.skip_converged:
    for s in routes:
        for r in range(2):
            f = grid(s, 10000, 1e-4)
        print(json.dumps({"run": "default eps / maxit", "quant_slots": s, "loops_wall_s": f.stats["t_loop"], "niter": f.niter.tolist(), "total_s": f.stats["t_total"]}), flush=True)

if args.parent_tree:
    # free this process's copy of the data before the children allocate theirs
    del xt, y, b, noise, X, Y
    torch.cuda.empty_cache()
    trees = {"this": ROOT, "parent": os.path.abspath(args.parent_tree)}
    ab = {k: [] for k in trees}
    for rnd in range(args.rounds):
        for k, tree in trees.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--lad-child", tree, "--n", str(n), "--p", str(p), "--repeats", str(args.repeats),
                                  "--maxit", str(args.maxit)], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit(f"admm_lad child on {tree} failed ({out.returncode}):\n{out.stderr[-2000:]}")
            got = json.loads(out.stdout.strip().splitlines()[-1])
            ab[k].append(statistics.median(got["rates"]))
            print(json.dumps({"run": "admm_lad A/B", "round": rnd, "tree": k, "iters_per_s": ab[k][-1], "rates": got["rates"]}), flush=True)
    med = {k: statistics.median(v) for k, v in ab.items()}
    print(json.dumps({"lad_ab": med, "spread": {k: spread(v) for k, v in ab.items()}, "this_over_parent": med["this"] / med["parent"],
                      "within_parent_spread": min(ab["parent"]) <= med["this"] <= max(ab["parent"]) or med["this"] >= med["parent"]}), flush=True)

best = max(fixed, key=lambda s: fixed[s]["fit_iters_per_s"])
noise_band = max(fixed[1]["spread"], fixed[best]["spread"])
auto = best if best != 1 and fixed[best]["fit_iters_per_s"] > fixed[1]["fit_iters_per_s"] * (1 + noise_band) else 1
print(json.dumps({"auto": auto, "serial_fit_iters_per_s": fixed[1]["fit_iters_per_s"], "best": best, "best_fit_iters_per_s": fixed[best]["fit_iters_per_s"]}), flush=True)
