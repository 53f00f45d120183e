#!/usr/bin/env python
"""Measure admm_hip_logit_multi (k label columns on one setup) against what the parent commit offers for the same task, k separate
admm_hip_logit calls, at n = 50000, k = 8, fp64, device-resident input, intercept FALSE, with p = 1000 (one double2 per thread and row:
up to four slots) and p = 5000 (five: the logit form has no second slot there, only the shared setup is left).  `--p` takes other
layouts (3000: three double2, four slots; 4000: four double2, two slots).

Run 1 (fixed work): maxit = `--maxit` with eps so small that no column converges, one warm-up and `--repeats` timed repeats, median and
spread (max - min) / median of
  * "k calls": the wall time of k admm_logit calls, one per column (upload is none -- the input is device resident --, but every call
    standardises, forms the Gram matrix, inverts it and transposes), and the column-iterations per second of their loops;
  * "multi S=1": the new call on its serial route (QUANT_SLOTS=1): the wall time of the ONE call and its loop's column-iterations/s;
  * "multi S=s" for every s >= 2 the layout's register table admits: the same on the slotted route.
Run 2 (`--parent-tree DIR`: a built checkout of the parent commit): admm_logit's and admm_huber's iterations/s on this tree and on the
parent's, in `--rounds` alternating rounds, each measurement in a fresh process that imports admm_amd from its own tree.  Their kernels
are unchanged instruction for instruction: the rates must overlap.
Prints one JSON line per measurement.
Usage: bench_logit_multi.py [--n N --p P[,P...] --k K --repeats R --rounds R --maxit M --parent-tree DIR]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--p", default="1000,5000")
ap.add_argument("--k", type=int, default=8)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--maxit", type=int, default=100)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--single-child", default=None, help="(internal) measure admm_logit and admm_huber with the package of this tree and print one JSON line")
args = ap.parse_args()
n, k = args.n, args.k
PS = [int(v) for v in str(args.p).split(",")]
TREE = os.path.abspath(args.single_child) if args.single_child else ROOT
sys.path.insert(0, TREE)
import torch  # noqa: E402  (before libadmm_hip)
import admm_amd  # noqa: E402
from admm_amd import DevicePtr, admm_huber, admm_logit, options  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(admm_amd.__file__))) == TREE, admm_amd.__file__
dev = torch.device("cuda", 0)
LOGIT_MAX_SLOTS = {1: 4, 2: 4, 3: 4, 4: 2, 5: 1, 6: 1}      # fadmm_dense.hip, kProxKinds[kProxLogitS].max_slots


def make(p):
    """x = 2 N(0, 1) as p x n row-major (= n x p column-major), a response for Huber, and k label columns (k x n row-major) drawn from k
    logistic models with their own coefficients and class balances: not separable."""
    g = torch.Generator(device=dev)
    g.manual_seed(123)
    xt = torch.empty((p, n), dtype=torch.float64, device=dev)
    chunk = max(1, (1 << 27) // n)
    for c0 in range(0, p, chunk):
        c1 = min(p, c0 + chunk)
        xt[c0:c1] = torch.randn((c1 - c0, n), generator=g, device=dev, dtype=torch.float64) * 2.0
    b = torch.rand(p, generator=g, device=dev, dtype=torch.float64)
    y = b @ xt + torch.randn(n, generator=g, device=dev, dtype=torch.float64) * (1 + 0.3 * xt[0].abs())
    lab = torch.empty((k, n), dtype=torch.float64, device=dev)
    for c in range(k):
        bc = (2 * torch.rand(p, generator=g, device=dev, dtype=torch.float64) - 1) / p ** 0.5
        eta = 0.5 * (bc @ xt) - 0.8 + 1.6 * c / max(1, k - 1)
        lab[c] = (torch.rand(n, generator=g, device=dev, dtype=torch.float64) < torch.sigmoid(eta)).to(torch.float64)
    torch.cuda.synchronize()
    return xt, y, lab


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def fixed(builder):
    f = builder().opts(maxit=args.maxit, eps_abs=1e-100, eps_rel=1e-100).fit()
    niter = [int(f.niter)] if not hasattr(f.niter, "__len__") else [int(v) for v in f.niter]
    assert niter == [args.maxit + 1] * len(niter), niter
    return f


if args.single_child:
    p = PS[0]
    xt, y, lab = make(p)
    X, Y, L = DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr()), DevicePtr(lab.data_ptr())
    res = {"tree": TREE}
    for name, builder in (("admm_logit", lambda: admm_logit(X, L, intercept=False, n=n, p=p)),
                          ("admm_huber", lambda: admm_huber(X, Y, 1.345, 0.5, intercept=False, n=n, p=p))):
        rates = []
        for r in range(args.repeats + 1):
            f = fixed(builder)
            if r:
                rates.append(args.maxit / f.stats["t_loop"])
        res[name] = rates
    print(json.dumps(res), flush=True)
    sys.exit(0)

from admm_amd import admm_logit_multi  # noqa: E402

for p in PS:
    xt, _, lab = make(p)
    X, L = DevicePtr(xt.data_ptr()), DevicePtr(lab.data_ptr())
    npt = ((p + 31) // 32 * 32 // 2 + 511) // 512

    def k_calls():
        t0, loop = time.perf_counter(), 0.0
        for c in range(k):
            loop += fixed(lambda: admm_logit(X, DevicePtr(lab[c].data_ptr()), intercept=False, n=n, p=p)).stats["t_loop"]
        return time.perf_counter() - t0, loop, 1

    def multi(slots):
        def run():
            t0 = time.perf_counter()
            with options(QUANT_SLOTS=slots):
                f = fixed(lambda: admm_logit_multi(X, L, intercept=False, n=n, p=p, k=k))
            return time.perf_counter() - t0, f.stats["t_loop"], int(f.stats["xupdate_variant"])
        return run

    routes = [("k calls", k_calls), ("multi S=1", multi(1))] + [(f"multi S={s}", multi(s)) for s in range(2, min(LOGIT_MAX_SLOTS[npt], k) + 1)]
    med = {}
    for name, run in routes:
        walls, rates, variant = [], [], None
        for r in range(args.repeats + 1):
            wall, loop, variant = run()
            if r:
                walls.append(wall)
                rates.append(k * args.maxit / loop)
        med[name] = (statistics.median(walls), statistics.median(rates))
        print(json.dumps({"run": "fixed work", "route": name, "n": n, "p": p, "k": k, "npt": npt, "maxit": args.maxit, "variant": variant,
                          "wall_s": med[name][0], "wall_spread": spread(walls), "column_iters_per_s": med[name][1], "rate_spread": spread(rates),
                          "walls": walls, "rates": rates}), flush=True)
    print(json.dumps({"p": p, "npt": npt, "wall_over_k_calls": {r: med[r][0] / med["k calls"][0] for r in med},
                      "rate_over_serial": {r: med[r][1] / med["multi S=1"][1] for r in med}}), flush=True)
    del xt, lab, X, L
    torch.cuda.empty_cache()

if args.parent_tree:
    trees = {"this": ROOT, "parent": os.path.abspath(args.parent_tree)}
    ab = {(t, s): [] for t in trees for s in ("admm_logit", "admm_huber")}
    for rnd in range(args.rounds):
        for t, tree in trees.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--single-child", tree, "--n", str(n), "--p", str(PS[-1]), "--k", str(k),
                                  "--repeats", str(args.repeats), "--maxit", str(args.maxit)], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit(f"child on {tree} failed ({out.returncode}):\n{out.stderr[-2000:]}")
            res = json.loads(out.stdout.strip().splitlines()[-1])
            for s in ("admm_logit", "admm_huber"):
                ab[(t, s)].append(statistics.median(res[s]))
            print(json.dumps({"run": "A/B", "round": rnd, "tree": t, "p": PS[-1], "admm_logit": res["admm_logit"], "admm_huber": res["admm_huber"]}), flush=True)
    for s in ("admm_logit", "admm_huber"):
        this, parent = ab[("this", s)], ab[("parent", s)]
        print(json.dumps({"ab": s, "p": PS[-1], "this": statistics.median(this), "parent": statistics.median(parent), "spread_this": spread(this),
                          "spread_parent": spread(parent), "this_over_parent": statistics.median(this) / statistics.median(parent),
                          "ranges_overlap": max(min(this), min(parent)) <= min(max(this), max(parent))}), flush=True)
