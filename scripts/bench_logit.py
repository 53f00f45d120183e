#!/usr/bin/env python
"""Measure admm_hip_logit against admm_hip_huber (the same kernels with a closed-form prox: the yardstick for what the Newton prox
costs) and admm_hip_lad, at n = 50000 with p = 5000 (five double2 per thread and row) and p = 1000 (one: where the prox weighs most),
fp64, device-resident input, intercept FALSE.

Run 1 (fixed work): maxit = `--maxit` with eps so small that nothing converges; iterations/s of the loop (stats t_loop) of admm_logit,
of admm_huber with ONE fit (delta = 1.345, tau = 0.5) and of admm_lad at the same shape and options, one warm-up and `--repeats`
timed repeats, median and spread (max - min) / median.  The rows launch streams 8 n p bytes per iteration: the achieved bytes/s of
the whole iteration is printed beside each rate.
Run 2 (default eps / maxit): iterations and wall time of admm_logit's loop to convergence.
Run 3 (`--parent-tree DIR`: a built checkout of the parent commit): admm_lad's iterations/s on this tree and on the parent's, in
`--rounds` alternating rounds, each measurement in a fresh process that imports admm_amd from its own tree.  LAD's kernels are meant
to be unchanged: the rate of this tree must lie within the spread of the parent's repeats.
Prints one JSON line per measurement.
Usage: bench_logit.py [--n N --p P[,P...] --repeats K --rounds R --maxit M --parent-tree DIR --skip-converged]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--p", default="5000,1000")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--maxit", type=int, default=200)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--skip-converged", action="store_true")
ap.add_argument("--lad-child", default=None, help="(internal) measure admm_lad with the package of this tree and print one JSON line")
args = ap.parse_args()
n = args.n
PS = [int(v) for v in str(args.p).split(",")]
TREE = os.path.abspath(args.lad_child) if args.lad_child else ROOT
sys.path.insert(0, TREE)
import torch  # noqa: E402  (before libadmm_hip)
import admm_amd  # noqa: E402
from admm_amd import DevicePtr, admm_lad  # noqa: E402

assert os.path.dirname(os.path.dirname(os.path.abspath(admm_amd.__file__))) == TREE, admm_amd.__file__
dev = torch.device("cuda", 0)


def make(p):
    """x = 2 N(0, 1), a response for LAD / Huber and labels for the logistic fit (about 40 % ones, not separable)."""
    g = torch.Generator(device=dev)
    g.manual_seed(123)
    xt = torch.empty((p, n), dtype=torch.float64, device=dev)
    chunk = max(1, (1 << 27) // n)
    for c0 in range(0, p, chunk):
        c1 = min(p, c0 + chunk)
        xt[c0:c1] = torch.randn((c1 - c0, n), generator=g, device=dev, dtype=torch.float64) * 2.0
    b = torch.rand(p, generator=g, device=dev, dtype=torch.float64)
    noise = torch.randn(n, generator=g, device=dev, dtype=torch.float64)
    y = b @ xt + noise * (1 + 0.3 * xt[0].abs())
    eta = 0.5 * ((2 * b - 1) / p ** 0.5) @ xt - 0.4
    lab = (torch.rand(n, generator=g, device=dev, dtype=torch.float64) < torch.sigmoid(eta)).to(torch.float64)
    torch.cuda.synchronize()
    return xt, y, lab


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def rates_of(builder, repeats):
    out = []
    for r in range(repeats + 1):
        f = builder().opts(maxit=args.maxit, eps_abs=1e-100, eps_rel=1e-100).fit()
        niter = int(f.niter if not hasattr(f.niter, "__len__") else f.niter[0])
        assert niter == args.maxit + 1, niter
        if r:
            out.append((niter - 1) / f.stats["t_loop"])
    return out, f.stats


if args.lad_child:
    p = PS[0]
    xt, y, _ = make(p)
    rates, _ = rates_of(lambda: admm_lad(DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr()), intercept=False, n=n, p=p), args.repeats)
    print(json.dumps({"tree": TREE, "rates": rates}), flush=True)
    sys.exit(0)

from admm_amd import admm_huber, admm_logit  # noqa: E402

for p in PS:
    xt, y, lab = make(p)
    X, Y, L = DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr()), DevicePtr(lab.data_ptr())
    npt = ((p + 31) // 32 * 32 // 2 + 511) // 512
    got = {}
    for name, builder in (("admm_lad", lambda: admm_lad(X, Y, intercept=False, n=n, p=p)),
                          ("admm_huber", lambda: admm_huber(X, Y, 1.345, 0.5, intercept=False, n=n, p=p)),
                          ("admm_logit", lambda: admm_logit(X, L, intercept=False, n=n, p=p))):
        rates, st = rates_of(builder, args.repeats)
        got[name] = statistics.median(rates)
        print(json.dumps({"run": "fixed work", "solver": name, "n": n, "p": p, "npt": npt, "maxit": args.maxit, "variant": int(st["xupdate_variant"]),
                          "iters_per_s": got[name], "spread": spread(rates), "rates": rates,
                          "x_bytes_per_s": 8.0 * n * p * got[name], "x_and_inverse_bytes_per_s": (8.0 * n * p + 8.0 * p * p) * got[name]}), flush=True)
    print(json.dumps({"p": p, "npt": npt, "logit_over_huber": got["admm_logit"] / got["admm_huber"], "logit_over_lad": got["admm_logit"] / got["admm_lad"]}), flush=True)
    if not args.skip_converged:
        for r in range(2):
            f = admm_logit(X, L, intercept=False, n=n, p=p).fit()
        print(json.dumps({"run": "default eps / maxit", "solver": "admm_logit", "p": p, "niter": int(f.niter), "loop_wall_s": f.stats["t_loop"],
                          "total_s": f.stats["t_total"]}), flush=True)
    del xt, y, lab, X, Y, L
    torch.cuda.empty_cache()

if args.parent_tree:
    trees = {"this": ROOT, "parent": os.path.abspath(args.parent_tree)}
    ab = {k: [] for k in trees}
    for rnd in range(args.rounds):
        for k, tree in trees.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--lad-child", tree, "--n", str(n), "--p", str(PS[0]), "--repeats", str(args.repeats),
                                  "--maxit", str(args.maxit)], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit(f"admm_lad child on {tree} failed ({out.returncode}):\n{out.stderr[-2000:]}")
            res = json.loads(out.stdout.strip().splitlines()[-1])
            ab[k].append(statistics.median(res["rates"]))
            print(json.dumps({"run": "admm_lad A/B", "round": rnd, "tree": k, "iters_per_s": ab[k][-1], "rates": res["rates"]}), flush=True)
    med = {k: statistics.median(v) for k, v in ab.items()}
    print(json.dumps({"lad_ab": med, "spread": {k: spread(v) for k, v in ab.items()}, "this_over_parent": med["this"] / med["parent"],
                      "within_parent_spread": min(ab["parent"]) <= med["this"] <= max(ab["parent"]) or med["this"] >= med["parent"]}), flush=True)
