#!/usr/bin/env python
"""Dev tool (GPU box): the group lasso's and the sparse-group lasso's ADMM rates beside the Lasso's on the same data and build
(device-resident inputs).

    bench_grplasso.py [--n 100000] [--p 10000] [--group-size 4] [--big-group 0] [--alpha 0.5] [--nlambda 100] [--steps 3] [--warmup 1]

The models are prepared once (LassoPlan) and every step is one cold-started warm-chained lambda path; the rate is
iterations / loop time as the library reports them (admm_stats.total_iter, t_loop), the median over the steps.  The x-update is the
same kernel in all three, so the gaps between the rates are the tails' (tall_group_tail_kernel, plain and sparse, against
tall_tail_kernel).  --alpha A: the mixing parameter of the sparse form (admm_sgl, l1 weights uniform in [0.5, 2]).
--big-group G: instead of equal groups, ONE group of G columns (<= 1024) among singletons -- the cost of the multi-pass workgroup.
Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before libadmm_hip: one HIP runtime per process)
import numpy as np  # noqa: E402
from admm_amd import DevicePtr, admm_grplasso, admm_lasso, admm_sgl  # noqa: E402
from admm_amd.api import LassoPlan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--p", type=int, default=10000)
ap.add_argument("--group-size", type=int, default=4)
ap.add_argument("--big-group", type=int, default=0)
ap.add_argument("--alpha", type=float, default=0.5)
ap.add_argument("--nlambda", type=int, default=100)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
a = ap.parse_args()
n, p = a.n, a.p

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(5)
xt = torch.empty((p, n), dtype=torch.float64, device=dev)          # p x n row-major == n x p column-major
chunk = max(1, (1 << 27) // n)
for c0 in range(0, p, chunk):
    c1 = min(p, c0 + chunk)
    xt[c0:c1] = torch.randn((c1 - c0, n), generator=g, device=dev, dtype=torch.float64) * 2
b = torch.zeros(p, dtype=torch.float64, device=dev)
b[:1000] = torch.rand(1000, generator=g, device=dev, dtype=torch.float64)
y = b @ xt + torch.randn(n, generator=g, device=dev, dtype=torch.float64)
torch.cuda.synchronize()

if a.big_group > 0:
    group = np.concatenate([np.zeros(a.big_group, dtype=np.int64), 1 + np.arange(p - a.big_group)])
else:
    group = np.arange(p) // a.group_size
l1_weights = np.random.default_rng(6).uniform(0.5, 2.0, p)
xp, yp = DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr())


def rate(model):
    plan = LassoPlan(model)
    rows = []
    for k in range(a.warmup + a.steps):
        st = plan.run().stats
        if k >= a.warmup:
            rows.append((st["total_iter"] / st["t_loop"], st["total_iter"], st["t_loop"]))
    plan.close()
    rows.sort()
    r = rows[len(rows) // 2]
    return {"iterations_per_s": round(r[0], 1), "iterations": int(r[1]), "loop_s": round(r[2], 4),
            "min_max_iterations_per_s": [round(rows[0][0], 1), round(rows[-1][0], 1)]}


out = {"n": n, "p": p, "nlambda": a.nlambda, "steps": a.steps,
       "groups": f"one group of {a.big_group} among singletons" if a.big_group > 0 else f"groups of {a.group_size}",
       "grplasso": rate(admm_grplasso(xp, yp, group, n=n, p=p).penalty(nlambda=a.nlambda)),
       "sgl": dict(rate(admm_sgl(xp, yp, group, alpha=a.alpha, n=n, p=p).penalty(nlambda=a.nlambda, l1_weights=l1_weights)), alpha=a.alpha),
       "lasso": rate(admm_lasso(xp, yp, n=n, p=p).penalty(nlambda=a.nlambda))}
print(json.dumps(out))
