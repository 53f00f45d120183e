#!/usr/bin/env python
"""Dev tool (GPU box): the box-constrained, weighted elastic net's ADMM rate beside the Lasso's on the same data and build
(device-resident inputs).

    bench_boxenet.py [--n 100000] [--p 10000] [--nlambda 100] [--rounds 5]

Prepared models (LassoPlan) on one data set: admm_lasso, and admm_boxenet in three settings --
    free     no bounds, unit factors (the Lasso's problem on tall_box_tail_kernel: the tail's own cost),
    pattern  the tests' pattern (a quarter of the columns non-negative, a quarter capped, a quarter in a band, every 37th excluded;
             factors in [0.5, 2], two columns unpenalised), Lasso prox,
    enet     the pattern at alpha = 0.5.
They are run in turn, round after round in one process (one warm-up round first), every run one cold-started warm-chained lambda
path; the rate is iterations / loop time as the library reports them (admm_stats.total_iter, t_loop).  The x-update is the same
kernel in all of them, so `free` against `lasso` is tall_box_tail_kernel against tall_tail_kernel; the other two solve other problems
and take other numbers of iterations.  `lasso` and `free` are prepared TWICE (`lasso_b`, `free_b`: the same model, another plan with
buffers of its own): the x-update's time depends on where a plan's 4p^2-byte inverse landed by more than the tails differ, so the
gap between two plans of one model is the yardstick for the gap between the models.  Prints one JSON line: per plan the rate of
every round, and their range."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before libadmm_hip: one HIP runtime per process)
import numpy as np  # noqa: E402
from admm_amd import DevicePtr, admm_boxenet, admm_lasso  # noqa: E402
from admm_amd.api import LassoPlan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--p", type=int, default=10000)
ap.add_argument("--nlambda", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
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
b[:1000] = torch.rand(1000, generator=g, device=dev, dtype=torch.float64) - 0.3
y = b @ xt + torch.randn(n, generator=g, device=dev, dtype=torch.float64)
torch.cuda.synchronize()

j = np.arange(p)
lower, upper = np.full(p, -np.inf), np.full(p, np.inf)
lower[j % 4 == 0] = 0.0
upper[j % 4 == 1] = 0.25
lower[j % 4 == 2], upper[j % 4 == 2] = -0.1, 0.1
lower[j % 37 == 5], upper[j % 37 == 5] = 0.0, 0.0
u = np.random.default_rng(31).uniform(0.5, 2.0, p)
u[7] = u[20] = 0.0
xp, yp = DevicePtr(xt.data_ptr()), DevicePtr(y.data_ptr())

models = {
    "lasso": admm_lasso(xp, yp, n=n, p=p).penalty(nlambda=a.nlambda),
    "free": admm_boxenet(xp, yp, n=n, p=p).penalty(nlambda=a.nlambda),
    "pattern": admm_boxenet(xp, yp, lower, upper, n=n, p=p).penalty(nlambda=a.nlambda, penalty_factor=u),
    "enet": admm_boxenet(xp, yp, lower, upper, n=n, p=p).penalty(nlambda=a.nlambda, penalty_factor=u, alpha=0.5),
    "free_b": admm_boxenet(xp, yp, n=n, p=p).penalty(nlambda=a.nlambda),
    "lasso_b": admm_lasso(xp, yp, n=n, p=p).penalty(nlambda=a.nlambda),
}
plans = {k: LassoPlan(m) for k, m in models.items()}
rows = {k: [] for k in plans}
for r in range(a.rounds + 1):
    for k, plan in plans.items():
        st = plan.run().stats
        if r > 0:                                                     # round 0 warms up
            rows[k].append((st["total_iter"] / st["t_loop"], int(st["total_iter"]), st["t_loop"]))
for plan in plans.values():
    plan.close()

out = {"n": n, "p": p, "nlambda": a.nlambda, "rounds": a.rounds}
for k, rr in rows.items():
    rates = [x[0] for x in rr]
    out[k] = {"iterations_per_s": [round(v, 1) for v in rates], "min_max_iterations_per_s": [round(min(rates), 1), round(max(rates), 1)],
              "iterations": rr[0][1], "loop_s": [round(x[2], 4) for x in rr]}
print(json.dumps(out))
